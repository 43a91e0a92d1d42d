"""OCR validation on the device (csrc/ocr_data.hip): loss_mask's targets (OCR/OCR.py:77-100), the two losses of train_the
(OCR/OCR.py:103-119, 264-265) with their gradient at the logits, and the valid mode (OCR/OCR.py:301-343) as counts instead of a
printed text.  The data is LPGenerator.render_device's (yolo_amd/render.py).  No backward pass of the DenseNet body, no train-mode
BatchNorm, no optimiser: ocr_loss's dlogits is where a later OCR trainer attaches."""
import torch

from . import lib as L
from .dense import PlateReader

SCORE_WORDS = 6            # include/yolo_amd.h: YOLO_OCR_SCORE_WORDS
SCORE_WEIGHT, CLASS_WEIGHT = 0.1, 1.0          # OCR/OCR.py:235-236


def _want(t, name, dtype, shape=None):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous() or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError('%s should be a contiguous %s CUDA tensor%s' % (name, str(dtype).replace('torch.', ''), '' if shape is None else ' of shape %r' % (tuple(shape),)))
    return t


def ocr_targets(labels, Wp=24, order=None):
    """loss_mask: labels (B,nobj,3) float32 [class, left, right] on the device (LPGenerator.render_device's) -> (score_y (B,Wp)
    float32, class_y (B,Wp) int32; 0 and -1 where no label covers).  order (B,nobj) int32: the visiting order of each image's
    labels (LPGenerator.ocr_order: the host's draw of the reference's shuffle; a later label overwrites an earlier one), None:
    the given order.  Current stream, no synchronisation."""
    _want(labels, 'labels', torch.float32)
    if labels.dim() != 3 or labels.shape[2] != 3:
        raise ValueError('labels should have the shape (B, nobj, 3)')
    B, nobj = labels.shape[0], labels.shape[1]
    L.require_current_device(labels.device, 'this ocr_targets call')
    if order is not None:
        _want(order, 'order', torch.int32, (B, nobj))
    score_y = torch.empty((B, Wp), dtype=torch.float32, device=labels.device)
    class_y = torch.empty((B, Wp), dtype=torch.int32, device=labels.device)
    L.check(L.load().yolo_ocr_targets(L.ptr(labels), L.ptr(order), L.ptr(score_y), L.ptr(class_y), B, nobj, int(Wp), L.stream_ptr()), 'ocr_targets')
    return score_y, class_y


def ocr_loss(logits, score_y, class_y, grad=False, score_weight=SCORE_WEIGHT, class_weight=CLASS_WEIGHT):
    """logits (B,Wp,1+ncls) float32 as OCRNet.logits returns them, score_y / class_y from ocr_targets -> losses (2,B) float32
    [score, class] per image: score_weight * LogisticLoss(binary) of the score column and class_weight * SoftmaxCrossEntropyLoss
    of the class columns weighted by score_y.  grad=True: -> (losses, dlogits), dlogits the gradient of losses.sum() (not divided
    by the batch).  Current stream, no synchronisation."""
    _want(logits, 'logits', torch.float32)
    if logits.dim() != 3 or logits.shape[2] < 2:
        raise ValueError('logits should have the shape (B, Wp, 1 + ncls)')
    B, Wp, C = logits.shape
    _want(score_y, 'score_y', torch.float32, (B, Wp))
    _want(class_y, 'class_y', torch.int32, (B, Wp))
    L.require_current_device(logits.device, 'this ocr_loss call')
    losses = torch.empty((2, B), dtype=torch.float32, device=logits.device)
    dlogits = torch.empty_like(logits) if grad else None
    L.check(L.load().yolo_ocr_loss_fwd_bwd(L.ptr(logits), L.ptr(score_y), L.ptr(class_y), L.ptr(dlogits), L.ptr(losses), B, Wp, C - 1,
                                           float(score_weight), float(class_weight), L.stream_ptr()), 'ocr_loss')
    return (losses, dlogits) if grad else losses


def ocr_score(codes, count, labels, class_y, logits):
    """The counts of one validation step, (B, 6) int32 per image: truth length (labels whose centre lies in [0, 1), left to right),
    predicted length, Levenshtein distance, exact match, labelled columns, labelled columns whose class argmax is right.  codes and
    count as PlateReader.read_device returns them.  nobj <= 16, Wp <= 64."""
    B, Wp, C = logits.shape
    counts = torch.empty((B, SCORE_WORDS), dtype=torch.int32, device=logits.device)
    L.check(L.load().yolo_ocr_score(L.ptr(_want(codes, 'codes', torch.int32, (B, Wp))), L.ptr(_want(count, 'count', torch.int32, (B,))),
                                    L.ptr(_want(labels, 'labels', torch.float32)), L.ptr(_want(class_y, 'class_y', torch.int32, (B, Wp))),
                                    L.ptr(_want(logits, 'logits', torch.float32)), L.ptr(counts), B, labels.shape[1], Wp, C - 1, L.stream_ptr()),
            'ocr_score')
    return counts


class OCRValidator(object):
    """The valid mode (OCR/OCR.py:301-343) as numbers: the net, the peaks at `threshold` (0.2 there), the targets, the two losses
    and the counts, accumulated on the device (int64 / float64); only result() copies.

        val = OCRValidator(ocr_net)
        for _ in range(steps):
            x, labels = plates.render_device(backgrounds.next_batch())
            val.update(x, labels)
        print(val.result())

    net_or_reader: an OCRNet, or a PlateReader (whose net and names are used; the threshold is this object's)."""

    def __init__(self, net_or_reader, threshold=0.2):
        net = net_or_reader.net if isinstance(net_or_reader, PlateReader) else net_or_reader
        self.reader = PlateReader(net, threshold=threshold, names=net_or_reader.names) if isinstance(net_or_reader, PlateReader) \
            else PlateReader(net, threshold=threshold)
        self.net = net
        self.reset()

    def reset(self):
        self._counts = torch.zeros((SCORE_WORDS,), dtype=torch.int64, device=self.net.device)
        self._losses = torch.zeros((2,), dtype=torch.float64, device=self.net.device)
        self._plates = 0

    def update(self, x, labels, order=None):
        """x (B,3,H,W) float32 0..1 and labels (B,nobj,3) on the net's device.  Everything on the current stream, no synchronisation."""
        _, codes, count = self.reader.read_device(x)
        logits = self.net.held_logits(x)                          # (read_device has just run the net)
        score_y, class_y = ocr_targets(labels, logits.shape[1], order)
        losses = ocr_loss(logits, score_y, class_y)
        counts = ocr_score(codes, count, labels, class_y, logits)
        self._counts += counts.sum(dim=0, dtype=torch.int64)
        self._losses += losses.sum(dim=1, dtype=torch.float64)
        self._plates += int(x.shape[0])

    def result(self):
        c = [int(v) for v in self._counts.cpu().tolist()]
        ls = self._losses.cpu().tolist()
        n = self._plates
        return {'score_loss': ls[0] / n if n else float('nan'), 'class_loss': ls[1] / n if n else float('nan'),
                'plate_accuracy': c[3] / n if n else float('nan'), 'cer': c[2] / c[0] if c[0] else float('nan'),
                'column_accuracy': c[5] / c[4] if c[4] else float('nan'), 'n_plates': n, 'n_chars': c[0]}
