"""DenseNet bodies: OCRNet, LPDenseNet (inference, and the train-mode FORWARD with batch-statistic BatchNorm) and the PlateReader that
turns a rectified plate into text.

The reference's video pipeline publishes the rectified licence plate on /YOLO/clipped_LP; its only subscriber is OCR/OCR.py, which
resizes the plate to 160x384, runs OCRDenseNet (OCR/OCR.py:34-74) and reads the text off 24 score columns (predict, :180-201).
LPDenseNet (licence_plate/LP_detection.py:59-97) and CarDenseNet (car/utils.py:48-61) share the same gluoncv DenseNet body.

gluoncv is not part of the reference tree, so its builder (model_zoo/densenet.py: _make_dense_block / _make_dense_layer /
_make_transition) is RESTATED HERE FROM RECALL, not copied:
  stem        Conv 7x7 s2 p3 no bias 3 -> F0, BN, ReLU, MaxPool 3x3 s2 p1
  dense layer BN, ReLU, Conv 1x1 no bias Cin -> bn_size*G, BN, ReLU, Conv 3x3 p1 no bias -> G; output = concat(x, new), no dropout
  transition  BN, ReLU, Conv 1x1 no bias C -> C // 2, AvgPool 2x2 s2; after every block but the last
  then        BN, ReLU and the head of the net at hand
Every arithmetic operation of a forward pass runs in libyolo_amd.so (csrc/dense.hip, csrc/ocr.hip and yolo_conv_fwd for the heads);
torch owns the memory and the stream.

forward(x, training=True) is the TRAIN-MODE forward (csrc/dense_train.hip): every BatchNorm normalises with the batch's statistics,
keeps them (net.batch_stats) and updates its running statistics as Gluon does.  The inference kernels run unchanged with (scale, bias)
pairs folded from batch statistics; the statistics of a block's channels are measured once, as the channels are written.  It serves
validation losses in train mode and recalibrate_bn.  The backward pass, the optimiser and an OCRTrainer are not offered.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import lib as L
from .spec import BN_EPS

_TORCH_DT = {'bf16': torch.bfloat16, 'f32': torch.float32}
_LIB_DT = {'bf16': L.BF16, 'f32': L.F32}
BN_FIELDS = ('gamma', 'beta', 'running_mean', 'running_var')
HEAD_WIDTH = 512

# cls_names of OCR/OCR.py:220-224 (no I and no O)
OCR_NAMES = list('0123456789ABCDEFGHJKLMNPQRSTUVWXYZ')
_ALPHABET = 'ABCDEFGHJKLMNPQRSTUVWXYZ'     # OCR/OCR.py:29
_NUMBER = '012356789'                      # OCR/OCR.py:30 (the reference's list has no 4)


def plate_format_ok(text):
    """The AAA9999 filter of cv2_show_OCR_result (OCR/OCR.py:150-157), with the reference's own character lists."""
    return len(text) == 7 and all(ch in _ALPHABET for ch in text[:3]) and all(ch in _NUMBER for ch in text[3:])


# ---- structure (pure Python: the host tests use it without a device) ---------------------------------------------------------------
def round_up(a, b):
    return -(-a // b) * b


def stem_out_hw(H, W):
    """Conv 7x7 s2 p3 then MaxPool 3x3 s2 p1: floor((n + 6 - 7) / 2) + 1, then floor((n + 2 - 3) / 2) + 1."""
    f = lambda n: ((n - 1) // 2 + 1 - 1) // 2 + 1
    return f(H), f(W)


def block_channels(F0, G, block_config):
    """[(channels entering block i, channels leaving it)]: OCR 32->104, 52->196, 98->386."""
    out, c = [], F0
    for i, n in enumerate(block_config):
        out.append((c, c + n * G))
        c = (c + n * G) // 2 if i != len(block_config) - 1 else c + n * G
    return out


def block_maps(H, W, nblocks):
    """[(h, w)] of every block's map for an (H, W) input; a transition halves with floor."""
    h, w = stem_out_hw(H, W)
    out = []
    for _ in range(nblocks):
        out.append((h, w))
        h, w = h // 2, w // 2
    return out


def dense_param_shapes(F0, G, block_config, bn_size, head):
    """Ordered {name: shape} of a net's parameters.  head: ('ocr', KH, classes) or ('lpd', classes)."""
    P = {}

    def bn(name, c):
        for f in BN_FIELDS:
            P['%s.%s' % (name, f)] = (c,)
    P['stem.weight'] = (F0, 3, 7, 7)
    bn('stem', F0)
    Cm = bn_size * G
    chans = block_channels(F0, G, block_config)
    for s, n in enumerate(block_config):
        cin = chans[s][0]
        for k in range(n):
            pre = 'stage%d.layer%d.' % (s + 1, k)
            bn(pre + 'bn1', cin)
            P[pre + 'conv1.weight'] = (Cm, cin, 1, 1)
            bn(pre + 'bn2', Cm)
            P[pre + 'conv2.weight'] = (G, Cm, 3, 3)
            cin += G
        if s != len(block_config) - 1:
            bn('trans%d.bn' % (s + 1), cin)
            P['trans%d.conv.weight' % (s + 1)] = (cin // 2, cin, 1, 1)
    cf = chans[-1][1]
    bn('final.bn', cf)
    if head[0] == 'ocr':
        P['head.conv1.weight'] = (HEAD_WIDTH, cf, head[1], 1)
        nout = head[2] + 1
    else:
        P['head.conv1.weight'] = (HEAD_WIDTH, cf, 3, 3)
        nout = 7 + head[1]
    P['head.conv1.bias'] = (HEAD_WIDTH,)
    bn('head.bn', HEAD_WIDTH)
    P['head.conv2.weight'] = (nout, HEAD_WIDTH, 1, 1)
    P['head.conv2.bias'] = (nout,)
    return P


def pack_operand(A, torch_dtype):
    """The dense operand image (include/yolo_amd.h) of a matrix A (M, K): [M/16][K/32][64][8], lane l element j =
    A[16 mt + (l & 15)][32 kc + 8 (l >> 4) + j], zero padded."""
    M, K = A.shape
    Mp, Kp = round_up(M, 16), round_up(K, 32)
    P = torch.zeros((Mp, Kp), dtype=torch.float32, device=A.device)
    P[:M, :K] = A
    return P.view(Mp // 16, 16, Kp // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous().to(torch_dtype)


def conv3_matrix(w):
    """(G, Cm, 3, 3) -> (G, 9 * round_up(Cm, 32)): column (3 ky + kx) * Cmp + j."""
    G, Cm = w.shape[:2]
    Cmp = round_up(Cm, 32)
    m = torch.zeros((G, 9, Cmp), dtype=torch.float32, device=w.device)
    m[:, :, :Cm] = w.permute(0, 2, 3, 1).reshape(G, 9, Cm)
    return m.reshape(G, 9 * Cmp)


_MOMENTUM = object()       # placeholder of the per-call momentum in a cached argument tuple


class _Plan(object):
    def __init__(self):
        self.ops = []          # (name, function, argument tuple without the stream)
        self.keep = []         # tensors and descriptors the arguments point into
        self.out = None


class DenseNet(object):
    """The DenseNet body + a head chosen by the subclass.  Parameters follow CarNet's conventions: initialize(seed),
    load_params(dict), params, a version that makes forward re-fold and re-pack.  One cached launch list per input shape; nothing is
    allocated after the first call with a shape -- so net(x) returns the SAME output tensors for every call with that shape, and
    the next call overwrites them: clone what has to outlive it."""
    head = None      # ('ocr', KH, classes) / ('lpd', classes): set by the subclass before DenseNet.__init__

    def __init__(self, num_init_features, growth_rate, block_config, bn_size=4, dtype='bf16', device='cuda:0'):
        if dtype not in _TORCH_DT:
            raise ValueError("dtype must be 'bf16' or 'f32'")
        self.F0, self.G, self.block_config, self.bn_size = int(num_init_features), int(growth_rate), [int(n) for n in block_config], int(bn_size)
        self.Cm = self.bn_size * self.G
        if self.F0 % 8 or self.F0 > 64 or self.G % 4 or self.G > 32 or self.Cm % 16 or self.Cm > 128 or not self.block_config:
            raise L.YoloError('unsupported DenseNet: F0 %% 8 == 0, F0 <= 64, G %% 4 == 0, G <= 32, bn_size * G %% 16 == 0 and <= 128 '
                              '(got F0 %d, G %d, bn_size %d)' % (self.F0, self.G, self.bn_size))
        self.dtype = dtype
        self.device = L.resolve_device(device) if torch.device(device).type == 'cuda' and torch.cuda.is_available() else torch.device(device)
        self.channels = block_channels(self.F0, self.G, self.block_config)
        self.shapes = dense_param_shapes(self.F0, self.G, self.block_config, self.bn_size, self.head)
        self.params = {}
        self._prepared = {}
        self._plans = {}
        self._version = 0
        self._prepared_version = -1
        self._folds_stale = False     # a training forward has updated the running statistics since the last fold
        self._train_plans = {}
        self.batch_stats = {}
        self._lib = L.load()

    # ---- parameters ----------------------------------------------------------------------------------------------------------------
    def initialize(self, seed=0):
        """Xavier weights (mxnet.init.Xavier defaults, as init_NN uses), gamma 1, beta / mean 0, var 1, biases 0."""
        gen = torch.Generator(device='cpu').manual_seed(seed)
        for name, shp in self.shapes.items():
            if name.endswith('.weight'):
                fan = (shp[1] + shp[0]) * shp[2] * shp[3] / 2.0
                t = (torch.rand(shp, generator=gen) * 2 - 1) * math.sqrt(3.0 / fan)
            elif name.endswith('.gamma') or name.endswith('.running_var'):
                t = torch.ones(shp)
            else:
                t = torch.zeros(shp)
            self._set_param(name, t.to(self.device))
        self._version += 1
        return self

    def _set_param(self, name, t):
        old = self.params.get(name)
        if old is not None and old.shape == t.shape:
            old.copy_(t)
        else:
            self.params[name] = t

    def load_params(self, params):
        for name, shp in self.shapes.items():
            if name not in params:
                raise KeyError('missing parameter %s' % name)
            v = params[name]
            t = torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v
            if tuple(t.shape) != tuple(shp):
                raise ValueError('parameter %s has shape %s, expected %s' % (name, tuple(t.shape), tuple(shp)))
            self._set_param(name, t.detach().to(self.device, torch.float32).contiguous())
        self._version += 1
        return self

    def collect_params(self):
        return self.params

    def load_gluon_params(self, path):
        from . import mxparams
        return self.load_params(mxparams.dense_from_gluon(self, mxparams.read_params(path)))

    def save_gluon_params(self, path, prefix=None):
        from . import mxparams
        mxparams.write_params(path, mxparams.dense_to_gluon(self, self.params, prefix))

    # ---- one-off preparation: BN folding and operand images ------------------------------------------------------------------------
    def _fold(self, name, c, conv_bias=None):
        lib, st = self._lib, L.stream_ptr()
        cp = lib.yolo_padded_channels(c)
        if name in self._prepared:
            scale, bias = self._prepared[name]
        else:
            scale = torch.empty(cp, dtype=torch.float32, device=self.device)
            bias = torch.empty(cp, dtype=torch.float32, device=self.device)
            self._prepared[name] = (scale, bias)
        p = lambda f: L.ptr(self.params['%s.%s' % (name, f)])
        L.check(lib.yolo_fold_bn(p('gamma'), p('beta'), p('running_mean'), p('running_var'), BN_EPS, L.ptr(scale), L.ptr(bias), c, st),
                'fold ' + name)
        if conv_bias is not None:                     # BN((conv + b)) = conv * s + (beta - mean * s + b * s)
            bias[:c] += conv_bias * scale[:c]
        return scale, bias

    def _image(self, name, matrix):
        img = pack_operand(matrix, _TORCH_DT[self.dtype])
        old = self._prepared.get(name)
        if old is not None and old.shape == img.shape:
            old.copy_(img)
        else:
            self._prepared[name] = img

    def _packed_conv(self, name, w, k):
        """A yolo_pack_conv_weights image of OIHW weights w for the head's yolo_conv_fwd calls."""
        lib, st, dt = self._lib, L.stream_ptr(), _LIB_DT[self.dtype]
        cout, cin = w.shape[:2]
        nbytes = lib.yolo_packed_weight_bytes(cout, cin, k, dt)
        if nbytes < 0:
            raise L.YoloError('unsupported head convolution %s' % name)
        wp = self._prepared.get(name)
        if wp is None or wp.numel() != nbytes:
            wp = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._prepared[name] = wp
        w = w.contiguous()
        L.check(lib.yolo_pack_conv_weights(L.ptr(w), L.ptr(wp), cout, cin, k, dt, st), 'pack ' + name)
        torch.cuda.current_stream().synchronize()     # (w is a temporary)
        return wp

    def _plain_bias(self, name, b):
        lib, st = self._lib, L.stream_ptr()
        c = b.numel()
        cp = lib.yolo_padded_channels(c)
        if name not in self._prepared:
            self._prepared[name] = (torch.empty(cp, dtype=torch.float32, device=self.device),
                                    torch.empty(cp, dtype=torch.float32, device=self.device))
        scale, bias = self._prepared[name]
        L.check(lib.yolo_fold_bn(None, L.ptr(b), None, None, BN_EPS, L.ptr(scale), L.ptr(bias), c, st), 'bias ' + name)

    def prepare(self):
        L.require_current_device(self.device, 'this DenseNet')
        P = self.params
        if not P:
            raise L.YoloError('the net has no parameters: call initialize() or load_params()')
        self._fold_all()
        for s, n in enumerate(self.block_config):
            cin = self.channels[s][0]
            for k in range(n):
                pre = 'stage%d.layer%d.' % (s + 1, k)
                self._image(pre + 'conv1', P[pre + 'conv1.weight'].reshape(self.Cm, cin))
                self._image(pre + 'conv2', conv3_matrix(P[pre + 'conv2.weight']))
                cin += self.G
            if s != len(self.block_config) - 1:
                self._image('trans%d.conv' % (s + 1), P['trans%d.conv.weight' % (s + 1)].reshape(cin // 2, cin))
        cf = self.channels[-1][1]
        # the head's first convolution over the zero-padded Cp channels that yolo_dense_bn_relu writes
        w, Cp = P['head.conv1.weight'], round_up(cf, 32)
        wpad = torch.zeros((HEAD_WIDTH, Cp) + tuple(w.shape[2:]), dtype=torch.float32, device=self.device)
        wpad[:, :cf] = w
        if self.head[0] == 'ocr':                    # (KH, 1) without padding = 1x1 over the column layout: channel h * Cp + c
            KH = self.head[1]
            self._packed_conv('head.conv1', wpad[:, :, :, 0].permute(0, 2, 1).reshape(HEAD_WIDTH, KH * Cp, 1, 1), 1)
        else:
            self._packed_conv('head.conv1', wpad, 3)
        self._packed_conv('head.conv2', P['head.conv2.weight'], 1)
        self._plain_bias('head.conv2.b', P['head.conv2.bias'])
        self._plain_bias('head.conv1.b', P['head.conv1.bias'])       # the training forward's raw first convolution
        self._prepared_version = self._version
        return self

    def bn_names(self):
        """[(name, channels)] of every BatchNorm, in network order."""
        return [(k[:-len('.gamma')], shp[0]) for k, shp in self.shapes.items() if k.endswith('.gamma')]

    def _fold_all(self):
        """Every BatchNorm folded from its RUNNING statistics: what the inference path reads."""
        for name, c in self.bn_names():
            self._fold(name, c, conv_bias=self.params['head.conv1.bias'] if name == 'head.bn' else None)
        self._folds_stale = False

    def _ensure_prepared(self, folds=True):
        if self._prepared_version != self._version:
            self.prepare()
        elif folds and self._folds_stale:
            self._fold_all()

    # ---- the launch list of one input shape ------------------------------------------------------------------------------------------
    def _conv_desc(self, plan, x, wname, sbname, y, N, H, W, cin, cout, k, slope, out_f32):
        d = L.ConvDesc()
        scale, bias = self._prepared[sbname]
        d.x, d.w_packed, d.scale, d.bias, d.y = L.ptr(x), L.ptr(self._prepared[wname]), L.ptr(scale), L.ptr(bias), L.ptr(y)
        d.N, d.H, d.W, d.Cin, d.Cout = N, H, W, cin, cout
        d.ksize, d.stride, d.dtype, d.out_f32, d.slope = k, 1, _LIB_DT[self.dtype], 1 if out_f32 else 0, slope
        plan.keep.append(d)
        plan.ops.append((wname, self._lib.yolo_conv_fwd, (C.byref(d),)))

    def _build_plan(self, N, H, W):
        lib, dt, tdt = self._lib, _LIB_DT[self.dtype], _TORCH_DT[self.dtype]
        plan = _Plan()
        maps = block_maps(H, W, len(self.block_config))
        if min(maps[-1]) < 1:
            raise L.YoloError('a %dx%d input leaves no pixel after %d blocks' % (H, W, len(self.block_config)))
        pr = self._prepared
        bufs = [torch.empty((N, h, w, round_up(c1, 32)), dtype=tdt, device=self.device) for (h, w), (_, c1) in zip(maps, self.channels)]
        plan.keep += bufs
        plan.bufs = bufs
        s, b = pr['stem']
        # (the first argument, the image, is filled in by forward: the caller's tensor is read in place)
        plan.ops.append(('stem', lib.yolo_dense_stem_fwd, (None, L.ptr(self.params['stem.weight']), L.ptr(s), L.ptr(b),
                                                           L.ptr(bufs[0]), N, H, W, self.F0, bufs[0].shape[3], dt)))
        for si, n in enumerate(self.block_config):
            (h, w), buf, cin = maps[si], bufs[si], self.channels[si][0]
            Cs = buf.shape[3]
            for k in range(n):
                pre = 'stage%d.layer%d.' % (si + 1, k)
                s1, t1 = pr[pre + 'bn1']
                s2, t2 = pr[pre + 'bn2']
                plan.ops.append((pre[:-1], lib.yolo_dense_layer_fwd,
                                 (L.ptr(buf), L.ptr(pr[pre + 'conv1']), L.ptr(s1), L.ptr(t1), L.ptr(pr[pre + 'conv2']), L.ptr(s2), L.ptr(t2),
                                  N, h, w, Cs, cin, self.Cm, self.G, dt)))
                cin += self.G
            if si != len(self.block_config) - 1:
                s1, t1 = pr['trans%d.bn' % (si + 1)]
                plan.ops.append(('trans%d' % (si + 1), lib.yolo_dense_transition_fwd,
                                 (L.ptr(buf), L.ptr(pr['trans%d.conv' % (si + 1)]), L.ptr(s1), L.ptr(t1), L.ptr(bufs[si + 1]), N, h, w, cin,
                                  Cs, bufs[si + 1].shape[3], dt)))
        self._head_ops(plan, bufs[-1], N, maps[-1][0], maps[-1][1])
        return plan

    def _head_ops(self, plan, buf, N, h, w):
        raise NotImplementedError

    def _head_front(self, plan, buf, act, mid, N, h, w, conv_hw, conv_cin, k, columns):
        """The final BN + ReLU into act and the head's first convolution (+ its folded BN + ReLU) into mid; the subclass appends the
        rest of its head.  plan.head is what the training plan needs to restate these two steps with batch statistics."""
        lib, dt = self._lib, _LIB_DT[self.dtype]
        cf = self.channels[-1][1]
        s, b = self._prepared['final.bn']
        plan.ops.append(('final.bn', lib.yolo_dense_bn_relu, (L.ptr(buf), L.ptr(s), L.ptr(b), L.ptr(act), N, h, w, cf, buf.shape[3],
                                                               round_up(cf, 32), columns, dt)))
        self._conv_desc(plan, act, 'head.conv1', 'head.bn', mid, N, conv_hw[0], conv_hw[1], conv_cin, HEAD_WIDTH, k, 0.0, False)
        plan.head = dict(act=act, mid=mid, conv_hw=conv_hw, conv_cin=conv_cin, k=k, columns=columns, tail=len(plan.ops))

    def _plan(self, x, folds=True):
        if x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32:
            raise ValueError('input must be (B, 3, H, W) float32')
        if not x.is_contiguous() or x.device != self.device:
            # (read in place by the stem kernel: a silent copy would allocate on every call)
            raise ValueError('input must be a contiguous tensor on %s' % self.device)
        L.require_current_device(self.device, 'this DenseNet')
        self._ensure_prepared(folds)
        key = tuple(x.shape)
        plan = self._plans.get(key)
        if plan is None:
            plan = self._plans[key] = self._build_plan(x.shape[0], x.shape[2], x.shape[3])
        return plan

    def forward(self, x, training=False, momentum=0.9):
        """training=False: inference with the running statistics.  training=True: BatchNorm with the batch's statistics (see
        _forward_train); the same output tensors either way."""
        if training:
            return self._forward_train(x, momentum)
        plan = self._plan(x)
        st = L.stream_ptr()
        for name, fn, args in plan.ops:
            if args[0] is None:
                args = (L.ptr(x),) + args[1:]
            L.check(fn(*args, st), name)
        return plan.out

    __call__ = forward

    # ---- the train-mode forward ------------------------------------------------------------------------------------------------------
    def _batch_fold(self, tp, name, c, mean, var):
        """The yolo_bn_batch_fold of BatchNorm `name` over mean[:c] / var[:c]; its (scale, bias) pair is the training plan's own."""
        P = self.params
        cp = self._lib.yolo_padded_channels(c)
        scale = torch.empty(cp, dtype=torch.float32, device=self.device)
        bias = torch.empty(cp, dtype=torch.float32, device=self.device)
        d = L.BnBatchFold()
        d.gamma, d.beta = L.ptr(P[name + '.gamma']), L.ptr(P[name + '.beta'])
        d.running_mean, d.running_var = L.ptr(P[name + '.running_mean']), L.ptr(P[name + '.running_var'])
        d.scale, d.bias, d.C, d.eps, d.momentum = L.ptr(scale), L.ptr(bias), c, BN_EPS, 0.9
        tp.folds.append(d)
        tp.pairs[name] = (scale, bias)
        tp.stats[name] = (mean[:c], var[:c])
        return C.byref(d), scale, bias

    def _build_train_plan(self, plan, N, H, W):
        """The launch list of one training forward on the buffers and outputs of the inference plan of the same shape.  Per dense
        layer: the bottleneck's statistics (+ fold of BN2), the unchanged layer kernel, the statistics of the G channels it appended
        (+ fold of the NEXT BatchNorm over the block's channels: the next layer's BN1, the transition's or the final one)."""
        lib, dt, dev = self._lib, _LIB_DT[self.dtype], self.device
        pr, bufs = self._prepared, plan.bufs
        tp = _Plan()
        tp.folds, tp.pairs, tp.stats, tp.out, tp.bufs, tp.head = [], {}, {}, plan.out, bufs, plan.head
        f32 = lambda n: torch.empty(n, dtype=torch.float32, device=dev)
        widest = max([self.Cm, self.F0, HEAD_WIDTH] + [b.shape[3] for b in bufs])
        ws = torch.empty(lib.yolo_dense_stats_workspace_bytes(widest), dtype=torch.uint8, device=dev)
        maps = block_maps(H, W, len(self.block_config))
        nblocks = len(self.block_config)
        ops = tp.ops

        def next_bn(si, k):
            if k + 1 < self.block_config[si]:
                return 'stage%d.layer%d.bn1' % (si + 1, k + 1)
            return 'trans%d.bn' % (si + 1) if si != nblocks - 1 else 'final.bn'

        m, v = f32(self.F0), f32(self.F0)
        fd, s, b = self._batch_fold(tp, 'stem', self.F0, m, v)
        wstem = L.ptr(self.params['stem.weight'])
        ops.append(('stem.stats', lib.yolo_dense_stem_stats, (None, wstem, L.ptr(m), L.ptr(v), L.ptr(ws), fd, N, H, W, self.F0)))
        ops.append(('stem', lib.yolo_dense_stem_fwd, (None, wstem, L.ptr(s), L.ptr(b), L.ptr(bufs[0]), N, H, W, self.F0, bufs[0].shape[3], dt)))
        for si, n in enumerate(self.block_config):
            (h, w), buf, cin = maps[si], bufs[si], self.channels[si][0]
            Cs = buf.shape[3]
            bm, bv = f32(Cs), f32(Cs)                       # the block's channel statistics: every BN1 of the block is a view of them
            fd, s1, t1 = self._batch_fold(tp, 'stage%d.layer0.bn1' % (si + 1), cin, bm, bv)
            ops.append(('stage%d.stats' % (si + 1), lib.yolo_dense_channel_stats, (L.ptr(buf), L.ptr(bm), L.ptr(bv), L.ptr(ws), fd, N, h, w, Cs, 0, cin, dt)))
            for k in range(n):
                pre = 'stage%d.layer%d.' % (si + 1, k)
                m2, v2 = f32(self.Cm), f32(self.Cm)
                fd, s2, t2 = self._batch_fold(tp, pre + 'bn2', self.Cm, m2, v2)
                ops.append((pre + 'bn2.stats', lib.yolo_dense_bottleneck_stats,
                            (L.ptr(buf), L.ptr(pr[pre + 'conv1']), L.ptr(s1), L.ptr(t1), L.ptr(m2), L.ptr(v2), L.ptr(ws), fd, N, h, w, Cs, cin,
                             self.Cm, dt)))
                ops.append((pre[:-1], lib.yolo_dense_layer_fwd,
                            (L.ptr(buf), L.ptr(pr[pre + 'conv1']), L.ptr(s1), L.ptr(t1), L.ptr(pr[pre + 'conv2']), L.ptr(s2), L.ptr(t2),
                             N, h, w, Cs, cin, self.Cm, self.G, dt)))
                fd, s1, t1 = self._batch_fold(tp, next_bn(si, k), cin + self.G, bm, bv)
                ops.append((pre + 'stats', lib.yolo_dense_channel_stats, (L.ptr(buf), L.ptr(bm), L.ptr(bv), L.ptr(ws), fd, N, h, w, Cs, cin, self.G, dt)))
                cin += self.G
            if si != nblocks - 1:
                ops.append(('trans%d' % (si + 1), lib.yolo_dense_transition_fwd,
                            (L.ptr(buf), L.ptr(pr['trans%d.conv' % (si + 1)]), L.ptr(s1), L.ptr(t1), L.ptr(bufs[si + 1]), N, h, w, cin,
                             Cs, bufs[si + 1].shape[3], dt)))
        # the head: final BN + ReLU with the folded pair, the first convolution RAW (scale 1, its bias), yolo_bn_train_fwd in place
        hd, (h, w), buf, cf = plan.head, maps[-1], bufs[-1], self.channels[-1][1]
        ops.append(('final.bn', lib.yolo_dense_bn_relu, (L.ptr(buf), L.ptr(s1), L.ptr(t1), L.ptr(hd['act']), N, h, w, cf, buf.shape[3],
                                                          round_up(cf, 32), hd['columns'], dt)))
        ch, cw = hd['conv_hw']
        self._conv_desc(tp, hd['act'], 'head.conv1', 'head.conv1.b', hd['mid'], N, ch, cw, hd['conv_cin'], HEAD_WIDTH, hd['k'], 1.0, False)
        hm, hv, hinv = f32(HEAD_WIDTH), f32(HEAD_WIDTH), f32(HEAD_WIDTH)
        tp.stats['head.bn'], tp.head_invstd = (hm, hv), hinv
        ops.append(('head.bn.stats', lib.yolo_dense_channel_stats, (L.ptr(hd['mid']), L.ptr(hm), L.ptr(hv), L.ptr(ws), None, N, ch, cw, HEAD_WIDTH,
                                                                     0, HEAD_WIDTH, dt)))
        bnws = torch.zeros(2 * HEAD_WIDTH, dtype=torch.float64, device=dev)          # zero on entry, left zero by every call
        hmean = f32(HEAD_WIDTH)
        P = self.params
        ops.append(('head.bn', lib.yolo_bn_train_fwd,
                    (L.ptr(hd['mid']), L.ptr(P['head.bn.gamma']), L.ptr(P['head.bn.beta']), None, L.ptr(hd['mid']), L.ptr(hmean), L.ptr(hinv),
                     L.ptr(P['head.bn.running_mean']), L.ptr(P['head.bn.running_var']), L.ptr(bnws), N * ch * cw, HEAD_WIDTH, BN_EPS,
                     _MOMENTUM, 0.0, dt)))
        ops += plan.ops[hd['tail']:]
        tp.keep += [ws, bnws, hmean, plan]
        return tp

    def _train_plan(self, x):
        plan = self._plan(x, folds=False)                    # (the running statistics are not read: no re-fold for a training call)
        tp = self._train_plans.get(tuple(x.shape))
        if tp is None or tp.version != self._prepared_version:       # (a plan holds pointers to the parameters it was built with)
            tp = self._train_plans[tuple(x.shape)] = self._build_train_plan(plan, x.shape[0], x.shape[2], x.shape[3])
            tp.version = self._prepared_version
        return tp

    def _forward_train(self, x, momentum):
        """One forward pass with batch statistics.  Every BatchNorm's running statistics in `params` are updated in place (running =
        momentum * running + (1 - momentum) * batch, the biased variance: Gluon) and the net is marked for re-folding, so the next
        inference call folds the updated statistics.  net.batch_stats = {bn name: (mean, var)} float32 device tensors for every
        BatchNorm of dense_param_shapes (the BN1 entries of one block are views of one array): the state a backward pass reads,
        OVERWRITTEN by the next training call with this input shape.  Nothing is allocated after the first such call."""
        momentum = float(momentum)
        if not 0.0 <= momentum <= 1.0:
            raise ValueError('momentum must lie in [0, 1]')
        tp = self._train_plan(x)
        for d in tp.folds:
            d.momentum = momentum
        st, xp = L.stream_ptr(), L.ptr(x)
        for name, fn, args in tp.ops:
            if args[0] is None:
                args = (xp,) + args[1:]
            elif name == 'head.bn':
                args = tuple(momentum if a is _MOMENTUM else a for a in args)
            L.check(fn(*args, st), name)
        self._folds_stale = True
        self.batch_stats = tp.stats
        return tp.out

    def training_buffers(self, x):
        """For the tests' stage-by-stage comparison: what the last training (or inference) forward with x's shape left in the block
        buffers [(N, h, w, Cs)], the head's activated input and its hidden map."""
        plan = self._plans[tuple(x.shape)]
        return dict(blocks=plan.bufs, act=plan.head['act'], mid=plan.head['mid'])

    def recalibrate_bn(self, batches):
        """Re-estimates every BatchNorm's running statistics on `batches` (an iterable of input tensors): the training forward on
        each, the k-th at momentum 1 - 1 / k, so that the running statistics end as the plain average of the batches' statistics
        (the first batch replaces what was loaded).  Weights, gamma and beta are untouched.  Returns the number of batches."""
        k = 0
        for x in batches:
            k += 1
            self._forward_train(x, 1.0 - 1.0 / k)
        if k == 0:
            raise ValueError('recalibrate_bn needs at least one batch')
        return k

    @property
    def launches(self):
        """Kernel launches of one forward pass (the same for every input shape)."""
        return 1 + sum(self.block_config) + (len(self.block_config) - 1) + self._head_launches

    @property
    def train_launches(self):
        """Kernel launches of one training forward: a statistics entry is two (partial rows, finish + fold), yolo_bn_train_fwd three.
        Stem 3 + 2, a dense layer 2 + 1 + 2, a transition 1 + 2, the head's BatchNorm 2 + 3 more than in inference."""
        return 5 + 5 * sum(self.block_config) + 3 * (len(self.block_config) - 1) + self._head_launches + 5


class OCRNet(DenseNet):
    """OCRDenseNet(32, 12, [6, 12, 24], classes=34) (OCR/OCR.py:34-74): net(x) takes (B, 3, 160, 384) float32 0..1 on the device and
    returns [score_x (B, 1, W', 1), class_x (B, 1, W', classes)] float32 logits, W' = 24.  size fixes the head's (KH, 1) kernel: KH =
    the final map's height for that input height (10); other widths are accepted as they come."""
    _head_launches = 3       # final BN into the column layout, two 1x1 convolutions

    def __init__(self, classes=34, num_init_features=32, growth_rate=12, block_config=(6, 12, 24), bn_size=4, size=(160, 384),
                 dtype='bf16', device='cuda:0'):
        self.classes, self.size = int(classes), tuple(size)
        KH = block_maps(size[0], size[1], len(block_config))[-1][0]
        if KH < 1:
            raise L.YoloError('input height %d leaves no row after %d blocks' % (size[0], len(block_config)))
        self.head = ('ocr', KH, self.classes)
        DenseNet.__init__(self, num_init_features, growth_rate, block_config, bn_size, dtype, device)

    def _head_ops(self, plan, buf, N, h, w):
        if h != self.head[1]:
            raise L.YoloError("the final map is %d rows high, the head's kernel %d: build the net with size=(H, W) of its inputs" % (h, self.head[1]))
        lib, dt, tdt = self._lib, _LIB_DT[self.dtype], _TORCH_DT[self.dtype]
        cf, Cp, nout = self.channels[-1][1], round_up(self.channels[-1][1], 32), self.classes + 1
        cols = torch.empty((N, 1, w, h * Cp), dtype=tdt, device=self.device)
        mid = torch.empty((N, 1, w, HEAD_WIDTH), dtype=tdt, device=self.device)
        logits = torch.empty((N, 1, w, nout), dtype=torch.float32, device=self.device)
        plan.keep += [cols, mid, logits]
        self._head_front(plan, buf, cols, mid, N, h, w, (1, w), h * Cp, 1, 1)
        self._conv_desc(plan, mid, 'head.conv2', 'head.conv2.b', logits, N, 1, w, HEAD_WIDTH, nout, 1, 1.0, True)
        plan.logits = logits
        plan.out = [logits[..., :1], logits[..., 1:]]

    def logits(self, x, training=False, momentum=0.9):
        """(B, W', 1 + classes) float32: score and class logits side by side, as yolo_ocr_decode reads them (a view of the cached
        output: overwritten by the next call with this shape).  training=True: the train-mode forward (DenseNet.forward)."""
        self.forward(x, training, momentum)
        return self.held_logits(x)

    def held_logits(self, x):
        """The same view WITHOUT running the net: what the last forward pass with x's shape left (PlateReader.read_device has just
        run it)."""
        lg = self._plans[tuple(x.shape)].logits
        return lg.view(lg.shape[0], lg.shape[2], lg.shape[3])


class LPDenseNet(DenseNet):
    """LPDenseNet (licence_plate/LP_detection.py:59-97) built from a spec's num_init_features, growth_rate, block_config and
    LP_num_class (licence_plate/v2/spec.yaml: 64, 16, [6, 12, 24, 16], 3): net(x) returns (B, 7 + classes, h, w) float32, what
    yolo_predict_lp takes."""
    _head_launches = 4       # final BN, 3x3, 1x1, NHWC -> NCHW

    def __init__(self, spec, bn_size=4, dtype='bf16', device='cuda:0'):
        self.classes = int(spec['LP_num_class'])
        self.head = ('lpd', self.classes)
        DenseNet.__init__(self, spec['num_init_features'], spec['growth_rate'], spec['block_config'], bn_size, dtype, device)

    def _head_ops(self, plan, buf, N, h, w):
        lib, dt, tdt = self._lib, _LIB_DT[self.dtype], _TORCH_DT[self.dtype]
        cf, Cp, nout = self.channels[-1][1], round_up(self.channels[-1][1], 32), 7 + self.classes
        act = torch.empty((N, h, w, Cp), dtype=tdt, device=self.device)
        mid = torch.empty((N, h, w, HEAD_WIDTH), dtype=tdt, device=self.device)
        nhwc = torch.empty((N, h, w, nout), dtype=torch.float32, device=self.device)
        out = torch.empty((N, nout, h, w), dtype=torch.float32, device=self.device)
        plan.keep += [act, mid, nhwc, out]
        self._head_front(plan, buf, act, mid, N, h, w, (h, w), Cp, 3, 0)
        self._conv_desc(plan, mid, 'head.conv2', 'head.conv2.b', nhwc, N, h, w, HEAD_WIDTH, nout, 1, 1.0, True)
        plan.ops.append(('nchw', lib.yolo_nhwc_to_nchw, (L.ptr(nhwc), L.ptr(out), N, nout, h, w, L.F32)))
        plan.out = out


class PlateReader(object):
    """OCR.predict (OCR/OCR.py:180-201) on the device: the net, a sigmoid, the strict peak rule and the class argmax at the peaks.

        overlay = FrameOverlay(..., LP_size=(160, 384))
        frames, clipped, lp_valid = overlay(frames, pred=pred, lp=lp)
        texts = PlateReader(ocr_net).read(clipped, lp_valid)

    FrameOverlay rectifies the plate with one bilinear tap at the OCR's size, where the reference clips at 160x380 and then
    cv2.resizes to 160x384: the same kind of picture, not the same pixels.  threshold: 0.6 in predict, 0.2 in valid."""

    def __init__(self, net, threshold=0.6, names=OCR_NAMES):
        if len(names) < net.classes:
            raise ValueError('%d names for %d classes' % (len(names), net.classes))
        self.net, self.threshold, self.names = net, float(threshold), list(names)
        self._out = {}

    def read_device(self, plates, valid=None):
        """(score (N, W') float32, codes (N, W') int32: the class at a peak and -1 elsewhere, count (N) int32), on the device,
        without synchronising.  valid (N) uint8 / bool on the net's device: a row with 0 reads as no peaks.  The three tensors are
        cached per (N, W') and overwritten by the next call with that shape: clone them to keep two frames' results side by side."""
        net = self.net
        lg = net.logits(plates)
        N, Wp = lg.shape[0], lg.shape[1]
        if valid is not None:
            if valid.dtype == torch.bool:
                valid = valid.view(torch.uint8)
            if valid.dtype != torch.uint8 or valid.numel() != N or not valid.is_contiguous() or valid.device != net.device:
                raise ValueError('valid must be (N) uint8 or bool, contiguous, on %s' % net.device)
        out = self._out.get((N, Wp))
        if out is None:
            out = self._out[(N, Wp)] = (torch.empty((N, Wp), dtype=torch.float32, device=net.device),
                                        torch.empty((N, Wp), dtype=torch.int32, device=net.device),
                                        torch.empty((N,), dtype=torch.int32, device=net.device))
        L.check(net._lib.yolo_ocr_decode(L.ptr(lg), L.ptr(valid), L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]), N, Wp, net.classes,
                                         self.threshold, L.stream_ptr()), 'ocr decode')
        return out

    @property
    def launches(self):
        return self.net.launches + 1

    def read(self, plates, valid=None):
        """The texts, one str per plate: one D2H copy (of the codes)."""
        codes = self.read_device(plates, valid)[1].cpu().numpy()
        return [''.join(self.names[c] for c in row if c >= 0) for row in codes]
