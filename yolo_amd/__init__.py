"""yolo_amd: MI355X (gfx950) native YOLOv3 hot path -- Darknet-style backbone + 3-scale heads,
anchor decode, top-1 / NMS -- as hand-written HIP kernels behind a C ABI (include/yolo_amd.h)."""
from .spec import NetGraph, ConvSpec, darknet53_spec      # noqa: F401


def __getattr__(name):
    # torch-dependent pieces are imported lazily so `import yolo_amd` works in tooling contexts
    if name in ('CarNet', 'CarLPNet'):
        from . import net
        return getattr(net, name)
    if name in ('Detector', 'get_iou', 'cv_img_2_ndarray', 'make_grid', 'predict_LP', 'predict_LP_batch', 'predict_LP_rows', 'default_ltrb'):
        from . import detect
        return getattr(detect, name)
    if name == 'Evaluator':
        from . import evaluate
        return evaluate.Evaluator
    if name in ('FrameIntake', 'intake_matrix', 'warp_u8', 'rectify_plates'):
        from . import intake
        return getattr(intake, name)
    if name in ('RenderCar', 'SpriteAtlas', 'LPGenerator', 'PlateCamera'):
        from . import render
        return getattr(render, name)
    if name == 'BackgroundBank':
        from . import background
        return background.BackgroundBank
    if name in ('FrameOverlay', 'BitmapFont', 'default_font'):
        from . import overlay
        return getattr(overlay, name)
    if name in ('fit_anchors', 'sample_sizes', 'anchor_quality', 'AnchorFit'):
        from . import anchors
        return getattr(anchors, name)
    if name in ('DenseNet', 'OCRNet', 'LPDenseNet', 'PlateReader', 'OCR_NAMES', 'plate_format_ok'):
        from . import dense
        return getattr(dense, name)
    if name in ('OCRValidator', 'ocr_targets', 'ocr_loss', 'ocr_score'):
        from . import ocr
        return getattr(ocr, name)
    raise AttributeError(name)
