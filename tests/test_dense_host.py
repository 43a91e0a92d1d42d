"""DenseNet bodies, OCR reading rule and their parameter files without a GPU: the shape arithmetic of the OCR and LPD-v2 instances,
tests/dense_ref.py against itself (float32 vs float64), gluon parameter names and a .params round trip, the peak rule on crafted
columns, plate_format_ok, and the error codes of every new entry (validation comes before any launch)."""
import numpy as np
import pytest
import torch

import dense_ref as R
from yolo_amd import dense as D
from yolo_amd import lib as L
from yolo_amd import mxparams as M

MICRO = dict(F0=16, G=8, blocks=[2, 3, 2], bn_size=4)


def test_ocr_instance_arithmetic():
    assert D.block_channels(32, 12, [6, 12, 24]) == [(32, 104), (52, 196), (98, 386)]
    assert D.block_maps(160, 384, 3) == [(40, 96), (20, 48), (10, 24)]
    shapes = D.dense_param_shapes(32, 12, [6, 12, 24], 4, ('ocr', 10, 34))
    assert shapes['head.conv1.weight'] == (512, 386, 10, 1) and shapes['head.conv2.weight'] == (35, 512, 1, 1)
    assert shapes['stage3.layer23.conv1.weight'] == (48, 386 - 12, 1, 1) and shapes['stage1.layer0.conv2.weight'] == (12, 48, 3, 3)
    assert shapes['trans2.conv.weight'] == (98, 196, 1, 1)
    assert D.round_up(386, 32) * 10 == 4160                 # the K of the head's first convolution as a 1x1
    assert len(D.OCR_NAMES) == 34 and 'I' not in D.OCR_NAMES and 'O' not in D.OCR_NAMES


def test_lpd_v2_instance_arithmetic():
    assert D.block_channels(64, 16, [6, 12, 24, 16]) == [(64, 160), (80, 272), (136, 520), (260, 516)]
    assert D.block_maps(320, 512, 4) == [(80, 128), (40, 64), (20, 32), (10, 16)]
    shapes = D.dense_param_shapes(64, 16, [6, 12, 24, 16], 4, ('lpd', 3))
    assert shapes['head.conv1.weight'] == (512, 516, 3, 3) and shapes['head.conv2.weight'] == (10, 512, 1, 1)
    assert max(c for _, c in D.block_channels(64, 16, [6, 12, 24, 16])) == 520


def test_stem_and_transition_sizes_floor():
    assert D.stem_out_hw(21, 37) == (6, 10)                  # conv 11 x 19, pool floor((n + 2 - 3) / 2) + 1
    assert D.block_maps(52, 602, 3) == [(13, 151), (6, 75), (3, 37)]


def test_dense_ref_f32_against_f64():
    shapes = D.dense_param_shapes(16, 8, [2, 3, 2], 4, ('ocr', 3, 5))
    P = R.random_params(shapes, 3)
    x = torch.rand((2, 3, 52, 90), generator=torch.Generator().manual_seed(4))
    o64 = R.ocr_forward(MICRO, P, x, R.Mode('f64'))
    o32 = R.ocr_forward(MICRO, P, x, R.Mode('f32'))
    ob = R.ocr_forward(MICRO, P, x, R.Mode('bf16'))
    assert o64.shape == (2, 1, 5, 6) and o64.dtype == torch.float64 and o32.dtype == torch.float32
    assert float(o64.std()) > 0.05
    assert R.rel_err(o32, o64) < 1e-5
    assert 1e-5 < R.rel_err(ob, o32) < 0.1                   # the emulation does round, and not absurdly


def test_dense_ref_pads_the_activated_map():
    """With t2 > 0 everywhere, padding the 1x1's output instead of the activated map changes the border pixels."""
    shapes = D.dense_param_shapes(16, 8, [1], 4, ('ocr', 1, 2))
    P = R.random_params(shapes, 5)
    pre = 'stage1.layer0.'
    P[pre + 'bn2.beta'] = P[pre + 'bn2.beta'].abs() + 2.0
    x = torch.rand((1, 16, 4, 5), generator=torch.Generator().manual_seed(6))
    mode = R.Mode('f32')
    y = R.dense_layer(x, P, pre, mode)[:, 16:]
    s1, t1 = R.fold(P, pre + 'bn1', mode)
    s2, t2 = R.fold(P, pre + 'bn2', mode)
    assert float(t2.min()) > 0
    m = torch.nn.functional.conv2d(R.affine_relu(x, s1, t1), P[pre + 'conv1.weight'])
    m = torch.nn.functional.pad(m, (1, 1, 1, 1))            # the WRONG rule: pad m, then activate
    wrong = torch.nn.functional.conv2d(R.affine_relu(m, s2, t2), P[pre + 'conv2.weight'])
    assert torch.allclose(y[:, :, 1:-1, 1:-1], wrong[:, :, 1:-1, 1:-1], atol=1e-5)
    assert float((y - wrong).abs().max()) > 0.1


def test_gluon_dense_param_names():
    n = M.gluon_dense_param_names('ocr', 32, 12, [6, 12, 24])
    theirs = list(n.values())
    assert len(theirs) == len(set(theirs)) == len(D.dense_param_shapes(32, 12, [6, 12, 24], 4, ('ocr', 10, 34)))
    assert n['stem.weight'] == 'ocrdensenet0_conv0_weight' and n['stem.gamma'] == 'ocrdensenet0_batchnorm0_gamma'
    assert n['stage2.layer3.bn1.beta'] == 'ocrdensenet0_stage2_batchnorm6_beta'
    assert n['stage2.layer3.conv2.weight'] == 'ocrdensenet0_stage2_conv7_weight'
    assert n['trans1.conv.weight'] == 'ocrdensenet0_conv1_weight' and n['trans2.bn.gamma'] == 'ocrdensenet0_batchnorm2_gamma'
    assert n['final.bn.running_var'] == 'ocrdensenet0_batchnorm3_running_var'
    assert n['head.conv1.bias'] == 'ocrdensenet0_conv3_bias' and n['head.conv2.bias'] == 'ocrdensenet0_conv4_bias'
    assert n['head.bn.beta'] == 'ocrdensenet0_batchnorm4_beta'
    top = set(t.split('_')[1] for t in theirs if 'stage' not in t)
    assert top == set('conv%d' % i for i in range(5)) | set('batchnorm%d' % i for i in range(5))
    lp = M.gluon_dense_param_names('lpd', 64, 16, [6, 12, 24, 16])
    assert lp['head.conv2.weight'] == 'lpdensenet0_conv5_weight' and lp['final.bn.gamma'] == 'lpdensenet0_batchnorm4_gamma'
    with pytest.raises(ValueError):
        M.gluon_dense_param_names('car', 64, 16, [6])


class _Shape(object):
    """What mxparams needs to know of a net (no device)."""
    def __init__(self, kind, F0, G, blocks, head):
        self.head, self.F0, self.G, self.block_config, self.bn_size = head, F0, G, blocks, 4
        self.shapes = D.dense_param_shapes(F0, G, blocks, 4, head)


def test_params_round_trip(tmp_path):
    net = _Shape('ocr', 16, 8, [2, 3, 2], ('ocr', 3, 5))
    P = {k: v.numpy() for k, v in R.random_params(net.shapes, 7).items()}
    path = str(tmp_path / 'ocr.params')
    # another net prefix and shifted counters, in scrambled order: a second net of one process, written through a Python-2 dict
    named = M.dense_to_gluon(net, P, prefix='ocrdensenet3_')
    shifted = {}
    for k, v in named.items():
        if 'stage' not in k:
            kind = 'conv' if '_conv' in k else 'batchnorm'
            i = int(k.split(kind)[1].split('_')[0])
            k = k.replace('%s%d_' % (kind, i), '%s%d_' % (kind, i + 11))
        shifted[k] = v
    keys = sorted(shifted, key=lambda s: hash(s) % 1009)
    M.write_params(path, {k: shifted[k] for k in keys})
    back = M.dense_from_gluon(net, M.read_params(path))
    assert sorted(back) == sorted(P)
    for k in P:
        assert np.array_equal(back[k], P[k]), k
    bad = dict(shifted)
    bad.pop(next(k for k in bad if k.endswith('conv15_bias')))
    with pytest.raises(M.ParamsFormatError):
        M.dense_from_gluon(net, bad)


def test_peak_rule_on_crafted_columns():
    z = lambda p: float(np.log(p / (1 - p)))
    ncls = 4
    cols = [0.9, 0.3, 0.7, 0.7, 0.1, 0.65, 0.61, 0.3, 0.5, 0.8]      # peaks: 0; equal neighbours 2, 3: neither; 5; 9
    lg = np.zeros((len(cols), 1 + ncls))
    lg[:, 0] = [z(p) for p in cols]
    lg[:, 1:] = np.arange(ncls)[None, :] * 0.1
    lg[5, 1:] = [2.0, 2.0, 1.0, 2.0]                                # a tie: the first index wins
    score, codes = R.read_columns(lg, 0.6)
    assert np.allclose(score, cols)
    assert codes.tolist() == [3, -1, -1, -1, -1, 0, -1, -1, -1, 3]
    assert R.text_of(codes, 'ABCD') == 'DAD'
    _, codes2 = R.read_columns(lg, 0.2)
    assert codes2.tolist() == codes.tolist()                        # 0.5 at column 8 is below its right neighbour
    lg[9, 0] = z(0.4)
    assert R.read_columns(lg, 0.2)[1].tolist() == [3, -1, -1, -1, -1, 0, -1, -1, 3, -1]
    assert R.read_columns(lg, 0.6)[1].tolist() == [3, -1, -1, -1, -1, 0, -1, -1, -1, -1]


def test_plate_format_ok():
    assert D.plate_format_ok('ABC1235')
    assert not D.plate_format_ok('ABC123')           # length
    assert not D.plate_format_ok('AB11235')
    assert not D.plate_format_ok('ABCD235')
    assert not D.plate_format_ok('AIC1235')          # no I in the reference's alphabet
    assert not D.plate_format_ok('ABC1245')          # ... and no 4 in its digits (OCR/OCR.py:30)
    assert not D.plate_format_ok('')


def test_dtype_is_checked():
    with pytest.raises(ValueError):
        D.OCRNet(dtype='f16')
    with pytest.raises(ValueError):
        D.LPDenseNet(dict(num_init_features=16, growth_rate=8, block_config=[2], LP_num_class=3), dtype='bf16x3')


def test_launch_count():
    assert D.OCRNet().launches + 1 <= 42 + 2 + 8
    assert D.PlateReader(D.OCRNet()).launches <= 42 + 2 + 8


# ---- error codes: nothing is launched, so any non-NULL integer stands for a pointer -------------------------------------------------
P_ = 0x1000


def test_dense_layer_rejects(lib):
    ok = dict(N=1, H=5, W=7, Cs=64, Cin=32, Cm=48, G=12, dtype=L.BF16)

    def call(buf=P_, w1=P_, s1=P_, t1=P_, w2=P_, s2=P_, t2=P_, **kw):
        a = dict(ok, **kw)
        return lib.yolo_dense_layer_fwd(buf, w1, s1, t1, w2, s2, t2, a['N'], a['H'], a['W'], a['Cs'], a['Cin'], a['Cm'], a['G'], a['dtype'], None)
    for name in ('buf', 'w1', 's1', 't1', 'w2', 's2', 't2'):
        assert call(**{name: None}) == L.EINVAL, name
    for name in ('N', 'H', 'W', 'Cs', 'Cin', 'Cm', 'G'):
        assert call(**{name: 0}) == L.EINVAL and call(**{name: -3}) == L.EINVAL, name
    assert call(dtype=9) == L.EINVAL
    for dt in (L.F16, L.BF16X3, L.F16X3):
        assert call(dtype=dt) == L.EUNSUPPORTED
    for kw in (dict(G=10), dict(G=36, Cs=96), dict(Cm=40), dict(Cm=144), dict(Cin=4), dict(Cin=56), dict(Cs=48), dict(Cin=53, G=12)):
        assert call(**kw) == L.EUNSUPPORTED, kw
    assert call(N=4096, H=512, W=512, Cs=64, dtype=L.F32) == L.EUNSUPPORTED          # 2^32 bytes
    assert call(N=2, H=4096, W=4096, Cs=32, Cin=16, dtype=L.BF16) == L.EUNSUPPORTED  # exactly 2^31 bytes


def test_stem_transition_bn_relu_reject(lib):
    stem = lambda x=P_, w=P_, s=P_, t=P_, y=P_, N=1, H=20, W=20, F0=16, Cs=32, dt=L.BF16: lib.yolo_dense_stem_fwd(x, w, s, t, y, N, H, W, F0, Cs, dt, None)
    assert [stem(x=None), stem(w=None), stem(s=None), stem(t=None), stem(y=None)] == [L.EINVAL] * 5
    assert [stem(N=0), stem(H=0), stem(W=-1), stem(F0=0), stem(Cs=0), stem(dt=7)] == [L.EINVAL] * 6
    assert [stem(F0=12), stem(F0=72, Cs=96), stem(Cs=40), stem(F0=64, Cs=32), stem(dt=L.F16)] == [L.EUNSUPPORTED] * 5
    assert stem(N=64, H=2048, W=2048, dt=L.F32) == L.EUNSUPPORTED
    tr = lambda x=P_, w=P_, s=P_, t=P_, y=P_, N=1, H=6, W=8, C=104, ci=128, co=64, dt=L.BF16: lib.yolo_dense_transition_fwd(x, w, s, t, y, N, H, W, C, ci, co, dt, None)
    assert [tr(x=None), tr(w=None), tr(s=None), tr(t=None), tr(y=None)] == [L.EINVAL] * 5
    assert [tr(N=0), tr(H=0), tr(W=0), tr(C=0), tr(ci=0), tr(co=-1), tr(dt=-1)] == [L.EINVAL] * 7
    assert [tr(H=1), tr(W=1), tr(ci=96), tr(co=32), tr(ci=100), tr(dt=L.BF16X3)] == [L.EUNSUPPORTED] * 6
    assert tr(N=8192, H=512, W=512, C=32, ci=32, co=32) == L.EUNSUPPORTED
    br = lambda x=P_, s=P_, t=P_, y=P_, N=1, H=3, W=9, C=50, Cs=64, Cp=64, col=1, dt=L.F32: lib.yolo_dense_bn_relu(x, s, t, y, N, H, W, C, Cs, Cp, col, dt, None)
    assert [br(x=None), br(s=None), br(t=None), br(y=None)] == [L.EINVAL] * 4
    assert [br(N=0), br(H=0), br(W=0), br(C=0), br(Cs=0), br(Cp=0), br(dt=5)] == [L.EINVAL] * 7
    assert [br(Cs=32), br(Cp=32), br(dt=L.F16X3)] == [L.EUNSUPPORTED] * 3
    assert br(N=4096, H=512, W=512, Cs=64, Cp=64) == L.EUNSUPPORTED
    assert lib.yolo_dense_operand_bytes(48, 44, L.BF16) == 48 * 64 * 2 and lib.yolo_dense_operand_bytes(12, 9 * 64, L.F32) == 16 * 576 * 4
    assert lib.yolo_dense_operand_bytes(0, 4, L.BF16) == L.EINVAL and lib.yolo_dense_operand_bytes(4, 4, L.F16) == L.EUNSUPPORTED


def test_ocr_decode_rejects(lib):
    dec = lambda lg=P_, v=None, s=P_, c=P_, n=P_, N=2, Wp=24, ncls=34: lib.yolo_ocr_decode(lg, v, s, c, n, N, Wp, ncls, 0.6, None)
    assert [dec(lg=None), dec(s=None), dec(c=None), dec(n=None)] == [L.EINVAL] * 4
    assert [dec(N=0), dec(Wp=0), dec(ncls=0), dec(N=-1)] == [L.EINVAL] * 4
    assert dec(N=1 << 20, Wp=1 << 10, ncls=34) == L.EUNSUPPORTED
    assert dec(N=1 << 14, Wp=1 << 10, ncls=31) == L.EUNSUPPORTED           # exactly 2^31 BYTES of logits (2^29 elements)


def test_pack_operand_layout():
    A = torch.arange(20 * 40, dtype=torch.float32).reshape(20, 40)
    img = D.pack_operand(A, torch.float32)
    assert img.shape == (2, 2, 4, 16, 8) and img.numel() * 4 == 32 * 64 * 4
    flat = img.reshape(2, 2, 64, 8)
    for mt, kc, lane, j in ((0, 0, 0, 0), (0, 1, 37, 5), (1, 0, 19, 7), (1, 1, 3, 2), (1, 1, 63, 7)):
        r, c = 16 * mt + (lane & 15), 32 * kc + 8 * (lane >> 4) + j
        want = float(A[r, c]) if r < 20 and c < 40 else 0.0
        assert float(flat[mt, kc, lane, j]) == want
    w = torch.arange(4 * 16 * 9, dtype=torch.float32).reshape(4, 16, 3, 3)
    m = D.conv3_matrix(w)
    assert m.shape == (4, 9 * 32) and float(m[2, 5 * 32 + 7]) == float(w[2, 7, 1, 2]) and float(m[2, 5 * 32 + 16]) == 0.0
