"""CPU checks of the evaluation: average precision by hand and against tests/eval_ref.py, Evaluator's numpy finish on fuzzed
records, the two C ABI entries (declared, bound, argument counts, revision still 5, NULL arguments refused without a GPU) and
the built kernels (no scratch, scalar memory only loaded)."""
import ctypes as C
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import eval_ref as er
from yolo_amd import lib as L
from yolo_amd import evaluate as ev
from test_isa_lint import LLVM, _device_code_objects

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'yolo_amd.h')
NEW = ('yolo_eval_match', 'yolo_eval_top1')
KERNELS = ['eval_match_kernel', 'eval_top1_kernel']


def test_ap_known_answer_five_ninths():
    """Scores .9 .8 .7 .6, flags TP FP TP FP, three ground truths: recall 1/3 1/3 2/3 2/3, precision 1 1/2 2/3 1/2; the
    envelope is 1 up to recall 1/3 and 2/3 up to recall 2/3, nothing beyond: AP = 1/3 * 1 + 1/3 * 2/3 = 5/9."""
    by_hand = Fraction(1, 3) * 1 + (Fraction(2, 3) - Fraction(1, 3)) * Fraction(2, 3)
    assert by_hand == Fraction(5, 9)
    ap, prec, rec, sc = ev.average_precision([.9, .8, .7, .6], [1, 0, 1, 0], 3)
    assert abs(ap - 5.0 / 9.0) < 1e-15
    np.testing.assert_allclose(prec, [1, .5, 2. / 3, .5], rtol=1e-15)
    np.testing.assert_allclose(rec, [1. / 3, 1. / 3, 2. / 3, 2. / 3], rtol=1e-15)
    assert sc.tolist() == [np.float32(v) for v in (.9, .8, .7, .6)]
    ref, _, _ = er.ap_all_point([(.9, 0, 0, 1), (.8, 0, 1, 0), (.7, 0, 2, 1), (.6, 0, 3, 0)], 3)
    assert abs(ref - 5.0 / 9.0) < 1e-15
    # the same records given out of rank order
    assert abs(ev.average_precision([.6, .9, .7, .8], [0, 1, 1, 0], 3)[0] - 5.0 / 9.0) < 1e-15


def test_ap_edge_cases():
    assert ev.average_precision([.9, .5, .4], [1, 1, 1], 3)[0] == 1.0                     # all TP
    for n in (7, 49, 100, 1000):                                                          # ... exactly, whatever the count
        assert ev.average_precision(np.linspace(1, .1, n), np.ones(n, np.int32), n)[0] == 1.0
    assert ev.average_precision([], [], 4)[0] == 0.0                                      # no detections
    assert ev.average_precision([.9, .8], [0, 0], 2)[0] == 0.0
    # a class without ground truth is excluded from mAP (and has no AP), whatever was detected as it
    det_class = np.asarray([[0, 1, 1, -1]], np.int32)
    det_tp = np.asarray([[1, 0, 0, -1]], np.int32)
    det_score = np.asarray([[.9, .8, .7, 0]], np.float32)
    gt_class = np.asarray([[0, -1]], np.int32)
    top1 = np.asarray([[.7, 0.1, 1.0, 1.0]], np.float32)
    r = ev.finish(det_class, det_tp, det_score, gt_class, top1, [0.0], 3)
    assert r['ap'][0] == 1.0 and np.isnan(r['ap'][1]) and np.isnan(r['ap'][2]) and r['mAP'] == 1.0
    assert r['n_gt'].tolist() == [1, 0, 0] and r['n_det'].tolist() == [1, 2, 0] and r['images'] == 1
    # nothing at all
    e = ev.finish(np.zeros((0, 4), np.int32), np.zeros((0, 4), np.int32), np.zeros((0, 4), np.float32), np.zeros((0, 1), np.int32),
                  np.zeros((0, 4), np.float32), np.zeros(0, np.float32), 2)
    assert e['images'] == 0 and np.isnan(e['mAP']) and np.isnan(e['mean_iou']) and e['azimuth_images'] == 0


def test_ap_ties_keep_image_slot_order():
    """Equal scores rank in (image, slot) order: FP first then TP gives AP 1/2, TP first gives 1."""
    assert ev.average_precision([.5, .5], [0, 1], 1)[0] == 0.5
    assert ev.average_precision([.5, .5], [1, 0], 1)[0] == 1.0
    assert er.ap_all_point([(.5, 0, 1, 1), (.5, 0, 0, 0)], 1)[0] == 0.5       # (slot 0, the FP, ranks first)
    # through finish(): image 0 slot 1 and image 1 slot 0 tie with image 0 slot 0
    det_class = np.zeros((2, 2), np.int32)
    det_score = np.full((2, 2), .25, np.float32)
    det_tp = np.asarray([[0, 1], [1, 0]], np.int32)
    r = ev.finish(det_class, det_tp, det_score, np.zeros((2, 2), np.int32), np.zeros((2, 4), np.float32), np.zeros(2), 1)
    want = er.ap_all_point([(.25, i, k, det_tp[i, k]) for i in range(2) for k in range(2)], 4)[0]
    # precision 0, 1/2, 2/3, 1/2 at recall 0, 1/4, 2/4, 2/4: the envelope is 2/3 up to recall 1/2 -> AP = 1/2 * 2/3
    assert abs(r['ap'][0] - want) < 1e-15 and abs(want - 1.0 / 3.0) < 1e-15
    assert r['pr'][0]['precision'].tolist() == [0.0, 0.5, 2. / 3, 0.5]


@pytest.mark.parametrize('seed', [0, 1, 2, 3])
def test_finish_equals_the_restatement_on_fuzzed_records(seed):
    rng = np.random.default_rng(seed)
    images, post_nms, nobj, ncls = 9, 12, 5, 4
    det_class = rng.integers(-1, ncls, (images, post_nms)).astype(np.int32)
    det_tp = np.where(det_class < 0, -1, rng.integers(0, 2, (images, post_nms))).astype(np.int32)
    det_score = (rng.integers(1, 20, (images, post_nms)) / 20.0).astype(np.float32)       # many ties
    gt_class = rng.integers(-1, ncls if seed else ncls - 1, (images, nobj)).astype(np.int32)    # (seed 0: a class without ground truth)
    top1 = rng.random((images, 4), dtype=np.float32)
    top1[:, 1] = (top1[:, 1] - 0.5) * 2 * np.pi
    top1[:, 3] = rng.integers(0, 2, images)
    az = (rng.random(images) * 360).astype(np.float32)
    got = ev.finish(det_class, det_tp, det_score, gt_class, top1, az, ncls)
    want = er.summarise(det_class, det_tp, det_score, gt_class, top1, az, ncls)
    assert got['images'] == want['images'] and got['azimuth_images'] == want['azimuth_images']
    assert got['n_gt'].tolist() == want['n_gt'] and got['n_det'].tolist() == want['n_det']
    np.testing.assert_allclose(got['ap'], want['ap'], rtol=0, atol=1e-12, equal_nan=True)
    np.testing.assert_allclose([got['mAP'], got['mean_iou'], got['azimuth_rmse_deg']],
                               [want['mAP'], want['mean_iou'], want['azimuth_rmse_deg']], rtol=1e-12, equal_nan=True)
    for c in range(ncls):
        _, prec, rec = er.ap_all_point([(det_score[i, k], i, k, det_tp[i, k]) for i in range(images) for k in range(post_nms)
                                        if det_class[i, k] == c], want['n_gt'][c])
        np.testing.assert_allclose(got['pr'][c]['precision'], prec, rtol=1e-15)
        np.testing.assert_allclose(got['pr'][c]['recall'], rec, rtol=1e-15)


def test_evaluator_is_exported_lazily():
    import yolo_amd
    assert yolo_amd.Evaluator is ev.Evaluator


def test_eval_entries_declared_and_bound():
    h = open(HEADER).read()
    assert int(re.search(r'#define YOLO_ABI_VERSION (\d+)', h).group(1)) == L.ABI_VERSION == 5
    for name in NEW:
        assert re.search(r'\b%s\(' % name, h), name
        assert name in L.SIGNATURES, name
        proto = re.search(r'(?:int|long long) %s\(([^)]*)\)' % name, h).group(1)
        assert len(proto.split(',')) == len(L.SIGNATURES[name][1]), name


def test_eval_entries_refuse_null_and_bad_sizes_without_a_gpu(lib):
    assert lib.yolo_version() == 5
    p = C.c_void_p(4096)                   # never dereferenced: validation comes before any launch
    f = C.c_float
    ok_m = [p, p, p, p, 2, 100, 30, 24, 100, 4, 30, 1, f(0.5), p, p, p, p, p, None]
    for k in (0, 1, 2, 3, 13, 14, 15, 16, 17):
        a = list(ok_m)
        a[k] = None
        assert lib.yolo_eval_match(*a) == L.EINVAL, k
    for k in (4, 5, 7, 8, 9):
        a = list(ok_m)
        a[k] = 0
        assert lib.yolo_eval_match(*a) == L.EINVAL, k
    for k, v in ((6, 4), (10, 4), (11, 2)):
        a = list(ok_m)
        a[k] = v
        assert lib.yolo_eval_match(*a) == L.EINVAL, k
    a = list(ok_m); a[9] = 513
    assert lib.yolo_eval_match(*a) == L.EUNSUPPORTED
    a = list(ok_m); a[8] = 1025
    assert lib.yolo_eval_match(*a) == L.EUNSUPPORTED
    assert lib.yolo_eval_match_supported(512, 1024) == 1 and lib.yolo_eval_match_supported(513, 100) == 0
    assert lib.yolo_eval_match_supported(1, 1025) == 0 and lib.yolo_eval_match_supported(0, 100) == L.EINVAL
    ok_t = [p, p, p, p, 2, 30, 1, 30, None]
    for k in (0, 1, 2, 3):
        a = list(ok_t)
        a[k] = None
        assert lib.yolo_eval_top1(*a) == L.EINVAL, k
    for k, v in ((4, 0), (5, 6), (6, 0), (7, 4)):
        a = list(ok_t)
        a[k] = v
        assert lib.yolo_eval_top1(*a) == L.EINVAL, k


def test_eval_kernels_have_no_scratch(tmp_path):
    readelf = os.path.join(LLVM, 'llvm-readelf')
    if not os.path.exists(readelf) or not shutil.which('make') or not shutil.which('c++filt'):
        pytest.skip('no ROCm LLVM tools here')
    L.build()
    so = os.path.join(L.CSRC, 'libyolo_amd.so')
    found = {}
    for co in _device_code_objects(so, str(tmp_path)):
        notes = subprocess.run([readelf, '--notes', co], capture_output=True, text=True, check=True).stdout
        blocks = notes.split('- .agpr_count:')[1:]
        names = [dict(re.findall(r'\.(\w+):\s+(\S+)', '.agpr_count:' + b.split('\n    - .a')[0])) for b in blocks]
        dem = subprocess.run(['c++filt'], input='\n'.join(f.get('name', '?') for f in names), capture_output=True, text=True).stdout.split('\n')
        for f, d in zip(names, dem):
            for pat in KERNELS:
                if pat in d:
                    found.setdefault(pat, []).append((d, int(f.get('private_segment_fixed_size', -1))))
    assert sorted(found) == sorted(KERNELS), 'evaluation kernels not in the library: %s' % sorted(set(KERNELS) - set(found))
    spilled = [(d, s) for v in found.values() for d, s in v if s != 0]
    assert not spilled, 'evaluation kernels with scratch: %s' % spilled


# The scalar-memory (SMEM) encoding of gfx9-family code: the first dword's bits [31:26] are 0b110000.
SMEM_ALLOWED = ('s_load_', 's_buffer_load_', 's_dcache_inv', 's_memtime', 's_memrealtime')


def test_eval_kernels_scalar_memory_is_loads_only(tmp_path):
    objdump = os.path.join(LLVM, 'llvm-objdump')
    if not os.path.exists(objdump) or not shutil.which('make') or not shutil.which('c++filt'):
        pytest.skip('no ROCm LLVM tools here')
    L.build()
    so = os.path.join(L.CSRC, 'libyolo_amd.so')
    seen, smem, other = set(), 0, []
    for co in _device_code_objects(so, str(tmp_path)):
        dis = subprocess.run([objdump, '-d', '--demangle', '--mcpu=gfx950', co], capture_output=True, text=True, check=True).stdout
        for sym in re.split(r'\n(?=[0-9a-f]+ <)', dis):
            m = re.match(r'[0-9a-f]+ <(.*)>:\s*$', sym.split('\n', 1)[0])
            hit = [p for p in KERNELS if m and p in m.group(1)]
            if not hit:
                continue
            seen.update(hit)
            for ln in sym.split('\n'):
                e = re.search(r'//\s*[0-9A-Fa-f]+:\s*([0-9A-Fa-f]{8})', ln)
                if e and (int(e.group(1), 16) >> 26) == 0b110000:
                    smem += 1
                    if not ln.strip().startswith(SMEM_ALLOWED):
                        other.append(ln.strip())
    assert set(KERNELS) <= seen, 'evaluation kernels not found in the disassembly: %s' % sorted(set(KERNELS) - seen)
    assert smem > 0, 'no scalar-memory instruction recognised: the encoding column of the disassembly changed?'
    assert not other, other[:5]
