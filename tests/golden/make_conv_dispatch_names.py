"""Fixture for tests/test_conv_dispatch_host.py: what the conv dispatcher answers, host only, over a grid of descriptors.

For every query: the status of yolo_conv_kernel_name, the kernel instantiation it names, and -- where the descriptor carries
statistics -- what yolo_conv_stats_rows returns.  A refactor of the dispatcher must leave every answer as it is; a pull request
that changes a choice on purpose regenerates the file and says which answers moved.

Generate it from a build of the commit BEFORE the change, never from the code under test:

    YOLO_AMD_LIB=/path/to/parent/libyolo_amd.so python tests/golden/make_conv_dispatch_names.py

Stored: names (the distinct kernel names, sorted), codes int16 (index into names, or the negative status), rows int32
(NO_ROWS where the query has no statistics), and the grid's size as a guard against an edited grid.
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'conv_dispatch_names.npz')
NO_ROWS = -9
P = 4096                     # any non-NULL pointer: the queries launch nothing

BATCHES = (1, 32)
MAPS = ((13, 13), (26, 26), (52, 52), (19, 19), (7, 5), (104, 104))
CHANNELS = ((32, 64), (64, 32), (128, 256), (256, 128), (512, 1024), (1024, 512), (24, 40), (256, 75))
WINDOWS = ((1, 1), (3, 1), (3, 2))
DTYPES = ('bf16', 'f16', 'f32', 'bf16x3', 'f16x3')
UNASSIGNED = (15, 29, 34, 44)


def _pad32(c):
    return (c + 31) // 32 * 32


# name -> (fields, split element types only).  ci / co: the shape's channels.
VARIANTS = (
    ('plain', lambda ci, co: {}, False),
    ('residual', lambda ci, co: dict(residual=P), False),
    ('out_f32', lambda ci, co: dict(out_f32=1), False),
    ('upsample2x', lambda ci, co: dict(upsample2x=1), False),
    ('stats1', lambda ci, co: dict(stats=P, stats_mode=1), False),
    ('stats2', lambda ci, co: dict(stats=P, stats_mode=2, stats_y=P, stats_mean=P, stats_invstd=P, stats_gamma=P, stats_beta=P), False),
    ('tail', lambda ci, co: dict(tail_w_packed=P, tail_y=P, tail_cout=128, tail_slope=0.1), False),
    # x and y as channel slices of wider buffers (room for two padded planes, so the split types accept it too)
    ('strided', lambda ci, co: dict(x_pixel_stride=2 * _pad32(ci) + 32, y_pixel_stride=2 * _pad32(co) + 32), False),
    # the lo planes 32 elements behind the padded hi planes
    ('lo_offset', lambda ci, co: dict(x_pixel_stride=2 * _pad32(ci) + 64, x_lo_offset=_pad32(ci) + 32,
                                      y_pixel_stride=2 * _pad32(co) + 64, y_lo_offset=_pad32(co) + 32), True),
    # a lo plane that overlaps the hi plane: refused
    ('lo_overlap', lambda ci, co: dict(x_lo_offset=_pad32(ci) - 8), True),
)


def queries():
    """(shape, dtype name, variant name, id, fields) in the fixture's order.  shape = (N, Cin, H, W, Cout, k, stride)."""
    from yolo_amd.net import CarNet
    ids = (0,) + tuple(CarNet.ALGOS) + UNASSIGNED
    for N in BATCHES:
        for (H, W) in MAPS:
            for (ci, co) in CHANNELS:
                for (k, s) in WINDOWS:
                    for dn in DTYPES:
                        for vn, fields, split_only in VARIANTS:
                            if split_only and not dn.endswith('x3'):
                                continue
                            f = fields(ci, co)
                            for a in ids:
                                yield (N, ci, H, W, co, k, s), dn, vn, a, f


def walk(lib, L):
    """Every query against `lib`: (keys, status list, name list, rows list)."""
    dts = {'bf16': L.BF16, 'f16': L.F16, 'f32': L.F32, 'bf16x3': L.BF16X3, 'f16x3': L.F16X3}
    buf = C.create_string_buffer(256)
    keys, rcs, names, rows = [], [], [], []
    for sh, dn, vn, a, f in queries():
        N, ci, H, W, co, k, s = sh
        d = L.ConvDesc()
        d.x = d.w_packed = d.y = d.scale = d.bias = P
        d.N, d.H, d.W, d.Cin, d.Cout, d.ksize, d.stride, d.dtype, d.slope, d.algo = N, H, W, ci, co, k, s, dts[dn], 0.1, a
        for name, val in f.items():
            setattr(d, name, val)
        buf.value = b''
        rc = lib.yolo_conv_kernel_name(C.byref(d), buf, 256)
        keys.append((sh, dn, vn, a))
        rcs.append(rc)
        names.append(buf.value.decode() if rc == 0 else '')
        rows.append(lib.yolo_conv_stats_rows(C.byref(d)) if 'stats' in f else NO_ROWS)
    return keys, rcs, names, rows


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from yolo_amd import lib as L
    if not os.environ.get('YOLO_AMD_LIB'):
        sys.exit('set YOLO_AMD_LIB to a build of the parent commit (see the docstring)')
    keys, rcs, names, rows = walk(L.load(), L)
    table = sorted({n for n, rc in zip(names, rcs) if rc == 0})
    index = {n: i for i, n in enumerate(table)}
    codes = np.array([index[n] if rc == 0 else rc for n, rc in zip(names, rcs)], dtype=np.int16)
    rows = np.array(rows, dtype=np.int32)
    np.savez_compressed(OUT, names=np.array(table), codes=codes, rows=rows, n_queries=np.int64(len(keys)))
    print('%d queries, %d accepted, %d distinct kernel names, statuses %s, %d positive row counts, %d bytes' % (
        len(keys), sum(rc == 0 for rc in rcs), len(table), sorted(set(rcs)), int((rows > 0).sum()), os.path.getsize(OUT)))
    for vn, _, _ in VARIANTS:
        sel = [rc for (sh, dn, v, a), rc in zip(keys, rcs) if v == vn]
        print('  %-10s %6d queries, %5d accepted, statuses %s' % (vn, len(sel), sum(rc == 0 for rc in sel), sorted(set(sel))))


if __name__ == '__main__':
    main()
