"""What the conv dispatcher chooses, pinned on the host: yolo_conv_kernel_name and yolo_conv_stats_rows launch nothing, so the grid of
tests/golden/make_conv_dispatch_names.py (shapes x element types x descriptor variants x every id, algo 0 included) is replayed
against the built library and compared with the answers recorded from the commit before the dispatcher was last restructured."""
import importlib.util
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _generator():
    spec = importlib.util.spec_from_file_location('make_conv_dispatch_names', os.path.join(GOLDEN, 'make_conv_dispatch_names.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_conv_dispatch_answers_are_the_recorded_ones(lib):
    """Status, kernel name and (with statistics) partial-row count of every query equal the fixture's."""
    from yolo_amd import lib as L
    gen = _generator()
    want = np.load(os.path.join(GOLDEN, 'conv_dispatch_names.npz'))
    table = [str(n) for n in want['names']]
    codes, rows = want['codes'], want['rows']
    keys, rcs, names, got_rows = gen.walk(lib, L)
    assert len(keys) == int(want['n_queries']) == len(codes) == len(rows), 'the grid and the fixture differ in size: regenerate it from the parent commit'
    assert len(keys) >= 453600 and (codes >= 0).sum() > 60000 and (rows > 0).sum() > 4000        # (the fixture is the full grid, not a stub)
    diffs = []
    for i, key in enumerate(keys):
        old = (0, table[codes[i]]) if codes[i] >= 0 else (int(codes[i]), '')
        new = (rcs[i], names[i])
        if old != new or int(rows[i]) != got_rows[i]:
            diffs.append('%s: recorded status %d %r rows %d, now status %d %r rows %d' % (key, old[0], old[1], int(rows[i]), new[0], new[1], got_rows[i]))
    assert not diffs, '%d of %d queries answer differently (shape = N, Cin, H, W, Cout, k, stride); the first:\n  %s' % (
        len(diffs), len(keys), '\n  '.join(diffs[:8]))
