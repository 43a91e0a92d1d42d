"""yolo_amd/tuner.py without a GPU or a built library: the selection rules under scripted timers and launchers, the Tuner's modes,
dry run, keys and state.  Each rule was paid for with a wrong pick on a real box (NOTES.md); here it is pinned on the host."""
import json

import pytest

from yolo_amd import lib as L
from yolo_amd import plans
from yolo_amd import tuner as T


class Script(object):
    """A launcher and a timer that answer from a script.  launch(algo) -> status (non-zero for the ids in `refused`); time follows
    tuner.hip_time's contract -- one status launch, None when it is non-zero -- and answers the next scripted value for
    (what ran, launches).  `log` holds every (what, launches, windows) the timer was asked for."""
    def __init__(self, times, refused=()):
        self.times = {k: list(v) for k, v in times.items()}
        self.refused, self.log, self.last = set(refused), [], None

    def launch(self, algo):
        self.last = algo
        return 3 if algo in self.refused else 0

    def fn(self, name):
        def run():
            return self.launch(name)
        return run

    def time(self, fn, launches, windows=1):
        status = fn()
        self.log.append((self.last, launches, windows))
        return None if status else self.times[(self.last, launches)].pop(0)


def never(*a, **k):
    raise AssertionError('the timer was called')


def desc(N=32, H=13, W=13, Cin=512, Cout=1024, k=3, stride=1, dtype=L.BF16, **kw):
    d = L.ConvDesc()
    d.N, d.H, d.W, d.Cin, d.Cout, d.ksize, d.stride, d.dtype = N, H, W, Cin, Cout, k, stride, dtype
    for name, v in kw.items():
        setattr(d, name, v)
    return d


# ---- the rules ---------------------------------------------------------------------------------------------------------------
def test_conv_rule_two_passes_interleaved_top_three():
    """A is fastest in the short pass, B in the interleaved rounds: B.  The refused id 5 is asked once and never again; 4, fourth in
    the short pass, is not re-timed; exactly the top three are, three rounds each, interleaved, at twice the launches."""
    s = Script({(1, 5): [1.0], (2, 5): [1.1], (3, 5): [1.2], (4, 5): [2.0],
                (1, 10): [1.30, 1.25, 1.30], (2, 10): [1.20, 1.05, 1.20], (3, 10): [1.5, 1.5, 1.5]}, refused=[5])
    assert T.pick_conv((4, 5, 3, 2, 1), s.launch, s.time) == 2
    assert s.log[:5] == [(4, 5, 1), (5, 5, 1), (3, 5, 1), (2, 5, 1), (1, 5, 1)]
    assert s.log[5:] == [(1, 10, 1), (2, 10, 1), (3, 10, 1)] * 3
    assert all(not v for v in s.times.values())                       # every scripted answer was used: nothing else was timed


def test_conv_rule_keeps_each_candidates_fastest_round_and_returns_1_when_none_ran():
    s = Script({(1, 5): [1.0], (2, 5): [2.0], (1, 10): [3.0, 0.9, 3.0], (2, 10): [1.0, 1.0, 1.0]})
    assert T.pick_conv((1, 2), s.launch, s.time) == 1                # (0.9 beats 1.0 although two of 1's rounds were slower)
    s = Script({}, refused=[1, 2, 3])
    assert T.pick_conv((1, 2, 3), s.launch, s.time) == 1
    assert s.log == [(1, 5, 1), (2, 5, 1), (3, 5, 1)]


@pytest.mark.parametrize('later, want', [(0.99, 0), (0.97, 2)])
def test_wgrad_rule_a_later_candidate_must_win_by_two_per_cent(later, want):
    s = Script({(0, 6): [1.0], (2, 6): [later], (3, 6): [1.0]}, refused=[4])
    assert T.pick_wgrad((0, 2, 3, 4), s.launch, s.time) == want
    assert s.log == [(0, 6, 1), (2, 6, 1), (3, 6, 1), (4, 6, 1)]


def test_wgrad_rule_single_candidate_or_none_ran():
    assert T.pick_wgrad((0,), never, never) == 0
    s = Script({}, refused=[0, 1, 5])
    assert T.pick_wgrad((0, 1, 5), s.launch, s.time) == 0


def test_fused_rule_needs_a_strict_gain():
    for fused, want in ((1.0, False), (0.999, True), (1.001, False)):
        s = Script({('fused', 20): [fused], ('separate', 20): [1.0]})
        assert T.pick_fused(s.fn('fused'), s.fn('separate'), s.time, windows=3) is want
        assert s.log == [('fused', 20, 3), ('separate', 20, 3)]
    s = Script({}, refused=['fused'])                                 # the library refuses the fused launch: separate, untimed
    assert T.pick_fused(s.fn('fused'), s.fn('separate'), s.time) is False and s.log == [('fused', 20, 1)]


def test_timing_helper_warms_up_per_window_and_keeps_the_best(monkeypatch):
    """hip_time on a scripted clock: per window two warm-up launches outside the events and `launches` inside; the fastest window
    per launch; None as soon as a window's first launch reports a status."""
    import torch
    clock = {'t': 0.0, 'calls': 0, 'cost': [5.0] * 2 + [2.0] * 4 + [9.0] * 2 + [1.0] * 4 + [7.0] * 2 + [3.0] * 4}

    class Event(object):
        def __init__(self, enable_timing=False):
            self.t = None

        def record(self):
            self.t = clock['t']

        def synchronize(self):
            pass

        def elapsed_time(self, other):
            return other.t - self.t

    def fn():
        clock['t'] += clock['cost'][clock['calls']]
        clock['calls'] += 1
    monkeypatch.setattr(torch.cuda, 'Event', Event)
    assert T.hip_time(fn, 4, windows=3) == 1.0 and clock['calls'] == 18
    clock.update(t=0.0, calls=0)
    assert T.hip_time(fn, 4) == 2.0 and clock['calls'] == 6
    assert T.hip_time(lambda: 3, 4) is None


# ---- the Tuner ---------------------------------------------------------------------------------------------------------------
KEY = (32, 13, 13, 512, 1024, 3, 1, 0, False, 1)                      # desc()'s key: held by profiles/plan.json


def plan_file(tmp_path, state):
    path = str(tmp_path / 'plan.json')
    plans.save(path, plans.merge(state), {'commit': 'test'})
    return path


def test_key_function_literal_tuples():
    assert T.conv_key(desc()) == KEY
    assert T.conv_key(desc(residual=4096)) == (32, 13, 13, 512, 1024, 3, 1, 0, True, 1)
    assert T.conv_key(desc(H=26, W=26, k=3, stride=2, x_pixel_stride=1024)) == (32, 26, 26, 512, 1024, 3, 2, 0, False, 1, 1024, 0, 0)
    up = desc(Cin=1024, Cout=512, k=1, upsample2x=1, y_pixel_stride=1024)
    assert T.conv_key(up) == (32, 13, 13, 1024, 512, 1, 1, 0, False, 1, 0, 1, 1024)
    head = dict(Cin=1024, Cout=30, k=1, y_pixel_stride=30, y_batch_stride=30 * 10647)
    assert T.conv_key(desc(out_f32=1, **head)) == (32, 13, 13, 1024, 30, 1, 1, 1, False, 1)              # fp32 logits: no extension
    assert T.conv_key(desc(out_f32=0, **head)) == (32, 13, 13, 1024, 30, 1, 1, 0, False, 1, 0, 0, 30)
    assert T.conv_key(desc(Cin=128, Cout=256, H=52, W=52, residual=4096), ('tail', 128, 0)) == \
        (32, 52, 52, 128, 256, 3, 1, 0, True, 1, 'tail', 128, 0)
    held = plans.load(plans.DEFAULT)[0]['algo']
    assert KEY in held and T.conv_key(up) in held and T.conv_key(desc(H=26, W=26, k=3, stride=2, x_pixel_stride=1024)) in held


def test_auto_mode_applies_nothing():
    t = T.Tuner('auto', valid=never, time=never)
    assert (t.applies, t.live) == (False, False)
    d = desc()
    assert t.conv(d, (1, 2), never) == 0 and t.wgrad(('k',), (0, 1), never) == 0 and t.dgrad(('k',), never) == 0
    assert t.fused(('res', 1), True, never) is True and t.fused(('tail', 1), False, never) is False
    assert t.state() == {'algo': {}, 'dgrad': {}, 'wgrad': {}}
    with pytest.raises(ValueError):
        T.Tuner('fastest')


def test_plan_mode_missing_shape_gets_the_heuristic_and_nothing_is_timed(tmp_path):
    held = {'algo': {KEY: 7, ('res', 32, 208, 208, 64, 1): 0, ('tail', 9): 1}, 'dgrad': {('s2', (1, 2, 3, 4), 4, 2, 0): 6},
            'wgrad': {(64, 13, 13, 512, 1024, 3, 1): 3}}
    t = T.Tuner('plan', plan_file(tmp_path, held), valid=lambda d: True, time=never)
    assert (t.applies, t.live) == (True, False) and t.plan_meta['commit'] == 'test' and t.plan_meta['md5'] == plans.md5(held)
    # held shapes
    assert t.conv(desc(), (1, 2), never) == 7
    assert t.fused(('res', 32, 208, 208, 64, 1), True, never) is False and t.fused(('tail', 9), False, never) is True
    assert t.wgrad((64, 13, 13, 512, 1024, 3, 1), (0, 2, 3), never) == 3
    assert t.dgrad(('s2', (1, 2, 3, 4), 4, 2, 0), never) == 6
    # missing shapes: a variant 0, 'res' True, 'tail' False, a weight gradient 0 -- none of them recorded
    assert t.conv(desc(N=2), (1, 2), never) == 0
    assert t.fused(('res', 2, 8, 8, 64, 1), True, never) is True and t.fused(('tail', 2), False, never) is False
    assert t.wgrad((2, 13, 13, 512, 1024, 3, 1), (0, 2, 3), never) == 0
    assert t.state() == held and t.stale == 0
    # ... but a missing data-gradient shape is recorded, as a copy of the forward key space's answer (0, or a held forward choice)
    d = desc(N=2)
    assert t.dgrad(((2, 13, 13, 512), 512, 1024, 3, False), lambda: t.conv(d, (1, 2), never)) == 0
    assert t.dgrad(((32, 13, 13, 512), 512, 1024, 3, False), lambda: t.conv(desc(), (1, 2), never)) == 7
    assert plans.new_keys(t.state(), held) == 2 and t.state()['algo'] == held['algo']


def test_measure_mode_times_a_missing_shape_once_and_never_a_held_one():
    s = Script({(1, 5): [2.0], (2, 5): [1.0], (1, 10): [2.0] * 3, (2, 10): [1.0] * 3, ('fused', 20): [1.0, 1.0], ('separate', 20): [2.0, 0.5],
                (0, 6): [1.0], (5, 6): [0.5]})
    t = T.Tuner('measure', time=s.time)
    d = desc()
    assert t.conv(d, (1, 2), lambda: s.launch(d.algo)) == 2 and d.algo == 0
    assert t.fused(('res', 1), True, lambda: (s.fn('fused'), s.fn('separate'))) is True
    assert t.fused(('tail', 1), False, lambda: (s.fn('fused'), s.fn('separate')), windows=3) is False
    assert [e for e in s.log if e[0] == 'fused'] == [('fused', 20, 1), ('fused', 20, 3)]          # the tail: best of three windows
    order = []

    def bracket(pick):
        order.append('wait')
        best = pick(s.launch)
        order.append('rejoin')
        return best
    assert t.wgrad(('w',), (0, 5), bracket) == 5 and order == ['wait', 'rejoin']
    assert t.wgrad(('w1',), (0,), never) == 0                          # one candidate: recorded, no stream wait, no timing
    assert t.dgrad(('d',), lambda: t.conv(desc(), (1, 2), never)) == 2     # a data gradient with a forward conv's key reuses its choice
    want = {'algo': {KEY: 2, ('res', 1): 1, ('tail', 1): 0}, 'dgrad': {('d',): 2}, 'wgrad': {('w',): 5, ('w1',): 0}}
    assert t.state() == want
    # every shape is held now: a second Tuner loaded with the state answers without a timer
    u = T.Tuner('measure', time=never)
    u.load(want)
    assert u.conv(desc(), (1, 2), never) == 2 and u.fused(('res', 1), False, never) is True and u.fused(('tail', 1), True, never) is False
    assert u.wgrad(('w',), (0, 5), never) == 5 and u.dgrad(('d',), never) == 2 and u.state() == want
    # loading the 'algo' section alone (CarNet.load_tuning_state) leaves the gradient sections empty
    v = T.Tuner('measure', time=never)
    v.load(want, ('algo',))
    assert v.state() == dict(want, dgrad={}, wgrad={}) and v.state(('algo',)) == {'algo': want['algo']}


def test_dry_run_drops_a_refused_choice(tmp_path):
    refuse7 = lambda d: d.algo != 7
    s = Script({(1, 5): [1.0], (1, 10): [1.0] * 3})
    t = T.Tuner('measure', valid=refuse7, time=s.time)
    t.load({'algo': {KEY: 7}}, ('algo',))
    d = desc()
    assert t.conv(d, (1,), lambda: s.launch(d.algo)) == 1 and t.stale == 1 and len(s.log) == 4        # measured again
    assert t.state()['algo'] == {KEY: 1}
    # tune='plan': dropped and counted, the heuristic's answer, nothing timed
    p = T.Tuner('plan', plan_file(tmp_path, {'algo': {KEY: 7}}), valid=refuse7, time=never)
    assert p.conv(desc(), (1,), never) == 0 and p.stale == 1 and p.state()['algo'] == {}
    # not validated: a held 1 ("none ran"), another entry point's ids (dry_run=False), a choice the validator takes
    q = T.Tuner('plan', plan_file(tmp_path, {'algo': {KEY: 1, T.conv_key(desc(k=2)): 7, T.conv_key(desc(N=2)): 8}}),
                valid=lambda d: d.algo == 8, time=never)
    assert q.conv(desc(), (1,), never) == 1 and q.conv(desc(k=2), (2, 6), never, dry_run=False) == 7
    d = desc(N=2)
    assert q.conv(d, (1,), never) == 8 and d.algo == 0 and q.stale == 0 and len(q.state()['algo']) == 3


def test_state_round_trip_and_tune_cache_file(tmp_path):
    st = {'algo': {KEY: 12, ('tail', 32, 52, 52, 128, 256, 1, True, 128, 0, 0, 1, 0, 0, 0): 1, ('res', 32, 208, 208, 64, 1): 1},
          'dgrad': {('s2', (64, 26, 26, 512), 512, 256, True): 6, ((64, 13, 13, 1024), 1024, 512, 3, False): 2},
          'wgrad': {(64, 13, 13, 512, 1024, 3, 1): 3}}
    t = T.Tuner('measure', time=never)
    t.load(st)
    back = plans.from_json(json.loads(json.dumps(plans.to_json(t.state()))))
    u = T.Tuner('measure', time=never)
    u.load(back)
    assert u.state() == st and plans.md5(u.state()) == plans.md5(st) == plans.md5(t.state())
    # the tune_cache file: written when a choice is measured, read back identically by the next Tuner; 'algo' only, its old format
    path = str(tmp_path / 'cache.json')
    s = Script({(1, 5): [1.0], (1, 10): [1.0] * 3, ('fused', 20): [1.0], ('separate', 20): [2.0]})
    a = T.Tuner('measure', tune_cache=path, time=s.time)
    d = desc(residual=4096)
    assert a.conv(d, (1,), lambda: s.launch(d.algo), key_extra=('tail', 128, 0)) == 1
    assert a.fused(('res', 2, 8, 8, 64, 1), True, lambda: (s.fn('fused'), s.fn('separate'))) is True
    a.wgrad(('w',), (0,), never)
    with open(path) as f:
        assert json.load(f) == {'[32, 13, 13, 512, 1024, 3, 1, 0, true, 1, "tail", 128, 0]': 1, '["res", 2, 8, 8, 64, 1]': 1}
    b = T.Tuner('measure', tune_cache=path, time=never)
    assert b.state() == {'algo': a.state()['algo'], 'dgrad': {}, 'wgrad': {}} and len(b.state()['algo']) == 2
    assert b.conv(desc(residual=4096), (1,), never, key_extra=('tail', 128, 0)) == 1


def test_committed_plan_loads_with_its_tail_and_res_entries():
    t = T.Tuner('plan', time=never)
    state, meta = plans.load(plans.DEFAULT)
    assert t.state() == state and t.plan_meta['md5'] == meta['md5'] == plans.md5(t.state())
    tails = [k for k in state['algo'] if k[0] == 'tail']
    assert len(tails) == 8 and all(t.fused(k, True, never) is False for k in tails)
    res = [k for k in state['algo'] if k[0] == 'res']
    assert res and all(t.fused(k, True, never) is bool(state['algo'][k]) for k in res)
