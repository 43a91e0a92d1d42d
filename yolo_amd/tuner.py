"""Tuner: which kernel variant a layer launches -- the policy behind tune='auto' | 'measure' | 'plan'.

A CarNet creates one and the Trainer attached to that net shares it.  It owns the mode, the three sections of per-shape choices
(plans.SECTIONS) with the stale counter and the optional tune_cache file, the key of a conv descriptor, the one HIP-event timing
helper, the selection rules and the dry run of adopted choices.  CarNet and Trainer build descriptors and launch closures and ask
for an algo id or a yes / no.  The rules are plain functions of a timing function, so they are tested without a GPU
(tests/test_tuner_host.py).  What callers rely on:
  * the public names stay: CarNet.tuning_state / load_tuning_state / stale_choices / plan_signature / plan_kernels / plan_meta /
    fuse_tail_note and the keywords tune, tune_cache, fuse_tail; Trainer.tuning_state / load_tuning_state / tune;
  * CarNet.tuning_state() returns, and CarNet.load_tuning_state() adopts, the 'algo' section only; Trainer's take all three -- so
    the first Trainer of a tune='measure' net starts with empty 'dgrad' / 'wgrad', one on a tune='plan' net with the plan's (every
    Trainer of one net -- net.trainer(size), resized() -- shares the net's Tuner, so a later one finds the earlier ones' choices);
  * data-gradient convs share the forward convs' key space (no slope in the key) and cache: the 'dgrad' entry is a copy of that
    answer; under tune='plan' a missing data-gradient shape is recorded as 0, a missing weight-gradient shape returns 0 unrecorded;
  * profiles/plan.json is loaded as it is (meta.md5 verified); its 'tail', 'res' and 'stem_res' entries are honoured;
  * nothing here touches the library: the same kernels, the same ids.
"""
import json
import os

from . import plans


def conv_key(d, key_extra=()):
    """The key of a forward / data-gradient conv descriptor (lib.ConvDesc): the shape, and the strided views only where one is set."""
    key = (d.N, d.H, d.W, d.Cin, d.Cout, d.ksize, d.stride, d.out_f32, bool(d.residual), d.dtype)
    if d.x_pixel_stride or d.upsample2x or (d.y_pixel_stride and not d.out_f32):
        key = key + (int(d.x_pixel_stride), int(d.upsample2x), int(d.y_pixel_stride))
    return key + tuple(key_extra)


def hip_time(fn, launches, windows=1):
    """ms per launch of fn() on the current stream: per window two warm-up launches, then `launches` between two HIP events; the
    fastest window.  None when a first warm-up launch returns a non-zero status (fn may return None: it checks for itself)."""
    import torch
    best = float('inf')
    for _ in range(windows):
        if fn():
            return None
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1) / launches)
    return best


# ---- the selection rules: launch(algo) -> status; time = hip_time or a test's scripted one ---------------------------------
def pick_conv(algos, launch, time, iters=5, top=3, mult=2, rounds=3):
    """Fastest conv variant; 1 = none ran.  Two passes: a short one over every variant, then the three fastest again with twice
    the launches -- a single short timing is noisy enough (DVFS, neighbours' tails) to pick a variant that is 5 % slower.
    (round 3: the second pass INTERLEAVES its candidates over three rounds and keeps each one's fastest round -- timed one after
    the other, a clock / power drift of a few per cent between two candidates' windows picked the slower one: the 64 -> 128
    stride-2 layer at 608x608 ran the generic kernel, 446 us, where the streaming one takes 417)"""
    first = sorted((t, a) for a in algos for t in [time(lambda: launch(a), iters)] if t is not None)
    cands = [a for _, a in first[:top]]
    fastest = {a: float('inf') for a in cands}
    for _ in range(rounds):
        for a in cands:
            t = time(lambda: launch(a), mult * iters)
            if t is not None:
                fastest[a] = min(fastest[a], t)
    return min(cands, key=lambda a: fastest[a]) if cands else 1


def pick_fused(fused, separate, time, windows=1):
    """True when the fused launch is strictly faster than the separate ones: windows of 20 launches, the best one each."""
    t = time(fused, 20, windows)
    return t is not None and t < time(separate, 20, windows)


def pick_wgrad(algos, launch, time):
    """Weight-gradient id, candidates in order (0 = the library's choice first): a later one must win by 2 %; 0 = nothing to choose."""
    best, best_t = 0, float('inf')
    for a in algos if len(algos) > 1 else ():
        t = time(lambda: launch(a), 6)
        if t is not None and t < best_t * 0.98:
            best, best_t = a, t
    return best


class Tuner(object):
    def __init__(self, mode, tune_cache=None, valid=None, time=hip_time):
        """mode 'plan': tune_cache names the plan file (default plans.DEFAULT) and nothing is written; 'measure': tune_cache is an
        optional JSON file remembering the 'algo' choices (so a profiled run launches only the chosen kernels).  valid(d) -> bool:
        whether the library takes forward conv descriptor d with its d.algo (yolo_conv_kernel_name: host only, no launch)."""
        if mode not in ('auto', 'measure', 'plan'):
            raise ValueError("tune must be 'auto', 'measure' or 'plan'")
        self.mode, self._valid, self._time = mode, valid, time
        self.applies = mode != 'auto'       # choices are looked up and applied ('auto': the library's heuristic everywhere)
        self.live = mode == 'measure'       # a shape without a choice is timed ('plan': it gets the heuristic's answer)
        self.stale = 0                      # adopted 'algo' choices this library no longer takes: dropped (measured again when live)
        self.plan_meta, self._file = None, None
        self._held = {sec: {} for sec in plans.SECTIONS}
        if mode == 'plan':
            self._held, self.plan_meta = plans.load(tune_cache or plans.DEFAULT)
        elif tune_cache:
            self._file = tune_cache
            if os.path.exists(tune_cache):
                with open(tune_cache) as f:
                    self._held['algo'] = {tuple(json.loads(k)): v for k, v in json.load(f).items()}

    # ---- the choices as a value -------------------------------------------------------------------------------------------
    def state(self, sections=plans.SECTIONS):
        return {sec: dict(self._held[sec]) for sec in sections}

    def load(self, state, sections=plans.SECTIONS):
        for sec in sections:
            self._held[sec].update(state[sec])

    def _choice(self, sec, key, measure, default):
        held = self._held[sec]
        if key not in held:
            if not self.live:
                return default
            held[key] = int(measure())
            if sec == 'algo' and self._file:
                with open(self._file, 'w') as f:
                    json.dump({json.dumps(list(k)): v for k, v in held.items()}, f)
        return held[key]

    # ---- the questions ------------------------------------------------------------------------------------------------------
    def conv(self, d, algos, run, key_extra=(), dry_run=True):
        """The algo id for descriptor d (0: the library's heuristic; d.algo is left 0).  run() launches d and returns the status;
        timing overwrites d's outputs.  dry_run (forward convs, not another entry point's ids): a choice adopted from a plan file /
        another rank that a library built since no longer takes (a tile's halo budget changed, an id was retired) is dropped,
        counted in `stale` and, when live, measured again -- which plans.new_keys() then counts as measured live."""
        if not self.applies:
            return 0
        key, held = conv_key(d, key_extra), self._held['algo']
        if dry_run and self._valid is not None and held.get(key, 1) != 1:
            d.algo = held[key]
            if not self._valid(d):
                del held[key]
                self.stale += 1

        def launch(algo):
            d.algo = algo
            return run()
        best = self._choice('algo', key, lambda: pick_conv(algos, launch, self._time), 0)
        d.algo = 0
        return best

    def fused(self, key, default, setup, windows=1):
        """Whether the fused kernel of `key` ('res' / 'tail' / 'stem_res' entries of the 'algo' section) is used; setup() -> (fused, separate) launch closures,
        built only when the pair is timed.  The closures must OWN the memory their launches touch: nothing else setup() made outlives it."""
        if not self.applies:
            return default
        return bool(self._choice('algo', key, lambda: pick_fused(*setup(), self._time, windows), default))

    def dgrad(self, key, conv):
        """The Trainer-level data-gradient entry: a copy of conv()'s answer (a Tuner.conv call), recorded in every applied mode."""
        if not self.applies:
            return 0
        held = self._held['dgrad']
        if key not in held:
            held[key] = conv()
        return held[key]

    def wgrad(self, key, algos, bracket):
        """The weight-gradient id (0: the library's choice).  bracket(pick) -> pick(launch), run between the caller's stream waits
        with launch(algo) -> status on a scratch gradient; not called when there is nothing to choose."""
        def measure():
            return bracket(lambda launch: pick_wgrad(algos, launch, self._time)) if len(algos) > 1 else 0
        return self._choice('wgrad', key, measure, 0) if self.applies else 0
