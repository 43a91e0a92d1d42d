#!/usr/bin/env python
"""What a Trainer asks of the library.  yolo_amd.lib._lib is replaced by a proxy BEFORE the net is built; every call is logged as
[symbol, stream ordinal (first-seen order; None: a host-side query, which takes no stream), arguments]: a c_void_p as 0 / 1, integers
and floats verbatim, a ConvDesc / GridDesc by reference as its fields (pointer fields 0 / 1), float arrays as lists.  A case is the log
of two train_steps (the first builds the plan), then one forward / backward(grads) / step() round, and the growth of the allocator's
`allocation.all.allocated` across the second train_step.  Per case: `md5` over the calls that take a stream (what the device is
asked to do, in order), `md5_queries` over the host-side queries in order, and the count of every symbol.  The rule for the queries:
two symbols are left out of `md5_queries` (QUERIES_MOVED: yolo_stem_stats_rows moved from every forward into the plan build, and the
yolo_padded_channels queries of arrays no path reads went), their counts are recorded; every other query must match in order and
arguments (yolo_padded_channels goes as a whole symbol -- the log cannot tell its callers apart; the forward's per-layer value is still
checked, as the `cpad` launch argument of yolo_bn_train_fwd_partials).  --parent compares both md5s and the allocation counts, and
the exit status says whether all agree.  tune='measure' / 'plan' are not recorded: their timing launches are not reproducible.  One
child process per case, each under its own time limit; the first failure ends the run.
    python tools/train_trace.py [--train-py other/train.py] [--commit HASH] [--parent parent_trace.json] [--dump DIR] > trace.json"""
import argparse, collections, ctypes as C, hashlib, importlib.util, json, os, subprocess, sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

QUERIES_MOVED = ('yolo_stem_stats_rows', 'yolo_padded_channels')
# name -> (set-up, dtype, batch, lab knob)
CASES = collections.OrderedDict([
    ('f32_b2', ('car', 'f32', 2, None)), ('bf16_b2', ('car', 'bf16', 2, None)), ('bf16_b3', ('car', 'bf16', 3, None)),
    ('bf16x3_b2', ('car', 'bf16x3', 2, None)), ('lp_bf16_b4', ('lp', 'bf16', 4, None)), ('lp_bf16x3_b4', ('lp', 'bf16x3', 4, None)),
    ('bf16_b3_bn3', ('car', 'bf16', 3, 'YOLO_TRAIN_BN3')), ('bf16_b3_serial_wgrad', ('car', 'bf16', 3, 'YOLO_TRAIN_SERIAL_WGRAD')),
    ('bf16_b3_no_stats_fusion', ('car', 'bf16', 3, 'YOLO_TRAIN_NO_STATS_FUSION'))])


def _fields(s):
    out = {}
    for name, tp in s._fields_:
        v = getattr(s, name)
        out[name] = int(bool(v)) if tp is C.c_void_p else (list(v) if isinstance(v, C.Array) else v)
    return out


class Proxy(object):
    def __init__(self, lib, signatures):
        self._lib, self._sig, self.log, self._streams = lib, signatures, [], {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in self._sig:
            return fn
        argtypes = self._sig[name][1]

        def call(*args):
            rec, stream = [], None
            for i, (tp, a) in enumerate(zip(argtypes, args)):
                if tp is C.c_void_p and i == len(argtypes) - 1:
                    stream = self._streams.setdefault(a or 0, len(self._streams))
                elif tp is C.c_void_p:
                    rec.append(int(bool(a)))
                elif tp is C.c_char_p:
                    rec.append('buffer')
                elif hasattr(a, '_obj'):                       # byref(struct)
                    rec.append(_fields(a._obj))
                elif isinstance(a, C.Array):
                    rec.append(list(a))
                else:
                    rec.append(a)
            self.log.append([name, stream, rec])
            return fn(*args)
        self.__dict__[name] = call
        return call


def run_case(name, train_py):
    import numpy as np
    import torch
    from oracle import graph as og, train as ot
    import yolo_amd.lib as L
    kind, dtype, B, _ = CASES[name]
    proxy = L._lib = Proxy(L.load(), L.SIGNATURES)
    from yolo_amd import net as ynet
    if train_py:
        spec = importlib.util.spec_from_file_location('yolo_amd._traced_train', train_py)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        spec.loader.exec_module(mod)
        Trainer = mod.Trainer
    else:
        from yolo_amd.train import Trainer
    dev = torch.device('cuda', 0)
    # seeded as tests/test_gpu_train.py::_setup / _lp_setup
    spec_, size = og.spec_micro(), (64, 96)
    kw, kwt = {}, {}
    if kind == 'lp':
        spec_ = dict(spec_, LP_slice_point=[1, 3, 4, 7, 10], LP_r_max=[45, 60, 45])
        lpl = ot.synthetic_lp_labels(B, size, seed=2, add_rate=0.75)
        lpl[0, 0, 7:9] = [size[1] + 40.0, -3.0]
        lpl[0, 0, 0] = 1
        kw, kwt = dict(lp_labels=torch.from_numpy(lpl).to(dev)), dict(lp_r_max=spec_['LP_r_max'])
    P = og.init_params(og.build_graph(spec_), seed=0, bn='random')
    x = torch.from_numpy(np.random.default_rng(2).random((B, 3) + size, dtype=np.float32)).to(dev)
    lab = torch.from_numpy(ot.synthetic_labels(B, seed=1, render_rate=0.25 if kind == 'lp' else 0.0, num_class=4)).to(dev)
    net = (ynet.CarLPNet if kind == 'lp' else ynet.CarNet)(spec_, dtype=dtype, device=dev, tune='auto').load_params(P)
    tr = Trainer(net, size, **kwt)
    tr.train_step(x, lab, **kw)
    torch.cuda.synchronize()
    a0 = torch.cuda.memory_stats()['allocation.all.allocated']
    tr.train_step(x, lab, **kw)
    torch.cuda.synchronize()
    grown = torch.cuda.memory_stats()['allocation.all.allocated'] - a0
    outs = tr.forward(x)
    if kind == 'lp':
        outs, lps = outs
        tr.backward([torch.full_like(o, 1e-3) for o in outs], lp_grads=[torch.full_like(lps[0], 1e-3)])
    else:
        tr.backward([torch.full_like(o, 1e-3) for o in outs])
    tr.step()
    torch.cuda.synchronize()
    md5 = lambda rows: hashlib.md5(json.dumps(rows, sort_keys=True).encode()).hexdigest()
    launches = [r for r in proxy.log if r[1] is not None]
    queries = [r for r in proxy.log if r[1] is None and r[0] not in QUERIES_MOVED]
    res = dict(md5=md5(launches), md5_queries=md5(queries), launches=len(launches), streams=len(proxy._streams),
               alloc_second_step=grown, symbols=dict(sorted(collections.Counter(r[0] for r in proxy.log).items())))
    return res, proxy.log


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--train-py', default=None, help='load the Trainer from this file (it joins the yolo_amd package) instead of yolo_amd/train.py')
    ap.add_argument('--commit', default=None, help='recorded in the output: the commit the traced train.py is of')
    ap.add_argument('--dump', default=None, help='directory that receives the full log of every case as <case>.json')
    ap.add_argument('--parent', default=None, help="this tool's output for the parent commit's train.py (--train-py): its md5s and allocation "
                    'counts are recorded next to this run\'s; exit status 1 if an md5 differs or a count grew')
    ap.add_argument('--case', default=None, help='(child) run this one case and print its record')
    ap.add_argument('--timeout', type=int, default=180, help='seconds per case')
    a = ap.parse_args()
    if a.case:
        res, log = run_case(a.case, a.train_py)
        if a.dump:
            os.makedirs(a.dump, exist_ok=True)
            with open(os.path.join(a.dump, a.case + '.json'), 'w') as f:
                f.write('\n'.join(json.dumps(r, sort_keys=True) for r in log) + '\n')
        print('RESULT ' + json.dumps(res, sort_keys=True))
        return 0
    out = dict(train_py=a.train_py or 'yolo_amd/train.py', commit=a.commit, spec='oracle.graph.spec_micro() at 64x96, tune=auto', cases={})
    for name, (_, _, _, knob) in CASES.items():
        env = dict(os.environ)
        if knob:
            env.update({'YOLO_LAB': '1', knob: '1'})
        cmd = [sys.executable, os.path.abspath(__file__), '--case', name] + (['--train-py', a.train_py] if a.train_py else []) \
            + (['--dump', a.dump] if a.dump else [])
        p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, universal_newlines=True, timeout=a.timeout)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')]
        if p.returncode != 0 or not line:
            sys.stderr.write('case %s ended with status %d: stopping\n' % (name, p.returncode))
            return 1
        out['cases'][name] = dict(json.loads(line[0][7:]), knob=knob)
        sys.stderr.write('%s %s\n' % (name, out['cases'][name]['md5']))
    same = True
    if a.parent:
        with open(a.parent) as f:
            par = json.load(f)
        keys = ('md5', 'md5_queries', 'alloc_second_step')
        out['parent'] = dict(commit=par['commit'], cases={n: dict({k: c[k] for k in keys}, moved={q: c['symbols'].get(q, 0) for q in QUERIES_MOVED})
                                                          for n, c in par['cases'].items()})
        same = all(c['md5'] == par['cases'][n]['md5'] and c['md5_queries'] == par['cases'][n]['md5_queries']
                   and c['alloc_second_step'] <= par['cases'][n]['alloc_second_step'] for n, c in out['cases'].items())
        out['same_as_parent'] = same
    print(json.dumps(out, indent=1, sort_keys=True))
    return 0 if same else 1


if __name__ == '__main__':
    sys.exit(main())
