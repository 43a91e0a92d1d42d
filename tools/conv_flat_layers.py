#!/usr/bin/env python
"""Per-layer times of the flat streaming 1x1 (csrc/conv_flat.hip, algo 43) against the committed plan's kernel and against a
streaming yardstick, for every distinct eligible layer shape of the three inference workloads of the plan (416x416 bs 32 and
608x608 bs 64 in bf16, 416x416 bs 32 in IEEE half):
    python tools/conv_flat_layers.py [--plan profiles/plan.json] [--out profiles/conv_flat_layers.json] [--adopt]
Eligible: 1x1, stride 1, Cin in {256, 512}, Cout in {128, 256}, dense input and output (found in CarNet's launch plan).
Every figure is ms per launch by the tuner's HIP-event timing (yolo_amd/tuner.py:hip_time, 20 launches, best of 3 windows) of the
PAIR (writer, kernel) minus the writer alone: the writer is a device copy that rewrites the layer's input, so the kernel under
test starts in the cache state of the network -- directly behind the kernel that wrote its input.  The yardstick is a plain
elementwise kernel that reads the layer's input bytes once and writes its output bytes once (out = first half + second half of
the input: Cin = 2 Cout).  The flat kernel and the plan's choice alternate three times; --adopt writes algo 43 into the plan for
the shapes where it won all three (plans.save: the md5 follows)."""
import argparse, ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from yolo_amd import lib as L, plans
from yolo_amd.net import CarNet
from yolo_amd.spec import darknet53_spec
from yolo_amd.tuner import conv_key, hip_time

ap = argparse.ArgumentParser()
ap.add_argument('--plan', default=plans.DEFAULT)
ap.add_argument('--out', default=os.path.join(os.path.dirname(plans.DEFAULT), 'conv_flat_layers.json'))
ap.add_argument('--adopt', action='store_true')
ap.add_argument('--commit', default='conv_flat')
a = ap.parse_args()
dev = torch.device('cuda', 0)
torch.cuda.set_device(0)
lib = L.load()
FLAT = L.CONV_FLAT_ALGO
TDT = {L.BF16: torch.bfloat16, L.F16: torch.float16}
WORKLOADS = (('bf16', 32, 416), ('bf16', 64, 608), ('f16', 32, 416))


def eligible(d):
    return (d.ksize == 1 and d.stride == 1 and d.Cin in (256, 512) and d.Cout in (128, 256) and not d.out_f32
            and not (d.x_pixel_stride or d.y_pixel_stride or d.y_batch_stride or d.upsample2x))


# ---- the shapes, and what the plan launches for them ----------------------------------------------------------------------
shapes = {}            # key -> dict(workloads, launches per step, plan algo, plan kernel)
for dt, B, S in WORKLOADS:
    net = CarNet(darknet53_spec(), dtype=dt, device=dev, tune='plan', tune_cache=a.plan).initialize(seed=1234)
    net.prepare()
    buf = C.create_string_buffer(256)
    for kind, d, name in net._plan_for(B, S, S).ops:
        if kind != 'conv' or not eligible(d):
            continue
        L.check(lib.yolo_conv_kernel_name(C.byref(d), buf, 256), 'kernel_name')
        e = shapes.setdefault(conv_key(d), dict(workloads={}, plan_algo=int(d.algo), plan_kernel=buf.value.decode(), residual=bool(d.residual)))
        w = '%s %dx%d bs %d' % (dt, S, S, B)
        e['workloads'][w] = e['workloads'].get(w, 0) + 1
    del net
    torch.cuda.empty_cache()

st = L.stream_ptr()
rows = []
for key, e in sorted(shapes.items()):
    N, H, W, Cin, Cout, dtype = key[0], key[1], key[2], key[3], key[4], key[9]
    tdt = TDT[dtype]
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn((N, H, W, Cin), device=dev, generator=g).to(tdt)
    xsrc = x.clone()
    y = torch.empty((N, H, W, Cout), device=dev, dtype=tdt)
    res = torch.randn((N, H, W, Cout), device=dev, generator=g).to(tdt) if e['residual'] else None
    w = torch.randn((Cout, Cin, 1, 1), device=dev, generator=g) / Cin ** 0.5
    wp = torch.empty(lib.yolo_packed_weight_bytes(Cout, Cin, 1, dtype), dtype=torch.uint8, device=dev)
    L.check(lib.yolo_pack_conv_weights(w.data_ptr(), wp.data_ptr(), Cout, Cin, 1, dtype, st), 'pack')
    cp = lib.yolo_padded_channels(Cout)
    sc, bi = torch.ones(cp, device=dev), torch.zeros(cp, device=dev)
    d = L.ConvDesc()
    d.x, d.w_packed, d.scale, d.bias, d.residual, d.y = x.data_ptr(), wp.data_ptr(), sc.data_ptr(), bi.data_ptr(), L.ptr(res), y.data_ptr()
    d.N, d.H, d.W, d.Cin, d.Cout, d.ksize, d.stride, d.dtype, d.slope = N, H, W, Cin, Cout, 1, 1, dtype, 0.1
    xa, xb = x.view(-1)[:x.numel() // 2].view(y.shape), x.view(-1)[x.numel() // 2:].view(y.shape)

    def writer():
        x.copy_(xsrc)

    def conv(algo):
        def fn():
            writer()
            d.algo = algo
            return lib.yolo_conv_fwd(C.byref(d), st)
        return fn

    def yard():
        writer()
        torch.add(xa, xb, out=y)

    T = lambda fn: hip_time(fn, 20, 3)
    tw = T(writer)
    ty = T(yard) - tw
    alt = []
    for _ in range(3):
        tp_ = T(conv(e['plan_algo'])) - tw
        tf_ = T(conv(FLAT)) - tw
        alt.append([round(tp_, 5), round(tf_, 5)])
    won = all(f < p for p, f in alt)
    best_p, best_f = min(p for p, _ in alt), min(f for _, f in alt)
    nbytes = (x.numel() + y.numel() * (2 if res is not None else 1)) * 2
    rows.append(dict(key=list(key), workloads=e['workloads'], bytes=nbytes, plan_algo=e['plan_algo'], plan_kernel=e['plan_kernel'],
                     writer_ms=round(tw, 5), yardstick_ms=round(ty, 5), alternations_plan_flat_ms=alt, flat_won_all_three=won,
                     plan_over_yardstick=round(best_p / ty, 3), flat_over_yardstick=round(best_f / ty, 3),
                     plan_TBps=round(nbytes / best_p / 1e9, 3), flat_TBps=round(nbytes / best_f / 1e9, 3), yardstick_TBps=round(nbytes / ty / 1e9, 3)))
    print(json.dumps(rows[-1]), flush=True)
    del x, xsrc, y, res, xa, xb
    torch.cuda.empty_cache()

within = all(r['plan_over_yardstick'] <= 1.10 for r in rows)
out = dict(device=torch.cuda.get_device_name(0), made=time.strftime('%Y-%m-%d %H:%M:%S'), plan=os.path.basename(a.plan),
           method=__doc__.split('Every figure')[1].strip().replace('\n', ' '), plan_within_10pct_of_yardstick_everywhere=within, layers=rows)
if a.adopt:
    state, meta = plans.load(a.plan)
    adopted = [r['key'] for r in rows if r['flat_won_all_three']]
    for k in adopted:
        state['algo'][plans._freeze(k)] = FLAT
    meta = dict(meta, commit=a.commit, base=os.path.basename(a.plan), made=time.strftime('%Y-%m-%d %H:%M:%S'))
    meta.pop('md5', None)
    plans.save(a.plan, state, meta)
    out['adopted'] = adopted
    out['plan_md5_after'] = plans.md5(state)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, 'w') as f:
    json.dump(out, f, indent=1)
    f.write('\n')
print('wrote %s: %d layers, flat won on %d' % (a.out, len(rows), sum(r['flat_won_all_three'] for r in rows)))
