"""Random train-mode BatchNorm shapes (pixels x channels, fp32 and bf16, with and without the residual) through the three-launch
and the two-launch (_pp) forms of yolo_bn_train_fwd / _bwd against the float64 restatement of tests/bn_cond_ref.py, evaluated on
the GPU on the same rounded y.  Three cases in four draw the benign 2 randn + 0.5 and are judged end to end (float64 statistics);
one in four draws the ill-conditioned channel classes of tests/bn_cond_ref.py: there the statistics are held to that file's bars
(mean, invstd, running_var) and everything behind them is judged one hop at a time, with the kernel's own float32 mean and invstd.
    python tools/fuzz_bn.py <seed> <seconds>"""
import sys, os, time
ROOT = os.environ.get("GRAFT_REPO_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np, torch
import bn_cond_ref as B
from yolo_amd import lib as L
lib = L.load(); dev = torch.device('cuda:0')
rng = np.random.default_rng(int(sys.argv[1]) if len(sys.argv) > 1 else 0)
budget = float(sys.argv[2]) if len(sys.argv) > 2 else 120
st = torch.cuda.current_stream().cuda_stream
ncase = ncond = 0
bad = []
t0 = time.time()
def close(name, a, b, rtol, atol, ctx):
    d = (a.double() - b.double()).abs()
    if not bool((d <= atol + rtol * b.double().abs()).all()):
        bad.append((name, 'max err %.3g' % float(d.max()), ctx))
while time.time() - t0 < budget:
    C_ = int(rng.choice([8, 16, 32, 64, 72, 128, 256, 512, 1000, 1024, 2048, 2112]))
    npix = int(rng.choice([1, 2, 3, 7, 64, 169, 1000, 4097, 21632, 86528]) if rng.random() < 0.5 else rng.integers(1, 30000))
    if npix * C_ > 3e7: continue
    cond = bool(rng.random() < 0.25) and npix * C_ <= 4e6          # (the classes are drawn column by column on the host)
    dtype = 'f32' if rng.random() < 0.3 else 'bf16'
    ldt, tdt = (L.F32, torch.float32) if dtype == 'f32' else (L.BF16, torch.bfloat16)
    with_res = bool(rng.random() < 0.3)
    g = torch.Generator(device=dev).manual_seed(int(rng.integers(1 << 30)))
    if cond:
        yh, names, _ = B.channels(npix, C_, dtype, int(rng.integers(1 << 30)))
        y = torch.from_numpy(yh).to(dev).to(tdt)
        ncond += 1
    else:
        y = (2 * torch.randn((npix, C_), device=dev, generator=g) + 0.5).to(tdt)
    res = torch.randn((npix, C_), device=dev, generator=g).to(tdt) if with_res else None
    dz = torch.randn((npix, C_), device=dev, generator=g).to(tdt)
    gamma = (0.5 + torch.rand(C_, device=dev, generator=g)); beta = 0.1 * torch.randn(C_, device=dev, generator=g)
    if cond:                                                 # |beta| >= 0.05: a constant channel (xhat = 0) stays off LeakyReLU's kink
        beta = torch.where(beta < 0, beta - 0.05, beta + 0.05)
    # float64 two-pass statistics around pixel 0 (tests/bn_cond_ref.py stats64, on the device)
    yd = y.double(); d0 = yd - yd[:1]; dm = d0.mean(dim=0)
    mean = yd[0] + dm; var = ((d0 - dm) ** 2).mean(dim=0)
    ctx = (dtype, npix, C_, with_res, 'classes' if cond else 'benign')
    ncase += 1
    tol = (1e-4, 1e-5) if dtype == 'f32' else (1e-2, 1e-2)
    if npix < 16: tol = (tol[0] * 20, tol[1] * 20)            # (invstd up to 316: rounding noise of y - mean is amplified)
    for form in ('three', 'pp'):
        zd = torch.full_like(y, float('nan')); m_ = torch.empty(C_, device=dev); is_ = torch.empty(C_, device=dev)
        rm = torch.zeros(C_, device=dev); rv = torch.ones(C_, device=dev)
        dyd = torch.full_like(y, float('nan')); dg = torch.empty(C_, device=dev); db = torch.empty(C_, device=dev)
        if form == 'three':
            ws = torch.zeros(3 * C_, dtype=torch.float64, device=dev)
            rc = lib.yolo_bn_train_fwd(y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), res.data_ptr() if with_res else None, zd.data_ptr(), m_.data_ptr(),
                                       is_.data_ptr(), rm.data_ptr(), rv.data_ptr(), ws.data_ptr(), npix, C_, 1e-5, 0.9, 0.1, ldt, st)
            rc2 = lib.yolo_bn_train_bwd(dz.data_ptr(), y.data_ptr(), m_.data_ptr(), is_.data_ptr(), gamma.data_ptr(), beta.data_ptr(), dyd.data_ptr(),
                                        dg.data_ptr(), db.data_ptr(), ws.data_ptr(), npix, C_, 0.1, ldt, st) if rc == 0 else -9
        else:
            wa = torch.zeros(2 * 2112, dtype=torch.float64, device=dev); wb = torch.zeros(2 * 2112, dtype=torch.float64, device=dev)
            rc = lib.yolo_bn_train_fwd_pp(y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), res.data_ptr() if with_res else None, zd.data_ptr(), m_.data_ptr(),
                                          is_.data_ptr(), rm.data_ptr(), rv.data_ptr(), wa.data_ptr(), wb.data_ptr(), 2 * 2112, npix, C_, 1e-5, 0.9, 0.1, ldt, st)
            rc2 = lib.yolo_bn_train_bwd_pp(dz.data_ptr(), y.data_ptr(), m_.data_ptr(), is_.data_ptr(), gamma.data_ptr(), beta.data_ptr(), dyd.data_ptr(),
                                           dg.data_ptr(), db.data_ptr(), wb.data_ptr(), wa.data_ptr(), 2 * 2112, npix, C_, 0.1, ldt, st) if rc == 0 else -9
        if rc != 0 or rc2 != 0:
            bad.append(('refused', form, rc, rc2, ctx)); continue
        torch.cuda.synchronize()
        if torch.isnan(zd.float()).any() or torch.isnan(dyd.float()).any():
            bad.append(('NaN (unwritten) output', form, ctx)); continue
        # the statistics, at the bars of tests/bn_cond_ref.py, on every case
        if not bool(((m_.double() - mean).abs() <= 2.0 ** -23 * mean.abs() + 1e-6 * var.sqrt()).all()):
            bad.append((form + ' mean', 'max err %.3g' % float((m_.double() - mean).abs().max()), ctx))
        ierr = (is_.double() * torch.sqrt(var + 1e-5) - 1).abs()
        if not bool((ierr <= B.INVSTD_BAR).all()):
            bad.append((form + ' invstd', 'max relative err %.3g' % float(ierr.max()), ctx))
        rvr = 0.9 + 0.1 * var
        if not bool(((rv.double() - rvr).abs() <= 1e-4 * var + 2.0 ** -23 * rvr.abs()).all()):
            bad.append((form + ' running_var', 'max err %.3g' % float((rv.double() - rvr).abs().max()), ctx))
        # everything behind them: the float64 restatement (tests/bn_cond_ref.py forward64 / backward64) with the float64 statistics
        # (benign: end to end) or with the kernel's own (classes: one hop -- the float32 mean of a rho = 1e8 channel moves xhat by 3e-4)
        md, isd = (m_.double(), is_.double()) if cond else (mean, 1.0 / torch.sqrt(var + 1e-5))
        xh = (yd - md) * isd
        a_ref = gamma.double() * xh + beta.double()
        z = torch.where(a_ref > 0, a_ref, 0.1 * a_ref)
        if with_res: z = z + res.double()
        da = dz.double() * torch.where(a_ref > 0, torch.ones_like(a_ref), torch.full_like(a_ref, 0.1))
        dbr, dgr = da.sum(dim=0), (da * xh).sum(dim=0)
        dyr = gamma.double() * isd * (da - dbr / npix - xh * dgr / npix)
        # LeakyReLU's kink: an element whose pre-activation is within rounding noise of 0 may take either slope, which moves ITS dy and
        # its channel's dgamma / dbeta (and through them every dy of the channel) by O(dz): such channels are compared on z only
        chan_ok = ~(a_ref.abs() < 2e-5 * (1 + a_ref.abs().amax(dim=0, keepdim=True))).any(dim=0)
        close(form + ' z', zd, z, tol[0], tol[1], ctx)
        if not bool(chan_ok.any()):
            continue
        # (a batch of two pixels normalises to +-1: its true dy is ~0 and everything left is rounding noise of O(eps * dz) -- the
        #  scale of the comparison does not go below that; found by seed 61 in round 6.  Classes: the scale is taken per channel,
        #  a constant channel's dy is 316 times a benign one's)
        floor = 1e-4 * float(dz.float().abs().max()) + 1e-6
        if cond:
            gscale = torch.clamp(dyr[:, chan_ok].abs().amax(dim=0, keepdim=True), min=floor)
        else:
            gscale = max(float(dyr[:, chan_ok].abs().max()), floor)
        d = (dyd[:, chan_ok].double() - dyr[:, chan_ok]).abs()
        if not bool((d <= tol[1] * gscale * (1 if dtype == 'bf16' else 10) + tol[0] * 10 * dyr[:, chan_ok].abs()).all()):
            bad.append((form + ' dy', 'max err %.3g' % float(d.max()), ctx))
        close(form + ' dgamma', dg[chan_ok], dgr[chan_ok], 2e-3, 2e-3 * (float(dgr[chan_ok].abs().max()) + 1e-6), ctx)
        close(form + ' dbeta', db[chan_ok], dbr[chan_ok], 2e-3, 2e-3 * (float(dbr[chan_ok].abs().max()) + 1e-6), ctx)
print('cases %d (%d from the ill-conditioned classes), problems %d' % (ncase, ncond, len(bad)))
for b in bad[:30]: print('  ', b)
