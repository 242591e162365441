"""Windows through the C-ABI (hbx_evaluate_real_window / _threshold_window, hbx_backward_window,
hbx_loss_window, hbx_loss_weight_window): a hologram of any size zero-filled into the plan's grid, and
the field, intensity, statistics, loss and gradient taken over another rectangle of it.

Every windowed call here goes through ctypes with each compact buffer, inputs included, inside a
larger NaN-filled allocation: the guard elements must stand afterwards, and a read outside a compact
input would put a NaN into an output.  The reference is the unwindowed entry point on the explicitly
zero-embedded input, sliced to the output window, and the float64 oracle on the same array.
Shapes (N, G, P, B): all four sizes at P = 2, P = 4 and G = 3 at N = 64, and B = 3 on a plan of one
job per launch (n_env > max_jobs).  Windows at every size: offsets and extents that are multiples of
none of 8, 16 and R with in != out, each border touched, a single row, a single column, 1 x 1, windows
that share no row, odd widths, and the full grid."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import hbx_oracle as O  # noqa: E402
from tests.test_threshold_ste_host import STE_SIGMOID, STE_WINDOW, binarize, field_values  # noqa: E402

FIELD_RTOL = 2e-5
MSE_RTOL = 2.31e-5
PSNR_ATOL = 1e-4
TAU = 0.5
PAD = 98   # guard elements on either side of a compact buffer (even: complex64 stays 8-byte aligned)

# name: (N, G, P, B, max_jobs)
CASES = {"64": (64, 1, 2, 2, 2), "64p4": (64, 1, 4, 1, 1), "64rgb": (64, 3, 2, 1, 3), "64chunk": (64, 1, 2, 3, 1),
         "256": (256, 1, 2, 1, 1), "896": (896, 1, 2, 1, 1), "1024": (1024, 1, 2, 1, 1)}
KINDS = {"amplitude": O.FIELD_AMPLITUDE, "phase": O.FIELD_PHASE}


def windows(n):
    """name: (input window, output window), each (y0, x0, h, w)"""
    return {
        "odd": ((5, 9, n - 24, n - 31), (3, 20, n - 30, n - 41)),          # multiples of none of 8, 16, R
        "borders": ((0, 0, n - 7, n - 3), (7, 3, n - 7, n - 3)),           # top / left, bottom / right
        "row_col": ((n // 2 + 1, 3, 1, n - 5), (2, n // 3, n - 9, 1)),     # a single row in, a single column out
        "pixel": ((n - 1, n - 1, 1, 1), (0, 0, 1, 1)),                     # 1 x 1, opposite corners
        "disjoint": ((0, 1, n // 4 - 1, n - 2), (n // 2 + 1, 0, n // 4 + 3, n - 1)),   # no common row
        "full": ((0, 0, n, n), (0, 0, n, n)),
    }


WNAMES = list(windows(64))


def ocfg_for(name, field_kind=O.FIELD_AMPLITUDE):
    n, g, p = CASES[name][:3]
    return O.OpticsConfig(n, n, g, p, O.WL_RGB if g == 3 else O.WL_MONO, field_kind=field_kind)


def dev_cfg(o, z=None):
    import hbx
    return hbx.OpticsConfig(o.height, o.width, o.groups, o.planes, tuple(o.wavelengths), o.dx, o.dy,
                            o.z if z is None else z, o.tf_kind, o.field_kind, o.rel_scale, o.peak)


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm GPU")
    import hbx
    hbx.load_library()
    yield


@functools.lru_cache(maxsize=None)
def plan_for(name, kind="amplitude", z=None, precision=0):
    import hbx
    return hbx.Plan(dev_cfg(ocfg_for(name, KINDS[kind]), z), max_jobs=CASES[name][4], precision=precision)


# -- guarded buffers ---------------------------------------------------------------------------------
class Guarded:
    """a contiguous tensor of `shape` in the middle of a NaN-filled allocation"""

    def __init__(self, shape, dtype=torch.float32, data=None):
        self.n = int(np.prod(shape))
        self.big = torch.full((self.n + 2 * PAD,), float("nan"), dtype=dtype, device="cuda")
        self.t = self.big[PAD:PAD + self.n].view(shape)
        if data is not None:
            self.t.copy_(torch.from_numpy(np.array(data, order="C")))

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr())

    def intact(self):
        return bool(torch.isnan(self.big[:PAD]).all()) and bool(torch.isnan(self.big[PAD + self.n:]).all())


def _win(w):
    from hbx import _lib
    return C.byref(_lib.Window(*w)) if w is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def evaluate_window(plan, x, thr, in_win, target, out_win, field=True, inten=True, null_windows=False):
    """the raw call on guarded buffers -> (field complex64 | None, intensity | None, stats | None, psnr | None)"""
    from hbx import _lib
    c = plan.cfg
    b = x.shape[0]
    ho, wo = out_win[2:]
    gx = Guarded(x.shape, data=x)
    gt = Guarded(target.shape, data=target) if target is not None else None
    gf = Guarded((b, c.channels, ho, wo, 2)) if field else None
    gi = Guarded((b, c.groups, ho, wo)) if inten else None
    gs = Guarded((b, c.groups, 3), torch.float64) if target is not None else None
    gp = Guarded((b,), torch.float64) if target is not None else None
    p = lambda g: g.ptr if g is not None else None   # noqa: E731
    wi, wo_ = (None, None) if null_windows else (_win(in_win), _win(out_win))
    if thr is None:
        rc = plan.lib.hbx_evaluate_real_window(plan._h, gx.ptr, wi, p(gt), wo_, b, p(gf), p(gi), p(gs), p(gp), _stream())
    else:
        rc = plan.lib.hbx_evaluate_threshold_window(plan._h, gx.ptr, float(thr), wi, p(gt), wo_, b, p(gf), p(gi), p(gs),
                                                    p(gp), _stream())
    _lib.check(rc, "evaluate_window")
    torch.cuda.synchronize()
    out = []
    for g in (gf, gi, gs, gp):
        if g is None:
            out.append(None)
            continue
        assert g.intact(), "a guard element next to an output was written"
        assert not torch.isnan(g.t).any(), "an output element is NaN (unwritten, or read from outside an input)"
        out.append(g.t)
    for g in (gx, gt):
        assert g is None or g.intact()
    if out[0] is not None:
        out[0] = torch.view_as_complex(out[0])
    return out


def embed(a, win, n, fill=0.0):
    """compact [.., h, w] -> [.., n, n] with `a` at win and `fill` elsewhere"""
    y0, x0, h, w = win
    assert a.shape[-2:] == (h, w)
    out = np.full(a.shape[:-2] + (n, n), fill, a.dtype)
    out[..., y0:y0 + h, x0:x0 + w] = a
    return out


def crop(a, win):
    y0, x0, h, w = win
    return a[..., y0:y0 + h, x0:x0 + w]


@functools.lru_cache(maxsize=None)
def _inputs(name, wname):
    """(x float32 [B, G P, h_i, w_i] in [-0.5, 1.5] with tau planted, target float32 [B, G, h_o, w_o]), read-only"""
    n, g, p, b, _ = CASES[name]
    wi, wo = windows(n)[wname]
    rng = np.random.default_rng(4200 + n + 7 * p + g + 13 * WNAMES.index(wname))
    x = (2.0 * rng.random((b, g * p) + wi[2:], dtype=np.float32) - 0.5).astype(np.float32)
    x.reshape(-1)[:: max(1, x.size // 7)] = np.float32(TAU)
    target = rng.random((b, g) + wo[2:], dtype=np.float32)
    for a in (x, target):
        a.setflags(write=False)
    return x, target


def _with_nan(x):
    """the threshold leaf: NaN (bit off) planted too; never fed to the real path"""
    x = x.copy()
    x.reshape(-1)[1:: max(2, x.size // 5)] = np.float32(np.nan)
    return x


def _eq(a, b):
    if a.is_complex():
        a, b = torch.view_as_real(a), torch.view_as_real(b)
    return torch.equal(a, b)   # -0.0 == +0.0


def _eq_nan(a, b):
    """equal where neither is NaN, and NaN in the same places (the sigmoid surrogate of a NaN sample)"""
    nan = torch.isnan(b)
    return torch.equal(torch.isnan(a), nan) and torch.equal(a[~nan], b[~nan])


def _stats64(inten, target):
    """float64 (sum I T, sum I^2, sum T^2) per [B, G]"""
    i, t = inten.astype(np.float64), target.astype(np.float64)
    return np.stack([(i * t).sum((-2, -1)), (i * i).sum((-2, -1)), (t * t).sum((-2, -1))], -1)


def _mse64(stats, count):
    """the relative MSE of hbx_loss (HBX_REL_LSQ) from [B, G, 3] statistics, float64"""
    s = stats.sum(1)
    return (s[:, 2] - s[:, 0] * s[:, 0] / s[:, 1]) / count


# -- 1. null and full-grid windows ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ["64rgb", "256", "896", "1024"])
def test_null_and_full_windows_are_the_unwindowed_calls(name):
    import hbx  # noqa: F401
    from hbx import _lib
    n, g, p, b, _ = CASES[name]
    full = (0, 0, n, n)
    x, target = _inputs(name, "full")
    xt = _with_nan(x)
    plan = plan_for(name, "phase")
    X, XT, T = (torch.from_numpy(a.copy()).cuda() for a in (x, xt, target))
    ref_r = plan.evaluate_real(X, T)
    ref_t = plan.evaluate_threshold(XT, TAU, T)
    for null in (True, False):
        for ref, (xx, thr) in ((ref_r, (x, None)), (ref_t, (xt, TAU))):
            got = evaluate_window(plan, xx, thr, full, target, full, null_windows=null)
            for a, r in zip(got, ref):
                assert _eq(a, r)
    # the Plan methods, windows None; the lean form (intensity alone) and the field alone
    for got, ref in ((plan.evaluate_real_window(X, None, T, None), ref_r),
                     (plan.evaluate_threshold_window(XT, TAU, None, T, None), ref_t)):
        for a, r in zip(got, ref):
            assert _eq(a, r)
    _, i_alone, s_none, _ = plan.evaluate_threshold_window(XT, TAU, full, None, full, want_field=False)
    f_alone, i_none, _, _ = plan.evaluate_real_window(X, full, None, full, want_intensity=False)
    assert s_none is None and i_none is None and _eq(i_alone, ref_t[1]) and _eq(f_alone, ref_r[0])
    assert _eq(plan.loss_window(ref_t[2], None), plan.loss(ref_t[2]))
    assert _eq(plan.loss_window(ref_t[2], full, _lib.LOSS_PSNR), plan.loss(ref_t[2], _lib.LOSS_PSNR))
    assert _eq(plan.loss_weight_window(ref_t[1], T, ref_t[2], None), plan.loss_weight(ref_t[1], T, ref_t[2]))
    # backward: the real part and both surrogates
    back = plan_for(name, "phase", z=-ocfg_for(name).z)
    rng = np.random.default_rng(7)
    v = torch.from_numpy((rng.standard_normal((b, g * p // 2, n, n, 2))).astype(np.float32)).cuda()
    v = torch.view_as_complex(v)
    w = torch.from_numpy(rng.random((b, g, n, n), dtype=np.float32)).cuda()
    s = XT[:, : g * p // 2].contiguous()
    _, re = back.simulate_complex(v, want_field=False, want_real=True, weight=w, scale=0.5)
    assert _eq(back.backward_window(v, None, None, weight=w, scale=0.5), re)
    assert _eq(back.backward_window(v, full, full), back.simulate_complex(v, want_field=False, want_real=True)[1])
    for sur, p0, p1 in ((STE_WINDOW, 0.2, 0.8), (STE_SIGMOID, TAU, 4.0)):
        want = back.threshold_backward(v, s, weight=w, scale=0.5, surrogate=sur, p0=p0, p1=p1)
        got = back.backward_window(v, None, full, samples=s, weight=w, scale=0.5, surrogate=sur, p0=p0, p1=p1)
        assert _eq_nan(got, want)


# -- 2, 4, 5, 6, 7, 8. embed and crop, forward ---------------------------------------------------------
WORST = {}


@pytest.mark.parametrize("wname", WNAMES)
@pytest.mark.parametrize("name", list(CASES))
def test_forward_is_the_embedded_call_cropped(name, wname):
    from hbx import _lib
    n, g, p, b, _ = CASES[name]
    wi, wo = windows(n)[wname]
    x, target = _inputs(name, wname)
    xt = _with_nan(x)
    count = g * wo[2] * wo[3]
    for kind, fk in KINDS.items():
        plan = plan_for(name, kind)
        runs = [("threshold", xt, TAU, embed(binarize(xt, TAU, fk), wi, n))]
        if kind == "amplitude":   # the real path does not see the field kind
            runs.append(("real", x, None, embed(x, wi, n)))
        for what, xx, thr, emb in runs:
            f, i, s, ps = evaluate_window(plan, xx, thr, wi, target, wo)
            rf, ri, _, _ = plan.evaluate_real(torch.from_numpy(emb).cuda(),
                                              torch.from_numpy(embed(target, wo, n)).cuda())
            assert _eq(f, crop(rf, wo).contiguous()) and _eq(i, crop(ri, wo).contiguous())
            # the lean form and the field alone
            _, i_lean, _, _ = evaluate_window(plan, xx, thr, wi, None, wo, field=False)
            f_only, _, _, _ = evaluate_window(plan, xx, thr, wi, None, wo, inten=False)
            assert _eq(i_lean, i) and _eq(f_only, f)
            # 4. statistics: float64 sums over the returned intensity, within n 2^-52 relative
            i_np, s_np = i.cpu().numpy(), s.cpu().numpy()
            want_s = _stats64(i_np, target)
            npix = wo[2] * wo[3]
            rel = np.max(np.abs(s_np - want_s) / np.where(want_s > 0, want_s, 1.0))
            print(f"{name} {wname} {kind} {what}: stats rel err {rel:.3e} (bound {npix * 2.0 ** -52:.3e})")
            assert rel <= npix * 2.0 ** -52
            # 5. psnr and the losses from those statistics, count G h_o w_o
            mse_want = _mse64(s_np, count)
            psnr_want = np.array([O.psnr_from_stats(s_np[k], count) for k in range(b)])
            mse = plan.loss_window(s, wo).cpu().numpy()
            lpsnr = plan.loss_window(s, wo, _lib.LOSS_PSNR).cpu().numpy()
            ok = np.isfinite(psnr_want)
            assert np.all(np.abs(mse - mse_want) <= 1e-12 * np.abs(mse_want) + 1e-300)
            assert np.all(np.abs(ps.cpu().numpy()[ok] - psnr_want[ok]) <= 1e-10)
            assert np.all(np.abs(lpsnr[ok] - psnr_want[ok]) <= 1e-10)
            # 6. the loss weight per pixel, hbx_loss_weight's a I + c T with a = 2 s^2 / n, c = -2 s / n,
            # s = sum IT / sum I^2.  The kernel rounds a and c to float32 once, then c T, then the fma: four
            # roundings of 2^-24 on terms of size |a I| and |c T| (which cancel where s I is near T)
            wgt = plan.loss_weight_window(i, torch.from_numpy(target.copy()).cuda(), s, wo).cpu().numpy()
            st = s_np.sum(1)
            if np.all(st[:, 1] > 0):
                sc = (st[:, 0] / st[:, 1])[:, None, None, None]
                ta = (2.0 * sc * sc / count) * i_np.astype(np.float64)
                tc = (-2.0 * sc / count) * target.astype(np.float64)
                assert np.all(np.abs(wgt - (ta + tc)) <= 4 * 2.0 ** -24 * (np.abs(ta) + np.abs(tc)) + 1e-45)
            # 7. the float64 oracle on the embedded array
            if wname in ("odd", "borders"):
                ocfg = ocfg_for(name, fk)
                u = emb.astype(np.float64)
                worst_f = 0.0
                for bb in range(b):
                    want = np.concatenate([O.propagate(u[bb, k * p:(k + 1) * p], ocfg.transfer(k)) for k in range(g)])
                    want_c = crop(want, wo)
                    ferr = float(np.max(np.abs(f[bb].cpu().numpy() - want_c)) / np.max(np.abs(want)))
                    worst_f = max(worst_f, ferr)
                    assert ferr <= FIELD_RTOL
                    wi64 = (np.abs(want_c) ** 2).reshape(g, p, *wo[2:]).mean(1)
                    ws = O.chan_stats(wi64, target[bb].astype(np.float64))
                    wp = O.psnr_from_stats(ws, count)
                    wm = float(_mse64(ws[None, None], count)[0])   # chan_stats sums the groups: [3]
                    merr = abs(mse[bb] - wm) / wm
                    perr = abs(float(ps[bb]) - wp)
                    print(f"{name} {wname} {kind} {what} env {bb}: field {ferr:.3e} mse rel {merr:.3e} psnr {perr:.3e} dB")
                    assert merr <= MSE_RTOL and perr <= PSNR_ATOL


# -- 3, 8. embed and crop, backward --------------------------------------------------------------------
@pytest.mark.parametrize("wname", WNAMES)
@pytest.mark.parametrize("name", list(CASES))
def test_backward_is_the_embedded_call_cropped(name, wname):
    from hbx import _lib
    n, g, p, b, _ = CASES[name]
    gw, vw = windows(n)[wname]      # the forward's input window takes the gradient, its output window the values
    q = g * p // 2
    rng = np.random.default_rng(5300 + n + WNAMES.index(wname))
    v = rng.standard_normal((b, q) + vw[2:] + (2,)).astype(np.float32)
    w = rng.random((b, g) + vw[2:], dtype=np.float32)
    s = _with_nan((2.0 * rng.random((b, q) + gw[2:], dtype=np.float32) - 0.5).astype(np.float32))
    plan = plan_for(name, "phase", z=-ocfg_for(name).z)
    V = torch.view_as_complex(torch.from_numpy(np.moveaxis(embed(np.moveaxis(v, -1, 0), vw, n), 0, -1).copy()).cuda())
    W = torch.from_numpy(embed(w, vw, n)).cuda()
    S = torch.from_numpy(embed(s, gw, n)).cuda()
    scale = 2.0 / p

    def run(samples, weight, sur=STE_WINDOW, p0=0.0, p1=0.0):
        gv, gwt = Guarded(v.shape, data=v), (Guarded(w.shape, data=w) if weight else None)
        gs = Guarded(s.shape, data=s) if samples else None
        gg = Guarded((b, q) + gw[2:])
        rc = plan.lib.hbx_backward_window(plan._h, gv.ptr, gwt.ptr if gwt else None, C.c_float(scale), _win(vw),
                                          gs.ptr if gs else None, sur, C.c_float(p0), C.c_float(p1), _win(gw), b,
                                          gg.ptr, _stream())
        _lib.check(rc, "hbx_backward_window")
        torch.cuda.synchronize()
        assert all(x is None or x.intact() for x in (gv, gwt, gs, gg))
        return gg.t

    _, re_w = plan.simulate_complex(V, want_field=False, want_real=True, weight=W, scale=scale)
    _, re = plan.simulate_complex(V, want_field=False, want_real=True)
    got_w, got = run(False, True), run(False, False)
    assert not torch.isnan(got_w).any() and not torch.isnan(got).any()
    assert _eq(got_w, crop(re_w, gw).contiguous()) and _eq(got, crop(re, gw).contiguous())
    for sur, p0, p1 in ((STE_WINDOW, 0.2, 0.8), (STE_SIGMOID, TAU, 4.0)):
        want = plan.threshold_backward(V, S, weight=W, scale=scale, surrogate=sur, p0=p0, p1=p1)
        got_s = run(True, True, sur, p0, p1)
        assert _eq_nan(got_s, crop(want, gw).contiguous())   # NaN: the sigmoid of a NaN sample; a closed gate is +0


# -- 9. errors -----------------------------------------------------------------------------------------
def test_bad_windows_and_reduced_precision_are_refused():
    from hbx import _lib
    name = "64"
    n, g, p, b, _ = CASES[name]
    plan = plan_for(name)
    x = torch.zeros((b, g * p, n, n), device="cuda")
    out = torch.empty((b, g, n, n), device="cuda")
    stats = torch.zeros((b, g, 3), dtype=torch.float64, device="cuda")
    ld = torch.empty((b,), dtype=torch.float64, device="cuda")
    cv = torch.zeros((b, g * p // 2, n, n, 2), device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    ok = (0, 0, n, n)
    bad = [(0, 0, n + 1, n), (0, 1, n, n), (-1, 0, 4, 4), (0, -1, 4, 4), (3, 3, 0, 4), (3, 3, 4, 0), (n, 0, 1, 1),
           (0, 0, 2 ** 31 - 1, 1)]
    lib, h = plan.lib, plan._h
    for w in bad:
        for wi, wo in ((w, ok), (ok, w)):
            assert lib.hbx_evaluate_real_window(h, ptr(x), _win(wi), None, _win(wo), b, None, ptr(out), None, None,
                                                _stream()) == _lib.ERR_INVALID
            assert lib.hbx_evaluate_threshold_window(h, ptr(x), C.c_float(TAU), _win(wi), None, _win(wo), b, None,
                                                     ptr(out), None, None, _stream()) == _lib.ERR_INVALID
            assert lib.hbx_backward_window(h, ptr(cv), None, C.c_float(1), _win(wi), None, 0, C.c_float(0),
                                           C.c_float(0), _win(wo), b, ptr(out), _stream()) == _lib.ERR_INVALID
        assert lib.hbx_loss_window(h, ptr(stats), _win(w), b, 0, 1, ptr(ld), _stream()) == _lib.ERR_INVALID
        assert lib.hbx_loss_weight_window(h, ptr(out), ptr(out), ptr(stats), None, _win(w), b, 0, 1, ptr(out),
                                          _stream()) == _lib.ERR_INVALID
    assert b"window" in lib.hbx_last_error()
    torch.cuda.synchronize()   # nothing was enqueued, and nothing faulted
    low = plan_for(name, precision=_lib.PRECISION_BF16_STORE)
    assert low.lib.hbx_evaluate_real_window(low._h, ptr(x), None, None, None, b, None, ptr(out), None, None,
                                            _stream()) == _lib.ERR_UNSUPPORTED
    assert low.lib.hbx_backward_window(low._h, ptr(cv), None, C.c_float(1), None, None, 0, C.c_float(0), C.c_float(0),
                                       None, b, ptr(out), _stream()) == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()
