"""hbx_evaluate_real, hbx_evaluate_complex, hbx_loss and hbx_loss_weight through hbx.Plan (ABI v15,
additive).

  1. evaluate_complex's field == simulate_complex's field bit for bit at all four built sizes (G = 2
     with two wavelengths, Q = 2 complex planes per group); the intensity-only and field-less calls
     give the full call's intensity bits;
  2. plane-loop edges, Q in {1, 2, 3} at N = 64 and 256: the intensity against float64
     mean_q |F_q|^2 of the GPU's own downloaded field and against the float64 oracle from the
     samples; chan_stats, psnr and hbx_loss (MSE and PSNR, both scales) against the oracle;
  3. the intensity and chan_stats at 896 and 1024 (G = 1, Q = 2);
  4. evaluate_real == simulate_real's field and propagate_real's intensity / stats / psnr, bit for
     bit, with and without the field, at all four sizes;
  5. chunking by max_jobs (three different chunk strides) for both calls;
  6. determinism;
  7. hbx_loss_weight against the float64 formulas within three float32 roundings, a null grad_loss,
     a degenerate env;
  8. argument and precision checks.
Tolerances are the project's (tests/test_gpu_real_field.py): field and intensity 2e-5 of the
maximum, chan_stats rtol 2e-5, PSNR 1e-4 dB, MSE relative 2.31e-5 (= 10^(1e-5) - 1, the PSNR bound
restated)."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import hbx_oracle as O  # noqa: E402
from tests.test_loss_host import LOSS_MSE, LOSS_PSNR, REL_LSQ, REL_NONE, loss_coeffs  # noqa: E402

INTEN_RTOL = 2e-5
STATS_RTOL = 2e-5
PSNR_ATOL = 1e-4
MSE_RTOL = 2.31e-5
WL2 = (638e-9, 450e-9)
BATCH = {64: 2, 256: 2, 896: 1, 1024: 1}
SIZES = [64, 256, 896, 1024]


def dev_cfg(n, planes, groups=2):
    import hbx
    o = O.OpticsConfig(n, n, groups, planes, WL2[:groups])
    return hbx.OpticsConfig(n, n, groups, planes, tuple(o.wavelengths), o.dx, o.dy, o.z, o.tf_kind, o.field_kind,
                            o.rel_scale, o.peak)


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm GPU")
    import hbx
    hbx.load_library()
    yield


@functools.lru_cache(maxsize=None)
def _cplx_case(n, b, g, q):
    """(values complex64 [b, g q, n, n] in [-1, 1)^2, target f32 [b, g, n, n] in [0, 1) -- no multiple of
    any intensity --), read-only"""
    rng = np.random.default_rng(1200 + n + 7 * b + 3 * g + q)
    shape = (b, g * q, n, n)
    vals = np.empty(shape, np.complex64)
    vals.real = 2.0 * rng.random(shape, dtype=np.float32) - 1.0
    vals.imag = 2.0 * rng.random(shape, dtype=np.float32) - 1.0
    tgt = rng.random((b, g, n, n), dtype=np.float32)
    vals.setflags(write=False)
    tgt.setflags(write=False)
    return vals, tgt


@functools.lru_cache(maxsize=None)
def _real_case(n, b, g, p):
    rng = np.random.default_rng(1300 + n + 7 * b + 3 * g + p)
    vals = (2.0 * rng.random((b, g * p, n, n), dtype=np.float32) - 1.0).astype(np.float32)
    tgt = rng.random((b, g, n, n), dtype=np.float32)
    vals.setflags(write=False)
    tgt.setflags(write=False)
    return vals, tgt


def _cuda(a):
    return torch.from_numpy(a.copy()).cuda()


def _bits(t):
    a = t.cpu().numpy()
    return a.view(np.float32) if np.iscomplexobj(a) else a


def _mean_abs2(field, g):
    """float64 mean over each group's planes of |field|^2: [b, g q, n, n] -> [b, g, n, n]"""
    f = field.astype(np.complex128)
    b, c, n, _ = f.shape
    return (f.real ** 2 + f.imag ** 2).reshape(b, g, c // g, n, n).mean(axis=2)


# -- 1. the field's bits -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_evaluate_complex_field_equals_simulate_complex_bitwise(n):
    import hbx
    b, g, q = BATCH[n], 2, 2
    vals, tgt = _cplx_case(n, b, g, q)
    plan = hbx.Plan(dev_cfg(n, 2 * q, g), max_jobs=b * g)
    v, t = _cuda(vals), _cuda(tgt)
    field, inten, stats, psnr = plan.evaluate_complex(v, t)
    want_f, _ = plan.simulate_complex(v)
    _, inten_only, s0, p0 = plan.evaluate_complex(v, None, want_field=False)
    f1, inten_nf, stats_nf, psnr_nf = plan.evaluate_complex(v, t, want_field=False)
    f2, i2, stats_only, _ = plan.evaluate_complex(v, t, want_field=False, want_intensity=False)
    torch.cuda.synchronize()
    assert s0 is None and p0 is None and f1 is None and f2 is None and i2 is None
    assert field.dtype == torch.complex64 and tuple(field.shape) == vals.shape
    assert inten.dtype == torch.float32 and tuple(inten.shape) == (b, g, n, n)
    assert stats.dtype == torch.float64 and tuple(stats.shape) == (b, g, 3)
    assert psnr.dtype == torch.float64 and tuple(psnr.shape) == (b,)
    assert float(want_f.abs().max()) > 0.0
    assert np.array_equal(_bits(field), _bits(want_f))
    assert np.array_equal(_bits(inten_only), _bits(inten))
    assert np.array_equal(_bits(inten_nf), _bits(inten))
    assert np.array_equal(_bits(stats_nf), _bits(stats)) and np.array_equal(_bits(stats_only), _bits(stats))
    assert np.array_equal(_bits(psnr_nf), _bits(psnr))
    # the two groups differ (another wavelength and target each), so a wrong index shows
    assert not np.array_equal(_bits(inten)[0, 0], _bits(inten)[0, 1])
    want_i = _mean_abs2(field.cpu().numpy(), g)
    err = np.max(np.abs(inten.cpu().numpy() - want_i)) / np.max(want_i)
    print(f"N={n}: intensity against float64 mean |F|^2 of the downloaded field {err:.3e} of max I")
    assert err <= INTEN_RTOL
    plan.close()


# -- 2. plane-loop edges against the oracle ------------------------------------------------------------
@pytest.mark.parametrize("q", [1, 2, 3])
@pytest.mark.parametrize("n", [64, 256])
def test_evaluate_complex_plane_counts_against_the_oracle(n, q):
    import hbx
    b, g = 2, 2
    vals, tgt = _cplx_case(n, b, g, q)
    ocfg = O.OpticsConfig(n, n, g, 2 * q, WL2)
    plan = hbx.Plan(dev_cfg(n, 2 * q, g), max_jobs=b * g)
    field, inten, stats, psnr = plan.evaluate_complex(_cuda(vals), _cuda(tgt))
    got_loss = {(k, r): plan.loss(stats, k, r).cpu().numpy()
                for k in (LOSS_MSE, LOSS_PSNR) for r in (REL_LSQ, REL_NONE)}
    same_psnr = plan.psnr(stats)
    torch.cuda.synchronize()
    gi = inten.cpu().numpy()
    # the GPU's own field, float64 arithmetic
    own = _mean_abs2(field.cpu().numpy(), g)
    e_own = np.max(np.abs(gi - own)) / np.max(own)
    # the oracle from the samples
    u = vals.astype(np.complex128)
    want_f = np.stack([np.concatenate([O.propagate(u[e, k * q:(k + 1) * q], ocfg.transfer(k)) for k in range(g)])
                       for e in range(b)])
    want_i = _mean_abs2(want_f, g)
    e_or = np.max(np.abs(gi - want_i)) / np.max(want_i)
    print(f"N={n} Q={q}: intensity err {e_own:.3e} (own field) {e_or:.3e} (oracle) of max I")
    assert e_own <= INTEN_RTOL
    assert e_or <= INTEN_RTOL
    t64 = tgt.astype(np.float64)
    gs, gp = stats.cpu().numpy(), psnr.cpu().numpy()
    assert np.array_equal(_bits(same_psnr), gp)        # hbx_psnr on the same statistics
    assert np.array_equal(got_loss[(LOSS_PSNR, REL_LSQ)], gp)   # the plan's rel_scale: hbx_psnr's bits
    for e in range(b):
        ws = np.stack([O.chan_stats(want_i[e, k], t64[e, k]) for k in range(g)])
        np.testing.assert_allclose(gs[e], ws, rtol=STATS_RTOL)
        assert abs(gp[e] - O.psnr_from_stats(ws, g * n * n, O.REL_LSQ, 1.0)) <= PSNR_ATOL
        for r in (REL_LSQ, REL_NONE):
            wm = O.relative_mse(want_i[e], t64[e], r)
            wp = O.psnr_from_stats(ws, g * n * n, r, 1.0)
            gm, gpp = got_loss[(LOSS_MSE, r)][e], got_loss[(LOSS_PSNR, r)][e]
            print(f"  env {e} rel {r}: mse {gm:.9e} (rel err {abs(gm - wm) / wm:.2e}), psnr {gpp:.6f} "
                  f"(err {abs(gpp - wp):.2e} dB)")
            assert abs(gm - wm) <= MSE_RTOL * wm
            assert abs(gpp - wp) <= PSNR_ATOL
    plan.close()


# -- 3. the large sizes ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [896, 1024])
def test_evaluate_complex_intensity_and_stats_at_the_large_sizes(n):
    import hbx
    b, g, q = 1, 1, 2
    vals, tgt = _cplx_case(n, b, g, q)
    plan = hbx.Plan(dev_cfg(n, 2 * q, g), max_jobs=b * g)
    field, inten, stats, _ = plan.evaluate_complex(_cuda(vals), _cuda(tgt))
    torch.cuda.synchronize()
    want_i = _mean_abs2(field.cpu().numpy(), g)
    gi = inten.cpu().numpy()
    err = np.max(np.abs(gi - want_i)) / np.max(want_i)
    print(f"N={n}: intensity err {err:.3e} of max I")
    assert err <= INTEN_RTOL
    ws = O.chan_stats(want_i[0, 0], tgt[0, 0].astype(np.float64))
    np.testing.assert_allclose(stats.cpu().numpy()[0, 0], ws, rtol=STATS_RTOL)
    plan.close()


# -- 4. evaluate_real ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_evaluate_real_equals_simulate_real_and_propagate_real_bitwise(n):
    import hbx
    b, g, p = BATCH[n], 2, 4
    vals, tgt = _real_case(n, b, g, p)
    plan = hbx.Plan(dev_cfg(n, p, g), max_jobs=b * g)
    v, t = _cuda(vals), _cuda(tgt)
    field, inten, stats, psnr = plan.evaluate_real(v, t)
    none_f, inten2, stats2, psnr2 = plan.evaluate_real(v, t, want_field=False)
    want_f, _ = plan.simulate_real(v)
    want_i, want_s, want_p = plan.propagate_real(v, t)
    torch.cuda.synchronize()
    assert none_f is None
    assert field.dtype == torch.complex64 and tuple(field.shape) == vals.shape
    assert float(want_f.abs().max()) > 0.0 and float(want_i.max()) > 0.0
    assert np.array_equal(_bits(field), _bits(want_f))
    for got in ((inten, stats, psnr), (inten2, stats2, psnr2)):
        assert np.array_equal(_bits(got[0]), _bits(want_i))
        assert np.array_equal(_bits(got[1]), _bits(want_s))
        assert np.array_equal(_bits(got[2]), _bits(want_p))
    plan.close()


# -- 5. chunking -------------------------------------------------------------------------------------
def test_evaluate_complex_chunked_equals_one_launch():
    """n_env = 3 on a plan of max_jobs = G (one env per chunk) and on one of 3 G (one chunk): the
    planes', the images' and the statistics' chunk strides all differ"""
    import hbx
    g, q = 2, 2
    vals, tgt = _cplx_case(64, 3, g, q)
    v, t = _cuda(vals), _cuda(tgt)
    small, big = hbx.Plan(dev_cfg(64, 2 * q, g), max_jobs=g), hbx.Plan(dev_cfg(64, 2 * q, g), max_jobs=3 * g)
    a, c = small.evaluate_complex(v, t), big.evaluate_complex(v, t)
    torch.cuda.synchronize()
    for x, y in zip(a, c):
        assert np.array_equal(_bits(x), _bits(y))
        assert not np.array_equal(_bits(x)[2], _bits(x)[0])
    small.close()
    big.close()


def test_evaluate_real_chunked_equals_one_launch():
    import hbx
    g, p = 2, 4
    vals, tgt = _real_case(64, 3, g, p)
    v, t = _cuda(vals), _cuda(tgt)
    small, big = hbx.Plan(dev_cfg(64, p, g), max_jobs=g), hbx.Plan(dev_cfg(64, p, g), max_jobs=3 * g)
    a, c = small.evaluate_real(v, t), big.evaluate_real(v, t)
    torch.cuda.synchronize()
    for x, y in zip(a, c):
        assert np.array_equal(_bits(x), _bits(y))
        assert not np.array_equal(_bits(x)[2], _bits(x)[0])
    small.close()
    big.close()


# -- 6. determinism ----------------------------------------------------------------------------------
def test_evaluate_complex_is_deterministic():
    import hbx
    b, g, q = 2, 2, 2
    vals, tgt = _cplx_case(256, b, g, q)
    plan = hbx.Plan(dev_cfg(256, 2 * q, g), max_jobs=b * g)
    v, t = _cuda(vals), _cuda(tgt)
    first = plan.evaluate_complex(v, t)
    second = plan.evaluate_complex(v, t)
    torch.cuda.synchronize()
    for x, y in zip(first, second):
        assert np.array_equal(_bits(x), _bits(y))
    plan.close()


# -- 7. hbx_loss_weight ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [LOSS_MSE, LOSS_PSNR], ids=["mse", "psnr"])
@pytest.mark.parametrize("rel", [REL_LSQ, REL_NONE], ids=["lsq", "none"])
def test_loss_weight_against_the_float64_formulas(kind, rel):
    """|w - w64| <= 4 * 2^-24 (|a I| + |c T|) per pixel: the roundings of a, c to float32, of c * T and of
    the fused multiply-add.  Env 2 is all zeros: degenerate under the least-squares scale."""
    import hbx
    b, g, q, n = 3, 2, 2, 64
    vals, tgt = _cplx_case(n, b, g, q)
    vals = vals.copy()
    vals[2] = 0
    plan = hbx.Plan(dev_cfg(n, 2 * q, g), max_jobs=b * g)
    t = _cuda(tgt)
    _, inten, stats, _ = plan.evaluate_complex(_cuda(vals), t, want_field=False)
    up = np.array([1.0, -0.5, 2.0])
    w = plan.loss_weight(inten, t, stats, torch.from_numpy(up).cuda(), kind, rel)
    w_null = plan.loss_weight(inten, t, stats, None, kind, rel)
    w_ones = plan.loss_weight(inten, t, stats, torch.ones(b, dtype=torch.float64, device="cuda"), kind, rel)
    torch.cuda.synchronize()
    gw, gi, gs = w.cpu().numpy(), inten.cpu().numpy().astype(np.float64), stats.cpu().numpy()
    assert w.dtype == torch.float32 and tuple(w.shape) == (b, g, n, n)
    assert np.all(np.isfinite(gw)) and np.all(np.isfinite(w_null.cpu().numpy()))
    assert np.array_equal(_bits(w_null), _bits(w_ones))
    assert float(np.max(gi[2])) == 0.0 and gs[2, 0, 1] == 0.0
    t64 = tgt.astype(np.float64)
    for e in range(b):
        a, c = loss_coeffs(gs[e], kind, rel, g * n * n, up[e])
        w64 = a * gi[e] + c * t64[e]
        bound = 4.0 * 2.0 ** -24 * (np.abs(a * gi[e]) + np.abs(c * t64[e]))
        over = np.max(np.abs(gw[e] - w64) - bound)
        print(f"env {e}: a {a:.6e} c {c:.6e} max|w| {np.max(np.abs(w64)):.3e} worst excess over the bound {over:.3e}")
        assert over <= 0.0
        if e < 2:
            assert np.max(np.abs(w64)) > 0.0
    if rel == REL_LSQ:
        assert not gw[2].any()                          # the degenerate env: an all-zero weight
    plan.close()


# -- 8. argument and precision checks -------------------------------------------------------------------
def test_c_abi_argument_checks():
    import hbx
    from hbx import _lib
    lib = _lib.load()
    g, p, n = 2, 4, 64
    plan = hbx.Plan(dev_cfg(n, p, g), max_jobs=g)
    v = torch.zeros((1, g * p // 2, n, n), dtype=torch.complex64, device="cuda")
    vr = torch.zeros((1, g * p, n, n), dtype=torch.float32, device="cuda")
    tg = torch.ones((1, g, n, n), dtype=torch.float32, device="cuda")
    f = torch.empty((1, g * p, n, n, 2), dtype=torch.float32, device="cuda")
    it = torch.empty((1, g, n, n), dtype=torch.float32, device="cuda")
    cs = torch.ones((1, g, 3), dtype=torch.float64, device="cuda")
    ps = torch.empty((1,), dtype=torch.float64, device="cuda")
    h, null = plan._h, C.c_void_p(None)
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    ok, bad = _lib.OK, _lib.ERR_INVALID
    ec, er = lib.hbx_evaluate_complex, lib.hbx_evaluate_real
    assert ec(h, P(v), P(tg), 1, P(f), P(it), P(cs), P(ps), null) == ok
    assert ec(h, P(v), P(tg), 1, null, null, P(cs), null, null) == ok      # at least chan_stats is written
    assert ec(h, P(v), null, 1, null, P(it), null, null, null) == ok       # the intensity-only call
    assert ec(h, P(v), null, 1, P(f), P(it), null, null, null) == ok
    assert ec(h, null, P(tg), 1, P(f), P(it), P(cs), P(ps), null) == bad
    assert ec(h, P(v), P(tg), 1, P(f), P(it), null, null, null) == bad     # target without chan_stats
    assert ec(h, P(v), null, 1, P(f), P(it), P(cs), null, null) == bad     # chan_stats without target
    assert ec(h, P(v), null, 1, P(f), null, null, null, null) == bad       # neither target nor intensity
    assert ec(h, P(v), null, 1, null, P(it), null, P(ps), null) == bad     # psnr without statistics
    assert ec(h, null, null, 0, null, null, null, null, null) == ok
    assert ec(h, P(v), P(tg), -1, P(f), P(it), P(cs), P(ps), null) == bad
    assert er(h, P(vr), P(tg), 1, P(f), P(it), P(cs), P(ps), null) == ok
    assert er(h, P(vr), P(tg), 1, null, null, P(cs), null, null) == ok
    assert er(h, null, P(tg), 1, P(f), P(it), P(cs), P(ps), null) == bad
    assert er(h, P(vr), null, 1, P(f), P(it), P(cs), P(ps), null) == bad
    assert er(h, P(vr), P(tg), 1, P(f), P(it), null, P(ps), null) == bad
    assert er(h, null, null, 0, null, null, null, null, null) == ok
    assert er(h, P(vr), P(tg), -1, P(f), P(it), P(cs), P(ps), null) == bad
    ls, lw = lib.hbx_loss, lib.hbx_loss_weight
    assert ls(h, P(cs), 1, LOSS_MSE, REL_LSQ, P(ps), null) == ok
    assert ls(h, null, 1, LOSS_MSE, REL_LSQ, P(ps), null) == bad
    assert ls(h, P(cs), 1, LOSS_MSE, REL_LSQ, null, null) == bad
    assert ls(h, P(cs), 1, 2, REL_LSQ, P(ps), null) == bad
    assert ls(h, P(cs), 1, LOSS_PSNR, 2, P(ps), null) == bad
    assert ls(h, null, 0, LOSS_MSE, REL_LSQ, null, null) == ok
    assert ls(h, P(cs), -1, LOSS_MSE, REL_LSQ, P(ps), null) == bad
    wt = torch.empty((1, g, n, n), dtype=torch.float32, device="cuda")
    assert lw(h, P(it), P(tg), P(cs), P(ps), 1, LOSS_MSE, REL_LSQ, P(wt), null) == ok
    assert lw(h, P(it), P(tg), P(cs), null, 1, LOSS_PSNR, REL_NONE, P(wt), null) == ok
    assert lw(h, null, P(tg), P(cs), null, 1, LOSS_MSE, REL_LSQ, P(wt), null) == bad
    assert lw(h, P(it), null, P(cs), null, 1, LOSS_MSE, REL_LSQ, P(wt), null) == bad
    assert lw(h, P(it), P(tg), null, null, 1, LOSS_MSE, REL_LSQ, P(wt), null) == bad
    assert lw(h, P(it), P(tg), P(cs), null, 1, LOSS_MSE, REL_LSQ, null, null) == bad
    assert lw(h, P(it), P(tg), P(cs), null, 1, -1, REL_LSQ, P(wt), null) == bad
    assert lw(h, P(it), P(tg), P(cs), null, 1, LOSS_MSE, 7, P(wt), null) == bad
    assert lw(h, null, null, null, null, 0, LOSS_MSE, REL_LSQ, null, null) == ok
    assert lw(h, P(it), P(tg), P(cs), null, -1, LOSS_MSE, REL_LSQ, P(wt), null) == bad
    torch.cuda.synchronize()
    plan.close()


def test_reduced_precision_plan_is_unsupported():
    import hbx
    from hbx import _lib
    g, p, n = 2, 4, 64
    plan = hbx.Plan(dev_cfg(n, p, g), max_jobs=g, precision=_lib.PRECISION_BF16_STORE)
    v = torch.zeros((1, g * p // 2, n, n), dtype=torch.complex64, device="cuda")
    vr = torch.zeros((1, g * p, n, n), dtype=torch.float32, device="cuda")
    tg = torch.ones((1, g, n, n), dtype=torch.float32, device="cuda")
    with pytest.raises(_lib.HbxError) as e:
        plan.evaluate_complex(v, tg)
    assert e.value.code == _lib.ERR_UNSUPPORTED
    with pytest.raises(_lib.HbxError) as e:
        plan.evaluate_real(vr, tg)
    assert e.value.code == _lib.ERR_UNSUPPORTED
    plan.precision = _lib.PRECISION_F32
    plan.evaluate_complex(v, tg)
    plan.evaluate_real(vr, tg)
    plan.close()


def test_plan_method_argument_checks():
    import hbx
    g, p, n = 2, 4, 64
    plan = hbx.Plan(dev_cfg(n, p, g), max_jobs=g)
    v = torch.zeros((1, g * p // 2, n, n), dtype=torch.complex64, device="cuda")
    vr = torch.zeros((1, g * p, n, n), dtype=torch.float32, device="cuda")
    tg = torch.ones((1, g, n, n), dtype=torch.float32, device="cuda")
    _, inten, stats, _ = plan.evaluate_complex(v, tg, want_field=False)
    with pytest.raises(ValueError):     # without a target the intensity is the only output
        plan.evaluate_complex(v, None, want_intensity=False)
    with pytest.raises(TypeError):
        plan.evaluate_complex(vr, tg)
    with pytest.raises(ValueError):     # one target image per group, not per plane
        plan.evaluate_complex(v, torch.ones((1, g * p // 2, n, n), dtype=torch.float32, device="cuda"))
    with pytest.raises(TypeError):
        plan.evaluate_complex(v, tg.double())
    with pytest.raises(TypeError):
        plan.evaluate_real(v, tg)
    with pytest.raises(ValueError):
        plan.evaluate_real(vr, tg[:, :1])
    with pytest.raises(ValueError):
        plan.evaluate_real(vr, tg.cpu())
    with pytest.raises(TypeError):
        plan.loss(stats.float())
    with pytest.raises(ValueError):
        plan.loss(stats[:, :1])
    with pytest.raises(TypeError):      # grad_loss is float64
        plan.loss_weight(inten, tg, stats, torch.ones(1, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        plan.loss_weight(inten, tg, stats, torch.ones(2, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        plan.loss_weight(inten.transpose(2, 3), tg, stats)
    with pytest.raises(hbx._lib.HbxError):
        plan.loss(stats, 5)
    plan.close()
