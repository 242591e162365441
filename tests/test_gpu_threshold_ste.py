"""Binary holograms from a real leaf through the C-ABI (Plan.evaluate_threshold / threshold_backward).

The first pass forms u = va + vb [x >= tau] from float32 samples x as it loads them, so every output
is evaluate_real's on the materialised samples bit for bit; the last pass of threshold_backward
writes vb s(x) Re g instead of the complex plane g, s the window or the sigmoid surrogate.
Samples: uniform in [-0.5, 1.5], with tau, the window's two ends, +-inf and NaN planted in every plane.
Shapes (N, G, P): 64 with G = 1 and 3, 256 with P = 2 and 6 (the R = 16 last pass double-buffers
plane pairs: three pairs run its odd tail) and with G = 3, 896 and 1024 with P = 2.  P is the plan's
real plane count per group: P planes of the forward leaf, P / 2 complex planes of the backward."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import hbx_oracle as O  # noqa: E402
from tests.test_threshold_ste_host import (STE_SIGMOID, STE_WINDOW, binarize, field_values,  # noqa: E402
                                           ste_gradient)

FIELD_RTOL = 2e-5
MSE_RTOL = 2.31e-5
PSNR_ATOL = 1e-4
TAU = 0.5
WIDTH = np.float32(0.3)
LO, HI = float(np.float32(np.float32(TAU) - WIDTH)), float(np.float32(np.float32(TAU) + WIDTH))
# the sigmoid form against its float64 restatement, as a fraction of (k / 4) max|real_part|: the worst
# case measured over the shapes below and both field kinds on one MI355X (N = 1024, binary phase; the
# record is in profiles/binary_ste/new_tests_gpu.txt), asserted at four times that
SIGMOID_MEASURED = 2.447e-7
SIGMOID_K = 4.0

# name: (N, G, P)
CASES = {"64": (64, 1, 2), "64rgb": (64, 3, 2), "256p2": (256, 1, 2), "256p6": (256, 1, 6), "256rgb": (256, 3, 2),
         "896": (896, 1, 2), "1024": (1024, 1, 2)}
ALL = list(CASES)
KINDS = {"amplitude": O.FIELD_AMPLITUDE, "phase": O.FIELD_PHASE}


def ocfg_for(name, field_kind=O.FIELD_AMPLITUDE):
    n, g, p = CASES[name]
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


SPECIALS = (TAU, LO, HI, np.inf, -np.inf, np.nan, np.nextafter(np.float32(TAU), np.float32(0)),
            np.nextafter(np.float32(LO), np.float32(-1)), np.nextafter(np.float32(HI), np.float32(2)))


def _samples(rng, shape):
    """uniform in [-0.5, 1.5], float32; every plane gets each special value at a few pixels of its own
    (the first and the last pixel of the plane among them)"""
    x = (2.0 * rng.random(shape, dtype=np.float32) - 0.5).astype(np.float32)
    flat = x.reshape(-1, shape[-2] * shape[-1])
    for plane in flat:
        idx = rng.choice(plane.size - 2, size=3 * len(SPECIALS), replace=False) + 1
        plane[idx] = np.tile(np.array(SPECIALS, np.float32), 3)
        plane[0], plane[-1] = np.float32(TAU), np.float32(np.nan)
    return x


@functools.lru_cache(maxsize=None)
def _case(name):
    """(x float32 [1, G P, N, N], target float32 [1, G, N, N]), read-only"""
    n, g, p = CASES[name]
    rng = np.random.default_rng(3100 + n + 7 * p + g)
    x = _samples(rng, (1, g * p, n, n))
    target = rng.random((1, g, n, n), dtype=np.float32)
    for a in (x, target):
        a.setflags(write=False)
    return x, target


@functools.lru_cache(maxsize=None)
def _oracle_field(name, field_kind):
    """complex128 [G P, N, N]: the float64 oracle's field of the binarised samples"""
    n, g, p = CASES[name]
    ocfg = ocfg_for(name)
    u = binarize(_case(name)[0][0], TAU, field_kind).astype(np.float64)
    want = np.concatenate([O.propagate(u[k * p:(k + 1) * p], ocfg.transfer(k)) for k in range(g)])
    want.setflags(write=False)
    return want


def _err(got, want):
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


def _eq(a, b):
    if a.is_complex():
        a, b = torch.view_as_real(a), torch.view_as_real(b)
    return torch.equal(a, b)


# -- forward ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("name", ALL)
def test_evaluate_threshold_is_evaluate_real_on_the_binarised_samples(name, kind):
    """Every output, every subset of the outputs, with array_equal; the amplitude statistics and PSNR
    also equal the bit path's on hbx.pack_mask(x, threshold=tau) bit for bit (binary phase: printed, and
    both held to the oracle bounds); the field within FIELD_RTOL of the float64 oracle.  At 896 the
    four padding slots of a lane must stay zero: `lo` = 1 there under binary phase would put a constant
    into the row FFT."""
    import hbx
    from hbx import _lib
    fk = KINDS[kind]
    n, g, p = CASES[name]
    ocfg = ocfg_for(name, fk)
    x_np, t_np = _case(name)
    mat_np = binarize(x_np, TAU, fk)
    va, vb = field_values(fk)
    assert set(np.unique(mat_np).tolist()) == {va, va + vb}
    x, mat, target = (torch.from_numpy(a.copy()).cuda() for a in (x_np, mat_np, t_np))
    plan = hbx.Plan(dev_cfg(ocfg), max_jobs=g)
    f_t, i_t, s_t, p_t = plan.evaluate_threshold(x, TAU, target)
    f_r, i_r, s_r, p_r = plan.evaluate_real(mat, target)
    none_f, i_n, s_n, p_n = plan.evaluate_threshold(x, TAU, target, want_field=False)
    _, none_i, s_only, p_only = plan.evaluate_threshold(x, TAU, target, want_field=False, want_intensity=False)
    _, i_alone, s_none, p_none = plan.evaluate_threshold(x, TAU, None, want_field=False)
    f_alone, i_none, _, _ = plan.evaluate_threshold(x, TAU, None, want_intensity=False)
    f_sim, i_sim = plan.simulate_real(mat, want_intensity=True)
    _, s_bits, p_bits = plan.propagate(hbx.pack_mask(x, threshold=TAU), target, want_intensity=False)
    mse = plan.loss(s_t, _lib.LOSS_MSE, _lib.REL_LSQ)
    torch.cuda.synchronize()
    assert f_t.dtype == torch.complex64 and tuple(f_t.shape) == x_np.shape
    assert none_f is None and none_i is None and s_none is None and p_none is None and i_none is None
    assert _eq(f_t, f_r) and _eq(i_t, i_r) and _eq(s_t, s_r) and _eq(p_t, p_r)
    assert _eq(i_n, i_r) and _eq(s_n, s_r) and _eq(p_n, p_r)
    assert _eq(s_only, s_r) and _eq(p_only, p_r)
    assert _eq(i_alone, plan.intensity_real(mat))
    assert _eq(f_alone, f_sim) and _eq(i_alone, i_sim) and _eq(f_alone, f_t)
    d_s = float((s_t - s_bits).abs().max() / s_bits.abs().max())
    d_p = float((p_t - p_bits).abs().max())
    print(f"{name} {kind}: against the bit path: chan_stats {d_s:.3e} of max, psnr {d_p:.3e} dB")
    if fk == O.FIELD_AMPLITUDE:
        assert _eq(s_t, s_bits) and _eq(p_t, p_bits)
    want = _oracle_field(name, fk)
    e_f = _err(f_t[0].cpu().numpy(), want)
    want_i = np.mean(np.abs(want.reshape(g, p, n, n)) ** 2, axis=1)
    t64 = t_np[0].astype(np.float64)
    w_mse, w_psnr = O.relative_mse(want_i, t64, O.REL_LSQ), O.relative_psnr(want_i, t64, O.REL_LSQ)
    e_mse, e_psnr = abs(float(mse[0]) - w_mse) / w_mse, abs(float(p_t[0]) - w_psnr)
    e_bits = abs(float(p_bits[0]) - w_psnr)
    print(f"{name} {kind}: field err {e_f:.3e} of max|field|, MSE rel err {e_mse:.3e}, PSNR err {e_psnr:.3e} dB "
          f"(bit path {e_bits:.3e} dB)")
    assert e_f <= FIELD_RTOL
    assert e_mse <= MSE_RTOL
    assert e_psnr <= PSNR_ATOL and e_bits <= PSNR_ATOL
    plan.close()


# -- backward --------------------------------------------------------------------------------------
def _backward_inputs(name):
    n, g, p = CASES[name]
    q = p // 2
    rng = np.random.default_rng(3300 + n + 7 * p + g)
    shape = (1, g * q, n, n)
    x = _samples(rng, shape)
    v = ((2 * rng.random(shape, dtype=np.float32) - 1) + 1j * (2 * rng.random(shape, dtype=np.float32) - 1))
    w = rng.random((1, g, n, n), dtype=np.float32)
    return x, v.astype(np.complex64), w, q


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("name", ALL)
def test_window_backward_is_the_gated_real_part(name, kind, weighted):
    """grad = where(lo <= x <= hi, vb real_part, +0) with array_equal, real_part what simulate_complex
    (_weighted) writes for the same inputs; vb = 1 or -2 is exact.  Samples at lo and hi are inside,
    their float32 neighbours outside, NaN and +-inf outside.  The infinite window is vb real_part."""
    import hbx
    fk = KINDS[kind]
    n, g, p = CASES[name]
    vb = field_values(fk)[1]
    x_np, v_np, w_np, q = _backward_inputs(name)
    vals, x = torch.from_numpy(v_np).cuda(), torch.from_numpy(x_np).cuda()
    w = torch.from_numpy(w_np).cuda() if weighted else None
    plan = hbx.Plan(dev_cfg(ocfg_for(name, fk), z=-O.Z_DEFAULT), max_jobs=g)
    grad = plan.threshold_backward(vals, x, weight=w, scale=2.0 / q, surrogate=STE_WINDOW, p0=LO, p1=HI)
    full = plan.threshold_backward(vals, x, weight=w, scale=2.0 / q)
    _, real = plan.simulate_complex(vals, want_field=False, want_real=True, weight=w, scale=2.0 / q)
    again = plan.threshold_backward(vals, x, weight=w, scale=2.0 / q, surrogate=STE_WINDOW, p0=LO, p1=HI)
    torch.cuda.synchronize()
    assert grad.dtype == torch.float32 and tuple(grad.shape) == x_np.shape
    assert torch.equal(again, grad)
    got, r = grad.cpu().numpy(), real.cpu().numpy()
    gate = (x_np >= np.float32(LO)) & (x_np <= np.float32(HI))
    assert 0.2 < gate.mean() < 0.4                               # [0.2, 0.8] of [-0.5, 1.5]
    assert gate[x_np == np.float32(LO)].all() and gate[x_np == np.float32(HI)].all() and not gate[~np.isfinite(x_np)].any()
    want = np.where(gate, np.float32(vb) * r, np.float32(0))
    assert np.array_equal(got, want)
    assert not np.signbit(got[~gate]).any()                      # a closed gate is +0
    nan = np.isnan(x_np)
    want_full = np.where(nan, np.float32(0), np.float32(vb) * r)  # a NaN sample closes even the infinite window
    assert np.array_equal(full.cpu().numpy(), want_full)
    assert np.abs(got).max() > 0
    plan.close()


def test_a_closed_gate_writes_zero_whatever_the_gradient_holds():
    """One NaN and one inf among `values` make every sample of g NaN: open gates pass it on, closed
    gates store +0.0 (a select, not a multiply by 0)."""
    import hbx
    for kind, fk in KINDS.items():
        x_np, v_np, w_np, q = _backward_inputs("64")
        v_np = v_np.copy()
        v_np[0, 0, 3, 5] = np.nan
        v_np[0, 0, 40, 41] = np.inf
        plan = hbx.Plan(dev_cfg(ocfg_for("64", fk), z=-O.Z_DEFAULT), max_jobs=1)
        vals, x = torch.from_numpy(v_np).cuda(), torch.from_numpy(x_np).cuda()
        grad = plan.threshold_backward(vals, x, surrogate=STE_WINDOW, p0=LO, p1=HI).cpu().numpy()
        _, real = plan.simulate_complex(vals, want_field=False, want_real=True)
        assert bool(torch.isnan(real).all())
        gate = (x_np >= np.float32(LO)) & (x_np <= np.float32(HI))
        assert np.isnan(grad[gate]).all()
        assert (grad[~gate] == 0).all() and not np.signbit(grad[~gate]).any()
        plan.close()


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("name", ALL)
def test_sigmoid_backward_against_the_float64_formula(name, kind):
    """grad against vb s(x) real_part in float64 from the kernel's own real_part (weighted), s = k sg
    (1 - sg), as a fraction of (k / 4) max|real_part| -- k / 4 is the surrogate's maximum.  The float32
    evaluation rounds k (x - tau), exp, 1 + e, the square, the quotient and two products: a few ulp of
    a value <= k / 4, and float32 exp implementations differ by a few ulp.
    Measured: 7.2e-8 to 1.2e-7 with binary amplitude (vb = 1) and twice that, 1.4e-7 to 2.447e-7, with
    binary phase (vb = -2; the fraction does not count |vb|) over the seven shapes; the worst,
    2.447e-7 at N = 1024, is SIGMOID_MEASURED.  Asserted at four times that, 9.8e-7, and a value above
    1e-5 is a bug, not a tolerance.  NaN samples give NaN; +-inf give 0."""
    import hbx
    fk = KINDS[kind]
    n, g, p = CASES[name]
    vb = field_values(fk)[1]
    x_np, v_np, w_np, q = _backward_inputs(name)
    vals, x, w = torch.from_numpy(v_np).cuda(), torch.from_numpy(x_np).cuda(), torch.from_numpy(w_np).cuda()
    plan = hbx.Plan(dev_cfg(ocfg_for(name, fk), z=-O.Z_DEFAULT), max_jobs=g)
    grad = plan.threshold_backward(vals, x, weight=w, scale=2.0 / q, surrogate=STE_SIGMOID, p0=TAU, p1=SIGMOID_K)
    _, real = plan.simulate_complex(vals, want_field=False, want_real=True, weight=w, scale=2.0 / q)
    torch.cuda.synchronize()
    got, r = grad.cpu().numpy().astype(np.float64), real.cpu().numpy().astype(np.float64)
    want = ste_gradient(r, x_np, vb, STE_SIGMOID, TAU, SIGMOID_K)
    nan = np.isnan(x_np)
    assert np.isnan(got[nan]).all() and not np.isnan(got[~nan]).any()
    assert (got[np.isinf(x_np)] == 0).all()
    rmax = float(np.max(np.abs(r)))
    e = float(np.max(np.abs(got[~nan] - want[~nan]))) / (SIGMOID_K / 4 * rmax)
    print(f"{name} {kind}: sigmoid |grad - want| = {e:.3e} of (k / 4) max|real_part|, max|real_part| = {rmax:.3e}")
    assert rmax > 0
    assert e <= 1e-5
    assert e <= 4 * SIGMOID_MEASURED
    plan.close()


# -- chunking --------------------------------------------------------------------------------------
def test_chunking_by_max_jobs():
    """n_env = 3 on a plan of two envs per chunk (max_jobs = 2 G) against a plan that takes all three
    at once: values advance in floats per chunk forward, in float2 backward, samples and grad in floats."""
    import hbx
    n, g, p = CASES["64rgb"]
    q = p // 2
    rng = np.random.default_rng(3400)
    x = torch.from_numpy(_samples(rng, (3, g * p, n, n))).cuda()
    xs = torch.from_numpy(_samples(rng, (3, g * q, n, n))).cuda()
    v = torch.from_numpy(((2 * rng.random((3, g * q, n, n), dtype=np.float32) - 1) +
                          1j * rng.random((3, g * q, n, n), dtype=np.float32)).astype(np.complex64)).cuda()
    target = torch.from_numpy(rng.random((3, g, n, n), dtype=np.float32)).cuda()
    out = []
    for jobs in (2 * g, 3 * g):
        plan = hbx.Plan(dev_cfg(ocfg_for("64rgb", O.FIELD_PHASE)), max_jobs=jobs)
        f, i, s, ps = plan.evaluate_threshold(x, TAU, target)
        _, i_alone, _, _ = plan.evaluate_threshold(x, TAU, None, want_field=False)
        gw = plan.threshold_backward(v, xs, weight=target, scale=1.0, surrogate=STE_WINDOW, p0=LO, p1=HI)
        gs = plan.threshold_backward(v, xs, surrogate=STE_SIGMOID, p0=TAU, p1=SIGMOID_K)
        torch.cuda.synchronize()
        out.append([torch.view_as_real(f), i, s, ps, i_alone, gw, torch.nan_to_num(gs, nan=-7.0)])
        plan.close()
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert not torch.equal(out[0][5][2], out[0][5][0])      # the envs differ
    assert not torch.equal(out[0][1][2], out[0][1][0])


# -- error paths -----------------------------------------------------------------------------------
def test_error_paths_return_the_header_codes_and_enqueue_nothing():
    import hbx
    from hbx import _lib
    from hbx.plan import _ptr, _stream
    ocfg = O.OpticsConfig(64, 64, 1, 2, O.WL_MONO)
    plan = hbx.Plan(dev_cfg(ocfg), max_jobs=1)
    lib, h, st = plan.lib, plan._h, _stream(None)
    x = torch.zeros((1, 2, 64, 64), dtype=torch.float32, device="cuda")
    xs = torch.zeros((1, 1, 64, 64), dtype=torch.float32, device="cuda")
    v = torch.ones((1, 1, 64, 64), dtype=torch.complex64, device="cuda")
    tgt = torch.zeros((1, 1, 64, 64), dtype=torch.float32, device="cuda")
    sentinel = 7.0
    outs = {k: torch.full(s, sentinel, dtype=d, device="cuda") for k, (s, d) in {
        "field": ((1, 2, 64, 64, 2), torch.float32), "inten": ((1, 1, 64, 64), torch.float32),
        "stats": ((1, 1, 3), torch.float64), "psnr": ((1,), torch.float64),
        "grad": ((1, 1, 64, 64), torch.float32)}.items()}
    f, i, s, p, g = (_ptr(outs[k]) for k in ("field", "inten", "stats", "psnr", "grad"))
    inv, uns = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
    W, S = STE_WINDOW, STE_SIGMOID
    ev, bw = lib.hbx_evaluate_threshold, lib.hbx_threshold_backward
    calls = [
        (inv, lambda: ev(h, None, 0.5, _ptr(tgt), 1, f, i, s, p, st)),
        (inv, lambda: ev(h, _ptr(x), 0.5, _ptr(tgt), 1, f, i, None, p, st)),        # target without chan_stats
        (inv, lambda: ev(h, _ptr(x), 0.5, None, 1, f, i, s, None, st)),             # chan_stats without target
        (inv, lambda: ev(h, _ptr(x), 0.5, None, 1, f, i, None, p, st)),             # no target: no psnr
        (inv, lambda: ev(h, _ptr(x), 0.5, None, 1, None, None, None, None, st)),    # no output
        (inv, lambda: ev(h, _ptr(x), 0.5, _ptr(tgt), -2, f, i, s, p, st)),
        (inv, lambda: bw(h, None, _ptr(tgt), 1.0, _ptr(xs), W, 0.0, 1.0, 1, g, st)),
        (inv, lambda: bw(h, _ptr(v), _ptr(tgt), 1.0, None, W, 0.0, 1.0, 1, g, st)),
        (inv, lambda: bw(h, _ptr(v), _ptr(tgt), 1.0, _ptr(xs), W, 0.0, 1.0, 1, None, st)),
        (inv, lambda: bw(h, _ptr(v), None, 1.0, _ptr(xs), 2, 0.0, 1.0, 1, g, st)),      # an unknown surrogate
        (inv, lambda: bw(h, _ptr(v), None, 1.0, _ptr(xs), -1, 0.0, 1.0, 1, g, st)),
        (inv, lambda: bw(h, _ptr(v), None, 1.0, _ptr(xs), S, 0.5, 0.0, 1, g, st)),      # the sigmoid's p1 <= 0
        (inv, lambda: bw(h, _ptr(v), None, 1.0, _ptr(xs), S, 0.5, -1.0, 1, g, st)),
        (inv, lambda: bw(h, _ptr(v), None, 1.0, _ptr(xs), S, 0.5, float("nan"), 1, g, st)),
        (inv, lambda: bw(h, _ptr(v), None, 1.0, _ptr(xs), W, 0.0, 1.0, -1, g, st)),
    ]
    for k, (code, call) in enumerate(calls):
        assert call() == code, k
    # n_env == 0 is OK and does nothing
    assert ev(h, _ptr(x), 0.5, _ptr(tgt), 0, f, i, s, p, st) == _lib.OK
    assert bw(h, _ptr(v), None, 1.0, _ptr(xs), W, 0.0, 1.0, 0, g, st) == _lib.OK
    plan.precision = _lib.PRECISION_BF16_STORE
    assert ev(h, _ptr(x), 0.5, _ptr(tgt), 1, f, i, s, p, st) == uns
    assert bw(h, _ptr(v), None, 1.0, _ptr(xs), W, 0.0, 1.0, 1, g, st) == uns
    with pytest.raises(_lib.HbxError) as e:
        plan.evaluate_threshold(x, 0.5)
    assert e.value.code == uns and "F32" in str(e.value)
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert bool((t == sentinel).all()), f"{k} was written by a refused call"
    plan.precision = _lib.PRECISION_F32
    # the same buffers, accepted: every output is written (a window that is empty still stores its zeros)
    assert ev(h, _ptr(x), 0.5, _ptr(tgt), 1, f, i, s, p, st) == _lib.OK
    assert bw(h, _ptr(v), None, 1.0, _ptr(xs), W, 1.0, -1.0, 1, g, st) == _lib.OK
    torch.cuda.synchronize()
    for k in ("field", "inten", "stats", "psnr", "grad"):
        assert not bool((outs[k] == sentinel).any()), k
    assert bool((outs["grad"] == 0).all())
    plan.close()


def test_plan_argument_checks():
    import hbx
    ocfg = O.OpticsConfig(64, 64, 1, 4, O.WL_MONO)
    plan = hbx.Plan(dev_cfg(ocfg), max_jobs=1)
    x = torch.zeros((1, 4, 64, 64), dtype=torch.float32, device="cuda")
    xs = torch.zeros((1, 2, 64, 64), dtype=torch.float32, device="cuda")
    v = torch.zeros((1, 2, 64, 64), dtype=torch.complex64, device="cuda")
    t = torch.zeros((1, 1, 64, 64), dtype=torch.float32, device="cuda")
    plan.evaluate_threshold(x, 0.5)
    plan.threshold_backward(v, xs)
    for call in (lambda: plan.evaluate_threshold(x.double(), 0.5), lambda: plan.evaluate_threshold(x, 0.5, t.double()),
                 lambda: plan.threshold_backward(xs, xs), lambda: plan.threshold_backward(v, v)):
        with pytest.raises(TypeError):
            call()
    for call in (lambda: plan.evaluate_threshold(xs, 0.5), lambda: plan.evaluate_threshold(x.cpu(), 0.5),
                 lambda: plan.evaluate_threshold(x.transpose(2, 3), 0.5),
                 lambda: plan.evaluate_threshold(x, 0.5, None, want_field=False, want_intensity=False),
                 lambda: plan.evaluate_threshold(x, 0.5, x), lambda: plan.threshold_backward(v, x),
                 lambda: plan.threshold_backward(v, xs, weight=xs)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(hbx._lib.HbxError):
        plan.threshold_backward(v, xs, surrogate=STE_SIGMOID, p0=0.5, p1=0.0)
    plan.close()
