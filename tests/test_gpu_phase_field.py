"""Phase holograms through the C-ABI (Plan.simulate_phase / evaluate_phase / phase_backward).

The first pass forms u = exp(i pi x) from float32 samples x as it loads them; the last pass of
phase_backward writes dL/dx = pi (Im g cos pi x - Re g sin pi x) instead of the complex gradient g.
Oracle: O.propagate(exp(i pi x64), h) with x64 the float64 of the float32 samples, so no input
rounding enters a comparison.  Bounds are the project's: field 2e-5 of max|field| (FIELD_RTOL),
intensity 2e-5 of max I, MSE 2.31e-5 relative, PSNR 1e-4 dB, and "new <= 2 x parent" where the parent
is simulate_complex on u formed in float64 on the host and rounded to complex64.
Shapes (N, G, Q complex planes per group): 64 with G = 3 for the logic, 256 with Q = 1, 2, 3 (the
R = 16 last pass double-buffers plane pairs), 896 and 1024 with Q = 2 (their plane loops)."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import hbx_oracle as O  # noqa: E402

FIELD_RTOL = 2e-5
MSE_RTOL = 2.31e-5
PSNR_ATOL = 1e-4

# name: (N, G, Q)
CASES = {"64": (64, 3, 2), "256q1": (256, 1, 1), "256q2": (256, 1, 2), "256q3": (256, 1, 3), "896": (896, 1, 2),
         "1024": (1024, 1, 2)}
ALL = list(CASES)


def ocfg_for(name):
    n, g, q = CASES[name]
    return O.OpticsConfig(n, n, g, 2 * q, O.WL_RGB if g == 3 else O.WL_MONO)


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


def _oracle_field(ocfg, x, q):
    """x [G * q, N, N] float32 phase samples -> complex128 field of every plane"""
    u = np.exp(1j * np.pi * x.astype(np.float64))
    return np.concatenate([O.propagate(u[k * q:(k + 1) * q], ocfg.transfer(k)) for k in range(ocfg.groups)])


@functools.lru_cache(maxsize=None)
def _case(name, span=1.0):
    """(x float32 [1, G Q, N, N] uniform in [-span, span), want complex128 [G Q, N, N], target float32
    [1, G, N, N]), read-only"""
    n, g, q = CASES[name]
    rng = np.random.default_rng(2100 + n + 7 * q + int(span))
    x = ((2.0 * rng.random((1, g * q, n, n)) - 1.0) * span).astype(np.float32)
    want = _oracle_field(ocfg_for(name), x[0], q)
    target = rng.random((1, g, n, n), dtype=np.float32)
    for a in (x, want, target):
        a.setflags(write=False)
    return x, want, target


def _err(got, want):
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


# -- 3. the field against the oracle -------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_simulate_phase_vs_oracle_and_the_complex_route(name):
    """At 896 the four padding slots of a lane must be zero, not exp(0) = 1: a one there puts a
    constant into the row FFT and misses the bound by orders of magnitude."""
    import hbx
    ocfg = ocfg_for(name)
    x, want, _ = _case(name)
    u = np.exp(1j * np.pi * x.astype(np.float64)).astype(np.complex64)
    plan = hbx.Plan(dev_cfg(ocfg), max_jobs=ocfg.groups)
    field, none_r = plan.simulate_phase(torch.from_numpy(x.copy()).cuda())
    ref, _ = plan.simulate_complex(torch.from_numpy(u).cuda())
    torch.cuda.synchronize()
    assert none_r is None and field.dtype == torch.complex64 and tuple(field.shape) == x.shape
    e_new, e_ref = _err(field[0].cpu().numpy(), want), _err(ref[0].cpu().numpy(), want)
    print(f"{name}: simulate_phase err {e_new:.3e}, simulate_complex(host u) err {e_ref:.3e} of max|field|")
    assert e_new <= FIELD_RTOL
    assert e_new <= 2.0 * e_ref
    plan.close()


# -- 4. wrapped phase ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["64", "256q2"])
def test_unwrapped_phase_keeps_the_field_bound(name):
    """Samples in [-4096, 4096): x * float32(pi) rounds the argument by up to 4096 * 2^-24 * pi turns
    (3.1e-4 of max|field| measured on the host formation); an exact reduction does not see |x|."""
    import hbx
    ocfg = ocfg_for(name)
    x, want, _ = _case(name, 4096.0)
    plan = hbx.Plan(dev_cfg(ocfg), max_jobs=ocfg.groups)
    field, _ = plan.simulate_phase(torch.from_numpy(x.copy()).cuda())
    torch.cuda.synchronize()
    e = _err(field[0].cpu().numpy(), want)
    print(f"{name}: |x| < 4096: field err {e:.3e} of max|field|")
    assert e <= FIELD_RTOL
    plan.close()


def test_exact_phases_give_the_exact_fields():
    """Whole planes of x = 0, 1, 0.5, -0.5, 2, -3 are u = 1, -1, i, -i, 1, -1 exactly."""
    import hbx
    ocfg = O.OpticsConfig(64, 64, 1, 12, O.WL_MONO)
    xs = np.array([0.0, 1.0, 0.5, -0.5, 2.0, -3.0], np.float32)
    us = np.array([1, -1, 1j, -1j, 1, -1], np.complex64)
    x = np.broadcast_to(xs[None, :, None, None], (1, 6, 64, 64)).copy()
    u = np.broadcast_to(us[None, :, None, None], (1, 6, 64, 64)).copy()
    plan = hbx.Plan(dev_cfg(ocfg), max_jobs=1)
    field, _ = plan.simulate_phase(torch.from_numpy(x).cuda())
    ref, _ = plan.simulate_complex(torch.from_numpy(u).cuda())
    torch.cuda.synchronize()
    got, want = field.cpu().numpy(), ref.cpu().numpy()
    for p in range(6):
        e = float(np.max(np.abs(got[0, p] - want[0, p])) / np.max(np.abs(want[0, p])))
        print(f"x = {xs[p]}: {e:.3e} of max")
        assert e <= 4e-7, (xs[p], e)
    plan.close()


# -- 5. bits -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["64", "256q3", "896", "1024"])
def test_outputs_agree_bit_for_bit(name):
    import hbx
    ocfg = ocfg_for(name)
    x_np, _, t_np = _case(name)
    x, target = torch.from_numpy(x_np.copy()).cuda(), torch.from_numpy(t_np.copy()).cuda()
    plan = hbx.Plan(dev_cfg(ocfg), max_jobs=ocfg.groups)
    field, real = plan.simulate_phase(x, want_field=True, want_real=True)
    _, r_only = plan.simulate_phase(x, want_field=False, want_real=True)
    f_ev, i_f, s_f, p_f = plan.evaluate_phase(x, target)
    none_f, i_n, s_n, p_n = plan.evaluate_phase(x, target, want_field=False)
    _, i_alone, s_none, p_none = plan.evaluate_phase(x, None, want_field=False)
    f_again, i_again, s_again, p_again = plan.evaluate_phase(x, target)
    torch.cuda.synchronize()
    assert none_f is None and s_none is None and p_none is None
    assert torch.equal(real, field.real) and torch.equal(r_only, real)
    assert torch.equal(torch.view_as_real(f_ev), torch.view_as_real(field))
    assert torch.equal(i_n, i_f) and torch.equal(s_n, s_f) and torch.equal(p_n, p_f)
    assert torch.equal(i_alone, i_f)
    assert torch.equal(torch.view_as_real(f_again), torch.view_as_real(f_ev))
    assert torch.equal(i_again, i_f) and torch.equal(s_again, s_f) and torch.equal(p_again, p_f)
    plan.close()


# -- 6. evaluate_phase against the oracle --------------------------------------------------------------
@pytest.mark.parametrize("name", ["64", "256q1", "256q2", "256q3"])
def test_evaluate_phase_vs_oracle(name):
    import hbx
    from hbx import _lib
    n, g, q = CASES[name]
    ocfg = ocfg_for(name)
    x_np, want, t_np = _case(name)
    want_i = np.mean(np.abs(want.reshape(g, q, n, n)) ** 2, axis=1)
    t64 = t_np[0].astype(np.float64)
    x, target = torch.from_numpy(x_np.copy()).cuda(), torch.from_numpy(t_np.copy()).cuda()
    plan = hbx.Plan(dev_cfg(ocfg), max_jobs=g)
    _, inten, stats, psnr = plan.evaluate_phase(x, target, want_field=False)
    _, i_alone, _, _ = plan.evaluate_phase(x, None, want_field=False)
    mse = plan.loss(stats, _lib.LOSS_MSE, _lib.REL_LSQ)
    torch.cuda.synchronize()
    for label, got in (("with target", inten), ("intensity only", i_alone)):
        e = _err(got[0].cpu().numpy().astype(np.float64), want_i)
        print(f"{name} {label}: intensity err {e:.3e} of max I")
        assert e <= FIELD_RTOL
    w_mse, w_psnr = O.relative_mse(want_i, t64, O.REL_LSQ), O.relative_psnr(want_i, t64, O.REL_LSQ)
    e_mse, e_psnr = abs(float(mse[0]) - w_mse) / w_mse, abs(float(psnr[0]) - w_psnr)
    print(f"{name}: MSE rel err {e_mse:.3e}, PSNR err {e_psnr:.3e} dB")
    assert e_mse <= MSE_RTOL
    assert e_psnr <= PSNR_ATOL
    plan.close()


# -- 7. phase_backward ---------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("name", ALL)
def test_phase_backward_is_the_chain_rule_of_its_own_g(name, weighted):
    """g = what simulate_complex(_weighted) writes for the same inputs (the same kernels up to the last
    pass's store, the same bits); want = pi (Im g cos pi x - Re g sin pi x) in float64 from that g.
    Error: the product roundings of the two terms and of the factor pi (a fused multiply-add, one
    multiply, pi itself: <= 3.5 * 2^-24 |g|) plus the sincos (<= 2 ulp each on values <= 1), derived
    as <= 4.2e-7 pi |g|; the bound is twice that."""
    import hbx
    n, g_, q = CASES[name]
    ocfg = ocfg_for(name)
    x_np, _, t_np = _case(name)
    rng = np.random.default_rng(2300 + n + q)
    v = ((2 * rng.random(x_np.shape, dtype=np.float32) - 1) +
         1j * (2 * rng.random(x_np.shape, dtype=np.float32) - 1)).astype(np.complex64)
    vals, x = torch.from_numpy(v).cuda(), torch.from_numpy(x_np.copy()).cuda()
    w = torch.from_numpy(t_np.copy()).cuda() if weighted else None
    plan = hbx.Plan(dev_cfg(ocfg, z=-ocfg.z), max_jobs=g_)
    grad = plan.phase_backward(vals, x, weight=w, scale=2.0 / q)
    gfield, _ = plan.simulate_complex(vals, weight=w, scale=2.0 / q)
    again = plan.phase_backward(vals, x, weight=w, scale=2.0 / q)
    torch.cuda.synchronize()
    assert grad.dtype == torch.float32 and tuple(grad.shape) == x_np.shape
    assert torch.equal(again, grad)
    g64, x64 = gfield.cpu().numpy().astype(np.complex128), x_np.astype(np.float64)
    want = np.pi * (g64.imag * np.cos(np.pi * x64) - g64.real * np.sin(np.pi * x64))
    gmax = float(np.max(np.abs(g64)))
    e = float(np.max(np.abs(grad.cpu().numpy().astype(np.float64) - want))) / (np.pi * gmax)
    print(f"{name} weighted={weighted}: |grad - want| <= {e:.3e} pi max|g|, max|g| = {gmax:.3e}")
    assert gmax > 0.0
    assert e <= 1e-6
    plan.close()


# -- 8. chunking ---------------------------------------------------------------------------------------
def test_chunking_by_max_jobs():
    """n_env = 3 on a plan of one env per chunk (max_jobs = G) against a plan that takes all three at
    once: phase and grad_phase advance in floats per chunk, values in float2."""
    import hbx
    ocfg = ocfg_for("64")
    n, g, q = CASES["64"]
    rng = np.random.default_rng(2400)
    x = torch.from_numpy((2 * rng.random((3, g * q, n, n), dtype=np.float32) - 1).astype(np.float32)).cuda()
    v = torch.from_numpy(((2 * rng.random((3, g * q, n, n), dtype=np.float32) - 1) +
                          1j * rng.random((3, g * q, n, n), dtype=np.float32)).astype(np.complex64)).cuda()
    target = torch.from_numpy(rng.random((3, g, n, n), dtype=np.float32)).cuda()
    out = []
    for jobs in (g, 3 * g):
        plan = hbx.Plan(dev_cfg(ocfg), max_jobs=jobs)
        field, real = plan.simulate_phase(x, want_field=True, want_real=True)
        f_ev, inten, stats, psnr = plan.evaluate_phase(x, target)
        grad = plan.phase_backward(v, x, weight=target, scale=1.0)
        grad_plain = plan.phase_backward(v, x)
        torch.cuda.synchronize()
        out.append([torch.view_as_real(field), real, torch.view_as_real(f_ev), inten, stats, psnr, grad, grad_plain])
        plan.close()
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert not torch.equal(out[0][6][2], out[0][6][0])      # the envs differ


# -- 9. error paths ------------------------------------------------------------------------------------
def test_error_paths_return_the_header_codes_and_enqueue_nothing():
    import hbx
    from hbx import _lib
    from hbx.plan import _ptr, _stream
    ocfg = O.OpticsConfig(64, 64, 1, 2, O.WL_MONO)
    plan = hbx.Plan(dev_cfg(ocfg), max_jobs=1)
    lib, h, st = plan.lib, plan._h, _stream(None)
    x = torch.zeros((1, 1, 64, 64), dtype=torch.float32, device="cuda")
    v = torch.ones((1, 1, 64, 64), dtype=torch.complex64, device="cuda")
    tgt = torch.zeros((1, 1, 64, 64), dtype=torch.float32, device="cuda")
    sentinel = 7.0
    outs = {k: torch.full(s, sentinel, dtype=d, device="cuda") for k, (s, d) in {
        "field": ((1, 1, 64, 64, 2), torch.float32), "real": ((1, 1, 64, 64), torch.float32),
        "inten": ((1, 1, 64, 64), torch.float32), "stats": ((1, 1, 3), torch.float64), "psnr": ((1,), torch.float64),
        "grad": ((1, 1, 64, 64), torch.float32)}.items()}
    f, r, i, s, p, g = (_ptr(outs[k]) for k in ("field", "real", "inten", "stats", "psnr", "grad"))
    inv, uns = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
    calls = [
        (inv, lambda: lib.hbx_simulate_phase(h, None, 1, f, r, st)),
        (inv, lambda: lib.hbx_simulate_phase(h, _ptr(x), 1, None, None, st)),
        (inv, lambda: lib.hbx_simulate_phase(h, _ptr(x), -1, f, r, st)),
        (inv, lambda: lib.hbx_evaluate_phase(h, None, _ptr(tgt), 1, f, i, s, p, st)),
        (inv, lambda: lib.hbx_evaluate_phase(h, _ptr(x), _ptr(tgt), 1, f, i, None, p, st)),   # target without chan_stats
        (inv, lambda: lib.hbx_evaluate_phase(h, _ptr(x), None, 1, f, i, s, None, st)),        # chan_stats without target
        (inv, lambda: lib.hbx_evaluate_phase(h, _ptr(x), None, 1, f, None, None, None, st)),  # no target: intensity needed
        (inv, lambda: lib.hbx_evaluate_phase(h, _ptr(x), None, 1, f, i, None, p, st)),        # no target: no psnr
        (inv, lambda: lib.hbx_evaluate_phase(h, _ptr(x), _ptr(tgt), -2, f, i, s, p, st)),
        (inv, lambda: lib.hbx_phase_backward(h, None, _ptr(tgt), 1.0, _ptr(x), 1, g, st)),
        (inv, lambda: lib.hbx_phase_backward(h, _ptr(v), _ptr(tgt), 1.0, None, 1, g, st)),
        (inv, lambda: lib.hbx_phase_backward(h, _ptr(v), _ptr(tgt), 1.0, _ptr(x), 1, None, st)),
        (inv, lambda: lib.hbx_phase_backward(h, _ptr(v), None, 1.0, _ptr(x), -1, g, st)),
    ]
    for k, (code, call) in enumerate(calls):
        assert call() == code, k
    # n_env == 0 is OK and does nothing
    assert lib.hbx_simulate_phase(h, _ptr(x), 0, f, r, st) == _lib.OK
    assert lib.hbx_evaluate_phase(h, _ptr(x), _ptr(tgt), 0, f, i, s, p, st) == _lib.OK
    assert lib.hbx_phase_backward(h, _ptr(v), None, 1.0, _ptr(x), 0, g, st) == _lib.OK
    plan.precision = _lib.PRECISION_BF16_STORE
    assert lib.hbx_simulate_phase(h, _ptr(x), 1, f, r, st) == uns
    assert lib.hbx_evaluate_phase(h, _ptr(x), _ptr(tgt), 1, f, i, s, p, st) == uns
    assert lib.hbx_phase_backward(h, _ptr(v), None, 1.0, _ptr(x), 1, g, st) == uns
    with pytest.raises(_lib.HbxError) as e:
        plan.simulate_phase(x)
    assert e.value.code == uns and "F32" in str(e.value)
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert bool((t == sentinel).all()), f"{k} was written by a refused call"
    plan.precision = _lib.PRECISION_F32
    # the same buffers, accepted: every output is written
    assert lib.hbx_evaluate_phase(h, _ptr(x), _ptr(tgt), 1, f, i, s, p, st) == _lib.OK
    assert lib.hbx_simulate_phase(h, _ptr(x), 1, None, r, st) == _lib.OK
    assert lib.hbx_phase_backward(h, _ptr(v), None, 1.0, _ptr(x), 1, g, st) == _lib.OK
    torch.cuda.synchronize()
    for k in ("field", "real", "inten", "grad"):
        assert not bool((outs[k] == sentinel).any()), k
    plan.close()


def test_plan_argument_checks():
    import hbx
    ocfg = O.OpticsConfig(64, 64, 1, 4, O.WL_MONO)
    plan = hbx.Plan(dev_cfg(ocfg), max_jobs=1)
    x = torch.zeros((1, 2, 64, 64), dtype=torch.float32, device="cuda")
    v = torch.zeros((1, 2, 64, 64), dtype=torch.complex64, device="cuda")
    plan.simulate_phase(x)
    for call in (lambda: plan.simulate_phase(x.double()), lambda: plan.simulate_phase(v),
                 lambda: plan.phase_backward(x, x), lambda: plan.phase_backward(v, v),
                 lambda: plan.evaluate_phase(x, x.double()[:, :1])):
        with pytest.raises(TypeError):
            call()
    for call in (lambda: plan.simulate_phase(x[:, :1]), lambda: plan.simulate_phase(x.cpu()),
                 lambda: plan.simulate_phase(x.transpose(2, 3)),
                 lambda: plan.simulate_phase(x, want_field=False, want_real=False),
                 lambda: plan.evaluate_phase(x, None, want_intensity=False),
                 lambda: plan.evaluate_phase(x, x), lambda: plan.phase_backward(v, x, weight=x),
                 lambda: plan.phase_backward(v[:, :1], x)):
        with pytest.raises(ValueError):
            call()
    plan.close()
