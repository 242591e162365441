"""Quantized phase holograms through the C-ABI (hbx.quantize_phase, Plan.simulate_phase_levels /
evaluate_phase_levels / phase_levels_backward).

The first pass quantizes each float32 phase sample to the nearest of L levels as it loads it, the
backward's last pass does the same to the samples it differentiates at (the straight-through estimator),
and neither the quantized samples q nor exp(i pi q) is written.  The contract is bit for bit: every
output equals the continuous call's on the materialised q, which hbx.quantize_phase exports and which
tests/test_phase_levels_host.py restates in numpy.  Shapes are the phase tests' own CASES; the bounds
against the float64 oracle are theirs, imported."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import hbx_oracle as O  # noqa: E402
from tests.test_gpu_phase_field import ALL, CASES, FIELD_RTOL, MSE_RTOL, PSNR_ATOL, dev_cfg, ocfg_for  # noqa: E402
from tests.test_gpu_window import PAD, Guarded  # noqa: E402
from tests.test_phase_levels_host import LEVELS, host_samples, quantize_np  # noqa: E402

F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm GPU")
    import hbx
    hbx.load_library()
    yield


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def samples(shape, levels, seed, span=1.0):
    """float32 samples uniform in [-span, span) with every seventh one a tie (2 j + 1) / L"""
    rng = np.random.default_rng(seed)
    x = ((2 * rng.random(shape) - 1) * span).astype(F32)
    flat = x.reshape(-1)
    j = rng.integers(-levels, levels, size=flat[::7].shape)
    flat[::7] = ((2 * j + 1) / levels).astype(F32) + F32(2) * np.rint(flat[::7] * F32(.5))
    return x


def materialise(x, levels):
    """q of the device tensor x by hbx.quantize_phase -- checked against numpy in the first test"""
    import hbx
    return hbx.quantize_phase(x, levels, want_levels=False, want_samples=True)


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    if a.is_complex():
        a, b = torch.view_as_real(a), torch.view_as_real(b)
    return a.dtype == b.dtype and torch.equal(a, b)


# -- 1. the export against the numpy restatement -------------------------------------------------------
class GuardedBytes:
    """Guarded for uint8: the tensor in the middle of an allocation of 0xA5 bytes, itself filled with `fill`"""

    def __init__(self, n, fill):
        self.n = n
        self.big = torch.full((n + 2 * PAD,), 0xA5, dtype=torch.uint8, device="cuda")
        self.t = self.big[PAD:PAD + n]
        self.t.fill_(fill)

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr())

    def intact(self):
        return bool((self.big[:PAD] == 0xA5).all()) and bool((self.big[PAD + self.n:] == 0xA5).all())


@pytest.mark.parametrize("levels", LEVELS)
def test_quantize_phase_equals_the_numpy_restatement_bit_for_bit(levels):
    """Lengths 1, 63, 4097 and one 256 x 256 plane, each inside guarded allocations, levels alone, q alone
    and both.  Every output element is written: the level buffer is prefilled with 0 and with 255 and both
    runs give the expected bytes; q is prefilled with a value no q takes.  NaN and +-inf: level 0, q NaN."""
    from hbx import _lib
    lib = _lib.load()
    special = np.array([1.25, np.nan, np.inf, -np.inf, -0.0], F32)
    pool = np.concatenate([special, host_samples(levels)[::-1]])
    for n in (1, 63, 4097, 256 * 256):
        x = pool[:n]
        _, _, q_want, lv_want = quantize_np(x, levels)
        finite = np.isfinite(x)
        assert np.all(np.isnan(q_want[~finite])) and np.all(lv_want[~finite] == 0)
        gx = Guarded((n,), data=x)
        for fill in (0, 255):
            for want_lv, want_q in ((True, True), (True, False), (False, True)):
                glv = GuardedBytes(n, fill) if want_lv else None
                gq = Guarded((n,), data=np.full(n, 12345.0, F32)) if want_q else None
                rc = lib.hbx_quantize_phase(gx.ptr, n, levels, glv.ptr if glv else None, gq.ptr if gq else None,
                                            _stream())
                torch.cuda.synchronize()
                assert rc == _lib.OK, lib.hbx_last_error()
                assert gx.intact() and torch.equal(gx.t.cpu().view(torch.int32),
                                                   torch.from_numpy(x.copy()).view(torch.int32))
                if glv:
                    assert glv.intact()
                    assert np.array_equal(glv.t.cpu().numpy(), lv_want), (levels, n, fill)
                if gq:
                    assert gq.intact()
                    q = gq.t.cpu().numpy()
                    assert np.array_equal(np.isnan(q), ~finite)
                    assert np.array_equal(q[finite].view(np.uint32), q_want[finite].view(np.uint32)), (levels, n)


def test_quantize_phase_python_surface():
    import hbx
    x_np = samples((3, 5, 17), 6, 3300, span=40.0)
    x = torch.from_numpy(x_np).cuda()
    _, _, q_want, lv_want = quantize_np(x_np, 6)
    lv = hbx.quantize_phase(x, 6)
    q = hbx.quantize_phase(x, 6, want_levels=False, want_samples=True)
    lv2, q2 = hbx.quantize_phase(x, 6, want_levels=True, want_samples=True)
    torch.cuda.synchronize()
    assert lv.dtype == torch.uint8 and q.dtype == torch.float32 and lv.shape == x.shape == q.shape
    assert np.array_equal(lv.cpu().numpy(), lv_want) and np.array_equal(q.cpu().numpy(), q_want)
    assert torch.equal(lv2, lv) and torch.equal(q2, q)
    view = x.transpose(1, 2)                           # a non-contiguous view: the result has the view's shape
    assert np.array_equal(hbx.quantize_phase(view, 6).cpu().numpy(), lv_want.transpose(0, 2, 1))
    assert hbx.quantize_phase(x[:0], 6).numel() == 0
    with pytest.raises(ValueError):
        hbx.quantize_phase(x, 6, want_levels=False, want_samples=False)
    with pytest.raises(ValueError):
        hbx.quantize_phase(x.cpu(), 6)
    with pytest.raises(TypeError):
        hbx.quantize_phase(x.double(), 6)
    with pytest.raises(TypeError):
        hbx.quantize_phase(x, 6.0)
    for bad in (0, 1, 257, -4):
        with pytest.raises(hbx.HbxError, match="levels"):
            hbx.quantize_phase(x, bad)
    torch.cuda.synchronize()


# -- 2. forward: the levels calls equal the continuous calls on q --------------------------------------
FORWARD = [(name, 4, 1.0) for name in ALL] + [(name, lv, 1.0) for name in ("64", "256q3") for lv in (2, 3, 256)] + \
          [("64", lv, 4096.0) for lv in (4, 3)]


@pytest.mark.parametrize("name,levels,span", FORWARD, ids=[f"{n}-L{lv}-span{int(s)}" for n, lv, s in FORWARD])
def test_forward_equals_the_continuous_calls_on_q(name, levels, span):
    import hbx
    n, g, nq = CASES[name]
    ocfg = ocfg_for(name)
    x = torch.from_numpy(samples((1, g * nq, n, n), levels, 3400 + n + nq + levels, span)).cuda()
    target = torch.from_numpy(np.random.default_rng(3401 + n).random((1, g, n, n), dtype=F32)).cuda()
    q = materialise(x, levels)
    assert not torch.equal(q, x)
    plan = hbx.Plan(dev_cfg(ocfg), max_jobs=g)
    pairs = [
        (plan.simulate_phase_levels(x, levels, want_field=True, want_real=True),
         plan.simulate_phase(q, want_field=True, want_real=True)),
        (plan.simulate_phase_levels(x, levels), plan.simulate_phase(q)),
        (plan.simulate_phase_levels(x, levels, want_field=False, want_real=True),
         plan.simulate_phase(q, want_field=False, want_real=True)),
        (plan.evaluate_phase_levels(x, levels, target), plan.evaluate_phase(q, target)),
        (plan.evaluate_phase_levels(x, levels, target, want_field=False),                      # no field
         plan.evaluate_phase(q, target, want_field=False)),
        (plan.evaluate_phase_levels(x, levels, target, want_field=False, want_intensity=False),  # statistics alone
         plan.evaluate_phase(q, target, want_field=False, want_intensity=False)),
        (plan.evaluate_phase_levels(x, levels, None, want_field=False),                       # intensity alone
         plan.evaluate_phase(q, None, want_field=False)),
    ]
    torch.cuda.synchronize()
    for k, (got, want) in enumerate(pairs):
        assert len(got) == len(want)
        for i, (a, b) in enumerate(zip(got, want)):
            assert same_bits(a, b), (name, levels, k, i)
    assert pairs[0][0][0] is not None and pairs[3][0][2] is not None and pairs[3][0][3] is not None
    assert bool(torch.isfinite(pairs[3][0][1]).all())
    plan.close()


# -- 3. it quantizes -----------------------------------------------------------------------------------
def test_it_actually_quantizes():
    """Whole planes of x = 0.2, -0.2 and 1.8 at L = 4 are the level-0 plane: the field of a plane of x = 0.
    On random x the result differs from the continuous call's."""
    import hbx
    ocfg = O.OpticsConfig(64, 64, 1, 8, O.WL_MONO)
    xs = np.array([0.0, 0.2, -0.2, 1.8], F32)
    x = torch.from_numpy(np.broadcast_to(xs[None, :, None, None], (1, 4, 64, 64)).copy()).cuda()
    plan = hbx.Plan(dev_cfg(ocfg), max_jobs=1)
    field, _ = plan.simulate_phase_levels(x, 4)
    zero, _ = plan.simulate_phase(torch.zeros_like(x))
    cont, _ = plan.simulate_phase(x)
    r = torch.from_numpy(samples((1, 4, 64, 64), 4, 3500)).cuda()
    fr, _ = plan.simulate_phase_levels(r, 4)
    cr, _ = plan.simulate_phase(r)
    torch.cuda.synchronize()
    assert bool((field.abs() > 0).any())
    for p in range(4):
        assert same_bits(field[0, p], zero[0, 0]), f"x = {xs[p]}"
    assert not same_bits(cont[0, 1], zero[0, 0])
    assert not same_bits(fr, cr)
    plan.close()


# -- 4. against the float64 oracle of the displayed levels ---------------------------------------------
@pytest.mark.parametrize("levels", [4, 256])
@pytest.mark.parametrize("name", ["64", "256q2"])
def test_levels_calls_vs_the_oracle_of_the_exported_levels(name, levels):
    """reference: O.propagate(exp(2 pi i level / L), H) with the levels hbx.quantize_phase exports"""
    import hbx
    from hbx import _lib
    n, g, nq = CASES[name]
    ocfg = ocfg_for(name)
    x = torch.from_numpy(samples((1, g * nq, n, n), levels, 3600 + n + levels)).cuda()
    t_np = np.random.default_rng(3601 + n).random((1, g, n, n), dtype=F32)
    target = torch.from_numpy(t_np).cuda()
    lv = hbx.quantize_phase(x, levels).cpu().numpy().astype(np.float64)
    u = np.exp(2j * np.pi * lv[0] / levels)
    want = np.concatenate([O.propagate(u[k * nq:(k + 1) * nq], ocfg.transfer(k)) for k in range(g)])
    want_i = np.mean(np.abs(want.reshape(g, nq, n, n)) ** 2, axis=1)
    t64 = t_np[0].astype(np.float64)
    plan = hbx.Plan(dev_cfg(ocfg), max_jobs=g)
    field, inten, stats, psnr = plan.evaluate_phase_levels(x, levels, target)
    mse = plan.loss(stats, _lib.LOSS_MSE, _lib.REL_LSQ)
    torch.cuda.synchronize()
    e_f = float(np.max(np.abs(field[0].cpu().numpy() - want)) / np.max(np.abs(want)))
    e_i = float(np.max(np.abs(inten[0].cpu().numpy().astype(np.float64) - want_i)) / np.max(want_i))
    w_mse, w_psnr = O.relative_mse(want_i, t64, O.REL_LSQ), O.relative_psnr(want_i, t64, O.REL_LSQ)
    e_mse, e_psnr = abs(float(mse[0]) - w_mse) / w_mse, abs(float(psnr[0]) - w_psnr)
    print(f"{name} L={levels}: field {e_f:.3e} of max|field|, intensity {e_i:.3e} of max I, "
          f"MSE rel {e_mse:.3e}, PSNR {e_psnr:.3e} dB")
    assert e_f <= FIELD_RTOL
    assert e_i <= FIELD_RTOL
    assert e_mse <= MSE_RTOL
    assert e_psnr <= PSNR_ATOL
    plan.close()


# -- 5. backward ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("name", ALL)
def test_backward_equals_phase_backward_on_q(name, weighted):
    import hbx
    n, g, nq = CASES[name]
    ocfg = ocfg_for(name)
    levels = 4
    rng = np.random.default_rng(3700 + n + nq)
    shape = (1, g * nq, n, n)
    x = torch.from_numpy(samples(shape, levels, 3701 + n + nq)).cuda()
    v = torch.from_numpy(((2 * rng.random(shape, dtype=F32) - 1) +
                          1j * (2 * rng.random(shape, dtype=F32) - 1)).astype(np.complex64)).cuda()
    w = torch.from_numpy(rng.random((1, g, n, n), dtype=F32)).cuda() if weighted else None
    q = materialise(x, levels)
    plan = hbx.Plan(dev_cfg(ocfg, z=-ocfg.z), max_jobs=g)
    got = plan.phase_levels_backward(v, x, levels, weight=w, scale=2.0 / nq)
    want = plan.phase_backward(v, q, weight=w, scale=2.0 / nq)
    cont = plan.phase_backward(v, x, weight=w, scale=2.0 / nq)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and tuple(got.shape) == shape
    assert bool((got != 0).any()) and bool(torch.isfinite(got).all())
    assert same_bits(got, want)
    assert not same_bits(got, cont)
    plan.close()


@pytest.mark.parametrize("levels", [2, 3, 256])
def test_backward_at_other_level_counts(levels):
    import hbx
    n, g, nq = CASES["256q3"]
    ocfg = ocfg_for("256q3")
    rng = np.random.default_rng(3800 + levels)
    shape = (1, g * nq, n, n)
    x = torch.from_numpy(samples(shape, levels, 3801 + levels, span=64.0)).cuda()
    v = torch.from_numpy((rng.random(shape, dtype=F32) - 1j * rng.random(shape, dtype=F32)).astype(np.complex64)).cuda()
    plan = hbx.Plan(dev_cfg(ocfg, z=-ocfg.z), max_jobs=g)
    got = plan.phase_levels_backward(v, x, levels)
    want = plan.phase_backward(v, materialise(x, levels))
    torch.cuda.synchronize()
    assert same_bits(got, want)
    plan.close()


# -- 6. chunking ---------------------------------------------------------------------------------------
def test_chunking_by_max_jobs():
    """n_env = 3 on a plan of one env per chunk (max_jobs = G) against a plan that takes all three at once"""
    import hbx
    ocfg = ocfg_for("64")
    n, g, nq = CASES["64"]
    rng = np.random.default_rng(3900)
    shape = (3, g * nq, n, n)
    x = torch.from_numpy(samples(shape, 4, 3901)).cuda()
    v = torch.from_numpy(((2 * rng.random(shape, dtype=F32) - 1) + 1j * rng.random(shape, dtype=F32))
                         .astype(np.complex64)).cuda()
    target = torch.from_numpy(rng.random((3, g, n, n), dtype=F32)).cuda()
    out = []
    for jobs in (g, 3 * g):
        plan = hbx.Plan(dev_cfg(ocfg), max_jobs=jobs)
        field, real = plan.simulate_phase_levels(x, 4, want_field=True, want_real=True)
        f_ev, inten, stats, psnr = plan.evaluate_phase_levels(x, 4, target)
        grad = plan.phase_levels_backward(v, x, 4, weight=target, scale=1.0)
        grad_plain = plan.phase_levels_backward(v, x, 4)
        torch.cuda.synchronize()
        out.append([field, real, f_ev, inten, stats, psnr, grad, grad_plain])
        plan.close()
    for a, b in zip(*out):
        assert same_bits(a, b)
    assert not torch.equal(out[0][6][2], out[0][6][0])      # the envs differ
    # and each env is the single-env call's on q
    plan = hbx.Plan(dev_cfg(ocfg), max_jobs=g)
    one, _ = plan.simulate_phase(materialise(x[2:3].contiguous(), 4))
    torch.cuda.synchronize()
    assert same_bits(out[0][0][2:3], one)
    plan.close()


# -- 7. error paths ------------------------------------------------------------------------------------
def test_error_paths_return_the_header_codes_and_enqueue_nothing():
    import hbx
    from hbx import _lib
    from hbx.plan import _ptr
    ocfg = O.OpticsConfig(64, 64, 1, 2, O.WL_MONO)
    plan = hbx.Plan(dev_cfg(ocfg), max_jobs=1)
    lib, h, st = plan.lib, plan._h, _stream()
    x = torch.zeros((1, 1, 64, 64), dtype=torch.float32, device="cuda")
    v = torch.ones((1, 1, 64, 64), dtype=torch.complex64, device="cuda")
    tgt = torch.zeros((1, 1, 64, 64), dtype=torch.float32, device="cuda")
    sentinel = 7.0
    outs = {k: torch.full(s, sentinel, dtype=d, device="cuda") for k, (s, d) in {
        "field": ((1, 1, 64, 64, 2), torch.float32), "real": ((1, 1, 64, 64), torch.float32),
        "inten": ((1, 1, 64, 64), torch.float32), "stats": ((1, 1, 3), torch.float64), "psnr": ((1,), torch.float64),
        "grad": ((1, 1, 64, 64), torch.float32), "q": ((1, 1, 64, 64), torch.float32)}.items()}
    lvl = torch.full((1, 1, 64, 64), 7, dtype=torch.uint8, device="cuda")
    f, r, i, s, p, g, q = (_ptr(outs[k]) for k in ("field", "real", "inten", "stats", "psnr", "grad", "q"))
    inv, uns = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
    nv = x.numel()
    for bad in (0, 1, 257, -4):
        for call in (lambda: lib.hbx_simulate_phase_levels(h, _ptr(x), bad, 1, f, r, st),
                     lambda: lib.hbx_evaluate_phase_levels(h, _ptr(x), bad, _ptr(tgt), 1, f, i, s, p, st),
                     lambda: lib.hbx_phase_levels_backward(h, _ptr(v), _ptr(tgt), 1.0, _ptr(x), bad, 1, g, st),
                     lambda: lib.hbx_phase_levels_backward(h, _ptr(v), None, 1.0, _ptr(x), bad, 1, g, st),
                     lambda: lib.hbx_quantize_phase(_ptr(x), nv, bad, _ptr(lvl), q, st)):
            assert call() == inv, bad
            assert b"levels" in lib.hbx_last_error(), bad
    calls = [
        (inv, lambda: lib.hbx_simulate_phase_levels(h, None, 4, 1, f, r, st)),
        (inv, lambda: lib.hbx_simulate_phase_levels(h, _ptr(x), 4, 1, None, None, st)),
        (inv, lambda: lib.hbx_simulate_phase_levels(h, _ptr(x), 4, -1, f, r, st)),
        (inv, lambda: lib.hbx_evaluate_phase_levels(h, None, 4, _ptr(tgt), 1, f, i, s, p, st)),
        (inv, lambda: lib.hbx_evaluate_phase_levels(h, _ptr(x), 4, _ptr(tgt), 1, f, i, None, p, st)),
        (inv, lambda: lib.hbx_evaluate_phase_levels(h, _ptr(x), 4, None, 1, f, i, s, None, st)),
        (inv, lambda: lib.hbx_evaluate_phase_levels(h, _ptr(x), 4, None, 1, f, None, None, None, st)),
        (inv, lambda: lib.hbx_evaluate_phase_levels(h, _ptr(x), 4, None, 1, f, i, None, p, st)),
        (inv, lambda: lib.hbx_phase_levels_backward(h, None, _ptr(tgt), 1.0, _ptr(x), 4, 1, g, st)),
        (inv, lambda: lib.hbx_phase_levels_backward(h, _ptr(v), _ptr(tgt), 1.0, None, 4, 1, g, st)),
        (inv, lambda: lib.hbx_phase_levels_backward(h, _ptr(v), _ptr(tgt), 1.0, _ptr(x), 4, 1, None, st)),
        (inv, lambda: lib.hbx_phase_levels_backward(h, _ptr(v), None, 1.0, _ptr(x), 4, -1, g, st)),
        (inv, lambda: lib.hbx_quantize_phase(_ptr(x), nv, 4, None, None, st)),     # both outputs null
        (inv, lambda: lib.hbx_quantize_phase(None, nv, 4, _ptr(lvl), q, st)),
        (inv, lambda: lib.hbx_quantize_phase(_ptr(x), -1, 4, _ptr(lvl), q, st)),
    ]
    for k, (code, call) in enumerate(calls):
        assert call() == code, k
    # an empty batch is OK and does nothing
    assert lib.hbx_simulate_phase_levels(h, _ptr(x), 4, 0, f, r, st) == _lib.OK
    assert lib.hbx_evaluate_phase_levels(h, _ptr(x), 4, _ptr(tgt), 0, f, i, s, p, st) == _lib.OK
    assert lib.hbx_phase_levels_backward(h, _ptr(v), None, 1.0, _ptr(x), 4, 0, g, st) == _lib.OK
    assert lib.hbx_quantize_phase(_ptr(x), 0, 4, _ptr(lvl), q, st) == _lib.OK
    plan.precision = _lib.PRECISION_BF16_STORE
    assert lib.hbx_simulate_phase_levels(h, _ptr(x), 4, 1, f, r, st) == uns
    assert lib.hbx_evaluate_phase_levels(h, _ptr(x), 4, _ptr(tgt), 1, f, i, s, p, st) == uns
    assert lib.hbx_phase_levels_backward(h, _ptr(v), None, 1.0, _ptr(x), 4, 1, g, st) == uns
    with pytest.raises(_lib.HbxError) as e:
        plan.simulate_phase_levels(x, 4)
    assert e.value.code == uns and "F32" in str(e.value)
    with pytest.raises(_lib.HbxError) as e:
        plan.simulate_phase_levels(x, 257)
    assert e.value.code == inv and "levels" in str(e.value)
    torch.cuda.synchronize()                                 # clean: nothing was enqueued, nothing faulted
    for k, t in outs.items():
        assert bool((t == sentinel).all()), f"{k} was written by a refused call"
    assert bool((lvl == 7).all())
    plan.precision = _lib.PRECISION_F32
    # the same buffers, accepted: every output is written
    assert lib.hbx_evaluate_phase_levels(h, _ptr(x), 4, _ptr(tgt), 1, f, i, s, p, st) == _lib.OK
    assert lib.hbx_simulate_phase_levels(h, _ptr(x), 4, 1, None, r, st) == _lib.OK
    assert lib.hbx_phase_levels_backward(h, _ptr(v), None, 1.0, _ptr(x), 4, 1, g, st) == _lib.OK
    assert lib.hbx_quantize_phase(_ptr(x), nv, 4, _ptr(lvl), q, st) == _lib.OK
    torch.cuda.synchronize()
    for k in ("field", "real", "inten", "grad", "q"):
        assert not bool((outs[k] == sentinel).any()), k
    assert bool((lvl == 0).all())
    plan.close()


def test_plan_argument_checks():
    import hbx
    ocfg = O.OpticsConfig(64, 64, 1, 4, O.WL_MONO)
    plan = hbx.Plan(dev_cfg(ocfg), max_jobs=1)
    x = torch.zeros((1, 2, 64, 64), dtype=torch.float32, device="cuda")
    v = torch.zeros((1, 2, 64, 64), dtype=torch.complex64, device="cuda")
    plan.simulate_phase_levels(x, 4)
    for call in (lambda: plan.simulate_phase_levels(x.double(), 4), lambda: plan.simulate_phase_levels(v, 4),
                 lambda: plan.simulate_phase_levels(x, 4.0), lambda: plan.evaluate_phase_levels(x, "4"),
                 lambda: plan.phase_levels_backward(v, x, True),
                 lambda: plan.phase_levels_backward(x, x, 4), lambda: plan.phase_levels_backward(v, v, 4),
                 lambda: plan.evaluate_phase_levels(x, 4, x.double()[:, :1])):
        with pytest.raises(TypeError):
            call()
    for call in (lambda: plan.simulate_phase_levels(x[:, :1], 4), lambda: plan.simulate_phase_levels(x.cpu(), 4),
                 lambda: plan.simulate_phase_levels(x.transpose(2, 3), 4),
                 lambda: plan.simulate_phase_levels(x, 4, want_field=False, want_real=False),
                 lambda: plan.evaluate_phase_levels(x, 4, None, want_intensity=False),
                 lambda: plan.evaluate_phase_levels(x, 4, x), lambda: plan.phase_levels_backward(v, x, 4, weight=x),
                 lambda: plan.phase_levels_backward(v[:, :1], x, 4)):
        with pytest.raises(ValueError):
            call()
    torch.cuda.synchronize()
    plan.close()
