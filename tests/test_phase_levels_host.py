"""Quantized phase holograms (hbx_simulate_phase_levels / hbx_evaluate_phase_levels /
hbx_phase_levels_backward / hbx_quantize_phase) without a GPU: the numpy restatement of the quantizer
of include/hbx.h and its properties; the straight-through gradient, pi (Im g cos pi q - Re g sin pi q),
against central differences of the continuous float64 oracle loss taken at q; the header, the exports
and the ctypes declarations; hbx::check_pass_call on the calls the entry points build; and the shim's
argument errors before any GPU use."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.test_loss_host import LOSS_MSE, LOSS_PSNR, REL_LSQ, REL_NONE, loss_gradient, oracle_loss
from tests.test_phase_field_host import RGB, _sig, phase_gradient

HEADER = os.path.join(ROOT, "include", "hbx.h")
NAMES = ("hbx_simulate_phase_levels", "hbx_evaluate_phase_levels", "hbx_phase_levels_backward", "hbx_quantize_phase")
LEVELS = (2, 3, 4, 6, 16, 255, 256)
F32 = np.float32


def quantize_np(x, levels):
    """The quantizer of include/hbx.h restated in numpy, every operation float32 and round-half-to-even:
    x float32 -> (r, k, q float32, level uint8).  A non-finite x: q = NaN, level 0 (a select, no NaN cast)."""
    x = np.asarray(x, dtype=F32)
    with np.errstate(invalid="ignore"):
        r = x - F32(2) * np.rint(x * F32(.5))
        k = np.rint(r * F32(levels / 2))
        q = k * F32(2.0 / levels)
    assert r.dtype == k.dtype == q.dtype == F32
    ki = np.where(np.isnan(k), F32(0), k).astype(np.int32)
    level = np.where(ki < 0, ki + levels, ki).astype(np.uint8)
    return r, k, q, level


def planted(levels):
    """the ties (2 j + 1) / L (as float32 has them), +-0 and whole numbers, over a few turns"""
    j = np.arange(-3 * levels, 3 * levels)
    return np.concatenate([((2 * j + 1) / levels).astype(F32), np.array([0.0, -0.0], F32),
                           np.arange(-9, 10).astype(F32), np.array([4095, -4096, 2047, -2049], F32)])


def host_samples(levels, n=1 << 16, seed=0):
    rng = np.random.default_rng(3100 + levels + seed)
    return np.concatenate([((2 * rng.random(n) - 1) * 4096).astype(F32), planted(levels)])


# -- 1. the quantizer ----------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", LEVELS)
def test_numpy_restatement_of_the_quantizer(levels):
    x = host_samples(levels)
    r, k, q, level = quantize_np(x, levels)
    x64 = x.astype(np.float64)
    r64 = x64 - 2.0 * np.rint(x64 * 0.5)
    assert np.array_equal(r.astype(np.float64), r64), "the reduction to [-1, 1] is exact"
    assert np.all(np.abs(r) <= 1)
    assert level.dtype == np.uint8 and int(level.max()) < levels
    assert np.array_equal(level.astype(np.int64), np.mod(k.astype(np.int64), levels))
    d = q.astype(np.float64) - x64
    d -= 2.0 * np.rint(d * 0.5)
    worst = float(np.max(np.abs(d)))
    print(f"L={levels}: max |q - x| mod 2 = {worst:.9f}, 1 / L = {1 / levels:.9f}")
    assert worst <= 1.0 / levels + 2.0 ** -23
    # the displayed phase is the propagated one: exp(i pi q) against exp(2 pi i level / L)
    e = np.abs(np.exp(1j * np.pi * q.astype(np.float64)) - np.exp(2j * np.pi * level / levels))
    assert float(e.max()) <= 2.4e-7


def test_quantizer_ties_non_finite_samples_and_the_constants():
    # ties go to the even k, on both sides of zero (not threshold='s >= rule)
    _, k, q, level = quantize_np([0.25, 0.75, -0.25, -0.75, 1.25, 1.0, -1.0, 3.0], 4)
    assert k.tolist() == [0, 2, 0, -2, -2, 2, -2, -2]
    assert q.tolist() == [0, 1, 0, -1, -1, 1, -1, -1]
    assert level.tolist() == [0, 2, 0, 2, 2, 2, 2, 2]
    _, _, q, level = quantize_np([np.nan, np.inf, -np.inf], 16)
    assert np.all(np.isnan(q)) and level.tolist() == [0, 0, 0]
    # h = L / 2 is exact in float32 for every L, and s = float32(2.0 / L) is 1 / h correctly rounded
    for levels in range(2, 257):
        assert float(F32(levels / 2)) == levels / 2
        assert F32(2.0 / levels) == F32(1) / F32(levels / 2)


# -- 2. the straight-through gradient against central differences at q ---------------------------------
@pytest.mark.parametrize("levels", [4, 256])
@pytest.mark.parametrize("groups", [1, 3], ids=["mono", "rgb"])
@pytest.mark.parametrize("kind,rel", [(LOSS_MSE, REL_LSQ), (LOSS_PSNR, REL_NONE)], ids=["mse-lsq", "psnr-none"])
def test_straight_through_gradient_is_the_continuous_one_at_q(groups, kind, rel, levels):
    """dq/dx := 1: the gradient handed to x is dL/dq, the continuous chain rule at the displayed phase.
    N = 64, two phase planes per group, x in [-1, 1) quantized to q; central differences (step 1e-6) of the
    float64 oracle loss of exp(i pi q) along single samples against the formula applied to the oracle's
    dL/du at q; 5e-6 of max|dL/dq|, the machinery and the bound of tests/test_phase_field_host.py."""
    from oracle import hbx_oracle as O
    n, nq = 64, 2
    wls = RGB if groups == 3 else (515e-9,)
    cfg = O.OpticsConfig(n, n, groups, 2 * nq, wls)
    hs = [cfg.transfer(g) for g in range(groups)]
    rng = np.random.default_rng(3200 + 4 * groups + 2 * kind + rel + levels)
    x = (2 * rng.random((groups, nq, n, n)) - 1).astype(F32)
    q = quantize_np(x, levels)[2].astype(np.float64)
    assert len(np.unique(q)) <= levels + 1 and not np.array_equal(q, x.astype(np.float64))

    def loss_of(qs):
        return oracle_loss(np.exp(1j * np.pi * qs), target, hs, kind, rel)

    target = np.zeros((groups, n, n))
    _, _, i0 = oracle_loss(np.exp(1j * np.pi * q), target, hs, LOSS_MSE, REL_NONE)
    target = rng.random((groups, n, n)) * 2.0 * i0.mean()
    _, field, inten = loss_of(q)
    grad = phase_gradient(loss_gradient(field, inten, target, hs, kind, rel, False), q)
    gmax = np.max(np.abs(grad))
    assert gmax > 0.0
    eps, worst = 1e-6, 0.0
    for _ in range(12):
        idx = tuple(int(rng.integers(0, s)) for s in q.shape)
        up, dn = q.copy(), q.copy()
        up[idx] += eps
        dn[idx] -= eps
        fd = (loss_of(up)[0] - loss_of(dn)[0]) / (2 * eps)
        worst = max(worst, abs(fd - grad[idx]) / gmax)
    print(f"L={levels} G={groups} kind={kind} rel={rel}: worst |fd - dL/dq| / max|dL/dq| = {worst:.3e}")
    assert worst <= 5e-6


# -- 3. header, exports, ctypes ------------------------------------------------------------------------
def test_header_declares_the_four_entry_points_and_abi_stays_15():
    from hbx import _lib
    raw = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\bint\s+hbx_simulate_phase_levels" + _sig(
        "hbx_plan_t plan", "const float*phase", "int32_t levels", "int32_t n_env", "float*field", "float*real_part",
        "void*stream"), src)
    assert re.search(r"\bint\s+hbx_evaluate_phase_levels" + _sig(
        "hbx_plan_t plan", "const float*phase", "int32_t levels", "const float*target", "int32_t n_env", "float*field",
        "float*intensity", "double*chan_stats", "double*psnr", "void*stream"), src)
    assert re.search(r"\bint\s+hbx_phase_levels_backward" + _sig(
        "hbx_plan_t plan", "const float*values", "const float*weight", "float scale", "const float*phase",
        "int32_t levels", "int32_t n_env", "float*grad_phase", "void*stream"), src)
    assert re.search(r"\bint\s+hbx_quantize_phase" + _sig(
        "const float*src", "int64_t n_values", "int32_t levels", "uint8_t*out_levels", "float*out_phase",
        "void*stream"), src)
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS
    assert int(re.search(r"#define\s+HBX_ABI_VERSION\s+(\d+)", src).group(1)) == _lib.ABI_VERSION == 15
    # the header says how the ties differ from the threshold's rule
    assert re.search(r"Ties go to the even k\.\s+This is deliberately not hbx_evaluate_threshold's", raw)


def test_library_exports_and_lib_declares_the_four_entry_points():
    import ctypes as C
    from hbx import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in NAMES:
        assert name in syms, f"{name} not exported with C linkage"
    lib = _lib.load()
    assert lib.hbx_abi_version() == 15
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    assert lib.hbx_simulate_phase_levels.argtypes == [vp, vp, i32, i32, vp, vp, vp]
    assert lib.hbx_evaluate_phase_levels.argtypes == [vp, vp, i32, vp, i32, vp, vp, vp, vp, vp]
    assert lib.hbx_phase_levels_backward.argtypes == [vp, vp, vp, C.c_float, vp, i32, i32, vp, vp]
    assert lib.hbx_quantize_phase.argtypes == [vp, i64, i32, vp, vp, vp]
    calls = (lambda: lib.hbx_simulate_phase_levels(None, None, 4, 1, None, None, None),
             lambda: lib.hbx_evaluate_phase_levels(None, None, 4, None, 1, None, None, None, None, None),
             lambda: lib.hbx_phase_levels_backward(None, None, None, 1.0, None, 4, 1, None, None))
    for fn, call in zip(NAMES, calls):
        assert getattr(lib, fn).restype == C.c_int
        assert call() == _lib.ERR_INVALID
        assert b"null plan" in lib.hbx_last_error()
    # the plan-free export: every refusal comes before anything is enqueued, so none needs a GPU
    assert lib.hbx_quantize_phase.restype == C.c_int
    one = (C.c_float * 1)()
    lv = (C.c_uint8 * 1)()
    src, dst = C.cast(one, vp), C.cast(lv, vp)
    assert lib.hbx_quantize_phase(None, 1, 4, dst, None, None) == _lib.ERR_INVALID       # null src
    assert lib.hbx_quantize_phase(src, 1, 4, None, None, None) == _lib.ERR_INVALID       # no output
    assert lib.hbx_quantize_phase(src, -1, 4, dst, None, None) == _lib.ERR_INVALID
    for bad in (0, 1, 257, -4):
        assert lib.hbx_quantize_phase(src, 1, bad, dst, None, None) == _lib.ERR_INVALID
        assert b"levels" in lib.hbx_last_error()
    assert lib.hbx_quantize_phase(None, 0, 4, dst, None, None) == _lib.OK                # nothing to do


def test_pass_call_rules_for_phase_levels_calls_under_asan(tmp_path):
    """hbx::check_pass_call on every PassCall the three propagation entry points build (accepted) and one
    call per rule on the level count (rejected), the kinds and constants the dispatchers derive from it,
    and the quantizer's host instance: tests/c/pass_call_check_levels.hip, a stand-alone program with the
    host code under ASan + UBSan.  No GPU, no library."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not present")
    csrc = os.path.join(ROOT, "binary-hologram-reinforcement-learning_amd", "csrc")
    exe = str(tmp_path / "pass_call_check_levels")
    subprocess.run([hipcc, "-std=c++17", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined",
                    "-I", os.path.join(ROOT, "include"), "-I", csrc,
                    os.path.join(ROOT, "tests", "c", "pass_call_check_levels.hip"), "-o", exe], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stdout + r.stderr
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr


# -- 4. the shim's argument checks, before any GPU use -------------------------------------------------
META = {"dx": (7.56e-6, 7.56e-6), "wl": 515e-9}
BAD = {
    "complex": dict(levels=4, field="phase", x="complex"),
    "amplitude": dict(levels=4, field="amplitude"),
    "threshold": dict(levels=4, field="phase", threshold=0.5),
    "grid": dict(levels=4, field="phase", grid=256),
    "float": dict(levels=4.0, field="phase"),
    "str": dict(levels="4", field="phase"),
    "bool": dict(levels=True, field="phase"),
    "one": dict(levels=1, field="phase"),
    "zero": dict(levels=0, field="phase"),
    "257": dict(levels=257, field="phase"),
    "negative": dict(levels=-4, field="phase"),
}


def _shim_call(tt, torch, fn, kw):
    kw = dict(kw)
    dtype = torch.complex64 if kw.pop("x", None) == "complex" else torch.float32
    x = tt.Tensor(torch.zeros((1, 2, 64, 64), dtype=dtype), meta=META)
    if fn == "simulate":
        return tt.simulate(x, 2e-3, binary=kw.pop("binary", False), **kw)
    if fn == "intensity":
        return tt.intensity(x, 2e-3, **kw)
    return tt.loss(x, torch.zeros((1, 1, 64, 64)), 2e-3, **kw)


@pytest.fixture
def no_gpu(monkeypatch):
    torch = pytest.importorskip("torch")

    def fail():
        raise AssertionError("reached the GPU runtime")
    monkeypatch.setattr(torch.cuda, "is_available", fail)
    return torch


@pytest.mark.parametrize("fn", ["simulate", "intensity", "loss"])
@pytest.mark.parametrize("case", list(BAD))
def test_shim_refuses_bad_levels_before_any_gpu_use(fn, case, no_gpu):
    import torchOptics.optics as tt
    with pytest.raises(ValueError):
        _shim_call(tt, no_gpu, fn, BAD[case])


def test_shim_refuses_levels_on_the_binary_path(no_gpu):
    import torchOptics.optics as tt
    with pytest.raises(ValueError):
        _shim_call(tt, no_gpu, "simulate", dict(levels=4, field="phase", binary=True))
    with pytest.raises(ValueError):   # binary=True is simulate's default
        tt.simulate(tt.Tensor(no_gpu.zeros((1, 2, 64, 64)), meta=META), 2e-3, levels=4, field="phase")


@pytest.mark.parametrize("fn", ["simulate", "intensity", "loss"])
def test_shim_passes_a_well_formed_levels_call_on_to_the_gpu(fn, no_gpu):
    import torchOptics.optics as tt
    with pytest.raises(AssertionError, match="reached the GPU runtime"):
        _shim_call(tt, no_gpu, fn, dict(levels=4, field="phase"))
    with pytest.raises(AssertionError, match="reached the GPU runtime"):
        _shim_call(tt, no_gpu, fn, dict(levels=np.int64(256), field="phase"))
