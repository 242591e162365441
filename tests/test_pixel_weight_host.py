"""Per-pixel loss weights without a GPU (hbx_evaluate_pw, hbx_evaluate_stack_pw, hbx_pixel_weight_sum,
hbx_loss_pw, hbx_loss_weight_pw; tt.loss / tt.loss_stack with pixel_weight=): the header, the exports and the
ctypes prototypes, check_pass_call's rules for the weight (a stand-alone program under ASan + UBSan), the
shim's argument checks, which raise before any GPU use, and the weighted loss and its gradient (stated here
in numpy from oracle.propagate / oracle.transfer_function; the GPU tests import them) against central
differences of the float64 loss."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.test_loss_host import LOSS_MSE, LOSS_PSNR, REL_LSQ, REL_NONE

HEADER = os.path.join(ROOT, "include", "hbx.h")
NAMES = ("hbx_evaluate_pw", "hbx_evaluate_stack_pw", "hbx_pixel_weight_sum", "hbx_loss_pw", "hbx_loss_weight_pw")
METHODS = ("evaluate_pw", "evaluate_stack_pw", "pixel_weight_sum", "loss_pw", "loss_weight_pw")
META = {"dx": (7.56e-6, 7.56e-6), "wl": 515e-9}
RGB = (638e-9, 515e-9, 450e-9)


def _sig(*params):
    return r"\s*\(\s*" + r"\s*,\s*".join(re.escape(p).replace(r"\ ", r"\s+").replace(r"\*", r"\s*\*\s*")
                                          for p in params) + r"\s*\)"


# -- the weighted formulas of include/hbx.h, float64 ---------------------------------------------------
def pw_sums(intens, targets, v):
    """(S_xy, S_xx, S_yy, W) of one env: intens, targets, v of one shape ([G, n, n] or [D, G, n, n])"""
    i, t, v = (np.asarray(a, np.float64) for a in (intens, targets, v))
    return float((v * i * t).sum()), float((v * i * i).sum()), float((v * t * t).sum()), float(v.sum())


def pw_loss_from_sums(sxy, sxx, syy, w, kind, rel, peak=1.0):
    """hbx_loss's formulas with the pixel count replaced by W; W = 0: MSE 0, PSNR +inf"""
    if w == 0.0:
        return 0.0 if kind == LOSS_MSE else math.inf
    if rel == REL_LSQ:
        mse = (syy - sxy * sxy / sxx) / w if sxx > 0.0 else syy / w
    else:
        mse = (sxx - 2.0 * sxy + syy) / w
    if kind == LOSS_MSE:
        return mse
    return 10.0 * math.log10(peak * peak / mse) if mse > 0.0 else math.inf


def pw_coeffs(sxy, sxx, syy, w, kind, rel, up=1.0):
    """(a, c) with d loss / d I = v (a I + c T): hbx_loss_weight's formulas (tests/test_loss_host.loss_coeffs)
    with W for the pixel count; a degenerate env -- W = 0 included -- gets (0, 0)"""
    if w == 0.0:
        return 0.0, 0.0
    if rel == REL_LSQ:
        if sxx > 0.0:
            s = sxy / sxx
            a, c, mse = 2.0 * s * s / w, -2.0 * s / w, (syy - sxy * sxy / sxx) / w
        else:
            a, c, mse = 0.0, 0.0, syy / w
    else:
        a, c, mse = 2.0 / w, -2.0 / w, (sxx - 2.0 * sxy + syy) / w
    if kind == LOSS_PSNR:
        f = -(10.0 / math.log(10.0)) / mse if mse > 0.0 else 0.0
        a, c = a * f, c * f
    return a * up, c * up


def pw_forward(u, hs_by_depth):
    """(fields [D][G, Pc, n, n] complex128, intensities [D, G, n, n]) of one env's samples u [G, Pc, n, n]"""
    from oracle import hbx_oracle as O
    fields = [np.stack([O.propagate(u[g], hs[g]) for g in range(u.shape[0])]) for hs in hs_by_depth]
    intens = np.stack([np.mean(f.real ** 2 + f.imag ** 2, axis=1) for f in fields])
    return fields, intens


def pw_loss(u, targets, v, hs_by_depth, kind, rel):
    """the weighted loss of one env, float64: u [G, Pc, n, n], targets and v [D, G, n, n] (D = 1: one depth)"""
    _, intens = pw_forward(u, hs_by_depth)
    return pw_loss_from_sums(*pw_sums(intens, targets, v), kind, rel)


def pw_gradient(u, targets, v, hs_by_depth, kind, rel, real_input, up=1.0):
    """d loss / d u of one env, float64: sum over d of A(-z_d)[(2 / Pc) v_d (a I_d + c T_d) F_d], one (a, c)"""
    from oracle import hbx_oracle as O
    g_, pc = u.shape[:2]
    fields, intens = pw_forward(u, hs_by_depth)
    a, c = pw_coeffs(*pw_sums(intens, targets, v), kind, rel, up)
    out = np.zeros(u.shape, np.complex128)
    for d, hs in enumerate(hs_by_depth):
        w = v[d] * (a * intens[d] + c * targets[d])
        out += np.stack([O.propagate((2.0 / pc) * w[g] * fields[d][g], np.conj(hs[g])) for g in range(g_)])
    return out.real if real_input else out


def random_weight(rng, shape):
    """uniform in [0, 1) with a quarter of the pixels exactly 0, float32"""
    v = rng.random(shape, dtype=np.float32)
    v[rng.random(shape) < 0.25] = 0.0
    return v


# -- 1. header, exports, ctypes, Plan methods ----------------------------------------------------------
def test_header_declares_the_pw_entry_points_and_abi_stays_15():
    from hbx import _lib
    raw = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    ev = ("hbx_plan_t plan", "const void*values", "const hbx_leaf_t*leaf", "const float*target",
          "const float*pixel_weight", "int32_t n_env", "float*field", "float*intensity", "double*chan_stats",
          "void*stream")
    assert re.search(r"\bint\s+hbx_evaluate_pw" + _sig(*ev), src)
    assert re.search(r"\bint\s+hbx_evaluate_stack_pw" + _sig(*ev), src)
    assert re.search(r"\bint\s+hbx_pixel_weight_sum" + _sig(
        "hbx_plan_t plan", "const float*pixel_weight", "int32_t n_env", "int32_t n_depths", "double*weight_sum",
        "void*stream"), src)
    assert re.search(r"\bint\s+hbx_loss_pw" + _sig(
        "hbx_plan_t plan", "const double*chan_stats", "const double*weight_sum", "int32_t n_env", "int32_t n_depths",
        "int32_t kind", "int32_t rel_scale", "double*loss", "void*stream"), src)
    assert re.search(r"\bint\s+hbx_loss_weight_pw" + _sig(
        "hbx_plan_t plan", "const float*intensity", "const float*target", "const float*pixel_weight",
        "const double*chan_stats", "const double*weight_sum", "const double*grad_loss", "int32_t n_env",
        "int32_t n_depths", "int32_t kind", "int32_t rel_scale", "float*weight", "void*stream"), src)
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS
    assert int(re.search(r"#define\s+HBX_ABI_VERSION\s+(\d+)", src).group(1)) == _lib.ABI_VERSION == 15
    # the header defines the terms and says what is out of scope
    assert "sxy = fma(vI, T, sxy)" in raw and "windows together with weights" in raw
    assert "a differentiable weight" in raw


def test_library_exports_and_lib_declares_the_pw_entry_points():
    import ctypes as C
    from hbx import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in NAMES:
        assert name in syms, f"{name} not exported with C linkage"
    lib = _lib.load()
    assert lib.hbx_abi_version() == 15
    vp, i32, lp = C.c_void_p, C.c_int32, C.POINTER(_lib.Leaf)
    assert lib.hbx_evaluate_pw.argtypes == [vp, vp, lp, vp, vp, i32, vp, vp, vp, vp]
    assert lib.hbx_evaluate_stack_pw.argtypes == [vp, vp, lp, vp, vp, i32, vp, vp, vp, vp]
    assert lib.hbx_pixel_weight_sum.argtypes == [vp, vp, i32, i32, vp, vp]
    assert lib.hbx_loss_pw.argtypes == [vp, vp, vp, i32, i32, i32, i32, vp, vp]
    assert lib.hbx_loss_weight_pw.argtypes == [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp]
    leaf = _lib.Leaf(_lib.LEAF_COMPLEX, 0, 0.0, 0, 0.0, 0.0)
    calls = (lambda: lib.hbx_evaluate_pw(None, None, C.byref(leaf), None, None, 1, None, None, None, None),
             lambda: lib.hbx_evaluate_stack_pw(None, None, C.byref(leaf), None, None, 1, None, None, None, None),
             lambda: lib.hbx_pixel_weight_sum(None, None, 1, 0, None, None),
             lambda: lib.hbx_loss_pw(None, None, None, 1, 0, LOSS_MSE, REL_LSQ, None, None),
             lambda: lib.hbx_loss_weight_pw(None, None, None, None, None, None, None, 1, 0, LOSS_MSE, REL_LSQ, None,
                                            None))
    for name, call in zip(NAMES, calls):
        assert getattr(lib, name).restype == C.c_int
        assert call() == _lib.ERR_INVALID
        assert b"null plan" in lib.hbx_last_error()


def test_plan_has_the_pw_methods_and_the_existing_signatures_stand():
    import inspect
    import hbx
    for m in METHODS:
        assert callable(getattr(hbx.Plan, m))
    assert list(inspect.signature(hbx.Plan.evaluate_pw).parameters)[:5] == ["self", "values", "kind", "target",
                                                                            "pixel_weight"]
    assert list(inspect.signature(hbx.Plan.loss_pw).parameters)[:3] == ["self", "chan_stats", "weight_sum"]
    assert "pixel_weight" not in inspect.signature(hbx.Plan.evaluate_stack).parameters
    assert "weight_sum" not in inspect.signature(hbx.Plan.loss).parameters
    import torchOptics.optics as tt
    assert inspect.signature(tt.loss).parameters["pixel_weight"].default is None
    assert inspect.signature(tt.loss_stack).parameters["pixel_weight"].default is None


# -- 2. check_pass_call's rules for the weight -----------------------------------------------------------
def test_pass_call_rules_for_the_pixel_weight_under_asan(tmp_path):
    """hbx::check_pass_call on the calls hbx_evaluate_pw and hbx_evaluate_stack_pw build for every leaf kind and
    size (accepted) and one call per refusal: tests/c/pass_call_check_pw.hip, a stand-alone program with the
    host code under ASan + UBSan.  No GPU, no library."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not present")
    csrc = os.path.join(ROOT, "binary-hologram-reinforcement-learning_amd", "csrc")
    exe = str(tmp_path / "pass_call_check_pw")
    subprocess.run([hipcc, "-std=c++17", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined",
                    "-I", os.path.join(ROOT, "include"), "-I", csrc,
                    os.path.join(ROOT, "tests", "c", "pass_call_check_pw.hip"), "-o", exe], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stdout + r.stderr
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr


# -- 3. the shim's argument checks, before any GPU use ------------------------------------------------------
@pytest.fixture
def no_gpu(monkeypatch):
    torch = pytest.importorskip("torch")

    def fail():
        raise AssertionError("reached the GPU runtime")
    monkeypatch.setattr(torch.cuda, "is_available", fail)
    return torch


def _loss_call(tt, torch, pw, kw=None, shape=(2, 2, 64, 64), stack=False, squeeze=False, groups=1):
    kw = dict(kw or {})
    wl = RGB[:groups] if groups > 1 else 515e-9
    x = torch.zeros(shape[1:] if squeeze else shape)
    hw = (64, 64) if "grid" not in kw and "roi" not in kw else kw.get("roi", (0, 0, 64, 64))[2:]
    tshape = ((shape[0],) if not squeeze else ()) + (groups,) + tuple(hw)
    if stack:
        return tt.loss_stack(tt.Tensor(x, meta=dict(META, wl=wl)), torch.zeros((2,) + tshape), [1e-3, 2e-3],
                             pixel_weight=pw, **kw)
    return tt.loss(tt.Tensor(x, meta=dict(META, wl=wl)), torch.zeros(tshape), 2e-3, pixel_weight=pw, **kw)


@pytest.mark.parametrize("kw", [dict(grid=256), dict(roi=(0, 0, 32, 32), grid=64), dict(origin=(0, 0), grid=64)], ids=str)
def test_shim_refuses_a_weight_with_a_window_before_any_gpu_use(kw, no_gpu):
    torch = no_gpu
    import torchOptics.optics as tt
    with pytest.raises(ValueError, match="pixel_weight"):
        _loss_call(tt, torch, torch.ones((64, 64)), kw, shape=(2, 2, 32, 32) if "roi" not in kw else (2, 2, 64, 64))


@pytest.mark.parametrize("stack", [False, True], ids=["loss", "loss_stack"])
def test_shim_refuses_bad_weights_before_any_gpu_use(stack, no_gpu):
    torch = no_gpu
    import torchOptics.optics as tt
    with pytest.raises(ValueError, match="real"):              # a complex weight
        _loss_call(tt, torch, torch.ones((64, 64), dtype=torch.complex64), stack=stack)
    with pytest.raises(ValueError, match="constant"):          # a differentiable weight
        _loss_call(tt, torch, torch.ones((64, 64), requires_grad=True), stack=stack)
    for bad in ((64, 32), (3, 64, 64), (3, 1, 64, 64), (1, 1, 1, 1, 1, 64, 64)):   # no broadcast to the target
        with pytest.raises(ValueError, match="broadcast"):
            _loss_call(tt, torch, torch.ones(bad), stack=stack)
    with pytest.raises(ValueError, match="broadcast"):          # a 3-D x: the weight has no env axis either
        _loss_call(tt, torch, torch.ones((2, 1, 64, 64)), stack=False, squeeze=True)
    with pytest.raises(ValueError):                             # the checks of the unweighted call still run
        _loss_call(tt, torch, torch.ones((64, 64)), dict(tf="nope"), stack=stack)


@pytest.mark.parametrize("stack", [False, True], ids=["loss", "loss_stack"])
def test_shim_passes_a_well_formed_weighted_call_on_to_the_gpu(stack, no_gpu):
    torch = no_gpu
    import torchOptics.optics as tt
    d = (2,) if stack else ()
    shapes = [(64, 64), (1, 64, 64), (2, 1, 64, 64), (1, 1, 64, 64)] + ([(2, 1, 1, 64, 64), (2, 2, 1, 64, 64)] if stack else [])
    for shape in shapes:
        with pytest.raises(AssertionError, match="reached the GPU runtime"):
            _loss_call(tt, torch, torch.ones(shape), stack=stack)
    with pytest.raises(AssertionError, match="reached the GPU runtime"):     # float64 and numpy weights are cast
        _loss_call(tt, torch, np.ones(d + (2, 1, 64, 64)), stack=stack)
    with pytest.raises(AssertionError, match="reached the GPU runtime"):     # a 3-D x with a [G, H, W] weight
        _loss_call(tt, torch, torch.ones((1, 64, 64)), stack=stack, squeeze=True)
    for kw in (dict(field="phase"), dict(field="phase", levels=8), dict(threshold=0.5, field="phase")):
        with pytest.raises(AssertionError, match="reached the GPU runtime"):
            _loss_call(tt, torch, torch.ones((64, 64)), kw, stack=stack)


# -- 4. the weighted loss and its gradient against central differences ---------------------------------------
@pytest.mark.parametrize("depths", [1, 3], ids=["one-depth", "stack"])
@pytest.mark.parametrize("complex_u", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("kind,rel", [(LOSS_MSE, REL_LSQ), (LOSS_MSE, REL_NONE), (LOSS_PSNR, REL_LSQ),
                                      (LOSS_PSNR, REL_NONE)], ids=["mse-lsq", "mse-none", "psnr-lsq", "psnr-none"])
def test_weighted_gradient_formulas_against_central_differences(depths, complex_u, kind, rel):
    """The criterion of tests/test_phase_levels_host.py's gradient test: N = 64, G = 2, central differences
    (step 1e-6) of the float64 weighted loss along single samples against pw_gradient at those samples, within
    5e-6 of max|g|.  The weight is uniform in [0, 1) with a quarter of the pixels exactly 0, one per depth."""
    from oracle import hbx_oracle as O
    n, g_, p = 64, 2, 4
    pc = p // 2 if complex_u else p
    zs = (2e-3, -1.5e-3, 2e-3)[:depths]
    wl = (638e-9, 450e-9)
    dx = O.OpticsConfig(n, n, g_, p, wl).dx
    hs = [[O.transfer_function(n, n, dx, dx, wl[g], z) for g in range(g_)] for z in zs]
    rng = np.random.default_rng(4100 + 8 * depths + 4 * complex_u + 2 * kind + rel)
    u = 2 * rng.random((g_, pc, n, n)) - 1
    if complex_u:
        u = u + 1j * (2 * rng.random((g_, pc, n, n)) - 1)
    i0 = pw_forward(u, hs)[1]
    targets = rng.random((depths, g_, n, n)) * 2.0 * i0.mean()
    v = random_weight(rng, (depths, g_, n, n)).astype(np.float64)
    assert 0.2 < float((v == 0).mean()) < 0.3
    grad = pw_gradient(u, targets, v, hs, kind, rel, not complex_u)
    gmax = np.max(np.abs(grad))
    assert gmax > 0.0
    eps, worst = 1e-6, 0.0
    for _ in range(8):
        idx = tuple(int(rng.integers(0, s)) for s in u.shape)
        for part in ((1.0, 1j) if complex_u else (1.0,)):
            up, dn = u.copy(), u.copy()
            up[idx] += eps * part
            dn[idx] -= eps * part
            fd = (pw_loss(up, targets, v, hs, kind, rel) - pw_loss(dn, targets, v, hs, kind, rel)) / (2 * eps)
            an = grad[idx].imag if part == 1j else np.real(grad[idx])
            worst = max(worst, abs(fd - an) / gmax)
    print(f"D={depths} complex={complex_u} kind={kind} rel={rel}: worst |fd - g| / max|g| = {worst:.3e}")
    assert worst <= 5e-6


def test_unit_weight_is_the_unweighted_loss_and_degenerate_envs_get_zero():
    from oracle import hbx_oracle as O
    from tests.test_loss_host import loss_coeffs
    rng = np.random.default_rng(6)
    i, t = rng.random((3, 8, 8)), rng.random((3, 8, 8))
    ones = np.ones_like(i)
    sums = pw_sums(i, t, ones)
    assert sums[3] == 3 * 64
    assert pw_loss_from_sums(*sums, LOSS_MSE, REL_LSQ) == pytest.approx(O.relative_mse(i, t, REL_LSQ), rel=1e-12)
    assert pw_loss_from_sums(*sums, LOSS_PSNR, REL_NONE) == pytest.approx(O.relative_psnr(i, t, REL_NONE), rel=1e-12)
    stats = np.stack([O.chan_stats(i[g], t[g]) for g in range(3)])
    for kind in (LOSS_MSE, LOSS_PSNR):
        for rel in (REL_LSQ, REL_NONE):
            assert pw_coeffs(*sums, kind, rel) == pytest.approx(loss_coeffs(stats, kind, rel, 3 * 64), rel=1e-12)
    # a rectangle's indicator: the sums over the rectangle, W its pixel count
    box = np.zeros_like(i)
    box[:, 2:7, 1:4] = 1.0
    sb = pw_sums(i, t, box)
    assert sb[3] == 3 * 5 * 3 and sb[0] == pytest.approx(float((i * t)[:, 2:7, 1:4].sum()), rel=1e-14)
    # an all-zero weight: loss 0 / +inf, coefficients 0, never a NaN
    z = pw_sums(i, t, np.zeros_like(i))
    assert z == (0.0, 0.0, 0.0, 0.0)
    assert pw_loss_from_sums(*z, LOSS_MSE, REL_LSQ) == 0.0 and pw_loss_from_sums(*z, LOSS_PSNR, REL_NONE) == math.inf
    for kind in (LOSS_MSE, LOSS_PSNR):
        for rel in (REL_LSQ, REL_NONE):
            assert pw_coeffs(*z, kind, rel) == (0.0, 0.0)
