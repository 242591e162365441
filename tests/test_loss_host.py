"""hbx_evaluate_real / hbx_evaluate_complex / hbx_loss / hbx_loss_weight and tt.loss without a GPU: the
header and the exports, the gradient formulas of hbx_loss_weight (restated here in numpy; the GPU
tests import them as their expected values) against central differences of the float64 oracle, and
the shim's argument checks, which raise before any GPU use."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT

HEADER = os.path.join(ROOT, "include", "hbx.h")
NAMES = ("hbx_evaluate_real", "hbx_evaluate_complex", "hbx_loss", "hbx_loss_weight")
LOSS_MSE, LOSS_PSNR = 0, 1
REL_NONE, REL_LSQ = 0, 1


# -- the formulas of include/hbx.h (hbx_loss_weight), float64 ----------------------------------------
def loss_coeffs(stats, kind, rel, count, up=1.0):
    """(a, c) with d loss / d I = a I + c T for one env: stats [G, 3] = (sum IT, sum I^2, sum T^2) per
    group, count = G H W, up = the incoming gradient.  A degenerate env gets (0, 0)."""
    sxy, sxx, syy = (float(v) for v in np.asarray(stats, np.float64).reshape(-1, 3).sum(axis=0))
    if rel == REL_LSQ:
        if sxx > 0.0:
            s = sxy / sxx
            a, c, mse = 2.0 * s * s / count, -2.0 * s / count, (syy - sxy * sxy / sxx) / count
        else:
            a, c, mse = 0.0, 0.0, syy / count
    else:
        a, c, mse = 2.0 / count, -2.0 / count, (sxx - 2.0 * sxy + syy) / count
    if kind == LOSS_PSNR:
        f = -(10.0 / math.log(10.0)) / mse if mse > 0.0 else 0.0
        a, c = a * f, c * f
    return a * up, c * up


def loss_gradient(field, inten, target, hs, kind, rel, real_input, up=1.0):
    """d loss / d u for one env, float64: field [G, Pc, n, n] complex (the propagated planes), inten and
    target [G, n, n], hs the G transfer functions.  w = a I + c T, then A^H((2 / Pc) w F) through
    conj h; the real part for a real u."""
    from oracle import hbx_oracle as O
    g_, pc, n, _ = field.shape
    a, c = loss_coeffs(O_stats(inten, target), kind, rel, g_ * n * n, up)
    w = a * inten + c * target
    out = np.stack([O.propagate((2.0 / pc) * w[g] * field[g], np.conj(hs[g])) for g in range(g_)])
    return out.real if real_input else out


def O_stats(inten, target):
    from oracle import hbx_oracle as O
    return np.stack([O.chan_stats(inten[g], target[g]) for g in range(inten.shape[0])])


def oracle_loss(u, target, hs, kind, rel):
    """(loss, field [G, Pc, n, n], intensity [G, n, n]) of one env's samples u [G, Pc, n, n], float64"""
    from oracle import hbx_oracle as O
    field = np.stack([O.propagate(u[g], hs[g]) for g in range(u.shape[0])])
    inten = np.mean(field.real ** 2 + field.imag ** 2, axis=1)
    val = O.relative_psnr(inten, target, rel) if kind == LOSS_PSNR else O.relative_mse(inten, target, rel)
    return val, field, inten


# -- header and exports --------------------------------------------------------------------------
def test_header_declares_the_four_entry_points_and_abi_stays_15():
    from hbx import _lib
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    ev = (r"\s*\(\s*hbx_plan_t\s+plan\s*,\s*const\s+float\s*\*\s*values\s*,\s*const\s+float\s*\*\s*target\s*,"
          r"\s*int32_t\s+n_env\s*,\s*float\s*\*\s*field\s*,\s*float\s*\*\s*intensity\s*,\s*double\s*\*\s*chan_stats\s*,"
          r"\s*double\s*\*\s*psnr\s*,\s*void\s*\*\s*stream\s*\)")
    assert re.search(r"\bint\s+hbx_evaluate_real" + ev, src)
    assert re.search(r"\bint\s+hbx_evaluate_complex" + ev, src)
    assert re.search(r"\bint\s+hbx_loss\s*\(\s*hbx_plan_t\s+plan\s*,\s*const\s+double\s*\*\s*chan_stats\s*,"
                     r"\s*int32_t\s+n_env\s*,\s*int32_t\s+kind\s*,\s*int32_t\s+rel_scale\s*,\s*double\s*\*\s*loss\s*,"
                     r"\s*void\s*\*\s*stream\s*\)", src)
    assert re.search(r"\bint\s+hbx_loss_weight\s*\(\s*hbx_plan_t\s+plan\s*,\s*const\s+float\s*\*\s*intensity\s*,"
                     r"\s*const\s+float\s*\*\s*target\s*,\s*const\s+double\s*\*\s*chan_stats\s*,"
                     r"\s*const\s+double\s*\*\s*grad_loss\s*,\s*int32_t\s+n_env\s*,\s*int32_t\s+kind\s*,"
                     r"\s*int32_t\s+rel_scale\s*,\s*float\s*\*\s*weight\s*,\s*void\s*\*\s*stream\s*\)", src)
    assert int(re.search(r"#define\s+HBX_LOSS_MSE\s+(\d+)", src).group(1)) == _lib.LOSS_MSE == LOSS_MSE
    assert int(re.search(r"#define\s+HBX_LOSS_PSNR\s+(\d+)", src).group(1)) == _lib.LOSS_PSNR == LOSS_PSNR
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS
    version = int(re.search(r"#define\s+HBX_ABI_VERSION\s+(\d+)", src).group(1))
    assert version == _lib.ABI_VERSION == 15


def test_nm_exports_the_four_entry_points_and_null_plan_is_invalid():
    from hbx import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in NAMES:
        assert name in syms, f"{name} not exported with C linkage"
    lib = _lib.load()
    assert lib.hbx_abi_version() == 15
    calls = (lambda: lib.hbx_evaluate_real(None, None, None, 1, None, None, None, None, None),
             lambda: lib.hbx_evaluate_complex(None, None, None, 1, None, None, None, None, None),
             lambda: lib.hbx_loss(None, None, 1, LOSS_MSE, REL_LSQ, None, None),
             lambda: lib.hbx_loss_weight(None, None, None, None, None, 1, LOSS_MSE, REL_LSQ, None, None))
    for call in calls:
        assert call() == _lib.ERR_INVALID
        assert b"null plan" in lib.hbx_last_error()


# -- the gradient formulas against central differences -------------------------------------------
@pytest.mark.parametrize("complex_u", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("kind", [LOSS_MSE, LOSS_PSNR], ids=["mse", "psnr"])
@pytest.mark.parametrize("rel", [REL_LSQ, REL_NONE], ids=["lsq", "none"])
def test_gradient_formulas_against_central_differences(complex_u, kind, rel):
    """N = 64, G = 2, P = 4 real planes (or 2 complex planes) per group, step 1e-6.  The central
    difference of the float64 oracle loss along single samples (real and, for a complex u, imaginary
    parts) against the formulas' gradient at those samples; bound 5e-6 of max|g|: ten times the worst
    deviation seen (4.6e-7), which leaves room for the difference quotient's rounding."""
    from oracle import hbx_oracle as O
    n, g_, p = 64, 2, 4
    pc = p // 2 if complex_u else p
    cfg = O.OpticsConfig(n, n, g_, p, (638e-9, 450e-9))
    hs = [cfg.transfer(g) for g in range(g_)]
    rng = np.random.default_rng(11 + 2 * kind + rel)
    u = 2 * rng.random((g_, pc, n, n)) - 1
    if complex_u:
        u = u + 1j * (2 * rng.random((g_, pc, n, n)) - 1)
    # a target of the intensity's magnitude that is no multiple of it: the residual s I - T stays
    _, _, i0 = oracle_loss(u, np.zeros((g_, n, n)), hs, LOSS_MSE, REL_NONE)
    target = rng.random((g_, n, n)) * 2.0 * i0.mean()
    _, field, inten = oracle_loss(u, target, hs, kind, rel)
    grad = loss_gradient(field, inten, target, hs, kind, rel, not complex_u)
    gmax = np.max(np.abs(grad))
    assert gmax > 0.0
    eps, worst = 1e-6, 0.0
    for _ in range(12):
        idx = tuple(int(rng.integers(0, s)) for s in u.shape)
        for part in ((1.0, 1j) if complex_u else (1.0,)):
            up, dn = u.copy(), u.copy()
            up[idx] += eps * part
            dn[idx] -= eps * part
            fd = (oracle_loss(up, target, hs, kind, rel)[0] - oracle_loss(dn, target, hs, kind, rel)[0]) / (2 * eps)
            an = grad[idx].imag if part == 1j else np.real(grad[idx])
            worst = max(worst, abs(fd - an) / gmax)
    print(f"complex={complex_u} kind={kind} rel={rel}: worst |fd - g| / max|g| = {worst:.3e}")
    assert worst <= 5e-6


def test_degenerate_coefficients_are_zero():
    zero_i = np.array([[0.0, 0.0, 3.0]])
    assert loss_coeffs(zero_i, LOSS_MSE, REL_LSQ, 4096) == (0.0, 0.0)
    assert loss_coeffs(zero_i, LOSS_PSNR, REL_LSQ, 4096) == (0.0, 0.0)
    exact = np.array([[2.0, 2.0, 2.0]])                  # I == T: MSE = 0
    assert loss_coeffs(exact, LOSS_PSNR, REL_NONE, 4096) == (0.0, 0.0)


# -- tt.loss argument checks ---------------------------------------------------------------------
def _t(shape, complex_input=False):
    import torch
    return torch.zeros(shape, dtype=torch.complex64 if complex_input else torch.float32)


RGB = (638e-9, 515e-9, 450e-9)


@pytest.mark.parametrize("shape, complex_input, wl, tshape, kw, exc", [
    ((1, 6, 64, 64), False, RGB, (1, 3, 64, 64), {}, None),                       # passes every check
    ((6, 64, 64), False, RGB, (3, 64, 64), {}, None),                             # 3-D x, 3-D target
    ((1, 3, 64, 64), True, RGB, (1, 3, 64, 64), {}, None),                        # complex: any C / G >= 1
    ((1, 3, 64, 64), False, RGB, (1, 3, 64, 64), {"field": "phase"}, None),       # phase: any C / G >= 1
    ((1, 5, 64, 64), False, (638e-9, 450e-9), (1, 2, 64, 64), {}, ValueError),    # C % G != 0
    ((1, 3, 64, 64), False, RGB, (1, 3, 64, 64), {}, ValueError),                 # real x with odd C / G
    ((1, 3, 64, 64), False, 515e-9, (1, 1, 64, 64), {}, ValueError),              # ... also with G = 1
    ((1, 2, 64, 64), True, 515e-9, (1, 1, 64, 64), {"field": "phase"}, ValueError),
    ((64, 64), False, 515e-9, (64, 64), {}, ValueError),                          # neither 3-D nor 4-D
    ((1, 10, 64, 64), False, (1e-6,) * 5, (1, 5, 64, 64), {}, ValueError),        # more than HBX_MAX_GROUPS
    ((1, 2, 64, 64), False, 515e-9, (1, 2, 64, 64), {}, ValueError),              # target per plane, not per group
    ((1, 2, 64, 64), False, 515e-9, (1, 64, 64), {}, ValueError),                 # 3-D target with a 4-D x
    ((2, 2, 64, 64), False, 515e-9, (1, 1, 64, 64), {}, ValueError),              # target batch
    ((1, 2, 64, 64), False, 515e-9, (1, 1, 64, 64), {"tf": "nope"}, ValueError),
    ((1, 2, 64, 64), False, 515e-9, (1, 1, 64, 64), {"metric": "l1"}, ValueError),
    ((1, 2, 64, 64), False, 515e-9, (1, 1, 64, 64), {"rel_scale": "max"}, ValueError),
])
def test_shim_argument_checks_raise_before_any_gpu_use(shape, complex_input, wl, tshape, kw, exc, monkeypatch):
    torch = pytest.importorskip("torch")
    import torchOptics.optics as tt

    class Reached(Exception):
        pass

    def no_gpu():
        raise Reached()
    # the first thing loss asks the GPU runtime: reaching it means every argument check passed
    monkeypatch.setattr(torch.cuda, "is_available", no_gpu)
    x = tt.Tensor(_t(shape, complex_input), meta={"dx": (7.56e-6, 7.56e-6), "wl": wl})
    with pytest.raises(exc or Reached):
        tt.loss(x, _t(tshape), 2e-3, **kw)


def test_shim_target_is_a_constant_and_meta_is_needed(monkeypatch):
    torch = pytest.importorskip("torch")
    import torchOptics.optics as tt
    assert "loss" in tt.__all__

    def no_gpu():
        raise AssertionError("reached the GPU runtime")
    monkeypatch.setattr(torch.cuda, "is_available", no_gpu)
    x = tt.Tensor(torch.zeros((1, 2, 64, 64)), meta={"dx": (7.56e-6, 7.56e-6), "wl": 515e-9})
    with pytest.raises(ValueError):
        tt.loss(x, torch.zeros((1, 1, 64, 64), requires_grad=True), 2e-3)
    with pytest.raises(ValueError):
        tt.loss(torch.zeros((1, 2, 64, 64)), torch.zeros((1, 1, 64, 64)), 2e-3)
    with pytest.raises(ValueError):
        tt.loss(x, torch.zeros((1, 1, 64, 64), dtype=torch.complex64), 2e-3)
