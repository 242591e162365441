"""hbx_simulate_complex_weighted, hbx_intensity_real and tt.intensity without a GPU: the header and
the exports, the gradient formula the GPU tests use as their expected value (against a central
difference of the float64 oracle), and the shim's argument checks, which raise before any GPU use."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT

HEADER = os.path.join(ROOT, "include", "hbx.h")
NAMES = ("hbx_simulate_complex_weighted", "hbx_intensity_real")


def test_header_declares_both_entry_points_and_abi_stays_15():
    from hbx import _lib
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+hbx_simulate_complex_weighted\s*\(\s*hbx_plan_t\s+plan\s*,\s*const\s+float\s*\*\s*values\s*,"
                     r"\s*const\s+float\s*\*\s*weight\s*,\s*float\s+scale\s*,\s*int32_t\s+n_env\s*,\s*float\s*\*\s*field\s*,"
                     r"\s*float\s*\*\s*real_part\s*,\s*void\s*\*\s*stream\s*\)", src)
    assert re.search(r"\bint\s+hbx_intensity_real\s*\(\s*hbx_plan_t\s+plan\s*,\s*const\s+float\s*\*\s*values\s*,"
                     r"\s*int32_t\s+n_env\s*,\s*float\s*\*\s*intensity\s*,\s*void\s*\*\s*stream\s*\)", src)
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS
    version = int(re.search(r"#define\s+HBX_ABI_VERSION\s+(\d+)", src).group(1))
    assert version == _lib.ABI_VERSION == 15
    assert text.count("(ABI v15, additive)") >= 3


def test_nm_exports_both_entry_points_and_null_plan_is_invalid():
    import ctypes as C
    from hbx import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in NAMES:
        assert name in syms, f"{name} not exported with C linkage"
    lib = _lib.load()
    assert lib.hbx_abi_version() == 15
    assert lib.hbx_simulate_complex_weighted(None, None, None, C.c_float(1.0), 1, None, None, None) == _lib.ERR_INVALID
    assert b"null plan" in lib.hbx_last_error()
    assert lib.hbx_intensity_real(None, None, 1, None, None) == _lib.ERR_INVALID
    assert b"null plan" in lib.hbx_last_error()


def test_gradient_formula_against_a_central_difference():
    """L(x) = sum w mean_p |A x_p|^2 for real x; g = Re A^H((2 / P) w A x), A^H through conj h.  L is
    quadratic in x, so the central difference along a direction d is <g, d> up to rounding."""
    from oracle import hbx_oracle as O
    n, p = 64, 4
    h = O.transfer_function(n, n, O.PIXEL_PITCH, O.PIXEL_PITCH, 515e-9, 2e-3)
    rng = np.random.default_rng(5)
    x = 2 * rng.random((p, n, n)) - 1
    d = 2 * rng.random((p, n, n)) - 1
    w = rng.random((n, n))

    def loss(v):
        return float(np.sum(w * np.mean(np.abs(O.propagate(v, h)) ** 2, axis=0)))

    g = O.propagate((2.0 / p) * w * O.propagate(x, h), np.conj(h)).real
    eps = 1e-3
    fd = (loss(x + eps * d) - loss(x - eps * d)) / (2 * eps)
    an = float(np.sum(g * d))
    print(f"central difference {fd:.15e}, <g, d> {an:.15e}, relative {abs(fd - an) / abs(an):.3e}")
    assert abs(an) > 0.0
    assert abs(fd - an) <= 1e-9 * abs(an)


def _t(shape, dtype=np.float32):
    import torch
    return torch.zeros(shape, dtype=torch.complex64 if dtype is complex else torch.float32)


@pytest.mark.parametrize("shape, complex_input, wl, kw, exc", [
    ((1, 5, 64, 64), False, (638e-9, 450e-9), {}, ValueError),             # C % G != 0
    ((1, 6, 64, 64), False, (638e-9, 515e-9, 450e-9), {}, None),           # even C / G: passes the checks
    ((1, 3, 64, 64), False, (638e-9, 515e-9, 450e-9), {}, ValueError),     # G > 1 with odd C / G
    ((1, 2, 64, 64), True, 515e-9, {"field": "phase"}, ValueError),        # complex input with field="phase"
    ((64, 64), False, 515e-9, {}, ValueError),                             # neither 3-D nor 4-D
    ((1, 1, 2, 64, 64), False, 515e-9, {}, ValueError),
    ((1, 10, 64, 64), False, (1e-6,) * 5, {}, ValueError),                 # more than HBX_MAX_GROUPS wavelengths
    ((1, 2, 64, 64), False, 515e-9, {"tf": "nope"}, ValueError),
])
def test_shim_argument_checks_raise_before_any_gpu_use(shape, complex_input, wl, kw, exc, monkeypatch):
    torch = pytest.importorskip("torch")
    import torchOptics.optics as tt

    class Reached(Exception):
        pass

    def no_gpu():
        raise Reached()
    # the first thing intensity asks the GPU runtime: reaching it means every argument check passed
    monkeypatch.setattr(torch.cuda, "is_available", no_gpu)
    x = tt.Tensor(_t(shape, complex if complex_input else np.float32), meta={"dx": (7.56e-6, 7.56e-6), "wl": wl})
    with pytest.raises(exc or Reached):
        tt.intensity(x, 2e-3, **kw)


def test_shim_needs_meta(monkeypatch):
    torch = pytest.importorskip("torch")
    import torchOptics.optics as tt
    assert "intensity" in tt.__all__
    with pytest.raises(ValueError):
        tt.intensity(torch.zeros((1, 2, 64, 64)), 2e-3)
    with pytest.raises(ValueError):
        tt.intensity(tt.Tensor(torch.zeros((1, 2, 64, 64))), 2e-3)
