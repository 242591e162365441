"""threshold= on real leaves through tt.simulate / tt.intensity / tt.loss: binary holograms with the
straight-through estimator, the fused route.

The shim hands the float32 samples x to hbx_evaluate_threshold (u = va + vb [x >= tau] formed in the
first pass's load) and takes dL/dx = vb s(x) Re(dL/du) from the last pass of hbx_threshold_backward.
Checked against the float64 oracle at u = the binarised samples: the forward within the project's
bounds (field and intensity 2e-5 of the maximum, MSE 2.31e-5 relative, PSNR 1e-4 dB), x.grad within
2e-5 of max|want| with want = vb s(x) times the oracle's real-leaf gradient -- the bounds of
tests/test_gpu_shim_loss.py.  threshold=None calls are compared with the Plan calls they ran before."""
import functools
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import hbx_oracle as O  # noqa: E402
from tests.test_loss_host import LOSS_MSE, LOSS_PSNR, REL_LSQ, REL_NONE, loss_gradient  # noqa: E402
from tests.test_threshold_ste_host import (STE_SIGMOID, STE_WINDOW, binarize, field_values,  # noqa: E402
                                           ste_surrogate)

Z = 2e-3
WL = 515e-9
TAU = 0.5
FIELD_RTOL = 2e-5
PSNR_ATOL = 1e-4
MSE_RTOL = 2.31e-5
KIND = {"mse": LOSS_MSE, "psnr": LOSS_PSNR}
REL = {"lsq": REL_LSQ, "none": REL_NONE}
FIELD = {"amplitude": O.FIELD_AMPLITUDE, "phase": O.FIELD_PHASE}
UP = np.array([1.0, -0.5])      # per-env upstream gradients that differ
# name: (ste, ste_width) -> the keyword arguments and (surrogate, p0, p1) as the shim forms them in float32
STE = {
    "default": ({}, (STE_WINDOW, 0.0, 1.0)),
    "window": ({"ste": "window", "ste_width": 0.3},
               (STE_WINDOW, float(np.float32(np.float32(TAU) - np.float32(0.3))),
                float(np.float32(np.float32(TAU) + np.float32(0.3))))),
    "plain": ({"ste_width": math.inf}, (STE_WINDOW, -math.inf, math.inf)),
    "sigmoid": ({"ste": "sigmoid", "ste_width": 0.25}, (STE_SIGMOID, TAU, 4.0)),
}

# name: (shape [B, C, N, N], wavelengths)
SHAPES = {
    "mono": ((2, 2, 64, 64), (WL,)),
    "rgb": ((2, 6, 64, 64), tuple(O.WL_RGB)),
    "mono256": ((1, 4, 256, 256), (WL,)),
    "rgb256": ((1, 6, 256, 256), tuple(O.WL_RGB)),
    "odd": ((2, 3, 64, 64), (WL,)),               # odd C with G = 1: tt.simulate alone
}


def _meta(wls):
    return {"dx": (O.PIXEL_PITCH, O.PIXEL_PITCH), "wl": wls[0] if len(wls) == 1 else tuple(wls)}


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm GPU")
    import hbx
    hbx.load_library()
    yield


@functools.lru_cache(maxsize=None)
def _case(name):
    """x float32 [B, C, N, N] uniform in [-0.5, 1.5] with tau and the windows' ends planted; target f32
    [B, G, N, N]; a complex upstream w [B, C, N, N] and a real one gi [B, G, N, N]; the G transfer
    functions.  Read-only."""
    shape, wls = SHAPES[name]
    b, c, n, _ = shape
    g = len(wls)
    rng = np.random.default_rng(4100 + len(name) + c + n)
    x = (2 * rng.random(shape, dtype=np.float32) - 0.5).astype(np.float32)
    ends = [TAU, 0.0, 1.0, STE["window"][1][1], STE["window"][1][2]]
    for plane in x.reshape(-1, n * n):
        plane[rng.choice(n * n, size=2 * len(ends), replace=False)] = np.tile(np.array(ends, np.float32), 2)
    target = rng.random((b, g, n, n), dtype=np.float32)
    w = ((2 * rng.random(shape, dtype=np.float32) - 1) + 1j * (2 * rng.random(shape, dtype=np.float32) - 1))
    w = w.astype(np.complex64)
    gi = (2 * rng.random((b, g, n, n), dtype=np.float32) - 1).astype(np.float32)
    hs = tuple(O.transfer_function(n, n, O.PIXEL_PITCH, O.PIXEL_PITCH, wl, Z, O.TF_ASM) for wl in wls)
    for a in (x, target, w, gi) + hs:
        a.setflags(write=False)
    return x, target, w, gi, hs


@functools.lru_cache(maxsize=None)
def _oracle(name, field):
    """the float64 field [B, G, P, N, N] and intensity [B, G, N, N] of the binarised samples"""
    shape, wls = SHAPES[name]
    b, c, n, _ = shape
    g = len(wls)
    x, _, _, _, hs = _case(name)
    u = binarize(x, TAU, FIELD[field]).astype(np.float64).reshape(b, g, c // g, n, n)
    fld = np.stack([np.stack([O.propagate(u[e, k], hs[k]) for k in range(g)]) for e in range(b)])
    inten = np.mean(fld.real ** 2 + fld.imag ** 2, axis=2)
    fld.setflags(write=False)
    inten.setflags(write=False)
    return fld, inten


def _ste(name, field, ste, real_grad):
    """want = vb s(x) (the oracle's gradient with respect to a real u), float64, x's shape"""
    x = _case(name)[0]
    vb = field_values(FIELD[field])[1]
    kind, p0, p1 = STE[ste][1]
    return vb * ste_surrogate(x, kind, p0, p1) * real_grad.reshape(x.shape)


def _leaf(name, dtype):
    return torch.from_numpy(_case(name)[0].copy()).to(dtype).cuda().requires_grad_()


def _check_gradient(label, x, dtype, want):
    torch.cuda.synchronize()
    assert x.grad is not None and x.grad.dtype == dtype and tuple(x.grad.shape) == tuple(x.shape)
    got = x.grad.cpu().numpy().astype(np.float64)
    scale = np.max(np.abs(want))
    e = np.max(np.abs(got - want)) / scale
    print(f"{label}: grad err {e:.3e} of max|want| = {scale:.3e}")
    assert scale > 0.0
    assert e <= FIELD_RTOL


# -- simulate --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, field, ste, dtype", [
    ("mono", "amplitude", "default", torch.float32), ("mono", "phase", "sigmoid", torch.float64),
    ("odd", "phase", "window", torch.float32), ("odd", "amplitude", "plain", torch.float32),
    ("mono256", "phase", "default", torch.float32)])
def test_simulate_binary_leaf(name, field, ste, dtype):
    """The field of every plane, an odd plane count padded and sliced as the bit path does; equal to
    binary=True on the 0 / 1 mask within the field bound of both; L = Re <w, F> gives dL/du = A^H w."""
    import torchOptics.optics as tt
    shape, wls = SHAPES[name]
    x_np, _, w_np, _, hs = _case(name)
    kw = dict(STE[ste][0], binary=False, field=field, threshold=TAU)
    meta = _meta(wls)
    plain = tt.simulate(tt.Tensor(torch.from_numpy(x_np.copy()).to(dtype).cuda(), meta=meta), Z, **kw)
    xr = _leaf(name, dtype)
    with torch.no_grad():
        quiet = tt.simulate(tt.Tensor(xr, meta=meta), Z, **kw)
    graph = tt.simulate(tt.Tensor(xr, meta=meta), Z, **kw)
    mask = torch.from_numpy((x_np >= np.float32(TAU)).astype(np.float32)).cuda()
    bits = tt.simulate(tt.Tensor(mask, meta=meta), Z, strict=True, field=field)
    torch.cuda.synchronize()
    assert plain.dtype == torch.complex64 and tuple(plain.shape) == shape
    assert plain.grad_fn is None and quiet.grad_fn is None and graph.grad_fn is not None
    assert torch.equal(torch.view_as_real(graph.detach()), torch.view_as_real(plain))
    assert torch.equal(torch.view_as_real(quiet), torch.view_as_real(plain))
    want_f = _oracle(name, field)[0].reshape(shape)
    fmax = np.max(np.abs(want_f))
    e = np.max(np.abs(plain.cpu().numpy() - want_f)) / fmax
    e_bits = np.max(np.abs(bits.cpu().numpy() - want_f)) / fmax
    print(f"simulate {name} {field}: field err {e:.3e} of max|field| (the bit path: {e_bits:.3e})")
    assert e <= FIELD_RTOL and e_bits <= FIELD_RTOL

    w = torch.from_numpy(w_np.copy()).cuda()
    f = tt.simulate(tt.Tensor(xr, meta=meta), Z, **kw)
    (torch.view_as_real(f) * torch.view_as_real(w)).sum().backward()
    adj = np.stack([O.propagate(w_np[e_].astype(np.complex128), np.conj(hs[0])) for e_ in range(shape[0])])
    _check_gradient(f"simulate {name} {field} {ste}", xr, dtype, _ste(name, field, ste, adj.real))


# -- intensity -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, field, ste, dtype", [
    ("mono", "amplitude", "default", torch.float32), ("mono", "phase", "window", torch.float64),
    ("rgb", "phase", "sigmoid", torch.float32), ("rgb256", "amplitude", "plain", torch.float32)])
def test_intensity_binary_leaf(name, field, ste, dtype):
    import torchOptics.optics as tt
    shape, wls = SHAPES[name]
    x_np, _, _, gi_np, hs = _case(name)
    field64, inten64 = _oracle(name, field)
    b, c, n, _ = shape
    g = len(wls)
    meta = _meta(wls)
    kw = dict(STE[ste][0], field=field, threshold=TAU)
    plain = tt.intensity(tt.Tensor(torch.from_numpy(x_np.copy()).to(dtype).cuda(), meta=meta), Z, **kw)
    xr = _leaf(name, dtype)
    with torch.no_grad():
        quiet = tt.intensity(tt.Tensor(xr, meta=meta), Z, **kw)
    graph = tt.intensity(tt.Tensor(xr, meta=meta), Z, **kw)
    torch.cuda.synchronize()
    assert plain.dtype == torch.float32 and tuple(plain.shape) == (b, g, n, n)
    assert plain.grad_fn is None and quiet.grad_fn is None and graph.grad_fn is not None
    assert torch.equal(graph.detach(), plain) and torch.equal(quiet, plain)
    e = np.max(np.abs(plain.cpu().numpy() - inten64)) / np.max(inten64)
    print(f"intensity {name} {field}: err {e:.3e} of max I")
    assert e <= FIELD_RTOL

    gi = torch.from_numpy(gi_np.copy()).cuda()
    (graph * gi).sum().backward()
    pc = c // g
    adj = np.stack([np.stack([O.propagate((2.0 / pc) * gi_np[e_, k].astype(np.float64) * field64[e_, k],
                                          np.conj(hs[k])) for k in range(g)]) for e_ in range(b)])
    _check_gradient(f"intensity {name} {field} {ste}", xr, dtype, _ste(name, field, ste, adj.real))


# -- loss ------------------------------------------------------------------------------------------
LOSS_CASES = [("mono", "mse", "lsq", "amplitude", "default", torch.float32),
              ("mono", "psnr", "lsq", "phase", "default", torch.float32),
              ("mono", "mse", "none", "phase", "window", torch.float32),
              ("mono", "psnr", "none", "amplitude", "sigmoid", torch.float64),
              ("rgb", "mse", "lsq", "phase", "sigmoid", torch.float32),
              ("rgb", "psnr", "lsq", "amplitude", "plain", torch.float32),
              ("mono256", "mse", "lsq", "amplitude", "window", torch.float32),
              ("mono256", "psnr", "none", "phase", "default", torch.float64),
              ("rgb256", "mse", "none", "amplitude", "default", torch.float32),
              ("rgb256", "psnr", "lsq", "phase", "sigmoid", torch.float32)]


@pytest.mark.parametrize("name, metric, rel, field, ste, dtype", LOSS_CASES,
                         ids=["-".join(c[:5]) + ("-f64" if c[5] == torch.float64 else "-f32") for c in LOSS_CASES])
def test_loss_binary_leaf(name, metric, rel, field, ste, dtype):
    import torchOptics.optics as tt
    shape, wls = SHAPES[name]
    x_np, t_np, _, _, hs = _case(name)
    field64, inten64 = _oracle(name, field)
    b = shape[0]
    meta = _meta(wls)
    target = torch.from_numpy(t_np.copy()).cuda()
    kw = dict(STE[ste][0], field=field, threshold=TAU, metric=metric, rel_scale=rel)

    def call(inp):
        return tt.loss(tt.Tensor(inp, meta=meta), target, Z, **kw)
    plain = call(torch.from_numpy(x_np.copy()).to(dtype).cuda())
    xr = _leaf(name, dtype)
    with torch.no_grad():
        quiet = call(xr)
    graph = call(xr)
    torch.cuda.synchronize()
    assert plain.dtype == torch.float64 and tuple(plain.shape) == (b,)
    assert plain.grad_fn is None and quiet.grad_fn is None and graph.grad_fn is not None
    assert torch.equal(graph.detach(), plain) and torch.equal(quiet, plain)
    got = plain.cpu().numpy()
    for e in range(b):
        t64 = t_np[e].astype(np.float64)
        if metric == "mse":
            want = O.relative_mse(inten64[e], t64, REL[rel])
            print(f"loss {name} {field} env {e}: MSE rel err {abs(got[e] - want) / want:.2e}")
            assert abs(got[e] - want) <= MSE_RTOL * want
        else:
            want = O.relative_psnr(inten64[e], t64, REL[rel])
            print(f"loss {name} {field} env {e}: PSNR err {abs(got[e] - want):.2e} dB")
            assert abs(got[e] - want) <= PSNR_ATOL

    up = torch.from_numpy(UP[:b].copy()).cuda()
    (graph * up).sum().backward()
    adj = np.stack([loss_gradient(field64[e], inten64[e], t_np[e].astype(np.float64), hs, KIND[metric], REL[rel],
                                  True, UP[e]) for e in range(b)])
    _check_gradient(f"loss {name} {metric} {rel} {field} {ste}", xr, dtype, _ste(name, field, ste, adj))


# -- threshold=None is what it was -----------------------------------------------------------------
def test_threshold_none_takes_the_calls_it_took_before():
    """simulate, intensity and loss without a threshold, with the new keywords at their defaults or
    left out, against the Plan calls of the continuous path (hbx_simulate_real, hbx_intensity_real,
    hbx_evaluate_real + hbx_loss, hbx_loss_weight + hbx_simulate_complex_weighted), bit for bit."""
    import hbx
    import torchOptics.optics as tt
    from hbx import _lib
    shape, wls = SHAPES["mono"]
    b, c, n, _ = shape
    x_np, t_np, _, _, _ = _case("mono")
    meta = _meta(wls)
    x, target = torch.from_numpy(x_np.copy()).cuda(), torch.from_numpy(t_np.copy()).cuda()
    cfg = hbx.OpticsConfig(n, n, 1, c, wls, O.PIXEL_PITCH, O.PIXEL_PITCH, Z, _lib.TF_ASM, _lib.FIELD_AMPLITUDE,
                           _lib.REL_LSQ, 1.0)
    plan = hbx.Plan(cfg, max_jobs=b)
    adj = hbx.Plan(hbx.OpticsConfig(n, n, 1, 2 * c, wls, O.PIXEL_PITCH, O.PIXEL_PITCH, -Z, _lib.TF_ASM,
                                    _lib.FIELD_AMPLITUDE, _lib.REL_LSQ, 1.0), max_jobs=b)
    for kw in ({}, {"threshold": None}, {"threshold": None, "ste": "sigmoid", "ste_width": 0.1}):
        f = tt.simulate(tt.Tensor(x, meta=meta), Z, binary=False, **kw)
        i = tt.intensity(tt.Tensor(x, meta=meta), Z, **kw)
        lo = tt.loss(tt.Tensor(x, meta=meta), target, Z, **kw)
        assert torch.equal(torch.view_as_real(f), torch.view_as_real(plan.simulate_real(x)[0]))
        assert torch.equal(i, plan.intensity_real(x))
        field, inten, stats, _ = plan.evaluate_real(x, target)
        assert torch.equal(lo, plan.loss(stats, _lib.LOSS_MSE, _lib.REL_LSQ))
        xr = x.clone().requires_grad_()
        tt.loss(tt.Tensor(xr, meta=meta), target, Z, **kw).sum().backward()
        wgt = adj.loss_weight(inten, target, stats, torch.ones(b, dtype=torch.float64, device="cuda"))
        _, want = adj.simulate_complex(field, want_field=False, want_real=True, weight=wgt, scale=2.0 / c)
        assert torch.equal(xr.grad, want)
    # and a 0 / 1 leaf is its own binarisation: the thresholded call returns the continuous call's bits
    m = (x >= TAU).to(torch.float32)
    assert torch.equal(tt.intensity(tt.Tensor(m, meta=meta), Z, threshold=TAU), tt.intensity(tt.Tensor(m, meta=meta), Z))
    assert torch.equal(tt.loss(tt.Tensor(x, meta=meta), target, Z, threshold=TAU),
                       tt.loss(tt.Tensor(m, meta=meta), target, Z))
    plan.close()
    adj.close()


# -- errors ----------------------------------------------------------------------------------------
def test_value_errors():
    import torchOptics.optics as tt
    meta = _meta((WL,))
    real = torch.zeros((1, 2, 64, 64), device="cuda")
    cplx = torch.zeros((1, 2, 64, 64), dtype=torch.complex64, device="cuda")
    odd = torch.zeros((1, 3, 64, 64), device="cuda")
    tgt = torch.zeros((1, 1, 64, 64), device="cuda")
    calls = [lambda: tt.simulate(tt.Tensor(cplx, meta=meta), Z, binary=False, threshold=TAU),
             lambda: tt.intensity(tt.Tensor(cplx, meta=meta), Z, threshold=TAU),
             lambda: tt.loss(tt.Tensor(cplx, meta=meta), tgt, Z, threshold=TAU),
             lambda: tt.simulate(tt.Tensor(real, meta=meta), Z, threshold=TAU),                    # binary=True
             lambda: tt.intensity(tt.Tensor(odd, meta=meta), Z, threshold=TAU),
             lambda: tt.intensity(tt.Tensor(odd, meta=meta), Z, threshold=TAU, field="phase"),
             lambda: tt.loss(tt.Tensor(odd, meta=meta), tgt, Z, threshold=TAU, field="phase"),
             lambda: tt.loss(tt.Tensor(real, meta=meta), tgt, Z, threshold=TAU, ste="hard"),
             lambda: tt.loss(tt.Tensor(real, meta=meta), tgt, Z, threshold=TAU, ste_width=-1.0),
             lambda: tt.loss(tt.Tensor(real, meta=meta), tgt, Z, threshold=TAU, ste="sigmoid", ste_width=0.0)]
    for k, call in enumerate(calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {k} was accepted")
    # the odd plane count that tt.simulate pads is fine, and double backward is refused
    out = tt.simulate(tt.Tensor(odd, meta=meta), Z, binary=False, threshold=TAU, field="phase")
    assert tuple(out.shape) == (1, 3, 64, 64)
    xr = real.clone().requires_grad_()
    val = tt.loss(tt.Tensor(xr, meta=meta), tgt + 1.0, Z, threshold=TAU).sum()
    g, = torch.autograd.grad(val, xr, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


# -- descent ---------------------------------------------------------------------------------------
def test_adam_on_logits_lowers_the_loss_of_the_mask_the_bit_path_sees():
    """The INTEGRATION.md loop: Adam on logits through tt.loss(sigmoid(logits), threshold=0.5), then
    hbx.pack_mask(x, threshold=0.5) into the bit path: hbx_propagate's MSE of that mask is the loss the
    loop minimised, and it is below the first step's."""
    import hbx
    import torchOptics.optics as tt
    from hbx import _lib
    rng = np.random.default_rng(44)
    n, c = 64, 4
    logits = torch.from_numpy(rng.standard_normal((1, c, n, n)).astype(np.float32)).cuda().requires_grad_()
    target = torch.from_numpy(rng.random((1, 1, n, n), dtype=np.float32)).cuda()
    meta = _meta((WL,))
    opt = torch.optim.Adam([logits], lr=0.1)
    losses = []
    for _ in range(16):
        opt.zero_grad()
        val = tt.loss(tt.Tensor(torch.sigmoid(logits), meta=meta), target, Z, threshold=0.5).sum()
        val.backward()
        opt.step()
        losses.append(val.detach())
    with torch.no_grad():
        x = torch.sigmoid(logits)
        last = tt.loss(tt.Tensor(x, meta=meta), target, Z, threshold=0.5)
        plan = hbx.Plan(hbx.OpticsConfig(n, n, 1, c, (WL,), O.PIXEL_PITCH, O.PIXEL_PITCH, Z), max_jobs=1)
        _, stats, _ = plan.propagate(hbx.pack_mask(x, threshold=0.5), target, want_intensity=False)
        bits = plan.loss(stats, _lib.LOSS_MSE, _lib.REL_LSQ)
    losses = [float(v) for v in losses]
    print("binary losses", " ".join(f"{v:.6f}" for v in losses), "final", float(last[0]), "bit path", float(bits[0]))
    assert float(last[0]) < losses[0]
    assert torch.equal(last, bits)
    plan.close()
