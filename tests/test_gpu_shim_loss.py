"""tt.loss: the relative MSE / PSNR per env of the plane-mean intensity against a target, and its
gradient, on the HIP path.

Forward: against the float64 oracle (O.relative_mse / O.relative_psnr of the oracle intensity, per
env) within the project's bounds -- MSE relative 2.31e-5, PSNR 1e-4 dB.
Backward, split form: `want` is built in float64 from the GPU's own downloaded field, intensity and
chan_stats -- the weight a I + c T by the formulas of include/hbx.h (tests/test_loss_host.py), then
O.propagate((2 / P_c) w F, conj h) --, so one propagation and the float32 weight separate the two
sides: 2e-5 of max|want| (tests/test_gpu_shim_intensity.py).
Backward, end to end: against the all-float64 oracle gradient from the samples, next to the parent
route's (autograd through tt.relativeLoss(tt.intensity(x), target, F.mse_loss)): both are float32
routes that differ in rounding order, so the new route's error may be at most twice the parent's.
Measured on an MI355X (errors as a fraction of max|oracle gradient|, new route / parent route):
real 2.85e-7 / 2.65e-7, complex 3.11e-7 / 3.64e-7, phase 3.05e-7 / 3.20e-7, rgb 2.54e-7 / 2.90e-7."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import hbx_oracle as O  # noqa: E402
from tests.test_loss_host import LOSS_MSE, LOSS_PSNR, REL_LSQ, REL_NONE, loss_coeffs, loss_gradient  # noqa: E402

Z = 2e-3
WL = 515e-9
FIELD_RTOL = 2e-5
PSNR_ATOL = 1e-4
MSE_RTOL = 2.31e-5
KIND = {"mse": LOSS_MSE, "psnr": LOSS_PSNR}
REL = {"lsq": REL_LSQ, "none": REL_NONE}
UP = np.array([1.0, -0.5])      # per-env upstream gradients that differ


def _meta(wl=WL):
    return {"dx": (O.PIXEL_PITCH, O.PIXEL_PITCH), "wl": wl}


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm GPU")
    import hbx
    hbx.load_library()
    yield


CASES = {
    # name: (shape, complex leaf, wavelengths, loss keywords, oracle tf kind, phase)
    "real": ((2, 4, 64, 64), False, (WL,), {}, O.TF_ASM, False),
    "complex": ((2, 3, 64, 64), True, (WL,), {}, O.TF_ASM, False),
    "phase": ((2, 3, 64, 64), False, (WL,), {"field": "phase"}, O.TF_ASM, True),
    "fresnel": ((2, 4, 64, 64), False, (WL,), {"tf": "fresnel"}, O.TF_FRESNEL, False),
    "rgb": ((2, 6, 64, 64), False, tuple(O.WL_RGB), {}, O.TF_ASM, False),
    "real_256": ((1, 2, 256, 256), False, (WL,), {}, O.TF_ASM, False),
}
FORWARD = [("real", "mse", "lsq"), ("real", "mse", "none"), ("real", "psnr", "lsq"), ("real", "psnr", "none"),
           ("complex", "mse", "lsq"), ("complex", "psnr", "lsq"), ("phase", "mse", "lsq"), ("phase", "psnr", "lsq"),
           ("fresnel", "mse", "lsq"), ("fresnel", "psnr", "lsq"), ("rgb", "mse", "lsq"), ("rgb", "psnr", "lsq"),
           ("real_256", "mse", "lsq"), ("real_256", "psnr", "lsq")]
GRADIENT = [("real", "mse", "lsq"), ("real", "psnr", "lsq"), ("real", "mse", "none"), ("real", "psnr", "none"),
            ("complex", "mse", "lsq"), ("complex", "psnr", "none"), ("phase", "psnr", "lsq"), ("phase", "mse", "none"),
            ("fresnel", "mse", "lsq"), ("rgb", "mse", "lsq"), ("rgb", "psnr", "lsq"), ("real_256", "psnr", "lsq")]


@functools.lru_cache(maxsize=None)
def _case(name):
    """(x, u64 = the float64 field samples [B, G, Pc, N, N], target f32 [B, G, N, N] in [0, 1) -- no
    multiple of the intensity, so the residual s I - T does not vanish --, the G transfer functions),
    read-only"""
    shape, complex_leaf, wls, _, tf_kind, phase = CASES[name]
    b, c, n, _ = shape
    g = len(wls)
    rng = np.random.default_rng(1500 + len(name) + c)
    x = (2 * rng.random(shape, dtype=np.float32) - 1).astype(np.float32)
    if complex_leaf:
        x = (x + 1j * (2 * rng.random(shape, dtype=np.float32) - 1).astype(np.float32)).astype(np.complex64)
    x64 = x.astype(np.complex128 if complex_leaf else np.float64)
    u64 = (np.exp(1j * np.pi * x64) if phase else x64).reshape(b, g, c // g, n, n)
    target = rng.random((b, g, n, n), dtype=np.float32)
    hs = tuple(O.transfer_function(n, n, O.PIXEL_PITCH, O.PIXEL_PITCH, wl, Z, tf_kind) for wl in wls)
    for a in (x, u64, target) + hs:
        a.setflags(write=False)
    return x, u64, target, hs


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """float64 (field [B, G, Pc, N, N], intensity [B, G, N, N]) from the samples"""
    _, u64, _, hs = _case(name)
    field = np.stack([np.stack([O.propagate(u64[e, k], hs[k]) for k in range(len(hs))]) for e in range(u64.shape[0])])
    inten = np.mean(field.real ** 2 + field.imag ** 2, axis=2)
    field.setflags(write=False)
    inten.setflags(write=False)
    return field, inten


def _wl_arg(wls):
    return wls[0] if len(wls) == 1 else tuple(wls)


def _call(tt, name, x, target, metric, rel):
    _, _, wls, kw, _, _ = CASES[name]
    return tt.loss(tt.Tensor(x, meta=_meta(_wl_arg(wls))), target, Z, metric=metric, rel_scale=rel, **kw)


# -- 9. forward ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, metric, rel", FORWARD)
def test_forward_is_the_oracle_loss_per_env(name, metric, rel):
    import torchOptics.optics as tt
    shape = CASES[name][0]
    x_np, _, t_np, _ = _case(name)
    _, want_i = _oracle(name)
    x, target = torch.from_numpy(x_np.copy()).cuda(), torch.from_numpy(t_np.copy()).cuda()
    got = _call(tt, name, x, target, metric, rel)
    xr = x.clone().requires_grad_()
    with torch.no_grad():
        quiet = _call(tt, name, xr, target, metric, rel)
    graph = _call(tt, name, xr, target, metric, rel)
    torch.cuda.synchronize()
    assert got.dtype == torch.float64 and tuple(got.shape) == (shape[0],) and got.is_cuda
    assert got.grad_fn is None and not got.requires_grad
    assert quiet.grad_fn is None and not quiet.requires_grad
    assert graph.grad_fn is not None and graph.dtype == torch.float64
    assert torch.equal(graph.detach(), got) and torch.equal(quiet, got)   # the plain call's values, bit for bit
    g = got.cpu().numpy()
    for e in range(shape[0]):
        if metric == "mse":
            want = O.relative_mse(want_i[e], t_np[e].astype(np.float64), REL[rel])
            print(f"{name} {metric} {rel} env {e}: {g[e]:.9e} want {want:.9e} rel err {abs(g[e] - want) / want:.2e}")
            assert abs(g[e] - want) <= MSE_RTOL * want
        else:
            want = O.relative_psnr(want_i[e], t_np[e].astype(np.float64), REL[rel])
            print(f"{name} {metric} {rel} env {e}: {g[e]:.6f} dB want {want:.6f} err {abs(g[e] - want):.2e} dB")
            assert abs(g[e] - want) <= PSNR_ATOL


def test_chw_input_gives_a_zero_dim_loss():
    import torchOptics.optics as tt
    x_np, _, t_np, _ = _case("real")
    x, target = torch.from_numpy(x_np.copy()).cuda(), torch.from_numpy(t_np.copy()).cuda()
    full = tt.loss(tt.Tensor(x, meta=_meta()), target, Z)
    one = tt.loss(tt.Tensor(x[1], meta=_meta()), target[1], Z)
    assert one.dim() == 0 and one.dtype == torch.float64
    assert torch.equal(one, full[1])
    xr = x[1].clone().requires_grad_()
    tt.loss(tt.Tensor(xr, meta=_meta()), target[1], Z).backward()
    assert xr.grad is not None and tuple(xr.grad.shape) == tuple(xr.shape)


# -- 10. gradient, split form ----------------------------------------------------------------------------
def _backward(tt, name, metric, rel):
    """x.grad of sum_b UP[b] loss_b through tt.loss (a fresh leaf)"""
    x_np, _, t_np, _ = _case(name)
    x = torch.from_numpy(x_np.copy()).cuda().requires_grad_()
    target = torch.from_numpy(t_np.copy()).cuda()
    loss = _call(tt, name, x, target, metric, rel)
    assert loss.grad_fn is not None
    up = torch.from_numpy(UP[:x.shape[0]].copy()).cuda()
    (loss * up).sum().backward()
    assert x.grad is not None and x.grad.dtype == x.dtype and tuple(x.grad.shape) == tuple(x.shape)
    return x.grad.cpu().numpy()


def _leaf_gradient(name, adj):
    """the gradient at the leaf from dL/du [B, G, Pc, N, N]: real part, field, or the phase chain rule"""
    shape, complex_leaf, _, _, _, phase = CASES[name]
    _, u64, _, _ = _case(name)
    if phase:
        adj = (np.conj(1j * np.pi * u64) * adj).real
    elif not complex_leaf:
        adj = adj.real
    return adj.reshape(shape)


@pytest.mark.parametrize("name, metric, rel", GRADIENT)
def test_gradient_split_form(name, metric, rel):
    import torchOptics.optics as tt
    from hbx import _lib
    shape, complex_leaf, wls, kw, _, phase = CASES[name]
    x_np, _, t_np, hs = _case(name)
    b, c, n, _ = shape
    g = len(wls)
    got = _backward(tt, name, metric, rel)

    # the forward pass's own field, intensity and statistics (the call is deterministic)
    t = torch.from_numpy(x_np.copy()).cuda()
    if phase:
        ph = t.to(torch.float32) * np.float32(np.pi)
        t = torch.complex(torch.cos(ph), torch.sin(ph))
    tf_kind = _lib.TF_FRESNEL if kw.get("tf") == "fresnel" else _lib.TF_ASM
    geom = (wls, O.PIXEL_PITCH, O.PIXEL_PITCH, Z, t.device.index, tf_kind)
    _, field, inten, stats = tt._evaluate(t, torch.from_numpy(t_np.copy()).cuda(), geom, g, True)
    torch.cuda.synchronize()
    f64 = field.cpu().numpy().astype(np.complex128).reshape(b, g, -1, n, n)
    i64, s64 = inten.cpu().numpy().astype(np.float64), stats.cpu().numpy()
    pc = c // g
    assert f64.shape[2] == pc
    adj = np.empty_like(f64)
    for e in range(b):
        a, cc = loss_coeffs(s64[e], KIND[metric], REL[rel], g * n * n, UP[e])
        w = a * i64[e] + cc * t_np[e].astype(np.float64)
        for k in range(g):
            adj[e, k] = O.propagate((2.0 / pc) * w[k] * f64[e, k], np.conj(hs[k]))
    want = _leaf_gradient(name, adj)
    scale = np.max(np.abs(want))
    err = np.max(np.abs(got - want)) / scale
    print(f"{name} {metric} {rel}: grad err {err:.3e} of max|want| = {scale:.3e}")
    assert scale > 0.0
    assert err <= FIELD_RTOL


# -- 11. gradient, end to end ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["real", "complex", "phase", "rgb"])
def test_gradient_end_to_end_against_the_parent_route(name):
    import torch.nn.functional as Fn
    import torchOptics.optics as tt
    shape, _, wls, kw, _, _ = CASES[name]
    x_np, _, t_np, hs = _case(name)
    b = shape[0]
    field, inten = _oracle(name)
    adj = np.stack([loss_gradient(field[e], inten[e], t_np[e].astype(np.float64), hs, LOSS_MSE, REL_LSQ, False, UP[e])
                    for e in range(b)])
    want = _leaf_gradient(name, adj)
    new = _backward(tt, name, "mse", "lsq")

    xp = torch.from_numpy(x_np.copy()).cuda().requires_grad_()
    target = torch.from_numpy(t_np.copy()).cuda()
    chain = tt.intensity(tt.Tensor(xp, meta=_meta(_wl_arg(wls))), Z, **kw)
    total = sum(float(UP[e]) * tt.relativeLoss(chain[e], target[e], Fn.mse_loss) for e in range(b))
    total.backward()
    torch.cuda.synchronize()
    parent = xp.grad.cpu().numpy()
    scale = np.max(np.abs(want))
    e_new, e_par = np.max(np.abs(new - want)) / scale, np.max(np.abs(parent - want)) / scale
    print(f"{name}: end-to-end grad err of max|oracle grad| = {scale:.3e}: new route {e_new:.3e}, parent route {e_par:.3e}")
    assert scale > 0.0
    assert e_new <= 2.0 * e_par


# -- 12. descent -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaf", ["amplitude", "phase"])
def test_adam_descent_lowers_the_loss(leaf):
    import torchOptics.optics as tt
    rng = np.random.default_rng(33)
    logits = torch.from_numpy((rng.random((2, 4, 64, 64), dtype=np.float32) - 0.5).astype(np.float32)).cuda()
    logits.requires_grad_()
    target = torch.from_numpy(rng.random((2, 1, 64, 64), dtype=np.float32)).cuda()
    opt = torch.optim.Adam([logits], lr=0.05)
    losses = []
    for _ in range(11):
        opt.zero_grad()
        if leaf == "amplitude":
            loss = tt.loss(tt.Tensor(torch.sigmoid(logits), meta=_meta()), target, Z).sum()
        else:
            loss = tt.loss(tt.Tensor(logits, meta=_meta()), target, Z, field="phase").sum()
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    losses = [float(v) for v in losses]
    print(leaf, "losses", " ".join(f"{v:.6f}" for v in losses))
    assert losses[-1] < losses[0]                    # the loss after ten steps against the first
