"""tt.intensity: the plane-mean intensity I[b, g] = mean_p |A u[b, p]|^2 and its gradient.

Forward: against the float64 oracle's plane-mean intensity within 2e-5 of max I.  Backward: for
L = sum w I the gradient that reaches the propagation is g = (2 / P) w_g F, so x.grad is compared
with the oracle's adjoint O.propagate(g, conj h_g) of the g that the downloaded GPU field (the
parent path, tt.simulate(.., binary=False)) and w imply: one propagation separates the two sides,
so the single-propagation bound FIELD_RTOL x max|want| applies (tests/test_gpu_shim_autograd.py).
A real leaf takes the real part, a complex leaf the whole field, a phase leaf (u = exp(i pi x))
Re(conj(i pi u) A^H g)."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import hbx_oracle as O  # noqa: E402

Z = 2e-3
WL = 515e-9
FIELD_RTOL = 2e-5
INTEN_RTOL = 2e-5


def _meta(wl=WL):
    return {"dx": (O.PIXEL_PITCH, O.PIXEL_PITCH), "wl": wl}


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm GPU")
    import hbx
    hbx.load_library()
    yield


def _h(n, wl=WL, tf_kind=O.TF_ASM):
    return O.transfer_function(n, n, O.PIXEL_PITCH, O.PIXEL_PITCH, wl, Z, tf_kind)


CASES = {
    # name: (shape, complex leaf, wavelengths, intensity keywords, oracle tf kind, phase, leaf dtype)
    "real": ((2, 4, 64, 64), False, (WL,), {}, O.TF_ASM, False, np.float32),
    "complex": ((2, 3, 64, 64), True, (WL,), {}, O.TF_ASM, False, np.float32),
    "phase": ((1, 4, 64, 64), False, (WL,), {"field": "phase"}, O.TF_ASM, True, np.float32),
    "fresnel": ((2, 4, 64, 64), False, (WL,), {"tf": "fresnel"}, O.TF_FRESNEL, False, np.float32),
    "odd_planes_chw": ((3, 64, 64), False, (WL,), {}, O.TF_ASM, False, np.float32),
    "rgb": ((2, 6, 64, 64), False, O.WL_RGB, {}, O.TF_ASM, False, np.float32),
    "float64": ((1, 2, 64, 64), False, (WL,), {}, O.TF_ASM, False, np.float64),
    "real_256": ((1, 2, 256, 256), False, (WL,), {}, O.TF_ASM, False, np.float32),
}
FORWARD = ["real", "complex", "phase", "fresnel", "odd_planes_chw", "rgb", "real_256"]
GRADIENT = ["real", "complex", "phase", "rgb", "odd_planes_chw", "float64", "real_256"]


@functools.lru_cache(maxsize=None)
def _case(name):
    """(x, u64 = the float64 field samples, w [.., G, N, N] f32 -- another image per group --, wls),
    read-only"""
    shape, complex_leaf, wls, _, _, phase, dtype = CASES[name]
    rng = np.random.default_rng(900 + len(name) + shape[-3])
    x = (2 * rng.random(shape, dtype=np.float32) - 1).astype(np.float32)
    if complex_leaf:
        x = (x + 1j * (2 * rng.random(shape, dtype=np.float32) - 1).astype(np.float32)).astype(np.complex64)
    else:
        x = x.astype(dtype)
    x64 = x.astype(np.complex128 if complex_leaf else np.float64)
    u64 = np.exp(1j * np.pi * x64) if phase else x64
    w = rng.random(shape[:-3] + (len(wls),) + shape[-2:], dtype=np.float32)
    for a in (x, u64, w):
        a.setflags(write=False)
    return x, u64, w, wls


def _groups(a, g):
    """[.., C, N, N] -> [.., G, C / G, N, N]"""
    return a.reshape(a.shape[:-3] + (g, a.shape[-3] // g) + a.shape[-2:])


def _oracle_intensity(name):
    _, _, _, _, tf_kind, _, _ = CASES[name]
    _, u64, _, wls = _case(name)
    n, g = u64.shape[-1], len(wls)
    ug = _groups(u64, g)
    out = [np.mean(np.abs(O.propagate(ug[..., k, :, :, :], _h(n, wls[k], tf_kind))) ** 2, axis=-3) for k in range(g)]
    return np.stack(out, axis=-3)


def _wl_arg(wls):
    return wls[0] if len(wls) == 1 else tuple(wls)


@pytest.mark.parametrize("name", FORWARD)
def test_forward_is_the_oracle_plane_mean_intensity(name):
    import torchOptics.optics as tt
    shape, _, wls, kw, _, _, _ = CASES[name]
    x_np = _case(name)[0]
    want = _oracle_intensity(name)
    got = tt.intensity(tt.Tensor(torch.from_numpy(x_np.copy()).cuda(), meta=_meta(_wl_arg(wls))), Z, **kw)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and got.grad_fn is None
    assert tuple(got.shape) == shape[:-3] + (len(wls),) + shape[-2:]
    err = np.max(np.abs(got.cpu().numpy() - want)) / np.max(want)
    print(f"{name}: intensity err {err:.3e} of max I")
    assert err <= INTEN_RTOL


def test_rgb_call_equals_three_single_wavelength_calls():
    import torchOptics.optics as tt
    x = torch.from_numpy(_case("rgb")[0].copy()).cuda()
    rgb = tt.intensity(tt.Tensor(x, meta=_meta(tuple(O.WL_RGB))), Z)
    for k, wl in enumerate(O.WL_RGB):
        one = tt.intensity(tt.Tensor(x[:, 2 * k:2 * k + 2].contiguous(), meta=_meta(wl)), Z)
        assert tuple(one.shape) == (2, 1, 64, 64)
        assert torch.equal(one[:, 0], rgb[:, k]), k
    assert not torch.equal(rgb[:, 0], rgb[:, 2])


def _chain_intensity(tt, x, wls, kw):
    """The parent path: tt.simulate(.., binary=False) per group, |.|^2 and the mean as torch ops;
    returns (intensity [.., G, N, N], the fields by group)"""
    g = len(wls)
    per = x.shape[-3] // g
    fields = [tt.simulate(tt.Tensor(x[..., k * per:(k + 1) * per, :, :], meta=_meta(wls[k])), Z, binary=False, **kw)
              for k in range(g)]
    return torch.stack([(f.abs() ** 2).mean(-3) for f in fields], dim=-3), fields


@pytest.mark.parametrize("name", GRADIENT)
def test_gradient_is_the_oracle_adjoint(name):
    import torchOptics.optics as tt
    shape, complex_leaf, wls, kw, tf_kind, phase, _ = CASES[name]
    x_np, u64, w_np, _ = _case(name)
    n, g = shape[-1], len(wls)
    per = shape[-3] // g
    w = torch.from_numpy(w_np.copy()).cuda()

    x = torch.from_numpy(x_np.copy()).cuda().requires_grad_()
    inten = tt.intensity(tt.Tensor(x, meta=_meta(_wl_arg(wls))), Z, **kw)
    assert inten.grad_fn is not None and inten.dtype == torch.float32
    (w * inten).sum().backward()

    # the same loss through the torch-op chain on the parent path, and the fields it propagates
    xc = torch.from_numpy(x_np.copy()).cuda().requires_grad_()
    chain, fields = _chain_intensity(tt, xc, wls, kw)
    (w * chain).sum().backward()
    torch.cuda.synchronize()

    want = np.empty(shape, np.complex128 if complex_leaf else np.float64)
    wg = _groups(want, g)
    for k in range(g):
        f_gpu = fields[k].detach().cpu().numpy().astype(np.complex128)
        gk = (2.0 / per) * w_np[..., k:k + 1, :, :].astype(np.float64) * f_gpu
        adj = O.propagate(gk, np.conj(_h(n, wls[k], tf_kind)))
        if phase:
            adj = (np.conj(1j * np.pi * _groups(u64, g)[..., k, :, :, :]) * adj).real
        wg[..., k, :, :, :] = adj if complex_leaf else adj.real
    assert x.grad is not None and x.grad.dtype == x.dtype and tuple(x.grad.shape) == shape
    got = x.grad.cpu().numpy()
    scale = np.max(np.abs(want))
    eg = np.max(np.abs(got - want)) / scale
    ec = np.max(np.abs(got - xc.grad.cpu().numpy())) / scale
    print(f"{name}: grad err {eg:.3e} of max|want|, against autograd through the torch-op chain {ec:.3e}")
    assert scale > 0.0
    assert eg <= FIELD_RTOL
    assert ec <= 2 * FIELD_RTOL
    if name == "float64":
        assert x.grad.dtype == torch.float64


@pytest.mark.parametrize("name", ["real", "odd_planes_chw", "rgb"])
def test_save_field_off_gives_the_same_gradient(name):
    import torchOptics.optics as tt
    _, _, wls, kw, _, _, _ = CASES[name]
    x_np, _, w_np, _ = _case(name)
    w = torch.from_numpy(w_np.copy()).cuda()
    grads, intens = [], []
    for save in (True, False):
        x = torch.from_numpy(x_np.copy()).cuda().requires_grad_()
        inten = tt.intensity(tt.Tensor(x, meta=_meta(_wl_arg(wls))), Z, save_field=save, **kw)
        (w * inten).sum().backward()
        grads.append(x.grad.cpu().numpy())
        intens.append(inten.detach().cpu().numpy())
    d = np.max(np.abs(grads[0] - grads[1])) / np.max(np.abs(grads[0]))
    print(f"{name}: save_field off against on {d:.3e} of max|grad|, gradients bit-equal "
          f"{np.array_equal(grads[0], grads[1])}, intensities bit-equal {np.array_equal(intens[0], intens[1])}")
    assert d <= FIELD_RTOL
    assert np.array_equal(intens[0], intens[1])      # hbx_intensity_real == hbx_simulate_real's intensity


def test_graph_only_with_a_gradient_request():
    import torchOptics.optics as tt
    x_np = _case("real")[0]
    x = torch.from_numpy(x_np.copy()).cuda()
    assert tt.intensity(tt.Tensor(x, meta=_meta()), Z).grad_fn is None
    xr = x.clone().requires_grad_()
    with torch.no_grad():
        out = tt.intensity(tt.Tensor(xr, meta=_meta()), Z)
    assert out.grad_fn is None and not out.requires_grad
    out_g = tt.intensity(tt.Tensor(xr, meta=_meta()), Z)
    assert out_g.grad_fn is not None
    assert torch.equal(out_g.detach(), out)          # the values are those of the plain call, bit for bit
    loss = out_g.sum()
    loss.backward()
    with pytest.raises(RuntimeError):                # the saved field is gone: torch's rule
        loss.backward()


def test_adam_descent_lowers_the_loss():
    import torch.nn.functional as Fn
    import torchOptics.optics as tt
    rng = np.random.default_rng(33)
    logits = torch.from_numpy((rng.random((2, 4, 64, 64), dtype=np.float32) - 0.5).astype(np.float32)).cuda()
    logits.requires_grad_()
    target = torch.from_numpy(rng.random((2, 1, 64, 64), dtype=np.float32)).cuda()
    opt = torch.optim.Adam([logits], lr=0.05)
    losses = []
    for _ in range(11):
        opt.zero_grad()
        x = torch.sigmoid(logits)
        loss = tt.relativeLoss(tt.intensity(tt.Tensor(x, meta=_meta()), Z), target, Fn.mse_loss)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("losses", " ".join(f"{v:.6f}" for v in losses))
    assert losses[-1] < losses[0]                    # the loss after ten steps against the first
