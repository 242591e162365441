"""tt.simulate_stack, tt.intensity_stack and tt.loss_stack: one hologram at D depths on the HIP path.

Forward: depth d of simulate_stack / intensity_stack is tt.simulate(.., binary=False) / tt.intensity at
zs[d], bit for bit, for a real, complex, phase, L-level and thresholded leaf.  loss_stack with
rel_scale="none" is the sum of D tt.loss calls times the pixel-count ratio 1 / D (MSE_RTOL).
Backward, end to end (the criterion of tests/test_gpu_shim_loss.py): the gradient of sum_b UP[b] loss_b
against the all-float64 chain from the samples (tests/test_focal_stack_host.stack_gradient and the leaf's
chain rule), next to the route the stack replaces -- autograd through D tt.intensity calls and torch ops
for the loss: both are float32 routes that differ in rounding order, so the stack's error may be at most
twice the other's.  Ten Adam steps on a two-depth, two-target problem lower the loss."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import hbx_oracle as O  # noqa: E402
from tests.test_focal_stack_host import stack_gradient  # noqa: E402
from tests.test_gpu_evaluate import INTEN_RTOL, MSE_RTOL  # noqa: E402
from tests.test_gpu_phase_field import FIELD_RTOL  # noqa: E402
from tests.test_loss_host import LOSS_MSE, REL_LSQ  # noqa: E402
from tests.test_phase_levels_host import quantize_np  # noqa: E402
from tests.test_threshold_ste_host import STE_WINDOW, binarize, field_values, ste_surrogate  # noqa: E402

WL = 515e-9
ZS = (2e-3, -1.5e-3, 2e-3)          # unequal, one repeated, one negative
UP = np.array([1.0, -0.5])
TAU, WIDTH, NLEVELS = 0.1, 0.5, 6


def _meta(wl=WL):
    return {"dx": (O.PIXEL_PITCH, O.PIXEL_PITCH), "wl": wl}


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm GPU")
    import hbx
    hbx.load_library()
    yield


# name: (shape, complex leaf, wavelengths, keywords of the leaf kind)
CASES = {
    "real": ((2, 4, 64, 64), False, (WL,), {}),
    "complex": ((2, 3, 64, 64), True, (WL,), {}),
    "phase": ((2, 3, 64, 64), False, (WL,), {"field": "phase"}),
    "levels": ((2, 3, 64, 64), False, (WL,), {"field": "phase", "levels": NLEVELS}),
    "threshold": ((2, 4, 64, 64), False, (WL,), {"threshold": TAU, "ste_width": WIDTH}),
    "threshold_phase": ((2, 4, 64, 64), False, (WL,), {"threshold": TAU, "ste_width": WIDTH, "field": "phase"}),
    "rgb": ((2, 6, 64, 64), False, tuple(O.WL_RGB), {}),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(x, target f32 [D, B, G, N, N] in [0, 1), transfer functions [D][G]), read-only"""
    shape, complex_leaf, wls, _ = CASES[name]
    b, c, n, _ = shape
    rng = np.random.default_rng(2700 + len(name) + c)
    x = (2 * rng.random(shape, dtype=np.float32) - 1).astype(np.float32)
    if complex_leaf:
        x = (x + 1j * (2 * rng.random(shape, dtype=np.float32) - 1).astype(np.float32)).astype(np.complex64)
    target = rng.random((len(ZS), b, len(wls), n, n), dtype=np.float32)
    hs = tuple(tuple(O.transfer_function(n, n, O.PIXEL_PITCH, O.PIXEL_PITCH, wl, z) for wl in wls) for z in ZS)
    x.setflags(write=False)
    target.setflags(write=False)
    return x, target, hs


def _wl_arg(wls):
    return wls[0] if len(wls) == 1 else tuple(wls)


def _x(tt, name, t):
    return tt.Tensor(t, meta=_meta(_wl_arg(CASES[name][2])))


# -- forward ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_forward_depths_are_the_single_depth_calls_bit_for_bit(name):
    import torchOptics.optics as tt
    shape, _, wls, kw = CASES[name]
    x_np, t_np, _ = _case(name)
    x, target = torch.from_numpy(x_np.copy()).cuda(), torch.from_numpy(t_np.copy()).cuda()
    fields = tt.simulate_stack(_x(tt, name, x), ZS, **kw)
    intens = tt.intensity_stack(_x(tt, name, x), ZS, **kw)
    assert fields.dtype == torch.complex64 and tuple(fields.shape) == (len(ZS),) + shape
    assert intens.dtype == torch.float32 and tuple(intens.shape) == (len(ZS), shape[0], len(wls)) + shape[2:]
    assert fields.grad_fn is None and intens.grad_fn is None
    for d, z in enumerate(ZS):
        pc = shape[1] // len(wls)       # tt.simulate takes one wavelength: colour group by colour group
        for k, wl in enumerate(wls):
            xg = tt.Tensor(x[:, k * pc:(k + 1) * pc].contiguous(), meta=_meta(wl))
            assert torch.equal(fields[d][:, k * pc:(k + 1) * pc], tt.simulate(xg, z, binary=False, **kw))
        single = tt.intensity(_x(tt, name, x), z, **kw)
        if CASES[name][1]:      # a complex x: tt.intensity forms |.|^2 and the mean as torch ops, in another order
            assert float((intens[d] - single).abs().max()) <= INTEN_RTOL * float(single.abs().max())
        else:
            assert torch.equal(intens[d], single)
    # rel_scale="none": the mean of the D per-depth losses
    got = tt.loss_stack(_x(tt, name, x), target, ZS, rel_scale="none", **kw)
    parts = sum(tt.loss(_x(tt, name, x), target[d], z, rel_scale="none", **kw) for d, z in enumerate(ZS))
    want = (parts / len(ZS)).cpu().numpy()
    assert got.dtype == torch.float64 and tuple(got.shape) == (shape[0],) and got.grad_fn is None
    assert np.all(np.abs(got.cpu().numpy() - want) <= MSE_RTOL * want)
    # a 3-D x drops the batch axis everywhere
    one = tt.loss_stack(_x(tt, name, x[1]), target[:, 1], ZS, **kw)
    full = tt.loss_stack(_x(tt, name, x), target, ZS, **kw)
    assert one.dim() == 0 and torch.equal(one, full[1])
    assert tuple(tt.simulate_stack(_x(tt, name, x[1]), ZS[:2], **kw).shape) == (2,) + shape[1:]
    # a graph gives the plain call's values
    xr = x.clone().requires_grad_()
    graph = tt.loss_stack(_x(tt, name, xr), target, ZS, **kw)
    assert graph.grad_fn is not None and torch.equal(graph.detach(), full)
    with torch.no_grad():
        assert tt.loss_stack(_x(tt, name, xr), target, ZS, **kw).grad_fn is None


# -- backward, end to end ----------------------------------------------------------------------------------
def _field64(name, x64):
    """the float64 field samples u [B, G, Pc, N, N] of the leaf and what turns dL/du into dL/dx"""
    shape, complex_leaf, wls, kw = CASES[name]
    b, c, n, _ = shape
    g = len(wls)
    fk = O.FIELD_PHASE if kw.get("field") == "phase" else O.FIELD_AMPLITUDE
    if "threshold" in kw:
        u = binarize(x64.astype(np.float32), np.float32(TAU), fk).astype(np.float64)
        lo, hi = float(np.float32(np.float32(TAU) - np.float32(WIDTH))), float(np.float32(np.float32(TAU) + np.float32(WIDTH)))
        s = ste_surrogate(x64, STE_WINDOW, lo, hi)
        back = lambda adj: field_values(fk)[1] * s * adj.real            # noqa: E731
    elif "levels" in kw:
        q = quantize_np(x64.astype(np.float32), NLEVELS)[2].astype(np.float64)
        u = np.exp(1j * np.pi * q)
        back = lambda adj: (np.conj(1j * np.pi * u) * adj).real          # noqa: E731
    elif fk == O.FIELD_PHASE:
        u = np.exp(1j * np.pi * x64)
        back = lambda adj: (np.conj(1j * np.pi * u) * adj).real          # noqa: E731
    elif complex_leaf:
        u, back = x64, (lambda adj: adj)
    else:
        u, back = x64, (lambda adj: adj.real)
    return u.reshape(b, g, c // g, n, n), back


def _stack_backward(tt, name, metric="mse", rel="lsq"):
    shape, _, _, kw = CASES[name]
    x_np, t_np, _ = _case(name)
    x = torch.from_numpy(x_np.copy()).cuda().requires_grad_()
    target = torch.from_numpy(t_np.copy()).cuda()
    loss = tt.loss_stack(_x(tt, name, x), target, ZS, metric=metric, rel_scale=rel, **kw)
    assert loss.grad_fn is not None
    (loss * torch.from_numpy(UP[:shape[0]].copy()).cuda()).sum().backward()
    assert x.grad is not None and x.grad.dtype == x.dtype and tuple(x.grad.shape) == shape
    return x.grad.cpu().numpy()


def _route_backward(tt, name):
    """the route the stack replaces: D tt.intensity calls, the least-squares MSE over the stack as torch ops"""
    shape, _, _, kw = CASES[name]
    x_np, t_np, _ = _case(name)
    x = torch.from_numpy(x_np.copy()).cuda().requires_grad_()
    target = torch.from_numpy(t_np.copy()).cuda()
    inten = torch.stack([tt.intensity(_x(tt, name, x), z, **kw) for z in ZS])          # [D, B, G, N, N]
    total = 0.0
    for e in range(shape[0]):
        i, t = inten[:, e], target[:, e]
        s = (i * t).sum() / (i * i).sum()
        total = total + float(UP[e]) * ((s * i - t) ** 2).mean()
    total.backward()
    return x.grad.cpu().numpy()


@pytest.mark.parametrize("name", list(CASES))
def test_gradient_reaches_every_leaf_kind_end_to_end(name):
    import torchOptics.optics as tt
    shape, complex_leaf, wls, kw = CASES[name]
    x_np, t_np, hs = _case(name)
    x64 = x_np.astype(np.complex128 if complex_leaf else np.float64)
    u64, back = _field64(name, x64)
    t64 = t_np.astype(np.float64)
    adj = np.stack([stack_gradient(u64[e], t64[:, e], hs, LOSS_MSE, REL_LSQ, False, UP[e]) for e in range(shape[0])])
    want = back(adj.reshape(x64.shape))
    new = _stack_backward(tt, name)
    route = _route_backward(tt, name)
    torch.cuda.synchronize()
    scale = np.max(np.abs(want))
    e_new, e_route = np.max(np.abs(new - want)) / scale, np.max(np.abs(route - want)) / scale
    print(f"FOCALSHIM {name}: end-to-end grad err of max|float64 grad| = {scale:.3e}: stack {e_new:.3e}, "
          f"D tt.intensity calls {e_route:.3e}")
    assert scale > 0.0
    assert e_new <= 2.0 * e_route


@pytest.mark.parametrize("name, metric, rel", [("real", "psnr", "lsq"), ("phase", "mse", "none"),
                                               ("complex", "psnr", "none")])
def test_gradient_of_the_other_metrics_is_finite_and_matches_autograd_of_the_intensities(name, metric, rel):
    """loss_stack's backward against autograd through intensity_stack and float64 torch ops for the same loss:
    both end in hbx_backward_stack on the same saved fields, with weights that differ by their float32
    rounding -- FIELD_RTOL of max|gradient|, the single-depth gradient tests' bound"""
    import torchOptics.optics as tt
    shape, _, _, kw = CASES[name]
    x_np, t_np, _ = _case(name)
    got = _stack_backward(tt, name, metric, rel)
    x = torch.from_numpy(x_np.copy()).cuda().requires_grad_()
    target = torch.from_numpy(t_np.copy()).cuda()
    inten = tt.intensity_stack(_x(tt, name, x), ZS, **kw)
    assert inten.grad_fn is not None
    total = 0.0
    for e in range(shape[0]):
        i, t = inten[:, e].double(), target[:, e].double()
        s = (i * t).sum() / (i * i).sum() if rel == "lsq" else 1.0
        mse = ((s * i - t) ** 2).mean()
        total = total + float(UP[e]) * (mse if metric == "mse" else 10.0 * torch.log10(1.0 / mse))
    total.backward()
    want = x.grad.cpu().numpy()
    scale = np.max(np.abs(want))
    err = np.max(np.abs(got - want)) / scale
    print(f"FOCALSHIM {name} {metric} {rel}: loss_stack vs autograd of intensity_stack {err:.3e}")
    assert np.isfinite(got).all() and scale > 0.0 and err <= FIELD_RTOL


def test_simulate_stack_backward_is_the_sum_of_the_adjoints():
    import torchOptics.optics as tt
    name = "phase"
    _, _, _, kw = CASES[name]
    x_np, _, _ = _case(name)
    rng = np.random.default_rng(5)
    gout = torch.from_numpy((rng.random((len(ZS),) + x_np.shape) - 0.5 + 1j * (rng.random((len(ZS),) + x_np.shape) - 0.5))
                            .astype(np.complex64)).cuda()
    x = torch.from_numpy(x_np.copy()).cuda().requires_grad_()
    out = tt.simulate_stack(_x(tt, name, x), ZS, **kw)
    assert out.grad_fn is not None
    torch.view_as_real(out * gout.conj()).select(-1, 0).sum().backward()        # Re <gout, out>
    xs = torch.from_numpy(x_np.copy()).cuda().requires_grad_()
    parts = sum(torch.view_as_real(tt.simulate(_x(tt, name, xs), z, binary=False, **kw) * gout[d].conj()).select(-1, 0).sum()
                for d, z in enumerate(ZS))
    parts.backward()
    a, b = x.grad.cpu().numpy(), xs.grad.cpu().numpy()
    assert np.max(np.abs(a - b)) <= FIELD_RTOL * np.max(np.abs(b))


# -- descent -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaf", ["amplitude", "phase"])
def test_adam_descent_lowers_the_stack_loss(leaf):
    """64 x 64, two depths, two different targets, ten Adam steps"""
    import torchOptics.optics as tt
    rng = np.random.default_rng(44)
    logits = torch.from_numpy((rng.random((2, 4, 64, 64), dtype=np.float32) - 0.5).astype(np.float32)).cuda()
    logits.requires_grad_()
    target = torch.from_numpy(rng.random((2, 2, 1, 64, 64), dtype=np.float32)).cuda()
    zs = (2e-3, 3.5e-3)
    opt = torch.optim.Adam([logits], lr=0.05)
    losses = []
    for _ in range(11):
        opt.zero_grad()
        if leaf == "amplitude":
            loss = tt.loss_stack(tt.Tensor(torch.sigmoid(logits), meta=_meta()), target, zs).sum()
        else:
            loss = tt.loss_stack(tt.Tensor(logits, meta=_meta()), target, zs, field="phase").sum()
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    losses = [float(v) for v in losses]
    print(leaf, "stack losses", " ".join(f"{v:.6f}" for v in losses))
    assert losses[-1] < losses[0]


def test_plan_cache_key_holds_the_depths():
    import torchOptics.optics as tt
    name = "real"
    x_np, _, _ = _case(name)
    x = torch.from_numpy(x_np.copy()).cuda()
    a = tt.intensity_stack(_x(tt, name, x), (2e-3, 3e-3))
    b = tt.intensity_stack(_x(tt, name, x), (2e-3, 4e-3))        # same first depth, another stack
    assert torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1])
    keys = [k for k in tt._PLANS if k[-1] in ((2e-3, 3e-3), (2e-3, 4e-3))]
    assert len(keys) == 2
    assert torch.equal(tt.intensity(_x(tt, name, x), 2e-3), a[0])  # the single-depth plan for z = 2e-3 is its own
