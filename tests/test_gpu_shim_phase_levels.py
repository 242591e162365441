"""levels=L with field="phase" through tt.simulate / tt.intensity / tt.loss: the quantized phase leaf.

The shim hands the float32 samples x to hbx_simulate_phase_levels / hbx_evaluate_phase_levels, whose first
pass quantizes them to L levels on load, and takes the straight-through gradient from the last pass of
hbx_phase_levels_backward.  The contract is the C-ABI's, bit for bit: the result of a call with levels=L is
the same call's without levels on a leaf that holds q = hbx.quantize_phase(x, L, want_samples=True), and
x.grad is that leaf's gradient.  Then an Adam run on a 4-level hologram, and the memory the fused route
saves against the torch-op route (quantize with torch ops, the detach trick, the continuous call)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import hbx_oracle as O  # noqa: E402
from tests.test_gpu_phase_levels import samples  # noqa: E402

Z = 2e-3
WL = 515e-9
F32 = np.float32
# name: (shape [B, C, N, N], wavelengths)
SHAPES = {"64rgb": ((2, 6, 64, 64), tuple(O.WL_RGB)), "256mono": ((1, 2, 256, 256), (WL,))}
DTYPES = [torch.float32, torch.float64]


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm GPU")
    import hbx
    hbx.load_library()
    yield


def _meta(wls):
    return {"dx": (O.PIXEL_PITCH, O.PIXEL_PITCH), "wl": wls[0] if len(wls) == 1 else tuple(wls)}


def _leaves(name, dtype, levels, mono=False):
    """(x, q): two leaves of `dtype` that require grad -- the samples, and their quantized values from
    hbx.quantize_phase of the float32 the shim casts them to -- both tt.Tensors with the case's meta"""
    import hbx
    import torchOptics.optics as tt
    shape, wls = SHAPES[name]
    if mono:
        wls = (WL,)
    x32 = torch.from_numpy(samples(shape, levels, 4100 + shape[-1] + shape[1])).cuda()
    q32 = hbx.quantize_phase(x32, levels, want_levels=False, want_samples=True)
    assert not torch.equal(q32, x32)
    x = x32.to(dtype).requires_grad_()
    q = q32.to(dtype).requires_grad_()
    wrap = lambda t: tt.Tensor(t, meta=_meta(wls))   # noqa: E731
    return x, q, wrap, len(wls)


def _same(a, b):
    if a.is_complex():
        a, b = torch.view_as_real(a), torch.view_as_real(b)
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def _check_pair(run, x, q, wrap, dtype):
    """run(leaf, kw) -> (result, scalar): with levels on x against without on q, results and gradients"""
    out_x, s_x = run(wrap(x), {"levels": 4})
    out_q, s_q = run(wrap(q), {})
    assert out_x.grad_fn is not None
    s_x.backward()
    s_q.backward()
    torch.cuda.synchronize()
    assert _same(out_x.detach(), out_q.detach())
    assert x.grad is not None and x.grad.dtype == dtype and x.grad.shape == x.shape
    assert bool((x.grad != 0).any()) and bool(torch.isfinite(x.grad).all())
    assert _same(x.grad, q.grad)
    with torch.no_grad():
        plain, _ = run(wrap(x), {"levels": 4})
    free, _ = run(wrap(x.detach()), {"levels": 4})
    torch.cuda.synchronize()
    assert plain.grad_fn is None and free.grad_fn is None and not free.requires_grad
    assert _same(plain, out_q.detach()) and _same(free, out_q.detach())


# -- 8. the three entry points -------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_simulate_levels_is_simulate_on_q(name, dtype):
    import torchOptics.optics as tt
    x, q, wrap, _ = _leaves(name, dtype, 4, mono=True)      # simulate takes one wavelength per call
    rng = np.random.default_rng(4200)
    w = torch.from_numpy((rng.random(x.shape, dtype=F32) + 1j * rng.random(x.shape, dtype=F32) - 0.5)
                         .astype(np.complex64)).cuda()

    def run(leaf, kw):
        out = tt.simulate(leaf, Z, binary=False, field="phase", **kw)
        out = out.as_subclass(torch.Tensor)
        assert out.dtype == torch.complex64 and out.shape == x.shape
        return out, (out * w).real.sum()
    _check_pair(run, x, q, wrap, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_intensity_levels_is_intensity_on_q(name, dtype):
    import torchOptics.optics as tt
    x, q, wrap, g = _leaves(name, dtype, 4)
    b, _, n, _ = x.shape
    gi = torch.from_numpy(np.random.default_rng(4300).random((b, g, n, n), dtype=F32) - F32(0.5)).cuda()

    def run(leaf, kw):
        out = tt.intensity(leaf, Z, field="phase", **kw).as_subclass(torch.Tensor)
        assert out.dtype == torch.float32 and tuple(out.shape) == (b, g, n, n)
        return out, (out * gi).sum()
    _check_pair(run, x, q, wrap, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("rel", ["lsq", "none"])
@pytest.mark.parametrize("metric", ["mse", "psnr"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_loss_levels_is_loss_on_q(name, metric, rel, dtype):
    import torchOptics.optics as tt
    x, q, wrap, g = _leaves(name, dtype, 4)
    b, _, n, _ = x.shape
    target = torch.from_numpy(np.random.default_rng(4400).random((b, g, n, n), dtype=F32)).cuda()
    up = torch.tensor([1.0, -0.5][:b], dtype=torch.float64, device="cuda")

    def run(leaf, kw):
        out = tt.loss(leaf, target, Z, metric=metric, rel_scale=rel, field="phase", **kw).as_subclass(torch.Tensor)
        assert out.dtype == torch.float64 and tuple(out.shape) == (b,)
        return out, (out * up).sum()
    _check_pair(run, x, q, wrap, dtype)


def test_three_dimensional_input_and_the_argument_errors_on_the_gpu():
    """[C, H, W] in, [C, H, W] out; and the refusals hold with a GPU present too (tests/test_phase_levels_host.py
    has them without one)"""
    import hbx
    import torchOptics.optics as tt
    x32 = torch.from_numpy(samples((2, 64, 64), 4, 4500)).cuda()
    x = tt.Tensor(x32, meta=_meta((WL,)))
    q = tt.Tensor(hbx.quantize_phase(x32, 4, want_levels=False, want_samples=True), meta=_meta((WL,)))
    a = tt.simulate(x, Z, binary=False, field="phase", levels=4)
    b = tt.simulate(q, Z, binary=False, field="phase")
    torch.cuda.synchronize()
    assert tuple(a.shape) == (2, 64, 64) and _same(a.as_subclass(torch.Tensor), b.as_subclass(torch.Tensor))
    for kw in (dict(levels=4), dict(levels=4, field="phase", threshold=0.0), dict(levels=4, field="phase", grid=256),
               dict(levels=1, field="phase"), dict(levels=2.0, field="phase")):
        with pytest.raises(ValueError):
            tt.intensity(x, Z, **kw)
    with pytest.raises(ValueError):
        tt.simulate(x, Z, field="phase", levels=4)           # binary=True
    torch.cuda.synchronize()


# -- 9. an optimiser run on the displayed hologram -----------------------------------------------------
def test_adam_on_a_four_level_hologram_lowers_its_loss():
    """64 x 64, two phase planes, 30 Adam steps on the loss of the 4-level hologram itself (the
    straight-through gradient): the loss through levels=4 ends below where it began, and it is the loss of
    the exported hologram -- tt.loss on hbx.quantize_phase's q."""
    import hbx
    import torchOptics.optics as tt
    meta = _meta((WL,))
    rng = np.random.default_rng(4600)
    goal = torch.from_numpy(rng.integers(0, 4, (1, 2, 64, 64)).astype(F32) * F32(0.5)).cuda()
    with torch.no_grad():
        target = tt.intensity(tt.Tensor(goal, meta=meta), Z, field="phase").as_subclass(torch.Tensor).clone()
    x = torch.from_numpy((2 * rng.random((1, 2, 64, 64), dtype=F32) - 1)).cuda().requires_grad_()
    opt = torch.optim.Adam([x], lr=0.05)

    def displayed_loss():
        with torch.no_grad():
            return float(tt.loss(tt.Tensor(x.detach(), meta=meta), target, Z, field="phase", levels=4)[0])
    first = displayed_loss()
    for _ in range(30):
        opt.zero_grad()
        tt.loss(tt.Tensor(x, meta=meta), target, Z, field="phase", levels=4).sum().backward()
        opt.step()
    last = displayed_loss()
    q = hbx.quantize_phase(x.detach(), 4, want_levels=False, want_samples=True)
    with torch.no_grad():
        of_q = float(tt.loss(tt.Tensor(q, meta=meta), target, Z, field="phase")[0])
    torch.cuda.synchronize()
    print(f"4-level hologram, 30 Adam steps: relative MSE {first:.6e} -> {last:.6e}; on the exported q {of_q:.6e}")
    assert np.isfinite(first) and np.isfinite(last)
    assert last < first
    assert last == of_q


# -- 10. memory ----------------------------------------------------------------------------------------
def _torch_quantize(x, levels):
    """the quantizer by torch ops: what a user writes without the fused route"""
    r = x - 2.0 * torch.round(x * 0.5)
    return torch.round(r * F32(levels / 2)) * F32(2.0 / levels)


def test_fused_route_peaks_below_the_torch_op_route():
    """One forward-backward pair of tt.loss at 256 x 256, B = 4, four phase planes each.  The torch-op route
    materialises the quantized leaf -- at least one N^2 float32 tensor per plane that the fused route never
    writes -- so its peak above the resident set is strictly higher."""
    import torchOptics.optics as tt
    meta = _meta((WL,))
    shape = (4, 4, 256, 256)
    x0 = torch.from_numpy(samples(shape, 4, 4700)).cuda()
    target = torch.from_numpy(np.random.default_rng(4701).random((4, 1, 256, 256), dtype=F32)).cuda()

    def fused(x):
        return tt.loss(tt.Tensor(x, meta=meta), target, Z, field="phase", levels=4).sum()

    def torch_ops(x):
        xq = x + (_torch_quantize(x, 4) - x).detach()
        return tt.loss(tt.Tensor(xq, meta=meta), target, Z, field="phase").sum()

    def peak(route):
        x = x0.clone().requires_grad_()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        route(x).backward()
        torch.cuda.synchronize()
        assert x.grad is not None
        return torch.cuda.max_memory_allocated() - base, x.grad

    for route in (fused, torch_ops):     # plans and their workspaces exist before anything is measured
        peak(route)
    p_fused, g_fused = peak(fused)
    p_torch, g_torch = peak(torch_ops)
    plane_bytes = 4 * x0.numel()
    print(f"peak above the resident set: fused {p_fused} B, torch ops {p_torch} B (+{p_torch - p_fused}); "
          f"one float32 copy of x is {plane_bytes} B")
    assert p_fused < p_torch
    assert bool(torch.isfinite(g_fused).all()) and bool(torch.isfinite(g_torch).all())
