"""field="phase" on real leaves through tt.simulate / tt.intensity / tt.loss: the fused route.

The shim hands the float32 samples x to hbx_simulate_phase / hbx_evaluate_phase (u = exp(i pi x) formed
in the first pass's load) and takes dL/dx from the last pass of hbx_phase_backward; no torch op forms
u or walks back through it.  Checked here against the float64 oracle from the samples (forward within
the project's bounds, gradient within 2e-5 of max|want|) and against the parent route -- the complex
leaf torch.complex(cos(x * float32(pi)), sin(..)) handed to the same call with field="amplitude",
which is what field="phase" ran before -- whose gradient error the fused route may at most double."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import hbx_oracle as O  # noqa: E402
from tests.test_loss_host import LOSS_MSE, LOSS_PSNR, REL_LSQ, REL_NONE, loss_gradient  # noqa: E402

Z = 2e-3
WL = 515e-9
FIELD_RTOL = 2e-5
PSNR_ATOL = 1e-4
MSE_RTOL = 2.31e-5
KIND = {"mse": LOSS_MSE, "psnr": LOSS_PSNR}
REL = {"lsq": REL_LSQ, "none": REL_NONE}
UP = np.array([1.0, -0.5])      # per-env upstream gradients that differ

# name: (shape [B, C, N, N], wavelengths)
SHAPES = {
    "mono": ((2, 2, 64, 64), (WL,)),
    "rgb": ((2, 6, 64, 64), tuple(O.WL_RGB)),
    "odd": ((2, 3, 64, 64), (WL,)),               # odd C with G = 1
    "rgb_odd": ((2, 3, 64, 64), tuple(O.WL_RGB)),  # C / G = 1 with G = 3
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
    """x float32 [B, C, N, N] in [-1, 1); u64 = exp(i pi x64) [B, G, Q, N, N]; target f32 [B, G, N, N];
    a complex upstream w [B, C, N, N] and a real one gi [B, G, N, N]; the G transfer functions; the
    float64 field [B, G, Q, N, N] and intensity [B, G, N, N].  Read-only."""
    shape, wls = SHAPES[name]
    b, c, n, _ = shape
    g = len(wls)
    rng = np.random.default_rng(3100 + len(name) + c)
    x = (2 * rng.random(shape, dtype=np.float32) - 1).astype(np.float32)
    u64 = np.exp(1j * np.pi * x.astype(np.float64)).reshape(b, g, c // g, n, n)
    target = rng.random((b, g, n, n), dtype=np.float32)
    w = ((2 * rng.random(shape, dtype=np.float32) - 1) + 1j * (2 * rng.random(shape, dtype=np.float32) - 1))
    w = w.astype(np.complex64)
    gi = (2 * rng.random((b, g, n, n), dtype=np.float32) - 1).astype(np.float32)
    hs = tuple(O.transfer_function(n, n, O.PIXEL_PITCH, O.PIXEL_PITCH, wl, Z, O.TF_ASM) for wl in wls)
    field = np.stack([np.stack([O.propagate(u64[e, k], hs[k]) for k in range(g)]) for e in range(b)])
    inten = np.mean(field.real ** 2 + field.imag ** 2, axis=2)
    out = (x, u64, target, w, gi, hs, field, inten)
    for a in out[:5] + hs + out[6:]:
        a.setflags(write=False)
    return out


def _chain(name, adj):
    """dL/dx from dL/du [B, G, Q, N, N] (float64), the formula of include/hbx.h"""
    x, u64 = _case(name)[:2]
    return (np.conj(1j * np.pi * u64) * adj).real.reshape(x.shape)


def _leaf(name, dtype):
    return torch.from_numpy(_case(name)[0].copy()).to(dtype).cuda().requires_grad_()


def _parent_u(x):
    """the complex leaf the parent formed with torch ops"""
    ph = x.to(torch.float32) * np.float32(np.pi)
    return torch.complex(torch.cos(ph), torch.sin(ph))


def _grad_pair(run, name, dtype):
    """x.grad through the fused route and through the parent route of scalar = run(input, kw)"""
    out = []
    for parent in (False, True):
        x = _leaf(name, dtype)
        run(_parent_u(x) if parent else x, {} if parent else {"field": "phase"}).backward()
        torch.cuda.synchronize()
        assert x.grad is not None and x.grad.dtype == dtype and tuple(x.grad.shape) == tuple(x.shape)
        out.append(x.grad.cpu().numpy().astype(np.float64))
    return out


def _check_gradient(label, new, parent, want):
    scale = np.max(np.abs(want))
    e_new, e_par = np.max(np.abs(new - want)) / scale, np.max(np.abs(parent - want)) / scale
    print(f"{label}: grad err of max|want| = {scale:.3e}: fused {e_new:.3e}, parent route {e_par:.3e}")
    assert scale > 0.0
    assert e_new <= FIELD_RTOL
    assert e_new <= 2.0 * e_par


# -- 10. simulate --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", ["mono", "odd"])
def test_simulate_phase_leaf(name, dtype):
    import torchOptics.optics as tt
    shape, wls = SHAPES[name]
    x_np, _, _, w_np, _, hs, field64, _ = _case(name)
    meta = _meta(wls)
    plain = tt.simulate(tt.Tensor(torch.from_numpy(x_np.copy()).to(dtype).cuda(), meta=meta), Z, binary=False,
                        field="phase")
    xr = _leaf(name, dtype)
    with torch.no_grad():
        quiet = tt.simulate(tt.Tensor(xr, meta=meta), Z, binary=False, field="phase")
    graph = tt.simulate(tt.Tensor(xr, meta=meta), Z, binary=False, field="phase")
    torch.cuda.synchronize()
    assert plain.dtype == torch.complex64 and tuple(plain.shape) == shape
    assert plain.grad_fn is None and quiet.grad_fn is None and graph.grad_fn is not None
    assert torch.equal(torch.view_as_real(graph.detach()), torch.view_as_real(plain))
    assert torch.equal(torch.view_as_real(quiet), torch.view_as_real(plain))
    want_f = field64.reshape(shape)
    e = np.max(np.abs(plain.cpu().numpy() - want_f)) / np.max(np.abs(want_f))
    print(f"simulate {name} {dtype}: field err {e:.3e} of max|field|")
    assert e <= FIELD_RTOL

    w = torch.from_numpy(w_np.copy()).cuda()

    def run(inp, kw):     # L = Re <w, F>: dL/dF = w in torch's convention
        f = tt.simulate(tt.Tensor(inp, meta=meta), Z, binary=False, **kw)
        return (torch.view_as_real(f) * torch.view_as_real(w)).sum()
    new, parent = _grad_pair(run, name, dtype)
    adj = np.stack([O.propagate(w_np[e_].astype(np.complex128), np.conj(hs[0])) for e_ in range(shape[0])])
    _check_gradient(f"simulate {name} {dtype}", new, parent, _chain(name, adj.reshape(_case(name)[1].shape)))


# -- 10. intensity -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, dtype", [("mono", torch.float32), ("mono", torch.float64), ("rgb", torch.float32),
                                         ("odd", torch.float32)], ids=["mono-f32", "mono-f64", "rgb-f32", "odd-f32"])
def test_intensity_phase_leaf(name, dtype):
    import torchOptics.optics as tt
    shape, wls = SHAPES[name]
    x_np, _, _, _, gi_np, hs, field64, inten64 = _case(name)
    b, c, n, _ = shape
    g = len(wls)
    meta = _meta(wls)
    plain = tt.intensity(tt.Tensor(torch.from_numpy(x_np.copy()).to(dtype).cuda(), meta=meta), Z, field="phase")
    xr = _leaf(name, dtype)
    with torch.no_grad():
        quiet = tt.intensity(tt.Tensor(xr, meta=meta), Z, field="phase")
    graph = tt.intensity(tt.Tensor(xr, meta=meta), Z, field="phase")
    torch.cuda.synchronize()
    assert plain.dtype == torch.float32 and tuple(plain.shape) == (b, g, n, n)
    assert plain.grad_fn is None and quiet.grad_fn is None and graph.grad_fn is not None
    assert torch.equal(graph.detach(), plain) and torch.equal(quiet, plain)
    e = np.max(np.abs(plain.cpu().numpy() - inten64)) / np.max(inten64)
    print(f"intensity {name} {dtype}: err {e:.3e} of max I")
    assert e <= FIELD_RTOL

    gi = torch.from_numpy(gi_np.copy()).cuda()

    def run(inp, kw):
        return (tt.intensity(tt.Tensor(inp, meta=meta), Z, **kw) * gi).sum()
    new, parent = _grad_pair(run, name, dtype)
    pc = c // g
    adj = np.stack([np.stack([O.propagate((2.0 / pc) * gi_np[e_, k].astype(np.float64) * field64[e_, k],
                                          np.conj(hs[k])) for k in range(g)]) for e_ in range(b)])
    _check_gradient(f"intensity {name} {dtype}", new, parent, _chain(name, adj))


# -- 10. loss ------------------------------------------------------------------------------------------
LOSS_CASES = [("mono", "mse", "lsq", torch.float32), ("mono", "psnr", "lsq", torch.float32),
              ("mono", "mse", "none", torch.float32), ("mono", "mse", "lsq", torch.float64),
              ("rgb", "mse", "lsq", torch.float32), ("odd", "psnr", "lsq", torch.float32),
              ("rgb_odd", "mse", "lsq", torch.float32), ("rgb_odd", "psnr", "none", torch.float64)]


@pytest.mark.parametrize("name, metric, rel, dtype", LOSS_CASES,
                         ids=[f"{a}-{m}-{r}-{'f64' if d == torch.float64 else 'f32'}" for a, m, r, d in LOSS_CASES])
def test_loss_phase_leaf(name, metric, rel, dtype):
    import torchOptics.optics as tt
    shape, wls = SHAPES[name]
    x_np, _, t_np, _, _, hs, field64, inten64 = _case(name)
    b = shape[0]
    meta = _meta(wls)
    target = torch.from_numpy(t_np.copy()).cuda()

    def call(inp, kw):
        return tt.loss(tt.Tensor(inp, meta=meta), target, Z, metric=metric, rel_scale=rel, **kw)
    plain = call(torch.from_numpy(x_np.copy()).to(dtype).cuda(), {"field": "phase"})
    xr = _leaf(name, dtype)
    with torch.no_grad():
        quiet = call(xr, {"field": "phase"})
    graph = call(xr, {"field": "phase"})
    torch.cuda.synchronize()
    assert plain.dtype == torch.float64 and tuple(plain.shape) == (b,)
    assert plain.grad_fn is None and quiet.grad_fn is None and graph.grad_fn is not None
    assert torch.equal(graph.detach(), plain) and torch.equal(quiet, plain)
    got = plain.cpu().numpy()
    for e in range(b):
        t64 = t_np[e].astype(np.float64)
        if metric == "mse":
            want = O.relative_mse(inten64[e], t64, REL[rel])
            print(f"loss {name} env {e}: MSE rel err {abs(got[e] - want) / want:.2e}")
            assert abs(got[e] - want) <= MSE_RTOL * want
        else:
            want = O.relative_psnr(inten64[e], t64, REL[rel])
            print(f"loss {name} env {e}: PSNR err {abs(got[e] - want):.2e} dB")
            assert abs(got[e] - want) <= PSNR_ATOL

    up = torch.from_numpy(UP[:b].copy()).cuda()
    new, parent = _grad_pair(lambda inp, kw: (call(inp, kw) * up).sum(), name, dtype)
    adj = np.stack([loss_gradient(field64[e], inten64[e], t_np[e].astype(np.float64), hs, KIND[metric], REL[rel],
                                  False, UP[e]) for e in range(b)])
    _check_gradient(f"loss {name} {metric} {rel} {dtype}", new, parent, _chain(name, adj))


# -- 11. descent ---------------------------------------------------------------------------------------
def test_adam_descent_on_a_phase_hologram_lowers_the_loss():
    import torchOptics.optics as tt
    rng = np.random.default_rng(34)
    x = torch.from_numpy((2 * rng.random((2, 4, 64, 64), dtype=np.float32) - 1).astype(np.float32)).cuda()
    x.requires_grad_()
    target = torch.from_numpy(rng.random((2, 1, 64, 64), dtype=np.float32)).cuda()
    opt = torch.optim.Adam([x], lr=0.05)
    losses = []
    for _ in range(11):
        opt.zero_grad()
        loss = tt.loss(tt.Tensor(x, meta=_meta((WL,))), target, Z, field="phase").sum()
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    losses = [float(v) for v in losses]
    print("phase losses", " ".join(f"{v:.6f}" for v in losses))
    assert losses[-1] < losses[0]                    # the loss after ten steps against the first


# -- 12. peak memory -----------------------------------------------------------------------------------
def test_fused_route_allocates_less_than_the_parent_route():
    """One forward + backward of tt.loss at 256 x 256, 8 phase planes, B = 8: the fused route allocates
    none of ph, cos, sin, u or the complex gradient, so its peak is strictly below the parent route's."""
    import torchOptics.optics as tt
    rng = np.random.default_rng(35)
    x_np = (2 * rng.random((8, 8, 256, 256), dtype=np.float32) - 1).astype(np.float32)
    target = torch.from_numpy(rng.random((8, 1, 256, 256), dtype=np.float32)).cuda()
    meta = _meta((WL,))
    x = torch.from_numpy(x_np).cuda().requires_grad_()

    def step(parent):
        inp, kw = (_parent_u(x), {}) if parent else (x, {"field": "phase"})
        tt.loss(tt.Tensor(inp, meta=meta), target, Z, **kw).sum().backward()
        torch.cuda.synchronize()

    peaks = {}
    for parent in (False, True, False, True):          # the first pair builds the plans and warms the allocator
        x.grad = None
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        step(parent)
        peaks[parent] = torch.cuda.max_memory_allocated() - base
    print(f"peak over one forward + backward: fused {peaks[False] / 2**20:.1f} MiB, parent {peaks[True] / 2**20:.1f} MiB")
    assert peaks[False] < peaks[True]
