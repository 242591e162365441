"""source= on tt.simulate / tt.intensity / tt.loss: the fused route under an illumination field.

The shim hands the leaf and the complex64 source [G, H, W] to hbx_evaluate_source (u = s f(x) formed in the
first pass's load) and takes the leaf's gradient from the last pass of hbx_backward_source; no torch op forms
u or walks back through it.  Checked against the float64 chain of tests/_source_model.py from the float32
samples: the forward within the siblings' bounds (FIELD_RTOL, MSE_RTOL, PSNR_ATOL), x.grad within FIELD_RTOL
of max|want|.  64 x 64 with G = 3 (simulate: one wavelength), one case at 256 x 256 mono."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import hbx_oracle as O  # noqa: E402
from tests import _source_model as M  # noqa: E402
from tests.test_loss_host import LOSS_MSE, LOSS_PSNR, REL_LSQ, loss_gradient  # noqa: E402

Z = 2e-3
WL = 515e-9
FIELD_RTOL = 2e-5
PSNR_ATOL = 1e-4
MSE_RTOL = 2.31e-5
TAU, WIDTH, LEVELS = 0.5, 0.25, 8
VA, VB = 1.0, -2.0              # threshold= with field="phase": u = 1 - 2 [x >= tau]
UP = np.array([1.0, -0.5])      # per-env upstream gradients that differ
KINDS = ["real", "threshold", "complex", "phase", "levels"]
KW = {"real": {}, "complex": {}, "phase": dict(field="phase"), "levels": dict(field="phase", levels=LEVELS),
      "threshold": dict(field="phase", threshold=TAU, ste="window", ste_width=WIDTH)}

# name: (shape [B, C, N, N], wavelengths)
SHAPES = {"mono": ((2, 2, 64, 64), (WL,)), "rgb": ((2, 6, 64, 64), tuple(O.WL_RGB)), "mono256": ((1, 2, 256, 256), (WL,)),
          "odd": ((2, 3, 64, 64), (WL,))}               # an odd C: no padding plane under a source


def _meta(wls):
    return {"dx": (O.PIXEL_PITCH, O.PIXEL_PITCH), "wl": wls[0] if len(wls) == 1 else tuple(wls)}


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm GPU")
    import hbx
    hbx.load_library()
    yield


def _ocfg(name, kind="complex"):
    (b, c, n, _), wls = SHAPES[name]
    return O.OpticsConfig(n, n, len(wls), 2 * c // len(wls), wls, z=Z,
                          field_kind=O.FIELD_PHASE if kind == "threshold" else O.FIELD_AMPLITUDE)


@functools.lru_cache(maxsize=None)
def _source(name):
    """complex64 [G, N, N]: a Gaussian envelope times a tilt that differs per group, 0 outside r <= 0.4 N"""
    (_, _, n, _), wls = SHAPES[name]
    yy, xx = np.mgrid[:n, :n].astype(np.float64) - (n - 1) / 2.0
    r2 = xx ** 2 + yy ** 2
    s = np.stack([np.exp(-r2 / (0.3 * n) ** 2) * np.exp(2j * np.pi * ((0.11 + 0.05 * k) * xx - (0.07 + 0.03 * k) * yy))
                  for k in range(len(wls))])
    s[:, r2 > (0.4 * n) ** 2] = 0.0
    s = s.astype(np.complex64)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def _case(name, kind):
    """x [B, C, N, N] (phase in [-1, 1), real in [0, 1), complex in the square), target f32 [B, G, N, N], a
    complex upstream w [B, C, N, N] and a real one gi [B, G, N, N]; read-only"""
    shape, wls = SHAPES[name]
    b, c, n, _ = shape
    g = len(wls)
    rng = np.random.default_rng(5100 + 3 * len(name) + KINDS.index(kind))
    if kind == "complex":
        x = ((2 * rng.random(shape, dtype=np.float32) - 1) + 1j * (2 * rng.random(shape, dtype=np.float32) - 1)).astype(np.complex64)
    elif kind in ("phase", "levels"):
        x = (2 * rng.random(shape, dtype=np.float32) - 1).astype(np.float32)
    else:
        x = rng.random(shape, dtype=np.float32)
    target = rng.random((b, g, n, n), dtype=np.float32)
    w = ((2 * rng.random(shape, dtype=np.float32) - 1) + 1j * (2 * rng.random(shape, dtype=np.float32) - 1)).astype(np.complex64)
    gi = (2 * rng.random((b, g, n, n), dtype=np.float32) - 1).astype(np.float32)
    for a in (x, target, w, gi):
        a.setflags(write=False)
    return x, target, w, gi


def _model(name, kind):
    """per env: (u64, field [G Q, N, N], intensity [G, N, N], the leaf keywords of M.leaf_gradient)"""
    import hbx
    x = _case(name, kind)[0]
    ocfg, s = _ocfg(name, kind), _source(name)
    qs = None
    if kind == "levels":
        qs = hbx.quantize_phase(torch.from_numpy(x.copy()).cuda(), LEVELS, want_levels=False, want_samples=True).cpu().numpy()
    out = []
    for e in range(x.shape[0]):
        u = M.sourced(kind, x[e], s, q=None if qs is None else qs[e], tau=TAU, va=VA, vb=VB)
        f = M.forward(ocfg, u)
        leaf = dict(x=x[e], q=None if qs is None else qs[e], vb=VB, surrogate="window", p0=TAU - WIDTH, p1=TAU + WIDTH)
        out.append((u, f, M.intensity(ocfg, f), leaf))
    return out


def _leaf_grad(name, kind, e, adj, leaf):
    """the leaf's gradient of env e from dL/du = adj [G Q, N, N] (already back-propagated)"""
    q = adj.shape[0] // len(SHAPES[name][1])
    gp = np.conj(M.per_plane(_source(name).astype(np.complex128), q)) * adj
    return M.leaf_gradient(kind, gp, **leaf)


def _leaf(name, kind, dtype=None):
    x = torch.from_numpy(_case(name, kind)[0].copy())
    if dtype is not None:
        x = x.to(dtype)
    return x.cuda().requires_grad_()


def _check_grad(label, x, want):
    got = x.grad.cpu().numpy()
    assert np.iscomplexobj(got) == np.iscomplexobj(want)
    scale = float(np.max(np.abs(want)))
    e = float(np.max(np.abs(got - want))) / scale
    print(f"{label}: grad err {e:.3e} of max|want| = {scale:.3e}")
    assert scale > 0.0 and tuple(got.shape) == tuple(want.shape)
    assert e <= FIELD_RTOL


# -- simulate ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_simulate_with_a_source(kind):
    import torchOptics.optics as tt
    name = "mono"
    shape, wls = SHAPES[name]
    x_np, _, w_np, _ = _case(name, kind)
    meta, s = _meta(wls), torch.from_numpy(_source(name).copy())
    model = _model(name, kind)
    plain = tt.simulate(tt.Tensor(torch.from_numpy(x_np.copy()).cuda(), meta=meta), Z, binary=False, source=s, **KW[kind])
    torch.cuda.synchronize()
    assert plain.dtype == torch.complex64 and tuple(plain.shape) == shape and plain.grad_fn is None
    want_f = np.stack([m[1] for m in model])
    e = np.max(np.abs(plain.cpu().numpy() - want_f)) / np.max(np.abs(want_f))
    print(f"simulate {kind}: field err {e:.3e} of max|field|")
    assert e <= FIELD_RTOL
    x = _leaf(name, kind)
    f = tt.simulate(tt.Tensor(x, meta=meta), Z, binary=False, source=s.cuda(), **KW[kind])
    assert f.grad_fn is not None and torch.equal(torch.view_as_real(f.detach()), torch.view_as_real(plain))
    (torch.view_as_real(f) * torch.view_as_real(torch.from_numpy(w_np.copy()).cuda())).sum().backward()   # L = Re <w, F>
    torch.cuda.synchronize()
    ocfg = _ocfg(name, kind)
    want = np.stack([_leaf_grad(name, kind, e_, M.adjoint(ocfg, w_np[e_].astype(np.complex128)), model[e_][3])
                     for e_ in range(shape[0])])
    _check_grad(f"simulate {kind}", x, want)


# -- intensity --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_intensity_with_a_source(kind):
    import torchOptics.optics as tt
    name = "rgb"
    shape, wls = SHAPES[name]
    g, q = len(wls), shape[1] // len(wls)
    x_np, _, _, gi_np = _case(name, kind)
    meta, s = _meta(wls), torch.from_numpy(_source(name).copy())
    model = _model(name, kind)
    x = _leaf(name, kind)
    with torch.no_grad():
        quiet = tt.intensity(tt.Tensor(x, meta=meta), Z, source=s, **KW[kind])
    inten = tt.intensity(tt.Tensor(x, meta=meta), Z, source=s, **KW[kind])
    torch.cuda.synchronize()
    assert quiet.grad_fn is None and inten.grad_fn is not None and torch.equal(quiet, inten.detach())
    want_i = np.stack([m[2] for m in model])
    e = np.max(np.abs(inten.detach().cpu().numpy() - want_i)) / np.max(want_i)
    print(f"intensity {kind}: err {e:.3e} of max I")
    assert tuple(inten.shape) == (shape[0], g) + shape[2:] and e <= FIELD_RTOL
    (inten * torch.from_numpy(gi_np.copy()).cuda()).sum().backward()
    torch.cuda.synchronize()
    ocfg = _ocfg(name, kind)
    want = np.stack([_leaf_grad(name, kind, e_, M.adjoint(ocfg, (2.0 / q) * M.per_plane(gi_np[e_].astype(np.float64), q) * model[e_][1]),
                                model[e_][3]) for e_ in range(shape[0])])
    _check_grad(f"intensity {kind}", x, want)


# -- loss -------------------------------------------------------------------------------------------------
def _loss_case(name, kind, metric, dtype=None, source=None):
    import torchOptics.optics as tt
    shape, wls = SHAPES[name]
    b, g, q, n = shape[0], len(wls), shape[1] // len(wls), shape[2]
    x_np, t_np, _, _ = _case(name, kind)
    meta = _meta(wls)
    s = torch.from_numpy(_source(name).copy()) if source is None else source
    model = _model(name, kind)
    lk = LOSS_MSE if metric == "mse" else LOSS_PSNR
    x = _leaf(name, kind, dtype)
    target = torch.from_numpy(t_np.copy()).cuda()
    with torch.no_grad():
        quiet = tt.loss(tt.Tensor(x, meta=meta), target, Z, metric=metric, source=s, **KW[kind])
    val = tt.loss(tt.Tensor(x, meta=meta), target, Z, metric=metric, source=s, **KW[kind])
    torch.cuda.synchronize()
    assert val.dtype == torch.float64 and tuple(val.shape) == (b,) and torch.equal(quiet, val.detach())
    up = UP[:b]
    (val * torch.from_numpy(up.copy()).cuda()).sum().backward()
    torch.cuda.synchronize()
    ocfg = _ocfg(name, kind)
    hs = tuple(ocfg.transfer(k) for k in range(g))
    want = []
    for e in range(b):
        _, f, inten, leaf = model[e]
        t64 = t_np[e].astype(np.float64)
        w_val = O.relative_psnr(inten, t64, O.REL_LSQ) if lk == LOSS_PSNR else O.relative_mse(inten, t64, O.REL_LSQ)
        got = float(val.detach()[e])
        err = abs(got - w_val) if lk == LOSS_PSNR else abs(got - w_val) / w_val
        print(f"loss {name} {kind} {metric} env {e}: {got:.9g} vs {w_val:.9g} (err {err:.3e})")
        assert err <= (PSNR_ATOL if lk == LOSS_PSNR else MSE_RTOL)
        adj = loss_gradient(f.reshape(g, q, n, n), inten, t64, hs, lk, REL_LSQ, False, up=up[e]).reshape(g * q, n, n)
        want.append(_leaf_grad(name, kind, e, adj, leaf))
    return x, np.stack(want)


@pytest.mark.parametrize("metric", ["mse", "psnr"])
@pytest.mark.parametrize("kind", KINDS)
def test_loss_with_a_source(kind, metric):
    x, want = _loss_case("rgb", kind, metric)
    _check_grad(f"loss {kind} {metric}", x, want)


def test_loss_with_a_source_at_256_mono():
    x, want = _loss_case("mono256", "phase", "mse")
    _check_grad("loss 256 phase mse", x, want)


@pytest.mark.parametrize("kind", ["real", "threshold"])
def test_an_odd_plane_count_needs_no_padding_under_a_source(kind):
    """three planes of a real or thresholded leaf are three complex planes: tt.loss and tt.intensity take
    them with a source (without one they ask for plane pairs), and the gradient has the leaf's shape"""
    import torchOptics.optics as tt
    x, want = _loss_case("odd", kind, "mse")
    assert tuple(x.grad.shape) == SHAPES["odd"][0]
    _check_grad(f"loss odd {kind}", x, want)
    shape, wls = SHAPES["odd"]
    xs = torch.from_numpy(_case("odd", kind)[0].copy()).cuda()
    inten = tt.intensity(tt.Tensor(xs, meta=_meta(wls)), Z, source=torch.from_numpy(_source("odd").copy()), **KW[kind])
    torch.cuda.synchronize()
    want_i = np.stack([m[2] for m in _model("odd", kind)])
    e = np.max(np.abs(inten.cpu().numpy() - want_i)) / np.max(want_i)
    print(f"intensity odd {kind}: err {e:.3e} of max I")
    assert e <= FIELD_RTOL
    if kind == "threshold":
        with pytest.raises(ValueError):
            tt.loss(tt.Tensor(xs, meta=_meta(wls)), torch.zeros((2, 1, 64, 64)), Z, **KW[kind])


@pytest.mark.parametrize("kind", ["phase", "threshold"])
def test_loss_with_a_pixel_weight_and_a_source(kind):
    """pixel_weight= together with source= through the shim: the loss equals tt.loss(.., pixel_weight=v) on the
    complex tensor plan.source_field writes, bit for bit (the last pass is hbx_evaluate_pw's), and x.grad is
    within FIELD_RTOL of the gradient torch walks back through s f(x) formed with torch ops on that route
    (phase), whose weighted loss is pinned against float64 by the pixel-weight tests"""
    import hbx
    import torchOptics.optics as tt
    from hbx import _lib
    name = "rgb"
    shape, wls = SHAPES[name]
    x_np, t_np, _, _ = _case(name, kind)
    meta, target = _meta(wls), torch.from_numpy(t_np.copy()).cuda()
    s = torch.from_numpy(_source(name).copy()).cuda()
    pw = torch.from_numpy(np.random.default_rng(5300).random((1, 1, 64, 64), dtype=np.float32)).cuda()
    pw[..., :12, :] = 0.0
    x = _leaf(name, kind)
    fused = tt.loss(tt.Tensor(x, meta=meta), target, Z, source=s, pixel_weight=pw, **KW[kind])
    plain = tt.loss(tt.Tensor(x, meta=meta), target, Z, source=s, **KW[kind])
    o = _ocfg(name, kind)
    plan = hbx.Plan(hbx.OpticsConfig(o.height, o.width, o.groups, o.planes, tuple(o.wavelengths), o.dx, o.dy, o.z,
                                     o.tf_kind, o.field_kind, o.rel_scale, o.peak), max_jobs=o.groups)
    leaf = _lib.LEAF_PHASE if kind == "phase" else _lib.LEAF_THRESHOLD
    u = plan.source_field(x.detach(), leaf, s, threshold=TAU)
    mat = tt.loss(tt.Tensor(u, meta=meta), target, Z, pixel_weight=pw)
    torch.cuda.synchronize()
    assert torch.equal(fused.detach(), mat) and not torch.equal(fused.detach(), plain.detach())
    (fused * torch.from_numpy(UP.copy()).cuda()).sum().backward()
    torch.cuda.synchronize()
    assert x.grad is not None and bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0.0
    if kind == "phase":
        x2 = _leaf(name, kind)
        u2 = s.repeat_interleave(shape[1] // len(wls), dim=0) * torch.exp(1j * np.pi * x2)
        (tt.loss(tt.Tensor(u2, meta=meta), target, Z, pixel_weight=pw) * torch.from_numpy(UP.copy()).cuda()).sum().backward()
        torch.cuda.synchronize()
        want = x2.grad.cpu().numpy().astype(np.float64)
        _check_grad("loss phase with a pixel weight", x, want)
    plan.close()


def test_a_source_changed_in_place_before_the_backward_is_an_error():
    """the source is saved with the other tensors: the caller's own complex64 [G, H, W] device tensor is used
    without a copy, and changing it between the two passes raises instead of giving a wrong gradient"""
    import torchOptics.optics as tt
    name, kind = "rgb", "phase"
    shape, wls = SHAPES[name]
    meta, target = _meta(wls), torch.from_numpy(_case(name, kind)[1].copy()).cuda()
    s = torch.from_numpy(_source(name).copy()).cuda()
    x = _leaf(name, kind)
    val = tt.loss(tt.Tensor(x, meta=meta), target, Z, field="phase", source=s).sum()
    s.mul_(2.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        val.backward()


def test_a_float64_leaf_and_a_real_hw_source_work_through_the_casts():
    """a float64 leaf receives a float64 gradient; a real [H, W] source is cast to complex64 and expanded to
    the three groups -- the model runs on the same expanded source"""
    import torchOptics.optics as tt
    name, kind = "rgb", "phase"
    shape, wls = SHAPES[name]
    n = shape[2]
    yy, xx = np.mgrid[:n, :n].astype(np.float64) - (n - 1) / 2.0
    env = np.exp(-(xx ** 2 + yy ** 2) / (0.3 * n) ** 2)                       # float64, [H, W]
    x, want = _loss_case(name, kind, "mse", dtype=torch.float64, source=torch.from_numpy(_source(name).copy()))
    assert x.grad.dtype == torch.float64
    _check_grad("loss f64 leaf", x, want)
    x_np, t_np, _, _ = _case(name, kind)
    meta, target = _meta(wls), torch.from_numpy(t_np.copy()).cuda()
    xs = torch.from_numpy(x_np.copy()).cuda()
    a = tt.loss(tt.Tensor(xs, meta=meta), target, Z, field="phase", source=env)                        # numpy float64 [H, W]
    b = tt.loss(tt.Tensor(xs, meta=meta), target, Z, field="phase",
                source=torch.from_numpy(env.astype(np.complex64)).expand(3, n, n).cuda())               # what it is cast to
    c = tt.loss(tt.Tensor(xs, meta=meta), target, Z, field="phase")
    torch.cuda.synchronize()
    assert torch.equal(a, b) and not torch.equal(a, c)


def test_loss_equals_the_loss_of_the_materialised_complex_tensor_bit_for_bit():
    import hbx
    import torchOptics.optics as tt
    from hbx import _lib
    name, kind = "rgb", "phase"
    shape, wls = SHAPES[name]
    x_np, t_np, _, _ = _case(name, kind)
    meta, target = _meta(wls), torch.from_numpy(t_np.copy()).cuda()
    xs, s = torch.from_numpy(x_np.copy()).cuda(), torch.from_numpy(_source(name).copy()).cuda()
    o = _ocfg(name)
    plan = hbx.Plan(hbx.OpticsConfig(o.height, o.width, o.groups, o.planes, tuple(o.wavelengths), o.dx, o.dy, o.z,
                                     o.tf_kind, o.field_kind, o.rel_scale, o.peak), max_jobs=o.groups)
    u = plan.source_field(xs, _lib.LEAF_PHASE, s)
    for metric in ("mse", "psnr"):
        fused = tt.loss(tt.Tensor(xs, meta=meta), target, Z, metric=metric, field="phase", source=s)
        mat = tt.loss(tt.Tensor(u, meta=meta), target, Z, metric=metric)
        torch.cuda.synchronize()
        assert torch.equal(fused, mat), (metric, fused, mat)
    plan.close()


@pytest.mark.parametrize("kind", ["real", "phase", "threshold"])
def test_source_none_runs_the_code_as_it_was(kind):
    import torchOptics.optics as tt
    name = "rgb"
    shape, wls = SHAPES[name]
    x_np, t_np, _, _ = _case(name, kind)
    meta, target = _meta(wls), torch.from_numpy(t_np.copy()).cuda()
    grads = []
    for kw in ({}, dict(source=None)):
        x = _leaf(name, kind)
        val = tt.loss(tt.Tensor(x, meta=meta), target, Z, **KW[kind], **kw)
        inten = tt.intensity(tt.Tensor(x, meta=meta), Z, **KW[kind], **kw)
        val.sum().backward()
        torch.cuda.synchronize()
        grads.append((val.detach(), inten.detach(), x.grad))
    for a, b in zip(*grads):
        assert torch.equal(a, b)
    m = _meta((WL,))
    x1 = torch.from_numpy(_case("mono", kind)[0].copy()).cuda()
    assert torch.equal(torch.view_as_real(tt.simulate(tt.Tensor(x1, meta=m), Z, binary=False, **KW[kind])),
                       torch.view_as_real(tt.simulate(tt.Tensor(x1, meta=m), Z, binary=False, source=None, **KW[kind])))


def test_thirty_adam_steps_on_a_binary_hologram_under_an_oblique_gaussian_beam():
    """a 64 x 64 thresholded (binary amplitude) hologram lit by a plane wave at a few degrees times a Gaussian
    beam: thirty Adam steps through the straight-through gradient lower the relative MSE"""
    import torchOptics.optics as tt
    n, dx = 64, O.PIXEL_PITCH
    meta = {"dx": (dx, dx), "wl": WL}
    s = tt.sources.plane_wave((n, n), dx, WL, angle=(np.deg2rad(1.0), np.deg2rad(-0.5))) * tt.sources.gaussian((n, n), dx, 20 * dx)
    gen = torch.Generator().manual_seed(7)
    x = torch.rand((1, 4, n, n), generator=gen).cuda().requires_grad_()
    target = torch.zeros((1, 1, n, n))
    target[:, :, 20:44, 24:40] = 1.0
    target = target.cuda()
    opt = torch.optim.Adam([x], lr=0.05)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        val = tt.loss(tt.Tensor(x, meta=meta), target, Z, threshold=0.5, ste="sigmoid", ste_width=0.25, source=s).sum()
        val.backward()
        opt.step()
        losses.append(float(val.detach()))
    with torch.no_grad():
        losses.append(float(tt.loss(tt.Tensor(x, meta=meta), target, Z, threshold=0.5, source=s).sum()))
    print(f"binary hologram under an oblique Gaussian beam: loss {losses[0]:.6g} -> {losses[-1]:.6g}")
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
