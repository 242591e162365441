"""Per-pixel loss weights on the GPU: hbx_evaluate_pw, hbx_evaluate_stack_pw, hbx_pixel_weight_sum, hbx_loss_pw,
hbx_loss_weight_pw and tt.loss / tt.loss_stack with pixel_weight=.

v = 1 gives the unweighted calls' bits (statistics, weight sum, loss, loss weight, the leaf's gradient); v = the
indicator of a rectangle gives the windowed route's bits; a random v (a quarter of the pixels exactly 0) holds
the project's bounds against the float64 statement of tests/test_pixel_weight_host.py -- loss MSE_RTOL, PSNR
PSNR_ATOL, the gradient end to end FIELD_RTOL of max|gradient| -- with the written intensity and field
unchanged; a stack takes one weight per depth; and the use case: 30 Adam steps on a binary phase hologram with
a signal window and a don't-care region around it.  The case shapes are tests/test_gpu_phase_field.py's."""
import functools
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import hbx_oracle as O  # noqa: E402
from tests.test_gpu_phase_field import CASES, FIELD_RTOL, MSE_RTOL, PSNR_ATOL  # noqa: E402
from tests.test_loss_host import LOSS_MSE, LOSS_PSNR, REL_LSQ, REL_NONE  # noqa: E402
from tests.test_phase_levels_host import quantize_np  # noqa: E402
from tests.test_pixel_weight_host import pw_gradient, pw_loss, random_weight  # noqa: E402
from tests.test_threshold_ste_host import STE_WINDOW, binarize, field_values, ste_surrogate  # noqa: E402

Z = 2e-3
ZS = (2e-3, -1.5e-3, 3.5e-3)
UP = np.array([1.0, -0.5])
TAU, WIDTH, NLEVELS = 0.1, 0.5, 6
KINDS = {"real": {}, "threshold": {"threshold": TAU, "ste_width": WIDTH}, "complex": {}, "phase": {"field": "phase"},
         "levels": {"field": "phase", "levels": NLEVELS}}
METRICS = {"mse": LOSS_MSE, "psnr": LOSS_PSNR}
RELS = {"lsq": REL_LSQ, "none": REL_NONE}
# a rectangle aligned to nothing, per size
RECTS = {64: (5, 9, 40, 33), 256: (20, 38, 161, 129), 896: (69, 130, 561, 449), 1024: (79, 148, 641, 513)}


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm GPU")
    import hbx
    hbx.load_library()
    yield


def _leaf_id(kind):
    from hbx import _lib
    return {"real": _lib.LEAF_REAL, "threshold": _lib.LEAF_THRESHOLD, "complex": _lib.LEAF_COMPLEX,
            "phase": _lib.LEAF_PHASE, "levels": _lib.LEAF_PHASE_LEVELS}[kind]


def _wls(g):
    return tuple(O.WL_RGB) if g == 3 else tuple(O.WL_MONO)


def _batch_of(n):
    return 2 if n <= 256 else 1


@functools.lru_cache(maxsize=None)
def _inputs(name, kind, depths=0):
    """(x [B, C, N, N] float32 / complex64, target float32 [(D,) B, G, N, N] in [0, 1), random weight of the
    target's shape), read-only.  A real or thresholded leaf has 2 Q real planes per group, the others Q."""
    n, g, q = CASES[name]
    b = _batch_of(n)
    c = g * (2 * q if kind in ("real", "threshold") else q)
    rng = np.random.default_rng(5100 + 31 * sorted(CASES).index(name) + 7 * sorted(KINDS).index(kind) + depths)
    x = (2 * rng.random((b, c, n, n), dtype=np.float32) - 1).astype(np.float32)
    if kind == "complex":
        x = (x + 1j * (2 * rng.random((b, c, n, n), dtype=np.float32) - 1).astype(np.float32)).astype(np.complex64)
    tshape = ((depths,) if depths else ()) + (b, g, n, n)
    target = rng.random(tshape, dtype=np.float32)
    v = random_weight(rng, tshape)
    for a in (x, target, v):
        a.setflags(write=False)
    return x, target, v


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()             # a copy: the shared inputs are read-only


def _plan(name, kind, z=Z, depths=None):
    import hbx
    n, g, q = CASES[name]
    plan = hbx.Plan(hbx.OpticsConfig(n, n, g, 2 * q, _wls(g), O.PIXEL_PITCH, O.PIXEL_PITCH, z), max_jobs=_batch_of(n) * g)
    if depths:
        plan.set_depths(depths)
    return plan


def _evaluate(plan, kind, x, target):
    """the unweighted evaluate call of a leaf kind -> (field, intensity, chan_stats)"""
    if kind == "real":
        return plan.evaluate_real(x, target)[:3]
    if kind == "threshold":
        return plan.evaluate_threshold(x, TAU, target)[:3]
    if kind == "complex":
        return plan.evaluate_complex(x, target)[:3]
    if kind == "phase":
        return plan.evaluate_phase(x, target)[:3]
    return plan.evaluate_phase_levels(x, NLEVELS, target)[:3]


def _evaluate_pw(plan, kind, x, target, v, stack=False):
    call = plan.evaluate_stack_pw if stack else plan.evaluate_pw
    return call(x, _leaf_id(kind), target, v, levels=NLEVELS if kind == "levels" else None, threshold=TAU)


def _tt_x(tt, name, t):
    g = CASES[name][1]
    wls = _wls(g)
    return tt.Tensor(t, meta={"dx": (O.PIXEL_PITCH, O.PIXEL_PITCH), "wl": wls[0] if g == 1 else wls})


def _tt_loss_and_grad(tt, name, kind, x_np, target, metric, rel, depths=None, **kw):
    """(loss [B] float64, x.grad) of sum_b UP[b] loss_b through tt.loss / tt.loss_stack"""
    x = _cuda(x_np).requires_grad_()
    if depths:
        val = tt.loss_stack(_tt_x(tt, name, x), target, depths, metric=metric, rel_scale=rel, **KINDS[kind], **kw)
    else:
        val = tt.loss(_tt_x(tt, name, x), target, Z, metric=metric, rel_scale=rel, **KINDS[kind], **kw)
    assert val.grad_fn is not None and val.dtype == torch.float64
    (val * _cuda(UP[:x.shape[0]])).sum().backward()
    return val.detach(), x.grad


# -- the float64 statement of a leaf kind ----------------------------------------------------------------
def _field64(name, kind, x_np):
    """(u float64 / complex128 [B, G, Pc, N, N], what turns dL/du into dL/dx) for the float32 leaf x"""
    n, g, _ = CASES[name]
    b, c = x_np.shape[:2]
    x64 = x_np.astype(np.complex128 if kind == "complex" else np.float64)
    if kind == "threshold":
        u = binarize(x_np, np.float32(TAU), O.FIELD_AMPLITUDE).astype(np.float64)
        lo = float(np.float32(np.float32(TAU) - np.float32(WIDTH)))
        hi = float(np.float32(np.float32(TAU) + np.float32(WIDTH)))
        s = ste_surrogate(x64, STE_WINDOW, lo, hi)
        back = lambda adj: field_values(O.FIELD_AMPLITUDE)[1] * s * adj.real      # noqa: E731
    elif kind in ("phase", "levels"):
        ph = quantize_np(x_np, NLEVELS)[2].astype(np.float64) if kind == "levels" else x64
        u = np.exp(1j * np.pi * ph)
        back = lambda adj: (np.conj(1j * np.pi * u) * adj).real                   # noqa: E731
    elif kind == "complex":
        u, back = x64, (lambda adj: adj)
    else:
        u, back = x64, (lambda adj: adj.real)
    return u.reshape(b, g, c // g, n, n), back


def _transfer(name, zs):
    n, g, _ = CASES[name]
    return [[O.transfer_function(n, n, O.PIXEL_PITCH, O.PIXEL_PITCH, wl, z) for wl in _wls(g)] for z in zs]


def _check_against_float64(tt, name, kind, depths=None):
    """test 7's bounds for one case: the loss (both metrics, both scales) and the end-to-end gradient"""
    x_np, t_np, v_np = _inputs(name, kind, len(depths) if depths else 0)
    zs = depths or (Z,)
    hs = _transfer(name, zs)
    u64, back = _field64(name, kind, x_np)
    t64, v64 = t_np.astype(np.float64), v_np.astype(np.float64)
    if not depths:
        t64, v64 = t64[None], v64[None]
    b = x_np.shape[0]
    target, v = _cuda(t_np), _cuda(v_np)
    for metric, rel in (("mse", "lsq"), ("psnr", "none"), ("mse", "none"), ("psnr", "lsq")):
        want = np.array([pw_loss(u64[e], t64[:, e], v64[:, e], hs, METRICS[metric], RELS[rel]) for e in range(b)])
        with_grad = (metric, rel) in (("mse", "lsq"), ("psnr", "none"))
        if with_grad:
            got, grad = _tt_loss_and_grad(tt, name, kind, x_np, target, metric, rel, depths, pixel_weight=v)
        else:
            with torch.no_grad():
                xt = _tt_x(tt, name, _cuda(x_np))
                got = (tt.loss_stack(xt, target, depths, metric=metric, rel_scale=rel, pixel_weight=v, **KINDS[kind])
                       if depths else tt.loss(xt, target, Z, metric=metric, rel_scale=rel, pixel_weight=v, **KINDS[kind]))
            assert got.grad_fn is None
        got = got.cpu().numpy()
        err = np.abs(got - want)
        if metric == "mse":
            print(f"PIXW {name} {kind} D={len(zs)} mse/{rel}: loss rel err {np.max(err / want):.3e} (bound {MSE_RTOL})")
            assert np.all(err <= MSE_RTOL * want)
        else:
            print(f"PIXW {name} {kind} D={len(zs)} psnr/{rel}: psnr err {np.max(err):.3e} dB (bound {PSNR_ATOL})")
            assert np.all(err <= PSNR_ATOL)
        if with_grad:
            adj = np.stack([pw_gradient(u64[e], t64[:, e], v64[:, e], hs, METRICS[metric], RELS[rel], False, UP[e])
                            for e in range(b)])
            want_g = back(adj.reshape(x_np.shape))
            scale = np.max(np.abs(want_g))
            e_g = np.max(np.abs(grad.cpu().numpy() - want_g)) / scale
            print(f"PIXW {name} {kind} D={len(zs)} {metric}/{rel}: end-to-end grad err {e_g:.3e} of max|grad| = "
                  f"{scale:.3e} (bound {FIELD_RTOL})")
            assert scale > 0.0 and grad.dtype == (torch.complex64 if kind == "complex" else torch.float32)
            assert e_g <= FIELD_RTOL


# -- 5. v = 1: the unweighted calls' bits ------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("name", list(CASES))
def test_unit_weight_gives_the_unweighted_calls_bit_for_bit(name, kind):
    import torchOptics.optics as tt
    n, g, _ = CASES[name]
    x_np, t_np, _ = _inputs(name, kind)
    x, target = _cuda(x_np), _cuda(t_np)
    ones = torch.ones_like(target)
    plan = _plan(name, kind)
    f0, i0, s0 = _evaluate(plan, kind, x, target)
    f1, i1, s1 = _evaluate_pw(plan, kind, x, target, ones)
    assert torch.equal(s1, s0) and torch.equal(i1, i0) and torch.equal(f1, f0)
    wsum = plan.pixel_weight_sum(ones)
    assert wsum.dtype == torch.float64 and torch.equal(wsum, torch.full_like(wsum, float(g * n * n)))
    gl = _cuda(UP[:x.shape[0]])
    for kd in (LOSS_MSE, LOSS_PSNR):
        for rel in (REL_LSQ, REL_NONE):
            assert torch.equal(plan.loss_pw(s1, wsum, kd, rel), plan.loss(s0, kd, rel))
            assert torch.equal(plan.loss_weight_pw(i1, target, ones, s1, wsum, gl, kd, rel),
                               plan.loss_weight(i0, target, s0, gl, kd, rel))
    plan.close()
    for metric in METRICS:
        for rel in RELS:
            l0, g0 = _tt_loss_and_grad(tt, name, kind, x_np, target, metric, rel)
            l1, g1 = _tt_loss_and_grad(tt, name, kind, x_np, target, metric, rel, pixel_weight=ones)
            assert torch.equal(l1, l0) and torch.equal(g1, g0)
    torch.cuda.synchronize()


# -- 6. v = a rectangle's indicator: the windowed route's bits ------------------------------------------------
@pytest.mark.parametrize("kind", ["real", "threshold"])
@pytest.mark.parametrize("name", list(CASES))
def test_rectangle_indicator_gives_the_windowed_route_bit_for_bit(name, kind):
    import torchOptics.optics as tt
    n, g, _ = CASES[name]
    y0, x0, h, w = rect = RECTS[n]
    x_np, t_np, _ = _inputs(name, kind)
    x, target = _cuda(x_np), _cuda(t_np)
    v = torch.zeros_like(target)
    v[..., y0:y0 + h, x0:x0 + w] = 1.0
    troi = target[..., y0:y0 + h, x0:x0 + w].contiguous()
    plan = _plan(name, kind)
    _, _, s1 = _evaluate_pw(plan, kind, x, target, v, )
    if kind == "real":
        _, _, sw, _ = plan.evaluate_real_window(x, None, troi, rect)
    else:
        _, _, sw, _ = plan.evaluate_threshold_window(x, TAU, None, troi, rect)
    assert torch.equal(s1, sw)
    wsum = plan.pixel_weight_sum(v)
    assert torch.equal(wsum, torch.full_like(wsum, float(g * h * w)))
    for kd in (LOSS_MSE, LOSS_PSNR):
        for rel in (REL_LSQ, REL_NONE):
            assert torch.equal(plan.loss_pw(s1, wsum, kd, rel), plan.loss_window(sw, rect, kd, rel))
    plan.close()
    for metric, rel in (("mse", "lsq"), ("psnr", "none")):
        l1, g1 = _tt_loss_and_grad(tt, name, kind, x_np, target, metric, rel, pixel_weight=v)
        lw, gw = _tt_loss_and_grad(tt, name, kind, x_np, troi, metric, rel, grid=n, roi=rect)
        assert torch.equal(l1, lw) and torch.equal(g1, gw)
    torch.cuda.synchronize()


# -- 7. a random v against float64 ------------------------------------------------------------------------
RANDOM = [(name, kind) for name in ("64", "256q2") for kind in KINDS] + [("896", "threshold"), ("1024", "phase")]


@pytest.mark.parametrize("name, kind", RANDOM, ids=[f"{n}-{k}" for n, k in RANDOM])
def test_random_weight_against_float64_and_outputs_unchanged(name, kind):
    import torchOptics.optics as tt
    x_np, t_np, v_np = _inputs(name, kind)
    assert 0.2 < float((v_np == 0).mean()) < 0.3
    x, target, v = _cuda(x_np), _cuda(t_np), _cuda(v_np)
    plan = _plan(name, kind)
    f0, i0, s0 = _evaluate(plan, kind, x, target)
    f1, i1, s1 = _evaluate_pw(plan, kind, x, target, v)
    assert torch.equal(i1, i0) and torch.equal(f1, f0) and not torch.equal(s1, s0)
    wsum = plan.pixel_weight_sum(v)
    want_w = v_np.astype(np.float64).reshape(v_np.shape[0], -1).sum(axis=1)
    assert np.all(np.abs(wsum.cpu().numpy() - want_w) <= 1e-12 * want_w)
    assert torch.equal(wsum, plan.pixel_weight_sum(v))                     # bitwise reproducible
    plan.close()
    _check_against_float64(tt, name, kind)
    torch.cuda.synchronize()


# -- 8. stacks ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_one_depth_stack_is_the_single_depth_weighted_call(kind):
    import torchOptics.optics as tt
    name = "64"
    x_np, t_np, v_np = _inputs(name, kind)
    x, target, v = _cuda(x_np), _cuda(t_np), _cuda(v_np)
    single, stack = _plan(name, kind), _plan(name, kind, depths=(Z,))
    f0, i0, s0 = _evaluate_pw(single, kind, x, target, v)
    f1, i1, s1 = _evaluate_pw(stack, kind, x, target[None], v[None], stack=True)
    assert torch.equal(s1[0], s0) and torch.equal(i1[0], i0) and torch.equal(f1[0], f0)
    w0, w1 = single.pixel_weight_sum(v), stack.pixel_weight_sum(v[None], stack=True)
    assert torch.equal(w1, w0)
    gl = _cuda(UP[:x.shape[0]])
    for kd in (LOSS_MSE, LOSS_PSNR):
        for rel in (REL_LSQ, REL_NONE):
            assert torch.equal(stack.loss_pw(s1, w1, kd, rel, stack=True), single.loss_pw(s0, w0, kd, rel))
            assert torch.equal(stack.loss_weight_pw(i1, target[None], v[None], s1, w1, gl, kd, rel, stack=True)[0],
                               single.loss_weight_pw(i0, target, v, s0, w0, gl, kd, rel))
    single.close()
    stack.close()
    l0, g0 = _tt_loss_and_grad(tt, name, kind, x_np, target, "mse", "lsq", pixel_weight=v)
    l1, g1 = _tt_loss_and_grad(tt, name, kind, x_np, target[None], "mse", "lsq", depths=(Z,), pixel_weight=v[None])
    assert torch.equal(l1, l0) and torch.equal(g1, g0)
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("depths", [2, 3])
def test_stack_with_a_weight_per_depth_against_float64(depths, kind):
    import torchOptics.optics as tt
    _check_against_float64(tt, "64", kind, ZS[:depths])
    torch.cuda.synchronize()


@pytest.mark.parametrize("name, kind", [("64", "real"), ("64", "levels"), ("256q3", "threshold"), ("256q1", "complex"),
                                        ("896", "phase"), ("1024", "real")])
def test_stack_depth_blocks_are_the_single_depth_weighted_calls(name, kind):
    x_np, t_np, v_np = _inputs(name, kind, 3)
    x, target, v = _cuda(x_np), _cuda(t_np), _cuda(v_np)
    stack = _plan(name, kind, depths=ZS)
    f, i, s = _evaluate_pw(stack, kind, x, target, v, stack=True)
    stack.close()
    for d, z in enumerate(ZS):
        single = _plan(name, kind, z=z)
        fd, idd, sd = _evaluate_pw(single, kind, x, target[d], v[d])
        assert torch.equal(s[d], sd) and torch.equal(i[d], idd) and torch.equal(f[d], fd)
        single.close()
    torch.cuda.synchronize()


# -- 9. the use case ------------------------------------------------------------------------------------
def test_adam_on_a_binary_phase_hologram_with_a_signal_window():
    """64 x 64, one wavelength, two planes, field="phase" binary hologram m = [x >= 0.5] under the plain
    straight-through estimator, lsq scale; target 0.05 + a Gaussian blob (sigma = N / 6) times (0.5 + 0.5
    uniform); weight 1 on the central 32 x 32 and 0 elsewhere.  30 Adam steps at lr 0.05 through
    tt.loss(.., pixel_weight=v): the last loss is at most half the first (the float64 run gives 0.19; the
    float32 and float64 trajectories part at the hard threshold, so nothing tighter is held), and it is the
    loss of the exported mask -- tt.loss on hbx.pack_mask's round trip of the final x."""
    import hbx
    import torchOptics.optics as tt
    n = 64
    rng = np.random.default_rng(4700)
    yy, xx = np.meshgrid(np.arange(n) - (n - 1) / 2, np.arange(n) - (n - 1) / 2, indexing="ij")
    blob = np.exp(-(yy ** 2 + xx ** 2) / (2 * (n / 6) ** 2))
    target = _cuda((0.05 + blob * (0.5 + 0.5 * rng.random((n, n)))).astype(np.float32)[None, None])
    v = torch.zeros((n, n), device="cuda")
    v[16:48, 16:48] = 1.0
    x = _cuda(rng.random((1, 2, n, n), dtype=np.float32)).requires_grad_()
    meta = {"dx": (O.PIXEL_PITCH, O.PIXEL_PITCH), "wl": 515e-9}
    kw = dict(field="phase", threshold=0.5, ste_width=math.inf, rel_scale="lsq", pixel_weight=v)
    opt = torch.optim.Adam([x], lr=0.05)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        val = tt.loss(tt.Tensor(x, meta=meta), target, Z, **kw).sum()
        val.backward()
        opt.step()
        losses.append(val.detach())
    with torch.no_grad():
        last = tt.loss(tt.Tensor(x, meta=meta), target, Z, **kw)
        mask = hbx.unpack_bits(hbx.pack_mask(x.detach(), threshold=0.5), n).to(torch.float32)
        exported = tt.loss(tt.Tensor(mask, meta=meta), target, Z, **kw)
        plain = tt.loss(tt.Tensor(x, meta=meta), target, Z, **dict(kw, pixel_weight=None))
    losses = [float(t) for t in losses] + [float(last[0])]
    print("PIXW use case: in-window losses", " ".join(f"{t:.4f}" for t in losses), "| ratio last / first",
          f"{losses[-1] / losses[0]:.3f}", "| unweighted loss of the final x", f"{float(plain[0]):.4f}")
    assert torch.equal(exported, last)
    assert losses[-1] <= 0.5 * losses[0]


# -- 10. broadcasting and casts -------------------------------------------------------------------------------
def test_weight_shapes_and_dtypes_give_the_same_bits():
    import torchOptics.optics as tt
    name, kind = "64", "phase"
    n, g, _ = CASES[name]
    x_np, t_np, v_np = _inputs(name, kind)
    target = _cuda(t_np)
    b = x_np.shape[0]
    hw = _cuda(v_np[0, 0])
    ghw = _cuda(v_np[0])
    full_hw = hw.expand(b, g, n, n).contiguous()
    full_ghw = ghw.expand(b, g, n, n).contiguous()
    l_hw, g_hw = _tt_loss_and_grad(tt, name, kind, x_np, target, "mse", "lsq", pixel_weight=hw)
    l_f1, g_f1 = _tt_loss_and_grad(tt, name, kind, x_np, target, "mse", "lsq", pixel_weight=full_hw)
    assert torch.equal(l_hw, l_f1) and torch.equal(g_hw, g_f1)
    l_g, g_g = _tt_loss_and_grad(tt, name, kind, x_np, target, "mse", "lsq", pixel_weight=ghw)
    l_f2, g_f2 = _tt_loss_and_grad(tt, name, kind, x_np, target, "mse", "lsq", pixel_weight=full_ghw)
    assert torch.equal(l_g, l_f2) and torch.equal(g_g, g_f2) and not torch.equal(l_g, l_hw)
    for cast in (full_ghw.double(), full_ghw.cpu().numpy().astype(np.float64), full_ghw.cpu()):
        l_c, g_c = _tt_loss_and_grad(tt, name, kind, x_np, target, "mse", "lsq", pixel_weight=cast)
        assert torch.equal(l_c, l_f2) and torch.equal(g_c, g_f2)
    # a stack: one weight per depth for every env, [D, 1, G, H, W]
    t3 = _cuda(_inputs(name, kind, 2)[1])
    v3 = _cuda(_inputs(name, kind, 2)[2][:, :1])
    l_b, g_b = _tt_loss_and_grad(tt, name, kind, x_np, t3, "mse", "lsq", depths=ZS[:2], pixel_weight=v3)
    l_e, g_e = _tt_loss_and_grad(tt, name, kind, x_np, t3, "mse", "lsq", depths=ZS[:2],
                                 pixel_weight=v3.expand(2, b, g, n, n).contiguous())
    assert torch.equal(l_b, l_e) and torch.equal(g_b, g_e)
    # a 3-D x with a [G, H, W] weight is env 0 of the batched call
    with torch.no_grad():
        one = tt.loss(_tt_x(tt, name, _cuda(x_np[0])), target[0], Z, pixel_weight=ghw, **KINDS[kind])
    assert one.dim() == 0 and torch.equal(one, l_g[0])
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", ["threshold", "levels"])
def test_chunking_by_max_jobs(kind):
    """n_env = 3 on a plan of one env per chunk (max_jobs = G) against a plan that takes all three at once: the
    weight advances with the target, and the weight sum goes through the plan's scratch a chunk at a time"""
    import hbx
    n, g, q = CASES["64"]
    rng = np.random.default_rng(77)
    c = g * (2 * q if kind == "threshold" else q)
    x = _cuda((2 * rng.random((3, c, n, n), dtype=np.float32) - 1).astype(np.float32))
    target = _cuda(rng.random((3, g, n, n), dtype=np.float32))
    v = _cuda(random_weight(rng, (3, g, n, n)))
    cfg = hbx.OpticsConfig(n, n, g, 2 * q, _wls(g), O.PIXEL_PITCH, O.PIXEL_PITCH, Z)
    outs = []
    for max_jobs in (g, 3 * g):
        plan = hbx.Plan(cfg, max_jobs=max_jobs)
        outs.append(_evaluate_pw(plan, kind, x, target, v) + (plan.pixel_weight_sum(v),))
        plan.close()
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    want_w = v.double().sum((1, 2, 3))
    assert float(((outs[0][3] - want_w).abs() / want_w).max()) <= 1e-12
    torch.cuda.synchronize()


# -- error paths and degenerate envs ------------------------------------------------------------------------
def test_error_paths_and_an_all_zero_weight():
    import ctypes as C
    import hbx
    from hbx import _lib
    from hbx.plan import _ptr, _stream
    name, kind = "64", "real"
    x_np, t_np, v_np = _inputs(name, kind)
    x, target, v = _cuda(x_np), _cuda(t_np), _cuda(v_np)
    plan = _plan(name, kind)
    lib, h, st = plan.lib, plan._h, _stream(None)
    leaf = _lib.Leaf(_lib.LEAF_REAL, 0, 0.0, 0, 0.0, 0.0)
    stats = torch.empty((2, 3, 3), dtype=torch.float64, device="cuda")
    args = lambda **k: [h, k.get("x", _ptr(x)), k.get("leaf", C.byref(leaf)), k.get("t", _ptr(target)),   # noqa: E731
                        k.get("v", _ptr(v)), k.get("n", 2), None, None, k.get("s", _ptr(stats)), st]
    assert lib.hbx_evaluate_pw(*args()) == _lib.OK
    for bad in (dict(x=None), dict(t=None), dict(v=None), dict(s=None), dict(leaf=None), dict(n=-1),
                dict(leaf=C.byref(_lib.Leaf(7, 0, 0.0, 0, 0.0, 0.0))),
                dict(leaf=C.byref(_lib.Leaf(_lib.LEAF_PHASE_LEVELS, 1, 0.0, 0, 0.0, 0.0))),
                dict(leaf=C.byref(_lib.Leaf(_lib.LEAF_PHASE_LEVELS, 257, 0.0, 0, 0.0, 0.0)))):
        assert lib.hbx_evaluate_pw(*args(**bad)) == _lib.ERR_INVALID, bad
    assert lib.hbx_evaluate_pw(*args(n=0, x=None, t=None, v=None, s=None)) == _lib.OK
    assert lib.hbx_evaluate_stack_pw(*args()) == _lib.ERR_INVALID           # no depths set
    wsum = torch.empty((2,), dtype=torch.float64, device="cuda")
    assert lib.hbx_pixel_weight_sum(h, _ptr(v), 2, 2, _ptr(wsum), st) == _lib.ERR_INVALID   # not the plan's depths
    assert lib.hbx_pixel_weight_sum(h, None, 2, 0, _ptr(wsum), st) == _lib.ERR_INVALID
    assert lib.hbx_pixel_weight_sum(h, None, 0, 0, None, st) == _lib.OK
    assert lib.hbx_loss_pw(h, _ptr(stats), None, 2, 0, 0, 1, _ptr(wsum), st) == _lib.ERR_INVALID
    assert lib.hbx_loss_pw(h, _ptr(stats), _ptr(wsum), 2, 0, 9, 1, _ptr(wsum), st) == _lib.ERR_INVALID
    assert lib.hbx_loss_weight_pw(h, None, None, None, None, None, None, 2, 0, 0, 1, None, st) == _lib.ERR_INVALID
    plan.precision = _lib.PRECISION_BF16_STORE
    assert lib.hbx_evaluate_pw(*args()) == _lib.ERR_UNSUPPORTED
    plan.precision = _lib.PRECISION_F32
    with pytest.raises(ValueError):
        plan.evaluate_pw(x, _lib.LEAF_REAL, target, v[0])
    with pytest.raises(TypeError):
        plan.evaluate_pw(x, _lib.LEAF_REAL, target, v.double())
    # env 1's weight all zero: loss 0 / +inf, a zero gradient, env 0 untouched
    vz = v.clone()
    vz[1] = 0.0
    _, inten, s = plan.evaluate_pw(x, _lib.LEAF_REAL, target, vz)
    w = plan.pixel_weight_sum(vz)
    assert float(w[1]) == 0.0 and float(w[0]) > 0.0
    assert float(plan.loss_pw(s, w, LOSS_MSE, REL_LSQ)[1]) == 0.0
    assert float(plan.loss_pw(s, w, LOSS_PSNR, REL_NONE)[1]) == math.inf
    for kd in (LOSS_MSE, LOSS_PSNR):
        for rel in (REL_LSQ, REL_NONE):
            lw = plan.loss_weight_pw(inten, target, vz, s, w, None, kd, rel)
            assert bool(torch.isfinite(lw).all()) and float(lw[1].abs().max()) == 0.0 and float(lw[0].abs().max()) > 0.0
    plan.close()
    torch.cuda.synchronize()
