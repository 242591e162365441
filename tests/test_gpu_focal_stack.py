"""Focal stacks through the C-ABI (hbx_plan_set_depths, hbx_evaluate_stack, hbx_backward_stack,
hbx_loss_stack, hbx_loss_weight_stack): one hologram at D depths, the first pass run once, and the
backward's depth-summing last pass.

Forward: depth d's block of every output is the single-depth call's on a plan created with z = z[d], bit
for bit, for the five leaf kinds at the four sizes; the stack call runs through ctypes on NaN-guarded
buffers (tests/test_gpu_window.Guarded).  Backward: at D = 1 the single-depth backward call's bits (int32
views: the sign of a zero counts); at D > 1 the float64 gradient sum_d A(z_d)[scale w_d V_d], built with
oracle.transfer_function and oracle.propagate, within FIELD_RTOL of max|gradient| (the single-depth
gradient tests' bound, tests/test_gpu_phase_field.py), next to the error of D single-depth calls added in
float32.  Shapes (N, G, P, B): 64 with G = 3, P = 2 and G = 1, P = 4 at B = 3; 256 at B = 2; 896 and 1024
at B = 1.  Depths: unequal, one repeated, one negative."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import hbx_oracle as O  # noqa: E402
from tests.test_focal_stack_host import stack_loss, stack_loss_coeffs  # noqa: E402
from tests.test_gpu_evaluate import MSE_RTOL, PSNR_ATOL  # noqa: E402
from tests.test_gpu_phase_field import FIELD_RTOL  # noqa: E402
from tests.test_gpu_window import Guarded  # noqa: E402
from tests.test_loss_host import LOSS_MSE, LOSS_PSNR, REL_LSQ, REL_NONE  # noqa: E402
from tests.test_phase_field_host import phase_gradient  # noqa: E402
from tests.test_phase_levels_host import quantize_np  # noqa: E402
from tests.test_threshold_ste_host import STE_SIGMOID, STE_WINDOW, ste_gradient  # noqa: E402

# name: (N, G, P, B)
CASES = {"64rgb": (64, 3, 2, 3), "64p4": (64, 1, 4, 3), "256": (256, 1, 2, 2), "896": (896, 1, 2, 1),
         "1024": (1024, 1, 2, 1)}
DEPTHS = {1: (2e-3,), 2: (2e-3, -1.5e-3), 3: (1e-3, -1.5e-3, 1e-3)}
REAL, THRESHOLD, COMPLEX, PHASE, LEVELS = range(5)
KIND_NAMES = {"real": REAL, "threshold": THRESHOLD, "complex": COMPLEX, "phase": PHASE, "levels": LEVELS}
TAU, NLEVELS = 0.1, 6
SIGMOID = (STE_SIGMOID, TAU, 4.0)
WINDOW = (STE_WINDOW, -0.4, 0.6)


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm GPU")
    import hbx
    hbx.load_library()
    yield


def dev_cfg(name, z, field_kind=O.FIELD_AMPLITUDE):
    import hbx
    n, g, p, _ = CASES[name]
    return hbx.OpticsConfig(n, n, g, p, tuple(O.WL_RGB if g == 3 else O.WL_MONO), O.PIXEL_PITCH, O.PIXEL_PITCH, z,
                            O.TF_ASM, field_kind, O.REL_LSQ, 1.0)


@functools.lru_cache(maxsize=None)
def single_plan(name, z, field_kind=O.FIELD_AMPLITUDE):
    """the plan created with z: one chunk holds the case's batch"""
    import hbx
    n, g, p, b = CASES[name]
    return hbx.Plan(dev_cfg(name, z, field_kind), max_jobs=b * g)


@functools.lru_cache(maxsize=None)
def stack_plan(name, zs, max_jobs=None, field_kind=O.FIELD_AMPLITUDE):
    """a plan whose own z is none of the depths, with the depths set"""
    import hbx
    n, g, p, b = CASES[name]
    plan = hbx.Plan(dev_cfg(name, 7e-3, field_kind), max_jobs=max_jobs or b * g * len(zs))
    plan.set_depths(zs)
    assert plan.depths == len(zs)
    return plan


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _bits(t):
    return torch.view_as_real(t).view(torch.int32) if t.is_complex() else t.view(torch.int32)


def _leaf(kind, surrogate=(STE_WINDOW, 0.0, 0.0)):
    from hbx import _lib
    return _lib.Leaf(kind, NLEVELS if kind == LEVELS else 0, TAU, surrogate[0], surrogate[1], surrogate[2])


@functools.lru_cache(maxsize=None)
def samples(name, kind):
    """the leaf's samples as the forward takes them (read-only numpy) and a target [3][B][G][N][N] in [0, 1)"""
    n, g, p, b = CASES[name]
    rng = np.random.default_rng(7100 + 10 * len(name) + kind + n)
    planes = g * p if kind in (REAL, THRESHOLD) else g * p // 2
    x = (2 * rng.random((b, planes, n, n), dtype=np.float32) - 1).astype(np.float32)
    if kind == COMPLEX:
        x = (x + 1j * (2 * rng.random(x.shape, dtype=np.float32) - 1)).astype(np.complex64)
    target = rng.random((3, b, g, n, n), dtype=np.float32)
    x.setflags(write=False)
    target.setflags(write=False)
    return x, target


def single_evaluate(plan, kind, x, target):
    """the single-depth call of the kind -> (field, intensity, chan_stats)"""
    if kind == REAL:
        out = plan.evaluate_real(x, target)
    elif kind == THRESHOLD:
        out = plan.evaluate_threshold(x, TAU, target)
    elif kind == COMPLEX:
        out = plan.evaluate_complex(x, target)
    elif kind == PHASE:
        out = plan.evaluate_phase(x, target)
    else:
        out = plan.evaluate_phase_levels(x, NLEVELS, target)
    return out[:3]


def raw_evaluate_stack(plan, kind, x, target, field=True, inten=True):
    """hbx_evaluate_stack on guarded buffers -> (field complex64 [D, B, C, N, N] | None, intensity | None, stats | None)"""
    from hbx import _lib
    c = plan.cfg
    d, b = plan.depths, x.shape[0]
    gx = Guarded(tuple(x.shape) + ((2,) if x.is_complex() else ()), data=(torch.view_as_real(x) if x.is_complex() else x).cpu().numpy())
    gt = Guarded((d, b, c.groups, c.height, c.width), data=target.cpu().numpy()) if target is not None else None
    gf = Guarded((d,) + tuple(x.shape) + (2,)) if field else None
    gi = Guarded((d, b, c.groups, c.height, c.width)) if inten else None
    gs = Guarded((d, b, c.groups, 3), torch.float64) if target is not None else None
    p = lambda g: g.ptr if g is not None else None   # noqa: E731
    leaf = _leaf(kind)
    rc = plan.lib.hbx_evaluate_stack(plan._h, gx.ptr, C.byref(leaf), p(gt), b, p(gf), p(gi), p(gs), _stream())
    _lib.check(rc, "hbx_evaluate_stack")
    torch.cuda.synchronize()
    out = []
    for g in (gf, gi, gs):
        if g is None:
            out.append(None)
            continue
        assert g.intact(), "a guard element next to an output was written"
        assert not torch.isnan(g.t).any(), "an output element is NaN (unwritten, or read from outside an input)"
        out.append(g.t)
    for g in (gx, gt):
        assert g is None or g.intact()
    if out[0] is not None:
        out[0] = torch.view_as_complex(out[0])
    return out


# -- 1. tables and forward, bit for bit -------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KIND_NAMES))
@pytest.mark.parametrize("name", list(CASES))
def test_forward_depth_blocks_are_the_single_depth_calls_bit_for_bit(name, kind):
    k = KIND_NAMES[kind]
    zs = DEPTHS[3]
    x_np, t_np = samples(name, k)
    x, target = torch.from_numpy(x_np.copy()).cuda(), torch.from_numpy(t_np.copy()).cuda()
    field, inten, stats = raw_evaluate_stack(stack_plan(name, zs), k, x, target)
    for d, z in enumerate(zs):
        wf, wi, ws = single_evaluate(single_plan(name, z), k, x, target[d].contiguous())
        torch.cuda.synchronize()
        assert torch.equal(_bits(field[d]), _bits(wf)), f"field of depth {d}"
        assert torch.equal(_bits(inten[d]), _bits(wi)), f"intensity of depth {d}"
        assert torch.equal(stats[d], ws), f"chan_stats of depth {d}"
    # the repeated depth gives the same field twice; the unequal ones do not
    assert torch.equal(field[0], field[2]) and not torch.equal(field[0], field[1])


@pytest.mark.parametrize("kind", list(KIND_NAMES))
def test_forward_subsets_of_the_outputs(kind):
    """without a target: the intensity alone (every kind), the field alone (the two real kinds); with one:
    the statistics alone.  Each what the full call writes, bit for bit."""
    k = KIND_NAMES[kind]
    name, zs = "64rgb", DEPTHS[2]
    x_np, t_np = samples(name, k)
    x, target = torch.from_numpy(x_np.copy()).cuda(), torch.from_numpy(t_np[:2].copy()).cuda()
    plan = stack_plan(name, zs)
    field, inten, stats = raw_evaluate_stack(plan, k, x, target)
    f2, i2, s2 = raw_evaluate_stack(plan, k, x, None, field=False)
    assert f2 is None and s2 is None and torch.equal(_bits(i2), _bits(inten))
    f3, i3, s3 = raw_evaluate_stack(plan, k, x, target, field=False, inten=False)
    assert torch.equal(s3, stats)
    if k in (REAL, THRESHOLD):
        f4, _, _ = raw_evaluate_stack(plan, k, x, None, inten=False)
        assert torch.equal(_bits(f4), _bits(field))


def test_threshold_forward_on_a_binary_phase_plan():
    name, zs = "64p4", DEPTHS[2]
    x_np, t_np = samples(name, THRESHOLD)
    x, target = torch.from_numpy(x_np.copy()).cuda(), torch.from_numpy(t_np[:2].copy()).cuda()
    field, inten, stats = raw_evaluate_stack(stack_plan(name, zs, None, O.FIELD_PHASE), THRESHOLD, x, target)
    for d, z in enumerate(zs):
        wf, wi, ws = single_evaluate(single_plan(name, z, O.FIELD_PHASE), THRESHOLD, x, target[d].contiguous())
        assert torch.equal(field[d], wf) and torch.equal(inten[d], wi) and torch.equal(stats[d], ws)


def test_set_depths_replaces_frees_and_refuses():
    import hbx
    from hbx import _lib
    plan = hbx.Plan(dev_cfg("64p4", 2e-3), max_jobs=4)
    assert plan.depths == 0
    plan.set_depths(DEPTHS[3])
    assert plan.depths == 3
    plan.set_depths(DEPTHS[2])          # replaces the earlier set
    assert plan.depths == 2
    z = (C.c_double * 9)(*([1e-3] * 9))
    for bad_z, n in ((z, 9), (z, -1), (None, 2), ((C.c_double * 2)(1e-3, float("nan")), 2),
                     ((C.c_double * 1)(float("inf")), 1)):
        assert plan.lib.hbx_plan_set_depths(plan._h, bad_z, n) == _lib.ERR_INVALID
        assert plan.depths == 2         # the earlier set stays
    # the plan's own z and its single-depth calls are untouched by the depths
    x_np, t_np = samples("64p4", COMPLEX)
    x, target = torch.from_numpy(x_np.copy()).cuda(), torch.from_numpy(t_np[0].copy()).cuda()
    got = plan.evaluate_complex(x, target)
    want = single_plan("64p4", 2e-3).evaluate_complex(x, target)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    plan.set_depths(())                 # frees the tables
    assert plan.depths == 0
    plan.close()


# -- 2. backward ---------------------------------------------------------------------------------------------
# output name: (leaf kind, surrogate)
OUTPUTS = {"field": (COMPLEX, None), "real": (REAL, None), "phase": (PHASE, None), "levels": (LEVELS, None),
           "ste_window": (THRESHOLD, WINDOW), "ste_sigmoid": (THRESHOLD, SIGMOID)}


@functools.lru_cache(maxsize=None)
def backward_inputs(name, d):
    """values complex64 [D][B][G P/2][N][N], weight f32 [D][B][G][N][N], leaf samples f32 [B][G P/2][N][N]"""
    n, g, p, b = CASES[name]
    rng = np.random.default_rng(9300 + 10 * len(name) + d + n)
    shape = (d, b, g * p // 2, n, n)
    v = ((2 * rng.random(shape, dtype=np.float32) - 1) + 1j * (2 * rng.random(shape, dtype=np.float32) - 1)).astype(np.complex64)
    w = (2 * rng.random((d, b, g, n, n), dtype=np.float32) - 1).astype(np.float32)
    x = (2 * rng.random(shape[1:], dtype=np.float32) - 1).astype(np.float32)
    for a in (v, w, x):
        a.setflags(write=False)
    return v, w, x


def stack_backward(plan, out, values, weight, x, scale=0.25):
    kind, sur = OUTPUTS[out]
    kw = dict(zip(("surrogate", "p0", "p1"), sur)) if sur else {}
    needs = kind in (PHASE, LEVELS, THRESHOLD)
    return plan.backward_stack(values, kind, samples=x if needs else None, weight=weight, scale=scale,
                               levels=NLEVELS if kind == LEVELS else None, **kw)


def single_backward(plan, out, values, weight, x, scale=0.25):
    kind, sur = OUTPUTS[out]
    if kind == COMPLEX:
        return plan.simulate_complex(values, want_field=True, want_real=False, weight=weight, scale=scale)[0]
    if kind == REAL:
        return plan.simulate_complex(values, want_field=False, want_real=True, weight=weight, scale=scale)[1]
    if kind == PHASE:
        return plan.phase_backward(values, x, weight=weight, scale=scale)
    if kind == LEVELS:
        return plan.phase_levels_backward(values, x, NLEVELS, weight=weight, scale=scale)
    return plan.threshold_backward(values, x, weight=weight, scale=scale, surrogate=sur[0], p0=sur[1], p1=sur[2])


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("out", list(OUTPUTS))
@pytest.mark.parametrize("name", list(CASES))
def test_backward_at_one_depth_is_the_single_depth_call_bit_for_bit(name, out, weighted):
    """the running sum starts from depth 0's value, never from 0.0f: env 0's first complex plane is all
    -0.0 (its B planes are signed zeros), and the int32 views compare the signs of the zeros too"""
    z = DEPTHS[1][0]
    v_np, w_np, x_np = backward_inputs(name, 1)
    v = torch.from_numpy(v_np.copy()).cuda()
    v[0, 0, 0] = torch.complex(torch.tensor(-0.0), torch.tensor(-0.0))
    w = torch.from_numpy(w_np.copy()).cuda() if weighted else None
    x = torch.from_numpy(x_np.copy()).cuda()
    got = stack_backward(stack_plan(name, DEPTHS[1]), out, v, w, x)
    want = single_backward(single_plan(name, z), out, v[0].contiguous(), w[0].contiguous() if weighted else None, x)
    torch.cuda.synchronize()
    assert got.dtype == want.dtype and got.shape == want.shape
    assert torch.equal(_bits(got), _bits(want))
    if out in ("field", "real"):
        zero = _bits(got[0, 0])
        assert bool(((zero == 0) | (zero == -2 ** 31)).all())       # the zero plane's gradient: signed zeros


def leaf_gradient64(out, g, x, vb=1.0):
    """the leaf's gradient from g = the summed adjoint field [B, C, N, N] complex128, float64 formulas"""
    kind, sur = OUTPUTS[out]
    if kind == COMPLEX:
        return g
    if kind == REAL:
        return g.real
    if kind == PHASE:
        return phase_gradient(g, x.astype(np.float64))
    if kind == LEVELS:
        return phase_gradient(g, quantize_np(x, NLEVELS)[2].astype(np.float64))
    return ste_gradient(g.real, x, vb, *sur)


@functools.lru_cache(maxsize=None)
def adjoint64(name, d, weighted, scale=0.25):
    """sum_d A(z_d)[scale w_d V_d], float64 [B, G P/2, N, N]"""
    n, g, p, b = CASES[name]
    zs = DEPTHS[d]
    v, w, _ = backward_inputs(name, d)
    wls = O.WL_RGB if g == 3 else O.WL_MONO
    q = p // 2
    total = np.zeros(v.shape[1:], np.complex128)
    for i, z in enumerate(zs):
        for k in range(g):
            h = O.transfer_function(n, n, O.PIXEL_PITCH, O.PIXEL_PITCH, wls[k], z)
            u = v[i, :, k * q:(k + 1) * q].astype(np.complex128)
            if weighted:
                u = scale * w[i, :, k, None].astype(np.float64) * u
            total[:, k * q:(k + 1) * q] += O.propagate(u, h)
    total.setflags(write=False)
    return total


BACKWARD64 = ([(n, o, d) for n in ("64rgb", "64p4") for o in OUTPUTS for d in (2, 3)] +
              [("256", "field", 3), ("256", "phase", 2), ("256", "ste_sigmoid", 3),
               ("896", "field", 2), ("896", "levels", 3), ("1024", "real", 3), ("1024", "phase", 2)])


@pytest.mark.parametrize("name, out, d", BACKWARD64)
def test_backward_sums_the_depths_against_float64(name, out, d):
    """the stack call and the route it replaces -- D single-depth calls added in float32 -- against the same
    float64 gradient on the same inputs.  The bound is the single-depth gradient tests' (FIELD_RTOL of
    max|gradient|); measured on an MI355X both routes sit near 3e-7 (profiles/focal_stack/new_tests_gpu.txt)."""
    zs = DEPTHS[d]
    v_np, w_np, x_np = backward_inputs(name, d)
    v, w, x = (torch.from_numpy(a.copy()).cuda() for a in (v_np, w_np, x_np))
    got = stack_backward(stack_plan(name, zs), out, v, w, x)
    g32 = sum(single_backward(single_plan(name, z), "field", v[i].contiguous(), w[i].contiguous(), x)
              for i, z in enumerate(zs))
    torch.cuda.synchronize()
    want = leaf_gradient64(out, adjoint64(name, d, True), x_np)
    route = leaf_gradient64(out, g32.cpu().numpy().astype(np.complex128), x_np)
    scale = np.max(np.abs(want))
    err = np.max(np.abs(got.cpu().numpy() - want)) / scale
    err_route = np.max(np.abs(route - want)) / scale
    print(f"FOCAL64 {name} {out} D={d}: stack {err:.3e}  D single-depth calls added in float32 {err_route:.3e}"
          f"  of max|gradient| = {scale:.3e}")
    assert scale > 0.0
    assert err <= FIELD_RTOL


@pytest.mark.parametrize("name, out", [("64rgb", "field"), ("64p4", "phase"), ("256", "real"), ("1024", "field")])
def test_backward_with_the_depths_permuted(name, out):
    """depths, values and weight permuted alike: the same sum in another float32 order -- within FIELD_RTOL of
    the float64 reference, and within that same bound of the unpermuted call (no equality is claimed)"""
    zs = DEPTHS[3]
    perm = [2, 0, 1]
    v_np, w_np, x_np = backward_inputs(name, 3)
    v, w, x = (torch.from_numpy(a.copy()).cuda() for a in (v_np, w_np, x_np))
    a = stack_backward(stack_plan(name, zs), out, v, w, x).cpu().numpy()
    pz = tuple(zs[i] for i in perm)
    b = stack_backward(stack_plan(name, pz), out, v[perm].contiguous(), w[perm].contiguous(), x).cpu().numpy()
    want = leaf_gradient64(out, adjoint64(name, 3, True), x_np)
    scale = np.max(np.abs(want))
    e_perm, e_pair = np.max(np.abs(b - want)) / scale, np.max(np.abs(b - a)) / scale
    print(f"FOCALPERM {name} {out}: permuted vs float64 {e_perm:.3e}, permuted vs unpermuted {e_pair:.3e}")
    assert e_perm <= FIELD_RTOL and e_pair <= FIELD_RTOL


# -- 3. chunking ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["real", "phase"])
def test_forward_in_chunks_gives_the_one_chunk_bits(kind):
    k = KIND_NAMES[kind]
    name, zs = "64rgb", DEPTHS[3]                 # B G = 9 jobs
    x_np, t_np = samples(name, k)
    x, target = torch.from_numpy(x_np.copy()).cuda(), torch.from_numpy(t_np.copy()).cuda()
    whole = raw_evaluate_stack(stack_plan(name, zs, 9), k, x, target)
    for max_jobs in (3, 7):                       # one env, two envs per chunk
        parts = raw_evaluate_stack(stack_plan(name, zs, max_jobs), k, x, target)
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(parts[:2], whole[:2]))
        assert torch.equal(parts[2], whole[2])


@pytest.mark.parametrize("out", ["field", "ste_window"])
def test_backward_in_chunks_gives_the_one_chunk_bits(out):
    name, zs = "64rgb", DEPTHS[3]                 # G D = 9 slots per env, B = 3
    v_np, w_np, x_np = backward_inputs(name, 3)
    v, w, x = (torch.from_numpy(a.copy()).cuda() for a in (v_np, w_np, x_np))
    whole = stack_backward(stack_plan(name, zs, 27), out, v, w, x)
    parts = stack_backward(stack_plan(name, zs, 9), out, v, w, x)     # one env per chunk
    two = stack_backward(stack_plan(name, zs, 20), out, v, w, x)      # two envs, then one
    assert torch.equal(_bits(parts), _bits(whole)) and torch.equal(_bits(two), _bits(whole))


def test_backward_refuses_a_plan_too_small_for_one_env_before_anything_is_enqueued():
    from hbx import _lib
    name, zs = "64rgb", DEPTHS[3]
    plan = stack_plan(name, zs, 8)                # G D - 1
    v_np, w_np, _ = backward_inputs(name, 3)
    v, w = torch.from_numpy(v_np.copy()).cuda(), torch.from_numpy(w_np.copy()).cuda()
    out = torch.full(tuple(v.shape[1:]) + (2,), 123.0, dtype=torch.float32, device="cuda")
    leaf = _leaf(COMPLEX)
    rc = plan.lib.hbx_backward_stack(plan._h, _ptr(v), _ptr(w), 0.25, C.byref(leaf), None, v.shape[1], _ptr(out), None,
                                     _stream())
    torch.cuda.synchronize()
    assert rc == _lib.ERR_INVALID and b"max_jobs" in plan.lib.hbx_last_error()
    assert bool((out == 123.0).all())


def test_timer_slots_one_column_and_one_last_pass_record_per_depth():
    import hbx
    name, zs = "64p4", DEPTHS[3]
    n, g, p, b = CASES[name]
    plan = hbx.Plan(dev_cfg(name, 7e-3), max_jobs=b * g * 3)
    plan.set_depths(zs)
    x_np, t_np = samples(name, PHASE)
    x, target = torch.from_numpy(x_np.copy()).cuda(), torch.from_numpy(t_np.copy()).cuda()
    plan.set_timing(16)
    plan.evaluate_stack(x, PHASE, target)
    t = plan.read_timing()
    assert (t["k_rowfwd"][1], t["k_col"][1], t["k_rowinv"][1]) == (1, 3, 3)     # 1 + 2 D launches
    plan.set_timing(16)
    v_np, w_np, xs = backward_inputs(name, 3)
    plan.backward_stack(torch.from_numpy(v_np.copy()).cuda(), PHASE, samples=torch.from_numpy(xs.copy()).cuda())
    t = plan.read_timing()
    assert (t["k_rowfwd"][1], t["k_col"][1], t["k_rowinv"][1]) == (3, 3, 1)     # 2 D + 1 launches
    plan.set_timing(0)
    plan.close()


# -- 4. the loss over the stack ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def device_stack(name, d):
    """(plan, intensity, target, chan_stats) of the case's phase leaf at D depths, on the device"""
    x_np, t_np = samples(name, PHASE)
    plan = stack_plan(name, DEPTHS[d])
    x, target = torch.from_numpy(x_np.copy()).cuda(), torch.from_numpy(t_np[:d].copy()).cuda()
    _, inten, stats = plan.evaluate_stack(x, PHASE, target, want_field=False)
    torch.cuda.synchronize()
    return plan, inten, target, stats


@pytest.mark.parametrize("rel", [REL_LSQ, REL_NONE], ids=["lsq", "none"])
@pytest.mark.parametrize("kind", [LOSS_MSE, LOSS_PSNR], ids=["mse", "psnr"])
@pytest.mark.parametrize("name, d", [("64rgb", 3), ("64p4", 2), ("256", 3)])
def test_loss_stack_is_the_float64_formula_on_the_device_statistics(name, d, kind, rel):
    n, g, p, b = CASES[name]
    plan, _, _, stats = device_stack(name, d)
    got = plan.loss_stack(stats, kind, rel).cpu().numpy()
    s = stats.cpu().numpy()
    for e in range(b):
        want = stack_loss(s[:, e], kind, rel, n * n)
        print(f"FOCALLOSS {name} D={d} kind={kind} rel={rel} env {e}: {got[e]:.9e} want {want:.9e}")
        if kind == LOSS_MSE:
            assert abs(got[e] - want) <= MSE_RTOL * want
        else:
            assert abs(got[e] - want) <= PSNR_ATOL


@pytest.mark.parametrize("rel", [REL_LSQ, REL_NONE], ids=["lsq", "none"])
@pytest.mark.parametrize("kind", [LOSS_MSE, LOSS_PSNR], ids=["mse", "psnr"])
def test_loss_stack_at_one_depth_is_hbx_loss_bit_for_bit(kind, rel):
    plan, inten, target, stats = device_stack("64rgb", 1)
    up = torch.tensor([1.0, -0.5, 2.0], dtype=torch.float64, device="cuda")
    assert torch.equal(plan.loss_stack(stats, kind, rel), plan.loss(stats[0].contiguous(), kind, rel))
    got = plan.loss_weight_stack(inten, target, stats, up, kind, rel)
    want = plan.loss_weight(inten[0].contiguous(), target[0].contiguous(), stats[0].contiguous(), up, kind, rel)
    assert torch.equal(_bits(got[0]), _bits(want))


@pytest.mark.parametrize("rel", [REL_LSQ, REL_NONE], ids=["lsq", "none"])
@pytest.mark.parametrize("kind", [LOSS_MSE, LOSS_PSNR], ids=["mse", "psnr"])
def test_loss_weight_stack_is_a_i_plus_c_t_with_one_pair_per_env(kind, rel):
    name, d = "64rgb", 3
    n, g, p, b = CASES[name]
    plan, inten, target, stats = device_stack(name, d)
    up = np.array([1.0, -0.5, 2.0])
    got = plan.loss_weight_stack(inten, target, stats, torch.from_numpy(up).cuda(), kind, rel).cpu().numpy()
    i64, t64, s = inten.cpu().numpy().astype(np.float64), target.cpu().numpy().astype(np.float64), stats.cpu().numpy()
    for e in range(b):
        a, c = stack_loss_coeffs(s[:, e], kind, rel, n * n, up[e])
        want = a * i64[:, e] + c * t64[:, e]
        assert np.max(np.abs(got[:, e] - want)) <= FIELD_RTOL * np.max(np.abs(want))
    ones = plan.loss_weight_stack(inten, target, stats, None, kind, rel)
    assert torch.equal(ones, plan.loss_weight_stack(inten, target, stats, torch.ones(b, dtype=torch.float64, device="cuda"),
                                                    kind, rel))


def test_a_degenerate_env_gets_an_all_zero_weight():
    name, d = "64rgb", 2
    n, g, p, b = CASES[name]
    plan, inten, target, stats = device_stack(name, d)
    inten, stats = inten.clone(), stats.clone()
    inten[:, 1] = 0.0                 # env 1 is dark at every depth: S_xy = S_xx = 0
    stats[:, 1, :, :2] = 0.0
    for kind in (LOSS_MSE, LOSS_PSNR):
        w = plan.loss_weight_stack(inten, target, stats, None, kind, REL_LSQ)
        assert bool((w[:, 1] == 0).all()) and bool(torch.isfinite(w).all()) and bool((w[:, 0] != 0).any())
    same = target.clone()             # I == T at every depth: MSE = 0, the PSNR's weight is zero, not infinite
    st = stats.clone()
    st[..., 0] = st[..., 1] = st[..., 2]
    w = plan.loss_weight_stack(same, same, st, None, LOSS_PSNR, REL_NONE)
    assert bool((w == 0).all())


# -- 5. errors -------------------------------------------------------------------------------------------
def test_errors():
    import hbx
    from hbx import _lib
    name = "64p4"
    n, g, p, b = CASES[name]
    lib = _lib.load()
    v_np, w_np, xs_np = backward_inputs(name, 2)
    v, xs = torch.from_numpy(v_np.copy()).cuda(), torch.from_numpy(xs_np.copy()).cuda()
    x_np, t_np = samples(name, COMPLEX)
    x, target = torch.from_numpy(x_np.copy()).cuda(), torch.from_numpy(t_np[:2].copy()).cuda()
    field = torch.full((2,) + tuple(x.shape) + (2,), 5.0, dtype=torch.float32, device="cuda")
    inten = torch.full((2, b, g, n, n), 5.0, dtype=torch.float32, device="cuda")
    stats = torch.full((2, b, g, 3), 5.0, dtype=torch.float64, device="cuda")
    gfield = torch.full(tuple(v.shape[1:]) + (2,), 5.0, dtype=torch.float32, device="cuda")
    grad = torch.full(tuple(v.shape[1:]), 5.0, dtype=torch.float32, device="cuda")
    loss = torch.full((b,), 5.0, dtype=torch.float64, device="cuda")
    cl, pl = _leaf(COMPLEX), _leaf(PHASE)

    def ev(plan, values=x, leaf=cl, tg=target, nb=b, f=field, i=inten, s=stats):
        return lib.hbx_evaluate_stack(plan._h, _ptr(values), C.byref(leaf) if leaf is not None else None, _ptr(tg), nb,
                                      _ptr(f), _ptr(i), _ptr(s), _stream())

    def bw(plan, values=v, leaf=cl, smp=None, nb=b, gf=gfield, gr=None):
        return lib.hbx_backward_stack(plan._h, _ptr(values), None, 1.0, C.byref(leaf) if leaf is not None else None,
                                      _ptr(smp), nb, _ptr(gf), _ptr(gr), _stream())

    # no depths set: INVALID, and the message names the depths
    bare = hbx.Plan(dev_cfg(name, 2e-3), max_jobs=2 * b * g)
    for call in (lambda: ev(bare), lambda: bw(bare),
                 lambda: lib.hbx_loss_stack(bare._h, _ptr(stats), b, LOSS_MSE, REL_LSQ, _ptr(loss), _stream()),
                 lambda: lib.hbx_loss_weight_stack(bare._h, _ptr(inten), _ptr(target), _ptr(stats), None, b, LOSS_MSE,
                                                   REL_LSQ, _ptr(inten), _stream())):
        assert call() == _lib.ERR_INVALID and b"depths" in lib.hbx_last_error()
    # a reduced-precision plan: UNSUPPORTED
    bare.set_depths(DEPTHS[2])
    bare.precision = _lib.PRECISION_BF16_STORE
    assert ev(bare) == _lib.ERR_UNSUPPORTED and bw(bare) == _lib.ERR_UNSUPPORTED
    bare.precision = _lib.PRECISION_F32
    plan = bare
    # null required pointers, an unknown kind, bad levels
    assert ev(plan, values=None) == _lib.ERR_INVALID and ev(plan, leaf=None) == _lib.ERR_INVALID
    assert ev(plan, leaf=_lib.Leaf(9, 0, 0.0, 0, 0.0, 0.0)) == _lib.ERR_INVALID
    assert ev(plan, tg=None) == _lib.ERR_INVALID               # chan_stats without a target
    assert ev(plan, s=None) == _lib.ERR_INVALID                # a target without chan_stats
    assert ev(plan, tg=None, s=None, i=None) == _lib.ERR_INVALID   # complex kinds: the intensity is the output then
    lv = _lib.Leaf(LEVELS, 1, 0.0, 0, 0.0, 0.0)
    assert ev(plan, values=xs, leaf=lv) == _lib.ERR_INVALID and b"levels" in lib.hbx_last_error()
    assert bw(plan, values=None) == _lib.ERR_INVALID and bw(plan, leaf=None) == _lib.ERR_INVALID
    # grad_field and grad: exactly one, the one the leaf kind writes; samples with the kinds that read them
    assert bw(plan, gf=gfield, gr=grad) == _lib.ERR_INVALID
    assert bw(plan, gf=None, gr=None) == _lib.ERR_INVALID
    assert bw(plan, gf=None, gr=grad) == _lib.ERR_INVALID      # a complex leaf writes grad_field
    assert bw(plan, leaf=pl, smp=xs, gf=gfield) == _lib.ERR_INVALID
    assert bw(plan, leaf=pl, smp=None, gf=None, gr=grad) == _lib.ERR_INVALID
    assert bw(plan, smp=xs) == _lib.ERR_INVALID                # a complex leaf has no samples
    bad_ste = _lib.Leaf(THRESHOLD, 0, 0.0, STE_SIGMOID, 0.0, 0.0)
    assert bw(plan, leaf=bad_ste, smp=xs, gf=None, gr=grad) == _lib.ERR_INVALID
    # n_env: 0 is OK before any buffer is looked at, negative is INVALID
    assert ev(plan, values=None, nb=0) == _lib.OK and bw(plan, values=None, nb=0) == _lib.OK
    assert ev(plan, nb=-1) == _lib.ERR_INVALID and bw(plan, nb=-1) == _lib.ERR_INVALID
    assert lib.hbx_loss_stack(plan._h, None, 0, LOSS_MSE, REL_LSQ, None, _stream()) == _lib.OK
    assert lib.hbx_loss_stack(plan._h, _ptr(stats), -1, LOSS_MSE, REL_LSQ, _ptr(loss), _stream()) == _lib.ERR_INVALID
    assert lib.hbx_loss_stack(plan._h, _ptr(stats), b, 7, REL_LSQ, _ptr(loss), _stream()) == _lib.ERR_INVALID
    assert lib.hbx_loss_stack(plan._h, None, b, LOSS_MSE, REL_LSQ, _ptr(loss), _stream()) == _lib.ERR_INVALID
    assert lib.hbx_loss_weight_stack(plan._h, _ptr(inten), None, _ptr(stats), None, b, LOSS_MSE, REL_LSQ, _ptr(inten),
                                     _stream()) == _lib.ERR_INVALID
    torch.cuda.synchronize()
    # nothing was enqueued by any refusal
    for t in (field, inten, stats, gfield, grad, loss):
        assert bool((t == 5.0).all())
    assert ev(plan) == _lib.OK and bw(plan) == _lib.OK            # and the well-formed calls run
    torch.cuda.synchronize()
    assert not bool((field == 5.0).all()) and not bool((gfield == 5.0).all())
    plan.close()
