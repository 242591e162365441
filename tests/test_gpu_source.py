"""Illumination fields through the C-ABI (Plan.source_field / evaluate_source / backward_source).

The forward's first pass forms u = s f(x) as it loads the leaf's samples and the source row; the backward's
last pass multiplies the back-propagated plane by conj(s) before the leaf's gradient formula.  Model:
tests/_source_model.py (float64, from O.propagate / OpticsConfig.transfer) on the float64 of the float32
inputs, so no input rounding enters a comparison.  Bounds are the project's: 2e-5 of the normalising
maximum (FIELD_RTOL) and "new <= 2 x parent", the parent being simulate_complex on the host-formed
complex64 u (forward) or simulate_complex on the plan for -z followed by conj(s) g and the leaf's formula
in float64 on the host (backward).

Shapes (N, G, Q complex planes per group): (64, 3, 2) group indexing, (256, 1, 1), (256, 1, 3) the R = 16
last pass double-buffers plane pairs, (896, 1, 2) padding slots, (1024, 1, 2) the R = 32 kernels.  The test
source differs per group: a Gaussian envelope times a tilted phase, modulus <= 1, exactly 0 outside a disc
of radius 0.4 N -- the zeros are part of the test."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import hbx_oracle as O  # noqa: E402
from tests import _source_model as M  # noqa: E402

FIELD_RTOL = 2e-5
TAU, LEVELS = 0.5, 8
VA, VB = 1.0, -2.0          # the thresholded kind runs on a FIELD_PHASE plan: u = 1 - 2 [x >= tau]

# name: (N, G, Q)
CASES = {"64": (64, 3, 2), "256q1": (256, 1, 1), "256q3": (256, 1, 3), "896": (896, 1, 2), "1024": (1024, 1, 2)}
ALL = list(CASES)
BACKWARD = ["64", "256q3", "896", "1024"]
KINDS = ["complex", "real", "threshold", "phase", "levels"]
# the backward's cases: (model kind, surrogate, p0, p1)
GRADS = {"complex": ("complex", None, 0.0, 0.0), "real": ("real", None, 0.0, 0.0), "phase": ("phase", None, 0.0, 0.0),
         "levels": ("levels", None, 0.0, 0.0), "ste-window": ("threshold", "window", 0.25, 0.75),
         "ste-sigmoid": ("threshold", "sigmoid", TAU, 4.0)}


def leaf_of(kind):
    from hbx import _lib
    return {"complex": _lib.LEAF_COMPLEX, "real": _lib.LEAF_REAL, "threshold": _lib.LEAF_THRESHOLD,
            "phase": _lib.LEAF_PHASE, "levels": _lib.LEAF_PHASE_LEVELS}[kind]


def ocfg_for(name, kind="complex"):
    n, g, q = CASES[name]
    return O.OpticsConfig(n, n, g, 2 * q, O.WL_RGB if g == 3 else O.WL_MONO,
                          field_kind=O.FIELD_PHASE if kind == "threshold" else O.FIELD_AMPLITUDE)


def dev_cfg(o, z=None):
    import hbx
    return hbx.OpticsConfig(o.height, o.width, o.groups, o.planes, tuple(o.wavelengths), o.dx, o.dy,
                            o.z if z is None else z, o.tf_kind, o.field_kind, o.rel_scale, o.peak)


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm GPU")
    import hbx
    hbx.load_library()
    yield


@functools.lru_cache(maxsize=None)
def _source(n, g):
    """complex64 [G, N, N], read-only: exp(-r^2 / (0.3 N)^2) times a tilt that differs per group, 0 outside
    the disc r <= 0.4 N"""
    yy, xx = np.mgrid[:n, :n].astype(np.float64) - (n - 1) / 2.0
    r2 = xx ** 2 + yy ** 2
    s = np.stack([np.exp(-r2 / (0.3 * n) ** 2) * np.exp(2j * np.pi * ((0.11 + 0.05 * k) * xx - (0.07 + 0.03 * k) * yy))
                  for k in range(g)])
    s[:, r2 > (0.4 * n) ** 2] = 0.0
    s = s.astype(np.complex64)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def _samples(name, kind, b=1):
    """the siblings' generators, float32 / complex64 [B, G Q, N, N], read-only: phase in [-1, 1), real in
    [0, 1), complex in the square [-1, 1)^2"""
    n, g, q = CASES[name]
    rng = np.random.default_rng(4100 + n + 7 * q + 13 * KINDS.index(kind) + b)
    shape = (b, g * q, n, n)
    if kind == "complex":
        x = ((2 * rng.random(shape, dtype=np.float32) - 1) + 1j * (2 * rng.random(shape, dtype=np.float32) - 1)).astype(np.complex64)
    elif kind in ("phase", "levels"):
        x = (2.0 * rng.random(shape, dtype=np.float32) - 1.0).astype(np.float32)
    else:
        x = rng.random(shape, dtype=np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _target(name, b=1):
    n, g, _ = CASES[name]
    t = np.random.default_rng(4200 + n + b).random((b, g, n, n), dtype=np.float32)
    t.setflags(write=False)
    return t


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _quantized(x_dev):
    import hbx
    return hbx.quantize_phase(x_dev, LEVELS, want_levels=False, want_samples=True).cpu().numpy()


def _leaf_kw(kind):
    return dict(levels=LEVELS if kind == "levels" else None, threshold=TAU if kind == "threshold" else 0.0)


def _err(got, want, scale=None):
    return float(np.max(np.abs(got - want)) / (np.max(np.abs(want)) if scale is None else scale))


def _same(a, b):
    a = torch.view_as_real(a) if a.is_complex() else a
    b = torch.view_as_real(b) if b.is_complex() else b
    return torch.equal(a, b)


# -- 1. the field against the model ---------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ALL)
def test_field_vs_model_and_the_complex_route(name, kind):
    import hbx
    n, g, q = CASES[name]
    ocfg = ocfg_for(name, kind)
    x_np, s_np = _samples(name, kind), _source(n, g)
    x, s = _dev(x_np), _dev(s_np)
    qs = _quantized(x)[0] if kind == "levels" else None
    u64 = M.sourced(kind, x_np[0], s_np, q=qs, tau=TAU, va=VA, vb=VB)
    want = M.forward(ocfg, u64)
    plan = hbx.Plan(dev_cfg(ocfg), max_jobs=g)
    field, inten, stats = plan.evaluate_source(x, leaf_of(kind), s, **_leaf_kw(kind))
    ref, _ = plan.simulate_complex(_dev(u64.astype(np.complex64)[None]))
    torch.cuda.synchronize()
    assert stats is None and field.dtype == torch.complex64 and tuple(field.shape) == (1, g * q, n, n)
    e_new, e_ref = _err(field[0].cpu().numpy(), want), _err(ref[0].cpu().numpy(), want)
    e_int = _err(inten[0].cpu().numpy().astype(np.float64), M.intensity(ocfg, want))
    print(f"{name} {kind}: evaluate_source err {e_new:.3e}, simulate_complex(host u) err {e_ref:.3e} of max|field|; "
          f"intensity {e_int:.3e} of max I")
    assert e_new <= FIELD_RTOL
    assert e_new <= 2.0 * e_ref
    assert e_int <= FIELD_RTOL
    plan.close()


# -- 2. bit identity with the materialised route ----------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ALL)
def test_evaluate_source_is_evaluate_complex_on_source_field_bit_for_bit(name, kind):
    import hbx
    n, g, q = CASES[name]
    ocfg = ocfg_for(name, kind)
    x, s, target = _dev(_samples(name, kind)), _dev(_source(n, g)), _dev(_target(name))
    plan = hbx.Plan(dev_cfg(ocfg), max_jobs=g)
    u = plan.source_field(x, leaf_of(kind), s, **_leaf_kw(kind))
    f_s, i_s, st_s = plan.evaluate_source(x, leaf_of(kind), s, target, **_leaf_kw(kind))
    f_c, i_c, st_c, _ = plan.evaluate_complex(u, target)
    _, i_alone, none = plan.evaluate_source(x, leaf_of(kind), s, want_field=False, **_leaf_kw(kind))
    torch.cuda.synchronize()
    assert none is None and u.dtype == torch.complex64 and tuple(u.shape) == (1, g * q, n, n)
    assert float(i_s.max()) > 0.0
    assert _same(f_s, f_c) and _same(i_s, i_c) and _same(st_s, st_c) and _same(i_alone, i_c)
    plan.close()


def test_evaluate_source_with_a_pixel_weight_is_evaluate_pw_on_source_field():
    import hbx
    from hbx import _lib
    name, kind = "64", "complex"
    n, g, q = CASES[name]
    x, s, target = _dev(_samples(name, kind)), _dev(_source(n, g)), _dev(_target(name))
    pw = _dev(np.random.default_rng(4300).random((1, g, n, n), dtype=np.float32))
    pw[:, :, :9] = 0.0
    plan = hbx.Plan(dev_cfg(ocfg_for(name)), max_jobs=g)
    u = plan.source_field(x, _lib.LEAF_COMPLEX, s)
    f_s, i_s, st_s = plan.evaluate_source(x, _lib.LEAF_COMPLEX, s, target, pixel_weight=pw)
    f_c, i_c, st_c = plan.evaluate_pw(u, _lib.LEAF_COMPLEX, target, pw)
    _, _, st_plain = plan.evaluate_source(x, _lib.LEAF_COMPLEX, s, target)
    torch.cuda.synchronize()
    assert _same(f_s, f_c) and _same(i_s, i_c) and _same(st_s, st_c)
    assert not _same(st_s, st_plain)
    plan.close()


# -- 3. a source of 1 + 0i is no source ---------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["complex", "phase", "levels"])
@pytest.mark.parametrize("name", ALL)
def test_unit_source_equals_the_unsourced_call(name, kind):
    """under ==, not bitwise: fmaf(fr, 1, -(fi * 0)) and fmaf(fr, 0, fi * 1) may turn the sign of a zero"""
    import hbx
    n, g, q = CASES[name]
    x, target = _dev(_samples(name, kind)), _dev(_target(name))
    one = torch.ones((g, n, n), dtype=torch.complex64, device="cuda")
    plan = hbx.Plan(dev_cfg(ocfg_for(name)), max_jobs=g)
    f_s, i_s, st_s = plan.evaluate_source(x, leaf_of(kind), one, target, **_leaf_kw(kind))
    if kind == "complex":
        f_u, i_u, st_u, _ = plan.evaluate_complex(x, target)
    elif kind == "phase":
        f_u, i_u, st_u, _ = plan.evaluate_phase(x, target)
    else:
        f_u, i_u, st_u, _ = plan.evaluate_phase_levels(x, LEVELS, target)
    torch.cuda.synchronize()
    assert bool((f_s == f_u).all()) and bool((i_s == i_u).all()) and bool((st_s == st_u).all())
    plan.close()


# -- 4. dark pixels -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["64", "896"])
def test_source_field_is_zero_where_the_source_is(name, kind):
    import hbx
    n, g, q = CASES[name]
    x_np, s_np = _samples(name, kind), _source(n, g)
    plan = hbx.Plan(dev_cfg(ocfg_for(name, kind)), max_jobs=g)
    u = plan.source_field(_dev(x_np), leaf_of(kind), _dev(s_np), **_leaf_kw(kind)).cpu().numpy()
    dark = M.per_plane(s_np == 0, q)
    assert dark.any() and not dark.all()
    assert np.all(u[0][dark] == 0) and np.any(u[0][~dark] != 0)
    qs = _quantized(_dev(x_np))[0] if kind == "levels" else None
    u64 = M.sourced(kind, x_np[0], s_np, q=qs, tau=TAU, va=VA, vb=VB)
    assert _err(u[0], u64) <= 4 * 2.0 ** -24 * (3 if kind in ("phase", "levels") else 1)   # product roundings (+ sincos)
    plan.close()


def test_896_phase_plane_of_zeros_has_no_constant_term():
    """x = 0 under the test source is u = s: a lane's four padding slots hold 0, not s f(0) of some pixel and
    not exp(0) = 1 -- a one there puts a constant into the row FFT and misses the bound by orders of
    magnitude (the 896 remark of the unsourced sibling test, with a source)."""
    import hbx
    from hbx import _lib
    n, g, q = CASES["896"]
    ocfg = ocfg_for("896")
    s_np = _source(n, g)
    x = torch.zeros((1, g * q, n, n), dtype=torch.float32, device="cuda")
    want = M.forward(ocfg, M.sourced("phase", np.zeros((g * q, n, n), np.float32), s_np))
    plan = hbx.Plan(dev_cfg(ocfg), max_jobs=g)
    field, _, _ = plan.evaluate_source(x, _lib.LEAF_PHASE, _dev(s_np))
    torch.cuda.synchronize()
    e = _err(field[0].cpu().numpy(), want)
    print(f"896, x = 0: field err {e:.3e} of max|field|")
    assert e <= FIELD_RTOL
    plan.close()


# -- 5. the backward against the model ------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("grad_kind", list(GRADS))
@pytest.mark.parametrize("name", BACKWARD)
def test_backward_vs_model_and_the_host_route(name, grad_kind, weighted):
    """Normalised as the sibling test of the kind normalises: max|g'| (complex, real), pi max|g'| (phase,
    L-level), |vb| max(s) max|g'| with max(s) = 1 for both surrogates here (window: 1; sigmoid: k / 4, k = 4)."""
    import hbx
    from hbx import _lib
    kind, surrogate, p0, p1 = GRADS[grad_kind]
    n, g, q = CASES[name]
    ocfg = ocfg_for(name, kind)
    s_np = _source(n, g)
    rng = np.random.default_rng(4400 + n + q)
    v_np = ((2 * rng.random((1, g * q, n, n), dtype=np.float32) - 1) +
            1j * (2 * rng.random((1, g * q, n, n), dtype=np.float32) - 1)).astype(np.complex64)
    needs = kind in ("phase", "levels", "threshold")
    x_np = _samples(name, kind) if needs else None
    x = _dev(x_np) if needs else None
    w_np = _target(name) if weighted else None
    w, scale = (_dev(w_np) if weighted else None), 2.0 / q
    qs = _quantized(x)[0] if kind == "levels" else None
    leaf = dict(x=x_np[0] if needs else None, q=qs, vb=VB, surrogate=surrogate, p0=p0, p1=p1)
    gp, want = M.backward(ocfg, kind, v_np[0], s_np, weight=w_np[0] if weighted else None, scale=scale, **leaf)
    ste = {} if surrogate is None else dict(surrogate=_lib.STE_WINDOW if surrogate == "window" else _lib.STE_SIGMOID,
                                            p0=p0, p1=p1)
    plan = hbx.Plan(dev_cfg(ocfg, z=-ocfg.z), max_jobs=g)
    grad = plan.backward_source(_dev(v_np), leaf_of(kind), _dev(s_np), samples=x, weight=w, scale=scale,
                                levels=LEVELS if kind == "levels" else None, **ste)
    again = plan.backward_source(_dev(v_np), leaf_of(kind), _dev(s_np), samples=x, weight=w, scale=scale,
                                 levels=LEVELS if kind == "levels" else None, **ste)
    gfield, _ = plan.simulate_complex(_dev(v_np), weight=w, scale=scale)
    torch.cuda.synchronize()
    assert _same(grad, again)
    assert grad.dtype == (torch.complex64 if kind == "complex" else torch.float32) and tuple(grad.shape) == v_np.shape
    g64 = gfield[0].cpu().numpy().astype(np.complex128)
    host = M.leaf_gradient(kind, np.conj(M.per_plane(s_np.astype(np.complex128), q)) * g64, **leaf)
    norm = float(np.max(np.abs(gp))) * {"complex": 1.0, "real": 1.0, "phase": np.pi, "levels": np.pi, "threshold": abs(VB)}[kind]
    got = grad[0].cpu().numpy()
    got = got.astype(np.complex128 if kind == "complex" else np.float64)
    e_new, e_ref = _err(got, want, norm), _err(host, want, norm)
    print(f"{name} {grad_kind} weighted={weighted}: backward_source err {e_new:.3e}, host route err {e_ref:.3e} "
          f"of the norm {norm:.3e}")
    assert norm > 0.0
    assert e_new <= FIELD_RTOL
    assert e_new <= 2.0 * e_ref
    if grad_kind == "ste-window":                     # a closed gate stores +0.0, the sign bit too
        closed = (x_np[0] < p0) | (x_np[0] > p1)
        assert closed.any() and np.all(grad[0].cpu().numpy().view(np.int32)[closed] == 0)
    dark = M.per_plane(s_np == 0, q)
    assert np.all(got[dark] == 0)                     # no light, no gradient
    plan.close()


def test_closed_window_gate_stores_plus_zero_whatever_the_gradient_holds():
    """values with an inf make every back-propagated sample non-finite; the closed gate is a select"""
    import hbx
    from hbx import _lib
    name = "64"
    n, g, q = CASES[name]
    x_np = _samples(name, "threshold")
    v = torch.ones((1, g * q, n, n), dtype=torch.complex64, device="cuda")
    v[:, :, 3, 5] = float("inf")
    plan = hbx.Plan(dev_cfg(ocfg_for(name, "threshold"), z=-ocfg_for(name).z), max_jobs=g)
    grad = plan.backward_source(v, _lib.LEAF_THRESHOLD, _dev(_source(n, g)), samples=_dev(x_np),
                                surrogate=_lib.STE_WINDOW, p0=0.25, p1=0.75)
    torch.cuda.synchronize()
    got = grad.cpu().numpy()
    closed = (x_np < 0.25) | (x_np > 0.75)
    assert np.all(got.view(np.int32)[closed] == 0)
    assert not np.all(np.isfinite(got[~closed]))
    plan.close()


# -- 6. chunking, n_env, error paths ---------------------------------------------------------------------------
def test_chunking_by_max_jobs():
    """B = 3 on a plan of one env per chunk (max_jobs = G, three chunks) against a plan that takes all three
    at once: every output of the three calls bit for bit; the source does not advance with the chunk."""
    import hbx
    from hbx import _lib
    name = "64"
    n, g, q = CASES[name]
    s = _dev(_source(n, g))
    x, xc, target = _dev(_samples(name, "phase", 3)), _dev(_samples(name, "complex", 3)), _dev(_target(name, 3))
    xr = _dev(_samples(name, "real", 3))
    out = []
    for jobs in (g, 3 * g):
        plan = hbx.Plan(dev_cfg(ocfg_for(name)), max_jobs=jobs)
        res = [plan.source_field(x, _lib.LEAF_PHASE, s)]
        res += list(plan.evaluate_source(x, _lib.LEAF_PHASE, s, target))
        res += list(plan.evaluate_source(xr, _lib.LEAF_REAL, s, target))
        res += list(plan.evaluate_source(xc, _lib.LEAF_COMPLEX, s, target, pixel_weight=target))
        res.append(plan.backward_source(xc, _lib.LEAF_PHASE, s, samples=x, weight=target, scale=0.5))
        res.append(plan.backward_source(xc, _lib.LEAF_COMPLEX, s))
        res.append(plan.backward_source(xc, _lib.LEAF_REAL, s))
        torch.cuda.synchronize()
        out.append(res)
        plan.close()
    for a, b in zip(*out):
        assert _same(a, b)
    assert not _same(out[0][-1][2], out[0][-1][0])      # the envs differ


def test_n_env_zero_is_ok_and_a_null_source_is_invalid():
    import hbx
    from hbx import _lib
    from hbx.plan import _ptr, _stream
    ocfg = O.OpticsConfig(64, 64, 1, 2, O.WL_MONO)
    plan = hbx.Plan(dev_cfg(ocfg), max_jobs=1)
    lib, h, st = plan.lib, plan._h, _stream(None)
    x = torch.zeros((1, 1, 64, 64), dtype=torch.float32, device="cuda")
    v = torch.ones((1, 1, 64, 64), dtype=torch.complex64, device="cuda")
    s = torch.ones((1, 64, 64), dtype=torch.complex64, device="cuda")
    sentinel = 7.0
    f = torch.full((1, 1, 64, 64, 2), sentinel, dtype=torch.float32, device="cuda")
    i = torch.full((1, 1, 64, 64), sentinel, dtype=torch.float32, device="cuda")
    gr = torch.full((1, 1, 64, 64), sentinel, dtype=torch.float32, device="cuda")
    leaf = _lib.Leaf(_lib.LEAF_PHASE, 0, 0.0, 0, 0.0, 0.0)
    lp = C.byref(leaf)
    inv = _lib.ERR_INVALID
    # n_env == 0 is OK and does nothing; < 0 is invalid
    assert lib.hbx_source_field(h, _ptr(x), lp, _ptr(s), 0, _ptr(f), st) == _lib.OK
    assert lib.hbx_evaluate_source(h, _ptr(x), lp, _ptr(s), None, None, 0, _ptr(f), _ptr(i), None, st) == _lib.OK
    assert lib.hbx_backward_source(h, _ptr(v), None, 1.0, lp, _ptr(s), _ptr(x), 0, None, _ptr(gr), st) == _lib.OK
    assert lib.hbx_source_field(h, _ptr(x), lp, _ptr(s), -1, _ptr(f), st) == inv
    # a null source names itself
    for call in (lambda: lib.hbx_source_field(h, _ptr(x), lp, None, 1, _ptr(f), st),
                 lambda: lib.hbx_evaluate_source(h, _ptr(x), lp, None, None, None, 1, _ptr(f), _ptr(i), None, st),
                 lambda: lib.hbx_backward_source(h, _ptr(v), None, 1.0, lp, None, _ptr(x), 1, None, _ptr(gr), st)):
        assert call() == inv
        assert b"source" in lib.hbx_last_error()
    # null values, a null leaf, an unknown kind, levels outside [2, 256]
    bad_kind = _lib.Leaf(9, 0, 0.0, 0, 0.0, 0.0)
    bad_levels = _lib.Leaf(_lib.LEAF_PHASE_LEVELS, 1, 0.0, 0, 0.0, 0.0)
    assert lib.hbx_source_field(h, None, lp, _ptr(s), 1, _ptr(f), st) == inv
    assert lib.hbx_source_field(h, _ptr(x), None, _ptr(s), 1, _ptr(f), st) == inv
    assert lib.hbx_evaluate_source(h, _ptr(x), C.byref(bad_kind), _ptr(s), None, None, 1, _ptr(f), _ptr(i), None, st) == inv
    assert lib.hbx_backward_source(h, _ptr(v), None, 1.0, C.byref(bad_levels), _ptr(s), _ptr(x), 1, None, _ptr(gr), st) == inv
    # the backward's output rules
    assert lib.hbx_backward_source(h, _ptr(v), None, 1.0, lp, _ptr(s), _ptr(x), 1, _ptr(f), _ptr(gr), st) == inv
    assert lib.hbx_backward_source(h, _ptr(v), None, 1.0, lp, _ptr(s), None, 1, None, _ptr(gr), st) == inv
    plan.precision = _lib.PRECISION_BF16_STORE
    assert lib.hbx_evaluate_source(h, _ptr(x), lp, _ptr(s), None, None, 1, _ptr(f), _ptr(i), None, st) == _lib.ERR_UNSUPPORTED
    plan.precision = _lib.PRECISION_F32
    torch.cuda.synchronize()
    for t in (f, i, gr):
        assert bool((t == sentinel).all()), "a refused call wrote an output"
    assert lib.hbx_evaluate_source(h, _ptr(x), lp, _ptr(s), None, None, 1, _ptr(f), _ptr(i), None, st) == _lib.OK
    assert lib.hbx_backward_source(h, _ptr(v), None, 1.0, lp, _ptr(s), _ptr(x), 1, None, _ptr(gr), st) == _lib.OK
    torch.cuda.synchronize()
    for t in (f, i, gr):
        assert not bool((t == sentinel).any())
    plan.close()
