"""The weighted complex first pass (hbx_simulate_complex_weighted) and hbx_intensity_real, through
hbx.Plan (ABI v15, additive).

hbx_simulate_complex_weighted propagates (scale * weight[env][group]) * values: the first pass forms
m = scale * w, re * m and im * m with one float32 multiply each as it loads the samples.  The same
three multiplies on the host give the samples hbx_simulate_complex would need, so the two calls
must agree bit for bit.  Checked here:
  1. weighted == pre-multiplied, field and real_part, at all four built sizes (896: the zero-filled
     slots; two groups with different weights and wavelengths: the group index), and the
     single-output calls == the two-output call;
  2. chunking by max_jobs: the weight's chunk stride (G N^2) differs from the planes' (G P/2 N^2);
  3. hbx_intensity_real == hbx_simulate_real's intensity bit for bit, chunked too;
  4. the float64 oracle at N = 64 and 256 within the project's single-propagation bound (2e-5 of
     max|want|, tests/test_gpu_real_field.py);
  5. argument checks.
Shapes: G = 2 (two wavelengths), P = 4 real planes = 2 complex planes per group, so two complex
planes share each weight image; B = 2 at N = 64 / 256, B = 1 at 896 / 1024."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import hbx_oracle as O  # noqa: E402

FIELD_RTOL = 2e-5
G, P = 2, 4                    # P real planes per group = P / 2 complex planes per group
WL2 = (638e-9, 450e-9)
BATCH = {64: 2, 256: 2, 896: 1, 1024: 1}
SIZES = [64, 256, 896, 1024]
SCALE = np.float32(0.37)


def dev_cfg(n, planes=P, groups=G):
    import hbx
    o = O.OpticsConfig(n, n, groups, planes, WL2[:groups])
    return hbx.OpticsConfig(n, n, groups, planes, tuple(o.wavelengths), o.dx, o.dy, o.z, o.tf_kind, o.field_kind,
                            o.rel_scale, o.peak)


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm GPU")
    import hbx
    hbx.load_library()
    yield


@functools.lru_cache(maxsize=None)
def _case(n, b):
    """(values complex64 [b, G P/2, n, n] in [-1, 1)^2, weight f32 [b, G, n, n] in [0.5, 1.5) -- another
    image for every (env, group) --, premultiplied complex64), read-only"""
    rng = np.random.default_rng(700 + n + b)
    shape = (b, G * (P // 2), n, n)
    re = (2.0 * rng.random(shape, dtype=np.float32) - 1.0).astype(np.float32)
    im = (2.0 * rng.random(shape, dtype=np.float32) - 1.0).astype(np.float32)
    w = (rng.random((b, G, n, n), dtype=np.float32) + np.float32(0.5)).astype(np.float32)
    m = (SCALE * w).astype(np.float32)                    # one f32 multiply
    mc = np.repeat(m, P // 2, axis=1)                     # complex plane c -> group c // (P / 2)
    u2 = np.empty(shape, np.complex64)
    u2.real = re * mc                                     # one f32 multiply each
    u2.imag = im * mc
    vals = np.empty(shape, np.complex64)
    vals.real, vals.imag = re, im
    for a in (vals, w, u2):
        a.setflags(write=False)
    return vals, w, u2


def _bits(t):
    a = t.cpu().numpy()
    return a.view(np.float32) if np.iscomplexobj(a) else a


# -- 1. weighted == pre-multiplied -----------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_weighted_equals_premultiplied_bitwise(n):
    import hbx
    b = BATCH[n]
    vals, w, u2 = _case(n, b)
    plan = hbx.Plan(dev_cfg(n), max_jobs=b * G)
    v, wt = torch.from_numpy(vals.copy()).cuda(), torch.from_numpy(w.copy()).cuda()
    field, real = plan.simulate_complex(v, want_field=True, want_real=True, weight=wt, scale=float(SCALE))
    f_only, none_r = plan.simulate_complex(v, weight=wt, scale=float(SCALE))
    none_f, r_only = plan.simulate_complex(v, want_field=False, want_real=True, weight=wt, scale=float(SCALE))
    want_f, want_r = plan.simulate_complex(torch.from_numpy(u2.copy()).cuda(), want_field=True, want_real=True)
    torch.cuda.synchronize()
    assert none_r is None and none_f is None
    assert field.dtype == torch.complex64 and real.dtype == torch.float32
    assert tuple(field.shape) == tuple(real.shape) == vals.shape
    gf, gr, wf, wr = _bits(field), _bits(real), _bits(want_f), _bits(want_r)
    print(f"N={n}: max|field - premultiplied| {np.max(np.abs(gf - wf)):.3e}, real_part {np.max(np.abs(gr - wr)):.3e}, "
          f"max|want| {np.max(np.abs(wf)):.3e}")
    assert np.max(np.abs(wf)) > 0.0
    assert np.array_equal(gf, wf)
    assert np.array_equal(gr, wr)
    assert np.array_equal(_bits(f_only), gf)
    assert np.array_equal(_bits(r_only), gr)
    # the two groups and envs differ (another weight and wavelength each), so a wrong index shows
    assert not np.array_equal(gr[0, 0], gr[0, P // 2])
    plan.close()


# -- 2. chunking -----------------------------------------------------------------------------------
def test_weighted_chunked_equals_one_launch():
    """n_env = 3 on a plan of max_jobs = G (one env per chunk) and on one of 3 G (one chunk)"""
    import hbx
    vals, w, _ = _case(64, 3)
    v, wt = torch.from_numpy(vals.copy()).cuda(), torch.from_numpy(w.copy()).cuda()
    small, big = hbx.Plan(dev_cfg(64), max_jobs=G), hbx.Plan(dev_cfg(64), max_jobs=3 * G)
    fs, rs = small.simulate_complex(v, want_field=True, want_real=True, weight=wt, scale=float(SCALE))
    fb, rb = big.simulate_complex(v, want_field=True, want_real=True, weight=wt, scale=float(SCALE))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(fs), _bits(fb))
    assert np.array_equal(_bits(rs), _bits(rb))
    assert not np.array_equal(_bits(rs)[2], _bits(rs)[0])
    small.close()
    big.close()


# -- 3. hbx_intensity_real -------------------------------------------------------------------------
def _real_values(n, b):
    rng = np.random.default_rng(800 + n + b)
    return (2.0 * rng.random((b, G * P, n, n), dtype=np.float32) - 1.0).astype(np.float32)


@pytest.mark.parametrize("n", SIZES)
def test_intensity_real_equals_simulate_real_intensity(n):
    import hbx
    b = BATCH[n]
    plan = hbx.Plan(dev_cfg(n), max_jobs=b * G)
    v = torch.from_numpy(_real_values(n, b)).cuda()
    got = plan.intensity_real(v)
    _, want = plan.simulate_real(v, want_intensity=True)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and tuple(got.shape) == (b, G, n, n)
    assert float(want.max()) > 0.0
    assert np.array_equal(got.cpu().numpy(), want.cpu().numpy())
    plan.close()


def test_intensity_real_chunked():
    import hbx
    v = torch.from_numpy(_real_values(64, 3)).cuda()
    small, big = hbx.Plan(dev_cfg(64), max_jobs=G), hbx.Plan(dev_cfg(64), max_jobs=3 * G)
    got = small.intensity_real(v)
    _, want = big.simulate_real(v, want_intensity=True)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want.cpu().numpy())
    assert not np.array_equal(got[2].cpu().numpy(), got[0].cpu().numpy())
    small.close()
    big.close()


# -- 4. the float64 oracle -------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 256])
def test_weighted_vs_oracle(n):
    import hbx
    b = BATCH[n]
    vals, w, _ = _case(n, b)
    ocfg = O.OpticsConfig(n, n, G, P, WL2)
    q = P // 2
    u = vals.astype(np.complex128) * (np.float64(SCALE) * np.repeat(w.astype(np.float64), q, axis=1))
    want = np.stack([np.concatenate([O.propagate(u[e, k * q:(k + 1) * q], ocfg.transfer(k)) for k in range(G)])
                     for e in range(b)])
    plan = hbx.Plan(dev_cfg(n), max_jobs=b * G)
    field, _ = plan.simulate_complex(torch.from_numpy(vals.copy()).cuda(), weight=torch.from_numpy(w.copy()).cuda(),
                                     scale=float(SCALE))
    torch.cuda.synchronize()
    err = np.max(np.abs(field.cpu().numpy() - want)) / np.max(np.abs(want))
    print(f"N={n}: weighted field err {err:.3e} of max|want|")
    assert err <= FIELD_RTOL
    plan.close()


# -- 5. argument checks ----------------------------------------------------------------------------
def test_c_abi_argument_checks():
    import hbx
    from hbx import _lib
    lib = _lib.load()
    plan = hbx.Plan(dev_cfg(64), max_jobs=G)
    v = torch.zeros((1, G * P // 2, 64, 64), dtype=torch.complex64, device="cuda")
    w = torch.ones((1, G, 64, 64), dtype=torch.float32, device="cuda")
    f = torch.empty((1, G * P // 2, 64, 64, 2), dtype=torch.float32, device="cuda")
    vr = torch.zeros((1, G * P, 64, 64), dtype=torch.float32, device="cuda")
    it = torch.empty((1, G, 64, 64), dtype=torch.float32, device="cuda")
    h, null = plan._h, C.c_void_p(None)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    one = C.c_float(1.0)
    assert lib.hbx_simulate_complex_weighted(h, p(v), p(w), one, 1, p(f), null, null) == _lib.OK
    assert lib.hbx_simulate_complex_weighted(h, p(v), null, one, 1, p(f), null, null) == _lib.ERR_INVALID
    assert lib.hbx_simulate_complex_weighted(h, null, p(w), one, 1, p(f), null, null) == _lib.ERR_INVALID
    assert lib.hbx_simulate_complex_weighted(h, p(v), p(w), one, 1, null, null, null) == _lib.ERR_INVALID
    assert lib.hbx_simulate_complex_weighted(h, null, null, one, 0, null, null, null) == _lib.OK
    assert lib.hbx_simulate_complex_weighted(h, p(v), p(w), one, -1, p(f), null, null) == _lib.ERR_INVALID
    assert lib.hbx_intensity_real(h, p(vr), 1, p(it), null) == _lib.OK
    assert lib.hbx_intensity_real(h, null, 1, p(it), null) == _lib.ERR_INVALID
    assert lib.hbx_intensity_real(h, p(vr), 1, null, null) == _lib.ERR_INVALID
    assert lib.hbx_intensity_real(h, null, 0, null, null) == _lib.OK
    assert lib.hbx_intensity_real(h, p(vr), -1, p(it), null) == _lib.ERR_INVALID
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        plan.simulate_complex(v, want_field=False, want_real=False, weight=w)
    plan.close()


def test_reduced_precision_plan_is_unsupported():
    import hbx
    from hbx import _lib
    plan = hbx.Plan(dev_cfg(64), max_jobs=G, precision=_lib.PRECISION_BF16_STORE)
    v = torch.zeros((1, G * P // 2, 64, 64), dtype=torch.complex64, device="cuda")
    w = torch.ones((1, G, 64, 64), dtype=torch.float32, device="cuda")
    vr = torch.zeros((1, G * P, 64, 64), dtype=torch.float32, device="cuda")
    with pytest.raises(_lib.HbxError) as e:
        plan.simulate_complex(v, weight=w)
    assert e.value.code == _lib.ERR_UNSUPPORTED
    with pytest.raises(_lib.HbxError) as e:
        plan.intensity_real(vr)
    assert e.value.code == _lib.ERR_UNSUPPORTED
    plan.precision = _lib.PRECISION_F32
    plan.simulate_complex(v, weight=w)
    plan.intensity_real(vr)
    plan.close()


def test_weight_argument_checks():
    import hbx
    plan = hbx.Plan(dev_cfg(64), max_jobs=G)
    v = torch.zeros((1, G * P // 2, 64, 64), dtype=torch.complex64, device="cuda")
    w = torch.ones((1, G, 64, 64), dtype=torch.float32, device="cuda")
    plan.simulate_complex(v, weight=w)
    with pytest.raises(ValueError):     # one image per group, not per plane
        plan.simulate_complex(v, weight=torch.ones((1, G * P // 2, 64, 64), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        plan.simulate_complex(v, weight=w[:, :1])
    with pytest.raises(TypeError):
        plan.simulate_complex(v, weight=w.double())
    with pytest.raises(ValueError):
        plan.simulate_complex(v, weight=w.cpu())
    with pytest.raises(ValueError):
        plan.simulate_complex(v, weight=w.transpose(2, 3))
    with pytest.raises(TypeError):
        plan.intensity_real(v)
    with pytest.raises(ValueError):
        plan.intensity_real(torch.zeros((1, G, 64, 64), dtype=torch.float32, device="cuda"))
    plan.close()
