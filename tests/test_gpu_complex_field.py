"""Propagation of complex fields (hbx_simulate_complex, ABI v15 additive).

The first pass reads complex64 samples, the last pass recombines each plane pair with one inverse
row FFT per complex plane and writes the field and / or its real part.  Checked here:
  1. the float64 oracle on continuous complex samples within the project's field tolerance
     (tests/test_gpu_real_field.py: 2e-5 of max|want|), real_part against max|Re want|, real_part
     == field.real bit for bit, and single-output calls == the two-output call bit for bit;
  2. the lane-to-pixel and re / im map on single samples;
  3. chunking by max_jobs;
  4. consistency with hbx_simulate_real on a field with zero imaginary part (both within the
     tolerance of the same oracle field; not bit equality, the pair partner differs);
  5. adjointness <g, A u> = <A^H g, u> with A on the z plan and A^H on the -z plan, no oracle;
  6. the documented limits and argument errors.
Samples are drawn as float32 and handed to the oracle as their float64 upcast, so no input
rounding enters a comparison.  Shapes (N, G, P) are the smallest that cover the plane loop."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import hbx_oracle as O  # noqa: E402

FIELD_RTOL = 2e-5

# (N, G, P): P real planes per group = P / 2 complex planes per group
SHAPES = {64: (3, 2), 256: (1, 4), 896: (1, 2), 1024: (1, 4)}
SIZES = [64, 256, 896, 1024]


def ocfg_for(n, planes=None):
    g, p = SHAPES[n]
    return O.OpticsConfig(n, n, g, planes or p, O.WL_RGB if g == 3 else O.WL_MONO)


def dev_cfg(o: O.OpticsConfig, planes=None, z=None):
    import hbx
    return hbx.OpticsConfig(o.height, o.width, o.groups, planes or o.planes, tuple(o.wavelengths), o.dx, o.dy,
                            o.z if z is None else z, o.tf_kind, o.field_kind, o.rel_scale, o.peak)


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm GPU")
    import hbx
    hbx.load_library()
    yield


def _complex_samples(rng, shape, signed):
    re = rng.random(shape, dtype=np.float32)
    im = rng.random(shape, dtype=np.float32)
    if signed:
        re, im = (2.0 * re - 1.0).astype(np.float32), (2.0 * im - 1.0).astype(np.float32)
    return (re + 1j * im).astype(np.complex64)


def _oracle_field(ocfg, u, per_group):
    """u [G * per_group, N, N] (any dtype) -> complex128 field of every plane"""
    u = np.asarray(u)
    u64 = u.astype(np.complex128 if np.iscomplexobj(u) else np.float64)
    return np.concatenate([O.propagate(u64[k * per_group:(k + 1) * per_group], ocfg.transfer(k))
                           for k in range(ocfg.groups)])


# -- 1. continuous complex samples against the float64 oracle --------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_case(n, kind):
    """(values complex64 [1, G * P / 2, N, N], want complex128 [G * P / 2, N, N]), read-only"""
    ocfg = ocfg_for(n)
    q = ocfg.planes // 2
    rng = np.random.default_rng(300 + n + (0 if kind == "unit" else 1))
    vals = _complex_samples(rng, (1, ocfg.groups * q, n, n), kind == "signed")
    want = _oracle_field(ocfg, vals[0], q)
    vals.setflags(write=False)
    want.setflags(write=False)
    return vals, want


@pytest.mark.parametrize("kind", ["unit", "signed"])
@pytest.mark.parametrize("n", SIZES)
def test_complex_samples_vs_oracle(n, kind):
    import hbx
    ocfg = ocfg_for(n)
    vals, want = _oracle_case(n, kind)
    plan = hbx.Plan(dev_cfg(ocfg), max_jobs=ocfg.groups)
    v = torch.from_numpy(vals.copy()).cuda()      # the cached case stays read-only
    field, real = plan.simulate_complex(v, want_field=True, want_real=True)
    f_only, none_r = plan.simulate_complex(v)
    none_f, r_only = plan.simulate_complex(v, want_field=False, want_real=True)
    torch.cuda.synchronize()
    assert none_r is None and none_f is None
    assert field.dtype == torch.complex64 and real.dtype == torch.float32
    assert tuple(field.shape) == tuple(real.shape) == vals.shape
    ef = np.max(np.abs(field[0].cpu().numpy() - want)) / np.max(np.abs(want))
    er = np.max(np.abs(real[0].cpu().numpy() - want.real)) / np.max(np.abs(want.real))
    print(f"N={n} {kind}: field err {ef:.3e} of max|want|, real_part err {er:.3e} of max|Re want|")
    assert ef <= FIELD_RTOL
    assert er <= FIELD_RTOL
    assert torch.equal(real, field.real)
    assert torch.equal(torch.view_as_real(f_only), torch.view_as_real(field))
    assert torch.equal(r_only, real)
    plan.close()


# -- 2. index map ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 896])
def test_single_sample_index_map(n):
    """One sample 0.37 - 0.21j in an otherwise zero env of two complex planes, at the four corners
    and (N/2, 31) of either plane (one env each): a swapped re / im, a wrong lane-to-pixel map or a
    swapped plane shows as the single-pixel response in the wrong place, phase or plane."""
    import hbx
    ocfg = O.OpticsConfig(n, n, 1, 4, O.WL_MONO)
    pix = [(0, 0), (0, n - 1), (n - 1, 0), (n - 1, n - 1), (n // 2, 31)]
    cases = [(pl, y, x) for pl in (0, 1) for (y, x) in pix]
    vals = np.zeros((len(cases), 2, n, n), np.complex64)
    for e, (pl, y, x) in enumerate(cases):
        vals[e, pl, y, x] = 0.37 - 0.21j
    plan = hbx.Plan(dev_cfg(ocfg), max_jobs=len(cases))
    field, _ = plan.simulate_complex(torch.from_numpy(vals).cuda())
    torch.cuda.synchronize()
    got = field.cpu().numpy()
    h = ocfg.transfer(0)
    for e, (pl, y, x) in enumerate(cases):
        want = O.propagate(vals[e].astype(np.complex128), h)
        err = np.max(np.abs(got[e] - want))
        assert err <= FIELD_RTOL * np.max(np.abs(want)), (pl, y, x, err)
        assert np.max(np.abs(got[e, 1 - pl])) <= FIELD_RTOL * np.max(np.abs(want)), (pl, y, x)
    plan.close()


def test_lazily_conjugated_values_are_read_conjugated():
    """values.conj() is a contiguous complex64 view with torch's conjugate bit set over the
    unconjugated memory: the plan must propagate conj(values), not what data_ptr() points at."""
    import hbx
    ocfg = ocfg_for(64)
    vals, _ = _oracle_case(64, "signed")
    want = _oracle_field(ocfg, np.conj(vals[0]), ocfg.planes // 2)
    plan = hbx.Plan(dev_cfg(ocfg), max_jobs=ocfg.groups)
    vc = torch.from_numpy(vals.copy()).cuda().conj()
    assert vc.is_conj() and vc.is_contiguous()
    field, real = plan.simulate_complex(vc, want_field=True, want_real=True)
    torch.cuda.synchronize()
    assert np.max(np.abs(field[0].cpu().numpy() - want)) <= FIELD_RTOL * np.max(np.abs(want))
    assert torch.equal(real, field.real)
    plan.close()


# -- 3. chunking -----------------------------------------------------------------------------------
def test_chunked_call_equals_single_env_calls():
    """max_jobs = 2, G = 1, B = 3: two chunks, the second starting at env 2 of every buffer"""
    import hbx
    ocfg = O.OpticsConfig(64, 64, 1, 2, O.WL_MONO)
    vals = torch.from_numpy(_complex_samples(np.random.default_rng(3), (3, 1, 64, 64), True)).cuda()
    plan = hbx.Plan(dev_cfg(ocfg), max_jobs=2)
    field, real = plan.simulate_complex(vals, want_field=True, want_real=True)
    for e in range(3):
        f1, r1 = plan.simulate_complex(vals[e:e + 1].contiguous(), want_field=True, want_real=True)
        assert torch.equal(torch.view_as_real(field[e]), torch.view_as_real(f1[0])), e
        assert torch.equal(real[e], r1[0]), e
    assert not torch.equal(real[2], real[0])
    plan.close()


# -- 4. consistency with the real path -------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_zero_imaginary_part_agrees_with_real_path(n):
    """P real planes through hbx_simulate_real (a plan of P planes) and the same P planes as
    complex samples with zero imaginary part (a plan of 2 P planes): both within the tolerance of
    the one oracle field."""
    import hbx
    ocfg = ocfg_for(n)
    g, p = ocfg.groups, ocfg.planes
    rng = np.random.default_rng(400 + n)
    a = (2.0 * rng.random((1, g * p, n, n), dtype=np.float32) - 1.0).astype(np.float32)
    want = _oracle_field(ocfg, a[0], p)
    scale = np.max(np.abs(want))
    rplan = hbx.Plan(dev_cfg(ocfg), max_jobs=g)
    f_real, _ = rplan.simulate_real(torch.from_numpy(a).cuda())
    torch.cuda.synchronize()
    f_real = f_real[0].cpu().numpy()
    rplan.close()
    cplan = hbx.Plan(dev_cfg(ocfg, planes=2 * p), max_jobs=g)
    f_cplx, _ = cplan.simulate_complex(torch.from_numpy(a.astype(np.complex64)).cuda())
    torch.cuda.synchronize()
    f_cplx = f_cplx[0].cpu().numpy()
    cplan.close()
    e_r = np.max(np.abs(f_real - want)) / scale
    e_c = np.max(np.abs(f_cplx - want)) / scale
    print(f"N={n}: real path err {e_r:.3e}, complex path err {e_c:.3e} of max|want|, "
          f"between them {np.max(np.abs(f_real - f_cplx)) / scale:.3e}")
    assert e_r <= FIELD_RTOL
    assert e_c <= FIELD_RTOL


# -- 5. adjointness --------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_minus_z_plan_is_the_adjoint(n):
    """Re<g, A u> = <u, Re(A^H g)> for real u, complex g: A u from hbx_simulate_real on the z plan,
    Re(A^H g) from hbx_simulate_complex(real_part) on the -z plan.  Each side's elements carry at
    most FIELD_RTOL of its maximum, so the sums differ by at most
    FIELD_RTOL (max|A u| sum|g| + max|r| sum|u|)."""
    import hbx
    ocfg = ocfg_for(n)
    g_, p = ocfg.groups, ocfg.planes
    rng = np.random.default_rng(500 + n)
    u = (2.0 * rng.random((1, g_ * p, n, n), dtype=np.float32) - 1.0).astype(np.float32)
    g = _complex_samples(rng, (1, g_ * p, n, n), True)
    zplan = hbx.Plan(dev_cfg(ocfg), max_jobs=g_)
    au, _ = zplan.simulate_real(torch.from_numpy(u).cuda())
    torch.cuda.synchronize()
    au = au.cpu().numpy().astype(np.complex128)
    zplan.close()
    mplan = hbx.Plan(dev_cfg(ocfg, planes=2 * p, z=-ocfg.z), max_jobs=g_)
    _, r = mplan.simulate_complex(torch.from_numpy(g).cuda(), want_field=False, want_real=True)
    torch.cuda.synchronize()
    r = r.cpu().numpy().astype(np.float64)
    mplan.close()
    g64, u64 = g.astype(np.complex128), u.astype(np.float64)
    lhs = float(np.sum(np.conj(g64) * au).real)
    rhs = float(np.sum(u64 * r))
    bound = FIELD_RTOL * (np.max(np.abs(au)) * np.sum(np.abs(g64)) + np.max(np.abs(r)) * np.sum(np.abs(u64)))
    print(f"N={n}: Re<g, A u> = {lhs:.9e}, <u, Re A^H g> = {rhs:.9e}, |diff| = {abs(lhs - rhs):.3e}, "
          f"bound {bound:.3e}")
    assert abs(lhs) > 0.0
    assert abs(lhs - rhs) <= bound


# -- 6. limits, argument checks --------------------------------------------------------------------
def test_reduced_precision_plan_is_unsupported():
    import hbx
    from hbx import _lib
    ocfg = O.OpticsConfig(64, 64, 1, 2, O.WL_MONO)
    plan = hbx.Plan(dev_cfg(ocfg), max_jobs=1, precision=_lib.PRECISION_BF16_STORE)
    vals = torch.zeros((1, 1, 64, 64), dtype=torch.complex64, device="cuda")
    with pytest.raises(_lib.HbxError) as e:
        plan.simulate_complex(vals)
    assert e.value.code == _lib.ERR_UNSUPPORTED and "F32" in str(e.value)
    plan.precision = _lib.PRECISION_F32
    plan.simulate_complex(vals)
    plan.close()


def test_values_argument_checks():
    import hbx
    ocfg = O.OpticsConfig(64, 64, 1, 4, O.WL_MONO)
    plan = hbx.Plan(dev_cfg(ocfg), max_jobs=1)
    good = torch.zeros((1, 2, 64, 64), dtype=torch.complex64, device="cuda")
    plan.simulate_complex(good)
    with pytest.raises(TypeError):
        plan.simulate_complex(good.real.contiguous())
    with pytest.raises(TypeError):
        plan.simulate_complex(good.to(torch.complex128))
    with pytest.raises(ValueError):
        plan.simulate_complex(good[:, :1])
    with pytest.raises(ValueError):     # the plan's CH real planes are CH / 2 complex planes
        plan.simulate_complex(torch.zeros((1, 4, 64, 64), dtype=torch.complex64, device="cuda"))
    with pytest.raises(ValueError):
        plan.simulate_complex(good.cpu())
    with pytest.raises(ValueError):
        plan.simulate_complex(good.transpose(2, 3))
    with pytest.raises(ValueError):
        plan.simulate_complex(good, want_field=False, want_real=False)
    plan.close()
