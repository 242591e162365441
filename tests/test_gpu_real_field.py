"""Propagation of real-valued fields (hbx_simulate_real / hbx_propagate_real, ABI v15).

The real path differs from the bit path in its first pass only (float32 samples instead of mask
bits, then the same row FFT, Hermitian split and stores), so
  * on 0 / 1 samples (and on +1 / -1 samples against a FIELD_PHASE plan) it gives the bit path's
    bits: torch.equal on field, intensity, chan_stats and psnr, at all four built sizes;
  * on continuous samples it meets the float64 oracle within the project's tolerances
    (tests/test_gpu_parity.py): field <= 2e-5 max|want|, intensity <= 2e-5 max(want),
    chan_stats rtol 2e-5, PSNR <= 1e-4 dB.  Samples are drawn as float32 and handed to the
    oracle as their float64 upcast, so no input rounding enters the comparison.
The real first pass runs one row block per workgroup at every launch size (no small / large
launch switch as on the bit path), so the first pass has no second regime to cover; k_col2 behind it
switches with the job count as on the bit path, and tests/test_gpu_launch_size.py puts real samples
through both of its forms."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import hbx_oracle as O  # noqa: E402

PSNR_TOL = 1e-4
STATS_RTOL = 2e-5
FIELD_RTOL = 2e-5
INTEN_RTOL = 2e-5

# the smallest shapes per built size: (N, G, P)
SHAPES = {64: (3, 2), 256: (1, 8), 896: (1, 2), 1024: (1, 2)}


def ocfg_for(n, **kw):
    g, p = SHAPES[n]
    return O.OpticsConfig(n, n, g, p, O.WL_RGB if g == 3 else O.WL_MONO, **kw)


def dev_cfg(o: O.OpticsConfig):
    import hbx
    return hbx.OpticsConfig(o.height, o.width, o.groups, o.planes, tuple(o.wavelengths), o.dx, o.dy, o.z,
                            o.tf_kind, o.field_kind, o.rel_scale, o.peak)


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm GPU")
    import hbx
    hbx.load_library()
    yield


def _target(n, b, g, seed):
    return np.random.default_rng(seed).random((b, g, n, n), dtype=np.float32)


# -- 1. the bit path's bits on 0 / 1 samples ------------------------------------------------------
def _equal_to_bit_path(ocfg, b, seed, phase=False):
    import hbx
    n, ch = ocfg.height, ocfg.channels
    gen = torch.Generator(device="cuda").manual_seed(seed)
    mask = torch.rand((b, ch, n, n), generator=gen, device="cuda") >= 0.5
    tgt = torch.from_numpy(_target(n, b, ocfg.groups, seed)).cuda()
    bits = hbx.pack_bits(mask)
    vals = mask.float()
    if phase:
        vals = 1.0 - 2.0 * vals
    plan = hbx.Plan(dev_cfg(ocfg), max_jobs=b * ocfg.groups)
    f_bit, i_bit = plan.simulate(bits, want_intensity=True)
    f_real, i_real = plan.simulate_real(vals.contiguous(), want_intensity=True)
    p_bit = plan.propagate(bits, tgt)
    p_real = plan.propagate_real(vals.contiguous(), tgt)
    torch.cuda.synchronize()
    df = float((torch.view_as_real(f_real) - torch.view_as_real(f_bit)).abs().max())
    di = float((i_real - i_bit).abs().max())
    print(f"N={n} phase={phase}: max |field diff| {df:.3e}, max |intensity diff| {di:.3e}")
    assert torch.equal(torch.view_as_real(f_real), torch.view_as_real(f_bit))
    assert torch.equal(i_real, i_bit)
    assert torch.equal(p_real[0], p_bit[0])
    assert torch.equal(p_real[1], p_bit[1])      # chan_stats
    assert torch.equal(p_real[2], p_bit[2])      # psnr
    plan.close()


@pytest.mark.parametrize("n", [64, 256, 896, 1024])
def test_binary_samples_equal_bit_path(n):
    _equal_to_bit_path(ocfg_for(n), 2, 11 + n)


def test_signed_samples_equal_phase_bit_path():
    _equal_to_bit_path(ocfg_for(64, field_kind=O.FIELD_PHASE), 2, 7, phase=True)


# -- 3. chunking -----------------------------------------------------------------------------------
def test_chunked_call_equals_single_env_calls():
    """max_jobs = 2, G = 1, B = 3: two chunks, the second starting at env 2 of `values`"""
    import hbx
    ocfg = O.OpticsConfig(64, 64, 1, 2, O.WL_MONO)
    rng = np.random.default_rng(3)
    vals = torch.from_numpy(rng.random((3, 2, 64, 64), dtype=np.float32)).cuda()
    tgt = torch.from_numpy(_target(64, 3, 1, 4)).cuda()
    plan = hbx.Plan(dev_cfg(ocfg), max_jobs=2)
    field, inten = plan.simulate_real(vals, want_intensity=True)
    pi, ps, pp = plan.propagate_real(vals, tgt)
    for e in range(3):
        f1, i1 = plan.simulate_real(vals[e:e + 1].contiguous(), want_intensity=True)
        a, s, p = plan.propagate_real(vals[e:e + 1].contiguous(), tgt[e:e + 1].contiguous())
        assert torch.equal(torch.view_as_real(field[e]), torch.view_as_real(f1[0])), e
        assert torch.equal(inten[e], i1[0]), e
        assert torch.equal(pi[e], a[0]) and torch.equal(ps[e], s[0]) and torch.equal(pp[e], p[0]), e
    assert not torch.equal(inten[2], inten[0])
    plan.close()


# -- 4. continuous samples against the float64 oracle ----------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_case(n, kind):
    """(values f32 [1, CH, N, N], target f32 [1, G, N, N], want field, intensity, stats, psnr)"""
    ocfg = ocfg_for(n)
    g, p = ocfg.groups, ocfg.planes
    rng = np.random.default_rng(100 + n + (0 if kind == "unit" else 1))
    vals = rng.random((1, g * p, n, n), dtype=np.float32)
    if kind == "signed":
        vals = (2.0 * vals - 1.0).astype(np.float32)
    tgt = _target(n, 1, g, 200 + n)
    v64 = vals.astype(np.float64)
    field = np.stack([O.propagate(v64[0, k * p:(k + 1) * p], ocfg.transfer(k)) for k in range(g)])   # [G, P, N, N]
    inten = np.mean(field.real ** 2 + field.imag ** 2, axis=1)
    stats = np.stack([O.chan_stats(inten[k], tgt[0, k]) for k in range(g)])
    psnr = O.psnr_from_stats(stats, g * n * n, ocfg.rel_scale, ocfg.peak)
    for a in (vals, tgt, field, inten, stats):
        a.setflags(write=False)
    return vals, tgt, field.reshape(g * p, n, n), inten, stats, psnr


@pytest.mark.parametrize("kind", ["unit", "signed"])
@pytest.mark.parametrize("n", [64, 256, 896, 1024])
def test_continuous_samples_vs_oracle(n, kind):
    import hbx
    ocfg = ocfg_for(n)
    vals, tgt, want_f, want_i, want_st, want_ps = _oracle_case(n, kind)
    plan = hbx.Plan(dev_cfg(ocfg), max_jobs=ocfg.groups)
    v = torch.from_numpy(vals.copy()).cuda()      # the cached case stays read-only
    field, inten = plan.simulate_real(v, want_intensity=True)
    torch.cuda.synchronize()
    ef = np.max(np.abs(field[0].cpu().numpy() - want_f)) / np.max(np.abs(want_f))
    ei = np.max(np.abs(inten[0].cpu().numpy() - want_i)) / np.max(want_i)
    print(f"N={n} {kind}: field err {ef:.3e} of max|want|, intensity err {ei:.3e} of max(want)")
    assert ef <= FIELD_RTOL
    assert ei <= INTEN_RTOL
    if n in (64, 256):
        i2, stats, psnr = plan.propagate_real(v, torch.from_numpy(tgt.copy()).cuda())
        torch.cuda.synchronize()
        st = stats[0].cpu().numpy()
        print(f"N={n} {kind}: stats rel err {np.max(np.abs(st / want_st - 1)):.3e}, "
              f"psnr err {abs(float(psnr[0]) - want_ps):.3e} dB")
        assert np.max(np.abs(i2[0].cpu().numpy() - want_i)) <= INTEN_RTOL * np.max(want_i)
        assert np.allclose(st, want_st, rtol=STATS_RTOL, atol=0.0)
        assert abs(float(psnr[0]) - want_ps) <= PSNR_TOL
    plan.close()


# -- 5. index map ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 896])
def test_single_sample_index_map(n):
    """One sample of 0.37 in an otherwise zero plane pair, at the four corners and (N/2, 31),
    in plane pa and again in plane pb (one env each): a wrong lane-to-pixel map or a swapped
    plane pair shows as the single-pixel response in the wrong place or plane."""
    import hbx
    ocfg = O.OpticsConfig(n, n, 1, 2, O.WL_MONO)
    pix = [(0, 0), (0, n - 1), (n - 1, 0), (n - 1, n - 1), (n // 2, 31)]
    cases = [(pl, y, x) for pl in (0, 1) for (y, x) in pix]
    vals = np.zeros((len(cases), 2, n, n), np.float32)
    for e, (pl, y, x) in enumerate(cases):
        vals[e, pl, y, x] = 0.37
    plan = hbx.Plan(dev_cfg(ocfg), max_jobs=len(cases))
    field, _ = plan.simulate_real(torch.from_numpy(vals).cuda())
    torch.cuda.synchronize()
    got = field.cpu().numpy()
    h = ocfg.transfer(0)
    for e, (pl, y, x) in enumerate(cases):
        want = O.propagate(vals[e].astype(np.float64), h)
        err = np.max(np.abs(got[e] - want))
        assert err <= FIELD_RTOL * np.max(np.abs(want)), (pl, y, x, err)
        assert np.max(np.abs(got[e, 1 - pl])) <= FIELD_RTOL * np.max(np.abs(want)), (pl, y, x)
    plan.close()


# -- 6. reduced precision, argument checks ---------------------------------------------------------
def test_reduced_precision_plan_is_unsupported():
    import hbx
    from hbx import _lib
    ocfg = O.OpticsConfig(64, 64, 1, 2, O.WL_MONO)
    plan = hbx.Plan(dev_cfg(ocfg), max_jobs=1, precision=_lib.PRECISION_BF16_STORE)
    vals = torch.zeros((1, 2, 64, 64), dtype=torch.float32, device="cuda")
    tgt = torch.zeros((1, 1, 64, 64), dtype=torch.float32, device="cuda")
    with pytest.raises(_lib.HbxError) as e:
        plan.simulate_real(vals)
    assert e.value.code == _lib.ERR_UNSUPPORTED and "F32" in str(e.value)
    with pytest.raises(_lib.HbxError) as e:
        plan.propagate_real(vals, tgt)
    assert e.value.code == _lib.ERR_UNSUPPORTED
    plan.precision = _lib.PRECISION_F32
    plan.simulate_real(vals)
    plan.close()


def test_values_argument_checks():
    import hbx
    ocfg = O.OpticsConfig(64, 64, 1, 2, O.WL_MONO)
    plan = hbx.Plan(dev_cfg(ocfg), max_jobs=1)
    good = torch.zeros((1, 2, 64, 64), dtype=torch.float32, device="cuda")
    with pytest.raises(TypeError):
        plan.simulate_real(good.double())
    with pytest.raises(ValueError):
        plan.simulate_real(good[:, :1])
    with pytest.raises(ValueError):
        plan.simulate_real(good.cpu())
    with pytest.raises(ValueError):
        plan.simulate_real(good.transpose(2, 3))
    with pytest.raises(ValueError):
        plan.propagate_real(good, torch.zeros((1, 2, 64, 64), dtype=torch.float32, device="cuda"))
    plan.close()
