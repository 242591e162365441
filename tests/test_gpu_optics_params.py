"""Parity away from the reference's optics: unequal pixel pitch, an active evanescent cut, odd
plane-pair counts, G = 2 and G = 4.

Every other GPU test builds its plan with dx = dy = 7.56 um, z = +-2 mm and the reference
wavelengths, where H(fy, fx) = H(fx, fy), |H| = 1 in every bin and h = IFFT2(H) is its own
transpose: an exchange of x and y anywhere between meta['dx'] and the column passes' transfer table,
a transposed single-pixel response in the incremental mode, or a path that assumes unit modulus
would pass all of them.  Two parameter sets break those properties:

  ANISO  dx = 7.56 um, dy = 5.04 um, z = 2 mm: |H| = 1, no cut, max |H - H^T| ~ 2;
  EVAN   dx = 0.40 um, dy = 0.30 um, z = 20 um: 17.2 % (638 nm), 1.0 % (515 nm), 0 % (450 nm) of
         the bins are evanescent and H = 0 there; mono configs use 638 nm.

Each test computes its expected value with the float64 oracle (oracle/hbx_oracle.py, which takes
dx, dy and the cut in general form) and holds the project's existing tolerances.  The inputs are
built by the `*_case` functions below from a config, so tests/test_optics_params_host.py can
rebuild every expected value with dx and dy exchanged, or with the cut taken out, and show that
it moves far beyond the tolerance: a pass here then means the device got x, y and the cut right.
Shapes (N, G, P) are the smallest per built size; P = 6 and P = 10 are odd pair counts (3 and 5
plane pairs per group), G = 2 and G = 4 = HBX_MAX_GROUPS have no other test."""
import dataclasses
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
MAP_TOL = 1e-8          # dB (tests/test_gpu_parity.py)
GRAD_RTOL = 5e-7        # of max|oracle gradient|, end to end (tests/test_gpu_shim_loss.py measures 2.5e-7 .. 3.1e-7)
ENERGY_RTOL = 2e-6      # tests/test_gpu_parity.py::test_parseval_full_size_batch

ANISO = dict(dx=7.56e-6, dy=5.04e-6, z=2e-3)
EVAN = dict(dx=0.40e-6, dy=0.30e-6, z=20e-6)
SETS = {"aniso": ANISO, "evan": EVAN}
WL4 = tuple(O.WL_RGB) + (405e-9,)
WL_EVAN_MONO = (638e-9,)        # the wavelength whose cut is active

# (set, transfer function): Fresnel has no cut, so it runs under ANISO only
TFSETS = [("aniso", O.TF_ASM), ("aniso", O.TF_FRESNEL), ("evan", O.TF_ASM)]
TFSET_IDS = ["aniso-asm", "aniso-fresnel", "evan-asm"]
SIZES = [64, 256, 896, 1024]


def wavelengths(pset, groups):
    if groups == 1:
        return WL_EVAN_MONO if pset == "evan" else tuple(O.WL_MONO)
    return WL4[:groups]


def ocfg(pset, n, g, p, **kw):
    return O.OpticsConfig(n, n, g, p, wavelengths(pset, g), **SETS[pset], **kw)


@dataclasses.dataclass
class _NoCutConfig(O.OpticsConfig):
    """the same optics with the evanescent bins at modulus one instead of zero"""

    def transfer(self, g):
        h = super().transfer(g)
        h[h == 0] = 1.0
        return h


def variant(cfg, kind):
    """kind "true": cfg; "swap": dx and dy exchanged; "nocut": |H| = 1 in the evanescent bins"""
    if kind == "true":
        return cfg
    if kind == "swap":
        return dataclasses.replace(cfg, dx=cfg.dy, dy=cfg.dx)
    if kind == "nocut":
        return _NoCutConfig(**{f.name: getattr(cfg, f.name) for f in dataclasses.fields(O.OpticsConfig)})
    raise ValueError(kind)


def dev_cfg(o: O.OpticsConfig, planes=None, z=None):
    import hbx
    return hbx.OpticsConfig(o.height, o.width, o.groups, planes or o.planes, tuple(o.wavelengths), o.dx, o.dy,
                            o.z if z is None else z, o.tf_kind, o.field_kind, o.rel_scale, o.peak)


def to_dev_bits(bits: np.ndarray):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int64)).cuda()


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _complex_samples(rng, shape):
    re = (2.0 * rng.random(shape, dtype=np.float32) - 1.0).astype(np.float32)
    im = (2.0 * rng.random(shape, dtype=np.float32) - 1.0).astype(np.float32)
    return (re + 1j * im).astype(np.complex64)


def shaped_target(noise, inten):
    """Half uniform noise, half the case's own oracle intensity scaled to [0, 1] per group.  Against a
    purely random target a changed intensity pattern averages out of the PSNR like 1 / N; with the
    pattern in the target the PSNR tells dx, dy exchanged (or the cut gone) apart at every size
    (tests/test_optics_params_host.py).  Variants of a case keep the true config's target."""
    return (0.5 * noise + 0.5 * inten / inten.max(axis=(-2, -1), keepdims=True)).astype(np.float32)


def field_of(cfg, u, per_group):
    """u [G * per_group, N, N] -> complex128 field of every plane"""
    u = np.asarray(u)
    u64 = u.astype(np.complex128 if np.iscomplexobj(u) else np.float64)
    return np.concatenate([O.propagate(u64[k * per_group:(k + 1) * per_group], cfg.transfer(k))
                           for k in range(cfg.groups)])


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm GPU")
    import hbx
    hbx.load_library()
    yield


# -- 1. complex field against the oracle ----------------------------------------------------------
COMPLEX_SHAPES = {64: (3, 2), 256: (1, 4), 896: (1, 2), 1024: (1, 2)}


@functools.lru_cache(maxsize=None)
def complex_case(pset, tf, n, kind="true"):
    """(values complex64 [1, G P / 2, N, N], want complex128 [G P / 2, N, N]), read-only"""
    g, p = COMPLEX_SHAPES[n]
    cfg = variant(ocfg(pset, n, g, p, tf_kind=tf), kind)
    vals = _complex_samples(np.random.default_rng(700 + n), (1, g * p // 2, n, n))
    return _freeze(vals, field_of(cfg, vals[0], p // 2))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pset,tf", TFSETS, ids=TFSET_IDS)
def test_complex_field_vs_oracle(pset, tf, n):
    import hbx
    g, p = COMPLEX_SHAPES[n]
    cfg = ocfg(pset, n, g, p, tf_kind=tf)
    vals, want = complex_case(pset, tf, n)
    plan = hbx.Plan(dev_cfg(cfg), max_jobs=g)
    field, real = plan.simulate_complex(torch.from_numpy(vals.copy()).cuda(), want_field=True, want_real=True)
    torch.cuda.synchronize()
    ef = np.max(np.abs(field[0].cpu().numpy() - want)) / np.max(np.abs(want))
    er = np.max(np.abs(real[0].cpu().numpy() - want.real)) / np.max(np.abs(want.real))
    print(f"complex {pset} tf={tf} N={n}: field err {ef:.3e} of max|want|, real_part err {er:.3e} of max|Re want|")
    assert ef <= FIELD_RTOL
    assert er <= FIELD_RTOL
    assert torch.equal(real, field.real)
    plan.close()


SINGLE_VALUE = 0.37 - 0.21j


def single_pixels(n):
    return [(n // 2, 31), (n - 1, 0)]


def single_response(cfg, y, x):
    """the oracle's h = IFFT2(H) shifted to (y, x), times the sample"""
    return SINGLE_VALUE * np.roll(O.single_pixel_field(cfg, 0), (y, x), axis=(0, 1))


@pytest.mark.parametrize("n", [64, 896])
@pytest.mark.parametrize("pset", ["aniso", "evan"])
def test_single_sample_response_is_h_shifted_not_transposed(pset, n):
    """One sample in an otherwise zero env of two complex planes, at (N/2, 31) and (N-1, 0) of either
    plane: the field is the oracle's h rolled to (row, column).  With dx != dy, h differs from its
    transpose by far more than the tolerance (tests/test_optics_params_host.py), so a response
    rolled to (column, row), or a transposed h, fails here."""
    import hbx
    cfg = ocfg(pset, n, 1, 4)
    cases = [(pl, y, x) for pl in (0, 1) for (y, x) in single_pixels(n)]
    vals = np.zeros((len(cases), 2, n, n), np.complex64)
    for e, (pl, y, x) in enumerate(cases):
        vals[e, pl, y, x] = SINGLE_VALUE
    plan = hbx.Plan(dev_cfg(cfg), max_jobs=len(cases))
    field, _ = plan.simulate_complex(torch.from_numpy(vals).cuda())
    torch.cuda.synchronize()
    got = field.cpu().numpy()
    for e, (pl, y, x) in enumerate(cases):
        want = single_response(cfg, y, x)
        scale = np.max(np.abs(want))
        err = np.max(np.abs(got[e, pl] - want)) / scale
        print(f"single {pset} N={n} plane {pl} ({y}, {x}): err {err:.3e} of max|h|")
        assert err <= FIELD_RTOL, (pl, y, x)
        assert np.max(np.abs(got[e, 1 - pl])) <= FIELD_RTOL * scale, (pl, y, x)
    plan.close()


# -- 2. real path ---------------------------------------------------------------------------------
REAL_SHAPES = {64: (3, 2), 256: (1, 6), 896: (1, 6), 1024: (1, 2)}


@functools.lru_cache(maxsize=None)
def real_case(pset, tf, n, kind="true"):
    """(values f32 [1, CH, N, N], target f32 [1, G, N, N], want field, intensity, stats, psnr)"""
    g, p = REAL_SHAPES[n]
    cfg = variant(ocfg(pset, n, g, p, tf_kind=tf), kind)
    rng = np.random.default_rng(710 + n)
    vals = (2.0 * rng.random((1, g * p, n, n), dtype=np.float32) - 1.0).astype(np.float32)
    noise = rng.random((1, g, n, n), dtype=np.float32)
    field = field_of(cfg, vals[0], p)
    inten = np.mean((field.real ** 2 + field.imag ** 2).reshape(g, p, n, n), axis=1)
    tgt = shaped_target(noise[0], inten)[None] if kind == "true" else real_case(pset, tf, n)[1]
    stats = np.stack([O.chan_stats(inten[k], tgt[0, k]) for k in range(g)])
    psnr = O.psnr_from_stats(stats, g * n * n, cfg.rel_scale, cfg.peak)
    return _freeze(vals, tgt, field, inten, stats) + (psnr,)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pset,tf", TFSETS, ids=TFSET_IDS)
def test_real_field_vs_oracle(pset, tf, n):
    import hbx
    g, p = REAL_SHAPES[n]
    cfg = ocfg(pset, n, g, p, tf_kind=tf)
    vals, tgt, want_f, want_i, want_st, want_ps = real_case(pset, tf, n)
    plan = hbx.Plan(dev_cfg(cfg), max_jobs=g)
    v = torch.from_numpy(vals.copy()).cuda()
    field, inten = plan.simulate_real(v, want_intensity=True)
    i2, stats, psnr = plan.propagate_real(v, torch.from_numpy(tgt.copy()).cuda())
    torch.cuda.synchronize()
    ef = np.max(np.abs(field[0].cpu().numpy() - want_f)) / np.max(np.abs(want_f))
    ei = np.max(np.abs(inten[0].cpu().numpy() - want_i)) / np.max(want_i)
    st = stats[0].cpu().numpy()
    es, ep = np.max(np.abs(st / want_st - 1)), abs(float(psnr[0]) - want_ps)
    print(f"real {pset} tf={tf} N={n} P={p}: field err {ef:.3e}, intensity err {ei:.3e} of max, "
          f"stats rel err {es:.3e}, psnr err {ep:.3e} dB")
    assert ef <= FIELD_RTOL
    assert ei <= INTEN_RTOL
    assert np.max(np.abs(i2[0].cpu().numpy() - want_i)) <= INTEN_RTOL * np.max(want_i)
    assert np.allclose(st, want_st, rtol=STATS_RTOL, atol=0.0)
    assert ep <= PSNR_TOL
    plan.close()


# -- 3. bit path ----------------------------------------------------------------------------------
# name: (N, G, P, field kind, rel scale, peak)
BIT_SHAPES = {
    "64x4x2": (64, 4, 2, O.FIELD_AMPLITUDE, O.REL_LSQ, 1.0),
    "64x4x2-phase-none": (64, 4, 2, O.FIELD_PHASE, O.REL_NONE, 1.0),
    "64x2x10-none-peak255": (64, 2, 10, O.FIELD_AMPLITUDE, O.REL_NONE, 255.0),
    "64x2x10-phase": (64, 2, 10, O.FIELD_PHASE, O.REL_LSQ, 1.0),
    "64x3x2": (64, 3, 2, O.FIELD_AMPLITUDE, O.REL_LSQ, 1.0),
    "256x1x6": (256, 1, 6, O.FIELD_AMPLITUDE, O.REL_LSQ, 1.0),
    "256x1x6-none": (256, 1, 6, O.FIELD_AMPLITUDE, O.REL_NONE, 1.0),
    "896x1x2": (896, 1, 2, O.FIELD_AMPLITUDE, O.REL_LSQ, 1.0),
    "1024x1x2": (1024, 1, 2, O.FIELD_AMPLITUDE, O.REL_NONE, 1.0),
}
# kept energy of the amplitude mask at 64 x (3 x 2) under EVAN (its DC half is always kept)
EVAN_KEPT_64 = (0.912, 0.995, 1.0)


def bit_cfg(pset, tf, name):
    n, g, p, fk, rs, peak = BIT_SHAPES[name]
    return ocfg(pset, n, g, p, tf_kind=tf, field_kind=fk, rel_scale=rs, peak=peak)


@functools.lru_cache(maxsize=None)
def bit_case(pset, tf, name, kind="true"):
    """(mask u8 [CH, N, N], target f32 [G, N, N], want intensity, stats, psnr, energy in per group)"""
    cfg = variant(bit_cfg(pset, tf, name), kind)
    n, g, p = cfg.height, cfg.groups, cfg.planes
    pre, noise = O.synthetic_inputs(cfg, 720 + n + 7 * g + p)
    mask = (pre >= 0.5).astype(np.uint8)
    prop = O.Propagator(cfg)
    inten = prop.all_intensity(mask)
    tgt = shaped_target(noise, inten) if kind == "true" else bit_case(pset, tf, name)[1]
    stats = np.stack([O.chan_stats(inten[k], tgt[k]) for k in range(g)])
    u = O.mask_to_field(mask, cfg.field_kind).reshape(g, -1)
    energy = np.sum(u * u, axis=1) / p                    # sum_xy I_g where |H| = 1 (Parseval)
    return _freeze(mask, tgt, inten, stats) + (prop.psnr(stats), energy)


@pytest.mark.parametrize("name", list(BIT_SHAPES))
@pytest.mark.parametrize("pset,tf", TFSETS, ids=TFSET_IDS)
def test_bit_path_vs_oracle(pset, tf, name):
    import hbx
    cfg = bit_cfg(pset, tf, name)
    g = cfg.groups
    mask, tgt, want_i, want_st, want_ps, energy = bit_case(pset, tf, name)
    plan = hbx.Plan(dev_cfg(cfg), max_jobs=g)
    inten, stats, psnr = plan.propagate(to_dev_bits(O.pack_mask(mask))[None], torch.from_numpy(tgt.copy()).cuda()[None])
    torch.cuda.synchronize()
    got_i, st = inten[0].cpu().numpy(), stats[0].cpu().numpy()
    ei = np.max(np.abs(got_i - want_i)) / np.max(want_i)
    es, ep = np.max(np.abs(st / want_st - 1)), abs(float(psnr[0]) - want_ps)
    kept = got_i.astype(np.float64).reshape(g, -1).sum(axis=1) / energy
    want_kept = want_i.reshape(g, -1).sum(axis=1) / energy
    print(f"bit {pset} tf={tf} {name}: intensity err {ei:.3e} of max, stats rel err {es:.3e}, psnr err {ep:.3e} dB, "
          f"kept energy {np.array2string(kept, precision=7)} (oracle {np.array2string(want_kept, precision=7)})")
    assert ei <= INTEN_RTOL
    assert np.allclose(st, want_st, rtol=STATS_RTOL, atol=0.0)
    assert ep <= PSNR_TOL
    if pset == "aniso":                                   # |H| = 1: sum_xy I_g = sum |u|^2 / P
        assert np.allclose(kept, 1.0, rtol=ENERGY_RTOL, atol=0.0)
    else:                                                 # the cut removes what the oracle's removes
        assert np.allclose(kept, want_kept, rtol=ENERGY_RTOL, atol=0.0)
    plan.close()


# -- 4. trial flips, FFT mode ---------------------------------------------------------------------
FLIP_SHAPES = {64: (3, 2), 256: (1, 6)}


@functools.lru_cache(maxsize=None)
def flips_case(pset, n, kind="true"):
    """(pre_model, target, 16 flips, base psnr, psnr after each flip): pixel 0, the last pixel, one in
    the second plane of every group, the rest drawn"""
    g, p = FLIP_SHAPES[n]
    cfg = variant(ocfg(pset, n, g, p), kind)
    pre, tgt = O.synthetic_inputs(cfg, 730 + n)
    env = O.OracleEnv(cfg)
    base = env.reset(pre, tgt)
    npx, ch = n * n, g * p
    fixed = [0, ch * npx - 1] + [(k * p + 1) * npx + (7 + k) * n + 13 for k in range(g)]
    drawn = np.random.default_rng(731 + n).integers(0, ch * npx, 16 - len(fixed))
    flips = np.concatenate([fixed, drawn]).astype(np.int64)
    want = np.array([env.evaluate_flip(int(a))[0] for a in flips])
    return _freeze(pre, tgt, flips, want) + (base,)


@pytest.mark.parametrize("n", list(FLIP_SHAPES))
@pytest.mark.parametrize("pset", ["aniso", "evan"])
def test_eval_flips_vs_oracle(pset, n):
    import hbx
    g, p = FLIP_SHAPES[n]
    cfg = ocfg(pset, n, g, p)
    pre, tgt, flips, want, base = flips_case(pset, n)
    plan = hbx.Plan(dev_cfg(cfg), max_jobs=16)
    bits = to_dev_bits(O.pack_mask((pre >= 0.5).astype(np.uint8)))
    t = torch.from_numpy(tgt.copy()).cuda()
    _, st, ps0 = plan.propagate(bits[None], t[None])
    got, _ = plan.eval_flips(bits, t, st[0].contiguous(), torch.from_numpy(flips.copy()).cuda())
    torch.cuda.synchronize()
    err = np.max(np.abs(got.cpu().numpy() - want))
    print(f"flips {pset} N={n} P={p}: base psnr err {abs(float(ps0[0]) - base):.3e} dB, worst flip psnr err {err:.3e} dB, "
          f"largest |change| {np.max(np.abs(want - base)):.3e} dB")
    assert abs(float(ps0[0]) - base) <= PSNR_TOL
    assert err <= PSNR_TOL
    plan.close()


# -- 5. incremental (PSF) mode --------------------------------------------------------------------
PSF_SHAPES = {64: (3, 2, 8), 256: (1, 6, 2)}      # N: (G, P, envs)
PSF_STEPS, PSF_REFRESH = 12, 8


def psf_inputs(cfg, n_env):
    return [O.synthetic_inputs(cfg, 740 + cfg.height + 2 * b) for b in range(n_env)]


@pytest.mark.parametrize("n", list(PSF_SHAPES))
@pytest.mark.parametrize("pset", ["aniso", "evan"])
def test_psf_mode_vs_fft_mode_and_oracle(pset, n):
    """The incremental mode reads the folded quadrant of h = IFFT2(H) at (row offset, column offset).
    Next to an FFT-mode env and one float64 oracle env per env: the field after reset, then every
    step's PSNR of both modes against the oracle on the same state (the two modes share the
    transfer table, so an error in it cancels between them), the decisions wherever the change is
    clear of f32 resolution, and the final masks."""
    from hbx.env import HologramVecEnv
    g, p, B = PSF_SHAPES[n]
    cfg = ocfg(pset, n, g, p)
    ins = psf_inputs(cfg, B)
    kw = dict(pre_model_source=lambda i: ins[i][0], obs_keys=(), auto_reset=False)
    fft = HologramVecEnv(dev_cfg(cfg), B, lambda i: ins[i][1], **kw)
    psf = HologramVecEnv(dev_cfg(cfg), B, lambda i: ins[i][1], mode="psf", refresh_every=PSF_REFRESH, **kw)
    fft.reset()
    psf.reset()
    oenvs = [O.OracleEnv(cfg) for _ in range(B)]
    for b in range(B):
        oenvs[b].reset(*ins[b])
    e0 = max(abs(float(psf.state.init_psnr[b]) - oenvs[b].initial_psnr) for b in range(B))
    mask0 = (ins[0][0] >= 0.5).astype(np.uint8)
    want_f = field_of(cfg, O.mask_to_field(mask0), p)
    got_f = psf.state.field[0].cpu().numpy()
    got_f = got_f[..., 0] + 1j * got_f[..., 1]
    ef = np.max(np.abs(got_f - want_f)) / np.max(np.abs(want_f))
    print(f"psf {pset} N={n} P={p}: init psnr err {e0:.3e} dB, field after reset err {ef:.3e} of max|want|")
    assert e0 <= PSNR_TOL
    assert ef <= FIELD_RTOL
    rng = np.random.default_rng(741 + n)
    worst_fft = worst_psf = 0.0
    clear = 0
    for k in range(PSF_STEPS):
        acts = rng.integers(0, cfg.channels * n * n, B)
        a_dev = torch.from_numpy(acts).cuda()
        _, p1, a1, _, _ = fft.step_device(a_dev)
        _, p2, a2, _, _ = psf.step_device(a_dev)
        p1, p2, a1, a2 = p1.cpu().numpy(), p2.cpu().numpy(), a1.cpu().numpy(), a2.cpu().numpy()
        for b in range(B):
            oe = oenvs[b]
            want, gg, ig, st = oe.evaluate_flip(int(acts[b]))
            change = want - oe.previous_psnr
            worst_fft, worst_psf = max(worst_fft, abs(p1[b] - want)), max(worst_psf, abs(p2[b] - want))
            assert abs(p1[b] - want) <= PSNR_TOL, (k, b)
            assert abs(p2[b] - want) <= PSNR_TOL, (k, b)
            if abs(change) > 1e-5:
                clear += 1
                assert bool(a1[b]) == bool(a2[b]) == (change >= 0), (k, b)
            if bool(a2[b]):                                # follow the device's decision
                ch, row, col = (int(v) for v in O.decode_action(int(acts[b]), n, n))
                oe.state[ch, row, col] ^= 1
                oe.stats, oe.intensity[gg], oe.previous_psnr = st, ig, want
    print(f"psf {pset} N={n} P={p}: worst step psnr err fft mode {worst_fft:.3e} dB, psf mode {worst_psf:.3e} dB, "
          f"{clear} of {PSF_STEPS * B} decisions clear")
    assert clear > 0
    assert torch.equal(fft.state.mask, psf.state.mask)
    for b in range(B):
        want_bits = torch.from_numpy(O.pack_mask(oenvs[b].state.astype(np.uint8)).view(np.int64))
        assert torch.equal(psf.state.mask[b].cpu(), want_bits), b
    fft.close()
    psf.close()


GREEDY_CANDIDATES = 200


@functools.lru_cache(maxsize=None)
def greedy_case(kind="true"):
    """64 x (3 x 2) under EVAN: (pre_model, target, order, accepted flags, psnr per candidate, initial
    psnr, final psnr, final mask u8) of the serial float64 greedy"""
    cfg = variant(ocfg("evan", 64, 3, 2), kind)
    pre, tgt = O.synthetic_inputs(cfg, 750)
    order = np.random.default_rng(751).integers(0, cfg.channels * 64 * 64, GREEDY_CANDIDATES)
    env = O.OracleEnv(cfg)
    env.reset(pre, tgt)
    acc, psnrs, final = O.dbs_greedy(env, order)
    return _freeze(pre, tgt, order, acc, psnrs) + (env.initial_psnr, final, env.state.astype(np.uint8))


def test_psf_greedy_walk_vs_oracle_evan():
    """The device walk's kernels (hbx_walk.hip) read hpsf at the folded offsets too: 200 candidates of
    the incremental greedy under EVAN accept what the serial float64 greedy accepts wherever its
    change is resolved (|change| > 1e-7 dB, as tests/test_gpu_parity.py)."""
    import hbx
    from hbx import dbs
    cfg = ocfg("evan", 64, 3, 2)
    pre, tgt, order, want, psnrs, initial, final, final_mask = greedy_case()
    prev = np.maximum.accumulate(np.concatenate([[initial], psnrs]))[:-1]
    clear = np.abs(psnrs - prev) > 1e-7
    plan = hbx.Plan(dev_cfg(cfg), max_jobs=16)
    mask = hbx.pack_bits(torch.from_numpy(pre.copy()).cuda() >= 0.5)
    res = dbs.greedy(plan, mask, torch.from_numpy(tgt.copy()).cuda(), order.copy(), mode="psf", refresh_every=64)
    plan.close()
    got = np.zeros(len(order), bool)
    got[res.accepted_positions] = True
    print(f"greedy evan 64x(3x2): {int(want.sum())} of {len(order)} accepted by the oracle, {int(got.sum())} by the walk, "
          f"{int((~clear).sum())} unresolved, final psnr err {abs(res.final_psnr - final):.3e} dB")
    assert res.steps == len(order)
    assert 0 < want.sum() < len(order)
    assert np.array_equal(got[clear], want[clear])
    if clear.all():
        assert abs(res.final_psnr - final) <= PSNR_TOL
        assert np.array_equal(mask.cpu().numpy().view("<u8"), O.pack_mask(final_mask))


# -- 6. flip map ----------------------------------------------------------------------------------
MAP_SHAPES = {64: (3, 2), 256: (1, 8)}


@functools.lru_cache(maxsize=None)
def map_case(pset, n, kind="true", base_only=False):
    """(pre_model, target, flips, psnr change of each, base psnr): every flip at N = 64 (by linearity,
    O.LinearGreedy, exact in float64), 48 drawn flips at N = 256 (re-propagated); base_only: no flips"""
    g, p = MAP_SHAPES[n]
    cfg = variant(ocfg(pset, n, g, p), kind)
    pre, tgt = O.synthetic_inputs(cfg, 764 + n)
    if base_only:
        env = O.OracleEnv(cfg)
        return pre, tgt, None, None, env.reset(pre, tgt)
    if n == 64:
        lg = O.LinearGreedy(cfg, pre, tgt)
        base = lg.initial_psnr
        flips = np.arange(cfg.channels * n * n, dtype=np.int64)
        want = np.array([lg.evaluate(int(a))[0] - base for a in flips])
    else:
        env = O.OracleEnv(cfg)
        base = env.reset(pre, tgt)
        flips = np.random.default_rng(761).integers(0, cfg.channels * n * n, 48).astype(np.int64)
        want = np.array([env.evaluate_flip(int(a))[0] - base for a in flips])
    return _freeze(pre, tgt, flips, want) + (base,)


@pytest.mark.parametrize("n", list(MAP_SHAPES))
@pytest.mark.parametrize("pset", ["aniso", "evan"])
def test_flip_map_vs_oracle(pset, n):
    import hbx
    g, p = MAP_SHAPES[n]
    cfg = ocfg(pset, n, g, p)
    pre, tgt, flips, want, base = map_case(pset, n)
    plan = hbx.Plan(dev_cfg(cfg), max_jobs=8)
    bits = to_dev_bits(O.pack_mask((pre >= 0.5).astype(np.uint8)))
    dmap, b = plan.flip_map(bits, torch.from_numpy(tgt.copy()).cuda())
    torch.cuda.synchronize()
    flat = dmap.reshape(-1).cpu().numpy().astype(np.float64)
    err = np.max(np.abs(flat[flips] - want))
    print(f"map {pset} N={n}: base psnr err {abs(float(b.item()) - base):.3e} dB, worst of {len(flips)} flips "
          f"{err:.3e} dB, largest |change| {np.max(np.abs(want)):.3e} dB")
    assert np.all(np.isfinite(flat))
    assert abs(float(b.item()) - base) <= PSNR_TOL
    assert err <= MAP_TOL
    plan.close()


# -- 7. adjoint under the cut ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 256])
def test_minus_z_plan_is_the_adjoint_under_the_cut(n):
    """<v, A u> = <A^H v, u> for complex u, v with A on the z plan and A^H on the -z plan, where H = 0 in
    17 % of the bins: H(-z) = conj H(z) must hold there too (zero both ways).  Each side's elements
    carry at most FIELD_RTOL of its maximum, so the sums differ by at most
    FIELD_RTOL (max|A u| sum|v| + max|A^H v| sum|u|) (tests/test_gpu_complex_field.py)."""
    import hbx
    g, p = COMPLEX_SHAPES[n]
    cfg = ocfg("evan", n, g, p)
    rng = np.random.default_rng(770 + n)
    u = _complex_samples(rng, (1, g * p // 2, n, n))
    v = _complex_samples(rng, (1, g * p // 2, n, n))
    zplan = hbx.Plan(dev_cfg(cfg), max_jobs=g)
    au, _ = zplan.simulate_complex(torch.from_numpy(u).cuda())
    torch.cuda.synchronize()
    au = au.cpu().numpy().astype(np.complex128)
    zplan.close()
    mplan = hbx.Plan(dev_cfg(cfg, z=-cfg.z), max_jobs=g)
    ahv, _ = mplan.simulate_complex(torch.from_numpy(v).cuda())
    torch.cuda.synchronize()
    ahv = ahv.cpu().numpy().astype(np.complex128)
    mplan.close()
    u64, v64 = u.astype(np.complex128), v.astype(np.complex128)
    lhs, rhs = np.sum(np.conj(v64) * au), np.sum(np.conj(ahv) * u64)
    bound = FIELD_RTOL * (np.max(np.abs(au)) * np.sum(np.abs(v64)) + np.max(np.abs(ahv)) * np.sum(np.abs(u64)))
    lost = 1.0 - np.sum(np.abs(au) ** 2) / np.sum(np.abs(u64) ** 2)
    print(f"adjoint evan N={n}: <v, A u> = {lhs:.9e}, <A^H v, u> = {rhs:.9e}, |diff| = {abs(lhs - rhs):.3e}, "
          f"bound {bound:.3e}, energy cut from u {lost:.4f}")
    assert lost > 0.05                                   # the cut is active in this case
    assert abs(lhs) > 0.0
    assert abs(lhs - rhs) <= bound


# -- 8. shim ----------------------------------------------------------------------------------------
SHIM_N = 64
SHIM_SHAPE = (2, 6, SHIM_N, SHIM_N)     # 3 colour groups x 2 planes for tt.intensity / tt.loss
UP = np.array([1.0, -0.5])              # per-env upstream gradients that differ


def shim_meta(pset, wl):
    """meta['dx'] = (dx, dy): the first element is the pitch along the width axis (it feeds fx)"""
    s = SETS[pset]
    return {"dx": (s["dx"], s["dy"]), "wl": wl}


def shim_transfer(pset, wl, kind="true"):
    cfg = variant(O.OpticsConfig(SHIM_N, SHIM_N, 1, 2, (wl,), **SETS[pset]), kind)
    return cfg.transfer(0)


@functools.lru_cache(maxsize=None)
def shim_inputs():
    """(x f32 [2, 6, N, N] in (-1, 1), binary mask f32 of the same shape, target f32 [2, 3, N, N])"""
    rng = np.random.default_rng(780)
    x = (2.0 * rng.random(SHIM_SHAPE, dtype=np.float32) - 1.0).astype(np.float32)
    m = (rng.random(SHIM_SHAPE, dtype=np.float32) >= 0.5).astype(np.float32)
    t = rng.random((SHIM_SHAPE[0], 3, SHIM_N, SHIM_N), dtype=np.float32)
    return _freeze(x, m, t)


def shim_intensity(pset, u, kind="true"):
    """float64 plane-mean intensity [B, 3, N, N] of field samples u [B, 6, N, N] (real or complex)"""
    b, c, n, _ = u.shape
    hs = [shim_transfer(pset, wl, kind) for wl in O.WL_RGB]
    u64 = np.asarray(u).astype(np.complex128).reshape(b, 3, c // 3, n, n)
    f = np.stack([np.stack([O.propagate(u64[e, k], hs[k]) for k in range(3)]) for e in range(b)])
    return np.mean(f.real ** 2 + f.imag ** 2, axis=2)


@pytest.mark.parametrize("pset", ["aniso", "evan"])
def test_shim_simulate_forward(pset):
    """tt.simulate with meta['dx'] = (dx, dy), one wavelength: the binary path and the continuous
    path against the oracle built with the same (dx, dy) order"""
    import torchOptics.optics as tt
    x, m, _ = shim_inputs()
    wl = wavelengths(pset, 1)[0]
    z = SETS[pset]["z"]
    h = shim_transfer(pset, wl)
    for name, src, binary in (("binary", m, True), ("continuous", x, False)):
        got = tt.simulate(tt.Tensor(torch.from_numpy(src.copy()).cuda(), meta=shim_meta(pset, wl)), z, binary=binary)
        torch.cuda.synchronize()
        want = O.propagate(src.astype(np.float64), h)
        err = np.max(np.abs(got.cpu().numpy() - want)) / np.max(np.abs(want))
        print(f"shim simulate {pset} {name}: field err {err:.3e} of max|want|")
        assert got.dtype == torch.complex64 and tuple(got.shape) == SHIM_SHAPE
        assert err <= FIELD_RTOL
    tt.check_binary()


@pytest.mark.parametrize("pset", ["aniso", "evan"])
def test_shim_intensity_and_loss_forward(pset):
    import torchOptics.optics as tt
    x, _, t = shim_inputs()
    z = SETS[pset]["z"]
    meta = shim_meta(pset, tuple(O.WL_RGB))
    xd, td = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(t.copy()).cuda()
    want_i = shim_intensity(pset, x)
    got_i = tt.intensity(tt.Tensor(xd, meta=meta), z)
    torch.cuda.synchronize()
    ei = np.max(np.abs(got_i.cpu().numpy() - want_i)) / np.max(want_i)
    print(f"shim intensity {pset}: err {ei:.3e} of max(want)")
    assert ei <= INTEN_RTOL
    t64 = t.astype(np.float64)
    for rel_name, rel in (("lsq", O.REL_LSQ), ("none", O.REL_NONE)):
        mse = tt.loss(tt.Tensor(xd, meta=meta), td, z, metric="mse", rel_scale=rel_name).cpu().numpy()
        psnr = tt.loss(tt.Tensor(xd, meta=meta), td, z, metric="psnr", rel_scale=rel_name).cpu().numpy()
        for e in range(SHIM_SHAPE[0]):
            want_m = O.relative_mse(want_i[e], t64[e], rel)
            want_p = O.relative_psnr(want_i[e], t64[e], rel)
            print(f"shim loss {pset} {rel_name} env {e}: mse rel err {abs(mse[e] - want_m) / want_m:.3e}, "
                  f"psnr err {abs(psnr[e] - want_p):.3e} dB")
            assert abs(mse[e] - want_m) <= 2.31e-5 * want_m      # PSNR_TOL as a relative MSE (tests/test_gpu_shim_loss.py)
            assert abs(psnr[e] - want_p) <= PSNR_TOL


def shim_oracle_gradient(pset, leaf, metric, kind="true"):
    """d sum_b UP[b] loss_b / dx in float64 by torch autograd on the CPU, through a restatement of the
    oracle's operations (O.propagate, the plane mean, O.relative_mse / O.relative_psnr with the
    least-squares scale); leaf "real": u = x, "phase": u = exp(i pi x)"""
    x, _, t = shim_inputs()
    b, c, n, _ = x.shape
    hs = torch.from_numpy(np.stack([shim_transfer(pset, wl, kind) for wl in O.WL_RGB]))      # [3, N, N] complex128
    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_()
    u = torch.exp(1j * np.pi * xt) if leaf == "phase" else xt.to(torch.complex128)
    f = torch.fft.ifft2(torch.fft.fft2(u.reshape(b, 3, c // 3, n, n)) * hs[None, :, None])
    inten = (f.real ** 2 + f.imag ** 2).mean(dim=2)
    tt64 = torch.from_numpy(t.astype(np.float64))
    s = (inten * tt64).sum(dim=(1, 2, 3)) / (inten * inten).sum(dim=(1, 2, 3))
    mse = ((s[:, None, None, None] * inten - tt64) ** 2).mean(dim=(1, 2, 3))
    loss = mse if metric == "mse" else 10.0 * torch.log10(1.0 / mse)
    (loss * torch.from_numpy(UP)).sum().backward()
    return loss.detach().numpy(), xt.grad.numpy()


@pytest.mark.parametrize("metric", ["mse", "psnr"])
@pytest.mark.parametrize("leaf", ["real", "phase"])
@pytest.mark.parametrize("pset", ["aniso", "evan"])
def test_shim_loss_backward(pset, leaf, metric):
    """tt.loss(..).backward() to a real leaf and to a phase leaf, three wavelengths, against float64
    autograd of the oracle restatement: the backward pass runs on the plan for -z built from the
    same meta['dx'], so an exchange there alone would show here"""
    import torchOptics.optics as tt
    x, _, t = shim_inputs()
    z = SETS[pset]["z"]
    want_l, want_g = shim_oracle_gradient(pset, leaf, metric)
    xd = torch.from_numpy(x.copy()).cuda().requires_grad_()
    kw = {"field": "phase"} if leaf == "phase" else {}
    loss = tt.loss(tt.Tensor(xd, meta=shim_meta(pset, tuple(O.WL_RGB))), torch.from_numpy(t.copy()).cuda(), z,
                   metric=metric, **kw)
    (loss * torch.from_numpy(UP).cuda()).sum().backward()
    torch.cuda.synchronize()
    got = xd.grad.cpu().numpy()
    scale = np.max(np.abs(want_g))
    err = np.max(np.abs(got - want_g)) / scale
    el = np.max(np.abs(loss.detach().cpu().numpy() - want_l) / (np.abs(want_l) if metric == "mse" else 1.0))
    print(f"shim backward {pset} {leaf} {metric}: loss err {el:.3e}, grad err {err:.3e} of max|oracle grad| = {scale:.3e}")
    assert scale > 0.0
    assert el <= (2.31e-5 if metric == "mse" else PSNR_TOL)
    assert err <= GRAD_RTOL


# -- 9. plane cache, odd pair count ---------------------------------------------------------------
def test_planes_mode_bit_exact_p6_aniso():
    """256 mono, P = 6 (three plane pairs: an odd count in the slot bookkeeping) under ANISO, 60 steps:
    the plane-cached mode gives the FFT mode's bits (tests/test_gpu_planes.py)"""
    from hbx.env import HologramVecEnv, OBS_KEYS
    cfg = dev_cfg(ocfg("aniso", 256, 1, 6))
    B, steps = 4, 60
    g = torch.Generator(device="cuda").manual_seed(790)
    pres = [torch.rand((cfg.channels, 256, 256), generator=g, device="cuda") for _ in range(B)]
    tgts = [torch.rand((cfg.groups, 256, 256), generator=g, device="cuda") for _ in range(B)]
    kw = dict(pre_model_source=lambda i: pres[i], auto_reset=True, max_steps=25, obs_keys=OBS_KEYS)
    fft = HologramVecEnv(cfg, B, lambda i: tgts[i], mode="fft", **kw)
    planes = HologramVecEnv(cfg, B, lambda i: tgts[i], mode="planes", **kw)
    o1, o2 = fft.reset(), planes.reset()
    assert torch.equal(o1["recon_image"], o2["recon_image"])
    acts = torch.randint(0, cfg.channels * 256 * 256, (steps, B), generator=g, device="cuda")
    n_acc = n_rej = n_done = 0
    for k in range(steps):
        o1, r1, d1, _ = fft.step(acts[k])
        o2, r2, d2, _ = planes.step(acts[k])
        assert np.array_equal(r1, r2), k
        assert np.array_equal(d1, d2), k
        l1, l2 = fft.last_step(), planes.last_step()
        assert np.array_equal(l1["psnr"], l2["psnr"]), k
        assert np.array_equal(l1["accepted"], l2["accepted"]), k
        assert torch.equal(o1["recon_image"], o2["recon_image"]), k
        assert torch.equal(o1["state"], o2["state"]), k
        n_acc += int(l1["accepted"].sum())
        n_rej += int((~l1["accepted"]).sum())
        n_done += int(np.sum(d1))
    for key in ("mask", "record", "chan_stats", "prev_psnr", "init_psnr", "steps", "flip_count", "sustained"):
        assert torch.equal(getattr(fft.state, key), getattr(planes.state, key)), key
    print(f"planes aniso 256 P=6: {n_acc} accepted, {n_rej} rejected, {n_done} resets, all bits equal")
    assert n_acc > 0 and n_rej > 0 and n_done > 0
    fft.close()
    planes.close()
