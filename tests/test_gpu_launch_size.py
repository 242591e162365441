"""The walking forms of the first pass and of k_col2 (N = 1024 / 256), pixel for pixel.

hbx::pass_launch_small (csrc/hbx_internal.hpp) runs a launch of fewer than 2048 workgroups on the
one-block-per-workgroup forms k_rowfwd32<SK, 1> / k_rowfwd<R, NT, SK, 1> / k_col2<R, SK, 1> and every
larger launch -- the benchmark, the 128-env step, every large sample batch -- on the walking forms.  The
other GPU files compare pixels with the float64 oracle on a handful of jobs, i.e. on the small forms.
Here every case takes its job count from tests/_launch_size.py (held to the C++ function by
tests/test_launch_size_host.py) and asserts through `walking(...)` which form each of its launches runs:

  a. the walking forms against the float64 oracle directly: intensity, chan_stats, PSNR and the complex
     field of every plane, with the tolerances the small-launch files assert for the same quantities;
  b. small launch EQUAL large launch (the contract in launch_passes' comment, and what the plane cache's
     equality guarantee rests on): the same inputs once on a plan whose max_jobs keeps every launch below
     the line and once on one that takes them in a single launch at or just above it, torch.equal on
     every output array -- the bit path, the reduced-precision stores, candidate flips with and without
     the plane cache, and the sample paths, where only k_col2 switches;
  c. the env step across the line, small and large max_jobs and mode="planes" against mode="fft".

Job counts are the smallest that cross the line plus one odd count above it.  The largest case holds
about 1 GiB of field and 1.5 GiB of workspace; every plan is closed when its case ends."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import hbx_oracle as O  # noqa: E402
from tests import _launch_size as L  # noqa: E402
# the tolerances of the small-launch tests, for the same quantities
from tests.test_gpu_complex_field import FIELD_RTOL as COMPLEX_FIELD_RTOL  # noqa: E402
from tests.test_gpu_parity import PSNR_TOL, STATS_RTOL, dev_cfg  # noqa: E402
from tests.test_gpu_real_field import FIELD_RTOL, INTEN_RTOL  # noqa: E402

# name: (N, groups, planes per group, envs, small max_jobs, large max_jobs)
SHAPES = {
    "1024x8-16": (1024, 1, 8, 16, 15, 16),
    "1024x8-17": (1024, 1, 8, 17, 15, 17),
    "1024x24-6": (1024, 3, 8, 6, 15, 18),      # 18 jobs of three colour groups in one launch
    "256x8-64": (256, 1, 8, 64, 63, 64),
    "256x8-65": (256, 1, 8, 65, 63, 65),
    "256x2-256": (256, 1, 2, 256, 255, 256),
}
MONO = ["1024x8-16", "1024x8-17", "256x8-64", "256x8-65"]
AT_LINE = ["256x8-64", "1024x8-16"]


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm GPU")
    import hbx
    hbx.load_library()
    yield


def _ocfg(name, **kw):
    n, g, p = SHAPES[name][:3]
    return O.OpticsConfig(n, n, g, p, O.WL_RGB if g == 3 else O.WL_MONO, **kw)


def _full_launches(envs, groups, max_jobs):
    """job counts of a full propagation's launches: max_jobs / G envs per launch, G jobs per env"""
    return [c * groups for c in L.launches(envs, max_jobs // groups)]


def _assert_sides(n, planes, small, large, pair=False):
    """every launch of the small side below the line, the large side one launch at or above it"""
    assert small and all(not L.walking(n, planes, j, pair) for j in small), (n, planes, small, pair)
    assert len(large) == 1 and L.walking(n, planes, large[0], pair), (n, planes, large, pair)
    assert sum(small) == large[0]


def _two_plans(name, precision=None, **kw):
    """(small plan, large plan) of a shape, the sides of a full propagation asserted"""
    import hbx
    n, g, p, envs, ms, ml = SHAPES[name]
    _assert_sides(n, p, _full_launches(envs, g, ms), _full_launches(envs, g, ml))
    cfg = dev_cfg(_ocfg(name, **kw))
    extra = {} if precision is None else {"precision": precision}
    return hbx.Plan(cfg, max_jobs=ms, **extra), hbx.Plan(cfg, max_jobs=ml, **extra)


def _inputs(name, seed):
    """seeded random pre-model values [B, CH, N, N], their packed bits and targets [B, G, N, N]"""
    import hbx
    n, g, p, envs = SHAPES[name][:4]
    gen = torch.Generator(device="cuda").manual_seed(seed)
    pre = torch.rand((envs, g * p, n, n), generator=gen, device="cuda")
    tgt = torch.rand((envs, g, n, n), generator=gen, device="cuda")
    return pre, hbx.pack_bits(pre >= 0.5), tgt


def _first_difference(a, b):
    i = torch.nonzero((a != b).reshape(-1))[0].item()
    idx = np.unravel_index(i, tuple(a.shape))
    return f"{int((a != b).sum())} of {a.numel()} differ, first at {tuple(int(v) for v in idx)}: " \
           f"{a.reshape(-1)[i].item()!r} != {b.reshape(-1)[i].item()!r}"


def _same(small, large, what):
    """torch.equal; the message names the first differing index (env, plane, row, column, ...)"""
    if small is None and large is None:
        return
    if small.is_complex():
        small, large = torch.view_as_real(small), torch.view_as_real(large)
    assert small.shape == large.shape and small.dtype == large.dtype, what
    assert torch.equal(small, large), f"{what}: small launch != large launch, {_first_difference(small, large)}"


def _same_all(small, large, names):
    assert len(small) == len(large) == len(names)
    for s, l, k in zip(small, large, names):
        _same(s, l, k)


# -- a. the walking forms against the float64 oracle ----------------------------------------------
def _oracle_envs(name):
    """first, middle and last env at 256; two of them at 1024 (the numpy FFTs stay at a few seconds)"""
    n, envs = SHAPES[name][0], SHAPES[name][3]
    if n == 256:
        return [0, envs // 2, envs - 1]
    return [0, envs - 1] if envs % 2 == 0 else [envs // 2, envs - 1]


@pytest.mark.parametrize("name", MONO)
def test_walking_forms_vs_oracle(name):
    import hbx
    n, g, p, envs, _, ml = SHAPES[name]
    assert _full_launches(envs, g, ml) == [envs] and L.walking(n, p, envs)
    ocfg = _ocfg(name)
    pre, bits, tgt = _inputs(name, 700 + envs)
    plan = hbx.Plan(dev_cfg(ocfg), max_jobs=ml)
    inten, stats, psnr = plan.propagate(bits, tgt)
    field, inten2 = plan.simulate(bits, want_intensity=True)
    torch.cuda.synchronize()
    plan.close()
    assert torch.equal(inten, inten2)
    prop = O.Propagator(ocfg)
    for e in _oracle_envs(name):
        mask = (pre[e] >= 0.5).cpu().numpy().astype(np.uint8)
        t = tgt[e].cpu().numpy()
        want_f = O.propagate(O.mask_to_field(mask, ocfg.field_kind), prop.h[0])
        want_i = np.mean(want_f.real ** 2 + want_f.imag ** 2, axis=0)[None]
        want_st = O.chan_stats(want_i[0], t[0])[None]
        ef = np.max(np.abs(field[e].cpu().numpy() - want_f)) / np.max(np.abs(want_f))
        ei = np.max(np.abs(inten[e].cpu().numpy() - want_i)) / np.max(want_i)
        st = stats[e].cpu().numpy()
        ep = abs(float(psnr[e]) - prop.psnr(want_st))
        print(f"{name} env {e}: field err {ef:.3e} of max|want|, intensity err {ei:.3e} of max(want), "
              f"stats rel err {np.max(np.abs(st / want_st - 1)):.3e}, psnr err {ep:.3e} dB")
        assert ef <= FIELD_RTOL, e
        assert ei <= INTEN_RTOL, e
        assert np.allclose(st, want_st, rtol=STATS_RTOL), e
        assert ep <= PSNR_TOL, e


def test_simulate_complex_walking_col2_vs_oracle():
    """hbx_simulate_complex's field with k_col2's walking form (64 envs of 4 complex planes at N = 256)"""
    import hbx
    name = "256x8-64"
    n, g, p, envs, _, ml = SHAPES[name]
    assert L.walking(n, p, envs)
    ocfg = _ocfg(name)
    vals = _complex_values(name, 31)
    plan = hbx.Plan(dev_cfg(ocfg), max_jobs=ml)
    field, _ = plan.simulate_complex(vals)
    torch.cuda.synchronize()
    plan.close()
    h = ocfg.transfer(0)
    for e in _oracle_envs(name):
        want = O.propagate(vals[e].cpu().numpy().astype(np.complex128), h)
        err = np.max(np.abs(field[e].cpu().numpy() - want)) / np.max(np.abs(want))
        print(f"{name} env {e}: complex field err {err:.3e} of max|want|")
        assert err <= COMPLEX_FIELD_RTOL, e


# -- b. small launch EQUAL large launch -----------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_propagate_and_simulate_small_equals_large(name):
    _, bits, tgt = _inputs(name, 11)
    small, large = _two_plans(name)
    try:
        _same_all(small.propagate(bits, tgt), large.propagate(bits, tgt), ("intensity", "chan_stats", "psnr"))
        fs, i_s = small.simulate(bits, want_intensity=True)
        fl, il = large.simulate(bits, want_intensity=True)
        _same(i_s, il, "simulate intensity")
        _same(fs, fl, "field")
    finally:
        small.close()
        large.close()


@pytest.mark.parametrize("precision", ["bf16", "f16"])
@pytest.mark.parametrize("name", AT_LINE)
def test_reduced_precision_small_equals_large(name, precision):
    import hbx
    kind = hbx.PRECISION_BF16_STORE if precision == "bf16" else hbx.PRECISION_F16_STORE
    _, bits, tgt = _inputs(name, 12)
    small, large = _two_plans(name, precision=kind)
    try:
        assert small.precision == large.precision == kind
        _same_all(small.propagate(bits, tgt), large.propagate(bits, tgt), ("intensity", "chan_stats", "psnr"))
    finally:
        small.close()
        large.close()


def _same_with_nan(small, large, bad, what):
    """candidate results: NaN exactly at the out-of-range flips, equal everywhere else"""
    for t in (small, large):
        nan = torch.isnan(t).reshape(t.shape[0], -1).all(dim=1)
        assert torch.equal(nan, bad), what
        assert not torch.isnan(t[~bad]).any(), what
    _same(small[~bad], large[~bad], what)


@pytest.mark.parametrize("name,k", [("1024x24-6", 16), ("256x8-64", 64), ("256x8-65", 65)])
def test_eval_flips_small_equals_large(name, k):
    """K candidate flips of one base env, one job each: K at the line (and one above it), the flips spread
    over every channel, one of them out of range (an invalid job inside a walking launch: NaN, as
    test_empty_batches_and_chunked_invalid_flips has it)."""
    import hbx
    n, g, p = SHAPES[name][:3]
    ms = L.first_walking(n, p) - 1
    assert ms >= g, "no launch below the line"
    _assert_sides(n, p, L.launches(k, ms), L.launches(k, k))
    ch = g * p
    rng = np.random.default_rng(5 + k)
    chan = (np.arange(k) * 5) % ch                                  # 5 is coprime to 8 and 24
    assert len(set(chan)) == min(ch, k) and set(chan // p) == set(range(g))
    flips = chan * n * n + rng.integers(0, n * n, k)
    flips[k // 2] = ch * n * n                                      # one past the last pixel
    flips[0], flips[-1] = 0, ch * n * n - 1                          # the two corners
    bad = torch.zeros(k, dtype=torch.bool, device="cuda")
    bad[k // 2] = True
    f = torch.from_numpy(flips.astype(np.int64)).cuda()
    _, bits, tgt = _inputs(name, 13)
    bits, tgt = bits[0].contiguous(), tgt[0].contiguous()
    cfg = dev_cfg(_ocfg(name))
    small, large = hbx.Plan(cfg, max_jobs=ms), hbx.Plan(cfg, max_jobs=k)
    try:
        _, st, _ = small.propagate(bits[None], tgt[None], want_intensity=False)      # one env: small on both
        ps, gs = small.eval_flips(bits, tgt, st[0].contiguous(), f)
        pl, gl = large.eval_flips(bits, tgt, st[0].contiguous(), f)
        _same_with_nan(ps, pl, bad, "psnr")
        _same(gs[~bad], gl[~bad], "group_stats")
        assert len(torch.unique(ps[~bad])) > k // 2                  # the candidates are not all alike
    finally:
        small.close()
        large.close()


def test_eval_flips_planes_small_equals_large():
    """The plane-cached candidates at the pair line: N = 256, K = 256 spare pairs, one pair per job.
    PSNRs, group statistics and the whole pool (every candidate's fresh pair in its own spare slots)."""
    import hbx
    name, k = "256x8-64", 256
    n, g, p = SHAPES[name][:3]
    assert L.first_walking(n, p, pair=True) == k
    _assert_sides(n, p, L.launches(k, k - 1), L.launches(k, k), pair=True)
    ch = g * p
    rng = np.random.default_rng(17)
    flips = (np.arange(k) % ch) * n * n + rng.integers(0, n * n, k)
    flips[0], flips[-1] = 0, ch * n * n - 1
    f = torch.from_numpy(flips.astype(np.int64)).cuda()
    _, bits, tgt = _inputs(name, 14)
    bits, tgt = bits[0].contiguous(), tgt[0].contiguous()
    cfg = dev_cfg(_ocfg(name))
    plans = hbx.Plan(cfg, max_jobs=k - 1), hbx.Plan(cfg, max_jobs=k)
    try:
        out = []
        for plan in plans:
            pool, slot = plan.plane_pool(k)
            pool.zero_()
            st, ps0 = plan.planes_fill(bits, tgt, pool, slot)            # one job: small on both
            ps, gs = plan.eval_flips_planes(bits, tgt, st, pool, slot, f)
            full, _ = plan.eval_flips(bits, tgt, st, f[:8].contiguous())   # the cache's own guarantee, 8 jobs
            assert torch.equal(ps[:8], full)
            out.append((st, ps0, ps, gs, pool, slot))
        _same_all(out[0], out[1], ("base chan_stats", "base psnr", "psnr", "group_stats", "plane pool", "plane slots"))
        assert not torch.isnan(out[0][2]).any() and len(torch.unique(out[0][2])) > k // 2
    finally:
        for plan in plans:
            plan.close()


def _complex_values(name, seed):
    n, g, p, envs = SHAPES[name][:4]
    gen = torch.Generator(device="cuda").manual_seed(seed)
    ri = 2.0 * torch.rand((envs, g * p // 2, n, n, 2), generator=gen, device="cuda") - 1.0
    return torch.view_as_complex(ri.contiguous())


def _real_values(name, seed, shape=None):
    n, g, p, envs = SHAPES[name][:4]
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand(shape or (envs, g * p, n, n), generator=gen, device="cuda")


def _evaluate_real(name, small, large, minus_z):
    tgt = _inputs(name, 21)[2]
    x = 2.0 * _real_values(name, 22) - 1.0
    return small.evaluate_real(x, tgt), large.evaluate_real(x, tgt), ("field", "intensity", "chan_stats", "psnr")


def _simulate_complex(name, small, large, minus_z):
    v = _complex_values(name, 23)
    return (small.simulate_complex(v, want_real=True), large.simulate_complex(v, want_real=True),
            ("complex field", "real part"))


def _evaluate_phase(name, small, large, minus_z):
    tgt = _inputs(name, 21)[2]
    n, g, p, envs = SHAPES[name][:4]
    x = 2.0 * _real_values(name, 24, (envs, g * p // 2, n, n)) - 1.0
    return small.evaluate_phase(x, tgt), large.evaluate_phase(x, tgt), ("field", "intensity", "chan_stats", "psnr")


def _evaluate_threshold(name, small, large, minus_z):
    tgt = _inputs(name, 21)[2]
    x = _real_values(name, 25)
    return (small.evaluate_threshold(x, 0.5, tgt), large.evaluate_threshold(x, 0.5, tgt),
            ("field", "intensity", "chan_stats", "psnr"))


def _evaluate_real_window(name, small, large, minus_z):
    n, g, p, envs = SHAPES[name][:4]
    in_win, out_win = (5, 9, n - 24, n - 31), (3, 20, n - 30, n - 41)      # multiples of nothing, in != out
    x = 2.0 * _real_values(name, 26, (envs, g * p) + in_win[2:]) - 1.0
    tgt = _real_values(name, 27, (envs, g) + out_win[2:])
    return (small.evaluate_real_window(x, in_win, tgt, out_win), large.evaluate_real_window(x, in_win, tgt, out_win),
            ("field", "intensity", "chan_stats", "psnr"))


def _phase_backward(name, small, large, minus_z):
    assert minus_z
    n, g, p, envs = SHAPES[name][:4]
    v = _complex_values(name, 28)
    x = 2.0 * _real_values(name, 29, (envs, g * p // 2, n, n)) - 1.0
    return (small.phase_backward(v, x),), (large.phase_backward(v, x),), ("phase gradient",)


SAMPLE_OPS = {"evaluate_real": _evaluate_real, "simulate_complex": _simulate_complex, "evaluate_phase": _evaluate_phase,
              "evaluate_threshold": _evaluate_threshold, "evaluate_real_window": _evaluate_real_window,
              "phase_backward": _phase_backward}


@pytest.mark.parametrize("op", list(SAMPLE_OPS))
@pytest.mark.parametrize("name", AT_LINE)
def test_sample_paths_small_equals_large(name, op):
    """Real, complex, phase, thresholded and windowed samples and the phase gradient: their first passes
    run one row block per workgroup at every launch size, k_col2 switches with the launch (the same rule,
    jobs = envs of P = 8 planes), and every array the call writes is compared."""
    minus_z = op == "phase_backward"                                   # the backward pass: the plan for -z
    small, large = _two_plans(name, **({"z": -O.Z_DEFAULT} if minus_z else {}))
    try:
        got_s, got_l, names = SAMPLE_OPS[op](name, small, large, minus_z)
        _same_all(got_s, got_l, names)
        assert all(bool(torch.isfinite(torch.view_as_real(t) if t.is_complex() else t).all()) for t in got_l)
    finally:
        small.close()
        large.close()


# -- c. the env step across the line ---------------------------------------------------------------
STEPS = 6
STATE_KEYS = ("mask", "record", "chan_stats", "prev_psnr", "init_psnr", "steps", "flip_count", "sustained")


def _envs(cfg, B, seed, variants):
    """HologramVecEnvs of the same seeded inputs, one per (mode, max_jobs) of `variants`, reset"""
    from hbx.env import HologramVecEnv
    gen = torch.Generator(device="cuda").manual_seed(seed)
    pres = [torch.rand((cfg.channels, cfg.height, cfg.width), generator=gen, device="cuda") for _ in range(B)]
    tgts = [torch.rand((cfg.groups, cfg.height, cfg.width), generator=gen, device="cuda") for _ in range(B)]
    acts = torch.randint(0, cfg.channels * cfg.height * cfg.width, (STEPS, B), generator=gen, device="cuda")
    out = {}
    for key, (mode, max_jobs) in variants.items():
        out[key] = HologramVecEnv(cfg, B, lambda i: tgts[i], pre_model_source=lambda i: pres[i], mode=mode,
                                  max_jobs=max_jobs, max_steps=STEPS - 1, auto_reset=False,
                                  obs_keys=("state", "recon_image"))
        out[key].reset()
    return out, acts


def _same_env(a, b, what, cache):
    """masks, records, statistics and counters; the state and recon_image observations; with `cache`
    (the same mode on both sides) the cached intensity too"""
    for k in STATE_KEYS + ("state_bytes", "recon") + (("intensity",) if cache else ()):
        _same(getattr(a.state, k), getattr(b.state, k), f"{what}: {k}")


def _step_all(envs, acts, pairs):
    """STEPS steps of every env with the same actions; after each, every (a, b, same mode) of `pairs` agrees
    on reward, PSNR, accepted, terminated, truncated and the state"""
    for key_a, key_b, cache in pairs:
        _same_env(envs[key_a], envs[key_b], f"reset, {key_a} vs {key_b}", cache)
    n_acc = n_rej = n_trunc = 0
    for k in range(STEPS):
        res = {key: [t.clone() for t in env.step_device(acts[k])] for key, env in envs.items()}
        for key_a, key_b, cache in pairs:
            what = f"step {k}, {key_a} vs {key_b}"
            _same_all(res[key_a], res[key_b], [f"{what}: {r}" for r in ("reward", "psnr", "accepted", "terminated",
                                                                         "truncated")])
            _same_env(envs[key_a], envs[key_b], what, cache)
        first = next(iter(res.values()))
        n_acc += int(first[2].sum())
        n_rej += int((first[2] == 0).sum())
        n_trunc += int(first[4].sum())
    for env in envs.values():
        env.state.check_error()
    assert n_acc > 0 and n_rej > 0 and n_trunc > 0      # accepts, rollbacks and the max_steps flag all occurred


def _close(envs):
    for env in envs.values():
        env.close()


def test_env_step_1024_rgb_16_small_equals_large():
    """16 envs at 1024 x 24: the reset (48 jobs) and the FFT-mode step (16 jobs) run the walking forms with
    max_jobs = 48, the small ones with max_jobs = 15 (5 envs per reset launch; 15 + 1 envs per step).  The
    plane-cached step of 16 pairs stays on the small forms behind a walking reset -- the mid-sized batch
    (16 <= B < 64) at which the plane cache's equality with the FFT mode spans both forms."""
    import hbx
    cfg, B = hbx.rgb_config(1024), 16
    _assert_sides(1024, 8, _full_launches(B, 3, 15), _full_launches(B, 3, 48))
    _assert_sides(1024, 8, L.launches(B, 15), L.launches(B, 48))
    assert not L.walking(1024, 8, B, pair=True)
    envs, acts = _envs(cfg, B, 51, {"small": ("fft", 15), "large": ("fft", 48), "planes": ("planes", 48)})
    try:
        _step_all(envs, acts, [("small", "large", True), ("planes", "large", False)])
    finally:
        _close(envs)


def test_env_step_256_mono_64_small_large_and_planes():
    """64 envs at 256 x 8: the FFT-mode step crosses the line at 64 jobs; the plane-cached step (a pair per
    job) stays on the small forms there, so mode="planes" against the large mode="fft" is the plane cache's
    equality guarantee across the two forms."""
    import hbx
    cfg, B = hbx.mono_config(256), 64
    _assert_sides(256, 8, L.launches(B, 63), L.launches(B, 64))
    assert not L.walking(256, 8, B, pair=True)
    envs, acts = _envs(cfg, B, 52, {"small": ("fft", 63), "large": ("fft", 64), "planes": ("planes", 64)})
    try:
        _step_all(envs, acts, [("small", "large", True), ("planes", "large", False)])
    finally:
        _close(envs)


def test_env_step_256_mono_256_planes_equals_fft():
    """256 envs at 256 x 8: the FFT-mode step and the plane-cached step (256 pairs) both run the walking
    forms; a plane-cached env stepped in launches of 255 + 1 pairs (the small forms) must agree as well."""
    import hbx
    cfg, B = hbx.mono_config(256), 256
    assert L.launches(B, 256) == [B] and L.walking(256, 8, B) and L.walking(256, 8, B, pair=True)
    _assert_sides(256, 8, L.launches(B, 255), L.launches(B, 256), pair=True)
    envs, acts = _envs(cfg, B, 53, {"fft": ("fft", 256), "planes": ("planes", 256), "planes_small": ("planes", 255)})
    try:
        _step_all(envs, acts, [("planes", "fft", False), ("planes_small", "planes", True)])
    finally:
        _close(envs)
