"""The HIP path against RECORDED RUNS OF THE REFERENCE'S OWN PROGRAMS (tests/golden/ref_*.npz; how they
are made and what they pin: tests/golden/make_ref_golden.py, tests/test_ref_parity_host.py).  Only the
fixtures are read here.  The recorded PSNRs are float64 on the oracle's physics, so the tolerances are
the suite's own for the sizes and modes used, no new numbers:

  PSNR          |gpu - recorded| <= 1e-4 dB
  reward        |gpu - recorded| <= 800 * 2e-4 (tests/test_gpu_parity.py); the importance reward as
                tests/test_gpu_parity.py::test_env_group_importance_trace compares it
  recon_image   max |gpu - oracle| <= 2e-5 * max(oracle)
  env traces    every decision, flag and counter equal at every step: the generator redrew every action
                whose |change| was within 10 x the resolution the GPU tests use (256: 1e-6 dB,
                64: 1e-7 dB), so no step is skipped
  DBS sweeps    no disagreement with the recorded accept sequence before the fixture's first near-tie
                index for the mode; at a first disagreement the recorded |change| is at or below the
                mode's resolution (what follows a flipped near-tie is another walk and is not compared)
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import hbx_oracle as O  # noqa: E402

PSNR_TOL = 1e-4
REWARD_TOL = O.RW * 2 * PSNR_TOL
RECON_RTOL = 2e-5
ENV_TRACES = ("a", "b", "c", "d", "e", "f", "g")


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm GPU")
    import hbx
    hbx.load_library()
    yield


def load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name), allow_pickle=False)


def cfg_of(d) -> O.OpticsConfig:
    h, w, g, p = (int(v) for v in d["size"])
    return O.OpticsConfig(h, w, g, p, O.WL_MONO if g == 1 else O.WL_RGB)


def dev_cfg(o: O.OpticsConfig):
    import hbx
    return hbx.OpticsConfig(o.height, o.width, o.groups, o.planes, tuple(o.wavelengths))


def dense_record(d, cfg):
    rec = np.zeros(cfg.channels * cfg.height * cfg.width, np.int8)
    rec[d["record_index"]] = d["record_value"]
    return rec.reshape(cfg.channels, cfg.height, cfg.width)


def env_kw(d):
    ms, tp, ts, td = d["params"]
    return dict(max_steps=int(ms), T_PSNR=float(tp), T_steps=int(ts), T_PSNR_DIFF=float(td))


def write_importance(vec, d):
    """The recorded importance pass into the device state (the device's own sample is drawn by another
    RNG -- a stated deviation), as test_env_group_importance_trace reads these tensors."""
    st = vec.state
    st.imp_changes[0].copy_(torch.from_numpy(d["changes"]))
    st.imp_values[0].copy_(torch.from_numpy(d["importance"]))
    st.t_psnr_diff[0] = float(d["t_psnr_diff_final"])


def check_importance_reward(d, k, prev, reward):
    """reward = importance of the sampled change nearest to the step's change (+ bonus): the device may
    pick a neighbour where two sampled changes are closer than its PSNR error (the margins of
    test_env_group_importance_trace)."""
    dist = np.abs(d["changes"] - (d["psnr"][k] - prev))
    cand = d["importance"][dist <= dist.min() + 2 * 1e-7]
    bonus = d["reward"][k] - d["importance"][np.argmin(dist)]
    assert np.min(np.abs(cand + bonus - reward)) <= 1e-6, k


def replay_vec(d, mode, importance=False):
    from hbx.env import HologramVecEnv
    cfg = cfg_of(d)
    pre, tgt = O.synthetic_inputs(cfg, int(d["seed"]))
    kw = dict(reward="importance", importance_samples=len(d["changes"])) if importance else {}
    vec = HologramVecEnv(dev_cfg(cfg), 1, lambda i: torch.from_numpy(tgt).cuda(),
                         pre_model_source=lambda i: torch.from_numpy(pre).cuda(), obs_keys=(), auto_reset=False,
                         mode=mode, refresh_every=64, **env_kw(d), **kw)
    vec.reset()
    if importance:
        write_importance(vec, d)
    st = vec.state
    assert abs(float(st.init_psnr[0]) - float(d["initial_psnr"])) <= PSNR_TOL
    prev = float(d["initial_psnr"])
    for k, a in enumerate(d["actions"]):
        r, ps, acc, term, trunc = vec.step_device(torch.tensor([int(a)], device="cuda"))
        got = (bool(acc[0]), bool(term[0]), bool(trunc[0]), int(st.steps[0]), int(st.flip_count[0]),
               int(st.sustained[0]))
        want = (bool(d["accepted"][k]), bool(d["terminated"][k]), bool(d["truncated"][k]), int(d["steps"][k]),
                int(d["flip_count"][k]), int(d["psnr_sustained_steps"][k]))
        assert abs(float(ps[0]) - d["psnr"][k]) <= PSNR_TOL, k
        assert got == want, (k, got, want)
        if importance:
            check_importance_reward(d, k, prev, float(r[0]))
        else:
            assert abs(float(r[0]) - d["reward"][k]) <= REWARD_TOL, (k, float(r[0]), d["reward"][k])
        if want[0]:
            prev = float(d["psnr"][k])
    assert np.array_equal(st.mask[0].cpu().numpy().view("<u8"), d["final_mask_bits"])
    assert np.array_equal(st.record[0].cpu().numpy().astype(np.int8), dense_record(d, cfg))
    vec.close()


@pytest.mark.parametrize("mode", ["fft", "planes", "psf"])
@pytest.mark.parametrize("name", ENV_TRACES)
def test_vec_env_replays_reference_env(golden_dir, name, mode):
    """env.py's recorded traces (a)..(g) at 256x256x8 through k_env_step_finalize in every env mode."""
    replay_vec(load(golden_dir, f"ref_env_{name}.npz"), mode)


@pytest.mark.parametrize("mode", ["fft", "psf"])
def test_vec_env_replays_reference_env_group(golden_dir, mode):
    """env_group.py's recorded trace at 64x64x8 (k_importance_reward: np.argmin's tie rule, the linear
    bonuses, the dynamic T_PSNR_DIFF) on the recorded importance lists."""
    replay_vec(load(golden_dir, "ref_env_group_64.npz"), mode, importance=True)


class _Loader:
    def __init__(self, tgt):
        self.tgt = tgt

    def __iter__(self):
        yield torch.from_numpy(self.tgt[None]), ["/data/valid/0801.png"]


def replay_dropin(d, cls, multidiscrete=False, importance=False, **kw):
    cfg = cfg_of(d)
    pre, tgt = O.synthetic_inputs(cfg, int(d["seed"]))
    env = cls(lambda t: torch.from_numpy(pre[None]).to(t.device), _Loader(tgt), config=dev_cfg(cfg), verbose=False,
              **env_kw(d), **kw)
    obs, info = env.reset()
    if importance:
        write_importance(env._vec, d)
        env.psnr_change_list, env.importance_ranks = d["changes"], d["importance"]
        env.T_PSNR_DIFF = float(d["t_psnr_diff_final"])
    assert abs(env.initial_psnr - float(d["initial_psnr"])) <= PSNR_TOL
    prev = float(d["initial_psnr"])
    for k, a in enumerate(d["actions"]):
        act = tuple(int(v) for v in O.decode_action(a, cfg.height, cfg.width)) if multidiscrete else int(a)
        obs, reward, term, trunc, step_info = env.step(act)
        assert step_info == {} and isinstance(reward, float)
        got = (term, trunc, env.steps, env.flip_count, env.psnr_sustained_steps)
        want = (bool(d["terminated"][k]), bool(d["truncated"][k]), int(d["steps"][k]), int(d["flip_count"][k]),
                int(d["psnr_sustained_steps"][k]))
        assert got == want, (k, got, want)
        if importance:
            check_importance_reward(d, k, prev, reward)
        else:
            assert abs(reward - d["reward"][k]) <= REWARD_TOL, k
        if d["accepted"][k]:
            prev = float(d["psnr"][k])
            assert abs(env.previous_psnr - prev) <= PSNR_TOL, k
    # the last step's recon_image is the stepped (pre-rollback) state's, against the oracle's propagation
    ch, r, col = (int(v) for v in O.decode_action(int(d["actions"][-1]), cfg.height, cfg.width))
    final = O.unpack_mask(d["final_mask_bits"], cfg.width).astype(np.int8)
    stepped = final.copy()
    if not d["accepted"][-1]:
        stepped[ch, r, col] ^= 1
    want_recon = O.Propagator(cfg).all_intensity(stepped)
    assert obs["recon_image"].shape == (1,) + want_recon.shape
    assert np.max(np.abs(obs["recon_image"][0] - want_recon)) <= RECON_RTOL * np.max(want_recon)
    assert np.array_equal(obs["state"][0], final) and np.array_equal(env.state[0], final)
    assert np.array_equal(obs["state_record"][0], dense_record(d, cfg))
    dc = env.device_counters()
    assert (dc["steps"], dc["flip_count"], dc["psnr_sustained_steps"]) == \
        (env.steps, env.flip_count, env.psnr_sustained_steps)
    import hbx
    assert np.array_equal(hbx.unpack_bits(env._vec.state.mask[0], cfg.width).cpu().numpy(), final)
    env.close()


@pytest.mark.parametrize("name", ENV_TRACES)
def test_dropin_env_replays_reference_env(golden_dir, name):
    from hbx.env import BinaryHologramEnv
    replay_dropin(load(golden_dir, f"ref_env_{name}.npz"), BinaryHologramEnv)


def test_dropin_env_md_replays_reference_env_md(golden_dir):
    from hbx.env import BinaryHologramEnvMD
    replay_dropin(load(golden_dir, "ref_env_md.npz"), BinaryHologramEnvMD, multidiscrete=True)


def test_dropin_env_group_replays_reference_env_group(golden_dir):
    from hbx.env import BinaryHologramEnvGroup
    d = load(golden_dir, "ref_env_group_64.npz")
    replay_dropin(d, BinaryHologramEnvGroup, importance=True, importance_samples=len(d["changes"]))


# ---- DBS ------------------------------------------------------------------------------------------
def dbs_order(d, n_pix):
    if "order" in d.files:
        return d["order"].astype(np.int64)
    order = np.arange(n_pix)
    np.random.RandomState(int(d["np_seed"])).shuffle(order)
    return order


def recorded_change(d):
    """psnr - (the last accepted psnr before it, else the initial psnr) per recorded candidate."""
    n = len(d["psnr"])
    acc = np.unpackbits(d["accepted"])[:n].astype(bool)
    best = np.maximum.accumulate(np.concatenate([[float(d["initial_psnr"])], np.where(acc, d["psnr"], -np.inf)]))
    return d["psnr"] - best[:-1]


def check_walk(d, res, mode, n):
    """The accept sequence over the first n candidates against the recording (see the module docstring)."""
    want = np.unpackbits(d["accepted"])[:n].astype(bool)
    got = np.zeros(n, bool)
    got[np.asarray(res.accepted_positions, np.int64)] = True
    differ = np.nonzero(got != want)[0]
    assert abs(res.initial_psnr - float(d["initial_psnr"])) <= PSNR_TOL
    if differ.size == 0:
        return True
    first = int(differ[0])
    assert first >= int(d[f"first_tie_{mode}"]), (mode, first)
    change = recorded_change(d)[first]
    assert abs(change) <= float(d[f"res_{mode}"]), (mode, first, change)
    return False


@pytest.mark.parametrize("mode", ["fft", "psf", "psf_host"])
def test_dbs_greedy_replays_reference_sweep(golden_dir, mode):
    """DBS.py's recorded full 64x64x8 sweep (32,768 candidates; the host-decided mode its first 8,192)."""
    import hbx
    from hbx import dbs
    d = load(golden_dir, "ref_dbs_64.npz")
    cfg = cfg_of(d)
    pre, tgt = O.synthetic_inputs(cfg, int(d["seed"]))
    order = dbs_order(d, cfg.channels * cfg.height * cfg.width)
    n = len(order) if mode != "psf_host" else 8192
    plan = hbx.Plan(dev_cfg(cfg), max_jobs=128)
    mask = hbx.pack_bits(torch.from_numpy(pre).cuda() >= 0.5)
    res = dbs.greedy(plan, mask, torch.from_numpy(tgt).cuda(), order, mode=mode, refresh_every=64, max_candidates=n)
    assert res.steps == n
    if check_walk(d, res, mode, n):
        acc = np.unpackbits(d["accepted"])[:n].astype(bool)
        assert abs(res.final_psnr - np.max(d["psnr"][:n][acc])) <= PSNR_TOL
        if n == len(order):
            assert np.array_equal(mask.cpu().numpy().view("<u8"), d["final_mask_bits"])
    plan.close()


@pytest.mark.parametrize("mode", ["fft", "psf", "psf_host"])
def test_dbs_greedy_replays_reference_early_stop(golden_dir, mode):
    """DBS_ratio_0.5.py's recorded run: the walk stops at the recorded candidate (the generator keeps the
    0.5 dB crossing 1e-4 dB clear on both sides)."""
    import hbx
    from hbx import dbs
    d = load(golden_dir, "ref_dbs_ratio05_64.npz")
    cfg = cfg_of(d)
    n_pix = cfg.channels * cfg.height * cfg.width
    pre, tgt = O.synthetic_inputs(cfg, int(d["seed"]))
    full = np.arange(n_pix)
    np.random.RandomState(int(d["np_seed"])).shuffle(full)
    n = int(d["visited"])
    assert np.array_equal(full[:n], d["order"])
    plan = hbx.Plan(dev_cfg(cfg), max_jobs=128)
    mask = hbx.pack_bits(torch.from_numpy(pre).cuda() >= 0.5)
    res = dbs.greedy(plan, mask, torch.from_numpy(tgt).cuda(), full, mode=mode, refresh_every=64,
                     stop_diff=float(d["stop_diff"]))
    assert res.stopped_early
    m = min(res.steps, n)
    res.accepted_positions = [p for p in res.accepted_positions if p < m]
    if check_walk(d, res, mode, m):                         # else a flipped near-tie: another walk from there
        assert res.steps == n
        assert abs(res.final_psnr - d["psnr"][n - 1]) <= PSNR_TOL
        assert np.array_equal(mask.cpu().numpy().view("<u8"), d["final_mask_bits"])
    plan.close()


@pytest.mark.parametrize("mode", ["fft", "psf", "psf_host"])
def test_dbs_greedy_replays_reference_rgb_sweep(golden_dir, mode):
    """DBS_1024_24.py's recorded 64x64x24 RGB sweep (group slicing, per-group wavelengths, cached group
    means): the first 32,768 candidates (the host-decided mode 8,192), the part whose PSNRs are kept."""
    import hbx
    from hbx import dbs
    d = load(golden_dir, "ref_dbs_rgb_64x24.npz")
    cfg = cfg_of(d)
    pre, tgt = O.synthetic_inputs(cfg, int(d["seed"]))
    order = dbs_order(d, cfg.channels * cfg.height * cfg.width)
    n = len(d["psnr"]) if mode != "psf_host" else 8192
    plan = hbx.Plan(dev_cfg(cfg), max_jobs=128)
    mask = hbx.pack_bits(torch.from_numpy(pre).cuda() >= 0.5)
    res = dbs.greedy(plan, mask, torch.from_numpy(tgt).cuda(), order, mode=mode, refresh_every=64, max_candidates=n)
    assert res.steps == n
    if check_walk(d, res, mode, n):
        acc = np.unpackbits(d["accepted"])[:n].astype(bool)
        assert abs(res.final_psnr - np.max(d["psnr"][:n][acc])) <= PSNR_TOL
        flips = np.zeros(cfg.channels * cfg.height * cfg.width, np.uint8)
        flips[order[:n][acc]] = 1
        want = (pre >= 0.5).astype(np.uint8) ^ flips.reshape(pre.shape)
        assert np.array_equal(mask.cpu().numpy().view("<u8"), O.pack_mask(want))
    plan.close()
