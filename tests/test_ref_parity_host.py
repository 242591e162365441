"""The float64 oracle against RECORDED RUNS OF THE REFERENCE'S OWN PROGRAMS (tests/golden/ref_*.npz,
written by tests/golden/make_ref_golden.py through oracle/ref_run.py): env.py, env_md.py, env_group.py
and the loop functions of DBS.py, DBS_ratio_0.5.py and DBS_1024_24.py, run unmodified on the oracle's
physics.  The recordings pin the control logic -- accept / rollback, which counters a rolled-back step
moves, the rollback-at-max_steps quirk, the `diff < 0.1` clause, the two cubic constants, the linear
bonuses, np.argmin's tie rule, the strict > of the DBS loops, the early stop, the pre-model histogram --
not the physics (torchOptics is absent; a recorded PSNR is the oracle's own number).

What must hold: masks, records, counters, flags and accept sequences exactly; PSNR within 1e-11 dB and
reward within 1e-9 (a torch-formula PSNR in place of the oracle's moved the reward by 4.3e-12; the
bound is 200 x that and seven orders below the 0.04 between the two cubic constants).

The regeneration guard re-runs a prefix of two recordings through oracle/ref_run.py when the reference
checkout is present, and skips otherwise."""
import os
import zlib

import numpy as np
import pytest

from oracle import hbx_oracle as O

PSNR_TOL = 1e-11
REWARD_TOL = 1e-9
ENV_TRACES = ("a", "b", "c", "d", "e", "f", "g")


def load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name), allow_pickle=False)


def cfg_of(d) -> O.OpticsConfig:
    h, w, g, p = (int(v) for v in d["size"])
    return O.OpticsConfig(h, w, g, p, O.WL_MONO if g == 1 else O.WL_RGB)


def dense_record(d, cfg):
    rec = np.zeros(cfg.channels * cfg.height * cfg.width, np.int8)
    rec[d["record_index"]] = d["record_value"]
    return rec.reshape(cfg.channels, cfg.height, cfg.width)


def env_params(d):
    ms, tp, ts, td = d["params"]
    return dict(max_steps=int(ms), T_PSNR=float(tp), T_steps=int(ts), T_PSNR_DIFF=float(td))


def replay_env(d, oe):
    """Steps the (reset) oracle env through the recording; every per-step output compared."""
    assert abs(oe.initial_psnr - float(d["initial_psnr"])) <= PSNR_TOL
    for k, a in enumerate(d["actions"]):
        prev = oe.previous_psnr
        r = oe.step(int(a))
        assert abs(r.psnr - d["psnr"][k]) <= PSNR_TOL, k
        assert abs(r.psnr - prev) > float(d["clear"]), k              # the recording's decisions are clear
        assert abs(r.reward - d["reward"][k]) <= REWARD_TOL, (k, r.reward, d["reward"][k])
        assert (r.accepted, r.terminated, r.truncated) == \
            (bool(d["accepted"][k]), bool(d["terminated"][k]), bool(d["truncated"][k])), k
        assert (oe.steps, oe.flip_count, oe.psnr_sustained_steps) == \
            (int(d["steps"][k]), int(d["flip_count"][k]), int(d["psnr_sustained_steps"][k])), k
    assert np.array_equal(O.pack_mask(oe.state.astype(np.uint8)), d["final_mask_bits"])
    assert np.array_equal(oe.state_record, dense_record(d, oe.cfg))


@pytest.mark.parametrize("name", ENV_TRACES)
def test_oracle_env_replays_reference_env(golden_dir, name):
    d = load(golden_dir, f"ref_env_{name}.npz")
    cfg = cfg_of(d)
    assert (cfg.height, cfg.channels) == (256, 8)                     # env.py at its own size
    oe = O.OracleEnv(cfg, **env_params(d))
    oe.reset(*O.synthetic_inputs(cfg, int(d["seed"])))
    replay_env(d, oe)


def test_reference_env_traces_walk_every_branch(golden_dir):
    """What each recording is there for, read off the recording itself (the reference's outputs)."""
    t = {n: load(golden_dir, f"ref_env_{n}.npz") for n in ENV_TRACES}

    def cubic(d, k, const):
        s = d["flip_count"][k] / d["steps"][k]
        return 1828.57 * s ** 3 - 3733.33 * s ** 2 + 2800 * s + const

    def change(d, k):
        acc = np.nonzero(d["accepted"][:k])[0]
        return d["psnr"][k] - (d["psnr"][acc[-1]] if acc.size else d["initial_psnr"])

    a = t["a"]
    assert len(a["actions"]) == 300 and 0 < a["accepted"].sum() < 300 and not a["terminated"].any()
    assert a["steps"][-1] == 300 and a["flip_count"][-1] == a["accepted"].sum()
    assert a["record_value"].sum() == 300                             # rolled-back steps are recorded too
    assert np.array_equal(a["reward"] < 0, ~a["accepted"])            # env.py:188-196: 800 * change either way
    b = t["b"]                                                         # success: -595.2, terminated alone
    assert b["terminated"][-1] and not b["truncated"][-1] and b["psnr_sustained_steps"][-1] == 2
    assert not b["terminated"][:-1].any() and 1 in b["psnr_sustained_steps"][:-1]
    assert abs(b["reward"][-1] - (800 * change(b, len(b["psnr"]) - 1) + cubic(b, -1, -595.2))) <= REWARD_TOL
    c = t["c"]                                                         # the diff < 0.1 clause: ends, no bonus
    assert c["terminated"][-1] and not c["truncated"][-1] and c["psnr_sustained_steps"][-1] == 3
    assert abs(c["reward"][-1] - 800 * change(c, len(c["psnr"]) - 1)) <= REWARD_TOL and (~c["accepted"]).any()
    d = t["d"]                                                         # max_steps: -595.24, both flags
    assert d["terminated"][-1] and d["truncated"][-1] and d["steps"][-1] == int(d["params"][0])
    assert abs(d["reward"][-1] - (800 * change(d, len(d["psnr"]) - 1) + cubic(d, -1, -595.24))) <= REWARD_TOL
    e = t["e"]                                                         # the rollback at max_steps does not end
    ms = int(e["params"][0])
    assert e["steps"][ms - 1] == ms and not e["accepted"][ms - 1]
    assert not e["terminated"][ms - 1] and not e["truncated"][ms - 1]
    assert e["accepted"][ms] and e["terminated"][ms] and e["truncated"][ms] and e["steps"][ms] == ms + 1
    f = t["f"]                                                         # both cubics on one step
    assert f["terminated"][-1] and f["truncated"][-1] and f["psnr_sustained_steps"][-1] == 1
    assert abs(f["reward"][-1] - (800 * change(f, len(f["psnr"]) - 1) + cubic(f, -1, -595.2)
                                  + cubic(f, -1, -595.24))) <= REWARD_TOL
    g = t["g"]                                                         # the int8 record wraps past 127
    assert str(g["raised"]) == "" and len(g["actions"]) == 130 and len(set(g["actions"].tolist())) == 1
    assert g["record_value"].tolist() == [np.int8(130 - 256)]


def test_oracle_env_replays_reference_env_md(golden_dir):
    """env_md.py: (channel, row, col) actions step like env.py's flat index."""
    d = load(golden_dir, "ref_env_md.npz")
    cfg = cfg_of(d)
    oe = O.OracleEnv(cfg, **env_params(d))
    oe.reset(*O.synthetic_inputs(cfg, int(d["seed"])))
    assert len(d["actions"]) == 60 and 0 < d["accepted"].sum() < 60
    replay_env(d, oe)


def test_oracle_env_group_replays_reference(golden_dir):
    """env_group.py at IPS = 64: the K = 10,000 importance pass (sampled by np.random.randint after
    np.random.seed -- replayed here from the seed), psnr_change_list, importance_ranks, the dynamic
    T_PSNR_DIFF, np.argmin's first-minimum rule in the reward and both linear bonuses."""
    d = load(golden_dir, "ref_env_group_64.npz")
    cfg = cfg_of(d)
    n_pix = cfg.channels * cfg.height * cfg.width
    rs = np.random.RandomState(int(d["np_seed"]))
    sample = np.array([rs.randint(n_pix) for _ in range(len(d["sample"]))])
    assert len(sample) == 10000 and np.array_equal(sample, d["sample"])
    p = env_params(d)
    oe = O.OracleEnvGroup(cfg, **p)
    oe.reset_group(*O.synthetic_inputs(cfg, int(d["seed"])), sample)
    assert np.max(np.abs(oe.psnr_change_list - d["changes"])) <= PSNR_TOL
    assert abs(oe.T_PSNR_DIFF - float(d["t_psnr_diff_final"])) <= len(sample) * PSNR_TOL
    # equal sampled changes (a pixel drawn twice) tie in the sort: whichever order the reference's
    # np.argsort left them in, the oracle's ranks must be a permutation of them WITHIN each tie
    # group and equal everywhere else
    ranks = np.asarray(oe.importance_ranks)
    _, inverse, counts = np.unique(d["changes"], return_inverse=True, return_counts=True)
    single = counts[inverse] == 1
    assert single.sum() > 5000 and (~single).sum() > 0
    assert np.max(np.abs(ranks[single] - d["importance"][single])) <= 1e-12
    for g in np.nonzero(counts > 1)[0]:
        idx = np.nonzero(inverse == g)[0]
        assert np.max(np.abs(np.sort(ranks[idx]) - np.sort(d["importance"][idx]))) <= 1e-12
    # the step rewards read the RECORDED lists (the reference's tie order), as the device test writes them
    oe.psnr_change_list, oe.importance_ranks = d["changes"], d["importance"]
    oe.T_PSNR_DIFF = float(d["t_psnr_diff_final"])
    replay_env(d, oe)
    n = len(d["actions"])
    bonus = O.group_linear_bonus(n)
    assert d["terminated"][-1] and d["truncated"][-1] and int(d["params"][0]) == n
    assert d["reward"][-1] > 2 * bonus - 1 and 1 in d["psnr_sustained_steps"][:-1]


def recorded_change(d):
    """psnr - (the last accepted psnr before it, else the initial psnr) per recorded candidate."""
    n = len(d["psnr"])
    acc = np.unpackbits(d["accepted"])[:n].astype(bool)
    best = np.maximum.accumulate(np.concatenate([[float(d["initial_psnr"])], np.where(acc, d["psnr"], -np.inf)]))
    return d["psnr"] - best[:-1]


def dbs_arrays(d, n_pix):
    """(visited part of the order, accept flags, visited count); the order is what np.random.seed(np_seed)
    followed by np.random.shuffle(arange) gives (the fixture's checksum, and its stored order if any)."""
    n = int(d["visited"])
    full = np.arange(n_pix)
    np.random.RandomState(int(d["np_seed"])).shuffle(full)
    assert zlib.crc32(full.tobytes()) == int(d["order_crc"])
    if "order" in d.files:
        assert np.array_equal(full[:len(d["order"])], d["order"])
    return full[:n], np.unpackbits(d["accepted"])[:n].astype(bool), n


def test_oracle_dbs_replays_reference_sweep(golden_dir):
    """DBS.py's loop, a full 64x64x8 sweep: the strict >, every candidate's PSNR (re-propagating oracle
    on a prefix, the linear oracle over the whole sweep), the final mask; the reference's last print
    was reached (a threshold print came first)."""
    d = load(golden_dir, "ref_dbs_64.npz")
    cfg = cfg_of(d)
    n_pix = cfg.channels * cfg.height * cfg.width
    order, accepted, n = dbs_arrays(d, n_pix)
    assert n == n_pix and sorted(order.tolist()) == list(range(n_pix))
    assert len(d["printed_steps"]) >= 2 and d["printed_steps"][-1] == n
    assert int(d["first_tie_fft"]) >= 2000
    pre, tgt = O.synthetic_inputs(cfg, int(d["seed"]))
    env = O.OracleEnv(cfg, accept_rule=1)
    env.reset(pre, tgt)
    assert abs(env.initial_psnr - float(d["initial_psnr"])) <= PSNR_TOL
    acc, ps, _ = O.dbs_greedy(env, order[:2000])
    assert np.array_equal(acc, accepted[:2000]) and np.max(np.abs(ps - d["psnr"][:2000])) <= PSNR_TOL
    lg = O.LinearGreedy(cfg, pre, tgt)
    acc, ps, ch = lg.run(order)
    assert np.array_equal(acc, accepted)
    assert np.max(np.abs(ps - d["psnr"])) <= PSNR_TOL and np.max(np.abs(ch - recorded_change(d))) <= 2 * PSNR_TOL
    assert np.array_equal(O.pack_mask(lg.state.astype(np.uint8)), d["final_mask_bits"])


def test_oracle_dbs_replays_reference_early_stop(golden_dir):
    """DBS_ratio_0.5.py's loop: the early stop (psnr - initial >= 0.5, checked after every candidate)."""
    d = load(golden_dir, "ref_dbs_ratio05_64.npz")
    cfg = cfg_of(d)
    n_pix = cfg.channels * cfg.height * cfg.width
    order, accepted, n = dbs_arrays(d, n_pix)
    assert 0 < n < n_pix
    full = np.arange(n_pix)
    np.random.RandomState(int(d["np_seed"])).shuffle(full)
    env = O.OracleEnv(cfg, accept_rule=1)
    env.reset(*O.synthetic_inputs(cfg, int(d["seed"])))
    acc, ps, final = O.dbs_greedy(env, full, stop_diff=float(d["stop_diff"]))
    assert len(acc) == n and np.array_equal(acc, accepted)
    assert np.max(np.abs(ps - d["psnr"])) <= PSNR_TOL
    assert ps[-1] - env.initial_psnr >= 0.5 > np.max(ps[:-1]) - env.initial_psnr
    assert np.array_equal(O.pack_mask(env.state.astype(np.uint8)), d["final_mask_bits"])


def test_oracle_dbs_replays_reference_rgb_sweep(golden_dir):
    """DBS_1024_24.py's loop on 64x64x24: group slicing by int(C/3) / int(2C/3), per-group wavelengths,
    cached group means, the pre-model histogram (with the reference's bookkeeping: a bin's total is its
    pixel count plus its improved count) and the artifact file names."""
    from hbx import dbs
    d = load(golden_dir, "ref_dbs_rgb_64x24.npz")
    cfg = cfg_of(d)
    assert (cfg.groups, cfg.planes) == (3, 8)
    n_pix = cfg.channels * cfg.height * cfg.width
    order, accepted, n = dbs_arrays(d, n_pix)
    assert n == n_pix
    pre, tgt = O.synthetic_inputs(cfg, int(d["seed"]))
    lg = O.LinearGreedy(cfg, pre, tgt)
    assert abs(lg.initial_psnr - float(d["initial_psnr"])) <= PSNR_TOL
    acc, ps, ch = lg.run(order)
    assert np.array_equal(acc, accepted)
    kept = len(d["psnr"])
    assert np.max(np.abs(ps[:kept] - d["psnr"])) <= PSNR_TOL
    assert abs(lg.previous_psnr - float(d["final_psnr"])) <= PSNR_TOL
    assert np.array_equal(O.pack_mask(lg.state.astype(np.uint8)), d["final_mask_bits"])
    for g in range(3):                                                 # every colour group took flips
        assert accepted[(order // (64 * 64)) // 8 == g].any()
    attempted, improved, dsum = O.premodel_histogram(pre, order, acc, ch, cfg.height, cfg.width)
    assert np.array_equal(improved, d["hist_improved"]) and improved.sum() == accepted.sum()
    bins = np.bincount([O.premodel_bin(float(v)) for v in pre.reshape(-1)], minlength=10)
    assert np.array_equal(bins + improved, d["hist_total"])
    assert np.max(np.abs(dsum - d["hist_psnr_sum"])) <= 5.1e-7         # printed with 6 decimals
    assert tuple(str(s) for s in d["saved_files"]) == dbs.rgb_artifact_paths("0801")
    assert d["saved_shapes"].tolist() == [[1, 3, 64, 64]] * 2


# ---- the regeneration guard -----------------------------------------------------------------------
def test_recordings_regenerate_from_the_reference(golden_dir):
    """Re-runs the reference through oracle/ref_run.py -- trace (a)'s first 60 steps and the first 2,000
    candidates of the DBS.py sweep -- and compares them array for array with the committed fixtures."""
    from oracle import ref_run
    if not ref_run.reference_available():
        pytest.skip(f"no reference checkout (set {ref_run.REF_ENV_VAR} to regenerate-check the ref_*.npz fixtures)")
    from tests.golden import make_ref_golden as M
    want = load(golden_dir, "ref_env_a.npz")
    n = M.GUARD_ENV_STEPS
    got = M.make_env_traces(None, None, only=("a",), steps_limit=n)["a"]
    for key in ("actions", "psnr", "reward", "accepted", "terminated", "truncated", "steps", "flip_count",
                "psnr_sustained_steps"):
        assert np.array_equal(got[key], want[key][:n]), key
    assert got["initial_psnr"] == want["initial_psnr"] and np.array_equal(got["params"], want["params"])
    want = load(golden_dir, "ref_dbs_64.npz")
    n = M.GUARD_DBS_CANDIDATES
    got = M.make_dbs(None, None, limit=n)
    assert int(got["visited"]) == n and got["seed"] == want["seed"]
    assert np.array_equal(got["order"], want["order"]) and np.array_equal(got["psnr"], want["psnr"][:n])
    assert np.array_equal(np.unpackbits(got["accepted"])[:n], np.unpackbits(want["accepted"])[:n])
    for mode in ("fft", "psf", "psf_host"):
        assert min(int(got[f"first_tie_{mode}"]), n) == min(int(want[f"first_tie_{mode}"]), n)
