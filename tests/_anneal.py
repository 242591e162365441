"""The float64 serial loop of the annealed greedy walk (hbx.dbs.greedy(slack=), an EXTENSION with no
reference counterpart), restated on the oracle's O.LinearGreedy.evaluate / .commit -- the oracle
itself has the strict rule alone and is not edited.

The candidate at position q of `order` is accepted iff  ps > (prev - slack[q])  in float64 (one
subtraction rounded once, then the compare; prev is the CURRENT state's PSNR).  A NaN slack
rejects, +inf accepts every candidate that has a PSNR; under fill = (target count, tol) an
inadmissible candidate has no PSNR and is rejected whatever its slack.  stop_diff is checked where
the device walk checks it: when a candidate is accepted, ps - initial >= stop_diff."""
import numpy as np

from oracle import hbx_oracle as O


def annealed_loop(lg: "O.LinearGreedy", order, slack, stop_diff=None, fill=None):
    """Runs the loop on `lg` (modified).  Returns (accepted flags, PSNR per candidate, margin per
    candidate = ps - (prev - slack[q])), each over the candidates visited; a candidate without a
    PSNR has NaN for both.  lg.fill_counts holds the per-group counts under `fill`."""
    c = lg.cfg
    accepted, psnrs, margins = [], [], []
    lg.fill_counts = None if fill is None else O.group_fill_counts(lg.state, c.groups)
    for q, a in enumerate(order):
        a = int(a)
        if fill is not None:
            ch, r, col = (int(v) for v in O.decode_action(a, c.height, c.width))
            g = ch // c.planes
            bit = int(lg.state[ch, r, col])
            if not O.fill_admissible(int(lg.fill_counts[g]), fill[0], fill[1], bit):
                accepted.append(False)
                psnrs.append(np.nan)
                margins.append(np.nan)
                continue
        ev = lg.evaluate(a)
        ps = float(ev[0])
        bar = float(lg.previous_psnr) - float(slack[q])        # rounded once
        ok = ps > bar
        accepted.append(ok)
        psnrs.append(ps)
        margins.append(ps - bar)
        if ok:
            if fill is not None:
                lg.fill_counts[g] += -1 if bit else 1
            lg.commit(a, ev)
            if stop_diff is not None and ps - lg.initial_psnr >= stop_diff:
                break
    return np.array(accepted, bool), np.array(psnrs, np.float64), np.array(margins, np.float64)


# the committed fixtures (tests/golden/make_anneal_golden.py): file -> (the existing fixture that
# names the image and the order, candidates, metropolis_slack's t_start, t_end, seed)
ANNEAL_FIXTURES = {
    "dbs_anneal_256.npz": ("dbs_ratio05_256.npz", 3000, 1.25e-4, 1.25e-6, 6),
    "dbs_anneal_1024x24.npz": ("dbs_prefix_1024x24_16k.npz", 1200, 2e-6, 2e-8, 9),
}


def base_fixture(golden_dir, name):
    """(ocfg, pre, tgt, order) of an existing DBS fixture (as tests/test_gpu_dbs_headline._fixture,
    restated here so that the CPU tests and the generator import no GPU test module)."""
    import os
    d = np.load(os.path.join(golden_dir, name), allow_pickle=False)
    n, g, p = int(d["size"]), int(d["groups"]), int(d["planes"])
    ocfg = O.OpticsConfig(n, n, g, p, O.WL_RGB if g == 3 else O.WL_MONO, field_kind=int(d["field_kind"]))
    pre, tgt = O.synthetic_inputs(ocfg, int(d["seed"]))
    order = np.random.default_rng(int(d["order_seed"])).permutation(ocfg.channels * n * n)
    return ocfg, pre, tgt, order


def make_fixture(golden_dir, name):
    """The arrays of one annealed fixture, computed (CPU, float64; seconds at 256, half a minute at 1024)."""
    from hbx import dbs
    base, n, t0, t1, seed = ANNEAL_FIXTURES[name]
    ocfg, pre, tgt, order = base_fixture(golden_dir, base)
    slack = dbs.metropolis_slack(n, t0, t1, seed)
    lg = O.LinearGreedy(ocfg, pre, tgt)
    acc, ps, margin = annealed_loop(lg, order[:n], slack)
    return dict(accepted=acc, psnr=ps, margin=margin, n=np.int64(n), t_start=np.float64(t0), t_end=np.float64(t1),
                slack_seed=np.int64(seed), initial_psnr=np.float64(lg.initial_psnr),
                final_psnr=np.float64(lg.previous_psnr))
