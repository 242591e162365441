"""Generates the annealed-walk fixtures (tests/_anneal.py ANNEAL_FIXTURES): the float64 serial loop
of hbx.dbs.greedy(slack=metropolis_slack(...)) over a prefix of an existing fixture's order --
accepted flags, PSNR and margin ps - (prev - slack) per candidate, and the schedule's parameters.
Deterministic, CPU only (about 3 s at 256x256x8, about half a minute at 1024x1024x24).

    python tests/golden/make_anneal_golden.py            # both files
    python tests/golden/make_anneal_golden.py dbs_anneal_256.npz
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "binary-hologram-reinforcement-learning_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from tests import _anneal  # noqa: E402


def main(names):
    for name in names or list(_anneal.ANNEAL_FIXTURES):
        arrays = _anneal.make_fixture(HERE, name)
        np.savez_compressed(os.path.join(HERE, name), **arrays)
        acc, ps, m = arrays["accepted"], arrays["psnr"], arrays["margin"]
        prev = np.concatenate([[float(arrays["initial_psnr"])], ps[acc]])[:-1] if acc.any() else np.zeros(0)
        order_m = np.argsort(np.abs(m))[:3]
        print(f"{name}: {int(acc.sum())} accepts of {len(acc)}, {int((ps[acc] < prev).sum())} downhill; "
              "smallest |margin| " + ", ".join(f"{abs(m[i]):.3g} dB at {int(i)}" for i in order_m))


if __name__ == "__main__":
    main(sys.argv[1:])
