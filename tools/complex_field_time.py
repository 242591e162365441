#!/usr/bin/env python3
"""Complex-field propagation: hbx_simulate_complex against the two-real-planes route, same plan.

At N = 1024 (G = 3, P = 8: 4 complex planes per group, 30 jobs) and N = 256 (mono, P = 8, 128
jobs), on one plan, blocks of the two routes are alternated after a warm-up of both:

    (a) fused   plan.simulate_complex(u)                       about 64 N^2 bytes per complex plane
    (b) pairs   u -> [re0, im0, re1, ..] planes (a torch permute copy), plan.simulate_real, then
                out[:, 0::2] + 1j * out[:, 1::2] in torch    about 112 N^2 bytes per complex plane

Printed: the device time per block of `calls` propagations (events around the block, pass timer
off; median and range over the blocks) and (b) / (a); then, from a second set of (a) blocks with
the plan's pass timer on, the time of each pass per launch and, for the first and last passes,
their algorithmic bytes over that time as a fraction of 8 TB/s:

    first pass   8 N^2 read + 8 N^2 written   per complex plane (two half spectra of 4 N^2)
    last pass   16 N^2 read + 8 N^2 written   per complex plane (a B plane pair in, one field out)

Needs a GPU; writes what it prints to --out as well.

    python tools/complex_field_time.py --out profiles/complex_field/complex_field_time.txt
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "binary-hologram-reinforcement-learning_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

PEAK_BPS = 8.0e12
PASSES = ("k_rowfwd", "k_col", "k_rowinv")


def measure(n: int, groups: int, planes: int, jobs: int, blocks: int, calls: int, warmup: int, emit):
    import torch

    import hbx

    wl = (638e-9, 515e-9, 450e-9)[:groups] if groups == 3 else (515e-9,)
    cfg = hbx.OpticsConfig(n, n, groups, planes, wl)
    n_env = jobs // groups
    jobs = n_env * groups                      # one launch per pass and call
    cplanes = groups * planes // 2
    plan = hbx.Plan(cfg, max_jobs=jobs)
    gen = torch.Generator(device="cuda").manual_seed(n)
    u = torch.view_as_complex(torch.rand((n_env, cplanes, n, n, 2), generator=gen, device="cuda") * 2.0 - 1.0)

    def fused():
        return plan.simulate_complex(u)[0]

    def pairs():
        vals = torch.view_as_real(u).permute(0, 1, 4, 2, 3).reshape(n_env, 2 * cplanes, n, n).contiguous()
        out, _ = plan.simulate_real(vals)
        return out[:, 0::2] + 1j * out[:, 1::2]

    routes = {"fused": fused, "pairs": pairs}
    for _ in range(warmup):
        a, b = fused(), pairs()
    torch.cuda.synchronize()
    scale = float(b.abs().max())
    diff = float((a - b).abs().max()) / scale
    del a, b
    per_block = {k: [] for k in routes}
    for _ in range(blocks):
        for name, fn in routes.items():        # alternated: fused block, pairs block, fused block, ...
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(calls):
                fn()
            stop.record()
            stop.synchronize()
            per_block[name].append(start.elapsed_time(stop))
    plan.set_timing(calls)
    per_launch = {p: [] for p in PASSES}
    for _ in range(blocks):
        for _ in range(calls):
            fused()
        tm = plan.read_timing()                # waits for the block and clears the timer
        for p in PASSES:
            ms, launches, jb = tm[p]
            assert launches == calls and jb == calls * jobs, (p, launches, jb)
            per_launch[p].append(ms / launches)
    plan.set_timing(0)
    plan.close()

    emit(f"N = {n}, G = {groups}, P = {planes}: {jobs} jobs = {n_env * cplanes} complex planes per call, "
         f"{blocks} alternated blocks x {calls} calls per route; max |fused - pairs| = {diff:.2e} of max|field|")
    emit("  device ms per block: median [min, max]")
    med = {}
    for name in routes:
        v = per_block[name]
        med[name] = statistics.median(v)
        emit(f"  {name:5s} {med[name]:9.3f} [{min(v):.3f}, {max(v):.3f}]   {med[name] / calls:8.4f} ms per call")
    emit(f"  pairs / fused = {med['pairs'] / med['fused']:.2f}x (fused / pairs = {med['fused'] / med['pairs']:.3f}; "
         f"algorithmic bytes 64 / 112 = 0.571)")
    nn = n_env * cplanes * n * n               # complex samples per call
    pass_bytes = {"k_rowfwd": 16.0 * nn, "k_rowinv": 24.0 * nn}
    emit("  fused route, ms per launch with the pass timer on: median [min, max]")
    for p in PASSES:
        v = per_launch[p]
        line = f"  {p:9s} {statistics.median(v):8.4f} [{min(v):.4f}, {max(v):.4f}]"
        if p in pass_bytes:
            frac = pass_bytes[p] / (statistics.median(v) * 1e-3) / PEAK_BPS
            line += f"   {pass_bytes[p] / 1e6:8.1f} MB  -> {frac:.3f} of 8 TB/s"
        emit(line)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--blocks", type=int, default=5, help="alternated timing blocks per route")
    ap.add_argument("--calls", type=int, default=8, help="propagations per block")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("complex_field_time.py needs a GPU")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"device: {torch.cuda.get_device_name(0)}")
    measure(1024, 3, 8, 30, a.blocks, a.calls, a.warmup, emit)
    measure(256, 1, 8, 128, a.blocks, a.calls, a.warmup, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
