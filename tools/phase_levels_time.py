#!/usr/bin/env python3
"""Quantized phase holograms: the fused route (hbx_evaluate_phase_levels / hbx_phase_levels_backward)
against the torch-op route (quantize with torch ops, the detach trick, the continuous phase call), and the
quantizing first and last passes against their continuous siblings.

(a) Forward plus backward of tt.loss on one box, blocks of the two routes alternated after a warm-up of
    both, for L = 4 and L = 256:

      torch   q = round-to-level of x by torch ops;  xq = x + (q - x).detach()
              tt.loss(xq, target, z, field="phase").sum().backward()
      fused   tt.loss(x, target, z, field="phase", levels=L).sum().backward()

    at 1024 x 1024, G = 3, P = 8 phase planes per group, B = 4 and at 256 x 256, mono, P = 8, B = 64.
    Printed: device ms per block of `calls` forward-backward pairs (events around the block; median and
    range over the blocks), torch / route, and torch.cuda.max_memory_allocated over one pair of each
    route above what is allocated before it.

(b) The plan's pass timer, blocks alternated, on the plan those shapes use, L = 4: the first pass
    (k_rowfwd slot) of hbx_simulate_phase against hbx_simulate_phase_levels', the last pass (k_rowinv
    slot) of hbx_phase_backward against hbx_phase_levels_backward's.  Each pair moves the same bytes -- the
    first pass reads 4 N^2 and writes 8 N^2 per complex plane, the last pass reads 16 N^2 + 4 N^2 and
    writes 4 N^2 -- and the quantizing one adds a few VALU instructions per sample.  Given as ms, as a
    fraction of 8 TB/s, as the ratio of the medians, and whether the two ranges over the blocks overlap.

The library is the one hbx._lib loads (HBX_LIB selects another build).  Needs a GPU; writes what it
prints to --out as well.

    python tools/phase_levels_time.py --out profiles/phase_levels/phase_levels_time.txt
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
Z = 2e-3
DX = 7.56e-6
WL_RGB = (638e-9, 515e-9, 450e-9)


def _stats(v):
    return f"{statistics.median(v):9.3f} [{min(v):.3f}, {max(v):.3f}]"


def torch_quantize(x, levels: int):
    """the quantizer of include/hbx.h by torch ops (torch.round is round-half-to-even)"""
    import numpy as np
    import torch
    r = x - 2.0 * torch.round(x * 0.5)
    return torch.round(r * np.float32(levels / 2)) * np.float32(2.0 / levels)


def routes_ab(n: int, groups: int, planes: int, n_env: int, levels: int, blocks: int, calls: int, warmup: int, emit):
    import torch

    import torchOptics.optics as tt

    wls = WL_RGB if groups == 3 else (515e-9,)
    gen = torch.Generator(device="cuda").manual_seed(n + levels)
    x = (torch.rand((n_env, groups * planes, n, n), generator=gen, device="cuda") * 2.0 - 1.0).requires_grad_()
    target = torch.rand((n_env, groups, n, n), generator=gen, device="cuda")
    meta = {"dx": (DX, DX), "wl": wls if groups > 1 else wls[0]}

    def by_torch():
        x.grad = None
        xq = x + (torch_quantize(x, levels) - x).detach()
        tt.loss(tt.Tensor(xq, meta=meta), target, Z, field="phase").sum().backward()
        return x.grad

    def fused():
        x.grad = None
        tt.loss(tt.Tensor(x, meta=meta), target, Z, field="phase", levels=levels).sum().backward()
        return x.grad

    routes = {"fused": fused, "torch": by_torch}
    for _ in range(warmup):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    x.grad = None
    peak = {}
    for name, fn in routes.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak[name] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        x.grad = None
    per_block = {k: [] for k in routes}
    for _ in range(blocks):
        for name, fn in routes.items():        # alternated: fused block, torch block, ...
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(calls):
                fn()
            stop.record()
            stop.synchronize()
            per_block[name].append(start.elapsed_time(stop))

    emit(f"(a) N = {n}, G = {groups}, P = {planes}, B = {n_env}, L = {levels}: forward + backward of tt.loss, "
         f"{blocks} alternated blocks x {calls} calls per route")
    emit("    device ms per block: median [min, max]; ms per call; torch / route; peak MiB above the inputs")
    med = {k: statistics.median(v) for k, v in per_block.items()}
    for name in routes:
        v = per_block[name]
        emit(f"    {name:7s} {_stats(v)}   {med[name] / calls:8.4f}   {med['torch'] / med[name]:5.2f}x   {peak[name]:9.1f}")
    apart = max(per_block["fused"]) < min(per_block["torch"])
    emit(f"    fused faster with the blocks' ranges apart: {'yes' if apart else 'NO'}; fused peak lower: "
         f"{'yes' if peak['fused'] < peak['torch'] else 'NO'} ({peak['torch'] - peak['fused']:.1f} MiB; one float32 "
         f"copy of x is {4.0 * x.numel() / 2 ** 20:.1f} MiB)")
    for p in list(tt._PLANS.values()):         # the next case starts from an empty plan cache
        p.close()
    tt._PLANS.clear()


def passes_ab(n: int, groups: int, planes: int, n_env: int, levels: int, blocks: int, calls: int, warmup: int, emit):
    """planes: phase planes per group = complex planes per group of the plan (2 x planes real planes)"""
    import torch

    import hbx

    wls = WL_RGB if groups == 3 else (515e-9,)
    jobs = n_env * groups
    cplanes = groups * planes
    plan = hbx.Plan(hbx.OpticsConfig(n, n, groups, 2 * planes, wls, DX, DX, Z), max_jobs=jobs)
    gen = torch.Generator(device="cuda").manual_seed(n + 2)
    x = torch.rand((n_env, cplanes, n, n), generator=gen, device="cuda") * 2.0 - 1.0
    vals = torch.view_as_complex(torch.rand((n_env, cplanes, n, n, 2), generator=gen, device="cuda") * 2.0 - 1.0)

    routes = {"phase in": lambda: plan.simulate_phase(x),
              "levels in": lambda: plan.simulate_phase_levels(x, levels),
              "gradient out": lambda: plan.phase_backward(vals, x),
              "levels gradient out": lambda: plan.phase_levels_backward(vals, x, levels)}
    for _ in range(warmup):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    plan.set_timing(calls)
    slots = {k: {"k_rowfwd": [], "k_rowinv": []} for k in routes}
    for _ in range(blocks):
        for name, fn in routes.items():
            for _ in range(calls):
                fn()
            tm = plan.read_timing()             # waits for the block and clears the timer
            for slot in ("k_rowfwd", "k_rowinv"):
                ms, launches, jb = tm[slot]
                assert launches == calls and jb == calls * jobs, (launches, jb)
                slots[name][slot].append(ms / launches)
    plan.set_timing(0)
    plan.close()
    px = float(n_env) * cplanes * n * n
    rows = [("first pass, phase load", "phase in", "k_rowfwd", 12.0 * px),
            ("first pass, L-level load", "levels in", "k_rowfwd", 12.0 * px),
            ("last pass, phase gradient", "gradient out", "k_rowinv", 24.0 * px),
            ("last pass, L-level gradient", "levels gradient out", "k_rowinv", 24.0 * px)]
    emit(f"(b) N = {n}, G = {groups}, L = {levels}: {jobs} jobs = {n_env * cplanes} complex planes, pass timer, "
         f"{blocks} alternated blocks x {calls} launches; ms per launch: median [min, max]")
    med, rng = {}, {}
    for label, route, slot, nbytes in rows:
        v = slots[route][slot]
        med[label], rng[label] = statistics.median(v), (min(v), max(v))
        emit(f"    {label:28s} {med[label]:8.4f} [{min(v):.4f}, {max(v):.4f}]   {nbytes / 1e6:8.1f} MB  -> "
             f"{nbytes / (med[label] * 1e-3) / PEAK_BPS:.3f} of 8 TB/s")
    for new, old in (("first pass, L-level load", "first pass, phase load"),
                     ("last pass, L-level gradient", "last pass, phase gradient")):
        overlap = rng[new][0] <= rng[old][1] and rng[old][0] <= rng[new][1]
        emit(f"    {new} / {old.split(', ')[1]} = {med[new] / med[old]:.3f}; the blocks' ranges "
             f"{'overlap' if overlap else 'are APART'}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--blocks", type=int, default=5, help="alternated timing blocks per route")
    ap.add_argument("--calls", type=int, default=8, help="calls per block")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="ab", help="sections to run, e.g. b")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("phase_levels_time.py needs a GPU")
    from hbx import _lib
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"device: {torch.cuda.get_device_name(0)}; library: {os.path.basename(_lib.LIB_PATH)}")
    shapes = ((1024, 3, 8, 4), (256, 1, 8, 64))
    if "a" in a.only:
        for shape in shapes:
            for levels in (4, 256):
                routes_ab(*shape, levels, a.blocks, a.calls, a.warmup, emit)
    if "b" in a.only:
        for shape in shapes:
            passes_ab(*shape, 4, a.blocks, a.calls, a.warmup, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
