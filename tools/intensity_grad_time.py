#!/usr/bin/env python3
"""Plane-mean intensity and its gradient: tt.intensity against the torch-op chain, and the weighted
complex first pass against the unweighted one.

(a) Forward plus backward of L = sum w I on one box, blocks of the routes alternated after a
    warm-up of all of them:

      fused      tt.intensity(x, z).mul(w).sum().backward()                  (save_field=True)
      recompute  the same with save_field=False (no field kept; the backward pass propagates again)
      chain      (tt.simulate(x, z, binary=False).abs() ** 2).mean(1, keepdim=True) per colour group
                 (one call per wavelength), .mul(w).sum().backward(): torch ops around the field

    at 1024 x 1024, G = 3, P = 8, B = 4 and at 256 x 256, mono, P = 8, B = 64.  Printed: device ms per
    block of `calls` forward-backward pairs (events around the block; median and range over the
    blocks), chain / route, and torch.cuda.max_memory_allocated over one pair of each route above
    what is allocated before it (x, w and the shim's cached plans).

(b) The first pass of the backward pass's launch set, from the plan's pass timer: on the -z plan
    with 2 P real planes per group, blocks of hbx_simulate_complex (real_part only) and of
    hbx_simulate_complex_weighted are alternated.  Per complex plane the unweighted first pass reads
    8 N^2 and writes 8 N^2 bytes, the weighted one reads 12 N^2 (the weight image is counted once per
    plane, as the kernel loads it) and writes 8 N^2; each is given as a fraction of 8 TB/s.

Needs a GPU; writes what it prints to --out as well.

    python tools/intensity_grad_time.py --out profiles/intensity_grad/intensity_grad_time.txt
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


def routes_ab(n: int, groups: int, planes: int, n_env: int, blocks: int, calls: int, warmup: int, emit):
    import torch

    import torchOptics.optics as tt

    wls = WL_RGB if groups == 3 else (515e-9,)
    gen = torch.Generator(device="cuda").manual_seed(n)
    x = torch.rand((n_env, groups * planes, n, n), generator=gen, device="cuda").requires_grad_()
    w = torch.rand((n_env, groups, n, n), generator=gen, device="cuda")
    meta_all = {"dx": (DX, DX), "wl": wls if groups > 1 else wls[0]}

    def fused(save=True):
        x.grad = None
        tt.intensity(tt.Tensor(x, meta=meta_all), Z, save_field=save).mul(w).sum().backward()
        return x.grad

    def chain():
        x.grad = None
        inten = torch.cat([(tt.simulate(tt.Tensor(x[:, k * planes:(k + 1) * planes], meta={"dx": (DX, DX), "wl": wls[k]}),
                                        Z, binary=False).abs() ** 2).mean(1, keepdim=True) for k in range(groups)], dim=1)
        inten.mul(w).sum().backward()
        return x.grad

    routes = {"fused": fused, "recompute": lambda: fused(False), "chain": chain}
    for _ in range(warmup):
        grads = {k: fn().clone() for k, fn in routes.items()}
    torch.cuda.synchronize()
    scale = float(grads["chain"].abs().max())
    diffs = {k: float((grads[k] - grads["chain"]).abs().max()) / scale for k in ("fused", "recompute")}
    del grads
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
        for name, fn in routes.items():        # alternated: fused block, recompute block, chain block, ...
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(calls):
                fn()
            stop.record()
            stop.synchronize()
            per_block[name].append(start.elapsed_time(stop))

    emit(f"(a) N = {n}, G = {groups}, P = {planes}, B = {n_env}: forward + backward of sum w I, {blocks} alternated "
         f"blocks x {calls} calls per route")
    emit(f"    max |grad - chain grad| of max|grad|: fused {diffs['fused']:.2e}, recompute {diffs['recompute']:.2e}")
    emit("    device ms per block: median [min, max]; ms per call; chain / route; peak MiB above the inputs")
    med = {k: statistics.median(v) for k, v in per_block.items()}
    for name in routes:
        v = per_block[name]
        emit(f"    {name:9s} {_stats(v)}   {med[name] / calls:8.4f}   {med['chain'] / med[name]:5.2f}x   {peak[name]:9.1f}")
    for name in ("fused", "recompute"):
        apart = max(per_block[name]) < min(per_block["chain"])
        emit(f"    {name} faster than chain with the blocks' ranges apart: {'yes' if apart else 'NO'}")
    for p in list(tt._PLANS.values()):         # the next shape starts from an empty plan cache
        p.close()
    tt._PLANS.clear()


def first_pass_ab(n: int, groups: int, planes: int, n_env: int, blocks: int, calls: int, warmup: int, emit):
    import torch

    import hbx

    wls = WL_RGB if groups == 3 else (515e-9,)
    cfg = hbx.OpticsConfig(n, n, groups, 2 * planes, wls, DX, DX, -Z)   # the backward pass's plan
    jobs = n_env * groups
    cplanes = groups * planes
    plan = hbx.Plan(cfg, max_jobs=jobs)
    gen = torch.Generator(device="cuda").manual_seed(n + 1)
    field = torch.view_as_complex(torch.rand((n_env, cplanes, n, n, 2), generator=gen, device="cuda") * 2.0 - 1.0)
    gi = torch.rand((n_env, groups, n, n), generator=gen, device="cuda")

    routes = {"unweighted": lambda: plan.simulate_complex(field, want_field=False, want_real=True),
              "weighted": lambda: plan.simulate_complex(field, want_field=False, want_real=True, weight=gi,
                                                        scale=2.0 / planes)}
    for _ in range(warmup):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    plan.set_timing(calls)
    per_launch = {k: [] for k in routes}
    for _ in range(blocks):
        for name, fn in routes.items():
            for _ in range(calls):
                fn()
            ms, launches, jb = plan.read_timing()["k_rowfwd"]   # waits for the block and clears the timer
            assert launches == calls and jb == calls * jobs, (launches, jb)
            per_launch[name].append(ms / launches)
    plan.set_timing(0)
    plan.close()
    nn = n_env * cplanes * n * n               # complex samples per launch
    nbytes = {"unweighted": 16.0 * nn, "weighted": 20.0 * nn}
    emit(f"(b) N = {n}, G = {groups}: first pass (k_rowfwd slot) of {jobs} jobs = {n_env * cplanes} complex planes, "
         f"{blocks} alternated blocks x {calls} launches; ms per launch: median [min, max]")
    med = {}
    for name in routes:
        v = per_launch[name]
        med[name] = statistics.median(v)
        frac = nbytes[name] / (med[name] * 1e-3) / PEAK_BPS
        emit(f"    {name:10s} {statistics.median(v):8.4f} [{min(v):.4f}, {max(v):.4f}]   {nbytes[name] / 1e6:8.1f} MB  "
             f"-> {frac:.3f} of 8 TB/s")
    emit(f"    weighted / unweighted = {med['weighted'] / med['unweighted']:.3f} (bytes 20 / 16 = 1.25)")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--blocks", type=int, default=5, help="alternated timing blocks per route")
    ap.add_argument("--calls", type=int, default=8, help="calls per block")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("intensity_grad_time.py needs a GPU")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"device: {torch.cuda.get_device_name(0)}")
    for shape in ((1024, 3, 8, 4), (256, 1, 8, 64)):
        routes_ab(*shape, a.blocks, a.calls, a.warmup, emit)
    for shape in ((1024, 3, 8, 4), (256, 1, 8, 64)):
        first_pass_ab(*shape, a.blocks, a.calls, a.warmup, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
