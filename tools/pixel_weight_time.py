#!/usr/bin/env python3
"""Per-pixel loss weights: tt.loss(.., pixel_weight=v) (hbx_evaluate_pw, hbx_pixel_weight_sum, hbx_loss_pw,
hbx_loss_weight_pw) against the route it replaces and against the unweighted loss, and each weighted last pass
against its unweighted sibling.

(a) Forward plus backward on one box, blocks of the three routes alternated after a warm-up of all, for a
    thresholded leaf (threshold=0.5) and a phase leaf:

      weighted  tt.loss(x, target, z, pixel_weight=v).sum().backward()
      torch     I = tt.intensity(x, z); the weighted sums, the least-squares scale and the loss as float32
                torch ops over the full-grid tensors; autograd back through them into tt.intensity's backward
      plain     tt.loss(x, target, z).sum().backward()         the feature's cost is weighted / plain

    At 1024 x 1024, G = 3, P = 8 planes per group, B = 4 and at 256 x 256, mono, P = 8, B = 64.  Printed:
    device ms per block of `calls` forward-backward pairs (events around the block; median and range over
    the blocks), ms per call, the ratio to the weighted route with whether the blocks' ranges overlap, and
    torch.cuda.max_memory_allocated over one pair of each route above what is allocated before it (torch's
    allocator only; the three routes use the same two plans).

(b) The plan's pass timer (k_rowinv slot), blocks alternated, on the forward plan of those shapes: the last
    pass of Plan.evaluate_pw against that of the unweighted evaluate call of the same leaf kind, with the
    field and the intensity written (what a gradient request runs) and, for the thresholded leaf, with neither
    (what a call without one runs: the sibling is then the lean, target-ahead form, which has no weighted
    form).  The weighted pass reads one more float row per group and row.

N = 896 and N = 64 are not timed.  The library is the one hbx._lib loads (HBX_LIB selects another build).
Needs a GPU; writes what it prints to --out as well.

    python tools/pixel_weight_time.py --out profiles/pixel_weight/pixel_weight_time.txt
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

DX = 7.56e-6
WL_RGB = (638e-9, 515e-9, 450e-9)
Z = 2e-3
LEAVES = {"threshold": {"threshold": 0.5}, "phase": {"field": "phase"}}


def _stats(v):
    return f"{statistics.median(v):9.3f} [{min(v):.3f}, {max(v):.3f}]"


def _overlap(a, b):
    return min(a) <= max(b) and min(b) <= max(a)


def _clear_plans(tt):
    for p in list(tt._PLANS.values()):         # the next case starts from an empty plan cache
        p.close()
    tt._PLANS.clear()


def _inputs(n, groups, planes, n_env, leaf):
    import torch
    gen = torch.Generator(device="cuda").manual_seed(n + len(leaf))
    x = torch.rand((n_env, groups * planes, n, n), generator=gen, device="cuda") * 2.0 - 1.0
    target = torch.rand((n_env, groups, n, n), generator=gen, device="cuda")
    v = torch.rand((n_env, groups, n, n), generator=gen, device="cuda")
    v[torch.rand((n_env, groups, n, n), generator=gen, device="cuda") < 0.25] = 0.0
    return x, target, v


def routes_ab(n: int, groups: int, planes: int, n_env: int, leaf: str, blocks: int, calls: int, warmup: int, emit):
    import torch

    import torchOptics.optics as tt

    wls = WL_RGB if groups == 3 else (515e-9,)
    x, target, v = _inputs(n, groups, planes, n_env, leaf)
    x.requires_grad_()
    meta = {"dx": (DX, DX), "wl": wls if groups > 1 else wls[0]}
    kw = LEAVES[leaf]

    def weighted():
        x.grad = None
        tt.loss(tt.Tensor(x, meta=meta), target, Z, pixel_weight=v, **kw).sum().backward()
        return x.grad

    def by_torch():
        x.grad = None
        i = tt.intensity(tt.Tensor(x, meta=meta), Z, **kw).as_subclass(torch.Tensor)
        vi = v * i
        s = (vi * target).sum((1, 2, 3)) / (vi * i).sum((1, 2, 3))
        d = s[:, None, None, None] * i - target
        ((v * d * d).sum((1, 2, 3)) / v.sum((1, 2, 3))).sum().backward()
        return x.grad

    def plain():
        x.grad = None
        tt.loss(tt.Tensor(x, meta=meta), target, Z, **kw).sum().backward()
        return x.grad

    routes = {"weighted": weighted, "torch": by_torch, "plain": plain}
    for _ in range(warmup):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    a, b = weighted().clone(), by_torch().clone()
    agree = float((a - b).abs().max() / b.abs().max())
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
        for name, fn in routes.items():        # alternated: weighted block, torch block, plain block, ...
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(calls):
                fn()
            stop.record()
            stop.synchronize()
            per_block[name].append(start.elapsed_time(stop))

    emit(f"(a) N = {n}, G = {groups}, P = {planes}, B = {n_env}, {leaf} leaf: forward + backward, {blocks} alternated "
         f"blocks x {calls} calls per route; weighted vs torch route: max |grad difference| / max |grad| = {agree:.2e}")
    emit("    device ms per block: median [min, max]; ms per call; route / weighted; torch peak MiB above the inputs")
    med = {k: statistics.median(v_) for k, v_ in per_block.items()}
    for name in routes:
        t = per_block[name]
        note = "" if name == "weighted" else ("  (ranges overlap)" if _overlap(t, per_block["weighted"]) else "  (ranges apart)")
        emit(f"    {name:9s} {_stats(t)}   {med[name] / calls:8.4f}   {med[name] / med['weighted']:5.3f}x   "
             f"{peak[name]:9.1f}{note}")
    emit(f"    the feature's cost, weighted / plain = {med['weighted'] / med['plain']:.3f}; one image set [B, G, N, N] is "
         f"{4.0 * n_env * groups * n * n / 2 ** 20:.1f} MiB")
    _clear_plans(tt)


def passes_ab(n: int, groups: int, planes: int, n_env: int, leaf: str, outputs: bool, blocks: int, calls: int,
              warmup: int, emit):
    import torch

    import hbx
    from hbx import _lib

    wls = WL_RGB if groups == 3 else (515e-9,)
    jobs = n_env * groups
    real_in = leaf == "threshold"
    plan = hbx.Plan(hbx.OpticsConfig(n, n, groups, planes if real_in else 2 * planes, wls, DX, DX, Z), max_jobs=jobs)
    x, target, v = _inputs(n, groups, planes, n_env, leaf)
    if real_in:
        routes = {"weighted": lambda: plan.evaluate_pw(x, _lib.LEAF_THRESHOLD, target, v, outputs, outputs, threshold=0.5),
                  "sibling": lambda: plan.evaluate_threshold(x, 0.5, target, outputs, outputs)}
    else:
        routes = {"weighted": lambda: plan.evaluate_pw(x, _lib.LEAF_PHASE, target, v, outputs, outputs),
                  "sibling": lambda: plan.evaluate_phase(x, target, outputs, outputs)}
    for _ in range(warmup):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    plan.set_timing(calls)
    slots = {k: [] for k in routes}
    for _ in range(blocks):
        for name, fn in routes.items():
            for _ in range(calls):
                fn()
            ms, launches, jb = plan.read_timing()["k_rowinv"]     # waits for the block and clears the timer
            assert launches == calls and jb == calls * jobs, (launches, jb)
            slots[name].append(ms / launches)
    plan.set_timing(0)
    plan.close()
    emit(f"(b) N = {n}, G = {groups}, P = {planes}, B = {n_env}, {leaf} leaf, field and intensity "
         f"{'written' if outputs else 'not written'}: pass timer (k_rowinv slot), {blocks} alternated blocks x {calls} "
         f"launches; ms per launch: median [min, max]")
    med = {k: statistics.median(t) for k, t in slots.items()}
    for name in routes:
        t = slots[name]
        emit(f"    {name:9s} {med[name]:8.4f} [{min(t):.4f}, {max(t):.4f}]")
    emit(f"    weighted / sibling = {med['weighted'] / med['sibling']:.3f}; the blocks' ranges "
         f"{'overlap' if _overlap(slots['weighted'], slots['sibling']) else 'are APART'}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--blocks", type=int, default=5, help="alternated timing blocks per route")
    ap.add_argument("--calls", type=int, default=4, help="calls per block")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="ab", help="sections to run, e.g. b")
    ap.add_argument("--sizes", default="1024,256", help="the N to time")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("pixel_weight_time.py needs a GPU")
    from hbx import _lib
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"device: {torch.cuda.get_device_name(0)}; library: {os.path.basename(_lib.LIB_PATH)}")
    shapes = [sh for sh in ((1024, 3, 8, 4), (256, 1, 8, 64)) if str(sh[0]) in a.sizes.split(",")]
    if "a" in a.only:
        for shape in shapes:
            for leaf in LEAVES:
                routes_ab(*shape, leaf, a.blocks, a.calls, a.warmup, emit)
    if "b" in a.only:
        for shape in shapes:
            for leaf, outputs in (("threshold", True), ("threshold", False), ("phase", True)):
                passes_ab(*shape, leaf, outputs, a.blocks, a.calls, a.warmup, emit)
    emit("N = 896 and N = 64 are not timed.")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
