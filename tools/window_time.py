#!/usr/bin/env python3
"""Windows (grid= / origin= / roi= of tt.loss; hbx_evaluate_threshold_window, hbx_loss_weight_window,
hbx_backward_window) against the route they replace, and the windowed first and last pass against
the full-grid passes of the same plan.  tools/threshold_ste_time.py's method: blocks of the routes
alternated on one box after a warm-up of both, block medians and ranges.

(a) Forward plus backward of the loss of a binary hologram (threshold 0.5, the default gate):

      fused   tt.loss(x, target, z, threshold=0.5, grid=N, origin=.., roi=..).sum().backward()
      parent  p = F.pad(x, ..)                                   # the N x N copy of the leaf
              I = tt.intensity(p, z, threshold=0.5)[roi]         # full-grid call, slice
              relativeLoss(I, target, F.mse_loss) per env, as batched torch ops in float64; .backward()
              (the slice's and the pad's backward write the gradient of pixels that do not exist)

    at  1024 x 768 in the 1024 grid, the loss over the hologram's own rectangle (G = 3, P = 8, B = 4),
        1024 x 1024 with the loss over the central 896 x 896 (a 64-pixel margin: the reference's crop
        before it compares, env_1024_24_128.py:144-149; G = 3, P = 8, B = 4),
        192 x 192 in the 256 grid, the loss over its own rectangle (mono, P = 8, B = 64).
    Printed: device ms per block of `calls` pairs (median and range over the blocks), ms per call,
    parent / route, torch.cuda.max_memory_allocated over one pair above what is allocated before it,
    and the largest difference of the two gradients as a fraction of max|grad|.

(b) The plan's pass timer on the forward plan, blocks alternated: hbx_evaluate_threshold on the padded
    leaf and the full-grid target against hbx_evaluate_threshold_window on the compact ones, field and
    intensity written by both (the forward of a step that wants a gradient); first pass (k_rowfwd slot)
    and last pass (k_rowinv slot), ms per launch.

The library is the one hbx._lib loads (HBX_LIB selects another build).  Needs a GPU; writes what it
prints to --out as well.

    python tools/window_time.py --out profiles/window/window_time.txt
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

Z = 2e-3
DX = 7.56e-6
WL_RGB = (638e-9, 515e-9, 450e-9)
TAU = 0.5

# label: (N, G, P, B, hologram (h, w), roi | None = the hologram's centred rectangle)
SHAPES = {
    "1024x768 in 1024": (1024, 3, 8, 4, (768, 1024), None),
    "1024, loss over the central 896": (1024, 3, 8, 4, (1024, 1024), (64, 64, 896, 896)),
    "192 in 256": (256, 1, 8, 64, (192, 192), None),
}


def _stats(v):
    return f"{statistics.median(v):9.3f} [{min(v):.3f}, {max(v):.3f}]"


def _windows(n, hw, roi):
    h, w = hw
    in_win = ((n - h) // 2, (n - w) // 2, h, w)
    return in_win, (roi if roi is not None else in_win)


def routes_ab(label, blocks: int, calls: int, warmup: int, emit):
    import torch
    import torch.nn.functional as F

    import torchOptics.optics as tt

    n, groups, planes, n_env, hw, roi = SHAPES[label]
    (y0, x0, h, w), (ry, rx, rh, rw) = _windows(n, hw, roi)
    wls = WL_RGB if groups == 3 else (515e-9,)
    gen = torch.Generator(device="cuda").manual_seed(n + h)
    x = (torch.rand((n_env, groups * planes, h, w), generator=gen, device="cuda") * 2.0 - 0.5).requires_grad_()
    target = torch.rand((n_env, groups, rh, rw), generator=gen, device="cuda")
    target64 = target.double()
    meta = {"dx": (DX, DX), "wl": wls if groups > 1 else wls[0]}

    def parent():
        x.grad = None
        p = F.pad(x, (x0, n - x0 - w, y0, n - y0 - h))
        inten = tt.intensity(tt.Tensor(p, meta=meta), Z, threshold=TAU)[:, :, ry:ry + rh, rx:rx + rw].double()
        s = (inten * target64).sum((1, 2, 3)) / (inten * inten).sum((1, 2, 3))
        ((s[:, None, None, None] * inten - target64) ** 2).mean((1, 2, 3)).sum().backward()
        return x.grad

    def fused():
        x.grad = None
        tt.loss(tt.Tensor(x, meta=meta), target, Z, threshold=TAU, grid=n, origin=(y0, x0),
                roi=(ry, rx, rh, rw)).sum().backward()
        return x.grad

    routes = {"fused": fused, "parent": parent}
    for _ in range(warmup):
        for fn in routes.values():
            fn()
    gf, gp = fused().clone(), parent().clone()
    diff = float((gf - gp).abs().max() / gp.abs().max())
    torch.cuda.synchronize()
    del gf, gp
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
        for name, fn in routes.items():        # alternated: fused block, parent block, ...
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(calls):
                fn()
            stop.record()
            stop.synchronize()
            per_block[name].append(start.elapsed_time(stop))
    emit(f"(a) {label}: N = {n}, G = {groups}, P = {planes}, B = {n_env}, hologram {h} x {w} at ({y0}, {x0}), roi "
         f"({ry}, {rx}, {rh}, {rw}): forward + backward, {blocks} alternated blocks x {calls} calls per route")
    emit("    device ms per block: median [min, max]; ms per call; parent / route; peak MiB above the inputs")
    med = {k: statistics.median(v) for k, v in per_block.items()}
    for name in routes:
        v = per_block[name]
        emit(f"    {name:7s} {_stats(v)}   {med[name] / calls:8.4f}   {med['parent'] / med[name]:5.2f}x   {peak[name]:9.1f}")
    slower = min(per_block["fused"]) > max(per_block["parent"])
    apart = max(per_block["fused"]) < min(per_block["parent"])
    emit(f"    largest gradient difference {diff:.3e} of max|grad|; fused slower beyond the blocks' spread: "
         f"{'YES' if slower else 'no'}; faster with the ranges apart: {'yes' if apart else 'no'}; fused peak lower: "
         f"{'yes' if peak['fused'] < peak['parent'] else 'NO'}")
    for p in list(tt._PLANS.values()):         # the next case starts from an empty plan cache
        p.close()
    tt._PLANS.clear()


def passes_ab(label, blocks: int, calls: int, warmup: int, emit):
    import torch
    import torch.nn.functional as F

    import hbx

    n, groups, planes, n_env, hw, roi = SHAPES[label]
    in_win, out_win = _windows(n, hw, roi)
    (y0, x0, h, w), (ry, rx, rh, rw) = in_win, out_win
    wls = WL_RGB if groups == 3 else (515e-9,)
    jobs = n_env * groups
    gen = torch.Generator(device="cuda").manual_seed(n + h + 2)
    x = torch.rand((n_env, groups * planes, h, w), generator=gen, device="cuda") * 2.0 - 0.5
    target = torch.rand((n_env, groups, rh, rw), generator=gen, device="cuda")
    # the full-grid call's inputs: the padding is below the threshold (bit off), the target zero outside the roi
    xp = F.pad(x, (x0, n - x0 - w, y0, n - y0 - h), value=-1.0).contiguous()
    tp = F.pad(target, (rx, n - rx - rw, ry, n - ry - rh)).contiguous()
    plan = hbx.Plan(hbx.OpticsConfig(n, n, groups, planes, wls, DX, DX, Z), max_jobs=jobs)
    routes = {"full grid": lambda: plan.evaluate_threshold(xp, TAU, tp),
              "windows": lambda: plan.evaluate_threshold_window(x, TAU, in_win, target, out_win)}
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
    emit(f"(b) {label}: {jobs} jobs, pass timer, {blocks} alternated blocks x {calls} launches; ms per launch: "
         "median [min, max]")
    med = {}
    for slot, what in (("k_rowfwd", "first pass"), ("k_rowinv", "last pass")):
        for name in routes:
            v = slots[name][slot]
            med[name] = statistics.median(v)
            emit(f"    {what + ', ' + name:24s} {med[name]:8.4f} [{min(v):.4f}, {max(v):.4f}]")
        slower = min(slots["windows"][slot]) > max(slots["full grid"][slot])
        emit(f"    {what}: windows / full grid = {med['windows'] / med['full grid']:.3f}"
             f"{' -- SLOWER beyond the spread of the blocks' if slower else ''}")


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
        sys.exit("window_time.py needs a GPU")
    from hbx import _lib
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"device: {torch.cuda.get_device_name(0)}; library: {os.path.basename(_lib.LIB_PATH)}")
    for label in SHAPES:
        if "a" in a.only:
            routes_ab(label, a.blocks, a.calls, a.warmup, emit)
        if "b" in a.only:
            passes_ab(label, a.blocks, a.calls, a.warmup, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
