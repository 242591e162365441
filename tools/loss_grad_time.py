#!/usr/bin/env python3
"""The relative MSE loss and its gradient: tt.loss against tt.relativeLoss(tt.intensity(..), ..,
F.mse_loss), the complex last pass with and without its statistics, and the loss-weight pass.

(a) Forward plus backward on one box, blocks of the two routes alternated after a warm-up of both:

      parent  tt.relativeLoss(tt.intensity(x, z), target, F.mse_loss).backward()   (float64 torch ops
              over [B, G, N, N] behind the intensity, and autograd through them)
      new     tt.loss(x, target, z).sum().backward()                                (hbx_evaluate_*,
              hbx_loss, hbx_loss_weight, one weighted launch set)

    for a real leaf and for a phase leaf (field="phase": u = exp(i pi x) with torch ops on both
    routes), at 1024 x 1024, G = 3, P = 8, B = 4 and at 256 x 256, mono, P = 8, B = 64.  The parent
    route takes one least-squares scale for the whole batch, the new one a scale per env: the same
    work, not the same number.  Printed: device ms per block of `calls` forward-backward pairs
    (events around the block; median and range over the blocks), parent / route, and
    torch.cuda.max_memory_allocated over one pair of each route above what is allocated before it.

(b) The complex last pass from the plan's pass timer (k_rowinv slot), blocks alternated:
    hbx_simulate_complex (field only: the statistics switch off), hbx_evaluate_complex with the
    field (switch on: field, intensity, partials) and without it (intensity and partials only).

(c) hbx_loss_weight: events around a block of back-to-back launches into one buffer, so the figure
    includes the gaps between launches -- an upper bound of the kernel's time.  It reads I and T and
    writes the weight, 12 G N^2 bytes per env, given as a fraction of 8 TB/s.

Needs a GPU; writes what it prints to --out as well.

    python tools/loss_grad_time.py --out profiles/loss_grad/loss_grad_time.txt
"""
from __future__ import annotations

import argparse
import ctypes as C
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


def routes_ab(n: int, groups: int, planes: int, n_env: int, leaf: str, blocks: int, calls: int, warmup: int, emit):
    import torch
    import torch.nn.functional as Fn

    import torchOptics.optics as tt

    wls = WL_RGB if groups == 3 else (515e-9,)
    gen = torch.Generator(device="cuda").manual_seed(n)
    x = torch.rand((n_env, groups * planes, n, n), generator=gen, device="cuda").requires_grad_()
    target = torch.rand((n_env, groups, n, n), generator=gen, device="cuda")
    meta = {"dx": (DX, DX), "wl": wls if groups > 1 else wls[0]}
    kw = {"field": "phase"} if leaf == "phase" else {}

    def parent():
        x.grad = None
        tt.relativeLoss(tt.intensity(tt.Tensor(x, meta=meta), Z, **kw), target, Fn.mse_loss).backward()
        return x.grad

    def new():
        x.grad = None
        tt.loss(tt.Tensor(x, meta=meta), target, Z, **kw).sum().backward()
        return x.grad

    routes = {"new": new, "parent": parent}
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
        for name, fn in routes.items():        # alternated: new block, parent block, ...
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(calls):
                fn()
            stop.record()
            stop.synchronize()
            per_block[name].append(start.elapsed_time(stop))

    emit(f"(a) N = {n}, G = {groups}, P = {planes}, B = {n_env}, {leaf} leaf: forward + backward of the relative MSE, "
         f"{blocks} alternated blocks x {calls} calls per route")
    emit("    device ms per block: median [min, max]; ms per call; parent / route; peak MiB above the inputs")
    med = {k: statistics.median(v) for k, v in per_block.items()}
    for name in routes:
        v = per_block[name]
        emit(f"    {name:7s} {_stats(v)}   {med[name] / calls:8.4f}   {med['parent'] / med[name]:5.2f}x   {peak[name]:9.1f}")
    not_slower = med["new"] <= med["parent"]
    apart = max(per_block["new"]) < min(per_block["parent"])
    emit(f"    new not slower than parent: {'yes' if not_slower else 'NO'}; the blocks' ranges apart: "
         f"{'yes' if apart else 'NO'}")
    for p in list(tt._PLANS.values()):         # the next case starts from an empty plan cache
        p.close()
    tt._PLANS.clear()


def last_pass_ab(n: int, groups: int, planes: int, n_env: int, blocks: int, calls: int, warmup: int, emit):
    """planes: real planes per group of the plan = 2 x complex planes per group"""
    import torch

    import hbx

    wls = WL_RGB if groups == 3 else (515e-9,)
    cfg = hbx.OpticsConfig(n, n, groups, planes, wls, DX, DX, Z)
    jobs = n_env * groups
    cplanes = groups * planes // 2
    plan = hbx.Plan(cfg, max_jobs=jobs)
    gen = torch.Generator(device="cuda").manual_seed(n + 2)
    vals = torch.view_as_complex(torch.rand((n_env, cplanes, n, n, 2), generator=gen, device="cuda") * 2.0 - 1.0)
    target = torch.rand((n_env, groups, n, n), generator=gen, device="cuda")

    routes = {"off, field": lambda: plan.simulate_complex(vals),
              "on, field": lambda: plan.evaluate_complex(vals, target),
              "on, no field": lambda: plan.evaluate_complex(vals, target, want_field=False)}
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
            ms, launches, jb = plan.read_timing()["k_rowinv"]   # waits for the block and clears the timer
            assert launches == calls and jb == calls * jobs, (launches, jb)
            per_launch[name].append(ms / launches)
    plan.set_timing(0)
    plan.close()
    px = float(n_env) * n * n
    read = 16.0 * cplanes * px                  # two B planes of 8 bytes per pixel and complex plane
    nbytes = {"off, field": read + 8.0 * cplanes * px,
              "on, field": read + 8.0 * cplanes * px + 8.0 * groups * px,    # + target read, intensity written
              "on, no field": read + 8.0 * groups * px}
    emit(f"(b) N = {n}, G = {groups}: complex last pass (k_rowinv slot) of {jobs} jobs = {n_env * cplanes} complex planes, "
         f"{blocks} alternated blocks x {calls} launches; ms per launch: median [min, max]")
    med = {}
    for name in routes:
        v = per_launch[name]
        med[name] = statistics.median(v)
        frac = nbytes[name] / (med[name] * 1e-3) / PEAK_BPS
        emit(f"    statistics {name:13s} {med[name]:8.4f} [{min(v):.4f}, {max(v):.4f}]   {nbytes[name] / 1e6:8.1f} MB  "
             f"-> {frac:.3f} of 8 TB/s")
    emit(f"    on / off with the field = {med['on, field'] / med['off, field']:.3f}; on without the field / off = "
         f"{med['on, no field'] / med['off, field']:.3f}")


def loss_weight_time(n: int, groups: int, n_env: int, blocks: int, calls: int, warmup: int, emit):
    import torch

    import hbx
    from hbx import _lib

    wls = WL_RGB if groups == 3 else (515e-9,)
    plan = hbx.Plan(hbx.OpticsConfig(n, n, groups, 2, wls, DX, DX, -Z), max_jobs=groups)
    gen = torch.Generator(device="cuda").manual_seed(n + 3)
    inten = torch.rand((n_env, groups, n, n), generator=gen, device="cuda")
    target = torch.rand((n_env, groups, n, n), generator=gen, device="cuda")
    stats = torch.stack([(inten * target).sum((2, 3)), (inten * inten).sum((2, 3)), (target * target).sum((2, 3))],
                        dim=2).double().contiguous()
    gl = torch.ones(n_env, dtype=torch.float64, device="cuda")
    weight = torch.empty_like(inten)
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = [C.c_void_p(t.data_ptr()) for t in (inten, target, stats, gl)]

    def launch():
        rc = lib.hbx_loss_weight(plan._h, *args, n_env, _lib.LOSS_MSE, _lib.REL_LSQ, C.c_void_p(weight.data_ptr()), st)
        if rc != _lib.OK:
            _lib.check(rc, "hbx_loss_weight")

    for _ in range(warmup):
        launch()
    torch.cuda.synchronize()
    per_launch = []
    for _ in range(blocks):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(calls):
            launch()
        stop.record()
        stop.synchronize()
        per_launch.append(start.elapsed_time(stop) / calls)
    plan.close()
    nbytes = 12.0 * groups * n * n * n_env
    med = statistics.median(per_launch)
    emit(f"(c) N = {n}, G = {groups}, B = {n_env}: hbx_loss_weight, {blocks} blocks x {calls} back-to-back launches "
         f"(gaps included); ms per launch: median [min, max]")
    emit(f"    {med:8.4f} [{min(per_launch):.4f}, {max(per_launch):.4f}]   {nbytes / 1e6:8.1f} MB  -> "
         f"{nbytes / (med * 1e-3) / PEAK_BPS:.3f} of 8 TB/s")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--blocks", type=int, default=5, help="alternated timing blocks per route")
    ap.add_argument("--calls", type=int, default=8, help="calls per block")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("loss_grad_time.py needs a GPU")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"device: {torch.cuda.get_device_name(0)}")
    for shape in ((1024, 3, 8, 4), (256, 1, 8, 64)):
        for leaf in ("real", "phase"):
            routes_ab(*shape, leaf, a.blocks, a.calls, a.warmup, emit)
    for shape in ((1024, 3, 8, 4), (256, 1, 8, 64)):
        last_pass_ab(*shape, a.blocks, a.calls, a.warmup, emit)
    for shape in ((1024, 3, 4), (256, 1, 64)):
        loss_weight_time(*shape, a.blocks, 25 * a.calls, a.warmup, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
