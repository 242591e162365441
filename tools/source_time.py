#!/usr/bin/env python3
"""Illumination fields: the fused route (hbx_evaluate_source / hbx_backward_source, source= on tt.loss) against
the torch-op route (form s f(x) with torch ops and hand tt.loss a complex leaf), and the sourced first and last
passes against their unsourced siblings.

(a) Forward plus backward of tt.loss on one box, blocks of the two routes alternated after a warm-up of both,
    for a phase leaf and for a thresholded (binary) leaf:

      phase      torch   u = s * torch.exp(1j * pi * x);  tt.loss(u, target, z).sum().backward()
                 fused   tt.loss(x, target, z, field="phase", source=s).sum().backward()
      threshold  torch   m = torch.where(x >= tau, hi, lo).requires_grad_()        # the +-1 copy of the hologram
                         tt.loss(s * m, target, z).sum().backward()
                         grad = torch.where((x >= lo_w) & (x <= hi_w), vb * m.grad, 0)   # the two gate ops
                 fused   tt.loss(x, target, z, field="phase", threshold=tau, source=s).sum().backward()

    at 1024 x 1024, G = 3, P = 8 leaf planes per group, B = 4 and at 256 x 256, mono, P = 8, B = 64.  Printed:
    device ms per block of `calls` forward-backward pairs (events around the block; median and range over the
    blocks), torch / route, whether the two ranges are apart, and torch.cuda.max_memory_allocated over one
    pair of each route above what is allocated before it.

(b) The plan's pass timer, blocks alternated, on the plan those shapes use: each sourced first pass (k_rowfwd
    slot of hbx_evaluate_source) against its unsourced sibling (hbx_evaluate_complex / _phase / _phase_levels on
    the same plane count; the two real kinds against hbx_evaluate_phase's load, which like theirs reads one
    float32 sample and writes one complex plane, 12 bytes per pixel), and each
    sourced last pass (k_rowinv slot of hbx_backward_source) against its sibling (hbx_simulate_complex's field
    and real-part forms, hbx_phase_backward, hbx_phase_levels_backward, hbx_threshold_backward).  Given as ms,
    as a fraction of 8 TB/s on the SIBLING's algorithmic bytes -- the source's bytes, 8 N^2 per group and
    re-read by every env and plane of the group, are not counted -- as the ratio of the medians, and whether
    the two ranges over the blocks overlap.

The library is the one hbx._lib loads (HBX_LIB selects another build).  Needs a GPU; writes what it prints to
--out as well.

    python tools/source_time.py --out profiles/source_field/source_time.txt
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
TAU, LO_W, HI_W = 0.5, 0.25, 0.75
LEVELS = 8


def _stats(v):
    return f"{statistics.median(v):9.3f} [{min(v):.3f}, {max(v):.3f}]"


def _source(n: int, wls):
    """an obliquely incident Gaussian beam per colour group (tt.sources), complex64 [G, N, N] on the GPU"""
    import numpy as np

    import torchOptics.optics as tt
    s = tt.sources.plane_wave((n, n), DX, tuple(wls), angle=(np.deg2rad(1.0), np.deg2rad(-0.5)))
    return (s * tt.sources.gaussian((n, n), DX, 0.3 * n * DX)).reshape(len(wls), n, n).cuda().contiguous()


def routes_ab(n: int, groups: int, planes: int, n_env: int, leaf: str, blocks: int, calls: int, warmup: int, emit):
    import numpy as np
    import torch

    import torchOptics.optics as tt

    wls = WL_RGB if groups == 3 else (515e-9,)
    gen = torch.Generator(device="cuda").manual_seed(n + len(leaf))
    x = torch.rand((n_env, groups * planes, n, n), generator=gen, device="cuda")
    if leaf == "phase":
        x = x * 2.0 - 1.0
    x.requires_grad_()
    target = torch.rand((n_env, groups, n, n), generator=gen, device="cuda")
    meta = {"dx": (DX, DX), "wl": wls if groups > 1 else wls[0]}
    s = _source(n, wls)
    s_planes = s.repeat_interleave(planes, dim=0)          # [G P, N, N]: the torch route's broadcast operand
    lo, vb = 1.0, -2.0                                     # field="phase": u = 1 - 2 [x >= tau]

    if leaf == "phase":
        def by_torch():
            x.grad = None
            u = s_planes * torch.exp(1j * np.pi * x)
            tt.loss(tt.Tensor(u, meta=meta), target, Z).sum().backward()
            return x.grad

        def fused():
            x.grad = None
            tt.loss(tt.Tensor(x, meta=meta), target, Z, field="phase", source=s).sum().backward()
            return x.grad
    else:
        def by_torch():
            xd = x.detach()
            m = torch.where(xd >= TAU, lo + vb, lo).requires_grad_()
            tt.loss(tt.Tensor(s_planes * m, meta=meta), target, Z).sum().backward()
            return torch.where((xd >= LO_W) & (xd <= HI_W), vb * m.grad, 0.0)

        def fused():
            x.grad = None
            tt.loss(tt.Tensor(x, meta=meta), target, Z, field="phase", threshold=TAU, ste="window",
                    ste_width=HI_W - TAU, source=s).sum().backward()
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

    emit(f"(a) N = {n}, G = {groups}, P = {planes}, B = {n_env}, {leaf} leaf: forward + backward of tt.loss under a source, "
         f"{blocks} alternated blocks x {calls} calls per route")
    emit("    device ms per block: median [min, max]; ms per call; torch / route; peak MiB above the inputs")
    med = {k: statistics.median(v) for k, v in per_block.items()}
    for name in routes:
        v = per_block[name]
        emit(f"    {name:7s} {_stats(v)}   {med[name] / calls:8.4f}   {med['torch'] / med[name]:5.2f}x   {peak[name]:9.1f}")
    apart = max(per_block["fused"]) < min(per_block["torch"])
    emit(f"    fused faster with the blocks' ranges apart: {'yes' if apart else 'NO'}; fused peak lower: "
         f"{'yes' if peak['fused'] < peak['torch'] else 'NO'} ({peak['torch'] - peak['fused']:.1f} MiB; one complex64 "
         f"copy of the hologram is {8.0 * x.numel() / 2 ** 20:.1f} MiB)")
    for p in list(tt._PLANS.values()):         # the next case starts from an empty plan cache
        p.close()
    tt._PLANS.clear()


def passes_ab(n: int, groups: int, planes: int, n_env: int, blocks: int, calls: int, warmup: int, emit):
    """planes: leaf planes per group = complex planes per group of the plan (2 x planes real planes)"""
    import torch

    import hbx
    from hbx import _lib

    wls = WL_RGB if groups == 3 else (515e-9,)
    jobs = n_env * groups
    cplanes = groups * planes
    plan = hbx.Plan(hbx.OpticsConfig(n, n, groups, 2 * planes, wls, DX, DX, Z), max_jobs=jobs)
    gen = torch.Generator(device="cuda").manual_seed(n + 3)
    x = torch.rand((n_env, cplanes, n, n), generator=gen, device="cuda") * 2.0 - 1.0
    vals = torch.view_as_complex(torch.rand((n_env, cplanes, n, n, 2), generator=gen, device="cuda") * 2.0 - 1.0)
    s = _source(n, wls)
    L = _lib

    routes = {
        # first passes: the statistics last pass behind each, intensity out, no field
        "complex in": lambda: plan.evaluate_complex(vals, None, want_field=False),
        "phase in": lambda: plan.evaluate_phase(x, None, want_field=False),
        "levels in": lambda: plan.evaluate_phase_levels(x, LEVELS, None, want_field=False),
        "src complex in": lambda: plan.evaluate_source(vals, L.LEAF_COMPLEX, s, want_field=False),
        "src phase in": lambda: plan.evaluate_source(x, L.LEAF_PHASE, s, want_field=False),
        "src levels in": lambda: plan.evaluate_source(x, L.LEAF_PHASE_LEVELS, s, want_field=False, levels=LEVELS),
        "src real in": lambda: plan.evaluate_source(x, L.LEAF_REAL, s, want_field=False),
        "src threshold in": lambda: plan.evaluate_source(x, L.LEAF_THRESHOLD, s, want_field=False, threshold=TAU),
        # last passes
        "field out": lambda: plan.simulate_complex(vals),
        "real out": lambda: plan.simulate_complex(vals, want_field=False, want_real=True),
        "phase out": lambda: plan.phase_backward(vals, x),
        "levels out": lambda: plan.phase_levels_backward(vals, x, LEVELS),
        "window out": lambda: plan.threshold_backward(vals, x, surrogate=L.STE_WINDOW, p0=LO_W, p1=HI_W),
        "sigmoid out": lambda: plan.threshold_backward(vals, x, surrogate=L.STE_SIGMOID, p0=TAU, p1=2.0),
        "src field out": lambda: plan.backward_source(vals, L.LEAF_COMPLEX, s),
        "src real out": lambda: plan.backward_source(vals, L.LEAF_REAL, s),
        "src phase out": lambda: plan.backward_source(vals, L.LEAF_PHASE, s, samples=x),
        "src levels out": lambda: plan.backward_source(vals, L.LEAF_PHASE_LEVELS, s, samples=x, levels=LEVELS),
        "src window out": lambda: plan.backward_source(vals, L.LEAF_THRESHOLD, s, samples=x, surrogate=L.STE_WINDOW,
                                                       p0=LO_W, p1=HI_W),
        "src sigmoid out": lambda: plan.backward_source(vals, L.LEAF_THRESHOLD, s, samples=x, surrogate=L.STE_SIGMOID,
                                                        p0=TAU, p1=2.0),
    }
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
            tm = plan.read_timing()             # waits for the block and clears the timer
            ms, launches, jb = tm["k_rowfwd" if name.endswith(" in") else "k_rowinv"]
            assert launches == calls and jb == calls * jobs, (name, launches, jb)
            slots[name].append(ms / launches)
    plan.set_timing(0)
    plan.close()
    px = float(n_env) * cplanes * n * n
    # (sourced route, sibling, the sibling's algorithmic bytes per pixel and plane)
    pairs = [("src complex in", "complex in", 16.0), ("src phase in", "phase in", 12.0), ("src levels in", "levels in", 12.0),
             ("src real in", "phase in", 12.0), ("src threshold in", "phase in", 12.0),
             ("src field out", "field out", 24.0), ("src real out", "real out", 20.0), ("src phase out", "phase out", 24.0),
             ("src levels out", "levels out", 24.0), ("src window out", "window out", 24.0),
             ("src sigmoid out", "sigmoid out", 24.0)]
    emit(f"(b) N = {n}, G = {groups}: {jobs} jobs = {n_env * cplanes} complex planes, pass timer, {blocks} alternated blocks "
         f"x {calls} launches; ms per launch: median [min, max]; fraction of 8 TB/s on the sibling's bytes")
    for new, old, bpp in pairs:
        nbytes = bpp * px
        a, b = slots[new], slots[old]
        ma, mb = statistics.median(a), statistics.median(b)
        overlap = min(a) <= max(b) and min(b) <= max(a)
        emit(f"    {new:17s} {ma:8.4f} [{min(a):.4f}, {max(a):.4f}] {nbytes / (ma * 1e-3) / PEAK_BPS:.3f}   | "
             f"{old:12s} {mb:8.4f} [{min(b):.4f}, {max(b):.4f}] {nbytes / (mb * 1e-3) / PEAK_BPS:.3f}   | "
             f"ratio {ma / mb:.3f}, ranges {'overlap' if overlap else 'APART'}")


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
        sys.exit("source_time.py needs a GPU")
    from hbx import _lib
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"device: {torch.cuda.get_device_name(0)}; library: {os.path.basename(_lib.LIB_PATH)}")
    shapes = ((1024, 3, 8, 4), (256, 1, 8, 64))
    if "a" in a.only:
        for shape in shapes:
            for leaf in ("phase", "threshold"):
                routes_ab(*shape, leaf, a.blocks, a.calls, a.warmup, emit)
    if "b" in a.only:
        for shape in shapes:
            passes_ab(*shape, a.blocks, a.calls, a.warmup, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
