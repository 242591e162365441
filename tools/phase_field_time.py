#!/usr/bin/env python3
"""Phase holograms: the fused route (hbx_evaluate_phase / hbx_phase_backward) against the parent route
(u = exp(i pi x) formed with torch ops and handed over as a complex leaf), the phase-loading first pass
and the phase-gradient last pass against their complex forms, and the accuracy of the sincos in use.

(a) Forward plus backward of tt.loss on one box, blocks of the two routes alternated after a warm-up
    of both:

      parent  tt.loss(torch.complex(cos(x * float32(pi)), sin(..)), target, z).sum().backward()
      fused   tt.loss(x, target, z, field="phase").sum().backward()

    at 1024 x 1024, G = 3, P = 8 phase planes per group, B = 4 and at 256 x 256, mono, P = 8, B = 64.
    Printed: device ms per block of `calls` forward-backward pairs (events around the block; median
    and range over the blocks), parent / route, and torch.cuda.max_memory_allocated over one pair of
    each route above what is allocated before it.

(b) The plan's pass timer, blocks alternated, on the plan those shapes use (2 P real planes per group):
    first pass (k_rowfwd slot) of hbx_simulate_complex against hbx_simulate_phase, last pass (k_rowinv
    slot) of hbx_simulate_complex (field only) against hbx_phase_backward (gradient only).  Bytes per
    complex plane: the first pass writes the two half row spectra (8 N^2) and reads 8 N^2 (complex) or
    4 N^2 (phase); the last pass reads two B planes (16 N^2) and writes 8 N^2 (field), or reads
    4 N^2 more and writes 4 N^2 (gradient).  Given as ms and as a fraction of 8 TB/s.

(c) Accuracy at 256 x 256, two phase planes, against the float64 oracle: the field of
    hbx_simulate_phase for samples in [-1, 1) and in [-4096, 4096), as a fraction of max|field|, and
    hbx_phase_backward against pi (Im g cos pi x - Re g sin pi x) in float64 from the g that
    hbx_simulate_complex writes, as a fraction of pi max|g|.

The library is the one hbx._lib loads (HBX_LIB selects another build, e.g. one made with `make exp`).
Needs a GPU; writes what it prints to --out as well.

    python tools/phase_field_time.py --out profiles/phase_field/phase_field_time.txt
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
    import numpy as np
    import torch

    import torchOptics.optics as tt

    wls = WL_RGB if groups == 3 else (515e-9,)
    gen = torch.Generator(device="cuda").manual_seed(n)
    x = (torch.rand((n_env, groups * planes, n, n), generator=gen, device="cuda") * 2.0 - 1.0).requires_grad_()
    target = torch.rand((n_env, groups, n, n), generator=gen, device="cuda")
    meta = {"dx": (DX, DX), "wl": wls if groups > 1 else wls[0]}

    def parent():
        x.grad = None
        ph = x * np.float32(np.pi)
        u = torch.complex(torch.cos(ph), torch.sin(ph))
        tt.loss(tt.Tensor(u, meta=meta), target, Z).sum().backward()
        return x.grad

    def fused():
        x.grad = None
        tt.loss(tt.Tensor(x, meta=meta), target, Z, field="phase").sum().backward()
        return x.grad

    routes = {"fused": fused, "parent": parent}
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
        for name, fn in routes.items():        # alternated: fused block, parent block, ...
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(calls):
                fn()
            stop.record()
            stop.synchronize()
            per_block[name].append(start.elapsed_time(stop))

    emit(f"(a) N = {n}, G = {groups}, P = {planes}, B = {n_env}, phase leaf: forward + backward of tt.loss, "
         f"{blocks} alternated blocks x {calls} calls per route")
    emit("    device ms per block: median [min, max]; ms per call; parent / route; peak MiB above the inputs")
    med = {k: statistics.median(v) for k, v in per_block.items()}
    for name in routes:
        v = per_block[name]
        emit(f"    {name:7s} {_stats(v)}   {med[name] / calls:8.4f}   {med['parent'] / med[name]:5.2f}x   {peak[name]:9.1f}")
    apart = max(per_block["fused"]) < min(per_block["parent"])
    emit(f"    fused faster with the blocks' ranges apart: {'yes' if apart else 'NO'}; fused peak lower: "
         f"{'yes' if peak['fused'] < peak['parent'] else 'NO'}")
    for p in list(tt._PLANS.values()):         # the next case starts from an empty plan cache
        p.close()
    tt._PLANS.clear()


def passes_ab(n: int, groups: int, planes: int, n_env: int, blocks: int, calls: int, warmup: int, emit):
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

    routes = {"complex in, field out": lambda: plan.simulate_complex(vals),
              "phase in, field out": lambda: plan.simulate_phase(x),
              "complex in, gradient out": lambda: plan.phase_backward(vals, x)}
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
    rows = [("first pass, complex load", "complex in, field out", "k_rowfwd", 16.0 * px),
            ("first pass, phase load", "phase in, field out", "k_rowfwd", 12.0 * px),
            ("last pass, field only", "complex in, field out", "k_rowinv", 24.0 * px),
            ("last pass, phase gradient", "complex in, gradient out", "k_rowinv", 24.0 * px)]
    emit(f"(b) N = {n}, G = {groups}: {jobs} jobs = {n_env * cplanes} complex planes, pass timer, {blocks} alternated "
         f"blocks x {calls} launches; ms per launch: median [min, max]")
    med = {}
    for label, route, slot, nbytes in rows:
        v = slots[route][slot]
        med[label] = statistics.median(v)
        emit(f"    {label:26s} {med[label]:8.4f} [{min(v):.4f}, {max(v):.4f}]   {nbytes / 1e6:8.1f} MB  -> "
             f"{nbytes / (med[label] * 1e-3) / PEAK_BPS:.3f} of 8 TB/s")
    emit(f"    phase / complex first pass = {med['first pass, phase load'] / med['first pass, complex load']:.3f}; "
         f"gradient / field last pass = {med['last pass, phase gradient'] / med['last pass, field only']:.3f}")


def accuracy(emit):
    import numpy as np
    import torch

    import hbx
    from oracle import hbx_oracle as O

    n, q = 256, 2
    ocfg = O.OpticsConfig(n, n, 1, 2 * q, O.WL_MONO)
    h = ocfg.transfer(0)
    plan = hbx.Plan(hbx.OpticsConfig(n, n, 1, 2 * q, tuple(ocfg.wavelengths), ocfg.dx, ocfg.dy, ocfg.z), max_jobs=1)
    rng = np.random.default_rng(5)
    emit(f"(c) N = {n}, {q} phase planes: errors against the float64 oracle")
    for span in (1.0, 512.0, 4096.0):
        x = ((2.0 * rng.random((1, q, n, n)) - 1.0) * span).astype(np.float32)
        want = O.propagate(np.exp(1j * np.pi * x[0].astype(np.float64)), h)
        field, _ = plan.simulate_phase(torch.from_numpy(x).cuda())
        torch.cuda.synchronize()
        err = np.max(np.abs(field[0].cpu().numpy() - want)) / np.max(np.abs(want))
        emit(f"    simulate_phase, |x| < {span:6.0f}: field error {err:.3e} of max|field|")
    v = ((2 * rng.random((1, q, n, n)) - 1) + 1j * (2 * rng.random((1, q, n, n)) - 1)).astype(np.complex64)
    vals, xs = torch.from_numpy(v).cuda(), torch.from_numpy(x).cuda()
    grad = plan.phase_backward(vals, xs)
    g, _ = plan.simulate_complex(vals)
    torch.cuda.synchronize()
    g64, x64 = g.cpu().numpy().astype(np.complex128), x.astype(np.float64)
    want = np.pi * (g64.imag * np.cos(np.pi * x64) - g64.real * np.sin(np.pi * x64))
    err = np.max(np.abs(grad.cpu().numpy() - want)) / (np.pi * np.max(np.abs(g64)))
    emit(f"    phase_backward, |x| < 4096: gradient error {err:.3e} of pi max|g|")
    plan.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--blocks", type=int, default=5, help="alternated timing blocks per route")
    ap.add_argument("--calls", type=int, default=8, help="calls per block")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="abc", help="sections to run, e.g. bc")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("phase_field_time.py needs a GPU")
    from hbx import _lib
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"device: {torch.cuda.get_device_name(0)}; library: {os.path.basename(_lib.LIB_PATH)}")
    shapes = ((1024, 3, 8, 4), (256, 1, 8, 64))
    if "a" in a.only:
        for shape in shapes:
            routes_ab(*shape, a.blocks, a.calls, a.warmup, emit)
    if "b" in a.only:
        for shape in shapes:
            passes_ab(*shape, a.blocks, a.calls, a.warmup, emit)
    if "c" in a.only:
        accuracy(emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
