#!/usr/bin/env python3
"""Binary holograms with the straight-through estimator: the fused route (hbx_evaluate_threshold /
hbx_threshold_backward) against the same optimisation step built from torch ops around tt.loss, the
thresholding first pass and the gated last pass against the forms they derive from, and the accuracy
of the sigmoid surrogate.

(a) Forward plus backward of tt.loss on one box, blocks of the two routes alternated after a warm-up
    of both:

      torch   m = torch.where(x >= tau, hi, lo).requires_grad_()       # the 0 / 1 copy of the hologram
              tt.loss(m, target, z).sum().backward()                   # the real part of the adjoint
              grad = torch.where((x >= lo_w) & (x <= hi_w), vb * m.grad, 0)
      fused   tt.loss(x, target, z, threshold=tau).sum().backward()

    at 1024 x 1024, G = 3, P = 8 planes per group, B = 4 and at 256 x 256, mono, P = 8, B = 64, for
    --field amplitude (the default) or phase.  Printed: device ms per block of `calls`
    forward-backward pairs (events around the block; median and range over the blocks), torch /
    route, and torch.cuda.max_memory_allocated over one pair of each route above what is allocated
    before it.  Both gradients are compared once (they are equal bit for bit).

(b) The plan's pass timer, blocks alternated.  First pass (k_rowfwd slot) on the forward plan:
    hbx_evaluate_real on the materialised samples against hbx_evaluate_threshold.  Last pass (k_rowinv
    slot) on the plan for -z (2 P real planes per group): hbx_simulate_complex writing the real part,
    hbx_phase_backward, and hbx_threshold_backward with the window and with the sigmoid.  Bytes per
    plane: the first pass reads 4 N^2 and writes 4 N^2 of half row spectra either way; the last pass
    reads two B planes (16 N^2) per complex plane and writes 4 N^2 (real part), or reads 4 N^2 more
    and writes 4 N^2 (the gradients).  Given as ms and as a fraction of 8 TB/s.

(c) The sigmoid form of hbx_threshold_backward at the four sizes against vb s(x) Re g in float64 from
    the real part hbx_simulate_complex writes, as a fraction of (k / 4) max|Re g|.

The library is the one hbx._lib loads (HBX_LIB selects another build).  Needs a GPU; writes what it
prints to --out as well.

    python tools/threshold_ste_time.py --out profiles/binary_ste/threshold_ste_time.txt
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
TAU = 0.5
LO_W, HI_W = 0.0, 1.0           # the default window, tau -+ 0.5


def _stats(v):
    return f"{statistics.median(v):9.3f} [{min(v):.3f}, {max(v):.3f}]"


def routes_ab(n: int, groups: int, planes: int, n_env: int, field: str, blocks: int, calls: int, warmup: int, emit):
    import torch

    import torchOptics.optics as tt

    wls = WL_RGB if groups == 3 else (515e-9,)
    lo, vb = (0.0, 1.0) if field == "amplitude" else (1.0, -2.0)
    gen = torch.Generator(device="cuda").manual_seed(n)
    x = (torch.rand((n_env, groups * planes, n, n), generator=gen, device="cuda") * 2.0 - 0.5).requires_grad_()
    target = torch.rand((n_env, groups, n, n), generator=gen, device="cuda")
    meta = {"dx": (DX, DX), "wl": wls if groups > 1 else wls[0]}

    def torch_ops():
        xd = x.detach()
        m = torch.where(xd >= TAU, lo + vb, lo).requires_grad_()
        tt.loss(tt.Tensor(m, meta=meta), target, Z).sum().backward()
        return torch.where((xd >= LO_W) & (xd <= HI_W), vb * m.grad, 0.0)

    def fused():
        x.grad = None
        tt.loss(tt.Tensor(x, meta=meta), target, Z, field=field, threshold=TAU).sum().backward()
        return x.grad

    routes = {"fused": fused, "torch": torch_ops}
    for _ in range(warmup):
        for fn in routes.values():
            fn()
    same = torch.equal(fused(), torch_ops())
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

    emit(f"(a) N = {n}, G = {groups}, P = {planes}, B = {n_env}, binary {field} leaf: forward + backward of tt.loss, "
         f"{blocks} alternated blocks x {calls} calls per route")
    emit("    device ms per block: median [min, max]; ms per call; torch / route; peak MiB above the inputs")
    med = {k: statistics.median(v) for k, v in per_block.items()}
    for name in routes:
        v = per_block[name]
        emit(f"    {name:7s} {_stats(v)}   {med[name] / calls:8.4f}   {med['torch'] / med[name]:5.2f}x   {peak[name]:9.1f}")
    slower = min(per_block["fused"]) > max(per_block["torch"])
    apart = max(per_block["fused"]) < min(per_block["torch"])
    emit(f"    gradients equal bit for bit: {'yes' if same else 'NO'}; fused slower beyond the blocks' spread: "
         f"{'YES' if slower else 'no'}; faster with the ranges apart: {'yes' if apart else 'no'}; fused peak lower: "
         f"{'yes' if peak['fused'] < peak['torch'] else 'NO'}")
    for p in list(tt._PLANS.values()):         # the next case starts from an empty plan cache
        p.close()
    tt._PLANS.clear()


def passes_ab(n: int, groups: int, planes: int, n_env: int, blocks: int, calls: int, warmup: int, emit):
    """planes: the leaf's real planes per group = complex planes per group of the plan for -z"""
    import torch

    import hbx
    from hbx import _lib

    wls = WL_RGB if groups == 3 else (515e-9,)
    jobs = n_env * groups
    ch = groups * planes
    gen = torch.Generator(device="cuda").manual_seed(n + 2)
    x = torch.rand((n_env, ch, n, n), generator=gen, device="cuda") * 2.0 - 0.5
    mat = torch.where(x >= TAU, 1.0, 0.0)
    target = torch.rand((n_env, groups, n, n), generator=gen, device="cuda")
    vals = torch.view_as_complex(torch.rand((n_env, ch, n, n, 2), generator=gen, device="cuda") * 2.0 - 1.0)
    px = float(n_env) * ch * n * n

    def run(plan, routes):
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
        return slots

    emit(f"(b) N = {n}, G = {groups}: {jobs} jobs, {n_env * ch} leaf planes, pass timer, {blocks} alternated "
         f"blocks x {calls} launches; ms per launch: median [min, max]")
    med = {}

    def row(label, v, nbytes):
        med[label] = statistics.median(v)
        emit(f"    {label:32s} {med[label]:8.4f} [{min(v):.4f}, {max(v):.4f}]   {nbytes / 1e6:8.1f} MB  -> "
             f"{nbytes / (med[label] * 1e-3) / PEAK_BPS:.3f} of 8 TB/s")

    fwd = hbx.Plan(hbx.OpticsConfig(n, n, groups, planes, wls, DX, DX, Z), max_jobs=jobs)
    s = run(fwd, {"real": lambda: fwd.evaluate_real(mat, target, want_field=False, want_intensity=False),
                  "threshold": lambda: fwd.evaluate_threshold(x, TAU, target, want_field=False, want_intensity=False)})
    row("first pass, real load", s["real"]["k_rowfwd"], 8.0 * px)
    row("first pass, threshold load", s["threshold"]["k_rowfwd"], 8.0 * px)
    adj = hbx.Plan(hbx.OpticsConfig(n, n, groups, 2 * planes, wls, DX, DX, -Z), max_jobs=jobs)
    s = run(adj, {"real": lambda: adj.simulate_complex(vals, want_field=False, want_real=True),
                  "phase": lambda: adj.phase_backward(vals, x),
                  "window": lambda: adj.threshold_backward(vals, x, surrogate=_lib.STE_WINDOW, p0=LO_W, p1=HI_W),
                  "sigmoid": lambda: adj.threshold_backward(vals, x, surrogate=_lib.STE_SIGMOID, p0=TAU, p1=2.0)})
    row("last pass, real part", s["real"]["k_rowinv"], 20.0 * px)
    row("last pass, phase gradient", s["phase"]["k_rowinv"], 24.0 * px)
    row("last pass, window gradient", s["window"]["k_rowinv"], 24.0 * px)
    row("last pass, sigmoid gradient", s["sigmoid"]["k_rowinv"], 24.0 * px)
    emit(f"    threshold / real first pass = {med['first pass, threshold load'] / med['first pass, real load']:.3f}; "
         f"window / real part = {med['last pass, window gradient'] / med['last pass, real part']:.3f}, window / phase "
         f"gradient = {med['last pass, window gradient'] / med['last pass, phase gradient']:.3f}, sigmoid / phase "
         f"gradient = {med['last pass, sigmoid gradient'] / med['last pass, phase gradient']:.3f}")


def accuracy(emit):
    import numpy as np
    import torch

    import hbx
    from hbx import _lib

    k = 4.0
    emit(f"(c) hbx_threshold_backward, HBX_STE_SIGMOID, tau = {TAU}, k = {k}, samples uniform in [-0.5, 1.5], one "
         "complex plane, binary phase (vb = -2): error against vb s(x) Re g in float64, of (k / 4) max|Re g|")
    worst = 0.0
    for n in (64, 256, 896, 1024):
        plan = hbx.Plan(hbx.OpticsConfig(n, n, 1, 2, (515e-9,), DX, DX, -Z, _lib.TF_ASM, _lib.FIELD_PHASE), max_jobs=1)
        rng = np.random.default_rng(5 + n)
        x = (2.0 * rng.random((1, 1, n, n), dtype=np.float32) - 0.5).astype(np.float32)
        v = ((2 * rng.random((1, 1, n, n)) - 1) + 1j * (2 * rng.random((1, 1, n, n)) - 1)).astype(np.complex64)
        vals, xs = torch.from_numpy(v).cuda(), torch.from_numpy(x).cuda()
        grad = plan.threshold_backward(vals, xs, surrogate=_lib.STE_SIGMOID, p0=TAU, p1=k)
        _, real = plan.simulate_complex(vals, want_field=False, want_real=True)
        torch.cuda.synchronize()
        r, x64 = real.cpu().numpy().astype(np.float64), x.astype(np.float64)
        e = np.exp(-np.abs(k * (x64 - TAU)))
        want = -2.0 * (k * e / ((1.0 + e) * (1.0 + e))) * r
        err = np.max(np.abs(grad.cpu().numpy() - want)) / (k / 4 * np.max(np.abs(r)))
        worst = max(worst, err)
        emit(f"    N = {n:4d}: {err:.3e}")
        plan.close()
    emit(f"    worst {worst:.3e}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--blocks", type=int, default=5, help="alternated timing blocks per route")
    ap.add_argument("--calls", type=int, default=8, help="calls per block")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--field", default="amplitude", choices=("amplitude", "phase"), help="section (a)'s field kind")
    ap.add_argument("--only", default="abc", help="sections to run, e.g. bc")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("threshold_ste_time.py needs a GPU")
    from hbx import _lib
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"device: {torch.cuda.get_device_name(0)}; library: {os.path.basename(_lib.LIB_PATH)}")
    shapes = ((1024, 3, 8, 4), (256, 1, 8, 64))
    if "a" in a.only:
        for shape in shapes:
            routes_ab(*shape, a.field, a.blocks, a.calls, a.warmup, emit)
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
