"""torchOptics.optics -- drop-in for the operator API the reference imports as ``tt``.

The reference calls (env.py:124-132,170-174; env_1024_24.py:149-166;
DBS_1024_24.py:244-257,326-352; range.py:225-309):

    x = tt.Tensor(state_or_numpy, meta={'dx': (7.56e-6, 7.56e-6), 'wl': 515e-9})
    sim = tt.simulate(x, z).abs() ** 2            # complex field of every plane
    psnr = tt.relativeLoss(mean_intensity, target, tm.get_PSNR)
    mse = tt.relativeLoss(mean_intensity, target, F.mse_loss)

``simulate`` runs on the MI355X through libhbx.so, on one of two paths (there is no CPU
fallback on either):

* ``binary=True`` (the default, what the reference does): one hbx_pack_mask launch turns the
  mask into bits (ABI v14), then hbx_simulate's three HIP FFT passes with the transfer function
  fused in.  This path propagates binary {0,1} masks only: a value other than 0 / 1 raises
  ValueError, and a complex input is refused.  The binary check is part of the pack kernel
  and costs no host sync: the kernel flags the value in host-mapped memory, and the shim
  raises at the first point the host has waited for that work -- inside the
  tt.relativeLoss(.., tm.get_PSNR) that consumes the result (it waits for its PSNR anyway,
  env.py:174 / DBS.py:270 compare it at once), at the next tt.simulate, or at check_binary().
  ``simulate(x, z, strict=True)`` waits and raises before returning.
* ``binary=False`` (the continuous path, ABI v15): the samples are the field.  Real float
  input goes through hbx_simulate_real, whose first pass reads float32 samples instead of
  bits; a complex field goes through hbx_simulate_complex, whose first pass reads complex64
  samples and whose last pass writes each complex plane once; ``field="phase"`` on real input
  (u = exp(i pi x)) goes through hbx_simulate_phase, the same with exp(i pi x) formed by the
  first pass as it loads x.  No pack kernel runs, the error word is never set and ``strict``
  has nothing to check.
  This path is differentiable: when the input requires grad the propagation runs as a
  torch.autograd.Function whose backward pass is hbx_simulate_complex of grad_output on the
  plan for -z (the adjoint: H(-z) = conj H(z)); a real input receives the real part only, and
  a phase leaf dL/dx = pi (Im g cos pi x - Re g sin pi x) from the last pass of
  hbx_phase_backward (``intensity`` and ``loss`` likewise): no torch op forms u or walks back
  through it.
  Without a gradient request the call is the plain one, with no graph.  Limits: the -z plan
  is a second workspace in the plan cache; there is no double backward; ``binary=True`` stays
  non-differentiable and builds no graph; ``relativeLoss(.., tm.get_PSNR)`` returns a float
  (its ``F.mse_loss`` form is torch ops and differentiates by itself).
* ``threshold=tau`` on that path (``simulate``, ``intensity`` and ``loss``; real input only): x is
  the leaf of the binary hologram m = [x >= tau], the field is the mask's (amplitude m, phase
  1 - 2 m), thresholded by the first pass of hbx_evaluate_threshold as it loads x, and the
  backward pass is the straight-through estimator: the last pass of hbx_threshold_backward
  writes vb s(x) Re g with the surrogate derivative s chosen by ``ste`` / ``ste_width``.  No
  0 / 1 copy of x is written in either direction.
* ``levels=L`` with ``field="phase"`` on that path (``simulate``, ``intensity`` and ``loss``; real
  input only, 2 <= L <= 256): x is the leaf of the hologram an L-level phase modulator displays.
  The first pass of hbx_simulate_phase_levels / hbx_evaluate_phase_levels rounds each sample to the
  nearest level 2 k / L as it loads it (ties to the even k; hbx.quantize_phase exports the levels),
  and the backward pass is the straight-through estimator dq/dx := 1: the last pass of
  hbx_phase_levels_backward writes the continuous gradient at the displayed phase.  Neither the
  quantized samples nor their field is written; ``levels=None`` is the continuous phase path.

``intensity`` returns the plane-mean intensity mean_p |A u_p|^2 per colour group -- what every loss
of the project is built on -- on the continuous path: several wavelengths in one call, no field
written when no gradient is wanted (hbx_intensity_real), and with a gradient request a backward
pass that is one hbx_simulate_complex_weighted on the plan for -z (the saved field times
(2 / P) grad_output, formed in the first pass's load).

``loss`` is ``relativeLoss(intensity(x, z), target, F.mse_loss)`` -- or its PSNR -- per env in one
launch set: the last pass leaves the float64 sums of I T, I^2 and T^2 (hbx_evaluate_real /
hbx_evaluate_complex), hbx_loss turns them into a float64 device tensor with no host wait, and
the backward pass is hbx_loss_weight (dL/dI = a I + c T per env) followed by the same weighted
launch set on the plan for -z.

``source=`` on simulate(.., binary=False), intensity and loss lights the modulator with a constant
complex illumination s [H, W] or [G, H, W] instead of the unit plane wave on axis, u = s f(x) for every
leaf kind (real, thresholded, complex, phase, L-level phase): the first pass multiplies by the source
row as it loads the leaf (hbx_evaluate_source) and the backward's last pass by conj(s) before the
leaf's gradient formula (hbx_backward_source), so an obliquely lit DMD, a phase SLM under a Gaussian
beam or a lit disc keep the fused loads and the fused gradients.  ``tt.sources`` builds the usual
ones (plane_wave, gaussian, lens).  Out of scope: a source on the binary=True path or with grid= /
the *_stack calls, a gradient with respect to the source, a per-env or per-plane source.

The physics follows the assumptions documented in DESIGN.md (the original torchOptics is
absent and unpinned): no padding; exact angular spectrum and amplitude field unless
``tf="fresnel"`` / ``field="phase"`` select the plan's other switches.  relativeLoss uses the
least-squares scale s = sum(xy)/sum(x^2) unless ``rel_scale="none"``; with tm.get_PSNR on GPU
tensors it is one fixed-order f64 reduction (hbx_rel_stats) whose PSNR is read from
host-mapped memory.
"""
from __future__ import annotations

import numbers

from typing import Callable, Dict, Optional, Tuple

import numpy as np
import torch

import hbx
from hbx import _lib

from . import metrics as _metrics
from . import sources  # noqa: F401  (tt.sources: illumination fields for source=)

__all__ = ["Tensor", "simulate", "intensity", "loss", "relativeLoss", "imread", "check_binary",
           "simulate_stack", "intensity_stack", "loss_stack", "sources"]


class Tensor(torch.Tensor):
    """A torch tensor with an optics ``meta`` dict ({'dx': (dx, dy), 'wl': wl}).

    Integer / numpy inputs (DBS_1024_24.py:326 passes an int8 numpy slice)
    become float32.  Results of torch ops on it are plain torch tensors."""

    @staticmethod
    def __new__(cls, data, meta: Optional[Dict] = None, **_):
        t = data if isinstance(data, torch.Tensor) else torch.as_tensor(np.asarray(data))
        if not (t.is_floating_point() or t.is_complex()):
            t = t.to(torch.float32)
        obj = t.as_subclass(cls)
        obj.meta = dict(meta or (getattr(data, "meta", None) or {}))
        return obj

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        with torch._C.DisableTorchFunctionSubclass():
            return func(*args, **(kwargs or {}))


_PLANS: Dict[Tuple, "hbx.Plan"] = {}


def _meta_of(x) -> Dict:
    meta = getattr(x, "meta", None)
    if not meta:
        raise ValueError("tt.simulate needs a tt.Tensor with meta={'dx': ..., 'wl': ...}")
    return meta


_TF_NAMES = {"asm": _lib.TF_ASM, "fresnel": _lib.TF_FRESNEL}
_FIELD_NAMES = {"amplitude": _lib.FIELD_AMPLITUDE, "phase": _lib.FIELD_PHASE}
_REL_NAMES = {"none": _lib.REL_NONE, "lsq": _lib.REL_LSQ}


def _switch(value, names: Dict[str, int], what: str) -> int:
    """A switch given by name or as its _lib integer -> the integer; anything else raises."""
    if isinstance(value, str):
        if value in names:
            return names[value]
    elif isinstance(value, (int, np.integer)) and not isinstance(value, bool) and int(value) in names.values():
        return int(value)
    raise ValueError(f"{what} must be one of {sorted(names)} (or the hbx._lib constant), got {value!r}")


def _plan_for(h: int, w: int, planes: int, wl, dx: float, dy: float, z: float, n: int, dev: int,
              tf: int = _lib.TF_ASM, field: int = _lib.FIELD_AMPLITUDE, depths: Tuple[float, ...] = (),
              depth_slots: bool = False):
    """The cached plan of `planes` real planes per group; wl: one wavelength, or a tuple of G (one
    colour group each, tt.intensity); n: envs per launch (the plan holds n * G jobs).  depths: the
    focal stack's distances (the *_stack calls; part of the cache key), or () for no stack.
    depth_slots: the plan runs a stack's backward pass, whose chunk of n envs takes n * G * D job
    slots (the forward reuses its workspace from depth to depth and takes n * G)."""
    wls = tuple(float(v) for v in wl) if isinstance(wl, (tuple, list)) else (float(wl),)
    groups = len(wls)
    depths = tuple(float(v) for v in depths)
    key = (h, w, groups, planes, wls, float(dx), float(dy), float(z), dev, tf, field, depths)
    jobs = max(n, 1) * groups * (max(len(depths), 1) if depth_slots else 1)
    p = _PLANS.get(key)
    if p is None or p.max_jobs < jobs:
        cfg = hbx.OpticsConfig(h, w, groups, planes, wls, float(dx), float(dy), float(z),
                               tf, field, _lib.REL_LSQ, 1.0)
        p = hbx.Plan(cfg, max_jobs=jobs, device=dev)
        if depths:
            p.set_depths(depths)
        _PLANS[key] = p
    return p


class _Scratch:
    """Per-device shim scratch: a host-mapped row (the pack kernel's binary-check word at
    byte 0, hbx_rel_stats' five doubles at byte 8) and the reduction's device workspace."""

    def __init__(self, dev: int):
        from hbx.env import HostRow
        self.row = HostRow(_lib.load(), 64)
        self.err = self.row.array[0:4].view(np.int32)
        self.out = self.row.array[8:48].view(np.float64)
        self.err_dev = self.row.device
        self.out_dev = self.row.device + 8
        self.work = torch.empty(_lib.REL_WORKSPACE_DOUBLES, dtype=torch.float64, device=f"cuda:{dev}")


_SCRATCH: Dict[int, _Scratch] = {}


def _scratch(dev: int) -> _Scratch:
    sc = _SCRATCH.get(dev)
    if sc is None:
        sc = _SCRATCH[dev] = _Scratch(dev)
    return sc


def _raise_pending(sc: _Scratch):
    if sc.err[0]:
        sc.err[0] = 0
        raise ValueError("tt.simulate (hbx) propagates binary {0,1} masks only, as the reference does: "
                         "a mask passed to tt.simulate held another value")


def check_binary(device: Optional[int] = None):
    """Wait for the device's queued work and raise ValueError if any tt.simulate input
    since the last check held a value other than 0 / 1."""
    dev = torch.cuda.current_device() if device is None else int(device)
    sc = _SCRATCH.get(dev)
    if sc is not None:
        torch.cuda.synchronize(dev)
        _raise_pending(sc)


_STE_NAMES = {"window": _lib.STE_WINDOW, "sigmoid": _lib.STE_SIGMOID}


def _ste_args(threshold, ste, ste_width, what: str):
    """threshold / ste / ste_width of simulate, intensity and loss -> None without a threshold,
    else (threshold, surrogate, p0, p1) as hbx_threshold_backward takes them, every number a
    float32 value formed here: the window's ends are float32(tau - w) and float32(tau + w)
    (w = inf: the plain straight-through estimator), the sigmoid's slope float32(1 / w)."""
    if threshold is None:
        return None
    kind = _switch(ste, _STE_NAMES, "ste")
    try:
        tau, w = np.float32(threshold), np.float32(ste_width)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: threshold and ste_width are numbers, got {threshold!r}, {ste_width!r}") from None
    if not np.isfinite(tau):
        raise ValueError(f"{what}: threshold must be finite, got {threshold!r}")
    if kind == _lib.STE_WINDOW:
        if not w >= 0:
            raise ValueError(f"{what}: ste_width must be >= 0 (math.inf: no window), got {ste_width!r}")
        return float(tau), kind, float(np.float32(tau - w)), float(np.float32(tau + w))
    if not (w > 0 and np.isfinite(w)):
        raise ValueError(f"{what}: ste=\"sigmoid\" needs a finite ste_width > 0, got {ste_width!r}")
    k = np.float32(1.0) / w
    if not (k > 0 and np.isfinite(k)):
        raise ValueError(f"{what}: 1 / ste_width is not a positive float32, got {ste_width!r}")
    return float(tau), kind, float(tau), float(k)


_GRIDS = (64, 256, 896, 1024)   # the sizes libhbx builds


def _levels_arg(levels, binary: bool, complex_in: bool, field_kind: int, thresholded: bool, grid, what: str):
    """levels= of simulate, intensity and loss -> None, or the level count L of a quantized phase leaf
    as an int, 2 <= L <= 256: a real x with field="phase" on the continuous path, neither thresholded
    (a binary hologram is threshold='s business) nor windowed (phase leaves are not).  Anything else
    raises ValueError before any GPU use."""
    if levels is None:
        return None
    if isinstance(levels, bool) or not isinstance(levels, numbers.Integral):
        raise ValueError(f"{what}: levels is an integer number of phase levels, got {levels!r}")
    if not 2 <= int(levels) <= 256:
        raise ValueError(f"{what}: 2 <= levels <= 256, got {levels}")
    if binary:
        raise ValueError(f"{what}: levels= quantizes a phase leaf on the continuous path (binary=False)")
    if complex_in:
        raise ValueError(f"{what}: levels= needs a real phase leaf, got a complex field")
    if field_kind != _lib.FIELD_PHASE:
        raise ValueError(f"{what}: levels= quantizes a phase, it needs field=\"phase\"")
    if thresholded:
        raise ValueError(f"{what}: levels= and threshold= are two different holograms; give one")
    if grid is not None:
        raise ValueError(f"{what}: levels= with grid= (phase leaves are not windowed)")
    return int(levels)


def _window_args(grid, origin, roi, shape, complex_in: bool, field_kind: int, thresholded: bool, what: str):
    """grid / origin / roi of simulate, intensity and loss -> None without a grid, else (N, the
    hologram's window, the output window), each window (y0, x0, h, w) in grid coordinates.  Every
    error is raised here, before any GPU use."""
    if grid is None:
        if origin is not None or roi is not None:
            raise ValueError(f"{what}: origin= and roi= place a hologram in grid=, which is not given")
        return None
    if isinstance(grid, bool) or not isinstance(grid, (int, np.integer)) or int(grid) not in _GRIDS:
        raise ValueError(f"{what}: grid must be one of {_GRIDS}, got {grid!r}")
    n = int(grid)
    if complex_in:
        raise ValueError(f"{what}: grid= takes a real leaf, got a complex field")
    if field_kind == _lib.FIELD_PHASE and not thresholded:
        raise ValueError(f"{what}: grid= with field=\"phase\" needs threshold= (phase leaves are not windowed)")
    h, w = int(shape[-2]), int(shape[-1])

    def inside(win, name):
        try:
            y0, x0, hh, ww = (int(v) for v in win)
        except (TypeError, ValueError):
            raise ValueError(f"{what}: {name} must be integers, got {win!r}") from None
        if y0 < 0 or x0 < 0 or hh < 1 or ww < 1 or y0 + hh > n or x0 + ww > n:
            raise ValueError(f"{what}: {name} {(y0, x0, hh, ww)} is not a non-empty rectangle of the {n} x {n} grid")
        return y0, x0, hh, ww

    if origin is None:
        if h > n or w > n:
            raise ValueError(f"{what}: a {h} x {w} hologram does not fit the {n} x {n} grid")
        origin = ((n - h) // 2, (n - w) // 2)
    elif not isinstance(origin, (tuple, list)) or len(origin) != 2:
        raise ValueError(f"{what}: origin must be (y0, x0), got {origin!r}")
    in_win = inside((origin[0], origin[1], h, w), "origin + the hologram")
    if roi is None:
        return n, in_win, in_win
    if not isinstance(roi, (tuple, list)) or len(roi) != 4:
        raise ValueError(f"{what}: roi must be (y0, x0, h, w), got {roi!r}")
    return n, in_win, inside(roi, "roi")


def _depths_arg(zs, what: str) -> Tuple[float, ...]:
    """zs of the *_stack calls -> a tuple of 1 to 8 finite floats; anything else raises ValueError."""
    try:
        out = tuple(float(v) for v in zs)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: zs is a sequence of depths (numbers), got {zs!r}") from None
    if not 1 <= len(out) <= _lib.MAX_DEPTHS:
        raise ValueError(f"{what}: 1 to {_lib.MAX_DEPTHS} depths, got {len(out)}")
    if not all(np.isfinite(v) for v in out):
        raise ValueError(f"{what}: every depth must be finite, got {out!r}")
    return out


def _phase_samples(t: torch.Tensor) -> torch.Tensor:
    """The float32 contiguous samples of a real leaf, by torch ops: autograd carries a float64
    leaf's cast back."""
    return t.to(torch.float32).resolve_neg().contiguous()


def _pad_real(t: torch.Tensor, cp: int) -> torch.Tensor:
    """float32 contiguous [B, cp, H, W] of a real device tensor [B, C, H, W], cp = C or C + 1 (a
    zero plane: the kernels take plane pairs)."""
    b, c, h, w = t.shape
    if cp == c:
        return t.to(torch.float32).resolve_neg().contiguous()
    vals = torch.zeros((b, cp, h, w), dtype=torch.float32, device=t.device)
    vals[:, :c] = t
    return vals


def _plane_mean(field: torch.Tensor, groups: int) -> torch.Tensor:
    """mean over each group's planes of |field|^2: complex [B, C, H, W] -> float32 [B, G, H, W]"""
    b, c, h, w = field.shape
    return torch.view_as_real(field).square().sum(-1).view(b, groups, c // groups, h, w).mean(2)


# the Plan methods of the two phase kinds at a single depth: field alone, evaluate, backward
_PHASE_CALLS = {_lib.LEAF_PHASE: ("simulate_phase", "evaluate_phase", "phase_backward"),
                _lib.LEAF_PHASE_LEVELS: ("simulate_phase_levels", "evaluate_phase_levels", "phase_levels_backward")}


class _Leaf:
    """What a call fixed before any GPU use: the geometry (wls, dx, dy, tf_kind; dev once the input
    is on its device), the leaf kind (_lib.LEAF_*) with field_kind, ste_args and levels, the planes c
    of the tensor the kernels read, and the extent -- exactly one of a single depth z, a window
    (N, in_win, out_win) at depth z (_window_args) or a focal stack zs.  Which Plan method a leaf kind
    and an extent take is decided here and nowhere else.

    A plan carries 2 C / G real planes per group for the complex and phase kinds and for every
    adjoint, C / G (padded to even) for a real or thresholded forward; a thresholded leaf's plans and
    a window's have the field kind given (the leaf's vb), every other plan FIELD_AMPLITUDE."""

    def __init__(self, wls, dx, dy, tf_kind, leaf, field_kind=_lib.FIELD_AMPLITUDE, ste_args=None, levels=None,
                 c=0, z=None, win=None, zs=None, recompute=False, dev=None, source=None):
        self.wls, self.dx, self.dy, self.tf_kind, self.leaf, self.dev = wls, dx, dy, tf_kind, leaf, dev
        self.field_kind, self.ste_args, self.levels, self.c = field_kind, ste_args, levels, c
        self.z, self.win, self.zs = z, win, zs
        self.groups = len(wls)
        # source: the illumination as given (checked, _source_arg); _device_leaf replaces it by the complex64
        # [G, H, W] device tensor the kernels read.  Under a source every kind is one complex plane per leaf
        # plane, the real and the thresholded one included (a single depth, no window: _leaf_args)
        self.source = source
        self.real_in = leaf in (_lib.LEAF_REAL, _lib.LEAF_THRESHOLD) and source is None
        self.plan_field = field_kind if leaf == _lib.LEAF_THRESHOLD or win is not None else _lib.FIELD_AMPLITUDE
        self.tau = ste_args[0] if ste_args is not None else 0.0
        self.ste = {} if ste_args is None else dict(surrogate=ste_args[1], p0=ste_args[2], p1=ste_args[3])
        # the backward's last pass reads the leaf's samples / the Functions save the leaf (a window and
        # a stack take the gradient's shape from it)
        self.reads_leaf = leaf in (_lib.LEAF_PHASE, _lib.LEAF_PHASE_LEVELS, _lib.LEAF_THRESHOLD)
        self.keeps_leaf = self.reads_leaf or win is not None or zs is not None
        # tt.intensity(save_field=False) of a real leaf at one depth: keep x, form the field again
        self.recompute = recompute and leaf == _lib.LEAF_REAL and not (win or zs) and source is None

    def _plan(self, b, planes, h, w, adjoint):
        if self.win is not None:
            h = w = self.win[0]
        if self.zs is None:
            return _plan_for(h, w, planes // self.groups, self.wls, self.dx, self.dy, -self.z if adjoint else self.z, b,
                             self.dev, self.tf_kind, self.plan_field)
        depths = tuple(-v for v in self.zs) if adjoint else self.zs
        return _plan_for(h, w, planes // self.groups, self.wls, self.dx, self.dy, depths[0], b, self.dev, self.tf_kind,
                         self.plan_field, depths, depth_slots=adjoint)

    def forward_plan(self, x):
        b, c, h, w = x.shape
        return self._plan(b, c + (c % 2) if self.real_in else 2 * c, h, w, False)

    def adjoint_plan(self, t):
        """The plan for -z (the negated depths) of one complex plane per plane of t [.., B, C, H, W]: the
        leaf, or the values of a backward pass that does not keep it.  A stack's takes B G D job slots."""
        b, c, h, w = t.shape[-4:]
        return self._plan(b, 2 * c, h, w, True)

    def kept(self, x):
        return (x,) if self.keeps_leaf else ()

    def kept_source(self):
        """the device source for save_for_backward, last of what a Function saves: the backward reads it from
        there, so a source changed in place between the two passes is an error, as it is for the target"""
        return () if self.source is None else (self.source,)

    def split_source(self, saved):
        """saved tensors -> (those without the source, the source | None)"""
        return (saved, None) if self.source is None else (saved[:-1], saved[-1])

    def evaluate(self, x, target=None, want_field=True, want_intensity=True, pixel_weight=None):
        """One forward launch set -> (plan, field | None, intensity | None, chan_stats | None).  A real
        or thresholded leaf of an odd C is padded with a zero plane here: the field keeps it, and the
        intensity is the mean over the C planes given.  pixel_weight (loss and loss_stack alone: a
        target, an even C for a real leaf, no window): the weighted statistics of hbx_evaluate_pw /
        hbx_evaluate_stack_pw."""
        plan, leaf = self.forward_plan(x), self.leaf
        if self.source is not None:                             # without a target the intensity is the call's output
            field, inten, stats = plan.evaluate_source(x, leaf, self.source, target, pixel_weight, want_field=want_field,
                                                       want_intensity=want_intensity or target is None,
                                                       levels=self.levels, threshold=self.tau)
            return plan, field, (inten if want_intensity else None), stats
        if pixel_weight is not None:
            call = plan.evaluate_pw if self.zs is None else plan.evaluate_stack_pw
            return (plan,) + call(x, leaf, target, pixel_weight, want_field=want_field, want_intensity=want_intensity,
                                  levels=self.levels, threshold=self.tau)
        if self.zs is not None:
            return (plan,) + plan.evaluate_stack(x, leaf, target, want_field=want_field, want_intensity=want_intensity,
                                                 levels=self.levels, threshold=self.tau)
        c = x.shape[1]
        cp = c + (c % 2) if self.real_in else c
        if cp != c:
            x = _pad_real(x, cp)
        if self.win is not None:
            _, in_win, out_win = self.win
            if leaf == _lib.LEAF_THRESHOLD:
                out = plan.evaluate_threshold_window(x, self.tau, in_win, target, out_win, want_field, want_intensity)
            else:
                out = plan.evaluate_real_window(x, in_win, target, out_win, want_field, want_intensity)
        elif leaf == _lib.LEAF_THRESHOLD:
            out = plan.evaluate_threshold(x, self.tau, target, want_field, want_intensity)
        elif leaf == _lib.LEAF_REAL:
            if target is not None:
                out = plan.evaluate_real(x, target, want_field, want_intensity)
            elif want_field:
                out = plan.simulate_real(x, want_intensity)
            else:
                out = None, plan.intensity_real(x)             # no field is written
        elif leaf == _lib.LEAF_COMPLEX:
            if target is not None:
                out = plan.evaluate_complex(x, target, want_field, want_intensity)
            else:                                               # |.|^2 and the mean are torch ops
                field, _ = plan.simulate_complex(x)
                out = (field if want_field else None), (_plane_mean(field, self.groups) if want_intensity else None)
        else:
            simulate, evaluate, _ = _PHASE_CALLS[leaf]
            lv = (self.levels,) if leaf == _lib.LEAF_PHASE_LEVELS else ()
            if target is None and not want_intensity:
                out = getattr(plan, simulate)(x, *lv)[:1]
            else:
                out = getattr(plan, evaluate)(x, *lv, target, want_field, want_intensity)
        field, inten, stats = (tuple(out) + (None, None))[:3]
        if cp != c and inten is not None:
            inten = inten * (cp / c)                            # the kernel's mean counts the zero plane
        return plan, field, inten, stats

    def field(self, x):
        """The propagated field of every plane of x (a stack's call also writes the intensity)"""
        field = self.evaluate(x, want_intensity=self.zs is not None)[1]
        return field if field.shape[-3] == x.shape[1] else field[:, :x.shape[1]]

    def backward(self, x, values, weight=None, scale=1.0, adj=None, source=None):
        """One launch set on the adjoint plan (adj, where the caller has fetched it already): the
        leaf's gradient from `values` (the gradient with respect to the field, or with `weight` the
        saved field).  x: the leaf where the Functions keep it, else None.  A real leaf receives the
        real part, a complex one the field, the phase kinds and a thresholded leaf what the last pass
        of their backward call writes."""
        if adj is None:
            adj = self.adjoint_plan(values if x is None else x)
        samples = x if self.reads_leaf else None
        if self.source is not None:                             # source: the saved one (split_source)
            return adj.backward_source(values, self.leaf, source, samples=samples, weight=weight, scale=scale,
                                       levels=self.levels, **self.ste)
        if self.zs is not None:
            return adj.backward_stack(values, self.leaf, samples=samples, weight=weight, scale=scale,
                                      levels=self.levels, **self.ste)
        if self.win is not None:                                # values at the forward's output window
            return adj.backward_window(values, self.win[2], self.win[1], samples=samples, weight=weight, scale=scale,
                                       **self.ste)
        if self.leaf == _lib.LEAF_THRESHOLD:
            return adj.threshold_backward(values, x, weight=weight, scale=scale, **self.ste)
        if self.leaf in _PHASE_CALLS:
            lv = (self.levels,) if self.leaf == _lib.LEAF_PHASE_LEVELS else ()
            return getattr(adj, _PHASE_CALLS[self.leaf][2])(values, x, *lv, weight=weight, scale=scale)
        cplx = self.leaf == _lib.LEAF_COMPLEX
        gf, gr = adj.simulate_complex(values, want_field=cplx, want_real=not cplx, weight=weight, scale=scale)
        grad = gf if cplx else gr
        return grad if grad.shape[1] == self.c else grad[:, :self.c]    # a padded field's zero plane

    def loss(self, plan, stats, kind, rel, weight_sum=None):
        if weight_sum is not None:                              # a per-pixel weight: its sum for the pixel count
            return plan.loss_pw(stats, weight_sum, kind, rel, stack=self.zs is not None)
        if self.zs is not None:
            return plan.loss_stack(stats, kind, rel)
        if self.win is not None:
            return plan.loss_window(stats, self.win[2], kind, rel)
        return plan.loss(stats, kind, rel)

    def loss_weight(self, adj, inten, target, stats, gl, kind, rel, pixel_weight=None, weight_sum=None):
        """dL/dI = a I + c T per env on the adjoint plan (its G and N only); with a per-pixel weight v,
        v (a I + c T) with the weight sum for the pixel count"""
        if pixel_weight is not None:
            return adj.loss_weight_pw(inten, target, pixel_weight, stats, weight_sum, gl, kind, rel,
                                      stack=self.zs is not None)
        if self.zs is not None:
            return adj.loss_weight_stack(inten, target, stats, gl, kind, rel)
        if self.win is not None:
            return adj.loss_weight_window(inten, target, stats, self.win[2], gl, kind, rel)
        return adj.loss_weight(inten, target, stats, gl, kind, rel)


def _evaluate(t: torch.Tensor, target: torch.Tensor, geom, groups: int, want_field: bool, phase: bool = False):
    """One launch set on a device tensor [B, C, H, W] at one depth (real, complex, or phase samples)
    -> (plan, field | None, intensity | None, chan_stats)"""
    wls, dx, dy, z, dev, tf_kind = geom
    leaf = _lib.LEAF_PHASE if phase else _lib.LEAF_COMPLEX if t.is_complex() else _lib.LEAF_REAL
    t = t.to(torch.complex64).resolve_conj().resolve_neg().contiguous() if t.is_complex() else _phase_samples(t)
    return _Leaf(wls, dx, dy, tf_kind, leaf, c=t.shape[1], z=z, dev=dev).evaluate(t, target, want_field, want_field)


def _materialised(grad_output: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """grad_output as the kernels read it: torch conjugates and negates lazily (the grad_output of a
    loss that ends in F.conj()), and the kernels read the memory behind data_ptr()"""
    g = grad_output.to(dtype)
    return (g.resolve_conj() if dtype.is_complex else g).resolve_neg().contiguous()


class _Simulate(torch.autograd.Function):
    """x -> the field A u(x) of every plane (every depth of a stack), for every leaf kind.  Backward:
    one launch set of grad_output on the adjoint plan (A^H g = IFFT2(FFT2(g) conj H(z)), and
    conj H(z) = H(-z) for both transfer functions), whose last pass writes the leaf's gradient
    (_Leaf.backward).  No double backward."""

    @staticmethod
    def forward(ctx, x, spec):
        ctx.spec = spec
        ctx.save_for_backward(*spec.kept(x), *spec.kept_source())
        return spec.field(x)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        saved, src = ctx.spec.split_source(ctx.saved_tensors)
        x, = saved or (None,)
        return ctx.spec.backward(x, _materialised(grad_output, torch.complex64), source=src), None


class _Intensity(torch.autograd.Function):
    """x -> I = mean_p |A u_p|^2 per colour group, with the field F = A u saved (and the leaf where
    its backward reads it).  dL/du = A^H((2 / P) gI F): one launch set of F on the adjoint plan, whose
    first pass applies (2 / P) gI as it loads F -- the complex tensor (2 / P) gI F is never
    written.  spec.recompute: only x is saved, and the backward forms F again first.  No double
    backward."""

    @staticmethod
    def forward(ctx, x, spec):
        ctx.spec = spec
        if spec.recompute:
            ctx.save_for_backward(x)
            return spec.evaluate(x, want_field=False)[2]
        _, field, inten, _ = spec.evaluate(x)
        ctx.save_for_backward(field, *spec.kept(x), *spec.kept_source())
        return inten

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        spec = ctx.spec
        saved, src = spec.split_source(ctx.saved_tensors)
        if spec.recompute:
            field, x = spec.evaluate(saved[0], want_intensity=False)[1], None
        else:
            field, x = saved[0], (saved[1] if len(saved) > 1 else None)
        gi = _materialised(grad_output, torch.float32)
        return spec.backward(x, field, weight=gi, scale=2.0 / (spec.c // spec.groups), source=src), None


class _Loss(torch.autograd.Function):
    """x -> the relative MSE or PSNR per env of I = mean_p |A u_p|^2 against a constant target (over
    the roi of a window, over all depths of a stack).  The forward pass is one launch set that leaves
    the field F, I and the statistics; with w = gL dL/dI = a I + c T (_Leaf.loss_weight: a, c per
    env from the statistics and the incoming gradient gL), dL/du = A^H((2 / P) w F): one launch set
    of F on the adjoint plan, as _Intensity's backward pass.  pw: a per-pixel weight v of the target's
    shape (or None), saved with its sum per env next to the target; the statistics, the loss and
    dL/dI = v (a I + c T) are then the weighted ones.  No double backward."""

    @staticmethod
    def forward(ctx, x, target, spec, kind, rel, pw=None):
        ctx.spec, ctx.kind, ctx.rel, ctx.weighted = spec, kind, rel, pw is not None
        plan, field, inten, stats = spec.evaluate(x, target, pixel_weight=pw)
        wsum = None if pw is None else plan.pixel_weight_sum(pw, stack=spec.zs is not None)
        ctx.save_for_backward(field, inten, stats, target, *spec.kept(x), *(() if pw is None else (pw, wsum)),
                              *spec.kept_source())
        return spec.loss(plan, stats, kind, rel, wsum)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        spec = ctx.spec
        saved, src = spec.split_source(ctx.saved_tensors)
        pw, wsum = saved[-2:] if ctx.weighted else (None, None)
        field, inten, stats, target, x = saved[:4] + ((saved[4],) if spec.keeps_leaf else (None,))
        gl = _materialised(grad_output, torch.float64)
        adj = spec.adjoint_plan(field if x is None else x)
        wgt = spec.loss_weight(adj, inten, target, stats, gl, ctx.kind, ctx.rel, pw, wsum)
        grad = spec.backward(x, field, weight=wgt, scale=2.0 / (spec.c // spec.groups), adj=adj, source=src)
        return grad, None, None, None, None, None


def _as_tensor(x) -> torch.Tensor:
    return x.as_subclass(torch.Tensor) if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))


def _source_arg(source, groups: int, h: int, w: int, what: str) -> torch.Tensor:
    """source= of simulate, intensity and loss -> a real or complex tensor that expands to [G, H, W], a
    constant, still as given (_device_leaf casts and expands it on the device); anything else raises
    ValueError."""
    try:
        src = _as_tensor(source)
    except (TypeError, ValueError, RuntimeError) as e:
        raise ValueError(f"{what}: source= must be a real or complex tensor or array ({e})") from None
    if src.dtype == torch.bool or not (src.is_complex() or src.is_floating_point() or
                                       src.dtype in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)):
        raise ValueError(f"{what}: source= must have a numeric dtype, got {src.dtype}")
    if src.requires_grad:
        raise ValueError(f"{what}: the source is a constant (it requires grad); there is no gradient with respect to it")
    want = (groups, h, w)
    try:
        ok = src.dim() in (2, 3) and tuple(torch.broadcast_shapes(tuple(src.shape), want)) == want
    except RuntimeError:
        ok = False
    if not ok:
        raise ValueError(f"{what}: source {tuple(src.shape)} is neither [H, W] nor [G, H, W] = {want}")
    return src


def _leaf_args(x, what: str, tf, field, threshold, ste, ste_width, grid, origin, roi, levels, z=None, zs=None,
               binary: bool = False, save_field: bool = True, pixel_weight=None, source=None):
    """The checks of every public call, all before any GPU use -> (t [B, C, H, W] as given, the _Leaf
    without its device, whether x was 3-D).  what: the public function's name; its own rules are
    `simulate`: one wavelength, any C (an odd one is padded); `intensity`: an odd C / G only for one
    group of a real or complex field or a phase; `loss`: an even C / G for a real field; the *_stack
    calls (zs given): no window, an even C / G for a real or thresholded leaf, a built grid."""
    stacked = zs is not None
    if pixel_weight is not None and (grid is not None or origin is not None or roi is not None):
        raise ValueError(f"{what}: pixel_weight= is not accepted with grid=, origin= or roi= (a rectangle is the "
                         "weight that is 1 inside it)")
    if source is not None:
        if stacked:
            raise ValueError(f"{what}: source= is not accepted (a focal stack is lit by the unit plane wave)")
        if binary:
            raise ValueError(f"{what}: source= lights a leaf on the continuous path (binary=False)")
        if grid is not None or origin is not None or roi is not None:
            raise ValueError(f"{what}: source= is not accepted with grid=, origin= or roi= (a source that is 0 "
                             "outside a rectangle is the dark surround)")
    if stacked:
        if grid is not None or origin is not None or roi is not None:
            raise ValueError(f"{what}: grid=, origin= and roi= are not accepted (focal stacks are not windowed)")
        zs = _depths_arg(zs, what)
    tf_kind = _switch(tf, _TF_NAMES, "tf")
    field_kind = _switch(field, _FIELD_NAMES, "field")
    ste_args = _ste_args(threshold, ste, ste_width, what)
    if ste_args is not None and binary:
        raise ValueError("simulate: threshold= binarizes a real leaf on the continuous path (binary=False)")
    meta = _meta_of(x)
    wl = meta["wl"]
    if what == "simulate":
        if isinstance(wl, (tuple, list)) and len(wl) != 1:
            raise ValueError("simulate: one wavelength per call (the reference splits RGB groups, "
                             "env_1024_24.py:149-155)")
    wls = tuple(float(v) for v in wl) if isinstance(wl, (tuple, list)) else (float(wl),)
    groups = len(wls)
    if not 1 <= groups <= _lib.MAX_GROUPS:
        raise ValueError(f"{what}: 1 to {_lib.MAX_GROUPS} wavelengths, got {groups}")
    dx, dy = meta.get("dx", (hbx.plan.PIXEL_PITCH,) * 2)
    t = _as_tensor(x)
    squeeze = t.dim() == 3
    if squeeze:
        t = t.unsqueeze(0)
    if t.dim() != 4:
        forms = "[B, C, H, W]" if what == "simulate" else "[B, C, H, W] or [C, H, W]"
        raise ValueError(f"{what} expects {forms}, got {tuple(t.shape)}")
    c, cplx, thresholded = t.shape[1], t.is_complex(), ste_args is not None
    if what != "simulate" and (c == 0 or c % groups):
        raise ValueError(f"{what}: {c} planes do not split into {groups} colour groups")
    per, odd = c // groups, (c // groups) % 2
    if what == "intensity" and groups > 1 and odd:
        raise ValueError(f"intensity: {groups} colour groups need an even number of planes each, got {per}")
    tt_what = what if stacked else "tt." + what
    if cplx and binary:
        raise ValueError("tt.simulate (hbx) propagates binary {0,1} masks only, as the reference does")
    if cplx and field_kind != _lib.FIELD_AMPLITUDE:
        raise ValueError(f"{tt_what}: a complex field is used as it is (field=\"amplitude\")")
    # (under a source every kind is one complex plane per leaf plane: no plane pairs, no even count asked)
    if what == "loss" and not cplx and field_kind == _lib.FIELD_AMPLITUDE and odd and source is None:
        raise ValueError(f"loss: a real field needs an even number of planes per colour group, got {per}")
    if thresholded:
        if cplx:
            raise ValueError(f"{tt_what}: threshold= needs a real leaf, got a complex field")
        if what in ("intensity", "loss") and odd and source is None:
            raise ValueError(f"{what}: threshold= needs an even number of planes per colour group, got {per}")
    if grid is not None and binary:
        raise ValueError("simulate: grid= places a real leaf on the continuous path (binary=False)")
    levels = _levels_arg(levels, binary, cplx, field_kind, thresholded, grid, what)
    win = _window_args(grid, origin, roi, t.shape, cplx, field_kind, thresholded, what)
    if win is not None and what == "intensity" and odd:
        raise ValueError(f"intensity: grid= needs an even number of planes per colour group, got {per}")
    if cplx:
        leaf = _lib.LEAF_COMPLEX
    elif thresholded:
        leaf = _lib.LEAF_THRESHOLD
    elif levels is not None:
        leaf = _lib.LEAF_PHASE_LEVELS
    elif field_kind == _lib.FIELD_PHASE:
        leaf = _lib.LEAF_PHASE
    else:
        leaf = _lib.LEAF_REAL
    if stacked:
        if leaf in (_lib.LEAF_REAL, _lib.LEAF_THRESHOLD) and odd:
            raise ValueError(f"{what}: a real or thresholded leaf needs an even number of planes per colour group, "
                             f"got {per}")
        if t.shape[2] != t.shape[3] or t.shape[2] not in _GRIDS:
            raise ValueError(f"{what}: the hologram is one of the built grids {_GRIDS} squared, got {tuple(t.shape[2:])}")
    # a windowed simulate pads an odd C by torch ops (the Function sees, and returns, the pair)
    c_seen = c + (c % 2) if win is not None else c
    if source is not None:
        source = _source_arg(source, groups, t.shape[2], t.shape[3], what)
    spec = _Leaf(wls, dx, dy, tf_kind, leaf, field_kind, ste_args, levels, c=c_seen, z=z, win=win, zs=zs,
                 recompute=not save_field, source=source)
    return t, spec, squeeze


def _target_arg(target, want: Tuple[int, ...], squeeze: bool, what: str) -> torch.Tensor:
    """target of loss and loss_stack -> the tensor of shape `want` (given without the env axis for a
    3-D x), a real constant; anything else raises ValueError."""
    tg = _as_tensor(target)
    axis = len(want) - 4                                        # the env axis: after a stack's depth axis
    if axis and tg.dim() != (4 if squeeze else 5):
        raise ValueError(f"{what}: target must be [D, B, G, H, W] ([D, G, H, W] for a 3-D x), got {tuple(tg.shape)}")
    if squeeze:
        tg = tg.unsqueeze(axis)
    if tg.is_complex() or tuple(tg.shape) != want:
        raise ValueError(f"{what}: target must be real {want}, got {tuple(tg.shape)} {tg.dtype}")
    if tg.requires_grad:
        raise ValueError(f"{what}: the target is a constant (it requires grad)")
    return tg


def _pixel_weight_arg(pixel_weight, want: Tuple[int, ...], squeeze: bool, what: str) -> torch.Tensor:
    """pixel_weight of loss and loss_stack -> a real tensor that broadcasts to the target's shape `want`
    (for a 3-D x: to the shape without the env axis), a constant; anything else raises ValueError.  It is
    still as given: _loss expands it on the device."""
    pw = _as_tensor(pixel_weight)
    if pw.is_complex():
        raise ValueError(f"{what}: pixel_weight must be a real tensor, got {pw.dtype}")
    if pw.requires_grad:
        raise ValueError(f"{what}: the pixel weight is a constant (it requires grad)")
    axis = len(want) - 4                                        # the env axis: after a stack's depth axis
    shape = want[:axis] + want[axis + 1:] if squeeze else want
    try:
        ok = pw.dim() <= len(shape) and tuple(torch.broadcast_shapes(tuple(pw.shape), shape)) == tuple(shape)
    except RuntimeError:
        ok = False
    if not ok:
        raise ValueError(f"{what}: pixel_weight {tuple(pw.shape)} does not broadcast to the target's shape {shape}")
    if squeeze and pw.dim() == len(shape):
        pw = pw.unsqueeze(axis)
    return pw


def _device_leaf(t: torch.Tensor, spec: _Leaf, what: str, cast: bool = True) -> torch.Tensor:
    """The device tensor the kernels read, cast by torch ops (autograd carries the casts of a float64
    or complex128 leaf back); names the device in the spec."""
    if not torch.cuda.is_available():
        raise RuntimeError(f"tt.{'*_stack' if spec.zs is not None else what} needs a ROCm GPU (libhbx.so)")
    if t.is_cuda:
        spec.dev = t.device.index
    else:
        spec.dev = torch.cuda.current_device()
        t = t.to(f"cuda:{spec.dev}")
    if spec.source is not None:                                 # once per call: complex64 [G, H, W], contiguous
        spec.source = (spec.source.to(device=t.device).to(torch.complex64).resolve_conj().resolve_neg()
                       .expand(spec.groups, t.shape[2], t.shape[3]).contiguous())
    if not cast:
        return t
    if spec.leaf == _lib.LEAF_COMPLEX:
        return t.to(torch.complex64).resolve_conj().resolve_neg().contiguous()
    return _pad_real(t, spec.c) if spec.c != t.shape[1] else _phase_samples(t)


def _wants_grad(xs: torch.Tensor) -> bool:
    return xs.requires_grad and torch.is_grad_enabled()


def _simulate(t, spec, squeeze, what):
    """simulate's continuous path and simulate_stack on the checked input: through _Simulate with a
    gradient request, else the plain call with no graph"""
    xs = _device_leaf(t, spec, what)
    out = _Simulate.apply(xs, spec) if _wants_grad(xs) else spec.field(xs)
    if out.shape[-3] != t.shape[1]:
        out = out[:, :t.shape[1]]                               # the plane a windowed odd C was padded with
    return out.select(0 if spec.zs is None else 1, 0) if squeeze else out


def _intensity(t, spec, squeeze, what):
    """intensity and intensity_stack on the checked input; without a gradient request no field is kept"""
    xs = _device_leaf(t, spec, what)
    out = _Intensity.apply(xs, spec) if _wants_grad(xs) else spec.evaluate(xs, want_field=False)[2]
    return out.select(0 if spec.zs is None else 1, 0) if squeeze else out


def _loss(t, target, spec, squeeze, what, kind, rel, pixel_weight=None):
    """loss and loss_stack on the checked input: the target has the shape of the intensity (a window's
    roi, a stack's depths first); without a gradient request neither field nor intensity is written.
    pixel_weight None: the code as it was; else the weight is expanded to the target's shape and made
    contiguous float32 on the device, once per call."""
    b, _, h, w = t.shape
    depths = () if spec.zs is None else (len(spec.zs),)
    want = depths + (b, spec.groups) + ((h, w) if spec.win is None else spec.win[2][2:])
    tg = _target_arg(target, want, squeeze, what)
    if pixel_weight is None:
        xs = _device_leaf(t, spec, what)
        tg = tg.to(device=xs.device, dtype=torch.float32).contiguous()
        if _wants_grad(xs):
            out = _Loss.apply(xs, tg, spec, kind, rel)
        else:
            plan, _, _, stats = spec.evaluate(xs, tg, want_field=False, want_intensity=False)
            out = spec.loss(plan, stats, kind, rel)
        return out[0] if squeeze else out
    pw = _pixel_weight_arg(pixel_weight, want, squeeze, what)
    xs = _device_leaf(t, spec, what)
    tg = tg.to(device=xs.device, dtype=torch.float32).contiguous()
    pw = pw.to(device=xs.device, dtype=torch.float32).expand(want).contiguous()
    if _wants_grad(xs):
        out = _Loss.apply(xs, tg, spec, kind, rel, pw)
    else:
        plan, _, _, stats = spec.evaluate(xs, tg, want_field=False, want_intensity=False, pixel_weight=pw)
        out = spec.loss(plan, stats, kind, rel, plan.pixel_weight_sum(pw, stack=spec.zs is not None))
    return out[0] if squeeze else out


def simulate(x, z: float, strict: bool = False, binary: bool = True, tf="asm", field="amplitude",
             threshold=None, ste="window", ste_width=0.5, grid=None, origin=None, roi=None, levels=None,
             source=None, **_) -> torch.Tensor:
    """Free-space propagation of a tensor [B, C, H, W] (or [C, H, W]) by z metres: the
    complex field of every plane, complex64, on the GPU.

    tf: "asm" (exact angular spectrum) or "fresnel"; field: "amplitude" or "phase" (both also
    take the hbx._lib TF_* / FIELD_* integers; an unknown value raises ValueError).

    binary=True (default): x is a binary {0,1} mask, packed to bits; amplitude u = m, phase
    u = exp(i pi m) = 1 - 2 m.  A value other than 0 / 1 raises ValueError -- deferred to the
    next point the host waits (module docstring), or here with strict=True (one host sync).
    Complex input is refused.

    binary=False: the continuous path; no binary check, `strict` is ignored.
      real x,    field="amplitude":  u = x (float64 is cast to float32), one real plane each;
      complex x, field="amplitude":  u = x (cast to complex64), through hbx_simulate_complex;
      real x,    field="phase":      u = exp(i pi x), formed by the first pass of hbx_simulate_phase
                                     (float64 is cast to float32; x and x + 2 are the same field).
    A complex plane takes the workspace of two real planes.  If x requires grad the result
    carries a grad_fn and loss.backward() reaches x (module docstring); otherwise it has none.

    binary=False with threshold=tau: real x is the leaf of a binary hologram m = [x >= tau], and
    the field is that of the mask, amplitude u = m or phase u = 1 - 2 m (what binary=True gives
    for m), thresholded by the first pass of hbx_evaluate_threshold as it loads x -- no 0 / 1 copy
    is written.  If x requires grad the backward pass is the straight-through estimator, one
    hbx_threshold_backward on the plan for -z: dL/dx = vb s(x) Re(A^H g) with vb = 1 or -2 and
    the surrogate derivative s of the step, ste="window": s = 1 on [tau - ste_width, tau +
    ste_width] (math.inf: everywhere), else 0; ste="sigmoid": the derivative of
    sigmoid((x - tau) / ste_width).  Complex x, or binary=True, with a threshold raises ValueError.

    binary=False with grid=N (64, 256, 896 or 1024; None runs the code above untouched): real x is a
    hologram [B, C, h, w] of any size h, w <= N, zero-filled into the N x N grid -- outside it there
    is no light, also for a thresholded field="phase" leaf -- so a guard band costs no F.pad copy and
    a non-square modulator propagates at all.  origin=(y0, x0) places it (default: centred, ((N - h)
    // 2, (N - w) // 2)); roi=(y0, x0, h, w) in grid coordinates is the rectangle the field is
    returned over (default: the hologram's own).  The first pass loads x only inside its rectangle
    and the last pass stores only the roi (hbx_evaluate_real_window / _threshold_window); the
    backward pass is one hbx_backward_window on the plan for -z.  A complex x, field="phase"
    without a threshold, binary=True, or an origin or roi outside the grid raises ValueError before
    any GPU use.

    binary=False with field="phase" and levels=L (2 <= L <= 256; None runs the code above untouched):
    real x is the leaf of the hologram an L-level phase modulator displays -- each sample goes to the
    nearest level 2 k / L (hbx.quantize_phase; ties to the even k) in the first pass of
    hbx_simulate_phase_levels as it loads x, and no quantized copy is written.  The result is
    simulate's on hbx.quantize_phase(x, L, want_levels=False, want_samples=True) bit for bit.  If x
    requires grad the backward pass is the straight-through estimator dq/dx := 1, one
    hbx_phase_levels_backward on the plan for -z: the continuous gradient at the displayed phase.
    levels with binary=True, a complex x, field="amplitude", threshold=, grid=, a non-integer or a
    value outside [2, 256] raises ValueError before any GPU use.

    binary=False with source=s (None runs the code above untouched; every leaf kind): the modulator is
    lit by the complex illumination s instead of a unit plane wave on axis, u = s f(x) with f the leaf
    kind's map above -- an oblique plane wave, a Gaussian beam, a converging reference wave, a lit disc
    (tt.sources has the usual ones; s = 0 is a dark surround for every kind).  s is a real or complex
    tensor or array [H, W] or [G, H, W], a constant, cast to complex64 and expanded once per call.  The
    first pass multiplies by the source row as it loads x (hbx_evaluate_source): neither s f(x) nor,
    for a phase or thresholded leaf, f(x) is written.  If x requires grad the backward pass is one
    hbx_backward_source on the plan for -z: its last pass multiplies the back-propagated plane by
    conj(s) and applies the leaf's own gradient formula (the phase gradient, the straight-through
    estimators); the source is saved for it with the other tensors.  An odd number of planes per group
    needs no padding plane under a source, also for a real or thresholded leaf of intensity and loss.  binary=True, grid= / origin= / roi=, a source that requires grad, a shape that does
    not expand to [G, H, W] or a non-numeric dtype raises ValueError before any GPU use; the *_stack
    calls take no source.  Out of scope: a gradient with respect to the source, a per-env or per-plane
    source, windows and focal stacks under a source."""
    t, spec, squeeze = _leaf_args(x, "simulate", tf, field, threshold, ste, ste_width, grid, origin, roi, levels, z=z,
                                  binary=binary, source=source)
    if not binary:
        return _simulate(t, spec, squeeze, "simulate")
    t = _device_leaf(t, spec, "simulate", cast=False)
    sc = _scratch(spec.dev)
    _raise_pending(sc)                              # an earlier call's input, already checked
    b, c, h, w = t.shape
    cp = c + (c % 2)                                # the kernels pack plane pairs
    plan = _plan_for(h, w, cp, spec.wls, spec.dx, spec.dy, z, b, spec.dev, spec.tf_kind, spec.field_kind)
    if cp == c:
        bits = hbx.pack_mask(t, error_ptr=sc.err_dev)
    else:
        bits = torch.zeros((b, cp, h, w // 64), dtype=torch.int64, device=t.device)
        bits[:, :c] = hbx.pack_mask(t, error_ptr=sc.err_dev)
    field, _ = plan.simulate(bits)
    if strict:
        torch.cuda.current_stream(spec.dev).synchronize()
        _raise_pending(sc)
    if cp != c:
        field = field[:, :c]
    return field[0] if squeeze else field


def intensity(x, z: float, tf="asm", field="amplitude", save_field: bool = True, threshold=None, ste="window",
              ste_width=0.5, grid=None, origin=None, roi=None, levels=None, source=None) -> torch.Tensor:
    """Plane-mean intensity of the propagated field, the quantity every loss of the project goes
    through: float32 [B, G, H, W] (or [G, H, W] for a 3-D x) with
        I[b, g] = mean over the planes p of group g of |IFFT2(FFT2(u[b, p]) H_g(z))|^2,
    what ``(tt.simulate(x, z, binary=False).abs() ** 2)`` averaged over each group's planes gives,
    without leaving the HIP path.  The continuous path only: the samples are the field, as with
    simulate(.., binary=False) (0 / 1 samples give the bit path's intensity); tf and field as there.

    meta['wl'] is one wavelength (G = 1) or a tuple of G <= 4 wavelengths: the C planes are then G
    colour groups of C / G planes in order (channel c belongs to group c // (C / G)), one plan and
    one launch set for all of them -- the reference's RGB reconstruction (env_1024_24.py:149-166)
    in one call.  C % G != 0 raises ValueError, and so does an odd C / G with G > 1; with G = 1 an
    odd C is padded with a zero plane and the mean is still over the C planes given.

    Without a gradient request no graph is built: real x goes through hbx_intensity_real, which
    writes the intensity and no field; complex x through hbx_simulate_complex, with |.|^2 and the
    mean as torch ops; field="phase" on real x (u = exp(i pi x)) through hbx_evaluate_phase, which
    writes the intensity and no field.
    If x requires grad the result carries a grad_fn whose backward pass is ONE
    hbx_simulate_complex_weighted on the plan for -z: the saved field is read with (2 / P) times
    the incoming gradient applied in the first pass's load, and a real x receives the real part
    only (a float64 leaf a float64 gradient).  The forward of a real x takes the intensity the
    last pass accumulates beside the field (hbx_simulate_real, one launch set).
    save_field=True keeps the complex field for the backward pass (8 bytes per pixel and plane);
    save_field=False (real x) keeps only x, writes no field in the forward pass and recomputes it
    at the start of the backward pass.  field="phase" with a gradient request: the forward is one
    hbx_evaluate_phase (field and intensity), the backward one hbx_phase_backward, which writes
    dL/dx itself; the field is always saved.  No double backward.

    threshold=tau (real x only; complex x raises ValueError): x is the leaf of a binary hologram
    m = [x >= tau] and I is the intensity of its field, amplitude u = m or phase u = 1 - 2 m,
    through hbx_evaluate_threshold; ste and ste_width choose the straight-through backward pass
    (hbx_threshold_backward) as in simulate.  C / G must be even: a padded plane would be
    thresholded too, and its `off` value is 1, not 0, under field="phase".  The field is always
    saved.

    grid=N, origin=, roi= as in simulate (real x, with or without threshold=; C / G even): the
    intensity [B, G, h_o, w_o] over the roi of a hologram zero-filled into the N x N grid.  The
    cropped field is saved, and the backward pass is one hbx_backward_window.

    levels=L with field="phase" (real x; as in simulate): the intensity of the hologram displayed at L
    phase levels, through hbx_evaluate_phase_levels; with a gradient request the backward pass is one
    hbx_phase_levels_backward, the straight-through estimator.  The field is always saved.

    source=s as in simulate (None runs the code above untouched; every leaf kind, no grid=): the
    intensity under the illumination s, through hbx_evaluate_source; the field is always saved, and the
    backward pass is one hbx_backward_source."""
    t, spec, squeeze = _leaf_args(x, "intensity", tf, field, threshold, ste, ste_width, grid, origin, roi, levels, z=z,
                                  save_field=bool(save_field), source=source)
    return _intensity(t, spec, squeeze, "intensity")


_METRIC_NAMES = {"mse": _lib.LOSS_MSE, "psnr": _lib.LOSS_PSNR}


def loss(x, target, z: float, metric="mse", rel_scale="lsq", tf="asm", field="amplitude", threshold=None,
         ste="window", ste_width=0.5, grid=None, origin=None, roi=None, levels=None, pixel_weight=None,
         source=None) -> torch.Tensor:
    """The relative loss of a continuous hologram against a target, one value per env, without
    leaving the HIP path and without a host wait: float64 [B] on the device (0-dim for a 3-D x),
        metric="mse"   what tt.relativeLoss(I[b], target[b], F.mse_loss) gives (env.py:131),
        metric="psnr"  what tt.relativeLoss(I[b], target[b], tm.get_PSNR) gives (env.py:132,174),
    with I = tt.intensity(x, z, tf, field) -- the plane-mean intensity per colour group -- and
    rel_scale "lsq" (the least-squares scale, the default) or "none" as in relativeLoss.

    x, meta['wl'] (one wavelength or up to four: C planes in G groups), tf and field are
    tt.intensity's; C / G must be even for a real x with field="amplitude" and may be any number
    >= 1 for a complex x or field="phase" (anything else raises ValueError).  target: float32
    [B, G, H, W] (or [G, H, W] for a 3-D x), a constant -- a target that requires grad raises
    ValueError.

    The last pass of the propagation accumulates the intensity and the float64 sums of I T, I^2
    and T^2 (hbx_evaluate_real / hbx_evaluate_complex) and hbx_loss turns them into the loss.
    Without a gradient request there is no graph, and neither field nor intensity is written.  If
    x requires grad the result carries a grad_fn: the forward pass also writes the field and the
    intensity, and the backward pass is hbx_loss_weight (the loss's gradient with respect to the
    intensity, a I + c T per env) followed by one hbx_simulate_complex_weighted on the plan for
    -z.  A real x receives the real part, a complex x the field.  field="phase": the first pass
    forms u = exp(i pi x) as it loads x (hbx_evaluate_phase), and the backward's launch set is
    hbx_phase_backward, whose last pass writes dL/dx -- neither u nor the complex gradient is
    written.  No double backward.

    threshold=tau (real x only; complex x raises ValueError, and so does an odd C / G): the loss of
    the binary hologram m = [x >= tau] itself -- the mask hbx.pack_mask(x, threshold=tau) hands to
    the env, the DBS walk and the display -- with field="amplitude" u = m or field="phase"
    u = 1 - 2 m, thresholded by the first pass of hbx_evaluate_threshold as it loads x.  If x
    requires grad the backward pass is the straight-through estimator: hbx_loss_weight, then one
    hbx_threshold_backward on the plan for -z, dL/dx = vb s(x) Re(A^H((2 / P) w F)) with ste and
    ste_width as in simulate.  Neither a 0 / 1 copy of x nor the field's gradient is written.

    grid=N, origin=, roi= as in simulate (real x, with or without threshold=): the loss of a hologram
    [B, C, h, w] zero-filled into the N x N grid, taken over the roi only -- target is [B, G, h_o,
    w_o], and the statistics and the pixel count n = G h_o w_o are the roi's (the reference's crop
    before it compares, env_1024_24_128.py:144-149).  The cropped field, the cropped intensity and
    the statistics are saved; the backward pass is hbx_loss_weight_window, then one
    hbx_backward_window on the plan for -z.

    levels=L with field="phase" (real x; as in simulate): the loss of the hologram an L-level phase
    modulator displays -- hbx.quantize_phase(x, L) is its export -- quantized by the first pass of
    hbx_evaluate_phase_levels as it loads x.  If x requires grad the backward pass is the
    straight-through estimator: hbx_loss_weight, then one hbx_phase_levels_backward on the plan for -z.
    Neither the quantized samples nor exp(i pi q) nor the complex gradient is written.

    pixel_weight=v (None runs the code above untouched; every leaf kind): a non-negative per-pixel
    weight -- a signal window with a don't-care region around it, or any weighting -- that the last
    pass takes into the three sums: sum v I T, sum v I^2, sum v T^2, and W = sum v per env takes the
    place of the pixel count n in the loss (hbx_evaluate_pw, hbx_pixel_weight_sum, hbx_loss_pw).  v is
    a real tensor of the target's shape or one that broadcasts to it ([H, W], [G, H, W], ..), cast to
    float32, and a constant: one that requires grad raises ValueError, as do a complex one, one that
    does not broadcast, and pixel_weight= together with grid=, origin= or roi= (all before any GPU
    use).  v = 1 gives the unweighted loss bit for bit, v = a rectangle's indicator roi='s statistics.
    With a gradient request dL/dI = v (a I + c T) (hbx_loss_weight_pw) goes into the same backward
    launch set; the energy the hologram cannot place may land where v = 0 at no cost.  Not checked
    (a check would cost a host wait): a negative weight is used as it stands, a NaN weight poisons
    that env's loss, an env whose weights are all zero has loss 0 (psnr: +inf) and a zero gradient.

    source=s as in simulate (None runs the code above untouched; every leaf kind, with or without
    pixel_weight=, no grid=): the loss of the hologram under the illumination s.  The forward is one
    hbx_evaluate_source, whose last pass and statistics are hbx_evaluate_complex's (hbx_evaluate_pw's
    with a pixel weight); the backward pass is hbx_loss_weight (or _pw), then one hbx_backward_source
    on the plan for -z.  The loss equals tt.loss on the complex tensor s f(x) bit for bit."""
    kind = _switch(metric, _METRIC_NAMES, "metric")
    rel = _switch(rel_scale, _REL_NAMES, "rel_scale")
    t, spec, squeeze = _leaf_args(x, "loss", tf, field, threshold, ste, ste_width, grid, origin, roi, levels, z=z,
                                  pixel_weight=pixel_weight, source=source)
    return _loss(t, target, spec, squeeze, "loss", kind, rel, pixel_weight)


# ---------------------------------------------------------------------------------------------
# Focal stacks: one hologram propagated to D depths (hbx_*_stack), outputs depth-major [D, B, ...]
# ---------------------------------------------------------------------------------------------
def simulate_stack(x, zs, tf="asm", field="amplitude", threshold=None, ste="window", ste_width=0.5, levels=None,
                   grid=None, origin=None, roi=None, source=None) -> torch.Tensor:
    """The propagated field of one hologram at every depth of `zs` (1 to 8 distances, repeats and
    negative values allowed): complex64 [D, B, C, H, W] ([D, C, H, W] for a 3-D x), depth d what
    ``tt.simulate(x, zs[d], binary=False, ...)`` returns, from ONE first pass, D column passes and D
    last passes (hbx_evaluate_stack).  x, tf, field, threshold / ste / ste_width and levels are the
    continuous path's as in simulate, intensity and loss: a real field, a complex field, a phase
    (field="phase"), an L-level phase (levels=) or the real leaf of a binary hologram (threshold=);
    a real or thresholded leaf needs an even number of planes per colour group.  If x requires grad
    the backward pass is one hbx_backward_stack on the plan for the negated depths, whose last pass
    adds the D adjoint propagations as it loads them and writes the leaf's gradient once.  grid=,
    origin= and roi= raise ValueError (focal stacks are not windowed), and so does source= (a stack is
    lit by the unit plane wave).  No double backward."""
    t, spec, squeeze = _leaf_args(x, "simulate_stack", tf, field, threshold, ste, ste_width, grid, origin, roi, levels,
                                  zs=zs, source=source)
    return _simulate(t, spec, squeeze, "simulate_stack")


def intensity_stack(x, zs, tf="asm", field="amplitude", threshold=None, ste="window", ste_width=0.5, levels=None,
                    grid=None, origin=None, roi=None, source=None) -> torch.Tensor:
    """``tt.intensity`` at every depth of `zs`: float32 [D, B, G, H, W] ([D, G, H, W] for a 3-D x), the
    arguments as simulate_stack's.  With a gradient request the per-depth fields are saved and the
    backward pass is one hbx_backward_stack with (2 / P) grad_output applied in the first passes'
    loads; without one no field is written."""
    t, spec, squeeze = _leaf_args(x, "intensity_stack", tf, field, threshold, ste, ste_width, grid, origin, roi, levels,
                                  zs=zs, source=source)
    return _intensity(t, spec, squeeze, "intensity_stack")


def loss_stack(x, target, zs, metric="mse", rel_scale="lsq", tf="asm", field="amplitude", threshold=None,
               ste="window", ste_width=0.5, levels=None, grid=None, origin=None, roi=None,
               pixel_weight=None, source=None) -> torch.Tensor:
    """``tt.loss`` over a focal stack: one value per env, float64 [B] on the device (0-dim for a 3-D
    x), of the intensities at every depth of `zs` against ``target`` float32 [D, B, G, H, W]
    ([D, G, H, W] for a 3-D x), a constant.  The sums of I T, I^2 and T^2 run over an env's D G
    channels and n = D G H W: with rel_scale="lsq" ONE least-squares scale per env for the whole
    stack (one source power), with "none" the mean of the D per-depth losses.  metric, rel_scale
    and the leaf arguments as in loss and simulate_stack.  If x requires grad the forward saves the
    per-depth fields, intensities and statistics, and the backward pass is hbx_loss_weight_stack
    followed by ONE hbx_backward_stack on the plan for the negated depths -- where D calls of
    tt.loss run D first passes forward, and D last passes and D - 1 additions of gradient-sized
    temporaries backward.  grid=, origin= and roi= raise ValueError.  No double backward.

    pixel_weight=v as in loss, of the target's shape [D, B, G, H, W] or one that broadcasts to it (e.g.
    [D, 1, G, H, W]: one weight per depth, each depth scored where its part of the scene is in focus):
    depth d's last pass takes depth d's weight (hbx_evaluate_stack_pw), and W = sum v over an env's
    D G images takes the place of n = D G H W."""
    kind = _switch(metric, _METRIC_NAMES, "metric")
    rel = _switch(rel_scale, _REL_NAMES, "rel_scale")
    t, spec, squeeze = _leaf_args(x, "loss_stack", tf, field, threshold, ste, ste_width, grid, origin, roi, levels,
                                  zs=zs, pixel_weight=pixel_weight, source=source)
    return _loss(t, target, spec, squeeze, "loss_stack", kind, rel, pixel_weight)


def relativeLoss(x: torch.Tensor, y, fn: Callable, rel_scale="lsq") -> torch.Tensor:
    """fn(s * x, y) with the least-squares scale s = sum(x y) / sum(x^2) (rel_scale="lsq",
    the default) or with s = 1 (rel_scale="none"; the hbx._lib REL_* integers are accepted
    too, an unknown value raises ValueError), all in
    float64: DBS_1024_24.py:355 compares two such PSNRs whose difference is
    ~1e-6 dB at 1024x24, below float32 resolution of the PSNR itself.

    fn = tm.get_PSNR on two same-shape GPU tensors (every PSNR call site of the reference):
    one hbx_rel_stats reduction (sum xy, sum x^2, sum y^2 in f64, fixed order) and the PSNR of
    the least-squares-scaled intensity, 10 log10(1 / ((sum y^2 - (sum xy)^2 / sum x^2) / n)),
    read from host-mapped memory after one wait -- the wait get_PSNR's float result needs
    anyway.  Other fns (F.mse_loss at env.py:131) run as torch ops."""
    rel = _switch(rel_scale, _REL_NAMES, "rel_scale")
    x = x.as_subclass(torch.Tensor) if isinstance(x, torch.Tensor) else torch.as_tensor(x)
    y = torch.as_tensor(np.asarray(y)) if not isinstance(y, torch.Tensor) else y.as_subclass(torch.Tensor)
    if fn is _metrics.get_PSNR and x.is_cuda and y.is_cuda and x.device == y.device and x.shape == y.shape \
            and x.dtype == y.dtype and x.dtype in (torch.float32, torch.float64) and x.numel() > 0:
        dev = x.device.index
        sc = _scratch(dev)
        xc, yc = x.contiguous(), y.contiguous()
        kind = _lib.SRC_F32 if x.dtype == torch.float32 else _lib.SRC_F64
        st = torch.cuda.current_stream(dev)
        rc = _lib.load().hbx_rel_stats(xc.data_ptr(), yc.data_ptr(), kind, xc.numel(), rel, 1.0,
                                       sc.work.data_ptr(), sc.out_dev, st.cuda_stream)
        if rc != _lib.OK:
            _lib.check(rc, "hbx_rel_stats")
        st.synchronize()
        _raise_pending(sc)                          # the simulate that produced x, if it was not binary
        return float(sc.out[3])
    xd, yd = x.double(), y.to(x.device).double()
    out = fn((torch.sum(xd * yd) / torch.sum(xd * xd)) * xd, yd) if rel == _lib.REL_LSQ else fn(xd, yd)
    if x.is_cuda and x.device.index in _SCRATCH and not isinstance(out, torch.Tensor):
        _raise_pending(_SCRATCH[x.device.index])    # fn waited for the device (a float result)
    return out


def imread(path: str, meta: Optional[Dict] = None, gray: bool = False) -> Tensor:
    """Image file -> tt.Tensor [1, C, H, W] in [0, 1] (Dataset512's loader, DBS_1024_24.py:191)."""
    from PIL import Image
    img = Image.open(path)
    img = img.convert("L" if gray else "RGB")
    a = np.asarray(img, dtype=np.float32) / 255.0
    a = a[None, None] if gray else np.transpose(a, (2, 0, 1))[None]
    return Tensor(torch.from_numpy(np.ascontiguousarray(a)), meta=meta)
