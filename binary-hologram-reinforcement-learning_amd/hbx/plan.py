"""Plan: one propagation configuration on one GPU (wraps hbx_plan_t).

Mirrors what ``tt.simulate(tt.Tensor(x, meta={'dx','wl'}), z)`` +
``tt.relativeLoss(.., tm.get_PSNR)`` compute in the reference
(env.py:123-133,170-174; DBS_1024_24.py:244-257,326-332), but for a whole
batch of bit-packed masks at once, entirely on the device.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers
from dataclasses import dataclass, field
from typing import Optional, Sequence

import torch

from . import _lib

PIXEL_PITCH = 7.56e-6          # env.py:124
Z_DEFAULT = 2e-3               # env.py:90
WL_MONO = (515e-9,)            # env.py:124
WL_RGB = (638e-9, 515e-9, 450e-9)   # env_1024_24.py:135-138


@dataclass
class OpticsConfig:
    height: int
    width: int
    groups: int = 1
    planes: int = 8
    wavelengths: Sequence[float] = WL_MONO
    dx: float = PIXEL_PITCH
    dy: float = PIXEL_PITCH
    z: float = Z_DEFAULT
    tf_kind: int = _lib.TF_ASM
    field_kind: int = _lib.FIELD_AMPLITUDE
    rel_scale: int = _lib.REL_LSQ
    peak: float = 1.0

    @property
    def channels(self) -> int:
        return self.groups * self.planes

    @property
    def words(self) -> int:
        return self.width // 64

    def to_c(self) -> _lib.Optics:
        o = _lib.Optics()
        o.height, o.width, o.groups, o.planes = self.height, self.width, self.groups, self.planes
        wl = list(self.wavelengths)
        if len(wl) != self.groups:
            raise ValueError(f"{len(wl)} wavelengths for {self.groups} groups")
        for i, w in enumerate(wl):
            o.wavelength[i] = float(w)
        o.dx, o.dy, o.z = float(self.dx), float(self.dy), float(self.z)
        o.tf_kind, o.field_kind, o.rel_scale = int(self.tf_kind), int(self.field_kind), int(self.rel_scale)
        o.peak = float(self.peak)
        return o


def mono_config(n: int = 256, **kw) -> OpticsConfig:
    """env.py: 1 group x 8 planes at 515 nm (IPS=256, CH=8)."""
    return OpticsConfig(n, n, 1, 8, WL_MONO, **kw)


def rgb_config(n: int = 1024, planes: int = 8, **kw) -> OpticsConfig:
    """env_1024_24.py: 3 groups x 8 planes at 638/515/450 nm (IPS=1024, CH=24)."""
    return OpticsConfig(n, n, 3, planes, WL_RGB, **kw)


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(stream: Optional[torch.cuda.Stream]):
    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


def _need(t: torch.Tensor, name: str, dtype: torch.dtype, shape, device: torch.device):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.dtype != dtype:
        raise TypeError(f"{name}: dtype {t.dtype} != {dtype}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: shape {tuple(t.shape)} != {tuple(shape)}")
    if t.device != device:
        raise ValueError(f"{name}: device {t.device} != {device}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def _batch(t, axis: int = 0) -> int:
    """The envs of an argument, its length along `axis`; 0 for what has no such axis (the _need
    that follows names the fault)."""
    return t.shape[axis] if isinstance(t, torch.Tensor) and t.dim() > axis else 0


def _complex(field: Optional[torch.Tensor]):
    return None if field is None else torch.view_as_complex(field)


_PACK_KIND = {torch.bool: _lib.SRC_U8, torch.int8: _lib.SRC_U8, torch.uint8: _lib.SRC_U8,
              torch.float32: _lib.SRC_F32, torch.float64: _lib.SRC_F64}
_PACK_ALIGN = {_lib.SRC_U8: 4, _lib.SRC_F32: 16, _lib.SRC_F64: 32}


def pack_mask(values: torch.Tensor, threshold: Optional[float] = None, out: Optional[torch.Tensor] = None,
              error_ptr: Optional[int] = None, stream=None) -> torch.Tensor:
    """Device tensor [..., H, W] -> int64 words [..., H, W/64] with ONE HIP launch
    (hbx_pack_mask, ABI v14; bit j of word w = column 64 w + j).

    threshold None: bit = (v != 0), and a value other than 0 / 1 stores 1 at `error_ptr`
    (an address the kernel may write: device or host-mapped memory) -- tt.simulate's binary
    check without a host sync.  threshold t: bit = (v >= t) -- env.py:120's `pre_model >= 0.5`.
    bool / int8 / uint8 / float32 / float64 are read as they are; other dtypes, and int8 against
    a threshold (the byte kind reads unsigned bytes), are converted to float32 on the device first.  `out`: a contiguous int64 tensor of the result's shape."""
    if not values.is_cuda:
        raise ValueError("pack_mask runs on the GPU (hbx_pack_mask); pack_bits packs host tensors")
    w = values.shape[-1]
    if w % 64:
        raise ValueError("width must be a multiple of 64")
    kind = _PACK_KIND.get(values.dtype)
    if kind is None or (threshold is not None and values.dtype == torch.int8):
        # the byte kind compares the unsigned byte: a negative int8 against a threshold goes through float32 (exact)
        values, kind = values.to(torch.float32), _lib.SRC_F32
    if not values.is_contiguous() or values.data_ptr() % _PACK_ALIGN[kind]:
        values = values.contiguous() if not values.is_contiguous() else values.clone()
    shape = (*values.shape[:-1], w // 64)
    if out is None:
        out = torch.empty(shape, dtype=torch.int64, device=values.device)
    elif tuple(out.shape) != shape or out.dtype != torch.int64 or not out.is_contiguous() \
            or out.device != values.device:
        raise ValueError(f"pack_mask out: a contiguous int64 {shape} tensor on {values.device}")
    lib = _lib.load()
    mode = _lib.PACK_BINARY if threshold is None else _lib.PACK_THRESHOLD
    s = stream.cuda_stream if stream is not None else torch._C._cuda_getCurrentRawStream(values.device.index)
    rc = lib.hbx_pack_mask(values.data_ptr(), kind, values.numel(), mode,
                           0.0 if threshold is None else float(threshold), out.data_ptr(), error_ptr, s)
    if rc != _lib.OK:
        _lib.check(rc, "hbx_pack_mask")
    return out


def _levels(levels) -> int:
    """The level count of the quantized-phase calls as an int: integral (a bool is not a count) -- its range,
    [2, 256], is the library's check (HBX_ERR_INVALID, "levels" in the message)."""
    if isinstance(levels, bool) or not isinstance(levels, numbers.Integral):
        raise TypeError(f"levels must be an integer, got {type(levels).__name__}")
    return int(levels)


def quantize_phase(x: torch.Tensor, levels: int, want_levels: bool = True, want_samples: bool = False, stream=None):
    """The phase quantizer on a device tensor, one HIP launch (hbx_quantize_phase): `x` float32 phase
    samples in units of pi, any shape.  Returns the uint8 level k mod L of every sample (what an L-level
    modulator displays: the phase 2 pi level / L) and / or the float32 quantized sample q = k * float32(2 / L)
    the `*_phase_levels` calls propagate, each of x's shape: one tensor when one is asked for, else
    (levels, samples).  Ties go to the even k; a non-finite sample gives level 0 and q = NaN."""
    if not (want_levels or want_samples):
        raise ValueError("quantize_phase: want_levels and want_samples are both off")
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
        raise TypeError("quantize_phase: x must be a float32 torch.Tensor")
    if not x.is_cuda:
        raise ValueError("quantize_phase runs on the GPU (hbx_quantize_phase)")
    levels = _levels(levels)
    x = x.contiguous().resolve_neg()
    lv = torch.empty(x.shape, dtype=torch.uint8, device=x.device) if want_levels else None
    q = torch.empty(x.shape, dtype=torch.float32, device=x.device) if want_samples else None
    lib = _lib.load()
    s = stream.cuda_stream if stream is not None else torch._C._cuda_getCurrentRawStream(x.device.index)
    with torch.cuda.device(x.device):
        _lib.check(lib.hbx_quantize_phase(_ptr(x), x.numel(), levels, _ptr(lv), _ptr(q), C.c_void_p(s)),
                   "hbx_quantize_phase")
    if want_levels and want_samples:
        return lv, q
    return lv if want_levels else q


def pack_bits(mask: torch.Tensor) -> torch.Tensor:
    """{0,1} tensor [..., H, W] -> int64 words [..., H, W/64] (bit j of word w = col 64w+j).

    GPU tensors: one hbx_pack_mask launch (bit = v != 0).  Host tensors (test fixtures,
    checkpoint tooling) are packed with torch ops on the CPU."""
    w = mask.shape[-1]
    if w % 64:
        raise ValueError("width must be a multiple of 64")
    if mask.is_cuda:
        return pack_mask(mask)
    m = (mask != 0).to(torch.int64).reshape(*mask.shape[:-1], w // 64, 64)
    shifts = torch.arange(64, device=mask.device, dtype=torch.int64)
    return (m << shifts).sum(dim=-1, dtype=torch.int64)   # bit 63 wraps into the sign: same bits


def unpack_bits(words: torch.Tensor, width: int) -> torch.Tensor:
    shifts = torch.arange(64, device=words.device, dtype=torch.int64)
    bits = (words.unsqueeze(-1) >> shifts) & 1
    return bits.reshape(*words.shape[:-1], width).to(torch.int8)


def crop(t: torch.Tensor, margin: int = 64) -> torch.Tensor:
    """Centre crop of ``margin`` pixels per side on the last two axes
    (env_1024_24_128.py:144-149, DBS_1024_24-128.py:210-216); 1024 -> 896."""
    if margin <= 0:
        return t
    return t[..., margin:-margin, margin:-margin].contiguous()


def crop_bits(words: torch.Tensor, margin: int = 64) -> torch.Tensor:
    """The same crop on packed masks [..., H, W/64]: a 64-aligned margin drops
    whole words, so this is a strided copy (no unpacking)."""
    if margin % 64:
        raise ValueError("crop_bits needs a margin that is a multiple of 64")
    k = margin // 64
    return words[..., margin:-margin, k:-k].contiguous()


def crop_config(cfg: "OpticsConfig", margin: int = 64) -> "OpticsConfig":
    """Optics of the cropped mask: same physics, N - 2 * margin pixels."""
    import dataclasses
    return dataclasses.replace(cfg, height=cfg.height - 2 * margin, width=cfg.width - 2 * margin)


class Plan:
    """hbx_plan_t owner.  ``max_jobs`` bounds the group propagations in flight
    (workspace = max_jobs * planes * N^2 * 8 bytes)."""

    def __init__(self, cfg: OpticsConfig, max_jobs: int = 8, device: Optional[int] = None,
                 precision: int = _lib.PRECISION_F32):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("hbx.Plan needs a ROCm GPU (torch.cuda.is_available() is False)")
        self.cfg = cfg
        self.device_index = torch.cuda.current_device() if device is None else int(device)
        self.device = torch.device("cuda", self.device_index)
        self.max_jobs = int(max_jobs)
        h = C.c_void_p()
        oc = cfg.to_c()
        with torch.cuda.device(self.device_index):
            _lib.check(self.lib.hbx_plan_create(C.byref(h), C.byref(oc), self.max_jobs,
                                                self.device_index), "hbx_plan_create")
        self._h = h
        # bumped by every call that changes what a launch sequence records (timing events,
        # precision variant): a captured HIP graph of this plan's launches is stale after it
        self.generation = 0
        if precision != _lib.PRECISION_F32:
            self.precision = precision

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.hbx_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def workspace_bytes(self) -> int:
        return int(self.lib.hbx_plan_workspace_bytes(self._h))

    # -- device timing of the three passes (hbx_plan_set_timing) --------------------
    def set_timing(self, capacity: int, every: int = 1):
        """Record up to `capacity` launches per pass, every `every`-th launch."""
        _lib.check(self.lib.hbx_plan_set_timing_sampled(self._h, int(capacity), int(every)),
                   "hbx_plan_set_timing_sampled")
        self.generation += 1

    def read_timing(self):
        """{pass: (total_ms, launches, jobs)} for k_rowfwd / k_col / k_rowinv (syncs)."""
        ms = (C.c_double * _lib.NUM_PASSES)()
        n = (C.c_int64 * _lib.NUM_PASSES)()
        jobs = (C.c_int64 * _lib.NUM_PASSES)()
        _lib.check(self.lib.hbx_plan_read_timing(self._h, ms, n, jobs), "hbx_plan_read_timing")
        names = _lib.PIPE_PASS_NAMES[self.pipeline]
        return {name: (ms[i], n[i], jobs[i]) for i, name in enumerate(names)}

    @property
    def precision(self) -> int:
        """hbx_plan_precision: rounding of the pass intermediates (_lib.PRECISION_*)."""
        rc = int(self.lib.hbx_plan_precision(self._h))
        if rc < 0:
            _lib.check(rc, "hbx_plan_precision")
        return rc

    @precision.setter
    def precision(self, kind: int):
        """PRECISION_F32 (the product path) or the bf16 / fp16 intermediate-storage
        numerics of SURVEY 8d cfg 5 (DBS_ratio_0.5.py fp32 vs bf16 sweep)."""
        _lib.check(self.lib.hbx_plan_set_precision(self._h, int(kind)), "hbx_plan_set_precision")
        self.generation += 1

    @property
    def pipeline(self) -> int:
        """hbx_plan_pipeline: _lib.PIPE_THREE_PASS (the only pipeline built since ABI v8)."""
        rc = int(self.lib.hbx_plan_pipeline(self._h))
        if rc < 0:
            _lib.check(rc, "hbx_plan_pipeline")
        return rc

    # -- buffer helpers -------------------------------------------------------
    def mask_shape(self, n_env: int):
        c = self.cfg
        return (n_env, c.channels, c.height, c.words)

    def target_shape(self, n_env: int):
        c = self.cfg
        return (n_env, c.groups, c.height, c.width)

    def _check_mask_target(self, mask, target, n):
        _need(mask, "mask", torch.int64, self.mask_shape(n), self.device)
        _need(target, "target", torch.float32, self.target_shape(n), self.device)

    # -- operators ---------------------------------------------------------------
    def propagate(self, mask: torch.Tensor, target: torch.Tensor, want_intensity: bool = True,
                  stream=None):
        """Full propagation of every group: returns (intensity|None, chan_stats, psnr)."""
        n = mask.shape[0]
        self._check_mask_target(mask, target, n)
        c = self.cfg
        inten = torch.empty((n, c.groups, c.height, c.width), dtype=torch.float32,
                            device=self.device) if want_intensity else None
        stats = torch.empty((n, c.groups, 3), dtype=torch.float64, device=self.device)
        psnr = torch.empty((n,), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.hbx_propagate(self._h, _ptr(mask), _ptr(target), n, _ptr(inten),
                                          _ptr(stats), _ptr(psnr), _stream(stream)), "hbx_propagate")
        return inten, stats, psnr

    def simulate(self, mask: torch.Tensor, want_intensity: bool = False, stream=None):
        """Complex field of every plane (tt.simulate restated): returns
        (field complex64 [B, CH, H, W], intensity [B, G, H, W] | None)."""
        n = mask.shape[0]
        c = self.cfg
        _need(mask, "mask", torch.int64, self.mask_shape(n), self.device)
        field = torch.empty((n, c.channels, c.height, c.width, 2), dtype=torch.float32, device=self.device)
        inten = torch.empty((n, c.groups, c.height, c.width), dtype=torch.float32,
                            device=self.device) if want_intensity else None
        _lib.check(self.lib.hbx_simulate(self._h, _ptr(mask), n, _ptr(field), _ptr(inten), _stream(stream)),
                   "hbx_simulate")
        return torch.view_as_complex(field), inten

    # -- the leaf calls: samples (real, complex, phase, thresholded) instead of bits ------------
    def _in(self, t, name: str, dtype: torch.dtype, shape, optional: bool = False):
        """_need, then the tensor whose memory the kernel may read: a lazily conjugated or negated
        view (t.conj()) shares the unresolved memory, so it is materialised (a copy only when such a
        bit is set).  optional: None passes through."""
        if optional and t is None:
            return None
        _need(t, name, dtype, shape, self.device)
        return t.resolve_conj().resolve_neg() if dtype.is_complex else t.resolve_neg()

    def _outputs(self, field_shape, image_shape, want_field: bool, want_intensity: bool, with_stats: bool):
        """The buffers of an evaluate call -> (field as float32 pairs | None, a float32 image per
        group | None, chan_stats | None, psnr | None); the last two come with a target."""
        dev = self.device
        field = torch.empty(field_shape + (2,), dtype=torch.float32, device=dev) if want_field else None
        inten = torch.empty(image_shape, dtype=torch.float32, device=dev) if want_intensity else None
        if not with_stats:
            return field, inten, None, None
        return (field, inten, torch.empty(image_shape[:2] + (3,), dtype=torch.float64, device=dev),
                torch.empty(image_shape[:1], dtype=torch.float64, device=dev))

    def values_shape(self, n: int):
        c = self.cfg
        return (n, c.channels, c.height, c.width)

    def simulate_real(self, values: torch.Tensor, want_intensity: bool = False, stream=None):
        """`simulate` on a real-valued field (hbx_simulate_real, ABI v15): `values` float32
        [B, CH, H, W] are the field samples themselves (u = value; the plan's field_kind is not
        applied).  Returns (field complex64 [B, CH, H, W], intensity [B, G, H, W] | None)."""
        n = _batch(values)
        values = self._in(values, "values", torch.float32, self.values_shape(n))
        field, inten, _, _ = self._outputs(self.values_shape(n), self.target_shape(n), True, want_intensity, False)
        _lib.check(self.lib.hbx_simulate_real(self._h, _ptr(values), n, _ptr(field), _ptr(inten),
                                              _stream(stream)), "hbx_simulate_real")
        return torch.view_as_complex(field), inten

    def simulate_complex(self, values: torch.Tensor, want_field: bool = True, want_real: bool = False,
                         weight: Optional[torch.Tensor] = None, scale: float = 1.0, stream=None):
        """`simulate` on a complex field (hbx_simulate_complex): `values` complex64
        [B, CH/2, H, W] are the field samples themselves; a plan with CH real planes carries CH/2
        complex planes.  Returns (field complex64 [B, CH/2, H, W] | None, real_part float32
        [B, CH/2, H, W] | None); real_part is field.real, written without the complex plane when
        want_field is off (the gradient of a real input: the plan for -z is the adjoint).

        weight float32 [B, G, H, W] (hbx_simulate_complex_weighted): the first pass propagates
        (scale * weight[b, g]) * values[b, c] for the complex planes c of group g, applied as it
        loads the samples -- with the saved field as values, the intensity's incoming gradient as
        weight and scale = 2 / planes this is the gradient of the plane-mean intensity.  weight
        None is hbx_simulate_complex itself (scale is then not applied)."""
        if not (want_field or want_real):
            raise ValueError("simulate_complex: want_field and want_real are both off")
        n = _batch(values)
        shape = self.phase_shape(n)
        values = self._in(values, "values", torch.complex64, shape)
        weight = self._in(weight, "weight", torch.float32, self.target_shape(n), optional=True)
        field, real, _, _ = self._outputs(shape, shape, want_field, want_real, False)
        if weight is None:
            _lib.check(self.lib.hbx_simulate_complex(self._h, _ptr(values), n, _ptr(field), _ptr(real),
                                                     _stream(stream)), "hbx_simulate_complex")
        else:
            _lib.check(self.lib.hbx_simulate_complex_weighted(self._h, _ptr(values), _ptr(weight), float(scale), n,
                                                              _ptr(field), _ptr(real), _stream(stream)),
                       "hbx_simulate_complex_weighted")
        return _complex(field), real

    def intensity_real(self, values: torch.Tensor, stream=None) -> torch.Tensor:
        """Plane-mean intensity float32 [B, G, H, W] of a real-valued field (hbx_intensity_real):
        `simulate_real(.., want_intensity=True)`'s intensity, bit for bit, with no field written."""
        n = _batch(values)
        values = self._in(values, "values", torch.float32, self.values_shape(n))
        inten = torch.empty(self.target_shape(n), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.hbx_intensity_real(self._h, _ptr(values), n, _ptr(inten), _stream(stream)),
                   "hbx_intensity_real")
        return inten

    def propagate_real(self, values: torch.Tensor, target: torch.Tensor, want_intensity: bool = True,
                       stream=None):
        """`propagate` on a real-valued field (hbx_propagate_real, ABI v15): returns
        (intensity|None, chan_stats, psnr)."""
        n = _batch(values)
        values = self._in(values, "values", torch.float32, self.values_shape(n))
        _need(target, "target", torch.float32, self.target_shape(n), self.device)
        _, inten, stats, psnr = self._outputs(None, self.target_shape(n), False, want_intensity, True)
        _lib.check(self.lib.hbx_propagate_real(self._h, _ptr(values), _ptr(target), n, _ptr(inten),
                                               _ptr(stats), _ptr(psnr), _stream(stream)), "hbx_propagate_real")
        return inten, stats, psnr

    def evaluate_real(self, values: torch.Tensor, target: torch.Tensor, want_field: bool = True,
                      want_intensity: bool = True, stream=None):
        """`propagate_real` that may also write `simulate_real`'s field, in one launch set
        (hbx_evaluate_real): returns (field complex64 [B, CH, H, W] | None, intensity | None,
        chan_stats, psnr), each bit for bit what those two calls give."""
        n = _batch(values)
        values = self._in(values, "values", torch.float32, self.values_shape(n))
        _need(target, "target", torch.float32, self.target_shape(n), self.device)
        field, inten, stats, psnr = self._outputs(self.values_shape(n), self.target_shape(n), want_field,
                                                  want_intensity, True)
        _lib.check(self.lib.hbx_evaluate_real(self._h, _ptr(values), _ptr(target), n, _ptr(field), _ptr(inten),
                                              _ptr(stats), _ptr(psnr), _stream(stream)), "hbx_evaluate_real")
        return _complex(field), inten, stats, psnr

    def evaluate_complex(self, values: torch.Tensor, target: Optional[torch.Tensor] = None, want_field: bool = True,
                         want_intensity: bool = True, stream=None):
        """A complex field's propagation with the plane-mean intensity and the statistics from the
        same last pass (hbx_evaluate_complex): `values` complex64 [B, CH/2, H, W] as
        `simulate_complex`; returns (field complex64 [B, CH/2, H, W] | None, intensity float32
        [B, G, H, W] | None, chan_stats | None, psnr | None).  intensity[b, g] is the mean of
        |field|^2 over the group's CH/2G complex planes; the field is `simulate_complex`'s bit for
        bit.  target None: the intensity alone (no statistics, no psnr)."""
        n = _batch(values)
        shape = self.phase_shape(n)
        values = self._in(values, "values", torch.complex64, shape)
        if target is None:
            if not want_intensity:
                raise ValueError("evaluate_complex: without a target the intensity is the only output")
        else:
            _need(target, "target", torch.float32, self.target_shape(n), self.device)
        field, inten, stats, psnr = self._outputs(shape, self.target_shape(n), want_field, want_intensity,
                                                  target is not None)
        _lib.check(self.lib.hbx_evaluate_complex(self._h, _ptr(values), _ptr(target), n, _ptr(field), _ptr(inten),
                                                 _ptr(stats), _ptr(psnr), _stream(stream)), "hbx_evaluate_complex")
        return _complex(field), inten, stats, psnr

    def phase_shape(self, n: int):
        c = self.cfg
        return (n, c.channels // 2, c.height, c.width)

    def simulate_phase(self, phase: torch.Tensor, want_field: bool = True, want_real: bool = False, stream=None):
        """`simulate_complex` of u = exp(i pi phase) (hbx_simulate_phase): `phase` float32
        [B, CH/2, H, W]; the first pass forms (cos, sin) as it loads the samples, with the argument
        reduced exactly.  Returns (field complex64 [B, CH/2, H, W] | None, real_part | None)."""
        if not (want_field or want_real):
            raise ValueError("simulate_phase: want_field and want_real are both off")
        n = _batch(phase)
        shape = self.phase_shape(n)
        phase = self._in(phase, "phase", torch.float32, shape)
        field, real, _, _ = self._outputs(shape, shape, want_field, want_real, False)
        _lib.check(self.lib.hbx_simulate_phase(self._h, _ptr(phase), n, _ptr(field), _ptr(real), _stream(stream)),
                   "hbx_simulate_phase")
        return _complex(field), real

    def evaluate_phase(self, phase: torch.Tensor, target: Optional[torch.Tensor] = None, want_field: bool = True,
                       want_intensity: bool = True, stream=None):
        """`evaluate_complex` of u = exp(i pi phase) (hbx_evaluate_phase): `phase` float32
        [B, CH/2, H, W] as `simulate_phase`; returns (field | None, intensity | None, chan_stats |
        None, psnr | None) as `evaluate_complex`, the field `simulate_phase`'s bit for bit.  target
        None: the intensity alone."""
        n = _batch(phase)
        shape = self.phase_shape(n)
        phase = self._in(phase, "phase", torch.float32, shape)
        if target is None:
            if not want_intensity:
                raise ValueError("evaluate_phase: without a target the intensity is the only output")
        else:
            _need(target, "target", torch.float32, self.target_shape(n), self.device)
        field, inten, stats, psnr = self._outputs(shape, self.target_shape(n), want_field, want_intensity,
                                                  target is not None)
        _lib.check(self.lib.hbx_evaluate_phase(self._h, _ptr(phase), _ptr(target), n, _ptr(field), _ptr(inten),
                                               _ptr(stats), _ptr(psnr), _stream(stream)), "hbx_evaluate_phase")
        return _complex(field), inten, stats, psnr

    def phase_backward(self, values: torch.Tensor, phase: torch.Tensor, weight: Optional[torch.Tensor] = None,
                       scale: float = 1.0, stream=None) -> torch.Tensor:
        """The backward pass of a phase leaf, on the plan for -z (hbx_phase_backward): `values`
        complex64 [B, CH/2, H, W] and `weight` / `scale` are `simulate_complex`'s (weight None: the
        samples as they are), `phase` float32 [B, CH/2, H, W] the leaf's samples x.  Returns
        float32 [B, CH/2, H, W] = pi (Im g cos pi x - Re g sin pi x), g the field `simulate_complex`
        would return -- which is not written.  With the saved field as values, the loss's or the
        intensity's incoming gradient as weight and scale = 2 / planes this is dL/dx."""
        n = _batch(values)
        shape = self.phase_shape(n)
        values = self._in(values, "values", torch.complex64, shape)
        phase = self._in(phase, "phase", torch.float32, shape)
        weight = self._in(weight, "weight", torch.float32, self.target_shape(n), optional=True)
        grad = torch.empty(shape, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.hbx_phase_backward(self._h, _ptr(values), _ptr(weight), float(scale), _ptr(phase), n,
                                               _ptr(grad), _stream(stream)), "hbx_phase_backward")
        return grad

    def simulate_phase_levels(self, phase: torch.Tensor, levels: int, want_field: bool = True, want_real: bool = False,
                              stream=None):
        """`simulate_phase` of the hologram an L-level modulator displays (hbx_simulate_phase_levels):
        the first pass quantizes each sample to the nearest of `levels` phase levels (2 <= levels <= 256,
        `quantize_phase`'s q) as it loads it; q is never written.  Every output equals
        `simulate_phase(quantize_phase(phase, levels, False, True))`'s bit for bit."""
        if not (want_field or want_real):
            raise ValueError("simulate_phase_levels: want_field and want_real are both off")
        levels = _levels(levels)
        n = _batch(phase)
        shape = self.phase_shape(n)
        phase = self._in(phase, "phase", torch.float32, shape)
        field, real, _, _ = self._outputs(shape, shape, want_field, want_real, False)
        _lib.check(self.lib.hbx_simulate_phase_levels(self._h, _ptr(phase), levels, n, _ptr(field), _ptr(real),
                                                      _stream(stream)), "hbx_simulate_phase_levels")
        return _complex(field), real

    def evaluate_phase_levels(self, phase: torch.Tensor, levels: int, target: Optional[torch.Tensor] = None,
                              want_field: bool = True, want_intensity: bool = True, stream=None):
        """`evaluate_phase` with `simulate_phase_levels`'s quantizing first pass
        (hbx_evaluate_phase_levels): the same returns, each `evaluate_phase`'s on the quantized samples
        bit for bit."""
        levels = _levels(levels)
        n = _batch(phase)
        shape = self.phase_shape(n)
        phase = self._in(phase, "phase", torch.float32, shape)
        if target is None:
            if not want_intensity:
                raise ValueError("evaluate_phase_levels: without a target the intensity is the only output")
        else:
            _need(target, "target", torch.float32, self.target_shape(n), self.device)
        field, inten, stats, psnr = self._outputs(shape, self.target_shape(n), want_field, want_intensity,
                                                  target is not None)
        _lib.check(self.lib.hbx_evaluate_phase_levels(self._h, _ptr(phase), levels, _ptr(target), n, _ptr(field),
                                                      _ptr(inten), _ptr(stats), _ptr(psnr), _stream(stream)),
                   "hbx_evaluate_phase_levels")
        return _complex(field), inten, stats, psnr

    def phase_levels_backward(self, values: torch.Tensor, phase: torch.Tensor, levels: int,
                              weight: Optional[torch.Tensor] = None, scale: float = 1.0, stream=None) -> torch.Tensor:
        """The backward pass of a quantized phase leaf under the straight-through estimator, on the
        plan for -z (hbx_phase_levels_backward): `phase_backward` with the last pass quantizing the
        leaf's samples as `simulate_phase_levels` does, pi (Im g cos pi q - Re g sin pi q) -- dq/dx := 1.
        Equals `phase_backward(values, quantize_phase(phase, levels, False, True), weight, scale)` bit
        for bit."""
        levels = _levels(levels)
        n = _batch(values)
        shape = self.phase_shape(n)
        values = self._in(values, "values", torch.complex64, shape)
        phase = self._in(phase, "phase", torch.float32, shape)
        weight = self._in(weight, "weight", torch.float32, self.target_shape(n), optional=True)
        grad = torch.empty(shape, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.hbx_phase_levels_backward(self._h, _ptr(values), _ptr(weight), float(scale), _ptr(phase),
                                                      levels, n, _ptr(grad), _stream(stream)),
                   "hbx_phase_levels_backward")
        return grad

    def evaluate_threshold(self, values: torch.Tensor, threshold: float, target: Optional[torch.Tensor] = None,
                           want_field: bool = True, want_intensity: bool = True, stream=None):
        """`evaluate_real` of the binary hologram m = [values >= threshold], u = va + vb m with the
        plan's field_kind (hbx_evaluate_threshold): `values` float32 [B, CH, H, W] is the real leaf;
        the first pass thresholds it as it loads it and no 0 / 1 copy is written.  Returns (field
        complex64 [B, CH, H, W] | None, intensity | None, chan_stats | None, psnr | None), each
        `evaluate_real`'s on the materialised samples bit for bit; chan_stats and psnr come with a
        target.  At least one of want_field, want_intensity and target is needed."""
        n = _batch(values)
        values = self._in(values, "values", torch.float32, self.values_shape(n))
        if target is not None:
            _need(target, "target", torch.float32, self.target_shape(n), self.device)
        elif not (want_field or want_intensity):
            raise ValueError("evaluate_threshold: no target, and want_field and want_intensity are both off")
        field, inten, stats, psnr = self._outputs(self.values_shape(n), self.target_shape(n), want_field, want_intensity,
                                                  target is not None)
        _lib.check(self.lib.hbx_evaluate_threshold(self._h, _ptr(values), float(threshold), _ptr(target), n,
                                                   _ptr(field), _ptr(inten), _ptr(stats), _ptr(psnr),
                                                   _stream(stream)), "hbx_evaluate_threshold")
        return _complex(field), inten, stats, psnr

    def threshold_backward(self, values: torch.Tensor, samples: torch.Tensor, weight: Optional[torch.Tensor] = None,
                           scale: float = 1.0, surrogate: int = _lib.STE_WINDOW, p0: float = -math.inf,
                           p1: float = math.inf, stream=None) -> torch.Tensor:
        """The backward pass of a binary hologram's real leaf under the straight-through estimator,
        on the plan for -z (hbx_threshold_backward): `values` complex64 [B, CH/2, H, W] and `weight`
        / `scale` are `phase_backward`'s, `samples` float32 [B, CH/2, H, W] the leaf's samples x
        (real plane q of the leaf is complex plane q here).  Returns float32 [B, CH/2, H, W] =
        vb s(x) Re g, vb this plan's (1 or -2) and g the field `simulate_complex` would return --
        which is not written.  STE_WINDOW: s = [p0 <= x <= p1] (the default is the plain estimator);
        STE_SIGMOID: s = k sg (1 - sg), sg = sigmoid(k (x - p0)), k = p1 > 0."""
        n = _batch(values)
        shape = self.phase_shape(n)
        values = self._in(values, "values", torch.complex64, shape)
        samples = self._in(samples, "samples", torch.float32, shape)
        weight = self._in(weight, "weight", torch.float32, self.target_shape(n), optional=True)
        grad = torch.empty(shape, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.hbx_threshold_backward(self._h, _ptr(values), _ptr(weight), float(scale), _ptr(samples),
                                                   int(surrogate), float(p0), float(p1), n, _ptr(grad),
                                                   _stream(stream)), "hbx_threshold_backward")
        return grad

    def loss(self, chan_stats: torch.Tensor, kind: int = _lib.LOSS_MSE, rel_scale: int = _lib.REL_LSQ,
             stream=None) -> torch.Tensor:
        """chan_stats [B, G, 3] -> the relative MSE or PSNR per env, float64 [B] on the device
        (hbx_loss): tt.relativeLoss(.., F.mse_loss / tm.get_PSNR) without the host wait."""
        n = _batch(chan_stats)
        _need(chan_stats, "chan_stats", torch.float64, (n, self.cfg.groups, 3), self.device)
        out = torch.empty((n,), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.hbx_loss(self._h, _ptr(chan_stats), n, int(kind), int(rel_scale), _ptr(out),
                                     _stream(stream)), "hbx_loss")
        return out

    def loss_weight(self, intensity: torch.Tensor, target: torch.Tensor, chan_stats: torch.Tensor,
                    grad_loss: Optional[torch.Tensor] = None, kind: int = _lib.LOSS_MSE,
                    rel_scale: int = _lib.REL_LSQ, stream=None) -> torch.Tensor:
        """The loss's gradient with respect to the intensity, float32 [B, G, H, W]
        (hbx_loss_weight): grad_loss[b] * d loss_b / d intensity[b] = a_b I + c_b T; grad_loss
        float64 [B] or None (ones).  `simulate_complex(field, weight=.., scale=2 / planes)` on the
        plan for -z turns it into the gradient with respect to the hologram."""
        n = _batch(intensity)
        _need(intensity, "intensity", torch.float32, self.target_shape(n), self.device)
        _need(target, "target", torch.float32, self.target_shape(n), self.device)
        _need(chan_stats, "chan_stats", torch.float64, (n, self.cfg.groups, 3), self.device)
        if grad_loss is not None:
            _need(grad_loss, "grad_loss", torch.float64, (n,), self.device)
        weight = torch.empty(self.target_shape(n), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.hbx_loss_weight(self._h, _ptr(intensity), _ptr(target), _ptr(chan_stats),
                                            _ptr(grad_loss), n, int(kind), int(rel_scale), _ptr(weight),
                                            _stream(stream)), "hbx_loss_weight")
        return weight

    # --- focal stacks (hbx_*_stack): one hologram at D depths, depth-major arrays [D, B, ...] ---
    def set_depths(self, zs):
        """The depths of this plan's focal stack (hbx_plan_set_depths): a sequence of 1 to 8 finite
        distances, or an empty one to free the tables.  Depth d's transfer-function table is that of
        a plan created with z = zs[d], bit for bit; the plan's own z and every other call are
        untouched.  Synchronises; not for use with work of this plan in flight."""
        zs = tuple(float(v) for v in zs)
        if len(zs) > _lib.MAX_DEPTHS:
            raise ValueError(f"set_depths: at most {_lib.MAX_DEPTHS} depths, got {len(zs)}")
        if not all(math.isfinite(v) for v in zs):
            raise ValueError(f"set_depths: every depth must be finite, got {zs!r}")
        arr = (C.c_double * max(len(zs), 1))(*zs)
        with torch.cuda.device(self.device_index):
            _lib.check(self.lib.hbx_plan_set_depths(self._h, arr, len(zs)), "hbx_plan_set_depths")
        self.generation += 1

    @property
    def depths(self) -> int:
        """hbx_plan_depths: the number of depths set (0: none)."""
        rc = int(self.lib.hbx_plan_depths(self._h))
        if rc < 0:
            _lib.check(rc, "hbx_plan_depths")
        return rc

    def _leaf(self, kind: int, levels=None, threshold: float = 0.0, surrogate: int = _lib.STE_WINDOW,
              p0: float = -math.inf, p1: float = math.inf) -> _lib.Leaf:
        if kind not in (_lib.LEAF_REAL, _lib.LEAF_THRESHOLD, _lib.LEAF_COMPLEX, _lib.LEAF_PHASE, _lib.LEAF_PHASE_LEVELS):
            raise ValueError(f"leaf kind must be one of hbx._lib.LEAF_*, got {kind!r}")
        lv = _levels(levels) if kind == _lib.LEAF_PHASE_LEVELS else 0
        return _lib.Leaf(int(kind), lv, float(threshold), int(surrogate), float(p0), float(p1))

    def evaluate_stack(self, values: torch.Tensor, kind: int, target: Optional[torch.Tensor] = None,
                       want_field: bool = True, want_intensity: bool = True, levels=None, threshold: float = 0.0,
                       stream=None):
        """The single-depth evaluate call of leaf kind `kind` (hbx._lib.LEAF_*) at every depth of the
        stack, with the first pass run once (hbx_evaluate_stack).  `values` as that call takes them
        ([B, CH, H, W] float32 for LEAF_REAL / LEAF_THRESHOLD, [B, CH/2, H, W] complex64 for
        LEAF_COMPLEX, float32 for the phase kinds); `target` float32 [D, B, G, H, W] or None.
        Returns (field complex64 [D, B, C, H, W] | None, intensity float32 [D, B, G, H, W] | None,
        chan_stats float64 [D, B, G, 3] | None); depth d of each equals the single-depth call's on a
        plan for zs[d] bit for bit."""
        leaf = self._leaf(kind, levels, threshold)
        n = _batch(values)
        c = self.cfg
        d = self.depths
        real_in = kind in (_lib.LEAF_REAL, _lib.LEAF_THRESHOLD)
        planes = c.channels if real_in else c.channels // 2
        shape = (n, planes, c.height, c.width)
        values = self._in(values, "values", torch.complex64 if kind == _lib.LEAF_COMPLEX else torch.float32, shape)
        tshape = (d,) + tuple(self.target_shape(n))
        if target is not None:
            _need(target, "target", torch.float32, tshape, self.device)
        elif not want_intensity and not (real_in and want_field):
            raise ValueError("evaluate_stack: no target, and nothing else asked for that the call can write alone")
        field = torch.empty((d,) + shape + (2,), dtype=torch.float32, device=self.device) if want_field else None
        inten = torch.empty(tshape, dtype=torch.float32, device=self.device) if want_intensity else None
        stats = torch.empty((d, n, c.groups, 3), dtype=torch.float64, device=self.device) if target is not None else None
        _lib.check(self.lib.hbx_evaluate_stack(self._h, _ptr(values), C.byref(leaf), _ptr(target), n, _ptr(field),
                                               _ptr(inten), _ptr(stats), _stream(stream)), "hbx_evaluate_stack")
        return _complex(field), inten, stats

    def backward_stack(self, values: torch.Tensor, kind: int, samples: Optional[torch.Tensor] = None,
                       weight: Optional[torch.Tensor] = None, scale: float = 1.0, levels=None,
                       surrogate: int = _lib.STE_WINDOW, p0: float = -math.inf, p1: float = math.inf,
                       stream=None) -> torch.Tensor:
        """The backward pass of a leaf under a loss over the stack, on the plan whose depths are the
        negated ones (hbx_backward_stack): `values` complex64 [D, B, CH/2, H, W] (per depth the
        gradient with respect to the field or, with `weight` float32 [D, B, G, H, W], the saved
        field), one depth-summing last pass, and the one output without a depth: complex64
        [B, CH/2, H, W] for LEAF_COMPLEX, else float32 [B, CH/2, H, W] -- the real part (LEAF_REAL),
        `phase_backward`'s, `phase_levels_backward`'s or `threshold_backward`'s gradient of the
        summed field, from `samples` float32 [B, CH/2, H, W] (the leaf's x) as those calls use it."""
        leaf = self._leaf(kind, levels, 0.0, surrogate, p0, p1)
        n = _batch(values, 1)
        d = self.depths
        shape = self.phase_shape(n)
        values = self._in(values, "values", torch.complex64, (d,) + tuple(shape))
        needs = kind in (_lib.LEAF_PHASE, _lib.LEAF_PHASE_LEVELS, _lib.LEAF_THRESHOLD)
        if needs != (samples is not None):
            raise ValueError("backward_stack: samples are the leaf of a phase, L-level or thresholded leaf, else None")
        samples = self._in(samples, "samples", torch.float32, shape, optional=True)
        weight = self._in(weight, "weight", torch.float32, (d,) + tuple(self.target_shape(n)), optional=True)
        cplx = kind == _lib.LEAF_COMPLEX
        out = torch.empty(tuple(shape) + ((2,) if cplx else ()), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.hbx_backward_stack(self._h, _ptr(values), _ptr(weight), float(scale), C.byref(leaf),
                                               _ptr(samples), n, _ptr(out) if cplx else None,
                                               None if cplx else _ptr(out), _stream(stream)), "hbx_backward_stack")
        return torch.view_as_complex(out) if cplx else out

    def loss_stack(self, chan_stats: torch.Tensor, kind: int = _lib.LOSS_MSE, rel_scale: int = _lib.REL_LSQ,
                   stream=None) -> torch.Tensor:
        """chan_stats [D, B, G, 3] -> `loss` per env over the whole stack, float64 [B] (hbx_loss_stack):
        the sums run over an env's D G channels, n = D G H W, one least-squares scale per env."""
        n = _batch(chan_stats, 1)
        _need(chan_stats, "chan_stats", torch.float64, (self.depths, n, self.cfg.groups, 3), self.device)
        out = torch.empty((n,), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.hbx_loss_stack(self._h, _ptr(chan_stats), n, int(kind), int(rel_scale), _ptr(out),
                                           _stream(stream)), "hbx_loss_stack")
        return out

    def loss_weight_stack(self, intensity: torch.Tensor, target: torch.Tensor, chan_stats: torch.Tensor,
                          grad_loss: Optional[torch.Tensor] = None, kind: int = _lib.LOSS_MSE,
                          rel_scale: int = _lib.REL_LSQ, stream=None) -> torch.Tensor:
        """`loss_stack`'s gradient with respect to the intensity, float32 [D, B, G, H, W]
        (hbx_loss_weight_stack): grad_loss[b] * d loss_b / d intensity[:, b] = a_b I + c_b T, one
        (a_b, c_b) per env for all depths; grad_loss float64 [B] or None (ones)."""
        n = _batch(intensity, 1)
        d = self.depths
        tshape = (d,) + tuple(self.target_shape(n))
        _need(intensity, "intensity", torch.float32, tshape, self.device)
        _need(target, "target", torch.float32, tshape, self.device)
        _need(chan_stats, "chan_stats", torch.float64, (d, n, self.cfg.groups, 3), self.device)
        if grad_loss is not None:
            _need(grad_loss, "grad_loss", torch.float64, (n,), self.device)
        weight = torch.empty(tshape, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.hbx_loss_weight_stack(self._h, _ptr(intensity), _ptr(target), _ptr(chan_stats),
                                                  _ptr(grad_loss), n, int(kind), int(rel_scale), _ptr(weight),
                                                  _stream(stream)), "hbx_loss_weight_stack")
        return weight

    # --- per-pixel loss weights (hbx_*_pw): a constant weight v of the target's shape in the statistics ---
    def _evaluate_pw(self, name, values, kind, target, pixel_weight, want_field, want_intensity, levels, threshold,
                     depths, stream):
        leaf = self._leaf(kind, levels, threshold)
        n = _batch(values)
        c = self.cfg
        real_in = kind in (_lib.LEAF_REAL, _lib.LEAF_THRESHOLD)
        shape = (n, c.channels if real_in else c.channels // 2, c.height, c.width)
        values = self._in(values, "values", torch.complex64 if kind == _lib.LEAF_COMPLEX else torch.float32, shape)
        tshape = depths + tuple(self.target_shape(n))
        _need(target, "target", torch.float32, tshape, self.device)
        _need(pixel_weight, "pixel_weight", torch.float32, tshape, self.device)
        field = torch.empty(depths + shape + (2,), dtype=torch.float32, device=self.device) if want_field else None
        inten = torch.empty(tshape, dtype=torch.float32, device=self.device) if want_intensity else None
        stats = torch.empty(depths + (n, c.groups, 3), dtype=torch.float64, device=self.device)
        _lib.check(getattr(self.lib, name)(self._h, _ptr(values), C.byref(leaf), _ptr(target), _ptr(pixel_weight), n,
                                           _ptr(field), _ptr(inten), _ptr(stats), _stream(stream)), name)
        return _complex(field), inten, stats

    def evaluate_pw(self, values: torch.Tensor, kind: int, target: torch.Tensor, pixel_weight: torch.Tensor,
                    want_field: bool = True, want_intensity: bool = True, levels=None, threshold: float = 0.0,
                    stream=None):
        """The single-depth evaluate call of leaf kind `kind` (hbx._lib.LEAF_*; `values`, `levels` and
        `threshold` as `evaluate_stack` takes them) with a per-pixel loss weight (hbx_evaluate_pw):
        `pixel_weight` float32 [B, G, H, W], non-negative, enters the statistics only -- chan_stats
        [B, G, 3] = (sum v I T, sum v I^2, sum v T^2) per group.  Returns (field | None, intensity |
        None, chan_stats); field and intensity are the unweighted call's bit for bit, and with
        pixel_weight = 1 so is chan_stats.  `target` is required."""
        return self._evaluate_pw("hbx_evaluate_pw", values, kind, target, pixel_weight, want_field, want_intensity,
                                 levels, threshold, (), stream)

    def evaluate_stack_pw(self, values: torch.Tensor, kind: int, target: torch.Tensor, pixel_weight: torch.Tensor,
                          want_field: bool = True, want_intensity: bool = True, levels=None, threshold: float = 0.0,
                          stream=None):
        """`evaluate_stack` with a per-pixel loss weight per depth (hbx_evaluate_stack_pw): `target` and
        `pixel_weight` float32 [D, B, G, H, W], both required.  Returns (field | None, intensity | None,
        chan_stats [D, B, G, 3]); depth d of each equals `evaluate_pw`'s on a plan for zs[d]."""
        return self._evaluate_pw("hbx_evaluate_stack_pw", values, kind, target, pixel_weight, want_field,
                                 want_intensity, levels, threshold, (self.depths,), stream)

    # --- illumination fields (hbx_*_source): a constant complex source [G, H, W] lights the modulator ---
    # Every leaf kind is one complex plane per leaf plane here: values [B, CH/2, H, W], the real and the
    # thresholded kind included.  Out of scope: the bit path and every env, DBS, plane-cache and incremental
    # entry point, windows, focal stacks, a gradient with respect to the source, reduced-precision plans, a
    # per-env or per-plane source, grids other than the four built.
    def _source_args(self, values, kind, source, levels, threshold, surrogate=_lib.STE_WINDOW, p0=-math.inf,
                     p1=math.inf):
        leaf = self._leaf(kind, levels, threshold, surrogate, p0, p1)
        n = _batch(values)
        shape = self.phase_shape(n)
        c = self.cfg
        source = self._in(source, "source", torch.complex64, (c.groups, c.height, c.width))
        return leaf, n, shape, source

    def source_field(self, values: torch.Tensor, kind: int, source: torch.Tensor, levels=None,
                     threshold: float = 0.0, stream=None) -> torch.Tensor:
        """The field at the modulator under the illumination `source` (hbx_source_field): u = s f(x),
        complex64 [B, CH/2, H, W], f the map of leaf kind `kind` (hbx._lib.LEAF_*), formed by the device
        functions `evaluate_source`'s first pass uses.  `values` [B, CH/2, H, W]: complex64 for
        LEAF_COMPLEX, float32 otherwise; `source` complex64 [G, H, W] on the plan's device."""
        leaf, n, shape, source = self._source_args(values, kind, source, levels, threshold)
        values = self._in(values, "values", torch.complex64 if kind == _lib.LEAF_COMPLEX else torch.float32, shape)
        out = torch.empty(tuple(shape) + (2,), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.hbx_source_field(self._h, _ptr(values), C.byref(leaf), _ptr(source), n, _ptr(out),
                                             _stream(stream)), "hbx_source_field")
        return torch.view_as_complex(out)

    def evaluate_source(self, values: torch.Tensor, kind: int, source: torch.Tensor,
                        target: Optional[torch.Tensor] = None, pixel_weight: Optional[torch.Tensor] = None,
                        want_field: bool = True, want_intensity: bool = True, levels=None, threshold: float = 0.0,
                        stream=None):
        """`evaluate_complex` of the sourced field without writing it (hbx_evaluate_source): the first pass
        forms u = s f(x) as it loads `values` and the source row.  Returns (field complex64
        [B, CH/2, H, W] | None, intensity float32 [B, G, H, W] | None, chan_stats float64 [B, G, 3] |
        None), each equal to `evaluate_complex`'s (with `pixel_weight`: `evaluate_pw`'s) on
        `source_field`'s output bit for bit.  `pixel_weight` needs a `target`."""
        leaf, n, shape, source = self._source_args(values, kind, source, levels, threshold)
        values = self._in(values, "values", torch.complex64 if kind == _lib.LEAF_COMPLEX else torch.float32, shape)
        tshape = tuple(self.target_shape(n))
        if target is not None:
            _need(target, "target", torch.float32, tshape, self.device)
        elif pixel_weight is not None:
            raise ValueError("evaluate_source: a pixel_weight needs a target")
        elif not want_intensity:
            raise ValueError("evaluate_source: without a target the intensity is the output")
        if pixel_weight is not None:
            _need(pixel_weight, "pixel_weight", torch.float32, tshape, self.device)
        field = torch.empty(tuple(shape) + (2,), dtype=torch.float32, device=self.device) if want_field else None
        inten = torch.empty(tshape, dtype=torch.float32, device=self.device) if want_intensity else None
        stats = torch.empty((n, self.cfg.groups, 3), dtype=torch.float64, device=self.device) if target is not None else None
        _lib.check(self.lib.hbx_evaluate_source(self._h, _ptr(values), C.byref(leaf), _ptr(source), _ptr(target),
                                                _ptr(pixel_weight), n, _ptr(field), _ptr(inten), _ptr(stats),
                                                _stream(stream)), "hbx_evaluate_source")
        return _complex(field), inten, stats

    def backward_source(self, values: torch.Tensor, kind: int, source: torch.Tensor,
                        samples: Optional[torch.Tensor] = None, weight: Optional[torch.Tensor] = None,
                        scale: float = 1.0, levels=None, surrogate: int = _lib.STE_WINDOW, p0: float = -math.inf,
                        p1: float = math.inf, stream=None) -> torch.Tensor:
        """The backward pass of a sourced leaf, on the plan for -z (hbx_backward_source): `values`
        complex64 [B, CH/2, H, W] (the gradient with respect to the propagated field or, with `weight`
        float32 [B, G, H, W], the saved field), back-propagated, times conj(source), then the leaf's
        formula: complex64 [B, CH/2, H, W] for LEAF_COMPLEX, else float32 -- the real part
        (LEAF_REAL), `phase_backward`'s, `phase_levels_backward`'s or `threshold_backward`'s gradient
        from `samples` float32 [B, CH/2, H, W] (the leaf's x).  The source has no gradient."""
        leaf, n, shape, source = self._source_args(values, kind, source, levels, 0.0, surrogate, p0, p1)
        values = self._in(values, "values", torch.complex64, shape)
        needs = kind in (_lib.LEAF_PHASE, _lib.LEAF_PHASE_LEVELS, _lib.LEAF_THRESHOLD)
        if needs != (samples is not None):
            raise ValueError("backward_source: samples are the leaf of a phase, L-level or thresholded leaf, else None")
        samples = self._in(samples, "samples", torch.float32, shape, optional=True)
        weight = self._in(weight, "weight", torch.float32, self.target_shape(n), optional=True)
        cplx = kind == _lib.LEAF_COMPLEX
        out = torch.empty(tuple(shape) + ((2,) if cplx else ()), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.hbx_backward_source(self._h, _ptr(values), _ptr(weight), float(scale), C.byref(leaf),
                                                _ptr(source), _ptr(samples), n, _ptr(out) if cplx else None,
                                                None if cplx else _ptr(out), _stream(stream)), "hbx_backward_source")
        return torch.view_as_complex(out) if cplx else out

    def _pw_depths(self, stack: bool):
        return ((self.depths,), self.depths, 1) if stack else ((), 0, 0)

    def pixel_weight_sum(self, pixel_weight: torch.Tensor, stack: bool = False, stream=None) -> torch.Tensor:
        """W[b] = the sum of env b's pixel weights, float64 [B] on the device (hbx_pixel_weight_sum):
        over [B, G, H, W], or with stack=True over [D, B, G, H, W] (D the plan's).  A fixed-order
        float64 reduction: bitwise reproducible, and exact for a 0 / 1 weight."""
        depths, d, axis = self._pw_depths(stack)
        n = _batch(pixel_weight, axis)
        _need(pixel_weight, "pixel_weight", torch.float32, depths + tuple(self.target_shape(n)), self.device)
        out = torch.empty((n,), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.hbx_pixel_weight_sum(self._h, _ptr(pixel_weight), n, d, _ptr(out), _stream(stream)),
                   "hbx_pixel_weight_sum")
        return out

    def loss_pw(self, chan_stats: torch.Tensor, weight_sum: torch.Tensor, kind: int = _lib.LOSS_MSE,
                rel_scale: int = _lib.REL_LSQ, stack: bool = False, stream=None) -> torch.Tensor:
        """`loss` (stack=True: `loss_stack`) on weighted statistics, with weight_sum float64 [B]
        (`pixel_weight_sum`) in the place of the pixel count (hbx_loss_pw).  An env whose weights are
        all zero gives MSE 0 / PSNR +inf."""
        depths, d, axis = self._pw_depths(stack)
        n = _batch(chan_stats, axis)
        _need(chan_stats, "chan_stats", torch.float64, depths + (n, self.cfg.groups, 3), self.device)
        _need(weight_sum, "weight_sum", torch.float64, (n,), self.device)
        out = torch.empty((n,), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.hbx_loss_pw(self._h, _ptr(chan_stats), _ptr(weight_sum), n, d, int(kind), int(rel_scale),
                                        _ptr(out), _stream(stream)), "hbx_loss_pw")
        return out

    def loss_weight_pw(self, intensity: torch.Tensor, target: torch.Tensor, pixel_weight: torch.Tensor,
                       chan_stats: torch.Tensor, weight_sum: torch.Tensor, grad_loss: Optional[torch.Tensor] = None,
                       kind: int = _lib.LOSS_MSE, rel_scale: int = _lib.REL_LSQ, stack: bool = False,
                       stream=None) -> torch.Tensor:
        """The weighted loss's gradient with respect to the intensity (hbx_loss_weight_pw): float32 of
        the intensity's shape, grad_loss[b] * pixel_weight * (a_b I + c_b T) with `loss_weight`'s
        (stack=True: `loss_weight_stack`'s) coefficients, weight_sum for the pixel count.  It goes into
        the backward calls as the unweighted loss weight does."""
        depths, d, axis = self._pw_depths(stack)
        n = _batch(intensity, axis)
        tshape = depths + tuple(self.target_shape(n))
        _need(intensity, "intensity", torch.float32, tshape, self.device)
        _need(target, "target", torch.float32, tshape, self.device)
        _need(pixel_weight, "pixel_weight", torch.float32, tshape, self.device)
        _need(chan_stats, "chan_stats", torch.float64, depths + (n, self.cfg.groups, 3), self.device)
        _need(weight_sum, "weight_sum", torch.float64, (n,), self.device)
        if grad_loss is not None:
            _need(grad_loss, "grad_loss", torch.float64, (n,), self.device)
        weight = torch.empty(tshape, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.hbx_loss_weight_pw(self._h, _ptr(intensity), _ptr(target), _ptr(pixel_weight),
                                               _ptr(chan_stats), _ptr(weight_sum), _ptr(grad_loss), n, d, int(kind),
                                               int(rel_scale), _ptr(weight), _stream(stream)), "hbx_loss_weight_pw")
        return weight

    # --- windows (hbx_*_window): holograms of any size zero-filled into the grid, outputs over a rectangle ---
    def window(self, win):
        """(y0, x0, h, w) | None -> (the _lib.Window to pass, or None for the full grid, and its
        (h, w)).  A window outside the grid or empty raises ValueError before any device work."""
        c = self.cfg
        if win is None:
            return None, (c.height, c.width)
        y0, x0, h, w = (int(v) for v in win)
        if y0 < 0 or x0 < 0 or h < 1 or w < 1 or y0 + h > c.height or x0 + w > c.width:
            raise ValueError(f"window {(y0, x0, h, w)}: not a non-empty rectangle of the {c.height} x {c.width} grid")
        return _lib.Window(y0, x0, h, w), (h, w)

    def _evaluate_window(self, name, values, threshold, in_win, target, out_win, want_field, want_intensity, stream):
        n = _batch(values)
        c = self.cfg
        wi, (hi, wd_i) = self.window(in_win)
        wo, (ho, wd_o) = self.window(out_win)
        values = self._in(values, "values", torch.float32, (n, c.channels, hi, wd_i))
        if target is not None:
            _need(target, "target", torch.float32, (n, c.groups, ho, wd_o), self.device)
        elif not (want_field or want_intensity):
            raise ValueError(f"{name}: no target, and want_field and want_intensity are both off")
        field, inten, stats, psnr = self._outputs((n, c.channels, ho, wd_o), (n, c.groups, ho, wd_o), want_field,
                                                  want_intensity, target is not None)
        pi, po = (C.byref(wi) if wi is not None else None), (C.byref(wo) if wo is not None else None)
        if threshold is None:
            rc = self.lib.hbx_evaluate_real_window(self._h, _ptr(values), pi, _ptr(target), po, n, _ptr(field),
                                                   _ptr(inten), _ptr(stats), _ptr(psnr), _stream(stream))
        else:
            rc = self.lib.hbx_evaluate_threshold_window(self._h, _ptr(values), float(threshold), pi, _ptr(target), po,
                                                        n, _ptr(field), _ptr(inten), _ptr(stats), _ptr(psnr),
                                                        _stream(stream))
        _lib.check(rc, "hbx_" + name)
        return _complex(field), inten, stats, psnr

    def evaluate_real_window(self, values: torch.Tensor, in_win=None, target: Optional[torch.Tensor] = None,
                             out_win=None, want_field: bool = True, want_intensity: bool = True, stream=None):
        """`evaluate_real` of a hologram of any size (hbx_evaluate_real_window): `values` float32
        [B, CH, h_i, w_i] sits at in_win = (y0, x0, h_i, w_i) of the grid, which is 0 elsewhere; the
        outputs are taken over out_win = (y0, x0, h_o, w_o).  Windows are compact arrays: target and
        intensity [B, G, h_o, w_o], field [B, CH, h_o, w_o]; chan_stats and psnr (with a target) are
        over out_win, n = G h_o w_o.  None is the full grid.  Returns (field | None, intensity |
        None, chan_stats | None, psnr | None): `evaluate_real` on the zero-embedded values, sliced."""
        return self._evaluate_window("evaluate_real_window", values, None, in_win, target, out_win, want_field,
                                     want_intensity, stream)

    def evaluate_threshold_window(self, values: torch.Tensor, threshold: float, in_win=None,
                                  target: Optional[torch.Tensor] = None, out_win=None, want_field: bool = True,
                                  want_intensity: bool = True, stream=None):
        """`evaluate_real_window` of the binary hologram m = [values >= threshold], u = va + vb m
        inside in_win and 0 (no light) outside it, under either field kind
        (hbx_evaluate_threshold_window)."""
        return self._evaluate_window("evaluate_threshold_window", values, threshold, in_win, target, out_win,
                                     want_field, want_intensity, stream)

    def backward_window(self, values: torch.Tensor, val_win=None, grad_win=None,
                        samples: Optional[torch.Tensor] = None, weight: Optional[torch.Tensor] = None,
                        scale: float = 1.0, surrogate: int = _lib.STE_WINDOW, p0: float = -math.inf,
                        p1: float = math.inf, stream=None) -> torch.Tensor:
        """The backward pass of a windowed forward, on the plan for -z (hbx_backward_window):
        `values` complex64 [B, CH/2, h_v, w_v] and the optional `weight` float32 [B, G, h_v, w_v]
        sit at val_win (the forward's output window), and the gradient float32 [B, CH/2, h_g, w_g]
        is taken over grad_win (the forward's input window).  samples None: the real part (a real
        leaf's gradient); samples [B, CH/2, h_g, w_g] (the leaf): `threshold_backward`'s
        vb s(x) Re g with its surrogates."""
        n = _batch(values)
        c = self.cfg
        wv, (hv, wd_v) = self.window(val_win)
        wg, (hg, wd_g) = self.window(grad_win)
        values = self._in(values, "values", torch.complex64, (n, c.channels // 2, hv, wd_v))
        gshape = (n, c.channels // 2, hg, wd_g)
        samples = self._in(samples, "samples", torch.float32, gshape, optional=True)
        weight = self._in(weight, "weight", torch.float32, (n, c.groups, hv, wd_v), optional=True)
        grad = torch.empty(gshape, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.hbx_backward_window(self._h, _ptr(values), _ptr(weight), float(scale),
                                                C.byref(wv) if wv is not None else None, _ptr(samples),
                                                int(surrogate), float(p0), float(p1),
                                                C.byref(wg) if wg is not None else None, n, _ptr(grad),
                                                _stream(stream)), "hbx_backward_window")
        return grad

    def loss_window(self, chan_stats: torch.Tensor, out_win=None, kind: int = _lib.LOSS_MSE,
                    rel_scale: int = _lib.REL_LSQ, stream=None) -> torch.Tensor:
        """`loss` on the statistics of an output window: n = G h_o w_o (hbx_loss_window)."""
        n = _batch(chan_stats)
        wo, _ = self.window(out_win)
        _need(chan_stats, "chan_stats", torch.float64, (n, self.cfg.groups, 3), self.device)
        out = torch.empty((n,), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.hbx_loss_window(self._h, _ptr(chan_stats), C.byref(wo) if wo is not None else None, n,
                                            int(kind), int(rel_scale), _ptr(out), _stream(stream)), "hbx_loss_window")
        return out

    def loss_weight_window(self, intensity: torch.Tensor, target: torch.Tensor, chan_stats: torch.Tensor,
                           out_win=None, grad_loss: Optional[torch.Tensor] = None, kind: int = _lib.LOSS_MSE,
                           rel_scale: int = _lib.REL_LSQ, stream=None) -> torch.Tensor:
        """`loss_weight` over an output window (hbx_loss_weight_window): intensity, target and the
        returned weight are compact float32 [B, G, h_o, w_o], n = G h_o w_o."""
        n = _batch(intensity)
        wo, (ho, wd_o) = self.window(out_win)
        shape = (n, self.cfg.groups, ho, wd_o)
        _need(intensity, "intensity", torch.float32, shape, self.device)
        _need(target, "target", torch.float32, shape, self.device)
        _need(chan_stats, "chan_stats", torch.float64, (n, self.cfg.groups, 3), self.device)
        if grad_loss is not None:
            _need(grad_loss, "grad_loss", torch.float64, (n,), self.device)
        weight = torch.empty(shape, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.hbx_loss_weight_window(self._h, _ptr(intensity), _ptr(target), _ptr(chan_stats),
                                                   _ptr(grad_loss), C.byref(wo) if wo is not None else None, n,
                                                   int(kind), int(rel_scale), _ptr(weight), _stream(stream)),
                   "hbx_loss_weight_window")
        return weight

    def psnr(self, chan_stats: torch.Tensor, stream=None) -> torch.Tensor:
        n = chan_stats.shape[0]
        _need(chan_stats, "chan_stats", torch.float64, (n, self.cfg.groups, 3), self.device)
        out = torch.empty((n,), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.hbx_psnr(self._h, _ptr(chan_stats), n, _ptr(out), _stream(stream)), "hbx_psnr")
        return out

    def flip_map(self, mask: torch.Tensor, target: torch.Tensor, out: Optional[torch.Tensor] = None,
                 stream=None):
        """PSNR change of every single-pixel flip of ONE env against its
        current state (hbx_flip_map): returns (dpsnr f32 [CH, H, W], base
        psnr f64 [1]).  dpsnr.flatten()[a] is the change for action a."""
        c = self.cfg
        _need(mask, "mask", torch.int64, self.mask_shape(1)[1:], self.device)
        _need(target, "target", torch.float32, self.target_shape(1)[1:], self.device)
        if out is None:
            out = torch.empty((c.channels, c.height, c.width), dtype=torch.float32, device=self.device)
        _need(out, "out", torch.float32, (c.channels, c.height, c.width), self.device)
        base = torch.empty((1,), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.hbx_flip_map(self._h, _ptr(mask), _ptr(target), _ptr(out), _ptr(base),
                                         _stream(stream)), "hbx_flip_map")
        return out, base

    def eval_flips(self, base_mask: torch.Tensor, target: torch.Tensor, base_stats: torch.Tensor,
                   flips: torch.Tensor, psnr_out: Optional[torch.Tensor] = None,
                   group_stats: Optional[torch.Tensor] = None, stream=None):
        """PSNR of K independent single-pixel flips of ONE base env."""
        c = self.cfg
        _need(base_mask, "base_mask", torch.int64, self.mask_shape(1)[1:], self.device)
        _need(target, "target", torch.float32, self.target_shape(1)[1:], self.device)
        _need(base_stats, "base_stats", torch.float64, (c.groups, 3), self.device)
        k = flips.shape[0]
        _need(flips, "flips", torch.int64, (k,), self.device)
        if psnr_out is None:
            psnr_out = torch.empty((k,), dtype=torch.float64, device=self.device)
        if group_stats is None:
            group_stats = torch.empty((k, 3), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.hbx_eval_flips(self._h, _ptr(base_mask), _ptr(target), _ptr(base_stats),
                                           _ptr(flips), k, _ptr(psnr_out), _ptr(group_stats),
                                           _stream(stream)), "hbx_eval_flips")
        return psnr_out, group_stats

    # -- plane-cached candidates (ABI v10): the FFT mode's bits, only the flipped pair propagated
    def plane_pool(self, spare_pairs: int):
        """(plane_inten f32 [CH + 2 S, H, W], plane_slot int32 [CH + 2 S]) for one base env."""
        c = self.cfg
        n = c.channels + 2 * int(spare_pairs)
        return (torch.empty((n, c.height, c.width), dtype=torch.float32, device=self.device),
                torch.empty((n,), dtype=torch.int32, device=self.device))

    def _check_pool(self, plane_inten, plane_slot):
        c = self.cfg
        n = plane_slot.shape[0] if isinstance(plane_slot, torch.Tensor) else -1
        _need(plane_slot, "plane_slot", torch.int32, (n,), self.device)
        _need(plane_inten, "plane_inten", torch.float32, (n, c.height, c.width), self.device)
        if n < c.channels + 2 or (n - c.channels) % 2:
            raise ValueError(f"plane pool of {n} slots: need CH + 2 S with S >= 1")
        return (n - c.channels) // 2

    def planes_fill(self, mask, target, plane_inten, plane_slot, stream=None):
        """Full propagation of ONE base env into its plane pool (hbx_planes_fill):
        returns (chan_stats f64 [G, 3], psnr f64 [1])."""
        c = self.cfg
        _need(mask, "mask", torch.int64, self.mask_shape(1)[1:], self.device)
        _need(target, "target", torch.float32, self.target_shape(1)[1:], self.device)
        s = self._check_pool(plane_inten, plane_slot)
        stats = torch.empty((c.groups, 3), dtype=torch.float64, device=self.device)
        psnr = torch.empty((1,), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.hbx_planes_fill(self._h, _ptr(mask), _ptr(target), _ptr(plane_inten), _ptr(plane_slot),
                                            s, _ptr(stats), _ptr(psnr), _stream(stream)), "hbx_planes_fill")
        return stats, psnr

    def eval_flips_planes(self, base_mask, target, base_stats, plane_inten, plane_slot, flips,
                          psnr_out=None, group_stats=None, stream=None):
        """eval_flips with the base env's plane pool: the same PSNRs bit for bit."""
        c = self.cfg
        _need(base_mask, "base_mask", torch.int64, self.mask_shape(1)[1:], self.device)
        _need(target, "target", torch.float32, self.target_shape(1)[1:], self.device)
        _need(base_stats, "base_stats", torch.float64, (c.groups, 3), self.device)
        s = self._check_pool(plane_inten, plane_slot)
        k = flips.shape[0]
        _need(flips, "flips", torch.int64, (k,), self.device)
        if psnr_out is None:
            psnr_out = torch.empty((k,), dtype=torch.float64, device=self.device)
        if group_stats is None:
            group_stats = torch.empty((k, 3), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.hbx_eval_flips_planes(self._h, _ptr(base_mask), _ptr(target), _ptr(base_stats),
                                                  _ptr(plane_inten), _ptr(plane_slot), s, _ptr(flips), k,
                                                  _ptr(psnr_out), _ptr(group_stats), _stream(stream)),
                   "hbx_eval_flips_planes")
        return psnr_out, group_stats

    def commit_flip_planes(self, base_mask, base_stats, prev_psnr, plane_inten, plane_slot, flips, psnr_out,
                           group_stats, k_dev: torch.Tensor, stream=None):
        """Commit candidate k_dev of an eval_flips_planes batch (its fresh pair swaps in)."""
        k = self._check_commit(base_mask, base_stats, prev_psnr, flips, psnr_out, group_stats, k_dev)
        s = self._check_pool(plane_inten, plane_slot)
        _lib.check(self.lib.hbx_commit_flip_planes(self._h, _ptr(base_mask), _ptr(base_stats), _ptr(prev_psnr),
                                                   _ptr(plane_slot), s, _ptr(flips), _ptr(psnr_out),
                                                   _ptr(group_stats), _ptr(k_dev), k, _stream(stream)),
                   "hbx_commit_flip_planes")

    def dbs_walk_planes(self, base_mask, target, base_stats, plane_inten, plane_slot, order: torch.Tensor,
                        walk: torch.Tensor, accept_pos: torch.Tensor, accept_psnr: torch.Tensor, K: int,
                        batches: int, stream=None, fill=None, slack=None):
        """hbx_dbs_walk_planes: enqueue `batches` device-decided batches of K candidates of the
        FFT-mode greedy on the base state's plane pool (no host round trip).  fill = (counts, target,
        tol): the on-pixel ratio constraint (hbx_dbs_walk_planes_fill, an extension; counts [G] int64
        on the device, updated by the walk).  slack: float64 [>= len(order)] on the device, the
        per-candidate acceptance slack (hbx_dbs_walk_planes_anneal, an extension; with or without fill)."""
        c = self.cfg
        _need(base_mask, "base_mask", torch.int64, self.mask_shape(1)[1:], self.device)
        _need(target, "target", torch.float32, self.target_shape(1)[1:], self.device)
        _need(base_stats, "base_stats", torch.float64, (c.groups, 3), self.device)
        s = self._check_pool(plane_inten, plane_slot)
        _need(order, "order", torch.int64, (order.shape[0],), self.device)
        _need(walk, "walk", torch.uint8, (C.sizeof(_lib.DbsWalk),), self.device)
        cap = accept_pos.shape[0]
        _need(accept_pos, "accept_pos", torch.int64, (cap,), self.device)
        _need(accept_psnr, "accept_psnr", torch.float64, (cap,), self.device)
        if slack is not None:
            _need(slack, "slack", torch.float64, (slack.shape[0],), self.device)
            counts, f_target, f_tol = fill if fill is not None else (None, 0, 0)
            if counts is not None:
                _need(counts, "fill counts", torch.int64, (c.groups,), self.device)
            _lib.check(self.lib.hbx_dbs_walk_planes_anneal(
                self._h, _ptr(base_mask), _ptr(target), _ptr(base_stats), _ptr(plane_inten), _ptr(plane_slot), s,
                _ptr(order), int(order.shape[0]), _ptr(walk), _ptr(accept_pos), _ptr(accept_psnr), cap, int(K),
                int(batches), None if counts is None else _ptr(counts), int(f_target), int(f_tol), _ptr(slack),
                int(slack.shape[0]), _stream(stream)), "hbx_dbs_walk_planes_anneal")
            return
        if fill is None:
            _lib.check(self.lib.hbx_dbs_walk_planes(self._h, _ptr(base_mask), _ptr(target), _ptr(base_stats),
                                                    _ptr(plane_inten), _ptr(plane_slot), s, _ptr(order),
                                                    int(order.shape[0]), _ptr(walk), _ptr(accept_pos),
                                                    _ptr(accept_psnr), cap, int(K), int(batches), _stream(stream)),
                       "hbx_dbs_walk_planes")
            return
        counts, f_target, f_tol = fill
        _need(counts, "fill counts", torch.int64, (c.groups,), self.device)
        _lib.check(self.lib.hbx_dbs_walk_planes_fill(self._h, _ptr(base_mask), _ptr(target), _ptr(base_stats),
                                                     _ptr(plane_inten), _ptr(plane_slot), s, _ptr(order),
                                                     int(order.shape[0]), _ptr(walk), _ptr(accept_pos),
                                                     _ptr(accept_psnr), cap, int(K), int(batches), _ptr(counts),
                                                     int(f_target), int(f_tol), _stream(stream)),
                   "hbx_dbs_walk_planes_fill")

    def eval_flips_psf(self, base_mask, target, base_stats, field, intensity, flips,
                       psnr_out=None, group_stats=None, stream=None):
        """eval_flips on the incremental-field path: field [CH, H, W, 2] f32 and
        intensity [G, H, W] f32 of the base state (from simulate)."""
        c = self.cfg
        _need(base_mask, "base_mask", torch.int64, self.mask_shape(1)[1:], self.device)
        _need(target, "target", torch.float32, self.target_shape(1)[1:], self.device)
        _need(base_stats, "base_stats", torch.float64, (c.groups, 3), self.device)
        _need(field, "field", torch.float32, (c.channels, c.height, c.width, 2), self.device)
        _need(intensity, "intensity", torch.float32, (c.groups, c.height, c.width), self.device)
        k = flips.shape[0]
        _need(flips, "flips", torch.int64, (k,), self.device)
        if psnr_out is None:
            psnr_out = torch.empty((k,), dtype=torch.float64, device=self.device)
        if group_stats is None:
            group_stats = torch.empty((k, 3), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.hbx_eval_flips_psf(self._h, _ptr(base_mask), _ptr(target), _ptr(base_stats),
                                               _ptr(field), _ptr(intensity), _ptr(flips), k, _ptr(psnr_out),
                                               _ptr(group_stats), _stream(stream)), "hbx_eval_flips_psf")
        return psnr_out, group_stats

    def _check_commit(self, base_mask, base_stats, prev_psnr, flips, psnr_out, group_stats, k_dev):
        c = self.cfg
        _need(base_mask, "base_mask", torch.int64, self.mask_shape(1)[1:], self.device)
        _need(base_stats, "base_stats", torch.float64, (c.groups, 3), self.device)
        _need(prev_psnr, "prev_psnr", torch.float64, (1,), self.device)
        k = flips.shape[0]
        _need(flips, "flips", torch.int64, (k,), self.device)
        if psnr_out.shape[0] < k or group_stats.shape[0] < k:
            raise ValueError(f"psnr_out / group_stats hold fewer than the {k} candidates of flips")
        _need(psnr_out, "psnr_out", torch.float64, (psnr_out.shape[0],), self.device)
        _need(group_stats, "group_stats", torch.float64, (group_stats.shape[0], 3), self.device)
        _need(k_dev, "k", torch.int32, (1,), self.device)
        return k

    def commit_flip_psf(self, base_mask, base_stats, prev_psnr, field, intensity, flips, psnr_out,
                        group_stats, k_dev: torch.Tensor, stream=None):
        """Commit candidate k_dev of an eval_flips_psf batch (a k outside the
        batch commits nothing)."""
        c = self.cfg
        k = self._check_commit(base_mask, base_stats, prev_psnr, flips, psnr_out, group_stats, k_dev)
        _need(field, "field", torch.float32, (c.channels, c.height, c.width, 2), self.device)
        _need(intensity, "intensity", torch.float32, (c.groups, c.height, c.width), self.device)
        _lib.check(self.lib.hbx_commit_flip_psf(self._h, _ptr(base_mask), _ptr(base_stats), _ptr(prev_psnr),
                                                _ptr(field), _ptr(intensity), _ptr(flips), _ptr(psnr_out),
                                                _ptr(group_stats), _ptr(k_dev), k, _stream(stream)),
                   "hbx_commit_flip_psf")

    def dbs_walk_psf(self, base_mask, target, base_stats, field, intensity, order: torch.Tensor,
                     walk: torch.Tensor, accept_pos: torch.Tensor, accept_psnr: torch.Tensor, K: int,
                     batches: int, stream=None):
        """hbx_dbs_walk_psf: enqueue `batches` speculative batches of K candidates of the
        device-resident greedy walk.  walk: uint8 [sizeof(hbx_dbs_walk_t)] on the device."""
        c = self.cfg
        _need(field, "field", torch.float32, (c.channels, c.height, c.width, 2), self.device)
        _need(intensity, "intensity", torch.float32, (c.groups, c.height, c.width), self.device)
        _need(base_mask, "base_mask", torch.int64, self.mask_shape(1)[1:], self.device)
        _need(target, "target", torch.float32, self.target_shape(1)[1:], self.device)
        _need(base_stats, "base_stats", torch.float64, (c.groups, 3), self.device)
        _need(order, "order", torch.int64, (order.shape[0],), self.device)
        _need(walk, "walk", torch.uint8, (C.sizeof(_lib.DbsWalk),), self.device)
        cap = accept_pos.shape[0]
        _need(accept_pos, "accept_pos", torch.int64, (cap,), self.device)
        _need(accept_psnr, "accept_psnr", torch.float64, (cap,), self.device)
        _lib.check(self.lib.hbx_dbs_walk_psf(self._h, _ptr(base_mask), _ptr(target), _ptr(base_stats),
                                             _ptr(field), _ptr(intensity), _ptr(order), int(order.shape[0]),
                                             _ptr(walk),
                                             _ptr(accept_pos), _ptr(accept_psnr), cap, int(K), int(batches),
                                             _stream(stream)), "hbx_dbs_walk_psf")

    def commit_flip(self, base_mask, base_stats, prev_psnr, flips, psnr_out, group_stats,
                    k_dev: torch.Tensor, stream=None):
        """Commit candidate k_dev of an eval_flips batch (a k outside the batch
        commits nothing)."""
        k = self._check_commit(base_mask, base_stats, prev_psnr, flips, psnr_out, group_stats, k_dev)
        _lib.check(self.lib.hbx_commit_flip(self._h, _ptr(base_mask), _ptr(base_stats), _ptr(prev_psnr),
                                            _ptr(flips), _ptr(psnr_out), _ptr(group_stats), _ptr(k_dev), k,
                                            _stream(stream)), "hbx_commit_flip")

    def step(self, mask, actions, target, chan_stats, prev_psnr, accept_rule=_lib.ACCEPT_DBS,
             stream=None):
        """DBS primitive (include/hbx.h hbx_step): returns (psnr, accepted)."""
        n = mask.shape[0]
        self._check_mask_target(mask, target, n)
        _need(actions, "actions", torch.int64, (n,), self.device)
        psnr = torch.empty((n,), dtype=torch.float64, device=self.device)
        acc = torch.empty((n,), dtype=torch.uint8, device=self.device)
        _lib.check(self.lib.hbx_step(self._h, _ptr(mask), _ptr(actions), n, _ptr(target), _ptr(chan_stats),
                                     _ptr(prev_psnr), _ptr(psnr), _ptr(acc), int(accept_rule),
                                     _stream(stream)), "hbx_step")
        return psnr, acc

    # env-level entry points are used by hbx.env (EnvState owns the buffers)
    def env_reset(self, bufs: _lib.EnvBuffers, n_env: int, env_ids: Optional[torch.Tensor] = None,
                  stream=None):
        n_ids = 0 if env_ids is None else int(env_ids.shape[0])
        _lib.check(self.lib.hbx_env_reset(self._h, C.byref(bufs), n_env, _ptr(env_ids), n_ids,
                                          _stream(stream)), "hbx_env_reset")

    def env_obs_sync(self, bufs: _lib.EnvBuffers, n_env: int, what: int = _lib.OBS_STATE | _lib.OBS_RECON,
                     env_ids: Optional[torch.Tensor] = None, stream=None):
        """Rebuild the observation mirrors (state_bytes from the mask, recon from the
        intensity cache) of the listed envs -- hbx_env_obs_sync."""
        n_ids = 0 if env_ids is None else int(env_ids.shape[0])
        _lib.check(self.lib.hbx_env_obs_sync(self._h, C.byref(bufs), n_env, _ptr(env_ids), n_ids, int(what),
                                             _stream(stream)), "hbx_env_obs_sync")

    def env_step_psf(self, bufs, params, n_env, actions, reward, psnr, accepted, terminated, truncated,
                     stream=None):
        _lib.check(self.lib.hbx_env_step_psf(self._h, C.byref(bufs), C.byref(params), n_env, _ptr(actions),
                                             _ptr(reward), _ptr(psnr), _ptr(accepted), _ptr(terminated),
                                             _ptr(truncated), _stream(stream)), "hbx_env_step_psf")

    def field_refresh(self, bufs, n_env, env_ids: Optional[torch.Tensor] = None, stream=None):
        n_ids = 0 if env_ids is None else int(env_ids.shape[0])
        _lib.check(self.lib.hbx_field_refresh(self._h, C.byref(bufs), n_env, _ptr(env_ids), n_ids,
                                              _stream(stream)), "hbx_field_refresh")

    def env_step(self, bufs, params, n_env, actions, reward, psnr, accepted, terminated, truncated,
                 group_intensity=None, stream=None):
        _lib.check(self.lib.hbx_env_step(self._h, C.byref(bufs), C.byref(params), n_env, _ptr(actions),
                                         _ptr(reward), _ptr(psnr), _ptr(accepted), _ptr(terminated),
                                         _ptr(truncated), _ptr(group_intensity), _stream(stream)),
                   "hbx_env_step")
