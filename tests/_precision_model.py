"""The cases, inputs and statistic that tests/test_precision_model_host.py (CPU) and tests/test_gpu_precision.py
(GPU) share, so that the CPU file checks the float64 rounding model's own margin at exactly the shapes, field
kinds and seeds the GPU file holds the kernels to.

The model is oracle.hbx_oracle.propagate_rounded: a float64 propagation that rounds the two pass intermediates
(row spectrum A, column-pass output B) as a plan with hbx_plan_set_precision stores them.  The statistic is

    rho(x) = rms(x - model) / rms(model - unrounded float64 field),

the distance of x from the model in units of what the rounding itself moves.  A float32 implementation that
rounds at the same two points lands near the model except where its float32 error carries a value across a
rounding boundary (rho a few percent); one that rounds elsewhere, otherwise or not at all is about one
rounding's worth away (rho ~ 0.7 and up).  rms only: the maximum over elements is heavy-tailed (one value near
a tie moves by a whole step of the store type).
"""
import functools

import numpy as np

from oracle import hbx_oracle as O

BF16, F16 = O.PRECISION_BF16_STORE, O.PRECISION_F16_STORE
STORE_NAMES = {BF16: "bf16", F16: "fp16"}
FIELD_NAMES = {O.FIELD_AMPLITUDE: "amplitude", O.FIELD_PHASE: "phase"}

# (N, planes, field kind, seed): one mono group each.  P = 8 at N = 64: with 2 planes the few elements let one
# large B entry near a tie carry rho past 0.1.  The seeds are fixed here and the CPU file asserts the emulation's
# rho <= RHO_EMULATION at every one of them.
CASES = [(n, p, fk, 10 * n + fk) for n, p in ((64, 8), (256, 8), (1024, 2))
         for fk in (O.FIELD_AMPLITUDE, O.FIELD_PHASE)]
STORES = (BF16, F16)

RHO_EMULATION = 0.1   # the correct complex64 emulation stays below this on the CPU ...
RHO_CAP = 0.3         # ... the kernels below this on the GPU (2.4 x the worst correct CPU figure on record,
RHO_MUTANT = 0.6      # 2.3 x below the best mutant), and every mutant or mismatched store kind above this


def case_id(case):
    n, p, fk, seed = case
    return f"{n}x{p}-{FIELD_NAMES[fk]}-s{seed}"


def ocfg_for(case):
    n, p, fk, _ = case
    return O.OpticsConfig(n, n, 1, p, O.WL_MONO, field_kind=fk)


def inputs(case):
    """(mask uint8 [P, N, N], target float32 [1, N, N]) of a case"""
    n, p, _, seed = case
    rng = np.random.default_rng(seed)
    mask = (rng.random((p, n, n), np.float32) >= 0.5).astype(np.uint8)
    target = rng.random((1, n, n), np.float32)
    return mask, target


def plane_mean(field):
    return np.mean(field.real ** 2 + field.imag ** 2, axis=0)


@functools.lru_cache(maxsize=None)
def reference(case):
    """(mask, target, h, unrounded float64 field [P, N, N]) of a case, computed once and read-only"""
    ocfg = ocfg_for(case)
    mask, target = inputs(case)
    h = ocfg.transfer(0)
    field = O.propagate(O.mask_to_field(mask, ocfg.field_kind), h)
    for a in (mask, target, h, field):
        a.setflags(write=False)
    return mask, target, h, field


@functools.lru_cache(maxsize=None)
def model(case, store_kind):
    """the rounding model's field [P, N, N] (complex128), computed once and read-only"""
    mask, _, h, _ = reference(case)
    f = O.propagate_rounded(O.mask_to_field(mask, ocfg_for(case).field_kind), h, store_kind)
    f.setflags(write=False)
    return f


def rms(x):
    x = np.asarray(x)
    return float(np.sqrt(np.mean(x.real ** 2 + x.imag ** 2)))


def rho(x, want, unrounded):
    """rms(x - want) / rms(want - unrounded): fields (complex) or intensities (real)"""
    return rms(np.asarray(x) - want) / rms(want - unrounded)


# -- the complex64 stand-in for the device (CPU tests) ------------------------------------------------
def truncate_bf16(x):
    """float32 -> the bfloat16 toward zero (the low 16 bits dropped): the truncation mutant"""
    return (np.asarray(x, np.float32).view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)


def _round_c64(x, fn):
    out = np.empty(x.shape, np.complex64)
    out.real = fn(x.real)
    out.imag = fn(x.imag)
    return out


def emulate(case, store_kind, round_a=True, round_b=True, truncate=False):
    """propagate_rounded's steps in complex64 (scipy.fft keeps single precision), H rounded once to
    complex64 as the device's table is: what a float32 implementation of the same roundings computes.
    round_a / round_b off and truncate are the mutants."""
    import scipy.fft as sf
    mask, _, h, _ = reference(case)
    n = mask.shape[-1]
    fn = truncate_bf16 if truncate else (O.round_bf16 if store_kind == BF16 else O.round_f16)
    u = O.mask_to_field(mask, ocfg_for(case).field_kind).astype(np.float32)
    a = sf.fft(u.astype(np.complex64), axis=-1)
    if round_a:
        a = _round_c64(a, fn)
    b = sf.ifft(sf.fft(a, axis=-2) * h.astype(np.complex64), axis=-2) * np.float32(1.0 / n)
    if round_b:
        b = _round_c64(b, fn)
    out = sf.ifft(b, axis=-1) * np.float32(n)
    assert out.dtype == np.complex64
    return out
