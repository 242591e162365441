"""The float64 rounding model of the bf16 / fp16 intermediate stores (oracle.hbx_oracle.propagate_rounded) and
the statistic tests/test_gpu_precision.py holds the kernels to, on the CPU.

  * the rounding helpers at the values where a rounding goes wrong: ties in both directions, signed zeros, the
    largest finite fp16, an fp16 subnormal, a bf16 rounding that carries into the exponent -- and bf16 against
    torch.bfloat16's conversion over random bit patterns;
  * the unrounded model is O.propagate;
  * the statistic separates right from wrong at every (N, P, field kind, seed, store kind) of the GPU tests: a
    complex64 emulation of the model (scipy.fft in single precision, tests/_precision_model.py) has
    rho <= 0.1, and each mutant -- no rounding, A only, B only, bf16 truncation -- has rho >= 0.6.  The GPU cap
    of 0.3 is a condition between the two; this file is the check that the reference alone stays inside it.
    The figures are printed (python -m pytest -s) and kept in profiles/precision_model/rho_cpu.txt.
"""
import numpy as np
import pytest

from oracle import hbx_oracle as O
from tests import _precision_model as M

pytest.importorskip("scipy.fft")


def f32(*v):
    return np.array(v, np.float32)


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


# -- rounding helpers -----------------------------------------------------------------------------
def test_round_bf16_known_values():
    e = 2.0 ** -7                                   # one bf16 step in [1, 2)
    x = f32(1 + e / 2,          # tie between 1 (even) and 1 + e: down
            1 + 3 * e / 2,      # tie between 1 + e and 1 + 2 e (even): up
            -(1 + e / 2), -(1 + 3 * e / 2),
            1 + e / 2 + 2.0 ** -23,                  # just past the tie: up
            1 + 3 * e / 2 - 2.0 ** -23,              # just short of it: down
            2 - e / 2,          # tie between 2 - e (odd) and 2: the carry runs into the exponent
            2 - e / 4,          # nearest is 2 outright
            0.0, -0.0, np.inf, -np.inf)
    want = f32(1, 1 + 2 * e, -1, -(1 + 2 * e), 1 + e, 1 + e, 2, 2, 0.0, -0.0, np.inf, -np.inf)
    got = O.round_bf16(x)
    assert got.dtype == np.float32
    assert np.array_equal(bits(got), bits(want)), (got, want)          # bits: the zeros keep their signs
    assert np.all(bits(got[np.isfinite(got)]) & 0xffff == 0)
    # past the largest finite bf16 (0x7f7f0000) by more than half a step: the infinity
    big = np.array([0x7f7f8000, 0x7f7f7fff, 0xff7f8000], np.uint32).view(np.float32)
    assert np.array_equal(bits(O.round_bf16(big)), np.array([0x7f800000, 0x7f7f0000, 0xff800000], np.uint32))
    assert np.isnan(O.round_bf16(f32(np.nan))[0])
    # float32 subnormals: the step of the lowest binade
    tiny = np.array([0x00008000, 0x00018000, 0x00008001], np.uint32).view(np.float32)   # ties down, up; past
    assert np.array_equal(bits(O.round_bf16(tiny)), np.array([0x0, 0x00020000, 0x00010000], np.uint32))


def test_round_bf16_equals_torch_conversion():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(0)
    u = rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32)
    u[:4] = [0x3f808000, 0x3f818000, 0x3fff8000, 0x7f7f8000]          # two ties, a carry, the overflow
    x = u.view(np.float32)
    x = x[~np.isnan(x)]
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).to(torch.float32).numpy()
    assert np.array_equal(bits(O.round_bf16(x)), bits(want))
    # ... and the mutant is a different function: toward zero on about half of the values
    trunc = M.truncate_bf16(x)
    assert 0.4 < np.mean(bits(trunc) != bits(want)) < 0.6


def test_round_f16_known_values():
    e = 2.0 ** -10                                  # one fp16 step in [1, 2)
    sub = 2.0 ** -24                                # the smallest fp16 subnormal
    x = f32(1 + e / 2, 1 + 3 * e / 2, -(1 + e / 2), -(1 + 3 * e / 2),      # ties: down, up, and mirrored
            0.0, -0.0,
            65504.0, 65519.0, 65520.0, -65520.0,                           # the largest finite; below / at the tie to inf
            5 * sub, 5.5 * sub, 6.5 * sub, 0.5 * sub, 0.75 * sub,          # subnormals: exact, ties to even, to 0, up
            2.0 ** -14 - sub / 2)                                          # the tie between the largest subnormal and the smallest normal
    want = f32(1, 1 + 2 * e, -1, -(1 + 2 * e), 0.0, -0.0, 65504.0, 65504.0, np.inf, -np.inf,
               5 * sub, 6 * sub, 6 * sub, 0.0, sub, 2.0 ** -14)
    got = O.round_f16(x)
    assert got.dtype == np.float32
    assert np.array_equal(bits(got), bits(want)), (got, want)
    # doubling does not commute with the rounding among the subnormals: why the model rounds A, not 2 A
    v = f32(2.5 * sub)
    assert O.round_f16(2 * v)[0] == 5 * sub and 2 * O.round_f16(v)[0] == 4 * sub


def test_store_round_rounds_re_and_im_apart():
    z = np.array([(1 + 2.0 ** -8) + 1j * (1 + 3 * 2.0 ** -8), -0.3 + 65520.0j], np.complex128)
    b = O.store_round(z, O.PRECISION_BF16_STORE)
    assert b[0] == 1 + 1j * (1 + 2.0 ** -6) and b.dtype == np.complex128
    f = O.store_round(z, O.PRECISION_F16_STORE)
    assert f[0] == z[0] and f[1].real == float(np.float16(-0.3)) and np.isinf(f[1].imag)
    assert O.store_round(z, None) is z
    with pytest.raises(ValueError):
        O.store_round(z, 3)


# -- the model ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", M.CASES[:4], ids=M.case_id)
def test_unrounded_model_is_propagate(case):
    mask, _, h, field = M.reference(case)
    u = O.mask_to_field(mask, M.ocfg_for(case).field_kind)
    got = O.propagate_rounded(u, h, None)
    assert np.max(np.abs(got - field)) <= 1e-12 * np.max(np.abs(field))
    # a store kind with both roundings off is the same function
    got = O.propagate_rounded(u, h, M.F16, round_a=False, round_b=False)
    assert np.max(np.abs(got - field)) <= 1e-12 * np.max(np.abs(field))


def test_model_moves_the_field_by_the_store_types_step():
    """rms(model - unrounded) / rms(field): a few bf16 (2^-9 relative, rms) or fp16 (2^-12) roundings' worth"""
    case = M.CASES[0]
    _, _, _, field = M.reference(case)
    for sk, lo, hi in ((M.BF16, 2.0 ** -10, 2.0 ** -6), (M.F16, 2.0 ** -13, 2.0 ** -9)):
        d = M.rms(M.model(case, sk) - field) / M.rms(field)
        assert lo < d < hi, (sk, d)


def test_fp16_model_rounds_b_at_its_stored_scale():
    """Where the scale shows: a field so weak that B = IFFT_y(FFT_y(A) H) / N sits among the fp16 subnormals.
    Rounding B at N times the scale (the last pass's 1 / N left out of the stored value) gives another field."""
    n, p = 64, 2
    rng = np.random.default_rng(5)
    u = (rng.random((p, n, n)) - 0.5) * 2.0 ** -10
    h = O.transfer_function(n, n, O.PIXEL_PITCH, O.PIXEL_PITCH, O.WL_MONO[0], O.Z_DEFAULT)
    want = O.propagate_rounded(u, h, M.F16)
    a = O.store_round(np.fft.fft(u, axis=-1), M.F16)
    b = np.fft.ifft(np.fft.fft(a, axis=-2) * h, axis=-2)
    assert np.quantile(np.abs(b), 0.9) / n < 2.0 ** -14   # B's stored values are fp16 subnormals, A's are not
    assert np.median(np.abs(a)) > 2.0 ** -13
    other = np.fft.ifft(O.store_round(b, M.F16), axis=-1)
    full = O.propagate(u, h)
    assert M.rho(other, want, full) > 0.5


# -- the statistic separates right from wrong -----------------------------------------------------
MUTANTS = {"no rounding": dict(round_a=False, round_b=False), "A only": dict(round_b=False),
           "B only": dict(round_a=False), "truncation": dict(truncate=True)}


@pytest.mark.parametrize("store_kind", M.STORES, ids=lambda s: M.STORE_NAMES[s])
@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_rho_separates_emulation_from_mutants(case, store_kind):
    _, _, _, field = M.reference(case)
    want = M.model(case, store_kind)
    want_i, full_i = M.plane_mean(want), M.plane_mean(field)
    good = M.emulate(case, store_kind)
    r_f, r_i = M.rho(good, want, field), M.rho(M.plane_mean(good.astype(np.complex128)), want_i, full_i)
    line = f"{M.case_id(case)} {M.STORE_NAMES[store_kind]}: emulation rho field {r_f:.4f} intensity {r_i:.4f};"
    worst = np.inf
    for name, kw in MUTANTS.items():
        if name == "truncation" and store_kind != M.BF16:
            continue
        bad = M.emulate(case, store_kind, **kw)
        m_f = M.rho(bad, want, field)
        m_i = M.rho(M.plane_mean(bad.astype(np.complex128)), want_i, full_i)
        line += f" {name} {m_f:.3f} / {m_i:.3f}"
        worst = min(worst, m_f, m_i)
    print(line)
    assert r_f <= M.RHO_EMULATION and r_i <= M.RHO_EMULATION, line
    assert worst >= M.RHO_MUTANT, line
