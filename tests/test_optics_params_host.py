"""The inputs of tests/test_gpu_optics_params.py discriminate (no GPU needed).

A GPU test that passes at unequal pitch proves that the device has x and y the right way round
only if the expected value itself depends on which way round they are.  For the exact configs,
seeds and masks of the GPU tests (their `*_case` builders, imported here) the float64 oracle
with dx and dy exchanged must move
    every compared PSNR by >= 10 x PSNR_TOL,
    every compared field, intensity and gradient by >= 100 x FIELD_RTOL of its maximum,
and under EVAN the oracle with the evanescent bins at |H| = 1 instead of 0 must move every
compared PSNR by the same margin.  These are conditions on the inputs, not tolerances: a case that
falls short gets another seed or shape, never a smaller factor.

Also here: the properties the two parameter sets are chosen for (H != H^T under ANISO, the share
of bins cut under EVAN), the distance of the nearest bin to the cut (the device table and the
oracle both evaluate the radicand in double, so they classify every bin alike as long as none
sits on the cut), and H(-z) = conj H(z) including the zeros."""
import numpy as np
import pytest

pytest.importorskip("torch")

from oracle import hbx_oracle as O  # noqa: E402
from tests import test_gpu_optics_params as G  # noqa: E402

PSNR_MOVE = 10 * G.PSNR_TOL
FIELD_MOVE = 100 * G.FIELD_RTOL
EVAN_CUT_SHARE = {638e-9: 0.172, 515e-9: 0.010, 450e-9: 0.0}
CUT_MARGIN = 1e-9


def _moved(a, b):
    """max |a - b| as a fraction of max |a|"""
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(a))


def _kinds(pset):
    return ("swap", "nocut") if pset == "evan" else ("swap",)


# -- the parameter sets --------------------------------------------------------------------------------
@pytest.mark.parametrize("n", G.SIZES)
def test_aniso_transfer_is_not_its_transpose_and_has_unit_modulus(n):
    for tf in (O.TF_ASM, O.TF_FRESNEL):
        for wl in G.WL4:
            h = O.transfer_function(n, n, wl=wl, tf_kind=tf, **G.ANISO)
            assert np.max(np.abs(np.abs(h) - 1.0)) < 1e-12
            assert np.max(np.abs(h - h.T)) > 1.9                     # two unit phasors nearly opposite
            hs = np.fft.ifft2(h)
            assert _moved(hs, hs.T) >= FIELD_MOVE


@pytest.mark.parametrize("n", G.SIZES)
def test_evan_cut_share_and_margin(n):
    fx = O.freq_grid(n, G.EVAN["dx"])[None, :]
    fy = O.freq_grid(n, G.EVAN["dy"])[:, None]
    f2 = fx * fx + fy * fy
    for wl in G.WL4:
        h = O.transfer_function(n, n, wl=wl, **G.EVAN)
        share = float(np.mean(h == 0))
        margin = float(np.min(np.abs(1.0 - wl * wl * f2)))
        print(f"N={n} wl={wl * 1e9:.0f} nm: {100 * share:.2f} % of the bins cut, nearest |1 - wl^2 f^2| = {margin:.3e}")
        assert margin >= CUT_MARGIN
        assert np.array_equal(h == 0, 1.0 - wl * wl * f2 <= 0)
        assert np.max(np.abs(np.abs(h[h != 0]) - 1.0)) < 1e-12
        if wl in EVAN_CUT_SHARE:
            assert abs(share - EVAN_CUT_SHARE[wl]) < 1.5e-3
        else:
            assert share == 0.0                                      # 405 nm: the fourth group of the G = 4 case
        if share > 0:
            assert not np.array_equal(h == 0, (h == 0).T)            # the cut itself is not symmetric in x, y


@pytest.mark.parametrize("pset,tf", G.TFSETS, ids=G.TFSET_IDS)
def test_minus_z_transfer_is_the_conjugate_including_zeros(pset, tf):
    s = G.SETS[pset]
    for n in (64, 896):
        for wl in G.WL4:
            hp = O.transfer_function(n, n, s["dx"], s["dy"], wl, s["z"], tf)
            hm = O.transfer_function(n, n, s["dx"], s["dy"], wl, -s["z"], tf)
            assert np.array_equal(hm, np.conj(hp))
            assert np.array_equal(hm == 0, hp == 0)


# -- fields ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", G.SIZES)
@pytest.mark.parametrize("pset,tf", G.TFSETS, ids=G.TFSET_IDS)
def test_complex_and_real_fields_move(pset, tf, n):
    _, want = G.complex_case(pset, tf, n)
    _, _, want_f, want_i, _, want_ps = G.real_case(pset, tf, n)
    for kind in _kinds(pset):
        if kind == "swap":
            moved = _moved(want, G.complex_case(pset, tf, n, kind)[1])
            print(f"complex {pset} tf={tf} N={n}: {kind} moves the field by {moved:.3e} of its max")
            assert moved >= FIELD_MOVE
        _, _, f, i, _, ps = G.real_case(pset, tf, n, kind)
        print(f"real {pset} tf={tf} N={n}: {kind} moves the field by {_moved(want_f, f):.3e}, the intensity by "
              f"{_moved(want_i, i):.3e} of max, the psnr by {abs(ps - want_ps):.3e} dB")
        assert abs(ps - want_ps) >= PSNR_MOVE
        if kind == "swap":
            assert _moved(want_f, f) >= FIELD_MOVE
            assert _moved(want_i, i) >= FIELD_MOVE


@pytest.mark.parametrize("n", [64, 896])
@pytest.mark.parametrize("pset", ["aniso", "evan"])
def test_single_sample_response_differs_from_its_transpose(pset, n):
    cfg = G.ocfg(pset, n, 1, 4)
    for y, x in G.single_pixels(n):
        want = G.single_response(cfg, y, x)
        assert _moved(want, G.single_response(G.variant(cfg, "swap"), y, x)) >= FIELD_MOVE     # h transposed
        assert _moved(want, G.single_response(cfg, x, y)) >= FIELD_MOVE                        # rolled to (col, row)


@pytest.mark.parametrize("n", list(G.PSF_SHAPES))
@pytest.mark.parametrize("pset", ["aniso", "evan"])
def test_psf_reset_field_and_psnr_move(pset, n):
    g, p, n_env = G.PSF_SHAPES[n]
    cfg = G.ocfg(pset, n, g, p)
    ins = G.psf_inputs(cfg, n_env)
    mask0 = (ins[0][0] >= 0.5).astype(np.uint8)
    want_f = G.field_of(cfg, O.mask_to_field(mask0), p)
    assert _moved(want_f, G.field_of(G.variant(cfg, "swap"), O.mask_to_field(mask0), p)) >= FIELD_MOVE
    for b in range(n_env):
        base = O.OracleEnv(cfg).reset(*ins[b])
        for kind in _kinds(pset):
            other = O.OracleEnv(G.variant(cfg, kind)).reset(*ins[b])
            print(f"psf {pset} N={n} env {b}: {kind} moves the initial psnr by {abs(other - base):.3e} dB")
            assert abs(other - base) >= PSNR_MOVE


# -- PSNRs -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(G.BIT_SHAPES))
@pytest.mark.parametrize("pset,tf", G.TFSETS, ids=G.TFSET_IDS)
def test_bit_path_intensity_and_psnr_move(pset, tf, name):
    _, _, want_i, _, want_ps, energy = G.bit_case(pset, tf, name)
    for kind in _kinds(pset):
        _, _, i, _, ps, _ = G.bit_case(pset, tf, name, kind)
        print(f"bit {pset} tf={tf} {name}: {kind} moves the intensity by {_moved(want_i, i):.3e} of max, "
              f"the psnr by {abs(ps - want_ps):.3e} dB")
        assert abs(ps - want_ps) >= PSNR_MOVE
        if kind == "swap":
            assert _moved(want_i, i) >= FIELD_MOVE
    if pset == "evan" and name == "64x3x2":
        kept = want_i.reshape(3, -1).sum(axis=1) / energy
        print("kept energy", kept)
        assert np.allclose(kept, G.EVAN_KEPT_64, rtol=0.0, atol=5e-3)


@pytest.mark.parametrize("pset", ["aniso", "evan"])
def test_flip_map_and_greedy_psnrs_move(pset):
    cases = [(f"flips N={n}", lambda kind, n=n: G.flips_case(pset, n, kind)[4]) for n in G.FLIP_SHAPES]
    cases += [(f"map N={n}", lambda kind, n=n: G.map_case(pset, n, kind, base_only=True)[4]) for n in G.MAP_SHAPES]
    if pset == "evan":
        cases.append(("greedy", lambda kind: G.greedy_case(kind)[5]))
    for name, base in cases:
        want = base("true")
        for kind in _kinds(pset):
            print(f"{name} {pset}: {kind} moves the base psnr by {abs(base(kind) - want):.3e} dB")
            assert abs(base(kind) - want) >= PSNR_MOVE


def test_greedy_oracle_trace_is_resolved():
    """the accept sequence the walk is compared with: some accepted, some rejected, (nearly) every
    change clear of the resolution below which the test does not compare decisions"""
    _, _, order, acc, psnrs, initial, _, _ = G.greedy_case()
    prev = np.maximum.accumulate(np.concatenate([[initial], psnrs]))[:-1]
    assert 0 < acc.sum() < len(order)
    assert np.sum(np.abs(psnrs - prev) <= 1e-7) < 5


# -- shim --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pset", ["aniso", "evan"])
def test_shim_expected_values_move(pset):
    x, m, t = G.shim_inputs()
    wl = G.wavelengths(pset, 1)[0]
    h, hs = G.shim_transfer(pset, wl), G.shim_transfer(pset, wl, "swap")
    for src in (m, x):
        assert _moved(O.propagate(src.astype(np.float64), h), O.propagate(src.astype(np.float64), hs)) >= FIELD_MOVE
    want_i = G.shim_intensity(pset, x)
    t64 = t.astype(np.float64)
    for kind in _kinds(pset):
        other = G.shim_intensity(pset, x, kind)
        if kind == "swap":
            assert _moved(want_i, other) >= FIELD_MOVE
        for rel in (O.REL_LSQ, O.REL_NONE):
            for e in range(x.shape[0]):
                d = abs(O.relative_psnr(other[e], t64[e], rel) - O.relative_psnr(want_i[e], t64[e], rel))
                print(f"shim {pset} rel {rel} env {e}: {kind} moves the psnr by {d:.3e} dB")
                assert d >= PSNR_MOVE
    for leaf in ("real", "phase"):
        for metric in ("mse", "psnr"):
            _, want_g = G.shim_oracle_gradient(pset, leaf, metric)
            _, other_g = G.shim_oracle_gradient(pset, leaf, metric, "swap")
            print(f"shim {pset} {leaf} {metric}: swap moves the gradient by {_moved(want_g, other_g):.3e} of its max")
            assert _moved(want_g, other_g) >= FIELD_MOVE


def test_shim_oracle_restatement_is_the_oracle_loss():
    """the torch restatement the gradients come from gives O.relative_mse / O.relative_psnr of the
    oracle intensity"""
    x, _, t = G.shim_inputs()
    want_i = G.shim_intensity("evan", x)
    for metric, fn in (("mse", O.relative_mse), ("psnr", O.relative_psnr)):
        got, _ = G.shim_oracle_gradient("evan", "real", metric)
        want = [fn(want_i[e], t[e].astype(np.float64), O.REL_LSQ) for e in range(x.shape[0])]
        assert np.allclose(got, want, rtol=1e-12, atol=0.0)
