"""bf16-rounded pass intermediates (hbx_plan_set_precision, BASELINE configs[4]'s fp32-vs-bf16
sweep) at the headline size.

r03 found the bf16 study variant of k_col2 at N = 1024 non-deterministic while the rounding sat
between the staged LDS read and the non-temporal tile store (launch-to-launch differences of ~0.4 %
in the channel sums, profiles/archive/r03/bf16_determinism_r03f.txt); the f32 product path was
deterministic in every check.  The rounding now happens where each lane writes its line into the
staging region.  These tests pin what the precision sweep relies on: a bf16 group propagation is a
function of its inputs alone, and a flip's PSNR change under bf16 stays within the measured error
of the f32 one (3.0e-7 dB rms, 1.3e-6 dB max over 2,048 flips; profiles/archive/r03/bench_r03g.json).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _state(n):
    import hbx
    rng = np.random.default_rng(0)
    pre = torch.from_numpy(rng.random((24, n, n), np.float32)).cuda()
    tgt = torch.from_numpy(rng.random((3, n, n), np.float32)).cuda()
    return hbx.rgb_config(n), hbx.pack_bits(pre >= 0.5), tgt


@pytest.mark.parametrize("prec_name", ["PRECISION_BF16_STORE", "PRECISION_F16_STORE", "PRECISION_F32"])
def test_reduced_precision_propagation_is_deterministic_1024(prec_name):
    import hbx
    from hbx.plan import Plan
    cfg, mask, tgt = _state(1024)
    plan = Plan(cfg, max_jobs=64, precision=getattr(hbx, prec_name))
    _, s1, _ = plan.propagate(mask.unsqueeze(0), tgt.unsqueeze(0), want_intensity=False)
    _, s2, _ = plan.propagate(mask.unsqueeze(0), tgt.unsqueeze(0), want_intensity=False)
    _, s3, _ = plan.propagate(torch.stack([mask] * 3), torch.stack([tgt] * 3), want_intensity=False)
    assert torch.equal(s1, s2)
    for e in range(3):
        assert torch.equal(s3[e], s1[0])
    f = torch.tensor([5 * 1024 * 1024 + 77 * 1024 + 300] * 5, device="cuda")
    _, g = plan.eval_flips(mask, tgt, s1[0].contiguous(), f)
    assert torch.equal(g, g[:1].expand_as(g))
    plan.close()


def test_bf16_flip_change_close_to_f32_1024():
    import hbx
    from hbx.plan import Plan
    cfg, mask, tgt = _state(1024)
    flips = torch.from_numpy(np.random.default_rng(4).integers(0, 24 * 1024 * 1024, 64)).cuda()
    ch = {}
    for name in ("PRECISION_F32", "PRECISION_BF16_STORE"):
        plan = Plan(cfg, max_jobs=64, precision=getattr(hbx, name))
        _, st, p0 = plan.propagate(mask.unsqueeze(0), tgt.unsqueeze(0), want_intensity=False)
        ps, _ = plan.eval_flips(mask, tgt, st[0].contiguous(), flips)
        ch[name] = (ps - p0).cpu().numpy()
        plan.close()
    e = ch["PRECISION_BF16_STORE"] - ch["PRECISION_F32"]
    # measured 3.0e-7 rms / 1.3e-6 max (2,048 flips); the broken variant gave 3e-3 rms
    assert np.sqrt(np.mean(e * e)) < 1e-6
    assert np.max(np.abs(e)) < 5e-6


# ---------------------------------------------------------------------------------------------------
# The reduced-precision stores against the float64 rounding model (oracle.propagate_rounded)
# ---------------------------------------------------------------------------------------------------
# hbx_plan_set_precision selects k_rowfwd / k_rowfwd32 / k_col2 instantiations the F32 product never runs; the
# tests above and tests/test_gpu_launch_size.py tie them to themselves (determinism, small launch == large
# launch) and to F32 loosely.  Here their outputs are compared with a float64 propagation that rounds at the
# two documented points -- A = FFT_x(u) and B = IFFT_y(FFT_y(A_r) H) / N, re and im each, to the store type --
# through rho(x) = rms(x - model) / rms(model - unrounded float64 field) (tests/_precision_model.py).  A kernel
# that rounds only A, only B, truncates, rounds at another scale in fp16 or misses one of the store sites is
# about one rounding away from the model (rho >= 0.69 on the CPU emulation of each mutant,
# tests/test_precision_model_host.py); a correct float32 implementation is within rho 0.062 there.  The cap
# 0.3 is a condition between the two, not a measurement.  One mono group and one env per case, so every launch
# is the small-launch form; the large form is tied to it bit for bit (tests/test_gpu_launch_size.py).
# Measured figures: profiles/precision_model/rho_gpu.txt (python -m pytest -s prints them).
import functools  # noqa: E402

from oracle import hbx_oracle as O  # noqa: E402
from tests import _precision_model as M  # noqa: E402
from tests.test_gpu_real_field import FIELD_RTOL  # noqa: E402

F32 = 0
PRECISIONS = {F32: "f32", M.BF16: "bf16", M.F16: "fp16"}
STATS_IDENTITY_RTOL = 1e-9    # test_gpu_parity.py::test_parseval_full_size_batch: stats' sum I^2 vs the returned intensity


def _dev(a):
    """a (read-only, cached) numpy array on the device: copied first, torch wants a writable source"""
    return torch.from_numpy(np.array(a)).cuda()


def _plan(ocfg, precision, max_jobs=8):
    import hbx
    cfg = hbx.OpticsConfig(ocfg.height, ocfg.width, ocfg.groups, ocfg.planes, tuple(ocfg.wavelengths),
                           field_kind=ocfg.field_kind)
    plan = hbx.Plan(cfg, max_jobs=max_jobs, precision=precision)
    assert plan.precision == precision
    return plan


@functools.lru_cache(maxsize=None)
def _device(case, precision):
    """(field complex64 [P, N, N] of simulate, intensity float32 [N, N] and chan_stats [3] of propagate) of a
    case on a plan of `precision`, as read-only numpy arrays: one propagation per case and precision"""
    import hbx
    mask, target, _, _ = M.reference(case)
    plan = _plan(M.ocfg_for(case), precision)
    bits = hbx.pack_bits(_dev(mask))[None]
    tgt = _dev(target)[None]
    field, inten_s = plan.simulate(bits, want_intensity=True)
    inten, stats, _ = plan.propagate(bits, tgt)
    torch.cuda.synchronize()
    assert torch.equal(inten, inten_s)
    out = field[0].cpu().numpy(), inten[0, 0].cpu().numpy(), stats[0, 0].cpu().numpy()
    plan.close()
    for a in out:
        a.setflags(write=False)
    return out


def _rhos(case, precision, store_kind):
    """rho of the plan's field and intensity against the model of store_kind"""
    field, inten, _ = _device(case, precision)
    full = M.reference(case)[3]
    want = M.model(case, store_kind)
    return (M.rho(field.astype(np.complex128), want, full),
            M.rho(inten.astype(np.float64), M.plane_mean(want), M.plane_mean(full)))


@pytest.mark.parametrize("store_kind", M.STORES, ids=lambda s: M.STORE_NAMES[s])
@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_reduced_precision_field_and_intensity_vs_rounding_model(case, store_kind):
    """The cap is a condition (2.4 x the worst correct CPU emulation on record, 2.3 x below the best mutant);
    a correct-looking kernel above it is a finding to explain from the code."""
    r_f, r_i = _rhos(case, store_kind, store_kind)
    print(f"rho gpu {M.case_id(case)} {M.STORE_NAMES[store_kind]} plan vs {M.STORE_NAMES[store_kind]} model: "
          f"field {r_f:.4f} intensity {r_i:.4f}")
    assert r_f <= M.RHO_CAP
    assert r_i <= M.RHO_CAP


@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_wrong_store_kind_is_far_from_the_model(case):
    """Negative controls: the statistic tells an F32 plan from the bf16 model and a bf16 plan from the fp16 one"""
    f32_f, f32_i = _rhos(case, F32, M.BF16)
    bf_f, bf_i = _rhos(case, M.BF16, M.F16)
    print(f"rho gpu {M.case_id(case)} controls: f32 plan vs bf16 model field {f32_f:.4f} intensity {f32_i:.4f}; "
          f"bf16 plan vs fp16 model field {bf_f:.4f} intensity {bf_i:.4f}")
    assert min(f32_f, f32_i) >= M.RHO_MUTANT
    assert min(bf_f, bf_i) >= M.RHO_MUTANT


@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_f32_plan_vs_unrounded_model(case):
    field, _, _ = _device(case, F32)
    full = M.reference(case)[3]
    err = np.max(np.abs(field - full)) / np.max(np.abs(full))
    print(f"{M.case_id(case)} f32 plan vs unrounded model: field err {err:.3e} of max|field|")
    assert err <= FIELD_RTOL


@pytest.mark.parametrize("precision", list(PRECISIONS), ids=lambda p: PRECISIONS[p])
@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_chan_stats_are_the_sums_over_the_plans_own_intensity(case, precision):
    """chan_stats = float64 sums of (I T, I^2, T^2) over the intensity the same plan returns, whatever the
    stores rounded on the way to it: the F32 identity (its tolerance, the F32 plan as the control)"""
    _, inten, stats = _device(case, precision)
    want = O.chan_stats(inten, M.reference(case)[1][0])
    rel = np.max(np.abs(stats / want - 1.0))
    print(f"{M.case_id(case)} {PRECISIONS[precision]}: chan_stats vs sums over own intensity, rel err {rel:.2e}")
    assert np.allclose(stats, want, rtol=STATS_IDENTITY_RTOL, atol=0.0)


# -- entry-point identities under every store kind (the F32 plan first: it fixes the identity's form) -----
IDENTITY_CASES = [c for c in M.CASES if c[0] in (64, 256) and c[2] == O.FIELD_AMPLITUDE]


def _flipped(bits, n, action):
    """the packed mask [CH, N, N / 64] with pixel `action` flipped"""
    ch, r, col = action // (n * n), (action // n) % n, action % n
    out = bits.clone()
    out[ch, r, col // 64] ^= torch.ones((), dtype=torch.int64, device=bits.device) << (col % 64)
    return out


@pytest.mark.parametrize("precision", list(PRECISIONS), ids=lambda p: PRECISIONS[p])
@pytest.mark.parametrize("case", IDENTITY_CASES, ids=M.case_id)
def test_eval_flips_equal_propagate_of_the_flipped_mask(case, precision):
    """group_stats[k] and psnr[k] of hbx_eval_flips are hbx_propagate's of the mask with that bit flipped, on the
    same plan, bit for bit: the flip is applied to the loaded words and every pass after it is the same code."""
    import hbx
    n, p = case[0], case[1]
    mask, target, _, _ = M.reference(case)
    rng = np.random.default_rng(case[3])
    flips = np.concatenate([[0, p * n * n - 1], rng.integers(0, p * n * n, 6)]).astype(np.int64)   # K = 8, both corners
    plan = _plan(M.ocfg_for(case), precision)
    try:
        bits = hbx.pack_bits(_dev(mask))
        tgt = _dev(target)
        _, st, p0 = plan.propagate(bits[None], tgt[None], want_intensity=False)
        ps, gs = plan.eval_flips(bits, tgt, st[0].contiguous(), torch.from_numpy(flips).cuda())
        for k, a in enumerate(flips):
            _, st_k, ps_k = plan.propagate(_flipped(bits, n, int(a))[None], tgt[None], want_intensity=False)
            assert torch.equal(gs[k], st_k[0, 0]), (k, int(a))
            assert torch.equal(ps[k], ps_k[0]), (k, int(a))
        assert len(torch.unique(ps)) == len(flips) and not torch.any(ps == p0)   # every flip moved the PSNR
    finally:
        plan.close()


@pytest.mark.parametrize("precision", list(PRECISIONS), ids=lambda p: PRECISIONS[p])
def test_env_step_fft_equals_planes_under_store_kinds(precision):
    """One FFT-mode and one plane-cached env step, B = 2, at 256 x 8 (the plane cache is built for N = 256 /
    896 / 1024): the same state, recon_image and statistics, bit for bit (tests/test_gpu_planes.py's identity)."""
    import hbx
    from hbx.env import HologramVecEnv, OBS_KEYS
    cfg = hbx.mono_config(256)
    g = torch.Generator(device="cuda").manual_seed(77)
    pres = [torch.rand((8, 256, 256), generator=g, device="cuda") for _ in range(2)]
    tgts = [torch.rand((1, 256, 256), generator=g, device="cuda") for _ in range(2)]
    envs = []
    for mode in ("fft", "planes"):
        env = HologramVecEnv(cfg, 2, lambda i: tgts[i], pre_model_source=lambda i: pres[i], auto_reset=False,
                             obs_keys=OBS_KEYS, mode=mode)
        env.plan.precision = precision
        assert env.plan.precision == precision
        envs.append(env)
    fft, planes = envs
    o1, o2 = fft.reset(), planes.reset()
    assert torch.equal(o1["recon_image"], o2["recon_image"])
    acts = torch.tensor([3 * 65536 + 255, 8 * 65536 - 1], device="cuda")      # an inner plane; the last pixel
    o1, r1, d1, _ = fft.step(acts)
    o2, r2, d2, _ = planes.step(acts)
    assert np.array_equal(r1, r2) and np.array_equal(d1, d2)
    assert torch.equal(o1["state"], o2["state"])
    assert torch.equal(o1["recon_image"], o2["recon_image"])
    for k in ("mask", "record", "chan_stats", "prev_psnr", "init_psnr", "steps", "flip_count", "sustained"):
        assert torch.equal(getattr(fft.state, k), getattr(planes.state, k)), k
    l1, l2 = fft.last_step(), planes.last_step()
    assert np.array_equal(l1["psnr"], l2["psnr"]) and np.array_equal(l1["accepted"], l2["accepted"])
    assert np.all(np.isfinite(l1["psnr"])) and np.all(r1 != 0.0)


@pytest.mark.parametrize("precision", list(PRECISIONS), ids=lambda p: PRECISIONS[p])
def test_fft_greedy_walk_equals_host_batches_under_store_kinds(precision):
    """A 512-candidate FFT-mode greedy prefix at 256 x 8: the device-decided walk on the plane cache and the
    host-decided full re-propagation accept the same candidates with the same PSNR bits and leave the same
    mask (tests/test_gpu_dbs_headline.py::test_fft_greedy_plane_cache_equals_full_repropagation's identity)."""
    import hbx
    from hbx import dbs
    case = IDENTITY_CASES[-1]
    assert case[0] == 256
    mask, target, _, _ = M.reference(case)
    order = np.random.default_rng(9).permutation(8 * 256 * 256)[:512]
    runs = []
    for planes, walk in ((False, False), (True, True)):
        plan = _plan(M.ocfg_for(case), precision, max_jobs=64)
        bits = hbx.pack_bits(_dev(mask))
        res = dbs.greedy(plan, bits, _dev(target), order, mode="fft", planes=planes,
                         device_walk=walk)
        runs.append((res, bits.cpu().numpy()))
        plan.close()
    (host, m_host), (walk, m_walk) = runs
    print(f"{PRECISIONS[precision]}: {host.steps} candidates, {len(host.accepted_positions)} accepts")
    assert walk.accepted_positions == host.accepted_positions
    assert walk.accepted_psnr == host.accepted_psnr                       # bit for bit
    assert walk.initial_psnr == host.initial_psnr and walk.final_psnr == host.final_psnr
    assert walk.steps == host.steps == 512
    assert np.array_equal(m_host, m_walk)
    assert 20 < len(host.accepted_positions) < 512
