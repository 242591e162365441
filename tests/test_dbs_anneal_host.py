"""Host side of the annealed FFT-mode walk (hbx.dbs.greedy(slack=), an EXTENSION with no reference
counterpart): the schedule helpers, the generalised first-accept helper, replay, the best-state
fields, the refusals before any GPU use, the header's documentation, and the 256 fixture
regenerated with the float64 loop of tests/_anneal.py."""
import os
import re

import numpy as np
import pytest

from tests import _anneal
from tests.conftest import ROOT

FFT_TOL_DB = 2e-9        # tests/test_gpu_dbs_headline.py FFT_TOL_DB (a GPU module: restated, asserted equal on the GPU)


def _dbs():
    pytest.importorskip("torch")
    from hbx import dbs
    return dbs


# ---------------------------------------------------------------------------- schedule helpers
def test_metropolis_slack_formula_bits_and_determinism():
    dbs = _dbs()
    total, t0, t1, seed = 1000, 1.25e-4, 1.25e-6, 6
    got = dbs.metropolis_slack(total, t0, t1, seed)
    assert got.dtype == np.float64 and got.shape == (total,)
    u = np.random.default_rng(seed).random(total)
    temp = np.array([t0 * (t1 / t0) ** (i / (total - 1)) for i in range(total)])
    want = -temp * np.log1p(-u)
    assert np.allclose(got, want, rtol=1e-14, atol=0) and np.all(got >= 0)
    assert np.array_equal(got, dbs.metropolis_slack(total, t0, t1, seed))          # same seed, same bits
    assert not np.array_equal(got, dbs.metropolis_slack(total, t0, t1, seed + 1))
    # the Metropolis probability: P(slack > d) = exp(-d / T)
    big = dbs.metropolis_slack(200000, 1e-3, 1e-3, 1)
    assert abs((big > 1e-3).mean() - np.exp(-1.0)) < 5e-3
    one = dbs.metropolis_slack(1, 0.5, 0.1, 3)
    assert one.shape == (1,) and one[0] == -0.5 * np.log1p(-np.random.default_rng(3).random(1))[0]


def test_threshold_slack_formula():
    dbs = _dbs()
    got = dbs.threshold_slack(257, 4e-3, 4e-6)
    want = np.array([4e-3 * (4e-6 / 4e-3) ** (i / 256) for i in range(257)])
    assert got.dtype == np.float64 and np.allclose(got, want, rtol=1e-14, atol=0)
    assert got[0] == 4e-3 and abs(got[-1] / 4e-6 - 1) < 1e-12 and np.all(np.diff(got) < 0)
    assert np.array_equal(dbs.threshold_slack(1, 2.0, 1.0), [2.0])


@pytest.mark.parametrize("bad", [(0, 1.0, 0.1), (-3, 1.0, 0.1), (2.5, 1.0, 0.1), (10, 0.0, 0.1), (10, 1.0, 0.0),
                                 (10, -1.0, 0.1), (10, 1.0, -0.1), (10, np.inf, 0.1), (10, 1.0, np.nan)])
def test_schedule_helpers_refuse_bad_arguments(bad):
    dbs = _dbs()
    with pytest.raises(ValueError):
        dbs.metropolis_slack(*bad, 0)
    with pytest.raises(ValueError):
        dbs.threshold_slack(*bad)


# ---------------------------------------------------------------------------- first_accepting
def _brute(ps, prev, slack):
    for i in range(len(ps)):
        if float(ps[i]) > float(prev) - float(slack[i]):
            return i
    return None


def test_first_accepting_against_brute_force():
    dbs = _dbs()
    rng = np.random.default_rng(0)
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -1e-3, 1e-3])
    for trial in range(300):
        k = int(rng.integers(1, 40))
        prev = 20.0 + rng.normal() * 1e-3
        ps = prev + rng.normal(size=k) * 1e-3
        ps[rng.random(k) < 0.15] = np.nan                    # candidates without a PSNR
        slack = rng.normal(size=k) * 1e-3
        sel = rng.random(k) < 0.4
        slack[sel] = rng.choice(special, size=int(sel.sum()))
        assert dbs.first_accepting(ps, prev, slack) == _brute(ps, prev, slack), (trial, ps, prev, slack)
        zero = np.zeros(k)
        assert dbs.first_accepting(ps, prev, zero) == dbs.first_improving(ps, prev)
    prev = 10.0
    assert dbs.first_accepting(np.array([9.0, 11.0]), prev, np.array([np.nan, np.nan])) is None     # NaN rejects
    assert dbs.first_accepting(np.array([np.nan, -50.0]), prev, np.array([np.inf, np.inf])) == 1   # +inf: any PSNR
    assert dbs.first_accepting(np.array([10.4, 10.6]), prev, np.array([-0.5, -0.5])) == 1          # minimum gain
    assert dbs.first_accepting(np.array([10.5]), prev, np.array([-0.5])) is None                   # "more than"
    assert dbs.first_accepting(np.array([11.0]), prev, np.array([-np.inf])) is None
    # one subtraction rounded once, then the compare: not ps + slack > prev
    prev, s = 1.0, 2.0 ** -54
    assert dbs.first_accepting(np.array([1.0]), prev, np.array([s])) is None        # 1 - 2^-54 rounds to 1


# ---------------------------------------------------------------------------- replay, best state
def test_replay_against_bitwise_reference_with_repeated_positions():
    torch = pytest.importorskip("torch")
    dbs = _dbs()
    rng = np.random.default_rng(5)
    ch, h, w = 3, 8, 128
    bits = rng.integers(0, 2, size=(ch, h, w)).astype(np.uint8)
    packed = np.packbits(bits.reshape(ch, h, w // 64, 64), axis=-1, bitorder="little").view("<u8").reshape(ch, h, w // 64)
    mask0 = packed.astype(np.uint64).view(np.int64)
    order = np.concatenate([rng.permutation(ch * h * w) for _ in range(3)])        # every pixel three times
    pos = np.sort(rng.choice(len(order), size=2500, replace=False))
    pos = np.concatenate([pos, pos[:7]])                                           # a position named twice too
    want = bits.copy()
    for p in pos:
        a = int(order[p])
        want[a // (h * w), (a % (h * w)) // w, a % w] ^= 1
    want_packed = np.packbits(want.reshape(ch, h, w // 64, 64), axis=-1, bitorder="little").view("<u8").reshape(ch, h, w // 64)
    got = dbs.replay(mask0, order, pos)
    assert got.dtype == np.int64 and np.array_equal(got.view(np.uint64), want_packed)
    assert np.array_equal(mask0.view(np.uint64), packed)                            # the start mask is left alone
    got_t = dbs.replay(torch.from_numpy(mask0.copy()), order, pos.tolist())
    assert isinstance(got_t, torch.Tensor) and np.array_equal(got_t.numpy(), got)
    assert np.array_equal(dbs.replay(mask0, order, []), mask0)
    twice = dbs.replay(mask0, order, [5, 5])
    assert np.array_equal(twice, mask0)
    with pytest.raises(ValueError):
        dbs.replay(mask0, np.array([ch * h * w]), [0])


def test_greedy_result_best_fields():
    dbs = _dbs()
    r = dbs.GreedyResult(10.0, 10.3, 5, [0, 2, 4], [10.1, 10.2, 10.3], 2)          # an existing construction
    assert (r.best_psnr, r.best_accepts) == (10.3, 3) == (r.final_psnr, len(r.accepted_positions))
    r = dbs.GreedyResult(10.0, 10.0, 3, [], [], 1)
    assert (r.best_psnr, r.best_accepts) == (10.0, 0)
    r = dbs.GreedyResult(10.0, 9.9, 9, [0, 1, 2, 3, 4], [10.2, 10.1, 10.4, 10.4, 9.9], 3)
    assert (r.best_psnr, r.best_accepts) == (10.4, 3)                               # the first time the maximum held
    r = dbs.GreedyResult(10.0, 9.5, 9, [0, 1], [9.0, 9.5], 3)
    assert (r.best_psnr, r.best_accepts) == (10.0, 0)                               # never above the start
    assert dbs.best_of_log(1.0, [1.0, 1.0]) == (1.0, 0)


# ---------------------------------------------------------------------------- refusals before any GPU use
@pytest.fixture
def no_gpu(monkeypatch):
    torch = pytest.importorskip("torch")

    def fail():
        raise AssertionError("reached the GPU runtime")
    monkeypatch.setattr(torch.cuda, "is_available", fail)
    return torch


class _NoPlan:
    def __getattr__(self, name):
        raise AssertionError(f"reached the plan ({name})")


def test_greedy_refuses_bad_slack_before_any_gpu_use(no_gpu):
    dbs = _dbs()
    order = np.arange(100)
    ok = np.zeros(100)
    bad = [dict(slack=ok, mode="psf"), dict(slack=ok, mode="psf_host"),
           dict(slack=np.zeros(99)),                                    # too short
           dict(slack=np.zeros(49), max_candidates=50),
           dict(slack=np.zeros((100, 1))),                              # not one value per position
           dict(slack=["a"] * 100), dict(slack=object()), dict(slack=[[0.0], [0.0, 1.0]])]
    for kw in bad:
        with pytest.raises(ValueError):
            dbs.greedy(_NoPlan(), None, None, order, **kw)
    plans = [_NoPlan(), _NoPlan()]
    many = [dict(slacks=[ok, None], mode="psf"), dict(slacks=[ok], mode="fft"),
            dict(slacks=[None, np.zeros(99)], mode="fft"), dict(slacks=[["x"] * 100, None], mode="fft"),
            dict(slacks=[np.zeros(9), None], mode="fft", max_candidates=10)]
    for kw in many:
        with pytest.raises(ValueError):
            dbs.greedy_many(plans, [None, None], [None, None], [order, order], **kw)


# ---------------------------------------------------------------------------- C-ABI declaration
def test_header_declares_the_annealed_walk():
    from hbx import _lib
    text = open(os.path.join(ROOT, "include", "hbx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    fill = re.search(r"\bint\s+hbx_dbs_walk_planes_fill\s*\((.*?)\)\s*;", src, flags=re.S).group(1)
    ann = re.search(r"\bint\s+hbx_dbs_walk_planes_anneal\s*\((.*?)\)\s*;", src, flags=re.S).group(1)
    norm = lambda s: [re.sub(r"\s+", " ", a).strip() for a in s.split(",")]
    f, a = norm(fill), norm(ann)
    # the fill call's arguments, then the slack and its length, then the stream
    assert a == f[:-1] + ["const double* slack", "int64_t n_slack", "void* stream"]
    assert "hbx_dbs_walk_planes_anneal" in _lib.EXPORTED_SYMBOLS
    assert int(re.search(r"#define\s+HBX_ABI_VERSION\s+(\d+)", src).group(1)) == _lib.ABI_VERSION == 15
    doc = [c for c in re.findall(r"/\*.*?\*/", text, flags=re.S) if "prev_psnr - slack[q]" in c]
    assert len(doc) == 1
    doc = re.sub(r"\s*\n\s*\*\s*", " ", doc[0])
    for word in ("EXTENSION, no reference counterpart", "NaN", "+inf", "negative slack", "stop_diff", "HBX_ERR_INVALID",
                 "rounded once", "slack NULL", "hbx_dbs_walk_planes_fill", "accept log"):
        assert word in doc, word


def test_library_exports_the_annealed_walk_and_null_plan_is_invalid():
    import ctypes as C
    from hbx import _lib
    lib = _lib.load()
    fn = lib.hbx_dbs_walk_planes_anneal
    assert fn.restype is C.c_int and len(fn.argtypes) == 21
    assert fn(None, None, None, None, None, None, 1, None, 0, None, None, None, 0, 1, 1, None, 0, 0, None, 0,
              None) == _lib.ERR_INVALID


# ---------------------------------------------------------------------------- the fixtures
def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name), allow_pickle=False)


def test_fixture_256_regenerates_array_for_array(golden_dir):
    _dbs()
    name = "dbs_anneal_256.npz"
    d = _load(golden_dir, name)
    fresh = _anneal.make_fixture(golden_dir, name)
    assert set(d.files) == set(fresh)
    for key in d.files:
        assert np.array_equal(d[key], np.asarray(fresh[key]), equal_nan=True), key
    base, n, t0, t1, seed = _anneal.ANNEAL_FIXTURES[name]
    assert (int(d["n"]), float(d["t_start"]), float(d["t_end"]), int(d["slack_seed"])) == (n, t0, t1, seed)


@pytest.mark.parametrize("name", list(_anneal.ANNEAL_FIXTURES))
def test_fixtures_hold_what_the_gpu_test_relies_on(golden_dir, name):
    """No |margin| within the f32 FFT resolution FFT_TOL_DB in the 256 fixture, none in the first
    quarter of the 1024 fixture; the schedule goes downhill often enough to exercise the rule."""
    d = _load(golden_dir, name)
    acc, ps, m = d["accepted"], d["psnr"], d["margin"]
    n = int(d["n"])
    assert len(acc) == len(ps) == len(m) == n == _anneal.ANNEAL_FIXTURES[name][1]
    assert np.array_equal(acc, m > 0) and not np.isnan(m).any()
    upto = n if name == "dbs_anneal_256.npz" else n // 4
    assert np.abs(m[:upto]).min() > FFT_TOL_DB, (int(np.argmin(np.abs(m[:upto]))), float(np.abs(m[:upto]).min()))
    prev = np.concatenate([[float(d["initial_psnr"])], ps[acc]])[:-1]
    downhill = int((ps[acc] < prev).sum())
    assert downhill > 50 and float(d["final_psnr"]) == ps[acc][-1]
    print(f"{name}: {int(acc.sum())} accepts, {downhill} downhill, smallest |margin| {np.abs(m).min():.3g} dB at "
          f"{int(np.argmin(np.abs(m)))}")
