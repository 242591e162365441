"""The annealed FFT-mode greedy walk -- an EXTENSION, no reference counterpart (the reference has
the strict rule psnr > prev alone, DBS_1024_24.py:355).

The rule (hbx.h hbx_dbs_walk_planes_anneal, hbx.dbs.first_accepting, tests/_anneal.py): the
candidate at position q of the order is accepted iff ps > (prev - slack[q]) in float64.  Checked
here as the fill extension is: the device-decided walk equals the host-decided batches (and, at
256, planes=False) bit for bit; both follow the float64 loop's fixture up to a candidate whose
|margin| lies within the f32 FFT resolution FFT_TOL_DB (the fixtures hold none in the stretches the
test relies on: tests/test_dbs_anneal_host.py); greedy_many equals the single walks; and the raw
C-ABI call's argument checks and slack bounds."""
import ctypes as C
import math
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import hbx_oracle as O  # noqa: E402

from tests import _anneal  # noqa: E402
from tests.test_gpu_dbs_headline import FFT_TOL_DB, _dev, _first_difference, _fixture  # noqa: E402

F256 = "dbs_ratio05_256.npz"
F1024 = "dbs_prefix_1024x24_16k.npz"


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm GPU")
    import hbx
    hbx.load_library()
    yield


ROUTES = {"device": dict(planes=True, device_walk=True), "host": dict(planes=True, device_walk=False),
          "full": dict(planes=False)}


def _run(ocfg, pre, tgt, order, route, max_jobs=256, **kw):
    from hbx import dbs
    plan, mask, target = _dev(ocfg, pre, tgt, max_jobs=max_jobs)
    res = dbs.greedy(plan, mask, target, order, mode="fft", **ROUTES[route], **kw)
    m = mask.cpu().numpy()
    plan.close()
    return res, m


def _same(a, b):
    (ra, ma), (rb, mb) = a, b
    assert ra.accepted_positions == rb.accepted_positions
    assert ra.accepted_psnr == rb.accepted_psnr                       # bit for bit
    assert ra.steps == rb.steps and ra.stopped_early == rb.stopped_early
    assert np.array_equal(ma, mb)
    assert (ra.best_psnr, ra.best_accepts) == (rb.best_psnr, rb.best_accepts)
    assert ra.fill_counts == rb.fill_counts


def _downhill(res):
    ps = np.asarray([res.initial_psnr] + list(res.accepted_psnr))
    return int((np.diff(ps) < 0).sum())


@pytest.mark.parametrize("name", list(_anneal.ANNEAL_FIXTURES))
def test_anneal_device_host_and_oracle_agree(golden_dir, name):
    from hbx import dbs
    assert FFT_TOL_DB == 2e-9            # the bound tests/test_dbs_anneal_host.py holds the fixtures to
    base, n, t0, t1, seed = _anneal.ANNEAL_FIXTURES[name]
    fx = np.load(os.path.join(golden_dir, name), allow_pickle=False)
    d, ocfg, pre, tgt, order = _fixture(golden_dir, base)
    order = order[:n]
    slack = dbs.metropolis_slack(n, t0, t1, seed)
    walk = _run(ocfg, pre, tgt, order, "device", slack=slack)
    _same(walk, _run(ocfg, pre, tgt, order, "host", slack=slack))
    if ocfg.height == 256:
        _same(walk, _run(ocfg, pre, tgt, order, "full", slack=slack))
    res = walk[0]
    assert res.steps == n
    down = _downhill(res)
    first = _first_difference(res.accepted_positions, fx["accepted"])
    print(f"{name}: {len(res.accepted_positions)} accepts ({down} downhill) of {n}, fixture {int(fx['accepted'].sum())}; "
          f"first difference {first}; final {res.final_psnr:.6f} best {res.best_psnr:.6f} after {res.best_accepts}")
    assert down > 50
    if first is None:
        assert abs(res.final_psnr - float(fx["final_psnr"])) <= 1e-4
    else:
        margin = float(fx["margin"][first])
        assert abs(margin) <= FFT_TOL_DB and first >= n // 4, \
            f"candidate {first}: decision differs from the float64 loop's at margin {margin:.3e} dB"


def test_zero_slack_equals_greedy(golden_dir):
    d, ocfg, pre, tgt, order = _fixture(golden_dir, F256)
    order = order[:1500]
    for route in ("device", "host"):
        _same(_run(ocfg, pre, tgt, order, route, slack=np.zeros(len(order))), _run(ocfg, pre, tgt, order, route))


def test_anneal_896_standalone_decision(golden_dir):
    """N = 896 decides in a launch of its own behind each batch (k_walk_planes_anneal, decide = 1):
    the device walk equals the host-decided batches there too."""
    from hbx import dbs
    d, ocfg, pre, tgt, order = _fixture(golden_dir, "dbs_prefix_896x24.npz")
    o = order[:400]
    slack = dbs.metropolis_slack(400, 2e-6, 2e-8, 9)
    dev = _run(ocfg, pre, tgt, o, "device", max_jobs=16, slack=slack)
    _same(dev, _run(ocfg, pre, tgt, o, "host", max_jobs=16, slack=slack))
    assert dev[0].steps == 400 and _downhill(dev[0]) > 10


def test_anneal_edges(golden_dir):
    from hbx import dbs
    d, ocfg, pre, tgt, order = _fixture(golden_dir, F256)
    o = order[:600]
    both = lambda **kw: (_run(ocfg, pre, tgt, o, "device", **kw), _run(ocfg, pre, tgt, o, "host", **kw))
    # +inf everywhere: every visited candidate is accepted
    dev, host = both(slack=np.full(600, np.inf))
    _same(dev, host)
    assert dev[0].steps == 600 and dev[0].accepted_positions == list(range(600))
    # a minimum gain g: the median greedy gain of these candidates
    greedy = _run(ocfg, pre, tgt, o, "device")[0]
    g = float(np.median(np.diff([greedy.initial_psnr] + greedy.accepted_psnr)))
    assert g > 0
    dev, host = both(slack=np.full(600, -g))
    _same(dev, host)
    chain = [dev[0].initial_psnr] + dev[0].accepted_psnr
    assert 0 < len(chain) - 1 < len(greedy.accepted_positions)
    assert all(ps > prev - (-g) for prev, ps in zip(chain, chain[1:]))          # the predicate's own expression
    # NaN on a stretch: none of its positions is accepted
    s = np.zeros(600)
    s[100:300] = np.nan
    dev, host = both(slack=s)
    _same(dev, host)
    pos = np.asarray(dev[0].accepted_positions)
    assert dev[0].steps == 600 and not ((pos >= 100) & (pos < 300)).any() and (pos >= 300).any() and (pos < 100).any()
    # k_max = 1, and stop_diff reached under a schedule that goes downhill
    m = dbs.metropolis_slack(600, 1.25e-4, 1.25e-6, 6)
    dev, host = both(slack=m, k_max=1)
    _same(dev, host)
    free = dev[0]
    assert _downhill(free) > 10
    stop = 0.5 * (free.best_psnr - free.initial_psnr)
    dev, host = both(slack=m, stop_diff=stop)
    _same(dev, host)
    assert dev[0].stopped_early and dev[0].steps < 600 and dev[0].final_psnr - dev[0].initial_psnr >= stop
    assert dev[0].accepted_positions == free.accepted_positions[:len(dev[0].accepted_positions)]
    assert all(p - free.initial_psnr < stop for p in dev[0].accepted_psnr[:-1])


def test_anneal_with_fill_ratio(golden_dir):
    from hbx import dbs
    d, ocfg, pre, tgt, order = _fixture(golden_dir, F256)
    o = order[:1500]
    per_group = ocfg.planes * ocfg.height * ocfg.width
    bits0 = (pre >= 0.5).astype(np.int8)
    c0 = int(O.group_fill_counts(bits0, 1)[0])
    ratio, tol = c0 / per_group, 1
    target = dbs.fill_target(ratio, ocfg.planes, ocfg.height, ocfg.width)
    kw = dict(fill_ratio=ratio, fill_tol=tol)
    m = dbs.metropolis_slack(1500, 1.25e-4, 1.25e-6, 6)
    dev, host = (_run(ocfg, pre, tgt, o, r, slack=m, **kw) for r in ("device", "host"))
    _same(dev, host)
    assert _downhill(dev[0]) > 10
    assert abs(dev[0].fill_counts[0] - target) <= max(abs(c0 - target), tol)
    assert dev[0].fill_counts == [int(v) for v in O.group_fill_counts(
        np.unpackbits(dev[1].view(np.uint8), bitorder="little").reshape(bits0.shape), 1)]
    # +inf: every admissible candidate is accepted and no other -- integer bookkeeping says which
    dev, host = (_run(ocfg, pre, tgt, o, r, slack=np.full(1500, np.inf), **kw) for r in ("device", "host"))
    _same(dev, host)
    bits, count, want = bits0.copy(), c0, []
    for q, a in enumerate(o):
        ch, r, col = (int(v) for v in O.decode_action(int(a), ocfg.height, ocfg.width))
        if dbs.fill_admissible(count, target, tol, int(bits[ch, r, col])):
            count += -1 if bits[ch, r, col] else 1
            bits[ch, r, col] ^= 1
            want.append(q)
    assert 0 < len(want) < 1500 and dev[0].accepted_positions == want and dev[0].fill_counts == [count]


def test_anneal_greedy_many_equals_single_walks(golden_dir):
    from hbx import dbs
    d, ocfg, pre, tgt, order = _fixture(golden_dir, F1024)
    rng = np.random.default_rng(9)
    imgs = [(pre, tgt, order[:1000], dbs.metropolis_slack(1000, 2e-6, 2e-8, 9)),
            (rng.random(pre.shape).astype(pre.dtype), rng.random(tgt.shape).astype(tgt.dtype),
             rng.permutation(order)[:800], None)]
    single = [_run(ocfg, p_, t_, o_, "device", max_jobs=16, slack=s_) for p_, t_, o_, s_ in imgs]
    assert _downhill(single[0][0]) > 20 and _downhill(single[1][0]) == 0
    devs = [_dev(ocfg, p_, t_, max_jobs=16) for p_, t_, _, _ in imgs]
    many = dbs.greedy_many([x[0] for x in devs], [x[1] for x in devs], [x[2] for x in devs],
                           [o_ for _, _, o_, _ in imgs], mode="fft", slacks=[s_ for _, _, _, s_ in imgs])
    for want, got, (plan, gm, _) in zip(single, many, devs):
        _same(want, (got, gm.cpu().numpy()))
        plan.close()


def test_replay_rebuilds_final_and_best_state(golden_dir):
    import hbx
    from hbx import dbs
    d, ocfg, pre, tgt, order = _fixture(golden_dir, F256)
    o = order[:1500]
    # hot to the end, so that the walk ends below its best state
    res, final = _run(ocfg, pre, tgt, o, "device", slack=dbs.metropolis_slack(1500, 2.5e-4, 2.5e-4, 4))
    plan, mask0, target = _dev(ocfg, pre, tgt)
    assert np.array_equal(dbs.replay(mask0, o, res.accepted_positions).cpu().numpy(), final)
    assert 0 < res.best_accepts < len(res.accepted_positions) and res.best_psnr > res.final_psnr
    assert res.best_psnr == max(res.accepted_psnr) == res.accepted_psnr[res.best_accepts - 1]
    best = dbs.replay(mask0, o, res.accepted_positions[:res.best_accepts])
    _, _, ps = plan.propagate(best.unsqueeze(0), target.unsqueeze(0), want_intensity=False)
    assert abs(float(ps.item()) - res.best_psnr) <= 1e-4
    plan.close()


# ---------------------------------------------------------------------------- the raw C-ABI call
class _Raw:
    """One walk's buffers, as hbx.dbs._PlanesWalk sets them up, for direct calls into the library."""

    def __init__(self, ocfg, pre, tgt, order, K=4):
        from hbx import _lib
        self.plan, self.mask, self.target = _dev(ocfg, pre, tgt)
        plan, dev = self.plan, self.plan.device
        self.K, self.total = K, len(order)
        self.order = torch.as_tensor(np.asarray(order, np.int64)).to(dev)
        self.pool = plan.plane_pool(K)
        self.spares = plan._check_pool(*self.pool)
        stats, psnr0 = plan.planes_fill(self.mask, self.target, *self.pool)
        self.stats = stats.contiguous()
        w = _lib.DbsWalk()
        w.total = self.total
        w.prev_psnr = w.init_psnr = float(psnr0.item())
        w.last_psnr = math.nan
        w.commit_ch = -1
        self.wbuf = torch.frombuffer(bytearray(bytes(w)), dtype=torch.uint8).to(dev)
        self.log_pos = torch.full((self.total,), -1, dtype=torch.int64, device=dev)
        self.log_psnr = torch.zeros(self.total, dtype=torch.float64, device=dev)

    def args(self):
        from hbx.plan import _ptr
        return [self.plan._h, _ptr(self.mask), _ptr(self.target), _ptr(self.stats), _ptr(self.pool[0]),
                _ptr(self.pool[1]), self.spares, _ptr(self.order), self.total, _ptr(self.wbuf), _ptr(self.log_pos),
                _ptr(self.log_psnr), self.total, self.K, self.total, None, 0, 0]     # batches = total: it finishes

    def state(self):
        from hbx import _lib
        torch.cuda.synchronize()
        st = _lib.DbsWalk.from_buffer_copy(self.wbuf.cpu().numpy().tobytes())
        n = int(st.accepted)
        return st, self.log_pos[:n].cpu().tolist(), self.log_psnr[:n].cpu().tolist(), self.mask.cpu().numpy()


def test_raw_abi_slack_checks_and_bounds(golden_dir):
    from hbx import _lib, dbs
    from hbx.plan import _stream
    lib = _lib.load()
    d, ocfg, pre, tgt, order = _fixture(golden_dir, F256)
    o = order[:300]
    slack = dbs.metropolis_slack(300, 1.25e-4, 1.25e-6, 6)
    # n_slack one short: refused before anything is enqueued, state and mask untouched
    r = _Raw(ocfg, pre, tgt, o)
    s_t = torch.from_numpy(slack).cuda()
    torch.cuda.synchronize()
    before = (r.wbuf.cpu().numpy().copy(), r.mask.cpu().numpy().copy(), r.stats.cpu().numpy().copy())
    rc = lib.hbx_dbs_walk_planes_anneal(*r.args(), C.c_void_p(s_t.data_ptr()), 299, _stream(None))
    assert rc == _lib.ERR_INVALID and b"slack" in lib.hbx_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(r.wbuf.cpu().numpy(), before[0]) and np.array_equal(r.mask.cpu().numpy(), before[1])
    assert np.array_equal(r.stats.cpu().numpy(), before[2]) and int((r.log_pos >= 0).sum()) == 0
    # the slack inside a NaN-filled allocation, n_slack exactly the candidates visited: a read
    # outside it rejects where the host route (its own copy of the slack) accepts
    big = torch.full((4096,), math.nan, dtype=torch.float64, device="cuda")
    big[1024:1324] = s_t
    rc = lib.hbx_dbs_walk_planes_anneal(*r.args(), C.c_void_p(big.data_ptr() + 1024 * 8), 300, _stream(None))
    assert rc == 0, lib.hbx_last_error()
    st, pos, ps, m = r.state()
    host, m_host = _run(ocfg, pre, tgt, o, "host", slack=slack)
    assert st.done and int(st.pos) == 300 and pos == host.accepted_positions and ps == host.accepted_psnr
    assert np.array_equal(m, m_host) and _downhill(host) > 10
    assert bool(torch.isnan(big[:1024]).all()) and bool(torch.isnan(big[1324:]).all())
    r.plan.close()
    # slack NULL is hbx_dbs_walk_planes_fill
    a, b = _Raw(ocfg, pre, tgt, o), _Raw(ocfg, pre, tgt, o)
    assert lib.hbx_dbs_walk_planes_anneal(*a.args(), None, 0, _stream(None)) == 0
    assert lib.hbx_dbs_walk_planes_fill(*b.args(), _stream(None)) == 0
    sa, sb = a.state(), b.state()
    assert bytes(sa[0]) == bytes(sb[0]) and sa[1] == sb[1] and sa[2] == sb[2] and np.array_equal(sa[3], sb[3])
    assert sa[0].done and len(sa[1]) > 20
    a.plan.close()
    b.plan.close()
