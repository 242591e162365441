"""Calls on one plan, issued in stream order, do not depend on what the plan ran before.

A hbx_plan_t owns one set of device workspaces (ws_a, ws_b, partial, job_stats, job_inten, jobs, the walk
ticket, ring and phase, the lazily built hpsf / map_* / walk scratch / depth tables) and every entry point
runs in them with a layout of its own.  The other GPU files check each entry point on a plan created for
that test; here every comparison is torch.equal between a USED plan and a FRESH one: same inputs, same
call, every array the call writes.  No tolerance appears.  The calls come from tests/_plan_ops.py (the op
catalogue; tests/test_plan_ops_host.py holds it to include/hbx.h), each in two batch sizes: `one` (a single
env or candidate) and `ragged` (2 (max_jobs // G) + 1 envs; for the flip ops, where a candidate is one job,
2 max_jobs + 1 candidates: two full launches and a short last one, every job slot touched).

Shapes (name: N, G groups x P planes, max_jobs) and the ops run on each:
  256x12    256, 3 x 4, 6    the full catalogue, both sizes: tiled R = 16 forms, plane cache.  backward_stack
                             runs at D = 2 here: hbx_backward_stack needs max_jobs >= G D, and 6 < 3 * 3
  64x2      64, 1 x 2, 3     the full catalogue minus the plane-cache ops (no plane cache at N = 64)
  896x2     896, 1 x 2, 3    the full catalogue (hbx_passes896.hip, its own reduce and walk decision)
  1024x2    1024, 1 x 2, 4   propagate, eval_flips, evaluate_complex, evaluate_phase, phase_backward,
                             evaluate_stack_phase, dbs_walk_planes (and the poison ops)
  walking   256, 1 x 2, 256  propagate, simulate, evaluate_real, evaluate_complex, eval_flips (and the poison
                             ops): the full launches of the ragged size (256 jobs) run the walking forms,
                             asserted through tests/_launch_size.walking; the short last launch (1 job) the
                             small ones.  Outputs of this shape above 64 MiB are kept in host memory and
                             compared piecewise, which keeps the file's device memory below 2 GiB
Poison ops (all-NaN inputs: evaluate_complex, evaluate_real, backward_stack at the deepest stack the job
slots take, eval_flips_psf, flip_map) are not compared; each asserts that its own outputs are all NaN (a PSNR
formed from NaN statistics is +inf: psnr_from returns INFINITY unless mse > 0, csrc/hbx_internal.hpp).  After
one, a compared op must show NaN only where a fresh plan does (eval_flips' out-of-range candidate).

  1. fresh == fresh for every op (the README's determinism claim), outputs finite and not constant, and the
     op calls the hbx_* functions the catalogue declares for it;
  2. order independence pair by pair: every op A at the ragged size on one long-lived dirty plan per shape,
     then op B, B == fresh; one seeded sequence of 200 ops per shape; the 256x12 sequence again on a
     stream of the test's own (internal work left on the null stream would show there);
  3. two HologramVecEnvs per mode stepped with the same actions, foreign calls on env.plan between the
     steps of one of them.  mode="psf" has no recon_image observation (the env refuses the key), so its pair
     compares the state observation and the cached field and intensity instead;
  4. walks split into several calls with foreign calls between them == the walk in one call.  include/hbx.h
     promises the accept sequence, every logged PSNR, the mask, base_chan_stats, the walk state and the cached
     planes bit for bit.  It does NOT promise which spare slot of the pool a candidate's pair was written to,
     and a call's first batch starts at ring 0 with every slot propagated in full
     (csrc/hbx_walk_planes.hpp), so the raw pool and slot table may differ across a call boundary: the
     plane cache is compared through the slot table (plane c = pool[slot[c]]), not slot for slot;
  5. set_precision / set_depths / set_timing and back, refused calls, two plans alive together.

Findings: none in the workspaces -- every case passed on the library as it was, so there is no
fix.  The net was shown to catch two seeded mistakes (set_precision ignoring the switch back to f32; the
plane-cache walk not restarting its spare-slot rotation at a call's first batch).  The poison ops brought out
that a PSNR formed from NaN statistics is +inf, or with a NaN sum I^2 the unscaled one -- psnr_from's rule, now
stated in include/hbx.h; the poison assertions follow it.  Run with -s for each shape's peak device memory.
"""
import ctypes as C
import math
from collections import OrderedDict

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import _launch_size as L  # noqa: E402
from tests import _plan_ops as P  # noqa: E402

# name: (N, groups, planes, max_jobs, the bases run (None: all), plane cache)
SHAPES = OrderedDict([
    ("256x12", (256, 3, 4, 6, None, True)),
    ("64x2", (64, 1, 2, 3, None, False)),
    ("896x2", (896, 1, 2, 3, None, True)),
    ("1024x2", (1024, 1, 2, 4, ("propagate", "eval_flips", "evaluate_complex", "evaluate_phase", "phase_backward",
                                "evaluate_stack_phase", "dbs_walk_planes"), True)),
    ("walking", (256, 1, 2, 256, ("propagate", "simulate", "evaluate_real", "evaluate_complex", "eval_flips"), False)),
])
HOST_BYTES = 64 << 20          # walking shape: larger outputs of a fresh plan wait in host memory
CACHE_BYTES = 128 << 20        # fresh-plan outputs kept on the device, least recently used first out
SEQUENCE = 200
STATE_KEYS = ("mask", "record", "chan_stats", "prev_psnr", "init_psnr", "steps", "flip_count", "sustained")


def _cfg(name):
    import hbx
    n, g, p = SHAPES[name][:3]
    return hbx.OpticsConfig(n, n, g, p, hbx.plan.WL_RGB if g == 3 else hbx.plan.WL_MONO)


def _ops(name):
    _, _, _, max_jobs, only, planes = SHAPES[name]
    return P.catalogue(_cfg(name), max_jobs, only=only, planes=planes)


def _compared(name):
    return [o for o in _ops(name) if not o.poison]


def _dirtiers(name):
    """every op at the ragged size (the ops of one env only as they are), poison included"""
    ops = _ops(name)
    ragged = {o.base for o in ops if o.size == "ragged"}
    return [o for o in ops if o.size == "ragged" or o.base not in ragged]


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm GPU")
    import hbx
    hbx.load_library()
    yield
    _World.drop()


class _Recorder:
    """libhbx with the names of the functions called through it"""

    def __init__(self, lib):
        self._lib, self.called = lib, set()

    def __getattr__(self, name):
        self.called.add(name)
        return getattr(self._lib, name)


class _World:
    """One shape at a time: its inputs, its long-lived dirty plan and the outputs of fresh plans."""
    current = None

    def __init__(self, name):
        self.name, self.cfg, self.max_jobs = name, _cfg(name), SHAPES[name][3]
        self.heavy = name == "walking"
        self.inp = P.Inputs(self.cfg, self.max_jobs, seed=list(SHAPES).index(name) + 1)
        self.ops = OrderedDict((o.name, o) for o in _ops(name))
        self.fresh = OrderedDict()
        self.fresh_bytes = 0
        self.checked = set()
        self.ws_bytes = 0
        self._dirty = None

    @classmethod
    def get(cls, name):
        if cls.current is None or cls.current.name != name:
            cls.drop()
            cls.current = cls(name)
        return cls.current

    @classmethod
    def drop(cls):
        w, cls.current = cls.current, None
        if w is not None:
            w.close_dirty()
            w.fresh.clear()
            w.inp = None
            print(f"{w.name}: peak device memory of tensors {torch.cuda.max_memory_allocated() / 2 ** 20:.0f} MiB, "
                  f"workspace of a plan {w.ws_bytes / 2 ** 20:.0f} MiB")      # shown with -s
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()

    def plan(self, **kw):
        import hbx
        plan = hbx.Plan(self.cfg, max_jobs=self.max_jobs, **kw)
        self.ws_bytes = plan.workspace_bytes
        return plan

    def dirty(self):
        if self._dirty is None:
            if self.heavy:                   # every fresh-plan output first: computing one closes the dirty plan
                for o in self.ops.values():
                    if not o.poison:
                        self.pristine(o)
            self._dirty = self.plan()
        return self._dirty

    def close_dirty(self):
        if self._dirty is not None:
            torch.cuda.synchronize()
            self._dirty.close()
            self._dirty = None

    def _run_fresh(self, op, record=False):
        plan = self.plan()
        try:
            if record:
                plan.lib = rec = _Recorder(plan.lib)
            out = op.run(plan, self.inp)
            torch.cuda.synchronize()
            if record:
                plan.lib = rec._lib
                assert op.fns <= rec.called, f"{op.name} declares {sorted(op.fns - rec.called)} and does not call them"
        finally:
            plan.close()
        return out

    def pristine(self, op):
        """the op's outputs on a plan created for it: checked once against a second such plan (determinism),
        for finiteness and variety, and for the functions it declares"""
        if op.name in self.fresh:
            self.fresh.move_to_end(op.name)
            return self.fresh[op.name]
        if self.heavy:
            self.close_dirty()               # two plans of this shape and a ragged output do not fit the budget
        self.inp.base()
        out = self._run_fresh(op, record=op.name not in self.checked)
        P.check_pristine(op, self.inp, out)
        if self.heavy:
            for i, (k, t) in enumerate(out):
                if t.numel() * t.element_size() > HOST_BYTES:
                    out[i] = (k, t.cpu().pin_memory())
            del t
        if op.name not in self.checked:       # once per op and shape; a recomputed entry is not checked again
            again = self._run_fresh(op)
            _assert_same(again, out, f"{self.name}: {op.name} on a second fresh plan (the same call twice: determinism)")
            del again
            self.checked.add(op.name)
        size = sum(t.numel() * t.element_size() for _, t in out if t.is_cuda)
        while self.fresh and self.fresh_bytes + size > CACHE_BYTES:
            _, old = self.fresh.popitem(last=False)
            self.fresh_bytes -= sum(t.numel() * t.element_size() for _, t in old if t.is_cuda)
        self.fresh[op.name] = out
        self.fresh_bytes += size
        return out


def _assert_same(got, want, what):
    """P.assert_same; an array of `want` kept in host memory is compared piecewise"""
    if all(w.is_cuda for _, w in want):
        return P.assert_same(got, want, what)
    assert [k for k, _ in got] == [k for k, _ in want], what
    step = HOST_BYTES // 4
    for (k, g), (_, w) in zip(got, want):
        if w.is_cuda:
            P.assert_same([(k, g)], [(k, w)], what)
            continue
        assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: {k}"
        gf, wf = g.reshape(-1), w.reshape(-1)
        for i in range(0, gf.numel(), step):
            piece = wf[i:i + step].cuda(non_blocking=True)
            if not P.same_array(gf[i:i + step], piece):
                j = i + torch.nonzero((gf[i:i + step] != piece).reshape(-1))[0].item()
                idx = tuple(int(v) for v in np.unravel_index(j, tuple(g.shape)))
                raise AssertionError(f"{what}: {k} differs from the fresh plan's, first at {idx}: "
                                     f"{gf[j].item()!r} != {wf[j].item()!r}")


def _params(select):
    return [pytest.param(name, o.name, id=f"{name}-{o.name}") for name in SHAPES for o in select(name)]


# -- 1. fresh == fresh -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,opname", _params(_compared))
def test_fresh_plans_agree(name, opname):
    w = _World.get(name)
    w.pristine(w.ops[opname])


@pytest.mark.parametrize("name", list(SHAPES))
def test_poison_reaches_memory(name):
    """each poison op on a fresh plan: its own outputs are all NaN (asserted inside the op)"""
    w = _World.get(name)
    poison = [o for o in w.ops.values() if o.poison]
    assert len(poison) == 5
    for o in poison:
        plan = w.plan()
        try:
            o.run(plan, w.inp)
            torch.cuda.synchronize()
        finally:
            plan.close()


def test_walking_shape_runs_the_walking_forms():
    n, g, p, max_jobs = SHAPES["walking"][:4]
    inp = P.Inputs(_cfg("walking"), max_jobs, 0)
    for total in (inp.envs["ragged"], inp.cands["ragged"]):
        launches = L.launches(total, max_jobs)
        assert launches == [max_jobs, max_jobs, 1]
        assert [L.walking(n, p, j) for j in launches] == [True, True, False]
    assert not L.walking(n, p, inp.envs["one"])


# -- 2. order independence ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,opname", _params(_compared))
def test_order_independence(name, opname):
    """B after every A on the shape's dirty plan == B on a fresh plan"""
    w = _World.get(name)
    b = w.ops[opname]
    want = w.pristine(b)
    plan = w.dirty()
    for a in _dirtiers(name):
        a.run(plan, w.inp)                     # its outputs are dropped at once
        got = b.run(plan, w.inp)
        _assert_same(got, want, f"{name}: {b.name} after {a.name}")
        del got


def _sequence(name, seed, stream=None):
    w = _World.get(name)
    ops = list(w.ops.values())
    rng = np.random.default_rng(seed)
    draws = rng.integers(0, len(ops), SEQUENCE)
    plan = w.dirty()
    torch.cuda.synchronize()
    prev = "a fresh plan" if stream is None else "the dirty plan"
    for pos, i in enumerate(draws):
        o = ops[i]
        want = None if o.poison else w.pristine(o)      # before the call: one set of outputs at a time
        got = o.run(plan, w.inp, stream=stream)
        if not o.poison:
            _assert_same(got, want, f"{name}: seed {seed}, position {pos}: {o.name} after {prev}")
        del got, want
        prev = o.name


@pytest.mark.parametrize("name", list(SHAPES))
def test_random_sequence(name):
    _sequence(name, seed=20240 + list(SHAPES).index(name))


def test_random_sequence_on_a_stream_of_its_own():
    """every call, allocation and clone of the 256x12 sequence on one torch.cuda.Stream: work the library left
    on the null stream (a lazy table build, a memset, the walk scratch) would not be ordered with it"""
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        _sequence("256x12", seed=77, stream=s)
    s.synchronize()
    torch.cuda.synchronize()


# -- 3. envs interrupted by foreign calls ------------------------------------------------------------
ENV_B, ENV_STEPS = 4, 8
FOREIGN = ("poison_evaluate_complex[ragged]", "evaluate_phase[ragged]", "poison_eval_flips_psf[ragged]",
           "flip_map[one]", "poison_backward_stack[ragged]", "evaluate_threshold[one]", "poison_flip_map[ragged]",
           "psf_eval_commit[ragged]", "poison_evaluate_real[ragged]", "propagate[ragged]")


def _same_env(a, b, what, keys):
    for k in keys:
        _assert_same([(k, getattr(a.state, k))], [(k, getattr(b.state, k))], what)


@pytest.mark.parametrize("mode", ["fft", "planes", "psf"])
def test_envs_interrupted_by_foreign_calls(mode):
    """hbx_env_reset, hbx_env_step / hbx_env_step_psf, hbx_field_refresh (refresh_every = 3) and
    hbx_env_obs_sync through two HologramVecEnvs; between the steps of the second one, a poison op and a
    sample op on its plan"""
    import hbx
    from hbx import _lib
    from hbx.env import HologramVecEnv
    _World.drop()
    cfg = hbx.mono_config(256)
    gen = torch.Generator(device="cuda").manual_seed(61)
    pres = [torch.rand((cfg.channels, 256, 256), generator=gen, device="cuda") for _ in range(ENV_B)]
    tgts = [torch.rand((cfg.groups, 256, 256), generator=gen, device="cuda") for _ in range(ENV_B)]
    acts = torch.randint(0, cfg.channels * 256 * 256, (ENV_STEPS, ENV_B), generator=gen, device="cuda")
    keys = ("state",) if mode == "psf" else ("state", "recon_image")
    envs = [HologramVecEnv(cfg, ENV_B, lambda i: tgts[i], pre_model_source=lambda i: pres[i], mode=mode,
                           max_steps=ENV_STEPS - 2, auto_reset=False, obs_keys=keys, refresh_every=3)
            for _ in range(2)]
    state = STATE_KEYS + ("state_bytes",) + (("field", "intensity") if mode == "psf" else ("recon",))
    try:
        plan = envs[1].plan
        inp = P.Inputs(cfg, plan.max_jobs, seed=9)
        foreign = {o.name: o for o in P.catalogue(cfg, plan.max_jobs)}
        for env in envs:
            env.reset()
        _same_env(envs[0], envs[1], f"{mode}: reset", state)
        n_acc = n_rej = n_trunc = 0
        for k in range(ENV_STEPS):
            res = [[t.clone() for t in env.step_device(acts[k])] for env in envs]
            if k == 3:
                for env in envs:
                    env.plan.env_obs_sync(env.state.bufs, ENV_B, _lib.OBS_STATE)
            what = f"{mode}: step {k}"
            _assert_same(list(zip(("reward", "psnr", "accepted", "terminated", "truncated"), res[1])),
                         list(zip(("reward", "psnr", "accepted", "terminated", "truncated"), res[0])), what)
            _same_env(envs[1], envs[0], what, state)
            n_acc += int(res[0][2].sum())
            n_rej += int((res[0][2] == 0).sum())
            n_trunc += int(res[0][4].sum())
            for j in (2 * k, 2 * k + 1):
                foreign[FOREIGN[j % len(FOREIGN)]].run(plan, inp)
        for env in envs:
            env.state.check_error()
        assert n_acc > 0 and n_rej > 0 and n_trunc > 0
    finally:
        for env in envs:
            env.close()


# -- 4. walks split into calls with foreign calls between them ------------------------------------------
WALK_FIELDS = ("pos", "total", "accepted", "batches", "prev_psnr", "init_psnr", "last_psnr", "done", "stopped_early")
WALK_CALLS, WALK_PER_CALL = 3, 2


def _walk_state(wbuf):
    from hbx import _lib
    return _lib.DbsWalk.from_buffer_copy(wbuf.cpu().numpy().tobytes())


def _split_walk(name, make, promised, between):
    w = _World.get(name)
    w.inp.base()
    ops = w.ops
    out = []
    for calls in (1, WALK_CALLS):
        plan = w.plan()
        try:
            walk = make(plan, w.inp)
            for c in range(calls):
                walk.advance(WALK_CALLS * WALK_PER_CALL // calls)
                if calls > 1:
                    for o in between:
                        ops[o].run(plan, w.inp)
            torch.cuda.synchronize()
            out.append(([(k, t.clone()) for k, t in walk.outputs() if k in promised], _walk_state(walk.wbuf)))
        finally:
            plan.close()
    (one, st1), (split, st3) = out
    _assert_same(split, one, f"{name}: the walk in {WALK_CALLS} calls with {', '.join(between)} between them "
                             f"against the walk in one call")
    return st1, st3


PLANES_PROMISED = ("mask", "base_chan_stats", "planes by slot", "accept_pos", "accept_psnr", "fill_count")
BETWEEN = ("poison_evaluate_complex[ragged]", "propagate[ragged]")


@pytest.mark.parametrize("name,fill,slack", [("256x12", False, False), ("256x12", True, False),
                                              ("256x12", False, True), ("896x2", False, False)])
def test_plane_cache_walk_split_across_calls(name, fill, slack):
    k = min(SHAPES[name][3], 4)
    st1, st3 = _split_walk(name, lambda plan, inp: P.PlanesWalk(plan, inp, k, fill, slack), PLANES_PROMISED, BETWEEN)
    for f in WALK_FIELDS:
        a, b = getattr(st1, f), getattr(st3, f)
        assert a == b or (isinstance(a, float) and math.isnan(a) and math.isnan(b)), (f, a, b)
    assert st1.batches == WALK_CALLS * WALK_PER_CALL and st1.pos > 0 and st1.accepted > 0


@pytest.mark.parametrize("k", [2, 5])
def test_incremental_walk_split_across_calls(k):
    """K = 2: the one-launch batch, whose accepts reach the field in the next launch (the pending commit crosses
    the call boundary in the walk state); K = 5: the three-launch batch.  The whole walk state is compared."""
    between = BETWEEN + ("poison_eval_flips_psf[ragged]",)
    promised = ("mask", "base_chan_stats", "field", "intensity", "accept_pos", "accept_psnr", "walk")
    st1, _ = _split_walk("256x12", lambda plan, inp: P.PsfWalk(plan, inp, k), promised, between)
    assert st1.pos > 0 and st1.accepted > 0 and not st1.fault


# -- 5. switches, refused calls, two plans -------------------------------------------------------------
def _check(w, plan, names, what):
    for n in names:
        o = w.ops[n]
        want = w.pristine(o)
        _assert_same(o.run(plan, w.inp), want, f"{w.name}: {o.name} {what}")


BIT_PATH = ("propagate[ragged]", "simulate[ragged]", "eval_flips[ragged]", "step[ragged]",
            "planes_eval_commit[ragged]", "dbs_walk_planes[ragged]")


def test_precision_switch_and_back():
    import hbx
    w = _World.get("256x12")
    plan = w.plan()
    try:
        for kind in (hbx.PRECISION_BF16_STORE, hbx.PRECISION_F16_STORE):
            plan.precision = kind
            assert plan.precision == kind
            w.ops["propagate[ragged]"].run(plan, w.inp)
        plan.precision = hbx.PRECISION_F32
        _check(w, plan, [o.name for o in _compared("256x12")], "at f32 after bf16 and f16 propagations")
    finally:
        plan.close()


def test_bf16_after_f32_sample_ops_equals_a_bf16_plan():
    import hbx
    w = _World.get("256x12")
    used, made = w.plan(), w.plan(precision=hbx.PRECISION_BF16_STORE)
    try:
        for n in ("evaluate_real[ragged]", "evaluate_complex[ragged]", "backward_stack[ragged]",
                  "evaluate_real_window[ragged]", "poison_evaluate_complex[ragged]"):
            w.ops[n].run(used, w.inp)
        used.precision = hbx.PRECISION_BF16_STORE
        for n in BIT_PATH:
            o = w.ops[n]
            _assert_same(o.run(used, w.inp), o.run(made, w.inp),
                         f"{o.name}: a bf16 plan that ran f32 sample ops before against a plan created with bf16")
    finally:
        used.close()
        made.close()


def _stack_calls(plan, inp, zs):
    """evaluate_stack and, where the job slots take the depth count, backward_stack at the depths `zs`"""
    from hbx import _lib
    c, d, size = plan.cfg, len(zs), "ragged"
    plan.set_depths(zs)
    plan._ops_zs = tuple(zs)
    assert plan.depths == d
    t = inp.stack("stack_t", size, d, c.groups)
    out = list(zip(P.L3, plan.evaluate_stack(inp.phase(size), _lib.LEAF_PHASE, t)))
    if d <= P.max_stack_depths(c, plan.max_jobs):
        v = inp.stack("stack_v", size, d, c.channels // 2, cplx=True, lo=-1.0)
        out.append(("grad", plan.backward_stack(v, _lib.LEAF_PHASE, samples=inp.phase(size))))
    return [(k, P._c(x)) for k, x in out]


def test_depth_switches():
    """3 depths, 1 other depth, 2 depths on one plan: each stack call equals a fresh plan's given that same
    last set_depths; the single-depth calls equal a fresh plan's throughout (64x2: backward_stack fits D = 3)"""
    w = _World.get("64x2")
    z = w.cfg.z
    single = ("evaluate_phase[ragged]", "propagate[ragged]", "evaluate_real[one]")
    plan = w.plan()
    try:
        for zs in (P.depth_zs(w.cfg, 3), (1.7 * z,), (0.8 * z, 1.3 * z)):
            got = _stack_calls(plan, w.inp, zs)
            fresh = w.plan()
            try:
                want = _stack_calls(fresh, w.inp, zs)
                torch.cuda.synchronize()
            finally:
                fresh.close()
            _assert_same(got, want, f"stack calls at depths {zs} after other depths")
            _check(w, plan, single, f"with {len(zs)} depths set")
        plan.set_depths(())
        plan._ops_zs = ()
        assert plan.depths == 0
        _check(w, plan, single, "after the depth tables were freed")
    finally:
        plan.close()


def test_timing_on_sampled_and_off():
    from hbx import _lib
    w = _World.get("256x12")
    names = ("propagate[ragged]", "evaluate_real[ragged]", "psf_eval_commit[ragged]", "dbs_walk_planes[ragged]",
             "step[one]")
    plan = w.plan()
    try:
        size = plan.workspace_bytes
        _lib.check(plan.lib.hbx_plan_set_timing(plan._h, 64), "hbx_plan_set_timing")
        _check(w, plan, names, "with every launch timed")
        plan.set_timing(64, every=3)
        _check(w, plan, names, "with every third launch timed")
        timing = plan.read_timing()
        assert sum(n for _, n, _ in timing.values()) > 0
        _check(w, plan, names, "after read_timing")
        plan.set_timing(0)
        _check(w, plan, names, "with timing off again")
        assert plan.workspace_bytes == size
    finally:
        plan.close()


def _refused(lib, rc, code, word):
    from hbx import _lib
    msg = lib.hbx_last_error()
    assert rc == code and msg and word in msg, (rc, msg)
    assert code in (_lib.ERR_INVALID, _lib.ERR_UNSUPPORTED)


def test_refused_calls_leave_the_plan_as_it_was():
    """Each refused call returns its documented code with a message, writes to none of the buffers it was
    handed (they keep their fill value: nothing was enqueued), and the next valid call equals a fresh plan's."""
    import hbx
    from hbx import _lib
    from hbx.plan import _ptr, _stream
    w = _World.get("256x12")
    inp, c = w.inp, w.cfg
    n = inp.n("ragged")
    after = ("evaluate_phase[ragged]", "propagate[ragged]", "dbs_walk_planes[ragged]")
    plan = w.plan()
    lib = plan.lib
    fill = 12345.0
    try:
        # a sample op on a bf16 plan
        plan.precision = hbx.PRECISION_BF16_STORE
        with pytest.raises(hbx.HbxError) as e:
            plan.evaluate_real(inp.vals("ragged"), inp.tgt("ragged"))
        assert e.value.code == _lib.ERR_UNSUPPORTED and "HBX_PRECISION_F32" in str(e.value)
        plan.precision = hbx.PRECISION_F32
        _check(w, plan, after, "after a sample op was refused on the bf16 plan")
        # a stack op before depths are set
        assert plan.depths == 0
        out = torch.full((1, n, c.groups, c.height, c.width), fill, device="cuda")
        leaf = plan._leaf(_lib.LEAF_PHASE)
        rc = lib.hbx_evaluate_stack(plan._h, _ptr(inp.phase("ragged")), C.byref(leaf), None, n, None, _ptr(out),
                                    None, _stream(None))
        _refused(lib, rc, _lib.ERR_INVALID, b"depths")
        # a window outside the grid: the wrapper refuses it before any device work, and so does the library
        with pytest.raises(ValueError):
            plan.evaluate_real_window(inp.vals("ragged"), (5, 9, c.height, c.width))
        x = inp.win("win_x", "ragged", c.channels, P.IN_WIN(c.height))
        bad = _lib.Window(5, 9, c.height - 24, c.width)
        out_w = torch.full((n, c.groups, c.height, c.width), fill, device="cuda")
        rc = lib.hbx_evaluate_real_window(plan._h, _ptr(x), C.byref(bad), None, None, n, None, _ptr(out_w), None, None,
                                          _stream(None))
        _refused(lib, rc, _lib.ERR_INVALID, b"window")
        # a null required buffer
        st = torch.full((n, c.groups, 3), fill, dtype=torch.float64, device="cuda")
        rc = lib.hbx_propagate(plan._h, None, _ptr(inp.tgt("ragged")), n, _ptr(out_w), _ptr(st), None, _stream(None))
        _refused(lib, rc, _lib.ERR_INVALID, b"null buffer")
        # K above max_jobs
        walk = P.PlanesWalk(plan, inp, plan.max_jobs + 1)
        torch.cuda.synchronize()
        before = [(k, t.clone()) for k, t in walk.outputs()]
        with pytest.raises(hbx.HbxError) as e:
            walk.advance(2)
        assert e.value.code == _lib.ERR_INVALID and "K must be" in str(e.value)
        torch.cuda.synchronize()
        _assert_same(walk.outputs(), before, "the buffers of a walk refused for K > max_jobs")
        for t in (out, out_w, st):
            assert bool((t == fill).all()), "a refused call wrote to an output buffer"
        _check(w, plan, after, "after four refused calls")
    finally:
        plan.close()


def test_sticky_action_error_cleared_then_step_equals_twin():
    """An out-of-range action sets the env's sticky error word and changes nothing else; check_error() raises and
    clears it (the documented way); the next step equals that of an env which never saw the bad action."""
    import hbx
    from hbx.env import HologramVecEnv
    _World.drop()
    cfg = hbx.mono_config(256)
    gen = torch.Generator(device="cuda").manual_seed(62)
    pre = torch.rand((cfg.channels, 256, 256), generator=gen, device="cuda")
    tgt = torch.rand((cfg.groups, 256, 256), generator=gen, device="cuda")
    acts = torch.randint(0, cfg.channels * 256 * 256, (2, 2), generator=gen, device="cuda")
    keys = STATE_KEYS + ("state_bytes", "recon")
    envs = [HologramVecEnv(cfg, 2, lambda i: tgt, pre_model_source=lambda i: pre, auto_reset=False,
                           obs_keys=("state", "recon_image")) for _ in range(2)]
    try:
        for env in envs:
            env.reset()
        for env in envs:
            env.step_device(acts[0])
        all_bad = torch.full((2,), cfg.channels * 256 * 256, dtype=torch.int64, device="cuda")
        envs[1].step_device(all_bad)
        with pytest.raises(ValueError):
            envs[1].state.check_error()
        res = [[t.clone() for t in env.step_device(acts[1])] for env in envs]
        names = ("reward", "psnr", "accepted", "terminated", "truncated")
        _assert_same(list(zip(names, res[1])), list(zip(names, res[0])), "the step after the cleared error")
        _same_env(envs[1], envs[0], "the step after the cleared error", keys)
        for env in envs:
            env.state.check_error()
    finally:
        for env in envs:
            env.close()


def test_two_plans_alive_together():
    """a 256 plan and a 64 plan of another z, called alternately: each result equals its solo run"""
    import dataclasses
    import hbx
    _World.drop()
    cfgs = (dataclasses.replace(_cfg("256x12"), z=1.5e-3), dataclasses.replace(_cfg("64x2"), z=3e-3))
    jobs = (6, 3)
    names = ("propagate[ragged]", "evaluate_phase[ragged]", "eval_flips[ragged]", "psf_eval_commit[ragged]",
             "evaluate_stack_phase[one]", "flip_map[one]", "step[ragged]", "poison_evaluate_real[ragged]")
    inps = [P.Inputs(c, m, seed=70 + i) for i, (c, m) in enumerate(zip(cfgs, jobs))]
    cats = [{o.name: o for o in P.catalogue(c, m)} for c, m in zip(cfgs, jobs)]
    solo = []
    for c, m, inp, cat in zip(cfgs, jobs, inps, cats):
        plan = hbx.Plan(c, max_jobs=m)
        try:
            solo.append([cat[n].run(plan, inp) for n in names])
            torch.cuda.synchronize()
        finally:
            plan.close()
    plans = [hbx.Plan(c, max_jobs=m) for c, m in zip(cfgs, jobs)]
    try:
        for j, n in enumerate(names):
            for i in (0, 1):
                got = cats[i][n].run(plans[i], inps[i])
                if not cats[i][n].poison:
                    _assert_same(got, solo[i][j], f"{n} on plan {i} of two plans called alternately")
    finally:
        for plan in plans:
            plan.close()
