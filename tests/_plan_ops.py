"""The op catalogue of tests/test_gpu_plan_reuse.py: every kind of call a caller sends through one hbx.Plan.

An op is a name, the `hbx_*` functions it calls and `run(plan, inp, stream=None)`, which returns a list of
(label, tensor) -- every array the call wrote, each allocated by that call or cloned by the op.  `Inputs` holds a shape's seeded tensors: each is
built once, on first use, from a seed that depends on its name alone, and no op writes to one -- ops that
update caller state (commit_flip*, the walks, step) work on clones.  Every op exists in two batch sizes,
`one` (a single env or candidate) and `ragged` (two full launches and a short last one).

tests/test_plan_ops_host.py holds the catalogue to include/hbx.h without a GPU: an entry point that takes a
plan and enqueues work has to be named by an op here, by SWITCH_FNS or by ENV_FNS, or the test fails with
its name.  This module imports without a GPU; only `run` needs one.
"""
import math
from collections import OrderedDict

import numpy as np
import torch

from hbx import _lib

SIZES = ("one", "ragged")
STACK_D = 3
IN_WIN = lambda n: (5, 9, n - 24, n - 31)        # noqa: E731  multiples of nothing, in != out
OUT_WIN = lambda n: (3, 20, n - 30, n - 41)      # noqa: E731
WALK_ORDER = 96                                  # positions of the walks' visiting order
WALK_BATCHES = 2

# entry points the switch tests of tests/test_gpu_plan_reuse.py call (section "switches and refused calls")
SWITCH_FNS = frozenset({"hbx_plan_set_precision", "hbx_plan_set_depths", "hbx_plan_set_timing",
                        "hbx_plan_set_timing_sampled", "hbx_plan_read_timing", "hbx_plan_workspace_bytes"})
# entry points reached through hbx.env.HologramVecEnv in test_envs_interrupted_by_foreign_calls
ENV_FNS = frozenset({"hbx_env_reset", "hbx_env_step", "hbx_env_step_psf", "hbx_env_obs_sync", "hbx_field_refresh"})
# not in the matrix: they take no plan, or enqueue nothing
EXCLUDED = {
    "hbx_abi_version": "takes no plan",
    "hbx_last_error": "takes no plan; read by the refused-call tests",
    "hbx_host_alloc": "takes no plan",
    "hbx_host_free": "takes no plan",
    "hbx_plan_create": "creates the plan",
    "hbx_plan_destroy": "destroys the plan",
    "hbx_plan_pipeline": "a getter: enqueues nothing",
    "hbx_plan_depths": "a getter: enqueues nothing",
    "hbx_plan_precision": "a getter: enqueues nothing",
    "hbx_pack_mask": "takes no plan",
    "hbx_quantize_phase": "takes no plan",
    "hbx_rel_stats": "takes no plan; its workspace is the caller's",
}


def depth_zs(cfg, d):
    """the d depths of a shape's focal stack: around the plan's own z, none equal to it"""
    return tuple(cfg.z * (0.6 + 0.35 * i) for i in range(d))


def max_stack_depths(cfg, max_jobs):
    """the deepest stack hbx_backward_stack takes on this plan: max_jobs >= groups * depths"""
    return min(_lib.MAX_DEPTHS, max_jobs // cfg.groups)


class Inputs:
    """Seeded inputs of one shape (cfg, max_jobs); tensors are made on first use and never modified."""

    NAMES = ("vals", "tgt", "pw", "inten", "source", "win_x", "win_t", "win_v", "win_s", "win_w", "stack_t",
             "stack_pw", "stack_v", "stack_w", "stack_i", "actions", "grad_loss", "order", "slack", "flips")

    def __init__(self, cfg, max_jobs, seed):
        self.cfg, self.max_jobs, self.seed = cfg, int(max_jobs), int(seed)
        self.envs = {"one": 1, "ragged": 2 * (self.max_jobs // cfg.groups) + 1}
        # a flip candidate is one job: 2 * max_jobs + 1 of them make two full launches and a short one
        self.cands = {"one": 1, "ragged": 2 * self.max_jobs + 1}
        self._t = {}
        self._base = None

    # -- seeded tensors ------------------------------------------------------------------------------
    def _gen(self, name, size):
        s = (self.seed * 1009 + self.NAMES.index(name)) * 2 + SIZES.index(size)
        return torch.Generator(device="cuda").manual_seed(s)

    def _rand(self, name, size, shape, lo=0.0, hi=1.0):
        key = (name, size, tuple(shape))
        if key not in self._t:
            t = torch.rand(tuple(shape), generator=self._gen(name, size), device="cuda")
            self._t[key] = t if (lo, hi) == (0.0, 1.0) else t.mul_(hi - lo).add_(lo)
        return self._t[key]

    def n(self, size):
        return self.envs[size]

    def vals(self, size):
        """float32 [n, CH, N, N] in [-1, 1): the real leaf; its bytes are the other leaves' samples too"""
        c = self.cfg
        return self._rand("vals", size, (self.n(size), c.channels, c.height, c.width), -1.0, 1.0)

    def cvals(self, size):
        """complex64 [n, CH/2, N, N]: the same memory as vals, read as pairs"""
        c = self.cfg
        return torch.view_as_complex(self.vals(size).view(self.n(size), c.channels // 2, c.height, c.width, 2))

    def phase(self, size):
        """float32 [n, CH/2, N, N]: the first half of vals' memory"""
        c = self.cfg
        shape = (self.n(size), c.channels // 2, c.height, c.width)
        return self.vals(size).view(-1)[:math.prod(shape)].view(shape)

    def bits(self, size):
        key = ("bits", size)
        if key not in self._t:
            from hbx.plan import pack_bits
            self._t[key] = pack_bits(self.vals(size) >= 0)
        return self._t[key]

    def tgt(self, size):
        c = self.cfg
        return self._rand("tgt", size, (self.n(size), c.groups, c.height, c.width))

    def inten(self, size):
        c = self.cfg
        return self._rand("inten", size, (self.n(size), c.groups, c.height, c.width), 0.0, 2.0)

    def pw(self, size):
        """pixel weights [n, G, N, N] in [0, 1) with a don't-care band of zeros"""
        key = ("pw0", size)
        if key not in self._t:
            c = self.cfg
            w = self._rand("pw", size, (self.n(size), c.groups, c.height, c.width)).clone()
            w[..., : c.height // 5, :] = 0.0
            self._t[key] = w
        return self._t[key]

    def source(self):
        c = self.cfg
        return torch.view_as_complex(self._rand("source", "one", (c.groups, c.height, c.width, 2), -1.0, 1.0))

    def win(self, name, size, planes, win, cplx=False, lo=-1.0, hi=1.0):
        shape = (self.n(size), planes) + tuple(win[2:]) + ((2,) if cplx else ())
        t = self._rand(name, size, shape, lo, hi)
        return torch.view_as_complex(t) if cplx else t

    def stack(self, name, size, d, planes, cplx=False, lo=0.0, hi=1.0):
        c = self.cfg
        shape = (d, self.n(size), planes, c.height, c.width) + ((2,) if cplx else ())
        t = self._rand(name, size, shape, lo, hi)
        return torch.view_as_complex(t) if cplx else t

    def stats_of(self, inten, tgt, pw=None):
        """(sum v I T, sum v I^2, sum v T^2) over the last two axes, float64: statistics that belong to
        the intensities the loss-weight ops receive (computed once; an input like any other)"""
        key = ("stats", inten.data_ptr(), tgt.data_ptr(), None if pw is None else pw.data_ptr())
        if key not in self._t:
            i, t = inten.double(), tgt.double()
            v = 1.0 if pw is None else pw.double()
            self._t[key] = torch.stack([(v * i * t).sum((-1, -2)), (v * i * i).sum((-1, -2)),
                                        (v * t * t).sum((-1, -2))], dim=-1).contiguous()
        return self._t[key]

    def grad_loss(self, size):
        key = ("grad_loss", size)
        if key not in self._t:
            self._t[key] = self._rand("grad_loss", size, (self.n(size),), 0.5, 1.5).double()
        return self._t[key]

    def actions(self, size):
        key = ("actions", size)
        if key not in self._t:
            c = self.cfg
            self._t[key] = torch.randint(0, c.channels * c.height * c.width, (self.n(size),),
                                         generator=self._gen("actions", size), device="cuda")
        return self._t[key]

    def flips(self, size, invalid=False):
        """K candidate flips of env 0, spread over every channel, the two corner pixels among them;
        invalid: candidate K // 2 is one past the last pixel (ragged only)"""
        key = ("flips", size, invalid)
        if key not in self._t:
            c, k = self.cfg, self.cands[size]
            hw, ch = c.height * c.width, c.channels
            rng = np.random.default_rng(self.seed * 31 + k)
            f = ((np.arange(k) * 5) % ch) * hw + rng.integers(0, hw, k)
            if k > 2:
                f[0], f[-1] = 0, ch * hw - 1
            bad = np.zeros(k, bool)
            if invalid and k > 2:
                f[k // 2], bad[k // 2] = ch * hw, True
            self._t[key] = (torch.from_numpy(f.astype(np.int64)).cuda(), torch.from_numpy(bad).cuda())
        return self._t[key]

    def order(self):
        key = ("order",)
        if key not in self._t:
            c = self.cfg
            rng = np.random.default_rng(self.seed * 37 + 1)
            o = rng.choice(c.channels * c.height * c.width, WALK_ORDER, replace=False)
            self._t[key] = torch.from_numpy(o.astype(np.int64)).cuda()
        return self._t[key]

    def slack(self):
        """per-position acceptance slack in dB: zero, positive (downhill accepts) and negative (a minimum gain)"""
        key = ("slack",)
        if key not in self._t:
            rng = np.random.default_rng(self.seed * 41 + 2)
            s = rng.choice([0.0, 2e-4, -1e-5, 1e-3], WALK_ORDER)
            self._t[key] = torch.from_numpy(s.astype(np.float64)).cuda()
        return self._t[key]

    # -- what a caller would hold from earlier calls: computed once on a plan of its own ----------------
    def base(self):
        """env 0's statistics, PSNR, field and intensity, every env's statistics and PSNR, the fill counts"""
        if self._base is None:
            import hbx
            from hbx.dbs import fill_counts
            plan = hbx.Plan(self.cfg, max_jobs=self.max_jobs)
            try:
                b = {}
                for size in SIZES:
                    _, st, ps = plan.propagate(self.bits(size), self.tgt(size), want_intensity=False)
                    b[size] = (st, ps)
                f, i = plan.simulate(self.bits("one"), want_intensity=True)
                b["field0"] = torch.view_as_real(f[0]).contiguous()
                b["inten0"] = i[0].contiguous()
                b["stats0"] = b["one"][0][0].contiguous()
                b["psnr0"] = float(b["one"][1][0].item())
                c = self.cfg
                b["fill"] = torch.as_tensor(fill_counts(self.bits("one")[0], c.groups, c.planes)).cuda()
                torch.cuda.synchronize()
            finally:
                plan.close()
            self._base = b
        return self._base


# ---------------------------------------------------------------------------------------------------
class Op:
    def __init__(self, base, size, fns, fn, poison=False, planes=False, depths=0):
        self.base, self.size, self.fns, self._fn = base, size, frozenset(fns), fn
        self.poison, self.planes, self.depths = poison, planes, depths
        self.name = f"{base}[{size}]"

    def zs(self, cfg, max_jobs):
        """the depths this op needs on its plan (None: any).  "fit": STACK_D or as many as hbx_backward_stack
        takes on this plan's job slots; "max": the most it takes"""
        if not self.depths:
            return None
        most = max_stack_depths(cfg, max_jobs)
        d = {"fit": min(STACK_D, most), "max": most}.get(self.depths, self.depths)
        return depth_zs(cfg, d)

    def run(self, plan, inp, stream=None):
        zs = self.zs(plan.cfg, plan.max_jobs)
        if zs is not None and getattr(plan, "_ops_zs", None) != zs:
            plan.set_depths(zs)
            plan._ops_zs = zs
        out = self._fn(plan, inp, self.size, stream)
        return [(k, _c(t)) for k, t in out if t is not None]


def _c(t):
    """an output as the comparisons take it: complex as float pairs.  Every tensor an op returns is already the
    caller's own -- the wrappers allocate their outputs per call, and state an op updates is a clone it made"""
    return torch.view_as_real(t) if t.is_complex() else t


OPS = OrderedDict()      # base name -> dict(fns, fn, flags); every base exists in both SIZES unless `sizes` says less


def op(base, *fns, sizes=SIZES, **flags):
    def deco(fn):
        assert base not in OPS, base
        OPS[base] = dict(fns=frozenset(fns), fn=fn, sizes=tuple(sizes), flags=flags)
        return fn
    return deco


def catalogue(cfg, max_jobs, only=None, planes=True):
    """the Op objects of a shape: `only` restricts the (non-poison) bases, planes=False drops the plane cache"""
    out = []
    for base, d in OPS.items():
        fl = d["flags"]
        if fl.get("planes") and not planes:
            continue
        if only is not None and not fl.get("poison") and base not in only:
            continue
        for size in d["sizes"]:
            out.append(Op(base, size, d["fns"], d["fn"], poison=fl.get("poison", False),
                          planes=fl.get("planes", False), depths=fl.get("depths", 0)))
    return out


def named_functions():
    """every hbx_* function some catalogue op declares"""
    return frozenset().union(*(d["fns"] for d in OPS.values()))


L4 = ("field", "intensity", "chan_stats", "psnr")
L3 = ("field", "intensity", "chan_stats")


def _lab(labels, values):
    return list(zip(labels, values))


# -- the bit path -------------------------------------------------------------------------------------
@op("propagate", "hbx_propagate")
def _propagate(plan, inp, size, s):
    return _lab(("intensity", "chan_stats", "psnr"), plan.propagate(inp.bits(size), inp.tgt(size), stream=s))


@op("simulate", "hbx_simulate")
def _simulate(plan, inp, size, s):
    return _lab(("field", "intensity"), plan.simulate(inp.bits(size), want_intensity=True, stream=s))


@op("eval_flips", "hbx_eval_flips")
def _eval_flips(plan, inp, size, s):
    """psnr is NaN at the out-of-range candidate (ragged), whose group_stats row is not written"""
    b = inp.base()
    f, bad = inp.flips(size, invalid=True)
    ps, gs = plan.eval_flips(inp.bits("one")[0], inp.tgt("one")[0], b["stats0"], f, stream=s)
    return [("psnr", ps), ("group_stats", gs[~bad])]


def _commit_state(inp):
    b = inp.base()
    return (inp.bits("one")[0].clone(), b["stats0"].clone(),
            torch.full((1,), b["psnr0"], dtype=torch.float64, device="cuda"))


def _k_dev(inp, size):
    return torch.tensor([inp.cands[size] - 1], dtype=torch.int32, device="cuda")


@op("commit_flip", "hbx_eval_flips", "hbx_commit_flip")
def _commit_flip(plan, inp, size, s):
    b = inp.base()
    f, _ = inp.flips(size)
    ps, gs = plan.eval_flips(inp.bits("one")[0], inp.tgt("one")[0], b["stats0"], f, stream=s)
    mask, st, prev = _commit_state(inp)
    plan.commit_flip(mask, st, prev, f, ps, gs, _k_dev(inp, size), stream=s)
    return [("psnr", ps), ("group_stats", gs), ("mask", mask), ("chan_stats", st), ("prev_psnr", prev)]


@op("step", "hbx_step")
def _step(plan, inp, size, s):
    st, ps = inp.base()[size]
    mask, st, prev = inp.bits(size).clone(), st.clone(), ps.clone()
    psnr, acc = plan.step(mask, inp.actions(size), inp.tgt(size), st, prev, stream=s)
    return [("psnr", psnr), ("accepted", acc), ("mask", mask), ("chan_stats", st), ("prev_psnr", prev)]


@op("psnr", "hbx_psnr")
def _psnr(plan, inp, size, s):
    return [("psnr", plan.psnr(inp.base()[size][0], stream=s))]


@op("flip_map", "hbx_flip_map", sizes=("one",))
def _flip_map(plan, inp, size, s):
    return _lab(("dpsnr", "base_psnr"), plan.flip_map(inp.bits("one")[0], inp.tgt("one")[0], stream=s))


# -- the plane cache ----------------------------------------------------------------------------------
def _pool(plan, k):
    pool, slot = plan.plane_pool(k)
    pool.zero_()
    slot.zero_()
    return pool, slot


@op("planes_eval_commit", "hbx_planes_fill", "hbx_eval_flips_planes", "hbx_commit_flip_planes", planes=True)
def _planes_eval_commit(plan, inp, size, s):
    f, _ = inp.flips(size)
    bits, tgt = inp.bits("one")[0], inp.tgt("one")[0]
    pool, slot = _pool(plan, inp.cands[size])
    st, ps0 = plan.planes_fill(bits, tgt, pool, slot, stream=s)
    ps, gs = plan.eval_flips_planes(bits, tgt, st, pool, slot, f, stream=s)
    mask, st2, prev = bits.clone(), st.clone(), ps0.clone()
    plan.commit_flip_planes(mask, st2, prev, pool, slot, f, ps, gs, _k_dev(inp, size), stream=s)
    return [("base chan_stats", st), ("base psnr", ps0), ("psnr", ps), ("group_stats", gs), ("plane pool", pool),
            ("plane slots", slot), ("mask", mask), ("chan_stats", st2), ("prev_psnr", prev)]


def walk_buffer(total, psnr0, refresh_every=0):
    w = _lib.DbsWalk()
    w.total = total
    w.prev_psnr = w.init_psnr = psnr0
    w.last_psnr = math.nan
    w.refresh_every = refresh_every
    w.commit_ch = -1
    return torch.frombuffer(bytearray(bytes(w)), dtype=torch.uint8).cuda()


class PlanesWalk:
    """One plane-cached walk's caller-owned buffers; `advance` enqueues batches of K candidates."""

    def __init__(self, plan, inp, k, fill=False, slack=False, stream=None):
        b = inp.base()
        self.plan, self.k, self.s = plan, k, stream
        self.mask, self.tgt = inp.bits("one")[0].clone(), inp.tgt("one")[0]
        self.pool, self.slot = _pool(plan, k)
        st, _ = plan.planes_fill(self.mask, self.tgt, self.pool, self.slot, stream=stream)
        self.stats = st
        self.order = inp.order()
        self.wbuf = walk_buffer(WALK_ORDER, b["psnr0"])
        self.log_pos = torch.full((WALK_ORDER,), -1, dtype=torch.int64, device="cuda")
        self.log_psnr = torch.zeros(WALK_ORDER, dtype=torch.float64, device="cuda")
        c = plan.cfg
        self.counts = b["fill"].clone() if fill else None
        self.fill = (self.counts, (c.planes * c.height * c.width) // 2, 0) if fill else None
        self.slack = inp.slack() if slack else None

    def advance(self, batches):
        self.plan.dbs_walk_planes(self.mask, self.tgt, self.stats, self.pool, self.slot, self.order, self.wbuf,
                                  self.log_pos, self.log_psnr, self.k, batches, stream=self.s, fill=self.fill,
                                  slack=self.slack)

    def outputs(self):
        ch = self.plan.cfg.channels
        out = [("mask", self.mask), ("base_chan_stats", self.stats), ("plane pool", self.pool),
               ("plane slots", self.slot), ("planes by slot", self.pool[self.slot[:ch].long()]),
               ("accept_pos", self.log_pos), ("accept_psnr", self.log_psnr), ("walk", self.wbuf)]
        return out + ([("fill_count", self.counts)] if self.counts is not None else [])


def _walk_k(plan, inp, size):
    """one candidate per batch, or a batch over every job slot (8 at the most)"""
    return 1 if size == "one" else min(plan.max_jobs, 8)


def _walk_planes(fill, slack):
    def run(plan, inp, size, s):
        w = PlanesWalk(plan, inp, _walk_k(plan, inp, size), fill, slack, s)
        w.advance(WALK_BATCHES)
        return w.outputs()
    return run


op("dbs_walk_planes", "hbx_planes_fill", "hbx_dbs_walk_planes", planes=True)(_walk_planes(False, False))
op("dbs_walk_planes_fill", "hbx_planes_fill", "hbx_dbs_walk_planes_fill", planes=True)(_walk_planes(True, False))
op("dbs_walk_planes_anneal", "hbx_planes_fill", "hbx_dbs_walk_planes_anneal", planes=True)(_walk_planes(False, True))


# -- the incremental mode -----------------------------------------------------------------------------
@op("psf_eval_commit", "hbx_eval_flips_psf", "hbx_commit_flip_psf")
def _psf_eval_commit(plan, inp, size, s):
    b = inp.base()
    f, _ = inp.flips(size)
    field, inten = b["field0"].clone(), b["inten0"].clone()
    ps, gs = plan.eval_flips_psf(inp.bits("one")[0], inp.tgt("one")[0], b["stats0"], field, inten, f, stream=s)
    mask, st, prev = _commit_state(inp)
    plan.commit_flip_psf(mask, st, prev, field, inten, f, ps, gs, _k_dev(inp, size), stream=s)
    return [("psnr", ps), ("group_stats", gs), ("mask", mask), ("chan_stats", st), ("prev_psnr", prev),
            ("field", field), ("intensity", inten)]


class PsfWalk:
    """One incremental walk's caller-owned buffers."""

    def __init__(self, plan, inp, k, stream=None):
        b = inp.base()
        self.plan, self.k, self.s = plan, k, stream
        self.mask, self.tgt = inp.bits("one")[0].clone(), inp.tgt("one")[0]
        self.stats, self.field, self.inten = b["stats0"].clone(), b["field0"].clone(), b["inten0"].clone()
        self.order = inp.order()
        self.wbuf = walk_buffer(WALK_ORDER, b["psnr0"])
        self.log_pos = torch.full((WALK_ORDER,), -1, dtype=torch.int64, device="cuda")
        self.log_psnr = torch.zeros(WALK_ORDER, dtype=torch.float64, device="cuda")

    def advance(self, batches):
        self.plan.dbs_walk_psf(self.mask, self.tgt, self.stats, self.field, self.inten, self.order, self.wbuf,
                               self.log_pos, self.log_psnr, self.k, batches, stream=self.s)

    def outputs(self):
        return [("mask", self.mask), ("base_chan_stats", self.stats), ("field", self.field),
                ("intensity", self.inten), ("accept_pos", self.log_pos), ("accept_psnr", self.log_psnr),
                ("walk", self.wbuf)]


@op("dbs_walk_psf", "hbx_dbs_walk_psf")
def _dbs_walk_psf(plan, inp, size, s):
    """one: K = 2, the one-launch batch; ragged: K = 5, the three-launch batch"""
    w = PsfWalk(plan, inp, 2 if size == "one" else 5, s)
    w.advance(WALK_BATCHES)
    return w.outputs()


# -- the sample paths ---------------------------------------------------------------------------------
@op("simulate_real", "hbx_simulate_real")
def _simulate_real(plan, inp, size, s):
    return _lab(("field", "intensity"), plan.simulate_real(inp.vals(size), want_intensity=True, stream=s))


@op("propagate_real", "hbx_propagate_real")
def _propagate_real(plan, inp, size, s):
    return _lab(("intensity", "chan_stats", "psnr"), plan.propagate_real(inp.vals(size), inp.tgt(size), stream=s))


@op("intensity_real", "hbx_intensity_real")
def _intensity_real(plan, inp, size, s):
    return [("intensity", plan.intensity_real(inp.vals(size), stream=s))]


@op("evaluate_real", "hbx_evaluate_real")
def _evaluate_real(plan, inp, size, s):
    return _lab(L4, plan.evaluate_real(inp.vals(size), inp.tgt(size), stream=s))


@op("simulate_complex", "hbx_simulate_complex")
def _simulate_complex(plan, inp, size, s):
    return _lab(("field", "real part"), plan.simulate_complex(inp.cvals(size), want_real=True, stream=s))


@op("simulate_complex_weighted", "hbx_simulate_complex_weighted")
def _simulate_complex_weighted(plan, inp, size, s):
    return _lab(("field", "real part"), plan.simulate_complex(inp.cvals(size), want_real=True, weight=inp.tgt(size),
                                                              scale=2.0 / plan.cfg.planes, stream=s))


@op("evaluate_complex", "hbx_evaluate_complex")
def _evaluate_complex(plan, inp, size, s):
    return _lab(L4, plan.evaluate_complex(inp.cvals(size), inp.tgt(size), stream=s))


@op("simulate_phase", "hbx_simulate_phase")
def _simulate_phase(plan, inp, size, s):
    return _lab(("field", "real part"), plan.simulate_phase(inp.phase(size), want_real=True, stream=s))


@op("evaluate_phase", "hbx_evaluate_phase")
def _evaluate_phase(plan, inp, size, s):
    return _lab(L4, plan.evaluate_phase(inp.phase(size), inp.tgt(size), stream=s))


@op("phase_backward", "hbx_phase_backward")
def _phase_backward(plan, inp, size, s):
    return [("grad", plan.phase_backward(inp.cvals(size), inp.phase(size), weight=inp.tgt(size),
                                         scale=2.0 / plan.cfg.planes, stream=s))]


def _levels_ops(levels):
    @op(f"simulate_phase_levels_{levels}", "hbx_simulate_phase_levels")
    def _sim(plan, inp, size, s):
        return _lab(("field", "real part"), plan.simulate_phase_levels(inp.phase(size), levels, want_real=True, stream=s))

    @op(f"evaluate_phase_levels_{levels}", "hbx_evaluate_phase_levels")
    def _ev(plan, inp, size, s):
        return _lab(L4, plan.evaluate_phase_levels(inp.phase(size), levels, inp.tgt(size), stream=s))

    @op(f"phase_levels_backward_{levels}", "hbx_phase_levels_backward")
    def _bw(plan, inp, size, s):
        return [("grad", plan.phase_levels_backward(inp.cvals(size), inp.phase(size), levels, stream=s))]


_levels_ops(2)
_levels_ops(256)


@op("evaluate_threshold", "hbx_evaluate_threshold")
def _evaluate_threshold(plan, inp, size, s):
    return _lab(L4, plan.evaluate_threshold(inp.vals(size), 0.0, inp.tgt(size), stream=s))


@op("threshold_backward_window", "hbx_threshold_backward")
def _threshold_backward_window(plan, inp, size, s):
    return [("grad", plan.threshold_backward(inp.cvals(size), inp.phase(size), surrogate=_lib.STE_WINDOW, p0=-0.5,
                                             p1=0.5, stream=s))]


@op("threshold_backward_sigmoid", "hbx_threshold_backward")
def _threshold_backward_sigmoid(plan, inp, size, s):
    return [("grad", plan.threshold_backward(inp.cvals(size), inp.phase(size), weight=inp.tgt(size), scale=0.5,
                                             surrogate=_lib.STE_SIGMOID, p0=0.0, p1=4.0, stream=s))]


def _wins(plan):
    n = plan.cfg.height
    return IN_WIN(n), OUT_WIN(n)


@op("evaluate_real_window", "hbx_evaluate_real_window")
def _evaluate_real_window(plan, inp, size, s):
    wi, wo = _wins(plan)
    c = plan.cfg
    x, t = inp.win("win_x", size, c.channels, wi), inp.win("win_t", size, c.groups, wo, lo=0.0)
    return _lab(L4, plan.evaluate_real_window(x, wi, t, wo, stream=s))


@op("evaluate_threshold_window", "hbx_evaluate_threshold_window")
def _evaluate_threshold_window(plan, inp, size, s):
    wi, wo = _wins(plan)
    c = plan.cfg
    x, t = inp.win("win_x", size, c.channels, wi), inp.win("win_t", size, c.groups, wo, lo=0.0)
    return _lab(L4, plan.evaluate_threshold_window(x, 0.0, wi, t, wo, stream=s))


@op("backward_window", "hbx_backward_window")
def _backward_window(plan, inp, size, s):
    """values and weight over the forward's output window, the gradient over its input window"""
    wi, wo = _wins(plan)
    c = plan.cfg
    v = inp.win("win_v", size, c.channels // 2, wo, cplx=True)
    x = inp.win("win_s", size, c.channels // 2, wi)
    w = inp.win("win_w", size, c.groups, wo, lo=0.0)
    return [("grad", plan.backward_window(v, wo, wi, samples=x, weight=w, scale=0.5, p0=-0.5, p1=0.5, stream=s))]


@op("evaluate_pw", "hbx_evaluate_pw")
def _evaluate_pw(plan, inp, size, s):
    return _lab(L3, plan.evaluate_pw(inp.phase(size), _lib.LEAF_PHASE, inp.tgt(size), inp.pw(size), stream=s))


@op("pixel_weight_sum", "hbx_pixel_weight_sum")
def _pixel_weight_sum(plan, inp, size, s):
    return [("weight_sum", plan.pixel_weight_sum(inp.pw(size), stream=s))]


@op("pixel_weight_sum_stack", "hbx_pixel_weight_sum", depths=STACK_D)
def _pixel_weight_sum_stack(plan, inp, size, s):
    w = inp.stack("stack_pw", size, STACK_D, plan.cfg.groups)
    return [("weight_sum", plan.pixel_weight_sum(w, stack=True, stream=s))]


def _source_ops(tag, kind):
    x = (lambda inp, size: inp.phase(size))

    @op(f"source_field_{tag}", "hbx_source_field")
    def _field(plan, inp, size, s):
        return [("field", plan.source_field(x(inp, size), kind, inp.source(), threshold=0.0, stream=s))]

    @op(f"evaluate_source_{tag}", "hbx_evaluate_source")
    def _ev(plan, inp, size, s):
        return _lab(L3, plan.evaluate_source(x(inp, size), kind, inp.source(), inp.tgt(size), inp.pw(size),
                                             threshold=0.0, stream=s))

    @op(f"backward_source_{tag}", "hbx_backward_source")
    def _bw(plan, inp, size, s):
        return [("grad", plan.backward_source(inp.cvals(size), kind, inp.source(), samples=x(inp, size),
                                              weight=inp.tgt(size), scale=0.5, p0=-0.5, p1=0.5, stream=s))]


_source_ops("phase", _lib.LEAF_PHASE)
_source_ops("threshold", _lib.LEAF_THRESHOLD)


# -- focal stacks -------------------------------------------------------------------------------------
@op("evaluate_stack_phase", "hbx_evaluate_stack", depths=STACK_D)
def _evaluate_stack_phase(plan, inp, size, s):
    t = inp.stack("stack_t", size, STACK_D, plan.cfg.groups)
    return _lab(L3, plan.evaluate_stack(inp.phase(size), _lib.LEAF_PHASE, t, stream=s))


@op("evaluate_stack_real", "hbx_evaluate_stack", depths=STACK_D)
def _evaluate_stack_real(plan, inp, size, s):
    t = inp.stack("stack_t", size, STACK_D, plan.cfg.groups)
    return _lab(L3, plan.evaluate_stack(inp.vals(size), _lib.LEAF_REAL, t, stream=s))


@op("backward_stack", "hbx_backward_stack", depths="fit")
def _backward_stack(plan, inp, size, s):
    """D = 3 where the plan's job slots take it (max_jobs >= G D), else the most they take"""
    c = plan.cfg
    d = min(STACK_D, max_stack_depths(c, plan.max_jobs))
    v = inp.stack("stack_v", size, d, c.channels // 2, cplx=True, lo=-1.0)
    w = inp.stack("stack_w", size, d, c.groups)
    return [("grad", plan.backward_stack(v, _lib.LEAF_PHASE, samples=inp.phase(size), weight=w,
                                         scale=2.0 / c.planes, stream=s))]


@op("evaluate_stack_pw", "hbx_evaluate_stack_pw", depths=STACK_D)
def _evaluate_stack_pw(plan, inp, size, s):
    g = plan.cfg.groups
    t, w = inp.stack("stack_t", size, STACK_D, g), inp.stack("stack_pw", size, STACK_D, g)
    return _lab(L3, plan.evaluate_stack_pw(inp.vals(size), _lib.LEAF_THRESHOLD, t, w, threshold=0.0, stream=s))


# -- the loss kernels that take the plan --------------------------------------------------------------
@op("loss", "hbx_loss")
def _loss(plan, inp, size, s):
    st = inp.stats_of(inp.inten(size), inp.tgt(size))
    return [("mse", plan.loss(st, _lib.LOSS_MSE, stream=s)), ("psnr", plan.loss(st, _lib.LOSS_PSNR, stream=s))]


@op("loss_weight", "hbx_loss_weight")
def _loss_weight(plan, inp, size, s):
    i, t = inp.inten(size), inp.tgt(size)
    return [("weight", plan.loss_weight(i, t, inp.stats_of(i, t), inp.grad_loss(size), _lib.LOSS_PSNR, stream=s))]


@op("loss_window", "hbx_loss_window")
def _loss_window(plan, inp, size, s):
    wo, g = OUT_WIN(plan.cfg.height), plan.cfg.groups
    i, t = inp.win("win_w", size, g, wo, lo=0.0), inp.win("win_t", size, g, wo, lo=0.0)
    return [("mse", plan.loss_window(inp.stats_of(i, t), wo, stream=s))]


@op("loss_weight_window", "hbx_loss_weight_window")
def _loss_weight_window(plan, inp, size, s):
    wo, g = OUT_WIN(plan.cfg.height), plan.cfg.groups
    i, t = inp.win("win_w", size, g, wo, lo=0.0), inp.win("win_t", size, g, wo, lo=0.0)
    return [("weight", plan.loss_weight_window(i, t, inp.stats_of(i, t), wo, inp.grad_loss(size), stream=s))]


@op("loss_stack", "hbx_loss_stack", depths=STACK_D)
def _loss_stack(plan, inp, size, s):
    g = plan.cfg.groups
    i, t = inp.stack("stack_i", size, STACK_D, g, hi=2.0), inp.stack("stack_t", size, STACK_D, g)
    return [("mse", plan.loss_stack(inp.stats_of(i, t), stream=s))]


@op("loss_weight_stack", "hbx_loss_weight_stack", depths=STACK_D)
def _loss_weight_stack(plan, inp, size, s):
    g = plan.cfg.groups
    i, t = inp.stack("stack_i", size, STACK_D, g, hi=2.0), inp.stack("stack_t", size, STACK_D, g)
    return [("weight", plan.loss_weight_stack(i, t, inp.stats_of(i, t), inp.grad_loss(size), _lib.LOSS_PSNR,
                                              stream=s))]


@op("loss_pw", "hbx_pixel_weight_sum", "hbx_loss_pw")
def _loss_pw(plan, inp, size, s):
    i, t, w = inp.inten(size), inp.tgt(size), inp.pw(size)
    ws = plan.pixel_weight_sum(w, stream=s)
    return [("weight_sum", ws), ("mse", plan.loss_pw(inp.stats_of(i, t, w), ws, stream=s))]


@op("loss_weight_pw", "hbx_pixel_weight_sum", "hbx_loss_weight_pw")
def _loss_weight_pw(plan, inp, size, s):
    i, t, w = inp.inten(size), inp.tgt(size), inp.pw(size)
    ws = plan.pixel_weight_sum(w, stream=s)
    return [("weight", plan.loss_weight_pw(i, t, w, inp.stats_of(i, t, w), ws, inp.grad_loss(size), _lib.LOSS_PSNR,
                                           stream=s))]


@op("loss_pw_stack", "hbx_pixel_weight_sum", "hbx_loss_pw", "hbx_loss_weight_pw", depths=STACK_D)
def _loss_pw_stack(plan, inp, size, s):
    g = plan.cfg.groups
    i, t = inp.stack("stack_i", size, STACK_D, g, hi=2.0), inp.stack("stack_t", size, STACK_D, g)
    w = inp.stack("stack_pw", size, STACK_D, g)
    st = inp.stats_of(i, t, w)
    ws = plan.pixel_weight_sum(w, stack=True, stream=s)
    return [("mse", plan.loss_pw(st, ws, stack=True, stream=s)),
            ("weight", plan.loss_weight_pw(i, t, w, st, ws, stack=True, stream=s))]


# -- poison: not compared; they leave NaN in the plan's workspaces and assert that it got there --------
def _nan(t):
    return torch.full_like(torch.view_as_real(t) if t.is_complex() else t, math.nan)


PSNR_LABELS = ("psnr", "base_psnr")       # psnr_from gives +inf, not NaN, for statistics that are NaN (mse > 0 fails)


def _all_nan(base, out):
    """every array NaN throughout; a PSNR formed from NaN statistics is +inf by the library's rule"""
    for k, t in out:
        if t is not None:
            r = torch.view_as_real(t) if t.is_complex() else t
            ok = ~torch.isfinite(r) if k in PSNR_LABELS else torch.isnan(r)
            assert bool(ok.all()), f"poison op {base}: {k} is not all NaN: the poison did not reach it " \
                                   f"({int(ok.sum())} of {ok.numel()} elements)"
    return out


@op("poison_evaluate_complex", "hbx_evaluate_complex", sizes=("ragged",), poison=True)
def _poison_evaluate_complex(plan, inp, size, s):
    """the workspaces take the NaNs whether or not the field is written out: intensity, statistics, PSNR"""
    v = torch.view_as_complex(_nan(inp.cvals(size)))
    return _all_nan("evaluate_complex", _lab(L4, plan.evaluate_complex(v, _nan(inp.tgt(size)), want_field=False,
                                                                       stream=s)))


@op("poison_evaluate_real", "hbx_evaluate_real", sizes=("ragged",), poison=True)
def _poison_evaluate_real(plan, inp, size, s):
    return _all_nan("evaluate_real", _lab(L4, plan.evaluate_real(_nan(inp.vals(size)), _nan(inp.tgt(size)),
                                                                 want_field=False, stream=s)))


@op("poison_backward_stack", "hbx_backward_stack", sizes=("ragged",), poison=True, depths="max")
def _poison_backward_stack(plan, inp, size, s):
    """at the deepest stack the plan's job slots take, two full chunks of envs and a short one: every
    d * stride slot range of ws_b"""
    c = plan.cfg
    d = max_stack_depths(c, plan.max_jobs)
    n = 2 * (plan.max_jobs // (d * c.groups)) + 1
    v = torch.full((d, n, c.channels // 2, c.height, c.width), complex(math.nan, math.nan),
                   dtype=torch.complex64, device="cuda")
    return _all_nan("backward_stack", [("grad", plan.backward_stack(v, _lib.LEAF_REAL, stream=s))])


@op("poison_eval_flips_psf", "hbx_eval_flips_psf", sizes=("ragged",), poison=True)
def _poison_eval_flips_psf(plan, inp, size, s):
    """the increments (sum dI T, sum (2 I + dI) dI) of every candidate are NaN; sum T^2 is the base's, and the
    PSNR of a NaN sum I^2 is the unscaled one (psnr_from: sxx > 0 fails), so neither is asserted"""
    b = inp.base()
    f, _ = inp.flips(size)
    ps, gs = plan.eval_flips_psf(inp.bits("one")[0], inp.tgt("one")[0], b["stats0"], _nan(b["field0"]),
                                 _nan(b["inten0"]), f, stream=s)
    _all_nan("eval_flips_psf", [("group_stats[:, :2]", gs[:, :2])])
    return [("psnr", ps), ("group_stats", gs)]


@op("poison_flip_map", "hbx_flip_map", sizes=("ragged",), poison=True)
def _poison_flip_map(plan, inp, size, s):
    d, base = plan.flip_map(inp.bits("one")[0], _nan(inp.tgt("one")[0]), stream=s)
    return _all_nan("flip_map", [("dpsnr", d), ("base_psnr", base)])


# -- comparison ---------------------------------------------------------------------------------------
def first_difference(a, b):
    """count and first index at which two arrays of one shape differ (a NaN equals a NaN)"""
    ne = (a != b) & ~(torch.isnan(a) & torch.isnan(b)) if a.is_floating_point() else (a != b)
    i = torch.nonzero(ne.reshape(-1))[0].item()
    idx = np.unravel_index(i, tuple(a.shape))
    return f"{int(ne.sum())} of {a.numel()} differ, first at {tuple(int(v) for v in idx)}: " \
           f"{a.reshape(-1)[i].item()!r} != {b.reshape(-1)[i].item()!r}"


def same_array(got, want):
    """torch.equal with the documented NaNs in place: the same elements are NaN, every other one is equal"""
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if not got.is_floating_point():
        return torch.equal(got, want)
    ng, nw = torch.isnan(got), torch.isnan(want)
    if not bool(nw.any() | ng.any()):
        return torch.equal(got, want)
    zero = torch.zeros((), dtype=got.dtype, device=got.device)
    return torch.equal(ng, nw) and torch.equal(torch.where(ng, zero, got), torch.where(nw, zero, want))


def assert_same(got, want, what):
    """every output of an op equal to the pristine one; the message names the array and the first index"""
    assert [k for k, _ in got] == [k for k, _ in want], what
    for (k, g), (_, w) in zip(got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: {k}: {tuple(g.shape)} {g.dtype} != " \
                                                           f"{tuple(w.shape)} {w.dtype}"
        if not same_array(g, w):
            raise AssertionError(f"{what}: {k} differs from the fresh plan's, {first_difference(g, w)}")


def documented_nan(op_, inp, label):
    """the elements of an output that are NaN on a fresh plan (None: none): eval_flips' out-of-range candidate"""
    if op_.base == "eval_flips" and label == "psnr":
        return inp.flips(op_.size, invalid=True)[1]
    return None


def _all_finite(t, step=1 << 24):
    """torch.isfinite(t).all() in pieces: isfinite makes a float copy of what it is given"""
    flat = t.reshape(-1)
    return all(bool(torch.isfinite(flat[i:i + step]).all()) for i in range(0, flat.numel(), step))


def check_pristine(op_, inp, out):
    """once per op: the fresh plan's outputs are finite apart from the documented NaNs, and not all alike"""
    varied = False
    for k, t in out:
        if t.is_floating_point():
            want = documented_nan(op_, inp, k)
            if want is None:
                assert _all_finite(t), f"{op_.name}: {k} is not finite on a fresh plan"
            else:
                assert torch.equal(torch.isnan(t), want), f"{op_.name}: {k} has NaNs the op does not document"
                assert bool(torch.isfinite(t[~want]).all()), f"{op_.name}: {k} is not finite on a fresh plan"
        if t.numel() > 1 and bool((t != t.reshape(-1)[0]).any()):
            varied = True
    if all(t.numel() <= 1 for _, t in out):      # one value per output (a loss of one env): it is not zero
        varied = any(bool((t != 0).any()) for _, t in out)
    assert varied, f"{op_.name}: every output array is constant: the entry tests nothing"
