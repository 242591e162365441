"""The op catalogue of the plan-reuse tests (tests/_plan_ops.py) against include/hbx.h, without a GPU.

Every `hbx_*` function that takes a plan and enqueues work is named by a catalogue op, by the switch tests
(SWITCH_FNS) or by the env test (ENV_FNS) of tests/test_gpu_plan_reuse.py; the only exclusions are listed
with a reason and take no plan or enqueue nothing.  A function in neither set fails here by name, so a new
entry point cannot be added without joining the matrix.  (That an op calls what it declares is checked on
the GPU, where the ops run: test_fresh_plans_agree.)"""
import pytest

from tests import _plan_ops as P
from tests.test_abi import header_functions

# the functions that may be excluded: they take no plan, or enqueue nothing
MAY_EXCLUDE = {"hbx_abi_version", "hbx_last_error", "hbx_host_alloc", "hbx_host_free", "hbx_plan_create",
               "hbx_plan_destroy", "hbx_plan_pipeline", "hbx_plan_depths", "hbx_plan_precision", "hbx_pack_mask",
               "hbx_quantize_phase", "hbx_rel_stats"}
ENV_FNS = {"hbx_env_reset", "hbx_env_step", "hbx_env_step_psf", "hbx_env_obs_sync", "hbx_field_refresh"}


def _uncovered(named):
    covered = set(named) | set(P.SWITCH_FNS) | set(P.ENV_FNS) | set(P.EXCLUDED)
    return sorted(set(header_functions()) - covered)


def test_every_entry_point_is_in_the_matrix_or_excluded_with_a_reason():
    missing = _uncovered(P.named_functions())
    assert not missing, f"no catalogue op, switch test or env test names {missing}: add an op to tests/_plan_ops.py"


def test_exclusions_are_the_allowed_ones_with_reasons():
    assert set(P.EXCLUDED) <= MAY_EXCLUDE, sorted(set(P.EXCLUDED) - MAY_EXCLUDE)
    assert all(isinstance(r, str) and r.strip() and "\n" not in r for r in P.EXCLUDED.values())
    assert set(P.ENV_FNS) == ENV_FNS
    named = P.named_functions() | P.SWITCH_FNS | P.ENV_FNS
    assert not named & set(P.EXCLUDED), sorted(named & set(P.EXCLUDED))


def test_only_declared_functions_are_named():
    known = set(header_functions())
    for base, d in P.OPS.items():
        assert d["fns"] and d["fns"] <= known, (base, sorted(d["fns"] - known))
    assert P.SWITCH_FNS <= known and P.ENV_FNS <= known and set(P.EXCLUDED) <= known


def test_removing_an_op_fails_with_the_function_name():
    """hbx_flip_map is named by the flip_map ops alone: without them the coverage test names it"""
    named = frozenset().union(*(d["fns"] for b, d in P.OPS.items() if "flip_map" not in b))
    assert _uncovered(named) == ["hbx_flip_map"]


def test_every_family_in_both_sizes_and_the_poison_ops():
    import hbx
    cfg = hbx.OpticsConfig(256, 256, 3, 4, hbx.plan.WL_RGB)
    ops = P.catalogue(cfg, 6)
    names = {o.name for o in ops}
    assert len(names) == len(ops)
    for o in ops:
        if o.poison or o.base == "flip_map":          # flip_map takes one env; the poison ops run at ragged
            continue
        assert f"{o.base}[one]" in names and f"{o.base}[ragged]" in names, o.base
    assert sorted(o.base for o in ops if o.poison) == ["poison_backward_stack", "poison_eval_flips_psf",
                                                       "poison_evaluate_complex", "poison_evaluate_real",
                                                       "poison_flip_map"]
    assert not any(o.planes for o in P.catalogue(cfg, 6, planes=False))
    only = P.catalogue(cfg, 6, only=("propagate",))
    assert {o.base for o in only if not o.poison} == {"propagate"} and sum(o.poison for o in only) == 5


@pytest.mark.parametrize("groups,max_jobs,fit,most", [(3, 6, 2, 2), (1, 3, 3, 3), (1, 4, 3, 4), (1, 256, 3, 8)])
def test_stack_depths_fit_the_job_slots(groups, max_jobs, fit, most):
    """hbx_backward_stack needs max_jobs >= groups * depths: the ops ask for no more"""
    import hbx
    cfg = hbx.OpticsConfig(256, 256, groups, 2, hbx.plan.WL_RGB if groups == 3 else hbx.plan.WL_MONO)
    ops = {o.name: o for o in P.catalogue(cfg, max_jobs)}
    assert len(ops["backward_stack[ragged]"].zs(cfg, max_jobs)) == fit
    assert len(ops["poison_backward_stack[ragged]"].zs(cfg, max_jobs)) == most
    assert len(ops["evaluate_stack_phase[one]"].zs(cfg, max_jobs)) == P.STACK_D
    assert ops["propagate[one]"].zs(cfg, max_jobs) is None
    zs = P.depth_zs(cfg, most)
    assert len(set(zs)) == most and cfg.z not in zs


def test_comparison_is_exact_and_names_the_first_index():
    """assert_same on host tensors: equal arrays pass, one differing element fails with the array's name and
    its index, a NaN matches a NaN in the same place only, and a last-bit change is a difference"""
    import numpy as np
    torch = pytest.importorskip("torch")
    a = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4)
    P.assert_same([("x", a.clone())], [("x", a)], "same")
    b = a.clone()
    b[1, 2, 3] = float(np.nextafter(np.float32(23), np.float32(24)))
    with pytest.raises(AssertionError, match=r"case: x differs .* 1 of 24 differ, first at \(1, 2, 3\)"):
        P.assert_same([("x", b)], [("x", a)], "case")
    n = a.clone()
    n[0, 1, 1] = float("nan")
    P.assert_same([("x", n.clone())], [("x", n)], "NaN in the same place")
    with pytest.raises(AssertionError, match=r"first at \(0, 1, 1\)"):
        P.assert_same([("x", n)], [("x", a)], "a NaN where the fresh plan has none")
    m = a.clone()
    m[1, 0, 0] = float("nan")
    with pytest.raises(AssertionError):
        P.assert_same([("x", m)], [("x", n)], "NaNs in different places")
    with pytest.raises(AssertionError):
        P.assert_same([("x", a.double())], [("x", a)], "another dtype")
    with pytest.raises(AssertionError):
        P.assert_same([("y", a)], [("x", a)], "another label")
    i = torch.arange(6, dtype=torch.int64)
    with pytest.raises(AssertionError, match=r"first at \(5,\)"):
        P.assert_same([("i", i + (i == 5))], [("i", i)], "integers")
