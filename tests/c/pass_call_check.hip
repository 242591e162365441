// Host-side check of hbx::check_pass_call (csrc/hbx_internal.hpp): which PassCalls run_jobs takes.
// One accepted call per shape the C-ABI layer (csrc/hbx_api.hip) builds, one rejected call per rule; for some
// of the accepted shapes also hbx::pass_reduces, the rule for when k_reduce_partials runs behind the last pass.
// Built by tests/test_abi.py::test_pass_call_rules_under_asan with the host code under ASan + UBSan;
// needs no GPU and no library: the validator only compares fields, no pointer is dereferenced.
#include <stdio.h>

#include "hbx_internal.hpp"

using namespace hbx;

static int fails = 0;
static void expect(bool accepted, const PlanDev& pd, const PassCall& c, int line) {
  const bool got = check_pass_call(pd, c) == hipSuccess;
  if (got != accepted) {
    printf("FAIL line %d: %s, expected %s\n", line, got ? "accepted" : "rejected", accepted ? "accepted" : "rejected");
    fails++;
  }
}
#define ACCEPT(pd, c) expect(true, pd, c, __LINE__)
#define REJECT(pd, c) expect(false, pd, c, __LINE__)
// pass_reduces: whether k_reduce_partials runs behind the last pass of this call
static void expect_reduce(bool want, const PassCall& c, int line) {
  if (pass_reduces(c) != want) {
    printf("FAIL line %d: pass_reduces is %d, expected %d\n", line, !want, want);
    fails++;
  }
}
#define REDUCES(c) expect_reduce(true, c, __LINE__)
#define NO_REDUCE(c) expect_reduce(false, c, __LINE__)

static PlanDev plan(int R, int store_kind = HBX_PRECISION_F32) {
  PlanDev pd = {};
  pd.R = R;
  pd.N = R ? R * R : 896;
  pd.G = 3;
  pd.P = 8;
  pd.store_kind = store_kind;
  return pd;
}

// stand-ins for device buffers: distinct non-null addresses, never read
static double store[16];
template <class T>
static T* buf(int i) { return reinterpret_cast<T*>(&store[i]); }

static PassCall bits() {   // the bare call of hbx_step / hbx_eval_flips
  PassCall c;
  c.jobs = buf<JobDesc>(0);
  c.n_jobs = 3;
  c.mask = buf<uint64_t>(1);
  c.target = buf<float>(2);
  return c;
}
static PassCall real() {   // hbx_propagate_real
  PassCall c = bits();
  c.mask = nullptr;
  c.real_values = buf<float>(1);
  c.inten_out = buf<float>(3);
  return c;
}
static PassCall cplx() {   // hbx_simulate_complex
  PassCall c;
  c.jobs = buf<JobDesc>(0);
  c.n_jobs = 3;
  c.complex_values = buf<float2>(1);
  c.complex_field = buf<float2>(4);
  return c;
}
static PassCall step_planes() {   // hbx_eval_flips_planes
  PassCall c = bits();
  c.plane_mode = kPlanesStep;
  c.plane_pool = buf<float>(5);
  c.plane_slot = buf<int32_t>(6);
  c.plane_spares = 4;
  c.spare_base = 2;
  return c;
}

int main() {
  const PlanDev p32 = plan(32), p16 = plan(16), p8 = plan(8), p896 = plan(0);
  const PlanDev p32h = plan(32, HBX_PRECISION_BF16_STORE);
  const PlanDev* every[] = {&p32, &p16, &p8, &p896};
  WalkPlanesArgs wa = {};

  // ---- accepted: every shape hbx_api.hip builds ----
  for (const PlanDev* pd : every) {
    PassCall c = bits();   // hbx_step, hbx_eval_flips
    ACCEPT(*pd, c);
    REDUCES(c);
    c.field_out = buf<float2>(4);   // ensure_hpsf, hbx_simulate, hbx_field_refresh
    c.inten_out = buf<float>(3);
    ACCEPT(*pd, c);
    c = real();   // hbx_propagate_real, hbx_intensity_real, hbx_evaluate_real / hbx_simulate_real
    ACCEPT(*pd, c);
    REDUCES(c);
    c.target = nullptr;
    ACCEPT(*pd, c);
    REDUCES(c);   // (the zero row's partials: reduced all the same, as before)
    c.field_out = buf<float2>(4);
    ACCEPT(*pd, c);
    c = cplx();   // hbx_simulate_complex: the field, the real part, both
    ACCEPT(*pd, c);
    NO_REDUCE(c);   // no statistics form: no partials
    c.real_part = buf<float>(7);
    ACCEPT(*pd, c);
    c.complex_field = nullptr;
    ACCEPT(*pd, c);
    c.complex_weight = buf<float>(8);   // hbx_simulate_complex_weighted
    c.complex_scale = 0.5f;
    ACCEPT(*pd, c);
    c = cplx();   // hbx_evaluate_complex: with a target, and the intensity alone
    c.complex_stats = 1;
    c.target = buf<float>(2);
    c.inten_out = buf<float>(3);
    ACCEPT(*pd, c);
    REDUCES(c);
    c.complex_field = nullptr;
    c.target = nullptr;
    ACCEPT(*pd, c);
    NO_REDUCE(c);   // statistics without a target: the intensity alone
    c = bits();   // hbx_env_step into the recon buffer, jobs from k_jobs_from_actions
    c.inten_by_env = 1;
    c.inten_out = buf<float>(3);
    ACCEPT(*pd, c);
  }
  ACCEPT(plan(8, HBX_PRECISION_F16_STORE), bits());   // the precision study at every R^2 size
  ACCEPT(p32h, step_planes());
  for (const PlanDev* pd : {&p32, &p16, &p896}) {
    PassCall c = bits();   // hbx_env_reset, hbx_planes_fill: full propagation into the plane cache
    c.plane_mode = kPlanesFill;
    c.plane_pool = buf<float>(5);
    c.plane_slot = buf<int32_t>(6);
    c.plane_spares = 1;
    ACCEPT(*pd, c);
    ACCEPT(*pd, step_planes());   // hbx_eval_flips_planes; hbx_env_step and the walk at N = 896
  }
  for (const PlanDev* pd : {&p32, &p16}) {
    PassCall c = step_planes();   // hbx_env_step, fused: actions decoded by the first pass, partials
    c.plane_spares = 0;           // left to the finalize, the previous step's reconcile in the last pass
    c.spare_base = 0;
    c.actions = buf<int64_t>(9);
    c.act_err = buf<int32_t>(10);
    c.skip_reduce = 1;
    c.inten_by_env = 1;
    c.inten_out = buf<float>(3);
    c.rc_pending = buf<int32_t>(11);
    c.rc_cache = buf<float>(12);
    ACCEPT(*pd, c);
    NO_REDUCE(c);   // skip_reduce: the finalize reads the partials
    c.plane_mode = kPlanesOff;   // ... without the plane cache
    c.plane_pool = nullptr;
    c.plane_slot = nullptr;
    ACCEPT(*pd, c);
    c = step_planes();   // hbx_dbs_walk_planes_fill, fused decision with retained candidates
    c.spare_base = 0;
    c.skip_reduce = 1;
    c.walk_planes = &wa;
    c.walk_phase = buf<uint8_t>(13);
    ACCEPT(*pd, c);
    c.walk_phase = nullptr;   // HBX_WALK_NO_RETAIN
    ACCEPT(*pd, c);
  }

  // ---- rejected: one call per rule ----
  {
    PassCall c = bits();   // exactly one input
    c.mask = nullptr;
    REJECT(p32, c);
    c = bits();
    c.real_values = buf<float>(1);
    REJECT(p32, c);
    c = cplx();
    c.mask = buf<uint64_t>(1);
    REJECT(p32, c);
    c = cplx();
    c.real_values = buf<float>(1);
    REJECT(p896, c);
  }
  {
    PassCall c = step_planes();   // the plane cache needs its pool and slots, and N = 1024 / 256 / 896
    REJECT(p8, c);
    c.plane_pool = nullptr;
    REJECT(p32, c);
    c = step_planes();
    c.plane_slot = nullptr;
    REJECT(p896, c);
  }
  {
    PassCall c = step_planes();   // the fused walk decision: a plane-cache step at N = 1024 / 256
    c.walk_planes = &wa;
    REJECT(p896, c);
    REJECT(p8, c);
    c.plane_mode = kPlanesFill;
    REJECT(p32, c);
    c = bits();
    c.walk_planes = &wa;
    REJECT(p16, c);
  }
  {
    PassCall c = bits();   // what the N = 896 kernels do not take
    c.walk_phase = buf<uint8_t>(13);
    REJECT(p896, c);
    c = bits();
    c.actions = buf<int64_t>(9);
    REJECT(p896, c);
    c = bits();
    c.skip_reduce = 1;
    REJECT(p896, c);
    c = bits();
    c.rc_pending = buf<int32_t>(11);
    c.rc_cache = buf<float>(12);
    REJECT(p896, c);
    REJECT(p8, c);   // ... nor k_rowinv at N = 64
    c.rc_cache = nullptr;   // a pending list without its cache
    REJECT(p32, c);
    c = bits();
    c.act_err = buf<int32_t>(10);   // an error word without actions
    REJECT(p32, c);
  }
  {
    PassCall c = real();   // real samples: f32 intermediates, no plane cache, no actions, no walk
    REJECT(p32h, c);
    c.plane_mode = kPlanesFill;
    c.plane_pool = buf<float>(5);
    c.plane_slot = buf<int32_t>(6);
    REJECT(p32, c);
    REJECT(p896, c);
    c = real();
    c.actions = buf<int64_t>(9);
    REJECT(p16, c);
    c = real();
    c.walk_phase = buf<uint8_t>(13);
    REJECT(p16, c);
  }
  {
    PassCall c = cplx();   // complex samples: the same, and something to write
    REJECT(p32h, c);
    c.plane_mode = kPlanesStep;
    c.plane_pool = buf<float>(5);
    c.plane_slot = buf<int32_t>(6);
    REJECT(p32, c);
    c = cplx();
    c.actions = buf<int64_t>(9);
    REJECT(p32, c);
    c = cplx();
    c.walk_phase = buf<uint8_t>(13);
    REJECT(p8, c);
    c = cplx();
    c.complex_field = nullptr;
    REJECT(p32, c);
    REJECT(p896, c);
    c = cplx();   // ... and nothing the pair-recombining last pass would ignore
    c.field_out = buf<float2>(4);
    REJECT(p32, c);
    c = cplx();
    c.inten_by_env = 1;
    REJECT(p32, c);
    c = cplx();
    c.skip_reduce = 1;
    REJECT(p16, c);
  }
  {
    PassCall c = bits();   // the complex-only fields with another input
    c.complex_weight = buf<float>(8);
    REJECT(p32, c);
    c = real();
    c.complex_weight = buf<float>(8);
    REJECT(p896, c);
    c = bits();
    c.complex_field = buf<float2>(4);
    REJECT(p32, c);
    c = real();
    c.real_part = buf<float>(7);
    REJECT(p32, c);
    c = bits();
    c.complex_stats = 1;
    REJECT(p896, c);
  }

  if (fails) printf("FAILED %d\n", fails);
  else printf("OK\n");
  return fails != 0;
}
