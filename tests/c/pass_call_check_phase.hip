// Host-side check of hbx::check_pass_call (csrc/hbx_internal.hpp) for the phase-hologram calls: one
// accepted PassCall per shape hbx_simulate_phase / hbx_evaluate_phase / hbx_phase_backward build
// (csrc/hbx_api.hip), one rejected call per rule that names phase_values, grad_samples or grad_phase,
// and hbx::pass_reduces for them.  The sibling of pass_call_check.hip; built by
// tests/test_phase_field_host.py with the host code under ASan + UBSan.  Needs no GPU and no
// library: the validator only compares fields, no pointer is dereferenced.
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
static void expect_reduce(bool want, const PassCall& c, int line) {
  if (pass_reduces(c) != want) {
    printf("FAIL line %d: pass_reduces is %d, expected %d\n", line, !want, want);
    fails++;
  }
}

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

static PassCall simulate_phase() {   // hbx_simulate_phase, field only
  PassCall c;
  c.jobs = buf<JobDesc>(0);
  c.n_jobs = 3;
  c.phase_values = buf<float>(1);
  c.complex_field = buf<float2>(2);
  return c;
}
static PassCall evaluate_phase() {   // hbx_evaluate_phase with target, field and intensity
  PassCall c = simulate_phase();
  c.complex_stats = 1;
  c.target = buf<float>(3);
  c.inten_out = buf<float>(4);
  return c;
}
static PassCall phase_backward(bool weighted) {   // hbx_phase_backward
  PassCall c;
  c.jobs = buf<JobDesc>(0);
  c.n_jobs = 3;
  c.complex_values = buf<float2>(1);
  if (weighted) {
    c.complex_weight = buf<float>(5);
    c.complex_scale = 0.25f;
  }
  c.grad_samples = buf<float>(6);
  c.grad_phase = buf<float>(7);
  return c;
}

int main() {
  const int sizes[4] = {32, 16, 8, 0};
  for (int R : sizes) {
    const PlanDev pd = plan(R);
    // -- accepted: what the three entry points build ------------------------------------------------
    PassCall c = simulate_phase();
    ACCEPT(pd, c);
    expect_reduce(false, c, __LINE__);
    c.real_part = buf<float>(8);                 // field and real part
    ACCEPT(pd, c);
    c.complex_field = nullptr;                   // real part alone
    ACCEPT(pd, c);
    c = evaluate_phase();
    ACCEPT(pd, c);
    expect_reduce(true, c, __LINE__);
    c.complex_field = nullptr;                   // statistics and intensity, no field
    ACCEPT(pd, c);
    c.target = nullptr;                          // the intensity alone: nothing to reduce
    ACCEPT(pd, c);
    expect_reduce(false, c, __LINE__);
    ACCEPT(pd, phase_backward(false));
    ACCEPT(pd, phase_backward(true));
    expect_reduce(false, phase_backward(true), __LINE__);
    c = simulate_phase();                        // phase in, gradient out: the kernels take it
    c.complex_field = nullptr;
    c.grad_samples = buf<float>(6);
    c.grad_phase = buf<float>(7);
    ACCEPT(pd, c);

    // -- rejected: the phase input is the one input ------------------------------------------------
    c = simulate_phase();
    c.complex_values = buf<float2>(9);
    REJECT(pd, c);
    c = simulate_phase();
    c.real_values = buf<float>(9);
    REJECT(pd, c);
    c = simulate_phase();
    c.mask = buf<uint64_t>(9);
    REJECT(pd, c);
    // ... f32 only, no plane cache, actions or walk
    REJECT(plan(R, HBX_PRECISION_BF16_STORE), simulate_phase());
    REJECT(plan(R, HBX_PRECISION_F16_STORE), phase_backward(false));
    c = simulate_phase();
    c.plane_mode = kPlanesFill;
    c.plane_pool = buf<float>(9);
    c.plane_slot = buf<int32_t>(10);
    REJECT(pd, c);
    c = simulate_phase();
    c.actions = buf<int64_t>(9);
    REJECT(pd, c);
    c = simulate_phase();
    c.walk_phase = buf<uint8_t>(9);
    REJECT(pd, c);
    // ... it needs an output of the complex path, and writes none of the bit path's
    c = simulate_phase();
    c.complex_field = nullptr;
    REJECT(pd, c);
    c = simulate_phase();
    c.field_out = buf<float2>(9);
    REJECT(pd, c);
    c = evaluate_phase();
    c.inten_by_env = 1;
    REJECT(pd, c);
    c = evaluate_phase();
    c.skip_reduce = 1;
    REJECT(pd, c);
    // ... the weight rides on complex samples only
    c = simulate_phase();
    c.complex_weight = buf<float>(5);
    REJECT(pd, c);

    // -- rejected: the gradient pair is complete and alone -------------------------------------------
    c = phase_backward(false);
    c.grad_samples = nullptr;
    REJECT(pd, c);
    c = phase_backward(false);
    c.grad_phase = nullptr;
    REJECT(pd, c);
    c = phase_backward(true);
    c.complex_field = buf<float2>(2);
    REJECT(pd, c);
    c = phase_backward(true);
    c.real_part = buf<float>(8);
    REJECT(pd, c);
    c = phase_backward(false);
    c.complex_stats = 1;
    REJECT(pd, c);
    c = phase_backward(false);
    c.target = buf<float>(3);
    REJECT(pd, c);
    c = phase_backward(false);
    c.inten_out = buf<float>(4);
    REJECT(pd, c);
    // ... and belongs to the complex path: not behind bits or real samples
    c = PassCall();
    c.jobs = buf<JobDesc>(0);
    c.n_jobs = 3;
    c.mask = buf<uint64_t>(1);
    c.target = buf<float>(3);
    ACCEPT(pd, c);
    c.grad_samples = buf<float>(6);
    c.grad_phase = buf<float>(7);
    REJECT(pd, c);
    c.mask = nullptr;
    c.real_values = buf<float>(1);
    REJECT(pd, c);
  }
  if (fails) return 1;
  printf("OK\n");
  return 0;
}
