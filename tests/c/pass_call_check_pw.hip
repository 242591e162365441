// Host-side check of hbx::check_pass_call (csrc/hbx_internal.hpp) for the per-pixel loss weight
// (PassCall::pixel_weight; hbx_evaluate_pw, hbx_evaluate_stack_pw): one accepted PassCall per leaf kind and size
// as those two calls build them (csrc/hbx_api.hip), one rejected call per rule -- the weight only together with
// a target and the reduced statistics, only on the f32 sample paths, never with a window, plane cache, actions,
// walk, reconcile or env-major output, never on a gradient form or a piece that stops in front of the last
// pass -- and that a call without the weight is judged as before.  The sibling of pass_call_check_stack.hip;
// built by tests/test_pixel_weight_host.py with the host code under ASan + UBSan.  Needs no GPU and no
// library: nothing here dereferences a device pointer.
#include <stdio.h>
#include <string.h>

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

// stand-ins for device buffers: distinct non-null addresses, never read
static double store[4096];
template <class T>
static T* buf(int i) { return reinterpret_cast<T*>(&store[i]); }

static PlanDev plan(int R, int depths, int store_kind = HBX_PRECISION_F32) {
  PlanDev pd = {};
  pd.R = R;
  pd.N = R ? R * R : 896;
  pd.G = 3;
  pd.P = 8;
  pd.store_kind = store_kind;
  pd.htab = buf<float2>(100);
  pd.htab_stack = depths ? buf<float2>(200) : nullptr;
  pd.n_depths = depths;
  return pd;
}

// the forward call of each leaf kind with every output on; d < 0: hbx_evaluate_pw's, else depth d's piece of
// hbx_evaluate_stack_pw
static PassCall forward(int kind, int d, bool weighted = true) {
  PassCall c;
  c.jobs = buf<JobDesc>(0);
  c.n_jobs = 3;
  c.target = buf<float>(3);
  c.inten_out = buf<float>(4);
  if (weighted) c.pixel_weight = buf<float>(8);
  switch (kind) {
    case HBX_LEAF_THRESHOLD: c.real_binarize = 1; c.real_threshold = 0.5f;   // fallthrough
    case HBX_LEAF_REAL: c.real_values = buf<float>(1); c.field_out = buf<float2>(2); break;
    case HBX_LEAF_COMPLEX: c.complex_values = buf<float2>(1); break;
    case HBX_LEAF_PHASE_LEVELS: c.phase_levels = 16;   // fallthrough
    default: c.phase_values = buf<float>(1); break;
  }
  if (pass_complex(c)) {
    c.complex_field = buf<float2>(2);
    c.complex_stats = 1;
  }
  if (d >= 0) {
    c.stack_depth = d;
    c.stack_skip_first = d > 0;
  }
  return c;
}

int main() {
  const int sizes[4] = {32, 16, 8, 0};
  const int kinds[5] = {HBX_LEAF_REAL, HBX_LEAF_THRESHOLD, HBX_LEAF_COMPLEX, HBX_LEAF_PHASE, HBX_LEAF_PHASE_LEVELS};
  const hbx_window_t full = {0, 0, 64, 64}, part = {5, 9, 40, 33};
  WalkPlanesArgs wk = {};

  for (int R : sizes) {
    const PlanDev pd = plan(R, 3), pd0 = plan(R, 0);
    for (int kind : kinds) {
      // accepted: the single-depth call and every depth's piece, with and without the field and the intensity
      ACCEPT(pd0, forward(kind, -1));
      for (int d = 0; d < 3; ++d) ACCEPT(pd, forward(kind, d));
      {
        PassCall c = forward(kind, -1);
        c.inten_out = nullptr;
        c.field_out = nullptr;
        c.complex_field = nullptr;
        ACCEPT(pd0, c);
      }
      // ... and the same calls without the weight stay what they were
      ACCEPT(pd0, forward(kind, -1, false));
      for (int d = 0; d < 3; ++d) ACCEPT(pd, forward(kind, d, false));

      // only together with a target ...
      { PassCall c = forward(kind, -1); c.target = nullptr; REJECT(pd0, c); }
      // ... and the reduced statistics
      if (kind == HBX_LEAF_REAL || kind == HBX_LEAF_THRESHOLD) {
        PassCall c = forward(kind, -1);
        c.skip_reduce = 1;
        REJECT(pd0, c);
      } else {
        PassCall c = forward(kind, -1);   // the complex path without its statistics form
        c.complex_stats = 0;
        REJECT(pd0, c);
        c = forward(kind, -1);            // the real part is not a weighted form's output
        c.real_part = buf<float>(9);
        REJECT(pd0, c);
      }
      // only on the f32 sample paths
      REJECT(plan(R, 0, HBX_PRECISION_BF16_STORE), forward(kind, -1));
      REJECT(plan(R, 0, HBX_PRECISION_F16_STORE), forward(kind, -1));
      // never with a window (a full-grid one included), ...
      if (kind == HBX_LEAF_REAL || kind == HBX_LEAF_THRESHOLD) {
        PassCall c = forward(kind, -1);
        c.windowed = 1;
        c.in_win = c.out_win = part;
        REJECT(pd0, c);
        c.pixel_weight = nullptr;
        ACCEPT(pd0, c);   // (the window alone is a call the kernels run)
        c = forward(kind, -1);
        c.windowed = 1;
        c.in_win = c.out_win = full;
        REJECT(pd0, c);
      }
      // ... the plane cache, actions, a walk, the reconcile or env-major output
      { PassCall c = forward(kind, -1); c.plane_mode = kPlanesFill; c.plane_pool = buf<float>(10); c.plane_slot = buf<int32_t>(11); REJECT(pd0, c); }
      { PassCall c = forward(kind, -1); c.actions = buf<int64_t>(12); REJECT(pd0, c); }
      { PassCall c = forward(kind, -1); c.walk_phase = buf<uint8_t>(13); REJECT(pd0, c); }
      { PassCall c = forward(kind, -1); c.walk_planes = &wk; c.plane_mode = kPlanesStep; c.plane_pool = buf<float>(10); c.plane_slot = buf<int32_t>(11); REJECT(pd0, c); }
      { PassCall c = forward(kind, -1); c.rc_pending = buf<int32_t>(14); c.rc_cache = buf<float>(15); REJECT(pd0, c); }
      { PassCall c = forward(kind, -1); c.inten_by_env = 1; REJECT(pd0, c); }
    }
    // the bit path takes no weight (the same call without it is the plain propagation)
    {
      PassCall c;
      c.jobs = buf<JobDesc>(0);
      c.n_jobs = 3;
      c.mask = buf<uint64_t>(1);
      c.target = buf<float>(3);
      c.inten_out = buf<float>(4);
      ACCEPT(pd0, c);
      c.pixel_weight = buf<float>(8);
      REJECT(pd0, c);
    }
    // a gradient form has no statistics to weight
    {
      PassCall c;
      c.jobs = buf<JobDesc>(0);
      c.n_jobs = 3;
      c.complex_values = buf<float2>(1);
      c.grad_samples = buf<float>(6);
      c.grad_phase = buf<float>(7);
      ACCEPT(pd0, c);
      c.pixel_weight = buf<float>(8);
      REJECT(pd0, c);
      c.target = buf<float>(3);
      REJECT(pd0, c);
    }
    // a backward piece of a stack stops behind the column pass: no last pass, no weight
    {
      PassCall c;
      c.jobs = buf<JobDesc>(0);
      c.n_jobs = 3;
      c.complex_values = buf<float2>(1);
      c.stack_depth = 1;
      c.stack_skip_last = 1;
      c.stack_slot0 = 3;
      ACCEPT(pd, c);
      c.pixel_weight = buf<float>(8);
      REJECT(pd, c);
    }
    // a stack piece with a weight still needs a depth the plan has a table for
    REJECT(pd0, forward(HBX_LEAF_PHASE, 0));
    REJECT(pd, forward(HBX_LEAF_REAL, 3));
  }
  if (fails) {
    printf("%d check(s) failed\n", fails);
    return 1;
  }
  printf("OK\n");
  return 0;
}
