// Host-side check of hbx::check_pass_call (csrc/hbx_internal.hpp) for illumination fields (PassCall::source,
// source_adjoint, source_real / source_binarize; hbx_evaluate_source, hbx_backward_source): one accepted
// PassCall per shape the entry points build (csrc/hbx_api.hip) -- the forward of each of the five leaf kinds
// with and without a target and a pixel weight, the adjoint of each kind with and without a weight -- and one
// rejected call per rule: a source never with the bit path or the real-pair path, a window, any stack field,
// a plane cache, actions, a walk, the reconcile, env-major output or a reduced-precision plan; the real
// samples in a complex slot and their threshold switch only in the forward of a sourced call.  A call
// without the source is judged as before.  The sibling of pass_call_check_pw.hip; built by
// tests/test_source_host.py with the host code under ASan + UBSan.  Needs no GPU and no library: nothing
// here dereferences a device pointer.
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

static PlanDev plan(int R, int depths = 0, int store_kind = HBX_PRECISION_F32) {
  PlanDev pd = {};
  pd.R = R;
  pd.N = R ? R * R : 896;
  pd.G = 3;
  pd.P = 8;
  pd.va = 1.0f;
  pd.vb = -2.0f;
  pd.store_kind = store_kind;
  pd.htab = buf<float2>(100);
  pd.htab_stack = depths ? buf<float2>(200) : nullptr;
  pd.n_depths = depths;
  return pd;
}

// hbx_evaluate_source's call of each leaf kind
static PassCall forward(int kind, bool target = true, bool weighted = false, bool sourced = true) {
  PassCall c;
  c.jobs = buf<JobDesc>(0);
  c.n_jobs = 3;
  if (sourced) c.source = buf<float2>(20);
  switch (kind) {
    case HBX_LEAF_THRESHOLD: c.source_binarize = 1; c.source_threshold = 0.5f;   // fallthrough
    case HBX_LEAF_REAL: c.source_real = buf<float>(1); break;
    case HBX_LEAF_COMPLEX: c.complex_values = buf<float2>(1); break;
    case HBX_LEAF_PHASE_LEVELS: c.phase_levels = 16;   // fallthrough
    default: c.phase_values = buf<float>(1); break;
  }
  if (target) c.target = buf<float>(3);
  if (weighted) c.pixel_weight = buf<float>(8);
  c.inten_out = buf<float>(4);
  c.complex_field = buf<float2>(2);
  c.complex_stats = 1;
  return c;
}

// hbx_backward_source's call of each leaf kind
static PassCall adjoint(int kind, bool weighted = false, bool sourced = true) {
  PassCall c;
  c.jobs = buf<JobDesc>(0);
  c.n_jobs = 3;
  c.complex_values = buf<float2>(1);
  if (weighted) {
    c.complex_weight = buf<float>(5);
    c.complex_scale = 0.25f;
  }
  if (sourced) {
    c.source = buf<float2>(20);
    c.source_adjoint = 1;
  }
  switch (kind) {
    case HBX_LEAF_COMPLEX: c.complex_field = buf<float2>(2); break;
    case HBX_LEAF_REAL: c.real_part = buf<float>(2); break;
    case HBX_LEAF_PHASE_LEVELS: c.phase_levels = 16;   // fallthrough
    case HBX_LEAF_PHASE: c.grad_samples = buf<float>(6); c.grad_phase = buf<float>(7); break;
    default:
      c.grad_samples = buf<float>(6); c.grad_phase = buf<float>(7);
      c.grad_kind = kGradSteSigmoid; c.grad_p0 = 0.5f; c.grad_p1 = 4.0f;
      break;
  }
  return c;
}

// one rejected call per refusal rule, on a call that is accepted without the offending field.  What isolates
// the source's own terms: the window, the stack fields and the precision here, and the bit-path and real-pair
// calls in main(), which are accepted without the source.  The plane cache, actions, a walk, the reconcile and
// env-major output are refused on the complex path with or without a source (the sample-path and complex-out
// rules of check_pass_call come first), so no accepted call exists to isolate those terms against; they
// are listed because the issue lists them, and this checks the verdict, not which rule gave it.
template <class F>
static void refusals(const PlanDev& pd, const PlanDev& pd_stack, int R, F make) {
  const hbx_window_t full = {0, 0, pd.N, pd.N}, part = {5, 9, 40, 33};
  static WalkPlanesArgs wk = {};
  ACCEPT(pd, make());
  // a window, a full-grid one included
  { PassCall c = make(); c.windowed = 1; c.in_win = c.out_win = part; REJECT(pd, c); }
  { PassCall c = make(); c.windowed = 1; c.in_win = c.out_win = full; REJECT(pd, c); }
  // any stack field
  { PassCall c = make(); c.stack_depth = 0; REJECT(pd_stack, c); }
  { PassCall c = make(); c.stack_depth = 1; c.stack_skip_first = 1; REJECT(pd_stack, c); }
  { PassCall c = make(); c.stack_depth = 1; c.stack_skip_last = 1; c.stack_slot0 = 3; REJECT(pd_stack, c); }
  // a plane cache, actions, a walk, the reconcile, env-major output
  { PassCall c = make(); c.plane_mode = kPlanesFill; c.plane_pool = buf<float>(10); c.plane_slot = buf<int32_t>(11); REJECT(pd, c); }
  { PassCall c = make(); c.actions = buf<int64_t>(12); REJECT(pd, c); }
  { PassCall c = make(); c.walk_phase = buf<uint8_t>(13); REJECT(pd, c); }
  { PassCall c = make(); c.walk_planes = &wk; c.plane_mode = kPlanesStep; c.plane_pool = buf<float>(10); c.plane_slot = buf<int32_t>(11); REJECT(pd, c); }
  { PassCall c = make(); c.rc_pending = buf<int32_t>(14); c.rc_cache = buf<float>(15); REJECT(pd, c); }
  { PassCall c = make(); c.inten_by_env = 1; REJECT(pd, c); }
  // a reduced-precision plan
  REJECT(plan(R, 0, HBX_PRECISION_BF16_STORE), make());
  REJECT(plan(R, 0, HBX_PRECISION_F16_STORE), make());
  // the bit path or the real-pair path as a second input
  { PassCall c = make(); c.mask = buf<uint64_t>(16); REJECT(pd, c); }
  { PassCall c = make(); c.real_values = buf<float>(17); REJECT(pd, c); }
}

int main() {
  const int sizes[4] = {32, 16, 8, 0};
  const int kinds[5] = {HBX_LEAF_REAL, HBX_LEAF_THRESHOLD, HBX_LEAF_COMPLEX, HBX_LEAF_PHASE, HBX_LEAF_PHASE_LEVELS};

  for (int R : sizes) {
    const PlanDev pd = plan(R), pd_stack = plan(R, 3);
    for (int kind : kinds) {
      // accepted: the forward with and without a target, with a pixel weight, without the field
      ACCEPT(pd, forward(kind));
      ACCEPT(pd, forward(kind, false));
      ACCEPT(pd, forward(kind, true, true));
      { PassCall c = forward(kind); c.complex_field = nullptr; c.inten_out = nullptr; ACCEPT(pd, c); }
      { PassCall c = forward(kind, true, true); c.complex_field = nullptr; c.inten_out = nullptr; ACCEPT(pd, c); }
      // ... and the adjoint with and without a weight
      ACCEPT(pd, adjoint(kind));
      ACCEPT(pd, adjoint(kind, true));
      refusals(pd, pd_stack, R, [&] { return forward(kind); });
      refusals(pd, pd_stack, R, [&] { return forward(kind, true, true); });
      refusals(pd, pd_stack, R, [&] { return adjoint(kind, true); });

      // the forward: no weighted load, no gradient form
      { PassCall c = forward(kind); c.complex_weight = buf<float>(5); REJECT(pd, c); }
      { PassCall c = forward(kind); c.grad_samples = buf<float>(6); c.grad_phase = buf<float>(7); REJECT(pd, c); }
      // the adjoint: complex samples in, one output, no statistics, target, intensity or pixel weight
      { PassCall c = adjoint(kind); c.complex_stats = 1; REJECT(pd, c); }
      { PassCall c = adjoint(kind); c.target = buf<float>(3); REJECT(pd, c); }
      { PassCall c = adjoint(kind); c.inten_out = buf<float>(4); REJECT(pd, c); }
      { PassCall c = adjoint(kind); c.pixel_weight = buf<float>(8); c.target = buf<float>(3); REJECT(pd, c); }
      { PassCall c = adjoint(kind); c.complex_values = nullptr; c.phase_values = buf<float>(1); REJECT(pd, c); }
      { PassCall c = adjoint(kind); c.complex_field = nullptr; c.real_part = nullptr; c.grad_samples = nullptr; c.grad_phase = nullptr; REJECT(pd, c); }
      if (kind == HBX_LEAF_COMPLEX) { PassCall c = adjoint(kind); c.real_part = buf<float>(9); REJECT(pd, c); }

      // without the source: the complex kinds are the calls they were, the real samples in a complex slot
      // and the adjoint switch mean nothing
      if (kind == HBX_LEAF_REAL || kind == HBX_LEAF_THRESHOLD) {
        REJECT(pd, forward(kind, true, false, false));
      } else {
        ACCEPT(pd, forward(kind, true, false, false));
        ACCEPT(pd, forward(kind, true, true, false));
      }
      ACCEPT(pd, adjoint(kind, true, false));
      { PassCall c = adjoint(kind, false, false); c.source_adjoint = 1; REJECT(pd, c); }
    }
    // the real samples in a complex slot: only in the forward, the threshold switch only with them
    { PassCall c = adjoint(HBX_LEAF_REAL); c.complex_values = nullptr; c.source_real = buf<float>(1); REJECT(pd, c); }
    { PassCall c = forward(HBX_LEAF_COMPLEX); c.source_binarize = 1; REJECT(pd, c); }
    { PassCall c = forward(HBX_LEAF_PHASE); c.source_binarize = 1; REJECT(pd, c); }
    // exactly one input: the new one counts
    { PassCall c = forward(HBX_LEAF_REAL); c.complex_values = buf<float2>(18); REJECT(pd, c); }
    { PassCall c = forward(HBX_LEAF_REAL); c.phase_values = buf<float>(18); REJECT(pd, c); }
    { PassCall c = forward(HBX_LEAF_REAL); c.source_real = nullptr; REJECT(pd, c); }
    // the bit path and the real-pair path take no source (the same calls without it are what they were)
    {
      PassCall c;
      c.jobs = buf<JobDesc>(0);
      c.n_jobs = 3;
      c.mask = buf<uint64_t>(1);
      c.target = buf<float>(3);
      c.inten_out = buf<float>(4);
      ACCEPT(pd, c);
      c.source = buf<float2>(20);
      REJECT(pd, c);
    }
    {
      PassCall c;
      c.jobs = buf<JobDesc>(0);
      c.n_jobs = 3;
      c.real_values = buf<float>(1);
      c.target = buf<float>(3);
      c.inten_out = buf<float>(4);
      ACCEPT(pd, c);
      c.source = buf<float2>(20);
      REJECT(pd, c);
      c.source_adjoint = 1;
      REJECT(pd, c);
    }
    // the kinds and parameters the sourced first pass is launched with
    {
      const PassCall c = forward(HBX_LEAF_THRESHOLD);
      const SourceParams sp = pass_source_params(pd, c);
      if (pass_source_kind(c) != kSrcThreshold || sp.p0 != 0.5f || sp.p1 != 1.0f || sp.p2 != -1.0f ||
          pass_source_samples(c) != buf<float>(1)) {
        printf("FAIL: the thresholded kind's parameters\n");
        fails++;
      }
      const PassCall l = forward(HBX_LEAF_PHASE_LEVELS);
      const SourceParams lp = pass_source_params(pd, l);
      if (pass_source_kind(l) != kSrcPhaseLevels || lp.p0 != 8.0f || lp.p1 != 0.125f) {
        printf("FAIL: the L-level kind's parameters\n");
        fails++;
      }
      if (pass_source_kind(forward(HBX_LEAF_REAL)) != kSrcReal || pass_source_kind(forward(HBX_LEAF_COMPLEX)) != kSrcComplex ||
          pass_source_kind(forward(HBX_LEAF_PHASE)) != kSrcPhase) {
        printf("FAIL: the leaf kinds\n");
        fails++;
      }
    }
  }
  if (fails) {
    printf("%d check(s) failed\n", fails);
    return 1;
  }
  printf("OK\n");
  return 0;
}
