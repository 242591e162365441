// Host-side check of hbx::check_pass_call and hbx::check_stack_last (csrc/hbx_internal.hpp) for the focal-stack
// calls: one accepted PassCall per piece hbx_evaluate_stack / hbx_backward_stack build (csrc/hbx_api.hip), one
// rejected call per rule on the stack fields (sample inputs only; no window, plane cache, actions, walk or
// reconcile; a depth the plan has a table for), the table pass_htab hands the column pass, and that a call
// without stack fields is judged as before.  The sibling of pass_call_check_levels.hip; built by
// tests/test_focal_stack_host.py with the host code under ASan + UBSan.  Needs no GPU and no library: nothing
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
#define CHECK(cond)                                        \
  do {                                                     \
    if (!(cond)) {                                         \
      printf("FAIL line %d: %s\n", __LINE__, #cond);       \
      fails++;                                             \
    }                                                      \
  } while (0)

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

// hbx_evaluate_stack's piece for depth d of each leaf kind, every output on
static PassCall forward_piece(int kind, int d) {
  PassCall c;
  c.jobs = buf<JobDesc>(0);
  c.n_jobs = 3;
  c.target = buf<float>(3);
  c.inten_out = buf<float>(4);
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
  c.stack_depth = d;
  c.stack_skip_first = d > 0;
  return c;
}

// hbx_backward_stack's piece for depth d: first and column pass into slot d * nj
static PassCall backward_piece(int d, int nj, bool weighted) {
  PassCall c;
  c.jobs = buf<JobDesc>(0);
  c.n_jobs = 3;
  c.complex_values = buf<float2>(1);
  if (weighted) {
    c.complex_weight = buf<float>(5);
    c.complex_scale = 0.25f;
  }
  c.stack_depth = d;
  c.stack_skip_last = 1;
  c.stack_slot0 = d * nj;
  return c;
}

// the depth-summing last pass's output description, per leaf kind
static PassCall last_piece(int kind) {
  PassCall c;
  c.jobs = buf<JobDesc>(0);
  c.n_jobs = 3;
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

int main() {
  const int sizes[4] = {32, 16, 8, 0};
  const int kinds[5] = {HBX_LEAF_REAL, HBX_LEAF_THRESHOLD, HBX_LEAF_COMPLEX, HBX_LEAF_PHASE, HBX_LEAF_PHASE_LEVELS};
  static_assert(HBX_MAX_DEPTHS == 8, "the issue's bound");
  for (int R : sizes) {
    const PlanDev pd = plan(R, 3);
    const PlanDev none = plan(R, 0);
    // -- accepted: every piece the two entry points build ---------------------------------------------
    for (int kind : kinds)
      for (int d = 0; d < 3; ++d) {
        PassCall c = forward_piece(kind, d);
        ACCEPT(pd, c);
        // the table the column pass reads: depth d's block of htab_stack, never the plan's own
        CHECK(pass_htab(pd, c) == pd.htab_stack + (size_t)d * pd.G * (size_t)(pd.N / 2 + 1) * pd.N);
        // subsets of the outputs, as the single-depth calls allow them
        c.target = nullptr;
        ACCEPT(pd, c);
        if (!pass_complex(c)) {
          c.inten_out = nullptr;
          ACCEPT(pd, c);
        }
      }
    for (int d = 0; d < 3; ++d) {
      ACCEPT(pd, backward_piece(d, 3, false));
      ACCEPT(pd, backward_piece(d, 3, true));
    }
    {   // a call without stack fields reads the plan's own table and is judged as before
      PassCall c = forward_piece(HBX_LEAF_COMPLEX, 0);
      c.stack_depth = -1;
      CHECK(!pass_stack(c));
      CHECK(pass_htab(pd, c) == pd.htab);
      ACCEPT(pd, c);
      ACCEPT(none, c);
    }
    // -- rejected: one call per rule -----------------------------------------------------------------
    for (int kind : kinds) {
      PassCall c = forward_piece(kind, 1);
      REJECT(none, c);                         // no depths set on the plan
      c.stack_depth = 3;
      REJECT(pd, c);                           // a depth the plan has no table for
      c = forward_piece(kind, 1);
      c.stack_depth = -1;
      REJECT(pd, c);                           // a piece that names no depth
      c = forward_piece(kind, 0);
      c.windowed = 1;
      c.in_win = c.out_win = hbx_window_t{0, 0, pd.N, pd.N};
      REJECT(pd, c);                           // no window
      c = forward_piece(kind, 0);
      c.inten_by_env = 1;
      REJECT(pd, c);                           // nothing env-major
      c = forward_piece(kind, 0);
      c.skip_reduce = 1;
      REJECT(pd, c);
      c = forward_piece(kind, 0);
      c.stack_slot0 = 3;
      REJECT(pd, c);                           // the slot offset is the backward's
      c = forward_piece(kind, 1);
      c.stack_skip_last = 1;
      REJECT(pd, c);                           // a call runs at least one of first and last pass
      REJECT(plan(R == 0 ? 32 : R, 3, HBX_PRECISION_BF16_STORE), forward_piece(kind, 0));   // f32 plans only
    }
    {   // the bit path and everything that rides on it
      PassCall c;
      c.jobs = buf<JobDesc>(0);
      c.n_jobs = 3;
      c.mask = buf<uint64_t>(1);
      c.target = buf<float>(3);
      ACCEPT(pd, c);
      c.stack_depth = 0;
      REJECT(pd, c);                           // sample inputs only
      if (R == 32 || R == 16 || R == 0) {
        PassCall p = c;
        p.stack_depth = -1;
        p.plane_mode = kPlanesFill;
        p.plane_pool = buf<float>(8);
        p.plane_slot = buf<int32_t>(9);
        ACCEPT(pd, p);
        p.stack_depth = 0;
        REJECT(pd, p);                         // no plane cache
      }
      if (R == 32 || R == 16) {
        PassCall a = c;
        a.stack_depth = -1;
        a.actions = buf<int64_t>(10);
        ACCEPT(pd, a);
        a.stack_depth = 0;
        REJECT(pd, a);                         // no actions
        PassCall w = c;
        w.stack_depth = -1;
        w.walk_phase = buf<uint8_t>(11);
        ACCEPT(pd, w);
        w.stack_depth = 0;
        REJECT(pd, w);                         // no walk
        PassCall r = c;
        r.stack_depth = -1;
        r.inten_out = buf<float>(4);
        r.rc_pending = buf<int32_t>(12);
        r.rc_cache = buf<float>(13);
        ACCEPT(pd, r);
        r.stack_depth = 0;
        REJECT(pd, r);                         // no reconcile
      }
    }
    {   // a backward piece: complex samples in, no output of its own
      PassCall c = backward_piece(1, 3, true);
      c.complex_field = buf<float2>(2);
      REJECT(pd, c);
      c = backward_piece(1, 3, true);
      c.grad_samples = buf<float>(6);
      c.grad_phase = buf<float>(7);
      REJECT(pd, c);
      c = backward_piece(1, 3, false);
      c.complex_values = nullptr;
      c.phase_values = buf<float>(1);
      REJECT(pd, c);
      c = backward_piece(1, 3, false);
      c.stack_slot0 = -3;
      REJECT(pd, c);
      c = backward_piece(1, 3, false);
      c.stack_skip_last = 0;                   // without the flag it needs an output, and may not sit at a slot
      REJECT(pd, c);
    }
    // -- the depth-summing last pass -------------------------------------------------------------------
    for (int kind : kinds) {
      const PassCall c = last_piece(kind);
      for (int D = 1; D <= HBX_MAX_DEPTHS; ++D) CHECK(check_stack_last(pd, c, D, 3) == hipSuccess);
      CHECK(check_stack_last(pd, c, 0, 3) != hipSuccess);
      CHECK(check_stack_last(pd, c, HBX_MAX_DEPTHS + 1, 3) != hipSuccess);
      CHECK(check_stack_last(pd, c, 2, 2) != hipSuccess);          // the slot ranges would overlap
      CHECK(check_stack_last(plan(R == 0 ? 32 : R, 3, HBX_PRECISION_F16_STORE), c, 2, 3) != hipSuccess);
      PassCall two = c;
      two.complex_field = buf<float2>(2);
      two.real_part = buf<float>(3);
      CHECK(check_stack_last(pd, two, 2, 3) != hipSuccess);        // one output
      PassCall in = c;
      in.complex_values = buf<float2>(1);
      CHECK(check_stack_last(pd, in, 2, 3) != hipSuccess);         // it loads from ws_b, not from samples
      PassCall win = c;
      win.windowed = 1;
      CHECK(check_stack_last(pd, win, 2, 3) != hipSuccess);
      PassCall st = c;
      st.complex_stats = 1;
      CHECK(check_stack_last(pd, st, 2, 3) != hipSuccess);
    }
    {
      PassCall c = last_piece(HBX_LEAF_THRESHOLD);
      c.grad_p1 = 0.0f;                                            // the sigmoid's slope is positive
      CHECK(check_stack_last(pd, c, 2, 3) != hipSuccess);
      c = last_piece(HBX_LEAF_PHASE);
      c.grad_phase = nullptr;                                      // the pair comes together
      CHECK(check_stack_last(pd, c, 2, 3) != hipSuccess);
      c = last_piece(HBX_LEAF_PHASE_LEVELS);
      c.phase_levels = 1;
      CHECK(check_stack_last(pd, c, 2, 3) != hipSuccess);
      c = last_piece(HBX_LEAF_REAL);
      c.phase_levels = 16;                                         // levels only on the phase gradient
      CHECK(check_stack_last(pd, c, 2, 3) != hipSuccess);
      PassCall none_out;
      none_out.jobs = buf<JobDesc>(0);
      none_out.n_jobs = 3;
      CHECK(check_stack_last(pd, none_out, 2, 3) != hipSuccess);
    }
    // what the dispatcher derives from the output description
    CHECK(pass_grad_kind(last_piece(HBX_LEAF_COMPLEX)) == kGradNone);
    CHECK(pass_grad_kind(last_piece(HBX_LEAF_REAL)) == kGradNone);
    CHECK(pass_grad_kind(last_piece(HBX_LEAF_PHASE)) == kGradPhase);
    CHECK(pass_grad_kind(last_piece(HBX_LEAF_PHASE_LEVELS)) == kGradPhaseLevels);
    CHECK(pass_grad_kind(last_piece(HBX_LEAF_THRESHOLD)) == kGradSteSigmoid);
  }
  if (fails) {
    printf("%d failures\n", fails);
    return 1;
  }
  printf("OK\n");
  return 0;
}
