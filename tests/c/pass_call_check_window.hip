// Host-side check of hbx::check_pass_call (csrc/hbx_internal.hpp) for the windowed calls: one accepted
// PassCall per shape hbx_evaluate_real_window / hbx_evaluate_threshold_window / hbx_backward_window build
// (csrc/hbx_api.hip) and one rejected call per rule that names the windows.  The sibling of
// pass_call_check_threshold.hip; built by tests/test_window_host.py with the host code under ASan +
// UBSan.  Needs no GPU and no library: the validator only compares fields, no pointer is dereferenced.
#include <math.h>
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

static PlanDev plan(int R, int store_kind = HBX_PRECISION_F32) {
  PlanDev pd = {};
  pd.R = R;
  pd.N = R ? R * R : 896;
  pd.G = 3;
  pd.P = 8;
  pd.store_kind = store_kind;
  pd.va = 1.0f;
  pd.vb = -2.0f;
  return pd;
}

// stand-ins for device buffers: distinct non-null addresses, never read
static double store[16];
template <class T>
static T* buf(int i) { return reinterpret_cast<T*>(&store[i]); }

static void windows(PassCall& c, int N) {   // multiples of nothing, in != out
  c.windowed = 1;
  c.in_win = {5, 9, N - 24, N - 31};
  c.out_win = {3, 20, N - 30, N - 41};
}
static PassCall evaluate_window(int N, bool binarize) {   // hbx_evaluate_real_window / _threshold_window
  PassCall c;
  c.jobs = buf<JobDesc>(0);
  c.n_jobs = 3;
  c.real_values = buf<float>(1);
  c.real_binarize = binarize;
  c.real_threshold = 0.5f;
  c.target = buf<float>(2);
  c.inten_out = buf<float>(3);
  c.field_out = buf<float2>(4);
  windows(c, N);
  return c;
}
static PassCall backward_window(int N, int kind, bool weighted) {   // hbx_backward_window; kGradNone: the real part
  PassCall c;
  c.jobs = buf<JobDesc>(0);
  c.n_jobs = 3;
  c.complex_values = buf<float2>(1);
  if (weighted) {
    c.complex_weight = buf<float>(5);
    c.complex_scale = 0.25f;
  }
  if (kind == kGradNone) {
    c.real_part = buf<float>(9);
  } else {
    c.grad_samples = buf<float>(6);
    c.grad_phase = buf<float>(7);
    c.grad_kind = kind;
    c.grad_p0 = kind == kGradSteWindow ? -INFINITY : 0.5f;
    c.grad_p1 = kind == kGradSteWindow ? INFINITY : 2.0f;
  }
  windows(c, N);
  return c;
}

int main() {
  const int sizes[4] = {32, 16, 8, 0};
  for (int R : sizes) {
    const PlanDev pd = plan(R);
    const int N = pd.N;
    // -- accepted: what the three entry points build ------------------------------------------------
    for (bool bin : {false, true}) {
      PassCall c = evaluate_window(N, bin);
      ACCEPT(pd, c);
      if (!pass_reduces(c)) {
        printf("FAIL line %d: a windowed evaluation reduces its partials\n", __LINE__);
        fails++;
      }
      c.field_out = nullptr;                     // statistics and intensity
      ACCEPT(pd, c);
      c.target = nullptr;                        // the intensity alone (the lean last pass)
      ACCEPT(pd, c);
      c = evaluate_window(N, bin);
      c.target = nullptr;
      c.inten_out = nullptr;                     // the field alone
      ACCEPT(pd, c);
      c = evaluate_window(N, bin);
      c.in_win = {0, 0, N, N};                   // the full grid, either window
      ACCEPT(pd, c);
      c.out_win = {0, 0, N, N};
      ACCEPT(pd, c);
      c.in_win = {N - 1, N - 1, 1, 1};           // 1 x 1 in the last corner; a single row, a single column
      c.out_win = {0, 0, 1, N};
      ACCEPT(pd, c);
      c.out_win = {0, N - 1, N, 1};
      ACCEPT(pd, c);
    }
    for (int kind : {kGradNone, kGradSteWindow, kGradSteSigmoid}) {
      ACCEPT(pd, backward_window(N, kind, false));
      ACCEPT(pd, backward_window(N, kind, true));
      if (pass_reduces(backward_window(N, kind, true))) {
        printf("FAIL line %d: a gradient call reduces partials\n", __LINE__);
        fails++;
      }
    }
    // the windows are not read without the switch
    PassCall c = evaluate_window(N, true);
    c.windowed = 0;
    c.in_win = {-7, -7, 0, 0};
    ACCEPT(pd, c);

    // -- rejected: a window is a non-empty rectangle of the grid ------------------------------------
    const hbx_window_t bad[] = {{0, 0, N + 1, N}, {0, 0, N, N + 1}, {1, 0, N, N}, {0, 1, N, N}, {-1, 0, 4, 4},
                                {0, -1, 4, 4},    {3, 3, 0, 4},     {3, 3, 4, 0}, {3, 3, -4, 4}, {N, 0, 1, 1},
                                {0, N, 1, 1},     {0, 0, 2147483647, 1}, {2147483647, 0, 1, 1}};
    for (const hbx_window_t& w : bad) {
      c = evaluate_window(N, false);
      c.in_win = w;
      REJECT(pd, c);
      c = evaluate_window(N, true);
      c.out_win = w;
      REJECT(pd, c);
      c = backward_window(N, kGradSteWindow, true);
      c.in_win = w;
      REJECT(pd, c);
      c = backward_window(N, kGradNone, false);
      c.out_win = w;
      REJECT(pd, c);
    }
    // -- rejected: a window on any other input ------------------------------------------------------
    c = evaluate_window(N, false);
    c.real_values = nullptr;
    c.mask = buf<uint64_t>(8);                   // the bit path
    REJECT(pd, c);
    c = PassCall();
    c.jobs = buf<JobDesc>(0);
    c.n_jobs = 3;
    c.phase_values = buf<float>(1);
    c.real_part = buf<float>(9);
    ACCEPT(pd, c);
    windows(c, N);                               // phase samples
    REJECT(pd, c);
    // -- rejected: complex samples in, anything but the real part or an STE gradient out -------------
    c = backward_window(N, kGradNone, false);
    c.complex_field = buf<float2>(2);            // the complex field
    REJECT(pd, c);
    c.real_part = nullptr;
    REJECT(pd, c);
    c = backward_window(N, kGradNone, true);
    c.real_part = nullptr;
    c.complex_stats = 1;                         // the statistics form (hbx_evaluate_complex)
    c.inten_out = buf<float>(3);
    REJECT(pd, c);
    c = backward_window(N, kGradSteWindow, true);
    c.grad_kind = kGradPhase;                    // a phase leaf's gradient
    REJECT(pd, c);
    c = backward_window(N, kGradSteSigmoid, false);
    c.grad_p1 = 0.0f;                            // the unwindowed rules hold
    REJECT(pd, c);
    // -- rejected: a window with a plane cache, actions, a walk, the reconcile, env-major rows --------
    c = evaluate_window(N, false);
    c.plane_mode = kPlanesFill;
    c.plane_pool = buf<float>(10);
    c.plane_slot = buf<int32_t>(11);
    REJECT(pd, c);
    c = evaluate_window(N, false);
    c.actions = buf<int64_t>(10);
    REJECT(pd, c);
    c = evaluate_window(N, false);
    c.walk_phase = buf<uint8_t>(10);
    REJECT(pd, c);
    c = evaluate_window(N, false);
    WalkPlanesArgs wk = {};
    c.walk_planes = &wk;
    REJECT(pd, c);
    c = evaluate_window(N, false);
    c.rc_pending = buf<int32_t>(10);
    c.rc_cache = buf<float>(11);
    REJECT(pd, c);
    c = evaluate_window(N, false);
    c.inten_by_env = 1;
    REJECT(pd, c);
    c = evaluate_window(N, false);
    c.skip_reduce = 1;
    REJECT(pd, c);

    // -- rejected: reduced-precision plans ----------------------------------------------------------
    for (int sk : {HBX_PRECISION_BF16_STORE, HBX_PRECISION_F16_STORE}) {
      const PlanDev lo = plan(R, sk);
      REJECT(lo, evaluate_window(N, false));
      REJECT(lo, evaluate_window(N, true));
      REJECT(lo, backward_window(N, kGradNone, true));
      REJECT(lo, backward_window(N, kGradSteSigmoid, false));
    }
  }
  if (fails) return 1;
  printf("OK\n");
  return 0;
}
