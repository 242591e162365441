// Host-side check of hbx::check_pass_call (csrc/hbx_internal.hpp) for the binary-hologram calls: one
// accepted PassCall per shape hbx_evaluate_threshold / hbx_threshold_backward build (csrc/hbx_api.hip)
// and one rejected call per rule that names real_binarize, grad_kind or the sigmoid's slope.  The
// sibling of pass_call_check_phase.hip; built by tests/test_threshold_ste_host.py with the host code
// under ASan + UBSan.  Needs no GPU and no library: the validator only compares fields, no pointer
// is dereferenced.
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

static PassCall evaluate_threshold() {   // hbx_evaluate_threshold with target, field and intensity
  PassCall c;
  c.jobs = buf<JobDesc>(0);
  c.n_jobs = 3;
  c.real_values = buf<float>(1);
  c.real_binarize = 1;
  c.real_threshold = 0.5f;
  c.target = buf<float>(2);
  c.inten_out = buf<float>(3);
  c.field_out = buf<float2>(4);
  return c;
}
static PassCall threshold_backward(int kind, bool weighted) {   // hbx_threshold_backward
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
  c.grad_kind = kind;
  c.grad_p0 = kind == kGradSteWindow ? -INFINITY : 0.5f;
  c.grad_p1 = kind == kGradSteWindow ? INFINITY : 2.0f;
  return c;
}

int main() {
  const int sizes[4] = {32, 16, 8, 0};
  for (int R : sizes) {
    const PlanDev pd = plan(R);
    // -- accepted: what the two entry points build --------------------------------------------------
    PassCall c = evaluate_threshold();
    ACCEPT(pd, c);
    c.field_out = nullptr;                       // statistics and intensity
    ACCEPT(pd, c);
    c.target = nullptr;                          // the intensity alone (the lean last pass)
    ACCEPT(pd, c);
    c = evaluate_threshold();
    c.target = nullptr;                          // field and intensity, hbx_simulate_real's set
    ACCEPT(pd, c);
    c.real_threshold = NAN;                      // a value, not a switch: every bit is off
    ACCEPT(pd, c);
    for (int kind : {kGradSteWindow, kGradSteSigmoid}) {
      ACCEPT(pd, threshold_backward(kind, false));
      ACCEPT(pd, threshold_backward(kind, true));
      if (pass_reduces(threshold_backward(kind, true))) {
        printf("FAIL line %d: a gradient call reduces partials\n", __LINE__);
        fails++;
      }
    }
    c = threshold_backward(kGradSteWindow, true);   // a window may be empty or inverted: the gate is closed
    c.grad_p0 = 1.0f;
    c.grad_p1 = -1.0f;
    ACCEPT(pd, c);

    // -- rejected: the threshold rides on the real load alone ---------------------------------------
    c = evaluate_threshold();
    c.real_values = nullptr;                     // no input at all
    REJECT(pd, c);
    c = evaluate_threshold();
    c.real_values = nullptr;
    c.mask = buf<uint64_t>(8);                   // bits are thresholded already
    REJECT(pd, c);
    c = threshold_backward(kGradSteWindow, false);
    c.real_binarize = 1;                         // complex samples have no threshold
    REJECT(pd, c);
    c = PassCall();
    c.jobs = buf<JobDesc>(0);
    c.n_jobs = 3;
    c.phase_values = buf<float>(1);
    c.complex_field = buf<float2>(2);
    ACCEPT(pd, c);
    c.real_binarize = 1;                         // nor have phase samples
    REJECT(pd, c);
    c = evaluate_threshold();
    c.complex_values = buf<float2>(9);           // one input
    REJECT(pd, c);
    // -- rejected: real samples in, the real path's outputs -----------------------------------------
    c = evaluate_threshold();
    c.grad_samples = buf<float>(6);
    c.grad_phase = buf<float>(7);
    c.grad_kind = kGradSteWindow;                // the gradient forms belong to the complex last pass
    REJECT(pd, c);
    c = evaluate_threshold();
    c.real_part = buf<float>(9);
    REJECT(pd, c);
    // -- rejected: the gradient kind ----------------------------------------------------------------
    c = threshold_backward(kGradSteWindow, false);
    c.grad_kind = kGradNone;                     // the pair without a kind
    REJECT(pd, c);
    c = threshold_backward(kGradSteWindow, false);
    c.grad_kind = 4;                             // unknown
    REJECT(pd, c);
    c = threshold_backward(kGradSteWindow, false);
    c.grad_kind = -1;
    REJECT(pd, c);
    c = threshold_backward(kGradSteSigmoid, false);
    c.grad_p1 = 0.0f;                            // the sigmoid's slope is positive
    REJECT(pd, c);
    c.grad_p1 = -2.0f;
    REJECT(pd, c);
    c.grad_p1 = NAN;
    REJECT(pd, c);
    c = threshold_backward(kGradSteSigmoid, true);
    c.grad_samples = nullptr;                    // both or neither
    REJECT(pd, c);
    c = threshold_backward(kGradSteSigmoid, true);
    c.grad_phase = nullptr;
    REJECT(pd, c);
    c = threshold_backward(kGradSteWindow, true);
    c.grad_samples = nullptr;
    c.grad_phase = nullptr;
    c.real_part = buf<float>(9);                 // a kind without the pair is not read
    REJECT(pd, c);
    c.grad_kind = kGradPhase;                    // (that call with the default kind is hbx_simulate_complex_weighted)
    ACCEPT(pd, c);
    c = threshold_backward(kGradSteWindow, false);
    c.real_part = buf<float>(9);                 // the gradient alone
    REJECT(pd, c);
    c = threshold_backward(kGradSteWindow, false);
    c.complex_stats = 1;
    REJECT(pd, c);
    c = threshold_backward(kGradSteWindow, false);
    c.target = buf<float>(2);
    REJECT(pd, c);
    c = threshold_backward(kGradSteWindow, false);
    c.inten_out = buf<float>(3);
    REJECT(pd, c);

    // -- rejected: reduced-precision plans ----------------------------------------------------------
    for (int sk : {HBX_PRECISION_BF16_STORE, HBX_PRECISION_F16_STORE}) {
      const PlanDev lo = plan(R, sk);
      REJECT(lo, evaluate_threshold());
      REJECT(lo, threshold_backward(kGradSteWindow, true));
      REJECT(lo, threshold_backward(kGradSteSigmoid, false));
    }
  }
  if (fails) return 1;
  printf("OK\n");
  return 0;
}
