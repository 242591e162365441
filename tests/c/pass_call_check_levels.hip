// Host-side check of hbx::check_pass_call (csrc/hbx_internal.hpp) for the quantized-phase calls: one
// accepted PassCall per shape hbx_simulate_phase_levels / hbx_evaluate_phase_levels /
// hbx_phase_levels_backward build (csrc/hbx_api.hip), one rejected call per rule that names
// phase_levels, and what the dispatchers derive from it: the load and gradient kinds, and the
// quantizer's two constants in the arguments the continuous kinds leave unread.  The sibling of
// pass_call_check_phase.hip; built by tests/test_phase_levels_host.py with the host code under
// ASan + UBSan.  Needs no GPU and no library: nothing here dereferences a device pointer.
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

static PassCall simulate_levels(int levels) {   // hbx_simulate_phase_levels, field only
  PassCall c;
  c.jobs = buf<JobDesc>(0);
  c.n_jobs = 3;
  c.phase_values = buf<float>(1);
  c.phase_levels = levels;
  c.complex_field = buf<float2>(2);
  return c;
}
static PassCall evaluate_levels(int levels) {   // hbx_evaluate_phase_levels with target, field and intensity
  PassCall c = simulate_levels(levels);
  c.complex_stats = 1;
  c.target = buf<float>(3);
  c.inten_out = buf<float>(4);
  return c;
}
static PassCall levels_backward(int levels, bool weighted) {   // hbx_phase_levels_backward
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
  c.phase_levels = levels;
  return c;
}

static float bits_to_float(int32_t w) {
  float f;
  memcpy(&f, &w, sizeof(f));
  return f;
}

int main() {
  const int sizes[4] = {32, 16, 8, 0};
  const int good[6] = {2, 3, 4, 16, 255, 256};
  for (int R : sizes) {
    const PlanDev pd = plan(R);
    // -- accepted: what the three entry points build ------------------------------------------------
    for (int L : good) {
      PassCall c = simulate_levels(L);
      ACCEPT(pd, c);
      CHECK(!pass_reduces(c));
      c.real_part = buf<float>(8);                 // field and real part
      ACCEPT(pd, c);
      c.complex_field = nullptr;                   // real part alone
      ACCEPT(pd, c);
      c = evaluate_levels(L);
      ACCEPT(pd, c);
      CHECK(pass_reduces(c));
      c.complex_field = nullptr;                   // statistics and intensity, no field
      ACCEPT(pd, c);
      c.target = nullptr;                          // the intensity alone
      ACCEPT(pd, c);
      CHECK(!pass_reduces(c));
      ACCEPT(pd, levels_backward(L, false));
      ACCEPT(pd, levels_backward(L, true));
      CHECK(!pass_reduces(levels_backward(L, true)));

      // what the dispatchers hand the kernels: h and s are the host's float32(L / 2), float32(2.0 / L)
      const float h = (float)(L / 2.0), s = (float)(2.0 / L);
      c = simulate_levels(L);
      c.in_win = {5, 6, 7, 8};                      // never read without windowed: must not leak through
      CHECK(pass_first_scale(c) == h);
      CHECK(bits_to_float(pass_first_window(c).y0) == s);
      CHECK(pass_grad_kind(c) == kGradNone);
      c = levels_backward(L, true);
      CHECK(pass_first_scale(c) == 0.25f);         // the backward's first pass is the weighted load's
      CHECK(pass_first_window(c).y0 == 0);
      CHECK(pass_grad_kind(c) == kGradPhaseLevels);
      CHECK(pass_grad_p0(c) == h && pass_grad_p1(c) == s);
    }
    // 0 = continuous: today's calls, today's arguments
    PassCall c = simulate_levels(0);
    ACCEPT(pd, c);
    c.complex_scale = 3.0f;
    c.in_win = {1, 2, 3, 4};
    CHECK(pass_first_scale(c) == 3.0f && pass_first_window(c).y0 == 1 && pass_first_window(c).w == 4);
    c = levels_backward(0, false);
    ACCEPT(pd, c);
    c.grad_p0 = 1.5f;
    c.grad_p1 = 2.5f;
    CHECK(pass_grad_kind(c) == kGradPhase && pass_grad_p0(c) == 1.5f && pass_grad_p1(c) == 2.5f);

    // -- rejected: a value outside {0} u [2, 256] ----------------------------------------------------
    const int bad[5] = {1, -1, -4, 257, 1 << 20};
    for (int L : bad) {
      REJECT(pd, simulate_levels(L));
      REJECT(pd, evaluate_levels(L));
      REJECT(pd, levels_backward(L, false));
      REJECT(pd, levels_backward(L, true));
    }
    // -- rejected: the level count on any other load kind ... ---------------------------------------
    c = PassCall();                                // mask bits
    c.jobs = buf<JobDesc>(0);
    c.n_jobs = 3;
    c.mask = buf<uint64_t>(1);
    c.target = buf<float>(3);
    ACCEPT(pd, c);
    c.phase_levels = 4;
    REJECT(pd, c);
    c.mask = nullptr;                              // real samples, plain and thresholded
    c.real_values = buf<float>(1);
    c.phase_levels = 0;
    ACCEPT(pd, c);
    c.phase_levels = 4;
    REJECT(pd, c);
    c.real_binarize = 1;
    REJECT(pd, c);
    c = simulate_levels(4);                        // complex samples, plain and weighted, plane out
    c.phase_values = nullptr;
    c.complex_values = buf<float2>(1);
    REJECT(pd, c);
    c.complex_weight = buf<float>(5);
    REJECT(pd, c);
    c = evaluate_levels(4);                        // complex samples, statistics out
    c.phase_values = nullptr;
    c.complex_values = buf<float2>(1);
    REJECT(pd, c);
    // ... on any other gradient kind ...
    c = levels_backward(4, true);
    c.grad_kind = kGradSteWindow;
    REJECT(pd, c);
    c.grad_kind = kGradSteSigmoid;
    c.grad_p1 = 2.0f;
    REJECT(pd, c);
    c.phase_levels = 0;
    ACCEPT(pd, c);
    // ... on the phase load with the gradient pair behind it (one quantizer per call) ...
    c = simulate_levels(4);
    c.complex_field = nullptr;
    c.grad_samples = buf<float>(6);
    c.grad_phase = buf<float>(7);
    REJECT(pd, c);
    c.phase_levels = 0;
    ACCEPT(pd, c);
    // ... and together with a window
    const hbx_window_t full = {0, 0, pd.N, pd.N};
    c = simulate_levels(4);
    c.windowed = 1;
    c.in_win = full;
    c.out_win = full;
    REJECT(pd, c);
    c = levels_backward(4, false);
    c.windowed = 1;
    c.in_win = full;
    c.out_win = full;
    REJECT(pd, c);
    // f32 plans only, as every sample path
    REJECT(plan(R, HBX_PRECISION_BF16_STORE), simulate_levels(4));
    REJECT(plan(R, HBX_PRECISION_F16_STORE), levels_backward(4, false));
  }

  // the quantizer on the host, the definition the kernels compile: ties to the even k, the level by a select
  const PhaseLevels q4 = phase_levels_of(4);
  CHECK(q4.h == 2.0f && q4.s == 0.5f);
  CHECK(quantize_phase_sample(0.25f, q4.h, q4.s) == 0.0f);    // k = rint(0.5) = 0
  CHECK(quantize_phase_sample(0.75f, q4.h, q4.s) == 1.0f);    // k = rint(1.5) = 2
  CHECK(quantize_phase_sample(-0.75f, q4.h, q4.s) == -1.0f);
  CHECK(quantize_phase_sample(1.8f, q4.h, q4.s) == 0.0f && quantize_phase_sample(4097.3f, q4.h, q4.s) == -0.5f);
  CHECK(quantize_phase_level(quantize_phase_k(-0.5f, q4.h), 4) == 3);
  CHECK(quantize_phase_level(quantize_phase_k(1.0f, q4.h), 4) == 2 && quantize_phase_level(quantize_phase_k(-1.0f, q4.h), 4) == 2);
  const float nan = quantize_phase_sample(INFINITY, q4.h, q4.s);
  CHECK(nan != nan);
  CHECK(quantize_phase_level(quantize_phase_k(INFINITY, q4.h), 4) == 0);
  CHECK(quantize_phase_level(quantize_phase_k(NAN, q4.h), 4) == 0);

  if (fails) return 1;
  printf("OK\n");
  return 0;
}
