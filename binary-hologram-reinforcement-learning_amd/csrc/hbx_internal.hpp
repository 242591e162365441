// hbx_internal.hpp -- types shared by the kernels and the C-ABI layer.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "hbx.h"

namespace hbx {

// tt.relativeLoss(.., tm.get_PSNR) from the channel sums (env.py:174):
// lsq scale s = sum IT / sum I^2, mse = mean((s I - T)^2), psnr = 10 log10(peak^2 / mse)
__device__ __forceinline__ double psnr_from(double sxy, double sxx, double syy, double count,
                                            int rel_scale, double peak) {
  double mse;
  if (rel_scale == 1) mse = (sxx > 0.0) ? (syy - sxy * sxy / sxx) / count : syy / count;
  else mse = (sxx - 2.0 * sxy + syy) / count;
  if (!(mse > 0.0)) return INFINITY;
  return 10.0 * log10(peak * peak / mse);
}

// Increment of one pixel's plane-mean intensity when a flip adds delta * h to
// its field u: (|u + delta h|^2 - |u|^2) / P = delta (2 Re(u conj h) + delta |h|^2) / P,
// formed without the two squares, so its f32 error is relative to the
// increment itself (differencing the squares loses it to the rounding of |u|^2
// wherever |h| << |u|, i.e. almost everywhere: ~1e-10 dB of noise per 1024x24
// candidate).  Incremental-field kernels (hbx_psf.hip, hbx_walk.hip).
__device__ __forceinline__ float flip_dI(float ur, float ui, float hr, float hi, float delta, float invp) {
  const float re = fmaf(ur, hr, ui * hi);
  const float hh = fmaf(hr, hr, hi * hi);
  return delta * fmaf(delta, hh, 2.0f * re) * invp;
}

// One colour-group propagation: env index (plan-local), group, optional flip.
struct JobDesc {
  int32_t env;         // < 0: invalid job (skipped, outputs neutral)
  int32_t group;
  int32_t flip_plane;  // plane within the group, -1 = no flip
  int32_t flip_pix;    // row * W + col
};

// env.py:157-161: action -> (channel, pixel) of env b; an action outside [0, CH*hw) is an
// invalid job (env -1).  Shared by k_jobs_from_actions and the first pass's fused decode.
__host__ __device__ __forceinline__ JobDesc job_of_action(int64_t a, int b, int64_t hw, int P, int CH) {
  JobDesc jd;
  if (a < 0 || a >= (int64_t)CH * hw) {
    jd.env = -1; jd.group = 0; jd.flip_plane = -1; jd.flip_pix = 0;
  } else {
    const int ch = (int)(a / hw);
    jd.env = b;
    jd.group = ch / P;
    jd.flip_plane = ch % P;
    jd.flip_pix = (int)(a % hw);
  }
  return jd;
}

// Intermediate layout of the fused N = R^2 path (hbx_passes.hip).  The row
// passes run blocks of row_nt(R) = 256 threads = panel_rows(R) rows; a plane of
// L lines is stored as N / PAN panels [L][PAN], panel q at q * PAN * L.  A is
// kept in panels of the row block height (8 rows at N = 1024: every k_rowfwd
// store is contiguous -- 0.69 ms for the 128-job A vs 1.19 ms as 64-B pieces of
// line-major A, tools/membw2.hip -- and k_col2's line reads cost nothing), B in
// panels of 16 rows (k_col2 writes 128-B pieces; 8-row B panels made its
// stores cost 1 ms more, 32 / 64 rows or a pad between panels were slower too:
// DESIGN.md 4).
constexpr int kPanelA = 8;
constexpr int kPanelB = 16;
__host__ __device__ constexpr int row_nt(int R) { return 256; }
__host__ __device__ constexpr int panel_rows(int R) { return row_nt(R) / R; }
__host__ __device__ constexpr int pan_of(int R, int rows) {
  return rows <= 0 || rows >= R * R ? R * R : (rows < panel_rows(R) ? panel_rows(R) : rows);
}
__host__ __device__ constexpr int pan_a(int R) { return pan_of(R, kPanelA); }
__host__ __device__ constexpr int pan_b(int R) { return pan_of(R, kPanelB); }
__host__ __device__ constexpr int panel_stride(int R, int L, int PAN) { return L * PAN; }
// float2 elements per intermediate plane: A (half spectrum, N/2 lines), B (N lines)
__host__ __device__ constexpr size_t plane_a_elems(int R) {
  return (size_t)(R * R / pan_a(R)) * panel_stride(R, R * R / 2, pan_a(R));
}
__host__ __device__ constexpr size_t plane_b_elems(int R) {
  return (size_t)(R * R / pan_b(R)) * panel_stride(R, R * R, pan_b(R));
}

// The launch-size switch of the bit path's first pass and of the column pass (hbx_passes.hip, N = 1024 /
// 256).  The walking forms -- a workgroup walks rowfwd_iters row blocks of a plane pair, col2_iters lines
// of a lane group -- trade parallelism for store overlap, which pays only when the launch fills the chip
// many times over; a launch of fewer than kSmallBlocks workgroups in both passes runs the forms with one
// row block / one line per workgroup instead.  pass_launch_small is the one place that decides
// (launch_passes calls it); tests/c/launch_size_table.hip prints where it turns, tests/_launch_size.py
// restates it for the GPU tests that put one input through both forms (tests/test_gpu_launch_size.py).
__host__ __device__ constexpr int pass_rowfwd_iters(int R) { return R == 32 ? 4 : (R == 16 ? 2 : 1); }
__host__ __device__ constexpr int pass_col2_iters(int R) { return R == 32 ? 4 : (R == 16 ? 2 : 1); }
constexpr unsigned kSmallBlocks = 2048;
// workgroups of the walking first pass / column pass for n_jobs jobs of P planes (pair: the plane-cached
// step, one plane pair per job)
inline unsigned pass_rowfwd_blocks(int R, int P, int n_jobs, bool pair) {
  const unsigned row_blocks = R * R / panel_rows(R);   // per plane pair
  return (unsigned)n_jobs * (pair ? 1 : P / 2) * row_blocks / pass_rowfwd_iters(R);
}
inline unsigned pass_col2_blocks(int R, int P, int n_jobs, bool pair) {
  const int gpb = 256 / R;                             // lane groups per workgroup
  return (unsigned)n_jobs * (pair ? 2 : P) * ((R * R / 2) / (gpb * pass_col2_iters(R)));
}
// N = 64 (R = 8) has one form of each kernel, N = 896 its own launcher: never small
inline bool pass_launch_small(int R, int P, int n_jobs, bool pair) {
  return (R == 32 || R == 16) && pass_rowfwd_blocks(R, P, n_jobs, pair) < kSmallBlocks &&
         pass_col2_blocks(R, P, n_jobs, pair) < kSmallBlocks;
}

// Line kx of a panel-layout plane as addressed by lane t of an R-lane group:
// element y = t + R jj sits at byte offset voff(t, kx) + joff(jj) from the
// plane base (joff is a compile-time constant per jj: an SGPR or immediate
// offset of a buffer instruction, so one address VGPR serves the whole line).
template <int R, int L, int PAN>
struct PanelLine {
  static constexpr int PS = panel_stride(R, L, PAN);
  // element (line, y) of the plane
  __device__ __forceinline__ static constexpr size_t at(int line, int y) {
    return (size_t)(y / PAN) * PS + (size_t)line * PAN + y % PAN;
  }
  __device__ __forceinline__ static int voff(int t, int kx) {
    if constexpr (R > PAN) return ((t / PAN) * PS + kx * PAN + t % PAN) * 8;
    else return (kx * PAN + t) * 8;
  }
  __device__ __forceinline__ static constexpr int joff(int jj) {
    if constexpr (R > PAN) return jj * (R / PAN) * PS * 8;
    else return (((R * jj) / PAN) * PS + (R * jj) % PAN) * 8;
  }
};

// Optional hipEvent pairs around every `every`-th pass launch (hbx_plan_set_timing*).
constexpr int kNumPasses = 5;  // rowfwd, col, rowinv, psf_eval, psf_commit
struct PassTimer {
  int capacity = 0;
  int every = 1;
  int count[kNumPasses] = {};
  int64_t calls[kNumPasses] = {};   // launches seen (recorded or not)
  bool open[kNumPasses] = {};       // begin() recorded, end() pending
  int64_t jobs[kNumPasses] = {};
  hipEvent_t* ev[kNumPasses] = {};  // [2 * capacity] start/stop
  __host__ void begin(int pass, hipStream_t st) {
    open[pass] = capacity && count[pass] < capacity && calls[pass] % every == 0;
    if (open[pass]) (void)hipEventRecord(ev[pass][2 * count[pass]], st);
  }
  __host__ void end(int pass, int n_jobs, hipStream_t st) {
    ++calls[pass];
    if (open[pass]) {
      (void)hipEventRecord(ev[pass][2 * count[pass] + 1], st);
      ++count[pass];
      jobs[pass] += n_jobs;
      open[pass] = false;
    }
  }
};

// the FFT-mode plane-cache walk's decision (hbx_walk_planes.hpp): everything it reads and writes
struct WalkPlanesArgs {
  hbx_dbs_walk_t* w;
  const int64_t* order;
  JobDesc* jobs;
  const double* partial;     // [K][RB][3] row-block partials of the batch just propagated
  uint64_t* mask;
  double* base_stats;
  int32_t* plane_slot;
  int64_t* accept_pos;
  double* accept_psnr;
  int64_t accept_cap;
  int32_t* ticket;           // fused decision: arrival counter of the k_rowinv_d workgroups
  int RB, K, G, P, H, W;
  double count;
  int rel_scale;
  double peak;
  // (ABI v13, extension) on-pixel ratio constraint: per-group on-pixel counts (nullptr = off),
  // the target count and the tolerance (hbx_dbs_walk_planes_fill)
  int64_t* fill_count = nullptr;
  int64_t fill_target = 0;
  int64_t fill_tol = 0;
  // (r06) candidate retention across batches (fused decision only; nullptr = off): the batch's
  // candidate i sits in job slot (*ring + i) % K, and phase[slot] tells the passes what a slot
  // still needs -- 0 everything, 1 only k_rowinv_d (its pair's B is still valid), 2 nothing (its
  // partials and fresh pair are still valid).  Slots are kept by the candidates a batch propagated
  // but did not visit (hbx_walk_planes.hpp)
  int32_t* ring = nullptr;
  uint8_t* phase = nullptr;
};

// (extension, hbx_dbs_walk_planes_anneal) the annealed walk's slack: it travels in the plan's 64-byte
// ticket block, behind the arrival counter, so WalkPlanesArgs -- a by-value argument of every
// k_rowinv_d -- keeps its size and no existing kernel's descriptor moves.  Written by the call's
// k_walk_planes_anneal launch, read by the fused decision of the launches behind it.
struct WalkAnnealBlock {
  const double* slack;
  int64_t n_slack;
};
__host__ __device__ __forceinline__ WalkAnnealBlock* walk_anneal_block(int32_t* ticket) {
  return reinterpret_cast<WalkAnnealBlock*>(ticket + 2);   // bytes 8..23 of the block
}

// What a plan owns: geometry, tables, workspaces.  Never copied to describe a launch -- what one
// propagation needs beyond the plan is a PassCall (below).
struct PlanDev {
  int R;               // N = R * R; 0: N = 896 = 28 x 32 (generic path)
  int N, G, P;
  float va, vb;        // field = va + vb * bit
  float2* tw;          // [N]  W_N^{t k1} at [k1 * R + t]; N = 1024 appends the
                       // whole-wave tables [16][64] W1024^{L k1}, [16][4] W64^{l0 m1}
  float2* htab;        // [G][N/2 + 1][N]  H(kx, ky) / (2 N^2): the row passes write 2 A
  float2* ws_a;        // [max_jobs][P][N/2][N]  half spectrum after k_rowfwd (line kx, over y)
  float2* ws_b;        // [max_jobs][P][N][N]    after k_col (line kx, over y)
  double* partial;     // [max_jobs][N / (256/R)][3]
  double* job_stats;   // [max_jobs][3]
  float2* hpsf;        // [G][N][N] single-pixel field h_g = IFFT2(H_g) (lazy, incremental mode)
  double* psf_partial; // [max_jobs][kPsfBlocks][2]
  int32_t* psf_order;  // [max_jobs] jobs sorted by colour group (launch order)
  float* zero_row;     // [N] zeros: the target row of a propagation without a target
  int store_kind;      // HBX_PRECISION_*: rounding of the pass intermediates (0 = f32, the product)
  PassTimer* timer;    // nullable
  // (extension, hbx_plan_set_depths) the focal stack's tables: depth d's table is the htab of a plan
  // created with optics.z = z[d], bit for bit.  Null / 0 until depths are set; only a PassCall with
  // stack_depth >= 0 reads them
  float2* htab_stack;  // [n_depths][G][N/2 + 1][N]
  int n_depths;
};

// plane-cached FFT mode (ABI v9; N = 1024 / 896 / 256), PassCall::plane_mode:
//   kPlanesOff    no plane cache
//   kPlanesFill   full propagation: every plane's |U_p|^2 also goes to its pool slot
//   kPlanesStep   env step: only the flipped plane's pair is propagated, the other planes'
//                 |U_q|^2 come from the pool (k_rowinv_d sums them in the same plane order,
//                 so the group intensity is the FFT mode's bit for bit); the pair's fresh
//                 |U|^2 go to the env's two spare slots (swapped in on accept)
constexpr int kPlanesOff = 0, kPlanesFill = 1, kPlanesStep = 2;

// What the real first passes (k_rowfwd_real, k_rowfwd32_real, k_rowfwd896_real) load a row with:
// real_load_row or threshold_load_row (hbx_rowcol.hpp) ...
constexpr int kLoadReal = 0, kLoadThreshold = 1;
// ... and the complex ones (k_rowfwd_cplx, k_rowfwd32_cplx, k_rowfwd896_cplx): complex_load_row,
// complex_load_row_weighted or phase_load_row; kLoadPhaseLevels (hbx_simulate_phase_levels): phase_load_row
// with the quantizer (quantize_phase_sample, below) between the load and the sincos
constexpr int kLoadComplex = 0, kLoadWeighted = 1, kLoadPhase = 2, kLoadPhaseLevels = 3;

// What the complex last passes (k_rowinv_d_cplx, k_rowinv_cplx, k_rowinv896_cplx) write: the plane
// (field, real part, statistics: kGradNone), or a real leaf's gradient instead of it --
// phase_grad_row, or ste_grad_row with one of the two surrogate derivatives (hbx_rowcol.hpp).
// PassCall::grad_kind is one of the last three.  kGradPhaseLevels (hbx_phase_levels_backward) is never
// named by a caller: it is kGradPhase with PassCall::phase_levels set (pass_grad_kind), phase_grad_row
// with the quantizer on the samples it loads
constexpr int kGradNone = 0, kGradPhase = 1, kGradSteWindow = 2, kGradSteSigmoid = 3, kGradPhaseLevels = 4;

// Illumination fields (hbx.h, "Illumination fields"): the leaf kind a sourced first pass (k_rowfwd_src,
// k_rowfwd32_src, k_rowfwd896_src) or the materialiser (k_source_field, hbx_pack.hip) forms f from, before
// it multiplies by the source sample s (source_leaf_field / source_mul, below).  Every kind fills one
// complex plane per leaf plane
constexpr int kSrcComplex = 0, kSrcPhase = 1, kSrcPhaseLevels = 2, kSrcReal = 3, kSrcThreshold = 4;

// The phase quantizer (hbx.h, "Quantized phase holograms"): the float32 phase sample x, in units of pi,
// to the nearest of L levels 2 k / L.  Every operation is float32, round-half-to-even:
//   r = x - 2 rint(x / 2)   exact, r in [-1, 1] (so a contraction of the subtract into an fma changes nothing)
//   k = rint(r h)           h = float32(L / 2): one multiply, then the rounding
//   q = k s                 s = float32(2.0 / L): one multiply
// Ties go to the even k -- deliberately not hbx_evaluate_threshold's >= rule: rint is one instruction, and
// a quantizer that is odd in x keeps q(-x) = -q(x).  A non-finite x gives q = NaN (inf - inf).
// h and s are the host's values (phase_levels_of) wherever a kernel quantizes: the pass kernels, the
// export kernel (hbx_pack.hip) and the host-side checks share this one definition.
struct PhaseLevels {
  float h, s;
};
inline PhaseLevels phase_levels_of(int levels) { return {(float)(levels / 2.0), (float)(2.0 / levels)}; }
__host__ __device__ __forceinline__ float quantize_phase_k(float x, float h) {
  const float r = x - 2.0f * rintf(x * 0.5f);
  return rintf(r * h);
}
__host__ __device__ __forceinline__ float quantize_phase_sample(float x, float h, float s) {
  return quantize_phase_k(x, h) * s;
}
// the level the device displays, k mod L in [0, L); a NaN k gives 0 by a select, no NaN is ever cast
__host__ __device__ __forceinline__ int quantize_phase_level(float k, int levels) {
  const int ki = (int)(k == k ? k : 0.0f);
  return ki < 0 ? ki + levels : ki;
}

// One three-pass propagation (run_jobs): everything a launch needs beyond the plan.  A call site
// names what it sets; check_pass_call states which combinations mean something.
struct PassCall {
  const JobDesc* jobs = nullptr;
  int n_jobs = 0;
  // the input, exactly one of four: the packed mask bits (u = va + vb * bit) ...
  const uint64_t* mask = nullptr;
  // ... (ABI v15) a real-valued field: [env][G*P][N][N] f32 samples the first pass reads instead of
  // the mask bits (u = value; va / vb are not applied).  f32 intermediates, no plane cache, no
  // actions, no walk ...
  const float* real_values = nullptr;
  // (ABI v15, additive) hbx_evaluate_threshold: 1 with real_values = the samples are the real leaf of a
  // binary hologram, and the first pass propagates u = va + vb [x >= real_threshold] (NaN: the bit is
  // off), formed as it loads x.  Everything behind the load is real_values' path
  int real_binarize = 0;
  float real_threshold = 0.0f;
  // ... or (ABI v15, additive) a complex field (hbx_simulate_complex): [env][G*P/2][N][N] complex64
  // samples the first pass reads, complex plane q into plane-pair slot q; the last pass recombines
  // each pair and writes complex_field [env][G*P/2][N][N] complex64 and / or real_part
  // [env][G*P/2][N][N] f32 (at least one non-null) and nothing else -- intensity, partials and
  // statistics only with complex_stats below.  f32 intermediates, no plane cache, no actions, no walk
  const float2* complex_values = nullptr;
  // (ABI v15, additive) hbx_simulate_complex_weighted: [env][G][N][N] f32, non-null only with
  // complex_values; the first pass propagates (complex_scale * complex_weight[env][group]) * values
  const float* complex_weight = nullptr;
  float complex_scale = 1.0f;
  // ... or (ABI v15, additive) a phase hologram (hbx_simulate_phase): [env][G*P/2][N][N] f32 samples x,
  // u = exp(i pi x) formed by the first pass as it loads them, phase plane q into plane-pair slot q.
  // Everything behind the load is complex_values' path: the same outputs and the same rules
  const float* phase_values = nullptr;
  // (ABI v15, additive) hbx_*_phase_levels: the number of levels L in [2, 256] the phase samples are
  // quantized to as they are loaded (quantize_phase_sample), 0 = continuous.  With phase_values: the first
  // pass propagates exp(i pi q(x)); with the phase-gradient pair below: the last pass evaluates its
  // gradient at q(grad_samples) -- the straight-through estimator dq/dx := 1.  Neither q nor u is written.
  // Never with a window (phase leaves are not windowed) or any other load or gradient kind
  int phase_levels = 0;
  // env step at N = 1024 / 256: the first pass decodes the actions itself (no
  // k_jobs_from_actions launch) and one of its workgroups per job writes the JobDesc the later
  // passes read
  const int64_t* actions = nullptr;
  int32_t* act_err = nullptr;
  // the outputs
  const float* target = nullptr;   // [env][G][N][N]; null: the plan's zero row, nothing meaningful reduced
  float* inten_out = nullptr;      // plane-mean intensity rows (nullable)
  int inten_by_env = 0;            // their order: 0 = job-major [job][N][N]; 1 = env-major
                                   // [env][G][N][N] at (job.env, job.group) (the obs recon buffer, ABI v8)
  float2* field_out = nullptr;     // [env][G*P][N][N] complex field of every propagated plane (nullable)
  float2* complex_field = nullptr; // complex input only, see complex_values
  float* real_part = nullptr;
  // (ABI v15, additive) hbx_evaluate_complex: 1 with complex_values = the last pass also accumulates
  // |F_q|^2 over the group's P/2 complex planes and runs the real last pass's tail -- the plane-mean
  // intensity to inten_out [job][N][N] (job-major; nullable) and the partials against target (null:
  // the zero row, nothing reduced).  complex_field and real_part may then both be null
  int complex_stats = 0;
  // (ABI v15, additive) hbx_phase_backward: with complex or phase input, both or neither.  The last
  // pass takes each recombined plane as the gradient g with respect to u = exp(i pi x), x =
  // grad_samples [env][G*P/2][N][N] f32, and writes grad_phase (same shape) = pi (Im g cos pi x -
  // Re g sin pi x) and nothing else: no complex_field, real_part or complex_stats
  const float* grad_samples = nullptr;
  float* grad_phase = nullptr;
  // (ABI v15, additive) hbx_threshold_backward: which gradient the pair above asks for.  kGradPhase is
  // the one just described.  kGradSteWindow / kGradSteSigmoid: grad_samples is the real leaf x of a
  // binary hologram u = va + vb [x >= thr], and grad_phase = vb s(x) Re g with the surrogate derivative
  // s = [grad_p0 <= x <= grad_p1], or s = k sg (1 - sg), sg = sigmoid(k (x - grad_p0)), k = grad_p1 > 0.
  // Any other kind than kGradPhase only with the pair
  int grad_kind = kGradPhase;
  float grad_p0 = 0.0f, grad_p1 = 0.0f;
  // (ABI v15, additive) hbx_*_window: 1 = the input sits in in_win of the grid and is 0 elsewhere, the
  // outputs are taken over out_win, and every array that belongs to a window is compact ([..][h][w], row
  // pitch w).  in_win: real_values, or complex_values and complex_weight; out_win: target, inten_out
  // (job-major) and field_out, or real_part, or grad_samples and grad_phase (the two STE kinds).  Both are
  // whole rectangles of the grid (a full-grid window is the unwindowed layout), never read with windowed = 0
  int windowed = 0;
  hbx_window_t in_win = {0, 0, 0, 0}, out_win = {0, 0, 0, 0};
  // the plane cache (kPlanes* above)
  int plane_mode = kPlanesOff;
  float* plane_pool = nullptr;          // [env][CH + 2S][N][N] f32 per-plane |U|^2 (env ids as the jobs carry them)
  const int32_t* plane_slot = nullptr;  // [env][CH + 2S] pool slot of every plane; [CH + 2s], [CH + 2s + 1] = spare pair s
  int plane_spares = 0;                 // S: spare pairs per env (0 / 1: the env step's one pair).  S > 1 (ABI v10,
                                        // hbx_eval_flips_planes): candidate j of a launch writes its pair to spare
  int spare_base = 0;                   // pair spare_base + j, so K candidates of one base keep K fresh pairs
  // (r04) env step with the recon observation at N = 1024 / 256: k_rowinv_d applies the previous
  // step's recon / intensity-cache reconcile (recon_pending, env-major like inten_out) itself
  const int32_t* rc_pending = nullptr;  // [env]
  float* rc_cache = nullptr;            // [env][G][N][N] the intensity cache
  int skip_reduce = 0;                  // 1: leave the per-row-block partials (a caller reduces them itself)
  const uint8_t* walk_phase = nullptr;          // (r06) per job slot: 0 all passes, 1 k_rowinv_d only,
                                                // 2 none (WalkPlanesArgs::phase; nullptr = all)
  const WalkPlanesArgs* walk_planes = nullptr;  // (r05) plane-cache walk batch: the last k_rowinv_d
                                                // workgroup decides (hbx_walk_planes.hpp)
  int walk_anneal = 0;                          // 1: the annealed decision (k_rowinv_walk_anneal; walk_planes set)
  // (extension, hbx_evaluate_stack / hbx_backward_stack) a focal stack runs the three passes in pieces.
  // stack_depth >= 0: the column pass multiplies by depth stack_depth's table (PlanDev::htab_stack), -1 by
  // the plan's own.  stack_skip_first: the first pass does not run -- ws_a holds the chunk's row spectra,
  // left by the call for depth 0 (they do not depend on z).  stack_skip_last: the call ends behind the
  // column pass -- the depth-summing last pass (StackLast, run_stack_last) reads the D slot ranges of ws_b.
  // stack_slot0: the job slot of ws_a / ws_b the call's job 0 runs in (the backward puts depth d's jobs at
  // d * nj).  Sample inputs only; no window, plane cache, actions, walk or reconcile (check_pass_call)
  int stack_depth = -1;
  int stack_skip_first = 0;
  int stack_skip_last = 0;
  int stack_slot0 = 0;
  // (extension, hbx_evaluate_pw / hbx_evaluate_stack_pw) a non-negative per-pixel loss weight v,
  // [env][G][N][N] f32 addressed as target: the last pass's three sums become sum v I T, sum v I^2 and
  // sum v T^2 (rowinv_epilogue_pw); the intensity and the field stay the unweighted ones.  Only with a
  // target and statistics on the f32 sample paths (complex or phase in: complex_stats and no real part);
  // never with a window, plane cache, actions, walk, reconcile or env-major output (check_pass_call).
  // Null: the launches a call ran before
  const float* pixel_weight = nullptr;
  // (extension, hbx_evaluate_source / hbx_backward_source) the illumination: [G][N][N] complex64, constant,
  // shared by every env and plane of a colour group.  source_adjoint = 0, the forward: the first pass
  // propagates u = s f (source_load_row), f from complex_values, phase_values (with phase_levels) or
  // source_real below, and the last pass is the complex path's as it is.  source_adjoint = 1, the backward
  // on the plan for -z: complex_values (with or without complex_weight) in through the existing loads, and
  // the last pass multiplies the plane by conj(s) before its one output -- complex_field, real_part, or the
  // gradient pair with its kind -- without statistics.  Only on the complex path of an f32 plan; never
  // with a window, a stack piece, the plane cache, actions, a walk, the reconcile or env-major output
  // (check_pass_call).  Null: the launches a call ran before
  const float2* source = nullptr;
  int source_adjoint = 0;
  // ... and the fifth input (counted by "exactly one"): real samples [env][G*P/2][N][N] f32 into complex
  // plane slots, u = s x, or with source_binarize u = s (va + vb [x >= source_threshold]).  Only with a
  // source in the forward: the real kinds have one plane per leaf plane there, not a pair
  const float* source_real = nullptr;
  int source_binarize = 0;
  float source_threshold = 0.0f;
};
// whether any focal-stack field is set
inline bool pass_stack(const PassCall& c) {
  return c.stack_depth >= 0 || c.stack_skip_first || c.stack_skip_last || c.stack_slot0 != 0;
}
// the transfer-function table the column pass of this call reads
inline const float2* pass_htab(const PlanDev& pd, const PassCall& c) {
  if (c.stack_depth < 0) return pd.htab;
  return pd.htab_stack + (size_t)c.stack_depth * pd.G * (size_t)(pd.N / 2 + 1) * pd.N;
}

// a window (hbx_window_t) that is a non-empty rectangle of the N x N grid
inline bool window_in_grid(const hbx_window_t& w, int N) {
  return w.y0 >= 0 && w.x0 >= 0 && w.h >= 1 && w.w >= 1 && w.y0 <= N - w.h && w.x0 <= N - w.w;
}

// Whether the first pass takes its predicated loads: an input window that is the whole grid is the
// unwindowed layout, and the plain loads measured 3 % faster there
inline bool pass_window_in(const PassCall& c, int N) {
  return c.windowed && !(c.in_win.y0 == 0 && c.in_win.x0 == 0 && c.in_win.h == N && c.in_win.w == N);
}

// The complex path: complex or phase samples in, the pair-recombining last pass out
inline bool pass_complex(const PassCall& c) { return c.complex_values || c.phase_values || c.source_real; }

// The quantizing forms' constants reach the kernels in arguments their load / gradient kind leaves unread, so
// no kernel signature changes (and no existing kernel's code): the first pass reads h where the weighted load
// reads scale and the bits of s in the first word of the window it is never given (phase leaves are not
// windowed); the last pass reads (h, s) where the STE kinds read (ga, gb).
inline float pass_first_scale(const PassCall& c) {
  return c.phase_values && c.phase_levels ? phase_levels_of(c.phase_levels).h : c.complex_scale;
}
inline hbx_window_t pass_first_window(const PassCall& c) {
  if (!(c.phase_values && c.phase_levels)) return c.in_win;
  const float s = phase_levels_of(c.phase_levels).s;
  hbx_window_t w = {0, 0, 0, 0};
  static_assert(sizeof(w.y0) == sizeof(s), "a float's bits in an int32");
  memcpy(&w.y0, &s, sizeof(s));
  return w;
}
// the last pass's gradient kind and its two parameters
inline int pass_grad_kind(const PassCall& c) {
  return !c.grad_phase ? kGradNone : (c.grad_kind == kGradPhase && c.phase_levels ? kGradPhaseLevels : c.grad_kind);
}
inline float pass_grad_p0(const PassCall& c) {
  return pass_grad_kind(c) == kGradPhaseLevels ? phase_levels_of(c.phase_levels).h : c.grad_p0;
}
inline float pass_grad_p1(const PassCall& c) {
  return pass_grad_kind(c) == kGradPhaseLevels ? phase_levels_of(c.phase_levels).s : c.grad_p1;
}

// the sourced first pass's leaf kind (kSrc*), its samples as floats and its three parameters (source_sample)
inline int pass_source_kind(const PassCall& c) {
  return c.source_real ? (c.source_binarize ? kSrcThreshold : kSrcReal)
                       : c.phase_values ? (c.phase_levels ? kSrcPhaseLevels : kSrcPhase) : kSrcComplex;
}
inline const float* pass_source_samples(const PassCall& c) {
  return c.source_real ? c.source_real : c.phase_values ? c.phase_values : reinterpret_cast<const float*>(c.complex_values);
}
struct SourceParams {
  float p0, p1, p2;
};
inline SourceParams pass_source_params(const PlanDev& pd, const PassCall& c) {
  const int sk = pass_source_kind(c);
  if (sk == kSrcPhaseLevels) return {phase_levels_of(c.phase_levels).h, phase_levels_of(c.phase_levels).s, 0.0f};
  if (sk == kSrcThreshold) return {c.source_threshold, pd.va, pd.va + pd.vb};
  return {0.0f, 0.0f, 0.0f};
}

// Which PassCalls the pass kernels of this plan can run: every field a selected kernel would not
// read is refused, not ignored.  run_jobs calls it before a timer slot opens or a kernel is enqueued.
inline hipError_t check_pass_call(const PlanDev& pd, const PassCall& c) {
  const bool tiled = pd.R == 32 || pd.R == 16;   // the k_rowinv_d sizes
  const bool f32 = pd.store_kind == HBX_PRECISION_F32;
  const bool planes = c.plane_mode != kPlanesOff;
  const bool walk = c.walk_phase || c.walk_planes;
  const bool complex_out = c.complex_field || c.real_part || c.complex_stats;
  const bool grad_out = c.grad_samples || c.grad_phase;
  bool ok = (c.mask != nullptr) + (c.real_values != nullptr) + (c.complex_values != nullptr) +
            (c.phase_values != nullptr) + (c.source_real != nullptr) == 1;
  ok = ok && (!planes || (c.plane_pool && c.plane_slot && (tiled || pd.R == 0)));
  ok = ok && (!c.walk_planes || (c.plane_mode == kPlanesStep && tiled));
  ok = ok && (!c.walk_anneal || c.walk_planes);
  ok = ok && (!c.rc_pending == !c.rc_cache) && (!c.rc_pending || tiled);
  ok = ok && (c.actions || !c.act_err);
  if (pd.R == 0) ok = ok && !c.walk_phase && !c.actions && !c.skip_reduce;
  // real, complex and phase samples: the f32 product path alone
  if (!c.mask) ok = ok && f32 && !planes && !c.actions && !walk;
  // complex or phase in, complex out: the pair-recombining last pass writes these and nothing else ...
  ok = ok && (pass_complex(c) ? (complex_out || grad_out || c.stack_skip_last) && !c.field_out && !c.inten_by_env && !c.rc_pending &&
                                    !c.skip_reduce
                              : !complex_out && !grad_out);
  // ... or the phase gradient alone, from its samples
  ok = ok && (!grad_out || (c.grad_samples && c.grad_phase && !complex_out && !c.target && !c.inten_out));
  // its kind: the phase form unless the pair is there; the sigmoid's slope is positive (NaN is not)
  ok = ok && (c.grad_kind == kGradPhase ||
              (grad_out && (c.grad_kind == kGradSteWindow || (c.grad_kind == kGradSteSigmoid && c.grad_p1 > 0.0f))));
  // the weight rides on the complex load, the threshold on the real one
  ok = ok && (c.complex_values || !c.complex_weight);
  ok = ok && (c.real_values || !c.real_binarize);
  // the level count: 0 or [2, 256], on the phase load or on the phase gradient and nowhere else, no window
  if (c.phase_levels != 0) {
    ok = ok && c.phase_levels >= 2 && c.phase_levels <= 256;
    ok = ok && (c.phase_values ? !grad_out : (grad_out && c.grad_kind == kGradPhase));
    ok = ok && !c.windowed;
  }
  // windows: whole rectangles of the grid; real samples in, or complex samples in and the real part or an
  // STE gradient out; no plane cache, actions, walk or reconcile, and nothing env-major
  if (c.windowed) {
    ok = ok && window_in_grid(c.in_win, pd.N) && window_in_grid(c.out_win, pd.N);
    ok = ok && (c.real_values || (c.complex_values && !c.complex_field && !c.complex_stats &&
                                  (c.real_part || (grad_out && c.grad_kind != kGradPhase))));
    ok = ok && !planes && !c.actions && !walk && !c.rc_pending && !c.inten_by_env && !c.skip_reduce;
  }
  // a focal stack's pieces: a depth the plan has a table for (every piece names one); sample inputs on the
  // f32 path; no window, plane cache, actions, walk or reconcile, nothing env-major, the reduction as it is.
  // A call that stops behind the column pass has complex samples in and no output of its own; one that
  // skips the first pass is a forward piece (the slot offset is the backward's)
  if (pass_stack(c)) {
    ok = ok && c.stack_depth >= 0 && c.stack_depth < pd.n_depths && pd.htab_stack;
    ok = ok && !c.mask && f32;
    ok = ok && !c.windowed && !planes && !c.actions && !walk && !c.rc_pending && !c.inten_by_env && !c.skip_reduce;
    ok = ok && c.stack_slot0 >= 0;
    ok = ok && !(c.stack_skip_first && (c.stack_skip_last || c.stack_slot0 != 0));
    ok = ok && (!c.stack_slot0 || c.stack_skip_last);
    if (c.stack_skip_last) ok = ok && c.complex_values && !complex_out && !grad_out && !c.target && !c.inten_out;
  }
  // a per-pixel loss weight: sample input on the f32 path, with a target and the reduced statistics (complex or
  // phase in: the statistics form, no real part, no gradient); no window, plane cache, actions, walk or
  // reconcile, nothing env-major, and not a piece that stops in front of the last pass
  if (c.pixel_weight) {
    ok = ok && !c.mask && f32 && c.target && !c.skip_reduce;
    ok = ok && (!pass_complex(c) || (c.complex_stats && !c.real_part && !grad_out));
    ok = ok && !c.windowed && !planes && !c.actions && !walk && !c.rc_pending && !c.inten_by_env;
    ok = ok && !c.stack_skip_last;
  }
  // an illumination source: the complex path of an f32 plan -- not the bit path, not the real-pair path -- and
  // no window, stack piece, plane cache, actions, walk, reconcile or env-major output.  The forward takes any
  // of the complex path's outputs (a pixel weight too: the last pass is the existing statistics form); the
  // adjoint has complex samples in and one output that is no statistics form, so no target and no pixel weight.
  // The real samples in a complex slot, and their threshold switch, only in the forward of a sourced call
  if (c.source) {
    ok = ok && !c.mask && !c.real_values && f32;
    ok = ok && !c.windowed && !pass_stack(c) && !planes && !c.actions && !walk && !c.rc_pending && !c.inten_by_env;
    if (c.source_adjoint)
      ok = ok && c.complex_values && !c.complex_stats && !c.target && !c.inten_out && !c.pixel_weight &&
           (c.complex_field != nullptr) + (c.real_part != nullptr) + (grad_out ? 1 : 0) == 1;
    else
      ok = ok && !c.complex_weight && !grad_out;
  }
  ok = ok && (c.source || (!c.source_adjoint && !c.source_real));
  ok = ok && (!c.source_real || !c.source_adjoint) && (c.source_real || !c.source_binarize);
  return ok ? hipSuccess : hipErrorInvalidValue;
}
// The target rows the last pass reads.  No target: the plan's zero row, every row offset masked to 0
struct PassTarget {
  const float* rows;
  size_t mask;
};
inline PassTarget pass_target(const PlanDev& pd, const PassCall& c) {
  return c.target ? PassTarget{c.target, ~(size_t)0} : PassTarget{pd.zero_row, (size_t)0};
}
// Whether k_reduce_partials runs behind the last pass.  Complex and phase samples: only the statistics
// form with a target left partials to reduce; otherwise unless the caller reduces them itself
inline bool pass_reduces(const PassCall& c) {
  return pass_complex(c) ? c.complex_stats && c.target : !c.skip_reduce;
}

constexpr int kPsfBlocks = 128;   // blocks per job of the incremental-field kernels
                                  // (measured 128 > 256 > 64 > 32, profiles/r01_psf_blocks_ab.txt)

struct EnvDev {
  uint64_t* mask;
  int8_t* record;
  const float* target;
  double* chan_stats;
  double* init_psnr;
  double* prev_psnr;
  double* max_psnr_diff;
  int64_t* steps;
  int64_t* flip_count;
  int64_t* sustained;
  const double* imp_changes;  // [B][imp_count] (importance rewards)
  const double* imp_values;
  const double* t_psnr_diff;  // [B] nullable
  int imp_count;
  int8_t* state_bytes;        // [B][CH][H][W] obs["state"] mirror of the mask bits (nullable, ABI v8)
  int32_t* recon_pending;     // [B] group the next step reconciles (nullable; with recon)
  int32_t* plane_slot;        // [B][CH + 2] plane-cache slots (nullable, ABI v9): an accepted step
                              // swaps the flipped pair's slots with the two spares
  const int32_t* error;       // the sticky error word (nullable)
  int32_t* error_host;        // its mirror, written by the env-step finalize (nullable, ABI v11)
};

struct EnvParams {
  int64_t max_steps;
  double t_psnr;
  int64_t t_steps;
  double t_psnr_diff;
  double reward_weight;
  int32_t accept_rule;
  int32_t reward_kind;  // 0 env.py, 1 env_group.py
};

// the three passes of one PassCall: check_pass_call, then the launches
hipError_t run_jobs(const PlanDev& pd, const PassCall& c, hipStream_t st);
// its N = 896 form (hbx_passes896.hip; run_jobs has checked the call)
hipError_t run_jobs_896(const PlanDev& pd, const PassCall& c, hipStream_t st);
// (extension, hbx_backward_stack) the depth-summing last pass: c names the jobs (n_jobs per depth) and the
// one output of a complex last pass -- complex_field, real_part, or grad_samples / grad_phase with their kind --
// and nothing else; depth d's column-pass output sits in job slots [d * slot_stride, d * slot_stride + n_jobs)
// of ws_b (the PassCalls with stack_skip_last and stack_slot0 = d * slot_stride put it there)
inline hipError_t check_stack_last(const PlanDev& pd, const PassCall& c, int n_depths, int slot_stride) {
  const bool grad_out = c.grad_samples || c.grad_phase;
  bool ok = pd.store_kind == HBX_PRECISION_F32 && n_depths >= 1 && n_depths <= HBX_MAX_DEPTHS;
  ok = ok && c.n_jobs >= 1 && slot_stride >= c.n_jobs;
  ok = ok && !c.mask && !c.real_values && !c.complex_values && !c.phase_values && !c.complex_weight;
  ok = ok && (c.complex_field != nullptr) + (c.real_part != nullptr) + (grad_out ? 1 : 0) == 1;
  ok = ok && (!grad_out || (c.grad_samples && c.grad_phase));
  ok = ok && (c.grad_kind == kGradPhase ||
              (grad_out && (c.grad_kind == kGradSteWindow || (c.grad_kind == kGradSteSigmoid && c.grad_p1 > 0.0f))));
  ok = ok && (c.phase_levels == 0 || (c.phase_levels >= 2 && c.phase_levels <= 256 && grad_out && c.grad_kind == kGradPhase));
  ok = ok && !c.target && !c.inten_out && !c.field_out && !c.complex_stats && !c.windowed && !c.actions &&
       c.plane_mode == kPlanesOff && !c.walk_phase && !c.walk_planes && !c.rc_pending && !c.skip_reduce && !pass_stack(c);
  return ok ? hipSuccess : hipErrorInvalidValue;
}
hipError_t run_stack_last(const PlanDev& pd, const PassCall& c, int n_depths, int slot_stride, hipStream_t st);
hipError_t run_stack_last_896(const PlanDev& pd, const PassCall& c, int n_depths, int slot_stride, hipStream_t st);
// One kernel launch of `blocks` workgroups of `nt` threads: the caller picks the instantiation (a
// function pointer: every variant of a kernel family has one signature) and writes the arguments once
template <class K, class... A>
inline void launch_kernel(K k, unsigned blocks, unsigned nt, hipStream_t st, A... a) {
  hipLaunchKernelGGL(k, dim3(blocks), dim3(nt), 0, st, a...);
}

// The sample passes' kernel pick, once for both dispatchers (launch_passes, run_jobs_896).  F = the size
// family's kernels (SampleKernels<R>, SampleKernels896): first_real<LK, WIN>(), first_cplx<LK, WIN>() and
// last_cplx<ST, GK, WIN>() return the instantiation.  The unwindowed forms are named before the windowed
// ones, and within each in the order the code object has had them: first use fixes a kernel's place in it,
// and the timings on record were taken with that layout (tools/isa_cmp.py reports a reordering).  What check_pass_call refuses is never named: a windowed
// phase load, windowed statistics, a windowed phase gradient.
template <class F>
inline auto pick_first_pass_real(bool threshold, bool win_in) {
  auto k = !threshold ? F::template first_real<kLoadReal, false>() : F::template first_real<kLoadThreshold, false>();
  if (win_in) k = !threshold ? F::template first_real<kLoadReal, true>() : F::template first_real<kLoadThreshold, true>();
  return k;
}
template <class F>
inline auto pick_first_pass_cplx(int lk, bool win_in) {
  auto k = lk == kLoadComplex ? F::template first_cplx<kLoadComplex, false>()
           : lk == kLoadPhase ? F::template first_cplx<kLoadPhase, false>()
                              : F::template first_cplx<kLoadWeighted, false>();
  if (win_in)
    k = lk == kLoadWeighted ? F::template first_cplx<kLoadWeighted, true>() : F::template first_cplx<kLoadComplex, true>();
  // (the quantizing phase load, named last: it takes its place behind every kernel on record)
  if (lk == kLoadPhaseLevels) k = F::template first_cplx<kLoadPhaseLevels, false>();
  return k;
}
// gk = kGradNone: the plane itself, with the statistics or without (hbx_evaluate_complex); kGradPhase
// (hbx_phase_backward) and the two STE kinds (hbx_threshold_backward): the leaf's gradient instead;
// windowed: the real part or an STE gradient over out_win
template <class F>
inline auto pick_last_pass_cplx(int gk, bool stats, bool windowed) {
  auto k = gk == kGradNone          ? (stats ? F::template last_cplx<true, kGradNone, false>()
                                             : F::template last_cplx<false, kGradNone, false>())
           : gk == kGradSteWindow  ? F::template last_cplx<false, kGradSteWindow, false>()
           : gk == kGradSteSigmoid ? F::template last_cplx<false, kGradSteSigmoid, false>()
                                   : F::template last_cplx<false, kGradPhase, false>();
  if (windowed)
    k = gk == kGradSteWindow    ? F::template last_cplx<false, kGradSteWindow, true>()
        : gk == kGradSteSigmoid ? F::template last_cplx<false, kGradSteSigmoid, true>()
                                : F::template last_cplx<false, kGradNone, true>();
  // (the quantizing phase gradient, named last as the quantizing load is; never windowed)
  if (gk == kGradPhaseLevels) k = F::template last_cplx<false, kGradPhaseLevels, false>();
  return k;
}
// 2-D FFT of n_planes [N][N] complex planes in a (result in a; b is scratch of
// the same size).  Unnormalised both ways.
hipError_t run_fft2d(const PlanDev& pd, float2* a, float2* b, int n_planes, bool inverse,
                     hipStream_t st);
// flip map (hbx_map.hip): h-side spectra q [G][4][N][N] + sum |h|^4 per group,
// then one group's dPSNR map [P][N][N] into out + g*P*N*N
hipError_t map_prepare_h(const PlanDev& pd, float2* q, float2* scratch, double* part, double* d4,
                         hipStream_t st);
hipError_t map_group(const PlanDev& pd, int g, const float2* field, const float* inten,
                     const float* target, const uint64_t* mask, const double* stats, const float2* q,
                     const double* d4, float2* X, float2* S, float2* Y, float* out, double count, int rel,
                     double peak, hipStream_t st);
hipError_t launch_psf_eval(const PlanDev& pd, const JobDesc* jobs, int n_jobs, const uint64_t* mask,
                           const float2* field, const float* inten, const float* target,
                           const double* chan_stats, hipStream_t st, const int64_t* actions = nullptr,
                           int32_t* err = nullptr);
// device-resident greedy DBS walk (hbx_walk.hip)
struct WalkLaunch {
  uint64_t* mask;
  const float* target;
  double* base_stats;
  float2* field;
  float* inten;
  const int64_t* order;
  int64_t n_order;   // length of order: the walk never visits past min(walk->total, n_order)
  hbx_dbs_walk_t* walk;
  int64_t* log_pos;
  double* log_psnr;
  int64_t log_cap;
  double* partial;   // split batch: [K][walk_blocks_per_job(N, K)][2]; fused step: [blocks][terms]
  int* counter;      // fused step: walk scratch (kWalkScratchBytes): tickets, then WalkPre
  int fused;         // 1: one k_walk_step launch per batch when K has a fused variant
  int persist;       // 1 (with fused): one cooperative launch runs all `batches` (grid barrier per batch)
  int K, batches;
  double count, peak;
  int rel;
};
constexpr int kWalkMaxK = 256;
int walk_blocks_per_job(int N, int K);
int walk_step_blocks(int N);
bool walk_fused_k(int K);
constexpr int kWalkStepMaxTerms = 26;   // 2 K + 3 K (K-1) / 2 at K = 4: max over the fused variants
// fused-step scratch: int counters [kWalkCounters] (arrival tickets [0, kWalkTickets),
// zero between launches), then the WalkPre the deciding block leaves for the next launch
constexpr int kWalkCounters = 16;
constexpr int kWalkTickets = 9;
constexpr int kWalkGen = 12;             // persistent walk: generation word (bumped per decided batch)
constexpr int kWalkAbort = 13;           //   and the abort word (a grid barrier timed out)
constexpr unsigned kWalkSpinMax = 1u << 20;   // polls (each ~1-2 us) before a waiting block gives up
constexpr int kWalkPreMax = 4;          // the largest fused K
struct WalkPre {
  int64_t pos;              // valid for this walk position (-1: invalid; cleared per API call)
  const int64_t* order;     //   and this order array
  int32_t n;                // actions filled
  int32_t pad;
  int32_t ch[kWalkPreMax];   // order[pos + j] decoded: channel (-1: not a valid action) ...
  int32_t pix[kWalkPreMax];  //   ... and pixel
  float delta[kWalkPreMax];  // vb (1 - 2 bit) of each action's pixel before its flip
  float cdelta[2];           // the pending commits' vb (2 bit - 1) after their flips
};
constexpr size_t kWalkScratchBytes = kWalkCounters * sizeof(int) + sizeof(WalkPre);
hipError_t launch_walk(const PlanDev& pd, const WalkLaunch& l, hipStream_t st);
hipError_t launch_psf_commit(const PlanDev& pd, const JobDesc* jobs, int n_jobs, const uint64_t* mask,
                             float2* field, float* inten, const int32_t* accept_flag, hipStream_t st);
hipError_t launch_jobs_from_actions(const int64_t* actions, int n, int H, int W, int P, int CH,
                                    JobDesc* jobs, int32_t* err, hipStream_t st);
hipError_t launch_jobs_from_flips(const int64_t* flips, int K, int H, int W, int P, int CH,
                                  JobDesc* jobs, hipStream_t st);
hipError_t launch_job_from_flip_k(const int64_t* flips, const int32_t* k, int K, int H, int W, int P, int CH,
                                  JobDesc* jobs, int32_t* order, int32_t* accept, hipStream_t st);
hipError_t launch_jobs_full(const int32_t* env_ids, int n_ids, int G, JobDesc* jobs, hipStream_t st);
hipError_t launch_full_finalize(const JobDesc* jobs, const double* job_stats, int n_ids, int G,
                                double* chan_stats, double* psnr, double count, int rel, double peak,
                                const EnvDev& env, int reset, hipStream_t st);
hipError_t launch_env_step_finalize(const JobDesc* jobs, const double* job_stats, int n, int G,
                                    int P, int H, int W, const EnvDev& env, const EnvParams& prm,
                                    double count, int rel, double peak, double* reward, double* psnr,
                                    uint8_t* acc, uint8_t* term, uint8_t* trunc, int32_t* accept_flag,
                                    double* delta_scratch, hipStream_t st,
                                    const double* partial = nullptr, int RB = 0);
hipError_t launch_dbs_step_finalize(const JobDesc* jobs, const double* job_stats, int n, int G, int P,
                                    int H, int W, uint64_t* mask, double* chan_stats, double* prev,
                                    double* psnr, uint8_t* acc, int rule, double count, int rel,
                                    double peak, hipStream_t st);
hipError_t launch_eval_finalize(const JobDesc* jobs, const double* job_stats, int K, int G,
                                const double* base_stats, double* psnr, double* gstats, double count,
                                int rel, double peak, hipStream_t st);
hipError_t launch_commit_flip(uint64_t* mask, double* stats, double* prev, const int64_t* flips,
                              const double* psnr, const double* gstats, const int32_t* k, int K,
                              int G, int P, int H, int W, hipStream_t st, int32_t* plane_slot = nullptr);
hipError_t launch_zero_record(int8_t* record, const int32_t* env_ids, int n_ids, size_t per_env,
                              hipStream_t st);
hipError_t launch_scatter_intensity(const JobDesc* jobs, int n_jobs, const float* src, float* cache,
                                    int G, size_t hw, const int32_t* accept_flag, hipStream_t st);
hipError_t launch_psnr(const double* chan_stats, int n, int G, double* psnr, double count, int rel,
                       double peak, hipStream_t st);
// observation mirrors (ABI v8): reconcile the previous step's group between recon and
// intensity (recon_pending), and rebuild state_bytes / recon of listed envs
hipError_t launch_recon_reconcile(const int32_t* pending, float* recon, float* intensity, int n, int G,
                                  size_t hw, hipStream_t st);
// plane cache (ABI v9): slot[env][i] = i for the listed envs (env_ids nullable: 0 .. n_ids - 1)
hipError_t launch_walk_planes(const WalkPlanesArgs& a, int decide, hipStream_t st);
hipError_t launch_walk_planes_anneal(const WalkPlanesArgs& a, int decide, const double* slack, int64_t n_slack,
                                     hipStream_t st);
hipError_t launch_plane_slot_init(const int32_t* env_ids, int n_ids, int32_t* slot, int CHS, hipStream_t st);
hipError_t launch_obs_sync(const int32_t* env_ids, int n_ids, const uint64_t* mask, int8_t* state_bytes,
                           float* intensity, float* recon, int32_t* pending, int resolve, int CH, int G, size_t hw,
                           hipStream_t st);
hipError_t launch_obs_settle(const int32_t* env_ids, int n_ids, float* intensity, const float* recon,
                             int32_t* pending, int G, size_t hw, hipStream_t st);
// (ABI v14) hbx_pack.hip: mask values -> bits, and relativeLoss statistics
hipError_t launch_pack_mask(const void* src, int kind, int64_t n_words, int mode, double thr, uint64_t* bits,
                            int32_t* err, hipStream_t st);
// (ABI v15, additive) hbx_pack.hip: the phase quantizer's export, level[n] uint8 and / or q[n] f32 (nullable)
hipError_t launch_quantize_phase(const float* src, int64_t n, int levels, uint8_t* out_levels, float* out_phase,
                                 hipStream_t st);
// (extension, illumination fields) hbx_pack.hip: out[n_planes][hw] complex64 = source[g] * f(values), leaf
// kind sk (kSrc*) with source_sample's (p0, p1, p2); plane i belongs to group (i / Q) % G
hipError_t launch_source_field(const float* values, const float2* source, int sk, int64_t n_planes, int G, int Q,
                               size_t hw, float p0, float p1, float p2, float2* out, hipStream_t st);
int rel_partial_slots();
hipError_t launch_rel_stats(const void* x, const void* y, int kind, int64_t n, double count, int rel_scale,
                            double peak, double* part, double* out, hipStream_t st);
// (ABI v15, additive) hbx_pack.hip: chan_stats[n][G][3] -> loss[n] (kind HBX_LOSS_*), and the
// loss's gradient with respect to the intensity, weight[n][G][hw] = a_b I + c_b T
hipError_t launch_loss(const double* chan_stats, int n, int G, int kind, int rel_scale, double count, double peak,
                       double* loss, hipStream_t st);
hipError_t launch_loss_weight(const float* inten, const float* target, const double* chan_stats,
                              const double* grad_loss, int n, int G, size_t hw, int kind, int rel_scale, double count,
                              float* weight, hipStream_t st);
// (extension) hbx_pack.hip: the same over a focal stack -- chan_stats[D][n][G][3] -> loss[n], and
// weight[D][n][G][hw] from inten / target [D][n][G][hw]; an env's sums run over its D G channels, d outer
hipError_t launch_loss_stack(const double* chan_stats, int n, int G, int D, int kind, int rel_scale, double count,
                             double peak, double* loss, hipStream_t st);
hipError_t launch_loss_weight_stack(const float* inten, const float* target, const double* chan_stats,
                                    const double* grad_loss, int n, int G, int D, size_t hw, int kind, int rel_scale,
                                    double count, float* weight, hipStream_t st);
// (extension, per-pixel loss weights) hbx_pack.hip: weight_sum[n] = the sum of pixel_weight[D][n][G][hw] over an
// env's D G images (d outer, g inner), f64 in a fixed order, a chunk of n envs from env b0 at a time in K slices
// per env through n K doubles of scratch; then the loss and its gradient with weight_sum[b]
// in the place of the pixel count, weight[d][b] = pixel_weight[d][b] * (a_b I + c_b T).  D = 1: a single depth
hipError_t launch_pixel_weight_sum(const float* pixel_weight, int b0, int n, int n_total, int G, int D, size_t hw,
                                   double* part, int K, double* weight_sum, hipStream_t st);
hipError_t launch_loss_pw(const double* chan_stats, const double* weight_sum, int n, int G, int D, int kind,
                          int rel_scale, double peak, double* loss, hipStream_t st);
hipError_t launch_loss_weight_pw(const float* inten, const float* target, const float* pixel_weight,
                                 const double* chan_stats, const double* weight_sum, const double* grad_loss, int n,
                                 int G, int D, size_t hw, int kind, int rel_scale, float* weight, hipStream_t st);

}  // namespace hbx
