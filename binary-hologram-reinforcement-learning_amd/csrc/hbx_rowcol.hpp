// hbx_rowcol.hpp -- helpers shared by the row / column passes (hbx_passes.hip,
// hbx_passes896.hip): LDS tile swizzle, XCD-aware row-block order, the first pass's
// workgroup decode, twiddle staging and real- / complex-field row loads, buffer descriptors of
// wave-uniform planes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "hbx_fft.hpp"

namespace hbx {

// Position of element (line, r) in an LDS tile [line][GPB rows], r XOR-swizzled
// by a function of (line mod R) only: lane t of a group reading line t + R*j
// then addresses base_t + j*R*GPB (immediate offsets, no per-j address VGPRs),
// ds_read_b64 is conflict-free and ds_write_b64 at most 2-way (checked
// exhaustively for R = 8, 16, 32).
template <int R, int GPB = 256 / R>
__device__ __forceinline__ int tile_pos(int line, int r) {
  if constexpr (GPB == 16) {
    // 16 rows (512-thread blocks, N = 1024): swizzle (line mod 16) ^ bit 4 of
    // line -- conflict-free for the lane-row reads / writes and the 16-B chunk
    // writes; the chunk reads of k_rowfwd stay 2-way (checked exhaustively)
    return line * GPB + (r ^ (((line & 15) ^ ((line >> 4) & 1)) & (GPB - 1)));
  } else if constexpr (R == 32 && GPB == 8) {
    // q ^ 5 b1 (q = bits 2-4 of line, b1 = bit 1): the lane-row reads stay
    // conflict-free (bijective in q for fixed line mod 4) and the two b64
    // writes -- lane rows t + 32 k2 (16-lane groups: bijective in bits 1-3)
    // and the 16-B chunk pairs of 4 consecutive lines (the b1 term flips the
    // parity) -- lose their 2-way conflicts (tools/lds_swizzle_model.py)
    return line * GPB + (r ^ ((((line & 31) >> 2) ^ (((line >> 1) & 1) * 5)) & 7));
  } else {
    constexpr int SR = ilog2c(32 / GPB);
    constexpr int SL = ilog2c(GPB / 8);
    return line * GPB + (r ^ ((((line & (R - 1)) >> SR) << SL) & (GPB - 1)));
  }
}

// Field value of mask bit sh of word w for the row passes: va + vb * bit (hbx_api.hip's field
// kinds: amplitude 0 / 1, binary phase exp(i pi bit) = +-1).  The two kinds the plans use are
// built from the bit with two integer ops instead of extract + convert + fma (the same f32
// values bit for bit: fmaf(1, b, 0) = b, fmaf(-2, b, 1) = +-1.0f = 0x3F800000 with the sign
// bit b).  r06: k_rowfwd32 1,311 -> ~1,250 VALU and 168 -> 152 VGPRs per row block,
// 0.874-0.887 -> 0.852-0.873 ms alternated 4x on one box (profiles/r06/rowfwd_bitop_ab_r06o.txt).
enum { kFieldAmp = 0, kFieldPhase = 1, kFieldAny = 2 };
template <int FK>
__device__ __forceinline__ float bit_value(uint32_t w, int sh, float va, float vb) {
  if constexpr (FK == kFieldAmp) return (float)((w >> sh) & 1u);
  else if constexpr (FK == kFieldPhase) return __uint_as_float(((w << (31 - sh)) & 0x80000000u) | 0x3F800000u);
  else return fmaf(vb, (float)((w >> sh) & 1u), va);
}
// f(integral_constant<int, FK>) under a uniform branch on the plan's (va, vb)
template <class F>
__device__ __forceinline__ void with_field_kind(float va, float vb, F&& f) {
  if (va == 0.0f && vb == 1.0f) f(std::integral_constant<int, kFieldAmp>{});
  else if (va == 1.0f && vb == -2.0f) f(std::integral_constant<int, kFieldPhase>{});
  else f(std::integral_constant<int, kFieldAny>{});
}

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// buffer descriptor of a wave-uniform plane (cdna_hip_programming.md T8 recipe)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t plane_rsrc(const void* base, unsigned bytes) {
  const uint64_t a = reinterpret_cast<uint64_t>(base);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
  void* p = reinterpret_cast<void*>(((uint64_t)hi << 32) | lo);
  return __builtin_amdgcn_make_buffer_rsrc(p, (short)0, (int)bytes, 0x00020000);
}

__device__ __forceinline__ float2 buf_ld2(__amdgpu_buffer_rsrc_t rs, int voff, int soff) {
  return __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rs, voff, soff, 0));
}

__device__ __forceinline__ void buf_st2(float2 v, __amdgpu_buffer_rsrc_t rs, int voff, int soff) {
  __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), rs, voff, soff, 0);
}

// The once-touched intermediate streams: loads keep the default cache policy (non-temporal
// loads slowed k_rowinv 1.80 -> 2.21 ms, r01); the row spectrum A and the column output B are
// STORED non-temporal since r03 -- with B in slot tiles and A read by k_col2 right after,
// default-policy stores left their dirty lines in the Infinity Cache to be written back during
// the next pass (N = 1024 headline 24.9k -> 25.9k (B) -> 26.1k (A and B) on one box; N = 256
// k_rowinv 0.140 -> 0.100 ms).  (r01, before the tiles: nt A stores 1.17 -> 1.27 ms.)
__device__ __forceinline__ float2 buf_ld2s(__amdgpu_buffer_rsrc_t rs, int voff, int soff) {
  return __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rs, voff, soff, 0));
}
__device__ __forceinline__ void buf_st2s(float2 v, __amdgpu_buffer_rsrc_t rs, int voff, int soff) {
  __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), rs, voff, soff, 0);
}
__device__ __forceinline__ float4 ld_stream4(const float2* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st_stream4(float2* p, float4 v) {
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  __builtin_nontemporal_store(f32x4{v.x, v.y, v.z, v.w}, reinterpret_cast<f32x4*>(p));
}
// cache-policy bit of buffer instructions (gfx950 aux operand): nt = non-temporal
constexpr int kBufNT = 2;

// Workgroups b, b+8, b+16, ... land on the same XCD (round-robin dispatch over
// the 8 XCDs; placement is a speed hint only, never relied on for
// correctness).  The row passes touch 64-B pieces of every 8-KB line, the
// piece for rows y0..y0+7: keep GS consecutive row blocks on one XCD so each
// line is read / written as GS*64 contiguous bytes through one L2.  Measured
// on 1024x24, 128 envs (k_rowfwd / k_rowinv ms): no remap 1.34 / 2.75,
// GS=2 1.18 / 2.43, GS=4 1.17 / 2.40, GS=8 1.12 / 2.08, GS=16 1.12 / 1.98.
constexpr int kXcdGroup = 16;
template <int RB>
__device__ __forceinline__ int xcd_pair(int bid) {
  constexpr int GS = (RB / 8 < kXcdGroup) ? RB / 8 : kXcdGroup;
  constexpr int SPAN = 8 * (GS > 0 ? GS : 1);
  if constexpr (GS > 1 && RB % SPAN == 0)
    return (bid / SPAN) * SPAN + (bid % 8) * GS + (bid / 8) % GS;
  else return bid;
}

// Where a first-pass workgroup works.  bid counts [job j][plane pair q of npair][rbw of the RBW
// workgroups that share a plane pair], rbw fastest; the caller passes blockIdx.x, or
// xcd_pair<RB>(blockIdx.x) where a workgroup is one row block.  writer: the one workgroup of job j
// that records what the job decoded to (first_pass_job).
struct FirstPassBlock {
  int rbw, j, q;
  bool writer;
};
template <int RBW>
__device__ __forceinline__ FirstPassBlock first_pass_block(int bid, int npair) {
  const int rbw = bid % RBW;
  bid /= RBW;
  return {rbw, bid / npair, bid % npair, rbw == 0 && bid % npair == 0};
}

// the row FFT's twiddles into LDS (visible after the caller's next block barrier)
template <int N, int NT>
__device__ __forceinline__ void stage_twiddles(float2* tw, const float2* __restrict__ tw_glob) {
  for (int i = threadIdx.x; i < N; i += NT) tw[i] = tw_glob[i];
}

// Real-valued fields (hbx_simulate_real / hbx_propagate_real): lane t of a row's group loads pixel
// x = t + R jj, jj < L, of the row at rowa and of the same row one plane further straight into the
// (re, im) of v[jj] -- one coalesced 4 R-byte run per lane group and jj, read once (non-temporal);
// v[L ..] = 0 (N = 896: L = 28 of the 32 slots, as the bit kernel).
template <int R, int L = R, class V>
__device__ __forceinline__ void real_load_row(V (&v)[R], const float* __restrict__ rowa, size_t plane, int t) {
  const float* rowb = rowa + plane;
  float a[L], b[L];
#pragma unroll
  for (int jj = 0; jj < L; ++jj) a[jj] = __builtin_nontemporal_load(rowa + t + R * jj);
#pragma unroll
  for (int jj = 0; jj < L; ++jj) b[jj] = __builtin_nontemporal_load(rowb + t + R * jj);
#pragma unroll
  for (int jj = 0; jj < L; ++jj) v[jj] = V{a[jj], b[jj]};
#pragma unroll
  for (int jj = L; jj < R; ++jj) v[jj] = V{0.f, 0.f};
}

// Binary holograms from a real leaf (hbx_evaluate_threshold): real_load_row's loads, in its order and
// all issued before the first use, then each sample x becomes the field of its mask bit [x >= thr]:
// hi = va + vb where the bit is set, lo = va where it is not -- NaN compares false and gives lo, as
// HBX_PACK_THRESHOLD packs it.  v[L ..] = 0, not lo (N = 896: the padding is no sample).  The tail
// then sees real_load_row's row of the materialised 0 / 1 (or 1 / -1) samples, which are never written.
template <int R, int L = R, class V>
__device__ __forceinline__ void threshold_load_row(V (&v)[R], const float* __restrict__ rowa, size_t plane, int t,
                                                   float thr, float lo, float hi) {
  const float* rowb = rowa + plane;
  float a[L], b[L];
#pragma unroll
  for (int jj = 0; jj < L; ++jj) a[jj] = __builtin_nontemporal_load(rowa + t + R * jj);
#pragma unroll
  for (int jj = 0; jj < L; ++jj) b[jj] = __builtin_nontemporal_load(rowb + t + R * jj);
#pragma unroll
  for (int jj = 0; jj < L; ++jj) v[jj] = V{a[jj] >= thr ? hi : lo, b[jj] >= thr ? hi : lo};
#pragma unroll
  for (int jj = L; jj < R; ++jj) v[jj] = V{0.f, 0.f};
}

// Complex fields (hbx_simulate_complex): lane t loads the complex64 sample of pixel x = t + R jj,
// jj < L, of the row at `row` straight into the (re, im) of v[jj] -- one 8-byte non-temporal load
// per element, a coalesced 8 R-byte run per lane group and jj; v[L ..] = 0 (N = 896).  The row FFT
// of u = a + i b followed by the Hermitian split is then the real path's pair of planes (a, b).
template <int R, int L = R, class V>
__device__ __forceinline__ void complex_load_row(V (&v)[R], const float2* __restrict__ row, int t) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const f32x2* r2 = reinterpret_cast<const f32x2*>(row);
#pragma unroll
  for (int jj = 0; jj < L; ++jj) {
    const f32x2 s = __builtin_nontemporal_load(r2 + t + R * jj);
    v[jj] = V{s.x, s.y};
  }
#pragma unroll
  for (int jj = L; jj < R; ++jj) v[jj] = V{0.f, 0.f};
}

// Weighted complex fields (hbx_simulate_complex_weighted): complex_load_row's samples times the
// real image scale * wrow[x], wrow = the [N] f32 weight row of the plane's colour group.  All L
// sample loads and all L weight loads are issued before the first use (as real_load_row's two
// planes); the samples are read once (non-temporal), the weight row is re-read by every complex
// plane of its group and keeps the default cache policy.  Three f32 multiplies per sample, in this
// order and never contracted (there is nothing to add): m = scale * w, re * m, im * m.
template <int R, int L = R, class V>
__device__ __forceinline__ void complex_load_row_weighted(V (&v)[R], const float2* __restrict__ row,
                                                          const float* __restrict__ wrow, float scale, int t) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const f32x2* r2 = reinterpret_cast<const f32x2*>(row);
  f32x2 s[L];
  float w[L];
#pragma unroll
  for (int jj = 0; jj < L; ++jj) s[jj] = __builtin_nontemporal_load(r2 + t + R * jj);
#pragma unroll
  for (int jj = 0; jj < L; ++jj) w[jj] = wrow[t + R * jj];
#pragma unroll
  for (int jj = 0; jj < L; ++jj) {
    const float m = scale * w[jj];
    v[jj] = V{s[jj].x * m, s[jj].y * m};
  }
#pragma unroll
  for (int jj = L; jj < R; ++jj) v[jj] = V{0.f, 0.f};
}

// Phase holograms (hbx_simulate_phase): u = exp(i pi x) from the float32 sample x.  sincospif reduces
// the argument exactly (x mod 2 has no rounding in float32, unlike x * float32(pi)), so the error of
// (c, s) does not grow with |x|: an unwrapped phase of thousands of turns is as good as a wrapped one.
// The hardware sine / cosine on fract(x / 2) (their input is in revolutions) met the same accuracy
// criteria and measured no shorter first pass, so the correctly reduced library form stays.
__device__ __forceinline__ void phase_sincos(float x, float& c, float& s) { sincospif(x, &s, &c); }

// Lane t loads the float32 phase sample of pixel x = t + R jj, jj < L, of the row at `row` -- one
// 4-byte non-temporal load per element, a coalesced 4 R-byte run per lane group and jj, all L issued
// before the first use (as real_load_row) -- and v[jj] = (cos pi x, sin pi x); v[L ..] = 0, not
// exp(0) (N = 896: the padding is no sample).  The tail then sees complex_load_row's row.
//   LK = kLoadPhaseLevels (hbx_simulate_phase_levels): each sample goes through the quantizer
//   (quantize_phase_sample, hbx_internal.hpp; qh, qs = its h and s, unused otherwise) between the load and
//   the sincos -- a few VALU instructions per sample, and the tail sees phase_load_row's row of the
//   materialised q, which is never written
template <int R, int L = R, int LK = kLoadPhase, class V>
__device__ __forceinline__ void phase_load_row(V (&v)[R], const float* __restrict__ row, int t, float qh = 0.0f,
                                               float qs = 0.0f) {
  static_assert(LK == kLoadPhase || LK == kLoadPhaseLevels, "a phase load kind");
  float a[L];
#pragma unroll
  for (int jj = 0; jj < L; ++jj) a[jj] = __builtin_nontemporal_load(row + t + R * jj);
#pragma unroll
  for (int jj = 0; jj < L; ++jj) {
    float c, s;
    if constexpr (LK == kLoadPhaseLevels) a[jj] = quantize_phase_sample(a[jj], qh, qs);
    phase_sincos(a[jj], c, s);
    v[jj] = V{c, s};
  }
#pragma unroll
  for (int jj = L; jj < R; ++jj) v[jj] = V{0.f, 0.f};
}

// The last pass of a phase leaf's backward (hbx_phase_backward): g = the inverse row FFT's output
// (natural layout, pixel x = t + R k of the row), u = exp(i pi x) the leaf's field, du/dx = i pi u, so
//   dL/dx = Re(conj(du/dx) g) = pi (Im g cos pi x - Re g sin pi x),
// one float32 per pixel to g0[R k]; g0 / p0 = the lane's pixel x = t of the gradient row and of the
// same row of the phase samples (read once, non-temporal, behind the FFT: no sample is live across
// it -- at N = 256, where the registers are there, loading them ahead of the FFT measured no faster,
// DESIGN.md 4q).  phase_load_row's sincos.
//   GK = kGradPhaseLevels (hbx_phase_levels_backward): the samples go through phase_load_row's quantizer
//   (qh, qs) first, so the gradient is the same expression at the displayed phase q(x) -- the
//   straight-through estimator dq/dx := 1
template <int R, int L, int GK = kGradPhase, class V, int NV>
__device__ __forceinline__ void phase_grad_row(const V (&v)[NV], const float* __restrict__ p0,
                                               float* __restrict__ g0, float qh = 0.0f, float qs = 0.0f) {
  static_assert(GK == kGradPhase || GK == kGradPhaseLevels, "a phase gradient kind");
  constexpr float kPiF = 3.14159265358979323846f;
  float a[L];
#pragma unroll
  for (int k = 0; k < L; ++k) a[k] = __builtin_nontemporal_load(p0 + R * k);
#pragma unroll
  for (int k = 0; k < L; ++k) {
    float c, s;
    if constexpr (GK == kGradPhaseLevels) a[k] = quantize_phase_sample(a[k], qh, qs);
    phase_sincos(a[k], c, s);
    g0[R * k] = kPiF * fmaf(v[k].y, c, -(v[k].x * s));
  }
}

// The last pass of a binary hologram's backward (hbx_threshold_backward): the leaf x is real, its
// field u = va + vb [x >= thr], g = the inverse row FFT's output = dL/du, and the straight-through
// estimator hands Re g to x through a surrogate derivative s(x) of the step:
//   dL/dx = vb s(x) Re g,
// one float32 per pixel to g0[R k] from the samples at p0 (phase_grad_row's geometry and loads: read
// once, non-temporal, behind the FFT).
//   kGradSteWindow  (a = lo, b = hi): s = 1 on lo <= x <= hi, else 0 -- a select, so a closed gate
//                   stores +0.0f whatever g holds (inf, NaN), and a NaN sample closes it
//   kGradSteSigmoid (a = thr, b = k > 0): s = k sg (1 - sg), sg = 1 / (1 + exp(-k (x - thr))), formed
//                   as k e / (1 + e)^2 with e = exp(-|k (x - thr)|) <= 1: the same value without the
//                   cancellation in 1 - sg, and no overflow for any x
template <int R, int L, int GK, class V, int NV>
__device__ __forceinline__ void ste_grad_row(const V (&v)[NV], const float* __restrict__ p0, float* __restrict__ g0,
                                             float vb, float a, float b) {
  static_assert(GK == kGradSteWindow || GK == kGradSteSigmoid, "a surrogate kind");
  float x[L];
#pragma unroll
  for (int k = 0; k < L; ++k) x[k] = __builtin_nontemporal_load(p0 + R * k);
#pragma unroll
  for (int k = 0; k < L; ++k) {
    if constexpr (GK == kGradSteWindow) {
      g0[R * k] = (x[k] >= a && x[k] <= b) ? vb * v[k].x : 0.0f;
    } else {
      const float e = expf(-fabsf(b * (x[k] - a)));
      const float d = 1.0f + e;
      g0[R * k] = vb * (b * e / (d * d)) * v[k].x;
    }
  }
}

// ---------------------------------------------------------------------------
// Illumination fields (hbx_source_field / hbx_evaluate_source / hbx_backward_source): the modulator is lit
// by a complex source s = (sr, si), source[G][N][N] complex64, and the field is u = s f with f the leaf
// kind's unsourced sample.  Every product is rounded on its own -- the bodies below are compiled with
// contraction off, so the one fma each formula names is the only one, and no multiply of theirs fuses
// with an add of the row FFT behind it: the first pass and the materialiser (k_source_field) then form
// the same float32 u, and hbx_evaluate_source equals hbx_evaluate_complex on hbx_source_field's output
// bit for bit.
//   u.re = fmaf(fr, sr, -(fi * si))     u.im = fmaf(fr, si, fi * sr)
__device__ __forceinline__ void source_mul(float fr, float fi, float sr, float si, float& ur, float& ui) {
#pragma clang fp contract(off)
  const float a = fi * si, b = fi * sr;
  ur = __builtin_fmaf(fr, sr, -a);
  ui = __builtin_fmaf(fr, si, b);
}
// the two real kinds: fi is absent, not 0 -- one multiply each
__device__ __forceinline__ void source_mul_real(float fr, float sr, float si, float& ur, float& ui) {
#pragma clang fp contract(off)
  ur = fr * sr;
  ui = fr * si;
}
// the adjoint: g' = conj(s) g,  g'.re = fmaf(g.re, sr, g.im * si)   g'.im = fmaf(g.im, sr, -(g.re * si))
__device__ __forceinline__ void source_mul_conj(float gr, float gi, float sr, float si, float& pr, float& pi) {
#pragma clang fp contract(off)
  const float a = gi * si, b = gr * si;
  pr = __builtin_fmaf(gr, sr, a);
  pi = __builtin_fmaf(gi, sr, -b);
}

// u = s f(x) of one sample, the leaf kind's map and the product (SK: kSrc*, hbx_internal.hpp).  (a, b) =
// the complex sample, or a = the float32 sample x and b unread.  (p0, p1, p2): kSrcPhaseLevels the
// quantizer's (h, s) (quantize_phase_sample); kSrcThreshold (thr, lo, hi), lo = va and hi = va + vb of the
// plan, NaN compares false and gives lo as threshold_load_row has it; unread by the other kinds
template <int SK>
__device__ __forceinline__ void source_sample(float a, float b, float sr, float si, float p0, float p1, float p2,
                                              float& ur, float& ui) {
  if constexpr (SK == kSrcComplex) {
    source_mul(a, b, sr, si, ur, ui);
  } else if constexpr (SK == kSrcPhase || SK == kSrcPhaseLevels) {
    float c, s;
    if constexpr (SK == kSrcPhaseLevels) a = quantize_phase_sample(a, p0, p1);
    phase_sincos(a, c, s);
    source_mul(c, s, sr, si, ur, ui);
  } else if constexpr (SK == kSrcThreshold) {
    source_mul_real(a >= p0 ? p2 : p1, sr, si, ur, ui);
  } else {
    static_assert(SK == kSrcReal, "a source leaf kind");
    source_mul_real(a, sr, si, ur, ui);
  }
}

// The sourced first-pass load: lane t loads the sample of pixel x = t + R jj, jj < L, of the leaf's row
// (`row`: complex64 pairs for kSrcComplex, float32 otherwise; read once, non-temporal) and the source
// sample of the same pixel (srow: the row of the group's source, re-read by every env and plane of the
// group, default cache policy as the weight row of complex_load_row_weighted), and v[jj] = s f.  The
// loads of C pixels -- samples, then source -- are all issued before the first use; C = L is the whole
// row, C = L / 2 loads and multiplies in halves (N = 1024: DESIGN.md has the register account).
// v[L ..] = 0 (N = 896: the padding is no sample and gets no light).
template <int R, int L, int SK, int C, class V>
__device__ __forceinline__ void source_load_row(V (&v)[R], const float* __restrict__ row,
                                                const float2* __restrict__ srow, int t, float p0, float p1,
                                                float p2) {
  static_assert(L % C == 0, "whole pieces");
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const f32x2* r2 = reinterpret_cast<const f32x2*>(row);
  const f32x2* s2 = reinterpret_cast<const f32x2*>(srow);
#pragma unroll
  for (int j0 = 0; j0 < L; j0 += C) {
    f32x2 a[C], s[C];
#pragma unroll
    for (int jj = 0; jj < C; ++jj) {
      if constexpr (SK == kSrcComplex) a[jj] = __builtin_nontemporal_load(r2 + t + R * (j0 + jj));
      else a[jj] = f32x2{__builtin_nontemporal_load(row + t + R * (j0 + jj)), 0.0f};
    }
#pragma unroll
    for (int jj = 0; jj < C; ++jj) s[jj] = s2[t + R * (j0 + jj)];
#pragma unroll
    for (int jj = 0; jj < C; ++jj) {
      float ur, ui;
      source_sample<SK>(a[jj].x, a[jj].y, s[jj].x, s[jj].y, p0, p1, p2, ur, ui);
      v[j0 + jj] = V{ur, ui};
    }
  }
#pragma unroll
  for (int jj = L; jj < R; ++jj) v[jj] = V{0.f, 0.f};
}

// The row load of the sourced first passes, once for every size (N = R L): complex plane q of the job's
// group of values [env][CH / 2][N][N] -- complex64 for kSrcComplex, float32 otherwise -- times row y of
// source[group].  The addresses are formed as first_pass_load_cplx forms them.
template <int R, int L, int SK, int C, class V>
__device__ __forceinline__ void first_pass_load_src(V (&v)[R], const float* values, const float2* source, int env,
                                                    int group, int P, int CH, int q, int y, int t, float p0,
                                                    float p1, float p2) {
  constexpr int N = R * L;
  const size_t row = (((size_t)env * (CH / 2) + group * (P / 2) + q) * N + y) * N;
  const size_t srow = ((size_t)group * N + y) * N;
  source_load_row<R, L, SK, C>(v, values + row * (SK == kSrcComplex ? 2 : 1), source + srow, t, p0, p1, p2);
}

// The sourced last passes: g' = conj(s) g on the plane in registers, behind the inverse row FFT and in
// front of cplx_plane_out (v: natural layout, x = t + R k).  s0 = the lane's pixel x = t of the source row;
// the source loads are issued behind the FFT, as phase_grad_row issues its samples: no source sample is live
// across it.  C of the L pixels are in flight at a time: C = L issues the whole row's loads together; the
// N = 64 last pass, whose registers also hold the next pair's tiles, takes them in pieces (kSrc8Piece).
template <int R, int L, int C = L, class V, int NV>
__device__ __forceinline__ void source_conj_row(V (&v)[NV], const float2* __restrict__ s0) {
  static_assert(L % C == 0, "whole pieces");
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const f32x2* s2 = reinterpret_cast<const f32x2*>(s0);
#pragma unroll
  for (int k0 = 0; k0 < L; k0 += C) {
    f32x2 s[C];
#pragma unroll
    for (int k = 0; k < C; ++k) s[k] = s2[R * (k0 + k)];
#pragma unroll
    for (int k = 0; k < C; ++k) {
      float pr, pi;
      source_mul_conj(v[k0 + k].x, v[k0 + k].y, s[k].x, s[k].y, pr, pi);
      v[k0 + k] = V{pr, pi};
    }
  }
}

// ---------------------------------------------------------------------------
// Windows (hbx_*_window): an array that belongs to a window of the grid is compact, [..][h][w] with
// row pitch w, and the row passes reach it through a predicate on their per-element loads and stores.
// WinRow is row y of such an array as lane t sees it: whether the row is inside, and for pixel
// x = t + R k its index x - x0 in the compact row -- unsigned, so one compare tells 0 <= x - x0 < w.
struct WinRow {
  bool in;        // y0 <= y < y0 + h: no load or store of any lane otherwise
  unsigned w;
  int xo;         // t - x0
  __device__ __forceinline__ WinRow(const hbx_window_t& win, int y, int t)
      : in((unsigned)(y - win.y0) < (unsigned)win.h), w((unsigned)win.w), xo(t - win.x0) {}
  __device__ __forceinline__ bool has(int xk) const { return in && (unsigned)(xo + xk) < w; }
  // element offset of row y of plane `plane` of a compact [planes][h][w] array
  __device__ __forceinline__ static size_t row_of(const hbx_window_t& win, size_t plane, int y) {
    return (plane * (size_t)win.h + (size_t)(y - win.y0)) * (size_t)win.w;
  }
};

// real_load_row / threshold_load_row (LK) on a hologram zero-filled into the grid: rowa = the compact
// row of plane pa (dereferenced only where wr.has), the same row of plane pb one compact plane further.
// A pixel outside the window is 0 -- no light, not the field `lo` of an unset bit -- and issues no load.
template <int R, int L, int LK, class V>
__device__ __forceinline__ void real_load_row_win(V (&v)[R], const float* __restrict__ rowa, size_t plane,
                                                  const WinRow& wr, float thr, float lo, float hi) {
  const float* rowb = rowa + plane;
  float a[L], b[L];
#pragma unroll
  for (int jj = 0; jj < L; ++jj) a[jj] = wr.has(R * jj) ? __builtin_nontemporal_load(rowa + wr.xo + R * jj) : 0.0f;
#pragma unroll
  for (int jj = 0; jj < L; ++jj) b[jj] = wr.has(R * jj) ? __builtin_nontemporal_load(rowb + wr.xo + R * jj) : 0.0f;
#pragma unroll
  for (int jj = 0; jj < L; ++jj) {
    if constexpr (LK == kLoadThreshold)
      v[jj] = wr.has(R * jj) ? V{a[jj] >= thr ? hi : lo, b[jj] >= thr ? hi : lo} : V{0.f, 0.f};
    else
      v[jj] = V{a[jj], b[jj]};
  }
#pragma unroll
  for (int jj = L; jj < R; ++jj) v[jj] = V{0.f, 0.f};
}

// complex_load_row / complex_load_row_weighted (LK) on compact rows embedded at the window: row and wrow
// = the compact rows of the samples and of the group's weight (the same window); the weighted form's
// three multiplies, in its order.  0 outside the window, and no load there.
template <int R, int L, int LK, class V>
__device__ __forceinline__ void complex_load_row_win(V (&v)[R], const float2* __restrict__ row,
                                                     const float* __restrict__ wrow, float scale, const WinRow& wr) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const f32x2* r2 = reinterpret_cast<const f32x2*>(row);
  f32x2 s[L];
#pragma unroll
  for (int jj = 0; jj < L; ++jj)
    s[jj] = wr.has(R * jj) ? __builtin_nontemporal_load(r2 + wr.xo + R * jj) : f32x2{0.f, 0.f};
  if constexpr (LK == kLoadWeighted) {
    float w[L];
#pragma unroll
    for (int jj = 0; jj < L; ++jj) w[jj] = wr.has(R * jj) ? wrow[wr.xo + R * jj] : 0.0f;
#pragma unroll
    for (int jj = 0; jj < L; ++jj) {
      const float m = scale * w[jj];
      v[jj] = wr.has(R * jj) ? V{s[jj].x * m, s[jj].y * m} : V{0.f, 0.f};
    }
  } else {
#pragma unroll
    for (int jj = 0; jj < L; ++jj) v[jj] = V{s[jj].x, s[jj].y};
  }
#pragma unroll
  for (int jj = L; jj < R; ++jj) v[jj] = V{0.f, 0.f};
}

// ---------------------------------------------------------------------------
// The sample first passes' row load, once for every size (N = R L; k_rowfwd_real / _cplx, their
// N = 1024 and N = 896 forms): row y of the job's plane into v, up to the barrier that publishes the
// twiddles.  (env, group) = the job's; they, P, CH and the plane index arrive as scalars and the window
// by reference, and the addresses are formed here in this order: handed over as a whole JobDesc, as
// ready size_t indices or with the window by value, the kernels compiled to other code.
//
// Real fields: values[env][CH][N][N] f32, planes pa and pa + 1 of the job's group into (re, im).
//   LK = kLoadReal       the samples as they are (real_load_row)
//   LK = kLoadThreshold  (hbx_evaluate_threshold) each sample becomes the field of its mask bit, hi where
//                        x >= thr and lo elsewhere, as it is loaded; thr / lo / hi are unused otherwise
//   WIN  (hbx_evaluate_real_window / _threshold_window) values is compact, [env][CH][win.h][win.w], and
//        sits at win of the grid, which is 0 elsewhere: real_load_row_win loads a pixel only inside
template <int R, int L, int LK, bool WIN, class V>
__device__ __forceinline__ void first_pass_load_real(V (&v)[R], const float* values, int env, int group,
                                                     int P, int CH, int pa, int y, int t, float thr, float lo,
                                                     float hi, const hbx_window_t& win) {
  constexpr int N = R * L;
  if constexpr (WIN) {
    const WinRow wr(win, y, t);
    const size_t ro = wr.in ? WinRow::row_of(win, (size_t)env * CH + group * P + pa, y) : 0;
    real_load_row_win<R, L, LK>(v, values + ro, (size_t)win.h * win.w, wr, thr, lo, hi);
  } else {
    const float* row = values + (((size_t)env * CH + group * P + pa) * N + y) * N;
    if constexpr (LK == kLoadThreshold)
      threshold_load_row<R, L>(v, row, (size_t)N * N, t, thr, lo, hi);
    else
      real_load_row<R, L>(v, row, (size_t)N * N, t);
  }
}

// Complex fields: values[env][CH / 2][N][N] complex64, complex plane q of the job's group as it is.
//   LK = kLoadComplex   (hbx_simulate_complex) complex_load_row
//   LK = kLoadWeighted  (hbx_simulate_complex_weighted) times scale * weight[env][group][y][x] as it is
//                       loaded -- L more VGPRs live across the load; weight / scale are unused otherwise
//   LK = kLoadPhase     (hbx_simulate_phase) phase[env][CH / 2][N][N] f32 instead of values, exp(i pi x)
//                       formed on load -- L floats live where the complex form holds L pairs; phase is
//                       unused by the other kinds
//   LK = kLoadPhaseLevels  (hbx_simulate_phase_levels) kLoadPhase on the quantized samples: the quantizer's
//                       h arrives in scale and the bits of its s in win.y0, both unread by kLoadPhase
//                       (pass_first_scale / pass_first_window, hbx_internal.hpp)
//   WIN  (hbx_backward_window; kLoadComplex and kLoadWeighted) values [env][CH / 2][win.h][win.w] and
//        weight [env][G][win.h][win.w] are compact and sit at win of the grid, 0 elsewhere
template <int R, int L, int LK, bool WIN, class V>
__device__ __forceinline__ void first_pass_load_cplx(V (&v)[R], const float2* values,
                                                     const float* weight, float scale,
                                                     const float* phase, int env, int group, int P,
                                                     int CH, int q, int y, int t, const hbx_window_t& win) {
  constexpr int N = R * L;
  if constexpr (WIN) {
    static_assert(LK != kLoadPhase && LK != kLoadPhaseLevels, "phase leaves are not windowed");
    const WinRow wr(win, y, t);
    const size_t ro = wr.in ? WinRow::row_of(win, (size_t)env * (CH / 2) + group * (P / 2) + q, y) : 0;
    const size_t wo = wr.in ? WinRow::row_of(win, (size_t)env * (CH / P) + group, y) : 0;
    complex_load_row_win<R, L, LK>(v, values + ro, LK == kLoadWeighted ? weight + wo : nullptr, scale, wr);
  } else {
    const size_t row = (((size_t)env * (CH / 2) + group * (P / 2) + q) * N + y) * N;
    if constexpr (LK == kLoadWeighted)
      complex_load_row_weighted<R, L>(v, values + row, weight + (((size_t)env * (CH / P) + group) * N + y) * N, scale, t);
    else if constexpr (LK == kLoadPhase)
      phase_load_row<R, L>(v, phase + row, t);
    else if constexpr (LK == kLoadPhaseLevels)
      phase_load_row<R, L, kLoadPhaseLevels>(v, phase + row, t, scale, __int_as_float(win.y0));
    else
      complex_load_row<R, L>(v, values + row, t);
  }
}

// The complex last passes' stores over an output window: g0 / p0 = the compact rows of the output and
// of the leaf's samples (dereferenced only where wr.has).  GK = kGradNone: the real part of the plane
// (the gradient of a real leaf); the two STE kinds: ste_grad_row's expressions on the pixels inside.
template <int R, int L, int GK, class V, int NV>
__device__ __forceinline__ void grad_row_win(const V (&v)[NV], const float* __restrict__ p0, float* __restrict__ g0,
                                             const WinRow& wr, float vb, float a, float b) {
  static_assert(GK == kGradNone || GK == kGradSteWindow || GK == kGradSteSigmoid, "real part or a surrogate kind");
  if constexpr (GK == kGradNone) {
#pragma unroll
    for (int k = 0; k < L; ++k)
      if (wr.has(R * k)) g0[wr.xo + R * k] = v[k].x;
  } else {
    float x[L];
#pragma unroll
    for (int k = 0; k < L; ++k) x[k] = wr.has(R * k) ? __builtin_nontemporal_load(p0 + wr.xo + R * k) : 0.0f;
#pragma unroll
    for (int k = 0; k < L; ++k) {
      if (!wr.has(R * k)) continue;
      if constexpr (GK == kGradSteWindow) {
        g0[wr.xo + R * k] = (x[k] >= a && x[k] <= b) ? vb * v[k].x : 0.0f;
      } else {
        const float e = expf(-fabsf(b * (x[k] - a)));
        const float d = 1.0f + e;
        g0[wr.xo + R * k] = vb * (b * e / (d * d)) * v[k].x;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Staged slot-tile stores of the column passes (k_col2 at N = 1024 / 256, k_col896 since r04):
// the output line sets of a block (TL lines: group g = slot g of slot tile st, TileB) go out
// through the groups' FFT scratch regions.  The writer puts row y of its line at col2_pos(g / 2,
// y) of its OWN region (no block barrier); after a block barrier col2_stage_store stores the set
// as 16-B chunks (slots 2 sp, 2 sp + 1 from regions 2 sp, 2 sp + 1) in memory order -- one
// contiguous run per 16-row band.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

template <int R>
constexpr int col2_region_stride() { return R * (R + 1) > R * R + 32 ? R * (R + 1) : R * R + 32; }
template <int R>
__device__ __forceinline__ float2* col2_region(float2* scratch, int g) {
  return scratch + g * col2_region_stride<R>();
}
// Where row y of slot pair sp's regions sits.  The readers (col2_stage_store) load the rows
// y0 = band * 16 + (tid / NSP) % 16 of the NSP = TL / 2 slot pairs sp = tid % NSP; gfx950 serves
// the compiler's ds_read2(st64)_b64 as 16-lane groups over 32 banks (16 float2: NSP pairs x
// 16 / NSP rows) and a ds_read_b64 as 32-lane groups over 64 banks (NSP pairs x 32 / NSP rows).
// A constant shift per pair cannot serve both (r03's (sp * 64 / TL) was the 64-bank one; the
// compiler emits read2st64, and rocprofv3 counted 67.1 M SQ_LDS_BANK_CONFLICT cycles per 128-job
// k_col2 launch = 8 extra cycles on each of the 32 stage reads per wave and line).  Shift sp by
// 32 / TL float2 and flip row bit 4 (+16 banks) when row bit HB (the bit splitting a 32-lane
// group's rows in halves) is set, except for the last pair: conflict-free in both models, and
// the writers' 16-lane runs of consecutive rows stay conflict-free (tools/lds_swizzle_model.py
// checks all three; found by exhaustive search over this family).
template <int R>
__device__ __forceinline__ int col2_pos(int sp, int y) {
  constexpr int TL = 256 / R, NSP = TL / 2, HB = ilog2c(16 / NSP);
  return sp * (32 / TL) + (y ^ ((((y >> HB) & 1) && sp != NSP - 1) ? 16 : 0));
}

template <int R, int N = R * R>
__device__ __forceinline__ void col2_stage_store(const float2* scratch, __amdgpu_buffer_rsrc_t rb, int st) {
  constexpr int TL = 256 / R, CH = N * TL / 2;   // 16-B chunks per line set (N = 896: R = 32's geometry)
  static_assert(CH % 256 == 0, "whole chunk rounds");
  // chunk c = tid + 256 i: band c / (8 TL) = tid / (8 TL) + (32 / TL) i, row (tid / (TL / 2)) % 16,
  // slot pair tid % (TL / 2); memory offset = lane part + i (32 / TL) 16 N + st 16 TL (soffset)
  const int tid = threadIdx.x, sp = tid % (TL / 2);
  const int band0 = tid / (8 * TL), r = (tid / (TL / 2)) % 16;
  const int y0 = band0 * 16 + r;
  // rows y0 + (32 / TL) 16 i differ from y0 in bits >= 5 only, so col2_pos moves with them
  static_assert((32 / TL) * 16 >= 32, "stage rows step past the swizzled bits");
  const float2* lo_r = col2_region<R>(const_cast<float2*>(scratch), 2 * sp) + col2_pos<R>(sp, y0);
  const float2* hi_r = col2_region<R>(const_cast<float2*>(scratch), 2 * sp + 1) + col2_pos<R>(sp, y0);
  const int voff = (band0 * 16 * N + r * TL + 2 * sp) * 8;
#pragma unroll
  for (int i = 0; i < CH / 256; ++i) {
    const float2 lo = lo_r[(32 / TL) * 16 * i];   // (rounded by col2_stage_write under SK)
    const float2 hi = hi_r[(32 / TL) * 16 * i];
    const u32x4 o = {__float_as_uint(lo.x), __float_as_uint(lo.y), __float_as_uint(hi.x), __float_as_uint(hi.y)};
    // non-temporal (nt): B streams out without taking Infinity-Cache residency, so its write-back
    // no longer lands on top of k_rowinv's reads (r03: N = 256 k_col2 0.143 -> 0.128 ms and
    // k_rowinv 0.140 -> 0.126; N = 1024 2.70 -> 2.66 and 1.474 -> 1.419).
    // soffset stays the literal 0, the whole offset rides in voffset: LLVM's gfx950 hazard
    // recognizer inserts the 2 wait states a VALU write of a >64-bit store's data VGPRs needs
    // only when the MUBUF soffset is not a register -- with an SGPR soffset (r03) it assumed no
    // hazard and scheduled such writes right behind the store, the cause of the r03 bf16
    // non-determinism and of the ITER = 1 wrong B rows (tools/hazard_scan.py
    // now rejects any wide buffer store with a register soffset)
    __builtin_amdgcn_raw_buffer_store_b128(o, rb, voff + (st * 16 * TL + i * (32 / TL) * 16 * N) * 8, 0, kBufNT);
  }
}

}  // namespace hbx
