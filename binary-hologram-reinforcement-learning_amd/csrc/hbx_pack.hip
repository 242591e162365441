// hbx_pack.hip -- the device side of the operator shim's per-call work (gfx950).
//
// k_pack_mask: mask values -> the bit-packed words every propagation reads (include/hbx.h
//   layout).  The reference builds its field from a float / int8 mask on every call
//   (env.py:120-123,170-171: `pre_model >= 0.5`, `torch.tensor(state, dtype=float32)`;
//   DBS_1024_24.py:326-327); here one streaming pass turns it into 1 bit per pixel.  Each wave
//   packs 4 words (256 values) per iteration: lane l loads values 4l .. 4l+3 with one vector
//   load (u32 / float4 / 2 x double2), four wave64 ballots give bit l of "value 4l + k is on"
//   for k = 0..3, and lane i < 4 interleaves the four 16-bit slices i of the ballots into word i
//   (word i bit 4j + k = ballot_k bit 16i + j).  HBM-bound: 1 / 4 / 8 bytes read and 1/8 byte
//   written per pixel.  The binary check of tt.simulate (a value not 0 or 1) is a ballot too:
//   one store of 1 into a caller word (device or host-mapped memory), no host sync.
// k_rel_partials / k_rel_final: tt.relativeLoss(x, y, tm.get_PSNR) (env.py:132,174;
//   DBS_1024_24.py:332) as sufficient statistics sum xy, sum x^2, sum y^2 in f64 (the products
//   formed in f64, as torch's x.double() * y.double()), a fixed-order two-stage reduction
//   (deterministic), then the same PSNR / MSE formula as the env kernels (psnr_from).
// k_loss / k_loss_weight: the same loss (env.py:131-132,174) per env from the statistics the last
//   pass left, and its gradient with respect to the intensity, weight = a_b I + c_b T: one
//   streaming pass, 8 bytes read and 4 written per pixel, no host wait (hbx_loss, hbx_loss_weight).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "hbx.h"
#include "hbx_internal.hpp"
#include "hbx_rowcol.hpp"

namespace hbx {

namespace {

// every 4th bit of a 64-bit word from a 16-bit value: bit j -> bit 4j
__device__ __forceinline__ uint64_t spread4(uint64_t x) {
  x &= 0xffffull;
  x = (x | (x << 24)) & 0x000000ff000000ffull;
  x = (x | (x << 12)) & 0x000f000f000f000full;
  x = (x | (x << 6)) & 0x0303030303030303ull;
  x = (x | (x << 3)) & 0x1111111111111111ull;
  return x;
}

// the four values 4l .. 4l+3 of one lane as floats / doubles + the binary check
struct Quad {
  bool on[4];
  bool bad;
};

template <int KIND>
__device__ __forceinline__ Quad load_quad(const void* __restrict__ src, int64_t q, int mode, double thr) {
  Quad r;
  r.bad = false;
  if constexpr (KIND == HBX_SRC_U8) {
    const uint32_t v = reinterpret_cast<const uint32_t*>(src)[q];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t b = (v >> (8 * k)) & 0xffu;
      r.on[k] = mode == HBX_PACK_THRESHOLD ? ((double)b >= thr) : (b != 0u);
    }
    r.bad = (v & 0xfefefefeu) != 0u;
  } else if constexpr (KIND == HBX_SRC_F32) {
    const float4 v = reinterpret_cast<const float4*>(src)[q];
    const float e[4] = {v.x, v.y, v.z, v.w};
    const float tf = (float)thr;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      r.on[k] = mode == HBX_PACK_THRESHOLD ? (e[k] >= tf) : (e[k] != 0.0f);
      r.bad |= !(e[k] == 0.0f || e[k] == 1.0f);
    }
  } else {
    const double2 a = reinterpret_cast<const double2*>(src)[2 * q];
    const double2 b = reinterpret_cast<const double2*>(src)[2 * q + 1];
    const double e[4] = {a.x, a.y, b.x, b.y};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      r.on[k] = mode == HBX_PACK_THRESHOLD ? (e[k] >= thr) : (e[k] != 0.0);
      r.bad |= !(e[k] == 0.0 || e[k] == 1.0);
    }
  }
  return r;
}

// grid-stride over groups of 4 words; n_words words (= values / 64).  A group past the end
// (n_words % 4 != 0) loads nothing for its missing words: their lanes report off / valid.
template <int KIND>
__global__ __launch_bounds__(256) void k_pack_mask(const void* __restrict__ src, int64_t n_words, int mode,
                                                   double thr, uint64_t* __restrict__ bits,
                                                   int32_t* __restrict__ err) {
  const int lane = threadIdx.x & 63;
  const int64_t n_groups = (n_words + 3) / 4;
  const int64_t stride = (int64_t)gridDim.x * (blockDim.x >> 6);
  bool bad = false;
  for (int64_t g = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); g < n_groups; g += stride) {
    const int64_t w_lane = 4 * g + (lane >> 4);   // the word this lane's four values belong to
    Quad v;
    if (w_lane < n_words) {
      v = load_quad<KIND>(src, 64 * g + lane, mode, thr);
    } else {
      v.on[0] = v.on[1] = v.on[2] = v.on[3] = false;
      v.bad = false;
    }
    bad |= v.bad;
    const uint64_t b0 = __ballot(v.on[0]), b1 = __ballot(v.on[1]);
    const uint64_t b2 = __ballot(v.on[2]), b3 = __ballot(v.on[3]);
    if (lane < 4 && 4 * g + lane < n_words) {
      const int s = 16 * lane;
      bits[4 * g + lane] = spread4(b0 >> s) | (spread4(b1 >> s) << 1) | (spread4(b2 >> s) << 2) |
                           (spread4(b3 >> s) << 3);
    }
  }
  if (err && mode == HBX_PACK_BINARY && __ballot(bad) != 0ull && lane == 0) *err = 1;
}

constexpr int kRelBlocks = 1024;   // partial slots of the relativeLoss reduction (fixed: deterministic)

template <typename T>
__global__ __launch_bounds__(256) void k_rel_partials(const T* __restrict__ x, const T* __restrict__ y, int64_t n,
                                                      double* __restrict__ part) {
  __shared__ double s[3][4];
  const int64_t per = (n + gridDim.x - 1) / gridDim.x;
  const int64_t i0 = (int64_t)blockIdx.x * per;
  const int64_t i1 = i0 + per < n ? i0 + per : n;
  double sxy = 0.0, sxx = 0.0, syy = 0.0;
  for (int64_t i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
    const double a = (double)x[i], b = (double)y[i];
    sxy = fma(a, b, sxy);
    sxx = fma(a, a, sxx);
    syy = fma(b, b, syy);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sxy += __shfl_xor(sxy, o);
    sxx += __shfl_xor(sxx, o);
    syy += __shfl_xor(syy, o);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { s[0][w] = sxy; s[1][w] = sxx; s[2][w] = syy; }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int k = threadIdx.x;
    part[3 * blockIdx.x + k] = ((s[k][0] + s[k][1]) + s[k][2]) + s[k][3];
  }
}

// one wave: the partials in fixed order, then out = {sum xy, sum x^2, sum y^2, psnr, mse}
__global__ __launch_bounds__(64) void k_rel_final(const double* __restrict__ part, int n_part, double count,
                                                  int rel_scale, double peak, double* __restrict__ out) {
  double a[3] = {0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < n_part; i += 64)
#pragma unroll
    for (int k = 0; k < 3; ++k) a[k] += part[3 * i + k];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int k = 0; k < 3; ++k) a[k] += __shfl_xor(a[k], o);
  if (threadIdx.x == 0) {
    const double sxy = a[0], sxx = a[1], syy = a[2];
    double mse;
    if (rel_scale == HBX_REL_LSQ) mse = (sxx > 0.0) ? (syy - sxy * sxy / sxx) / count : syy / count;
    else mse = (sxx - 2.0 * sxy + syy) / count;
    out[0] = sxy;
    out[1] = sxx;
    out[2] = syy;
    out[3] = psnr_from(sxy, sxx, syy, count, rel_scale, peak);
    out[4] = mse;
  }
}

// the relative MSE as k_rel_final and psnr_from (hbx_internal.hpp) form it: the same expressions in the
// same order (k_rel_final keeps its own copy: its instructions are those of the build before this one)
__device__ __forceinline__ double rel_mse_from(double sxy, double sxx, double syy, double count, int rel_scale) {
  if (rel_scale == HBX_REL_LSQ) return (sxx > 0.0) ? (syy - sxy * sxy / sxx) / count : syy / count;
  return (sxx - 2.0 * sxy + syy) / count;
}

// an env's sums over its G groups, in k_psnr's order
__device__ __forceinline__ void env_sums(const double* __restrict__ chan_stats, int b, int G, double& sxy,
                                         double& sxx, double& syy) {
  sxy = 0.0; sxx = 0.0; syy = 0.0;
  for (int g = 0; g < G; ++g) {
    const double* s = chan_stats + ((size_t)b * G + g) * 3;
    sxy += s[0]; sxx += s[1]; syy += s[2];
  }
}

// hbx_loss: chan_stats[B][G][3] -> loss[B], the relative MSE or its PSNR
__global__ void k_loss(const double* __restrict__ chan_stats, int n, int G, int kind, int rel_scale, double count,
                       double peak, double* __restrict__ loss) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  double sxy, sxx, syy;
  env_sums(chan_stats, b, G, sxy, sxx, syy);
  loss[b] = kind == HBX_LOSS_PSNR ? psnr_from(sxy, sxx, syy, count, rel_scale, peak)
                                  : rel_mse_from(sxy, sxx, syy, count, rel_scale);
}

// hbx_loss_weight: weight = a_b I + c_b T, the gradient of env b's loss with respect to its
// intensity (include/hbx.h has the formulas).  bx workgroups per env; a workgroup forms its env's two
// coefficients in f64 from 3 G statistics -- uniform per workgroup, so scalar loads and no LDS --
// rounds them to f32 once and streams kLossPer 16-byte pieces per thread
constexpr int kLossPer = 4;
// env b's two coefficients, rounded to f32 once
__device__ __forceinline__ void loss_weight_coeffs(const double* __restrict__ chan_stats,
                                                   const double* __restrict__ grad_loss, int b, int G, int kind,
                                                   int rel_scale, double count, float& af, float& cf) {
  double sxy, sxx, syy;
  env_sums(chan_stats, b, G, sxy, sxx, syy);
  double a, c;   // dMSE/dI = a I + c T
  if (rel_scale == HBX_REL_LSQ) {
    const double s = sxx > 0.0 ? sxy / sxx : 0.0;   // no scale to differentiate: a = c = 0
    a = 2.0 * s * s / count;
    c = sxx > 0.0 ? -2.0 * s / count : 0.0;
  } else {
    a = 2.0 / count;
    c = -2.0 / count;
  }
  if (kind == HBX_LOSS_PSNR) {   // PSNR = 10 log10(peak^2 / MSE): dPSNR = -(10 / ln 10) dMSE / MSE
    const double mse = rel_mse_from(sxy, sxx, syy, count, rel_scale);
    const double f = mse > 0.0 ? -(10.0 / 2.302585092994045684) / mse : 0.0;
    a *= f;
    c *= f;
  }
  const double up = grad_loss ? grad_loss[b] : 1.0;
  af = (float)(a * up), cf = (float)(c * up);
}

__global__ __launch_bounds__(256) void k_loss_weight(const float4* __restrict__ inten, const float4* __restrict__ target,
                                                     const double* __restrict__ chan_stats,
                                                     const double* __restrict__ grad_loss, int G, int64_t n4,
                                                     unsigned bx, int kind, int rel_scale, double count,
                                                     float4* __restrict__ weight) {
  const int b = blockIdx.x / bx;
  float af, cf;
  loss_weight_coeffs(chan_stats, grad_loss, b, G, kind, rel_scale, count, af, cf);
  const int64_t base = (int64_t)b * n4;
  const int64_t i0 = (int64_t)(blockIdx.x % bx) * (256 * kLossPer) + threadIdx.x;
  float4 I[kLossPer], T[kLossPer];
#pragma unroll
  for (int k = 0; k < kLossPer; ++k) {
    const int64_t i = i0 + 256 * k;
    if (i < n4) {
      I[k] = inten[base + i];
      T[k] = target[base + i];
    }
  }
#pragma unroll
  for (int k = 0; k < kLossPer; ++k) {
    const int64_t i = i0 + 256 * k;
    if (i < n4)
      weight[base + i] = make_float4(fmaf(af, I[k].x, cf * T[k].x), fmaf(af, I[k].y, cf * T[k].y),
                                     fmaf(af, I[k].z, cf * T[k].z), fmaf(af, I[k].w, cf * T[k].w));
  }
}

// k_loss_weight one float at a time (hbx_loss_weight_window): the images of an output window are compact,
// so an env's G h w floats are neither a multiple of four nor 16-byte aligned in general.  The same
// coefficients and the same fmaf per pixel: on a full-grid window it is k_loss_weight's weight bit for bit
__global__ __launch_bounds__(256) void k_loss_weight1(const float* __restrict__ inten, const float* __restrict__ target,
                                                      const double* __restrict__ chan_stats,
                                                      const double* __restrict__ grad_loss, int G, int64_t n1,
                                                      unsigned bx, int kind, int rel_scale, double count,
                                                      float* __restrict__ weight) {
  const int b = blockIdx.x / bx;
  float af, cf;
  loss_weight_coeffs(chan_stats, grad_loss, b, G, kind, rel_scale, count, af, cf);
  const int64_t base = (int64_t)b * n1;
  const int64_t i0 = (int64_t)(blockIdx.x % bx) * (256 * kLossPer) + threadIdx.x;
#pragma unroll
  for (int k = 0; k < kLossPer; ++k) {
    const int64_t i = i0 + 256 * k;
    if (i < n1) weight[base + i] = fmaf(af, inten[base + i], cf * target[base + i]);
  }
}

// (extension, focal stacks) an env's sums over its D G channels of chan_stats[D][n][G][3]: d outer, g inner,
// from 0.0 as env_sums -- at D = 1 the same additions in the same order
__device__ __forceinline__ void env_sums_stack(const double* __restrict__ chan_stats, int b, int n, int G, int D,
                                               double& sxy, double& sxx, double& syy) {
  sxy = 0.0; sxx = 0.0; syy = 0.0;
  for (int d = 0; d < D; ++d)
    for (int g = 0; g < G; ++g) {
      const double* s = chan_stats + (((size_t)d * n + b) * G + g) * 3;
      sxy += s[0]; sxx += s[1]; syy += s[2];
    }
}

// hbx_loss_stack: chan_stats[D][n][G][3] -> loss[n]; k_loss's expressions on the stack's sums, count = D G hw
__global__ void k_loss_stack(const double* __restrict__ chan_stats, int n, int G, int D, int kind, int rel_scale,
                             double count, double peak, double* __restrict__ loss) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  double sxy, sxx, syy;
  env_sums_stack(chan_stats, b, n, G, D, sxy, sxx, syy);
  loss[b] = kind == HBX_LOSS_PSNR ? psnr_from(sxy, sxx, syy, count, rel_scale, peak)
                                  : rel_mse_from(sxy, sxx, syy, count, rel_scale);
}

// hbx_loss_weight_stack: weight[d][b] = a_b I[d][b] + c_b T[d][b], one (a, c) per env for the whole stack,
// loss_weight_coeffs' expressions on the stack's sums.  bx workgroups per (depth, env) image set of n4 16-byte
// pieces; blockIdx.x = (d n + b) bx + piece block, so the images are indexed as k_loss_weight indexes an env's
__global__ __launch_bounds__(256) void k_loss_weight_stack(const float4* __restrict__ inten,
                                                           const float4* __restrict__ target,
                                                           const double* __restrict__ chan_stats,
                                                           const double* __restrict__ grad_loss, int n, int G, int D,
                                                           int64_t n4, unsigned bx, int kind, int rel_scale,
                                                           double count, float4* __restrict__ weight) {
  const int db = blockIdx.x / bx;   // d * n + b
  const int b = db % n;
  double sxy, sxx, syy;
  env_sums_stack(chan_stats, b, n, G, D, sxy, sxx, syy);
  double a, c;   // dMSE/dI = a I + c T
  if (rel_scale == HBX_REL_LSQ) {
    const double s = sxx > 0.0 ? sxy / sxx : 0.0;   // no scale to differentiate: a = c = 0
    a = 2.0 * s * s / count;
    c = sxx > 0.0 ? -2.0 * s / count : 0.0;
  } else {
    a = 2.0 / count;
    c = -2.0 / count;
  }
  if (kind == HBX_LOSS_PSNR) {
    const double mse = rel_mse_from(sxy, sxx, syy, count, rel_scale);
    const double f = mse > 0.0 ? -(10.0 / 2.302585092994045684) / mse : 0.0;
    a *= f;
    c *= f;
  }
  const double up = grad_loss ? grad_loss[b] : 1.0;
  const float af = (float)(a * up), cf = (float)(c * up);
  const int64_t base = (int64_t)db * n4;
  const int64_t i0 = (int64_t)(blockIdx.x % bx) * (256 * kLossPer) + threadIdx.x;
  float4 I[kLossPer], T[kLossPer];
#pragma unroll
  for (int k = 0; k < kLossPer; ++k) {
    const int64_t i = i0 + 256 * k;
    if (i < n4) {
      I[k] = inten[base + i];
      T[k] = target[base + i];
    }
  }
#pragma unroll
  for (int k = 0; k < kLossPer; ++k) {
    const int64_t i = i0 + 256 * k;
    if (i < n4)
      weight[base + i] = make_float4(fmaf(af, I[k].x, cf * T[k].x), fmaf(af, I[k].y, cf * T[k].y),
                                     fmaf(af, I[k].z, cf * T[k].z), fmaf(af, I[k].w, cf * T[k].w));
  }
}

}  // namespace

hipError_t launch_loss_stack(const double* chan_stats, int n, int G, int D, int kind, int rel_scale, double count,
                             double peak, double* loss, hipStream_t st) {
  hipLaunchKernelGGL(k_loss_stack, dim3((n + 63) / 64), dim3(64), 0, st, chan_stats, n, G, D, kind, rel_scale, count,
                     peak, loss);
  return hipGetLastError();
}

// (full-grid images only: G hw is a multiple of 4 at every built size, and the caller's arrays are whole
// tensors; a misaligned pointer is refused, not taken one float at a time)
hipError_t launch_loss_weight_stack(const float* inten, const float* target, const double* chan_stats,
                                    const double* grad_loss, int n, int G, int D, size_t hw, int kind, int rel_scale,
                                    double count, float* weight, hipStream_t st) {
  const int64_t n1 = (int64_t)G * (int64_t)hw;
  const auto misaligned = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) != 0; };
  if (n1 % 4 != 0 || misaligned(inten) || misaligned(target) || misaligned(weight)) return hipErrorInvalidValue;
  const int64_t n4 = n1 / 4;
  const unsigned bx = (unsigned)((n4 + 256 * kLossPer - 1) / (256 * kLossPer));
  hipLaunchKernelGGL(k_loss_weight_stack, dim3(bx * (unsigned)n * (unsigned)D), dim3(256), 0, st,
                     reinterpret_cast<const float4*>(inten), reinterpret_cast<const float4*>(target), chan_stats,
                     grad_loss, n, G, D, n4, bx, kind, rel_scale, count, reinterpret_cast<float4*>(weight));
  return hipGetLastError();
}

hipError_t launch_loss(const double* chan_stats, int n, int G, int kind, int rel_scale, double count, double peak,
                       double* loss, hipStream_t st) {
  hipLaunchKernelGGL(k_loss, dim3((n + 63) / 64), dim3(64), 0, st, chan_stats, n, G, kind, rel_scale, count, peak,
                     loss);
  return hipGetLastError();
}

hipError_t launch_loss_weight(const float* inten, const float* target, const double* chan_stats,
                              const double* grad_loss, int n, int G, size_t hw, int kind, int rel_scale, double count,
                              float* weight, hipStream_t st) {
  const int64_t n1 = (int64_t)G * (int64_t)hw;
  const auto misaligned = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) != 0; };
  if (n1 % 4 != 0 || misaligned(inten) || misaligned(target) || misaligned(weight)) {   // a window's compact images
    const unsigned bx1 = (unsigned)((n1 + 256 * kLossPer - 1) / (256 * kLossPer));
    hipLaunchKernelGGL(k_loss_weight1, dim3(bx1 * (unsigned)n), dim3(256), 0, st, inten, target, chan_stats, grad_loss,
                       G, n1, bx1, kind, rel_scale, count, weight);
    return hipGetLastError();
  }
  const int64_t n4 = n1 / 4;   // 16-byte pieces per env (N^2 is a multiple of 4)
  const unsigned bx = (unsigned)((n4 + 256 * kLossPer - 1) / (256 * kLossPer));
  hipLaunchKernelGGL(k_loss_weight, dim3(bx * (unsigned)n), dim3(256), 0, st,
                     reinterpret_cast<const float4*>(inten), reinterpret_cast<const float4*>(target), chan_stats,
                     grad_loss, G, n4, bx, kind, rel_scale, count, reinterpret_cast<float4*>(weight));
  return hipGetLastError();
}

// hbx_quantize_phase: the phase quantizer (quantize_phase_k, hbx_internal.hpp) on n float32 samples, one
// streaming pass, element i by thread i of a grid-stride loop (any n, no alignment asked of the pointers):
// level = k mod L as uint8 to out_levels and / or q = k s to out_phase, either nullable.  h and s are the
// host's values, the ones the pass kernels quantize with.
__global__ __launch_bounds__(256) void k_quantize_phase(const float* __restrict__ src, int64_t n, int levels, float h,
                                                        float s, uint8_t* __restrict__ out_levels,
                                                        float* __restrict__ out_phase) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const float k = quantize_phase_k(__builtin_nontemporal_load(src + i), h);
    if (out_levels) out_levels[i] = (uint8_t)quantize_phase_level(k, levels);
    if (out_phase) out_phase[i] = k * s;
  }
}

hipError_t launch_quantize_phase(const float* src, int64_t n, int levels, uint8_t* out_levels, float* out_phase,
                                 hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const int64_t want = (n + 1023) / 1024;   // 4 samples per thread before the grid is capped
  const unsigned blocks = (unsigned)(want < 256 * 16 ? want : 256 * 16);
  const PhaseLevels q = phase_levels_of(levels);
  hipLaunchKernelGGL(k_quantize_phase, dim3(blocks), dim3(256), 0, st, src, n, levels, q.h, q.s, out_levels, out_phase);
  return hipGetLastError();
}

hipError_t launch_pack_mask(const void* src, int kind, int64_t n_words, int mode, double thr, uint64_t* bits,
                            int32_t* err, hipStream_t st) {
  if (n_words <= 0) return hipSuccess;
  const int64_t groups = (n_words + 3) / 4;
  const int64_t want = (groups + 3) / 4;   // 4 waves per workgroup
  const unsigned blocks = (unsigned)(want < 256 * 8 ? want : 256 * 8);
  switch (kind) {
    case HBX_SRC_U8:
      hipLaunchKernelGGL(k_pack_mask<HBX_SRC_U8>, dim3(blocks), dim3(256), 0, st, src, n_words, mode, thr, bits, err);
      break;
    case HBX_SRC_F32:
      hipLaunchKernelGGL(k_pack_mask<HBX_SRC_F32>, dim3(blocks), dim3(256), 0, st, src, n_words, mode, thr, bits, err);
      break;
    case HBX_SRC_F64:
      hipLaunchKernelGGL(k_pack_mask<HBX_SRC_F64>, dim3(blocks), dim3(256), 0, st, src, n_words, mode, thr, bits, err);
      break;
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

int rel_partial_slots() { return kRelBlocks; }

hipError_t launch_rel_stats(const void* x, const void* y, int kind, int64_t n, double count, int rel_scale,
                            double peak, double* part, double* out, hipStream_t st) {
  const int64_t want = (n + 4095) / 4096;   // >= 4096 values per workgroup
  const unsigned blocks = (unsigned)(want < 1 ? 1 : (want < kRelBlocks ? want : kRelBlocks));
  if (kind == HBX_SRC_F32)
    hipLaunchKernelGGL(k_rel_partials<float>, dim3(blocks), dim3(256), 0, st, static_cast<const float*>(x),
                       static_cast<const float*>(y), n, part);
  else if (kind == HBX_SRC_F64)
    hipLaunchKernelGGL(k_rel_partials<double>, dim3(blocks), dim3(256), 0, st, static_cast<const double*>(x),
                       static_cast<const double*>(y), n, part);
  else
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_rel_final, dim3(1), dim3(64), 0, st, part, (int)blocks, count, rel_scale, peak, out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Per-pixel loss weights (hbx_pixel_weight_sum, hbx_loss_pw, hbx_loss_weight_pw; include/hbx.h)
// ---------------------------------------------------------------------------
// Behind every other kernel of this file.  The arrays are depth-major [D][n][..] as a focal stack's; D = 1 is the
// single depth, where env_sums_stack runs env_sums' additions in env_sums' order.
namespace {

constexpr int kPwSumNT = 256;

// hbx_pixel_weight_sum, first step: an env's D G images of pixel_weight in K slices.  Workgroup (b, k) adds slice
// k of depth 0's G hw floats (g inner), then of depth 1's, ..: thread t its elements t, t + NT, .. of the slice in
// f64, then the wave's lanes by xor shuffles, then the four waves in order -> part[b K + k].  A fixed order for a
// given K, bitwise reproducible, and exact whenever every partial sum is representable (a 0 / 1 indicator: the
// count of ones).  VEC: 16-byte pieces.  b0, n_total: the chunk's first env and the envs of the whole array
template <bool VEC>
__global__ __launch_bounds__(kPwSumNT) void k_pixel_weight_part(const float* __restrict__ pw, int b0, int n_total,
                                                                int D, int64_t n1, int K, double* __restrict__ part) {
  __shared__ double s[kPwSumNT / 64];
  const int b = blockIdx.x / K, k = blockIdx.x % K;
  const int64_t nv = VEC ? n1 / 4 : n1;             // pieces per depth
  const int64_t per = (nv + K - 1) / K;
  const int64_t lo = (int64_t)k * per, hi = lo + per < nv ? lo + per : nv;
  double a = 0.0;
  for (int d = 0; d < D; ++d) {
    const float* img = pw + ((int64_t)d * n_total + b0 + b) * n1;
    if constexpr (VEC) {
      const float4* img4 = reinterpret_cast<const float4*>(img);
      for (int64_t i = lo + threadIdx.x; i < hi; i += kPwSumNT) {
        const float4 x = img4[i];
        a += (double)x.x; a += (double)x.y; a += (double)x.z; a += (double)x.w;
      }
    } else {
      for (int64_t i = lo + threadIdx.x; i < hi; i += kPwSumNT) a += (double)img[i];
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) part[(int64_t)b * K + k] = ((s[0] + s[1]) + s[2]) + s[3];
}

// second step: env b's K partials in order -> weight_sum[b0 + b]
__global__ void k_pixel_weight_final(const double* __restrict__ part, int n, int K, double* __restrict__ weight_sum) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  double w = 0.0;
  for (int k = 0; k < K; ++k) w += part[(int64_t)b * K + k];
  weight_sum[b] = w;
}

// dMSE/dI = v (a I + c T): loss_weight_coeffs' expressions on the sums given, with the weight sum W as the
// count; an env with W = 0 (an all-zero weight) has nothing to differentiate: a = c = 0, never a NaN
__device__ __forceinline__ void loss_pw_coeffs(double sxy, double sxx, double syy, double count, double up, int kind,
                                               int rel_scale, float& af, float& cf) {
  double a, c;
  if (rel_scale == HBX_REL_LSQ) {
    const double s = sxx > 0.0 ? sxy / sxx : 0.0;   // no scale to differentiate: a = c = 0
    a = 2.0 * s * s / count;
    c = sxx > 0.0 ? -2.0 * s / count : 0.0;
  } else {
    a = 2.0 / count;
    c = -2.0 / count;
  }
  if (kind == HBX_LOSS_PSNR) {
    const double mse = rel_mse_from(sxy, sxx, syy, count, rel_scale);
    const double f = mse > 0.0 ? -(10.0 / 2.302585092994045684) / mse : 0.0;
    a *= f;
    c *= f;
  }
  if (count == 0.0) { a = 0.0; c = 0.0; }
  af = (float)(a * up), cf = (float)(c * up);
}

// hbx_loss_pw: k_loss_stack's expressions with weight_sum[b] as the count; W = 0: MSE 0, PSNR +inf
__global__ void k_loss_pw(const double* __restrict__ chan_stats, const double* __restrict__ weight_sum, int n, int G,
                          int D, int kind, int rel_scale, double peak, double* __restrict__ loss) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  double sxy, sxx, syy;
  env_sums_stack(chan_stats, b, n, G, D, sxy, sxx, syy);
  const double count = weight_sum[b];
  if (count == 0.0) {
    loss[b] = kind == HBX_LOSS_PSNR ? (double)INFINITY : 0.0;
    return;
  }
  loss[b] = kind == HBX_LOSS_PSNR ? psnr_from(sxy, sxx, syy, count, rel_scale, peak)
                                  : rel_mse_from(sxy, sxx, syy, count, rel_scale);
}

// hbx_loss_weight_pw: weight[d][b] = v[d][b] * fmaf(a_b, I, c_b T) -- k_loss_weight_stack's coefficients and fmaf,
// then one more multiply -- indexed as k_loss_weight_stack indexes the images.  V4 = float4 (16-byte pieces) or
// float (any count, any alignment)
template <class V4>
__global__ __launch_bounds__(256) void k_loss_weight_pw(const V4* __restrict__ inten, const V4* __restrict__ target,
                                                        const V4* __restrict__ pw,
                                                        const double* __restrict__ chan_stats,
                                                        const double* __restrict__ weight_sum,
                                                        const double* __restrict__ grad_loss, int n, int G, int D,
                                                        int64_t nv, unsigned bx, int kind, int rel_scale,
                                                        V4* __restrict__ weight) {
  const int db = blockIdx.x / bx;   // d * n + b
  const int b = db % n;
  double sxy, sxx, syy;
  env_sums_stack(chan_stats, b, n, G, D, sxy, sxx, syy);
  float af, cf;
  loss_pw_coeffs(sxy, sxx, syy, weight_sum[b], grad_loss ? grad_loss[b] : 1.0, kind, rel_scale, af, cf);
  const int64_t base = (int64_t)db * nv;
  const int64_t i0 = (int64_t)(blockIdx.x % bx) * (256 * kLossPer) + threadIdx.x;
  V4 I[kLossPer], T[kLossPer], v[kLossPer];
#pragma unroll
  for (int k = 0; k < kLossPer; ++k) {
    const int64_t i = i0 + 256 * k;
    if (i < nv) {
      I[k] = inten[base + i];
      T[k] = target[base + i];
      v[k] = pw[base + i];
    }
  }
#pragma unroll
  for (int k = 0; k < kLossPer; ++k) {
    const int64_t i = i0 + 256 * k;
    if (i < nv) {
      if constexpr (sizeof(V4) == 16)
        weight[base + i] = make_float4(v[k].x * fmaf(af, I[k].x, cf * T[k].x), v[k].y * fmaf(af, I[k].y, cf * T[k].y),
                                       v[k].z * fmaf(af, I[k].z, cf * T[k].z), v[k].w * fmaf(af, I[k].w, cf * T[k].w));
      else
        weight[base + i] = v[k] * fmaf(af, I[k], cf * T[k]);
    }
  }
}

}  // namespace

// n envs from env b0 of an array of n_total in K slices each; part: scratch of n K doubles
hipError_t launch_pixel_weight_sum(const float* pixel_weight, int b0, int n, int n_total, int G, int D, size_t hw,
                                   double* part, int K, double* weight_sum, hipStream_t st) {
  const int64_t n1 = (int64_t)G * (int64_t)hw;
  const bool vec = n1 % 4 == 0 && (reinterpret_cast<uintptr_t>(pixel_weight) & 15) == 0;
  if (K < 1) return hipErrorInvalidValue;
  if (vec)
    hipLaunchKernelGGL(k_pixel_weight_part<true>, dim3((unsigned)n * K), dim3(kPwSumNT), 0, st, pixel_weight, b0,
                       n_total, D, n1, K, part);
  else
    hipLaunchKernelGGL(k_pixel_weight_part<false>, dim3((unsigned)n * K), dim3(kPwSumNT), 0, st, pixel_weight, b0,
                       n_total, D, n1, K, part);
  hipLaunchKernelGGL(k_pixel_weight_final, dim3((n + 63) / 64), dim3(64), 0, st, part, n, K, weight_sum + b0);
  return hipGetLastError();
}

hipError_t launch_loss_pw(const double* chan_stats, const double* weight_sum, int n, int G, int D, int kind,
                          int rel_scale, double peak, double* loss, hipStream_t st) {
  hipLaunchKernelGGL(k_loss_pw, dim3((n + 63) / 64), dim3(64), 0, st, chan_stats, weight_sum, n, G, D, kind, rel_scale,
                     peak, loss);
  return hipGetLastError();
}

hipError_t launch_loss_weight_pw(const float* inten, const float* target, const float* pixel_weight,
                                 const double* chan_stats, const double* weight_sum, const double* grad_loss, int n,
                                 int G, int D, size_t hw, int kind, int rel_scale, float* weight, hipStream_t st) {
  const int64_t n1 = (int64_t)G * (int64_t)hw;
  const auto misaligned = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) != 0; };
  if (n1 % 4 != 0 || misaligned(inten) || misaligned(target) || misaligned(pixel_weight) || misaligned(weight)) {
    const unsigned bx1 = (unsigned)((n1 + 256 * kLossPer - 1) / (256 * kLossPer));
    hipLaunchKernelGGL(k_loss_weight_pw<float>, dim3(bx1 * (unsigned)n * (unsigned)D), dim3(256), 0, st, inten, target,
                       pixel_weight, chan_stats, weight_sum, grad_loss, n, G, D, n1, bx1, kind, rel_scale, weight);
    return hipGetLastError();
  }
  const int64_t n4 = n1 / 4;
  const unsigned bx = (unsigned)((n4 + 256 * kLossPer - 1) / (256 * kLossPer));
  hipLaunchKernelGGL(k_loss_weight_pw<float4>, dim3(bx * (unsigned)n * (unsigned)D), dim3(256), 0, st,
                     reinterpret_cast<const float4*>(inten), reinterpret_cast<const float4*>(target),
                     reinterpret_cast<const float4*>(pixel_weight), chan_stats, weight_sum, grad_loss, n, G, D, n4, bx,
                     kind, rel_scale, reinterpret_cast<float4*>(weight));
  return hipGetLastError();
}

// (extension, illumination fields) hbx_source_field: the field at the modulator, u = s f(x), one streaming
// pass with the device functions the sourced first passes form it with (source_sample, hbx_rowcol.hpp), so
// the materialised u is theirs bit for bit.  The leaf's [B][G Q][hw] samples -- complex64 pairs for
// kSrcComplex, float32 otherwise, read once (non-temporal) -- times source[g][pixel].  A workgroup row
// (blockIdx.y, strided) is a plane, so the group is found once per plane and no pixel divides; the pixels of
// a plane go to the threads of its workgroups in a grid-stride loop.
template <int SK>
__global__ __launch_bounds__(256) void k_source_field(const float* __restrict__ values,
                                                      const float2* __restrict__ source, int64_t n_planes, int G,
                                                      int Q, int hw, float p0, float p1, float p2,
                                                      float2* __restrict__ out) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const int stride = (int)gridDim.x * 256;
  for (int64_t plane = blockIdx.y; plane < n_planes; plane += gridDim.y) {
    const int g = (int)((plane / Q) % G);
    const float2* __restrict__ srow = source + (size_t)g * hw;
    const size_t base = (size_t)plane * hw;
    for (int pix = (int)blockIdx.x * 256 + threadIdx.x; pix < hw; pix += stride) {
      const float2 s = srow[pix];
      float a, b = 0.0f;
      if constexpr (SK == kSrcComplex) {
        const f32x2 x = __builtin_nontemporal_load(reinterpret_cast<const f32x2*>(values) + base + pix);
        a = x.x, b = x.y;
      } else {
        a = __builtin_nontemporal_load(values + base + pix);
      }
      float ur, ui;
      source_sample<SK>(a, b, s.x, s.y, p0, p1, p2, ur, ui);
      out[base + pix] = make_float2(ur, ui);
    }
  }
}

hipError_t launch_source_field(const float* values, const float2* source, int sk, int64_t n_planes, int G, int Q,
                               size_t hw, float p0, float p1, float p2, float2* out, hipStream_t st) {
  if (n_planes <= 0 || hw == 0) return hipSuccess;
  const size_t want = (hw + 1023) / 1024;   // 4 pixels per thread before the grid is capped
  const unsigned bx = (unsigned)(want < 64 ? want : 64);
  const unsigned by = (unsigned)(n_planes < 65535 ? n_planes : 65535);
  auto k = k_source_field<kSrcComplex>;
  if (sk == kSrcPhase) k = k_source_field<kSrcPhase>;
  if (sk == kSrcPhaseLevels) k = k_source_field<kSrcPhaseLevels>;
  if (sk == kSrcReal) k = k_source_field<kSrcReal>;
  if (sk == kSrcThreshold) k = k_source_field<kSrcThreshold>;
  hipLaunchKernelGGL(k, dim3(bx, by), dim3(256), 0, st, values, source, n_planes, G, Q, (int)hw, p0, p1, p2, out);
  return hipGetLastError();
}

}  // namespace hbx
