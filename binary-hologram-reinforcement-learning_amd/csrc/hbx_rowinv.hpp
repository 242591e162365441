// hbx_rowinv.hpp -- the pieces the last-pass kernels share across size classes (hbx_passes.hip:
// k_rowinv_d, k_rowinv and their _cplx forms; hbx_passes896.hip: k_rowinv896, k_rowinv896_cplx):
// invalid-job exit, the direct loads from the tiled B and the pair-combining load, the chunk decode
// of the N = 64 tile, the plane cache and its step schedule, the bit path's per-plane outputs and the tail;
// and, for the depth-summing last passes of a focal stack (k_rowinv_d_cplx_stack, k_rowinv_cplx_stack,
// k_rowinv896_cplx_stack), the pair load that adds the depth slots: rowinv_load_pair_stack.
// <int R, int L = R> as real_load_row: R lanes per group, L values per lane, N = R L (N = 896 is
// <32, 28>).  The block prologue (twiddle staging, the grp / t / rb / j decode) stays
// written out in the six kernels: as a helper it changed the code of every one of them (the group's
// scratch offset formed from the shifted instead of the masked thread id, another register assignment).
// The complex kernels' per-plane output step is cplx_plane_out, except its full-grid field / real-part
// form in k_rowinv_cplx and k_rowinv896_cplx: as a helper that form changed both (k_rowinv896_cplx's spills too).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hbx_fft.hpp"
#include "hbx_internal.hpp"
#include "hbx_rowcol.hpp"
#include "hbx_walk_planes.hpp"

namespace hbx {

// an invalid job's row block (jb.env < 0, uniform per block): neutral partials.  SC1: the write-through
// form of the walk batch, whose deciding workgroup reads them in the same launch (k_rowinv_d<R, true>)
template <bool SC1 = false>
__device__ __forceinline__ void rowinv_zero_partial(double* __restrict__ partial, int j, int RB, int rb) {
  if (threadIdx.x == 0) {
    double* o = partial + ((size_t)j * RB + rb) * 3;
    if constexpr (SC1) {
      const __amdgpu_buffer_rsrc_t ro = walk_planes_rsrc(o, 24);
      for (int i = 0; i < 3; ++i) __builtin_amdgcn_raw_buffer_store_b64(u32x2{0u, 0u}, ro, 8 * i, 0, kSc1Bit);
    } else {
      o[0] = 0.0; o[1] = 0.0; o[2] = 0.0;
    }
  }
}

// k_rowinv at N = 1024 / 256 (r03): every lane loads its own FFT input straight from
// the tiled B (TileB) -- lane t of group g (row y0 + g) needs kx = t + R jj, which for TL
// consecutive lanes is TL consecutive slots of one tile row (64 B at N = 1024: the two rows
// of a wave are adjacent, 128 B; 128 B at N = 256: a wave's four rows are one 512-B run),
// so no LDS tile and no block barrier sit in the plane loop: the group's FFT transpose
// (wave_sync) is its only LDS traffic.  The next plane's loads are issued as soon as this
// plane's FFT is done (two blocks per CU cover them; a second register set for a plane in
// flight took one block per CU and measured 1.80 ms against 1.47).  The r02
// kernel staged every plane through an LDS tile between three block barriers (1.80 ms).
// Lane bases (bytes from the job's first B plane) of row y for lane t of the row's group; slot s at
// TileB<R>::at(s, y):
//   jj < R/2 (and kx = N/2 for t = 0): s = kx = t + R jj -> lo + 16 R jj float2
//   jj >= R/2 otherwise: s = 3N/2 - kx -> hi - 16 R jj, written hiB + 16 R (R - 1 - jj)
//   so every offset stays non-negative
template <int R>
struct RowinvLanes {
  static constexpr int N = R * R, TL = 256 / R;
  static constexpr int kRegs = R;                   // FFT inputs per lane
  static constexpr int kPlaneBytes = N * N * 8;     // B plane stride
  static constexpr int JS = 16 * R * 8;             // bytes per jj
  int lo, hiB, vmid;
  __device__ __forceinline__ RowinvLanes(int y, int t) {
    const int yb = (y >> 4) * 16 * N + (y & 15) * TL;
    const int m = t / TL, u = t % TL;
    lo = (yb + m * 16 * TL + u) * 8;
    hiB = (yb + (u ? (3 * N / (2 * TL) - m - 1) * 16 * TL + TL - u : (3 * N / (2 * TL) - m) * 16 * TL) -
           16 * R * (R - 1)) * 8;
    vmid = t == 0 ? lo + JS * (R / 2) : hiB + JS * (R / 2 - 1);
  }
  // the lane's FFT input jj (kx = t + R jj) of the plane at byte offset po (wave-uniform)
  __device__ __forceinline__ float2 load(__amdgpu_buffer_rsrc_t rs, int po, int jj) const {
    const int vo = jj < R / 2 ? lo : (jj == R / 2 ? vmid : hiB);
    const int so = po + (jj < R / 2 ? JS * jj : (jj == R / 2 ? 0 : JS * (R - 1 - jj)));
    return buf_ld2s(rs, vo, so);
  }
};

// plane p of the job into v (V = pk2 or float2), through the size class's lane bases ln
// (RowinvLanes<R>, Rowinv896Lanes: load(rs, po, k), kRegs, kPlaneBytes)
template <class Lanes, class V>
__device__ __forceinline__ void rowinv_load_plane(V (&v)[Lanes::kRegs], const Lanes& ln, __amdgpu_buffer_rsrc_t rs, int p) {
  const int po = p * Lanes::kPlaneBytes;
#pragma unroll
  for (int k = 0; k < Lanes::kRegs; ++k) {
    const float2 f = ln.load(rs, po, k);
    v[k] = V{f.x, f.y};
  }
}

// Complex fields: v = B[2q] + i B[2q + 1].  Plane 2q + 1 arrives in two halves of kRegs / 2 values
// that are folded into v as they land, so two whole lines are never live (the second register set
// that cost k_rowinv_d its second block per CU).
template <class Lanes, class V>
__device__ __forceinline__ void rowinv_load_pair(V (&v)[Lanes::kRegs], const Lanes& ln, __amdgpu_buffer_rsrc_t rs, int q) {
  constexpr int H = Lanes::kRegs / 2;
  const int po = 2 * q * Lanes::kPlaneBytes;
  rowinv_load_plane(v, ln, rs, 2 * q);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    float2 w[H];
#pragma unroll
    for (int k = 0; k < H; ++k) w[k] = ln.load(rs, po + Lanes::kPlaneBytes, h * H + k);
#pragma unroll
    for (int k = 0; k < H; ++k) {
      v[h * H + k].x -= w[k].y;
      v[h * H + k].y += w[k].x;
    }
  }
}

// Focal stacks (hbx_backward_stack): the job's pair q summed over D depths whose B slots lie dstride float2
// apart, v = (((B_0[2q] + i B_0[2q + 1]) + B_1[2q]) + i B_1[2q + 1]) + ... in float32, d ascending.  Depth 0
// is rowinv_load_pair itself -- the running line starts from its value, never from 0.0f, so D = 1 gives the
// single-depth bits (the sign of a zero included) -- and every further plane arrives in halves of kRegs / 2
// values that are added as they land: v and half a line are live, as in rowinv_load_pair.  A job's planes are
// addressed through a descriptor of its own per depth (the stride between depths can pass 4 GiB).
template <class Lanes, class V>
__device__ __forceinline__ void rowinv_load_pair_stack(V (&v)[Lanes::kRegs], const Lanes& ln, const float2* job_b,
                                                       size_t dstride, unsigned job_bytes, int D, int q) {
  rowinv_load_pair(v, ln, plane_rsrc(job_b, job_bytes), q);
  constexpr int H = Lanes::kRegs / 2;
  const int po = 2 * q * Lanes::kPlaneBytes;
#pragma unroll 1
  for (int d = 1; d < D; ++d) {
    const __amdgpu_buffer_rsrc_t rs = plane_rsrc(job_b + (size_t)d * dstride, job_bytes);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float2 w[H];
#pragma unroll
      for (int k = 0; k < H; ++k) w[k] = ln.load(rs, po, h * H + k);
#pragma unroll
      for (int k = 0; k < H; ++k) {
        v[h * H + k].x += w[k].x;
        v[h * H + k].y += w[k].y;
      }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float2 w[H];
#pragma unroll
      for (int k = 0; k < H; ++k) w[k] = ln.load(rs, po + Lanes::kPlaneBytes, h * H + k);
#pragma unroll
      for (int k = 0; k < H; ++k) {
        v[h * H + k].x -= w[k].y;
        v[h * H + k].y += w[k].x;
      }
    }
  }
}

// N = 64 (LDS tile transpose): a plane tile is N lines x GPB rows, moved as 16-B chunks of two rows;
// thread tid's i-th chunk c = tid + NT i is rows r2, r2 + 1 of line c / (GPB / 2)
struct TileChunk {
  int line, r2;
};
template <int NT, int GPB>
__device__ __forceinline__ TileChunk tile_chunk(int i) {
  const int c = threadIdx.x + NT * i;
  return {c / (GPB / 2), (c % (GPB / 2)) * 2};
}
// (the tile writes and the transposed read stay written out in the two kernels: a helper that takes
// the LDS tile as a pointer changed k_rowinv's code)

// Plane cache (ABI v9; k_rowinv_d, and k_rowinv896 since r06): the slots of this env's planes and the
// pool rows of this lane group's row y.  Every plane's |U_p|^2 goes to its slot on a fill; on a step
// both planes of the flipped pair go to the job's two spares -- the partner's bits change too (the
// pair is ONE complex row FFT, so its rounding sees the flipped plane), which is why a step keeps both.
template <int R, int L = R>
struct PlaneCache {
  static constexpr int N = R * L;
  float* pool;
  const int32_t* slots;
  int env, group, P, CHS, spare, y;
  __device__ __forceinline__ PlaneCache(const JobDesc& jb, int j, int y_, int G, int P_, int plane_spares,
                                        int spare_base, float* plane_pool, const int32_t* plane_slot) {
    const int CH = G * P_;
    CHS = CH + 2 * (plane_spares > 1 ? plane_spares : 1);            // pool slots per env
    spare = CH + 2 * (plane_spares > 1 ? spare_base + j : 0);        // this job's fresh pair
    slots = plane_slot ? plane_slot + (size_t)jb.env * CHS : nullptr;
    pool = plane_pool, env = jb.env, group = jb.group, P = P_, y = y_;
  }
  __device__ __forceinline__ int slot_of_fill(int p) const { return slots[group * P + p]; }
  __device__ __forceinline__ int slot_of_step(int p) const { return slots[spare + (p & 1)]; }
  __device__ __forceinline__ float* row(int slot) const { return pool + (((size_t)env * CHS + slot) * N + y) * N; }
  // plane p's |U_p|^2 (plane_mode = kPlanesFill or kPlanesStep).  It takes the mode and the plane, not a
  // slot: with the slot chosen by the caller k_rowinv_d<16> grew by 21 instructions
  __device__ __forceinline__ void store(const float (&f)[L], int plane_mode, int p, int t) const {
    float* orow = row(plane_mode == kPlanesFill ? slot_of_fill(p) : slot_of_step(p));
#pragma unroll
    for (int k = 0; k < L; ++k) __builtin_nontemporal_store(f[k], orow + t + R * k);
  }
  // a cached plane's |U_q|^2 added in its place in the plane order (the sum is the FFT mode's
  // sum bit for bit: acc = ((0 + c_0) + c_1) + ..., each c_q the same f32 value)
  __device__ __forceinline__ void add_cached(float (&acc)[L], int q, int t) const {
    const float* crow = row(slot_of_fill(q));
    float c[L];
#pragma unroll
    for (int k = 0; k < L; ++k) c[k] = __builtin_nontemporal_load(crow + t + R * k);
#pragma unroll
    for (int k = 0; k < L; ++k) acc[k] += c[k];
  }
};

// One plane U_p out of the inverse row FFT (v: natural layout, x = t + R k): |U_p|^2 into acc, the
// exact field to field_out (nullable; incremental mode init / refresh) and, with the plane cache on,
// |U_p|^2 to its pool row
template <int R, int L, class V, int NV>
__device__ __forceinline__ void plane_out(const V (&v)[NV], float (&acc)[L], const PlaneCache<R, L>& pc,
                                          const JobDesc& jb, int G, int P, int p, int t,
                                          float2* field_out, int plane_mode) {
  float f[L];
#pragma unroll
  for (int k = 0; k < L; ++k) {
    f[k] = fmaf(v[k].x, v[k].x, v[k].y * v[k].y);
    acc[k] += f[k];
  }
  if (field_out) {
    float2* frow = field_out + (((size_t)jb.env * G * P + jb.group * P + p) * pc.N + pc.y) * pc.N;
#pragma unroll
    for (int k = 0; k < L; ++k) frow[t + R * k] = make_float2(v[k].x, v[k].y);
  }
  if (plane_mode != kPlanesOff) pc.store(f, plane_mode, p, t);
}

// The kPlanesStep schedule: only the flipped plane's pair is in B; the cached planes before it, the
// pair through the kernel's load(v, p) / finish(v, p), the cached planes after it.
template <int R, int L, class V, int NV, class Load, class Finish>
__device__ __forceinline__ void rowinv_planes_step(V (&v)[NV], float (&acc)[L], const PlaneCache<R, L>& pc,
                                                   const JobDesc& jb, int P, int t, Load&& load, Finish&& finish) {
  const int pa = jb.flip_plane & ~1;
  load(v, pa);
  __syncthreads();  // tw visible
#pragma unroll 1
  for (int q = 0; q < pa; ++q) pc.add_cached(acc, q, t);
  finish(v, pa);
  load(v, pa + 1);
  finish(v, pa + 1);
#pragma unroll 1
  for (int q = pa + 2; q < P; ++q) pc.add_cached(acc, q, t);
}

// The last pass's tail: plane mean, f64 partials of (I*T, I^2, T^2) against the target row,
// fixed-order reduction over the group's lanes and the block's rows.
//   SC1    write-through partials: k_rowinv_d<R, true> (the walk batch) alone
//   TPRE   the caller loaded the target row ahead: k_rowinv_d<32, false, true> alone
//   NTENV  the env-major intensity (inten_by_env) streams out non-temporal: every caller but the
//          N = 896 kernels, which reach it too (hbx_env_step's recon buffer) and keep their plain store
//   rc_pending / rc_cache  the fused reconcile: k_rowinv_d alone passes them (check_pass_call)
template <int R, int L, int GPB, bool SC1 = false, bool TPRE = false, bool NTENV = true>
__device__ __forceinline__ void rowinv_epilogue(float (&acc)[L], int P, int G, const JobDesc& jb, int j, int y,
                                                int rb, int grp, int t, const float* __restrict__ target,
                                                size_t tmask, float* __restrict__ inten_out, int inten_by_env,
                                                double* __restrict__ partial, double (&red)[GPB][3],
                                                const int32_t* __restrict__ rc_pending = nullptr,
                                                float* __restrict__ rc_cache = nullptr,
                                                const float* tpre = nullptr) {
  constexpr int N = R * L;
  constexpr int RB = N / GPB;
  const float invp = 1.0f / (float)P;
  // tmask = 0 points every row at the plan's zero row (no target): the loads
  // stay unconditional, so they issue early like the rest of the stream
  const float* trow = target + ((((size_t)jb.env * G + jb.group) * N + y) * N & tmask);
  double sxy = 0.0, sxx = 0.0, syy = 0.0;
#pragma unroll
  for (int k = 0; k < L; ++k) {
    const float I = acc[k] * invp;
    const float T = TPRE ? tpre[k] : trow[t + R * k];   // TPRE: the caller loaded the row ahead
    sxy = fma((double)I, (double)T, sxy);
    sxx = fma((double)I, (double)I, sxx);
    syy = fma((double)T, (double)T, syy);
    acc[k] = I;
  }
  if (inten_out) {
    const size_t slot = inten_by_env ? (size_t)jb.env * G + jb.group : (size_t)j;
    float* orow = inten_out + (slot * N + y) * N;
    if (rc_pending) {
      // (r04) the previous step's recon / intensity-cache reconcile of this env, fused here
      // instead of its own launch before the step (k_recon_reconcile): the previous step left
      // group gp's new intensity in recon only (p > 0, accepted: recon -> cache) or its stepped
      // intensity in recon (p < 0, rolled back: cache -> recon).  Row y of group gp is moved
      // by the lane group of row y; when gp is this step's group, an accepted row is read out
      // before this step overwrites it and a rolled-back one needs nothing.
      const int p = rc_pending[jb.env];
      if (p != 0) {
        const int gp = (p > 0 ? p : -p) - 1;
        const size_t grow = (((size_t)jb.env * G + gp) * N + y) * N;
        if (p > 0) {
#pragma unroll
          for (int k = 0; k < L; ++k) rc_cache[grow + t + R * k] = inten_out[grow + t + R * k];
        } else if (gp != jb.group) {
#pragma unroll
          for (int k = 0; k < L; ++k) inten_out[grow + t + R * k] = rc_cache[grow + t + R * k];
        }
      }
    }
    if (NTENV && inten_by_env) {
      // obs["recon_image"] (r05): streamed out non-temporal -- nothing on the device reads it
      // before the next step rewrites it (the settle copy at G > 1 takes the accepted half)
#pragma unroll
      for (int k = 0; k < L; ++k) __builtin_nontemporal_store(acc[k], orow + t + R * k);
    } else {
#pragma unroll
      for (int k = 0; k < L; ++k) orow[t + R * k] = acc[k];
    }
  }
  // reduce over the R lanes of the group, fixed order -> bitwise reproducible
#pragma unroll
  for (int off = R / 2; off >= 1; off >>= 1) {
    sxy += __shfl_xor(sxy, off, 64);
    sxx += __shfl_xor(sxx, off, 64);
    syy += __shfl_xor(syy, off, 64);
  }
  if (t == 0) { red[grp][0] = sxy; red[grp][1] = sxx; red[grp][2] = syy; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0, b = 0.0, cc = 0.0;
    for (int g = 0; g < GPB; ++g) { a += red[g][0]; b += red[g][1]; cc += red[g][2]; }
    double* o = partial + ((size_t)j * RB + rb) * 3;
    if constexpr (SC1) {   // read by the deciding workgroup of this launch (walk_planes_arrive)
      const __amdgpu_buffer_rsrc_t ro = walk_planes_rsrc(o, 24);
      __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, a), ro, 0, 0, kSc1Bit);
      __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, b), ro, 8, 0, kSc1Bit);
      __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, cc), ro, 16, 0, kSc1Bit);
    } else {
      o[0] = a; o[1] = b; o[2] = cc;
    }
  }
}

// rowinv_epilogue with a per-pixel loss weight (hbx_evaluate_pw / hbx_evaluate_stack_pw): the
// weight row of (env, group, y) is addressed as the target row, and the three f64 sums take it as
//   vI = (double)v (double)I, vT = (double)v (double)T      exact: 24 + 24 bits
//   sxy = fma(vI, T, sxy), sxx = fma(vI, I, sxx), syy = fma(vT, T, syy)
// in rowinv_epilogue's order -- over the lane's k, the group's lanes, the block's rows.  A pixel with v = 1
// adds rowinv_epilogue's term bit for bit, one with v = 0 leaves the running sums as they are (a finite
// I and T: 0 times inf is NaN).  The intensity written is the unweighted plane mean.  Always a target,
// job-major intensity rows, plain partials: no SC1, target-ahead, env-major or reconcile form.
template <int R, int L, int GPB>
__device__ __forceinline__ void rowinv_epilogue_pw(float (&acc)[L], int P, int G, const JobDesc& jb, int j, int y,
                                                   int rb, int grp, int t, const float* __restrict__ target,
                                                   const float* __restrict__ pixel_weight,
                                                   float* __restrict__ inten_out, double* __restrict__ partial,
                                                   double (&red)[GPB][3]) {
  constexpr int N = R * L;
  constexpr int RB = N / GPB;
  const float invp = 1.0f / (float)P;
  const size_t ro = (((size_t)jb.env * G + jb.group) * N + y) * N;
  const float* trow = target + ro;
  const float* vrow = pixel_weight + ro;
  double sxy = 0.0, sxx = 0.0, syy = 0.0;
#pragma unroll
  for (int k = 0; k < L; ++k) {
    const float I = acc[k] * invp;
    const float T = trow[t + R * k];
    const double v = (double)vrow[t + R * k];
    const double vI = v * (double)I, vT = v * (double)T;
    sxy = fma(vI, (double)T, sxy);
    sxx = fma(vI, (double)I, sxx);
    syy = fma(vT, (double)T, syy);
    acc[k] = I;
  }
  if (inten_out) {
    float* orow = inten_out + ((size_t)j * N + y) * N;
#pragma unroll
    for (int k = 0; k < L; ++k) orow[t + R * k] = acc[k];
  }
  // reduce over the R lanes of the group, fixed order -> bitwise reproducible
#pragma unroll
  for (int off = R / 2; off >= 1; off >>= 1) {
    sxy += __shfl_xor(sxy, off, 64);
    sxx += __shfl_xor(sxx, off, 64);
    syy += __shfl_xor(syy, off, 64);
  }
  if (t == 0) { red[grp][0] = sxy; red[grp][1] = sxx; red[grp][2] = syy; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0, b = 0.0, cc = 0.0;
    for (int g = 0; g < GPB; ++g) { a += red[g][0]; b += red[g][1]; cc += red[g][2]; }
    double* o = partial + ((size_t)j * RB + rb) * 3;
    o[0] = a; o[1] = b; o[2] = cc;
  }
}

// ---------------------------------------------------------------------------
// The last pass over an output window (hbx_*_window; WinRow, hbx_rowcol.hpp)
// ---------------------------------------------------------------------------
// a row block [y0, y0 + rows) that shares no row with the window: it has nothing to read from B
__device__ __forceinline__ bool rowinv_block_outside(const hbx_window_t& win, int y0, int rows) {
  return y0 + rows <= win.y0 || y0 >= win.y0 + win.h;
}

// plane_out without the plane cache: |U_p|^2 of every pixel into acc (the lanes outside the window carry
// theirs along unused), the field only inside the window, to the compact [env][G*P][h][w] field_out
template <int R, int L, class V, int NV>
__device__ __forceinline__ void plane_out_win(const V (&v)[NV], float (&acc)[L], const JobDesc& jb, int G, int P,
                                              int p, int y, const hbx_window_t& win, const WinRow& wr,
                                              float2* field_out) {
#pragma unroll
  for (int k = 0; k < L; ++k) acc[k] += fmaf(v[k].x, v[k].x, v[k].y * v[k].y);
  if (field_out) {
    float2* frow = field_out + WinRow::row_of(win, (size_t)jb.env * G * P + jb.group * P + p, y);
#pragma unroll
    for (int k = 0; k < L; ++k)
      if (wr.has(R * k)) frow[wr.xo + R * k] = make_float2(v[k].x, v[k].y);
  }
}

// One complex plane F_q out of the inverse row FFT of the complex last passes (k_rowinv_d_cplx, k_rowinv_cplx,
// k_rowinv896_cplx; v: natural layout, x = t + R k; V = pk2, or float2 at 896, stored as it is).  row0 = the
// lane's pixel x = t of row y of the group's complex plane 0 in an [env][G Q][N][N] array.
//   ST  (hbx_evaluate_complex) |F_q|^2 is also accumulated per pixel, acc += fmaf(re, re, im * im) as the
//       bit path's plane_out does; field_out and real_out may then both be null
//   GK = kGradNone   F_q to field_out and / or Re F_q to real_out, either nullable
//   GK = kGradPhase  (hbx_phase_backward) the plane is the gradient with respect to u = exp(i pi x): grad
//                    from the samples in `phase` (phase_grad_row) and nothing else
//   GK = kGradPhaseLevels  (hbx_phase_levels_backward) kGradPhase at the quantized samples; (ga, gb) = the
//                    quantizer's (h, s), which kGradPhase leaves unread (pass_grad_p0 / _p1)
//   GK = kGradSteWindow / kGradSteSigmoid  (hbx_threshold_backward) grad = gvb s(x) Re g for a binary
//                    hologram's real leaf x (in `phase`), s and (ga, gb) as ste_grad_row has them
//   WIN (hbx_backward_window; kGradNone and the two STE kinds, never ST) the one output, real_out or grad,
//       is compact over the window, [env][G Q][h][w], as are the leaf's samples (grad_row_win)
template <int R, int L, bool ST, int GK, bool WIN, class V, int NV>
__device__ __forceinline__ void cplx_plane_out(V (&v)[NV], float (&acc)[ST ? L : 1], int env, int group, int G,
                                               int Q, int q, int y, size_t row0, const hbx_window_t& win,
                                               const WinRow& wr, float2* field_out,
                                               float* real_out, const float* phase,
                                               float* grad, float gvb, float ga, float gb) {
  static_assert(!(ST && GK != kGradNone), "the gradient forms run no statistics");
  static_assert(!(WIN && (ST || GK == kGradPhase || GK == kGradPhaseLevels)), "windows: the real part or an STE gradient");
  constexpr int N = R * L;
  if constexpr (ST) {
#pragma unroll
    for (int k = 0; k < L; ++k) acc[k] += fmaf(v[k].x, v[k].x, v[k].y * v[k].y);
  }
  if constexpr (WIN) {
    const size_t ro = wr.in ? WinRow::row_of(win, ((size_t)env * G + group) * Q + q, y) : 0;
    grad_row_win<R, L, GK>(v, phase + ro, (GK == kGradNone ? real_out : grad) + ro, wr, gvb, ga, gb);
  } else {
    const size_t row = row0 + (size_t)q * N * N;
    if constexpr (GK == kGradPhase) {   // the samples are loaded behind the FFT: no second line is ever held
      phase_grad_row<R, L>(v, phase + row, grad + row);
    } else if constexpr (GK == kGradPhaseLevels) {
      phase_grad_row<R, L, kGradPhaseLevels>(v, phase + row, grad + row, ga, gb);
    } else if constexpr (GK != kGradNone) {
      ste_grad_row<R, L, GK>(v, phase + row, grad + row, gvb, ga, gb);
    } else {
      if (field_out) {
#pragma unroll
        for (int k = 0; k < L; ++k) {
          if constexpr (std::is_same<V, float2>::value) field_out[row + R * k] = v[k];
          else field_out[row + R * k] = from_pk(v[k]);
        }
      }
      if (real_out) {
#pragma unroll
        for (int k = 0; k < L; ++k) real_out[row + R * k] = v[k].x;
      }
    }
  }
}

// rowinv_epilogue over the window: the plane mean, the target row's loads, the job-major intensity
// stores and the f64 terms only for the pixels inside, in rowinv_epilogue's order -- over the lane's k,
// the group's lanes, the block's rows -- so the partials are its sums without the terms outside.  target
// and inten_out are compact, [env][G][h][w] and [job][h][w]; tmask = 0: the plan's zero row (w <= N).
template <int R, int L, int GPB>
__device__ __forceinline__ void rowinv_epilogue_win(float (&acc)[L], int P, int G, const JobDesc& jb, int j, int y,
                                                    int rb, int grp, int t, const float* __restrict__ target,
                                                    size_t tmask, float* __restrict__ inten_out,
                                                    double* __restrict__ partial, double (&red)[GPB][3],
                                                    const hbx_window_t& win, const WinRow& wr) {
  constexpr int N = R * L;
  constexpr int RB = N / GPB;
  const float invp = 1.0f / (float)P;
  const float* trow = target + ((wr.in ? WinRow::row_of(win, (size_t)jb.env * G + jb.group, y) : (size_t)0) & tmask);
  double sxy = 0.0, sxx = 0.0, syy = 0.0;
  float T[L];
#pragma unroll
  for (int k = 0; k < L; ++k) T[k] = wr.has(R * k) ? trow[wr.xo + R * k] : 0.0f;
#pragma unroll
  for (int k = 0; k < L; ++k) {
    const float I = acc[k] * invp;
    acc[k] = I;
    if (wr.has(R * k)) {
      sxy = fma((double)I, (double)T[k], sxy);
      sxx = fma((double)I, (double)I, sxx);
      syy = fma((double)T[k], (double)T[k], syy);
    }
  }
  if (inten_out && wr.in) {
    float* orow = inten_out + WinRow::row_of(win, (size_t)j, y);
#pragma unroll
    for (int k = 0; k < L; ++k)
      if (wr.has(R * k)) orow[wr.xo + R * k] = acc[k];
  }
  // reduce over the R lanes of the group, fixed order -> bitwise reproducible
#pragma unroll
  for (int off = R / 2; off >= 1; off >>= 1) {
    sxy += __shfl_xor(sxy, off, 64);
    sxx += __shfl_xor(sxx, off, 64);
    syy += __shfl_xor(syy, off, 64);
  }
  if (t == 0) { red[grp][0] = sxy; red[grp][1] = sxx; red[grp][2] = syy; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0, b = 0.0, cc = 0.0;
    for (int g = 0; g < GPB; ++g) { a += red[g][0]; b += red[g][1]; cc += red[g][2]; }
    double* o = partial + ((size_t)j * RB + rb) * 3;
    o[0] = a; o[1] = b; o[2] = cc;
  }
}

}  // namespace hbx
