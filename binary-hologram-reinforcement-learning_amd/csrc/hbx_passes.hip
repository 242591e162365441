// hbx_passes.hip -- the three propagation passes (gfx950, wave64).
//
// One "job" = one colour group (P planes, N x N) of one env, propagated with
// an optional single-pixel flip applied on the fly (env.py:164-172).  The
// intermediates are organised by spectral LINE kx (the N values over y), so
// the column pass streams whole lines and the two transposes a 2-D FFT needs
// live in LDS tiles of the row passes.  A is stored in panels of the row block
// height ([y / 8][kx][y % 8] at N = 1024: every k_rowfwd row block writes one
// contiguous 64-KB panel per plane pair); B in panels of 16 rows
// ([y / 16][kx][y % 16], hbx_internal.hpp), which gives
// the column pass 256-B pieces to write and the row inverse pass 128-B pieces
// to read (measured: 1-2 % over column-major B; 8-row panels made the column
// pass's scattered 64-B writes cost 1 ms).
//
//   k_rowfwd  GPB rows of a plane pair per block: bits -> one complex FFT per
//             row pair (plane a real, plane b imaginary) -> Hermitian split ->
//             half spectrum kx < N/2 (Nyquist packed in Im of kx = 0), stored doubled:
//             2 A, the split's 0.5 factors dropped (r06) and folded into htab = H / 2 ->
//             LDS tile transpose -> A panel y0 / GPB       [HBM: read N^2/8 B, write 4 N^2 B per plane]
//             (k_rowfwd32 at N = 1024.  k_rowfwd_real / k_rowfwd32_real read f32 samples instead of
//             bits; everything after the load -- FFT, split, tile, panel stores -- is one function
//             per size class, rowfwd_emit / rowfwd32_emit, called by the bit and the real kernel;
//             k_rowfwd_cplx / k_rowfwd32_cplx read complex64 samples, one complex plane per plane pair,
//             or f32 phase samples x that they turn into exp(i pi x) as they load them)
//   k_col2    one lane group per half-spectrum line kx: FFT over y -> x H and
//             x conj H (H is even in fx and ky) -> two IFFTs -> B lines kx
//             and N - kx (N/2 for kx = 0); buffer loads / stores with one
//             address VGPR per line; the next input line is prefetched under
//             the second IFFT                                    [read 4 N^2, write 8 N^2]
//   k_rowinv  GPB rows per block, all P planes: LDS tile transpose of the B
//             rows y0..y0+GPB (next plane's tile prefetched into registers
//             behind LDS-only barriers) -> IFFT over kx -> |U|^2 -> plane
//             mean -> f64 partials of (I*T, I^2, T^2) vs the target row   [read 8 N^2 per plane + 4 N^2]
//             (complex fields: k_rowinv_d_cplx / k_rowinv_cplx add B planes 2q and i * 2q + 1 on load,
//             one IFFT per complex plane, and store the field / its real part; their statistics
//             form, hbx_evaluate_complex, also sums |F_q|^2 and ends in the same plane mean and partials;
//             their gradient forms, hbx_phase_backward and hbx_threshold_backward, store dL/dx of a
//             phase leaf or of a binary hologram's real leaf instead of the plane)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hbx_fft.hpp"
#include "hbx_internal.hpp"
#include "hbx_rowcol.hpp"
#include "hbx_rowinv.hpp"
#include "hbx_walk_planes.hpp"

namespace hbx {

// Precision study (SURVEY 8d cfg 5, hbx_plan_set_precision): SK = HBX_PRECISION_BF16_STORE /
// _F16_STORE rounds every value written to the two pass intermediates (row spectrum,
// column-pass output) to bf16 / fp16, i.e. the numerics of half-width intermediate storage
// (the layout stays f32).  SK = HBX_PRECISION_F32 is the product path (no rounding code).
template <int SK>
__device__ __forceinline__ float2 store_round(float2 v) {
  if constexpr (SK == HBX_PRECISION_BF16_STORE) {
    auto r = [](float x) {
      uint32_t u = __float_as_uint(x);
      u += 0x7fffu + ((u >> 16) & 1u);   // round to nearest even
      return __uint_as_float(u & 0xffff0000u);
    };
    return make_float2(r(v.x), r(v.y));
  } else if constexpr (SK == HBX_PRECISION_F16_STORE) {
    return make_float2((float)(_Float16)v.x, (float)(_Float16)v.y);
  } else {
    return v;
  }
}

// The row passes' A stores: A is stored doubled (2 A, see htab), so the fp16 study rounds 0.5 v to
// fp16 and doubles it back -- the fp16 value of A itself (fp16 subnormals are not scale-invariant);
// bf16 shares f32's exponent range, where doubling commutes with rounding.
template <int SK>
__device__ __forceinline__ float2 store_round_a(float2 v) {
  if constexpr (SK == HBX_PRECISION_F16_STORE) {
    return make_float2(2.0f * (float)(_Float16)(0.5f * v.x), 2.0f * (float)(_Float16)(0.5f * v.y));
  } else {
    return store_round<SK>(v);
  }
}

// Threads per block of the row passes (row_nt, hbx_internal.hpp).  512-thread
// row blocks (16 rows) were measured slower at N = 1024 -- one 143-KB block per
// CU, whose barriers stall the whole CU: k_rowfwd 1.17 -> 1.54 ms, k_rowinv
// 2.01 -> 2.62 ms.
template <int R>
constexpr int kRowNT = row_nt(R);

// Intermediate layout (hbx_internal.hpp): panels of PAN = kRowNT / R rows, the
// row passes' block height.  A plane of L lines (L = N/2 for A, N for B) is
// N / PAN panels [L][PAN], element (line, y) at (y / PAN) * PS + line * PAN +
// y % PAN with PS = panel_stride(R, L).  A row block then writes (k_rowfwd)
// or reads (k_rowinv) ONE contiguous L * PAN * 8-B panel, while a column-pass
// lane group sees line kx as 64-B pieces of PAN consecutive y -- two adjacent
// lines per wave, so whole 128-B lines per wave instruction.
template <int R>
constexpr int kPanel = panel_rows(R);

template <int R>
using LayoutA = PanelLine<R, R * R / 2, pan_a(R)>;
template <int R>
using LayoutB = PanelLine<R, R * R, pan_b(R)>;

// B at N = 1024 and 256 (r03): tiles [y / 16][s / TL][16 rows][TL slots], TL = 256 / R
// (1 KB at N = 1024, 2 KB at N = 256), of the line SLOT
//   s(kx) = kx (kx <= N/2),  3N/2 - kx (kx > N/2),
// so the two output line sets of a k_col2 block -- its TL lines kx0 .. kx0 + TL - 1 and their
// mirrors N - kx0 - TL + 1 .. N - kx0 (N/2 for kx = 0) -- each fill one aligned tile, which
// the block writes as one contiguous run per 16-row band (staged through LDS), and a
// k_rowinv_d block reads 64-B (N = 1024) / 128-B (N = 256) runs per row straight into its
// FFT layout.  Replayed without arithmetic (tools/membw3.hip, N = 1024): k_col2's movement
// 2.39-2.43 ms (16-row panels 2.41-2.47), k_rowinv's 1.37-1.40 ms (1.62-1.65): DESIGN.md 4.
template <int R>
struct TileB {
  static constexpr int N = R * R, TL = 256 / R;
  __device__ static constexpr int at(int s, int y) {   // float2 offset of (slot s, row y)
    return (y >> 4) * 16 * N + (s / TL) * 16 * TL + (y & 15) * TL + s % TL;
  }
};
template <int R>
constexpr bool kTiledB = R == 32 || R == 16;



// ---------------------------------------------------------------------------
// Pass 1
// ---------------------------------------------------------------------------
// Row blocks per k_rowfwd workgroup (rowfwd_iters): a workgroup walks RIT
// consecutive row blocks of one plane pair, so the stores of block i stay in
// flight under the bit loads and row FFTs of block i + 1 (the next rows' mask
// words are prefetched before the stores are issued: vmcnt counts loads and
// stores in order, so waiting for them never waits for the stores).  With one
// row block per workgroup the load -> FFT -> LDS tile -> store chain of the
// two co-resident workgroups ran nearly serial.
template <int R>
constexpr int rowfwd_iters() { return pass_rowfwd_iters(R); }   // 4 / 2 / 1 (hbx_internal.hpp).  N = 256: 2 (r03,
// with nt A stores: 0.0634 -> 0.0585 ms; 4 row blocks 0.0611)

// The job of workgroup's job index j: jobs[j], or (actions non-null: the env step) decoded from
// actions[j] here, the workgroup with rbw = 0 of the job's first pair writing it to jobs[j] for
// the later passes and flagging an invalid action in *err
__device__ __forceinline__ JobDesc first_pass_job(const JobDesc* jobs, const int64_t* actions, int32_t* err,
                                                  int j, bool writer, int64_t hw, int P, int CH) {
  if (!actions) return jobs[j];
  const JobDesc jb = job_of_action(actions[j], j, hw, P, CH);
  if (writer && threadIdx.x == 0) {
    const_cast<JobDesc*>(jobs)[j] = jb;
    if (jb.env < 0 && err) atomicOr(err, 1);
  }
  return jb;
}

// float2 of LDS a row block of NT threads needs at N = R^2: the groups' padded FFT scratch, which
// the tile of both planes then reuses
template <int R, int NT>
constexpr int rowfwd_scratch() {
  static_assert(R * R * (NT / R) <= (NT / R) * R * (R + 1), "tile must fit in the scratch area");
  return (NT / R) * R * (R + 1);
}

// The N = 64 / 256 row block from "v holds the samples of row y0 + grp in planes pa (re), pb (im),
// lane t pixel x = t + R jj" to its panels stored: base = A plane pa of the job, lds the
// rowfwd_scratch float2, tw the staged twiddles.  Starts on the group's own scratch: the caller
// has seen every group leave the previous row block's tile.
template <int R, int NT, int SK>
__device__ __forceinline__ void rowfwd_emit(pk2 (&v)[R], int t, int grp, int lane_base, int y0, float2* lds,
                                            const float2* tw, float2* __restrict__ base) {
  constexpr int N = R * R;
  constexpr int GPB = NT / R;          // rows per row block
  constexpr size_t PLA = plane_a_elems(R);
  fft_group<R, false>(v, t, PaddedScratch<R>{lds + grp * R * (R + 1)}, tw);
  lds_barrier();    // every group is done with its scratch: reuse as the tile

  // Hermitian split -> tile[plane][kx][row]
  float2* tile = lds;
  const float2 zny = from_pk(v[R / 2]);  // Z[N/2] on lane 0
#pragma unroll
  for (int k2 = 0; k2 < R / 2; ++k2) {
    const float2 z = from_pk(v[k2]);
    const float2 m = mirror_conj<R>(v, k2, t, lane_base);
    float2 fa = make_float2(z.x + m.x, z.y + m.y);       // 2 A (htab holds H / 2)
    float2 fb = make_float2(z.y - m.y, m.x - z.x);
    if (k2 == 0 && t == 0) {  // DC and Nyquist of a real row are real
      fa = make_float2(z.x + z.x, zny.x + zny.x);
      fb = make_float2(z.y + z.y, zny.y + zny.y);
    }
    const int kx = t + R * k2;
    tile[tile_pos<R, GPB>(kx, grp)] = fa;
    tile[tile_pos<R, GPB>(N / 2 + kx, grp)] = fb;
  }
  lds_barrier();
  // store tile lines: A[pa|pb][kx][y0 .. y0+GPB), 16 B per thread per chunk
  constexpr int CHUNKS = N * GPB / 2;
  static_assert(CHUNKS % NT == 0, "chunking");
#pragma unroll
  for (int i = 0; i < CHUNKS / NT; ++i) {
    const int c = threadIdx.x + NT * i;
    const int r2 = (c % (GPB / 2)) * 2;
    const int line = c / (GPB / 2);  // pl * N/2 + kx : A planes pa, pb are adjacent
    float2 a, b;
    if constexpr (GPB == 16) {
      // (r05) rows r2, r2 + 1 sit in one aligned 16-B pair (the swizzle XORs whole pairs, its
      // bit 0 swaps the halves): one ds_read_b128 from a single lane base (the swizzle keys on
      // bits 0-4 of the line, which the chunk rounds i leave alone), conflict-free in the
      // 4 x 16-lane model; the two ds_read_b64 it replaces were 2-way (0.79 M extra LDS cycles
      // per 128-job launch at N = 256, profiles/r05/prof_mono_r05t); time unchanged (0.0587-0.0589
      // vs 0.0587-0.0588 ms, profiles/r05/rowfwd16_ab_r05u.txt)
      const int p0 = tile_pos<R, GPB>(line, r2);
      const float4 ab = *reinterpret_cast<const float4*>(tile + (p0 & ~1));
      const bool sw = (p0 & 1) != 0;
      a = sw ? make_float2(ab.z, ab.w) : make_float2(ab.x, ab.y);
      b = sw ? make_float2(ab.x, ab.y) : make_float2(ab.z, ab.w);
    } else {
      a = tile[tile_pos<R, GPB>(line, r2)];
      b = tile[tile_pos<R, GPB>(line, r2 + 1)];
    }
    a = store_round_a<SK>(a);
    b = store_round_a<SK>(b);
    const int pl = line / (N / 2);
    // panel layout: (line, y0 + r2) of plane pl -> contiguous 16-B chunks of the panel
    st_stream4(base + (size_t)pl * PLA + LayoutA<R>::at(line - pl * (N / 2), y0 + r2),
               make_float4(a.x, a.y, b.x, b.y));
  }
}

template <int R, int NT, int SK, int RIT = rowfwd_iters<R>()>
__global__ __launch_bounds__(NT, 512 / NT) void k_rowfwd(const JobDesc* jobs,
                                                   const uint32_t* __restrict__ mask,
                                                   float2* __restrict__ ws_a,
                                                   const float2* __restrict__ tw_glob, int P,
                                                   int CH, float va, float vb, int pair_step,
                                                   const int64_t* __restrict__ actions, int32_t* err,
                                                   const uint8_t* __restrict__ phase) {
  constexpr int N = R * R;
  constexpr int GPB = NT / R;          // rows per row block
  constexpr int WPR = N / 32;           // 32-bit mask words per row
  __shared__ float2 tw[N];
  __shared__ __attribute__((aligned(16))) float2 lds[rowfwd_scratch<R, NT>()];

  stage_twiddles<N, NT>(tw, tw_glob);

  const int grp = threadIdx.x / R;
  const int t = threadIdx.x % R;
  const int lane_base = (threadIdx.x & 63) - t;
  constexpr int RB = N / GPB;
  constexpr int RBW = RB / RIT;        // workgroups per plane pair
  // plane-cached step: only the flipped plane's pair
  const FirstPassBlock wg = first_pass_block<RBW>(RIT == 1 ? xcd_pair<RB>(blockIdx.x) : (int)blockIdx.x,
                                                  pair_step ? 1 : P / 2);
  const int rbw = wg.rbw, j = wg.j;
  const JobDesc jb = first_pass_job(jobs, actions, err, j, wg.writer, (int64_t)N * N, P, CH);
  if (jb.env < 0 || (phase && phase[j])) return;  // uniform per block (a walk slot whose A / B are kept)
  const int q = pair_step ? (jb.flip_plane >> 1) : wg.q;
  const int pa = 2 * q, pb = 2 * q + 1;
  const uint32_t* plane_a = mask + ((size_t)jb.env * CH + jb.group * P + pa) * N * WPR;
  uint32_t wa[WPR], wb[WPR];
  auto load_row = [&](int y) {
    const uint32_t* rowa = plane_a + (size_t)y * WPR;
    const uint32_t* rowb = rowa + (size_t)N * WPR;
    if constexpr (WPR % 4 == 0) {
#pragma unroll
      for (int i = 0; i < WPR / 4; ++i) {
        const uint4 a = reinterpret_cast<const uint4*>(rowa)[i];
        const uint4 b = reinterpret_cast<const uint4*>(rowb)[i];
        wa[4 * i] = a.x; wa[4 * i + 1] = a.y; wa[4 * i + 2] = a.z; wa[4 * i + 3] = a.w;
        wb[4 * i] = b.x; wb[4 * i + 1] = b.y; wb[4 * i + 2] = b.z; wb[4 * i + 3] = b.w;
      }
    } else {
#pragma unroll
      for (int i = 0; i < WPR; ++i) { wa[i] = rowa[i]; wb[i] = rowb[i]; }
    }
  };
  load_row(rbw * RIT * GPB + grp);
  __syncthreads();  // tw visible

  float2* base = ws_a + ((size_t)j * P + pa) * plane_a_elems(R);
  // RIT = 1: the loop condition is a constant and there is no loop.  Out of a loop of one row
  // block the compiler lifts rowfwd_emit's tile and panel addresses above the FFT (N = 256:
  // 84 VGPRs for 61, the small launch 1-3 % slower, profiles/rowfwd_dedup/small_launch_time.txt)
  int it = 0;
#pragma unroll 1
  do {
    const int y0 = (rbw * RIT + it) * GPB;
    const int y = y0 + grp;
    if (jb.flip_plane >= 0 && jb.flip_pix / N == y) {  // env.py:164 flip, on the fly
      const int col = jb.flip_pix % N;
      const uint32_t bit = 1u << (col & 31);
#pragma unroll
      for (int i = 0; i < WPR; ++i) {
        if (i == (col >> 5)) {
          if (jb.flip_plane == pa) wa[i] ^= bit;
          if (jb.flip_plane == pb) wb[i] ^= bit;
        }
      }
    }
    pk2 v[R];
    with_field_kind(va, vb, [&](auto fk) {
#pragma unroll
      for (int jj = 0; jj < R; ++jj) {
        const int w = (R * jj) >> 5;
        const int sh = ((R * jj) & 31) + t;
        v[jj] = (pk2){bit_value<fk()>(wa[w], sh, va, vb), bit_value<fk()>(wb[w], sh, va, vb)};
      }
    });
    if constexpr (RIT > 1) {
      // next rows' words (the last iteration re-reads its own row: no conditional load)
      load_row(it + 1 < RIT ? y + GPB : y);
      if (it > 0) lds_barrier();   // every group has read the previous tile: scratch reusable
    }
    rowfwd_emit<R, NT, SK>(v, t, grp, lane_base, y0, lds, tw, base);
  } while (RIT > 1 && ++it < RIT);
}

// k_rowfwd at N = 1024 with three workgroups per CU (the wide kernel above: 216 VGPRs,
// 75.8 KB LDS, two).  The pass is bound by how many row blocks' stores a CU keeps in
// flight, not by its arithmetic (the whole launch is ~75 us of VALU issue), so:
//  * lane t loads ONE mask word of its row per plane (word t) and a 32 x 32 bit
//    transpose across the group (five ds_swizzle levels) hands it bit t of every
//    word -- the 64 VGPRs of whole-row words the wide kernel keeps for its prefetch
//    are two here;
//  * the FFT transposes real and imaginary parts through a 4.2-KB float tile per
//    group (fft_group_split), and the Hermitian split goes out one plane at a time
//    through a 32-KB tile that aliases those FFT tiles: 8 KB twiddles + 33.8 KB.
// Same arithmetic as k_rowfwd, so the A it writes is bit-identical.
constexpr int kRowfwd32Scr = 8 * 32 * (32 + 1);          // floats: 8 FFT tiles
static_assert((1024 / 2) * 8 * 2 <= kRowfwd32Scr, "one plane's tile must fit in the FFT tiles");

// The N = 1024 row block from "v holds the samples of row y0 + grp in planes pa (re), pb (im), lane
// t pixel x = t + 32 jj" to its two panels stored: base = A plane pa of the job, lds the
// kRowfwd32Scr floats, tw the staged twiddles; k1 = mirror_k1(t).  Starts on the group's own FFT
// tile: the caller has seen every group leave the previous row block's tile.
template <int SK>
__device__ __forceinline__ void rowfwd32_emit(pk2 (&v)[32], int t, int k1, int grp, int y0, float* lds,
                                              const float2* tw, float2* __restrict__ base) {
  constexpr int R = 32, NT = 256, N = R * R, GPB = NT / R;
  constexpr size_t PLA = plane_a_elems(R);
  float2* tile = reinterpret_cast<float2*>(lds);
  // lane t now holds Z[k1 + 32 k2] (k1 = mirror_k1(t)): the mirror partner is lane t ^ 1
  fft_group_split_mirror<false>(v, t, k1, lds + grp * R * (R + 1), tw);

  // Hermitian split: plane a now, plane b kept in registers for the second tile
  float2 fb[R / 2];
  lds_barrier();    // every group is done with its FFT tile: reuse as the plane tile
  const float2 zny = from_pk(v[R / 2]);  // Z[N/2] on lane 0 (k1 = 0)
#pragma unroll
  for (int k2 = 0; k2 < R / 2; ++k2) {
    const float2 z = from_pk(v[k2]);
    const float2 m = mirror_conj_paired(v, k2, t);
    float2 fa = make_float2(z.x + m.x, z.y + m.y);       // 2 A (htab holds H / 2)
    fb[k2] = make_float2(z.y - m.y, m.x - z.x);
    if (k2 == 0 && t == 0) {  // DC and Nyquist of a real row are real
      fa = make_float2(z.x + z.x, zny.x + zny.x);
      fb[k2] = make_float2(z.y + z.y, zny.y + zny.y);
    }
    tile[tile_pos<R, GPB>(k1 + R * k2, grp)] = fa;
  }
  constexpr int CHUNKS = (N / 2) * GPB / 2;   // 16-B chunks of one plane's panel
  static_assert(CHUNKS % NT == 0, "chunking");
#pragma unroll
  for (int pl = 0; pl < 2; ++pl) {
    if (pl == 1) {
      lds_barrier();   // plane a's tile has been read
#pragma unroll
      for (int k2 = 0; k2 < R / 2; ++k2) tile[tile_pos<R, GPB>(k1 + R * k2, grp)] = fb[k2];
    }
    lds_barrier();
#pragma unroll
    for (int i = 0; i < CHUNKS / NT; ++i) {
      const int c = threadIdx.x + NT * i;
      const int r2 = (c % (GPB / 2)) * 2;
      const int line = c / (GPB / 2);
      const float2 a = store_round_a<SK>(tile[tile_pos<R, GPB>(line, r2)]);
      const float2 b = store_round_a<SK>(tile[tile_pos<R, GPB>(line, r2 + 1)]);
      st_stream4(base + (size_t)pl * PLA + LayoutA<R>::at(line, y0 + r2), make_float4(a.x, a.y, b.x, b.y));
    }
  }
}

template <int SK, int RIT = rowfwd_iters<32>()>
__global__ __launch_bounds__(256, 3) void k_rowfwd32(const JobDesc* jobs,
                                                     const uint32_t* __restrict__ mask,
                                                     float2* __restrict__ ws_a,
                                                     const float2* __restrict__ tw_glob, int P, int CH,
                                                     float va, float vb, int pair_step,
                                                     const int64_t* __restrict__ actions, int32_t* err,
                                                     const uint8_t* __restrict__ phase) {
  constexpr int R = 32, NT = 256, N = R * R;
  constexpr int GPB = NT / R;          // 8 rows per row block
  constexpr int WPR = N / 32;          // 32 mask words per row = one per lane
  __shared__ float2 tw[N];
  __shared__ __attribute__((aligned(16))) float lds[kRowfwd32Scr];

  stage_twiddles<N, NT>(tw, tw_glob);

  const int grp = threadIdx.x / R;
  const int t = threadIdx.x % R;
  const int k1 = mirror_k1(t);         // r05: the second FFT stage in mirror-paired lane order
  constexpr int RB = N / GPB;
  constexpr int RBW = RB / RIT;
  // first_pass_block written out: with the helper the pair index is formed ahead of the job load,
  // and the 12-job launch of k_rowfwd32<SK, 1> measured 95.1-97.1 us for 91.7-93.5
  // (profiles/rowfwd_dedup/small_launch_time.txt); this order measured 93.2-93.6
  int bid = RIT == 1 ? xcd_pair<RB>(blockIdx.x) : (int)blockIdx.x;
  const int rbw = bid % RBW;
  bid /= RBW;
  const int npair = pair_step ? 1 : P / 2;   // plane-cached step: only the flipped plane's pair
  const int j = bid / npair;
  const JobDesc jb = first_pass_job(jobs, actions, err, j, rbw == 0 && bid % npair == 0, (int64_t)N * N, P, CH);
  if (jb.env < 0 || (phase && phase[j])) return;  // uniform per block (a walk slot whose A / B are kept)
  const int q = pair_step ? (jb.flip_plane >> 1) : bid % npair;
  const int pa = 2 * q, pb = 2 * q + 1;
  const uint32_t* plane_a = mask + ((size_t)jb.env * CH + jb.group * P + pa) * N * WPR;
  uint32_t wa, wb;
  auto load_row = [&](int y) {
    wa = plane_a[(size_t)y * WPR + t];
    wb = plane_a[(size_t)(N + y) * WPR + t];
  };
  load_row(rbw * RIT * GPB + grp);
  __syncthreads();  // tw visible

  float2* base = ws_a + ((size_t)j * P + pa) * plane_a_elems(R);
  int it = 0;   // (RIT = 1: no loop, as k_rowfwd)
#pragma unroll 1
  do {
    const int y0 = (rbw * RIT + it) * GPB;
    const int y = y0 + grp;
    // bit r of ta / tb = pixel x = t + 32 r of the row
    uint32_t ta = group_bit_transpose(wa, t);
    uint32_t tb = group_bit_transpose(wb, t);
    if (jb.flip_plane >= 0 && jb.flip_pix / N == y) {  // env.py:164 flip, on the fly
      const int col = jb.flip_pix % N;
      if (t == (col & 31)) {
        if (jb.flip_plane == pa) ta ^= 1u << (col >> 5);
        if (jb.flip_plane == pb) tb ^= 1u << (col >> 5);
      }
    }
    pk2 v[R];
    with_field_kind(va, vb, [&](auto fk) {
#pragma unroll
      for (int jj = 0; jj < R; ++jj)
        v[jj] = (pk2){bit_value<fk()>(ta, jj, va, vb), bit_value<fk()>(tb, jj, va, vb)};
    });
    if constexpr (RIT > 1) {
      // next rows' words (the last iteration re-reads its own row: no conditional load)
      load_row(it + 1 < RIT ? y + GPB : y);
      if (it > 0) lds_barrier();   // every group has read the previous plane-b tile
    }
    rowfwd32_emit<SK>(v, t, k1, grp, y0, lds, tw, base);
  } while (RIT > 1 && ++it < RIT);
}

// ---------------------------------------------------------------------------
// Pass 1 on real-valued fields (hbx_simulate_real / hbx_propagate_real, ABI v15)
// ---------------------------------------------------------------------------
// values[env][CH][N][N] f32: real_load_row (hbx_rowcol.hpp) puts the samples of the row in planes
// pa, pb straight into the (re, im) of v, and rowfwd_emit / rowfwd32_emit -- the bit kernels' own
// row FFT, split, LDS tile and panel stores -- take it from there.  Full propagations
// only (no flip, no action decode, no pair step, no walk phase), f32 intermediates only.
// One row block per workgroup: the samples land in v itself, so a prefetch of the next row
// block would be a second v (64 VGPRs at N = 1024), which does not fit three workgroups per
// CU; the co-resident workgroups cover each other's loads instead.  This is the
// bit kernels' RIT = 1 form with another load, at every launch size (no small / large switch).
// LK and WIN: first_pass_load_real (hbx_rowcol.hpp); the registers, the tail and the geometry are the same
// for every load kind, and the A panel of every row is written whatever the window.
template <int R, int NT, int LK = kLoadReal, bool WIN = false>
__global__ __launch_bounds__(NT, 512 / NT) void k_rowfwd_real(const JobDesc* __restrict__ jobs,
                                                        const float* __restrict__ values,
                                                        float2* __restrict__ ws_a,
                                                        const float2* __restrict__ tw_glob, int P, int CH,
                                                        float thr, float lo, float hi, hbx_window_t win) {
  constexpr int N = R * R;
  constexpr int GPB = NT / R;          // rows per row block
  __shared__ float2 tw[N];
  __shared__ __attribute__((aligned(16))) float2 lds[rowfwd_scratch<R, NT>()];

  stage_twiddles<N, NT>(tw, tw_glob);

  const int grp = threadIdx.x / R;
  const int t = threadIdx.x % R;
  const int lane_base = (threadIdx.x & 63) - t;
  constexpr int RB = N / GPB;
  const FirstPassBlock wg = first_pass_block<RB>(xcd_pair<RB>(blockIdx.x), P / 2);
  const int j = wg.j;
  const JobDesc jb = jobs[j];
  if (jb.env < 0) return;  // uniform per block
  const int pa = 2 * wg.q;
  const int y0 = wg.rbw * GPB;
  const int y = y0 + grp;
  pk2 v[R];
  first_pass_load_real<R, R, LK, WIN>(v, values, jb.env, jb.group, P, CH, pa, y, t, thr, lo, hi, win);
  __syncthreads();  // tw visible

  float2* base = ws_a + ((size_t)j * P + pa) * plane_a_elems(R);
  rowfwd_emit<R, NT, HBX_PRECISION_F32>(v, t, grp, lane_base, y0, lds, tw, base);
}

// N = 1024: k_rowfwd32's three workgroups per CU (split FFT tiles, one plane's tile at a time;
// kLoadThreshold: profiles/binary_ste/resource_usage.txt)
template <int LK = kLoadReal, bool WIN = false>
__global__ __launch_bounds__(256, 3) void k_rowfwd32_real(const JobDesc* __restrict__ jobs,
                                                          const float* __restrict__ values,
                                                          float2* __restrict__ ws_a,
                                                          const float2* __restrict__ tw_glob, int P, int CH,
                                                          float thr, float lo, float hi, hbx_window_t win) {
  constexpr int R = 32, NT = 256, N = R * R;
  constexpr int GPB = NT / R;          // 8 rows per row block
  __shared__ float2 tw[N];
  __shared__ __attribute__((aligned(16))) float lds[kRowfwd32Scr];

  stage_twiddles<N, NT>(tw, tw_glob);

  const int grp = threadIdx.x / R;
  const int t = threadIdx.x % R;
  const int k1 = mirror_k1(t);         // the second FFT stage in mirror-paired lane order
  constexpr int RB = N / GPB;
  const FirstPassBlock wg = first_pass_block<RB>(xcd_pair<RB>(blockIdx.x), P / 2);
  const int j = wg.j;
  const JobDesc jb = jobs[j];
  if (jb.env < 0) return;  // uniform per block
  const int pa = 2 * wg.q;
  const int y0 = wg.rbw * GPB;
  const int y = y0 + grp;
  pk2 v[R];
  if constexpr (WIN) {
    // first_pass_load_real's window form, written out: through the helper this kernel compiles to two more
    // scalar instructions, and one of its timed medians lay outside the spread of the blocks before the change
    // (profiles/sample_passes/window_time_ab.txt)
    const WinRow wr(win, y, t);
    const size_t ro = wr.in ? WinRow::row_of(win, (size_t)jb.env * CH + jb.group * P + pa, y) : 0;
    real_load_row_win<R, R, LK>(v, values + ro, (size_t)win.h * win.w, wr, thr, lo, hi);
  } else {
    first_pass_load_real<R, R, LK, false>(v, values, jb.env, jb.group, P, CH, pa, y, t, thr, lo, hi, win);
  }
  __syncthreads();  // tw visible

  float2* base = ws_a + ((size_t)j * P + pa) * plane_a_elems(R);
  rowfwd32_emit<HBX_PRECISION_F32>(v, t, k1, grp, y0, lds, tw, base);
}

// ---------------------------------------------------------------------------
// Pass 1 on complex fields (hbx_simulate_complex)
// ---------------------------------------------------------------------------
// values[env][CH / 2][N][N] complex64: a job's group carries P / 2 complex planes, and complex plane
// q fills the plane-pair slot q of the workspace.  complex_load_row (hbx_rowcol.hpp) puts the row's
// samples into v as they are, and the shared tail does what it does for two real planes: the row
// FFT of u = a + i b, split into the half spectra of a = Re u (A plane 2q) and b = Im u (2q + 1).
// The real kernels' geometry: one row block per workgroup, wg.q = the complex plane.
// LK and WIN: first_pass_load_cplx (hbx_rowcol.hpp); a phase plane q fills plane-pair slot q as complex
// plane q does, and the tail and the geometry are the same for every load kind.
template <int R, int NT, int LK = kLoadComplex, bool WIN = false>
__global__ __launch_bounds__(NT, 512 / NT) void k_rowfwd_cplx(const JobDesc* __restrict__ jobs,
                                                        const float2* __restrict__ values,
                                                        float2* __restrict__ ws_a,
                                                        const float2* __restrict__ tw_glob, int P, int CH,
                                                        const float* __restrict__ weight, float scale,
                                                        const float* __restrict__ phase, hbx_window_t win) {
  constexpr int N = R * R;
  constexpr int GPB = NT / R;          // rows per row block
  __shared__ float2 tw[N];
  __shared__ __attribute__((aligned(16))) float2 lds[rowfwd_scratch<R, NT>()];

  stage_twiddles<N, NT>(tw, tw_glob);

  const int grp = threadIdx.x / R;
  const int t = threadIdx.x % R;
  const int lane_base = (threadIdx.x & 63) - t;
  constexpr int RB = N / GPB;
  const FirstPassBlock wg = first_pass_block<RB>(xcd_pair<RB>(blockIdx.x), P / 2);
  const int j = wg.j;
  const JobDesc jb = jobs[j];
  if (jb.env < 0) return;  // uniform per block
  const int y0 = wg.rbw * GPB;
  const int y = y0 + grp;
  pk2 v[R];
  first_pass_load_cplx<R, R, LK, WIN>(v, values, weight, scale, phase, jb.env, jb.group, P, CH, wg.q, y, t, win);
  __syncthreads();  // tw visible

  float2* base = ws_a + ((size_t)j * P + 2 * wg.q) * plane_a_elems(R);
  rowfwd_emit<R, NT, HBX_PRECISION_F32>(v, t, grp, lane_base, y0, lds, tw, base);
}

// N = 1024: k_rowfwd32's three workgroups per CU (kLoadWeighted: 111 VGPRs against 112, the weights die before the
// row FFT's temporaries are born; profiles/intensity_grad/resource_usage.txt; kLoadPhase:
// profiles/phase_field/resource_usage.txt)
template <int LK = kLoadComplex, bool WIN = false>
__global__ __launch_bounds__(256, 3) void k_rowfwd32_cplx(const JobDesc* __restrict__ jobs,
                                                          const float2* __restrict__ values,
                                                          float2* __restrict__ ws_a,
                                                          const float2* __restrict__ tw_glob, int P, int CH,
                                                          const float* __restrict__ weight, float scale,
                                                          const float* __restrict__ phase, hbx_window_t win) {
  constexpr int R = 32, NT = 256, N = R * R;
  constexpr int GPB = NT / R;          // 8 rows per row block
  __shared__ float2 tw[N];
  __shared__ __attribute__((aligned(16))) float lds[kRowfwd32Scr];

  stage_twiddles<N, NT>(tw, tw_glob);

  const int grp = threadIdx.x / R;
  const int t = threadIdx.x % R;
  const int k1 = mirror_k1(t);         // the second FFT stage in mirror-paired lane order
  constexpr int RB = N / GPB;
  const FirstPassBlock wg = first_pass_block<RB>(xcd_pair<RB>(blockIdx.x), P / 2);
  const int j = wg.j;
  const JobDesc jb = jobs[j];
  if (jb.env < 0) return;  // uniform per block
  const int y0 = wg.rbw * GPB;
  const int y = y0 + grp;
  pk2 v[R];
  first_pass_load_cplx<R, R, LK, WIN>(v, values, weight, scale, phase, jb.env, jb.group, P, CH, wg.q, y, t, win);
  __syncthreads();  // tw visible

  float2* base = ws_a + ((size_t)j * P + 2 * wg.q) * plane_a_elems(R);
  rowfwd32_emit<HBX_PRECISION_F32>(v, t, k1, grp, y0, lds, tw, base);
}

// ---------------------------------------------------------------------------
// Pass 2
// ---------------------------------------------------------------------------
// Column pass, one lane group per input line and both of its output lines:
// forward FFT over y -> Z; Z H and W = Z conj H from the same H(kx, .) row (H
// is even in fx and fy); inverse FFT of Z H -> B line kx.  H is even in ky, so
//   IFFT_y(M H)(y) = conj IFFT_y(Z conj H)(y),   M(ky) = conj Z(-ky),
// i.e. B line N - kx is the conjugate of the inverse FFT of W, formed in
// registers from the same H values (no LDS mirror of the line).  Only kx = 0 needs M itself
// ((Z + M)/2 and (Z - M)/2 are the transforms of the two real lines packed into
// A line 0: a register shuffle, mirror_conj; -> lines 0 and N/2).  One forward
// FFT per input line, one A read, one read of half the H row (N = 1024 / 256: H is even
// in ky, the other half comes mirrored through the group's scratch); the FFT and H hand-offs
// stay inside the group's own scratch (wave_sync only).  The next line's loads go into v
// as soon as line kx is stored and fly under the second inverse FFT.
// Scalar-f32 FFTs: with two lines in registers the packed variant spills.
// Measured and removed: the round-1 LDS mirror, packed DFTs,
// three workgroups per CU, H issued ahead, B panels of 8 / 32 / 64 rows.
//
// Lines per lane group.  Measured r03: N = 1024 ITER 2 / 4 / 8 = 2.94 / 2.72 / 2.76 ms (with the
// nt B stores, r03i: 2.82 / 2.58-2.60 / 2.68-2.70).  N = 256: ITER 4 = 0.152 ms, 2 = 0.144.  r03's
// ITER = 1 build wrote wrong B rows; the cause was the wide-store data hazard of the SGPR-soffset
// stage stores.  Rebuilt with the soffset-0 stores (r04) it is exact (the 256 flip
// map / mono / plane tests, profiles/r04/iter1_tests_r04b.txt) and no faster (0.1445-0.1447 ms vs
// 0.1432-0.1445 for ITER = 2, profiles/r04/iter1_ab_r04b.txt), so ITER = 2 stays; small launches
// use ITER = 1 (pass_launch_small, hbx_internal.hpp).
template <int R>
__host__ __device__ constexpr int col2_iters() { return pass_col2_iters(R); }   // 4 / 2 / 1

// N = 1024 / 256: the output line sets of a k_col2 block (TL lines: group g = slot g of
// slot tile st, TileB) go out through the FFT scratch.  col2_stage_write: each group
// writes its line (imaginary part times sy) into its OWN scratch region (the group's FFT
// is done with it; no block barrier), row y at col2_pos(g / 2, y).  After a block barrier,
// col2_stage_store: the block stores the set as 16-B chunks (slots 2 sp, 2 sp + 1 from
// regions 2 sp, 2 sp + 1) in memory order -- one contiguous run per 16-row band.
template <int R, int SK>
__device__ __forceinline__ void col2_stage_write(const float2 (&v)[R], float sy, float2* scratch, int grp, int t) {
  // row y = t + R k2: col2_pos only touches bits < 5, so rows R q apart with R q a multiple of
  // 32 share a lane base (constant offsets, the stores pair into ds_write2_b64)
  constexpr int PQ = R >= 32 ? 1 : 32 / R;
  float2* reg = col2_region<R>(scratch, grp);
  float2* base[PQ];
#pragma unroll
  for (int q = 0; q < PQ; ++q) base[q] = reg + col2_pos<R>(grp >> 1, t + R * q);
#pragma unroll
  for (int q = 0; q < PQ; ++q) {
#pragma unroll
    for (int k2 = q; k2 < R; k2 += PQ) base[q][R * (k2 - q)] = store_round<SK>(make_float2(v[k2].x, sy * v[k2].y));
  }
}

template <int R, int SK, int ITER = col2_iters<R>()>
__global__ __launch_bounds__(256, 2) void k_col2(const JobDesc* __restrict__ jobs,
                                                 const float2* __restrict__ ws_a,
                                                 float2* __restrict__ ws_b,
                                                 const float2* __restrict__ htab,
                                                 const float2* __restrict__ tw_glob, int P,
                                                 int pair_step, const uint8_t* __restrict__ phase) {
  constexpr int N = R * R;
  constexpr int GPB = 256 / R;          // lane groups (= input lines) per block iteration
  constexpr int LB = (N / 2) / (GPB * ITER);
  static_assert((N / 2) % (GPB * ITER) == 0, "line blocking");
  __shared__ float2 tw[N];
  constexpr int RS = kTiledB<R> ? col2_region_stride<R>() : R * (R + 1);   // per-group scratch region
  __shared__ float2 scratch[GPB * RS];

  for (int i = threadIdx.x; i < N; i += 256) tw[i] = tw_glob[i];

  const int grp = threadIdx.x / R;
  const int t = threadIdx.x % R;
  const int lane_base = (threadIdx.x & 63) - t;
  int bid = blockIdx.x;
  const int lb = bid % LB;
  bid /= LB;
  const int np = pair_step ? 2 : P;     // plane-cached step: the flipped plane's pair only
  const int j = bid / np;
  const JobDesc jb = jobs[j];
  if (jb.env < 0 || (phase && phase[j])) return;   // (a walk slot whose B is kept)
  const int p = pair_step ? (jb.flip_plane & ~1) + bid % 2 : bid % np;
  using PA = LayoutA<R>;   // A planes: N/2 lines
  using PB = LayoutB<R>;   // B planes: N lines
  const __amdgpu_buffer_rsrc_t ra = plane_rsrc(ws_a + ((size_t)j * P + p) * plane_a_elems(R), plane_a_elems(R) * 8);
  const __amdgpu_buffer_rsrc_t rb = plane_rsrc(ws_b + ((size_t)j * P + p) * plane_b_elems(R), plane_b_elems(R) * 8);
  // H rows of this group, natural [kx][ky]: element (kx, t + R k2) at (kx N + t) * 8 + k2 * R * 8
  const __amdgpu_buffer_rsrc_t rh = plane_rsrc(htab + (size_t)jb.group * (N / 2 + 1) * N, (N / 2 + 1) * N * 8);
  const PaddedScratch<R> sc{scratch + grp * RS};
  // the LB blocks of a plane run side by side: at iteration it they hold lines
  // it * LB * GPB + [0, LB * GPB), i.e. whole contiguous stretches of every panel
  constexpr int KSTEP = LB * GPB;
  const int kx0 = lb * GPB + grp;

  float2 v[R];
  {
    const int vo = PA::voff(t, kx0);
#pragma unroll
    for (int jj = 0; jj < R; ++jj) v[jj] = buf_ld2s(ra, vo, PA::joff(jj));
  }
  lds_barrier();  // tw visible (the line loads stay in flight)

#pragma unroll 1
  for (int it = 0; it < ITER; ++it) {
    const int kx = kx0 + it * KSTEP;
    const bool dc = (kx == 0);
    const int vh = (kx * N + t) * 8;
    // H(kx, .) of this line (N = 1024 / 256: the R/2 + 1 values of ky <= N/2 only, mirrored
    // below), issued before the second FFT stage so the loads fly under it
    constexpr int HP = kTiledB<R> ? R / 2 + 1 : 0;
    float2 hb[R];
    if constexpr (kTiledB<R>) {
      fft_group_s1<R, false, true>(v, t, tw);
      if (!dc) {
#pragma unroll
        for (int i = 0; i < HP; ++i) hb[i] = buf_ld2(rh, vh, i * R * 8);
      }
      if (it > 0) lds_barrier();   // the previous iteration's second set has been read out
      fft_group_s2<R, false, true>(v, t, sc);
    } else {
      fft_group<R, false, true>(v, t, sc, tw);
    }
    float2 w[R];
    if (!dc) {   // v <- Z H, w <- Z conj H
      if constexpr (kTiledB<R>) {
        // H(kx, N - ky) = H(kx, ky): lane t holds ky = t + R k2, whose mirror N - ky sits on
        // lane (R - t) mod R at k2' = R - 1 - k2 (lane 0: its own k2' = R - k2).  The group's
        // loads of k2 <= R/2 go through its FFT scratch (free between the forward and the
        // inverse FFT) and come back mirrored: 17 H loads per line instead of 32 at N = 1024,
        // k_col2 2.67 -> 2.58 ms
        float2* hs = scratch + grp * RS;
        wave_sync();
#pragma unroll
        for (int i = 0; i <= R / 2; ++i) hs[i * R + t] = hb[i];
        wave_sync();
        const float2* hm = hs + (t == 0 ? R : 0) + ((R - t) & (R - 1));
#pragma unroll
        for (int i = R / 2 + 1; i < R; ++i) hb[i] = hm[(R - 1 - i) * R];
        wave_sync();
      } else {
#pragma unroll
        for (int i = 0; i < R; ++i) hb[i] = buf_ld2(rh, vh, i * R * 8);
      }
#pragma unroll
      for (int i = 0; i < R; ++i) {
        w[i] = cmulc(v[i], hb[i]);
        v[i] = cmul(v[i], hb[i]);
      }
    } else {     // kx = 0: (Z + M)/2 H(0) -> line 0, -i (Z - M)/2 H(N/2) -> line N/2
      const int vn = ((N / 2) * N + t) * 8;
#pragma unroll
      for (int k2 = 0; k2 < R; ++k2) w[k2] = mirror_conj<R>(v, k2, t, lane_base);
#pragma unroll
      for (int k2 = 0; k2 < R; ++k2) {
        const float2 z = v[k2], mm = w[k2];
        v[k2] = cmul(make_float2(0.5f * (z.x + mm.x), 0.5f * (z.y + mm.y)), buf_ld2(rh, vh, k2 * R * 8));
        w[k2] = cmul(make_float2(0.5f * (z.y - mm.y), -0.5f * (z.x - mm.x)), buf_ld2(rh, vn, k2 * R * 8));
      }
    }
    fft_group<R, true, true>(v, t, sc, tw);
    const float sy = dc ? 1.0f : -1.0f;   // line N - kx = conj IFFT(W)
    if constexpr (kTiledB<R>) {
      const int kxb = kx - grp;            // the block's GPB lines: slot tile kxb / GPB
      col2_stage_write<R, SK>(v, 1.0f, scratch, grp, t);
      lds_barrier();
      col2_stage_store<R>(scratch, rb, kxb / GPB);
      if (it + 1 < ITER) {  // next line in flight under the second inverse FFT
        const int vo = PA::voff(t, kx + KSTEP);
#pragma unroll
        for (int jj = 0; jj < R; ++jj) v[jj] = buf_ld2s(ra, vo, PA::joff(jj));
      }
      fft_group_s1<R, true, true>(w, t, tw);
      lds_barrier();   // the first set has been read out: the regions are the FFTs' again
      fft_group_s2<R, true, true>(w, t, sc);
      col2_stage_write<R, SK>(w, sy, scratch, grp, t);
      lds_barrier();
      col2_stage_store<R>(scratch, rb, (N / 2 + kxb) / GPB);
    } else {
      {
        const int vo = PB::voff(t, kx);
#pragma unroll
        for (int k2 = 0; k2 < R; ++k2) buf_st2s(store_round<SK>(v[k2]), rb, vo, PB::joff(k2));
      }
      if (it + 1 < ITER) {  // next line in flight under the second inverse FFT
        const int vo = PA::voff(t, kx + KSTEP);
#pragma unroll
        for (int jj = 0; jj < R; ++jj) v[jj] = buf_ld2s(ra, vo, PA::joff(jj));
      }
      fft_group<R, true, true>(w, t, sc, tw);
      {
        const int vo = PB::voff(t, dc ? N / 2 : N - kx);
#pragma unroll
        for (int k2 = 0; k2 < R; ++k2)
          buf_st2s(store_round<SK>(make_float2(w[k2].x, sy * w[k2].y)), rb, vo, PB::joff(k2));
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Pass 3
// ---------------------------------------------------------------------------
// The tail (rowinv_epilogue), the lane bases of the direct loads (RowinvLanes), the plane cache and the
// other pieces shared with the N = 896 kernels are in hbx_rowinv.hpp.

// WIN (hbx_evaluate_real_window / _threshold_window; off by default, and the kernels without it compile as
// before): target [env][G][h][w], inten_out [job][h][w] and field_out [env][G*P][h][w] are compact arrays
// over the output window win.  A row block that shares no row with it writes neutral partials and reads
// nothing from B; the others run every row's FFTs and store, reduce and load the target only inside
// (plane_out_win, rowinv_epilogue_win).  No plane cache, reconcile or walk; LEAN: no field code.
template <int R, bool WALK = false, bool LEAN = false, bool WIN = false>
__global__ __launch_bounds__(256, 2) void k_rowinv_d(const JobDesc* __restrict__ jobs,
                                                     const float2* __restrict__ ws_b,
                                                     const float* __restrict__ target,
                                                     const float2* __restrict__ tw_glob, int P, int G,
                                                     double* __restrict__ partial, float* __restrict__ inten_out,
                                                     float2* __restrict__ field_out, size_t tmask, int inten_by_env,
                                                     int plane_mode, float* __restrict__ plane_pool,
                                                     const int32_t* __restrict__ plane_slot, int plane_spares,
                                                     int spare_base, const int32_t* __restrict__ rc_pending,
                                                     float* __restrict__ rc_cache, WalkPlanesArgs wk,
                                                     hbx_window_t win) {
  constexpr int N = R * R, GPB = 256 / R, RB = N / GPB;
  static_assert(!(WIN && WALK), "a walk batch is not windowed");
  static_assert(!WALK || walk_planes_lds_bytes(RB) <= GPB * R * (R + 1) * 8, "the decision's LDS fits the scratch");
  __shared__ float2 tw[N];
  __shared__ float2 scratch[GPB * R * (R + 1)];
  __shared__ double red[GPB][3];
  for (int i = threadIdx.x; i < N; i += 256) tw[i] = tw_glob[i];

  const int grp = threadIdx.x / R;
  const int t = threadIdx.x % R;
  const int bid = xcd_pair<RB>(blockIdx.x);
  const int rb = bid % RB;
  const int j = bid / RB;
  const JobDesc jb = jobs[j];
  if constexpr (WALK) {
    if (wk.phase && wk.phase[j] == 2) {   // (r06) a kept walk slot: its partials and fresh pair stand
      walk_planes_arrive(wk, reinterpret_cast<char*>(scratch));
      return;
    }
  }
  if (jb.env < 0) {
    rowinv_zero_partial<WALK>(partial, j, RB, rb);
    if constexpr (WALK) walk_planes_arrive(wk, reinterpret_cast<char*>(scratch));
    return;
  }
  if constexpr (LEAN) {   // the plain FFT-mode launch: no plane cache, field, reconcile or walk code
    plane_mode = kPlanesOff;
    field_out = nullptr;
    rc_pending = nullptr;
    rc_cache = nullptr;
  }
  if constexpr (WIN) {
    if (rowinv_block_outside(win, rb * GPB, GPB)) {   // uniform per block
      rowinv_zero_partial(partial, j, RB, rb);
      return;
    }
    plane_mode = kPlanesOff;
    rc_pending = nullptr;
    rc_cache = nullptr;
  }
  const int y = rb * GPB + grp;
  constexpr int PLB = N * N;                 // float2 per B plane
  const __amdgpu_buffer_rsrc_t rs = plane_rsrc(ws_b + (size_t)j * P * PLB, (unsigned)((size_t)P * PLB * 8));
  const RowinvLanes<R> ln(y, t);
  auto load_plane = [&](pk2 (&v)[R], int p) { rowinv_load_plane(v, ln, rs, p); };
  float acc[R];
#pragma unroll
  for (int k = 0; k < R; ++k) acc[k] = 0.0f;
  const PaddedScratch<R> sc{scratch + grp * R * (R + 1)};
  const PlaneCache<R> pc(jb, j, y, G, P, plane_spares, spare_base, plane_pool, plane_slot);
  const WinRow wr(win, y, t);   // (WIN alone reads it)
  auto finish_plane = [&](pk2 (&v)[R], int p) {
    fft_group<R, true>(v, t, sc, tw);
    if constexpr (WIN) plane_out_win<R, R>(v, acc, jb, G, P, p, y, win, wr, field_out);
    else plane_out<R, R>(v, acc, pc, jb, G, P, p, t, field_out, plane_mode);
  };
  pk2 va[R];
  if (plane_mode == kPlanesStep) {   // only the flipped plane's pair is in B
    rowinv_planes_step(va, acc, pc, jb, P, t, load_plane, finish_plane);
    rowinv_epilogue<R, R, GPB, WALK>(acc, P, G, jb, j, y, rb, grp, t, target, tmask, inten_out, inten_by_env, partial,
                                     red, rc_pending, rc_cache);
    if constexpr (WALK) {
      __syncthreads();   // every group is done with its scratch region: the decision's LDS
      walk_planes_arrive(wk, reinterpret_cast<char*>(scratch));
    }
    return;
  }
  load_plane(va, 0);
  __syncthreads();  // tw visible
  if constexpr (R == 16) {   // N = 256: registers to spare -- the next plane in flight under this one's FFT
    pk2 vb[R];
#pragma unroll 1
    for (int p = 0; p < P; p += 2) {         // P is even (hbx_plan_create)
      load_plane(vb, p + 1);
      finish_plane(va, p);
      load_plane(va, p + 2 < P ? p + 2 : p + 1);
      finish_plane(vb, p + 1);
    }
  } else if constexpr (LEAN && !WIN) {
    // (r06) the last plane peeled: its FFT runs with the target row's loads in flight instead of a
    // re-read of plane P - 1 (the loads the tail waited for; 32 more VGPRs fit the lean kernel)
#pragma unroll 1
    for (int p = 0; p < P - 1; ++p) {
      finish_plane(va, p);
      load_plane(va, p + 1);
    }
    const float* trow = target + ((((size_t)jb.env * G + jb.group) * N + y) * N & tmask);
    float tv[R];
#pragma unroll
    for (int k = 0; k < R; ++k) tv[k] = trow[t + R * k];
    finish_plane(va, P - 1);
    rowinv_epilogue<R, R, GPB, false, true>(acc, P, G, jb, j, y, rb, grp, t, target, tmask, inten_out, inten_by_env,
                                            partial, red, rc_pending, rc_cache, tv);
    return;
  } else {
#pragma unroll 1
    for (int p = 0; p < P; ++p) {
      finish_plane(va, p);
      load_plane(va, p + 1 < P ? p + 1 : p);   // unconditional: the last round re-reads plane P - 1
    }
  }
  if constexpr (WIN)
    rowinv_epilogue_win<R, R, GPB>(acc, P, G, jb, j, y, rb, grp, t, target, tmask, inten_out, partial, red, win, wr);
  else
    rowinv_epilogue<R, R, GPB>(acc, P, G, jb, j, y, rb, grp, t, target, tmask, inten_out, inten_by_env, partial, red,
                                rc_pending, rc_cache);
}

// WIN: as k_rowinv_d's
template <int R, int NT, bool WIN = false>
__global__ __launch_bounds__(NT, 512 / NT) void k_rowinv(const JobDesc* __restrict__ jobs,
                                                   const float2* __restrict__ ws_b,
                                                   const float* __restrict__ target,
                                                   const float2* __restrict__ tw_glob, int P,
                                                   int G, double* __restrict__ partial,
                                                   float* __restrict__ inten_out,
                                                   float2* __restrict__ field_out,
                                                   size_t tmask, int inten_by_env, hbx_window_t win) {
  constexpr int N = R * R;
  constexpr int GPB = NT / R;          // rows per block
  constexpr int RB = N / GPB;
  constexpr int CH16 = N * GPB / 2;     // 16-B chunks per plane tile
  constexpr int PER = CH16 / NT;
  static_assert(CH16 % NT == 0, "chunking");
  constexpr int SCR = GPB * R * (R + 1);   // padded transpose scratch reuses the tile
  __shared__ float2 tw[N];
  __shared__ __attribute__((aligned(16))) float2 tile[SCR > N * GPB ? SCR : N * GPB];
  __shared__ double red[GPB][3];

  for (int i = threadIdx.x; i < N; i += NT) tw[i] = tw_glob[i];

  const int grp = threadIdx.x / R;
  const int t = threadIdx.x % R;
  const int bid = xcd_pair<RB>(blockIdx.x);
  const int rb = bid % RB;
  const int j = bid / RB;
  const JobDesc jb = jobs[j];
  if (jb.env < 0) {
    rowinv_zero_partial(partial, j, RB, rb);
    return;
  }
  const int y0 = rb * GPB;
  const int y = y0 + grp;
  if constexpr (WIN) {
    if (rowinv_block_outside(win, y0, GPB)) {   // uniform per block
      rowinv_zero_partial(partial, j, RB, rb);
      return;
    }
  }
  const WinRow wr(win, y, t);   // (WIN alone reads it)
  constexpr size_t PLB = plane_b_elems(R);
  const float2* jbase = ws_b + (size_t)j * P * PLB;

  float4 pre[PER];   // this thread's share of a plane tile, one plane ahead
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const TileChunk ch = tile_chunk<NT, GPB>(i);
    pre[i] = ld_stream4(jbase + LayoutB<R>::at(ch.line, y0 + ch.r2));
  }
  float acc[R];
#pragma unroll
  for (int k = 0; k < R; ++k) acc[k] = 0.0f;

#pragma unroll 1
  for (int p = 0; p < P; ++p) {
    lds_barrier();  // previous plane's scratch use is over (also publishes tw)
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const TileChunk ch = tile_chunk<NT, GPB>(i);
      tile[tile_pos<R, GPB>(ch.line, ch.r2)] = make_float2(pre[i].x, pre[i].y);
      tile[tile_pos<R, GPB>(ch.line, ch.r2 + 1)] = make_float2(pre[i].z, pre[i].w);
    }
    if (p + 1 < P) {  // next plane's tile in flight under this plane's FFT
      const float2* nb = jbase + (size_t)(p + 1) * PLB;
#pragma unroll
      for (int i = 0; i < PER; ++i) {
        const TileChunk ch = tile_chunk<NT, GPB>(i);
        pre[i] = ld_stream4(nb + LayoutB<R>::at(ch.line, y0 + ch.r2));
      }
    }
    lds_barrier();
    pk2 v[R];
#pragma unroll
    for (int jj = 0; jj < R; ++jj) v[jj] = to_pk(tile[tile_pos<R, GPB>(t + R * jj, grp)]);
    lds_barrier();  // tile consumed: reuse it as transpose scratch
    fft_group<R, true>(v, t, PaddedScratch<R>{tile + grp * R * (R + 1)}, tw);
    if constexpr (WIN) {
      plane_out_win<R, R>(v, acc, jb, G, P, p, y, win, wr, field_out);
      continue;
    }
#pragma unroll
    for (int k = 0; k < R; ++k) acc[k] += fmaf(v[k].x, v[k].x, v[k].y * v[k].y);
    if (field_out) {  // exact field of this plane (incremental mode init / refresh)
      float2* frow = field_out + (((size_t)jb.env * G * P + jb.group * P + p) * N + y) * N;
#pragma unroll
      for (int k = 0; k < R; ++k) frow[t + R * k] = from_pk(v[k]);
    }
  }

  if constexpr (WIN)
    rowinv_epilogue_win<R, R, GPB>(acc, P, G, jb, j, y, rb, grp, t, target, tmask, inten_out, partial, red, win, wr);
  else
    rowinv_epilogue<R, R, GPB>(acc, P, G, jb, j, y, rb, grp, t, target, tmask, inten_out, inten_by_env, partial, red);
}

// ---------------------------------------------------------------------------
// Pass 3 on complex fields (hbx_simulate_complex): recombine a plane pair
// ---------------------------------------------------------------------------
// After k_col2, B planes 2q and 2q + 1 of a job hold the column-pass output of a = Re u_q and
// b = Im u_q, and the propagated plane is F_q = F[a] + i F[b].  The inverse row FFT is linear, so
// the pair is combined on load, v = B[2q] + i B[2q + 1], and ONE inverse FFT per complex plane gives
// F_q, stored once: 8 N^2 bytes to field and / or 4 N^2 bytes of Re F_q to real_part (both
// [env][CH / 2][N][N], either nullable).  No |.|^2, partials, plane cache or reconcile.
// What happens to a plane after its inverse FFT is cplx_plane_out (hbx_rowinv.hpp: ST, GK and WIN, off by
// default, and the kernels without them compile as before).  ST (hbx_evaluate_complex) also runs k_rowinv's
// tail (rowinv_epilogue) with Q = P / 2 as the plane count: the plane-mean intensity row to inten_out
// [job][N][N], the f64 partials against the target row (tmask = 0: the zero row).
//
// N = 1024 / 256: k_rowinv_d's direct loads from the tiled B (RowinvLanes).
// Plane 2q + 1 arrives in two halves of R / 2 values that are folded into v as they land, so the
// kernel never holds two whole lines (the second register set that cost k_rowinv_d its second
// block per CU).  N = 256 has the registers for a second line and keeps the next pair in flight
// under this one's FFT, as k_rowinv_d does with the next plane.
// WIN: a row block that shares no row with win reads nothing.
template <int R, bool ST = false, int GK = kGradNone, bool WIN = false>
__global__ __launch_bounds__(256, 2) void k_rowinv_d_cplx(const JobDesc* __restrict__ jobs,
                                                          const float2* __restrict__ ws_b,
                                                          const float2* __restrict__ tw_glob, int P, int G,
                                                          float2* __restrict__ field_out,
                                                          float* __restrict__ real_out,
                                                          const float* __restrict__ target, size_t tmask,
                                                          double* __restrict__ partial,
                                                          float* __restrict__ inten_out,
                                                          const float* __restrict__ phase,
                                                          float* __restrict__ grad, float gvb, float ga,
                                                          float gb, hbx_window_t win) {
  constexpr int N = R * R, GPB = 256 / R, RB = N / GPB;
  __shared__ float2 tw[N];
  __shared__ float2 scratch[GPB * R * (R + 1)];
  for (int i = threadIdx.x; i < N; i += 256) tw[i] = tw_glob[i];

  const int grp = threadIdx.x / R;
  const int t = threadIdx.x % R;
  const int bid = xcd_pair<RB>(blockIdx.x);
  const int rb = bid % RB;
  const int j = bid / RB;
  const JobDesc jb = jobs[j];
  if (jb.env < 0) {  // uniform per block
    if constexpr (ST) rowinv_zero_partial(partial, j, RB, rb);
    return;
  }
  if constexpr (WIN) {
    if (rowinv_block_outside(win, rb * GPB, GPB)) return;   // uniform per block
  }
  const int y = rb * GPB + grp;
  const WinRow wr(win, y, t);   // (WIN alone reads it)
  const int Q = P / 2;                        // complex planes per group
  constexpr int PLB = N * N;                 // float2 per B plane
  const __amdgpu_buffer_rsrc_t rs = plane_rsrc(ws_b + (size_t)j * P * PLB, (unsigned)((size_t)P * PLB * 8));
  const RowinvLanes<R> ln(y, t);
  auto load_pair = [&](pk2 (&v)[R], int q) { rowinv_load_pair(v, ln, rs, q); };
  const PaddedScratch<R> sc{scratch + grp * R * (R + 1)};
  const size_t row0 = (((size_t)jb.env * G + jb.group) * Q * N + y) * N + t;   // complex plane 0, pixel x = t
  float acc[ST ? R : 1];
  if constexpr (ST) {
#pragma unroll
    for (int k = 0; k < R; ++k) acc[k] = 0.0f;
  }
  auto finish_plane = [&](pk2 (&v)[R], int q) {
    fft_group<R, true>(v, t, sc, tw);
    cplx_plane_out<R, R, ST, GK, WIN>(v, acc, jb.env, jb.group, G, Q, q, y, row0, win, wr, field_out, real_out, phase,
                                      grad, gvb, ga, gb);
  };
  pk2 va[R];
  load_pair(va, 0);
  __syncthreads();  // tw visible
  if constexpr (R == 16) {
    pk2 vb[R];
#pragma unroll 1
    for (int q = 0; q < Q; q += 2) {
      if (q + 1 < Q) load_pair(vb, q + 1);
      finish_plane(va, q);
      if (q + 1 < Q) {
        if (q + 2 < Q) load_pair(va, q + 2);
        finish_plane(vb, q + 1);
      }
    }
  } else {
#pragma unroll 1
    for (int q = 0; q < Q; ++q) {
      finish_plane(va, q);
      if (q + 1 < Q) load_pair(va, q + 1);   // uniform: no pair is read twice
    }
  }
  if constexpr (ST) {
    __shared__ double red[GPB][3];
    rowinv_epilogue<R, R, GPB>(acc, Q, G, jb, j, y, rb, grp, t, target, tmask, inten_out, 0, partial, red);
  }
}

// N = 64: k_rowinv's LDS tile transpose; both planes' shares of the tile are prefetched one pair
// ahead and combined as they are written into the tile.
template <int R, int NT, bool ST = false, int GK = kGradNone, bool WIN = false>
__global__ __launch_bounds__(NT, 512 / NT) void k_rowinv_cplx(const JobDesc* __restrict__ jobs,
                                                        const float2* __restrict__ ws_b,
                                                        const float2* __restrict__ tw_glob, int P, int G,
                                                        float2* __restrict__ field_out,
                                                        float* __restrict__ real_out,
                                                        const float* __restrict__ target, size_t tmask,
                                                        double* __restrict__ partial,
                                                        float* __restrict__ inten_out,
                                                        const float* __restrict__ phase,
                                                        float* __restrict__ grad, float gvb, float ga,
                                                        float gb, hbx_window_t win) {
  constexpr int N = R * R;
  constexpr int GPB = NT / R;          // rows per block
  constexpr int RB = N / GPB;
  constexpr int CH16 = N * GPB / 2;     // 16-B chunks per plane tile
  constexpr int PER = CH16 / NT;
  static_assert(CH16 % NT == 0, "chunking");
  constexpr int SCR = GPB * R * (R + 1);   // padded transpose scratch reuses the tile
  __shared__ float2 tw[N];
  __shared__ __attribute__((aligned(16))) float2 tile[SCR > N * GPB ? SCR : N * GPB];

  for (int i = threadIdx.x; i < N; i += NT) tw[i] = tw_glob[i];

  const int grp = threadIdx.x / R;
  const int t = threadIdx.x % R;
  const int bid = xcd_pair<RB>(blockIdx.x);
  const int rb = bid % RB;
  const int j = bid / RB;
  const JobDesc jb = jobs[j];
  if (jb.env < 0) {  // uniform per block
    if constexpr (ST) rowinv_zero_partial(partial, j, RB, rb);
    return;
  }
  const int y0 = rb * GPB;
  const int y = y0 + grp;
  if constexpr (WIN) {
    if (rowinv_block_outside(win, y0, GPB)) return;   // uniform per block
  }
  const WinRow wr(win, y, t);   // (WIN alone reads it)
  const int Q = P / 2;
  constexpr size_t PLB = plane_b_elems(R);
  const float2* jbase = ws_b + (size_t)j * P * PLB;

  float4 pa[PER], pb[PER];   // this thread's share of the pair's two plane tiles, one pair ahead
  auto load_pair = [&](int q) {
    const float2* a = jbase + (size_t)(2 * q) * PLB;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const TileChunk ch = tile_chunk<NT, GPB>(i);
      pa[i] = ld_stream4(a + LayoutB<R>::at(ch.line, y0 + ch.r2));
      pb[i] = ld_stream4(a + PLB + LayoutB<R>::at(ch.line, y0 + ch.r2));
    }
  };
  load_pair(0);
  const size_t row0 = (((size_t)jb.env * G + jb.group) * Q * N + y) * N + t;
  float acc[ST ? R : 1];
  if constexpr (ST) {
#pragma unroll
    for (int k = 0; k < R; ++k) acc[k] = 0.0f;
  }

#pragma unroll 1
  for (int q = 0; q < Q; ++q) {
    lds_barrier();  // previous plane's scratch use is over (also publishes tw)
#pragma unroll
    for (int i = 0; i < PER; ++i) {   // B[2q] + i B[2q + 1]
      const TileChunk ch = tile_chunk<NT, GPB>(i);
      tile[tile_pos<R, GPB>(ch.line, ch.r2)] = make_float2(pa[i].x - pb[i].y, pa[i].y + pb[i].x);
      tile[tile_pos<R, GPB>(ch.line, ch.r2 + 1)] = make_float2(pa[i].z - pb[i].w, pa[i].w + pb[i].z);
    }
    if (q + 1 < Q) load_pair(q + 1);   // next pair's tiles in flight under this plane's FFT
    lds_barrier();
    pk2 v[R];
#pragma unroll
    for (int jj = 0; jj < R; ++jj) v[jj] = to_pk(tile[tile_pos<R, GPB>(t + R * jj, grp)]);
    lds_barrier();  // tile consumed: reuse it as transpose scratch
    fft_group<R, true>(v, t, PaddedScratch<R>{tile + grp * R * (R + 1)}, tw);
    if constexpr (GK == kGradNone && !WIN) {
      // cplx_plane_out's full-grid field / real-part form, written out: its null tests and stores on the
      // kernel's own pointers compile to other code here when they come through the helper
      if constexpr (ST) {
#pragma unroll
        for (int k = 0; k < R; ++k) acc[k] += fmaf(v[k].x, v[k].x, v[k].y * v[k].y);
      }
      const size_t row = row0 + (size_t)q * N * N;
      if (field_out) {
#pragma unroll
        for (int k = 0; k < R; ++k) field_out[row + R * k] = from_pk(v[k]);
      }
      if (real_out) {
#pragma unroll
        for (int k = 0; k < R; ++k) real_out[row + R * k] = v[k].x;
      }
    } else {
      cplx_plane_out<R, R, ST, GK, WIN>(v, acc, jb.env, jb.group, G, Q, q, y, row0, win, wr, field_out, real_out,
                                        phase, grad, gvb, ga, gb);
    }
  }
  if constexpr (ST) {
    __shared__ double red[GPB][3];
    rowinv_epilogue<R, R, GPB>(acc, Q, G, jb, j, y, rb, grp, t, target, tmask, inten_out, 0, partial, red);
  }
}

// ---------------------------------------------------------------------------
// Generic complex 2-D FFT (flip-map correlations): a row pass that writes its
// result transposed.  in [n][N][N] row-major -> out[n][k][y] = FFT_x in[n][y][x];
// two applications give the 2-D transform in natural orientation.  Same
// 32-lane group FFT and LDS tile transpose as k_rowfwd (64-B pieces of each
// output line, XCD-grouped row blocks).  INV: + sign, no 1/N^2.
// ---------------------------------------------------------------------------
template <int R, bool INV>
__global__ __launch_bounds__(256, 2) void k_fft_rt(const float2* __restrict__ in,
                                                   float2* __restrict__ out,
                                                   const float2* __restrict__ tw_glob) {
  constexpr int N = R * R;
  constexpr int GPB = 256 / R;
  constexpr int SCR = GPB * R * (R + 1);
  static_assert(N * GPB <= SCR, "tile must fit in the scratch area");
  constexpr int RB = N / GPB;
  __shared__ float2 tw[N];
  __shared__ __attribute__((aligned(16))) float2 lds[SCR];
  for (int i = threadIdx.x; i < N; i += 256) tw[i] = tw_glob[i];
  const int grp = threadIdx.x / R;
  const int t = threadIdx.x % R;
  int bid = xcd_pair<RB>(blockIdx.x);
  const int rb = bid % RB;
  const int plane = bid / RB;
  const int y0 = rb * GPB;
  const float2* row = in + ((size_t)plane * N + y0 + grp) * N + t;
  float2 v[R];
#pragma unroll
  for (int j = 0; j < R; ++j) v[j] = row[R * j];
  __syncthreads();  // tw visible
  fft_group<R, INV>(v, t, PaddedScratch<R>{lds + grp * R * (R + 1)}, tw);
  lds_barrier();    // scratch reused as the tile [k][row]
#pragma unroll
  for (int k2 = 0; k2 < R; ++k2) lds[tile_pos<R>(t + R * k2, grp)] = v[k2];
  lds_barrier();
  float2* base = out + (size_t)plane * N * N;
  constexpr int CHUNKS = N * GPB / 2;
#pragma unroll
  for (int i = 0; i < CHUNKS / 256; ++i) {
    const int c = threadIdx.x + 256 * i;
    const int r2 = (c % (GPB / 2)) * 2;
    const int line = c / (GPB / 2);
    const float2 a = lds[tile_pos<R>(line, r2)];
    const float2 b = lds[tile_pos<R>(line, r2 + 1)];
    *reinterpret_cast<float4*>(base + (size_t)line * N + y0 + r2) = make_float4(a.x, a.y, b.x, b.y);
  }
}

template <int R>
static hipError_t launch_fft2d(const PlanDev& pd, float2* a, float2* b, int n_planes, bool inverse,
                               hipStream_t st) {
  constexpr int N = R * R;
  const unsigned blocks = (unsigned)n_planes * (N / (256 / R));
  for (int pass = 0; pass < 2; ++pass) {
    const float2* src = pass == 0 ? a : b;
    float2* dst = pass == 0 ? b : a;
    if (inverse)
      hipLaunchKernelGGL((k_fft_rt<R, true>), dim3(blocks), dim3(256), 0, st, src, dst, pd.tw);
    else
      hipLaunchKernelGGL((k_fft_rt<R, false>), dim3(blocks), dim3(256), 0, st, src, dst, pd.tw);
  }
  return hipGetLastError();
}

// N = 896 (crop of a 1024 mask): the same transposing row pass on the 28 x 32
// lane-group FFT (natural layout in, slot layout out: lane k1 < 28 writes
// X[k1 + 28 k2] into the tile)
template <bool INV>
__global__ __launch_bounds__(256, 2) void k_fft_rt896(const float2* __restrict__ in,
                                                      float2* __restrict__ out,
                                                      const float2* __restrict__ tw_glob) {
  constexpr int N = 896, R = 32, GPB = 8, RB = N / GPB;
  constexpr int SCR = GPB * R * (R + 1);
  static_assert(N * GPB <= SCR, "tile must fit in the scratch area");
  __shared__ float2 tw[N];
  __shared__ __attribute__((aligned(16))) float2 lds[SCR];
  for (int i = threadIdx.x; i < N; i += 256) tw[i] = tw_glob[i];
  const int grp = threadIdx.x / R;
  const int t = threadIdx.x % R;
  int bid = xcd_pair<RB>(blockIdx.x);
  const int rb = bid % RB;
  const int plane = bid / RB;
  const int y0 = rb * GPB;
  const float2* row = in + ((size_t)plane * N + y0 + grp) * N + t;
  float2 v[32];
#pragma unroll
  for (int j = 0; j < 28; ++j) v[j] = row[R * j];
  __syncthreads();  // tw visible
  fft896_ns<INV>(v, t, PaddedScratch<R>{lds + grp * R * (R + 1)}, tw);
  lds_barrier();
  if (t < 28) {
#pragma unroll
    for (int k2 = 0; k2 < 32; ++k2) lds[tile_pos<R, GPB>(t + 28 * k2, grp)] = v[k2];
  }
  lds_barrier();
  float2* base = out + (size_t)plane * N * N;
  constexpr int CHUNKS = N * GPB / 2;
  static_assert(CHUNKS % 256 == 0, "chunking");
#pragma unroll
  for (int i = 0; i < CHUNKS / 256; ++i) {
    const int c = threadIdx.x + 256 * i;
    const int r2 = (c % (GPB / 2)) * 2;
    const int line = c / (GPB / 2);
    const float2 a = lds[tile_pos<R, GPB>(line, r2)];
    const float2 b = lds[tile_pos<R, GPB>(line, r2 + 1)];
    *reinterpret_cast<float4*>(base + (size_t)line * N + y0 + r2) = make_float4(a.x, a.y, b.x, b.y);
  }
}

hipError_t run_fft2d(const PlanDev& pd, float2* a, float2* b, int n_planes, bool inverse,
                     hipStream_t st) {
  if (n_planes <= 0) return hipSuccess;
  if (pd.R == 0) {   // N = 896
    const unsigned blocks = (unsigned)n_planes * (896 / 8);
    for (int pass = 0; pass < 2; ++pass) {
      const float2* src = pass == 0 ? a : b;
      float2* dst = pass == 0 ? b : a;
      if (inverse) hipLaunchKernelGGL((k_fft_rt896<true>), dim3(blocks), dim3(256), 0, st, src, dst, pd.tw);
      else hipLaunchKernelGGL((k_fft_rt896<false>), dim3(blocks), dim3(256), 0, st, src, dst, pd.tw);
    }
    return hipGetLastError();
  }
  switch (pd.R) {
    case 32: return launch_fft2d<32>(pd, a, b, n_planes, inverse, st);
    case 16: return launch_fft2d<16>(pd, a, b, n_planes, inverse, st);
    case 8: return launch_fft2d<8>(pd, a, b, n_planes, inverse, st);
    default: return hipErrorInvalidValue;
  }
}

// ---------------------------------------------------------------------------
// launch sequence for one batch of jobs
// ---------------------------------------------------------------------------
__global__ void k_reduce_partials(const double* __restrict__ partial, int n_jobs, int RB,
                                  double* __restrict__ job_stats);

// The sample kernels of N = R^2 for the shared pick (hbx_internal.hpp): N = 1024 has first passes of its
// own, N = 64 a last pass of its own
template <int R>
struct SampleKernels {
  static constexpr int NT = kRowNT<R>;
  template <int LK, bool WIN>
  static auto first_real() {
    if constexpr (R == 32) return k_rowfwd32_real<LK, WIN>;
    else return k_rowfwd_real<R, NT, LK, WIN>;
  }
  template <int LK, bool WIN>
  static auto first_cplx() {
    if constexpr (R == 32) {
      // (the weighted form keeps its place in front of the other two: first use fixes it in the code object)
      (void)k_rowfwd32_cplx<kLoadWeighted, false>;
      return k_rowfwd32_cplx<LK, WIN>;
    } else {
      return k_rowfwd_cplx<R, NT, LK, WIN>;
    }
  }
  template <bool ST, int GK, bool WIN>
  static auto last_cplx() {
    if constexpr (kTiledB<R>) return k_rowinv_d_cplx<R, ST, GK, WIN>;
    else return k_rowinv_cplx<R, NT, ST, GK, WIN>;
  }
};

// The annealed walk's last pass (hbx_dbs_walk_planes_anneal, EXTENSION): a walk batch of k_rowinv_d<R, true>
// -- always a plane-cache step -- whose last-arriving workgroup takes the annealed decision
// (walk_planes_arrive<true>).  A kernel of its own with k_rowinv_d's argument list, so that every k_rowinv_d
// instantiation keeps its name, code and place; it carries the walk batch's path alone (no full
// propagation, field, reconcile or window code).  field_out, rc_pending, rc_cache and win are not read.
template <int R>
__global__ __launch_bounds__(256, 2) void k_rowinv_walk_anneal(const JobDesc* __restrict__ jobs,
                                                               const float2* __restrict__ ws_b,
                                                               const float* __restrict__ target,
                                                               const float2* __restrict__ tw_glob, int P, int G,
                                                               double* __restrict__ partial,
                                                               float* __restrict__ inten_out,
                                                               float2* __restrict__ field_out, size_t tmask,
                                                               int inten_by_env, int plane_mode,
                                                               float* __restrict__ plane_pool,
                                                               const int32_t* __restrict__ plane_slot,
                                                               int plane_spares, int spare_base,
                                                               const int32_t* __restrict__ rc_pending,
                                                               float* __restrict__ rc_cache, WalkPlanesArgs wk,
                                                               hbx_window_t win) {
  constexpr int N = R * R, GPB = 256 / R, RB = N / GPB;
  static_assert(walk_planes_anneal_lds_bytes(RB) <= GPB * R * (R + 1) * 8, "the decision's LDS fits the scratch");
  __shared__ float2 tw[N];
  __shared__ float2 scratch[GPB * R * (R + 1)];
  __shared__ double red[GPB][3];
  for (int i = threadIdx.x; i < N; i += 256) tw[i] = tw_glob[i];

  const int grp = threadIdx.x / R;
  const int t = threadIdx.x % R;
  const int bid = xcd_pair<RB>(blockIdx.x);
  const int rb = bid % RB;
  const int j = bid / RB;
  const JobDesc jb = jobs[j];
  if (wk.phase && wk.phase[j] == 2) {   // a kept walk slot: its partials and fresh pair stand
    walk_planes_arrive<true>(wk, reinterpret_cast<char*>(scratch));
    return;
  }
  if (jb.env < 0) {
    rowinv_zero_partial<true>(partial, j, RB, rb);
    walk_planes_arrive<true>(wk, reinterpret_cast<char*>(scratch));
    return;
  }
  const int y = rb * GPB + grp;
  constexpr int PLB = N * N;                 // float2 per B plane
  const __amdgpu_buffer_rsrc_t rs = plane_rsrc(ws_b + (size_t)j * P * PLB, (unsigned)((size_t)P * PLB * 8));
  const RowinvLanes<R> ln(y, t);
  auto load_plane = [&](pk2 (&v)[R], int p) { rowinv_load_plane(v, ln, rs, p); };
  float acc[R];
#pragma unroll
  for (int k = 0; k < R; ++k) acc[k] = 0.0f;
  const PaddedScratch<R> sc{scratch + grp * R * (R + 1)};
  const PlaneCache<R> pc(jb, j, y, G, P, plane_spares, spare_base, plane_pool, plane_slot);
  auto finish_plane = [&](pk2 (&v)[R], int p) {
    fft_group<R, true>(v, t, sc, tw);
    plane_out<R, R>(v, acc, pc, jb, G, P, p, t, nullptr, kPlanesStep);
  };
  pk2 va[R];
  rowinv_planes_step(va, acc, pc, jb, P, t, load_plane, finish_plane);   // only the flipped plane's pair is in B
  rowinv_epilogue<R, R, GPB, true>(acc, P, G, jb, j, y, rb, grp, t, target, tmask, inten_out, inten_by_env, partial,
                                   red, nullptr, nullptr);
  __syncthreads();   // every group is done with its scratch region: the decision's LDS
  walk_planes_arrive<true>(wk, reinterpret_cast<char*>(scratch));
}

// (pixel weights) the weighted last passes and their pick, behind every other kernel of this file
template <int R>
static void launch_last_pw(const PlanDev& pd, const PassCall& c, float2* ws_b, unsigned blocks, hipStream_t st);
// (illumination fields) the sourced first and last passes and their picks, behind the weighted ones
template <int R>
static void launch_first_src(const PlanDev& pd, const PassCall& c, float2* ws_a, unsigned blocks, hipStream_t st);
template <int R>
static void launch_last_src(const PlanDev& pd, const PassCall& c, float2* ws_b, unsigned blocks, hipStream_t st);

template <int R, int SK>
static hipError_t launch_passes(const PlanDev& pd, const PassCall& c, hipStream_t st) {
  constexpr int N = R * R;
  constexpr int GPB = 256 / R;
  constexpr int NT = kRowNT<R>;
  constexpr int kRowBlocks = N / (NT / R);        // row blocks per plane (pair)
  const JobDesc* jobs = c.jobs;
  const int n_jobs = c.n_jobs;
  const int P = pd.P;
  const int CH = pd.G * pd.P;
  PassTimer* tm = pd.timer;
  const int pair = c.plane_mode == kPlanesStep ? 1 : 0;
  const PassTarget tg = pass_target(pd, c);
  // Small batches (greedy DBS, a few candidates per launch): the walk-per-workgroup loops
  // (rowfwd_iters row blocks, col2_iters lines) trade parallelism for store overlap, which pays
  // only when the launch fills the chip many times over.  Below kSmallBlocks workgroups the
  // launch runs one row block / one line per workgroup instead -- the same arithmetic, so
  // bit-identical results: tests/test_gpu_launch_size.py puts the same inputs through both forms
  // and compares every output array.  pass_launch_small (hbx_internal.hpp) decides.
  static_assert(kRowBlocks == N / panel_rows(R) && GPB == 256 / R, "pass_*_blocks count these workgroups");
  const unsigned rf_blocks = pass_rowfwd_blocks(R, P, n_jobs, pair != 0);
  const unsigned col_blocks = pass_col2_blocks(R, P, n_jobs, pair != 0);
  const bool small = pass_launch_small(R, P, n_jobs, pair != 0);
  // real and complex samples: the bit kernels' geometry (complex: wg.q = the complex plane), one row
  // block per workgroup at every launch size
  const unsigned sample_blocks = (unsigned)n_jobs * (P / 2) * kRowBlocks;

  // (focal stacks) the job slot the call runs in, and its pieces: a forward piece behind depth 0 finds the
  // row spectra in ws_a, a backward piece ends behind the column pass.  Every other call: slot 0, all three
  float2* const ws_a = pd.ws_a + (size_t)c.stack_slot0 * P * plane_a_elems(R);
  float2* const ws_b = pd.ws_b + (size_t)c.stack_slot0 * P * plane_b_elems(R);
  if (!c.stack_skip_first) {
    if (tm) tm->begin(0, st);
    if (c.source && !c.source_adjoint) {   // the sourced loads, only when the pointer is set
      launch_first_src<R>(pd, c, ws_a, sample_blocks, st);
    } else if (pass_complex(c)) {   // the load kind: complex samples as they are, times scale * weight, or exp(i pi phase)
      const int lk = c.phase_values ? (c.phase_levels ? kLoadPhaseLevels : kLoadPhase) : c.complex_weight ? kLoadWeighted : kLoadComplex;
      launch_kernel(pick_first_pass_cplx<SampleKernels<R>>(lk, pass_window_in(c, N)), sample_blocks, NT, st, jobs,
                    c.complex_values, ws_a, pd.tw, P, CH, c.complex_weight, pass_first_scale(c), c.phase_values, pass_first_window(c));
    } else if (c.real_values) {
      // the load kind: the samples as they are, or (hbx_evaluate_threshold) the field of the bit [x >= threshold]
      launch_kernel(pick_first_pass_real<SampleKernels<R>>(c.real_binarize != 0, pass_window_in(c, N)), sample_blocks, NT,
                    st, jobs, c.real_values, ws_a, pd.tw, P, CH, c.real_threshold, pd.va, pd.va + pd.vb, c.in_win);
    } else {
      auto k = [&] {
        if constexpr (R == 32) return small ? k_rowfwd32<SK, 1> : k_rowfwd32<SK>;
        else if constexpr (kTiledB<R>) return small ? k_rowfwd<R, NT, SK, 1> : k_rowfwd<R, NT, SK>;
        else return k_rowfwd<R, NT, SK>;
      }();
      launch_kernel(k, small ? rf_blocks * rowfwd_iters<R>() : rf_blocks, NT, st, jobs,
                    reinterpret_cast<const uint32_t*>(c.mask), ws_a, pd.tw, P, CH, pd.va, pd.vb, pair, c.actions,
                    c.act_err, c.walk_phase);
    }
    if (tm) tm->end(0, n_jobs, st);
  }

  if (tm) tm->begin(1, st);
  {
    auto k = [&] {
      if constexpr (kTiledB<R>) return small ? k_col2<R, SK, 1> : k_col2<R, SK>;
      else return k_col2<R, SK>;
    }();
    launch_kernel(k, small ? col_blocks * col2_iters<R>() : col_blocks, 256, st, jobs, ws_a, ws_b, pass_htab(pd, c),
                  pd.tw, P, pair, c.walk_phase);
  }
  if (tm) tm->end(1, n_jobs, st);
  if (c.stack_skip_last) return hipGetLastError();

  const unsigned blocks = (unsigned)n_jobs * kRowBlocks;
  if (tm) tm->begin(2, st);
  if (c.pixel_weight) {    // the weighted statistics forms, only when the pointer is set
    launch_last_pw<R>(pd, c, ws_b, blocks, st);
  } else if (c.source && c.source_adjoint) {   // conj(source) on the plane, then the leaf's gradient
    launch_last_src<R>(pd, c, ws_b, blocks, st);
  } else if (pass_complex(c)) {   // recombine each plane pair, or a leaf's gradient instead (pick_last_pass_cplx)
    const auto k = pick_last_pass_cplx<SampleKernels<R>>(pass_grad_kind(c), c.complex_stats != 0,
                                                         c.windowed != 0);
    launch_kernel(k, blocks, NT, st, jobs, ws_b, pd.tw, P, pd.G, c.complex_field, c.real_part, tg.rows, tg.mask,
                  pd.partial, c.inten_out, c.grad_samples, c.grad_phase, pd.vb, pass_grad_p0(c), pass_grad_p1(c), c.out_win);
  } else if constexpr (kTiledB<R>) {
    // WALK (r05): a plane-cache walk batch, the last workgroup decides.  LEAN (r06): the plain
    // FFT-mode launch (the headline), its own instantiation without the plane cache / field /
    // reconcile / walk code -- 1,687 instead of 4,988 instructions; same arithmetic and bits,
    // k_rowinv 1.465-1.515 -> 1.444-1.457 ms alternated on one box (profiles/r06/rowinv_lean_ab_r06e.txt)
    const bool lean = c.plane_mode == kPlanesOff && !c.field_out && !c.rc_pending;
    // (named WALK, LEAN, general on purpose: first use fixes a kernel's place in the code object, and
    // the timings on record were taken with this layout -- tools/isa_cmp.py reports a reordering)
    auto k = k_rowinv_d<R, true>;
    if (!c.walk_planes) k = lean ? k_rowinv_d<R, false, true> : k_rowinv_d<R>;
    if (c.windowed) k = lean ? k_rowinv_d<R, false, true, true> : k_rowinv_d<R, false, false, true>;
    if (c.walk_anneal) k = k_rowinv_walk_anneal<R>;   // (behind every k_rowinv_d: their layout stays)
    launch_kernel(k, blocks, 256, st, jobs, ws_b, tg.rows, pd.tw, P, pd.G, pd.partial, c.inten_out, c.field_out,
                  tg.mask, c.inten_by_env, c.plane_mode, c.plane_pool, c.plane_slot, c.plane_spares, c.spare_base,
                  c.rc_pending, c.rc_cache, c.walk_planes ? *c.walk_planes : WalkPlanesArgs{}, c.out_win);
  } else {
    launch_kernel(!c.windowed ? k_rowinv<R, NT> : k_rowinv<R, NT, true>, blocks, NT, st, jobs, ws_b, tg.rows, pd.tw,
                  P, pd.G, pd.partial, c.inten_out, c.field_out, tg.mask, c.inten_by_env, c.out_win);
  }
  if (tm) tm->end(2, n_jobs, st);
  if (pass_reduces(c))
    hipLaunchKernelGGL(k_reduce_partials, dim3(n_jobs), dim3(64), 0, st, pd.partial, n_jobs, kRowBlocks, pd.job_stats);
  return hipGetLastError();
}

hipError_t run_jobs(const PlanDev& pd, const PassCall& c, hipStream_t st) {
  const hipError_t e = check_pass_call(pd, c);
  if (e != hipSuccess) return e;
  if (pd.R == 0) return run_jobs_896(pd, c, st);
  switch (pd.R * 4 + pd.store_kind) {
#define HBX_PASSES_CASE(R_, SK_) \
    case R_ * 4 + SK_: return launch_passes<R_, SK_>(pd, c, st);
    HBX_PASSES_CASE(32, HBX_PRECISION_F32)
    HBX_PASSES_CASE(32, HBX_PRECISION_BF16_STORE)
    HBX_PASSES_CASE(32, HBX_PRECISION_F16_STORE)
    HBX_PASSES_CASE(16, HBX_PRECISION_F32)
    HBX_PASSES_CASE(16, HBX_PRECISION_BF16_STORE)
    HBX_PASSES_CASE(16, HBX_PRECISION_F16_STORE)
    HBX_PASSES_CASE(8, HBX_PRECISION_F32)
    HBX_PASSES_CASE(8, HBX_PRECISION_BF16_STORE)
    HBX_PASSES_CASE(8, HBX_PRECISION_F16_STORE)
#undef HBX_PASSES_CASE
    default: return hipErrorInvalidValue;
  }
}

// ---------------------------------------------------------------------------
// Focal stacks (hbx_backward_stack, EXTENSION): the depth-summing complex last pass
// ---------------------------------------------------------------------------
// The backward of a stack is linear: the leaf's gradient is the sum over the D depths of the adjoint
// propagations.  Depth d's first and column pass leave job j's B planes in slot d * slot_stride + j of ws_b;
// these kernels add the D slots' rows as they load them (rowinv_load_pair_stack; N = 64: as the shares of the
// tile arrive), run ONE inverse row FFT per complex plane and write the gradient once -- where D single-depth
// last passes run D FFTs and D stores, and D - 1 read-add-write passes follow.  Each is its single-depth
// sibling's geometry (k_rowinv_d_cplx, k_rowinv_cplx) without the statistics and window forms, with the
// argument list of its own (D and the float2 stride between depth slots), named and instantiated behind every
// other kernel of this file, so that none of them moves.  ws_b is the first depth's job 0.
template <int R, int GK = kGradNone>
__global__ __launch_bounds__(256, 2) void k_rowinv_d_cplx_stack(const JobDesc* __restrict__ jobs,
                                                                const float2* __restrict__ ws_b,
                                                                const float2* __restrict__ tw_glob, int P, int G,
                                                                int D, size_t dstride,
                                                                float2* __restrict__ field_out,
                                                                float* __restrict__ real_out,
                                                                const float* __restrict__ phase,
                                                                float* __restrict__ grad, float gvb, float ga,
                                                                float gb) {
  constexpr int N = R * R, GPB = 256 / R, RB = N / GPB;
  __shared__ float2 tw[N];
  __shared__ float2 scratch[GPB * R * (R + 1)];
  for (int i = threadIdx.x; i < N; i += 256) tw[i] = tw_glob[i];

  const int grp = threadIdx.x / R;
  const int t = threadIdx.x % R;
  const int bid = xcd_pair<RB>(blockIdx.x);
  const int rb = bid % RB;
  const int j = bid / RB;
  const JobDesc jb = jobs[j];
  if (jb.env < 0) return;   // uniform per block
  const int y = rb * GPB + grp;
  const hbx_window_t win = {0, 0, 0, 0};
  const WinRow wr(win, y, t);   // (unread: no window form)
  const int Q = P / 2;                        // complex planes per group
  constexpr int PLB = N * N;                 // float2 per B plane
  const float2* job_b = ws_b + (size_t)j * P * PLB;
  const unsigned job_bytes = (unsigned)((size_t)P * PLB * 8);
  const RowinvLanes<R> ln(y, t);
  auto load_pair = [&](pk2 (&v)[R], int q) { rowinv_load_pair_stack(v, ln, job_b, dstride, job_bytes, D, q); };
  const PaddedScratch<R> sc{scratch + grp * R * (R + 1)};
  const size_t row0 = (((size_t)jb.env * G + jb.group) * Q * N + y) * N + t;   // complex plane 0, pixel x = t
  float acc[1];
  auto finish_plane = [&](pk2 (&v)[R], int q) {
    fft_group<R, true>(v, t, sc, tw);
    cplx_plane_out<R, R, false, GK, false>(v, acc, jb.env, jb.group, G, Q, q, y, row0, win, wr, field_out, real_out,
                                           phase, grad, gvb, ga, gb);
  };
  pk2 va[R];
  load_pair(va, 0);
  __syncthreads();  // tw visible
  // (N = 256: its sibling keeps the next pair in flight in a second register set.  Here depth 0's pair in flight
  // under the FFT measured the same as this one set at D = 2, 3 and 4 -- the pass is bound by the D planes it
  // reads, profiles/focal_stack/stack256_prefetch_ab.txt -- so both sizes run the one loop)
#pragma unroll 1
  for (int q = 0; q < Q; ++q) {
    finish_plane(va, q);
    if (q + 1 < Q) load_pair(va, q + 1);   // uniform: no pair is read twice
  }
}

// N = 64: k_rowinv_cplx's LDS tile transpose.  A thread's share of the pair's two plane tiles is combined as
// it arrives, depth by depth in the same order -- (((a_0 + i b_0) + a_1) + i b_1) + ... -- and written to the tile
template <int R, int NT, int GK = kGradNone>
__global__ __launch_bounds__(NT, 512 / NT) void k_rowinv_cplx_stack(const JobDesc* __restrict__ jobs,
                                                                    const float2* __restrict__ ws_b,
                                                                    const float2* __restrict__ tw_glob, int P, int G,
                                                                    int D, size_t dstride,
                                                                    float2* __restrict__ field_out,
                                                                    float* __restrict__ real_out,
                                                                    const float* __restrict__ phase,
                                                                    float* __restrict__ grad, float gvb, float ga,
                                                                    float gb) {
  constexpr int N = R * R;
  constexpr int GPB = NT / R;          // rows per block
  constexpr int RB = N / GPB;
  constexpr int CH16 = N * GPB / 2;     // 16-B chunks per plane tile
  constexpr int PER = CH16 / NT;
  static_assert(CH16 % NT == 0, "chunking");
  constexpr int SCR = GPB * R * (R + 1);   // padded transpose scratch reuses the tile
  __shared__ float2 tw[N];
  __shared__ __attribute__((aligned(16))) float2 tile[SCR > N * GPB ? SCR : N * GPB];

  for (int i = threadIdx.x; i < N; i += NT) tw[i] = tw_glob[i];

  const int grp = threadIdx.x / R;
  const int t = threadIdx.x % R;
  const int bid = xcd_pair<RB>(blockIdx.x);
  const int rb = bid % RB;
  const int j = bid / RB;
  const JobDesc jb = jobs[j];
  if (jb.env < 0) return;   // uniform per block
  const int y0 = rb * GPB;
  const int y = y0 + grp;
  const hbx_window_t win = {0, 0, 0, 0};
  const WinRow wr(win, y, t);   // (unread: no window form)
  const int Q = P / 2;
  constexpr size_t PLB = plane_b_elems(R);
  const float2* jbase = ws_b + (size_t)j * P * PLB;

  float4 pv[PER];   // this thread's share of the summed, recombined pair, one pair ahead
  auto load_pair = [&](int q) {
    const float2* a = jbase + (size_t)(2 * q) * PLB;
#pragma unroll
    for (int i = 0; i < PER; ++i) {   // depth 0, as k_rowinv_cplx combines it: B[2q] + i B[2q + 1]
      const TileChunk ch = tile_chunk<NT, GPB>(i);
      const float4 pa = ld_stream4(a + LayoutB<R>::at(ch.line, y0 + ch.r2));
      const float4 pb = ld_stream4(a + PLB + LayoutB<R>::at(ch.line, y0 + ch.r2));
      pv[i] = make_float4(pa.x - pb.y, pa.y + pb.x, pa.z - pb.w, pa.w + pb.z);
    }
#pragma unroll 1
    for (int d = 1; d < D; ++d) {
      const float2* ad = a + (size_t)d * dstride;
#pragma unroll
      for (int i = 0; i < PER; ++i) {
        const TileChunk ch = tile_chunk<NT, GPB>(i);
        const float4 pa = ld_stream4(ad + LayoutB<R>::at(ch.line, y0 + ch.r2));
        const float4 pb = ld_stream4(ad + PLB + LayoutB<R>::at(ch.line, y0 + ch.r2));
        pv[i].x += pa.x; pv[i].y += pa.y; pv[i].z += pa.z; pv[i].w += pa.w;
        pv[i].x -= pb.y; pv[i].y += pb.x; pv[i].z -= pb.w; pv[i].w += pb.z;
      }
    }
  };
  load_pair(0);
  const size_t row0 = (((size_t)jb.env * G + jb.group) * Q * N + y) * N + t;
  float acc[1];

#pragma unroll 1
  for (int q = 0; q < Q; ++q) {
    lds_barrier();  // previous plane's scratch use is over (also publishes tw)
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const TileChunk ch = tile_chunk<NT, GPB>(i);
      tile[tile_pos<R, GPB>(ch.line, ch.r2)] = make_float2(pv[i].x, pv[i].y);
      tile[tile_pos<R, GPB>(ch.line, ch.r2 + 1)] = make_float2(pv[i].z, pv[i].w);
    }
    if (q + 1 < Q) load_pair(q + 1);   // next pair's tiles in flight under this plane's FFT
    lds_barrier();
    pk2 v[R];
#pragma unroll
    for (int jj = 0; jj < R; ++jj) v[jj] = to_pk(tile[tile_pos<R, GPB>(t + R * jj, grp)]);
    lds_barrier();  // tile consumed: reuse it as transpose scratch
    fft_group<R, true>(v, t, PaddedScratch<R>{tile + grp * R * (R + 1)}, tw);
    cplx_plane_out<R, R, false, GK, false>(v, acc, jb.env, jb.group, G, Q, q, y, row0, win, wr, field_out, real_out,
                                           phase, grad, gvb, ga, gb);
  }
}

// the stack kernels of N = R^2; gk: the output kind (pass_grad_kind), D = n_depths
template <int R>
static hipError_t launch_stack_last(const PlanDev& pd, const PassCall& c, int n_depths, int slot_stride,
                                    hipStream_t st) {
  constexpr int N = R * R;
  constexpr int NT = kRowNT<R>;
  constexpr int kRowBlocks = N / (NT / R);
  auto pick = [](int gk) {
    if constexpr (kTiledB<R>) {
      auto k = k_rowinv_d_cplx_stack<R, kGradNone>;
      if (gk == kGradPhase) k = k_rowinv_d_cplx_stack<R, kGradPhase>;
      if (gk == kGradSteWindow) k = k_rowinv_d_cplx_stack<R, kGradSteWindow>;
      if (gk == kGradSteSigmoid) k = k_rowinv_d_cplx_stack<R, kGradSteSigmoid>;
      if (gk == kGradPhaseLevels) k = k_rowinv_d_cplx_stack<R, kGradPhaseLevels>;
      return k;
    } else {
      auto k = k_rowinv_cplx_stack<R, NT, kGradNone>;
      if (gk == kGradPhase) k = k_rowinv_cplx_stack<R, NT, kGradPhase>;
      if (gk == kGradSteWindow) k = k_rowinv_cplx_stack<R, NT, kGradSteWindow>;
      if (gk == kGradSteSigmoid) k = k_rowinv_cplx_stack<R, NT, kGradSteSigmoid>;
      if (gk == kGradPhaseLevels) k = k_rowinv_cplx_stack<R, NT, kGradPhaseLevels>;
      return k;
    }
  };
  PassTimer* tm = pd.timer;
  if (tm) tm->begin(2, st);
  launch_kernel(pick(pass_grad_kind(c)), (unsigned)c.n_jobs * kRowBlocks, NT, st, c.jobs, pd.ws_b, pd.tw, pd.P, pd.G,
                n_depths, (size_t)slot_stride * pd.P * plane_b_elems(R), c.complex_field, c.real_part, c.grad_samples,
                c.grad_phase, pd.vb, pass_grad_p0(c), pass_grad_p1(c));
  if (tm) tm->end(2, c.n_jobs, st);
  return hipGetLastError();
}

hipError_t run_stack_last(const PlanDev& pd, const PassCall& c, int n_depths, int slot_stride, hipStream_t st) {
  const hipError_t e = check_stack_last(pd, c, n_depths, slot_stride);
  if (e != hipSuccess) return e;
  switch (pd.R) {
    case 0: return run_stack_last_896(pd, c, n_depths, slot_stride, st);
    case 32: return launch_stack_last<32>(pd, c, n_depths, slot_stride, st);
    case 16: return launch_stack_last<16>(pd, c, n_depths, slot_stride, st);
    case 8: return launch_stack_last<8>(pd, c, n_depths, slot_stride, st);
    default: return hipErrorInvalidValue;
  }
}

// ---------------------------------------------------------------------------
// Per-pixel loss weights (hbx_evaluate_pw / hbx_evaluate_stack_pw, EXTENSION): the weighted last passes
// ---------------------------------------------------------------------------
// The statistics-producing last passes of the sample paths with rowinv_epilogue_pw (hbx_rowinv.hpp) as their
// tail: the weight row of (env, group, y) enters the three f64 sums, and everything in front of the tail -- the
// loads, the inverse row FFTs, |U|^2, the field stores -- is the sibling's arithmetic in the sibling's order, so
// the field and the intensity are its bits.  Each is its sibling's general form without the plane cache, walk,
// reconcile, window, target-ahead and env-major code (check_pass_call refuses a weight with any of them), with an
// argument list of its own, named and instantiated behind every other kernel of this file, so that none of them
// moves (tools/isa_cmp.py).  k_rowinv_d_pw: k_rowinv_d (N = 1024 / 256), field_out nullable.
template <int R>
__global__ __launch_bounds__(256, 2) void k_rowinv_d_pw(const JobDesc* __restrict__ jobs,
                                                        const float2* __restrict__ ws_b,
                                                        const float* __restrict__ target,
                                                        const float* __restrict__ pixel_weight,
                                                        const float2* __restrict__ tw_glob, int P, int G,
                                                        double* __restrict__ partial, float* __restrict__ inten_out,
                                                        float2* __restrict__ field_out) {
  constexpr int N = R * R, GPB = 256 / R, RB = N / GPB;
  __shared__ float2 tw[N];
  __shared__ float2 scratch[GPB * R * (R + 1)];
  __shared__ double red[GPB][3];
  for (int i = threadIdx.x; i < N; i += 256) tw[i] = tw_glob[i];

  const int grp = threadIdx.x / R;
  const int t = threadIdx.x % R;
  const int bid = xcd_pair<RB>(blockIdx.x);
  const int rb = bid % RB;
  const int j = bid / RB;
  const JobDesc jb = jobs[j];
  if (jb.env < 0) {   // uniform per block
    rowinv_zero_partial(partial, j, RB, rb);
    return;
  }
  const int y = rb * GPB + grp;
  constexpr int PLB = N * N;                 // float2 per B plane
  const __amdgpu_buffer_rsrc_t rs = plane_rsrc(ws_b + (size_t)j * P * PLB, (unsigned)((size_t)P * PLB * 8));
  const RowinvLanes<R> ln(y, t);
  auto load_plane = [&](pk2 (&v)[R], int p) { rowinv_load_plane(v, ln, rs, p); };
  float acc[R];
#pragma unroll
  for (int k = 0; k < R; ++k) acc[k] = 0.0f;
  const PaddedScratch<R> sc{scratch + grp * R * (R + 1)};
  auto finish_plane = [&](pk2 (&v)[R], int p) {   // plane_out without the plane cache
    fft_group<R, true>(v, t, sc, tw);
#pragma unroll
    for (int k = 0; k < R; ++k) acc[k] += fmaf(v[k].x, v[k].x, v[k].y * v[k].y);
    if (field_out) {
      float2* frow = field_out + (((size_t)jb.env * G * P + jb.group * P + p) * N + y) * N;
#pragma unroll
      for (int k = 0; k < R; ++k) frow[t + R * k] = make_float2(v[k].x, v[k].y);
    }
  };
  pk2 va[R];
  load_plane(va, 0);
  __syncthreads();  // tw visible
  if constexpr (R == 16) {   // N = 256: the next plane in flight under this one's FFT, as k_rowinv_d
    pk2 vb[R];
#pragma unroll 1
    for (int p = 0; p < P; p += 2) {         // P is even (hbx_plan_create)
      load_plane(vb, p + 1);
      finish_plane(va, p);
      if (p + 2 < P) load_plane(va, p + 2);   // uniform: no plane is read twice
      finish_plane(vb, p + 1);
    }
  } else {
#pragma unroll 1
    for (int p = 0; p < P; ++p) {
      finish_plane(va, p);
      if (p + 1 < P) load_plane(va, p + 1);   // uniform
    }
  }
  rowinv_epilogue_pw<R, R, GPB>(acc, P, G, jb, j, y, rb, grp, t, target, pixel_weight, inten_out, partial, red);
}

// k_rowinv (N = 64) with the weighted tail
template <int R, int NT>
__global__ __launch_bounds__(NT, 512 / NT) void k_rowinv_pw(const JobDesc* __restrict__ jobs,
                                                      const float2* __restrict__ ws_b,
                                                      const float* __restrict__ target,
                                                      const float* __restrict__ pixel_weight,
                                                      const float2* __restrict__ tw_glob, int P, int G,
                                                      double* __restrict__ partial, float* __restrict__ inten_out,
                                                      float2* __restrict__ field_out) {
  constexpr int N = R * R;
  constexpr int GPB = NT / R;          // rows per block
  constexpr int RB = N / GPB;
  constexpr int CH16 = N * GPB / 2;     // 16-B chunks per plane tile
  constexpr int PER = CH16 / NT;
  static_assert(CH16 % NT == 0, "chunking");
  constexpr int SCR = GPB * R * (R + 1);   // padded transpose scratch reuses the tile
  __shared__ float2 tw[N];
  __shared__ __attribute__((aligned(16))) float2 tile[SCR > N * GPB ? SCR : N * GPB];
  __shared__ double red[GPB][3];

  for (int i = threadIdx.x; i < N; i += NT) tw[i] = tw_glob[i];

  const int grp = threadIdx.x / R;
  const int t = threadIdx.x % R;
  const int bid = xcd_pair<RB>(blockIdx.x);
  const int rb = bid % RB;
  const int j = bid / RB;
  const JobDesc jb = jobs[j];
  if (jb.env < 0) {   // uniform per block
    rowinv_zero_partial(partial, j, RB, rb);
    return;
  }
  const int y0 = rb * GPB;
  const int y = y0 + grp;
  constexpr size_t PLB = plane_b_elems(R);
  const float2* jbase = ws_b + (size_t)j * P * PLB;

  float4 pre[PER];   // this thread's share of a plane tile, one plane ahead
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const TileChunk ch = tile_chunk<NT, GPB>(i);
    pre[i] = ld_stream4(jbase + LayoutB<R>::at(ch.line, y0 + ch.r2));
  }
  float acc[R];
#pragma unroll
  for (int k = 0; k < R; ++k) acc[k] = 0.0f;

#pragma unroll 1
  for (int p = 0; p < P; ++p) {
    lds_barrier();  // previous plane's scratch use is over (also publishes tw)
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const TileChunk ch = tile_chunk<NT, GPB>(i);
      tile[tile_pos<R, GPB>(ch.line, ch.r2)] = make_float2(pre[i].x, pre[i].y);
      tile[tile_pos<R, GPB>(ch.line, ch.r2 + 1)] = make_float2(pre[i].z, pre[i].w);
    }
    if (p + 1 < P) {  // next plane's tile in flight under this plane's FFT
      const float2* nb = jbase + (size_t)(p + 1) * PLB;
#pragma unroll
      for (int i = 0; i < PER; ++i) {
        const TileChunk ch = tile_chunk<NT, GPB>(i);
        pre[i] = ld_stream4(nb + LayoutB<R>::at(ch.line, y0 + ch.r2));
      }
    }
    lds_barrier();
    pk2 v[R];
#pragma unroll
    for (int jj = 0; jj < R; ++jj) v[jj] = to_pk(tile[tile_pos<R, GPB>(t + R * jj, grp)]);
    lds_barrier();  // tile consumed: reuse it as transpose scratch
    fft_group<R, true>(v, t, PaddedScratch<R>{tile + grp * R * (R + 1)}, tw);
#pragma unroll
    for (int k = 0; k < R; ++k) acc[k] += fmaf(v[k].x, v[k].x, v[k].y * v[k].y);
    if (field_out) {
      float2* frow = field_out + (((size_t)jb.env * G * P + jb.group * P + p) * N + y) * N;
#pragma unroll
      for (int k = 0; k < R; ++k) frow[t + R * k] = from_pk(v[k]);
    }
  }
  rowinv_epilogue_pw<R, R, GPB>(acc, P, G, jb, j, y, rb, grp, t, target, pixel_weight, inten_out, partial, red);
}

// k_rowinv_d_cplx's statistics form (N = 1024 / 256) with the weighted tail; field_out nullable, no real part
template <int R>
__global__ __launch_bounds__(256, 2) void k_rowinv_d_cplx_pw(const JobDesc* __restrict__ jobs,
                                                             const float2* __restrict__ ws_b,
                                                             const float2* __restrict__ tw_glob, int P, int G,
                                                             float2* __restrict__ field_out,
                                                             const float* __restrict__ target,
                                                             const float* __restrict__ pixel_weight,
                                                             double* __restrict__ partial,
                                                             float* __restrict__ inten_out) {
  constexpr int N = R * R, GPB = 256 / R, RB = N / GPB;
  __shared__ float2 tw[N];
  __shared__ float2 scratch[GPB * R * (R + 1)];
  __shared__ double red[GPB][3];
  for (int i = threadIdx.x; i < N; i += 256) tw[i] = tw_glob[i];

  const int grp = threadIdx.x / R;
  const int t = threadIdx.x % R;
  const int bid = xcd_pair<RB>(blockIdx.x);
  const int rb = bid % RB;
  const int j = bid / RB;
  const JobDesc jb = jobs[j];
  if (jb.env < 0) {  // uniform per block
    rowinv_zero_partial(partial, j, RB, rb);
    return;
  }
  const int y = rb * GPB + grp;
  const hbx_window_t win = {0, 0, 0, 0};
  const WinRow wr(win, y, t);   // (unread: no window form)
  const int Q = P / 2;                        // complex planes per group
  constexpr int PLB = N * N;                 // float2 per B plane
  const __amdgpu_buffer_rsrc_t rs = plane_rsrc(ws_b + (size_t)j * P * PLB, (unsigned)((size_t)P * PLB * 8));
  const RowinvLanes<R> ln(y, t);
  auto load_pair = [&](pk2 (&v)[R], int q) { rowinv_load_pair(v, ln, rs, q); };
  const PaddedScratch<R> sc{scratch + grp * R * (R + 1)};
  const size_t row0 = (((size_t)jb.env * G + jb.group) * Q * N + y) * N + t;   // complex plane 0, pixel x = t
  float acc[R];
#pragma unroll
  for (int k = 0; k < R; ++k) acc[k] = 0.0f;
  auto finish_plane = [&](pk2 (&v)[R], int q) {
    fft_group<R, true>(v, t, sc, tw);
    cplx_plane_out<R, R, true, kGradNone, false>(v, acc, jb.env, jb.group, G, Q, q, y, row0, win, wr, field_out, nullptr,
                                                 nullptr, nullptr, 0.0f, 0.0f, 0.0f);
  };
  pk2 va[R];
  load_pair(va, 0);
  __syncthreads();  // tw visible
  if constexpr (R == 16) {
    pk2 vb[R];
#pragma unroll 1
    for (int q = 0; q < Q; q += 2) {
      if (q + 1 < Q) load_pair(vb, q + 1);
      finish_plane(va, q);
      if (q + 1 < Q) {
        if (q + 2 < Q) load_pair(va, q + 2);
        finish_plane(vb, q + 1);
      }
    }
  } else {
#pragma unroll 1
    for (int q = 0; q < Q; ++q) {
      finish_plane(va, q);
      if (q + 1 < Q) load_pair(va, q + 1);   // uniform: no pair is read twice
    }
  }
  rowinv_epilogue_pw<R, R, GPB>(acc, Q, G, jb, j, y, rb, grp, t, target, pixel_weight, inten_out, partial, red);
}

// k_rowinv_cplx's statistics form (N = 64) with the weighted tail
template <int R, int NT>
__global__ __launch_bounds__(NT, 512 / NT) void k_rowinv_cplx_pw(const JobDesc* __restrict__ jobs,
                                                           const float2* __restrict__ ws_b,
                                                           const float2* __restrict__ tw_glob, int P, int G,
                                                           float2* __restrict__ field_out,
                                                           const float* __restrict__ target,
                                                           const float* __restrict__ pixel_weight,
                                                           double* __restrict__ partial,
                                                           float* __restrict__ inten_out) {
  constexpr int N = R * R;
  constexpr int GPB = NT / R;          // rows per block
  constexpr int RB = N / GPB;
  constexpr int CH16 = N * GPB / 2;     // 16-B chunks per plane tile
  constexpr int PER = CH16 / NT;
  static_assert(CH16 % NT == 0, "chunking");
  constexpr int SCR = GPB * R * (R + 1);   // padded transpose scratch reuses the tile
  __shared__ float2 tw[N];
  __shared__ __attribute__((aligned(16))) float2 tile[SCR > N * GPB ? SCR : N * GPB];
  __shared__ double red[GPB][3];

  for (int i = threadIdx.x; i < N; i += NT) tw[i] = tw_glob[i];

  const int grp = threadIdx.x / R;
  const int t = threadIdx.x % R;
  const int bid = xcd_pair<RB>(blockIdx.x);
  const int rb = bid % RB;
  const int j = bid / RB;
  const JobDesc jb = jobs[j];
  if (jb.env < 0) {  // uniform per block
    rowinv_zero_partial(partial, j, RB, rb);
    return;
  }
  const int y0 = rb * GPB;
  const int y = y0 + grp;
  const int Q = P / 2;
  constexpr size_t PLB = plane_b_elems(R);
  const float2* jbase = ws_b + (size_t)j * P * PLB;

  float4 pa[PER], pb[PER];   // this thread's share of the pair's two plane tiles, one pair ahead
  auto load_pair = [&](int q) {
    const float2* a = jbase + (size_t)(2 * q) * PLB;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const TileChunk ch = tile_chunk<NT, GPB>(i);
      pa[i] = ld_stream4(a + LayoutB<R>::at(ch.line, y0 + ch.r2));
      pb[i] = ld_stream4(a + PLB + LayoutB<R>::at(ch.line, y0 + ch.r2));
    }
  };
  load_pair(0);
  const size_t row0 = (((size_t)jb.env * G + jb.group) * Q * N + y) * N + t;
  float acc[R];
#pragma unroll
  for (int k = 0; k < R; ++k) acc[k] = 0.0f;

#pragma unroll 1
  for (int q = 0; q < Q; ++q) {
    lds_barrier();  // previous plane's scratch use is over (also publishes tw)
#pragma unroll
    for (int i = 0; i < PER; ++i) {   // B[2q] + i B[2q + 1]
      const TileChunk ch = tile_chunk<NT, GPB>(i);
      tile[tile_pos<R, GPB>(ch.line, ch.r2)] = make_float2(pa[i].x - pb[i].y, pa[i].y + pb[i].x);
      tile[tile_pos<R, GPB>(ch.line, ch.r2 + 1)] = make_float2(pa[i].z - pb[i].w, pa[i].w + pb[i].z);
    }
    if (q + 1 < Q) load_pair(q + 1);   // next pair's tiles in flight under this plane's FFT
    lds_barrier();
    pk2 v[R];
#pragma unroll
    for (int jj = 0; jj < R; ++jj) v[jj] = to_pk(tile[tile_pos<R, GPB>(t + R * jj, grp)]);
    lds_barrier();  // tile consumed: reuse it as transpose scratch
    fft_group<R, true>(v, t, PaddedScratch<R>{tile + grp * R * (R + 1)}, tw);
#pragma unroll
    for (int k = 0; k < R; ++k) acc[k] += fmaf(v[k].x, v[k].x, v[k].y * v[k].y);
    if (field_out) {
      const size_t row = row0 + (size_t)q * N * N;
#pragma unroll
      for (int k = 0; k < R; ++k) field_out[row + R * k] = from_pk(v[k]);
    }
  }
  rowinv_epilogue_pw<R, R, GPB>(acc, Q, G, jb, j, y, rb, grp, t, target, pixel_weight, inten_out, partial, red);
}

// launch_passes' last pass of a call with PassCall::pixel_weight set (check_pass_call has passed: sample
// input, a target, statistics; tg.rows is the caller's target)
template <int R>
static void launch_last_pw(const PlanDev& pd, const PassCall& c, float2* ws_b, unsigned blocks, hipStream_t st) {
  constexpr int NT = kRowNT<R>;
  if (pass_complex(c)) {
    if constexpr (kTiledB<R>)
      launch_kernel(k_rowinv_d_cplx_pw<R>, blocks, 256, st, c.jobs, ws_b, pd.tw, pd.P, pd.G, c.complex_field, c.target,
                    c.pixel_weight, pd.partial, c.inten_out);
    else
      launch_kernel(k_rowinv_cplx_pw<R, NT>, blocks, NT, st, c.jobs, ws_b, pd.tw, pd.P, pd.G, c.complex_field, c.target,
                    c.pixel_weight, pd.partial, c.inten_out);
  } else {
    if constexpr (kTiledB<R>)
      launch_kernel(k_rowinv_d_pw<R>, blocks, 256, st, c.jobs, ws_b, c.target, c.pixel_weight, pd.tw, pd.P, pd.G,
                    pd.partial, c.inten_out, c.field_out);
    else
      launch_kernel(k_rowinv_pw<R, NT>, blocks, NT, st, c.jobs, ws_b, c.target, c.pixel_weight, pd.tw, pd.P, pd.G,
                    pd.partial, c.inten_out, c.field_out);
  }
}

// ---------------------------------------------------------------------------
// Illumination fields (hbx_evaluate_source / hbx_backward_source, EXTENSION)
// ---------------------------------------------------------------------------
// The modulator is lit by source[G][N][N] complex64 instead of a unit plane wave: the forward's first pass
// propagates u = s f(x), formed as it loads the leaf's samples and the source row (source_load_row,
// hbx_rowcol.hpp), and the backward's last pass multiplies the back-propagated plane by conj(s) behind its
// inverse row FFT and in front of the leaf's gradient formula (source_conj_row).  The column pass, the
// forward's last pass and the backward's first pass are the launches that exist.  The kernels are the
// siblings' bodies -- k_rowfwd_cplx / k_rowfwd32_cplx, k_rowinv_d_cplx / k_rowinv_cplx without their
// statistics and window forms -- with argument lists of their own, behind every other kernel of this file,
// so no existing instantiation's code, descriptor or place moves (tools/isa_cmp.py).
//
// SK (kSrc*): the leaf kind; all five fill one complex plane per leaf plane, the two real kinds included.
// values: [env][CH / 2][N][N] complex64 (kSrcComplex) or float32; (p0, p1, p2): source_sample's.
template <int R, int NT, int SK>
__global__ __launch_bounds__(NT, 512 / NT) void k_rowfwd_src(const JobDesc* __restrict__ jobs,
                                                       const float* __restrict__ values,
                                                       const float2* __restrict__ source,
                                                       float2* __restrict__ ws_a,
                                                       const float2* __restrict__ tw_glob, int P, int CH,
                                                       float p0, float p1, float p2) {
  constexpr int N = R * R;
  constexpr int GPB = NT / R;          // rows per row block
  __shared__ float2 tw[N];
  __shared__ __attribute__((aligned(16))) float2 lds[rowfwd_scratch<R, NT>()];

  stage_twiddles<N, NT>(tw, tw_glob);

  const int grp = threadIdx.x / R;
  const int t = threadIdx.x % R;
  const int lane_base = (threadIdx.x & 63) - t;
  constexpr int RB = N / GPB;
  const FirstPassBlock wg = first_pass_block<RB>(xcd_pair<RB>(blockIdx.x), P / 2);
  const int j = wg.j;
  const JobDesc jb = jobs[j];
  if (jb.env < 0) return;  // uniform per block
  const int y0 = wg.rbw * GPB;
  const int y = y0 + grp;
  pk2 v[R];
  first_pass_load_src<R, R, SK, R>(v, values, source, jb.env, jb.group, P, CH, wg.q, y, t, p0, p1, p2);
  __syncthreads();  // tw visible

  float2* base = ws_a + ((size_t)j * P + 2 * wg.q) * plane_a_elems(R);
  rowfwd_emit<R, NT, HBX_PRECISION_F32>(v, t, grp, lane_base, y0, lds, tw, base);
}

// N = 1024: k_rowfwd32_cplx's geometry and its three workgroups per CU.  A row is 32 samples and 32
// source pairs per lane, and all of them are in flight at once: 142 VGPRs for the complex kind, 112-115
// for the others, of the 168 that three workgroups leave, no scratch.  In halves (kSrc32Piece = 16) the
// complex kind takes 128 and occupies the same, so the whole row stays (DESIGN.md;
// profiles/source_field/resource_usage.txt)
constexpr int kSrc32Piece = 32;
template <int SK>
__global__ __launch_bounds__(256, 3) void k_rowfwd32_src(const JobDesc* __restrict__ jobs,
                                                         const float* __restrict__ values,
                                                         const float2* __restrict__ source,
                                                         float2* __restrict__ ws_a,
                                                         const float2* __restrict__ tw_glob, int P, int CH,
                                                         float p0, float p1, float p2) {
  constexpr int R = 32, NT = 256, N = R * R;
  constexpr int GPB = NT / R;          // 8 rows per row block
  __shared__ float2 tw[N];
  __shared__ __attribute__((aligned(16))) float lds[kRowfwd32Scr];

  stage_twiddles<N, NT>(tw, tw_glob);

  const int grp = threadIdx.x / R;
  const int t = threadIdx.x % R;
  const int k1 = mirror_k1(t);         // the second FFT stage in mirror-paired lane order
  constexpr int RB = N / GPB;
  const FirstPassBlock wg = first_pass_block<RB>(xcd_pair<RB>(blockIdx.x), P / 2);
  const int j = wg.j;
  const JobDesc jb = jobs[j];
  if (jb.env < 0) return;  // uniform per block
  const int y0 = wg.rbw * GPB;
  const int y = y0 + grp;
  pk2 v[R];
  first_pass_load_src<R, R, SK, kSrc32Piece>(v, values, source, jb.env, jb.group, P, CH, wg.q, y, t, p0, p1, p2);
  __syncthreads();  // tw visible

  float2* base = ws_a + ((size_t)j * P + 2 * wg.q) * plane_a_elems(R);
  rowfwd32_emit<HBX_PRECISION_F32>(v, t, k1, grp, y0, lds, tw, base);
}

// The sourced last passes: k_rowinv_d_cplx (N = 1024 / 256) and k_rowinv_cplx (N = 64) with g' = conj(s) g
// between the inverse row FFT and cplx_plane_out; source row y of the job's group, loaded behind the FFT.
// GK: kGradNone (g' to field_out, or Re g' to real_out -- one of the two), the two phase kinds, the two
// STE kinds.  No statistics, no window.
template <int R, int GK>
__global__ __launch_bounds__(256, 2) void k_rowinv_d_src(const JobDesc* __restrict__ jobs,
                                                         const float2* __restrict__ ws_b,
                                                         const float2* __restrict__ tw_glob, int P, int G,
                                                         const float2* __restrict__ source,
                                                         float2* __restrict__ field_out,
                                                         float* __restrict__ real_out,
                                                         const float* __restrict__ phase,
                                                         float* __restrict__ grad, float gvb, float ga,
                                                         float gb) {
  constexpr int N = R * R, GPB = 256 / R, RB = N / GPB;
  __shared__ float2 tw[N];
  __shared__ float2 scratch[GPB * R * (R + 1)];
  for (int i = threadIdx.x; i < N; i += 256) tw[i] = tw_glob[i];

  const int grp = threadIdx.x / R;
  const int t = threadIdx.x % R;
  const int bid = xcd_pair<RB>(blockIdx.x);
  const int rb = bid % RB;
  const int j = bid / RB;
  const JobDesc jb = jobs[j];
  if (jb.env < 0) return;  // uniform per block
  const int y = rb * GPB + grp;
  const hbx_window_t win = {0, 0, 0, 0};
  const WinRow wr(win, y, t);   // (unread: no window form)
  const int Q = P / 2;                        // complex planes per group
  constexpr int PLB = N * N;                 // float2 per B plane
  const __amdgpu_buffer_rsrc_t rs = plane_rsrc(ws_b + (size_t)j * P * PLB, (unsigned)((size_t)P * PLB * 8));
  const RowinvLanes<R> ln(y, t);
  auto load_pair = [&](pk2 (&v)[R], int q) { rowinv_load_pair(v, ln, rs, q); };
  const PaddedScratch<R> sc{scratch + grp * R * (R + 1)};
  const size_t row0 = (((size_t)jb.env * G + jb.group) * Q * N + y) * N + t;   // complex plane 0, pixel x = t
  const float2* s0 = source + ((size_t)jb.group * N + y) * N + t;               // the source row, pixel x = t
  float acc[1];
  auto finish_plane = [&](pk2 (&v)[R], int q) {
    fft_group<R, true>(v, t, sc, tw);
    source_conj_row<R, R>(v, s0);
    cplx_plane_out<R, R, false, GK, false>(v, acc, jb.env, jb.group, G, Q, q, y, row0, win, wr, field_out, real_out,
                                           phase, grad, gvb, ga, gb);
  };
  pk2 va[R];
  load_pair(va, 0);
  __syncthreads();  // tw visible
  if constexpr (R == 16) {
    pk2 vb[R];
#pragma unroll 1
    for (int q = 0; q < Q; q += 2) {
      if (q + 1 < Q) load_pair(vb, q + 1);
      finish_plane(va, q);
      if (q + 1 < Q) {
        if (q + 2 < Q) load_pair(va, q + 2);
        finish_plane(vb, q + 1);
      }
    }
  } else {
#pragma unroll 1
    for (int q = 0; q < Q; ++q) {
      finish_plane(va, q);
      if (q + 1 < Q) load_pair(va, q + 1);   // uniform: no pair is read twice
    }
  }
}

// N = 64: the registers also hold the next pair's tiles (pa, pb), and the unsourced gradient forms run five
// workgroups per CU (86-93 VGPRs).  To keep that: the launch bound asks for five, the source row is taken in
// pieces of kSrc8Piece pixels, and kGradNone is two instantiations -- RP: the real part to real_out, else the
// field to field_out -- so no null test sits between the product and the stores.  84-96 VGPRs, no scratch
// (whole row and one kGradNone form under the same bound: 12-68 bytes of scratch;
// profiles/source_field/resource_usage.txt)
constexpr int kSrc8Piece = 2;
template <int R, int NT, int GK, bool RP = false>
__global__ __launch_bounds__(NT, 5) void k_rowinv_src(const JobDesc* __restrict__ jobs,
                                                       const float2* __restrict__ ws_b,
                                                       const float2* __restrict__ tw_glob, int P, int G,
                                                       const float2* __restrict__ source,
                                                       float2* __restrict__ field_out,
                                                       float* __restrict__ real_out,
                                                       const float* __restrict__ phase,
                                                       float* __restrict__ grad, float gvb, float ga,
                                                       float gb) {
  constexpr int N = R * R;
  constexpr int GPB = NT / R;          // rows per block
  constexpr int RB = N / GPB;
  constexpr int CH16 = N * GPB / 2;     // 16-B chunks per plane tile
  constexpr int PER = CH16 / NT;
  static_assert(CH16 % NT == 0, "chunking");
  constexpr int SCR = GPB * R * (R + 1);   // padded transpose scratch reuses the tile
  __shared__ float2 tw[N];
  __shared__ __attribute__((aligned(16))) float2 tile[SCR > N * GPB ? SCR : N * GPB];

  for (int i = threadIdx.x; i < N; i += NT) tw[i] = tw_glob[i];

  const int grp = threadIdx.x / R;
  const int t = threadIdx.x % R;
  const int bid = xcd_pair<RB>(blockIdx.x);
  const int rb = bid % RB;
  const int j = bid / RB;
  const JobDesc jb = jobs[j];
  if (jb.env < 0) return;  // uniform per block
  const int y0 = rb * GPB;
  const int y = y0 + grp;
  const hbx_window_t win = {0, 0, 0, 0};
  const WinRow wr(win, y, t);   // (unread: no window form)
  const int Q = P / 2;
  constexpr size_t PLB = plane_b_elems(R);
  const float2* jbase = ws_b + (size_t)j * P * PLB;

  float4 pa[PER], pb[PER];   // this thread's share of the pair's two plane tiles, one pair ahead
  auto load_pair = [&](int q) {
    const float2* a = jbase + (size_t)(2 * q) * PLB;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const TileChunk ch = tile_chunk<NT, GPB>(i);
      pa[i] = ld_stream4(a + LayoutB<R>::at(ch.line, y0 + ch.r2));
      pb[i] = ld_stream4(a + PLB + LayoutB<R>::at(ch.line, y0 + ch.r2));
    }
  };
  load_pair(0);
  const size_t row0 = (((size_t)jb.env * G + jb.group) * Q * N + y) * N + t;
  const float2* s0 = source + ((size_t)jb.group * N + y) * N + t;   // the source row, pixel x = t
  float acc[1];

#pragma unroll 1
  for (int q = 0; q < Q; ++q) {
    lds_barrier();  // previous plane's scratch use is over (also publishes tw)
#pragma unroll
    for (int i = 0; i < PER; ++i) {   // B[2q] + i B[2q + 1]
      const TileChunk ch = tile_chunk<NT, GPB>(i);
      tile[tile_pos<R, GPB>(ch.line, ch.r2)] = make_float2(pa[i].x - pb[i].y, pa[i].y + pb[i].x);
      tile[tile_pos<R, GPB>(ch.line, ch.r2 + 1)] = make_float2(pa[i].z - pb[i].w, pa[i].w + pb[i].z);
    }
    if (q + 1 < Q) load_pair(q + 1);   // next pair's tiles in flight under this plane's FFT
    lds_barrier();
    pk2 v[R];
#pragma unroll
    for (int jj = 0; jj < R; ++jj) v[jj] = to_pk(tile[tile_pos<R, GPB>(t + R * jj, grp)]);
    lds_barrier();  // tile consumed: reuse it as transpose scratch
    fft_group<R, true>(v, t, PaddedScratch<R>{tile + grp * R * (R + 1)}, tw);
    source_conj_row<R, R, kSrc8Piece>(v, s0);
    if constexpr (GK == kGradNone) {
      // cplx_plane_out's full-grid form with the output chosen at compile time (check_pass_call: exactly one)
      const size_t row = row0 + (size_t)q * N * N;
      if constexpr (!RP) {
#pragma unroll
        for (int k = 0; k < R; ++k) field_out[row + R * k] = from_pk(v[k]);
      } else {
#pragma unroll
        for (int k = 0; k < R; ++k) real_out[row + R * k] = v[k].x;
      }
    } else {
      cplx_plane_out<R, R, false, GK, false>(v, acc, jb.env, jb.group, G, Q, q, y, row0, win, wr, field_out, real_out,
                                             phase, grad, gvb, ga, gb);
    }
  }
}

// the five leaf kinds' first passes, in the order the code object gets them
template <int R>
static void launch_first_src(const PlanDev& pd, const PassCall& c, float2* ws_a, unsigned blocks, hipStream_t st) {
  constexpr int NT = kRowNT<R>;
  const auto pick = [](int sk) {
    if constexpr (R == 32) {
      auto k = k_rowfwd32_src<kSrcComplex>;
      if (sk == kSrcPhase) k = k_rowfwd32_src<kSrcPhase>;
      if (sk == kSrcPhaseLevels) k = k_rowfwd32_src<kSrcPhaseLevels>;
      if (sk == kSrcReal) k = k_rowfwd32_src<kSrcReal>;
      if (sk == kSrcThreshold) k = k_rowfwd32_src<kSrcThreshold>;
      return k;
    } else {
      auto k = k_rowfwd_src<R, NT, kSrcComplex>;
      if (sk == kSrcPhase) k = k_rowfwd_src<R, NT, kSrcPhase>;
      if (sk == kSrcPhaseLevels) k = k_rowfwd_src<R, NT, kSrcPhaseLevels>;
      if (sk == kSrcReal) k = k_rowfwd_src<R, NT, kSrcReal>;
      if (sk == kSrcThreshold) k = k_rowfwd_src<R, NT, kSrcThreshold>;
      return k;
    }
  };
  const SourceParams sp = pass_source_params(pd, c);
  launch_kernel(pick(pass_source_kind(c)), blocks, NT, st, c.jobs, pass_source_samples(c), c.source, ws_a, pd.tw, pd.P,
                pd.G * pd.P, sp.p0, sp.p1, sp.p2);
}

// the sourced last pass of the call's gradient kind (check_pass_call has passed: one output, no statistics)
template <int R>
static void launch_last_src(const PlanDev& pd, const PassCall& c, float2* ws_b, unsigned blocks, hipStream_t st) {
  constexpr int NT = kRowNT<R>;
  const bool real_out = c.real_part != nullptr;   // kGradNone: the field or its real part, one of the two
  const auto pick = [real_out](int gk) {
    (void)real_out;   // (the tiled forms test the two pointers themselves)
    if constexpr (kTiledB<R>) {
      auto k = k_rowinv_d_src<R, kGradNone>;
      if (gk == kGradPhase) k = k_rowinv_d_src<R, kGradPhase>;
      if (gk == kGradPhaseLevels) k = k_rowinv_d_src<R, kGradPhaseLevels>;
      if (gk == kGradSteWindow) k = k_rowinv_d_src<R, kGradSteWindow>;
      if (gk == kGradSteSigmoid) k = k_rowinv_d_src<R, kGradSteSigmoid>;
      return k;
    } else {
      auto k = k_rowinv_src<R, NT, kGradNone>;
      if (gk == kGradNone && real_out) k = k_rowinv_src<R, NT, kGradNone, true>;
      if (gk == kGradPhase) k = k_rowinv_src<R, NT, kGradPhase>;
      if (gk == kGradPhaseLevels) k = k_rowinv_src<R, NT, kGradPhaseLevels>;
      if (gk == kGradSteWindow) k = k_rowinv_src<R, NT, kGradSteWindow>;
      if (gk == kGradSteSigmoid) k = k_rowinv_src<R, NT, kGradSteSigmoid>;
      return k;
    }
  };
  launch_kernel(pick(pass_grad_kind(c)), blocks, NT, st, c.jobs, ws_b, pd.tw, pd.P, pd.G, c.source, c.complex_field,
                c.real_part, c.grad_samples, c.grad_phase, pd.vb, pass_grad_p0(c), pass_grad_p1(c));
}

}  // namespace hbx
