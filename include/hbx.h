/*
 * hbx.h -- C-ABI of the MI355X-native binary-hologram hot path (libhbx.so).
 *
 * The reference (songyb111-gachon/binary-hologram-reinforcement-learning) is
 * pure Python: its hot path is a chain of torch ops behind the third-party
 * `torchOptics` API (tt.Tensor / tt.simulate / tt.relativeLoss / tm.get_PSNR)
 * called from gymnasium envs and DBS drivers.  This header is the boundary
 * those call sites bind to once the hot path is native.  Each entry point
 * names the reference interface it replaces (file:line under the reference).
 *
 * Conventions
 *   - Every buffer argument is a caller-owned DEVICE pointer (e.g. a
 *     torch-ROCm tensor's data_ptr()), contiguous, in the layout stated.
 *   - Masks are bit-packed: uint64 words [..][H][W/64], bit j of word w is
 *     pixel column 64*w + j (little-endian).  W % 64 == 0.
 *   - All calls are asynchronous on `stream` (a hipStream_t; NULL = default).
 *     A plan is bound to one device and is not re-entrant: one plan per
 *     stream / per GPU process.
 *   - Return 0 on success, a negative HBX_ERR_* code otherwise; the message
 *     is in hbx_last_error() (thread-local).  No C++ exception crosses it.
 *   - Channel c of an env belongs to colour group g = c / planes; group g
 *     propagates with wavelength[g]  (env_1024_24.py:135-147).
 */
#ifndef HBX_H
#define HBX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HBX_ABI_VERSION 15

#define HBX_OK 0
#define HBX_ERR_INVALID (-1)     /* bad argument / shape                          */
#define HBX_ERR_HIP (-2)         /* HIP runtime error                             */
#define HBX_ERR_UNSUPPORTED (-3) /* size not built (N must be 64, 256, 896, 1024)  */
#define HBX_ERR_NOMEM (-4)       /* workspace allocation failed                   */

/* Transfer function (tt.simulate, env.py:172; SURVEY a4 assumptions as switches) */
#define HBX_TF_ASM 0       /* exact angular spectrum, evanescent cut              */
#define HBX_TF_FRESNEL 1   /* Fresnel transfer function                           */
/* Mask -> field (env.py:170-171) */
#define HBX_FIELD_AMPLITUDE 0 /* u = m in {0,1}  (literal reference)              */
#define HBX_FIELD_PHASE 1     /* u = exp(i pi m) in {+1,-1}                       */
/* tt.relativeLoss scale (env.py:174) */
#define HBX_REL_NONE 0
#define HBX_REL_LSQ 1      /* s = sum(I T)/sum(I^2) over every channel            */
/* accept rule */
#define HBX_ACCEPT_ENV 0   /* roll back iff delta < 0   (env.py:191)              */
#define HBX_ACCEPT_DBS 1   /* accept iff psnr > prev    (DBS_1024_24.py:355)      */
/* reward: env.py:188-254 (RW * change, cubic success / max-steps bonuses)
 * or env_group.py:250-318 (importance rank of the nearest sampled change,
 * linear success / max-steps bonuses 100 - (200/1500) (steps - 1000)). */
#define HBX_REWARD_PSNR 0
#define HBX_REWARD_IMPORTANCE 1

#define HBX_MAX_GROUPS 4

/* Optics of one plan; replaces tt.Tensor meta {'dx','wl'} + simulate's z
 * (env.py:124,172; env_1024_24.py:135-138; DBS_1024_24.py:230-233).
 * dx is the pitch along the width axis (fx = kx / (N dx)), dy along the height axis; they may
 * differ.  HBX_TF_ASM: H(fx, fy) = exp(i 2 pi z sqrt(1/wl^2 - fx^2 - fy^2)) where the radicand is
 * positive and exactly 0 in the evanescent bins (radicand <= 0, reached once the pitch is below
 * wl / sqrt(2)); no path assumes |H| = 1.  H(-z) = conj H(z) in every bin, the zeros included, so
 * the plan for -z is the exact adjoint of the plan for z with or without a cut. */
typedef struct hbx_optics {
  int32_t height;                        /* N (64, 256, 896 or 1024), square */
  int32_t width;                         /* == height                         */
  int32_t groups;                        /* G: 1 mono, 3 RGB                  */
  int32_t planes;                        /* P planes per group (even)         */
  double wavelength[HBX_MAX_GROUPS];     /* metres, per group                 */
  double dx, dy;                         /* pixel pitch, metres               */
  double z;                              /* propagation distance, metres      */
  int32_t tf_kind;                       /* HBX_TF_*                          */
  int32_t field_kind;                    /* HBX_FIELD_*                       */
  int32_t rel_scale;                     /* HBX_REL_*                         */
  int32_t reserved;
  double peak;                           /* PSNR peak (1.0)                   */
} hbx_optics_t;

/* Device-resident state of B environments (BinaryHologramEnv attributes,
 * env.py:65-81: state, state_record, previous/initial psnr, counters). */
typedef struct hbx_env_buffers {
  uint64_t* mask;          /* [B][G*P][H][W/64]  env.state                    */
  int8_t* record;          /* [B][G*P][H][W]     env.state_record (nullable)  */
  const float* target;     /* [B][G][H][W]       target image                 */
  double* chan_stats;      /* [B][G][3]          sum I*T, sum I^2, sum T^2    */
  double* init_psnr;       /* [B]                env.initial_psnr             */
  double* prev_psnr;       /* [B]                env.previous_psnr            */
  double* max_psnr_diff;   /* [B]                env.max_psnr_diff            */
  int64_t* steps;          /* [B]                env.steps                    */
  int64_t* flip_count;     /* [B]                env.flip_count               */
  int64_t* sustained;      /* [B]                env.psnr_sustained_steps     */
  float* intensity;        /* [B][G][H][W] cached group means (nullable;
                              required by the incremental-field mode)          */
  int32_t* error;          /* [1] sticky device error word (nullable)         */
  float* field;            /* [B][G*P][H][W][2] complex64 propagated field of
                              every plane (nullable; incremental-field mode)   */
  /* env_group.py importance rewards (HBX_REWARD_IMPORTANCE only):            */
  const double* imp_changes;  /* [B][imp_count] psnr_change_list (env_group.py:90-120) */
  const double* imp_values;   /* [B][imp_count] importance_ranks (env_group.py:121-143) */
  const double* t_psnr_diff;  /* [B] per-env T_PSNR_DIFF (dynamic threshold,
                                 env_group.py:198; nullable -> params value)  */
  int32_t imp_count;          /* 10000 in the reference                       */
  int32_t reserved;
  /* ABI v8: zero-copy observations (env.py:135-140,176-181).  The reference
   * hands out env.state itself as obs["state"] and the stepped reconstruction
   * as obs["recon_image"]; these buffers are those observations, kept current
   * by reset and step so a caller can alias them instead of rebuilding them. */
  int8_t* state_bytes;     /* [B][G*P][H][W] 0/1 = the mask bits as int8:
                              obs["state"] (nullable).  Written by hbx_env_reset
                              / hbx_env_obs_sync and by the accepted flip of
                              every step (both modes).                        */
  float* recon;            /* [B][G][H][W] obs["recon_image"] (nullable; FFT
                              mode only; needs intensity and recon_pending).
                              After hbx_env_step the stepped group holds the
                              stepped (pre-rollback) intensity, env.py:179,
                              written there by the propagation itself; the
                              other groups hold the cached accepted ones.     */
  int32_t* recon_pending;  /* [B] internal: the group the next step reconciles
                              between recon and intensity (+g+1: accepted,
                              recon -> intensity; -(g+1): rolled back,
                              intensity -> recon; 0: none).  With recon given,
                              env->intensity of the last stepped group is
                              current only after that reconcile.
                              ABI v12: with ONE colour group (G = 1) every step
                              rewrites recon whole and nothing is ever restored,
                              so no reconcile runs: recon_pending stays 0 and
                              env->intensity keeps the last reset's / sync's
                              values (HBX_OBS_RECON re-propagates it).        */
  /* ABI v9: plane-cached FFT mode (N = 1024 / 256; both non-null, with
   * hbx_env_reset / hbx_field_refresh filling them).  A step changes ONE plane
   * of the touched group, and the FFT mode's re-propagation of the other plane
   * pairs reproduces their |U_q|^2 bit for bit (deterministic kernels), so the
   * step propagates only the flipped plane's pair and sums the cached planes
   * in the same plane order: the group intensity, statistics, PSNR, reward and
   * every decision are the FFT mode's bit for bit (env.py:170-174 work, 1/4 of
   * the propagation).  The pair is propagated, not the flipped plane alone:
   * k_rowfwd transforms two planes as the real and imaginary parts of one
   * complex FFT, so the partner's rounding sees the flipped plane and its bits
   * change too.  Both fresh |U|^2 go to the env's two spare slots and are
   * swapped in on accept (rollback: nothing to undo). */
  float* plane_inten;      /* [B][G*P + 2][H][W] f32 pool of per-plane |U|^2  */
  int32_t* plane_slot;     /* [B][G*P + 2] pool slot of each plane; [G*P] and
                              [G*P + 1] are the spares (caller-owned, filled
                              by reset)                                       */
  /* ABI v11: one-copy-free step readback.  hbx_env_step's last kernel copies
   * *error here (nullable; typically host memory from hbx_host_alloc, given by
   * its device address), so a caller whose reward / psnr / flag outputs also
   * live in such memory reads the whole step result on the host once the
   * stream work is complete, with no device-to-host copy. */
  int32_t* error_host;
} hbx_env_buffers_t;

/* BinaryHologramEnv.__init__ keyword arguments (env.py:38) + RW (env.py:29). */
typedef struct hbx_env_params {
  int64_t max_steps;       /* 10000 */
  double t_psnr;           /* 30    */
  int64_t t_steps;         /* 1     */
  double t_psnr_diff;      /* 0.1   */
  double reward_weight;    /* 800   */
  int32_t accept_rule;     /* HBX_ACCEPT_ENV */
  int32_t reward_kind;     /* HBX_REWARD_PSNR (env.py) | HBX_REWARD_IMPORTANCE (env_group.py) */
} hbx_env_params_t;

typedef struct hbx_plan* hbx_plan_t;

/* Library identity. */
int hbx_abi_version(void);
const char* hbx_last_error(void);

/* ABI v11: page-locked host memory that the GPU reads and writes directly
 * (mapped, coherent).  *host is the CPU address, *device the address to pass
 * to kernels (the step outputs of hbx_env_step, env->error_host).  The
 * reference's VecEnv hands numpy rewards / dones to SB3 every step
 * (train-PPO.py:296-322, env.py:259): the step kernels write them here and the
 * host reads them without a copy engine round trip.  Free with hbx_host_free. */
int hbx_host_alloc(size_t bytes, void** host, void** device);
int hbx_host_free(void* host);

/* Plan: owns twiddles, transfer-function tables and a workspace for up to
 * `max_jobs` concurrent group propagations (P * 12 * N^2 bytes per job:
 * 96 MiB at N = 1024, P = 8; hbx_plan_workspace_bytes gives the total).
 * Replaces the per-call setup hidden inside tt.simulate (env.py:172).
 *
 * Reuse contract (tests/test_gpu_plan_reuse.py): every entry point below runs in the plan's one set of
 * workspaces, and calls on one plan, issued in stream order, are independent of the calls before them
 * -- each call's results equal, bit for bit, those of the same call on a plan just created.  A call
 * reads no workspace element it did not write itself; the tables built on first use (the single-pixel
 * fields, the flip-map and walk scratch) depend on the optics alone; a refused call (a negative return
 * code) enqueues nothing and changes nothing.  All of a call's device work, the lazy table builds
 * included, is on the `stream` it was given; one plan serves one stream at a time.  What does persist:
 *   hbx_plan_set_precision  the rounding of the pass intermediates of every later call, until set again;
 *                           back at HBX_PRECISION_F32 the plan is as created
 *   hbx_plan_set_depths     the depth tables the hbx_*_stack calls read, until set again (it
 *                           synchronises the device); no single-depth call reads them
 *   hbx_plan_set_timing*    whether events are recorded around the pass launches; no result changes
 *   a walk                  nothing in the plan that a result depends on.  The walk's state is the
 *                           caller's (hbx_dbs_walk_t, mask, statistics, the plane pool or field, the
 *                           accept log): a walk may be split into calls at any batch, with other
 *                           calls on the plan between them, and gives the accept sequence, PSNRs,
 *                           mask, statistics and cached planes of the walk made in one call.  A
 *                           call's first batch propagates every candidate in full and starts the
 *                           spare-slot rotation of hbx_dbs_walk_planes* at 0, so WHICH spare slot of
 *                           the pool holds a candidate's fresh pair may differ across a call boundary.
 * A PSNR formed from statistics that are NaN is not NaN: +inf, or with sum I^2 NaN the unscaled one. */
int hbx_plan_create(hbx_plan_t* plan, const hbx_optics_t* optics, int32_t max_jobs,
                    int32_t device);
int hbx_plan_destroy(hbx_plan_t plan);
size_t hbx_plan_workspace_bytes(hbx_plan_t plan);
/* Propagation pipeline the plan runs (ABI v4): which kernels fill the pass
 * timer slots HBX_PASS_ROWFWD / HBX_PASS_COL below.  Since ABI v8 always
 *   HBX_PIPE_THREE_PASS  k_rowfwd -> k_col2 -> k_rowinv (N = 64, 256, 896, 1024; N = 896 runs
 *                        the fused mixed-radix 28 x 32 kernels of the same three passes)
 * (the r01 / r02 bits -> column pass and composed generic-N pipelines, values 1 and 2, were
 * measured slower and removed). */
#define HBX_PIPE_THREE_PASS 0
int hbx_plan_pipeline(hbx_plan_t plan);

/* Full propagation of every group of n_env masks (env.py:123-133 reset path,
 * env_1024_24.py:149-166, DBS_1024_24.py:244-257):
 *   intensity[B][G][H][W] = mean_p |IFFT2(FFT2(u_p) H_g)|^2   (nullable)
 *   chan_stats[B][G][3]   = per-channel sum I*T, sum I^2, sum T^2
 *   psnr[B]               = relativeLoss(rgb, target, get_PSNR)  (nullable)  */
int hbx_propagate(hbx_plan_t plan, const uint64_t* mask, const float* target, int32_t n_env,
                  float* intensity, double* chan_stats, double* psnr, void* stream);

/* tt.simulate(tt.Tensor(mask, meta), z) (env.py:170-172; DBS_1024_24.py:
 * 326-328) for binary masks: the propagated complex field of every plane,
 *   field[B][G*P][H][W][2] = IFFT2(FFT2(u) H_g)   (complex64, re/im pairs)
 * and optionally the plane-mean intensity[B][G][H][W] (nullable). */
int hbx_simulate(hbx_plan_t plan, const uint64_t* mask, int32_t n_env, float* field,
                 float* intensity, void* stream);

/* (ABI v15) The same two calls on a real-valued field instead of a binary mask:
 *   values[B][G*P][H][W] float32: the real field sample of every pixel, used as it is
 *   (u = value; the plan's field_kind maps bits only and is not applied).
 * Outputs, null-ability, chunking by the plan's max_jobs and n_env == 0 are those of
 * hbx_simulate / hbx_propagate; only the first pass differs (it reads 4 bytes per pixel instead
 * of one bit and fills the HBX_PASS_ROWFWD timer slot), so 0 / 1 samples give the bit path's
 * result.  A complex field u = a + i b goes through hbx_simulate_complex below (two calls' worth
 * of real planes a and b with F = F[a] + i F[b] is the same field by linearity, at about twice
 * the memory traffic).  All four built sizes; HBX_PRECISION_F32 only
 * (a plan set to a reduced-precision store kind returns HBX_ERR_UNSUPPORTED).  No env, DBS,
 * plane-cache or incremental mode runs on real-valued fields. */
int hbx_simulate_real(hbx_plan_t plan, const float* values, int32_t n_env, float* field,
                      float* intensity, void* stream);
int hbx_propagate_real(hbx_plan_t plan, const float* values, const float* target, int32_t n_env,
                       float* intensity, double* chan_stats, double* psnr, void* stream);

/* (ABI v15, additive) tt.simulate on a complex field.  A plan with P real planes per group
 * carries P/2 complex planes per group; each takes one plane-pair slot of the workspace.
 *   values   [B][G*P/2][H][W][2] complex64 samples as re/im pairs, used as they are (u = value)
 *   field    [B][G*P/2][H][W][2] = IFFT2(FFT2(u) H_g), complex64            (nullable)
 *   real_part[B][G*P/2][H][W]    = Re of the same field, float32            (nullable)
 * At least one of field and real_part must be non-null; with both, real_part holds exactly the
 * real parts stored in field.  The first pass reads the complex samples directly (the row FFT of
 * a + i b, split into the half spectra of a and b), the column pass is hbx_simulate_real's, and
 * the last pass forms B[a] + i B[b] on load, runs one inverse row FFT per complex plane and
 * writes it once -- about 64 N^2 bytes per complex plane against about 112 N^2 by way of two
 * real planes.  The adjoint of u -> IFFT2(FFT2(u) H) is this propagation on the plan for -z
 * (H(-z) = conj H(z)); real_part alone is then the gradient with respect to a real u.
 * Chunking by max_jobs, n_env (0: OK, < 0: HBX_ERR_INVALID), null arguments (HBX_ERR_INVALID),
 * HBX_PRECISION_F32 only (else HBX_ERR_UNSUPPORTED), the four built sizes and the pass-timer
 * slots HBX_PASS_ROWFWD / COL / ROWINV are those of hbx_simulate_real.  This call writes no
 * intensity or statistics (hbx_evaluate_complex does); no env, DBS, plane-cache or incremental
 * mode runs on complex fields. */
int hbx_simulate_complex(hbx_plan_t plan, const float* values, int32_t n_env, float* field,
                         float* real_part, void* stream);

/* (ABI v15, additive) hbx_simulate_complex on samples scaled by a real image per env and group:
 *   u[b][c][y][x] = (scale * weight[b][g(c)][y][x]) * values[b][c][y][x],
 *   g(c) = c / (P/2), the colour group of complex plane c
 *   weight[B][G][H][W] float32 (HBX_ERR_INVALID when null)
 * values, field and real_part are hbx_simulate_complex's, and so is every other rule (null
 * arguments, n_env, HBX_PRECISION_F32 only, chunking by max_jobs, the four built sizes, the timer
 * slots).  The first pass applies the weight as it loads the samples -- m = scale * w, then
 * re * m and im * m, one float32 multiply each -- so the result equals hbx_simulate_complex on
 * samples multiplied in that way bit for bit, and no weighted copy of values is written: the
 * first pass reads 12 N^2 bytes per complex plane instead of 8 N^2, the rest is unchanged.
 *
 * This is the vector-Jacobian product of the plane-mean intensity I = mean_p |A u_p|^2 (P planes
 * u_p per group, A u = IFFT2(FFT2(u) H_g)): with the saved field A u_p as values, the incoming
 * gradient gI[B][G][H][W] as weight and scale = 2/P, on the plan for -z that carries 2P real
 * planes (P complex planes) per group,
 *   for real u    dL/du = real_part of hbx_simulate_complex_weighted(field, gI, 2/P),
 *   for complex u dL/du = field of the same call (the conjugate-gradient convention, d/d conj u
 *                         times two, which is what torch.autograd uses). */
int hbx_simulate_complex_weighted(hbx_plan_t plan, const float* values, const float* weight,
                                  float scale, int32_t n_env, float* field, float* real_part,
                                  void* stream);

/* (ABI v15, additive) The plane-mean intensity of a real-valued field and nothing else:
 *   intensity[B][G][H][W] = mean_p |IFFT2(FFT2(u_p) H_g)|^2, values as hbx_simulate_real's.
 * hbx_simulate_real must write the field and hbx_propagate_real needs a target; this call writes
 * neither field nor statistics, and its intensity equals hbx_simulate_real's bit for bit.  Null
 * values or intensity: HBX_ERR_INVALID; n_env, HBX_PRECISION_F32 only and chunking by max_jobs as
 * hbx_simulate_real. */
int hbx_intensity_real(hbx_plan_t plan, const float* values, int32_t n_env, float* intensity,
                       void* stream);

/* (ABI v15, additive) The loss of a continuous hologram in one launch set (env.py:131-132,174:
 * tt.relativeLoss of the plane-mean intensity against the target).
 *
 * hbx_evaluate_real is hbx_propagate_real that may also write the field hbx_simulate_real writes:
 *   field[B][G*P][H][W][2] (nullable) equals hbx_simulate_real's bit for bit, and intensity
 *   (nullable), chan_stats and psnr (nullable) equal hbx_propagate_real's bit for bit; null
 *   values, target or chan_stats: HBX_ERR_INVALID.  One propagation where a loss with a gradient
 *   needed hbx_simulate_real (the field the backward pass reads) and a second one for the
 *   statistics.
 *
 * hbx_evaluate_complex is the same on a complex field: values and field are
 * hbx_simulate_complex's ([B][G*P/2][H][W][2]; a written field equals that call's bit for bit), and
 *   intensity[B][G][H][W] = mean over the group's P/2 complex planes q of |F_q|^2
 *   chan_stats[B][G][3]   = sum I*T, sum I^2, sum T^2 per channel against target[B][G][H][W]
 *   psnr[B]               = the plan's rel_scale and peak, as hbx_propagate
 * The last pass accumulates re^2 + im^2 per pixel after each complex plane's inverse row FFT and
 * ends in the real last pass's tail (plane mean, float64 partials in fixed order: results are
 * reproducible bit for bit); with field null it writes nothing but the intensity and the partials.
 * field, intensity and psnr are nullable.  target and chan_stats are given together or not at all:
 * without them the call returns the intensity alone (intensity is then required and psnr must be
 * null); with them at least chan_stats is written.  Anything else: HBX_ERR_INVALID.  Chunking by
 * max_jobs, n_env (0: OK, < 0: HBX_ERR_INVALID), HBX_PRECISION_F32 only (else
 * HBX_ERR_UNSUPPORTED), the four built sizes and the pass-timer slots are hbx_simulate_complex's. */
int hbx_evaluate_real(hbx_plan_t plan, const float* values, const float* target, int32_t n_env,
                      float* field, float* intensity, double* chan_stats, double* psnr, void* stream);
int hbx_evaluate_complex(hbx_plan_t plan, const float* values, const float* target, int32_t n_env,
                         float* field, float* intensity, double* chan_stats, double* psnr,
                         void* stream);

/* (ABI v15, additive) The relative loss per env from the statistics, on the device
 * (tt.relativeLoss(.., F.mse_loss) env.py:131, tt.relativeLoss(.., tm.get_PSNR) env.py:132,174,
 * without the host wait): chan_stats[B][G][3] -> loss[B] float64.  With S_xy, S_xx, S_yy the sums
 * over the env's G groups and n = G*H*W,
 *   rel_scale HBX_REL_LSQ   s = S_xy / S_xx, MSE = (S_yy - S_xy^2 / S_xx) / n  (S_xx = 0: S_yy / n)
 *   rel_scale HBX_REL_NONE  MSE = (S_xx - 2 S_xy + S_yy) / n
 *   kind HBX_LOSS_MSE  loss = MSE;  kind HBX_LOSS_PSNR  loss = 10 log10(peak^2 / MSE), +inf for MSE <= 0
 * rel_scale is the argument, not the plan's; HBX_LOSS_PSNR with the plan's own rel_scale gives
 * hbx_psnr's bits.  An unknown kind or rel_scale, or a null buffer: HBX_ERR_INVALID. */
#define HBX_LOSS_MSE 0
#define HBX_LOSS_PSNR 1
int hbx_loss(hbx_plan_t plan, const double* chan_stats, int32_t n_env, int32_t kind, int32_t rel_scale,
             double* loss, void* stream);

/* (ABI v15, additive) The gradient of that loss with respect to the intensity, one streaming pass
 * over intensity, target, weight [B][G][H][W] float32 (the plan's G, H, W):
 *   weight[b] = grad_loss[b] * d loss_b / d I[b] = a_b * I[b] + c_b * T[b]
 *   HBX_REL_LSQ   dMSE/dI = (2 s / n) (s I - T):  a = 2 s^2 / n, c = -2 s / n
 *   HBX_REL_NONE  dMSE/dI = (2 / n) (I - T):      a = 2 / n,     c = -2 / n
 *   HBX_LOSS_PSNR both times -(10 / ln 10) / MSE
 * grad_loss[B] float64 is the incoming gradient of the B losses (null: ones).  Each workgroup forms
 * its env's a and c in float64 from chan_stats and grad_loss, rounds them to float32 once and
 * computes fmaf(a, I, c * T) per pixel.  A degenerate env -- S_xx = 0 under HBX_REL_LSQ, or
 * MSE <= 0 with HBX_LOSS_PSNR -- gets a = c = 0: an all-zero weight, never a NaN or infinity.
 * Null intensity, target, chan_stats or weight, or an unknown kind or rel_scale: HBX_ERR_INVALID.
 * The backward pass of the loss is then hbx_simulate_complex_weighted(saved field, weight,
 * 2 / P_c) on the plan for -z, P_c the planes the mean ran over (P for hbx_evaluate_real, P/2 for
 * hbx_evaluate_complex). */
int hbx_loss_weight(hbx_plan_t plan, const float* intensity, const float* target,
                    const double* chan_stats, const double* grad_loss, int32_t n_env, int32_t kind,
                    int32_t rel_scale, float* weight, void* stream);

/* (ABI v15, additive) Phase holograms: the leaf is the phase, u = exp(i pi x).
 *   phase[B][G*P/2][H][W] float32 samples x, one per pixel of the plan's P/2 complex planes per
 *   group; the phase is pi x, so x = 1 is half a turn and x and x + 2 are the same field.
 * The first pass forms (cos pi x, sin pi x) as it loads x -- 4 N^2 bytes read per complex plane
 * instead of 8 N^2, and no complex copy of the hologram is ever written -- with the argument
 * reduced exactly (x mod 2 has no rounding in float32; x * float32(pi) has), so the field's error
 * does not grow with |x|: unwrapped phases of thousands of turns are as good as wrapped ones.
 *
 * hbx_simulate_phase: field, real_part and every rule are hbx_simulate_complex's (at least one of
 *   the two non-null; null phase: HBX_ERR_INVALID).
 * hbx_evaluate_phase: field, intensity, chan_stats, psnr, their null-ability and the target /
 *   chan_stats pairing are hbx_evaluate_complex's; only the first pass differs, and a written field
 *   equals hbx_simulate_phase's bit for bit.
 * hbx_phase_backward: the whole backward pass of a phase leaf, on the plan for -z.
 *   values    [B][G*P/2][H][W][2] complex64, the gradient with respect to the propagated field (or,
 *             with weight, the saved field itself)
 *   weight    [B][G][H][W] float32, nullable: with it the first pass is
 *             hbx_simulate_complex_weighted's (scale * weight applied on load); null: it is
 *             hbx_simulate_complex's, scale is ignored and the samples are used as they are
 *   phase     the leaf's samples x, as above
 *   grad_phase[B][G*P/2][H][W] float32 = pi (Im g cos pi x - Re g sin pi x), g the complex plane
 *             those two calls would write as field: Re(conj(du/dx) g) with du/dx = i pi u.
 *   The last pass reads x (4 N^2 bytes) and writes the one float (4 N^2) where the complex call
 *   stores g (8 N^2); g itself is never written.  With the saved field as values, hbx_loss_weight's
 *   output (or the incoming intensity gradient) as weight and scale = 2 / (P/2), grad_phase is
 *   dL/dx.  Null values, phase or grad_phase: HBX_ERR_INVALID.
 * Chunking by max_jobs, n_env (0: OK, < 0: HBX_ERR_INVALID), HBX_PRECISION_F32 only (else
 * HBX_ERR_UNSUPPORTED), the four built sizes and the pass-timer slots are hbx_simulate_complex's.
 * No env, DBS, plane-cache or incremental mode runs on phase samples (the binary phase mask,
 * HBX_FIELD_PHASE on bits, is the bit path and is not this). */
int hbx_simulate_phase(hbx_plan_t plan, const float* phase, int32_t n_env, float* field,
                       float* real_part, void* stream);
int hbx_evaluate_phase(hbx_plan_t plan, const float* phase, const float* target, int32_t n_env,
                       float* field, float* intensity, double* chan_stats, double* psnr,
                       void* stream);
int hbx_phase_backward(hbx_plan_t plan, const float* values, const float* weight, float scale,
                       const float* phase, int32_t n_env, float* grad_phase, void* stream);

/* (ABI v15, additive) Quantized phase holograms: the leaf is the phase x (in units of pi, as above),
 * the displayed hologram one of `levels` = L phase levels per pixel, 2 <= L <= 256.
 * The quantizer, one definition used by every entry point below (all float32, round-half-to-even):
 *   r = x - 2 rint(x / 2)     exact, r in [-1, 1]: unwrapped phases quantize as well as wrapped ones
 *   k = rint(r h)             h = float32(L / 2), one multiply, then the rounding
 *   q = k s                   s = float32(2.0 / L), one multiply: the quantized sample, |q - x| mod 2 <= 1 / L
 *   level = k mod L in [0, L) (k < 0: k + L): what the device displays, the phase 2 pi level / L
 *   u = exp(i pi q)           hbx_simulate_phase's own sincos applied to q
 * Ties go to the even k.  This is deliberately not hbx_evaluate_threshold's `>=` rule: the rounding is
 * one instruction, and the quantizer stays odd in x.  A non-finite x gives q = NaN -- its field and
 * gradient are whatever the continuous calls give for a NaN sample -- and level 0, formed by a select.
 *
 * hbx_simulate_phase_levels, hbx_evaluate_phase_levels, hbx_phase_levels_backward: hbx_simulate_phase,
 *   hbx_evaluate_phase and hbx_phase_backward in every rule (shapes, null-ability, the target /
 *   chan_stats pairing, chunking by max_jobs, n_env, HBX_PRECISION_F32 only, the four built sizes, the
 *   pass-timer slots), except that the first pass of the two forward calls quantizes x as it loads it,
 *   and the backward's last pass quantizes x the same way and writes the straight-through gradient
 *     grad_phase = pi (Im g cos pi q - Re g sin pi q),
 *   dq/dx := 1, the continuous chain rule at the displayed phase.  Neither q nor u nor g is ever
 *   written.  Bit for bit, every output of the forward calls equals the continuous call's on the
 *   materialised q (hbx_quantize_phase's out_phase), and grad_phase equals hbx_phase_backward's on q.
 * hbx_quantize_phase: the export for the display and the materialiser, one streaming kernel, no plan.
 *   src        n_values float32 samples x (n_values >= 0)
 *   out_levels n_values uint8 `level`, nullable
 *   out_phase  n_values float32 q, nullable; at least one of the two non-null
 * levels outside [2, 256] ("levels" in hbx_last_error()) or a null required pointer: HBX_ERR_INVALID
 * before anything is enqueued; a reduced-precision plan: HBX_ERR_UNSUPPORTED. */
int hbx_simulate_phase_levels(hbx_plan_t plan, const float* phase, int32_t levels, int32_t n_env,
                              float* field, float* real_part, void* stream);
int hbx_evaluate_phase_levels(hbx_plan_t plan, const float* phase, int32_t levels, const float* target,
                              int32_t n_env, float* field, float* intensity, double* chan_stats,
                              double* psnr, void* stream);
int hbx_phase_levels_backward(hbx_plan_t plan, const float* values, const float* weight, float scale,
                              const float* phase, int32_t levels, int32_t n_env, float* grad_phase,
                              void* stream);
int hbx_quantize_phase(const float* src, int64_t n_values, int32_t levels, uint8_t* out_levels,
                       float* out_phase, void* stream);

/* (ABI v15, additive) Binary holograms from a real leaf: m = [x >= threshold], u = va + vb m with
 * the plan's field_kind (HBX_FIELD_AMPLITUDE: 0 / 1; HBX_FIELD_PHASE: 1 / -1, vb = -2) -- the field
 * of the mask HBX_PACK_THRESHOLD packs from the same samples (NaN: the bit is off).
 *   values[B][G*P][H][W] float32 samples x, one per pixel of every plane, as hbx_evaluate_real's.
 * The first pass thresholds x as it loads it: no 0 / 1 copy of the hologram is ever written, and
 * everything behind the load is hbx_evaluate_real's, so every output equals hbx_evaluate_real's on
 * the materialised samples (x >= threshold ? va + vb : va) bit for bit.
 *
 * hbx_evaluate_threshold: field [B][G*P][H][W][2] complex64, intensity [B][G][H][W], chan_stats
 *   [B][G][3] and psnr [B] are hbx_evaluate_real's, each nullable: target and chan_stats are given
 *   together or not at all, psnr only with a target, and at least one of field, intensity and
 *   chan_stats is non-null (else, or with null values: HBX_ERR_INVALID).  With the intensity alone
 *   the last pass is hbx_intensity_real's lean form.
 * hbx_threshold_backward: the whole backward pass of such a leaf under the straight-through
 *   estimator, on the plan for -z.  The forward pass ran on the thresholded field; the gradient
 *   with respect to that field reaches x through a surrogate derivative s(x) of the step.
 *   values    [B][G*P/2][H][W][2] complex64, weight [B][G][H][W] float32 (nullable) and scale are
 *             hbx_phase_backward's: the first pass is hbx_simulate_complex(_weighted)'s
 *   samples   [B][G*P/2][H][W] float32, the leaf's samples x: complex plane q of this plan is real
 *             plane q of the leaf (a leaf of C real planes runs on the -z plan of 2 C channels)
 *   surrogate HBX_STE_WINDOW   (p0 = lo, p1 = hi): s = 1 for lo <= x <= hi, else 0.  A closed gate
 *                              stores +0.0f whatever g holds; a NaN sample closes it; lo = -inf,
 *                              hi = +inf is the plain straight-through estimator
 *             HBX_STE_SIGMOID  (p0 = the threshold, p1 = k > 0): s = k sg (1 - sg) with
 *                              sg = 1 / (1 + exp(-k (x - p0))), the derivative of the soft step,
 *                              evaluated in float32
 *   grad      [B][G*P/2][H][W] float32 = vb s(x) Re g, g the complex plane hbx_simulate_complex
 *             (_weighted) would write as field, vb the plan's own (1 or -2).  The last pass reads x
 *             and writes the one float; neither g nor its real part is written.
 *   An unknown surrogate, p1 <= 0 for HBX_STE_SIGMOID, or null values, samples or grad:
 *   HBX_ERR_INVALID before anything is enqueued.
 * Chunking by max_jobs, n_env (0: OK, < 0: HBX_ERR_INVALID), HBX_PRECISION_F32 only (else
 * HBX_ERR_UNSUPPORTED), the four built sizes and the pass-timer slots are hbx_evaluate_real's and
 * hbx_phase_backward's. */
#define HBX_STE_WINDOW 0
#define HBX_STE_SIGMOID 1
int hbx_evaluate_threshold(hbx_plan_t plan, const float* values, float threshold,
                           const float* target, int32_t n_env, float* field, float* intensity,
                           double* chan_stats, double* psnr, void* stream);
int hbx_threshold_backward(hbx_plan_t plan, const float* values, const float* weight, float scale,
                           const float* samples, int32_t surrogate, float p0, float p1,
                           int32_t n_env, float* grad, void* stream);

/* (ABI v15, additive) Windows: holograms of any size zero-filled into the plan's N x N grid, and
 * outputs, statistics and gradients taken over a rectangle of it.  A window is a rectangle of the
 * grid, 0 <= y0, 0 <= x0, 1 <= h, 1 <= w, y0 + h <= N, x0 + w <= N, with no alignment requirement; a
 * null window pointer is the full grid.  Arrays that belong to a window are compact, [..][h][w]
 * with row pitch w: no N x N copy of any of them is read or written.
 *   in_win   where the hologram's samples sit.  Outside it the field is 0 (no light), also under
 *            HBX_FIELD_PHASE, whose unset bit is 1 (as the padding slots at N = 896): the first pass
 *            loads a pixel only inside the window and takes zeros elsewhere.
 *   out_win  where the field, the intensity, the statistics and the pixel count n = G h_o w_o of
 *            psnr and of the losses are taken: the last pass stores, reduces and loads its target
 *            row only there, and a row block outside it reads nothing.
 * hbx_evaluate_real_window / hbx_evaluate_threshold_window: values [B][G*P][h_i][w_i] float32;
 *   target and intensity [B][G][h_o][w_o], field [B][G*P][h_o][w_o][2], chan_stats [B][G][3] over
 *   out_win, psnr [B] with n = G h_o w_o.  Null-ability and the target / chan_stats pairing are
 *   hbx_evaluate_threshold's for both calls; with the intensity alone the lean last pass runs.
 *   Every output equals the unwindowed call's on the zero-embedded samples, sliced to out_win, bit
 *   for bit (the statistics: the same pixels' terms, summed in the same order without the others).
 * hbx_backward_window: on the plan for -z.  values [B][G*P/2][h_v][w_v][2] complex64 and the
 *   nullable weight [B][G][h_v][w_v] are embedded at val_win by hbx_simulate_complex(_weighted)'s
 *   first pass; grad [B][G*P/2][h_g][w_g] float32 over grad_win is the real part (samples null:
 *   the gradient of a real leaf) or, with samples [B][G*P/2][h_g][w_g] (the leaf),
 *   hbx_threshold_backward's vb s(x) Re g with the same surrogates and rules.  The forward's
 *   out_win is this call's val_win, the forward's in_win its grad_win.
 * hbx_loss_window / hbx_loss_weight_window: hbx_loss / hbx_loss_weight with n = G h_o w_o and
 *   compact intensity / target / weight [B][G][h_o][w_o].
 * A window outside the grid or with h or w < 1: HBX_ERR_INVALID before anything is enqueued.  Every
 * other rule (null buffers, n_env, chunking by max_jobs, the pass-timer slots, HBX_PRECISION_F32
 * only, the four built sizes) is the unwindowed calls'.
 * Not windowed: complex and phase leaves, the bit path and every env, DBS, plane-cache and
 * incremental entry point, grids larger than 1024; the column pass is unchanged (it does not skip
 * the zero rows). */
typedef struct hbx_window {
  int32_t y0, x0, h, w;
} hbx_window_t;
int hbx_evaluate_real_window(hbx_plan_t plan, const float* values, const hbx_window_t* in_win,
                             const float* target, const hbx_window_t* out_win, int32_t n_env,
                             float* field, float* intensity, double* chan_stats, double* psnr,
                             void* stream);
int hbx_evaluate_threshold_window(hbx_plan_t plan, const float* values, float threshold,
                                  const hbx_window_t* in_win, const float* target,
                                  const hbx_window_t* out_win, int32_t n_env, float* field,
                                  float* intensity, double* chan_stats, double* psnr, void* stream);
int hbx_backward_window(hbx_plan_t plan, const float* values, const float* weight, float scale,
                        const hbx_window_t* val_win, const float* samples, int32_t surrogate,
                        float p0, float p1, const hbx_window_t* grad_win, int32_t n_env,
                        float* grad, void* stream);
int hbx_loss_window(hbx_plan_t plan, const double* chan_stats, const hbx_window_t* out_win,
                    int32_t n_env, int32_t kind, int32_t rel_scale, double* loss, void* stream);
int hbx_loss_weight_window(hbx_plan_t plan, const float* intensity, const float* target,
                           const double* chan_stats, const double* grad_loss,
                           const hbx_window_t* out_win, int32_t n_env, int32_t kind,
                           int32_t rel_scale, float* weight, void* stream);

/* (ABI v15, additive) Focal stacks: one hologram propagated to D depths, 1 <= D <= HBX_MAX_DEPTHS, with
 * the gradient of a loss over all of them.  A plan keeps its own z and table; the stack's depths are a
 * second set of tables on the same plan, and arrays that carry a depth are depth-major -- each depth a
 * contiguous block in the single-depth layout.
 *
 * hbx_plan_set_depths: builds the D transfer-function tables [D][G][N/2+1][N] with hbx_plan_create's own
 *   loop (one copy of it): depth d's table is, bit for bit, the table of a plan created with
 *   optics.z = z[d].  It replaces an earlier set; n_depths = 0 frees the tables (z may then be null).
 *   It synchronises the device, as plan creation does, and is not for use with work in flight.  The
 *   plan's own z, its table and every other call are untouched.  A non-finite z[d], a null z, or
 *   n_depths outside [0, HBX_MAX_DEPTHS]: HBX_ERR_INVALID, and the earlier set stays.
 * hbx_plan_depths: D (0: none set).
 *
 * hbx_evaluate_stack: the forward of every sample leaf kind, named by leaf->kind:
 *   HBX_LEAF_REAL          values [B][G*P][H][W] float32, hbx_evaluate_real's                (Pc = P)
 *   HBX_LEAF_THRESHOLD     the same, hbx_evaluate_threshold's with leaf->threshold           (Pc = P)
 *   HBX_LEAF_COMPLEX       values [B][G*P/2][H][W][2] complex64, hbx_evaluate_complex's      (Pc = P/2)
 *   HBX_LEAF_PHASE         values [B][G*P/2][H][W] float32, hbx_evaluate_phase's             (Pc = P/2)
 *   HBX_LEAF_PHASE_LEVELS  the same, hbx_evaluate_phase_levels' with leaf->levels            (Pc = P/2)
 *   (the leaf's other members are not read by the forward.)
 *   target, intensity [D][B][G][H][W] float32; field [D][B][G*Pc][H][W][2]; chan_stats [D][B][G][3].
 *   Depth d's block of every output equals, bit for bit, what the single-depth call of that kind writes
 *   on a plan created with z = z[d]; nothing outside a depth's block is written.  Null-ability and the
 *   target / chan_stats pairing are hbx_evaluate_threshold's for the two real kinds and
 *   hbx_evaluate_complex's for the other three (there is no psnr output).
 *   Per chunk of max_jobs / G envs the first pass runs ONCE -- the row spectrum it leaves does not depend
 *   on z -- then for d = 0 .. D - 1 the column pass with table d and the single-depth call's own last pass
 *   and reduction into depth d's block: 1 + 2 D pass launches where D calls run 3 D.  The pass-timer
 *   slots get one HBX_PASS_ROWFWD record per chunk and one HBX_PASS_COL and HBX_PASS_ROWINV record per depth.
 *   No depths set on the plan: HBX_ERR_INVALID ("depths" in hbx_last_error()); an unknown kind, a null
 *   leaf or values, levels outside [2, 256] for HBX_LEAF_PHASE_LEVELS: HBX_ERR_INVALID.
 *
 * hbx_backward_stack: the whole backward pass of a leaf under a loss over the stack, on the plan whose
 *   depths are the negated ones (set_depths(-z[d])), one call for all depths.
 *   values  [D][B][G*P/2][H][W][2] complex64: per depth the gradient with respect to the propagated field
 *           or, with weight, the saved field itself; weight [D][B][G][H][W] float32 (nullable) and scale
 *           are hbx_phase_backward's, per depth
 *   leaf    what the one output is, and where: exactly one of grad_field and grad is non-null
 *     HBX_LEAF_COMPLEX       grad_field [B][G*P/2][H][W][2] = sum_d g_d, g_d the plane
 *                            hbx_simulate_complex(_weighted) writes as field on the plan for -z[d]
 *     HBX_LEAF_REAL          grad [B][G*P/2][H][W] float32 = Re sum_d g_d
 *     HBX_LEAF_PHASE         grad = hbx_phase_backward's formula at sum_d g_d, samples the leaf's x
 *     HBX_LEAF_PHASE_LEVELS  grad = hbx_phase_levels_backward's, with leaf->levels
 *     HBX_LEAF_THRESHOLD     grad = hbx_threshold_backward's vb s(x) Re sum_d g_d, with leaf->surrogate,
 *                            leaf->p0 and leaf->p1 as that call takes them
 *   samples [B][G*P/2][H][W] float32, the leaf's x, used exactly as the single-depth backward calls use
 *           it: required for the last three kinds, null for the first two.  The outputs carry no depth.
 *   A chunk holds nj = max_jobs / D jobs (a whole number of envs): depth d's first pass (the unchanged
 *   complex or weighted load) and column pass (table d) run in job slots [d nj, (d + 1) nj) of the plan's
 *   workspace, and ONE depth-summing last pass adds the D slots' rows as it loads them, runs one inverse
 *   row FFT per complex plane and writes the gradient once -- where D single-depth calls run D inverse
 *   FFTs and D stores, and D - 1 read-add-write passes over gradient-sized temporaries follow.  The sum
 *   sits on the recombined side of the pair recombination: the running line starts from depth 0's
 *   recombined value B_0[2q] + i B_0[2q+1] (never from 0.0f) and takes B_d[2q], then i B_d[2q+1], d
 *   ascending, each one float32 addition per component.  D = 1 therefore gives the single-depth backward
 *   call's bits, the sign of a zero included; D > 1 agrees with D single-depth calls added in float32 up
 *   to the order of the additions.  max_jobs < G * D: HBX_ERR_INVALID ("max_jobs" in hbx_last_error())
 *   before anything is enqueued.  Timer slots: D HBX_PASS_ROWFWD and HBX_PASS_COL records and one
 *   HBX_PASS_ROWINV record per chunk.
 *
 * hbx_loss_stack / hbx_loss_weight_stack: hbx_loss / hbx_loss_weight with an env's sums taken over all
 *   D G channels in fixed order (d outer, g inner) and n = D G H W: chan_stats [D][B][G][3] -> loss [B],
 *   and weight [D][B][G][H][W] from intensity and target of that shape.  One least-squares scale per env
 *   for the whole stack (one source power).  D is the plan's.  At D = 1 both give hbx_loss's and
 *   hbx_loss_weight's bits; the degenerate-env rule (an all-zero weight, never a NaN) carries over.
 *
 * Every call with an n_env: 0 is OK and < 0 HBX_ERR_INVALID; the four built sizes.  hbx_evaluate_stack and
 * hbx_backward_stack run on HBX_PRECISION_F32 plans only (else HBX_ERR_UNSUPPORTED); hbx_plan_set_depths and
 * the two loss calls do not look at the plan's precision (as hbx_loss does not).  Out of scope: windows; the bit path and every env, DBS,
 * plane-cache and incremental entry point; reduced-precision plans; per-depth wavelengths or pitches;
 * more than HBX_MAX_DEPTHS depths; summing in the column pass. */
#define HBX_MAX_DEPTHS 8
#define HBX_LEAF_REAL 0          /* hbx_evaluate_real's input            */
#define HBX_LEAF_THRESHOLD 1     /* hbx_evaluate_threshold's (threshold)  */
#define HBX_LEAF_COMPLEX 2       /* hbx_evaluate_complex's                */
#define HBX_LEAF_PHASE 3         /* hbx_evaluate_phase's                  */
#define HBX_LEAF_PHASE_LEVELS 4  /* hbx_evaluate_phase_levels' (levels)   */
typedef struct hbx_leaf {
  int32_t kind, levels;
  float threshold;
  int32_t surrogate;
  float p0, p1;
} hbx_leaf_t;
int hbx_plan_set_depths(hbx_plan_t plan, const double* z, int32_t n_depths);
int hbx_plan_depths(hbx_plan_t plan);
int hbx_evaluate_stack(hbx_plan_t plan, const void* values, const hbx_leaf_t* leaf, const float* target,
                       int32_t n_env, float* field, float* intensity, double* chan_stats, void* stream);
int hbx_backward_stack(hbx_plan_t plan, const float* values, const float* weight, float scale,
                       const hbx_leaf_t* leaf, const float* samples, int32_t n_env, float* grad_field,
                       float* grad, void* stream);
int hbx_loss_stack(hbx_plan_t plan, const double* chan_stats, int32_t n_env, int32_t kind,
                   int32_t rel_scale, double* loss, void* stream);
int hbx_loss_weight_stack(hbx_plan_t plan, const float* intensity, const float* target,
                          const double* chan_stats, const double* grad_loss, int32_t n_env, int32_t kind,
                          int32_t rel_scale, float* weight, void* stream);

/* (ABI v15, additive) EXTENSION, no reference counterpart beyond its rectangular crop before the comparison
 * (env_1024_24_128.py:144-149): per-pixel loss weights -- a signal window plus a don't-care region, or any
 * non-negative weighting, for every leaf kind at one depth and over a focal stack.  A constant weight v of the
 * target's shape enters the three float64 sums the last pass leaves and everything downstream of them:
 *     S_xy = sum v I T    S_xx = sum v I^2    S_yy = sum v T^2    W = sum v   (per env)
 * hbx_loss's formulas hold with the pixel count n replaced by W, and dL/dI = v (a I + c T) with a and c per env
 * as hbx_loss_weight forms them, W for n.  The intensity and the field that are written stay the unweighted
 * ones.  Each term is formed in float64 as vI = (double)v (double)I and vT = (double)v (double)T (exact:
 * 24 + 24 bits), sxy = fma(vI, T, sxy), sxx = fma(vI, I, sxx), syy = fma(vT, T, syy), in the unweighted last
 * pass's order (the lane's pixels, the group's lanes, the block's rows): a pixel with v = 1 adds the unweighted
 * term bit for bit and one with v = 0 leaves the sums unchanged, so v = 1 everywhere gives the unweighted
 * calls' chan_stats and v = the indicator of a rectangle gives hbx_evaluate_*_window's over that out_win.
 *
 * hbx_evaluate_pw: the single-depth forward of every sample leaf kind, named through hbx_leaf_t as
 *   hbx_evaluate_stack names them (HBX_LEAF_REAL: hbx_evaluate_real, _THRESHOLD: hbx_evaluate_threshold with
 *   leaf->threshold, _COMPLEX: hbx_evaluate_complex, _PHASE: hbx_evaluate_phase, _PHASE_LEVELS:
 *   hbx_evaluate_phase_levels with leaf->levels), `values` as that call takes them.  Every rule of that call
 *   holds, except that target, pixel_weight [B][G][H][W] float32 and chan_stats [B][G][3] are required; field
 *   and intensity are nullable and are the unweighted call's bit for bit.  There is no psnr output.
 * hbx_evaluate_stack_pw: hbx_evaluate_stack with pixel_weight [D][B][G][H][W]; depth d's last pass takes depth
 *   d's block.  target, pixel_weight and chan_stats [D][B][G][3] are required.  Depth d's outputs equal
 *   hbx_evaluate_pw's on a plan for z[d] with that block, bit for bit.
 * hbx_pixel_weight_sum: weight_sum [B] float64 = the sum of an env's G images of pixel_weight (n_depths = 0:
 *   [B][G][H][W]) or of its D G images (n_depths = D >= 1, which must be the plan's: [D][B][G][H][W], d outer,
 *   g inner), a fixed-order float64 reduction, bitwise reproducible; a sum of ones is exact, so it is G H W for
 *   v = 1 and G h w for a rectangle's indicator.
 * hbx_loss_pw / hbx_loss_weight_pw: hbx_loss / hbx_loss_weight (n_depths = 0) or hbx_loss_stack /
 *   hbx_loss_weight_stack (n_depths = the plan's D) with weight_sum [B] where those calls use n, and
 *   weight = pixel_weight * (a I + c T): the same coefficients and fmaf, one more float32 multiply.  At v = 1
 *   both give the unweighted calls' bits.  An env with W = 0 (an all-zero weight) follows the degenerate-env
 *   rule: its MSE is 0, its PSNR +inf and its loss weight all zero, never a NaN.
 * The backward pass needs no new call: weight goes into hbx_simulate_complex_weighted, hbx_phase_backward,
 * hbx_phase_levels_backward, hbx_threshold_backward and hbx_backward_stack as the unweighted loss weight does.
 *
 * Undefined, and not checked (a check would cost a host wait): a negative weight is the caller's business (the
 * formulas are applied as they stand); a NaN weight poisons that env's statistics and loss; a non-finite I or T
 * under v = 0 gives NaN.  Null required pointers, an unknown leaf kind, levels outside [2, 256] and an n_depths
 * that is neither 0 nor the plan's: HBX_ERR_INVALID before anything is enqueued; a reduced-precision plan:
 * HBX_ERR_UNSUPPORTED (the two evaluate calls; the other three do not look at the precision, as hbx_loss does
 * not); n_env 0 is OK and < 0 HBX_ERR_INVALID.  Out of scope: windows together with weights; the bit path and
 * every env, DBS, plane-cache and incremental entry point; hbx_rel_stats; a weighted intensity; a weighted psnr
 * output of the evaluate calls; a differentiable weight. */
int hbx_evaluate_pw(hbx_plan_t plan, const void* values, const hbx_leaf_t* leaf, const float* target,
                    const float* pixel_weight, int32_t n_env, float* field, float* intensity,
                    double* chan_stats, void* stream);
int hbx_evaluate_stack_pw(hbx_plan_t plan, const void* values, const hbx_leaf_t* leaf, const float* target,
                          const float* pixel_weight, int32_t n_env, float* field, float* intensity,
                          double* chan_stats, void* stream);
int hbx_pixel_weight_sum(hbx_plan_t plan, const float* pixel_weight, int32_t n_env, int32_t n_depths,
                         double* weight_sum, void* stream);
int hbx_loss_pw(hbx_plan_t plan, const double* chan_stats, const double* weight_sum, int32_t n_env,
                int32_t n_depths, int32_t kind, int32_t rel_scale, double* loss, void* stream);
int hbx_loss_weight_pw(hbx_plan_t plan, const float* intensity, const float* target, const float* pixel_weight,
                       const double* chan_stats, const double* weight_sum, const double* grad_loss,
                       int32_t n_env, int32_t n_depths, int32_t kind, int32_t rel_scale, float* weight,
                       void* stream);

/* (ABI v15, additive) EXTENSION, no reference counterpart: illumination fields.  Every other entry point lights
 * the modulator with a unit plane wave on axis, u = f(x) with f the leaf kind's map.  Here it is lit by a
 * constant complex source, source [G][H][W] complex64, shared by all envs and all planes of a colour group:
 * an oblique plane wave, a Gaussian beam, a converging reference wave, a lit disc (0 outside).  With
 * s = (sr, si) the source sample and f = (fr, fi) the leaf's unsourced sample at a pixel, in float32 with every
 * product rounded on its own (no other contraction):
 *     forward   u.re  = fmaf(fr, sr, -(fi * si))        u.im  = fmaf(fr, si, fi * sr)
 *               (HBX_LEAF_REAL / _THRESHOLD: fi is absent, not 0:  u = (fr * sr, fr * si), one multiply each)
 *     backward  g'.re = fmaf(g.re, sr, g.im * si)       g'.im = fmaf(g.im, sr, -(g.re * si))      g' = conj(s) g
 * g = the plane the complex last pass would write on the plan for -z; the leaf's gradient is the existing
 * formula at g': complex g', real Re g', phase and L-level pi (Im g' cos pi q - Re g' sin pi q), thresholded
 * vb ste(x) Re g' with both surrogates.  The source is a constant and has no gradient.  At N = 896 the padding
 * slots stay 0.
 *
 * Layout: in these three calls every leaf kind, real and thresholded included, is ONE complex plane per leaf
 * plane: values [B][G*P/2][H][W] (complex64 pairs for HBX_LEAF_COMPLEX, float32 otherwise) on a plan of P real
 * planes per group -- hbx_evaluate_stack's Pc = P/2, here for all five kinds.  An odd number of leaf planes per
 * group needs no padding plane.
 *
 * hbx_source_field: the field at the modulator, out_field [B][G*P/2][H][W][2] = u, one streaming kernel with the
 *   device functions the first pass uses (no propagation).
 * hbx_evaluate_source: the first pass forms u as it loads the leaf's samples and the source row, then the
 *   column pass and hbx_evaluate_complex's last pass and reduction as they are.  Null-ability and the target /
 *   chan_stats pairing are hbx_evaluate_complex's (no psnr output); pixel_weight [B][G][H][W] is nullable and
 *   follows hbx_evaluate_pw's rules when given (target and chan_stats required).  Every output equals
 *   hbx_evaluate_complex's (hbx_evaluate_pw's with HBX_LEAF_COMPLEX) on hbx_source_field's output, bit for bit.
 * hbx_backward_source: on the plan for -z.  values [B][G*P/2][H][W][2], optionally times scale * weight
 *   [B][G][H][W] (hbx_simulate_complex_weighted's load), the column pass, and a last pass that multiplies the
 *   plane by conj(s) before the leaf's formula.  Exactly one of grad_field [B][G*P/2][H][W][2] (HBX_LEAF_COMPLEX)
 *   and grad [B][G*P/2][H][W] float32 (every other kind) is non-null; samples [B][G*P/2][H][W] float32 is the
 *   leaf's x for the phase, L-level and thresholded kinds and null otherwise; leaf carries levels / surrogate /
 *   p0 / p1 as hbx_backward_stack reads them.  A closed HBX_STE_WINDOW gate stores +0.0 whatever g' holds.
 * All three: chunked by max_jobs as their siblings; n_env 0 is OK, < 0 HBX_ERR_INVALID; the four built sizes;
 *   the pass-timer slots are the siblings'.  A null source, values or leaf, an unknown kind or levels outside
 *   [2, 256]: HBX_ERR_INVALID before anything is enqueued; a reduced-precision plan: HBX_ERR_UNSUPPORTED.
 * Out of scope: a source on the bit path or on any env, DBS, plane-cache or incremental entry point; a source
 *   with windows or focal stacks (the depth-summing last pass); a gradient with respect to the source;
 *   reduced-precision plans; a per-env or per-plane source; grids other than the four built. */
int hbx_source_field(hbx_plan_t plan, const void* values, const hbx_leaf_t* leaf, const float* source,
                     int32_t n_env, float* out_field, void* stream);
int hbx_evaluate_source(hbx_plan_t plan, const void* values, const hbx_leaf_t* leaf, const float* source,
                        const float* target, const float* pixel_weight, int32_t n_env, float* field,
                        float* intensity, double* chan_stats, void* stream);
int hbx_backward_source(hbx_plan_t plan, const float* values, const float* weight, float scale,
                        const hbx_leaf_t* leaf, const float* source, const float* samples, int32_t n_env,
                        float* grad_field, float* grad, void* stream);

/* PSNR from per-channel statistics (tt.relativeLoss(.., tm.get_PSNR),
 * env.py:174): chan_stats[B][G][3] -> psnr[B]. */
int hbx_psnr(hbx_plan_t plan, const double* chan_stats, int32_t n_env, double* psnr,
             void* stream);

/* Env reset tail (env.py:120-133): given env.mask already thresholded and
 * env.target set for the listed envs (env_ids nullable = all n_env), propagate
 * every group, fill chan_stats / intensity (and env.field when non-null),
 * set init_psnr = prev_psnr and zero steps / flip_count / sustained / record,
 * max_psnr_diff = -inf. */
int hbx_env_reset(hbx_plan_t plan, const hbx_env_buffers_t* env, int32_t n_env,
                  const int32_t* env_ids, int32_t n_ids, void* stream);

/* Batched env.step(action) (env.py:154-259 mono; DBS_1024_24.py:313-422
 * per-flip RGB with cached other-group statistics).  One action per env:
 * decode (env.py:157-161), flip + record, re-propagate the touched colour
 * group, relative PSNR, reward = RW * delta, rollback / bonus / termination.
 *   reward, psnr [B] f64; accepted, terminated, truncated [B] u8 (nullable; device
 *   addresses, e.g. of hbx_host_alloc'd host-mapped memory -- ABI v11: the kernels then
 *   write the results straight to the host, readable once the stream work is done)
 *   group_intensity [B][H][W] f32: the stepped (pre-rollback) group mean
 *   (nullable; not together with env->recon, which already holds it).
 * With env->recon (ABI v8) the last pass writes the stepped intensity straight
 * into recon[b][g] and the step starts by reconciling the previous step's
 * group (one N^2 f32 copy per env); without it, accepted steps refresh
 * env->intensity[b][g] when that cache is non-null.  env->state_bytes, when
 * non-null, follows every accepted flip. */
int hbx_env_step(hbx_plan_t plan, const hbx_env_buffers_t* env, const hbx_env_params_t* params,
                 int32_t n_env, const int64_t* actions, double* reward, double* psnr,
                 uint8_t* accepted, uint8_t* terminated, uint8_t* truncated,
                 float* group_intensity, void* stream);

/* DBS primitive (SURVEY 8b hbx_step): one candidate flip per env evaluated
 * against prev_psnr and applied iff accepted (accept_rule), without the
 * env's reward bookkeeping (DBS.py:247-294). */
int hbx_step(hbx_plan_t plan, uint64_t* mask, const int64_t* actions, int32_t n_env,
             const float* target, double* chan_stats, double* prev_psnr, double* psnr_out,
             uint8_t* accepted, int32_t accept_rule, void* stream);

/* Independent trial flips against ONE fixed base env (probe sweep
 * DBS_1024_24-128.py:310-373, range.py:294-335, env_group.py:96-120 and the
 * speculative batches of greedy DBS): for k < K
 *   psnr_out[k]      = PSNR with pixel flips[k] toggled
 *   group_stats[k][3] = stats of the touched group (nullable)            */
int hbx_eval_flips(hbx_plan_t plan, const uint64_t* base_mask, const float* target,
                   const double* base_chan_stats, const int64_t* flips, int32_t K,
                   double* psnr_out, double* group_stats, void* stream);

/* PSNR change of EVERY single-pixel flip of one env against its current
 * state, all CH*H*W of them at once (the full probe sweep
 * DBS_1024_24-128.py:310-373 / range.py:294-335 and env_group.py:90-143's
 * sampled importance pass, without one propagation per flip):
 *   dpsnr[c][r][col] = PSNR(state with (c, r, col) toggled) - PSNR(state)
 * By linearity a flip adds delta * h_g(. - x0) to one plane's field, so the
 * new (sum I T, sum I^2) are correlations of functions of the fields, the
 * intensity and the target with functions of the single-pixel field h_g,
 * evaluated with 2-D FFTs (hbx_map.hip).  mask [CH][H][W/64], target
 * [G][H][W] (one env), dpsnr [CH][H][W] f32, base_psnr (nullable) f64. */
int hbx_flip_map(hbx_plan_t plan, const uint64_t* mask, const float* target, float* dpsnr,
                 double* base_psnr, void* stream);

/* Commit one accepted candidate of hbx_eval_flips into the base env:
 * toggle mask bit `flips[k]`, chan_stats[g] = group_stats[k], prev_psnr =
 * psnr_out[k].  Device-side; `k` is a device int32 (from the host or a
 * device search); K (ABI v6) is the length of flips / psnr_out / group_stats:
 * a k outside [0, K) commits nothing. */
int hbx_commit_flip(hbx_plan_t plan, uint64_t* base_mask, double* base_chan_stats,
                    double* prev_psnr, const int64_t* flips, const double* psnr_out,
                    const double* group_stats, const int32_t* k, int32_t K, void* stream);

/* (ABI v10) hbx_eval_flips / hbx_commit_flip with the base env's per-plane
 * |U_p|^2 cached (N = 1024 / 256): the speculative greedy DBS of
 * DBS_1024_24.py:313-363 in the FFT mode, bit for bit, at a fraction of the
 * bytes.  A candidate flips one plane, so only that plane's PAIR (the two
 * planes one complex row FFT carries) is propagated; the group intensity sums
 * the cached planes and the pair's fresh ones in the FFT mode's plane order,
 * i.e. the same f32 sum.  Candidate k writes its pair's fresh |U|^2 to spare
 * pair k of the pool; committing candidate k swaps that pair's slots in.
 *   plane_inten [CH + 2 S][H][W] f32, plane_slot [CH + 2 S] int32 (S =
 *   n_spare_pairs >= K): filled by hbx_planes_fill from the base mask
 *   (identity slots, every plane's |U|^2, the base chan_stats / psnr).
 * Replaces the per-flip tt.simulate of the whole colour group
 * (DBS_1024_24.py:326-332) in speculative batches. */
int hbx_planes_fill(hbx_plan_t plan, const uint64_t* mask, const float* target, float* plane_inten,
                    int32_t* plane_slot, int32_t n_spare_pairs, double* chan_stats, double* psnr,
                    void* stream);
int hbx_eval_flips_planes(hbx_plan_t plan, const uint64_t* base_mask, const float* target,
                          const double* base_chan_stats, float* plane_inten, const int32_t* plane_slot,
                          int32_t n_spare_pairs, const int64_t* flips, int32_t K, double* psnr_out,
                          double* group_stats, void* stream);
int hbx_commit_flip_planes(hbx_plan_t plan, uint64_t* base_mask, double* base_chan_stats,
                           double* prev_psnr, int32_t* plane_slot, int32_t n_spare_pairs,
                           const int64_t* flips, const double* psnr_out, const double* group_stats,
                           const int32_t* k, int32_t K, void* stream);


/* hbx_eval_flips / hbx_commit_flip on the incremental-field path: the base
 * env additionally carries its per-plane field [CH][H][W][2] and group
 * intensities [G][H][W] (hbx_simulate), so a candidate costs one streaming
 * pass over one plane (no FFT) -- the speculative greedy DBS of
 * DBS_1024_24.py:313-422 at ~16 B/px per candidate.  The commit also rewrites
 * the accepted plane's field and its group intensity. */
int hbx_eval_flips_psf(hbx_plan_t plan, const uint64_t* base_mask, const float* target,
                       const double* base_chan_stats, const float* field, const float* intensity,
                       const int64_t* flips, int32_t K, double* psnr_out, double* group_stats,
                       void* stream);
int hbx_commit_flip_psf(hbx_plan_t plan, uint64_t* base_mask, double* base_chan_stats,
                        double* prev_psnr, float* field, float* intensity, const int64_t* flips,
                        const double* psnr_out, const double* group_stats, const int32_t* k,
                        int32_t K, void* stream);

/* Device-resident greedy DBS walk (ABI v5): the whole loop of DBS.py:247-294 /
 * DBS_1024_24.py:313-422 -- visit order[pos..], keep a flip iff PSNR strictly
 * improves -- as speculative batches that never return to the host.  Each
 * batch evaluates the next K candidates on the incremental-field path (as
 * hbx_eval_flips_psf); a one-block launch picks the first improving one in
 * visiting order, toggles its mask bit, updates base_chan_stats and the walk
 * state and appends (position, psnr) to the accept log; a third launch
 * rewrites the accepted plane's field and group intensity.  `batches` batches
 * are enqueued per call with no host synchronisation; batches after the walk
 * is done (or halted) cost three empty launches.  The accept sequence is the
 * serial loop's: every candidate before an accepted one was evaluated against
 * exactly the state the serial loop would have had.
 *
 * ABI v7: for K in 1..4 a batch is ONE launch (k_walk_step):
 * it first applies the previous batch's accepted flip(s) to field / intensity,
 * evaluates the K candidates on the updated state, and its last-arriving
 * workgroup decides; for K = 2..4 it also resolves the first candidate after
 * the first accept against the state WITH that accept (exact pairwise terms),
 * so a batch takes up to two accepts of the serial loop.  The accepted flips of
 * a batch therefore reach field / intensity in the NEXT launch: after the walk
 * is done make one more call (batches >= 1; it only commits).  K > 4 runs the
 * three-launch batch of ABI v5 (eval / decide / commit; also selected for every
 * K by HBX_WALK_SPLIT=1 in the environment at plan creation); a call that
 * switches from the one-launch to the three-launch form first issues one
 * commit-only step for the pending accepts.
 *
 * The walk state lives in DEVICE memory (caller-owned; commit_ch = -1,
 * commit2_ch1 = 0, split_ch1 = 0 and the counters zero at the start); the caller reads it back
 * between calls.  When halt == 1 (after every refresh_every-th accept) the
 * caller re-propagates field, intensity and base_chan_stats exactly
 * (hbx_simulate / hbx_propagate) -- the mask already holds every accepted flip,
 * so it also drops pending commits (commit_ch = -1, commit2_ch1 = 0) -- sets
 * prev_psnr to the exact PSNR and clears halt.
 * n_order (ABI v6) is the length of `order`: the walk never visits past
 * min(walk->total, n_order).
 * The walk's partial sums, arrival counters and decoded next actions live in
 * plan-owned scratch: at most one walk per plan may be in flight at a time
 * (walks of several images side by side need one plan each, as
 * hbx.dbs.greedy_many enforces); each call re-derives the decoded actions
 * from `order` once, so a new walk on the same plan needs no reset.
 *
 * Candidate evaluation is in increment form: each candidate's f64 partials
 * are sum dI T and sum (2 I + dI) dI with dI = delta (2 Re(U conj h) +
 * delta |h|^2) / P formed in f32 per pixel, added to base_chan_stats -- the
 * decision carries the increment's own f32 precision (~1e-13 dB at 1024x24),
 * not the rounding of full-image sums. */
typedef struct hbx_dbs_walk {
  int64_t pos;             /* next position of `order` to visit                  */
  int64_t total;           /* positions to visit (order length or a prefix)      */
  int64_t accepted;        /* accepts so far (log entries written: min(., cap))  */
  int64_t batches;         /* speculative batches evaluated                      */
  double prev_psnr;        /* PSNR of the current base                           */
  double init_psnr;        /* PSNR at the start of the walk                      */
  double last_psnr;        /* PSNR of the last visited candidate                 */
  double stop_diff;        /* DBS_ratio_0.5.py:366-372 early stop threshold      */
  int32_t stop_enabled;    /* 1: done once prev_psnr - init_psnr >= stop_diff    */
  int32_t refresh_every;   /* halt after every refresh_every-th accept (0: never) */
  int32_t done;            /* 1: pos == total, or stopped early                  */
  int32_t halt;            /* 1: paused for an exact refresh (caller clears)     */
  int32_t stopped_early;
  int32_t commit_ch;       /* internal: pending commit channel, -1 = none        */
  int32_t commit_pix;      /* internal                                           */
  int32_t commit2_ch1;     /* internal (ABI v7): channel + 1 of a second pending
                              commit, 0 = none                                   */
  int32_t commit_pix2;     /* internal                                           */
  int32_t split_ch1;       /* internal (ABI v7): channel + 1 of the split batch's
                              accept, applied within the batch, 0 = none          */
  int32_t split_pix;       /* internal                                           */
  int32_t fault;           /* (r03) 1: a persistent walk launch's grid barrier timed
                              out (done is set too; the state is unreliable)     */
} hbx_dbs_walk_t;
int hbx_dbs_walk_psf(hbx_plan_t plan, uint64_t* base_mask, const float* target,
                     double* base_chan_stats, float* field, float* intensity, const int64_t* order,
                     int64_t n_order, hbx_dbs_walk_t* walk, int64_t* accept_pos, double* accept_psnr,
                     int64_t accept_cap, int32_t K, int32_t batches, void* stream);

/* (ABI v10) The same greedy DBS with the decision on the device: `batches`
 * speculative batches of K candidates (order[pos .. pos + K)) are enqueued
 * without a host round trip; after each batch's propagation one block forms
 * the K PSNRs (as hbx_eval_flips_planes), commits the first strict improvement
 * (as hbx_commit_flip_planes) into base_mask / base_chan_stats / plane_slot,
 * logs it (accept_pos / accept_psnr, up to accept_cap) and advances the walk
 * state (hbx_dbs_walk_t: pos, total, accepted, batches, prev / init / last
 * PSNR, stop_enabled / stop_diff, done, stopped_early; the incremental-walk
 * fields are unused).  Batches after `done` are no-ops.  K <= n_spare_pairs,
 * max_jobs and 256.  The accept sequence and every logged PSNR are the
 * host-decided batches' (and the full re-propagation's) bit for bit. */
int hbx_dbs_walk_planes(hbx_plan_t plan, uint64_t* base_mask, const float* target,
                        double* base_chan_stats, float* plane_inten, int32_t* plane_slot,
                        int32_t n_spare_pairs, const int64_t* order, int64_t n_order,
                        hbx_dbs_walk_t* walk, int64_t* accept_pos, double* accept_psnr,
                        int64_t accept_cap, int32_t K, int32_t batches, void* stream);

/* (ABI v13) EXTENSION, no reference counterpart (DBS_ratio_0.5.py has no on-pixel
 * constraint; BASELINE configs[4] names one): hbx_dbs_walk_planes under an on-pixel ratio
 * constraint.  fill_count[G] (device, caller-initialised) holds each colour group's on-pixel
 * count over its P planes; a candidate that moves group g's count C by d = +1 (pixel 0 -> 1) or
 * -1 is admissible iff |C + d - fill_target| <= fill_tol or |C + d - fill_target| < |C -
 * fill_target|.  An inadmissible candidate is visited and rejected without a propagation (no
 * PSNR); an accepted one updates fill_count.  fill_count NULL: hbx_dbs_walk_planes.  The
 * host-decided batches of hbx.dbs.greedy(..., fill_ratio=) apply the same rule. */
int hbx_dbs_walk_planes_fill(hbx_plan_t plan, uint64_t* base_mask, const float* target,
                             double* base_chan_stats, float* plane_inten, int32_t* plane_slot,
                             int32_t n_spare_pairs, const int64_t* order, int64_t n_order,
                             hbx_dbs_walk_t* walk, int64_t* accept_pos, double* accept_psnr,
                             int64_t accept_cap, int32_t K, int32_t batches, int64_t* fill_count,
                             int64_t fill_target, int64_t fill_tol, void* stream);

/* (ABI v15, additive) EXTENSION, no reference counterpart (the reference has the strict rule alone,
 * DBS_1024_24.py:355): the device walk under a per-candidate acceptance slack -- simulated
 * annealing, threshold accepting and a minimum-gain rule in one predicate.  slack[n_slack] float64
 * (device), one value per position of `order`; the candidate at position q is accepted iff
 *     psnr_q > (prev_psnr - slack[q])      in float64: one subtraction, rounded once, then the compare
 * (hbx.dbs.first_accepting, the host-decided batches of hbx.dbs.greedy with slack=, is the same
 * expression, so both give the same accept sequence bit for bit).  slack 0: the greedy rule.  A NaN
 * slack rejects its candidate; +inf accepts every candidate that has a PSNR; a negative slack -g
 * demands an improvement of more than g.  Under fill_count an inadmissible candidate has no PSNR and
 * is rejected whatever its slack; both rules apply.  stop_diff stays where the walk has it: checked
 * when a candidate is accepted, psnr - init_psnr >= stop_diff; a candidate its slack rejects does not
 * stop the walk.  prev_psnr is the CURRENT state's PSNR, no longer the best seen: the best state is
 * recovered from the accept log (hbx.dbs.replay), no kernel tracks it.
 * n_slack < n_order: HBX_ERR_INVALID (the message names the slack), checked before anything is enqueued;
 * the device reads no slack at or past n_slack (or the walk's total).  slack NULL: this is
 * hbx_dbs_walk_planes_fill, kernel for kernel.  Every other rule is that call's: K bounds, one walk per
 * plan, batches after `done` are no-ops, the precision modes.  hbx_dbs_walk_t is unchanged. */
int hbx_dbs_walk_planes_anneal(hbx_plan_t plan, uint64_t* base_mask, const float* target,
                               double* base_chan_stats, float* plane_inten, int32_t* plane_slot,
                               int32_t n_spare_pairs, const int64_t* order, int64_t n_order,
                               hbx_dbs_walk_t* walk, int64_t* accept_pos, double* accept_psnr,
                               int64_t accept_cap, int32_t K, int32_t batches, int64_t* fill_count,
                               int64_t fill_target, int64_t fill_tol, const double* slack,
                               int64_t n_slack, void* stream);

/* Incremental-field ("PSF") mode (reported separately from
 * the FFT-mode headline).  tt.simulate is linear, so flipping pixel (c, r, col)
 * changes only plane c's field, by delta * h_g shifted to (r, col), where
 * h_g = IFFT2(H_g) is the single-pixel field and delta = vb * (1 - 2 bit_old):
 *   U_c' = U_c + delta h_g(y - r, x - col),  I_g' = I_g + (|U_c'|^2 - |U_c|^2) / P
 * The step streams U_c, I_g and the target channel once (no FFT), then the
 * same reward / accept / rollback tail as hbx_env_step; accepted steps
 * rewrite U_c and I_g.  Requires env->field and env->intensity, filled by
 * hbx_env_reset (or hbx_field_refresh) with the exact FFT path. */
int hbx_env_step_psf(hbx_plan_t plan, const hbx_env_buffers_t* env, const hbx_env_params_t* params,
                     int32_t n_env, const int64_t* actions, double* reward, double* psnr,
                     uint8_t* accepted, uint8_t* terminated, uint8_t* truncated, void* stream);

/* (ABI v8) Rebuild the observation mirrors of the listed envs (env_ids
 * nullable = all n_env) from the state they mirror:
 *   HBX_OBS_STATE  state_bytes <- the mask bits
 *   HBX_OBS_RECON  recon <- intensity, recon_pending <- 0; the intensity cache is
 *                  taken as authoritative (it was just rewritten: reset, checkpoint load).
 *                  ABI v12, G = 1: intensity is first re-propagated from the mask (the
 *                  step keeps no cache at one group; needs env->target)
 *   HBX_OBS_RESOLVE (ABI v10, with HBX_OBS_RECON) apply the last step's pending
 *                  reconcile first: after an accepted step the stepped group's new
 *                  intensity lives in recon only (recon_pending = group + 1), so that
 *                  group goes recon -> intensity and the others intensity -> recon.
 *                  Use it to re-sync mid-episode without rewriting intensity.
 *   HBX_OBS_SETTLE (ABI v11, alone) the accepted half of that reconcile only: envs
 *                  whose last step was accepted (recon_pending > 0) copy the stepped
 *                  group recon -> intensity and clear recon_pending; recon is not
 *                  touched (it is still the observation the step returned), rolled-back
 *                  envs keep their pending restore for the next step.  A VecEnv queues
 *                  it right behind the step's readback, so the copy runs while the host
 *                  turns the step around instead of inside the next step's k_rowinv.
 *                  ABI v12: a no-op at G = 1 (nothing is pending).
 * hbx_env_reset does both for the envs it resets; a caller that restores
 * masks or intensities by itself (checkpoint load) calls it after. */
#define HBX_OBS_STATE 1
#define HBX_OBS_RECON 2
#define HBX_OBS_RESOLVE 4
#define HBX_OBS_SETTLE 8
int hbx_env_obs_sync(hbx_plan_t plan, const hbx_env_buffers_t* env, int32_t n_env,
                     const int32_t* env_ids, int32_t n_ids, int32_t what, void* stream);

/* Exact re-propagation (FFT path) of env->field, env->intensity and
 * env->chan_stats for the listed envs (bounds the fp32 drift of the
 * incremental updates; counters and PSNR history are left untouched).
 * ABI v9: with env->plane_inten / plane_slot (and no field) it rebuilds the
 * plane cache instead (after a checkpoint load). */
int hbx_field_refresh(hbx_plan_t plan, const hbx_env_buffers_t* env, int32_t n_env,
                      const int32_t* env_ids, int32_t n_ids, void* stream);

/* Precision of the propagation intermediates (ABI v6; SURVEY 8d cfg 5,
 * DBS_ratio_0.5.py fp32-vs-bf16 sweep).  HBX_PRECISION_F32 is the product
 * path.  HBX_PRECISION_BF16_STORE / HBX_PRECISION_F16_STORE round every value
 * written to the two pass intermediates (row spectrum, column-pass output) to
 * bf16 / fp16 -- the numerics of half-width intermediate storage, measured
 * against f32 by tools/precision_sweep.py and bench.py (layout and traffic
 * stay f32).  N = 64 / 256 / 1024 three-pass path only (HBX_ERR_UNSUPPORTED
 * elsewhere). */
#define HBX_PRECISION_F32 0
#define HBX_PRECISION_BF16_STORE 1
#define HBX_PRECISION_F16_STORE 2
int hbx_plan_set_precision(hbx_plan_t plan, int32_t precision);
int hbx_plan_precision(hbx_plan_t plan);

/* Optional device timing of the three propagation passes (hipEvents recorded
 * on the launch stream around every pass launch; not for graph capture).
 * capacity = max launches recorded per pass before hbx_plan_read_timing;
 * 0 disables.  Replaces debug_env.py:165-306's per-phase time.time() prints. */
#define HBX_PASS_ROWFWD 0
#define HBX_PASS_COL 1
#define HBX_PASS_ROWINV 2
#define HBX_PASS_PSF_EVAL 3
#define HBX_PASS_PSF_COMMIT 4
#define HBX_NUM_PASSES 5
int hbx_plan_set_timing(hbx_plan_t plan, int32_t capacity);
/* As hbx_plan_set_timing, recording only every `every`-th launch of each pass
 * (every >= 1; 1 = hbx_plan_set_timing).  Each event pair costs a few us of
 * stream time (the record's release), a visible share of a 0.35 ms 256x256x8
 * step: sampling keeps the timed loop's step time within noise of an untimed
 * one while the recorded launches are still those of that loop. */
int hbx_plan_set_timing_sampled(hbx_plan_t plan, int32_t capacity, int32_t every);
/* Waits for the recorded events; ms_total[HBX_NUM_PASSES] = summed kernel
 * time, launches[HBX_NUM_PASSES], jobs[HBX_NUM_PASSES] = summed jobs per
 * launch; then clears the record. */
int hbx_plan_read_timing(hbx_plan_t plan, double* ms_total, int64_t* launches, int64_t* jobs);

/* (ABI v14) Mask -> bits on the device, one streaming pass (hbx_pack.hip).  Replaces the
 * per-call host / torch work in front of every propagation: env reset's `state =
 * (pre_model >= 0.5)` (env.py:120, env_1024_24.py:120-124) and the float / int8 mask that
 * tt.simulate receives (env.py:123,170-171 `tt.Tensor(torch.tensor(state, float32))`;
 * DBS_1024_24.py:326-327).
 *   src      `n_values` contiguous values of kind src_kind (HBX_SRC_U8: bool / int8 / uint8
 *            bytes; HBX_SRC_F32; HBX_SRC_F64), aligned to 4 (u8) / 16 (f32) / 32 (f64) bytes;
 *            n_values % 64 == 0 (rows of W values with W % 64 == 0 are contiguous words)
 *   bits     n_values / 64 words in the mask layout above (bit j of word w = value 64 w + j)
 *   mode     HBX_PACK_BINARY: bit = (v != 0); a value that is not 0 or 1 (NaN included)
 *            stores 1 into *error (nullable; any address the kernel may write, e.g. host
 *            memory from hbx_host_alloc, so the check needs no device -> host copy).
 *            HBX_PACK_THRESHOLD: bit = (v >= threshold) (NaN -> 0, as torch's `>=`).
 * Runs on the current device, asynchronously on `stream`; no plan needed. */
#define HBX_SRC_U8 0
#define HBX_SRC_F32 1
#define HBX_SRC_F64 2
#define HBX_PACK_BINARY 0
#define HBX_PACK_THRESHOLD 1
int hbx_pack_mask(const void* src, int32_t src_kind, int64_t n_values, int32_t mode, double threshold,
                  uint64_t* bits, int32_t* error, void* stream);

/* (ABI v14) tt.relativeLoss(x, y, tm.get_PSNR / F.mse_loss) (env.py:131-132,174;
 * DBS_1024_24.py:332,342,352) in one fixed-order f64 reduction: x, y `n` contiguous values
 * of kind HBX_SRC_F32 or HBX_SRC_F64 (both the same kind);
 *   out[5] = {sum x y, sum x^2, sum y^2, PSNR, MSE}  with the plans' rel_scale rule
 *   (HBX_REL_LSQ: s = sum xy / sum x^2, MSE = mean((s x - y)^2); HBX_REL_NONE: s = 1) and
 *   PSNR = 10 log10(peak^2 / MSE) (+inf at MSE <= 0).
 * `workspace` holds HBX_REL_WORKSPACE_DOUBLES doubles (device); `out` any address the kernel
 * may write (host-mapped memory reads back without a copy). */
#define HBX_REL_WORKSPACE_DOUBLES 3072
int hbx_rel_stats(const void* x, const void* y, int32_t src_kind, int64_t n, int32_t rel_scale, double peak,
                  double* workspace, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HBX_H */
