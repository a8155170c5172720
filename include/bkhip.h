/* bkhip.h -- C ABI of libbkhip.so: the MI355X (gfx950) many-chain HMC / MALA / DRGHMC
 * hot path that stands in for the per-draw arithmetic of flatironinstitute/bayes-kit.
 *
 * Conventions (all entry points)
 *   - extern "C", plain pointers and sizes; no torch / C++ types cross this boundary.
 *   - Every pointer is a DEVICE pointer owned by the caller (the library never allocates
 *     persistent memory and never frees caller memory).
 *   - Phase-space arrays are fp64, chain-major-contiguous ("[D][ld]"): element (d, c) of
 *     a D-dimensional state of chain c lives at  p[d*ld + c],  ld >= C.  One chain per
 *     GPU lane, so a wavefront touches 64 consecutive doubles for every d.
 *   - `stream` is a hipStream_t passed as void*; calls only enqueue work and return.
 *   - Return value: 0 = ok; < 0 = argument error (BK_E_*); > 0 = hipError_t of the launch.
 *   - No global mutable state: re-entrant across host threads and one-process-per-GPU.
 *   - Arithmetic is IEEE fp64 with every * and + individually rounded (the library is
 *     built with -ffp-contract=off) in the operation order of the cited reference lines,
 *     so elementwise results are bit-identical to the reference's NumPy expressions.
 *   - Two FORMS of every streaming kernel, one entry point: an even number of chains, an even ld and 16-byte aligned
 *     pointers get the 16-bytes-per-lane form (two chains per lane: `k_*_v2` in the sources -- what the many-chain
 *     samplers always pass); an odd chain count, an odd pitch or an unaligned view gets the 8-byte form (`k_*`), same
 *     arithmetic, same results.  The split is by SHAPE, decided inside the entry point (bk_leapfrog_kick_drift,
 *     bk_leapfrog_finish, bk_select_columns, bk_blend_columns, bk_welford_update, the Gaussian targets); the `_n`
 *     variants are the 8-byte form sized by a device-side lane count.  Neither is a superseded generation of the other.
 *
 * Each entry point cites the reference code (flatironinstitute/bayes-kit) it replaces.
 */
#ifndef BKHIP_H
#define BKHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BK_OK 0
#define BK_E_ARG (-1)      /* null pointer / bad extent / bad enum */
#define BK_E_ALIGN (-2)    /* ld < C or similar layout violation */

/* ---- per-chain random streams ------------------------------------------------------
 * state: u64 table [BK_RNG_WORDS][ldr], one chain per column.
 *   BK_RNG_PHILOX (np.random.Philox(key=[k0,k1])): rows 0-1 key, 2-5 counter,
 *       6-9 output buffer, 10 buffer_pos (4 = empty) -- the fields of numpy's
 *       bit_generator.state, so a reference stream can be resumed mid-way.
 *   BK_RNG_PCG64 (np.random.default_rng(int)): rows 0-1 state (hi, lo), 2-3 inc (hi, lo).
 */
#define BK_RNG_WORDS 11
#define BK_RNG_PHILOX 0
#define BK_RNG_PCG64 1

int bk_version(void);

/* Philox key = (key0, chain_id0 + c), counter 0, buffer empty: the stream of
 * np.random.Generator(np.random.Philox(key=[key0, chain_id0 + c])).  Replaces
 * `self._rng = np.random.default_rng(seed)` (hmc.py:23, mala.py:25, drghmc.py:71) for
 * chain c when the reference is seeded with that Philox bit generator. */
int bk_rng_init_philox(uint64_t* state, int64_t ldr, uint64_t key0, uint64_t chain_id0,
                       int64_t C, void* stream);

/* out[d*ld + c] = loc + scale * z,  z ~ N(0,1) drawn d = 0..D-1 in order from chain c's
 * stream (NumPy ziggurat; `rng.normal(loc, scale, size=D)`), where
 *     loc = loc_in ? loc_in[d*ld + c] * loc_mul : 0.0
 * and, if kin_out != NULL,  kin_out[c] = 0.5 * sum_d out*(metric[d]*out)  (metric NULL = 1).
 *   HMC momentum draw + kinetic term     hmc.py:56, :37      (loc_in NULL, scale 1)
 *   initial theta / rho                  hmc.py:24-28, drghmc.py:72-77
 *   DRGHMC partial refresh               drghmc.py:360-364, :250  (loc_mul = sqrt(1-damping),
 *                                                                  scale = sqrt(damping))
 * `active` (NULL = all): u8 mask per chain; inactive chains draw nothing.
 * `work` (may be NULL): caller-owned scratch of bk_refresh_work_elems(C, D) doubles.  With it
 * (Philox streams, no mask, D >= 32) the normals are produced by one WAVEFRONT per chain -- 256
 * stream words evaluated at once, the sequential consumption order resolved exactly -- instead
 * of one lane per chain: same stream, same values and final state, C wavefronts of parallelism
 * instead of C/64 (measured: 4.9x faster at 4096 chains x 128 dims, 17x at 1024 x 1024,
 * 1.3x at 65,536 x 1024 including the transpose into [D][C]). */
int64_t bk_refresh_work_elems(int64_t C, int64_t D);
int bk_momentum_refresh(int rng_kind, uint64_t* state, int64_t ldr,
                        const double* loc_in, double loc_mul, double scale,
                        double* out, int64_t ld, const double* metric, double* kin_out,
                        const uint8_t* active, int64_t C, int64_t D, double* work,
                        int64_t work_elems, void* stream);

/* The momentum draw of HMC with a proper diagonal preconditioner (HMCDiag(precond_diag=v)).  `precond` is the packed
 * array precond[3][D] = {v, sqrt(v), 1/v} (velocity variances, formed once per change of v); for every chain, from its
 * stream and in the stream order of bk_momentum_refresh,
 *     out[d][c]  = 0.0 + precond[D + d] * z_d                      rho0 = chol(diag v) z
 *     kin_out[c] = 0.5 * sum_d out*(precond[2*D + d]*out)          1/2 rho . (M^-1 rho), the quarter order of
 *                                                                  bk_leapfrog_finish; required
 * in the same launches as bk_momentum_refresh (lane per chain, or wavefront per chain with `work`): no extra pass. */
int bk_momentum_refresh_precond(int rng_kind, uint64_t* state, int64_t ldr, double* out, int64_t ld,
                                const double* precond, double* kin_out, int64_t C, int64_t D, double* work,
                                int64_t work_elems, void* stream);

/* DRGHMC: the partial momentum refresh with its kinetic energy (bk_momentum_refresh, no mask) followed by the
 * start of the draw (bk_dr_begin_retry with kin = kin_out) -- drghmc.py:360-371.  With `work` (Philox, D >= 32) the
 * transpose of the normals into the state layout, the kinetic energy and the start of the draw are ONE launch after
 * the generator's; otherwise the two calls in sequence.  Same values, same stream positions either way.
 * side (may be NULL): the PREVIOUS draw's diagnostics -- one bk_welford_update_dev call (mean NULL: none) and / or one
 * bk_record_series_dev call (series NULL: none) on the chains' current point as this draw finds it -- done by workgroups of
 * the generator's launch: the generator is bound by instruction issue, the Welford update by memory, and side by side they
 * take the longer of the two times instead of the sum (a draw sequence inside one hipGraph: DrGhmcDiag.advance(n)).  Where
 * the generator's launch cannot carry them (no `work`, odd C, ...) they are launches of their own, first. */
typedef struct bk_diag_job {
  const double* theta; /* [D][ld_theta]: the point both parts read */
  int64_t ld_theta;
  int64_t C, D;
  const int64_t* n_dev; /* the sampler's device-side draw count */
  double* mean;         /* bk_welford_update_dev(mean, m2, ld, theta, ld_theta, n_dev, n_offset, C, D) */
  double* m2;
  int64_t ld;
  int64_t n_offset;
  double* series; /* bk_record_series_dev(theta, ld_theta, dims, K, logp, series, capacity, n_dev, row_offset, C) */
  const int32_t* dims;
  int64_t K;
  const double* logp;
  int64_t capacity;
  int64_t row_offset;
} bk_diag_job;
int bk_dr_refresh_begin(int rng_kind, uint64_t* state, int64_t ldr, const double* loc_in, double loc_mul,
                        double scale, double* out, int64_t ld, const double* metric, double* kin_out, int64_t C,
                        int64_t D, double* work, int64_t work_elems, const double* logp, double* cur_H,
                        double* cur_h, double* rej, uint8_t* alive, double prob_retry, uint32_t* counters,
                        int64_t n_counters, int64_t* draw_counter, const bk_diag_job* side, void* stream);

/* out[c] = log(u), u = next double of chain c's stream: `np.log(self._rng.uniform())`
 * (hmc.py:60, metropolis.py:74, drghmc.py:370,378).  Inactive chains draw nothing and
 * keep out[c]. */
int bk_log_uniform(int rng_kind, uint64_t* state, int64_t ldr, double* out,
                   const uint8_t* active, int64_t C, void* stream);

/* out[c] = u itself (`rng.uniform()`): the resampling uniforms of smc.py:73. */
int bk_uniform(int rng_kind, uint64_t* state, int64_t ldr, double* out, const uint8_t* active,
               int64_t C, void* stream);

/* ---- leapfrog integrator -------------------------------------------------------------
 * One fused kick + drift over all chains and dimensions (the hot loop hmc.py:47-49,
 * drghmc.py:277-278,282-283):
 *     t      = metric[d] * grad            (metric NULL = ones, still multiplied by 1.0)
 *     r      = rho_in
 *     if use_pre:  r = r + pre  * t        (hmc.py:46 back half-step, pre = -(0.5*eps);
 *                                           drghmc.py:277 first half-kick, pre = 0.5*h)
 *     if use_kick: r = r + kick * t        (hmc.py:48 / drghmc.py:282, kick = eps)
 *     rho_out   = r
 *     theta_out = theta_in + eps * r       (hmc.py:49 / drghmc.py:278,283)
 * theta_out may alias theta_in and rho_out may alias rho_in (in-place), or differ (the
 * first step of a trajectory reads the current point and writes the proposal buffers).
 * grad may have any strides (ldg_d, ldg_c): element (d,c) at grad[d*ldg_d + c*ldg_c]; the
 * chain-contiguous case (ldg_c == 1) streams directly, the dimension-contiguous case
 * (ldg_d == 1, what a row-major (C, D) model output looks like) is transposed through
 * LDS tiles.  Algorithmic HBM bytes: 40 per element. */
int bk_leapfrog_kick_drift(const double* theta_in, double* theta_out,
                           const double* rho_in, double* rho_out, int64_t ld,
                           const double* grad, int64_t ldg_d, int64_t ldg_c,
                           const double* metric, double eps,
                           int use_pre, double pre, int use_kick, double kick,
                           int64_t C, int64_t D, void* stream);

/* Same step, but chain j of the outputs (compact, leading dimension ld_out) is chain
 * src_index[j] of the inputs (leading dimension ld_in): gathers the active chains of a
 * delayed-rejection stage into a dense buffer while taking their first leapfrog step
 * (drghmc.py:276-278 for the chains that reach proposal k). n = number of gathered chains. */
int bk_leapfrog_first_step_gather(const double* theta_in, const double* rho_in, const double* grad_in,
                                  int64_t ld_in, const int32_t* src_index, double* theta_out,
                                  double* rho_out, int64_t ld_out, const double* metric, double eps,
                                  double pre, int64_t n, int64_t D, const uint32_t* n_dev, void* stream);
/* (n_dev may be NULL: all n lanes; otherwise min(n, *n_dev), see "Lane counts on the device" below.) */

/* Final half-kick and kinetic energy of a trajectory:
 *     r = rho_in + half * (metric[d] * grad)      hmc.py:52, drghmc.py:286
 *     if negate: r = -r                           drghmc.py:345 (momentum flip)
 *     if rho_out: rho_out = r
 *     kin_out[c] = 0.5 * sum_d r*(metric[d]*r)    hmc.py:37, drghmc.py:250
 * grad NULL: no kick (r = rho_in), i.e. just the kinetic energy of a finished trajectory.
 * Per-chain sums (here, in bk_momentum_refresh, bk_mala_logq and the Gaussian targets' logp)
 * run over four contiguous quarters of the dimensions, each sequentially in d, combined as
 * ((p0+p1)+p2)+p3: a fixed order that depends on D only (np.dot uses yet another order:
 * results agree to ~1e-16 relative, see DESIGN.md tolerances). */
int bk_leapfrog_finish(const double* rho_in, double* rho_out, int64_t ld,
                       const double* grad, int64_t ldg_d, int64_t ldg_c,
                       const double* metric, double half, int negate,
                       double* kin_out, int64_t C, int64_t D, void* stream);

/* The packed form of a diagonal preconditioner from its D velocity variances v (finite, positive: the caller checks):
 *     precond[d] = v[d]     precond[D + d] = sqrt(v[d])     precond[2*D + d] = 1.0 / v[d]
 * square root and division correctly rounded (IEEE 754), so a host restatement has the same doubles.  v may be the first
 * row of precond. */
int bk_precond_pack(const double* v, double* precond, int64_t D, void* stream);

/* The same for a proper diagonal preconditioner, precond[3][D] = {v, sqrt(v), 1/v}: the kick vector and the
 * kinetic-energy vector differ,
 *     r = rho_in + half * (precond[d] * grad)
 *     kin_out[c] = 0.5 * sum_d r*(precond[2*D + d]*r)
 * everything else (negate, rho_out, grad NULL, the order of the sums) as above. */
int bk_leapfrog_finish_precond(const double* rho_in, double* rho_out, int64_t ld, const double* grad, int64_t ldg_d,
                               int64_t ldg_c, const double* precond, double half, int negate, double* kin_out,
                               int64_t C, int64_t D, void* stream);

/* ---- the same three steps over a lane set whose SIZE LIVES ON THE DEVICE -----------------------
 * (drghmc.py:276-278, :280-283, :285-286 for the chains that reach a delayed-rejection proposal or one
 * of its ghosts.)  n_dev: device pointer to the number of lanes in the set, written by an earlier launch
 * on the same stream (bk_compact_indices, the appending accept tests); the launch is sized for the bound
 * C / n and works on min(bound, *n_dev) lanes -- see "Lane counts on the device" below.  With these and a
 * counted gradient (bk_target_*_grad_n, bk_target_fn_n) a delayed-rejection draw over ANY model that the
 * library can call without the host is a fixed launch sequence: no lane count is read back, the draw
 * replays as one hipGraph.  n_dev NULL = the host-sized entry points above.  Same arithmetic. */
int bk_leapfrog_kick_drift_n(const double* theta_in, double* theta_out, const double* rho_in, double* rho_out,
                             int64_t ld, const double* grad, int64_t ldg_d, int64_t ldg_c,
                             const double* metric, double eps, int use_pre, double pre, int use_kick,
                             double kick, int64_t C, int64_t D, const uint32_t* n_dev, void* stream);
/* bk_leapfrog_finish for such a set, plus what the end of a delayed-rejection trajectory owes its level:
 * H_out / h_out / live_out (all or none; needs logp = the log density at the end point and kin_out):
 * bk_dr_level_begin for the produced lanes (H = -((-logp) + kin), h = 0, live = 1; drghmc.py:421 -> :249-251);
 * lanes_out (may be NULL) receives the number of lanes worked on, lanes_total (may be NULL) is incremented
 * by it (statistics: gradient evaluations = steps * lanes). */
int bk_leapfrog_finish_level(const double* rho_in, double* rho_out, int64_t ld, const double* grad,
                             int64_t ldg_d, int64_t ldg_c, const double* metric, double half, int negate,
                             double* kin_out, int64_t C, int64_t D, const uint32_t* n_dev,
                             const double* logp, double* H_out, double* h_out, uint8_t* live_out,
                             uint32_t* lanes_out, uint64_t* lanes_total, void* stream);

/* ---- Metropolis / Metropolis-Hastings accept ------------------------------------------
 * mode BK_ACCEPT_HMC  (hmc.py:57-63):  h0 = lp_cur - a_cur ; h1 = lp_prop - a_prop ;
 *        accept = log_u < h1 - h0 ;  ret[c] = accept ? h1 : h0   (joint log density)
 * mode BK_ACCEPT_MALA (mala.py:50-61, metropolis.py:70-76): a_cur = lp_forward,
 *        a_prop = lp_reverse ; accept = log_u < (lp_prop - lp_cur) + (a_prop - a_cur) ;
 *        ret[c] = accept ? lp_prop : lp_cur   (model log density, mala.py:66)
 * On accept lp_cur[c] <- lp_prop[c].  accept_mask[c] = 0/1.  *accept_count (device u32,
 * may be NULL) is incremented by the number of accepted chains, one atomic per wavefront
 * (ballot + popcount).  Strict `<` as in the reference. */
#define BK_ACCEPT_HMC 0
#define BK_ACCEPT_MALA 1
int bk_mh_accept(int mode, double* lp_cur, const double* a_cur, const double* lp_prop,
                 const double* a_prop, const double* log_u, uint8_t* accept_mask,
                 double* ret, uint32_t* accept_count, int64_t C, void* stream);

/* dst[d*ld + c] = mask[c] ? src[d*ld + c] : dst[d*ld + c] for up to two array pairs
 * (pair 1 may be NULL): `self._theta = theta_prop` (hmc.py:61, mala.py:62-64,
 * drghmc.py:379) applied to the accepted chains only.  Rejected chains keep their values; on
 * the 16-byte path (even C and ld, aligned pointers) they are re-written with them, so that no
 * partially written HBM sector results (a blend streams at full rate, holes do not).
 * `copy0` (may be NULL) additionally receives array 0 as it stands after the select, for every
 * chain (the stable array that sample() returns while the sampler keeps mutating its own; same
 * leading dimension). */
int bk_select_columns(const uint8_t* mask, double* dst0, const double* src0,
                      double* dst1, const double* src1, double* copy0, int64_t ld,
                      int64_t C, int64_t D, void* stream);

/* out[d*ld + c] = mask[c] ? b[d*ld + c] : a[d*ld + c]; a and b are only read.  The select for a sampler
 * that rebinds its state array every draw, as the reference does (`self._theta = theta_prop`,
 * hmc.py:61): `out` is the new state AND the array sample() returns, never written again.  About
 * 17 bytes of HBM traffic per element against 25 for bk_select_columns with copy0. */
int bk_blend_columns(const uint8_t* mask, const double* a, const double* b, double* out,
                     int64_t ld, int64_t C, int64_t D, void* stream);

/* ---- affine-invariant ensemble sampler: the stretch move (Goodman & Weare 2010; ensemble.py:47-65) -----
 * theta [D][ld] holds walkers in columns.  The n ACTIVE walkers are columns [col_act, col_act + n); they belong to
 * n / H ensembles of H consecutive columns each, and the other half of the e-th of them is columns
 * [col_oth + e*H, col_oth + (e + 1)*H).  For active walker k (ensemble e = k / H), from its uniforms u_j[k], u_z[k]:
 *     j            = col_oth + e*H + min(floor(u_j[k] * H), H - 1)       np.random.choice(other half), ensemble.py:60
 *     r            = inv_sqrt_a + (sqrt_a - inv_sqrt_a) * u_z[k] ;  z = r * r                         ensemble.py:49
 *     theta_prop[d*ldp + k] = theta[d*ld + j] + z * (theta[d*ld + col_act + k] - theta[d*ld + j])     ensemble.py:53
 *     zterm[k]     = (D - 1) * log(z)             ensemble.py:54 (the device log of bk_log_uniform)
 *     partner[k]   = j
 * Every operation is rounded on its own.  floor(u_j * H) is clamped to [0, H - 1], so any value of u_j gives a column
 * of the other half.  theta is only read; theta_prop must not overlap it.  Follow with the model's log density at
 * theta_prop and bk_mh_accept(BK_ACCEPT_MALA, lp, NULL, lp_prop, zterm, log_u, ...), bk_select_columns.
 * The two forms by shape: n, ld, ldp even with theta + col_act and theta_prop 16-byte aligned -> two walkers per lane;
 * anything else one walker per lane; same results.  HBM traffic 24*D bytes per active walker when the gather of theta_j
 * is served from cache (for one d all of them fall into n*8 contiguous bytes).
 * BK_E_ARG: a null pointer, n < 0, D < 0, a negative column, H < 1, n % H != 0, ld < max(col_act, col_oth) + n, ldp < n,
 * D > 262,140; decided before any HIP call.  n == 0 or D == 0: BK_OK, nothing launched. */
int bk_stretch_propose(const double* theta, int64_t ld, int64_t col_act, int64_t col_oth, int64_t n, int64_t H,
                       const double* u_j, const double* u_z, double inv_sqrt_a, double sqrt_a, double* theta_prop,
                       int64_t ldp, double* zterm, int32_t* partner, int64_t D, void* stream);

/* ---- differential-evolution move of the ensemble sampler (ter Braak 2006, DE-MC; emcee's DEMove) -----
 * The layout and the arguments theta, ld, col_act, col_oth, n, H, theta_prop, ldp, D are those of bk_stretch_propose.
 * Active walker k (ensemble e = k / H) draws an ordered pair of DIFFERENT walkers of the other half of its ensemble from
 * the uniforms u_1[k], u_2[k], and a step from the standard normal z[k]:
 *     i1 = clamp((int64)(u_1[k] * H), 0, H - 1)
 *     i2 = clamp((int64)(u_2[k] * (H - 1)), 0, H - 2);  i2 += (i2 >= i1)     uniform over the H (H - 1) ordered pairs
 *     j1 = col_oth + e*H + i1 ;  j2 = col_oth + e*H + i2
 *     g  = gamma0 * (1.0 + sigma * z[k])
 *     theta_prop[d*ldp + k] = theta[d*ld + col_act + k] + g * (theta[d*ld + j1] - theta[d*ld + j2])
 *     partner1[k] = j1 ;  partner2[k] = j2 ;  gamma[k] = g
 * Every operation is rounded on its own.  Both indices are clamped, so ANY values of u_1 and u_2 (NaN, negative, >= 1) give
 * two different columns of the other half.  The proposal is symmetric: follow with the model's log density at theta_prop
 * and bk_mh_accept(BK_ACCEPT_MALA, lp, NULL, lp_prop, zeros, log_u, ...) or bk_tempered_accept with a zterm of zeros.
 * theta is only read; theta_prop must not overlap it.  The two launch forms are chosen as in bk_stretch_propose, with the
 * same results.  HBM traffic 32*D bytes per active walker when both gathers are served from cache (24*D for the stretch
 * move): for one d all gathers fall into n*8 contiguous bytes.  Plain loads and stores only.
 * BK_E_ARG: a null pointer, n < 0, D < 0, a negative column, H < 2, n % H != 0, ld < max(col_act, col_oth) + n, ldp < n,
 * more than INT32_MAX columns, D > 262,140; decided before any HIP call.  n == 0 or D == 0: BK_OK, nothing launched. */
int bk_de_propose(const double* theta, int64_t ld, int64_t col_act, int64_t col_oth, int64_t n, int64_t H,
                  const double* u_1, const double* u_2, const double* z, double gamma0, double sigma, double* theta_prop,
                  int64_t ldp, int32_t* partner1, int32_t* partner2, double* gamma, int64_t D, void* stream);

/* ---- parallel tempering (replica exchange): a tempered accept test and the swap of two rungs' columns -----
 * A column (walker, chain) c targets lp0(theta) + beta[c] * ll(theta); ll and lp0 are cached per column, lp0 may be
 * absent (NULL: the whole log density is tempered).  beta is a per-column [n] / [C] array.
 *
 * bk_tempered_accept, for the n columns the pointers point at (an active slice):
 *     accept = log_u[k] < ((lp0_prop[k] - lp0[k]) + beta[k] * (ll_prop[k] - ll[k])) + zterm[k]
 * in exactly that order, every operation rounded on its own; lp0 == NULL: the first term is the literal 0.0 (with
 * beta = 1 the test is then the one of bk_mh_accept(BK_ACCEPT_MALA, ll, NULL, ll_prop, zterm, ...)).  Strict `<`; a NaN
 * on either side refuses.  On accept ll[k] <- ll_prop[k] (and lp0[k] <- lp0_prop[k]); accept_mask[k] = 0/1.
 * accept_counts (device u32 [n / H], may be NULL): entry k / H is incremented by the accepted columns of the k / H-th
 * block of H columns (an ensemble's active half).  Integer atomics only, so the counts are exact: one per wavefront
 * where all columns of the wavefront lie in one block (ballot + popcount), one per accepting lane otherwise.
 * BK_E_ARG: ll, ll_prop, beta, zterm, log_u or accept_mask null, lp0 without lp0_prop, n < 0, H < 1, n % H != 0;
 * decided before any HIP call.  n == 0: BK_OK, nothing launched.
 *
 * bk_replica_swap, on plain [D][ld] arrays and [C] vectors: every column c with lower[c] != 0 and c + H < C proposes to
 * change places with its partner, column c + H (the caller's pairs are disjoint: no partner is itself a lower column):
 *     swap = log_u[c] < (beta[c] - beta[c + H]) * (ll[c + H] - ll[c])
 * IEEE decides the edge cases (0 * inf and -inf - -inf are NaN, and NaN refuses).  If it holds, columns c and c + H of
 * theta (all D rows, in place), of theta2 (a second array of the same pitch, may be NULL: a cached gradient, the copy
 * of the state a sampler hands out), of ll and of lp0 (may be NULL) are exchanged.  swapped[c] = 1 for a lower column
 * that swapped, 0 for every other c < C.  proposed / accepted (device u32 [C / H], each may be NULL): entry c / H is
 * incremented by the lower columns of that block that proposed / swapped (integer atomics, as above).
 * The decision reads ll, which the swap overwrites: it is taken once per pair by a [C]-sized pass that writes
 * `swapped` and exchanges the scalars; the exchange of the columns is a second launch, tiled over blocks of 4 rows, that
 * reads only `swapped`: one lane per pair, both columns coalesced, loads before stores; two pairs per lane on 16-byte
 * words where H and ld are even and the array 16-byte aligned; same results.  A refused pair moves no bytes; HBM traffic
 * 32*D bytes per swapped pair and array.
 * BK_E_ARG: theta, ll, beta, log_u, lower or swapped null, C < 0, D < 0, H < 1, C % H != 0, ld < C, D > 262,140;
 * decided before any HIP call.  C == 0: BK_OK, nothing launched. */
int bk_tempered_accept(double* ll, double* lp0, const double* ll_prop, const double* lp0_prop, const double* beta,
                       const double* zterm, const double* log_u, uint8_t* accept_mask, uint32_t* accept_counts,
                       int64_t n, int64_t H, void* stream);
int bk_replica_swap(double* theta, double* theta2, int64_t ld, double* ll, double* lp0, const double* beta,
                    const double* log_u, const uint8_t* lower, uint8_t* swapped, uint32_t* proposed, uint32_t* accepted,
                    int64_t C, int64_t H, int64_t D, void* stream);

/* ---- the leapfrog integrator of a ladder (tempered HMC): per-column inverse temperature and step size -------
 * Column c targets lp0(theta) + beta[c] * ll(theta) and integrates with its own step size: beta, eps, pre, kick and half
 * are per-column [C] device vectors where bk_leapfrog_kick_drift / bk_leapfrog_finish take scalars.  Phase-space arrays
 * are [D][ld]; the gradients grad_ll and grad_lp0 are chain-contiguous [D][ldg] arrays with a pitch of their own (a
 * (C, D) row-major model output goes through bk_relayout first).  grad_lp0 may be NULL: the whole log density is
 * tempered.  metric may be NULL: ones, not multiplied in.  Every `*` and `+` below is rounded on its own.  The force on
 * element (d, c) is
 *     f = beta[c] * grad_ll[d*ldg + c] ;   if grad_lp0: f = grad_lp0[d*ldg + c] + f
 *     t = metric ? metric[d] * f : f
 *
 * bk_tempered_kick_drift:
 *     r = rho_in[d*ld + c] ;   if pre: r = r + pre[c] * t ;   if kick: r = r + kick[c] * t
 *     rho_out[d*ld + c] = r ;  theta_out[d*ld + c] = theta_in[d*ld + c] + eps[c] * r
 * pre and kick may be NULL (no such term).  In-place use (theta_out == theta_in, rho_out == rho_in) is allowed: every
 * element is loaded before it is stored, by one lane.  With beta all 1.0, grad_lp0 NULL and uniform vectors the result
 * is bk_leapfrog_kick_drift's bit for bit (1.0 * g is g).  HBM traffic 40 bytes per element, 48 with grad_lp0; the
 * per-column vectors are 8*C bytes each, read once per workgroup and 4 rows and served from cache.
 *
 * bk_tempered_finish:
 *     r = grad_ll ? rho_in[d*ld + c] + half[c] * t : rho_in[d*ld + c] ;   if rho_out: rho_out[d*ld + c] = r
 *     kin_out[c] = 0.5 * sum_d r * (metric ? metric[d] * r : r)
 * summed in bk_leapfrog_finish's order: four contiguous quarters of d (ceil(D / 4) rows each), sequentially inside each,
 * combined as ((p0 + p1) + p2) + p3.  rho_out and kin_out may be NULL; beta and half are not read without grad_ll.  In the
 * degenerate case above the result is bk_leapfrog_finish(negate = 0)'s bit for bit.  HBM traffic 16 bytes per element, 24
 * with grad_lp0, 8 more with rho_out.
 *
 * Both choose between two forms by shape: C, ld, ldg even and every array and vector 16-byte aligned -> two columns
 * (16 bytes) per lane, each with its own entry of the vectors; anything else one column per lane; same results.
 *
 * bk_tempered_hmc_accept, for n columns:
 *     h0 = (lp0 ? lp0[k] + beta[k] * ll[k] : beta[k] * ll[k]) - kin0[k]
 *     h1 = (lp0 ? lp0_prop[k] + beta[k] * ll_prop[k] : beta[k] * ll_prop[k]) - kin1[k]
 *     accept = log_u[k] < h1 - h0
 * Strict `<`; a NaN on either side refuses (0 * inf is NaN).  At beta = 1 without lp0 this is the comparison of
 * bk_mh_accept(BK_ACCEPT_HMC) exactly.  On accept ll[k] <- ll_prop[k] (and lp0[k] <- lp0_prop[k]); accept_mask[k] = 0/1;
 * accept_counts (device u32 [n / H], may be NULL) as in bk_tempered_accept: exact integer atomics per block of H columns.
 *
 * bk_exchange_columns: columns c and c + H of x change places where swapped[c] != 0, for c < C - H: the exchange pass
 * of bk_replica_swap on one further array, after the decision (which overwrote ll and cannot be repeated) was taken.
 * Same two forms and traffic (32*D bytes per swapped pair) as there.
 *
 * Errors, decided before any HIP call.  BK_E_ARG: a null required pointer (kick_drift: theta_in, theta_out, rho_in,
 * rho_out, grad_ll, beta, eps; finish: rho_in, and beta and half with grad_ll; accept: ll, kin0, ll_prop, kin1, beta,
 * log_u, accept_mask, lp0 without lp0_prop; exchange: x, swapped), a negative extent, H < 1, n % H != 0 or C % H != 0,
 * D > 262,140 (kick_drift, exchange).  BK_E_ALIGN: ld < C or ldg < C.  C == 0, D == 0 or n == 0: BK_OK, nothing launched. */
int bk_tempered_kick_drift(const double* theta_in, double* theta_out, const double* rho_in, double* rho_out, int64_t ld,
                           const double* grad_ll, const double* grad_lp0, int64_t ldg, const double* metric,
                           const double* beta, const double* eps, const double* pre, const double* kick, int64_t C,
                           int64_t D, void* stream);
int bk_tempered_finish(const double* rho_in, double* rho_out, int64_t ld, const double* grad_ll, const double* grad_lp0,
                       int64_t ldg, const double* metric, const double* beta, const double* half, double* kin_out,
                       int64_t C, int64_t D, void* stream);
int bk_tempered_hmc_accept(double* ll, double* lp0, const double* kin0, const double* ll_prop, const double* lp0_prop,
                           const double* kin1, const double* beta, const double* log_u, uint8_t* accept_mask,
                           uint32_t* accept_counts, int64_t n, int64_t H, void* stream);
int bk_exchange_columns(double* x, int64_t ld, const uint8_t* swapped, int64_t C, int64_t H, int64_t D, void* stream);

/* ---- the same three operations with ONE ROW PITCH PER ARRAY (the tile-major HMC schedule) ---------------
 * A tile of T chains keeps its proposal, momentum and trajectory gradient in contiguous [D][T] arrays that stay
 * in the Infinity Cache, while the state, the generator's momentum and the cached gradient are columns of [D][C]
 * arrays.  The launches at a tile's two ends therefore read one kind and write the other:
 *   bk_leapfrog_kick_drift_ld   the arithmetic of bk_leapfrog_kick_drift, element (d, c) of each array at its own
 *                               pitch (ld_theta_in, ld_theta_out, ld_rho_in, ld_rho_out); rho_out may be rho_in (then
 *                               the two pitches are equal), theta_out may be theta_in likewise.  Any strides of grad.
 *   bk_blend_columns_ld         out[d*ld_out + c] = mask[c] ? b[d*ld_b + c] : a[d*ld_a + c]
 *   bk_select_columns_ld        dst[d*ld_dst + c] = mask[c] ? src[d*ld_src + c] : dst[d*ld_dst + c]  (one pair)
 * The same two forms by shape: an even C, even pitches and 16-byte aligned pointers take the 16-byte form (blend and
 * select rewrite every 16-byte pair: no holes in sectors), anything else the 8-byte form; same results.  Access hints
 * are chosen per SIDE: a launch whose distinct arrays exceed the cache reads its full-width inputs non-temporally and
 * writes plainly what fits the cache afterwards (the tile), non-temporally what does not; the tile-resident operand of
 * blend / select (b, src: the narrower pitch) is read plainly (profiles/cache_tiles.md, section 6). */
int bk_leapfrog_kick_drift_ld(const double* theta_in, int64_t ld_theta_in, double* theta_out, int64_t ld_theta_out,
                              const double* rho_in, int64_t ld_rho_in, double* rho_out, int64_t ld_rho_out,
                              const double* grad, int64_t ldg_d, int64_t ldg_c, const double* metric, double eps,
                              int use_pre, double pre, int use_kick, double kick, int64_t C, int64_t D, void* stream);
int bk_blend_columns_ld(const uint8_t* mask, const double* a, int64_t ld_a, const double* b, int64_t ld_b, double* out,
                        int64_t ld_out, int64_t C, int64_t D, void* stream);
int bk_select_columns_ld(const uint8_t* mask, double* dst, int64_t ld_dst, const double* src, int64_t ld_src,
                         int64_t C, int64_t D, void* stream);

/* ---- delayed rejection (DRGHMC) stage helpers -------------------------------------------
 * The reference's recursive accept() with its gradient-cache stack (drghmc.py:82,391-446)
 * is run as a lockstep state machine over lane sets: the chains still inside the stage
 * loop are compacted into dense buffers per recursion level, so a trajectory only costs
 * bandwidth for the chains that actually take it.  Per-chain scalars of a level: H (joint
 * log density), h (log of the probability of rejecting all earlier proposals, the
 * "hastings" term), a (log acceptance probability), live (not yet early-exited).
 *
 * Lane counts on the device.  Every entry point that works on a lane set takes, besides the
 * host-side extent `n` (or `m`), an optional `n_dev`: a device pointer to the number of lanes
 * actually in the set, as written by bk_compact_indices earlier on the same stream.  With
 * n_dev != NULL the launch is sized for `n` (an upper bound, e.g. the parent set) and works on
 * min(n, *n_dev) lanes; surplus workgroups exit at once.  The host then never reads a count
 * back, and a whole delayed-rejection draw -- whose lane sets depend on the draw's own accept
 * decisions -- is a fixed launch sequence that can be captured as one hipGraph.
 */

/* Stable compaction: idx_out[k] = position of the k-th nonzero entry of mask[0..n),
 * *count_out = number of nonzero entries (ballot/popcount prefix sums per wavefront). */
int bk_compact_indices(const uint8_t* mask, int64_t n, int32_t* idx_out, uint32_t* count_out,
                       const uint32_t* n_dev, void* stream);

/* Start of a draw (drghmc.py:365-366): cur_H = -((-logp) + kin) (joint_logp, :249-251),
 * cur_h = 0, rej = 0, alive = 1. */
int bk_dr_begin(const double* logp, const double* kin, double* cur_H, double* cur_h, double* rej,
                uint8_t* alive, int64_t C, void* stream);

/* Retry test (drghmc.py:369-371) for the alive chains: u from the chain's stream, chain
 * leaves the stage loop unless log(u) < prob_retry * rej  (prob_retry is 1.0 or 0.0; the
 * product reproduces False * -inf = nan -> break). */
int bk_dr_retry_test(int rng_kind, uint64_t* state, int64_t ldr, const double* rej,
                     double prob_retry, uint8_t* alive, int64_t C, void* stream);

/* Level set-up for accept(): H = -((-logp) + kin) (drghmc.py:421 -> :249-251), h = 0,
 * live = 1 for the n lanes of a level. */
int bk_dr_level_begin(const double* logp, const double* kin, double* H, double* h, uint8_t* live,
                      int64_t n, const uint32_t* n_dev, void* stream);

/* After the recursive accept of ghost proposals (drghmc.py:426-436): ghost lane j belongs
 * to parent lane p = sub_index ? sub_index[j] : j.  If ga[j] == 0 the parent's result is
 * a = -inf and it stops (early-out, :430-432); otherwise h[p] += log1p(-exp(ga[j])). */
int bk_dr_ghost_update(const double* ga, const int32_t* sub_index, int64_t m, double* h,
                       uint8_t* live, double* a, const uint32_t* n_dev, void* stream);

/* Final acceptance probability of the still-live lanes (drghmc.py:438-446):
 * a = min(0, (H - cur_H) + (h - cur_h) + (pr*h - pr*cur_h)), with cur_* read at
 * cur_index ? cur_index[j] : j. */
int bk_dr_accept_prob(const double* H, const double* cur_H, const double* h, const double* cur_h,
                      const int32_t* cur_index, double prob_retry, const uint8_t* live, double* a,
                      int64_t n, const uint32_t* n_dev, void* stream);

/* Top-level accept test of a stage (drghmc.py:378-385) for the n compacted lanes; lane j is
 * chain g = chain_index ? chain_index[j] : j.  u from chain g's stream; if log(u) < a[j]:
 * accepted[j] = 1, cur_H[g] = H[j], alive[g] = 0; else accepted[j] = 0,
 * rej[g] = log1p(-exp(a[j])), cur_h[g] += rej[g]. */
int bk_dr_accept_test(int rng_kind, uint64_t* state, int64_t ldr, const int32_t* chain_index,
                      const double* a, const double* H, int64_t n, double* cur_H, double* cur_h,
                      double* rej, uint8_t* alive, uint8_t* accepted, const uint32_t* n_dev,
                      void* stream);

/* bk_dr_accept_prob for the chains' CURRENT point followed by bk_dr_accept_test, in one launch: lane j's
 * accept probability a[j] (written, if live[j]) is evaluated against cur_H / cur_h of its chain right before
 * the test draws its uniform.  Same arithmetic, one launch less per stage. */
int bk_dr_accept_prob_test(int rng_kind, uint64_t* state, int64_t ldr, const int32_t* chain_index,
                           const double* H, const double* h, const uint8_t* live, double* a,
                           double prob_retry, int64_t n, double* cur_H, double* cur_h, double* rej,
                           uint8_t* alive, uint8_t* accepted, const uint32_t* n_dev, void* stream);

/* Start of a draw and the first stage's retry test in one launch: bk_dr_begin, then bk_dr_retry_test for every
 * chain (drghmc.py:365-371: reject_logp = 0 at the first stage, the test passes, its uniform is drawn all the
 * same).  Also zeroes `n_counters` (<= 64) lane counters -- the `next_count` words of the two entry points below --
 * so that a whole draw needs no separate memset -- and adds 1 to *draw_counter (may be NULL): the sampler's draw
 * count in device memory, which bk_welford_update_dev / bk_record_series_dev launched later in the same draw read. */
int bk_dr_begin_retry(int rng_kind, uint64_t* state, int64_t ldr, const double* logp, const double* kin,
                      double* cur_H, double* cur_h, double* rej, uint8_t* alive, double prob_retry,
                      uint32_t* counters, int64_t n_counters, int64_t* draw_counter, int64_t C, void* stream);

/* bk_dr_accept_prob_test, then -- for the lanes it rejects -- the NEXT stage's retry test (bk_dr_retry_test: the
 * chain's next uniform, drghmc.py:369-371) and the compaction of the chains that propose again: chain g is
 * appended to next_index[0 .. *next_count) (one atomic per wavefront; *next_count must be zero beforehand).  The
 * list holds the same chains bk_compact_indices would give, in an order that depends on wavefront timing: lane
 * order carries no meaning (every chain's values are independent of the lane that computes them).
 * next_index must not be chain_index.  drghmc.py:378-385 and :369-371. */
int bk_dr_accept_prob_test_next(int rng_kind, uint64_t* state, int64_t ldr, const int32_t* chain_index,
                                const double* H, const double* h, const uint8_t* live, double* a,
                                double prob_retry, int64_t n, double* cur_H, double* cur_h, double* rej,
                                uint8_t* alive, uint8_t* accepted, const uint32_t* n_dev, int32_t* next_index,
                                uint32_t* next_count, void* stream);

/* bk_dr_accept_prob_ghost, then the parent lanes that are still live -- the lane set of the parent's NEXT ghost
 * (drghmc.py:424) -- are appended to next_index[0 .. *next_count) as above (instead of a bk_compact_indices
 * launch over parent_live).  next_index must not be sub_index. */
int bk_dr_accept_prob_ghost_next(const double* H, const double* parent_H, const double* h, double* parent_h,
                                 const int32_t* sub_index, double prob_retry, const uint8_t* live, double* a,
                                 int64_t n, const uint32_t* n_dev, uint8_t* parent_live, double* parent_a,
                                 int32_t* next_index, uint32_t* next_count, void* stream);

/* bk_dr_accept_prob of a GHOST level (against its parent level's H / h, lanes paired by sub_index) followed
 * by bk_dr_ghost_update of the parent (parent_h, parent_live, parent_a), in one launch: every ghost lane has
 * exactly one parent lane.  drghmc.py:426-446. */
int bk_dr_accept_prob_ghost(const double* H, const double* parent_H, const double* h, double* parent_h,
                            const int32_t* sub_index, double prob_retry, const uint8_t* live, double* a,
                            int64_t n, const uint32_t* n_dev, uint8_t* parent_live, double* parent_a,
                            void* stream);

/* Accepted lanes replace their chain's current point (drghmc.py:379): for up to three
 * array pairs dst[d*ld_dst + g] = src[d*ld_src + j] and one per-chain vector
 * sdst[g] = ssrc[j], where g = index ? index[j] : j and mask[j] != 0. */
int bk_scatter_columns(const uint8_t* mask, const int32_t* index, int64_t n, int64_t D,
                       double* dst0, const double* src0, double* dst1, const double* src1,
                       double* dst2, const double* src2, int64_t ld_dst, int64_t ld_src,
                       double* sdst, const double* ssrc, const uint32_t* n_dev, void* stream);

/* ---- MALA ---------------------------------------------------------------------------
 * theta_prop = (theta + eps*grad) + sqrt2eps * z, z from chain c's stream in d order
 * (mala.py:41-45). */
int bk_mala_propose(int rng_kind, uint64_t* state, int64_t ldr, const double* theta,
                    const double* grad, double* theta_prop, int64_t ld, double eps,
                    double sqrt2eps, int64_t C, int64_t D, void* stream);

/* The same proposal with the D normals already drawn (e.g. generated ahead on another stream):
 * theta_prop = (theta + eps*grad) + sqrt2eps * z, with z[d*z_stride_d + c*z_stride_c] either in
 * the state layout (strides ld, 1; from bk_momentum_refresh) or chain-major (strides 1, ldz;
 * from bk_normals_chain_major, turned through LDS tiles here). */
int bk_mala_propose_from_normals(const double* theta, const double* grad, const double* z,
                                 int64_t z_stride_d, int64_t z_stride_c, double* theta_prop,
                                 int64_t ld, double eps, double sqrt2eps, int64_t C, int64_t D,
                                 void* stream);

/* The proposal of MALA with a diagonal preconditioner v (extension; plain MALA, mala.py:41-45, on theta / sqrt(v)):
 *     theta_prop = (theta + eps*(v*grad)) + sqrt2eps * (sqrt(v)*z)
 * precond: the packed [3][D] = {v, sqrt(v), 1/v} that bk_precond_pack writes; z in either layout, as above.  With v = 1
 * every added factor is an exact multiplication by 1.0: the same doubles as bk_mala_propose_from_normals. */
int bk_mala_propose_from_normals_precond(const double* theta, const double* grad, const double* z,
                                         int64_t z_stride_d, int64_t z_stride_c, const double* precond,
                                         double* theta_prop, int64_t ld, double eps, double sqrt2eps,
                                         int64_t C, int64_t D, void* stream);

/* zt[c*ldz + d] = d-th next standard normal of chain c's stream, d = 0..D-1 (what
 * `rng.normal(size=D)` returns, mala.py:44 / hmc.py:56), 16 to 64 lanes of a wavefront per chain,
 * Philox streams only; state advanced exactly as by sequential consumption.  ldz >= D.
 * `snapshot` (may be NULL; a second table with the same ldr) receives the stream table as it was BEFORE
 * the call: a sampler that generates a draw's normals one draw ahead keeps its logical stream
 * position (where the reference's generator stands between two sample() calls) that way, without a
 * separate copy of the table.
 * max_workgroups (0 = no bound): a BACKGROUND launch of at most that many workgroups, each walking several groups of
 * chains -- with one workgroup per CU (256 on MI355X) the generator keeps one wavefront per SIMD and the rest of every CU
 * stays free for a bandwidth-bound kernel running beside it on another stream.  Same stream of normals. */
int bk_normals_chain_major(int rng_kind, uint64_t* state, int64_t ldr, double* zt, int64_t ldz, int64_t C,
                           int64_t D, uint64_t* snapshot, int64_t max_workgroups, void* stream);

/* Lanes of a wavefront per chain (16, 32 or 64) that the word-parallel generator uses for a launch of C chains x D
 * normals -- bk_normals_chain_major and every entry point that takes the same path (bk_momentum_refresh with scratch,
 * bk_momentum_refresh_precond, bk_dr_refresh_begin): a pass evaluates a window of 4 x lanes stream words per chain.
 * A function of (C, D) only; launches nothing.  0 for C < 1 or D < 1. */
int bk_normals_lanes_per_chain(int64_t C, int64_t D);

/* ONE chain driven by a host model (the reference's own call shape, README.md:13-32; mala.py:40-66): everything of a
 * draw that follows the model call, and the next draw's proposal, in ONE launch of one lane.
 *   have_prop != 0: host_in[0] = log density at theta_prop, host_in[1 .. D] = its gradient (written by the caller
 *     into host memory the device can address: pinned + mapped); proposal densities as bk_mala_logq, accept test
 *     as bk_mh_accept(BK_ACCEPT_MALA) with the next uniform of the chain's stream, select into theta / grad / lp
 *     (device, [D], [D], [1]); host_out[0 .. D) = theta after the draw, host_out[D] = the returned log density
 *     (mala.py:66), host_out[D + 1] = 1.0 / 0.0 accepted.
 *   always: snapshot (may be NULL; a table like state) = the stream table at this point -- where the reference's
 *     generator stands between two sample() calls --; then theta_prop = (theta + eps*grad) + sqrt2eps*z from the next
 *     D normals (mala.py:41-45), also to host_out[D + 2 .. 2D + 2); finally host_out[2D + 2] = seq, written last
 *     (system-scope release) so that the host may wait on it instead of synchronising the stream.
 * state: the table of ONE chain (column 0 of a table with row pitch ldr). */
int bk_mala_single_draw(int rng_kind, uint64_t* state, int64_t ldr, double* theta, double* grad, double* lp,
                        double* theta_prop, const double* host_in, double* host_out, uint64_t* snapshot,
                        int64_t lds, uint8_t* accept_mask, uint32_t* accept_count, double eps, double sqrt2eps,
                        int64_t D, int have_prop, double seq, void* stream);

/* lp_forward[c] = (-0.25/eps) * |(theta_prop - theta) - eps*grad|^2       mala.py:50-52
 * lp_reverse[c] = (-0.25/eps) * |(theta - theta_prop) - eps*grad_prop|^2   mala.py:53,68-79
 * Sums over four contiguous quarters of ceil(D/4) rows, each in order of d, combined ((p0+p1)+p2)+p3.
 * BK_E_ARG: a NULL array, C < 0 or D < 0; BK_E_ALIGN: ld < C.  C == 0 or D == 0: BK_OK, nothing launched and
 * nothing written (bk_mala_logq_precond the same). */
int bk_mala_logq(const double* theta, const double* grad, const double* theta_prop,
                 const double* grad_prop, int64_t ld, double eps, double* lp_forward,
                 double* lp_reverse, int64_t C, int64_t D, void* stream);

/* The same densities under a diagonal preconditioner v (mala.py:50-53, 68-79 on theta / sqrt(v); the log-determinant is
 * the same in both directions and is left out), precond = the packed [3][D] {v, sqrt(v), 1/v} of bk_precond_pack:
 *     xf_d = (theta_prop - theta) - eps*(v*grad)       lp_forward[c] = (-0.25/eps) * sum_d (xf_d*xf_d) * (1/v)_d
 *     xr_d = (theta - theta_prop) - eps*(v*grad_prop)  lp_reverse[c] = (-0.25/eps) * sum_d (xr_d*xr_d) * (1/v)_d
 * every product rounded on its own, the sums in bk_mala_logq's order (four contiguous quarters, ((p0+p1)+p2)+p3). */
int bk_mala_logq_precond(const double* theta, const double* grad, const double* theta_prop,
                         const double* grad_prop, int64_t ld, const double* precond, double eps,
                         double* lp_forward, double* lp_reverse, int64_t C, int64_t D, void* stream);

/* The rest of a MALA draw in ONE pass over HBM (mala.py:50-66), plus the next draw's proposal
 * (mala.py:41-45).  A workgroup owns 16 chains x all D dimensions and keeps them on chip (three
 * arrays in registers, grad_prop in LDS) between the per-chain sums and the select:
 *     fwd, rev as bk_mala_logq                                   mala.py:50-53, 68-79
 *     accept[c] = log_u[c] < (lp_prop - lp) + (rev - fwd)        metropolis.py:70-76 (strict <)
 *     theta_out = accept ? theta_prop : theta                    mala.py:62   (theta_out may be theta)
 *     grad      = accept ? grad_prop  : grad      (in place)     mala.py:64
 *     lp        = accept ? lp_prop    : lp        (in place);  ret[c] = the same   mala.py:63, :66
 *     accept_mask[c], *accept_count += number accepted            (each may be NULL)
 * and, if zt_next != NULL (chain-major normals zt_next[c*ldz + d] of the NEXT draw, from
 * bk_normals_chain_major):
 *     theta_prop = (theta_out + eps*grad) + sqrt2eps * z          mala.py:41-45   (in place)
 * Every element of theta_out / grad is rewritten (rejected chains with their own values: whole
 * sectors, no read-modify-write in the memory system).  HBM traffic: 32*D read + 16*D written per
 * chain, + 8*D read and 8*D written with zt_next -- with the model's gradient op (16*D) and the
 * generator's write of zt (8*D) a draw moves 88*D bytes per chain.
 * The per-chain sums run per thread over rows r, r+64, ..., then over a fixed xor tree of the 8
 * rows of a wavefront, then over the 8 wavefronts in order: an order that depends on D only.
 * Supported shapes (bk_mala_step_supported): 0 < D <= 1024, C and ld even, ld >= C, 16-byte aligned arrays,
 * and every byte offset the kernel forms below 2^32 with the 16 bytes of an access added.  The kernel
 * addresses with 32-bit offsets against a 32-bit range check, and a thread forms the offsets of rows
 * r + 64 e (r <= 63, e < E; E = 2, 4, 8, 16 for D <= 128, 256, 512, 1024) whatever D is, so with
 * S = (E - 1) * 64 * ld * 8:
 *     ((63*ld + C - 2) * 8) + S + 16 < 2^32   and   (((D - 1)*ld + C) * 8) + S + 16 < 2^32,
 * and D * ld < 2^28 as before.  With zt_next also ((C - 1)*ldz + D) * 8 < 2^32 and
 * (C - 1)*ldz*8 + 16*63 + 1024*(E/2 - 1) + 16 < 2^32 (bk_mala_step_supported does not see ldz; ldz <= 64 E
 * never adds a restriction).  Otherwise BK_E_ALIGN, decided before any HIP call -- callers then use
 * bk_mala_logq + bk_mh_accept + bk_select_columns.  C == 0 or D == 0: BK_OK, nothing launched. */
int bk_mala_step_supported(int64_t C, int64_t D, int64_t ld);
int bk_mala_step(const double* theta, double* theta_out, double* grad, double* theta_prop,
                 const double* grad_prop, int64_t ld, double* lp, const double* lp_prop,
                 const double* log_u, const double* zt_next, int64_t ldz, double eps,
                 double sqrt2eps, uint8_t* accept_mask, double* ret, uint32_t* accept_count,
                 int64_t C, int64_t D, void* stream);

/* bk_mala_step under a diagonal preconditioner (mala.py:41-66 on theta / sqrt(v)): fwd, rev as bk_mala_logq_precond -- in
 * THIS kernel's summation order --, the same decision and select, and the next proposal as
 * bk_mala_propose_from_normals_precond.  precond: the packed [3][D] {v, sqrt(v), 1/v} of bk_precond_pack (required; rows
 * are staged in LDS, 16 KiB more at D > 512).  Same shapes, checks and traffic as bk_mala_step (+ 24*D bytes of
 * cache-resident vectors per workgroup); with v = 1 the same draws bit for bit. */
int bk_mala_step_precond(const double* theta, double* theta_out, double* grad, double* theta_prop,
                         const double* grad_prop, int64_t ld, const double* precond, double* lp,
                         const double* lp_prop, const double* log_u, const double* zt_next, int64_t ldz,
                         double eps, double sqrt2eps, uint8_t* accept_mask, double* ret,
                         uint32_t* accept_count, int64_t C, int64_t D, void* stream);

/* ---- built-in targets: the "thin C-ABI callback" form of GradModel.log_density_gradient
 * (typing.py:25-27) batched over chains.  grad and/or logp may be NULL (HMC discards lp
 * inside the trajectory, hmc.py:45,50).  Operation order = oracle/models.py.
 *   iso     : logp = -0.5*sum th^2            grad = -th
 *   diag    : t = lam*th; logp = -0.5*sum th*t; grad = -t
 *   funnel  : v = th[0], n = D-1, ev = exp(-v), s = sum_{i>=1} th_i^2 in the library's canonical order for
 *             lane-spread densities (csrc/bk_lanes.hpp), for every D: row d is in class c = (d-1) mod 16;
 *             cs[c] = the class's rows summed in order; q[g] = ((cs[g] + cs[g+4]) + cs[g+8]) + cs[g+12];
 *             s = ((q[0] + q[1]) + q[2]) + q[3]
 *             logp = ((-(v*v)/18) - (0.5*n)*v) - (0.5*ev)*s
 *             grad0 = ((-v/9) - 0.5*n) + (0.5*ev)*s ; grad_i = -(ev*th_i)
 */
int bk_target_iso_gaussian_grad(const double* theta, double* grad, double* logp, int64_t ld,
                                int64_t C, int64_t D, void* stream);
int bk_target_diag_gaussian_grad(const double* theta, double* grad, double* logp, int64_t ld,
                                 const double* lam, int64_t C, int64_t D, void* stream);
int bk_target_funnel_grad(const double* theta, double* grad, double* logp, int64_t ld,
                          int64_t C, int64_t D, void* stream);

/* The same gradients for a lane set whose size lives on the device (n_dev, see bk_leapfrog_kick_drift_n):
 * chains [0, min(C, *n_dev)) of the arrays are evaluated, the launch is sized for C. */
int bk_target_iso_gaussian_grad_n(const double* theta, double* grad, double* logp, int64_t ld,
                                  int64_t C, int64_t D, const uint32_t* n_dev, void* stream);
int bk_target_diag_gaussian_grad_n(const double* theta, double* grad, double* logp, int64_t ld,
                                   const double* lam, int64_t C, int64_t D, const uint32_t* n_dev,
                                   void* stream);
int bk_target_funnel_grad_n(const double* theta, double* grad, double* logp, int64_t ld,
                            int64_t C, int64_t D, const uint32_t* n_dev, void* stream);

/* One leapfrog step {gradient, kick, drift} (drghmc.py:280-283; hmc.py:48-50) of Neal's funnel as ONE launch:
 * rho += h * (metric * grad(theta)); theta += h * rho, in place over chains [0, min(n, *n_dev)) (n_dev may be NULL).
 * The same arithmetic as bk_target_funnel_grad_n followed by bk_leapfrog_kick_drift_n -- bit-identical -- in half the
 * launches; the gradient never travels through memory.  (An instantiation of csrc/bk_lanes.hpp's k_lane_op, like the
 * funnel's gradient op; CTarget.from_source(form="lanes") exports the same entry for a user density.) */
int bk_leapfrog_step_funnel(double* theta, double* rho, int64_t ld, const double* metric, double h, int64_t n,
                            int64_t D, const uint32_t* n_dev, void* stream);

/* A whole HMC trajectory (hmc.py:40-53: backward half-kick, steps x {kick, drift, gradient}, forward half-kick) of every
 * chain on Neal's funnel in ONE launch, the gradient inlined (an instantiation of csrc/bk_lanes.hpp's trajectory kernel -- the
 * one behind bk_dr_proposal_funnel -- with hmc.py's first kick; requires D - 1 <= 128 and steps >= 1, BK_E_ARG otherwise).
 * In: theta_in, the momentum rho (OVERWRITTEN with minus the end momentum, which HMC discards) and grad_in, the gradient at
 * theta_in; out: theta_out, grad_out / logp_out there, kin_out = 1/2 sum rho*(metric*rho) at the end (hmc.py:59 -> :37).
 * All [D][ld] arrays share ld.  Follow with bk_mh_accept(BK_ACCEPT_HMC, ...) and bk_select_columns (theta AND grad).
 * CTarget.from_source(form="lanes") exports the same entry for a user density (bk_src_hmc_trajectory_lanes). */
int bk_hmc_trajectory_funnel(const double* theta_in, double* rho, const double* grad_in, double* theta_out,
                             double* grad_out, double* logp_out, double* kin_out, int64_t ld,
                             const double* metric, double eps, int64_t steps, int64_t C, int64_t D, void* stream);

/* ---- user targets (plugin ABI) ------------------------------------------------------------
 * A model the USER compiles into their own shared library plugs in below the samplers through
 * one exported function of this type: GradModel.log_density_gradient (typing.py:25-27) for all
 * chains at once.  theta[d*ld + c] in; grad[d*ld + c] and logp[c] out (either may be NULL);
 * `params` is an opaque pointer owned by the model (host or device memory, its choice); the
 * function only enqueues on `stream` and returns 0 or a nonzero status (hipError_t or its own
 * negative codes).  bayes_kit_amd.CTarget(library, symbol, dims, params) loads it; the samplers
 * then treat it exactly like the bk_target_* functions above (no torch, no Python in the
 * gradient call).  examples/plugin_target/ar1_target.hip is a complete one. */
typedef int (*bk_target_fn)(const double* theta, double* grad, double* logp, int64_t ld,
                            const void* params, int64_t C, int64_t D, void* stream);

/* The counted form of the plugin ABI (optional second export of a user target): as bk_target_fn, with the
 * number of chains to evaluate read ON THE DEVICE -- chains [0, min(C, *n_dev)), n_dev never NULL, the launch
 * sized for the bound C, surplus workgroups exit (one scalar load + compare per workgroup).  A target that
 * exports it (bayes_kit_amd.CTarget(..., counted_symbol=...)) runs DrGhmcDiag without any host
 * synchronisation inside a draw: the gradient calls of drghmc.py:280-283 for the data-dependent lane sets of
 * a delayed-rejection stage become part of one captured hipGraph.  examples/plugin_target/funnel_target.hip
 * exports both forms. */
typedef int (*bk_target_fn_n)(const double* theta, double* grad, double* logp, int64_t ld,
                              const void* params, int64_t C, int64_t D, const uint32_t* n_dev,
                              void* stream);

/* Whole HMC trajectory (hmc.py:40-53) for the separable Gaussian targets with the gradient
 * callback inlined: back half-step, `steps` x (kick, drift, grad = -(lam*theta)), forward
 * half-step, all in registers.  lam NULL = iso Gaussian; metric NULL = ones.  Outputs may
 * alias inputs.  Bit-identical to `steps` calls of bk_leapfrog_kick_drift +
 * bk_target_*_gaussian_grad followed by bk_leapfrog_finish's half-kick; HBM traffic 32 B per
 * element per trajectory; bound by the fp64 vector rate (6 flop per element-step). */
int bk_hmc_trajectory_gaussian(const double* theta_in, double* theta_out, const double* rho_in,
                               double* rho_out, int64_t ld, const double* lam, const double* metric,
                               double eps, int64_t steps, int64_t C, int64_t D, void* stream);

/* Trajectory AND energies of one HMC draw (hmc.py:55-59) on the separable Gaussian targets, in
 * one pass over the state: the trajectory above, plus
 *     kin0[c]   = 0.5 * sum_d rho0*(metric*rho0)     hmc.py:57 -> :37   (optional, may be NULL)
 *     kin1[c]   = 0.5 * sum_d rho1*(metric*rho1)     hmc.py:59 -> :37
 *     lp_out[c] = -0.5 * sum_d theta1*(lam*theta1)   the target's log density at the end point
 * with the per-chain sums taken exactly as bk_leapfrog_finish / bk_target_*_gaussian_grad take
 * them (four contiguous quarters of the dimensions, each sequential in d, combined
 * ((p0+p1)+p2)+p3), so the accept test sees bit-identical energies.  The momentum comes either
 * in the state layout (rho_in [D][ld]) or chain-major straight from bk_normals_chain_major
 * (zt[c*ldz + d], rho0 = 0.0 + 1.0*z: `rng.normal(size=D)`, hmc.py:56); exactly one of the two is
 * given.  The end momentum is not stored (hmc.py:58-63 never uses it again).
 * part: caller scratch of 12*C doubles.  HBM traffic 24*D bytes per chain.
 * With lp_cur != NULL (the target's log density at theta_in, per chain) and log_u, the accept test
 * of the draw (hmc.py:60-63) is evaluated by the same launch sequence, exactly as
 * bk_mh_accept(BK_ACCEPT_HMC, lp_cur, kin0, lp_out, kin1, log_u, accept_mask, ret, accept_count)
 * would: accept_mask / ret / accept_count optional, lp_cur updated in place on accepted chains. */
int bk_hmc_draw_gaussian(const double* theta_in, double* theta_out, int64_t ld, const double* rho_in,
                         const double* zt, int64_t ldz, const double* lam, const double* metric,
                         double eps, int64_t steps, double* part, double* kin0, double* kin1,
                         double* lp_out, double* lp_cur, const double* log_u, uint8_t* accept_mask,
                         double* ret, uint32_t* accept_count, int64_t C, int64_t D, void* stream);

/* bk_hmc_draw_gaussian with a proper diagonal preconditioner, precond[3][D] = {v, sqrt(v), 1/v} (required): the
 * trajectory kicks with precond[d] exactly as with a metric; chain-major normals become rho0 = 0.0 + precond[D + d]*z
 * (rho_in is taken as stored: bk_momentum_refresh_precond has scaled it), and
 *     kin0[c] = 0.5 * sum_d rho0*(precond[2*D + d]*rho0)      kin1[c] = 0.5 * sum_d rho1*(precond[2*D + d]*rho1)
 * in the same quarter order: bit-identical to bk_momentum_refresh_precond, the step-by-step trajectory with
 * metric = precond (its first D entries) and bk_leapfrog_finish_precond.  Every other argument as above. */
int bk_hmc_draw_gaussian_precond(const double* theta_in, double* theta_out, int64_t ld, const double* rho_in,
                                 const double* zt, int64_t ldz, const double* lam, const double* precond, double eps,
                                 int64_t steps, double* part, double* kin0, double* kin1, double* lp_out,
                                 double* lp_cur, const double* log_u, uint8_t* accept_mask, double* ret,
                                 uint32_t* accept_count, int64_t C, int64_t D, void* stream);

/* bk_mala_step for a SEPARABLE built-in density (the Gaussians: lam NULL = identity): proposal densities, accept, select and
 * the next draw's proposal (bayes_kit/mala.py:41-66) with both gradients RECOMPUTED from theta / theta_prop where bk_mala_step
 * loads them, and the gradient at the new state never stored -- 56*D bytes per chain-draw with the log-density launch
 * (lp_prop = bk_target_*_gaussian_grad with grad NULL) instead of 88*D.  Same arithmetic on the same values as
 * {bk_target_*_gaussian_grad, bk_mala_step}: bit-identical draws.  Arguments as bk_mala_step without grad / grad_prop. */
int bk_mala_step_gaussian(const double* theta, double* theta_out, double* theta_prop, int64_t ld, const double* lam,
                          double* lp, const double* lp_prop, const double* log_u, const double* zt_next, int64_t ldz,
                          double eps, double sqrt2eps, uint8_t* accept_mask, double* ret, uint32_t* accept_count, int64_t C,
                          int64_t D, void* stream);

/* bk_mala_step_gaussian under a diagonal preconditioner (mala.py:41-66 on theta / sqrt(v)): the arithmetic of
 * bk_mala_step_precond with both gradients recomputed; precond = the packed [3][D] {v, sqrt(v), 1/v} (required).  Same
 * draws bit for bit as {bk_target_*_gaussian_grad, bk_mala_step_precond}. */
int bk_mala_step_gaussian_precond(const double* theta, double* theta_out, double* theta_prop, int64_t ld, const double* lam,
                                  const double* precond, double* lp, const double* lp_prop, const double* log_u,
                                  const double* zt_next, int64_t ldz, double eps, double sqrt2eps, uint8_t* accept_mask,
                                  double* ret, uint32_t* accept_count, int64_t C, int64_t D, void* stream);

/* One whole delayed-rejection proposal (drghmc.py:319-346 -> :253-289) on Neal's funnel in a
 * single launch, gradient callback inlined: chain j of the outputs starts from chain
 * src_index[j] (NULL = j) of the source point (theta_in, rho_in and the source's cached
 * gradient grad_in); first half-kick + drift, (steps-1) x {gradient, kick, drift}, final
 * gradient and log density, last half-kick, momentum flip.  Outputs (compact, ld_out):
 * theta, -rho, gradient and log density at the proposal, kin = 0.5 sum rho*(metric*rho).
 * Requires D - 1 <= 128 (returns BK_E_ARG otherwise: use the step-by-step entry points).
 * The sum over coordinates uses the same fixed order as bk_target_funnel_grad, so the
 * proposal is bit-identical to the step-by-step path.
 * n_dev (may be NULL): device-side lane count, see "Lane counts on the device" above.
 * lanes_out (may be NULL): receives the number of lanes the launch worked on (statistics:
 * gradient evaluations = steps * lanes); lanes_total (may be NULL): the same count is ADDED to it.
 * H_out, h_out, live_out (all or none): additionally perform bk_dr_level_begin for the produced
 * lanes in the same launch (H = -((-logp) + kin), h = 0, live = 1).
 * grad_in NULL: the launch evaluates the source point's gradient itself instead of reading a cached one (the same
 * values: the gradient is a function of theta alone and its sums have one order); grad_out NULL: the end point's gradient
 * is not stored.  A caller that keeps no gradient cache at all (DrGhmcDiag's one-launch path) moves two arrays per launch
 * and per scatter instead of three. */
/* (prototype below, after the structs its optional jobs are described by.) */

/* The arguments of one bk_scatter_columns call, as a job a trajectory launch can carry along. */
typedef struct bk_scatter_job {
  const uint8_t* mask;
  const int32_t* index;
  int64_t n, D;
  double* dst0; const double* src0;
  double* dst1; const double* src1;
  double* dst2; const double* src2;
  int64_t ld_dst, ld_src;
  double* sdst; const double* ssrc;
  const uint32_t* n_dev;
} bk_scatter_job;

/* What a GHOST proposal without ghosts of its own (the first proposal kind: drghmc.py:424 with k = 0) owes its
 * parent level, so that the proposal's launch can do bk_dr_accept_prob_ghost[_next] itself: lane j's parent lane is
 * src_index[j] (the lane it was gathered from).  a_out: the ghost level's `a`; next_index / next_count may be NULL. */
typedef struct bk_ghost_link {
  const double* parent_H;
  double* parent_h;
  uint8_t* parent_live;
  double* parent_a;
  double* a_out;
  double prob_retry;
  int32_t* next_index;
  uint32_t* next_count;
} bk_ghost_link;

/* The FIRST GHOST of the produced proposals (drghmc.py:424 with i = 0), integrated by the proposal's own launch from its
 * registers: h / steps of the first proposal kind.  Every produced lane gets one, lane for lane; only the ghost's joint
 * log density is used, so no ghost arrays exist.  The launch then writes the level's h (= log1p(-exp(g)), or 0) and live
 * (g != 0) itself, parent_a[j] = -inf where g == 0, and appends the lanes that go on to their next ghost to
 * next_index (may be NULL).  lanes_out / lanes_total (may be NULL): the ghost trajectory's lane statistics. */
typedef struct bk_ghost0 {
  double h;
  int64_t steps;
  double* parent_a;
  double prob_retry;
  int32_t* next_index;
  uint32_t* next_count;
  uint32_t* lanes_out;
  uint64_t* lanes_total;
} bk_ghost0;

/* job (may be NULL): a scatter job run by surplus workgroups of the SAME launch: the
 * previous stage's accepted columns move into the chains' current point (drghmc.py:379-381) while this stage's
 * trajectories -- a sparse, latency-bound lane set -- integrate.  The caller guarantees that the job and the
 * proposal touch disjoint memory: the job writes columns of accepted chains and reads the previous stage's
 * proposal buffers, the proposal reads columns of rejected chains and writes its own buffers.
 * ghost (may be NULL; needs H_out): the launch also evaluates each produced lane's acceptance probability against
 * its parent lane and applies it to the parent (bk_ghost_link): one launch instead of two per such ghost.
 * ghost0 (may be NULL; needs H_out): the launch also integrates the first ghost of every produced lane (bk_ghost0) and
 * applies it to the produced level; together with `ghost` only for a level whose ONLY ghost it is
 * (ghost0->next_index NULL) -- the link then sees the level after that ghost. */
int bk_dr_proposal_funnel(const double* theta_in, const double* rho_in, const double* grad_in,
                          int64_t ld_in, const int32_t* src_index, double* theta_out,
                          double* rho_out, double* grad_out, double* logp_out, double* kin_out,
                          int64_t ld_out, const double* metric, double h, int64_t steps, int64_t n,
                          int64_t D, const uint32_t* n_dev, uint32_t* lanes_out, uint64_t* lanes_total,
                          double* H_out, double* h_out, uint8_t* live_out, const bk_scatter_job* job,
                              const bk_ghost_link* ghost, const bk_ghost0* ghost0, void* stream);

/* The separable Gaussians through the same kernel templates (a separable density is a lanes-form density without head
 * coordinates): bk_dr_proposal_funnel and bk_leapfrog_step_funnel for logp = -1/2 sum th*(lam*th), lam NULL = the
 * isotropic Gaussian.  D <= 128 for the proposal (BK_E_ARG otherwise), any D for the step.  theta and rho are bit-identical to
 * the step-by-step path; the log density is summed in the lanes' class order (csrc/bk_lanes.hpp), not in four quarters.
 * The step of a separable density needs no sums: bk_leapfrog_step_gaussian is a STREAMING launch (csrc/bk_elementwise.hpp,
 * every (d, c) element on its own, 16 bytes per lane): 32*D bytes per chain-step, min(n, *n_dev) chains. */
int bk_dr_proposal_gaussian(const double* theta_in, const double* rho_in, const double* grad_in,
                                int64_t ld_in, const int32_t* src_index, double* theta_out,
                                double* rho_out, double* grad_out, double* logp_out, double* kin_out,
                                int64_t ld_out, const double* metric, double h, int64_t steps, int64_t n,
                                int64_t D, const uint32_t* n_dev, uint32_t* lanes_out, uint64_t* lanes_total,
                                double* H_out, double* h_out, uint8_t* live_out, const bk_scatter_job* job,
                                const bk_ghost_link* ghost, const bk_ghost0* ghost0, const double* lam,
                                void* stream);
int bk_leapfrog_step_gaussian(double* theta, double* rho, int64_t ld, const double* lam, const double* metric,
                              double h, int64_t n, int64_t D, const uint32_t* n_dev, void* stream);

/* ---- dense mass matrix (no reference counterpart: parity unpinned) ----------------------------
 * Y[d*ld + c] = sum_k M[d*ldm + k] * X[k*ld + c] for all chains: one fp64 GEMM on the matrix
 * cores (v_mfma_f64_16x16x4_f64), 128 x 128 workgroup tiles, XCD-aware placement.  Used for
 * rho = chol(M) @ z, the kick's M @ grad and the kinetic energy's M^-1 @ rho, where the
 * reference has the elementwise `metric * grad` / `metric * rho` (hmc.py:37,46-52).
 * 2*D*D*C flop. */
int bk_dense_metric_apply(const double* M, int64_t ldm, const double* X, double* Y, int64_t ld,
                          int64_t C, int64_t D, void* stream);

/* The same MFMA GEMM with a rectangular left factor: Y[R x C] = A[R x K] @ X[K x C], all three
 * with the chain index contiguous on the right (design matrices: X_data @ Theta with R = number
 * of observations, X_data^T @ residuals with R = dims).  `work` (may be NULL; work_elems
 * doubles, caller-owned, at least bk_gemm_chains_work_elems(R, K, C) of them) lets the library split a
 * long inner dimension over several workgroups when the output has too few tiles to fill the chip; the
 * slabs are summed in a fixed order.  The split is a function of (R, K) only and calls wider than 2,048
 * chains are cut into column blocks: a chain's result does not depend on how many chains share its call
 * (chains sharded over GPUs reproduce the unsharded run bit for bit).  A `work` that is too small is
 * refused (BK_E_ARG), never answered with another split.  R = 0 or C = 0 returns without touching Y; K = 0 is the
 * empty sum: Y = 0 (bk_gemm_chains_logistic: y_rows[r] - 0.5), and A and X are not read.  A NULL A, X or Y is
 * BK_E_ARG at any size. */
int64_t bk_gemm_chains_work_elems(int64_t R, int64_t K, int64_t C);
int bk_gemm_chains(const double* A, int64_t lda, int64_t R, int64_t K, const double* X, int64_t ldx,
                   double* Y, int64_t ldy, int64_t C, double* work, int64_t work_elems, void* stream);

/* bk_gemm_chains whose result leaves as y_rows[r] - sigmoid(Y[r][c]): the logistic regression's first GEMM with the
 * residual pass (bk_logistic_residual without the log likelihood) in its epilogue -- a gradient-only evaluation is
 * then two launches.  Same values as the GEMM followed by bk_logistic_residual(part = NULL). */
int bk_gemm_chains_logistic(const double* A, int64_t lda, int64_t R, int64_t K, const double* X, int64_t ldx,
                            double* Y, int64_t ldy, int64_t C, const double* y_rows, void* stream);

/* Shifted scatter matrix of the state on the same matrix cores (csrc/bk_cov.hip), in place:
 *     S += (X - center 1^T)(X - center 1^T)^T      S: [D][lds], lds >= D
 *     s += rowsum(X - center 1^T)                  s: [D]
 * X: the engine's [D][ld] array of C chains, ld >= C; center: [D], or NULL = zeros, subtracted as the panels are
 * loaded.  With a center near the mean, (S - s s^T / n) / (n - 1) over n accumulated columns is their covariance
 * without cancellation (the dense-metric warmup, RunningCovariance).  The reduction runs over the chain index; only
 * tile blocks on or below the diagonal are computed and every value is written to (i, j) and (j, i) from S's LOWER
 * triangle: a symmetric S stays exactly symmetric (an asymmetric one takes its lower triangle).  The chains are split
 * into bk_cov_k_chunk(D)-sized chunks, grouped into slabs that are summed in a fixed order through `work` (caller-owned,
 * at least bk_cov_accumulate_work_elems(D, C) doubles): no atomics, the same bits for the same call; the grouping, and
 * with it the last bits, depends on C.  D^2 C (1 + 128 / D) flop.  Non-finite entries of X poison their rows and columns.
 * BK_E_ARG: a NULL X, S or s, C < 0, D < 0, ld < C, lds < D, a NULL or too small `work` (with C, D >= 1); decided before
 * any HIP call.  C == 0 or D == 0: BK_OK, nothing launched. */
int64_t bk_cov_k_chunk(int64_t D);
int64_t bk_cov_accumulate_work_elems(int64_t D, int64_t C);
int bk_cov_accumulate(const double* X, int64_t ld, int64_t C, int64_t D, const double* center, double* S, int64_t lds,
                      double* s, double* work, int64_t work_elems, void* stream);

/* Logistic regression target (BASELINE.json config 5; no reference oracle), between the two
 * GEMMs Z = X_data @ Theta and G = X_data^T @ R:
 *   bk_logistic_residual: Z[n*ldz + c] <- y[n] - sigmoid(z) in place, and
 *       part[s*C + c] = sum over the s-th block of observations of  y z - log(1 + e^z)
 *       (part NULL: gradient only -- no log likelihood is formed; bk_logistic_finish then takes part NULL too
 *       and writes grad only);
 *   bk_logistic_finish:   grad = t*G + (-(inv_prior_var*theta)),
 *       loglik[c] = sum_s part[s*C + c],  logp[c] = t*loglik + (-0.5*inv_prior_var*|theta|^2)
 *       (t = likelihood temperature of smc.py:47-51; 1 for plain sampling). */
int bk_logistic_residual(double* Z, int64_t ldz, const double* y, double* part, int64_t N, int64_t C,
                         int64_t segments, void* stream);
int bk_logistic_finish(const double* G, const double* theta, int64_t ld, const double* part,
                       int64_t segments, double inv_prior_var, double t, double* grad, double* logp,
                       double* loglik, int64_t C, int64_t D, void* stream);

/* GLM targets: regression with a canonical link (no reference counterpart), with the logistic target's structure --
 * one linear predictor, one cell-wise map between the two GEMMs, a residual that is y minus a mean.  Per cell, from
 * z = (X_data Theta)[n][c], the row's y[n], the row's aux[n] (BINOMIAL: trials m; GAUSSIAN: precision w = 1 / sd^2;
 * BERNOULLI, POISSON: no aux) and the row's offset[n] (optional), every line ONE rounded fp64 operation per
 * operator, in this association (the build does not contract):
 *
 *     eta = offset ? z + o : z                       (offset NULL: no load, no addition)
 *     BERNOULLI: e = exp(-|eta|); p = eta >= 0 ? 1/(1+e) : e/(1+e);  r = y - p
 *                term = y*eta - ((eta > 0 ? eta : 0) + log1p(e))
 *     BINOMIAL:  e, p as above;                                      r = y - a*p
 *                term = y*eta - a*((eta > 0 ? eta : 0) + log1p(e))
 *     POISSON:   mu = exp(eta);                                      r = y - mu;   term = y*eta - mu
 *     GAUSSIAN:  d = y - eta;                                        r = a*d;      term = -0.5*(r*d)
 *
 * BERNOULLI without an offset is bk_logistic_residual's / bk_gemm_chains_logistic's arithmetic: the same bits.  `term`
 * leaves out the observation's normalising constant (log binomial coefficient, -log y!, 0.5 (log w - log 2 pi)): the
 * caller adds its sum once (bk.GLM carries it as one more row of `part` for bk_logistic_finish to sum).
 * No clamping; a non-finite eta gives what IEEE gives (a: 1 for BERNOULLI, m for BINOMIAL; w finite and > 0):
 *
 *     BERNOULLI / BINOMIAL     r        term, y = 0          term, y > 0
 *       eta = +inf             y - a    NaN  (0 * inf)        NaN  (inf - inf)
 *       eta = -inf             y        NaN  (0 * -inf)       -inf
 *       eta = NaN              NaN      NaN                   NaN
 *     POISSON
 *       eta = +inf             -inf     NaN  (0 * inf - inf)  NaN  (inf - inf)
 *       eta > 709.78 (finite)  -inf     -inf                  -inf          (exp overflows)
 *       eta = -inf             y        NaN  (0 * -inf)       -inf
 *       eta = NaN              NaN      NaN                   NaN
 *     GAUSSIAN
 *       eta = +inf             -inf     -inf                  -inf
 *       eta = -inf             +inf     -inf                  -inf
 *       eta = NaN              NaN      NaN                   NaN
 *
 * A segment sum with a NaN term is NaN; one with -inf terms and no NaN is -inf.  Other cells and other segment sums
 * keep their bits.
 *
 *   bk_gemm_chains_glm: bk_gemm_chains whose result leaves as r (the cell rule in the GEMM's epilogue; never a split
 *       of K, no work buffer).  Same values as the GEMM followed by bk_glm_residual(part = NULL); degenerate sizes as
 *       bk_gemm_chains (K = 0: the cell rule of z = 0).
 *   bk_glm_residual: Z[n*ldz + c] <- r in place, and part[s*C + c] = the left-to-right sum of `term` over the s-th of
 *       `segments` blocks of ceil(max(N, 1) / segments) observations (blocks past the data: exactly +0.0).  part NULL:
 *       gradient only -- no log1p, nothing stored to part.
 *   bk_logistic_finish serves every family (grad = t*G + (-(inv_prior_var*theta)), the left-to-right sum of part).
 * BK_E_ARG, decided before any launch: an unknown family, aux NULL for BINOMIAL / GAUSSIAN, aux given for BERNOULLI /
 * POISSON, a NULL y (y_rows), segments outside [1, 65535], and what bk_gemm_chains / bk_logistic_residual refuse. */
#define BK_GLM_BERNOULLI 0
#define BK_GLM_BINOMIAL 1
#define BK_GLM_POISSON 2
#define BK_GLM_GAUSSIAN 3
int bk_gemm_chains_glm(const double* A, int64_t lda, int64_t R, int64_t K, const double* X, int64_t ldx, double* Y,
                       int64_t ldy, int64_t C, int family, const double* y_rows, const double* aux_rows,
                       const double* offset_rows, void* stream);
int bk_glm_residual(double* Z, int64_t ldz, int family, const double* y, const double* aux, const double* offset,
                    double* part, int64_t N, int64_t C, int64_t segments, void* stream);

/* out[c] = scale * sum_d x[d*ld + c] * y[d*ld + c]  (kinetic energy 0.5 * rho . (M rho)). */
int bk_dot_columns(const double* x, const double* y, int64_t ld, double scale, double* out,
                   int64_t C, int64_t D, void* stream);

/* ---- sequential Monte Carlo resampling (smc.py:64-75) ---------------------------------------
 * Multinomial resampling with exactly the arithmetic of the reference's
 *     np.random.choice(M, size=m, replace=True, p=weights / weights.sum())        (smc.py:73)
 * from the weights on: total = np.sum(weights) (numpy's pairwise summation, pieces of 8,192 values added in order),
 * p = weights / total, cdf = np.cumsum(p) as ONE sequential chain (written to cdf_work[n]),
 * idx_out[j] = searchsorted(cdf / cdf[n-1], u[j], side="right").  Given the uniforms RandomState.choice would
 * draw, the indices are bit-identical to the reference's (tests/golden/smc_*.npz). */
int bk_resample_indices(const double* weights, int64_t n, const double* u, int64_t m,
                        double* cdf_work, int32_t* idx_out, void* stream);

/* Systematic and stratified resampling (EXTENSION, not in the reference) on a fixed-point cumulative weight that is exact
 * under any summation order, so that the scan is parallel (csrc/bk_resample.hip: a reduce-then-scan of five launches, no
 * workgroup waiting for another of its launch).  weights[n]: unnormalised, finite, >= 0, at least one > 0 (a weight that is
 * not > 0 counts as zero).  m_total slots over all ranks, this call draws the m_local slots J = slot0 + j:
 *     wmax = max_i w_i,  s = 62 - bit_length(n - 1),  q_i = llrint(ldexp(w_i / wmax, s))   (round to nearest even)
 *     Q_i = q_0 + .. + q_i  (int64; non-decreasing; the same bits under every tiling),  Q = Q_{n-1} >= 2^s > m_total
 *     a = Q / m_total, r = Q % m_total,  base_J = J*a + (J*r) / m_total  (= floor(J*Q / m_total)),
 *     o_J = min(a - 1, (int64) floor(u * (double) a)),   idx_out[j] = #{ i : Q_i <= base_J + o_J }   in [0, n - 1]
 * BK_RESAMPLE_STRATIFIED: u = u[j], m_local uniforms in [0, 1); BK_RESAMPLE_SYSTEMATIC: u = u[0] for every slot.
 * No floating-point comparison decides an index: the indices are non-decreasing in J, a particle with q_i = 0 is never
 * chosen, every stratum [floor(J*Q/m), floor((J+1)*Q/m)) holds exactly one point, and under systematic resampling particle
 * i gets floor(m q_i / Q) or ceil(m q_i / Q) offspring.  The price of the quantisation: a weight below 2^-(s+1) of the
 * largest gets no offspring (n = 65,536: s = 46, 7e-15; n = 2^20: s = 42, 1e-13; its expected count was below m times that).
 * work: caller scratch of bk_resample_ordered_work_bytes(n) bytes (-1 for n > 2^31 - 1, 0 for n <= 0), 16-byte aligned;
 * afterwards bytes [16, 16 + 8 n) hold Q as int64.
 * BK_E_ARG: a null pointer, n < 1, m_total < 1, m_local < 0, slot0 < 0, slot0 + m_local > m_total, n or m_total above
 * 2^31 - 1, an unknown mode, work too small or not 16-byte aligned; decided before any HIP call.  m_local == 0: BK_OK,
 * nothing launched. */
#define BK_RESAMPLE_SYSTEMATIC 0
#define BK_RESAMPLE_STRATIFIED 1
int64_t bk_resample_ordered_work_bytes(int64_t n);
int bk_resample_ordered(const double* weights, int64_t n, const double* u, int64_t m_local, int64_t slot0,
                        int64_t m_total, int mode, void* work, int64_t work_bytes, int32_t* idx_out, void* stream);

/* dst[d*ld_dst + j] = src[d*ld_src + index[j]]: the resampled particles (thetas[idxs]). */
int bk_gather_columns(const int32_t* index, const double* src, int64_t ld_src, double* dst,
                      int64_t ld_dst, int64_t m, int64_t D, void* stream);

/* ---- layout helper --------------------------------------------------------------------
 * dst[d*ld + c] = src[c*lds_c + d*lds_d]  (LDS-tiled transpose/copy) -- brings a model's
 * (C, D) row-major output into the engine's chain-contiguous layout, and back with the
 * roles of the strides swapped. */
int bk_relayout(const double* src, int64_t lds_d, int64_t lds_c, double* dst, int64_t ldd_d,
                int64_t ldd_c, int64_t C, int64_t D, void* stream);

/* ---- streaming diagnostics --------------------------------------------------------------
 * Welford update with the n-th draw (n >= 1) of every chain and dimension: per-chain mean
 * and M2 from which rhat.py:163-166 (np.mean, np.var(ddof=1)) follow. */
/* theta has a row pitch of its own (a sampler's state rows may be padded off a power-of-two pitch while the moments are
 * dense: no staging copy of the draw). */
int bk_welford_update(double* mean, double* m2, int64_t ld, const double* theta, int64_t ld_theta,
                      int64_t n, int64_t C, int64_t D, void* stream);
/* ... with the update count in device memory: n = *n_dev - n_offset (e.g. a sampler's draw counter).  A launch like this
 * can be part of a captured draw (hipGraph): nothing of it changes from one replay to the next on the host side. */
int bk_welford_update_dev(double* mean, double* m2, int64_t ld, const double* theta, int64_t ld_theta,
                          const int64_t* n_dev, int64_t n_offset, int64_t C, int64_t D, void* stream);

/* Draw storage for ess / rhat post-processing: row `row` of the K (+1) tracked series,
 * series[k][row][c] = theta[dims[k]][c] (k < K) and series[K][row][c] = logp[c] (logp may be NULL); series is
 * [K (+1)][capacity][C], chain-contiguous -- the [N, C] layout bk_ess / bk_chain_mean_var consume.  dims: device. */
int bk_record_series(const double* theta, int64_t ld, const int32_t* dims, int64_t K, const double* logp,
                     double* series, int64_t capacity, int64_t row, int64_t C, void* stream);

/* The same with row = *row_dev - row_offset read on the device (rows outside [0, capacity) are not written). */
int bk_record_series_dev(const double* theta, int64_t ld, const int32_t* dims, int64_t K, const double* logp,
                         double* series, int64_t capacity, const int64_t* row_dev, int64_t row_offset, int64_t C,
                         void* stream);

/* Per-dimension partial sums over this rank's C chains for R-hat (rhat.py:163-171):
 * out[0*D + d] = sum_c mean ; out[1*D + d] = sum_c var_c (var_c = m2/(n-1)).
 * With `center` != NULL also out[2*D + d] = sum_c (mean - center[d])^2  (second pass of
 * np.var(means, ddof=1)).  Deterministic fixed-shape tree per dimension. */
int bk_rhat_partials(const double* mean, const double* m2, int64_t ld, int64_t n,
                     const double* center, double* out, int64_t C, int64_t D, void* stream);

/* Per-superchain moments for nested R-hat (Margossian et al., "Nested R-hat: assessing the convergence of Markov chain
 * Monte Carlo when running many short chains"): superchain k of a row is the M consecutive chains k*M .. k*M + M - 1 of
 * the [D][ld] Welford moments (n draws per chain), K = C / M superchains per row.
 *     s_out[d*ldk + k] = s  = (sum_m mean) / M
 *     w_out[d*ldk + k] = Bt + Wt,  Bt = sum_m (mean - s)^2 / (M - 1)  (0 for M = 1; centred on the rounded s),
 *                                  Wt = (sum_m m2 / (n - 1)) / M      (0 for n = 1: m2 is not read and may be NULL)
 * The order of every sum depends on M and on a chain's index inside its superchain only: M = 2^j <= 64 the xor butterfly
 * with strides 1, 2, .. M/2; M > 64 bk_rhat_partials' order inside the superchain (thread t adds m = t, t+256, .. in order,
 * the 256 sums are halved 128, 64, .. 1); any other M sequentially in m.  So a superchain's two doubles are the same bits
 * on every run and wherever it sits (other K, ld, a view that starts at a superchain boundary).  No floating-point
 * atomics.  NaN, infinities and a zero w_out are what IEEE arithmetic gives; nothing is filtered.
 * M < 1, n < 1, C % M != 0, a NULL array: BK_E_ARG; ld < C or ldk < K: BK_E_ALIGN; C == 0 or D == 0: BK_OK, no launch. */
int bk_superchain_moments(const double* mean, const double* m2, int64_t ld, int64_t n, int64_t M, double* s_out,
                          double* w_out, int64_t ldk, int64_t C, int64_t D, void* stream);

/* Fixed-grid histograms of every coordinate of a draw (RunningHistogram): counts[d][slot] += the number of chains c whose
 * theta[d][c] falls into `slot`, for theta [D][ld] and counts [D][ldc] int64, ldc >= B + 3.  Row d has B + 3 slots:
 *     0         below the grid            1 .. B    the bins            B + 1    above the grid            B + 2    NaN
 * The slot of x is decided by ONE rule, which is the contract (it is what lets NumPy restate the counts bit for bit):
 *     x != x                  -> B + 2
 *     t = (x - lo[d]) * scale[d]          one rounded fp64 subtraction, then one rounded fp64 multiplication
 *     t < 0                   -> 0        (-inf; not x == lo and not t == -0.0: those are bin 0)
 *     t >= B                  -> B + 1    (+inf, a product that overflows, x == hi on a dyadic grid: the range is half-open)
 *     otherwise               -> 1 + (int64)t
 * x * scale - lo * scale, fused or not, is a different function, and so is a comparison against precomputed edges.
 * lo and scale are device doubles [D]; the caller has made sure that they are finite and scale > 0.  1 <= B <= 65,536.
 * The call ADDS to counts and touches only slots 0 .. B + 2 of each of the D rows (never the padding up to ldc).  ld may be
 * odd: rows need not start on 16 bytes.
 * One workgroup per (row, slab of bk_hist_slab_chains(C, D, B) chains) counts in a private LDS histogram of 32-bit counters
 * (a slab is at most 2^30 chains) and adds its non-zero counters to counts with 64-bit integer atomics: integer sums, so
 * the result is the same bits for every slab size, launch geometry and arrival order.  Up to bk_hist_lds_bins() bins all
 * slots fit one LDS window and the slab is read once; above, the same kernel walks the slots window by window and reads
 * its slab once per window.  HBM traffic 8*C*D bytes plus the touched counters.
 * BK_E_ARG: a NULL pointer, C < 0, D < 0, B < 1, B > 65,536, ld < C, ldc < B + 3, more than 65,535 slabs; decided before
 * any HIP call.  C == 0 or D == 0: BK_OK, nothing launched.  bk_hist_slab_chains returns 0 for arguments without a launch. */
int64_t bk_hist_lds_bins(void);
int64_t bk_hist_slab_chains(int64_t C, int64_t D, int64_t B);
int bk_hist_accumulate(const double* theta, int64_t ld, int64_t C, int64_t D, const double* lo, const double* scale,
                       int64_t B, int64_t* counts, int64_t ldc, void* stream);

/* The acceptance statistic a step-size adaptation averages, before the accept test overwrites lp_cur:
 *     d_c    = (lp_prop[c] - a_prop[c]) - (lp_cur[c] - a_cur[c])      the h1 - h0 of bk_mh_accept in HMC mode
 *     out[0] = sum_c min(1, bk_exp(min(0, d_c)))   over the chains whose d_c is not NaN
 *     out[1] = number of chains whose d_c is NaN
 * a_cur / a_prop NULL = zeros.  bk_exp is include/bkhip_math.h's: the same double on host and device.  The sums are a
 * fixed-shape tree -- 64 chains by the xor butterfly (strides 1, 2, .. 32), four such as ((w0+w1)+w2)+w3 per 256 chains
 * into work, then thread t of ONE workgroup adds partials t, t+256, .. in order and the 256 sums are halved 128, 64, .. 1
 * -- so the bits depend on C only.  work: caller scratch of 2*ceil(C/256) doubles.  C = 0: out = {0, 0}. */
int bk_accept_stat(const double* lp_cur, const double* a_cur, const double* lp_prop, const double* a_prop, int64_t C,
                   double* out, double* work, void* stream);

/* The cross-chain statistic a trajectory-length adaptation ascends (ChEES: Hoffman, Radul, Sountsov 2021), in two
 * launches around the caller's division by the chain count.  theta / theta_p: state and proposal [D][ld / ldp], rho_p: the
 * proposal's velocity [D][ldr], all before the accept test.
 *
 * bk_chees_sums: out[d] = sum_c theta[d][c], out[D + d] = sum_c theta_p[d][c], in bk_rhat_partials' order (one workgroup
 * per d: thread t adds chains t, t+256, .. in order, the 256 sums are halved 128, 64, .. 1).
 *
 * bk_chees_stat: mean[0..D) / mean[D..2D) are the means of theta / theta_p over ALL chains (of all ranks).  Per chain
 *     dp = theta_p[d][c] - mean[D + d]     dc = theta[d][c] - mean[d]
 *     A = sum_d dp*dp     B = sum_d dc*dc     P = sum_d dp*rho_p[d][c]          g_c = (A - B) * P
 *     w_c = 0 if d_c is NaN, else min(1, bk_exp(min(0, d_c)))                     d_c as in bk_accept_stat
 *     out[0] = sum_c w_c*g_c   over the chains with w_c > 0 and g_c finite
 *     out[1] = number of chains with w_c > 0 and g_c not finite
 * The per-chain sums run over four contiguous quarters of d (ceil(D/4) each), sequential inside a quarter, combined
 * ((p0+p1)+p2)+p3, every product and sum rounded on its own; the sums over chains are bk_accept_stat's tree.  No
 * floating-point atomics: the bits depend on (C, D) only.  a_cur / a_prop NULL = zeros.
 * work: caller scratch of 12*C + 2*ceil(C/256) doubles.  C = 0: out = {0, 0}. */
int bk_chees_sums(const double* theta, int64_t ld, const double* theta_p, int64_t ldp, double* out, int64_t C, int64_t D,
                  void* stream);
int bk_chees_stat(const double* theta, int64_t ld, const double* theta_p, int64_t ldp, const double* rho_p, int64_t ldr,
                  const double* mean, const double* lp_cur, const double* a_cur, const double* lp_prop,
                  const double* a_prop, double* out, double* work, int64_t C, int64_t D, void* stream);

/* Energy diagnostics of an HMC accept test (EnergyDiagnostics): divergent transitions and the per-chain statistics of
 * E-BFMI, from the five vectors bk_mh_accept(BK_ACCEPT_HMC, ...) is about to read -- call it BEFORE that test overwrites
 * lp_cur.  One elementwise pass; per chain c, every operation rounded on its own, in this order:
 *     h0 = lp_cur - a_cur;  h1 = lp_prop - a_prop;  d = h1 - h0;  acc = log_u < d        (bk_mh_accept's, bit for bit)
 *     err[c] = d;   divergent = isnan(d) || d < -threshold;   div_mask[c] = divergent    (strict: d == -threshold is not;
 *                                                                                         d = -inf is, d = +inf is not)
 *     trans[c] += 1;   ndiv[c] += divergent
 *     E = -(acc ? h1 : h0)                                   minus the value bk_mh_accept writes to `ret`
 *     E not finite: counted in totals[3], the energy state stays as it is.  Otherwise
 *         cnt[c] += 1;  delta = E - mean;  mean = mean + delta / cnt;  m2 = m2 + delta * (E - mean)       (Welford)
 *         if this is not the chain's first finite energy:  t = E - last;  ssd = ssd + t * t
 *         last = E
 * totals[4] += {chains, divergent chains, chains whose d is NaN, chains whose E is not finite} of this call (64-bit integer
 * atomics after a wavefront ballot; there are no floating-point atomics).  a_cur / a_prop NULL = zeros.  The doubles need
 * 8-byte alignment only and the mask none: every array may be a column slice [c0, c1) of a larger one.
 * BK_E_ARG, decided before any HIP call: a NULL pointer other than a_cur / a_prop, C < 0, a threshold that is not finite
 * and > 0.  C == 0: BK_OK, nothing launched. */
int bk_energy_update(const double* lp_cur, const double* a_cur, const double* lp_prop, const double* a_prop,
                     const double* log_u, double threshold, double* mean_E, double* m2_E, double* last_E, double* ssd,
                     int64_t* trans, int64_t* cnt, int64_t* ndiv, uint8_t* div_mask, double* err, int64_t* totals,
                     int64_t C, void* stream);

/* Keep the columns of the chains flagged in div_mask (bk_energy_update's) in a fixed store of `cap` entries:
 *     theta_div[d][p] = theta[d][c] (theta [D][ld], theta_div [D][cap]),  chain[p] = chain0 + c,  draw[p] = trans[c],
 *     err_store[p] = err[c],   fill = {entries stored, flagged chains seen}.
 * The ORDER is a contract: entries fill in call order and, within a call, by ascending chain, whatever the launch geometry
 * -- an exclusive scan of the flags per block of 256 chains (one workgroup, into `work`), then a gather over (block of
 * chains, block of rows) in which a chain's position is the fill level the call found + its block's prefix + its rank in
 * the block, re-derived from ballots.  No atomic takes part.  Flagged chains past `cap` are counted in fill[1] and not
 * stored: the earliest are kept.  Both kernels are launched whatever the flags say (no host read); without a flag the
 * gather's workgroups return at once.  cap == 0, a NULL theta_div or D == 0: fill[1] alone is counted.
 * work: caller scratch of bk_divergence_capture_work_elems(C) = ceil(C / 256) + 2 int64.
 * BK_E_ARG, decided before any HIP call: div_mask, fill or work NULL, C < 0, D < 0, cap < 0, D > 1,048,560; with a store:
 * any other pointer NULL or ld < C.  C == 0: BK_OK, nothing launched. */
int64_t bk_divergence_capture_work_elems(int64_t C);
int bk_divergence_capture(const uint8_t* div_mask, const double* err, const int64_t* trans, const double* theta,
                          int64_t ld, int64_t C, int64_t D, int64_t chain0, double* theta_div, int64_t* chain,
                          int64_t* draw, double* err_store, int64_t cap, int64_t* fill, int64_t* work, void* stream);

/* Per-chain mean and ddof=1 variance of a stored series x[t*ld + c], t < len[c] (len NULL =
 * all N): the two list comprehensions of rhat.py:165-166 for ragged chains. */
int bk_chain_mean_var(const double* x, int64_t ld, const int32_t* len, int64_t N,
                      double* mean, double* var, int64_t C, void* stream);

/* Rank normalisation (rhat.py:62-108): out[i] = Phi^-1((rank[i] - 0.325) / (S - 0.25)), ranks as
 * doubles (1-based), S = total number of draws; Phi^-1 is Cephes ndtri, the function behind
 * scipy.stats.norm.ppf, evaluated in the same order. */
int bk_rank_normalize(const double* rank, double S, double* out, int64_t n, void* stream);

/* Building blocks of pooled ranks (rhat.py:27-59: every draw replaced by its rank among ALL draws
 * of ALL chains) without replicating the draws on every rank -- a sample sort:
 *   bk_sort_by_key    stable sort of (key, payload) pairs by the RAW ORDER OF THE KEYS' BIT PATTERNS: a key
 *                     with bits b sorts by ~b if its sign bit is set, by b | 2^63 otherwise.  For every
 *                     non-NaN double that is ascending order with -0.0 < +0.0; a NaN sorts by its sign
 *                     bit: sign-bit NaNs FIRST (before -inf), positive NaNs last (after +inf).  0.0 / 0.0
 *                     on an x86 host is a sign-bit NaN: a caller that wants NumPy's order (every NaN
 *                     last, the two zeros tied) canonicalises its keys first, as
 *                     bayes_kit_amd.diagnostics._canonical_keys does.  Equal bit patterns keep their
 *                     input order; every key comes back with its own bits (NaN payloads included) and
 *                     every payload with all 64 of its own.  `work`: caller scratch of
 *                     bk_sort_by_key_work_bytes(n) bytes, 16-byte aligned.  In and out arrays must not
 *                     overlap; n <= 2^31 - 1 (BK_E_ARG otherwise; bk_sort_by_key_work_bytes returns -1).
 *   bk_count_below    out[i] = number of sorted_keys[0..n) strictly below queries[i] in IEEE comparison
 *                     (bucket boundaries for the splitters), by binary search: sorted_keys ascending,
 *                     NaNs, if any, at the end.  A NaN query is below nothing and gives 0 (not n, as
 *                     np.searchsorted would).  n = 0 gives 0 for every query, and sorted_keys may then
 *                     be null.
 *   bk_scatter_ranks  out[payload[j]] = base + (j + 1), j < n: the (1-based, as doubles) ranks of a
 *                     sorted run whose first element has `base` elements before it. */
int64_t bk_sort_by_key_work_bytes(int64_t n);
int bk_sort_by_key(const double* keys_in, double* keys_out, const int64_t* vals_in, int64_t* vals_out,
                   int64_t n, void* work, int64_t work_bytes, void* stream);
int bk_count_below(const double* sorted_keys, int64_t n, const double* queries, int64_t m, int64_t* out,
                   void* stream);
int bk_scatter_ranks(const int64_t* payload, int64_t n, double base, double* out, void* stream);

/* Autocorrelation at all lags 0..N-1 of each chain of a stored series, out[n*ldo + c]
 * (autocorr.py:6-33; same normalisation: / np.var(x) / N).  Direct summation, the series staged in
 * LDS (16 chains per workgroup, one wavefront per chain, one lane per lag: N steps per 64 lags). */
int bk_autocorr(const double* x, int64_t ld, int64_t N, double* out, int64_t ldo, int64_t C,
                void* stream);

/* The same by FFT, as the reference computes it (autocorr.py:23-33: zero-padded to S = 2**ceil(log2(2N-1)), |fft|^2,
 * inverse, / var / N), for chains too long for the LDS-staged direct sums: O(N log N) per chain.  Stockham radix-16
 * passes across the rows of the [N, C] layout, one lane per column pair (two real series per complex transform);
 * work: caller-owned scratch of bk_autocorr_fft_work_bytes(N, C) bytes, 16-byte aligned. */
int64_t bk_autocorr_fft_work_bytes(int64_t N, int64_t C);
int bk_autocorr_fft(const double* x, int64_t ld, int64_t N, double* out, int64_t ldo, int64_t C, void* work,
                    int64_t work_bytes, void* stream);

/* IAT / ESS of each chain from an autocorrelation array acor[n*ld + c], n < N (iat.py:46-135: the
 * Geyer scan alone) -- for autocorrelations obtained elsewhere (bk_autocorr_fft for very long chains). */
int bk_iat_from_acor(const double* acor, int64_t ld, int64_t N, int estimator, double* ess_out,
                     double* iat_out, int64_t C, void* stream);

/* out[c] = index one past the last pair (0,1), (2,3), ... of acor[n*ld + c] before the first pair
 * with a negative sum (iat.py:7-43, the truncation point of both IAT estimators). */
int bk_end_pos_pairs(const double* acor, int64_t ld, int64_t N, int64_t* out, int64_t C,
                     void* stream);

/* ESS of each chain of a stored series (ess.py:52-69 -> iat.py:95-135 -> autocorr.py:6-33):
 * autocorrelations by direct summation (same quantity the reference gets by FFT) from an LDS-staged
 * tile -- 64 lags per N steps per wavefront, only as many 64-lag blocks as the truncation needs --, Geyer
 * initial-positive truncation at the first even lag pair with negative sum, initial
 * monotone running-min sum, IAT = 2*sum - 1, ESS = N/IAT.  estimator 0 = IMSE (ess /
 * ess_imse), 1 = IPSE (ess_ipse).  iat_out may be NULL. */
int bk_ess(const double* x, int64_t ld, int64_t N, int estimator, double* ess_out,
           double* iat_out, int64_t C, void* stream);

/* ---- multi-chain ESS (Vehtari, Gelman, Simpson, Carpenter and Buerkner 2021, "Rank-normalization, folding, and
 * localization: an improved R-hat for assessing convergence of MCMC", Bayesian Analysis 16(2), sec. 3.2, eqs. 10-11;
 * Stan's compute_effective_sample_size) -- the device parts of bulk / tail / mean ESS over all chains.
 * Split set: column c of the [N, C] series x[t*ld + c] gives the chains rows [0, n) and rows [N - n, N), n = N / 2;
 * chain m = h * C + c (h = half), M = 2 C.  indicator != 0 reads every draw as (x <= q) ? 1 : 0.  Sums over chains are
 * per-workgroup partials reduced in a fixed order: repeated calls are bit-identical.  work: caller scratch of
 * bk_ess_multi_work_bytes(n, C, nlags) bytes (nlags = the largest lag count of a call; 1 for the moments). */
int64_t bk_ess_multi_work_bytes(int64_t n, int64_t C, int64_t nlags);
/* Per split chain chain_mean[m] and gamma_{m,0} = (1/n) sum_i (x_{m,i} - mean_m)^2 (chain_g0[m]), [2C] each;
 * out[0] = sum_m mean_m, out[1] = sum_m gamma_{m,0}, out[2] = number of non-finite draws (of x itself). */
int bk_ess_split_moments(const double* x, int64_t ld, int64_t N, int64_t C, int indicator, double q, double* chain_mean,
                         double* chain_g0, double* out, void* work, int64_t work_bytes, void* stream);
/* out[0] = sum_m (chain_mean[m] - centre[0])^2 over M chains (the second pass of the between-chain variance around a
 * centre gathered over all ranks). */
int bk_ess_between_sq(const double* chain_mean, int64_t M, const double* centre, double* out, void* work,
                      int64_t work_bytes, void* stream);
/* Cross-chain lag sums out[t - lag0] = sum_m gamma_{m,t}, gamma_{m,t} = (1/n) sum_{i < n - t} (x_{m,i} - mean_m)
 * (x_{m,i+t} - mean_m), for t in [lag0, lag0 + nlags) (lag0 + nlags <= n); chain_mean from bk_ess_split_moments.  The
 * chains are staged in LDS once (one wavefront per chain, 64 lags per pass, register tiles from 288 draws on) for every
 * requested lag; a request whose per-workgroup partials would pass 256 MiB runs as several launches.  Halves longer than
 * bk_ess_lag_sums_max_half() return BK_E_ARG: bk_autocorr_fft on the half views, then bk_ess_acov_sums. */
int64_t bk_ess_lag_sums_max_half(void);
int bk_ess_lag_sums(const double* x, int64_t ld, int64_t N, int64_t C, int indicator, double q, const double* chain_mean,
                    int64_t lag0, int64_t nlags, double* out, void* work, int64_t work_bytes, void* stream);
/* out[t - lag0] = sum_c chain_g0[c] * acor[t*ldo + c] over C chains of an autocorrelation array (bk_autocorr_fft of one
 * half, a batch of chains); chains with chain_g0 = 0 (constant) contribute 0. */
int bk_ess_acov_sums(const double* acor, int64_t ldo, int64_t n, int64_t C, const double* chain_g0, int64_t lag0,
                     int64_t nlags, double* out, void* work, int64_t work_bytes, void* stream);
/* out[t*ldo + c] = (x[t*ld + c] <= q) ? 1 : 0, t < n: the indicator chains for the FFT route of tail ESS. */
int bk_ess_indicator(const double* x, int64_t ld, int64_t n, int64_t C, double q, double* out, int64_t ldo, void* stream);
/* Order statistics by global rank (the quantile of tail ESS across ranks): out[j] = values[i] for the element whose 1-based
 * rank[i] equals targets[j], j < k <= 8; other entries of out are left alone (zero them, then sum over ranks).  n = 0 (a rank
 * without chains) returns BK_OK without a launch, whatever rank and values point to. */
int bk_select_ranks(const double* rank, const double* values, int64_t n, const double* targets, int64_t k, double* out,
                    void* stream);

/* ---- host-side self-test hooks (tests only; they run the SAME source as the kernels on
 * the host so the RNG can be checked against numpy without a GPU).  Host pointers. */
int bk_host_normals(int rng_kind, uint64_t* state_words /*[BK_RNG_WORDS]*/, double* out,
                    int64_t n);
int bk_host_uniforms(int rng_kind, uint64_t* state_words, double* out, int64_t n);
double bk_host_log1p(double x);
/* bk_exp of include/bkhip_math.h (the funnel's exp: a specified fma sequence, restated in oracle/rng.py), host build. */
double bk_host_exp(double x);

#ifdef __cplusplus
}
#endif
#endif /* BKHIP_H */
