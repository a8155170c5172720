// Parallel tempering (replica exchange) on the [D][ld] state: the accept test of a tempered target and the swap of two
// rungs' columns (include/bkhip.h: bk_tempered_accept, bk_replica_swap), and the leapfrog integrator of a ladder: kick+drift,
// finish and accept test with a per-column inverse temperature and step size (bk_tempered_kick_drift, bk_tempered_finish,
// bk_tempered_hmc_accept), and the exchange pass on one further array (bk_exchange_columns).
//
// A swap pair is column c and column c + H: two adjacent slices of H contiguous columns.  The decision reads ll[c] and
// ll[c + H], which the swap itself overwrites, and the exchange of theta is tiled over row blocks: the decision is
// therefore taken ONCE, by a [C]-sized pass of its own that writes `swapped` and exchanges the scalars, and the
// row-blocked exchange pass that follows on the stream reads nothing but `swapped`.  No workgroup depends on another.
#include "bk_common.hpp"

namespace {

constexpr int TEMPER_BLOCK = 256;
constexpr int TEMPER_ROWS = 4;  // rows per workgroup of the exchange: 8 loads (16-byte ones on the wide form) in flight

// counts[g] += the number of lanes of this wavefront with `take`, g = the lane's block of H columns: one atomic per
// wavefront where all of its columns [k0, k1] lie in one block (ballot + popcount), one per lane otherwise.  Integer
// adds: exact in any order.  Every lane of the wavefront must call it; k0, k1: the wavefront's first and last column.
__device__ __forceinline__ void count_per_block(bool take, i64 k, i64 k0, i64 k1, i64 H, uint32_t* counts) {
  if (k0 / H == k1 / H) {  // wavefront-uniform
    const unsigned long long b = __ballot(take);
    if ((threadIdx.x & (BK_WAVE - 1)) == 0 && b) atomicAdd(counts + k0 / H, (uint32_t)__popcll(b));
  } else if (take) {
    atomicAdd(counts + k / H, 1u);
  }
}

__global__ __launch_bounds__(TEMPER_BLOCK) void k_tempered_accept(double* ll, double* lp0, const double* ll_prop,
                                                                  const double* lp0_prop, const double* beta,
                                                                  const double* zterm, const double* log_u,
                                                                  uint8_t* mask, uint32_t* counts, i64 n, i64 H) {
  const i64 k = (i64)blockIdx.x * TEMPER_BLOCK + threadIdx.x;
  bool acc = false;
  if (k < n) {
    const double l0 = ll[k], l1 = ll_prop[k];
    double p1 = 0.0, dp = 0.0;
    if (lp0) {
      p1 = lp0_prop[k];
      dp = p1 - lp0[k];
    }
    acc = log_u[k] < (dp + beta[k] * (l1 - l0)) + zterm[k];  // (NaN on either side: false)
    mask[k] = acc ? 1 : 0;
    if (acc) {
      ll[k] = l1;
      if (lp0) lp0[k] = p1;
    }
  }
  if (counts) {
    const i64 k0 = k - (threadIdx.x & (BK_WAVE - 1));
    if (k0 < n) count_per_block(acc, k, k0, k0 + BK_WAVE - 1 < n ? k0 + BK_WAVE - 1 : n - 1, H, counts);
  }
}

// the decision, once per pair, from the values before the swap; the scalars are exchanged here
__global__ __launch_bounds__(TEMPER_BLOCK) void k_swap_decide(double* ll, double* lp0, const double* beta,
                                                              const double* log_u, const uint8_t* lower,
                                                              uint8_t* swapped, uint32_t* proposed, uint32_t* accepted,
                                                              i64 C, i64 H) {
  const i64 c = (i64)blockIdx.x * TEMPER_BLOCK + threadIdx.x;
  bool prop = false, acc = false;
  if (c < C) {
    prop = c + H < C && lower[c] != 0;  // (a column without a partner inside the C columns takes no part)
    if (prop) {
      const double la = ll[c], lb = ll[c + H];
      acc = log_u[c] < (beta[c] - beta[c + H]) * (lb - la);  // (0 * inf, -inf - -inf: NaN, refused)
      if (acc) {
        ll[c] = lb;
        ll[c + H] = la;
        if (lp0) {
          const double pa = lp0[c], pb = lp0[c + H];
          lp0[c] = pb;
          lp0[c + H] = pa;
        }
      }
    }
    swapped[c] = acc ? 1 : 0;
  }
  const i64 c0 = c - (threadIdx.x & (BK_WAVE - 1));
  if (c0 < C) {
    const i64 c1 = c0 + BK_WAVE - 1 < C ? c0 + BK_WAVE - 1 : C - 1;
    if (proposed) count_per_block(prop, c, c0, c1, H, proposed);
    if (accepted) count_per_block(acc, c, c0, c1, H, accepted);
  }
}

// columns c and c + H of a [D][ld] array change places where swapped[c]; one lane per pair, TEMPER_ROWS rows per workgroup
__global__ __launch_bounds__(TEMPER_BLOCK) void k_swap_exchange(double* __restrict__ x, i64 ld,
                                                                const uint8_t* __restrict__ swapped, i64 m, i64 H,
                                                                i64 D) {
  const i64 c = (i64)blockIdx.x * TEMPER_BLOCK + threadIdx.x;
  if (c >= m || !swapped[c]) return;  // m = C - H: every column that has a partner; a refused pair moves no bytes
  const i64 d0 = (i64)blockIdx.y * TEMPER_ROWS;
  double* a = x + d0 * ld + c;
  double* b = a + H;
  double va[TEMPER_ROWS], vb[TEMPER_ROWS];
#pragma unroll
  for (int u = 0; u < TEMPER_ROWS; ++u)
    if (d0 + u < D) {
      va[u] = a[u * ld];
      vb[u] = b[u * ld];
    }
#pragma unroll
  for (int u = 0; u < TEMPER_ROWS; ++u)
    if (d0 + u < D) {
      a[u * ld] = vb[u];
      b[u * ld] = va[u];
    }
}

// two adjacent pairs per lane: H, ld, m even and x 16-byte aligned, so columns 2p, 2p + 1 and their partners are two
// aligned 16-byte words; a lane of which only one pair swapped moves that pair's 8-byte words alone
__global__ __launch_bounds__(TEMPER_BLOCK) void k_swap_exchange_v2(double* __restrict__ x, i64 ld,
                                                                   const uint8_t* __restrict__ swapped, i64 m2, i64 H,
                                                                   i64 D) {
  const i64 p = (i64)blockIdx.x * TEMPER_BLOCK + threadIdx.x;
  if (p >= m2) return;
  const i64 c = 2 * p;
  const bool s0 = swapped[c] != 0, s1 = swapped[c + 1] != 0;
  if (!s0 && !s1) return;
  const i64 d0 = (i64)blockIdx.y * TEMPER_ROWS;
  if (s0 && s1) {
    double* a = x + d0 * ld + c;
    double* b = a + H;
    double2 va[TEMPER_ROWS], vb[TEMPER_ROWS];
#pragma unroll
    for (int u = 0; u < TEMPER_ROWS; ++u)
      if (d0 + u < D) {
        va[u] = *reinterpret_cast<const double2*>(a + u * ld);
        vb[u] = *reinterpret_cast<const double2*>(b + u * ld);
      }
#pragma unroll
    for (int u = 0; u < TEMPER_ROWS; ++u)
      if (d0 + u < D) {
        *reinterpret_cast<double2*>(a + u * ld) = vb[u];
        *reinterpret_cast<double2*>(b + u * ld) = va[u];
      }
    return;
  }
  double* a = x + d0 * ld + c + (s1 ? 1 : 0);
  double* b = a + H;
  double va[TEMPER_ROWS], vb[TEMPER_ROWS];
#pragma unroll
  for (int u = 0; u < TEMPER_ROWS; ++u)
    if (d0 + u < D) {
      va[u] = a[u * ld];
      vb[u] = b[u * ld];
    }
#pragma unroll
  for (int u = 0; u < TEMPER_ROWS; ++u)
    if (d0 + u < D) {
      a[u * ld] = vb[u];
      b[u * ld] = va[u];
    }
}

void launch_exchange(double* x, i64 ld, const uint8_t* swapped, i64 C, i64 H, i64 D, hipStream_t s) {
  const i64 m = C - H;
  const unsigned rows = (unsigned)bk_cdiv(D, TEMPER_ROWS);
  if (H % 2 == 0 && ld % 2 == 0 && bk_aligned16(x))  // (C is a multiple of H: m is even too)
    k_swap_exchange_v2<<<dim3((unsigned)bk_cdiv(m / 2, TEMPER_BLOCK), rows), dim3(TEMPER_BLOCK), 0, s>>>(x, ld, swapped,
                                                                                                        m / 2, H, D);
  else
    k_swap_exchange<<<dim3((unsigned)bk_cdiv(m, TEMPER_BLOCK), rows), dim3(TEMPER_BLOCK), 0, s>>>(x, ld, swapped, m, H, D);
}

// ---- the leapfrog integrator of a ladder ------------------------------------------------------------------------------
// Column c has its own inverse temperature beta[c] and step size eps[c] (and pre[c], kick[c], half[c]: multiples of it the
// caller formed), so what bk_leapfrog_kick_drift takes as scalars are [C] vectors here.  The arithmetic per element is
// kd_elem's of bk_integrator.hip with the force f = grad_lp0 + beta * grad_ll in place of the gradient: with beta = 1,
// no grad_lp0 and uniform vectors the same doubles (1.0 * g is g).
//
// Traffic model of kick+drift: theta, rho and grad_ll read, theta and rho written = 40 bytes per element, 48 with grad_lp0,
// all streamed from HBM once.  The per-column vectors (beta, eps, pre, kick) are 8 C bytes each: a workgroup reads its
// columns' entries ONCE and keeps them in registers for its TKD_ROWS = 4 rows, so they add 32 / 4 = 8 bytes per element of
// requests, served from L2 / the Infinity Cache after each XCD's first touch (32 C bytes against 40 D C: 1 / (1.25 D) of the
// stream from HBM, 0.08 % at D = 1,024).  Finish: rho and grad_ll read = 16 bytes per element (24 with grad_lp0, +8 with
// rho_out); a lane walks a quarter of the rows of its columns, so beta and half are read once per lane: 16 C bytes x 4
// wavefronts per launch.
constexpr int TKD_ROWS = 4;
typedef double tvec2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ double tkd_force(double gl, double g0, bool has_g0, double beta, double m, bool has_m) {
  double f = beta * gl;
  if (has_g0) f = g0 + f;
  return has_m ? m * f : f;  // metric NULL == ones, not multiplied in
}

__device__ __forceinline__ double tkd_elem(double th, double rho, double t, double eps, bool use_pre, double pre,
                                           bool use_kick, double kick, double& rho_new) {
  double r = rho;
  if (use_pre) r = r + pre * t;
  if (use_kick) r = r + kick * t;
  rho_new = r;
  return th + eps * r;
}

// two columns (16 bytes) per lane: C, ld, ldg even and every array 16-byte aligned.  The two columns of a lane may lie on
// different rungs (odd H): each component takes its own entry of the vectors.
template <bool NT>
__global__ __launch_bounds__(TEMPER_BLOCK) void k_tempered_kick_drift_v2(
    const double* th_in, double* th_out, const double* rho_in, double* rho_out, i64 ld, const double* grad_ll,
    const double* grad_lp0, i64 ldg, const double* metric, const double* beta, const double* eps, const double* pre,
    const double* kick, i64 C2, i64 D) {
  const i64 c2 = (i64)blockIdx.x * TEMPER_BLOCK + threadIdx.x;
  const i64 d0 = (i64)blockIdx.y * TKD_ROWS;
  if (c2 >= C2) return;
  const tvec2 zero = {0.0, 0.0};
  const tvec2 b = *reinterpret_cast<const tvec2*>(beta + 2 * c2);
  const tvec2 e = *reinterpret_cast<const tvec2*>(eps + 2 * c2);
  const tvec2 p = pre ? *reinterpret_cast<const tvec2*>(pre + 2 * c2) : zero;
  const tvec2 k = kick ? *reinterpret_cast<const tvec2*>(kick + 2 * c2) : zero;
  tvec2 t[TKD_ROWS], r[TKD_ROWS], g[TKD_ROWS], g0[TKD_ROWS];
  double m[TKD_ROWS];
#pragma unroll
  for (int i = 0; i < TKD_ROWS; ++i) {
    const i64 d = d0 + i;
    if (d < D) {
      const tvec2* pt = reinterpret_cast<const tvec2*>(th_in + d * ld + 2 * c2);
      const tvec2* pr = reinterpret_cast<const tvec2*>(rho_in + d * ld + 2 * c2);
      const tvec2* pg = reinterpret_cast<const tvec2*>(grad_ll + d * ldg + 2 * c2);
      if (NT) {
        t[i] = __builtin_nontemporal_load(pt);
        r[i] = __builtin_nontemporal_load(pr);
        g[i] = __builtin_nontemporal_load(pg);
      } else {
        t[i] = *pt;
        r[i] = *pr;
        g[i] = *pg;
      }
      g0[i] = zero;
      if (grad_lp0) {
        const tvec2* p0 = reinterpret_cast<const tvec2*>(grad_lp0 + d * ldg + 2 * c2);
        g0[i] = NT ? __builtin_nontemporal_load(p0) : *p0;
      }
      m[i] = metric ? metric[d] : 1.0;
    }
  }
#pragma unroll
  for (int i = 0; i < TKD_ROWS; ++i) {
    const i64 d = d0 + i;
    if (d < D) {
      tvec2 rn, tn;
      double rx, ry;
      const double fx = tkd_force(g[i].x, g0[i].x, grad_lp0 != nullptr, b.x, m[i], metric != nullptr);
      const double fy = tkd_force(g[i].y, g0[i].y, grad_lp0 != nullptr, b.y, m[i], metric != nullptr);
      tn.x = tkd_elem(t[i].x, r[i].x, fx, e.x, pre != nullptr, p.x, kick != nullptr, k.x, rx);
      tn.y = tkd_elem(t[i].y, r[i].y, fy, e.y, pre != nullptr, p.y, kick != nullptr, k.y, ry);
      rn.x = rx;
      rn.y = ry;
      tvec2* qr = reinterpret_cast<tvec2*>(rho_out + d * ld + 2 * c2);
      tvec2* qt = reinterpret_cast<tvec2*>(th_out + d * ld + 2 * c2);
      if (NT) {
        __builtin_nontemporal_store(rn, qr);
        __builtin_nontemporal_store(tn, qt);
      } else {
        *qr = rn;
        *qt = tn;
      }
    }
  }
}

// one column (8 bytes) per lane: odd C or pitch, views that are 8-byte aligned only
__global__ __launch_bounds__(TEMPER_BLOCK) void k_tempered_kick_drift_s(
    const double* th_in, double* th_out, const double* rho_in, double* rho_out, i64 ld, const double* grad_ll,
    const double* grad_lp0, i64 ldg, const double* metric, const double* beta, const double* eps, const double* pre,
    const double* kick, i64 C, i64 D) {
  const i64 c = (i64)blockIdx.x * TEMPER_BLOCK + threadIdx.x;
  const i64 d0 = (i64)blockIdx.y * TKD_ROWS;
  if (c >= C) return;
  const double b = beta[c], e = eps[c], p = pre ? pre[c] : 0.0, k = kick ? kick[c] : 0.0;
  double t[TKD_ROWS], r[TKD_ROWS], g[TKD_ROWS], g0[TKD_ROWS], m[TKD_ROWS];
#pragma unroll
  for (int i = 0; i < TKD_ROWS; ++i) {
    const i64 d = d0 + i;
    if (d < D) {
      t[i] = th_in[d * ld + c];
      r[i] = rho_in[d * ld + c];
      g[i] = grad_ll[d * ldg + c];
      g0[i] = grad_lp0 ? grad_lp0[d * ldg + c] : 0.0;
      m[i] = metric ? metric[d] : 1.0;
    }
  }
#pragma unroll
  for (int i = 0; i < TKD_ROWS; ++i) {
    const i64 d = d0 + i;
    if (d < D) {
      double rn;
      const double f = tkd_force(g[i], g0[i], grad_lp0 != nullptr, b, m[i], metric != nullptr);
      const double tn = tkd_elem(t[i], r[i], f, e, pre != nullptr, p, kick != nullptr, k, rn);
      rho_out[d * ld + c] = rn;
      th_out[d * ld + c] = tn;
    }
  }
}

// The final half kick and the kinetic energy, in bk_leapfrog_finish's summation order: a workgroup of four wavefronts
// serves 64 lanes, wavefront w sums the contiguous quarter [w Dq, (w + 1) Dq) of the rows sequentially, the quarters are
// combined through LDS as ((p0 + p1) + p2) + p3.  The order depends on D alone.
constexpr int TFIN_WAVES = 4;
constexpr int TFIN_BLOCK = TFIN_WAVES * BK_WAVE;
constexpr int TFIN_UNROLL = 8;

__global__ __launch_bounds__(TFIN_BLOCK) void k_tempered_finish_s(const double* rho_in, double* rho_out, i64 ld,
                                                                  const double* grad_ll, const double* grad_lp0, i64 ldg,
                                                                  const double* metric, const double* beta,
                                                                  const double* half, double* kin_out, i64 C, i64 D) {
  __shared__ double part[TFIN_WAVES][BK_WAVE];
  constexpr int U = TFIN_UNROLL;
  const int lane = threadIdx.x & (BK_WAVE - 1), w = bk_wave_id();
  const i64 c = (i64)blockIdx.x * BK_WAVE + lane;
  const i64 Dq = (D + TFIN_WAVES - 1) / TFIN_WAVES;
  const i64 dlo = w * Dq, dhi = (dlo + Dq < D) ? dlo + Dq : D;
  double kin = 0.0;
  if (c < C) {
    const double b = grad_ll ? beta[c] : 0.0, h = grad_ll ? half[c] : 0.0;
    for (i64 d0 = dlo; d0 < dhi; d0 += U) {
      double r[U], g[U], g0[U];
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (d0 + u < dhi) {
          r[u] = rho_in[(d0 + u) * ld + c];
          g[u] = grad_ll ? grad_ll[(d0 + u) * ldg + c] : 0.0;
          g0[u] = (grad_ll && grad_lp0) ? grad_lp0[(d0 + u) * ldg + c] : 0.0;
        }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (d0 + u < dhi) {
          const double m = metric ? metric[d0 + u] : 1.0;
          double v = r[u];  // grad_ll NULL: the kinetic energy of rho_in as it is
          if (grad_ll) v = r[u] + h * tkd_force(g[u], g0[u], grad_lp0 != nullptr, b, m, metric != nullptr);
          if (rho_out) rho_out[(d0 + u) * ld + c] = v;
          const double mv = metric ? m * v : v;
          kin = kin + v * mv;
        }
    }
  }
  if (!kin_out) return;  // uniform: no barrier needed without the reduction
  part[w][lane] = kin;
  __syncthreads();
  if (w == 0 && c < C) {
    double s = part[0][lane];
#pragma unroll
    for (int k = 1; k < TFIN_WAVES; ++k) s = s + part[k][lane];
    kin_out[c] = 0.5 * s;
  }
}

// the same with two columns (16 bytes) per lane; each component runs the scalar kernel's operation sequence
__global__ __launch_bounds__(TFIN_BLOCK) void k_tempered_finish_v2(const double* rho_in, double* rho_out, i64 ld,
                                                                   const double* grad_ll, const double* grad_lp0, i64 ldg,
                                                                   const double* metric, const double* beta,
                                                                   const double* half, double* kin_out, i64 C2, i64 D) {
  __shared__ tvec2 part[TFIN_WAVES][BK_WAVE];
  constexpr int U = TFIN_UNROLL;
  const int lane = threadIdx.x & (BK_WAVE - 1), w = bk_wave_id();
  const i64 c2 = (i64)blockIdx.x * BK_WAVE + lane;
  const i64 Dq = (D + TFIN_WAVES - 1) / TFIN_WAVES;
  const i64 dlo = w * Dq, dhi = (dlo + Dq < D) ? dlo + Dq : D;
  const tvec2 zero = {0.0, 0.0};
  tvec2 kin = zero;
  if (c2 < C2) {
    const tvec2 b = grad_ll ? *reinterpret_cast<const tvec2*>(beta + 2 * c2) : zero;
    const tvec2 h = grad_ll ? *reinterpret_cast<const tvec2*>(half + 2 * c2) : zero;
    for (i64 d0 = dlo; d0 < dhi; d0 += U) {
      tvec2 r[U], g[U], g0[U];
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (d0 + u < dhi) {
          r[u] = __builtin_nontemporal_load(reinterpret_cast<const tvec2*>(rho_in + (d0 + u) * ld + 2 * c2));
          g[u] = zero;
          g0[u] = zero;
          if (grad_ll) g[u] = __builtin_nontemporal_load(reinterpret_cast<const tvec2*>(grad_ll + (d0 + u) * ldg + 2 * c2));
          if (grad_ll && grad_lp0)
            g0[u] = __builtin_nontemporal_load(reinterpret_cast<const tvec2*>(grad_lp0 + (d0 + u) * ldg + 2 * c2));
        }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (d0 + u < dhi) {
          const double m = metric ? metric[d0 + u] : 1.0;
          tvec2 v = r[u];
          if (grad_ll) {
            v.x = r[u].x + h.x * tkd_force(g[u].x, g0[u].x, grad_lp0 != nullptr, b.x, m, metric != nullptr);
            v.y = r[u].y + h.y * tkd_force(g[u].y, g0[u].y, grad_lp0 != nullptr, b.y, m, metric != nullptr);
          }
          if (rho_out) *reinterpret_cast<tvec2*>(rho_out + (d0 + u) * ld + 2 * c2) = v;
          const double mx = metric ? m * v.x : v.x, my = metric ? m * v.y : v.y;
          kin.x = kin.x + v.x * mx;
          kin.y = kin.y + v.y * my;
        }
    }
  }
  if (!kin_out) return;  // uniform: no barrier needed without the reduction
  part[w][lane] = kin;
  __syncthreads();
  if (w == 0 && c2 < C2) {
    tvec2 s = part[0][lane];
#pragma unroll
    for (int k = 1; k < TFIN_WAVES; ++k) {
      s.x = s.x + part[k][lane].x;
      s.y = s.y + part[k][lane].y;
    }
    s.x = 0.5 * s.x;
    s.y = 0.5 * s.y;
    *reinterpret_cast<tvec2*>(kin_out + 2 * c2) = s;
  }
}

// the accept test of HMC on a tempered target: the joint log densities h = (lp0 + beta ll) - kin of both ends, compared as
// bk_mh_accept(BK_ACCEPT_HMC) compares them
__global__ __launch_bounds__(TEMPER_BLOCK) void k_tempered_hmc_accept(double* ll, double* lp0, const double* kin0,
                                                                      const double* ll_prop, const double* lp0_prop,
                                                                      const double* kin1, const double* beta,
                                                                      const double* log_u, uint8_t* mask, uint32_t* counts,
                                                                      i64 n, i64 H) {
  const i64 k = (i64)blockIdx.x * TEMPER_BLOCK + threadIdx.x;
  bool acc = false;
  if (k < n) {
    const double b = beta[k], l1 = ll_prop[k];
    double e0 = b * ll[k], e1 = b * l1, p1 = 0.0;
    if (lp0) {
      p1 = lp0_prop[k];
      e0 = lp0[k] + e0;
      e1 = p1 + e1;
    }
    const double h0 = e0 - kin0[k], h1 = e1 - kin1[k];
    acc = log_u[k] < h1 - h0;  // (NaN on either side: false)
    mask[k] = acc ? 1 : 0;
    if (acc) {
      ll[k] = l1;
      if (lp0) lp0[k] = p1;
    }
  }
  if (counts) {
    const i64 k0 = k - (threadIdx.x & (BK_WAVE - 1));
    if (k0 < n) count_per_block(acc, k, k0, k0 + BK_WAVE - 1 < n ? k0 + BK_WAVE - 1 : n - 1, H, counts);
  }
}

}  // namespace

extern "C" {

int bk_tempered_accept(double* ll, double* lp0, const double* ll_prop, const double* lp0_prop, const double* beta,
                       const double* zterm, const double* log_u, uint8_t* accept_mask, uint32_t* accept_counts,
                       int64_t n, int64_t H, void* stream) {
  if (!ll || !ll_prop || !beta || !zterm || !log_u || !accept_mask || (lp0 && !lp0_prop)) return BK_E_ARG;
  if (n < 0 || H < 1 || n % H != 0) return BK_E_ARG;
  if (n == 0) return BK_OK;
  k_tempered_accept<<<dim3((unsigned)bk_cdiv(n, TEMPER_BLOCK)), dim3(TEMPER_BLOCK), 0, bk_stream(stream)>>>(
      ll, lp0, ll_prop, lp0_prop, beta, zterm, log_u, accept_mask, accept_counts, n, H);
  BK_RETURN_LAUNCH_STATUS();
}

int bk_replica_swap(double* theta, double* theta2, int64_t ld, double* ll, double* lp0, const double* beta,
                    const double* log_u, const uint8_t* lower, uint8_t* swapped, uint32_t* proposed, uint32_t* accepted,
                    int64_t C, int64_t H, int64_t D, void* stream) {
  if (!theta || !ll || !beta || !log_u || !lower || !swapped) return BK_E_ARG;
  if (C < 0 || D < 0 || H < 1 || C % H != 0 || ld < C) return BK_E_ARG;
  if (bk_cdiv(D, TEMPER_ROWS) > 65535 || C > (i64)INT32_MAX) return BK_E_ARG;
  if (C == 0) return BK_OK;
  hipStream_t s = bk_stream(stream);
  k_swap_decide<<<dim3((unsigned)bk_cdiv(C, TEMPER_BLOCK)), dim3(TEMPER_BLOCK), 0, s>>>(ll, lp0, beta, log_u, lower,
                                                                                        swapped, proposed, accepted, C, H);
  if (C > H && D > 0) {
    launch_exchange(theta, ld, swapped, C, H, D, s);
    if (theta2) launch_exchange(theta2, ld, swapped, C, H, D, s);
  }
  BK_RETURN_LAUNCH_STATUS();
}

int bk_tempered_kick_drift(const double* theta_in, double* theta_out, const double* rho_in, double* rho_out, int64_t ld,
                           const double* grad_ll, const double* grad_lp0, int64_t ldg, const double* metric,
                           const double* beta, const double* eps, const double* pre, const double* kick, int64_t C,
                           int64_t D, void* stream) {
  if (!theta_in || !theta_out || !rho_in || !rho_out || !grad_ll || !beta || !eps || C < 0 || D < 0) return BK_E_ARG;
  if (bk_cdiv(D, TKD_ROWS) > 65535) return BK_E_ARG;
  if (ld < C || ldg < C) return BK_E_ALIGN;
  if (C == 0 || D == 0) return BK_OK;
  hipStream_t s = bk_stream(stream);
  const unsigned rows = (unsigned)bk_cdiv(D, TKD_ROWS);
  const bool vec = C % 2 == 0 && ld % 2 == 0 && ldg % 2 == 0 && bk_aligned16(theta_in) && bk_aligned16(theta_out) &&
                   bk_aligned16(rho_in) && bk_aligned16(rho_out) && bk_aligned16(grad_ll) && bk_aligned16(grad_lp0) &&
                   bk_aligned16(beta) && bk_aligned16(eps) && bk_aligned16(pre) && bk_aligned16(kick);
  if (vec) {
    // streams well past the Infinity Cache take non-temporal accesses, as in bk_leapfrog_kick_drift
    const dim3 grid((unsigned)bk_cdiv(C / 2, TEMPER_BLOCK), rows);
    if (bk_streams_past_llc(bk_distinct_arrays({theta_in, theta_out, rho_in, rho_out, grad_ll, grad_lp0}) * C * D))
      k_tempered_kick_drift_v2<true><<<grid, dim3(TEMPER_BLOCK), 0, s>>>(theta_in, theta_out, rho_in, rho_out, ld, grad_ll,
                                                                         grad_lp0, ldg, metric, beta, eps, pre, kick, C / 2, D);
    else
      k_tempered_kick_drift_v2<false><<<grid, dim3(TEMPER_BLOCK), 0, s>>>(theta_in, theta_out, rho_in, rho_out, ld, grad_ll,
                                                                          grad_lp0, ldg, metric, beta, eps, pre, kick, C / 2, D);
  } else {
    k_tempered_kick_drift_s<<<dim3((unsigned)bk_cdiv(C, TEMPER_BLOCK), rows), dim3(TEMPER_BLOCK), 0, s>>>(
        theta_in, theta_out, rho_in, rho_out, ld, grad_ll, grad_lp0, ldg, metric, beta, eps, pre, kick, C, D);
  }
  BK_RETURN_LAUNCH_STATUS();
}

int bk_tempered_finish(const double* rho_in, double* rho_out, int64_t ld, const double* grad_ll, const double* grad_lp0,
                       int64_t ldg, const double* metric, const double* beta, const double* half, double* kin_out,
                       int64_t C, int64_t D, void* stream) {
  if (!rho_in || C < 0 || D < 0 || (grad_ll && (!beta || !half))) return BK_E_ARG;
  if (ld < C || (grad_ll && ldg < C)) return BK_E_ALIGN;
  if (C == 0 || D == 0) return BK_OK;
  hipStream_t s = bk_stream(stream);
  const bool vec = C % 2 == 0 && ld % 2 == 0 && bk_aligned16(rho_in) && bk_aligned16(rho_out) && bk_aligned16(kin_out) &&
                   (!grad_ll || (ldg % 2 == 0 && bk_aligned16(grad_ll) && bk_aligned16(grad_lp0) && bk_aligned16(beta) &&
                                 bk_aligned16(half)));
  if (vec)
    k_tempered_finish_v2<<<dim3((unsigned)bk_cdiv(C / 2, BK_WAVE)), dim3(TFIN_BLOCK), 0, s>>>(
        rho_in, rho_out, ld, grad_ll, grad_lp0, ldg, metric, beta, half, kin_out, C / 2, D);
  else
    k_tempered_finish_s<<<dim3((unsigned)bk_cdiv(C, BK_WAVE)), dim3(TFIN_BLOCK), 0, s>>>(
        rho_in, rho_out, ld, grad_ll, grad_lp0, ldg, metric, beta, half, kin_out, C, D);
  BK_RETURN_LAUNCH_STATUS();
}

int bk_tempered_hmc_accept(double* ll, double* lp0, const double* kin0, const double* ll_prop, const double* lp0_prop,
                           const double* kin1, const double* beta, const double* log_u, uint8_t* accept_mask,
                           uint32_t* accept_counts, int64_t n, int64_t H, void* stream) {
  if (!ll || !kin0 || !ll_prop || !kin1 || !beta || !log_u || !accept_mask || (lp0 && !lp0_prop)) return BK_E_ARG;
  if (n < 0 || H < 1 || n % H != 0) return BK_E_ARG;
  if (n == 0) return BK_OK;
  k_tempered_hmc_accept<<<dim3((unsigned)bk_cdiv(n, TEMPER_BLOCK)), dim3(TEMPER_BLOCK), 0, bk_stream(stream)>>>(
      ll, lp0, kin0, ll_prop, lp0_prop, kin1, beta, log_u, accept_mask, accept_counts, n, H);
  BK_RETURN_LAUNCH_STATUS();
}

int bk_exchange_columns(double* x, int64_t ld, const uint8_t* swapped, int64_t C, int64_t H, int64_t D, void* stream) {
  if (!x || !swapped || C < 0 || D < 0 || H < 1 || C % H != 0) return BK_E_ARG;
  if (bk_cdiv(D, TEMPER_ROWS) > 65535 || C > (i64)INT32_MAX) return BK_E_ARG;
  if (ld < C) return BK_E_ALIGN;
  if (C == 0 || D == 0 || C <= H) return BK_OK;  // (C == H: no column has a partner)
  launch_exchange(x, ld, swapped, C, H, D, bk_stream(stream));
  BK_RETURN_LAUNCH_STATUS();
}

}  // extern "C"
