// Kernels of the tile-major HMC schedule (hmc.py: the model-opaque loop on Infinity-Cache tiles): a tile's proposal, momentum
// and trajectory gradient are contiguous [D][T] arrays, the state, the generator's momentum and the cached gradient stay
// [D][C].  So the launches at a tile's two ends see arrays of DIFFERENT row pitch and of different residency (one side
// streams from / to HBM, the other is in the cache), and the per-chain reductions run on T chains instead of C.
//   * kick+drift, blend and select with one pitch per array and one access hint per side;
//   * the in-place step of a resident tile -- kick+drift and the Gaussian gradient-only kernel -- with a cache policy per
//     ACCESS (bk_mem_policy.hpp), so that the XCDs' L2s keep theta' across the two launches and nothing else;
//   * the Gaussian log density (+ gradient) and the finish kernel (half kick + kinetic energy) with enough loads in flight
//     to run at the cache's rate on a tile's few workgroups -- the SAME summation order as k_gauss_logp(_v2) / k_finish(_v2);
//   * the momentum refresh of ONE tile out of the generator's chain-major scratch, in the same row-spread style.
// Every shape is a template argument: the library instantiates the one it launches (bk_integrator.hip, bk_targets.hip,
// bk_rng.hip), tools/tile_seam_bench.hip instantiates the candidates it was chosen from (profiles/cache_tiles.md, sections 6, 9).
#pragma once
#include "bk_common.hpp"
#include "bk_mem_policy.hpp"

namespace bkt {

typedef double dvec2 __attribute__((ext_vector_type(2)));

// access hints of a launch: which side is non-temporal (streams past the cache); the other side is plain (stays resident)
constexpr int NT_IN = 1;    // the full-width inputs (kick+drift), the full-width old value (blend: a, select: dst)
constexpr int NT_OUT = 2;   // the outputs
constexpr int NT_TILE = 4;  // the tile-resident operand of blend / select (b, src)
constexpr int RHO_PLAIN = 8;  // kick+drift with NT_IN: the momentum is the tile's own (refreshed in place, resident) and read plain

template <bool NT, class T>
__device__ __forceinline__ T gload(const T* p) {
  return NT ? __builtin_nontemporal_load(p) : *p;
}
template <bool NT, class T>
__device__ __forceinline__ void gstore(T v, T* p) {
  if (NT) __builtin_nontemporal_store(v, p);
  else *p = v;
}

// the element operation of bk_leapfrog_kick_drift (bk_integrator.hip: kd_elem), operation for operation
__device__ __forceinline__ double kd_elem(double th, double rho, double g, double m, bool has_m, double eps, int use_pre,
                                          double pre, int use_kick, double kick, double& rho_new) {
  double t = has_m ? m * g : g;
  double r = rho;
  if (use_pre) r = r + pre * t;
  if (use_kick) r = r + kick * t;
  rho_new = r;
  return th + eps * r;
}

// ---- kick + drift, one pitch per array ------------------------------------------------------------------------------
// Two chains (16 B) per lane, one row per thread and pass; rows walk gridDim.y (any D).  rho_out may be rho_in.
constexpr int KDL_BLOCK = 256;
template <int HINTS>
__global__ __launch_bounds__(KDL_BLOCK) void k_kick_drift_ld(const double* th_in, i64 ld_ti, double* th_out, i64 ld_to,
                                                             const double* rho_in, i64 ld_ri, double* rho_out, i64 ld_ro,
                                                             const double* grad, i64 ldg, const double* metric, double eps,
                                                             int use_pre, double pre, int use_kick, double kick, i64 C2,
                                                             i64 D) {
  constexpr bool NI = (HINTS & NT_IN) != 0, NO = (HINTS & NT_OUT) != 0, NR = NI && (HINTS & RHO_PLAIN) == 0;
  const i64 c2 = (i64)blockIdx.x * KDL_BLOCK + threadIdx.x;
  if (c2 >= C2) return;
  for (i64 d = blockIdx.y; d < D; d += gridDim.y) {
    const dvec2 t = gload<NI>(reinterpret_cast<const dvec2*>(th_in + d * ld_ti + 2 * c2));
    const dvec2 r = gload<NR>(reinterpret_cast<const dvec2*>(rho_in + d * ld_ri + 2 * c2));
    const dvec2 g = gload<NI>(reinterpret_cast<const dvec2*>(grad + d * ldg + 2 * c2));
    const double m = metric ? metric[d] : 1.0;
    dvec2 rn, tn;
    double rx, ry;
    tn.x = kd_elem(t.x, r.x, g.x, m, metric != nullptr, eps, use_pre, pre, use_kick, kick, rx);
    tn.y = kd_elem(t.y, r.y, g.y, m, metric != nullptr, eps, use_pre, pre, use_kick, kick, ry);
    rn.x = rx;
    rn.y = ry;
    gstore<NO>(rn, reinterpret_cast<dvec2*>(rho_out + d * ld_ro + 2 * c2));
    gstore<NO>(tn, reinterpret_cast<dvec2*>(th_out + d * ld_to + 2 * c2));
  }
}

// ---- the in-place step of a resident tile, a cache policy per access -------------------------------------------------
// The plain in-cache pair (k_kick_drift_v2<1, false>, k_gauss_grad_v2<1, false>: two chains per lane, one row per thread,
// 256 threads, the gradient's rows swept from the last to the first) moves every byte between the XCDs and the Infinity
// Cache except the lines that survive in the 32 MiB of L2s from one launch to the next, and with plain accesses two thirds
// of those are lines nobody reads again: rho (the gradient op never touches it) and the gradient kick+drift has just
// consumed.  Theta' is the one array BOTH kernels read.  With the policies below the L2s hold theta' and little else:
//   kick+drift   theta load plain, theta store plain (kept);  rho load and store sc1, g load nt (passing through)
//   gradient     theta load plain (kept);  g store sc1 (written through, the line dropped)
// 63.9 -> 61.2 us per step of an 8,192 x 1,024 tile, 32.9 -> 29.6 at 4,096 chains, 66.8 -> 64.0 on a tile cut out of a
// 65,536-chain state (profiles/cache_tiles.md, section 8: 38 combinations).  Either kernel beside the other's plain form is no
// slower than the plain pair, so neither needs to know its partner.  Measured for grids whose gridDim.x is a multiple of
// 8 (a column block then meets the same XCD's L2 in both launches: tg_row_group() in bk_targets.hip); the callers route
// only those here.  Rows are addressed with 32-bit offsets: the callers' footprint rule keeps a row far below 4 GiB.
// The arithmetic is kd_elem / the gradient expression of k_gauss_grad_v2, operation for operation: the same bits.
#define BKT_KD_TILE_POLICY bkm::PLAIN, bkm::SC1, bkm::NT, bkm::PLAIN, bkm::SC1  // theta, rho, g loads; theta, rho stores
#define BKT_GRAD_TILE_POLICY bkm::PLAIN, bkm::SC1                               // theta load; g store

template <int PT, int PR, int PG, int ST, int SR>
__global__ __launch_bounds__(KDL_BLOCK) void k_kick_drift_tile(double* th, double* rho, i64 ld, const double* grad, i64 ldg,
                                                               const double* metric, double eps, int use_pre, double pre,
                                                               int use_kick, double kick, i64 C2, i64 D) {
  const i64 c2 = (i64)blockIdx.x * KDL_BLOCK + threadIdx.x, d = blockIdx.y;
  if (c2 >= C2) return;
  const uint32_t bytes = (uint32_t)(16 * C2), c = (uint32_t)c2;
  const bkm::Row rt = {th + d * ld, bytes}, rr = {rho + d * ld, bytes}, rg = {grad + d * ldg, bytes};
  const dvec2 t = bkm::load16<PT>(rt, c), r = bkm::load16<PR>(rr, c), g = bkm::load16<PG>(rg, c);
  const double m = metric ? metric[d] : 1.0;
  dvec2 rn, tn;
  double rx, ry;
  tn.x = kd_elem(t.x, r.x, g.x, m, metric != nullptr, eps, use_pre, pre, use_kick, kick, rx);
  tn.y = kd_elem(t.y, r.y, g.y, m, metric != nullptr, eps, use_pre, pre, use_kick, kick, ry);
  rn.x = rx;
  rn.y = ry;
  bkm::store16<SR>(rn, rr, c);
  bkm::store16<ST>(tn, rt, c);
}

// grad = -(lam*theta)  (lam NULL -> grad = -theta); row gridDim.y - 1 - blockIdx.y
template <int PT, int SG>
__global__ __launch_bounds__(KDL_BLOCK) void k_gauss_grad_tile(const double* th, double* g, i64 ld, const double* lam, i64 C2,
                                                               i64 D) {
  const i64 c2 = (i64)blockIdx.x * KDL_BLOCK + threadIdx.x, d = (i64)gridDim.y - 1 - blockIdx.y;
  if (c2 >= C2) return;
  const uint32_t bytes = (uint32_t)(16 * C2), c = (uint32_t)c2;
  const bkm::Row rt = {th + d * ld, bytes}, rg = {g + d * ld, bytes};
  const dvec2 t = bkm::load16<PT>(rt, c);
  const double l = lam ? lam[d] : 1.0;
  dvec2 o;
  o.x = lam ? -(l * t.x) : -t.x;
  o.y = lam ? -(l * t.y) : -t.y;
  bkm::store16<SG>(o, rg, c);
}

// any pitches, any alignment, any layout of the gradient: one chain per lane
static __global__ __launch_bounds__(KDL_BLOCK) void k_kick_drift_ld_s(const double* th_in, i64 ld_ti, double* th_out, i64 ld_to,
                                                               const double* rho_in, i64 ld_ri, double* rho_out, i64 ld_ro,
                                                               const double* grad, i64 ldg_d, i64 ldg_c,
                                                               const double* metric, double eps, int use_pre, double pre,
                                                               int use_kick, double kick, i64 C, i64 D) {
  const i64 c = (i64)blockIdx.x * KDL_BLOCK + threadIdx.x;
  if (c >= C) return;
  for (i64 d = blockIdx.y; d < D; d += gridDim.y) {
    double rn;
    const double m = metric ? metric[d] : 1.0;
    const double tn = kd_elem(th_in[d * ld_ti + c], rho_in[d * ld_ri + c], grad[d * ldg_d + c * ldg_c], m,
                              metric != nullptr, eps, use_pre, pre, use_kick, kick, rn);
    rho_out[d * ld_ro + c] = rn;
    th_out[d * ld_to + c] = tn;
  }
}

// ---- blend and select, one pitch per array --------------------------------------------------------------------------
// The forms of k_blend_v2 / k_select_v2: every 16-byte pair of the output is rewritten (no holes in sectors), a pair that
// is all-accept reads only the proposal, one that is all-reject only the old value.
constexpr int SELL_ROWS = 2;
template <int HINTS>
__global__ __launch_bounds__(256) void k_blend_ld(const uint8_t* mask, const double* a, i64 ld_a, const double* b, i64 ld_b,
                                                  double* out, i64 ld_o, i64 C2, i64 D) {
  constexpr bool NI = (HINTS & NT_IN) != 0, NO = (HINTS & NT_OUT) != 0, NB = (HINTS & NT_TILE) != 0;
  const i64 c2 = (i64)blockIdx.x * 256 + threadIdx.x;
  if (c2 >= C2) return;
  const bool m0 = mask[2 * c2] != 0, m1 = mask[2 * c2 + 1] != 0;
  for (i64 d0 = (i64)blockIdx.y * SELL_ROWS; d0 < D; d0 += (i64)gridDim.y * SELL_ROWS) {
    dvec2 v[SELL_ROWS];
#pragma unroll
    for (int i = 0; i < SELL_ROWS; ++i)
      if (d0 + i < D) {
        if (m0 || m1) v[i] = gload<NB>(reinterpret_cast<const dvec2*>(b + (d0 + i) * ld_b + 2 * c2));
        if (!(m0 && m1)) {
          const dvec2 old = gload<NI>(reinterpret_cast<const dvec2*>(a + (d0 + i) * ld_a + 2 * c2));
          if (!m0) v[i].x = old.x;
          if (!m1) v[i].y = old.y;
        }
      }
#pragma unroll
    for (int i = 0; i < SELL_ROWS; ++i)
      if (d0 + i < D) gstore<NO>(v[i], reinterpret_cast<dvec2*>(out + (d0 + i) * ld_o + 2 * c2));
  }
}

static __global__ __launch_bounds__(256) void k_blend_ld_s(const uint8_t* mask, const double* a, i64 ld_a, const double* b, i64 ld_b,
                                                    double* out, i64 ld_o, i64 C, i64 D) {
  const i64 c = (i64)blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const bool m = mask[c] != 0;
  for (i64 d = blockIdx.y; d < D; d += gridDim.y) out[d * ld_o + c] = m ? b[d * ld_b + c] : a[d * ld_a + c];
}

template <int HINTS>
__global__ __launch_bounds__(256) void k_select_ld(const uint8_t* mask, double* dst, i64 ld_d, const double* src, i64 ld_s,
                                                   i64 C2, i64 D) {
  constexpr bool NI = (HINTS & NT_IN) != 0, NO = (HINTS & NT_OUT) != 0, NB = (HINTS & NT_TILE) != 0;
  const i64 c2 = (i64)blockIdx.x * 256 + threadIdx.x;
  if (c2 >= C2) return;
  const bool m0 = mask[2 * c2] != 0, m1 = mask[2 * c2 + 1] != 0;
  for (i64 d0 = (i64)blockIdx.y * SELL_ROWS; d0 < D; d0 += (i64)gridDim.y * SELL_ROWS) {
    dvec2 v[SELL_ROWS];
#pragma unroll
    for (int i = 0; i < SELL_ROWS; ++i)
      if (d0 + i < D) {
        if (m0 || m1) v[i] = gload<NB>(reinterpret_cast<const dvec2*>(src + (d0 + i) * ld_s + 2 * c2));
        if (!(m0 && m1)) {
          const dvec2 old = gload<NI>(reinterpret_cast<const dvec2*>(dst + (d0 + i) * ld_d + 2 * c2));
          if (!m0) v[i].x = old.x;
          if (!m1) v[i].y = old.y;
        }
      }
#pragma unroll
    for (int i = 0; i < SELL_ROWS; ++i)
      if (d0 + i < D) gstore<NO>(v[i], reinterpret_cast<dvec2*>(dst + (d0 + i) * ld_d + 2 * c2));
  }
}

static __global__ __launch_bounds__(256) void k_select_ld_s(const uint8_t* mask, double* dst, i64 ld_d, const double* src, i64 ld_s,
                                                     i64 C, i64 D) {
  const i64 c = (i64)blockIdx.x * 256 + threadIdx.x;
  if (c >= C || !mask[c]) return;
  for (i64 d = blockIdx.y; d < D; d += gridDim.y) dst[d * ld_d + c] = src[d * ld_s + c];
}

// ---- per-chain reductions on a cache-resident tile -------------------------------------------------------------------
// The sums of k_gauss_logp(_v2) / k_finish(_v2), bit for bit: wavefront w of a workgroup owns the contiguous quarter
// [w*Dq, (w+1)*Dq) of the dimensions and adds its terms in increasing d, each product and sum rounded on its own; the
// quarters are added ((p0+p1)+p2)+p3 through LDS and the result is scaled once.  Those kernels give a chain (pair) to a
// LANE, which loads and adds its rows itself: 128 chains per workgroup, so a tile of 8,192 chains is 64 workgroups on 256
// CUs, each wavefront with 8 rows in flight and idle while it adds -- 73 us for what the gradient-only launch moves in 20.
// Only the ADDITION has to be sequential.  Here a wavefront spreads the rows of CP chain pairs over all its lanes: lane
// (j, ph) = (lane % CP, lane / CP) takes rows ph, ph + PH, ... (PH = 64 / CP) of pair j, so a chunk of R = U * PH rows is U
// independent 16-byte loads per lane; every lane forms its rows' terms (and writes the elementwise outputs: the gradient,
// rho_out), leaves the terms in LDS, issues the next chunk's loads, and the CP lanes with ph = 0 add the chunk's terms from
// LDS in row order while those loads are in flight.  The library launches CP = 8, U = 8 (16 chains per workgroup, 512
// workgroups for a tile, a full 128-byte line per row and wavefront): 30 and 33 us for log density + gradient and finish on
// 8,192 x 1,024 against 39 / 39 with CP = 16 and 65 / 62 with CP = 32 (profiles/cache_tiles.md, section 6).
constexpr int RED_WAVES = 4;
constexpr int RED_BLOCK = RED_WAVES * BK_WAVE;

template <int CP, int U, int HINTS>
__global__ __launch_bounds__(RED_BLOCK) void k_gauss_logp_t(const double* th, double* g, double* logp, i64 ld,
                                                            const double* lam, i64 C2, i64 D) {
  constexpr bool NI = (HINTS & NT_IN) != 0, NO = (HINTS & NT_OUT) != 0;
  constexpr int PH = BK_WAVE / CP, R = U * PH;
  __shared__ dvec2 term[RED_WAVES][R][CP];
  __shared__ dvec2 part[RED_WAVES][CP];
  const int lane = threadIdx.x & (BK_WAVE - 1), w = bk_wave_id(), j = lane % CP, ph = lane / CP;
  const i64 c2 = (i64)blockIdx.x * CP + j;
  const bool on = c2 < C2;
  const i64 Dq = (D + RED_WAVES - 1) / RED_WAVES;
  const i64 dlo = w * Dq, dhi = (dlo + Dq < D) ? dlo + Dq : D;
  const double* p = th + 2 * c2;
  double* q = g ? g + 2 * c2 : nullptr;
  dvec2 t[U];
  double l[U];
  auto load = [&](i64 d0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const i64 d = d0 + u * PH + ph;
      if (on && d < dhi) {
        t[u] = gload<NI>(reinterpret_cast<const dvec2*>(p + d * ld));
        l[u] = lam ? lam[d] : 1.0;
      }
    }
  };
  dvec2 s = {0.0, 0.0};
  load(dlo);
  for (i64 r0 = 0; r0 < Dq; r0 += R) {  // (the same trip count in the four wavefronts: there are barriers inside)
    const i64 d0 = dlo + r0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const i64 d = d0 + u * PH + ph;
      if (on && d < dhi) {
        dvec2 lt = t[u];
        if (lam) {
          lt.x = l[u] * t[u].x;
          lt.y = l[u] * t[u].y;
        }
        dvec2 tm;
        tm.x = t[u].x * lt.x;
        tm.y = t[u].y * lt.y;
        term[w][u * PH + ph][j] = tm;
        if (q) {
          dvec2 o = {-lt.x, -lt.y};
          gstore<NO>(o, reinterpret_cast<dvec2*>(q + d * ld));
        }
      }
    }
    load(d0 + R);
    __syncthreads();
    if (ph == 0 && on) {
      const i64 left = dhi - d0;
      const int nr = (int)(left < R ? (left < 0 ? 0 : left) : R);
#pragma unroll 8
      for (int r = 0; r < nr; ++r) {
        const dvec2 tm = term[w][r][j];
        s.x = s.x + tm.x;
        s.y = s.y + tm.y;
      }
    }
    __syncthreads();
  }
  if (ph == 0) part[w][j] = s;
  __syncthreads();
  if (w == 0 && ph == 0 && on) {
    dvec2 tot = part[0][j];
#pragma unroll
    for (int k = 1; k < RED_WAVES; ++k) {
      tot.x = tot.x + part[k][j].x;
      tot.y = tot.y + part[k][j].y;
    }
    tot.x = -0.5 * tot.x;
    tot.y = -0.5 * tot.y;
    *reinterpret_cast<dvec2*>(logp + 2 * c2) = tot;
  }
}

// KV: `metric` is the packed preconditioner {v, sqrt(v), 1/v} (k_finish_v2<KV>)
template <int CP, int U, int HINTS, bool KV>
__global__ __launch_bounds__(RED_BLOCK) void k_finish_t(const double* rho_in, double* rho_out, i64 ld, const double* grad,
                                                        i64 ldg, const double* metric, double half, int negate,
                                                        double* kin_out, i64 C2, i64 D) {
  constexpr bool NI = (HINTS & NT_IN) != 0, NO = (HINTS & NT_OUT) != 0;
  constexpr int PH = BK_WAVE / CP, R = U * PH;
  __shared__ dvec2 term[RED_WAVES][R][CP];
  __shared__ dvec2 part[RED_WAVES][CP];
  const int lane = threadIdx.x & (BK_WAVE - 1), w = bk_wave_id(), j = lane % CP, ph = lane / CP;
  const i64 c2 = (i64)blockIdx.x * CP + j;
  const bool on = c2 < C2;
  const i64 Dq = (D + RED_WAVES - 1) / RED_WAVES;
  const i64 dlo = w * Dq, dhi = (dlo + Dq < D) ? dlo + Dq : D;
  const double* pr = rho_in + 2 * c2;
  const double* pg = grad ? grad + 2 * c2 : nullptr;
  double* qr = rho_out ? rho_out + 2 * c2 : nullptr;
  dvec2 r[U], g[U];
  double m[U], km[U];
  auto load = [&](i64 d0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const i64 d = d0 + u * PH + ph;
      if (on && d < dhi) {
        r[u] = gload<NI>(reinterpret_cast<const dvec2*>(pr + d * ld));
        if (pg) g[u] = gload<NI>(reinterpret_cast<const dvec2*>(pg + d * ldg));
        m[u] = metric ? metric[d] : 1.0;
        km[u] = KV ? metric[2 * D + d] : m[u];
      }
    }
  };
  dvec2 kin = {0.0, 0.0};
  load(dlo);
  for (i64 r0 = 0; r0 < Dq; r0 += R) {  // (the same trip count in the four wavefronts: there are barriers inside)
    const i64 d0 = dlo + r0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const i64 d = d0 + u * PH + ph;
      if (on && d < dhi) {
        dvec2 v = r[u];
        if (pg) {
          const double tx = metric ? m[u] * g[u].x : g[u].x, ty = metric ? m[u] * g[u].y : g[u].y;
          v.x = r[u].x + half * tx;
          v.y = r[u].y + half * ty;
        }
        if (negate) {
          v.x = -v.x;
          v.y = -v.y;
        }
        if (qr) gstore<NO>(v, reinterpret_cast<dvec2*>(qr + d * ld));
        if (kin_out) {
          const double mx = metric ? km[u] * v.x : v.x, my = metric ? km[u] * v.y : v.y;
          dvec2 tm;
          tm.x = v.x * mx;
          tm.y = v.y * my;
          term[w][u * PH + ph][j] = tm;
        }
      }
    }
    load(d0 + R);
    if (!kin_out) continue;  // uniform: no reduction, no barriers
    __syncthreads();
    if (ph == 0 && on) {
      const i64 left = dhi - d0;
      const int nr = (int)(left < R ? (left < 0 ? 0 : left) : R);
#pragma unroll 8
      for (int i = 0; i < nr; ++i) {
        const dvec2 tm = term[w][i][j];
        kin.x = kin.x + tm.x;
        kin.y = kin.y + tm.y;
      }
    }
    __syncthreads();
  }
  if (!kin_out) return;
  if (ph == 0) part[w][j] = kin;
  __syncthreads();
  if (w == 0 && ph == 0 && on) {
    dvec2 s = part[0][j];
#pragma unroll
    for (int k = 1; k < RED_WAVES; ++k) {
      s.x = s.x + part[k][j].x;
      s.y = s.y + part[k][j].y;
    }
    s.x = 0.5 * s.x;
    s.y = 0.5 * s.y;
    *reinterpret_cast<dvec2*>(kin_out + 2 * c2) = s;
  }
}

// ---- the momentum of ONE tile, out of the generator's chain-major scratch ------------------------------------------------
// out[d][c] = lo + scale * zt[c][d] and kin[c] = 1/2 (((q0 + q1) + q2) + q3): k_refresh_apply_kin of bk_rng.hip, operation
// for operation -- lo = loc_in * loc_mul or 0.0, the metric forms (none, diagonal, PD: the packed {v, sqrt(v), 1/v}), each
// quarter of the dimensions summed in increasing d over v * (m * v).  That kernel serves 64 chains per workgroup (a tile of
// 8,192 chains: 128 workgroups on 256 CUs) and a lane adds its chain's terms between its own loads.  Here, as in the two
// reductions above, a workgroup serves CP chain pairs and only the addition is sequential: wavefront w brings the
// [2 CP chains] x [R = U * 64 / CP dims] piece of its quarter in with 2 U independent 8-byte loads per lane (R consecutive
// doubles of a chain's row per group of lanes), turns it through an LDS tile, lane (j, ph) writes rows ph, ph + PH, ... of
// pair j (16 bytes per lane, a full line per row at CP = 8) and leaves the rows' terms IN PLACE of the normals it took; the
// next piece's loads are issued, then the CP lanes with ph = 0 add the terms in row order.
// HINTS: NT_IN = the scratch is read non-temporally, NT_OUT = the momentum (and loc_in's pitch) side is.
// Needs an even chain count and pitch and 16-byte aligned out / loc_in / kin_out (the launch rule of bk_rng.hip); any D, ldz.
template <int CP, int U, int HINTS, bool PD>
__global__ __launch_bounds__(RED_BLOCK) void k_refresh_apply_kin_t(const double* zt, i64 ldz, const double* loc_in,
                                                                   double loc_mul, double scale, double* out, i64 ld,
                                                                   const double* metric, double* kin_out, i64 C2, i64 D) {
  constexpr bool NI = (HINTS & NT_IN) != 0, NO = (HINTS & NT_OUT) != 0;
  constexpr int PH = BK_WAVE / CP, R = U * PH, NC = 2 * CP;
  constexpr int TP = NC + 2;  // doubles per tile row: 16-byte aligned pairs, rows 144 bytes apart at CP = 8 (not 128)
  static_assert((U & (U - 1)) == 0 && (CP & (CP - 1)) == 0 && CP <= BK_WAVE, "powers of two");
  __shared__ __attribute__((aligned(16))) double tile[RED_WAVES][R][TP];
  __shared__ dvec2 part[RED_WAVES][CP];
  const int lane = threadIdx.x & (BK_WAVE - 1), w = bk_wave_id(), j = lane % CP, ph = lane / CP;
  const i64 c2 = (i64)blockIdx.x * CP + j, cb = (i64)blockIdx.x * NC, C = 2 * C2;
  const bool on = c2 < C2;
  const i64 Dq = (D + RED_WAVES - 1) / RED_WAVES;
  const i64 dlo = w * Dq, dhi = (dlo + Dq < D) ? dlo + Dq : D;
  double z[2 * U];
  auto load = [&](i64 d0) {  // element e = i * 64 + lane of the [NC][R] piece: chain e / R, dimension e % R
#pragma unroll
    for (int i = 0; i < 2 * U; ++i) {
      const int e = i * BK_WAVE + lane;
      const i64 cc = cb + e / R, d = d0 + e % R;
      z[i] = (cc < C && d < dhi) ? gload<NI>(zt + cc * ldz + d) : 0.0;
    }
  };
  dvec2 kin = {0.0, 0.0};
  load(dlo);
  for (i64 r0 = 0; r0 < Dq; r0 += R) {  // (the same trip count in the four wavefronts: there are barriers inside)
    const i64 d0 = dlo + r0;
#pragma unroll
    for (int i = 0; i < 2 * U; ++i) {
      const int e = i * BK_WAVE + lane;
      tile[w][e % R][e / R] = z[i];
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int row = u * PH + ph;
      const i64 d = d0 + row;
      if (on && d < dhi) {
        dvec2* cell = reinterpret_cast<dvec2*>(&tile[w][row][2 * j]);
        const dvec2 zz = *cell;
        dvec2 lo = {0.0, 0.0};
        if (loc_in) {
          const dvec2 l = gload<NO>(reinterpret_cast<const dvec2*>(loc_in + d * ld + 2 * c2));
          lo.x = l.x * loc_mul;
          lo.y = l.y * loc_mul;
        }
        const double sc = PD ? metric[D + d] : scale;
        dvec2 v;
        v.x = lo.x + sc * zz.x;
        v.y = lo.y + sc * zz.y;
        gstore<NO>(v, reinterpret_cast<dvec2*>(out + d * ld + 2 * c2));
        const double m = PD ? metric[2 * D + d] : (metric ? metric[d] : 1.0);
        const double mx = (PD || metric) ? m * v.x : v.x, my = (PD || metric) ? m * v.y : v.y;
        dvec2 tm;
        tm.x = v.x * mx;
        tm.y = v.y * my;
        *cell = tm;
      }
    }
    load(d0 + R);
    __syncthreads();
    if (ph == 0 && on) {
      const i64 left = dhi - d0;
      const int nr = (int)(left < R ? (left < 0 ? 0 : left) : R);
#pragma unroll 8
      for (int r = 0; r < nr; ++r) {
        const dvec2 tm = *reinterpret_cast<const dvec2*>(&tile[w][r][2 * j]);
        kin.x = kin.x + tm.x;
        kin.y = kin.y + tm.y;
      }
    }
    __syncthreads();
  }
  if (ph == 0) part[w][j] = kin;
  __syncthreads();
  if (w == 0 && ph == 0 && on) {
    dvec2 s = part[0][j];
#pragma unroll
    for (int k = 1; k < RED_WAVES; ++k) {
      s.x = s.x + part[k][j].x;
      s.y = s.y + part[k][j].y;
    }
    s.x = 0.5 * s.x;
    s.y = 0.5 * s.y;
    *reinterpret_cast<dvec2*>(kin_out + 2 * c2) = s;
  }
}

}  // namespace bkt
