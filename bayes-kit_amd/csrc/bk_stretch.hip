// The stretch move of the affine-invariant ensemble sampler (Goodman & Weare 2010; the commented intent of
// bayes_kit/ensemble.py:47-65): every ACTIVE walker k of a half proposes along the line through a walker j drawn
// from the other half of its own ensemble,
//     j      = other-half base of k's ensemble + min(floor(u_j * H), H - 1)     np.random.choice(other half)
//     r      = 1/sqrt(a) + (sqrt(a) - 1/sqrt(a)) * u_z ;  z = r * r             np.square(uniform(1/sqrt a, sqrt a))
//     theta* = theta_j + z * (theta_k - theta_j)                                 ensemble.py:53 (each operation rounded)
//     zterm  = (D - 1) * log(z)                                                  ensemble.py:54
// The state is [D][ld] with the walker index contiguous; the n active walkers are columns [col_act, col_act + n), their
// ensembles' other halves columns [col_oth, col_oth + n), H walkers per ensemble half (include/bkhip.h).
//
// One lane per active walker (two on the 16-byte form), STRETCH_ROWS rows per workgroup.  The lane's own column and the
// proposal are coalesced; theta_j is an 8-byte gather.  For one row all gathers of a launch fall into ONE segment of
// n * 8 bytes (256 KB at 32,768 walkers per half), so the gather is cheap exactly when the workgroups that share a row
// block share a cache: workgroups are dealt round-robin over the eight XCDs in launch order, and the launch order is
// decoded so that all column blocks of a row block carry the same `launch index % 8` and follow each other there (each
// XCD's L2 then holds a few row blocks' segments instead of every XCD fetching every segment).  The decode changes which
// workgroup does which tile, never what is computed: every tile recomputes j and z from the uniforms (a few flops), only
// row block 0 stores zterm and partner, there are no dependencies between workgroups and no atomics.
//
// The differential-evolution move (ter Braak 2006; bk_de_propose) lives here too: the same tiles, decode and launch forms,
// two gathers per row instead of one.  Active walker k draws an ordered pair (j1, j2), j1 != j2, from the other half of its
// own ensemble and proposes
//     theta* = theta_k + g * (theta_j1 - theta_j2),    g = gamma0 * (1.0 + sigma * z)
// For one row both gathers of a launch fall into the same n * 8 bytes, so the XCD grouping serves them alike.
#include "bk_common.hpp"

namespace {

constexpr int STRETCH_BLOCK = 256;
constexpr int STRETCH_ROWS = 4;  // rows per workgroup: 4 gathers (8 on the 16-byte form) in flight per lane
constexpr int STRETCH_XCDS = 8;

struct StretchLane {
  i64 j;     // partner column
  double z;  // stretch factor
};

__device__ __forceinline__ StretchLane stretch_lane(i64 k, i64 col_oth, i64 H, double uj, double uz, double inv_sqrt_a,
                                                    double sqrt_a) {
  // floor(u * H) of a u in [0, 1); clamped at both ends, so that ANY input value gives a column of the other half
  i64 i = (i64)(uj * (double)H);
  i = i > H - 1 ? H - 1 : i;
  i = i < 0 ? 0 : i;
  const double r = inv_sqrt_a + (sqrt_a - inv_sqrt_a) * uz;
  return {col_oth + (k / H) * H + i, r * r};
}

// (row block, column block) of this workgroup; false for the padding of the decoded grid
__device__ __forceinline__ bool stretch_tile(i64 ncb, i64 nrb, i64& cb, i64& rb) {
  const i64 b = (i64)blockIdx.y * gridDim.x + blockIdx.x;
  if (nrb < STRETCH_XCDS) {  // too few row blocks to give every XCD one: launch order as it is
    cb = b % ncb;
    rb = b / ncb;
    return rb < nrb;
  }
  const i64 q = b / STRETCH_XCDS;
  cb = q % ncb;
  rb = (q / ncb) * STRETCH_XCDS + b % STRETCH_XCDS;
  return rb < nrb;
}

__global__ __launch_bounds__(STRETCH_BLOCK) void k_stretch(const double* __restrict__ theta, i64 ld, i64 col_act,
                                                           i64 col_oth, i64 n, i64 H, const double* __restrict__ u_j,
                                                           const double* __restrict__ u_z, double inv_sqrt_a,
                                                           double sqrt_a, double* __restrict__ prop, i64 ldp,
                                                           double* __restrict__ zterm, int32_t* __restrict__ partner,
                                                           i64 D, i64 ncb, i64 nrb) {
  i64 cb, rb;
  if (!stretch_tile(ncb, nrb, cb, rb)) return;
  const i64 k = cb * STRETCH_BLOCK + threadIdx.x;
  if (k >= n) return;
  const StretchLane w = stretch_lane(k, col_oth, H, u_j[k], u_z[k], inv_sqrt_a, sqrt_a);
  if (rb == 0) {
    zterm[k] = (double)(D - 1) * log(w.z);
    partner[k] = (int32_t)w.j;
  }
  const i64 d0 = rb * STRETCH_ROWS;
  const double* own = theta + col_act + k;
  double tk[STRETCH_ROWS], tj[STRETCH_ROWS];
#pragma unroll
  for (int u = 0; u < STRETCH_ROWS; ++u)
    if (d0 + u < D) {
      tk[u] = own[(d0 + u) * ld];
      tj[u] = theta[(d0 + u) * ld + w.j];
    }
#pragma unroll
  for (int u = 0; u < STRETCH_ROWS; ++u)
    if (d0 + u < D) prop[(d0 + u) * ldp + k] = tj[u] + w.z * (tk[u] - tj[u]);
}

// two adjacent walkers per lane: n, ld, ldp even, theta + col_act and prop 16-byte aligned
__global__ __launch_bounds__(STRETCH_BLOCK) void k_stretch_v2(const double* __restrict__ theta, i64 ld, i64 col_act,
                                                              i64 col_oth, i64 n2, i64 H,
                                                              const double* __restrict__ u_j,
                                                              const double* __restrict__ u_z, double inv_sqrt_a,
                                                              double sqrt_a, double* __restrict__ prop, i64 ldp,
                                                              double* __restrict__ zterm,
                                                              int32_t* __restrict__ partner, i64 D, i64 ncb, i64 nrb) {
  i64 cb, rb;
  if (!stretch_tile(ncb, nrb, cb, rb)) return;
  const i64 p = cb * STRETCH_BLOCK + threadIdx.x;
  if (p >= n2) return;
  const i64 k = 2 * p;
  const StretchLane w0 = stretch_lane(k, col_oth, H, u_j[k], u_z[k], inv_sqrt_a, sqrt_a);
  const StretchLane w1 = stretch_lane(k + 1, col_oth, H, u_j[k + 1], u_z[k + 1], inv_sqrt_a, sqrt_a);
  if (rb == 0) {
    zterm[k] = (double)(D - 1) * log(w0.z);
    zterm[k + 1] = (double)(D - 1) * log(w1.z);
    partner[k] = (int32_t)w0.j;
    partner[k + 1] = (int32_t)w1.j;
  }
  const i64 d0 = rb * STRETCH_ROWS;
  const double* own = theta + col_act + k;
  double2 tk[STRETCH_ROWS];
  double tj0[STRETCH_ROWS], tj1[STRETCH_ROWS];
#pragma unroll
  for (int u = 0; u < STRETCH_ROWS; ++u)
    if (d0 + u < D) {
      tk[u] = *reinterpret_cast<const double2*>(own + (d0 + u) * ld);
      tj0[u] = theta[(d0 + u) * ld + w0.j];
      tj1[u] = theta[(d0 + u) * ld + w1.j];
    }
#pragma unroll
  for (int u = 0; u < STRETCH_ROWS; ++u)
    if (d0 + u < D) {
      double2 o;
      o.x = tj0[u] + w0.z * (tk[u].x - tj0[u]);
      o.y = tj1[u] + w1.z * (tk[u].y - tj1[u]);
      *reinterpret_cast<double2*>(prop + (d0 + u) * ldp + k) = o;
    }
}

struct DeLane {
  i64 j1, j2;  // the partner pair's columns, never equal
  double g;    // the step along their difference
};

__device__ __forceinline__ DeLane de_lane(i64 k, i64 col_oth, i64 H, double u1, double u2, double z, double gamma0,
                                          double sigma) {
  // floor(u_1 * H) and floor(u_2 * (H - 1)), each clamped at both ends, then i2 steps over i1: uniform over the ordered
  // pairs for u in [0, 1), and for ANY input values two different columns of the other half (H >= 2)
  i64 i1 = (i64)(u1 * (double)H);
  i1 = i1 > H - 1 ? H - 1 : i1;
  i1 = i1 < 0 ? 0 : i1;
  i64 i2 = (i64)(u2 * (double)(H - 1));
  i2 = i2 > H - 2 ? H - 2 : i2;
  i2 = i2 < 0 ? 0 : i2;
  i2 += i2 >= i1 ? 1 : 0;
  const i64 base = col_oth + (k / H) * H;
  return {base + i1, base + i2, gamma0 * (1.0 + sigma * z)};
}

__global__ __launch_bounds__(STRETCH_BLOCK) void k_de(const double* __restrict__ theta, i64 ld, i64 col_act, i64 col_oth,
                                                      i64 n, i64 H, const double* __restrict__ u_1,
                                                      const double* __restrict__ u_2, const double* __restrict__ z,
                                                      double gamma0, double sigma, double* __restrict__ prop, i64 ldp,
                                                      int32_t* __restrict__ partner1, int32_t* __restrict__ partner2,
                                                      double* __restrict__ gamma, i64 D, i64 ncb, i64 nrb) {
  i64 cb, rb;
  if (!stretch_tile(ncb, nrb, cb, rb)) return;
  const i64 k = cb * STRETCH_BLOCK + threadIdx.x;
  if (k >= n) return;
  const DeLane w = de_lane(k, col_oth, H, u_1[k], u_2[k], z[k], gamma0, sigma);
  if (rb == 0) {
    partner1[k] = (int32_t)w.j1;
    partner2[k] = (int32_t)w.j2;
    gamma[k] = w.g;
  }
  const i64 d0 = rb * STRETCH_ROWS;
  const double* own = theta + col_act + k;
  double tk[STRETCH_ROWS], ta[STRETCH_ROWS], tb[STRETCH_ROWS];
#pragma unroll
  for (int u = 0; u < STRETCH_ROWS; ++u)
    if (d0 + u < D) {
      tk[u] = own[(d0 + u) * ld];
      ta[u] = theta[(d0 + u) * ld + w.j1];
      tb[u] = theta[(d0 + u) * ld + w.j2];
    }
#pragma unroll
  for (int u = 0; u < STRETCH_ROWS; ++u)
    if (d0 + u < D) prop[(d0 + u) * ldp + k] = tk[u] + w.g * (ta[u] - tb[u]);
}

// two adjacent walkers per lane: n, ld, ldp even, theta + col_act and prop 16-byte aligned
__global__ __launch_bounds__(STRETCH_BLOCK) void k_de_v2(const double* __restrict__ theta, i64 ld, i64 col_act,
                                                         i64 col_oth, i64 n2, i64 H, const double* __restrict__ u_1,
                                                         const double* __restrict__ u_2, const double* __restrict__ z,
                                                         double gamma0, double sigma, double* __restrict__ prop, i64 ldp,
                                                         int32_t* __restrict__ partner1, int32_t* __restrict__ partner2,
                                                         double* __restrict__ gamma, i64 D, i64 ncb, i64 nrb) {
  i64 cb, rb;
  if (!stretch_tile(ncb, nrb, cb, rb)) return;
  const i64 p = cb * STRETCH_BLOCK + threadIdx.x;
  if (p >= n2) return;
  const i64 k = 2 * p;
  const DeLane w0 = de_lane(k, col_oth, H, u_1[k], u_2[k], z[k], gamma0, sigma);
  const DeLane w1 = de_lane(k + 1, col_oth, H, u_1[k + 1], u_2[k + 1], z[k + 1], gamma0, sigma);
  if (rb == 0) {
    partner1[k] = (int32_t)w0.j1;
    partner1[k + 1] = (int32_t)w1.j1;
    partner2[k] = (int32_t)w0.j2;
    partner2[k + 1] = (int32_t)w1.j2;
    gamma[k] = w0.g;
    gamma[k + 1] = w1.g;
  }
  const i64 d0 = rb * STRETCH_ROWS;
  const double* own = theta + col_act + k;
  double2 tk[STRETCH_ROWS];
  double ta0[STRETCH_ROWS], tb0[STRETCH_ROWS], ta1[STRETCH_ROWS], tb1[STRETCH_ROWS];
#pragma unroll
  for (int u = 0; u < STRETCH_ROWS; ++u)
    if (d0 + u < D) {
      const double* row = theta + (d0 + u) * ld;
      tk[u] = *reinterpret_cast<const double2*>(own + (d0 + u) * ld);
      ta0[u] = row[w0.j1];
      tb0[u] = row[w0.j2];
      ta1[u] = row[w1.j1];
      tb1[u] = row[w1.j2];
    }
#pragma unroll
  for (int u = 0; u < STRETCH_ROWS; ++u)
    if (d0 + u < D) {
      double2 o;
      o.x = tk[u].x + w0.g * (ta0[u] - tb0[u]);
      o.y = tk[u].y + w1.g * (ta1[u] - tb1[u]);
      *reinterpret_cast<double2*>(prop + (d0 + u) * ldp + k) = o;
    }
}

}  // namespace

extern "C" {

int bk_stretch_propose(const double* theta, int64_t ld, int64_t col_act, int64_t col_oth, int64_t n, int64_t H,
                       const double* u_j, const double* u_z, double inv_sqrt_a, double sqrt_a, double* theta_prop,
                       int64_t ldp, double* zterm, int32_t* partner, int64_t D, void* stream) {
  if (!theta || !u_j || !u_z || !theta_prop || !zterm || !partner) return BK_E_ARG;
  if (n < 0 || D < 0 || col_act < 0 || col_oth < 0 || H < 1 || n % H != 0) return BK_E_ARG;
  const i64 columns = (col_act > col_oth ? col_act : col_oth) + n;
  if (ld < columns || ldp < n || columns > (i64)INT32_MAX) return BK_E_ARG;
  if (n == 0 || D == 0) return BK_OK;
  const bool vec = n % 2 == 0 && ld % 2 == 0 && ldp % 2 == 0 && bk_aligned16(theta + col_act) && bk_aligned16(theta_prop);
  const i64 ncb = bk_cdiv(vec ? n / 2 : n, STRETCH_BLOCK);
  const i64 nrb = bk_cdiv(D, STRETCH_ROWS);
  // the grid the decode of stretch_tile covers: ncb x (nrb rounded up to whole groups of eight row blocks)
  const i64 rows_y = nrb < STRETCH_XCDS ? nrb : bk_cdiv(nrb, STRETCH_XCDS) * STRETCH_XCDS;
  if (ncb > (i64)INT32_MAX || rows_y > 65535) return BK_E_ARG;
  dim3 grid((unsigned)ncb, (unsigned)rows_y);
  hipStream_t s = bk_stream(stream);
  if (vec)
    k_stretch_v2<<<grid, dim3(STRETCH_BLOCK), 0, s>>>(theta, ld, col_act, col_oth, n / 2, H, u_j, u_z, inv_sqrt_a, sqrt_a,
                                                      theta_prop, ldp, zterm, partner, D, ncb, nrb);
  else
    k_stretch<<<grid, dim3(STRETCH_BLOCK), 0, s>>>(theta, ld, col_act, col_oth, n, H, u_j, u_z, inv_sqrt_a, sqrt_a,
                                                   theta_prop, ldp, zterm, partner, D, ncb, nrb);
  BK_RETURN_LAUNCH_STATUS();
}

int bk_de_propose(const double* theta, int64_t ld, int64_t col_act, int64_t col_oth, int64_t n, int64_t H,
                  const double* u_1, const double* u_2, const double* z, double gamma0, double sigma, double* theta_prop,
                  int64_t ldp, int32_t* partner1, int32_t* partner2, double* gamma, int64_t D, void* stream) {
  if (!theta || !u_1 || !u_2 || !z || !theta_prop || !partner1 || !partner2 || !gamma) return BK_E_ARG;
  if (n < 0 || D < 0 || col_act < 0 || col_oth < 0 || H < 2 || n % H != 0) return BK_E_ARG;
  const i64 columns = (col_act > col_oth ? col_act : col_oth) + n;
  if (ld < columns || ldp < n || columns > (i64)INT32_MAX) return BK_E_ARG;
  if (n == 0 || D == 0) return BK_OK;
  const bool vec = n % 2 == 0 && ld % 2 == 0 && ldp % 2 == 0 && bk_aligned16(theta + col_act) && bk_aligned16(theta_prop);
  const i64 ncb = bk_cdiv(vec ? n / 2 : n, STRETCH_BLOCK);
  const i64 nrb = bk_cdiv(D, STRETCH_ROWS);
  const i64 rows_y = nrb < STRETCH_XCDS ? nrb : bk_cdiv(nrb, STRETCH_XCDS) * STRETCH_XCDS;  // (as bk_stretch_propose)
  if (ncb > (i64)INT32_MAX || rows_y > 65535) return BK_E_ARG;
  dim3 grid((unsigned)ncb, (unsigned)rows_y);
  hipStream_t s = bk_stream(stream);
  if (vec)
    k_de_v2<<<grid, dim3(STRETCH_BLOCK), 0, s>>>(theta, ld, col_act, col_oth, n / 2, H, u_1, u_2, z, gamma0, sigma,
                                                 theta_prop, ldp, partner1, partner2, gamma, D, ncb, nrb);
  else
    k_de<<<grid, dim3(STRETCH_BLOCK), 0, s>>>(theta, ld, col_act, col_oth, n, H, u_1, u_2, z, gamma0, sigma, theta_prop,
                                              ldp, partner1, partner2, gamma, D, ncb, nrb);
  BK_RETURN_LAUNCH_STATUS();
}

}  // extern "C"
