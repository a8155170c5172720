// Parallel tempering (replica exchange) on the [D][ld] state: the accept test of a tempered target and the swap of two
// rungs' columns (include/bkhip.h: bk_tempered_accept, bk_replica_swap).
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

}  // extern "C"
