// bk_energy_update, bk_divergence_capture: the energy diagnostics of an HMC accept test (EnergyDiagnostics; include/bkhip.h).
//
// bk_energy_update is ONE elementwise pass over the five vectors bk_mh_accept(BK_ACCEPT_HMC) is about to read: the energy
// error h1 - h0 in that kernel's expressions and association, the divergence flag, the selected energy and its per-chain
// running statistics (a Welford step and the sum of squared successive differences).  About 160 bytes per chain; doubles
// are read and written one at a time (the tile-major schedule calls it on column slices that start at any chain), the
// four totals are integer atomics after a wavefront ballot.
//
// bk_divergence_capture keeps the columns of the flagged chains in a fixed store, in call order and by ascending chain:
//   k_div_scan    ONE workgroup: the number of flags of every block of 256 chains, their exclusive prefix into `work`, the
//                 store's fill level as this call found it, and the new fill level
//   k_div_gather  workgroups over (block of 256 chains, block of GATHER_ROWS rows): a chain's position is the fill level +
//                 its block's prefix + its rank inside the block, re-derived from ballots -- no atomic decides an order, so
//                 the store does not depend on the launch geometry or on which workgroup runs first.
// Both are launched whatever the flags say (the host never reads them: a draw with a tracker attached can be captured);
// without a flag every workgroup of the gather returns after one load.
#include "bk_common.hpp"

namespace {

constexpr int EN_THREADS = 256;
constexpr int GATHER_ROWS = 16;

__device__ __forceinline__ bool en_finite(double x) {
  return (__double_as_longlong(x) & 0x7ff0000000000000ll) != 0x7ff0000000000000ll;
}

__global__ __launch_bounds__(EN_THREADS) void k_energy_update(
    const double* __restrict__ lp_cur, const double* __restrict__ a_cur, const double* __restrict__ lp_prop,
    const double* __restrict__ a_prop, const double* __restrict__ log_u, double threshold, double* __restrict__ mean_E,
    double* __restrict__ m2_E, double* __restrict__ last_E, double* __restrict__ ssd, long long* __restrict__ trans,
    long long* __restrict__ cnt, long long* __restrict__ ndiv, uint8_t* __restrict__ div_mask, double* __restrict__ err,
    unsigned long long* __restrict__ totals, i64 C) {
  const i64 c = (i64)blockIdx.x * EN_THREADS + threadIdx.x;
  const bool live = c < C;
  bool divergent = false, nan_err = false, bad_E = false;
  if (live) {
    const double a0 = a_cur ? a_cur[c] : 0.0, a1 = a_prop ? a_prop[c] : 0.0;
    const double h0 = lp_cur[c] - a0, h1 = lp_prop[c] - a1;  // hmc.py:36-38, as k_mh_accept
    const double d = h1 - h0;
    const bool acc = log_u[c] < d;                            // hmc.py:60
    nan_err = d != d;
    divergent = nan_err || d < -threshold;
    err[c] = d;
    div_mask[c] = divergent ? 1 : 0;
    trans[c] = trans[c] + 1;
    if (divergent) ndiv[c] = ndiv[c] + 1;
    const double E = -(acc ? h1 : h0);
    bad_E = !en_finite(E);
    if (!bad_E) {
      const long long n0 = cnt[c], n1 = n0 + 1;
      double mu = mean_E[c], q = m2_E[c];
      const double delta = E - mu;  // the Welford step of bk_welford.hpp
      mu = mu + delta / (double)n1;
      q = q + delta * (E - mu);
      cnt[c] = n1;
      mean_E[c] = mu;
      m2_E[c] = q;
      if (n0 > 0) {
        const double t = E - last_E[c];
        ssd[c] = ssd[c] + t * t;
      }
      last_E[c] = E;
    }
  }
  // wavefront ballots -> at most four integer atomics per 64 chains
  const unsigned long long b_live = __ballot(live), b_div = __ballot(divergent), b_nan = __ballot(nan_err),
                           b_bad = __ballot(bad_E);
  if ((threadIdx.x & (BK_WAVE - 1)) == 0) {
    if (b_live) atomicAdd(&totals[0], (unsigned long long)__popcll(b_live));
    if (b_div) atomicAdd(&totals[1], (unsigned long long)__popcll(b_div));
    if (b_nan) atomicAdd(&totals[2], (unsigned long long)__popcll(b_nan));
    if (b_bad) atomicAdd(&totals[3], (unsigned long long)__popcll(b_bad));
  }
}

// work[b] = flags in the blocks before b (b < nb), work[nb] = flags in all, work[nb + 1] = fill[0] as the call found it;
// then fill = {min(cap, stored + flags), seen + flags}.  One workgroup; per trip wavefront w counts blocks
// [256 * trip + 64 * w, + 64), lane l keeps the count of the l-th of them, and the 256 counts are scanned.
__global__ __launch_bounds__(EN_THREADS) void k_div_scan(const uint8_t* __restrict__ mask, i64 C, i64 nb, i64 cap,
                                                         long long* __restrict__ fill, long long* __restrict__ work) {
  __shared__ long long wave_total[EN_THREADS / BK_WAVE];
  const int tid = (int)threadIdx.x, lane = tid & (BK_WAVE - 1), wave = bk_wave_id();
  long long carry = 0;
  for (i64 b0 = 0; b0 < nb; b0 += EN_THREADS) {
    long long mine = 0;
    for (int j = 0; j < BK_WAVE; ++j) {
      const i64 b = b0 + (i64)wave * BK_WAVE + j;  // wavefront-uniform
      if (b >= nb) break;
      int n = 0;
#pragma unroll
      for (int q = 0; q < EN_THREADS / BK_WAVE; ++q) {
        const i64 c = b * EN_THREADS + q * BK_WAVE + lane;
        const bool f = c < C && mask[c] != 0;
        n += __popcll(__ballot(f));
      }
      if (lane == j) mine = n;
    }
    // inclusive scan of the wavefront's 64 counts, then of the four wavefront totals
    long long inc = mine;
#pragma unroll
    for (int s = 1; s < BK_WAVE; s <<= 1) {
      const long long up = __shfl_up(inc, s);
      if (lane >= s) inc += up;
    }
    if (lane == BK_WAVE - 1) wave_total[wave] = inc;
    __syncthreads();
    long long before = carry, all = carry;
#pragma unroll
    for (int w = 0; w < EN_THREADS / BK_WAVE; ++w) {
      const long long t = wave_total[w];
      if (w < wave) before += t;
      all += t;
    }
    const i64 b = b0 + tid;
    if (b < nb) work[b] = before + (inc - mine);
    carry = all;
    __syncthreads();  // the next trip overwrites wave_total
  }
  if (tid == 0) {
    const long long stored = fill[0];
    work[nb] = carry;
    work[nb + 1] = stored;
    const long long room = cap > stored ? cap - stored : 0;
    fill[0] = stored + (carry < room ? carry : room);
    fill[1] = fill[1] + carry;
  }
}

__global__ __launch_bounds__(EN_THREADS) void k_div_gather(
    const uint8_t* __restrict__ mask, const double* __restrict__ err, const long long* __restrict__ trans,
    const double* __restrict__ theta, i64 ld, i64 C, i64 D, i64 chain0, double* __restrict__ theta_div,
    long long* __restrict__ chain, long long* __restrict__ draw, double* __restrict__ err_store, i64 cap, i64 nb,
    const long long* __restrict__ work) {
  __shared__ int wave_count[EN_THREADS / BK_WAVE];
  const i64 b = (i64)blockIdx.x;
  const long long before = work[b], upto = b + 1 < nb ? work[b + 1] : work[nb], base = work[nb + 1];
  if (upto == before || base + before >= cap) return;  // no flag in this block, or the store is full (workgroup-uniform)
  const int tid = (int)threadIdx.x, lane = tid & (BK_WAVE - 1), wave = bk_wave_id();
  const i64 c = b * EN_THREADS + tid;
  const bool f = c < C && mask[c] != 0;
  const unsigned long long bal = __ballot(f);
  if (lane == 0) wave_count[wave] = __popcll(bal);
  __syncthreads();
  if (!f) return;
  long long pos = base + before + (long long)__popcll(bal & ((1ull << lane) - 1ull));
#pragma unroll
  for (int w = 0; w < EN_THREADS / BK_WAVE; ++w)
    if (w < wave) pos += wave_count[w];
  if (pos >= cap) return;  // counted in `seen`, not stored: the earliest are kept
  const i64 d0 = (i64)blockIdx.y * GATHER_ROWS;
  if (d0 == 0) {
    chain[pos] = chain0 + c;
    draw[pos] = trans[c];
    err_store[pos] = err[c];
  }
  double x[GATHER_ROWS];
#pragma unroll
  for (int i = 0; i < GATHER_ROWS; ++i)
    if (d0 + i < D) x[i] = theta[(d0 + i) * ld + c];
#pragma unroll
  for (int i = 0; i < GATHER_ROWS; ++i)
    if (d0 + i < D) theta_div[(d0 + i) * cap + pos] = x[i];
}

static bool en_threshold_ok(double t) { return t == t && t > 0.0 && t <= 1.7976931348623157e308; }

}  // namespace

extern "C" {

int bk_energy_update(const double* lp_cur, const double* a_cur, const double* lp_prop, const double* a_prop,
                     const double* log_u, double threshold, double* mean_E, double* m2_E, double* last_E, double* ssd,
                     int64_t* trans, int64_t* cnt, int64_t* ndiv, uint8_t* div_mask, double* err, int64_t* totals,
                     int64_t C, void* stream) {
  if (!lp_cur || !lp_prop || !log_u || !mean_E || !m2_E || !last_E || !ssd || !trans || !cnt || !ndiv || !div_mask ||
      !err || !totals || C < 0 || !en_threshold_ok(threshold))
    return BK_E_ARG;
  if (C == 0) return BK_OK;
  const i64 nb = bk_cdiv(C, EN_THREADS);
  if (nb > 2147483647) return BK_E_ARG;
  k_energy_update<<<dim3((unsigned)nb), dim3(EN_THREADS), 0, bk_stream(stream)>>>(
      lp_cur, a_cur, lp_prop, a_prop, log_u, threshold, mean_E, m2_E, last_E, ssd, reinterpret_cast<long long*>(trans),
      reinterpret_cast<long long*>(cnt), reinterpret_cast<long long*>(ndiv), div_mask, err,
      reinterpret_cast<unsigned long long*>(totals), C);
  BK_RETURN_LAUNCH_STATUS();
}

int64_t bk_divergence_capture_work_elems(int64_t C) { return C < 0 ? 0 : bk_cdiv(C, EN_THREADS) + 2; }

int bk_divergence_capture(const uint8_t* div_mask, const double* err, const int64_t* trans, const double* theta,
                          int64_t ld, int64_t C, int64_t D, int64_t chain0, double* theta_div, int64_t* chain,
                          int64_t* draw, double* err_store, int64_t cap, int64_t* fill, int64_t* work, void* stream) {
  if (!div_mask || !fill || !work || C < 0 || D < 0 || cap < 0) return BK_E_ARG;
  const bool store = theta_div != nullptr && cap > 0 && D > 0;
  if (store && (!theta || !err || !trans || !chain || !draw || !err_store || ld < C)) return BK_E_ARG;
  if (C == 0) return BK_OK;
  const i64 nb = bk_cdiv(C, EN_THREADS), rows = bk_cdiv(D, GATHER_ROWS);
  if (nb > 2147483647 || rows > 65535) return BK_E_ARG;
  hipStream_t s = bk_stream(stream);
  k_div_scan<<<dim3(1), dim3(EN_THREADS), 0, s>>>(div_mask, C, nb, store ? cap : 0, reinterpret_cast<long long*>(fill),
                                                  reinterpret_cast<long long*>(work));
  if (store)
    k_div_gather<<<dim3((unsigned)nb, (unsigned)rows), dim3(EN_THREADS), 0, s>>>(
        div_mask, err, reinterpret_cast<const long long*>(trans), theta, ld, C, D, chain0, theta_div,
        reinterpret_cast<long long*>(chain), reinterpret_cast<long long*>(draw), err_store, cap, nb,
        reinterpret_cast<const long long*>(work));
  BK_RETURN_LAUNCH_STATUS();
}

}  // extern "C"
