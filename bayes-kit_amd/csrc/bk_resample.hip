// Ordered resampling for sequential Monte Carlo: systematic and stratified ancestor indices from a FIXED-POINT
// cumulative weight, built by a reduce-then-scan over integers (include/bkhip.h: bk_resample_ordered).
//
// A floating-point scan assembled as carry + local is not monotone at its thread, wavefront and tile seams, and its bits
// depend on the launch geometry.  Here the weights are quantised once,
//     wmax = max_i w_i                      s = 62 - bit_length(n - 1)            (n * 2^s <= 2^62)
//     q_i  = llrint(ldexp(w_i / wmax, s))   one rounded division, an exact scaling, round to nearest even
//     Q_i  = q_0 + .. + q_i                 int64: associative, so every tiling gives the same bits, and non-decreasing
// and every slot position is an exact integer: with Q = Q_{n-1}, a = Q / m, r = Q % m and the global slot J,
//     base_J = J * a + (J * r) / m          = floor(J * Q / m); every product fits in int64
//     o_J    = min(a - 1, (int64) floor(u * (double) a))      u: slot J's uniform (stratified) or ONE for all (systematic)
//     idx_J  = #{ i : Q_i <= base_J + o_J }                   in [0, n - 1], since base_J + o_J < Q
// (a weight that is not > 0 -- zero, negative, NaN -- counts as zero, in the maximum and in q.)
//
// Five launches on one stream; no workgroup ever waits for another workgroup of its own launch (no look-back, no flags,
// no grid barrier): the order between the stages is the stream's.
//   1. k_ro_max     grid-stride maximum, per-block maxima combined by a 64-bit integer atomicMax on the bit pattern
//                   (non-negative doubles order as their bit patterns)
//   2. k_ro_tile    one workgroup per tile of RO_TILE = 2,048 elements (256 threads x 8): q_i, the tile's int64 sum
//   3. k_ro_carry   ONE workgroup scans the tile sums into exclusive carries, RO_CARRY_W = 256 tile sums per pass of
//                   its loop (one per thread), a running total carried from pass to pass
//   4. k_ro_scan    each tile recomputes q_i and scans it: serial inside a thread (8), shuffles across the wavefront,
//                   LDS across the four wavefronts, + the tile's carry; Q_i stored as int64
//   5. k_ro_search  one slot per lane: base_J + o_J, binary search of Q (upper bound), int32 index
// work (16-byte aligned): [0, 8) wmax's bit pattern, [8, 16) unused, [16, 16 + 8 n) Q, then (from the next multiple of
// 16) the tile sums / carries, one int64 per tile.
#include "bk_common.hpp"

namespace {

constexpr int RO_THREADS = 256;
constexpr int RO_PER_THREAD = 8;
constexpr int RO_TILE = RO_THREADS * RO_PER_THREAD;  // 2,048
constexpr int RO_CARRY_W = RO_THREADS;               // tile sums per pass of k_ro_carry's loop
constexpr int RO_WAVES = RO_THREADS / BK_WAVE;
constexpr int RO_MAX_BLOCKS = 1024;

struct RoPlan {
  i64 n_tiles, off_q, off_carry, bytes;
};

inline RoPlan ro_plan(i64 n) {
  RoPlan p;
  p.n_tiles = bk_cdiv(n, RO_TILE);
  p.off_q = 16;
  p.off_carry = 16 + 8 * ((n + 1) & ~(i64)1);
  p.bytes = p.off_carry + 8 * p.n_tiles;
  return p;
}

inline int ro_shift(i64 n) {
  int bits = 0;
  for (i64 v = n - 1; v > 0; v >>= 1) ++bits;  // bit_length(n - 1)
  return 62 - bits;
}

__device__ __forceinline__ double ro_pos(double w) { return w > 0.0 ? w : 0.0; }

__device__ __forceinline__ i64 ro_quant(double w, double wmax, int s) {
  const double r = ro_pos(w) / wmax;  // in [0, 1]; NaN (0 / 0, inf / inf) counts as 0
  return r > 0.0 ? (i64)llrint(ldexp(r, s)) : (i64)0;
}

// the 8 weights of thread `tid` of tile `tile` (zeros past n); 16-byte loads where the tile is whole and w is aligned
template <bool ALIGNED>
__device__ __forceinline__ void ro_load8(const double* w, i64 n, i64 tile, int tid, double (&v)[RO_PER_THREAD]) {
  const i64 b = tile * RO_TILE + (i64)tid * RO_PER_THREAD;
  if (ALIGNED && b + RO_PER_THREAD <= n) {
    const double2* p = reinterpret_cast<const double2*>(w + b);
#pragma unroll
    for (int k = 0; k < RO_PER_THREAD / 2; ++k) {
      const double2 x = p[k];
      v[2 * k] = x.x, v[2 * k + 1] = x.y;
    }
  } else {
#pragma unroll
    for (int k = 0; k < RO_PER_THREAD; ++k) v[k] = b + k < n ? w[b + k] : 0.0;
  }
}

__device__ __forceinline__ i64 ro_wave_sum(i64 x) {
#pragma unroll
  for (int d = 1; d < BK_WAVE; d <<= 1) x += __shfl_xor(x, d);
  return x;
}

// inclusive scan over the wavefront's lanes
__device__ __forceinline__ i64 ro_wave_scan(i64 x, int lane) {
#pragma unroll
  for (int d = 1; d < BK_WAVE; d <<= 1) {
    const i64 y = __shfl_up(x, d);
    if (lane >= d) x += y;
  }
  return x;
}

template <bool ALIGNED>
__global__ __launch_bounds__(RO_THREADS) void k_ro_max(const double* w, i64 n, unsigned long long* wmax_bits) {
  __shared__ double part[RO_WAVES];
  double m = 0.0;
  const i64 t = (i64)blockIdx.x * RO_THREADS + threadIdx.x, stride = (i64)gridDim.x * RO_THREADS;
  if (ALIGNED) {
    const double2* p = reinterpret_cast<const double2*>(w);
    for (i64 i = t; i < n / 2; i += stride) {
      const double2 x = p[i];
      m = fmax(m, fmax(ro_pos(x.x), ro_pos(x.y)));
    }
    if ((n & 1) && t == 0) m = fmax(m, ro_pos(w[n - 1]));
  } else {
    for (i64 i = t; i < n; i += stride) m = fmax(m, ro_pos(w[i]));
  }
#pragma unroll
  for (int d = 1; d < BK_WAVE; d <<= 1) m = fmax(m, __shfl_xor(m, d));
  const int lane = threadIdx.x & (BK_WAVE - 1), wave = threadIdx.x / BK_WAVE;
  if (lane == 0) part[wave] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 1; k < RO_WAVES; ++k) m = fmax(m, part[k]);
    if (m > 0.0) atomicMax(wmax_bits, (unsigned long long)__double_as_longlong(m));
  }
}

template <bool ALIGNED>
__global__ __launch_bounds__(RO_THREADS) void k_ro_tile(const double* w, i64 n, int s, const unsigned long long* wmax_bits,
                                                        i64* tile_sum) {
  __shared__ i64 part[RO_WAVES];
  const double wmax = __longlong_as_double((long long)*wmax_bits);
  double v[RO_PER_THREAD];
  ro_load8<ALIGNED>(w, n, blockIdx.x, threadIdx.x, v);
  i64 sum = 0;
#pragma unroll
  for (int k = 0; k < RO_PER_THREAD; ++k) sum += ro_quant(v[k], wmax, s);
  sum = ro_wave_sum(sum);
  const int lane = threadIdx.x & (BK_WAVE - 1), wave = threadIdx.x / BK_WAVE;
  if (lane == 0) part[wave] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 1; k < RO_WAVES; ++k) sum += part[k];
    tile_sum[blockIdx.x] = sum;
  }
}

// exclusive scan of a value over the workgroup's 256 threads; *total: the sum of all 256 (every thread gets it)
__device__ __forceinline__ i64 ro_block_exclusive(i64 x, i64* part, i64* total) {
  const int lane = threadIdx.x & (BK_WAVE - 1), wave = threadIdx.x / BK_WAVE;
  const i64 inc = ro_wave_scan(x, lane);
  if (lane == BK_WAVE - 1) part[wave] = inc;
  __syncthreads();
  i64 before = 0, all = 0;
#pragma unroll
  for (int k = 0; k < RO_WAVES; ++k) {
    const i64 p = part[k];
    if (k < wave) before += p;
    all += p;
  }
  __syncthreads();  // (part is written again by the caller's next pass)
  *total = all;
  return before + inc - x;
}

// carry[t] <- sum of tile sums 0 .. t-1, in place
__global__ __launch_bounds__(RO_THREADS) void k_ro_carry(i64* carry, i64 n_tiles) {
  __shared__ i64 part[RO_WAVES];
  i64 running = 0;
  for (i64 lo = 0; lo < n_tiles; lo += RO_CARRY_W) {
    const i64 t = lo + threadIdx.x;
    const i64 x = t < n_tiles ? carry[t] : 0;
    i64 total;
    const i64 ex = ro_block_exclusive(x, part, &total);
    if (t < n_tiles) carry[t] = running + ex;
    running += total;
  }
}

template <bool ALIGNED>
__global__ __launch_bounds__(RO_THREADS) void k_ro_scan(const double* w, i64 n, int s, const unsigned long long* wmax_bits,
                                                        const i64* carry, i64* Q) {
  __shared__ i64 part[RO_WAVES];
  const double wmax = __longlong_as_double((long long)*wmax_bits);
  double v[RO_PER_THREAD];
  ro_load8<ALIGNED>(w, n, blockIdx.x, threadIdx.x, v);
  i64 q[RO_PER_THREAD];
  i64 sum = 0;
#pragma unroll
  for (int k = 0; k < RO_PER_THREAD; ++k) {
    sum += ro_quant(v[k], wmax, s);
    q[k] = sum;
  }
  i64 total;
  const i64 off = carry[blockIdx.x] + ro_block_exclusive(sum, part, &total);
  const i64 b = (i64)blockIdx.x * RO_TILE + (i64)threadIdx.x * RO_PER_THREAD;
  if (b + RO_PER_THREAD <= n) {  // (Q starts 16 bytes into the aligned work area, b is a multiple of 8)
    longlong2* p = reinterpret_cast<longlong2*>(Q + b);
#pragma unroll
    for (int k = 0; k < RO_PER_THREAD / 2; ++k) {
      longlong2 x;
      x.x = off + q[2 * k], x.y = off + q[2 * k + 1];
      p[k] = x;
    }
  } else {
#pragma unroll
    for (int k = 0; k < RO_PER_THREAD; ++k)
      if (b + k < n) Q[b + k] = off + q[k];
  }
}

__global__ __launch_bounds__(RO_THREADS) void k_ro_search(const i64* Q, i64 n, const double* u, int systematic, i64 m_local,
                                                          i64 slot0, i64 m_total, int32_t* idx) {
  const i64 j = (i64)blockIdx.x * RO_THREADS + threadIdx.x;
  if (j >= m_local) return;
  const i64 total = Q[n - 1];
  const i64 a = total / m_total, r = total % m_total, J = slot0 + j;
  const double uj = systematic ? u[0] : u[j];
  i64 o = (i64)floor(uj * (double)a);
  if (o > a - 1) o = a - 1;
  const i64 tau = J * a + (J * r) / m_total + o;
  i64 lo = 0, hi = n;  // #{ i : Q_i <= tau }
  while (lo < hi) {
    const i64 mid = (lo + hi) >> 1;
    if (Q[mid] <= tau) lo = mid + 1;
    else hi = mid;
  }
  if (lo > n - 1) lo = n - 1;  // (only for weights outside the contract: tau < Q otherwise)
  idx[j] = (int32_t)lo;
}

}  // namespace

extern "C" {

int64_t bk_resample_ordered_work_bytes(int64_t n) {
  if (n <= 0) return 0;
  if (n > 0x7fffffff) return -1;
  return ro_plan(n).bytes;
}

int bk_resample_ordered(const double* weights, int64_t n, const double* u, int64_t m_local, int64_t slot0, int64_t m_total,
                        int mode, void* work, int64_t work_bytes, int32_t* idx_out, void* stream) {
  if (!weights || !u || !work || !idx_out || n < 1 || n > 0x7fffffff || m_total < 1 || m_total > 0x7fffffff ||
      m_local < 0 || slot0 < 0 || slot0 > m_total - m_local ||
      (mode != BK_RESAMPLE_SYSTEMATIC && mode != BK_RESAMPLE_STRATIFIED))
    return BK_E_ARG;
  const RoPlan p = ro_plan(n);
  if (work_bytes < p.bytes || !bk_aligned16(work)) return BK_E_ARG;
  if (m_local == 0) return BK_OK;
  hipStream_t st = bk_stream(stream);
  char* base = static_cast<char*>(work);
  unsigned long long* wmax_bits = reinterpret_cast<unsigned long long*>(base);
  i64* Q = reinterpret_cast<i64*>(base + p.off_q);
  i64* carry = reinterpret_cast<i64*>(base + p.off_carry);
  const int s = ro_shift(n);
  const hipError_t e = hipMemsetAsync(wmax_bits, 0, 16, st);
  if (e != hipSuccess) return (int)e;
  const dim3 block(RO_THREADS), tiles((unsigned)p.n_tiles);
  const dim3 few((unsigned)(p.n_tiles < RO_MAX_BLOCKS ? p.n_tiles : RO_MAX_BLOCKS));
  if (bk_aligned16(weights)) {
    k_ro_max<true><<<few, block, 0, st>>>(weights, n, wmax_bits);
    k_ro_tile<true><<<tiles, block, 0, st>>>(weights, n, s, wmax_bits, carry);
    k_ro_carry<<<dim3(1), block, 0, st>>>(carry, p.n_tiles);
    k_ro_scan<true><<<tiles, block, 0, st>>>(weights, n, s, wmax_bits, carry, Q);
  } else {
    k_ro_max<false><<<few, block, 0, st>>>(weights, n, wmax_bits);
    k_ro_tile<false><<<tiles, block, 0, st>>>(weights, n, s, wmax_bits, carry);
    k_ro_carry<<<dim3(1), block, 0, st>>>(carry, p.n_tiles);
    k_ro_scan<false><<<tiles, block, 0, st>>>(weights, n, s, wmax_bits, carry, Q);
  }
  k_ro_search<<<dim3((unsigned)bk_cdiv(m_local, RO_THREADS)), block, 0, st>>>(Q, n, u, mode == BK_RESAMPLE_SYSTEMATIC,
                                                                             m_local, slot0, m_total, idx_out);
  BK_RETURN_LAUNCH_STATUS();
}

}  // extern "C"
