// Multi-chain effective sample size: the cross-chain estimator of Vehtari, Gelman, Simpson, Carpenter and Buerkner
// (2021), "Rank-normalization, folding, and localization: an improved R-hat for assessing convergence of MCMC",
// Bayesian Analysis 16(2), sec. 3.2, eqs. 10-11 (Stan's compute_effective_sample_size, posterior's ess_rfun), with
// Geyer's initial monotone sequence.  The device computes the moments of the split chains and the cross-chain lag sums
// Gamma_t = sum_m gamma_{m,t}; the Geyer scan over Gamma runs on the host (diagnostics._geyer_tau).
//
// Split set: column c of an [N, C] series x[t*ld + c] gives two chains, rows [0, n) and rows [N - n, N), n = N / 2 (the
// middle row of an odd N is dropped).  Chain m = h * C + c, h = half.  With `indicator` set, every draw is read as
// (x <= q) ? 1 : 0 (tail ESS: the chains of the quantile's indicator), nothing is materialised.
//
// Every sum over chains ends in per-workgroup partials part[k * B + b] that ONE workgroup per k sums in a fixed shape
// (k_sum_rows): repeated calls are bit-identical.
#include "bk_common.hpp"
#include "bk_ess_tile.hpp"

namespace {

using bke::ess_fold;
using bke::wave_sum;

constexpr int EM_BLOCK = 256, EM_WAVES = EM_BLOCK / BK_WAVE;
// register tiles from this half length on (the layout of k_ess_tile in bk_diag.hip: 9 draws per lane, 64 lag accumulators)
constexpr int EM_RT_MIN = 288, EM_RT_TAIL = 72;

__device__ __forceinline__ double em_value(double v, int indicator, double q) {
  return indicator ? (v <= q ? 1.0 : 0.0) : v;
}

// sum of the four wavefronts' values in a fixed order (red: [EM_WAVES][BK_WAVE])
__device__ __forceinline__ double em_waves_sum(const double* red, int lane) {
  return ((red[lane] + red[BK_WAVE + lane]) + red[2 * BK_WAVE + lane]) + red[3 * BK_WAVE + lane];
}

// out[k] = sum_b part[k * B + b]: thread t sums b = t, t + 256, ... in order, then a fixed tree
__global__ __launch_bounds__(EM_BLOCK) void k_sum_rows(const double* part, i64 B, double* out) {
  __shared__ double red[EM_WAVES];
  const int lane = threadIdx.x & (BK_WAVE - 1), w = bk_wave_id();
  const double* row = part + (i64)blockIdx.x * B;
  double s = 0.0;
  for (i64 b = threadIdx.x; b < B; b += EM_BLOCK) s = s + row[b];
  s = wave_sum(s);
  if (lane == 0) red[w] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// Per split chain: mean and gamma_{m,0} = (1/n) sum (x - mean)^2 (two passes, as k_chain_mean_var: lane = chain, wavefront
// w sums the draws w, w + 4, ... with eight loads in flight), written to chain_mean / chain_g0 [2C]; per workgroup
// part[0 * B + b] = sum of the means, part[1 * B + b] = sum of gamma_{m,0}, part[2 * B + b] = number of non-finite
// draws (the raw values, also in indicator mode).  Grid (cdiv(C, 64), 2 halves), B = 2 * gridDim.x.
__global__ __launch_bounds__(EM_BLOCK) void k_split_moments(const double* x, i64 ld, i64 N, i64 n, i64 C,
                                                            int indicator, double q, double* chain_mean,
                                                            double* chain_g0, double* part) {
  __shared__ double red[EM_WAVES * BK_WAVE], bad_red[EM_WAVES * BK_WAVE];
  const int lane = threadIdx.x & (BK_WAVE - 1), w = bk_wave_id(), h = blockIdx.y;
  const i64 c = (i64)blockIdx.x * BK_WAVE + lane;
  const bool ok = c < C;
  const double* xc = x + (h ? (N - n) * ld : 0) + (ok ? c : 0);
  double s = 0.0, bad = 0.0;
  for (i64 t0 = w; t0 < n; t0 += 8 * EM_WAVES) {
    double v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = (ok && t0 + EM_WAVES * k < n) ? xc[(t0 + EM_WAVES * k) * ld] : 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const bool in = ok && t0 + EM_WAVES * k < n;
      bad = bad + ((in && !isfinite(v[k])) ? 1.0 : 0.0);
      s = s + (in ? em_value(v[k], indicator, q) : 0.0);
    }
  }
  red[w * BK_WAVE + lane] = s;
  bad_red[w * BK_WAVE + lane] = bad;
  __syncthreads();
  const double mu = em_waves_sum(red, lane) / (double)n;
  __syncthreads();
  double sq = 0.0;
  for (i64 t0 = w; t0 < n; t0 += 8 * EM_WAVES) {
    double v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = (ok && t0 + EM_WAVES * k < n) ? xc[(t0 + EM_WAVES * k) * ld] : 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const double d = (ok && t0 + EM_WAVES * k < n) ? em_value(v[k], indicator, q) - mu : 0.0;
      sq = sq + d * d;
    }
  }
  red[w * BK_WAVE + lane] = sq;
  __syncthreads();
  if (w == 0) {
    const double g0 = em_waves_sum(red, lane) / (double)n;
    if (ok) {
      chain_mean[h * C + c] = mu;
      chain_g0[h * C + c] = g0;
    }
    const double sm = wave_sum(ok ? mu : 0.0), sg = wave_sum(ok ? g0 : 0.0), sb = wave_sum(em_waves_sum(bad_red, lane));
    if (lane == 0) {
      const i64 B = 2 * (i64)gridDim.x, b = (i64)h * gridDim.x + blockIdx.x;
      part[0 * B + b] = sm;
      part[1 * B + b] = sg;
      part[2 * B + b] = sb;
    }
  }
}

// part[b] = sum over the chains of workgroup b of (chain_mean[m] - centre[0])^2: the second pass of np.var(means, ddof=1)
// around the centre gathered over all ranks
__global__ __launch_bounds__(EM_BLOCK) void k_between_sq(const double* chain_mean, i64 M, const double* centre,
                                                         double* part) {
  __shared__ double red[EM_WAVES];
  const int lane = threadIdx.x & (BK_WAVE - 1), w = bk_wave_id();
  const i64 m = (i64)blockIdx.x * EM_BLOCK + threadIdx.x;
  const double d = m < M ? chain_mean[m] - centre[0] : 0.0;
  const double s = wave_sum(d * d);
  if (lane == 0) red[w] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// sum_t xc[t] * xc[t + n0 + lane] over t for a chain centred in LDS (length N, followed by >= EM_RT_TAIL zeros when RT):
// the lag block of k_ess_tile, lanes whose lag is >= N give 0.  RT: lane l owns the draws tc + 9 l + b of every chunk of
// 576 and keeps 64 accumulators, one per lag; a butterfly of 63 exchanges leaves lag n0 + l in lane l.
template <bool RT>
__device__ __forceinline__ double em_lag_block(const double* xc, i64 N, i64 n0, int lane) {
  const i64 nl = n0 + lane;
  const i64 tmax = N - n0;  // lane 0's term count; lane l stops l terms earlier
  double a = 0.0;
  if (RT) {
    double acc[64];
#pragma unroll
    for (int j = 0; j < 64; ++j) acc[j] = 0.0;
    for (i64 tc = 0; tc < tmax; tc += 9 * BK_WAVE) {
      const i64 t0 = tc + 9 * lane, ty = t0 + n0;
      const double* px = xc + (t0 < N ? t0 : N);  // (from N on: zeros)
      const double* py = xc + (ty < N ? ty : N);
      double X[9], win[16];
#pragma unroll
      for (int b = 0; b < 9; ++b) X[b] = px[b];
#pragma unroll
      for (int m = 0; m < 12; ++m) win[m] = py[m];
#pragma unroll
      for (int j = 0; j < 64; ++j) {
        if (j + 12 < EM_RT_TAIL) win[(j + 12) & 15] = py[j + 12];
#pragma unroll
        for (int b = 0; b < 9; ++b) acc[j] = __builtin_fma(X[b], win[(j + b) & 15], acc[j]);
      }
    }
    ess_fold<32>(acc, lane);
    ess_fold<16>(acc, lane);
    ess_fold<8>(acc, lane);
    ess_fold<4>(acc, lane);
    ess_fold<2>(acc, lane);
    ess_fold<1>(acc, lane);
    a = acc[0];
  } else {
    const i64 tsafe = tmax - (BK_WAVE - 1);  // tt + n0 + 63 < N  for tt < tsafe
    i64 tt = 0;
    for (; tt + 8 <= tsafe; tt += 8) {
      double u[8], v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        u[k] = xc[tt + k];
        v[k] = xc[tt + k + nl];
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) a = a + u[k] * v[k];
    }
    for (; tt < tmax; ++tt) {
      const i64 j = tt + nl;
      if (j < N) a = a + xc[tt] * xc[j];
    }
  }
  return nl < N ? a : 0.0;
}

// Cross-chain lag sums part[(t - lag0) * B + b] = sum over the workgroup's chains of gamma_{m,t}, t in [lag0, lag0 + nlags).
// A workgroup stages G chains of one half in LDS once (chain-major, odd pitch, centred by chain_mean, zero tail) and then
// loops over every requested 64-lag block while they stay there; lane l serves the lag n0 + l.  G >= 4: wavefront w serves
// the chains w, w + 4, ... in order.  G < 4 (long halves): the wavefronts that would have no chain take further lag
// blocks instead -- wavefront w serves chain w % G of the block w / G of each pass of 4 / G blocks.
// Grid (cdiv(C, G), 2 halves), B = 2 * gridDim.x.
template <int G, bool RT>
__global__ __launch_bounds__(EM_BLOCK) void k_lag_sums(const double* x, i64 ld, i64 N, i64 n, i64 C, int indicator,
                                                       double q, const double* chain_mean, int pitch, i64 lag0,
                                                       i64 nlags, double* part) {
  extern __shared__ __attribute__((aligned(16))) double xs[];  // [G][pitch], then [EM_WAVES][64] for the wave sums
  double* red = xs + (i64)G * pitch;
  const int t = threadIdx.x, lane = t & (BK_WAVE - 1), w = bk_wave_id(), h = blockIdx.y;
  const i64 c0 = (i64)blockIdx.x * G;
  {
    const int cl = t % G, r0 = t / G;
    constexpr int RS = EM_BLOCK / G;
    const bool ok = c0 + cl < C;
    const double mu = ok ? chain_mean[h * C + c0 + cl] : 0.0;
    const double* xh = x + (h ? (N - n) * ld : 0) + (ok ? c0 + cl : 0);
    for (i64 r = r0; r < n; r += RS) xs[cl * pitch + r] = ok ? em_value(xh[r * ld], indicator, q) - mu : 0.0;
    for (i64 r = n + r0; r < pitch; r += RS) xs[cl * pitch + r] = 0.0;  // (the zeros behind the series)
  }
  __syncthreads();
  const i64 B = 2 * (i64)gridDim.x, b = (i64)h * gridDim.x + blockIdx.x;
  const double inv_n = 1.0 / (double)n;
  constexpr int GW = G < EM_WAVES ? G : EM_WAVES;  // wavefronts per lag block
  constexpr int LB = EM_WAVES / GW;                 // lag blocks per pass
  const int jb = w / GW;
  const i64 lag_end = lag0 + nlags;
  for (i64 nb = lag0; nb < lag_end; nb += (i64)LB * BK_WAVE) {
    const i64 n0 = nb + (i64)jb * BK_WAVE;
    double s = 0.0;
    if (n0 < lag_end)  // (wave-uniform)
      for (int cl = w % GW; cl < G; cl += GW) {
        if (c0 + cl >= C) break;  // wave-uniform
        s = s + em_lag_block<RT>(xs + cl * pitch, n, n0, lane) * inv_n;
      }
    red[w * BK_WAVE + lane] = s;
    __syncthreads();
    if (w == 0)
#pragma unroll
      for (int j = 0; j < LB; ++j) {
        const i64 lag = nb + (i64)j * BK_WAVE + lane;
        double tot = red[(j * GW) * BK_WAVE + lane];
#pragma unroll
        for (int g = 1; g < GW; ++g) tot = tot + red[(j * GW + g) * BK_WAVE + lane];
        if (lag < lag_end) part[(lag - lag0) * B + b] = tot;
      }
    __syncthreads();
  }
}

// part[(t - lag0) * B + b] = sum over the 256 chains of workgroup b of chain_g0[c] * acor[t * ldo + c]: autocovariance from
// an autocorrelation (bk_autocorr_fft).  A chain with gamma_0 = 0 (constant) contributes 0: its 0/0 autocorrelation never
// reaches the sum.  Grid (cdiv(C, 256), <= 65535 lag strides), B = gridDim.x.
__global__ __launch_bounds__(EM_BLOCK) void k_acov_sums(const double* acor, i64 ldo, i64 C, const double* chain_g0,
                                                        i64 lag0, i64 nlags, double* part) {
  __shared__ double red[EM_WAVES];
  const int lane = threadIdx.x & (BK_WAVE - 1), w = bk_wave_id();
  const i64 c = (i64)blockIdx.x * EM_BLOCK + threadIdx.x;
  const double g0 = c < C ? chain_g0[c] : 0.0;
  for (i64 k = blockIdx.y; k < nlags; k += gridDim.y) {
    const double v = wave_sum(g0 != 0.0 ? acor[(lag0 + k) * ldo + c] * g0 : 0.0);
    if (lane == 0) red[w] = v;
    __syncthreads();
    if (threadIdx.x == 0) part[k * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
  }
}

// out[t * ldo + c] = (x[t * ld + c] <= q) ? 1 : 0 (the indicator chains, for the FFT route only)
__global__ __launch_bounds__(EM_BLOCK) void k_indicator(const double* x, i64 ld, i64 n, i64 C, double q, double* out,
                                                        i64 ldo) {
  const i64 c = (i64)blockIdx.x * EM_BLOCK + threadIdx.x;
  if (c >= C) return;
  for (i64 t = blockIdx.y; t < n; t += gridDim.y) out[t * ldo + c] = x[t * ld + c] <= q ? 1.0 : 0.0;
}

// out[j] = values[i] for the element i whose rank equals targets[j] (exact double compare of 1-based ranks); elements whose
// rank is not a target leave out alone.  Every rank is held by one element over all ranks of a process group.
__global__ __launch_bounds__(EM_BLOCK) void k_select_ranks(const double* rank, const double* values, i64 n,
                                                           const double* targets, int k, double* out) {
  const i64 i = (i64)blockIdx.x * EM_BLOCK + threadIdx.x;
  if (i >= n) return;
  const double r = rank[i];
  for (int j = 0; j < k; ++j)
    if (r == targets[j]) out[j] = values[i];
}

struct LagPlan {
  int G, pitch;
  bool rt;
  size_t bytes;
};

// LDS plan of k_lag_sums for half length n: two workgroups per CU when a tile allows it (as bk_ess), else the widest
// group that fits; G = 0 when even one chain does not fit (the FFT route then serves).
LagPlan lag_plan(i64 n) {
  LagPlan p{0, 0, n >= EM_RT_MIN, 0};
  if (n < 1 || n > 0x3fffffff) return p;
  p.pitch = (int)((p.rt ? n + EM_RT_TAIL : n + 1) | 1);
  const i64 red = EM_WAVES * BK_WAVE;
  const i64 cap = (i64)(160 * 1024 - 512) / 8 - red, cap2 = (i64)(78 * 1024) / 8 - red;
  for (int g : {16, 8, 4, 2, 1})
    if ((i64)g * p.pitch <= cap2) { p.G = g; break; }
  if (!p.G)
    for (int g : {16, 8, 4, 2, 1})
      if ((i64)g * p.pitch <= cap) { p.G = g; break; }
  p.bytes = ((size_t)p.G * p.pitch + red) * 8;
  return p;
}

i64 lag_blocks(i64 C, int G) { return 2 * bk_cdiv(C, G); }

// Lags per k_lag_sums launch: the partials ([lags][2 cdiv(C, G)] doubles) stay within EM_PART_BYTES, whatever the half
// length and chain count; a longer request is served by several launches, each staging the chains again.
constexpr i64 EM_PART_BYTES = (i64)256 << 20;
i64 lag_chunk(i64 C, int G, i64 nlags) {
  const i64 cap = EM_PART_BYTES / 8 / lag_blocks(C, G) / BK_WAVE * BK_WAVE;
  const i64 c = cap > BK_WAVE ? cap : BK_WAVE;
  return nlags < c ? nlags : c;
}

}  // namespace

extern "C" {

int64_t bk_ess_multi_work_bytes(int64_t n, int64_t C, int64_t nlags) {
  if (n < 1 || C < 0 || nlags < 0) return -1;
  const LagPlan p = lag_plan(n);
  i64 B = 2 * bk_cdiv(C, BK_WAVE) * 3;                                   // moments
  B = B > bk_cdiv(2 * C, EM_BLOCK) ? B : bk_cdiv(2 * C, EM_BLOCK);       // between-chain pass
  const i64 bl = p.G ? lag_blocks(C, p.G) * lag_chunk(C, p.G, nlags) : bk_cdiv(C, EM_BLOCK) * nlags;  // lag sums
  B = B > bl ? B : bl;
  return 8 * (B > 1 ? B : 1);
}

int64_t bk_ess_lag_sums_max_half(void) {
  i64 lo = 1, hi = 0x3fffffff;
  if (!lag_plan(lo).G) return 0;
  while (lo < hi) {  // (the largest n whose one-chain tile fits)
    const i64 mid = lo + (hi - lo + 1) / 2;
    if (lag_plan(mid).G) lo = mid; else hi = mid - 1;
  }
  return lo;
}

int bk_ess_split_moments(const double* x, int64_t ld, int64_t N, int64_t C, int indicator, double q, double* chain_mean,
                         double* chain_g0, double* out, void* work, int64_t work_bytes, void* stream) {
  const i64 n = N / 2;
  if (!x || !chain_mean || !chain_g0 || !out || !work || n < 1 || C < 1) return BK_E_ARG;
  if (ld < C) return BK_E_ALIGN;
  const i64 gx = bk_cdiv(C, BK_WAVE);
  if (work_bytes < 8 * 3 * 2 * gx || gx > 0x7fffffff) return BK_E_ARG;
  hipStream_t s = bk_stream(stream);
  double* part = static_cast<double*>(work);
  k_split_moments<<<dim3((unsigned)gx, 2), dim3(EM_BLOCK), 0, s>>>(x, ld, N, n, C, indicator, q, chain_mean, chain_g0,
                                                                   part);
  k_sum_rows<<<dim3(3), dim3(EM_BLOCK), 0, s>>>(part, 2 * gx, out);
  BK_RETURN_LAUNCH_STATUS();
}

int bk_ess_between_sq(const double* chain_mean, int64_t M, const double* centre, double* out, void* work,
                      int64_t work_bytes, void* stream) {
  if (!chain_mean || !centre || !out || !work || M < 1) return BK_E_ARG;
  const i64 gx = bk_cdiv(M, EM_BLOCK);
  if (work_bytes < 8 * gx || gx > 0x7fffffff) return BK_E_ARG;
  hipStream_t s = bk_stream(stream);
  double* part = static_cast<double*>(work);
  k_between_sq<<<dim3((unsigned)gx), dim3(EM_BLOCK), 0, s>>>(chain_mean, M, centre, part);
  k_sum_rows<<<dim3(1), dim3(EM_BLOCK), 0, s>>>(part, gx, out);
  BK_RETURN_LAUNCH_STATUS();
}

int bk_ess_lag_sums(const double* x, int64_t ld, int64_t N, int64_t C, int indicator, double q, const double* chain_mean,
                    int64_t lag0, int64_t nlags, double* out, void* work, int64_t work_bytes, void* stream) {
  const i64 n = N / 2;
  if (!x || !chain_mean || !out || !work || n < 1 || C < 1 || lag0 < 0 || nlags < 1 || lag0 + nlags > n) return BK_E_ARG;
  if (ld < C) return BK_E_ALIGN;
  const LagPlan p = lag_plan(n);
  if (!p.G) return BK_E_ARG;  // (longer halves: bk_autocorr_fft + bk_ess_acov_sums)
  const i64 gx = bk_cdiv(C, p.G), B = 2 * gx, chunk = lag_chunk(C, p.G, nlags);
  if (work_bytes < 8 * B * chunk || gx > 0x7fffffff || nlags > 0x7fffffff) return BK_E_ARG;
  hipStream_t s = bk_stream(stream);
  double* part = static_cast<double*>(work);
  dim3 grid((unsigned)gx, 2), block(EM_BLOCK);
#define BK_EM(GG)                                                                                                       \
  do {                                                                                                                  \
    const void* fn = p.rt ? reinterpret_cast<const void*>(&k_lag_sums<GG, true>)                                        \
                          : reinterpret_cast<const void*>(&k_lag_sums<GG, false>);                                      \
    if (p.bytes > 64 * 1024) {                                                                                          \
      hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.bytes);                 \
      if (e != hipSuccess) return (int)e;                                                                               \
    }                                                                                                                   \
    if (p.rt)                                                                                                           \
      k_lag_sums<GG, true><<<grid, block, p.bytes, s>>>(x, ld, N, n, C, indicator, q, chain_mean, p.pitch, l0, nl, part); \
    else                                                                                                                \
      k_lag_sums<GG, false><<<grid, block, p.bytes, s>>>(x, ld, N, n, C, indicator, q, chain_mean, p.pitch, l0, nl,     \
                                                         part);                                                         \
  } while (0)
  for (i64 l = 0; l < nlags; l += chunk) {
    const i64 l0 = lag0 + l, nl = nlags - l < chunk ? nlags - l : chunk;
    switch (p.G) {
      case 16: BK_EM(16); break;
      case 8: BK_EM(8); break;
      case 4: BK_EM(4); break;
      case 2: BK_EM(2); break;
      default: BK_EM(1); break;
    }
    k_sum_rows<<<dim3((unsigned)nl), dim3(EM_BLOCK), 0, s>>>(part, B, out + l);
  }
#undef BK_EM
  BK_RETURN_LAUNCH_STATUS();
}

int bk_ess_acov_sums(const double* acor, int64_t ldo, int64_t n, int64_t C, const double* chain_g0, int64_t lag0,
                     int64_t nlags, double* out, void* work, int64_t work_bytes, void* stream) {
  if (!acor || !chain_g0 || !out || !work || n < 1 || C < 1 || lag0 < 0 || nlags < 1 || lag0 + nlags > n) return BK_E_ARG;
  if (ldo < C) return BK_E_ALIGN;
  const i64 gx = bk_cdiv(C, EM_BLOCK);
  if (work_bytes < 8 * gx * nlags || gx > 0x7fffffff || nlags > 0x7fffffff) return BK_E_ARG;
  hipStream_t s = bk_stream(stream);
  double* part = static_cast<double*>(work);
  k_acov_sums<<<dim3((unsigned)gx, (unsigned)(nlags < 65535 ? nlags : 65535)), dim3(EM_BLOCK), 0, s>>>(acor, ldo, C,
                                                                                                     chain_g0, lag0,
                                                                                                     nlags, part);
  k_sum_rows<<<dim3((unsigned)nlags), dim3(EM_BLOCK), 0, s>>>(part, gx, out);
  BK_RETURN_LAUNCH_STATUS();
}

int bk_ess_indicator(const double* x, int64_t ld, int64_t n, int64_t C, double q, double* out, int64_t ldo,
                     void* stream) {
  if (!x || !out || n < 1 || C < 1) return BK_E_ARG;
  if (ld < C || ldo < C) return BK_E_ALIGN;
  k_indicator<<<dim3((unsigned)bk_cdiv(C, EM_BLOCK), (unsigned)(n < 4096 ? n : 4096)), dim3(EM_BLOCK), 0,
                bk_stream(stream)>>>(x, ld, n, C, q, out, ldo);
  BK_RETURN_LAUNCH_STATUS();
}

int bk_select_ranks(const double* rank, const double* values, int64_t n, const double* targets, int64_t k, double* out,
                    void* stream) {
  if (!targets || !out || n < 0 || k < 1 || k > 8) return BK_E_ARG;
  if (n == 0) return BK_OK;  // (a rank without chains: its empty arrays may come as null pointers)
  if (!rank || !values) return BK_E_ARG;
  k_select_ranks<<<dim3((unsigned)bk_cdiv(n, EM_BLOCK)), dim3(EM_BLOCK), 0, bk_stream(stream)>>>(rank, values, n, targets,
                                                                                                (int)k, out);
  BK_RETURN_LAUNCH_STATUS();
}

}  // extern "C"
