// Stand-alone measurement behind profiles/cache_tiles.md: shapes of kick+drift (bk_integrator.hip: k_kick_drift_v2) and of
// the Gaussian gradient op (bk_targets.hip: k_gauss_grad_v2) on one Infinity-Cache tile.  A trajectory's worth of launches --
// 64 alternating (kick+drift, gradient) pairs, in place, on columns [0, C) of a [D][ld] state -- timed by HIP events, for
// every pair of the variants listed below; the kernels are copies of the library's with the shape as template arguments
// (the policy mode instantiates the library's own templates of csrc/bk_tile_kernels.hpp).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off tools/cache_tile_bench.hip -o cache_tile_bench
//   cache_tile_bench C D ld              every pair (a tile of a 65,536-chain state: 8192 1024 65536)
//   cache_tile_bench C D ld KD G         one pair, e.g. under rocprofv3 --kernel-trace --stats
//   cache_tile_bench C D ld order        the library's plain pair with each kernel's rows swept ascending or descending: the
//                                        four combinations, then the first again (profiles/cache_tiles.md section 7)
//   cache_tile_bench C D ld order KD G   one of them (0 ascending, 1 descending), e.g. under rocprofv3 --pmc FETCH_SIZE
//   cache_tile_bench C D ld policy       the library's plain pair (gradient rows descending) with a cache policy per ACCESS
//                                        (csrc/bk_mem_policy.hpp): the candidates of POLICY[] below, the all-plain pair first
//                                        and again last; every candidate starts from the same state and prints a checksum of
//                                        what it leaves, which must be the same in every line (section 8)
//   cache_tile_bench C D ld policy KD G  candidate KD's kick+drift with candidate G's gradient kernel, e.g. under rocprofv3
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "../bayes-kit_amd/csrc/bk_tile_kernels.hpp"  // k_kick_drift_tile, k_gauss_grad_tile (+ bk_mem_policy.hpp): policy mode

typedef int64_t i64;
typedef double dvec2 __attribute__((ext_vector_type(2)));

#define CHECK(x)                                                                  \
  do {                                                                            \
    hipError_t e_ = (x);                                                          \
    if (e_ != hipSuccess) {                                                       \
      fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_));   \
      exit(2);                                                                    \
    }                                                                             \
  } while (0)

__device__ __forceinline__ double kd_elem(double th, double rho, double g, double m, bool has_m, double eps, int use_pre,
                                          double pre, int use_kick, double kick, double& rho_new) {
  double t = has_m ? m * g : g;
  double r = rho;
  if (use_pre) r = r + pre * t;
  if (use_kick) r = r + kick * t;
  rho_new = r;
  return th + eps * r;
}

template <int ROWS, int NT>
__device__ __forceinline__ void kd_unit(i64 c2, i64 d0, const double* th_in, double* th_out, const double* rho_in,
                                        double* rho_out, i64 ld, const double* grad, i64 ldg, const double* metric,
                                        double eps, int use_pre, double pre, int use_kick, double kick, i64 C2, i64 D) {
  if (c2 >= C2) return;
  dvec2 t[ROWS], r[ROWS], g[ROWS];
  double m[ROWS];
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {
    i64 d = d0 + i;
    if (d < D) {
      const dvec2* pt = reinterpret_cast<const dvec2*>(th_in + d * ld + 2 * c2);
      const dvec2* pr = reinterpret_cast<const dvec2*>(rho_in + d * ld + 2 * c2);
      const dvec2* pg = reinterpret_cast<const dvec2*>(grad + d * ldg + 2 * c2);
      if (NT & 1) {
        t[i] = __builtin_nontemporal_load(pt);
        r[i] = __builtin_nontemporal_load(pr);
        g[i] = __builtin_nontemporal_load(pg);
      } else {
        t[i] = *pt;
        r[i] = *pr;
        g[i] = *pg;
      }
      m[i] = metric ? metric[d] : 1.0;
    }
  }
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {
    i64 d = d0 + i;
    if (d < D) {
      dvec2 rn, tn;
      double rx, ry;
      tn.x = kd_elem(t[i].x, r[i].x, g[i].x, m[i], metric != nullptr, eps, use_pre, pre, use_kick, kick, rx);
      tn.y = kd_elem(t[i].y, r[i].y, g[i].y, m[i], metric != nullptr, eps, use_pre, pre, use_kick, kick, ry);
      rn.x = rx;
      rn.y = ry;
      dvec2* qr = reinterpret_cast<dvec2*>(rho_out + d * ld + 2 * c2);
      dvec2* qt = reinterpret_cast<dvec2*>(th_out + d * ld + 2 * c2);
      if (NT & 2) {
        __builtin_nontemporal_store(rn, qr);
        __builtin_nontemporal_store(tn, qt);
      } else {
        *qr = rn;
        *qt = tn;
      }
    }
  }
}

// PERSIST: grid of gridDim.x workgroups walks the (chain block, row group) units in launch order
// DESC: the row groups from the last to the first in launch order (the block-to-row map only)
template <int ROWS, int NT, int BLOCK, bool PERSIST, bool DESC = false>
__global__ __launch_bounds__(BLOCK) void k_kd(const double* th_in, double* th_out, const double* rho_in, double* rho_out,
                                              i64 ld, const double* grad, i64 ldg, const double* metric, double eps,
                                              int use_pre, double pre, int use_kick, double kick, i64 C2, i64 D) {
  if (PERSIST) {
    const i64 nx = (C2 + BLOCK - 1) / BLOCK, ny = (D + ROWS - 1) / ROWS;
    for (i64 u = blockIdx.x; u < nx * ny; u += gridDim.x)
      kd_unit<ROWS, NT>((u % nx) * BLOCK + threadIdx.x, (DESC ? ny - 1 - u / nx : u / nx) * ROWS, th_in, th_out, rho_in,
                        rho_out, ld, grad, ldg, metric, eps, use_pre, pre, use_kick, kick, C2, D);
  } else {
    const i64 y = DESC ? (i64)gridDim.y - 1 - blockIdx.y : (i64)blockIdx.y;
    kd_unit<ROWS, NT>((i64)blockIdx.x * BLOCK + threadIdx.x, y * ROWS, th_in, th_out, rho_in, rho_out, ld, grad, ldg, metric,
                      eps, use_pre, pre, use_kick, kick, C2, D);
  }
}

template <int ROWS, int NT>
__device__ __forceinline__ void g_unit(i64 c2, i64 d0, const double* th, double* g, i64 ld, const double* lam, i64 C2,
                                       i64 D) {
  if (c2 >= C2) return;
  dvec2 t[ROWS];
  double l[ROWS];
#pragma unroll
  for (int i = 0; i < ROWS; ++i)
    if (d0 + i < D) {
      const dvec2* p = reinterpret_cast<const dvec2*>(th + (d0 + i) * ld + 2 * c2);
      t[i] = (NT & 1) ? __builtin_nontemporal_load(p) : *p;
      l[i] = lam ? lam[d0 + i] : 1.0;
    }
#pragma unroll
  for (int i = 0; i < ROWS; ++i)
    if (d0 + i < D) {
      dvec2 o;
      o.x = lam ? -(l[i] * t[i].x) : -t[i].x;
      o.y = lam ? -(l[i] * t[i].y) : -t[i].y;
      dvec2* q = reinterpret_cast<dvec2*>(g + (d0 + i) * ld + 2 * c2);
      if (NT & 2) __builtin_nontemporal_store(o, q);
      else *q = o;
    }
}

template <int ROWS, int NT, int BLOCK, bool PERSIST, bool DESC = false>
__global__ __launch_bounds__(BLOCK) void k_g(const double* th, double* g, i64 ld, const double* lam, i64 C2, i64 D) {
  if (PERSIST) {
    const i64 nx = (C2 + BLOCK - 1) / BLOCK, ny = (D + ROWS - 1) / ROWS;
    for (i64 u = blockIdx.x; u < nx * ny; u += gridDim.x)
      g_unit<ROWS, NT>((u % nx) * BLOCK + threadIdx.x, (DESC ? ny - 1 - u / nx : u / nx) * ROWS, th, g, ld, lam, C2, D);
  } else {
    const i64 y = DESC ? (i64)gridDim.y - 1 - blockIdx.y : (i64)blockIdx.y;
    g_unit<ROWS, NT>((i64)blockIdx.x * BLOCK + threadIdx.x, y * ROWS, th, g, ld, lam, C2, D);
  }
}

struct Args {
  double *th, *rho, *g, *lam;
  i64 ld, C, D;
  hipStream_t s;
};

static i64 cdiv(i64 a, i64 b) { return (a + b - 1) / b; }
constexpr int PGRID = 256 * 8;  // persistent: 8 workgroups per CU

template <int ROWS, int NT, int BLOCK, bool PERSIST, bool DESC = false>
static void launch_kd(const Args& a) {
  dim3 grid = PERSIST ? dim3(PGRID) : dim3((unsigned)cdiv(a.C / 2, BLOCK), (unsigned)cdiv(a.D, ROWS));
  k_kd<ROWS, NT, BLOCK, PERSIST, DESC><<<grid, dim3(BLOCK), 0, a.s>>>(a.th, a.th, a.rho, a.rho, a.ld, a.g, a.ld, nullptr, 0.01, 0,
                                                                 0.0, 1, 0.01, a.C / 2, a.D);
}
template <int ROWS, int NT, int BLOCK, bool PERSIST, bool DESC = false>
static void launch_g(const Args& a) {
  dim3 grid = PERSIST ? dim3(PGRID) : dim3((unsigned)cdiv(a.C / 2, BLOCK), (unsigned)cdiv(a.D, ROWS));
  k_g<ROWS, NT, BLOCK, PERSIST, DESC><<<grid, dim3(BLOCK), 0, a.s>>>(a.th, a.g, a.ld, a.lam, a.C / 2, a.D);
}

struct Variant {
  const char* name;
  void (*fn)(const Args&);
};

#define V(f, R, N, B, P) {#f "<" #R "," #N "," #B "," #P ">", &f<R, N, B, P>}
// <rows per thread, non-temporal: 1 loads | 2 stores, threads per workgroup, persistent grid>
static const Variant KD[] = {
    V(launch_kd, 2, 3, 256, false),  // 0: the streaming variant (what the library launched at this shape before)
    V(launch_kd, 1, 0, 256, false),  // 1: the library's plain variant
    V(launch_kd, 1, 1, 256, false),  V(launch_kd, 1, 2, 256, false),  V(launch_kd, 2, 2, 256, false),
    V(launch_kd, 2, 0, 256, false),  V(launch_kd, 4, 0, 256, false),  V(launch_kd, 1, 0, 512, false),
    V(launch_kd, 2, 0, 512, false),  V(launch_kd, 1, 0, 1024, false), V(launch_kd, 2, 0, 1024, false),
    V(launch_kd, 1, 0, 256, true),   V(launch_kd, 2, 0, 256, true),   V(launch_kd, 4, 0, 256, true),
    V(launch_kd, 2, 0, 512, true),   V(launch_kd, 2, 3, 256, true),
};
static const Variant G[] = {
    V(launch_g, 2, 0, 256, false),  // 0: the library's plain variant before
    V(launch_g, 1, 3, 256, false),  // 1: the library's streaming variant
    V(launch_g, 1, 2, 256, false),  V(launch_g, 1, 1, 256, false), V(launch_g, 2, 2, 256, false),
    V(launch_g, 2, 3, 256, false),  V(launch_g, 1, 0, 256, false),  // 6: the library's plain variant now
    V(launch_g, 4, 2, 256, false),  V(launch_g, 4, 0, 256, false), V(launch_g, 2, 0, 512, false),
    V(launch_g, 2, 0, 1024, false), V(launch_g, 2, 0, 256, true),  V(launch_g, 4, 0, 256, true),
    V(launch_g, 2, 0, 512, true),
};
constexpr int NKD = sizeof(KD) / sizeof(KD[0]), NG = sizeof(G) / sizeof(G[0]);
// the library's plain pair (KD[1], G[6]) by row order: [0] ascending, [1] descending
static const Variant KD_ORDER[2] = {{"kd ascending", &launch_kd<1, 0, 256, false, false>},
                                    {"kd descending", &launch_kd<1, 0, 256, false, true>}};
static const Variant G_ORDER[2] = {{"g ascending", &launch_g<1, 0, 256, false, false>},
                                   {"g descending", &launch_g<1, 0, 256, false, true>}};

// ---- a cache policy per access: the library's templates (bk_tile_kernels.hpp), kick+drift ascending, the gradient descending
template <int PT, int PR, int PG, int ST, int SR>
static void launch_kd_pol(const Args& a) {
  bkt::k_kick_drift_tile<PT, PR, PG, ST, SR><<<dim3((unsigned)cdiv(a.C / 2, 256), (unsigned)a.D), dim3(256), 0, a.s>>>(
      a.th, a.rho, a.ld, a.g, a.ld, nullptr, 0.01, 0, 0.0, 1, 0.01, a.C / 2, a.D);
}
template <int PT, int SG>
static void launch_g_pol(const Args& a) {
  bkt::k_gauss_grad_tile<PT, SG><<<dim3((unsigned)cdiv(a.C / 2, 256), (unsigned)a.D), dim3(256), 0, a.s>>>(a.th, a.g, a.ld, a.lam,
                                                                                                       a.C / 2, a.D);
}

struct PolicyPair {
  const char* name;
  void (*kd)(const Args&);
  void (*g)(const Args&);
};
constexpr int P_ = bkm::PLAIN, N_ = bkm::NT, S1 = bkm::SC1, S01 = bkm::SC0_SC1, S01N = bkm::SC0_SC1_NT;
// kick+drift <theta load, rho load, g load, theta store, rho store> + gradient <theta load, g store>
#define PP(name, a, b, c, d, e, f, g) {name, &launch_kd_pol<a, b, c, d, e>, &launch_g_pol<f, g>}
static const PolicyPair POLICY[] = {
    PP("0 all plain", P_, P_, P_, P_, P_, P_, P_),
    PP("1 g load nt", P_, P_, N_, P_, P_, P_, P_),
    PP("2 rho load+store nt", P_, N_, P_, P_, N_, P_, P_),
    PP("3 g load, rho load+store nt", P_, N_, N_, P_, N_, P_, P_),
    PP("4 g load sc1", P_, P_, S1, P_, P_, P_, P_),
    PP("5 rho load+store sc1", P_, S1, P_, P_, S1, P_, P_),
    PP("6 g load, rho load+store sc1", P_, S1, S1, P_, S1, P_, P_),
    PP("7 g load sc0sc1", P_, P_, S01, P_, P_, P_, P_),
    PP("8 rho load+store sc0sc1", P_, S01, P_, P_, S01, P_, P_),
    PP("9 g load, rho load+store sc0sc1", P_, S01, S01, P_, S01, P_, P_),
    PP("10a all stores sc1", P_, P_, P_, S1, S1, P_, S1),
    PP("10b all stores sc0sc1", P_, P_, P_, S01, S01, P_, S01),
    PP("11a 1 + theta, rho, g stores sc1", P_, P_, N_, S1, S1, P_, S1),
    PP("11b 2 + theta, g stores sc1", P_, N_, P_, S1, N_, P_, S1),
    PP("11c 3 + theta, g stores sc1", P_, N_, N_, S1, N_, P_, S1),
    PP("11d 3 + g store sc1", P_, N_, N_, P_, N_, P_, S1),
    PP("11e 6 + theta, g stores sc1", P_, S1, S1, S1, S1, P_, S1),
    PP("11f g load nt, rho load nt, rho store sc1", P_, N_, N_, P_, S1, P_, P_),
    PP("12 theta load nt (control)", N_, P_, P_, P_, P_, P_, P_),
    PP("13 g load sc0sc1nt", P_, P_, S01N, P_, P_, P_, P_),
    PP("14 rho load+store sc0sc1nt", P_, S01N, P_, P_, S01N, P_, P_),
    PP("15 g load, rho load+store sc0sc1nt", P_, S01N, S01N, P_, S01N, P_, P_),
    PP("16 rho store only nt", P_, P_, P_, P_, N_, P_, P_),
    PP("17 rho store only sc1", P_, P_, P_, P_, S1, P_, P_),
    PP("18 g store sc1", P_, P_, P_, P_, P_, P_, S1),
    PP("19 g store nt", P_, P_, P_, P_, P_, P_, N_),
    PP("20 11d, rho store sc1", P_, N_, N_, P_, S1, P_, S1),
    PP("21 g load nt + g store sc1", P_, P_, N_, P_, P_, P_, S1),
    PP("22 2 + g store sc1", P_, N_, P_, P_, N_, P_, S1),
    PP("23 11d, g load sc1", P_, N_, S1, P_, N_, P_, S1),
    PP("24 11d, g store sc0sc1", P_, N_, N_, P_, N_, P_, S01),
    PP("25 11d, every nt as sc0sc1nt", P_, S01N, S01N, P_, S01N, P_, S01),
    PP("26 11d, rho load plain", P_, P_, N_, P_, N_, P_, S1),
    PP("27 11d, g store sc0sc1nt", P_, N_, N_, P_, N_, P_, S01N),
    PP("28 11d, rho load+store sc1", P_, S1, N_, P_, S1, P_, S1),
    PP("30 kick+drift of 28, gradient plain", P_, S1, N_, P_, S1, P_, P_),
    PP("31 rho load nt, rho store sc1", P_, N_, P_, P_, S1, P_, P_),
    PP("32 31 + g store sc1", P_, N_, P_, P_, S1, P_, S1),
    PP("33 5 + g store sc1", P_, S1, P_, P_, S1, P_, S1),
    PP("0 all plain (again)", P_, P_, P_, P_, P_, P_, P_),
};
#undef PP
constexpr int NPOL = sizeof(POLICY) / sizeof(POLICY[0]);

__global__ void k_fill(double* p, i64 n, double v) {
  for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) p[i] = v + 1e-9 * (double)(i & 1023);
}

constexpr int L = 64;

// one trajectory's worth of launches, `reps` times after one warm-up trajectory: out = {median, min, max} ms per trajectory
static void run_pair(const Args& a, const Variant& kd, const Variant& g, int reps, double out[3]) {
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  std::vector<float> tot;
  for (int r = 0; r < reps + 1; ++r) {
    CHECK(hipEventRecord(e0, a.s));
    for (int n = 0; n < L; ++n) {
      kd.fn(a);
      g.fn(a);
    }
    CHECK(hipEventRecord(e1, a.s));
    CHECK(hipEventSynchronize(e1));
    CHECK(hipGetLastError());
    float ms;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    if (r) tot.push_back(ms);
  }
  std::sort(tot.begin(), tot.end());
  out[0] = tot[tot.size() / 2];
  out[1] = tot.front();
  out[2] = tot.back();
  CHECK(hipEventDestroy(e0));
  CHECK(hipEventDestroy(e1));
}

int main(int argc, char** argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: cache_tile_bench C D ld [kd g | order [kd g] | policy [kd g]]\n");
    return 1;
  }
  Args a;
  a.C = atoll(argv[1]);
  a.D = atoll(argv[2]);
  a.ld = atoll(argv[3]);
  if (a.C % 2 || a.ld % 2 || a.ld < a.C || a.C <= 0 || a.D <= 0) return 1;
  CHECK(hipStreamCreate(&a.s));
  const i64 n = a.D * a.ld, n_total = n;
  CHECK(hipMalloc(&a.th, n * 8));
  CHECK(hipMalloc(&a.rho, n * 8));
  CHECK(hipMalloc(&a.g, n * 8));
  CHECK(hipMalloc(&a.lam, a.D * 8));
  k_fill<<<1024, 256, 0, a.s>>>(a.th, n, 0.5);
  k_fill<<<1024, 256, 0, a.s>>>(a.rho, n, 0.25);
  k_fill<<<1024, 256, 0, a.s>>>(a.g, n, 0.125);
  k_fill<<<4, 256, 0, a.s>>>(a.lam, a.D, 1.0);
  CHECK(hipStreamSynchronize(a.s));
  const double bytes = (double)L * 56.0 * (double)a.C * (double)a.D;
  double o[3];
  if (argc >= 5 && !strcmp(argv[4], "policy")) {  // a cache policy per access; every candidate from the same state
    const bool one = argc >= 7;
    const int k0 = one ? atoi(argv[5]) : 0, g0 = one ? atoi(argv[6]) : 0;
    if (k0 < 0 || k0 >= NPOL || g0 < 0 || g0 >= NPOL) return 1;
    std::vector<double> h(3 * 2048);
    const i64 nh = std::min<i64>(2048, a.C);
    for (int n = one ? k0 : 0; n < NPOL; n += one ? NPOL : 1) {
      k_fill<<<1024, 256, 0, a.s>>>(a.th, n_total, 0.5);
      k_fill<<<1024, 256, 0, a.s>>>(a.rho, n_total, 0.25);
      k_fill<<<1024, 256, 0, a.s>>>(a.g, n_total, 0.125);
      const Variant kd = {POLICY[n].name, POLICY[n].kd}, g = {POLICY[one ? g0 : n].name, POLICY[one ? g0 : n].g};
      run_pair(a, kd, g, one ? 5 : 7, o);
      // what the candidate left in the first columns of the last row: the same bits for every policy
      const i64 off = (a.D - 1) * a.ld;
      CHECK(hipMemcpy(h.data(), a.th + off, nh * 8, hipMemcpyDeviceToHost));
      CHECK(hipMemcpy(h.data() + 2048, a.rho + off, nh * 8, hipMemcpyDeviceToHost));
      CHECK(hipMemcpy(h.data() + 4096, a.g + off, nh * 8, hipMemcpyDeviceToHost));
      uint64_t sum = 1469598103934665603ull;
      for (int j = 0; j < 3; ++j)
        for (i64 i = 0; i < nh; ++i) {
          uint64_t b;
          memcpy(&b, &h[j * 2048 + i], 8);
          sum = (sum ^ b) * 1099511628211ull;
        }
      printf("POLICY C=%lld D=%lld ld=%lld %-42s median %.2f us/step (min %.2f max %.2f) %.2f TB/s  sum %016llx\n",
             (long long)a.C, (long long)a.D, (long long)a.ld, one ? "(kd of KD, g of G)" : POLICY[n].name, o[0] * 1e3 / L,
             o[1] * 1e3 / L, o[2] * 1e3 / L, bytes / (o[0] * 1e-3) / 1e12, (unsigned long long)sum);
      fflush(stdout);
    }
    return 0;
  }
  if (argc >= 5 && !strcmp(argv[4], "order")) {  // row orders of the library's plain pair, or one of them; the first
    const bool one = argc >= 7;                   // combination again at the end: drift of the box
    if (one && ((atoi(argv[5]) | atoi(argv[6])) & ~1)) return 1;
    for (int n = one ? 2 * atoi(argv[5]) + atoi(argv[6]) : 0; n < 5; n += one ? 5 : 1) {
      const int ik = (n >> 1) & 1, ig = n & 1;
      run_pair(a, KD_ORDER[ik], G_ORDER[ig], one ? 5 : 7, o);
      printf("ORDER C=%lld D=%lld ld=%lld %-13s + %-12s%s median %.1f us/step (min %.1f max %.1f) %.2f TB/s\n", (long long)a.C,
             (long long)a.D, (long long)a.ld, KD_ORDER[ik].name, G_ORDER[ig].name, n == 4 ? " (again)" : "", o[0] * 1e3 / L,
             o[1] * 1e3 / L, o[2] * 1e3 / L, bytes / (o[0] * 1e-3) / 1e12);
    }
    return 0;
  }
  if (argc >= 6) {  // one pair, for a kernel trace
    int ik = atoi(argv[4]), ig = atoi(argv[5]);
    if (ik < 0 || ik >= NKD || ig < 0 || ig >= NG) return 1;
    run_pair(a, KD[ik], G[ig], 5, o);
    printf("PAIR C=%lld D=%lld ld=%lld %s + %s: median %.4f ms per %d steps (min %.4f max %.4f) = %.1f us/step %.2f TB/s\n",
           (long long)a.C, (long long)a.D, (long long)a.ld, KD[ik].name, G[ig].name, o[0], L, o[1], o[2], o[0] * 1e3 / L,
           bytes / (o[0] * 1e-3) / 1e12);
    return 0;
  }
  double best = 1e30;
  int bk = 0, bg = 0;
  for (int ik = 0; ik < NKD; ++ik)
    for (int ig = 0; ig < NG; ++ig) {
      run_pair(a, KD[ik], G[ig], 7, o);
      printf("SWEEP C=%lld ld=%lld kd=%d g=%d %-32s + %-30s median %.1f us/step (min %.1f max %.1f) %.2f TB/s\n",
             (long long)a.C, (long long)a.ld, ik, ig, KD[ik].name, G[ig].name, o[0] * 1e3 / L, o[1] * 1e3 / L,
             o[2] * 1e3 / L, bytes / (o[0] * 1e-3) / 1e12);
      if (o[0] < best) best = o[0], bk = ik, bg = ig;
    }
  // the reference pair again at the end: drift of the box over the sweep
  run_pair(a, KD[0], G[0], 7, o);
  printf("SWEEP C=%lld ld=%lld kd=0 g=0 (again) median %.1f us/step (min %.1f max %.1f)\n", (long long)a.C, (long long)a.ld,
         o[0] * 1e3 / L, o[1] * 1e3 / L, o[2] * 1e3 / L);
  printf("BEST %d %d %.1f us/step\n", bk, bg, best * 1e3 / L);
  return 0;
}
