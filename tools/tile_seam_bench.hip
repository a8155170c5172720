// Stand-alone measurement behind profiles/cache_tiles.md, sections 6 and 9: the launches at the two ENDS of a tile of the
// tile-major HMC schedule, as the library's own kernel templates (csrc/bk_tile_kernels.hpp) with the candidate shapes and
// access hints.  One visit of a tile = what hmc.py queues, shortened in the middle:
//   the tile's normals written chain-major (a fill stands in for the generator: it leaves the 64 MiB chunk in the cache as the
//   generator does), the momentum refresh out of that chunk into the tile's momentum,
//   first step (full-width theta, gradient, the tile's momentum in place -> the tile's contiguous arrays), a few in-place
//   (gradient, kick+drift) steps,
//   gradient-only launch (the yardstick), log density + gradient, finish, blend into the output state, select into the
//   cached gradient.
// Every launch under test is bracketed by HIP events; a configuration visits the 8 tiles of a 65,536-chain state `reps` times,
// so each launch finds the cache as the previous tile left it.  Prints the median of every bracketed launch per configuration.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off tools/tile_seam_bench.hip -o tile_seam_bench
//   tile_seam_bench [C=65536] [T=8192] [D=1024] [reps=3]
#include "../bayes-kit_amd/csrc/bk_tile_kernels.hpp"

#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

using bkt::dvec2;

#define CHECK(x)                                                                \
  do {                                                                          \
    hipError_t e_ = (x);                                                        \
    if (e_ != hipSuccess) {                                                     \
      fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
      exit(2);                                                                  \
    }                                                                           \
  } while (0)

// the library's gradient-only launch at this shape (bk_targets.hip: k_gauss_grad_v2<1, false>)
__global__ __launch_bounds__(256) void k_grad(const double* th, double* g, i64 ld, const double* lam, i64 C2, i64 D) {
  const i64 c2 = (i64)blockIdx.x * 256 + threadIdx.x, d = blockIdx.y;
  if (c2 >= C2 || d >= D) return;
  const dvec2 t = *reinterpret_cast<const dvec2*>(th + d * ld + 2 * c2);
  const double l = lam[d];
  dvec2 o = {-(l * t.x), -(l * t.y)};
  *reinterpret_cast<dvec2*>(g + d * ld + 2 * c2) = o;
}

// the library's momentum refresh of every other call (bk_rng.hip: k_refresh_apply_kin, no location, no metric, plain): 64
// chains per workgroup -- the yardstick of the tile-rate shapes
__global__ __launch_bounds__(256) void k_refresh64(const double* zt, i64 ldz, double scale, double* out, i64 ld, double* kin_out,
                                                   i64 C, i64 D) {
  __shared__ double tile[4][64][17];
  __shared__ double part[4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x / 64;
  const i64 c0 = (i64)blockIdx.x * 64, c = c0 + lane;
  const i64 Dq = (D + 3) / 4;
  const i64 dlo = w * Dq, dhi = (dlo + Dq < D) ? dlo + Dq : D;
  const int sub = lane >> 4, dl = lane & 15;
  double kin = 0.0;
  for (i64 p0 = 0; p0 < Dq; p0 += 16) {
    const i64 d0 = dlo + p0;
    double z[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      i64 cc = c0 + 4 * i + sub, d = d0 + dl;
      z[i] = (cc < C && d < dhi) ? zt[cc * ldz + d] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) tile[w][4 * i + sub][dl] = z[i];
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      if (c < C && d0 + u < dhi) {
        double v = 0.0 + scale * tile[w][lane][u];
        out[(d0 + u) * ld + c] = v;
        kin = kin + v * v;
      }
    }
    __syncthreads();
  }
  part[w][lane] = kin;
  __syncthreads();
  if (w != 0 || c >= C) return;
  double s = part[0][lane];
  for (int k = 1; k < 4; ++k) s = s + part[k][lane];
  kin_out[c] = 0.5 * s;
}

__global__ void k_fill(double* p, i64 n, double v) {
  for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x)
    p[i] = v + 1e-9 * (double)(i & 1023);
}
__global__ void k_mask(uint8_t* m, i64 n) {  // accepts 4 of 5 chains: every (m0, m1) pair pattern occurs
  for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x)
    m[i] = (uint8_t)(((i * 2654435761u) >> 7) % 5 != 0);
}

struct Args {
  double *th, *rho, *g, *out;  // [D][C]: state, generator's momentum, cached gradient, output state
  double *thp, *rk, *gp;       // [D][T]: the tile's proposal, momentum, trajectory gradient
  double *zt, *kin0;           // [T][D]: the tile's normals, chain-major; [C]: the momentum's kinetic energy
  double *lam, *lp, *kin;
  uint8_t* mask;
  i64 C, T, D, c0;
  hipStream_t s;
};
static i64 cdiv(i64 a, i64 b) { return (a + b - 1) / b; }

template <int H>
static void first_step(const Args& a) {  // the tile's momentum in place (the refresh has just written it)
  dim3 grid((unsigned)cdiv(a.T / 2, 256), (unsigned)a.D);
  bkt::k_kick_drift_ld<H><<<grid, 256, 0, a.s>>>(a.th + a.c0, a.C, a.thp, a.T, a.rk, a.T, a.rk, a.T, a.g + a.c0, a.C,
                                                 nullptr, 0.01, 1, -0.005, 1, 0.01, a.T / 2, a.D);
}
template <int H>
static void first_step_full(const Args& a) {  // the momentum out of a full-width array in HBM: the schedule before section 9
  dim3 grid((unsigned)cdiv(a.T / 2, 256), (unsigned)a.D);
  bkt::k_kick_drift_ld<H><<<grid, 256, 0, a.s>>>(a.th + a.c0, a.C, a.thp, a.T, a.rho + a.c0, a.C, a.rk, a.T, a.g + a.c0, a.C,
                                                 nullptr, 0.01, 1, -0.005, 1, 0.01, a.T / 2, a.D);
}
static void normals(const Args& a) { k_fill<<<1024, 256, 0, a.s>>>(a.zt, a.T * a.D, 0.125); }
template <int CP, int U, int H>
static void refresh(const Args& a) {
  bkt::k_refresh_apply_kin_t<CP, U, H, false><<<(unsigned)cdiv(a.T / 2, CP), 256, 0, a.s>>>(
      a.zt, a.D, nullptr, 0.0, 1.0, a.rk, a.T, nullptr, a.kin0 + a.c0, a.T / 2, a.D);
}
static void refresh64(const Args& a) {
  k_refresh64<<<(unsigned)cdiv(a.T, 64), 256, 0, a.s>>>(a.zt, a.D, 1.0, a.rk, a.T, a.kin0 + a.c0, a.T, a.D);
}
static void step(const Args& a) {
  dim3 grid((unsigned)cdiv(a.T / 2, 256), (unsigned)a.D);
  bkt::k_kick_drift_ld<0><<<grid, 256, 0, a.s>>>(a.thp, a.T, a.thp, a.T, a.rk, a.T, a.rk, a.T, a.gp, a.T, nullptr, 0.01, 0, 0.0,
                                                 1, 0.01, a.T / 2, a.D);
}
static void grad_only(const Args& a) {
  dim3 grid((unsigned)cdiv(a.T / 2, 256), (unsigned)a.D);
  k_grad<<<grid, 256, 0, a.s>>>(a.thp, a.gp, a.T, a.lam, a.T / 2, a.D);
}
template <int CP, int U, int H>
static void logp(const Args& a) {
  bkt::k_gauss_logp_t<CP, U, H><<<(unsigned)cdiv(a.T / 2, CP), 256, 0, a.s>>>(a.thp, a.gp, a.lp + a.c0, a.T, a.lam, a.T / 2, a.D);
}
template <int CP, int U, int H>
static void finish(const Args& a) {
  bkt::k_finish_t<CP, U, H, false><<<(unsigned)cdiv(a.T / 2, CP), 256, 0, a.s>>>(a.rk, nullptr, a.T, a.gp, a.T, nullptr, 0.005,
                                                                             0, a.kin + a.c0, a.T / 2, a.D);
}
template <int H>
static void blend(const Args& a) {
  dim3 grid((unsigned)cdiv(a.T / 2, 256), (unsigned)cdiv(a.D, 2));
  bkt::k_blend_ld<H><<<grid, 256, 0, a.s>>>(a.mask + a.c0, a.th + a.c0, a.C, a.thp, a.T, a.out + a.c0, a.C, a.T / 2, a.D);
}
template <int H>
static void select(const Args& a) {
  dim3 grid((unsigned)cdiv(a.T / 2, 256), (unsigned)cdiv(a.D, 2));
  bkt::k_select_ld<H><<<grid, 256, 0, a.s>>>(a.mask + a.c0, a.g + a.c0, a.C, a.gp, a.T, a.T / 2, a.D);
}

typedef void (*Fn)(const Args&);
struct Cfg {
  const char* name;
  Fn first, logp, finish, blend, select, refresh;
};
constexpr int I = bkt::NT_IN, O = bkt::NT_OUT, B = bkt::NT_TILE, P = bkt::RHO_PLAIN;
#define BASE_FIRST first_step<I>
#define BASE_REF refresh<8, 8, 0>
#define BASE_LOGP logp<8, 8, 0>
#define BASE_FIN finish<8, 8, 0>
#define BASE_BLEND blend<I | O>
#define BASE_SEL select<I | O>
// <chain pairs per wavefront, loads in flight per lane, hints>
static const Cfg CFG[] = {
    {"base (what the library launches): first nt-in | logp <8,8> plain | finish <8,8> plain | blend, select nt full-width, plain tile",
     BASE_FIRST, BASE_LOGP, BASE_FIN, BASE_BLEND, BASE_SEL, BASE_REF},
    {"first plain", first_step<0>, BASE_LOGP, BASE_FIN, BASE_BLEND, BASE_SEL, BASE_REF},
    {"first nt-in nt-out", first_step<I | O>, BASE_LOGP, BASE_FIN, BASE_BLEND, BASE_SEL, BASE_REF},
    {"logp, finish <4,8>", BASE_FIRST, logp<4, 8, 0>, finish<4, 8, 0>, BASE_BLEND, BASE_SEL, BASE_REF},
    {"logp, finish <8,4>", BASE_FIRST, logp<8, 4, 0>, finish<8, 4, 0>, BASE_BLEND, BASE_SEL, BASE_REF},
    {"logp, finish <8,16>", BASE_FIRST, logp<8, 16, 0>, finish<8, 16, 0>, BASE_BLEND, BASE_SEL, BASE_REF},
    {"logp, finish <16,8>", BASE_FIRST, logp<16, 8, 0>, finish<16, 8, 0>, BASE_BLEND, BASE_SEL, BASE_REF},
    {"logp, finish <16,16>", BASE_FIRST, logp<16, 16, 0>, finish<16, 16, 0>, BASE_BLEND, BASE_SEL, BASE_REF},
    {"logp, finish <32,8>", BASE_FIRST, logp<32, 8, 0>, finish<32, 8, 0>, BASE_BLEND, BASE_SEL, BASE_REF},
    {"logp <8,8> nt stores | finish <8,8> nt loads", BASE_FIRST, logp<8, 8, O>, finish<8, 8, I>, BASE_BLEND, BASE_SEL, BASE_REF},
    {"blend, select all nt", BASE_FIRST, BASE_LOGP, BASE_FIN, blend<I | O | B>, select<I | O | B>, BASE_REF},
    {"blend, select all plain", BASE_FIRST, BASE_LOGP, BASE_FIN, blend<0>, select<0>, BASE_REF},
    // section 9: the momentum refresh <chain pairs per wavefront, rows in flight per lane, hints> and the first step behind it
    {"refresh as every other call launches it (64 chains per workgroup)", BASE_FIRST, BASE_LOGP, BASE_FIN, BASE_BLEND, BASE_SEL,
     refresh64},
    {"refresh <4,8>", BASE_FIRST, BASE_LOGP, BASE_FIN, BASE_BLEND, BASE_SEL, refresh<4, 8, 0>},
    {"refresh <8,4>", BASE_FIRST, BASE_LOGP, BASE_FIN, BASE_BLEND, BASE_SEL, refresh<8, 4, 0>},
    {"refresh <16,4>", BASE_FIRST, BASE_LOGP, BASE_FIN, BASE_BLEND, BASE_SEL, refresh<16, 4, 0>},
    {"refresh <16,8>", BASE_FIRST, BASE_LOGP, BASE_FIN, BASE_BLEND, BASE_SEL, refresh<16, 8, 0>},
    {"refresh <32,8>", BASE_FIRST, BASE_LOGP, BASE_FIN, BASE_BLEND, BASE_SEL, refresh<32, 8, 0>},
    {"refresh <8,8> nt scratch loads", BASE_FIRST, BASE_LOGP, BASE_FIN, BASE_BLEND, BASE_SEL, refresh<8, 8, I>},
    {"first nt-in, the resident momentum plain", first_step<I | P>, BASE_LOGP, BASE_FIN, BASE_BLEND, BASE_SEL, BASE_REF},
    {"first nt-in, momentum from a full-width array", first_step_full<I>, BASE_LOGP, BASE_FIN, BASE_BLEND, BASE_SEL, BASE_REF},
    {"base again", BASE_FIRST, BASE_LOGP, BASE_FIN, BASE_BLEND, BASE_SEL, BASE_REF},
};
constexpr int NCFG = sizeof(CFG) / sizeof(CFG[0]);
constexpr int NB = 8;  // bracketed launches per visit
static const char* WHAT[NB] = {"refresh", "first", "step(g+kd)", "grad-only", "logp+grad", "finish", "blend", "select"};

int main(int argc, char** argv) {
  Args a;
  a.C = argc > 1 ? atoll(argv[1]) : 65536;
  a.T = argc > 2 ? atoll(argv[2]) : 8192;
  a.D = argc > 3 ? atoll(argv[3]) : 1024;
  const int reps = argc > 4 ? atoi(argv[4]) : 3;
  if (a.C % a.T || a.T % 2 || a.T <= 0 || a.D <= 0 || a.D > 65535 || reps < 1) return 1;
  CHECK(hipStreamCreate(&a.s));
  const i64 n = a.D * a.C, nt = a.D * a.T;
  double** full[] = {&a.th, &a.rho, &a.g, &a.out};
  double** tile[] = {&a.thp, &a.rk, &a.gp};
  for (double** p : full) {
    CHECK(hipMalloc(p, n * 8));
    k_fill<<<1024, 256, 0, a.s>>>(*p, n, 0.5);
  }
  CHECK(hipMalloc(&a.zt, nt * 8));
  CHECK(hipMalloc(&a.kin0, a.C * 8));
  for (double** p : tile) {
    CHECK(hipMalloc(p, nt * 8));
    k_fill<<<1024, 256, 0, a.s>>>(*p, nt, 0.25);
  }
  CHECK(hipMalloc(&a.lam, a.D * 8));
  CHECK(hipMalloc(&a.lp, a.C * 8));
  CHECK(hipMalloc(&a.kin, a.C * 8));
  CHECK(hipMalloc(&a.mask, a.C));
  k_fill<<<4, 256, 0, a.s>>>(a.lam, a.D, 1.0);
  k_mask<<<64, 256, 0, a.s>>>(a.mask, a.C);
  CHECK(hipStreamSynchronize(a.s));

  const int tiles = (int)(a.C / a.T), visits = tiles * reps;
  std::vector<hipEvent_t> ev((size_t)visits * NB * 2);
  for (auto& e : ev) CHECK(hipEventCreate(&e));
  for (int ic = 0; ic < NCFG; ++ic) {
    const Cfg& c = CFG[ic];
    size_t k = 0;
    auto timed = [&](Fn f) {
      CHECK(hipEventRecord(ev[k++], a.s));
      f(a);
      CHECK(hipEventRecord(ev[k++], a.s));
    };
    for (int r = 0; r < reps + 1; ++r) {  // (the first pass over the tiles warms up and is overwritten)
      if (r == 1) k = 0;
      for (int t = 0; t < tiles; ++t) {
        if (r == 0) k = 0;
        a.c0 = (i64)t * a.T;
        normals(a);
        timed(c.refresh);
        timed(c.first);
        grad_only(a);
        step(a);
        CHECK(hipEventRecord(ev[k++], a.s));
        grad_only(a);
        step(a);
        CHECK(hipEventRecord(ev[k++], a.s));
        timed(grad_only);
        timed(c.logp);
        timed(c.finish);
        timed(c.blend);
        timed(c.select);
      }
    }
    CHECK(hipStreamSynchronize(a.s));
    CHECK(hipGetLastError());
    printf("CFG %2d %s\n   ", ic, c.name);
    for (int b = 0; b < NB; ++b) {
      std::vector<float> v;
      for (int i = 0; i < visits; ++i) {
        float ms;
        CHECK(hipEventElapsedTime(&ms, ev[((size_t)i * NB + b) * 2], ev[((size_t)i * NB + b) * 2 + 1]));
        v.push_back(ms * 1e3f);
      }
      std::sort(v.begin(), v.end());
      printf(" %s %.1f (%.1f-%.1f)", WHAT[b], v[v.size() / 2], v.front(), v.back());
    }
    printf(" us\n");
    fflush(stdout);
  }
  return 0;
}
