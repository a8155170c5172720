// Shifted scatter matrix of the state: S += (X - c 1^T)(X - c 1^T)^T and s += rowsum(X - c 1^T), on the fp64 matrix
// cores (v_mfma_f64_16x16x4_f64).  The dense-metric warmup's statistic: X is the engine's [D x C] state, c a fixed
// centre near the mean, and cov = (S - s s^T / n) / (n - 1) is formed by the caller once per window.
//
// The reduction dimension is the CHAIN index, so both operand panels are rows of X with k contiguous in memory (the
// load pattern k_dense_apply has for M, not the one it has for X).  Tiling as there: 256 threads = 4 wavefronts in
// 2 x 2, workgroup tile 128 x 128 outputs, each wavefront 64 x 64 = 4 x 4 MFMA tiles, K advances 16 chains at a time
// through double-buffered LDS panels.  What differs:
//   - Panels are loaded with 8 consecutive lanes on the 16 consecutive chains of ONE row (16 bytes each): a panel row
//     is one whole 128-byte cache line per load instruction, 8 rows per wavefront.  (k_dense_apply's mapping for M --
//     a lane per row, 64 bytes of it -- touches 64 lines per instruction.)
//   - LDS panels are [row][k] with a pitch of 18 doubles (144 B).  Stores: the 8 lanes of a 16-byte store group write
//     32 consecutive dwords of one row: no conflict.  Fragment reads (ds_read_b64, groups of 32 lanes = 16 rows x 2 k):
//     dword bank = 36 row + 2 k (+ 0, 1) mod 64; 36 row mod 64 runs through the 16 multiples of 4: all 64 banks once.
//     (A [k][row] panel as in k_dense_apply would put the 16 lanes of one row, which differ in k only, on one bank.)
//   - The centre is subtracted as a panel passes from the load's registers to LDS (no centred copy of the state); rows
//     and chains out of range are zero AFTER centring.
//   - Only tile blocks on or below the diagonal are computed.  A diagonal block loads one panel and reads both operands
//     from it; its upper-right wavefront (all outputs above the diagonal) issues no MFMA.  It also owns the row sums of
//     its 128 rows, accumulated from the registers of the panel load.
//   - Split over chains: slab q owns the chain range [q, q + 1) * chunks_per_slab * k_chunk, its own output tiles and row
//     sums in `work`; k_cov_finish adds the slabs in increasing q, then S's lower triangle, and writes every value to
//     (i, j) and (j, i): no floating-point atomics, the same bits every time, S exactly symmetric.
//   - Placement: consecutive slots of one XCD walk the tile blocks of one slab, so a slab's chains are fetched from HBM
//     once and then served by that XCD's L2.  k_chunk (a function of D only) keeps D x k_chunk doubles within half of
//     an XCD's 4 MiB L2; a slab of several chunks passes through them one after the other.
#include "bk_common.hpp"

namespace {

typedef double v4f64 __attribute__((ext_vector_type(4)));
typedef double dvec2 __attribute__((ext_vector_type(2)));

constexpr int BM = 128, BK = 16;
constexpr int PP = 18;                 // panel pitch in doubles
constexpr i64 TILE_ELEMS = BM * BM;    // one output tile block in a slab

struct alignas(16) CovLds {
  double a[2][BM][PP];  // [row of the row block][chain]
  double b[2][BM][PP];  // [row of the column block][chain]; unused by a diagonal block
  double ca[BM], cb[BM];  // the centre's entries of the two blocks' rows (zeros past D or without a centre)
};

// Thread t -> chains 2 (t & 7), + 1 of rows (t >> 3) + 32 i, i = 0..3 (global loads and LDS stores alike).  The loads
// return raw values (zeros outside); the centre is subtracted when the registers go to LDS, so that nothing waits for
// a load before the MFMAs it is meant to hide under.
template <bool FULL>
__device__ __forceinline__ void load_panel(const double* X, i64 ld, i64 r0, i64 k0, i64 D, i64 k_hi,
                                           double (&r)[8]) {
  const int t = threadIdx.x;
  const int kq = (t & 7) * 2, row = t >> 3;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const i64 rr = r0 + row + 32 * i;
    if (FULL) {
      const dvec2 v = *reinterpret_cast<const dvec2*>(X + rr * ld + k0 + kq);
      r[2 * i] = v.x;
      r[2 * i + 1] = v.y;
    } else {
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const i64 k = k0 + kq + e;
        r[2 * i + e] = (rr < D && k < k_hi) ? X[rr * ld + k] : 0.0;
      }
    }
  }
}

// registers - centre -> LDS panel; `left` = chains of the slab from this panel's first on: a chain past the slab's end
// stays zero AFTER centring (rows past D have a centre of zero and were loaded as zeros).  SUM: the centred values are
// also added to the thread's row sums.
template <bool FULL, bool SUM>
__device__ __forceinline__ void store_panel(double (*p)[PP], const double* cen, i64 left, const double (&r)[8],
                                            double (&rs)[4]) {
  const int t = threadIdx.x;
  const int kq = (t & 7) * 2, row = t >> 3;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const double c = cen[row + 32 * i];
    dvec2 v = {r[2 * i] - c, r[2 * i + 1] - c};
    if (!FULL) {
      if (kq >= left) v.x = 0.0;
      if (kq + 1 >= left) v.y = 0.0;
    }
    if (SUM) rs[i] = rs[i] + (v.x + v.y);
    *reinterpret_cast<dvec2*>(&p[row + 32 * i][kq]) = v;
  }
}

template <bool FULL, bool DIAG>
__device__ __forceinline__ void cov_tile(CovLds& lds, const double* X, i64 ld, i64 D, i64 r0, i64 c0, i64 k_lo, i64 k_hi,
                                         double* tp, double* sums) {
  const int lane = threadIdx.x & 63, w = bk_wave_id();
  const int wr = (w >> 1) * 64, wc = (w & 1) * 64;  // wavefront's 64 x 64 corner inside the tile
  const int l15 = lane & 15, l4 = lane >> 4;
  const bool idle = DIAG && wc > wr;  // every output above the diagonal: k_cov_finish never reads it

  v4f64 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (v4f64){0.0, 0.0, 0.0, 0.0};

  double ra[8], rb[8], rs[4] = {0.0, 0.0, 0.0, 0.0};
  load_panel<FULL>(X, ld, r0, k_lo, D, k_hi, ra);
  if (!DIAG) load_panel<FULL>(X, ld, c0, k_lo, D, k_hi, rb);
  store_panel<FULL, DIAG>(lds.a[0], lds.ca, k_hi - k_lo, ra, rs);
  if (!DIAG) store_panel<FULL, false>(lds.b[0], lds.cb, k_hi - k_lo, rb, rs);
  __syncthreads();
  const i64 nk = (k_hi - k_lo + BK - 1) / BK;
  for (i64 kb = 0; kb < nk; ++kb) {
    const int buf = (int)(kb & 1);
    const bool more = kb + 1 < nk;
    const i64 k_next = k_lo + (kb + 1) * BK;
    if (more) {  // in flight under the MFMAs
      load_panel<FULL>(X, ld, r0, k_next, D, k_hi, ra);
      if (!DIAG) load_panel<FULL>(X, ld, c0, k_next, D, k_hi, rb);
    }
    const double(*pa)[PP] = lds.a[buf];
    const double(*pb)[PP] = DIAG ? lds.a[buf] : lds.b[buf];
    if (!idle) {
      // (one fragment set: the loads of k-slice ks + 4 wait behind the 16 MFMAs of slice ks, 1,024 matrix cycles, and
      // the SIMD's other wavefront keeps the pipe busy meanwhile; a second set does not fit beside the accumulators)
#pragma unroll
      for (int ks = 0; ks < BK; ks += 4) {
        double a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = pa[wr + 16 * i + l15][ks + l4];
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = pb[wc + 16 * j + l15][ks + l4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
      }
    }
    if (more) {
      // the other buffer was last read one iteration ago, behind a barrier
      store_panel<FULL, DIAG>(lds.a[buf ^ 1], lds.ca, k_hi - k_next, ra, rs);
      if (!DIAG) store_panel<FULL, false>(lds.b[buf ^ 1], lds.cb, k_hi - k_next, rb, rs);
      __syncthreads();
    }
  }
  // C/D layout of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 * reg.  The slab holds whole tile
  // blocks (rows and columns past D are zeros), so nothing here is bounds-checked against D.
  if (!idle) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = wc + 16 * j + l15;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int r = wr + 16 * i + l4 + 4 * v;
          tp[r * BM + c] = acc[i][j][v];
        }
      }
  }
  if (DIAG) {
    // row sums of this slab's chains: the 8 lanes of a row in a fixed xor tree
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      double v = rs[i];
      v = v + __shfl_xor(v, 1);
      v = v + __shfl_xor(v, 2);
      v = v + __shfl_xor(v, 4);
      if ((threadIdx.x & 7) == 0) sums[(threadIdx.x >> 3) + 32 * i] = v;
    }
  }
}

template <bool FULL>
__global__ __launch_bounds__(256, 2) void k_cov_accumulate(const double* X, i64 ld, i64 C, i64 D, const double* center,
                                                           double* work, i64 slab_elems, int tiles, int slabs,
                                                           i64 slab_chains) {
  __shared__ CovLds lds;
  // XCD-aware placement: consecutive slots of one XCD walk the tile blocks of one slab
  int slab, tile;
  {
    const int xcds = 8;
    const int id = blockIdx.x, xcd = id % xcds, slot = id / xcds;
    slab = (slot / tiles) * xcds + xcd;
    tile = slot % tiles;
    if (slab >= slabs) return;
  }
  int rb_i = 0;  // tile -> (row block, column block <= row block)
  while ((rb_i + 1) * (rb_i + 2) / 2 <= tile) ++rb_i;
  const int cb_i = tile - rb_i * (rb_i + 1) / 2;
  const i64 r0 = (i64)rb_i * BM, c0 = (i64)cb_i * BM;
  const i64 k_lo = (i64)slab * slab_chains;
  const i64 k_hi = (k_lo + slab_chains < C) ? k_lo + slab_chains : C;
  double* out = work + (i64)slab * slab_elems;
  if (threadIdx.x < BM) {
    const i64 ra = r0 + threadIdx.x, rb = c0 + threadIdx.x;
    lds.ca[threadIdx.x] = (center && ra < D) ? center[ra] : 0.0;
    lds.cb[threadIdx.x] = (center && rb < D) ? center[rb] : 0.0;
  }
  __syncthreads();
  double* tp = out + (i64)tile * TILE_ELEMS;
  if (rb_i == cb_i)
    cov_tile<FULL, true>(lds, X, ld, D, r0, c0, k_lo, k_hi, tp, out + (i64)tiles * TILE_ELEMS + r0);
  else
    cov_tile<FULL, false>(lds, X, ld, D, r0, c0, k_lo, k_hi, tp, nullptr);
}

// S(i, j) = S(j, i) = S(i, j) + sum_q slab_q(i, j) for j <= i, slabs in increasing q; s(i) += sum_q rowsum_q(i)
__global__ __launch_bounds__(256) void k_cov_finish(const double* work, i64 slab_elems, int slabs, int tiles, double* S,
                                                    i64 lds, double* s, i64 D, i64 col_blocks) {
  const i64 i = (i64)blockIdx.x / col_blocks;
  const i64 j = ((i64)blockIdx.x % col_blocks) * 256 + threadIdx.x;
  if (i >= D || j > i) return;
  const i64 rb_i = i / BM, cb_i = j / BM;
  const i64 off = (rb_i * (rb_i + 1) / 2 + cb_i) * TILE_ELEMS + (i % BM) * BM + (j % BM);
  double a = work[off];
  for (int q = 1; q < slabs; ++q) a = a + work[(i64)q * slab_elems + off];
  const double v = S[i * lds + j] + a;
  S[i * lds + j] = v;
  S[j * lds + i] = v;
  if (j == 0) {
    const i64 so = (i64)tiles * TILE_ELEMS + i;
    double b = work[so];
    for (int q = 1; q < slabs; ++q) b = b + work[(i64)q * slab_elems + so];
    s[i] = s[i] + b;
  }
}

// The split: k_chunk is a function of D only (what keeps a chunk of D x k_chunk doubles within half an XCD's L2, and at
// the reference width of 2,048 chains gives about 512 workgroups); a slab is a whole number of chunks, as few slabs as
// keep about 1,024 workgroups in flight, so that the slab traffic stays small beside the panels at large C.
struct CovPlan {
  i64 nb, tiles, k_chunk, slab_chains, slabs, slab_elems;
};

static i64 cov_k_chunk(i64 D) {
  const i64 nb = bk_cdiv(D, BM), tiles = nb * (nb + 1) / 2;
  i64 k = bk_cdiv(4 * tiles, BK) * BK;
  if (k < 128) k = 128;
  i64 fit = (((i64)2 << 20) / (8 * D)) / BK * BK;
  if (fit < BK) fit = BK;
  return k < fit ? k : fit;
}

static CovPlan cov_plan(i64 D, i64 C) {
  CovPlan p;
  p.nb = bk_cdiv(D, BM);
  p.tiles = p.nb * (p.nb + 1) / 2;
  p.k_chunk = cov_k_chunk(D);
  const i64 chunks = bk_cdiv(C, p.k_chunk);
  i64 max_slabs = 1024 / p.tiles;
  if (max_slabs < 8) max_slabs = 8;  // one per XCD at least
  const i64 per = bk_cdiv(chunks, max_slabs);
  p.slab_chains = per * p.k_chunk;
  p.slabs = bk_cdiv(C, p.slab_chains);
  p.slab_elems = p.tiles * TILE_ELEMS + p.nb * BM;
  return p;
}

}  // namespace

extern "C" {

int64_t bk_cov_k_chunk(int64_t D) { return D < 1 ? 0 : cov_k_chunk(D); }

int64_t bk_cov_accumulate_work_elems(int64_t D, int64_t C) {
  if (D < 1 || C < 1) return 0;
  const CovPlan p = cov_plan(D, C);
  return p.slabs * p.slab_elems;
}

int bk_cov_accumulate(const double* X, int64_t ld, int64_t C, int64_t D, const double* center, double* S, int64_t lds,
                      double* s, double* work, int64_t work_elems, void* stream) {
  if (!X || !S || !s || C < 0 || D < 0 || ld < C || lds < D) return BK_E_ARG;
  if (C == 0 || D == 0) return BK_OK;
  const CovPlan p = cov_plan(D, C);
  if (!work || work_elems < p.slabs * p.slab_elems) return BK_E_ARG;
  const i64 grid = bk_cdiv(p.slabs, 8) * 8 * p.tiles;
  const i64 col_blocks = bk_cdiv(D, 256);
  if (grid > 0x7fffffff || p.slabs > 0x7fffffff || p.tiles > 0x7fffffff || D * col_blocks > 0x7fffffff) return BK_E_ARG;
  hipStream_t st = bk_stream(stream);
  const bool full = (D % BM == 0) && (C % BK == 0) && (ld % 2 == 0) && bk_aligned16(X);
  if (full)
    k_cov_accumulate<true><<<dim3((unsigned)grid), dim3(256), 0, st>>>(X, ld, C, D, center, work, p.slab_elems,
                                                                       (int)p.tiles, (int)p.slabs, p.slab_chains);
  else
    k_cov_accumulate<false><<<dim3((unsigned)grid), dim3(256), 0, st>>>(X, ld, C, D, center, work, p.slab_elems,
                                                                        (int)p.tiles, (int)p.slabs, p.slab_chains);
  k_cov_finish<<<dim3((unsigned)(D * col_blocks)), dim3(256), 0, st>>>(work, p.slab_elems, (int)p.slabs, (int)p.tiles, S,
                                                                       lds, s, D, col_blocks);
  BK_RETURN_LAUNCH_STATUS();
}

}  // extern "C"
