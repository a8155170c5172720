// bk_hist_accumulate: fixed-grid histograms of every coordinate of a [D][ld] draw (RunningHistogram; include/bkhip.h).
//
// One workgroup per (row d, slab of chains).  The workgroup keeps a private histogram of 32-bit counters in LDS, streams its
// slab of the row once with 16-byte loads (a scalar head and tail where the slab does not start or end on 16 bytes) and adds
// the counters that are not zero to the caller's int64 counts with 64-bit integer atomics.  Integer sums do not depend on
// their order: the counts are the same bits for every slab size, launch geometry and arrival order.
//
// More slots than the LDS window holds (B + 3 > HIST_WINDOW): the SAME kernel walks the slots window by window -- zero, stream
// the slab again (it was just read: the re-reads are cache hits), count the values whose slot falls into the window, flush.
// There is no second algorithm behind the seam, only a second trip of the loop.
//
// Hot bins.  Chains that share a value (superchain starts, copies after resampling) sit next to each other, and all lanes of
// a wavefront adding to one LDS address are served one after the other.  Before the LDS add a wavefront therefore merges RUNS
// of equal slots in consecutive lanes: the first lane of a run adds the run's length (one ballot, no loop).  An all-equal
// row costs one LDS atomic per wavefront and load component instead of 64.
#include "bk_common.hpp"

namespace {

constexpr int HIST_THREADS = 256;
constexpr int HIST_WINDOW = 8192;                 // 32-bit counters of one LDS window (32 KiB)
constexpr i64 HIST_UNIT = 2 * 4 * HIST_THREADS;   // chains: four 16-byte loads per thread
constexpr i64 HIST_MAX_SLAB = (i64)1 << 30;       // a 32-bit counter holds a whole slab (2^30 < 2^32)
constexpr i64 HIST_MAX_BINS = 65536;
constexpr i64 HIST_MIN_WORKGROUPS = 2048;         // 256 CUs x 8 workgroups of 256 threads

typedef double hvec2 __attribute__((ext_vector_type(2)));

// chains one workgroup covers: whole units; enough workgroups to fill the chip when C allows it; at least twice the slots
// of a window, so that zeroing and flushing the window stay below the cost of streaming the slab
static i64 hist_slab_chains(i64 C, i64 D, i64 B) {
  if (C < 1 || D < 1 || B < 1 || B > HIST_MAX_BINS) return 0;
  const i64 slabs_wanted = bk_cdiv(HIST_MIN_WORKGROUPS, D);
  i64 slab = bk_cdiv(bk_cdiv(C, slabs_wanted), HIST_UNIT) * HIST_UNIT;
  const i64 window = B + 3 < HIST_WINDOW ? B + 3 : HIST_WINDOW;
  const i64 floor_ = bk_cdiv(2 * window, HIST_UNIT) * HIST_UNIT;
  if (slab < floor_) slab = floor_;
  if (slab > HIST_MAX_SLAB) slab = HIST_MAX_SLAB;
  return slab;
}

// the slot of x: the contract of include/bkhip.h, one rounded subtraction and one rounded multiplication
__device__ __forceinline__ int hist_slot(double x, double lo, double scale, int B) {
  if (x != x) return B + 2;
  const double t = __dmul_rn(__dsub_rn(x, lo), scale);
  if (t < 0.0) return 0;
  if (t >= (double)B) return B + 1;
  return 1 + (int)t;  // 0 <= t < B <= 65536: the truncation is exact in 32 bits
}

// Every lane of the wavefront calls this with its slot relative to the window (anything outside [0, n_win) counts nothing).
// Lanes whose predecessor holds the same slot stay silent; the first lane of each run adds the run's length.
__device__ __forceinline__ void hist_add_runs(uint32_t* h, int rel, int n_win) {
  const int lane = (int)(threadIdx.x & (BK_WAVE - 1));
  const int prev = __shfl_up(rel, 1);
  const bool head = lane == 0 || prev != rel;
  const unsigned long long heads = __ballot(head);
  if (head && rel >= 0 && rel < n_win) {
    const unsigned long long above = lane == BK_WAVE - 1 ? 0ull : heads & (~0ull << (lane + 1));
    const int next = above ? __ffsll((long long)above) - 1 : BK_WAVE;
    atomicAdd(&h[rel], (uint32_t)(next - lane));
  }
}

__global__ __launch_bounds__(HIST_THREADS) void k_hist_accumulate(const double* __restrict__ theta, i64 ld, i64 C, i64 slab,
                                                                  const double* __restrict__ lo_, const double* __restrict__ scale_,
                                                                  int B, unsigned long long* __restrict__ counts, i64 ldc) {
  extern __shared__ __attribute__((aligned(16))) uint32_t h[];
  const int tid = (int)threadIdx.x;
  const i64 d = (i64)blockIdx.x;
  const i64 c0 = (i64)blockIdx.y * slab;
  const i64 n = (C - c0) < slab ? (C - c0) : slab;  // >= 1 by the grid
  const double* p = theta + d * ld + c0;
  const double lo = lo_[d], scale = scale_[d];
  unsigned long long* out = counts + d * ldc;
  // the 16-byte body: [head, head + 2 n2) of the slab; doubles are 8-byte aligned, so the head is 0 or 1 element
  const i64 head = ((reinterpret_cast<uintptr_t>(p) & 15u) != 0) ? 1 : 0;
  const i64 n2 = (n - head) / 2;
  const i64 tail = n - head - 2 * n2;  // 0 or 1
  const hvec2* body = reinterpret_cast<const hvec2*>(p + head);
  const int slots = B + 3;
  for (int w0 = 0; w0 < slots; w0 += HIST_WINDOW) {
    const int n_win = slots - w0 < HIST_WINDOW ? slots - w0 : HIST_WINDOW;
    for (int j = tid; j < n_win; j += HIST_THREADS) h[j] = 0u;
    __syncthreads();
    if (tid == 0) {  // the scalar head and tail
      if (head) {
        const int r = hist_slot(p[0], lo, scale, B) - w0;
        if (r >= 0 && r < n_win) atomicAdd(&h[r], 1u);
      }
      if (tail) {
        const int r = hist_slot(p[n - 1], lo, scale, B) - w0;
        if (r >= 0 && r < n_win) atomicAdd(&h[r], 1u);
      }
    }
    // two loads in flight per thread; the trip count is the same for every lane (the run merge needs whole wavefronts)
    for (i64 base = 0; base < n2; base += 2 * HIST_THREADS) {
      const i64 i0 = base + tid, i1 = i0 + HIST_THREADS;
      const bool v0 = i0 < n2, v1 = i1 < n2;
      hvec2 a = {0.0, 0.0}, b = {0.0, 0.0};
      if (v0) a = body[i0];
      if (v1) b = body[i1];
      hist_add_runs(h, v0 ? hist_slot(a.x, lo, scale, B) - w0 : -1, n_win);
      hist_add_runs(h, v0 ? hist_slot(a.y, lo, scale, B) - w0 : -1, n_win);
      hist_add_runs(h, v1 ? hist_slot(b.x, lo, scale, B) - w0 : -1, n_win);
      hist_add_runs(h, v1 ? hist_slot(b.y, lo, scale, B) - w0 : -1, n_win);
    }
    __syncthreads();
    for (int j = tid; j < n_win; j += HIST_THREADS) {
      const uint32_t v = h[j];
      if (v) atomicAdd(&out[w0 + j], (unsigned long long)v);
    }
    __syncthreads();  // the next window zeroes what this flush reads
  }
}

}  // namespace

extern "C" {

int64_t bk_hist_lds_bins(void) { return HIST_WINDOW - 3; }

int64_t bk_hist_slab_chains(int64_t C, int64_t D, int64_t B) { return hist_slab_chains(C, D, B); }

int bk_hist_accumulate(const double* theta, int64_t ld, int64_t C, int64_t D, const double* lo, const double* scale,
                       int64_t B, int64_t* counts, int64_t ldc, void* stream) {
  if (!theta || !lo || !scale || !counts || C < 0 || D < 0 || B < 1 || B > HIST_MAX_BINS || ld < C || ldc < B + 3)
    return BK_E_ARG;
  if (C == 0 || D == 0) return BK_OK;
  const i64 slab = hist_slab_chains(C, D, B);
  const i64 slabs = bk_cdiv(C, slab);
  if (D > 2147483647 || slabs > 65535) return BK_E_ARG;
  const i64 window = B + 3 < HIST_WINDOW ? B + 3 : HIST_WINDOW;
  k_hist_accumulate<<<dim3((unsigned)D, (unsigned)slabs), dim3(HIST_THREADS), (size_t)window * sizeof(uint32_t),
                      bk_stream(stream)>>>(theta, ld, C, slab, lo, scale, (int)B,
                                           reinterpret_cast<unsigned long long*>(counts), ldc);
  BK_RETURN_LAUNCH_STATUS();
}

}  // extern "C"
