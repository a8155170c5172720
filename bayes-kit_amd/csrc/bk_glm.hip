// GLM targets (Bernoulli, binomial, Poisson, Gaussian regression with canonical links): the stand-alone elementwise pass
// between the two GEMMs Z = X_data Theta and G = X_data^T r.  The cell rule is bk_glm_cell (bk_glm.hpp), shared with the
// fused epilogue of k_dense_apply; the pass keeps k_logistic_residual's shape (csrc/bk_dense.hip): 256 chains per
// workgroup, `segments` row blocks, RL_ROWS loads in flight, a segment's terms summed left to right.
#include "bk_common.hpp"
#include "bk_glm.hpp"

namespace {

constexpr int RL_ROWS = 8;

// Z[n][c] -> the residual of bk_glm_cell in place; part[seg][c] = the left-to-right sum of the segment's terms (a segment
// past the data: exactly +0.0).  LL false: the caller wants the gradient only -- no log1p, nothing written to part.
template <int FAM, bool OFF, bool LL>
__global__ __launch_bounds__(256) void k_glm_residual(double* Z, i64 ldz, const double* y, const double* aux,
                                                      const double* off, double* part, i64 N, i64 C, i64 rows_per_seg) {
  constexpr bool AUX = FAM == BK_GLM_BINOMIAL || FAM == BK_GLM_GAUSSIAN;
  i64 c = (i64)blockIdx.x * 256 + threadIdx.x;
  i64 seg = blockIdx.y;
  if (c >= C) return;
  i64 n0 = seg * rows_per_seg, n1 = n0 + rows_per_seg;
  if (n1 > N) n1 = N;
  double ll = 0.0;
  for (i64 nb = n0; nb < n1; nb += RL_ROWS) {
    double zz[RL_ROWS];
#pragma unroll
    for (int i = 0; i < RL_ROWS; ++i)
      if (nb + i < n1) zz[i] = Z[(nb + i) * ldz + c];
#pragma unroll
    for (int i = 0; i < RL_ROWS; ++i) {
      if (nb + i < n1) {
        double term = 0.0;
        const double r = bk_glm_cell<FAM, OFF, LL>(zz[i], y[nb + i], AUX ? aux[nb + i] : 0.0, OFF ? off[nb + i] : 0.0, term);
        if (LL) ll = ll + term;
        Z[(nb + i) * ldz + c] = r;
      }
    }
  }
  if (LL) part[seg * C + c] = ll;
}

}  // namespace

extern "C" {

int bk_glm_residual(double* Z, int64_t ldz, int family, const double* y, const double* aux, const double* offset,
                    double* part, int64_t N, int64_t C, int64_t segments, void* stream) {
  if (bk_glm_check(family, y, aux) != BK_OK) return BK_E_ARG;
  if (!Z || N < 0 || C < 0 || segments < 1 || segments > 65535) return BK_E_ARG;
  if (ldz < C) return BK_E_ALIGN;
  if (C == 0) return BK_OK;
  const i64 rows = bk_cdiv(N > 0 ? N : 1, segments);
  const dim3 grid((unsigned)bk_cdiv(C, 256), (unsigned)segments);
  hipStream_t st = bk_stream(stream);
#define BK_GLM_PASS(FAM, OFF)                                                                                  \
  do {                                                                                                         \
    if (part) k_glm_residual<FAM, OFF, true><<<grid, dim3(256), 0, st>>>(Z, ldz, y, aux, offset, part, N, C, rows); \
    else k_glm_residual<FAM, OFF, false><<<grid, dim3(256), 0, st>>>(Z, ldz, y, aux, offset, nullptr, N, C, rows);  \
  } while (0)
  BK_GLM_DISPATCH(family, offset != nullptr, BK_GLM_PASS);
#undef BK_GLM_PASS
  BK_RETURN_LAUNCH_STATUS();
}

}  // extern "C"
