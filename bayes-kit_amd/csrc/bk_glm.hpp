// The cell rule of the generalised linear models with canonical links (include/bkhip.h, "GLM targets"): ONE owner, called
// by the fused epilogue of k_dense_apply (csrc/bk_dense.hip) and by the stand-alone pass k_glm_residual (csrc/bk_glm.hip),
// so that the two cannot drift apart.  The build keeps -ffp-contract=off: every operation below is one rounded fp64
// operation, in this association.  No clamping: a non-finite eta gives what IEEE gives (the tables in the header).
#pragma once
#include "bk_common.hpp"

// EPI codes of k_dense_apply: 0 = plain GEMM, 1 = the logistic target's own epilogue, 2 + 2 * family + (offset ? 1 : 0)
// = the GLM cell rule.
constexpr int BK_EPI_GLM0 = 2;
__host__ __device__ constexpr int bk_glm_epi(int family, bool offset) { return BK_EPI_GLM0 + 2 * family + (offset ? 1 : 0); }

// z: the linear predictor's GEMM part; y: the row's response; a: the row's auxiliary value (BINOMIAL: trials m; GAUSSIAN:
// precision w = 1 / sd^2; otherwise not read); o: the row's offset (OFF false: not read, nothing added).  Returns the
// residual r = y - mean (GAUSSIAN: w (y - eta)); LL: `term` is the cell's log likelihood without its constant.
// BERNOULLI without an offset is k_logistic_residual's and EPI == 1's arithmetic, expression for expression.
template <int FAM, bool OFF, bool LL>
__device__ __forceinline__ double bk_glm_cell(double z, double y, double a, double o, double& term) {
  const double eta = OFF ? z + o : z;
  if (FAM == BK_GLM_BERNOULLI || FAM == BK_GLM_BINOMIAL) {
    const double e = exp(-fabs(eta));
    if (LL) {
      const double sp = (eta > 0.0 ? eta : 0.0) + log1p(e);  // log(1 + e^eta)
      term = FAM == BK_GLM_BINOMIAL ? y * eta - a * sp : y * eta - sp;
    }
    const double p = eta >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
    return FAM == BK_GLM_BINOMIAL ? y - a * p : y - p;
  }
  if (FAM == BK_GLM_POISSON) {
    const double mu = exp(eta);
    if (LL) term = y * eta - mu;
    return y - mu;
  }
  const double d = y - eta;  // GAUSSIAN
  const double r = a * d;
  if (LL) term = -0.5 * (r * d);
  return r;
}

// family / offset -> the template arguments: `body` is called with two integral constants
#define BK_GLM_DISPATCH(family, has_offset, CALL)                          \
  do {                                                                     \
    switch (2 * (family) + ((has_offset) ? 1 : 0)) {                       \
      case 0: CALL(BK_GLM_BERNOULLI, false); break;                        \
      case 1: CALL(BK_GLM_BERNOULLI, true); break;                         \
      case 2: CALL(BK_GLM_BINOMIAL, false); break;                         \
      case 3: CALL(BK_GLM_BINOMIAL, true); break;                          \
      case 4: CALL(BK_GLM_POISSON, false); break;                          \
      case 5: CALL(BK_GLM_POISSON, true); break;                           \
      case 6: CALL(BK_GLM_GAUSSIAN, false); break;                         \
      case 7: CALL(BK_GLM_GAUSSIAN, true); break;                          \
    }                                                                      \
  } while (0)

// the argument rule shared by both entry points: BK_OK or BK_E_ARG, decided before any launch
static inline int bk_glm_check(int family, const double* y, const double* aux) {
  if (family < BK_GLM_BERNOULLI || family > BK_GLM_GAUSSIAN || !y) return BK_E_ARG;
  const bool wants_aux = family == BK_GLM_BINOMIAL || family == BK_GLM_GAUSSIAN;
  if (wants_aux != (aux != nullptr)) return BK_E_ARG;
  return BK_OK;
}
