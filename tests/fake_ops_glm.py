"""tests/fake_ops.FakeOps plus the two GLM entry points in NumPy, in the contract's operation order (include/bkhip.h, "GLM
targets") -- TEST INFRASTRUCTURE ONLY.  The stand-in walks what the library walks: gemm_block's split into the FULL rows and
the partial last row block (with the per-row pointers advanced by R_full) and the residual pass's segments.

``FakeOpsGLM(fault=...)`` plants ONE fault; tests/test_glm_cpu.py shows each caught by the shared body named for it."""
import numpy as np

from bayes_kit_amd import _lib
from tests.fake_ops import FakeOps

BERNOULLI, BINOMIAL, POISSON, GAUSSIAN = range(4)
FAULTS = ("aux_not_advanced", "offset_not_advanced", "offset_after_exp", "binomial_m_not_in_term",
          "gaussian_precision_dropped_from_r", "poisson_term_from_yz", "const_per_segment", "const_left_out_of_loglik",
          "null_part_changes_r")
BM, BN, BK = 128, 128, 16  # k_dense_apply's tile


class GLMFakeMixin:
    """The two entry points (and the faults) on top of any FakeOps; ``fault`` is a plain attribute."""

    fault = None

    # -- the cell rule: every line one rounded fp64 operation per operator, in the header's association --------------
    def _cells(self, family, z, y, a, o, want_term):
        """(r, term or None) of z [n, C] with per-row y, a, o ([n] arrays or None)."""
        f = self.fault
        col = lambda v: None if v is None else v[:, None]  # noqa: E731
        y, a, o = col(y), col(a), col(o)
        term = None
        with np.errstate(all="ignore"):
            eta = z if o is None else z + o
            late = f == "offset_after_exp" and o is not None
            if family in (BERNOULLI, BINOMIAL):
                e = np.exp(-np.abs(z)) + o if late else np.exp(-np.abs(eta))
                if want_term:
                    sp = np.where(eta > 0.0, eta, 0.0) + np.log1p(e)
                    term = y * eta - (a * sp if family == BINOMIAL and f != "binomial_m_not_in_term" else sp)
                p = np.where(eta >= 0.0, 1.0 / (1.0 + e), e / (1.0 + e))
                r = y - (a * p if family == BINOMIAL else p)
            elif family == POISSON:
                mu = np.exp(z) + o if late else np.exp(eta)
                if want_term:
                    term = y * (z if f == "poisson_term_from_yz" else eta) - mu
                r = y - mu
            else:
                d = y - eta
                r = a * d
                if want_term:
                    term = -0.5 * (r * d)
                if f == "gaussian_precision_dropped_from_r":
                    r = d
        if f == "null_part_changes_r" and not want_term:
            r = np.nextafter(r, np.inf)
        return r, term

    @staticmethod
    def _check(name, family, y, aux):
        wants_aux = family in (BINOMIAL, GAUSSIAN)
        if family not in (BERNOULLI, BINOMIAL, POISSON, GAUSSIAN) or y is None or wants_aux != (aux is not None):
            raise _lib.BkHipError(f"{name} failed: BK_E_ARG")

    # -- bk_gemm_chains_glm ------------------------------------------------------------------------------------------
    def gemm_chains_glm(self, A, X, Y, family, y_rows, aux_rows=None, offset_rows=None):
        self._check("bk_gemm_chains_glm", family, y_rows, aux_rows)
        if not self._gemm(A, X, Y):
            return
        R, K = A.shape
        C = X.shape[1]
        lda, ldx = _lib._ld(A), _lib._ld(X)
        full_but_rows = (K > 0 and K % BK == 0 and C % BN == 0 and lda % 2 == 0 and ldx % 2 == 0
                         and A.data_ptr() % 16 == 0 and X.data_ptr() % 16 == 0)
        R_full = R - R % BM if full_but_rows else 0
        yv = y_rows.numpy()
        av = None if aux_rows is None else aux_rows.numpy()
        ov = None if offset_rows is None else offset_rows.numpy()
        out = Y.numpy()
        for lo, hi in ((0, R_full), (R_full, R)):  # the unchecked launch, then the checked one with advanced pointers
            if hi <= lo:
                continue
            a_lo = 0 if self.fault == "aux_not_advanced" else lo
            o_lo = 0 if self.fault == "offset_not_advanced" else lo
            out[lo:hi], _ = self._cells(family, out[lo:hi], yv[lo:hi], None if av is None else av[a_lo:a_lo + hi - lo],
                                        None if ov is None else ov[o_lo:o_lo + hi - lo], False)

    # -- bk_glm_residual ---------------------------------------------------------------------------------------------
    def glm_residual(self, Z, family, y, aux, offset, part, segments=None):
        self._check("bk_glm_residual", family, y, aux)
        S = part.shape[0] if part is not None else int(segments or 256)
        if not 1 <= S <= 65535:
            raise _lib.BkHipError("bk_glm_residual failed: BK_E_ARG")
        z = Z.numpy()
        N = z.shape[0]
        r, term = self._cells(family, z, y.numpy(), None if aux is None else aux.numpy(),
                              None if offset is None else offset.numpy(), part is not None)
        if part is not None:
            rows = -(-max(N, 1) // S)
            p = part.numpy()
            p[...] = 0.0
            for s in range(min(S, -(-N // rows))):
                acc = np.zeros(z.shape[1])
                for row in term[s * rows:(s + 1) * rows]:  # left to right
                    acc = acc + row
                p[s] = acc
        z[...] = r

    # -- the constant's carrier: the last row of `part` (faults only; the finish itself is FakeOps') -----------------
    def logistic_finish(self, G, theta, part, inv_prior_var, t, grad, logp, loglik):
        if self.fault == "const_per_segment" and part is not None and part.shape[0] > 1:
            import torch

            p = part.numpy()
            part = torch.from_numpy(np.concatenate([p[:-1] + p[-1], np.zeros((1, p.shape[1]))]))
        if self.fault == "const_left_out_of_loglik" and part is not None and part.shape[0] > 1 and loglik is not None:
            super().logistic_finish(None, theta, part[:-1], inv_prior_var, t, None, None, loglik)
            loglik = None
        super().logistic_finish(G, theta, part, inv_prior_var, t, grad, logp, loglik)


class FakeOpsGLM(GLMFakeMixin, FakeOps):
    def __init__(self, fault=None):
        super().__init__()
        assert fault is None or fault in FAULTS, fault
        self.fault = fault
