"""A plain high-precision restatement of the GLM targets -- TEST INFRASTRUCTURE ONLY, NumPy only.

    eta = X Theta + o,   r = y - mean(eta)  (gaussian: w (y - eta)),   loglik = sum_n term_n + const,   G = X^T r,
    logp = t * loglik - |theta|^2 / (2 s^2),   grad = t * G - theta / s^2

with the four cell rules of include/bkhip.h ("GLM targets") evaluated in ``np.longdouble`` and rounded to double once, at the
end, like tests/logistic_ref.py (whose GEMM, segment rule and unit roundoff are reused).  Next to each value the functions
return the magnitude sum its error bound is made of: the sum of the absolute values of THE TERMS THAT ARE ROUNDED,

    bernoulli:  |y eta| + softplus(eta)          binomial:  |y eta| + a softplus(eta)
    poisson:    |y eta| + mu                     gaussian:  0.5 w (y - eta)^2   (one product chain, no cancellation)
"""
import math

import numpy as np

from tests import logistic_ref as lref

LD, U = lref.LD, lref.U
FAMILIES = ("bernoulli", "binomial", "poisson", "gaussian")
HAS_AUX = {"bernoulli": False, "binomial": True, "poisson": False, "gaussian": True}
# rounded operations per cell on the way to `term`: the `k` of the segment-sum bound u (rows + k) magnitude (derivations in
# tests/glm_parity.check_cells)
TERM_OPS = {"bernoulli": 8, "binomial": 9, "poisson": 8, "gaussian": 4}


def _ld(a):
    return np.asarray(a, dtype=LD)


def _col(v):
    return None if v is None else _ld(v)[:, None]


def eta_ld(z, offset):
    z = _ld(z)
    return z if offset is None else z + _col(offset)


def cells_ld(family, z, y, aux=None, offset=None):
    """(r, term, term magnitude, eta) per cell of z [N, C], long double; y, aux, offset per row."""
    eta, yv, a = eta_ld(z, offset), _col(y), _col(aux)
    if family in ("bernoulli", "binomial"):
        p, sp = lref.sigmoid_softplus_ld(eta)
        if family == "binomial":
            p, sp = a * p, a * sp
        yz = yv * eta
        return yv - p, yz - sp, np.abs(yz) + sp, eta
    if family == "poisson":
        with np.errstate(under="ignore"):
            mu = np.exp(eta)
        yz = yv * eta
        return yv - mu, yz - mu, np.abs(yz) + mu, eta
    if family == "gaussian":
        d = yv - eta
        t = LD(0.5) * (a * d * d)
        return a * d, -t, t, eta
    raise ValueError(family)


def residual(family, z, y, aux=None, offset=None):
    return np.asarray(cells_ld(family, z, y, aux, offset)[0], dtype=np.float64)


def segment_sums(family, z, y, aux, offset, segments):
    """(part[segments, C] rounded once, its magnitude sums in double, rows per segment): logistic_ref.segment_sums' rule."""
    N, C = z.shape
    rows = lref.rows_per_segment(N, segments)
    _, term, mag, _ = cells_ld(family, z, y, aux, offset)
    part = np.zeros((segments, C), dtype=LD)
    pmag = np.zeros((segments, C), dtype=np.float64)
    for s in range(min(segments, -(-N // rows))):
        part[s] = term[s * rows:(s + 1) * rows].sum(axis=0)
        pmag[s] = mag[s * rows:(s + 1) * rows].sum(axis=0).astype(np.float64)
    return part.astype(np.float64), pmag, rows


def constants(family, y, aux=None):
    """The per-observation normalising constants (doubles, math.lgamma / math.log: what the issue defines the constant by)."""
    y = np.asarray(y, dtype=np.float64)
    if family == "bernoulli":
        return [0.0] * len(y)
    if family == "binomial":
        return [math.lgamma(m + 1.0) - math.lgamma(v + 1.0) - math.lgamma(m - v + 1.0) for v, m in zip(y.tolist(), aux.tolist())]
    if family == "poisson":
        return [-math.lgamma(v + 1.0) for v in y.tolist()]
    if family == "gaussian":
        return [0.5 * (math.log(w) - math.log(2.0 * math.pi)) for w in np.asarray(aux, dtype=np.float64).tolist()]
    raise ValueError(family)


class GLMRef:
    """The target for one data set; Theta is [D, C] (one chain per column), results per chain.  aux: trials (binomial) or the
    PRECISION w (gaussian), as doubles -- the values the library is handed."""

    def __init__(self, X, y, family, prior_scale=1.0, aux=None, offset=None):
        f = lambda v: None if v is None else np.asarray(v, dtype=np.float64)  # noqa: E731
        self.X, self.y, self.aux, self.offset, self.family = f(X), f(y), f(aux), f(offset), family
        self.inv_s2 = 1.0 / float(prior_scale) ** 2
        cs = constants(family, self.y, self.aux)
        self.const, self.const_mag = math.fsum(cs), math.fsum(abs(c) for c in cs)

    def evaluate(self, Theta, ts=(1.0,)):
        """dict: z (the GEMM part of eta), eta, r, loglik (WITH the constant), G, logp / grad (tuples, one per temperature) and
        the magnitudes zmag = |X||Theta|, llmag (terms only), prior = |theta|^2 / (2 s^2), absr = |r|, slope = |d r / d eta|."""
        Th = np.asarray(Theta, dtype=np.float64)
        z = lref.gemm_ld(self.X, Th)
        r, term, mag, eta = cells_ld(self.family, z, self.y, self.aux, self.offset)
        ll = term.sum(axis=0) + LD(self.const)
        G = lref.gemm_ld(self.X.T, r)
        s2 = (_ld(Th) * _ld(Th)).sum(axis=0)
        prior = -LD(0.5) * LD(self.inv_s2) * s2
        # |d r / d eta| per cell: how an error of eta reaches r
        if self.family in ("bernoulli", "binomial"):
            p, _ = lref.sigmoid_softplus_ld(eta)
            slope = p * (1 - p) * (1 if self.family == "bernoulli" else _col(self.aux))
        elif self.family == "poisson":
            slope = np.exp(eta)
        else:
            slope = np.broadcast_to(_col(self.aux), eta.shape)
        f = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
        zmag = np.abs(self.X) @ np.abs(Th)
        out = dict(z=f(z), eta=f(eta), r=f(r), loglik=f(ll), G=f(G), zmag=zmag, llmag=f(mag.sum(axis=0)), prior=f(-prior),
                   slope=f(slope), absr=f(np.abs(r)))
        out["logp"] = tuple(f(LD(float(t)) * ll + prior) for t in ts)
        out["grad"] = tuple(f(LD(float(t)) * G - LD(self.inv_s2) * _ld(Th)) for t in ts)
        return out
