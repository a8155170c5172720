"""A plain high-precision restatement of the logistic-regression target -- TEST INFRASTRUCTURE ONLY, NumPy only.

    z = X Theta,  r = y - sigmoid(z),  loglik = sum_n (y_n z_n - log(1 + e^z_n)),  G = X^T r,
    logp = t * loglik - |theta|^2 / (2 s^2),  grad = t * G - theta / s^2

Everything is evaluated in ``np.longdouble`` (x87 extended: 64-bit significand) with the stable forms -- ``exp(-|z|)``,
``log1p`` -- and rounded to double once, at the end.  Against a double-precision kernel whose error bound is a small
multiple of 2^-53 times a magnitude sum, this reference's own error is 2^-11 of that bound; the bounds in
tests/logistic_parity.py rely on it, hence the assertion on the format below.

Next to each value the functions return the magnitude sum its error bound is made of:
  * a GEMM:  |A| |X|  (componentwise);
  * the log likelihood:  sum of |term| over the TERMS THAT ARE ROUNDED, which are y_n z_n and log(1 + e^z_n), each on
    its own: ``|y z| + softplus(z)``.  (The difference ``y z - softplus(z)`` is not a usable magnitude: at y = 1,
    z = 36.7 it is 1e-16 while both of its operands, each rounded to 7e-15, are 36.7.)
The magnitude sums themselves are formed in double: K positive terms, relative error K * 2^-53, nothing next to the
bound they scale.
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "tests/logistic_ref.py needs a long double with a 64-bit significand"
U = 2.0 ** -53  # unit roundoff of double


def _ld(a):
    return np.asarray(a, dtype=LD)


def gemm(A, X):
    """(A @ X rounded once to double, |A| |X| in double)."""
    A, X = np.asarray(A, dtype=np.float64), np.asarray(X, dtype=np.float64)
    return gemm_ld(A, X).astype(np.float64), np.abs(A) @ np.abs(X)


def gemm_ld(A, X):
    """A @ X in long double, accumulated in increasing k: at most K roundings of 2^-64 each, relative to |A||X|.
    (Rank-one updates: about twice as fast as NumPy's long-double matmul, which has no BLAS behind it.)"""
    At, X = np.ascontiguousarray(_ld(A).T), _ld(X)
    acc = np.zeros((At.shape[1], X.shape[1]), dtype=LD)
    tmp = np.empty_like(acc)
    for k in range(At.shape[0]):
        np.multiply(At[k][:, None], X[k][None, :], out=tmp)
        acc += tmp
    return acc


def sigmoid_softplus_ld(z):
    """(sigmoid(z), log(1 + e^z)) in long double, stable at both ends."""
    z = _ld(z)
    with np.errstate(under="ignore"):
        e = np.exp(-np.abs(z))
    p = np.where(z >= 0, 1 / (1 + e), e / (1 + e))
    sp = np.where(z > 0, z, LD(0)) + np.log1p(e)
    return p, sp


def residual_ld(z, y_rows):
    """y[n] - sigmoid(z[n, c]) in long double (z: [N, C], y_rows: [N])."""
    p, _ = sigmoid_softplus_ld(z)
    return _ld(y_rows)[:, None] - p


def residual(z, y_rows):
    return residual_ld(z, y_rows).astype(np.float64)


def loglik_terms_ld(z, y_rows):
    """(term, |y z| + softplus(z)) per cell, long double."""
    z = _ld(z)
    _, sp = sigmoid_softplus_ld(z)
    yz = _ld(y_rows)[:, None] * z
    return yz - sp, np.abs(yz) + sp


def rows_per_segment(N, segments):
    return -(-max(int(N), 1) // int(segments))


def segment_sums(z, y_rows, segments):
    """(part[segments, C] rounded once to double, its magnitude sums in double, rows per segment): segment s holds
    rows [s * rows, min((s + 1) * rows, N)) with rows = ceil(max(N, 1) / segments); segments past the data are 0."""
    N, C = z.shape
    rows = rows_per_segment(N, segments)
    term, mag = loglik_terms_ld(z, y_rows)
    part = np.zeros((segments, C), dtype=LD)
    pmag = np.zeros((segments, C), dtype=np.float64)
    for s in range(min(segments, -(-N // rows))):
        part[s] = term[s * rows:(s + 1) * rows].sum(axis=0)
        pmag[s] = mag[s * rows:(s + 1) * rows].sum(axis=0).astype(np.float64)
    return part.astype(np.float64), pmag, rows


class LogisticRef:
    """The target for one design matrix; Theta is [D, C] (one chain per column), results per chain."""

    def __init__(self, X, y, prior_scale=1.0):
        self.X = np.asarray(X, dtype=np.float64)
        self.y = np.asarray(y, dtype=np.float64)
        self.inv_s2 = 1.0 / float(prior_scale) ** 2  # (the product and the oracle round 1 / s^2 to double first)

    def evaluate(self, Theta, t=1.0):
        """dict of double arrays: z, r, loglik, G, logp, grad and the magnitudes zmag = |X||Theta|,
        llmag = sum_n (|y z| + softplus z), Gmag = |X^T| |r|, prior = |theta|^2 / (2 s^2).  t may be a tuple of
        temperatures: logp and grad are then tuples, one entry per temperature (the data is walked once)."""
        if isinstance(t, tuple):
            es = [self.evaluate(Theta, t[0])]
            for ti in t[1:]:
                es.append(self._finish(es[0]["_ld"], ti))
            out = dict(es[0])
            out["logp"], out["grad"] = tuple(e["logp"] for e in es), tuple(e["grad"] for e in es)
            return out
        Th = np.asarray(Theta, dtype=np.float64)
        z = gemm_ld(self.X, Th)
        r = residual_ld(z, self.y)
        term, mag = loglik_terms_ld(z, self.y)
        ll = term.sum(axis=0)
        G = gemm_ld(self.X.T, r)
        s2 = (_ld(Th) * _ld(Th)).sum(axis=0)
        prior = -LD(0.5) * LD(self.inv_s2) * s2
        f = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
        out = dict(z=f(z), r=f(r), loglik=f(ll), G=f(G), zmag=np.abs(self.X) @ np.abs(Th), llmag=f(mag.sum(axis=0)),
                   Gmag=np.abs(self.X.T) @ np.abs(f(r)), prior=f(-prior), _ld=(ll, G, prior, _ld(Th)))
        out.update(self._finish(out["_ld"], t))
        return out

    def _finish(self, parts, t):
        ll, G, prior, Th = parts
        t = LD(float(t))
        return dict(logp=np.asarray(t * ll + prior, dtype=np.float64),
                    grad=np.asarray(t * G - LD(self.inv_s2) * Th, dtype=np.float64))


class LongDoubleLogistic:
    """oracle.models.LogisticRegression's interface (one theta at a time) evaluated through the long-double forms above
    and rounded to double at the end: the PERTURBED model of the fixture generator -- a density that differs from the
    oracle's by rounding alone.  A sampler run that makes the same decisions with either model is one whose decisions
    no rounding-level difference in the density can flip."""

    def __init__(self, X, y, prior_scale=1.0):
        self._ref = LogisticRef(X, y, prior_scale)
        self._X, self._Xt, self._y = _ld(self._ref.X), np.ascontiguousarray(_ld(self._ref.X).T), _ld(self._ref.y)

    def dims(self):
        return self._ref.X.shape[1]

    def _parts(self, theta):
        """(loglik, log prior, X^T r, theta), long double (matrix-vector products: NumPy's own long-double loop)."""
        th = _ld(np.asarray(theta, dtype=np.float64).reshape(-1))
        z = self._X @ th
        p, sp = sigmoid_softplus_ld(z)
        ll = (self._y * z - sp).sum()
        return ll, -LD(0.5) * LD(self._ref.inv_s2) * (th * th).sum(), self._Xt @ (self._y - p), th

    def log_likelihood(self, theta):
        return float(self._parts(theta)[0])

    def log_prior(self, theta):
        return float(self._parts(theta)[1])

    def log_density(self, theta):
        ll, lpr, _, _ = self._parts(theta)
        return float(ll + lpr)

    def log_density_gradient(self, theta):
        ll, lpr, G, th = self._parts(theta)
        return float(ll + lpr), np.asarray(G - LD(self._ref.inv_s2) * th, dtype=np.float64)
