"""NumPy restatement of the multi-chain ESS (Vehtari, Gelman, Simpson, Carpenter and Buerkner 2021, sec. 3.2, eqs. 10-11,
with Geyer's initial monotone sequence) and a FakeOps subclass with the multi-chain ESS entry points -- TEST
INFRASTRUCTURE ONLY.  Written from the estimator's text, independently of bayes_kit_amd.diagnostics: autocovariances by
FFT in float64, the scan transcribed line by line."""
import numpy as np
import scipy.stats
import torch

from tests.fake_ops import FakeOps


def split(x):
    """[N, C] -> [n, 2C]: rows [0, n) and rows [N - n, N) of every column (the middle row of an odd N dropped)."""
    N = x.shape[0]
    n = N // 2
    return np.concatenate([x[:n], x[N - n:]], axis=1)


def autocov(chains):
    """Biased autocovariance gamma[t, m] = (1/n) sum_{i < n - t} (x_i - xbar)(x_{i+t} - xbar) of each column, by FFT."""
    n = chains.shape[0]
    d = chains - chains.mean(axis=0)
    size = 1 << int(np.ceil(np.log2(2 * n - 1)))
    f = np.fft.rfft(d, n=size, axis=0)
    return np.fft.irfft(f * np.conj(f), n=size, axis=0)[:n] / n


def autocov_direct(chains):
    n, M = chains.shape
    d = chains - chains.mean(axis=0)
    return np.array([(d[: n - t] * d[t:]).sum(axis=0) / n for t in range(n)])


def scan(Gamma, W, var_plus, M, n):
    """The Geyer scan of the estimator's text -> (tau, max_t)."""
    def rho_of(t):
        return 1 - (W - Gamma[t]) / var_plus

    rho = np.zeros(n)
    rho[0] = 1
    r_even = 1.0
    r_odd = rho_of(1)
    rho[1] = r_odd
    t = 0
    while t < n - 5 and not np.isnan(r_even + r_odd) and r_even + r_odd > 0:
        t += 2
        r_even = rho_of(t)
        r_odd = rho_of(t + 1)
        if r_even + r_odd >= 0:
            rho[t] = r_even
            rho[t + 1] = r_odd
    max_t = t
    if r_even > 0:
        rho[max_t] = r_even
    t = 0
    while t <= max_t - 4:
        t += 2
        if rho[t] + rho[t + 1] > rho[t - 2] + rho[t - 1]:
            rho[t] = rho[t + 1] = (rho[t - 2] + rho[t - 1]) / 2
    tau = max(-1 + 2 * np.sum(rho[0:max_t]) + rho[max_t], 1 / np.log10(M * n))
    return tau, max_t


def ess_split_chains(ch, direct=False):
    """(ESS, max_t) of split chains ch [n, M]; NaN for non-finite draws or var_plus == 0."""
    n, M = ch.shape
    if not np.all(np.isfinite(ch)):
        return np.nan, None
    g = autocov_direct(ch) if direct else autocov(ch)
    W = np.mean(g[0]) * n / (n - 1)
    var_plus = W * (n - 1) / n + np.var(ch.mean(axis=0), ddof=1)
    if var_plus == 0:
        return np.nan, None
    tau, max_t = scan(g.mean(axis=1), W, var_plus, M, n)
    return M * n / tau, max_t


def z_scores(x):
    """Rank-normalised split set: ordinal stable ranks of the column-major pooled draws, (r - 0.325) / (S - 0.25)."""
    s = split_rows(x)
    flat = s.T.reshape(-1)
    r = np.empty(flat.size)
    r[np.argsort(flat, kind="stable")] = np.arange(1, flat.size + 1)
    z = scipy.stats.norm.ppf((r - 0.325) / (flat.size - 0.25))
    return z.reshape(s.shape[1], s.shape[0]).T


def split_rows(x):
    """[N, C] -> [2n, C] without the middle row of an odd N."""
    N = x.shape[0]
    n = N // 2
    return np.concatenate([x[:n], x[N - n:]], axis=0)


def ess_mean(x, direct=False):
    return ess_split_chains(split(x), direct)[0]


def ess_bulk(x):
    if not np.all(np.isfinite(split_rows(x))):  # (the split set: the middle row of an odd N is not part of the estimator)
        return np.nan
    return ess_split_chains(split(z_scores(x)))[0]


def ess_quantile(x, prob):
    s = split_rows(x)
    q = np.quantile(s, prob)
    ind = (s <= q).astype(np.float64)
    if not np.all(np.isfinite(s)):
        return np.nan
    return ess_split_chains(split(ind))[0]


def ess_tail(x):
    return float(np.min([ess_quantile(x, 0.05), ess_quantile(x, 0.95)]))  # (NaN if either is)


def mcse_mean(x):
    s = split_rows(x)
    return np.std(s, ddof=1) / np.sqrt(ess_mean(x))


def ar1(rng, N, C, phi, offset=None):
    """AR(1) chains x_t = phi x_{t-1} + e_t started from the stationary law (unit marginal variance) -> [N, C]."""
    e = rng.standard_normal((N, C)) * np.sqrt(1 - phi * phi)
    x = np.empty((N, C))
    x[0] = rng.standard_normal(C)
    for t in range(1, N):
        x[t] = phi * x[t - 1] + e[t]
    if offset is not None:
        x = x + offset
    return x


class MultiEssFakeOps(FakeOps):
    """FakeOps with the multi-chain ESS entry points of include/bkhip.h, restated in NumPy."""

    def __init__(self, max_half=10**9):
        super().__init__()
        self.max_half = max_half

    # Every entry point takes what the HIP wrappers take: strided [:, off:off + C] views of wider buffers and the leading
    # entries of longer (NaN-padded) vectors; only the cells of the views are read or written.
    @staticmethod
    def _split(x, q):
        a = x.numpy()
        s = split(a)
        if q is not None:
            s = (s <= q).astype(np.float64)
        return a, s

    def ess_lag_sums_max_half(self):
        return self.max_half

    def ess_split_moments(self, x, q, chain_mean, chain_g0):
        self._count("ess_split_moments")
        a, s = self._split(x, q)
        n, M = s.shape
        with np.errstate(invalid="ignore", over="ignore"):  # (a non-finite draw makes its chain's moments NaN, as on the device)
            mu = s.sum(axis=0) / n
            g0 = ((s - mu) ** 2).sum(axis=0) / n
            chain_mean.numpy()[:M] = mu
            chain_g0.numpy()[:M] = g0
            bad = float(np.sum(~np.isfinite(split(a))))
            return torch.tensor([mu.sum(), g0.sum(), bad], dtype=torch.float64)

    def ess_between_sq(self, chain_mean, centre):
        with np.errstate(invalid="ignore", over="ignore"):
            return torch.tensor([((chain_mean.numpy() - centre.numpy()[0]) ** 2).sum()], dtype=torch.float64)

    def ess_lag_sums(self, x, q, chain_mean, lag0, nlags):
        self._count("ess_lag_sums")
        _, s = self._split(x, q)
        n = s.shape[0]
        d = s - chain_mean.numpy()[:s.shape[1]]
        with np.errstate(invalid="ignore", over="ignore"):
            return torch.tensor([(d[: n - t] * d[t:]).sum() / n for t in range(lag0, lag0 + nlags)], dtype=torch.float64)

    def ess_acov_sums(self, acor, chain_g0, lag0, nlags):
        self._count("ess_acov_sums")
        a, g = acor.numpy(), chain_g0.numpy()[:acor.shape[1]]
        with np.errstate(invalid="ignore"):
            v = np.where(g != 0.0, a[lag0:lag0 + nlags] * g, 0.0)  # (a chain with gamma_0 = 0 contributes exactly 0)
        return torch.from_numpy(np.ascontiguousarray(v).sum(axis=1))

    def ess_indicator(self, x, q, out):
        with np.errstate(invalid="ignore"):
            out.numpy()[...] = (x.numpy() <= q).astype(np.float64)

    def select_ranks(self, rank, values, targets, out):
        if not 1 <= targets.numel() <= 8:
            raise ValueError("bk_select_ranks takes 1 to 8 targets")
        r, v = rank.numpy(), values.numpy()
        for j, t in enumerate(targets.numpy()):
            hit = np.nonzero(r == t)[0]
            if hit.size:
                out[j] = v[hit[0]]
