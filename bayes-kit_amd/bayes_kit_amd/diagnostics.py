"""Convergence diagnostics on the GPU: drop-ins for ``bayes_kit/rhat.py``, ``ess.py``,
``iat.py`` and ``autocorr.py``, plus the streaming / multi-GPU forms the many-chain engine
uses.

Inputs.  Every function accepts what the reference accepts (a 1-D chain, or a sequence of
1-D chains for the R-hat family) and, additionally, a 2-D float64 device tensor ``[N, C]``
(draw-major: N draws of C chains, one chain per GPU lane).  For a 2-D input the per-chain
functions (ess, iat, autocorr) return one value (or column) per chain.

Across GPUs.  Chains are sharded; the only cross-rank traffic is the per-dimension partial
sums of R-hat (a few doubles per dimension).  They are exchanged with ONE small
``all_gather`` per pass (RCCL when the tensors live on the GPU, gloo in the CPU tests) and
combined in rank order, so the result does not depend on the reduction order.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch
import torch.distributed as dist

from . import _lib
from . import dist as _bkdist


def _ops(ops):
    return ops if ops is not None else _lib.default_ops()


# ---------------------------------------------------------------------------------------------
# cross-rank combine
# ---------------------------------------------------------------------------------------------
def _gather_sum(t: torch.Tensor, group=None) -> torch.Tensor:
    """Sum of `t` over the ranks of `group`, accumulated in rank order (deterministic).
    No-op without an initialised process group."""
    from .dist import gather_sum

    return gather_sum(t, group)


def _cross_chain_moments(mean_dc, m2_dc, n: int, ops, group=None, ieee_division=False):
    """-> (mean over all ranks' chains of the per-chain variances, variance (ddof = 1) of the per-chain means), device
    tensors [D], from per-chain Welford moments ``mean, M2`` ([D, C_local] each, n draws per chain).

    Two passes, like ``np.var(means, ddof=1)``: first sum(mean) and sum(var) -> grand mean;
    then sum((mean - grand mean)^2).  Each pass is one kernel + one tiny all_gather.
    ieee_division: divide by the chain count as a TENSOR (PyTorch divides a device tensor by a host scalar by multiplying
    with its reciprocal, which is one ulp off the quotient for some values): the same doubles on every device.
    """
    D, C = mean_dc.shape
    dev = mean_dc.device
    if n < 2:
        raise ValueError("rhat requires len(chain) >= 2 for every chain in chains")
    part = torch.zeros(3 * D + 1, dtype=torch.float64, device=dev)
    ops.rhat_partials(mean_dc, m2_dc, n, None, part)
    part[3 * D] = float(C)
    tot = _gather_sum(part, group)
    M = float(tot[3 * D].item())
    if M < 2:
        raise ValueError(f"rhat requires len(chains) >= 2, but len(chains) = {int(M)}")
    Md = tot[3 * D:3 * D + 1] if ieee_division else M
    centre = (tot[0:D] / Md).contiguous()
    mean_var = tot[D:2 * D] / Md
    part2 = torch.zeros(3 * D + 1, dtype=torch.float64, device=dev)
    ops.rhat_partials(mean_dc, m2_dc, n, centre, part2)
    tot2 = _gather_sum(part2, group)
    var_means = tot2[2 * D:3 * D] / (Md - 1.0)
    return mean_var, var_means


def rhat_from_moments(mean_dc, m2_dc, n: int, ops=None, group=None) -> np.ndarray:
    """Per-dimension R-hat (bayes_kit/rhat.py:163-171) from per-chain Welford moments
    ``mean, M2`` ([D, C_local] each, n draws per chain), over ALL ranks' chains."""
    mean_var, var_means = _cross_chain_moments(mean_dc, m2_dc, n, _ops(ops), group)
    nf = float(n)
    return torch.sqrt((nf - 1.0) / nf + var_means / mean_var).cpu().numpy()


def pooled_mean_from_moments(mean_dc, m2_dc, n: int, ops=None, group=None) -> torch.Tensor:
    """Per-dimension mean of the draws of all chains of all ranks pooled (every chain holds n >= 1 draws, so it is the mean
    of the per-chain means): the first pass of ``_cross_chain_moments``, one kernel + one all_gather.  A device tensor [D]."""
    ops = _ops(ops)
    D, C = mean_dc.shape
    if n < 1:
        raise ValueError("pooled_mean requires len(chain) >= 1 for every chain in chains")
    part = torch.zeros(3 * D + 1, dtype=torch.float64, device=mean_dc.device)
    ops.rhat_partials(mean_dc, m2_dc, max(int(n), 2), None, part)  # (the row sums of the means do not depend on n)
    part[3 * D] = float(C)
    tot = _gather_sum(part, group)
    if float(tot[3 * D].item()) < 1:
        raise ValueError("pooled_mean requires len(chains) >= 1, but len(chains) = 0")
    return tot[0:D] / tot[3 * D:3 * D + 1]  # (divided as a TENSOR: the same doubles on every device)


def pooled_variance_from_moments(mean_dc, m2_dc, n: int, ops=None, group=None) -> torch.Tensor:
    """Per-dimension variance of the draws of all chains of all ranks pooled, from the same moments and the same two
    passes as R-hat: (n-1)/n * mean_c(var_c) + var_c(mean_c), both ddof = 1.  A device tensor [D]."""
    mean_var, var_means = _cross_chain_moments(mean_dc, m2_dc, n, _ops(ops), group, ieee_division=True)
    nf = float(n)
    return (nf - 1.0) / nf * mean_var + var_means


# ---------------------------------------------------------------------------------------------
# nested R-hat: many short chains
# ---------------------------------------------------------------------------------------------
# Margossian, Hoffman, Sountsov, Riou-Durand, Vehtari, Gelman: "Nested R-hat: assessing the convergence of Markov chain
# Monte Carlo when running many short chains".  The C chains are K superchains of M: chain c belongs to superchain c // M
# (contiguous blocks, as dist.shard's), the M chains of a superchain share a start and differ by their streams.  Per
# coordinate, with mu_km / M2_km the mean and Welford M2 of the n draws of chain k M + m:
#     s_k  = mean_m(mu_km)
#     Bt_k = sum_m (mu_km - s_k)^2 / (M - 1)      (0 for M = 1)
#     Wt_k = mean_m(M2_km / (n - 1))              (0 for n = 1)
#     B = var_k(s_k, ddof=1)       W = mean_k(Bt_k + Wt_k)       nested R-hat = sqrt(1 + B / W)
# It is defined from the first draw on (n = 1 needs M >= 2) and its threshold tightens with M, not with n.  For M = 1,
# nested R-hat^2 = R-hat^2 + 1/n.  NaN draws and W = 0 are not filtered: the result is what IEEE arithmetic gives (NaN, or
# inf for B > 0 = W).
#
# The device reduces per superchain (bk_superchain_moments: s_k and Bt_k + Wt_k, [D, K]); across superchains
# _cross_chain_moments already is mean_k / var_k over all ranks -- handed (s, w) as (mean, M2) with n = 2, its division by
# n - 1 is a division by 1.0.  A superchain must not straddle ranks: every rank's chain count is a multiple of M.  So that
# a rank which breaks this rule raises on EVERY rank inside the same two all_gathers, the arrays carry one more row: its
# w is 1.0 on such a rank (which then contributes one dummy superchain) and 0.0 elsewhere, and a positive mean says so.
def _check_superchain_args(n: int, M: int) -> None:
    if M < 1:
        raise ValueError(f"nested_rhat requires chains_per_superchain >= 1, but chains_per_superchain = {M}")
    if n < 1:
        raise ValueError("nested_rhat requires len(chain) >= 1 for every chain in chains")
    if M == 1 and n == 1:
        raise ValueError("nested_rhat requires chains_per_superchain >= 2 or len(chain) >= 2, but both are 1")


def nested_rhat_from_moments(mean_dc, m2_dc, n: int, chains_per_superchain: int, ops=None, group=None) -> np.ndarray:
    """Per-dimension nested R-hat from per-chain Welford moments ``mean, M2`` ([D, C_local] each, n draws per chain;
    ``m2_dc`` may be None for n = 1), over ALL ranks' superchains of ``chains_per_superchain`` consecutive chains."""
    ops = _ops(ops)
    n, M = int(n), int(chains_per_superchain)
    _check_superchain_args(n, M)
    D, C = mean_dc.shape
    dev = mean_dc.device
    straddles = C % M != 0
    multi = _bkdist.collectives_active(group)
    if straddles and not multi:
        raise ValueError(f"nested_rhat requires len(chains) to be a multiple of chains_per_superchain = {M}, "
                         f"but len(chains) = {C}")
    K = 1 if straddles else C // M
    if straddles:
        s = torch.zeros((D + 1, K), dtype=torch.float64, device=dev)
        w = torch.zeros((D + 1, K), dtype=torch.float64, device=dev)
        w[D] = 1.0
    else:  # (the kernel writes every cell of the first D rows: only the flag row is cleared)
        s = torch.empty((D + 1, K), dtype=torch.float64, device=dev)
        w = torch.empty((D + 1, K), dtype=torch.float64, device=dev)
        s[D].zero_()
        w[D].zero_()
        ops.superchain_moments(mean_dc, m2_dc if n > 1 else None, n, M, s[:D], w[:D])
    try:
        mean_w, var_s = _cross_chain_moments(s, w, 2, ops, group)
    except ValueError as e:  # (its message counts chains; here they are superchains)
        ours = f"nested_rhat requires len(chains) // {M} >= 2 superchains, but len(chains) // {M}"
        raise ValueError(str(e).replace("rhat requires len(chains) >= 2, but len(chains)", ours)) from None
    if multi and float(mean_w[D].item()) > 0.0:
        raise ValueError(f"nested_rhat requires len(chains) to be a multiple of chains_per_superchain = {M} on every rank "
                         "(a superchain must not straddle ranks)")
    return torch.sqrt(1.0 + var_s[:D] / mean_w[:D]).cpu().numpy()


def _nested_rhat_of_series(series, M: int, ops, group=None) -> np.ndarray:
    """nested R-hat of each stored [n, C] series (chains in columns): per-chain moments by bk_chain_mean_var, M2 = var (n - 1)."""
    if not series:
        return np.empty(0)
    n, C = series[0].shape
    _check_superchain_args(int(n), int(M))
    dev = series[0].device
    mean = torch.empty((len(series), C), dtype=torch.float64, device=dev)
    var = torch.empty((len(series), C), dtype=torch.float64, device=dev) if n > 1 else None
    for k, x in enumerate(series):
        x = x if (x.shape[1] == 1 or x.stride(1) == 1) and x.dtype == torch.float64 else x.to(torch.float64).contiguous()
        ops.chain_mean_var(x, None, mean[k], None if var is None else var[k])
    return nested_rhat_from_moments(mean, None if var is None else var * float(n - 1), n, M, ops, group)


def nested_rhat(chains, chains_per_superchain: int, *, ops=None, group=None):
    """Nested R-hat of one quantity (see the note above ``nested_rhat_from_moments``).

    ``chains``: a device tensor [N, C], or a sequence of equal-length 1-D chains; chains k M .. k M + M - 1 form
    superchain k (M = ``chains_per_superchain``).  With a process group ``chains`` is this rank's shard (whole
    superchains) and the statistic is over all ranks.  Defined from N = 1 on when M >= 2."""
    ops = _ops(ops)
    if _is_matrix(chains):
        x = chains
    else:
        arrs = [np.asarray(c, dtype=np.float64).reshape(-1) for c in chains]
        if len({a.shape[0] for a in arrs}) > 1:
            raise ValueError("nested_rhat requires chains of equal length")
        n0 = arrs[0].shape[0] if arrs else 0
        host = np.stack(arrs, axis=1) if arrs else np.zeros((n0, 0))
        x = torch.from_numpy(np.ascontiguousarray(host)).to(ops.device)
    if x.shape[0] < 1:
        raise ValueError("nested_rhat requires len(chain) >= 1 for every chain in chains")
    return np.float64(_nested_rhat_of_series([x], int(chains_per_superchain), ops, group)[0])


def superchain_init(points, chains_per_superchain: int):
    """(K, D) start points -> the (K M, D) ``init`` every sampler takes: point k repeated M = ``chains_per_superchain``
    times, contiguously, so that chain c starts at ``points[c // M]`` -- the c -> c // M convention of ``nested_rhat``.
    The M subchains of a superchain differ only by their random streams, which the samplers key by chain id."""
    M = int(chains_per_superchain)
    if M < 1:
        raise ValueError(f"superchain_init requires chains_per_superchain >= 1, but chains_per_superchain = {M}")
    if isinstance(points, torch.Tensor):
        if points.dim() != 2:
            raise ValueError(f"superchain_init takes (K, D) start points, got shape {tuple(points.shape)}")
        return points.repeat_interleave(M, dim=0)
    p = np.asarray(points, dtype=np.float64)
    if p.ndim != 2:
        raise ValueError(f"superchain_init takes (K, D) start points, got shape {p.shape}")
    return np.repeat(p, M, axis=0)


def _as_dc(theta, D: int, C: int, layout=None):
    """A sampler's draw as a logical [D, C] tensor.  ``sample()`` returns the (C, D) transpose view of the
    engine's [D, C] buffer.  For C != D the shape tells the two apart; for a square draw the strides do
    (the (C, D) view of a chain-contiguous buffer has stride(0) == 1, the buffer itself stride(1) == 1),
    and ``layout`` ("dc" or "cd") overrides both."""
    if theta.dim() != 2:
        raise ValueError(f"expected a 2-D draw, got shape {tuple(theta.shape)}")
    if layout not in (None, "dc", "cd"):
        raise ValueError("layout must be 'dc' ([D, C]) or 'cd' ((C, D))")
    shape = tuple(theta.shape)
    if layout is None:
        if C != D:
            if shape not in ((D, C), (C, D)):
                raise ValueError(f"draw of shape {shape} is neither [{D}, {C}] nor ({C}, {D})")
            layout = "dc" if shape == (D, C) else "cd"
        elif shape != (D, C):
            raise ValueError(f"draw of shape {shape}, expected ({C}, {D})")
        elif theta.stride(1) == 1 and theta.stride(0) != 1:
            layout = "dc"
        elif theta.stride(0) == 1 and theta.stride(1) != 1:
            layout = "cd"
        elif D == 1:
            layout = "dc"
        else:
            raise ValueError(f"a square {shape} draw with strides {tuple(theta.stride())}: pass layout='cd' for sample()'s "
                             "(C, D) or layout='dc' for a [D, C] buffer")
    want = (D, C) if layout == "dc" else (C, D)
    if shape != want:
        raise ValueError(f"draw of shape {shape} with layout={layout!r}, expected {want}")
    return theta if layout == "dc" else theta.t()


class RunningMoments:
    """Streaming per-chain mean / M2 of every dimension (Welford), fed one draw at a time."""

    def __init__(self, D: int, C: int, ops=None):
        self._ops = _ops(ops)
        dev = self._ops.device
        self.mean = torch.zeros((D, C), dtype=torch.float64, device=dev)
        self.m2 = torch.zeros((D, C), dtype=torch.float64, device=dev)
        self.n = 0

    def update(self, theta, layout=None) -> None:
        """theta: the sampler's draw, either the engine's [D, C] buffer or the (C, D) view
        returned by ``sample()`` (told apart by shape, for C == D by strides: see _as_dc)."""
        t = _as_dc(theta, self.mean.shape[0], self.mean.shape[1], layout)
        if (t.shape[1] > 1 and t.stride(1) != 1) or t.dtype != torch.float64:
            t = t.to(torch.float64).contiguous()  # (chains must be contiguous; theta's row pitch may differ from the moments')
        self.n += 1
        self._ops.welford_update(self.mean, self.m2, t, self.n)

    def _update_dev(self, theta_dc, n_dev, n_offset) -> None:
        """update() as a part of a sampler's draw (DrGhmcDiag.attach): the update count is read on the device,
        n = n_dev[0] - n_offset; the caller keeps self.n in step."""
        self._ops.welford_update_dev(self.mean, self.m2, theta_dc, n_dev, n_offset)

    def _update_job(self, n_offset):
        """_update_dev(...) as the Welford part of a job the NEXT draw's generator launch carries along
        (DrGhmcDiag.advance(n); ops.diag_job)."""
        return (self.mean, self.m2, n_offset)

    def rhat(self, group=None) -> np.ndarray:
        return rhat_from_moments(self.mean, self.m2, self.n, self._ops, group)

    def nested_rhat(self, chains_per_superchain: int, group=None) -> np.ndarray:
        """Per-dimension nested R-hat over superchains of ``chains_per_superchain`` consecutive chains (of all ranks):
        defined from the first draw on (nested_rhat_from_moments)."""
        return nested_rhat_from_moments(self.mean, self.m2, self.n, chains_per_superchain, self._ops, group)

    def pooled_variance(self, group=None) -> np.ndarray:
        """Per-dimension variance of all draws seen so far, pooled over the chains of all ranks:
        (n-1)/n * mean_c(var_c) + var_c(mean_c), both ddof = 1 (needs n >= 2 draws and >= 2 chains, as rhat)."""
        return pooled_variance_from_moments(self.mean, self.m2, self.n, self._ops, group).cpu().numpy()

    def pooled_mean(self, group=None) -> np.ndarray:
        """Per-dimension mean of all draws seen so far, pooled over the chains of all ranks (needs n >= 1 draws)."""
        return pooled_mean_from_moments(self.mean, self.m2, self.n, self._ops, group).cpu().numpy()

    def reset(self) -> None:
        """Forget every draw: the moments start again from nothing."""
        self.mean.zero_()
        self.m2.zero_()
        self.n = 0

    # checkpoint / resume: the Welford state is (n, mean, M2); restored, the stream of
    # updates continues bit for bit
    def state_dict(self):
        return {"n": self.n, "mean": self.mean.detach().cpu().clone(), "m2": self.m2.detach().cpu().clone()}

    def load_state_dict(self, sd):
        if tuple(sd["mean"].shape) != tuple(self.mean.shape):
            raise ValueError(f"checkpoint holds moments of shape {tuple(sd['mean'].shape)}, expected {tuple(self.mean.shape)}")
        self.mean.copy_(sd["mean"].to(self.mean.device))
        self.m2.copy_(sd["m2"].to(self.m2.device))
        self.n = int(sd["n"])


class RunningCovariance:
    """Streaming D x D covariance of the draws of ALL chains pooled -- the full-matrix counterpart of RunningMoments,
    fed one draw at a time.  Kept as the shifted sums S = sum (x - c)(x - c)^T and s = sum (x - c) over the n points
    seen (bk_cov_accumulate: one fp64 MFMA pass over the draw, D^2 C flop), with the centre c fixed by the FIRST update
    after construction or reset() to that draw's cross-chain mean (the row sums of bk_rhat_partials, divided on the
    device): the draws of a warmup window stay near it, so (S - s s^T / n) / (n - 1) does not cancel.  Sized for the dense
    metric's range, D up to a few hundred (or modest chain counts): the state is D^2 doubles, an update at
    1,024 x 65,536 chains is of the order of a second.  Non-finite chain states poison the estimate, as they do
    RunningMoments'; they are not filtered.

    Across ranks every rank must shift by the same vector: pass ``group`` to update() and the first update takes the mean
    over the chains of all ranks (sums gathered in rank order)."""

    def __init__(self, D: int, ops=None):
        self._ops = _ops(ops)
        dev = self._ops.device
        self._D = int(D)
        self.S = torch.zeros((self._D, self._D), dtype=torch.float64, device=dev)
        self.s = torch.zeros(self._D, dtype=torch.float64, device=dev)
        self.center = torch.zeros(self._D, dtype=torch.float64, device=dev)
        self.n = 0
        self._work, self._work_C = None, -1

    def update(self, theta, layout=None, group=None) -> None:
        """theta: the sampler's draw, the engine's [D, C] buffer or the (C, D) view returned by ``sample()`` (as
        RunningMoments.update; C may differ between updates).  n += C."""
        D = self._D
        if theta.dim() != 2:
            raise ValueError(f"expected a 2-D draw, got shape {tuple(theta.shape)}")
        if layout is None:  # (the chain count is whichever extent is not D; a square draw is told apart by _as_dc)
            C = theta.shape[1] if (theta.shape[0] == D and theta.shape[1] != D) else theta.shape[0]
        else:
            C = theta.shape[1] if layout == "dc" else theta.shape[0]
        t = _as_dc(theta, D, C, layout)
        if (t.shape[1] > 1 and t.stride(1) != 1) or t.dtype != torch.float64:
            t = t.to(torch.float64).contiguous()
        ops = self._ops
        if self.n == 0:
            part = torch.zeros(3 * D + 1, dtype=torch.float64, device=t.device)
            ops.rhat_partials(t, t, 2, None, part)  # part[0:D] = the row sums over this rank's chains
            part[3 * D] = float(C)
            tot = _gather_sum(part, group)
            self.center.copy_(tot[0:D] / tot[3 * D:3 * D + 1])  # (divided as a TENSOR: the same doubles on every device)
        if self._work_C != C:
            self._work, self._work_C = ops.cov_work(D, C), C
        ops.cov_accumulate(t, self.center, self.S, self.s, self._work)
        self.n += C

    def _totals(self, group):
        D = self._D
        if self.n == 0 and not _bkdist.collectives_active(group):
            raise ValueError("covariance of no draws")
        pack = torch.cat([self.S.reshape(-1), self.s, torch.tensor([float(self.n)], dtype=torch.float64,
                                                                    device=self.S.device)])
        tot = _gather_sum(pack, group)
        return tot[0:D * D].reshape(D, D), tot[D * D:D * D + D], tot[D * D + D:D * D + D + 1]

    def covariance(self, group=None) -> torch.Tensor:
        """Device tensor [D, D]: (S - s s^T / n) / (n - 1) with S, s, n summed over the ranks of `group` in rank order
        (every rank must have shifted by the same centre: update(..., group=group)).  Exactly symmetric."""
        S, s, n = self._totals(group)
        if float(n) < 2:
            raise ValueError("covariance needs at least 2 points")
        return (S - torch.outer(s, s) / n) / (n - 1.0)

    def mean(self, group=None) -> torch.Tensor:
        """Device tensor [D]: the mean of all points seen, center + s / n."""
        _, s, n = self._totals(group)
        return self.center + s / n

    def reset(self) -> None:
        """Forget every draw; the next update fixes a new centre."""
        self.S.zero_()
        self.s.zero_()
        self.center.zero_()
        self.n = 0

    def state_dict(self):
        return {"n": self.n, "S": self.S.detach().cpu().clone(), "s": self.s.detach().cpu().clone(),
                "center": self.center.detach().cpu().clone()}

    def load_state_dict(self, sd):
        if tuple(sd["S"].shape) != tuple(self.S.shape):
            raise ValueError(f"checkpoint holds a scatter matrix of shape {tuple(sd['S'].shape)}, expected "
                             f"{tuple(self.S.shape)}")
        self.S.copy_(sd["S"].to(self.S.device))
        self.s.copy_(sd["s"].to(self.s.device))
        self.center.copy_(sd["center"].to(self.center.device))
        self.n = int(sd["n"])


def _named(idx) -> str:
    """'coordinates [0, 3, 7]' for an error message, cut after eight."""
    idx = [int(i) for i in idx]
    return f"coordinate{'s' if len(idx) != 1 else ''} {idx[:8]}" + (f" and {len(idx) - 8} more" if len(idx) > 8 else "")


class RunningHistogram:
    """Streaming quantiles of EVERY coordinate in fixed memory: one fixed-grid histogram per coordinate, fed one draw at a
    time (bk_hist_accumulate: one pass over the [D, C] draw) -- medians and credible intervals for runs whose draws cannot
    be kept.  The state is ``D x (bins + 3)`` int64 counters, whatever the number of chains and draws.

    Coordinate d has ``bins`` equal bins on ``[lo[d], hi[d])`` plus three slots: 0 "below", bins + 1 "above", bins + 2 NaN.
    The slot of a value x is ``t = (x - lo) * scale`` (one rounded subtraction, one rounded multiplication, ``scale =
    bins / (hi - lo)`` computed once on the host): NaN -> bins + 2, t < 0 -> 0, t >= bins -> bins + 1, else 1 + int(t).  The
    counters are integers, so the counts are the same bits for every launch geometry and every split of the chains over
    ranks, and a few lines of NumPy restate them exactly.

    A quantile is read from the counts: the k-th smallest value, k = ceil(p n), lies in the first slot whose running count
    reaches k, and is placed inside that bin by its rank among the bin's values.  It differs from the k-th order statistic
    of everything fed by less than ONE bin width (both lie in the same bin); with ``from_moments`` at its defaults a bin is
    1/32 of a posterior standard deviation.  Values off the grid are counted, never dropped: ``coverage()`` says how many
    were on it, and a quantile that falls off the grid is -inf or +inf (with one warning)."""

    def __init__(self, lo, hi, bins: int = 512, ops=None):
        self._ops = _ops(ops)
        dev = self._ops.device
        lo_h, hi_h = (np.array(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float64).reshape(-1)
                      for v in (lo, hi))
        bins = int(bins)
        if not 1 <= bins <= 65536:
            raise ValueError(f"RunningHistogram requires 1 <= bins <= 65536, but bins = {bins}")
        if lo_h.shape != hi_h.shape or lo_h.size < 1:
            raise ValueError(f"RunningHistogram takes lo and hi of one length D >= 1, got {lo_h.size} and {hi_h.size}")
        bad = np.flatnonzero(~(np.isfinite(lo_h) & np.isfinite(hi_h)))
        if bad.size:
            raise ValueError(f"RunningHistogram requires finite edges: lo or hi is not finite at {_named(bad)}")
        bad = np.flatnonzero(hi_h <= lo_h)
        if bad.size:
            raise ValueError(f"RunningHistogram requires lo < hi: hi <= lo at {_named(bad)}")
        with np.errstate(over="ignore", divide="ignore"):
            scale_h = float(bins) / (hi_h - lo_h)
        bad = np.flatnonzero(~np.isfinite(scale_h) | (scale_h <= 0.0))
        if bad.size:
            raise ValueError(f"RunningHistogram: bins / (hi - lo) is not a finite positive number at {_named(bad)}")
        self.bins = bins
        self._lo_h, self._hi_h, self._scale_h = lo_h, hi_h, scale_h
        self.lo = torch.from_numpy(lo_h).to(dev)
        self.scale = torch.from_numpy(scale_h).to(dev)
        self._counts = torch.zeros((lo_h.size, bins + 3), dtype=torch.int64, device=dev)
        self.n = 0

    @classmethod
    def from_moments(cls, moments: "RunningMoments", bins: int = 512, width: float = 8.0, group=None):
        """The grid ``pooled mean -/+ width * sqrt(pooled variance)`` of a RunningMoments fed during warmup (over the chains
        of all ranks of ``group``: every rank gets the same grid).  At the defaults a bin is 1/32 of a posterior sd."""
        width = float(width)
        if not (np.isfinite(width) and width > 0.0):
            raise ValueError(f"from_moments requires a finite width > 0, but width = {width}")
        mean = moments.pooled_mean(group)
        var = moments.pooled_variance(group)
        bad = np.flatnonzero(~(np.isfinite(var) & (var > 0.0) & np.isfinite(mean)))
        if bad.size:
            raise ValueError(f"from_moments requires a finite mean and a finite variance > 0: not so at {_named(bad)}")
        half = width * np.sqrt(var)
        return cls(mean - half, mean + half, bins=bins, ops=moments._ops)

    @property
    def D(self) -> int:
        return self._counts.shape[0]

    def update(self, theta, layout=None) -> None:
        """theta: the sampler's draw, the engine's [D, C] buffer or the (C, D) view returned by ``sample()`` (as
        RunningMoments.update; C may differ between updates).  n += C."""
        D = self.D
        if theta.dim() != 2:
            raise ValueError(f"expected a 2-D draw, got shape {tuple(theta.shape)}")
        if layout is None:  # (the chain count is whichever extent is not D; a square draw is told apart by _as_dc)
            C = theta.shape[1] if (theta.shape[0] == D and theta.shape[1] != D) else theta.shape[0]
        else:
            C = theta.shape[1] if layout == "dc" else theta.shape[0]
        t = _as_dc(theta, D, C, layout)
        if (t.shape[1] > 1 and t.stride(1) != 1) or t.dtype != torch.float64:
            t = t.to(torch.float64).contiguous()
        self._ops.hist_accumulate(t, self.lo, self.scale, self.bins, self._counts)
        self.n += C

    # -- read-outs ---------------------------------------------------------------------------------------------------------
    def counts(self, group=None) -> torch.Tensor:
        """int64 [D, bins + 3], summed over the ranks of ``group`` (one all_gather; integer sums have no order)."""
        return _gather_sum(self._counts, group).clone()

    def edges(self) -> np.ndarray:
        """[D, bins + 1]: edge b of coordinate d is lo[d] + b / scale[d] (bin b is [edge b, edge b + 1))."""
        return self._lo_h[:, None] + np.arange(self.bins + 1, dtype=np.float64)[None, :] / self._scale_h[:, None]

    def _host_counts(self, group):
        return _gather_sum(self._counts, group).cpu().numpy()

    def coverage(self, group=None) -> np.ndarray:
        """[D]: the fraction of the non-NaN values of each coordinate inside [lo, hi) (NaN where there is none)."""
        c = self._host_counts(group)
        B = self.bins
        inside, n = c[:, 1:B + 1].sum(axis=1), c[:, :B + 2].sum(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(n > 0, inside / np.maximum(n, 1), np.nan)

    def quantile(self, probs, group=None) -> np.ndarray:
        """[len(probs), D] float64.  Per coordinate, with n the number of non-NaN values and c the counts: k = min(max(
        ceil(p n), 1), n); b = the first slot whose running count cum[b] reaches k; slot 0 -> -inf, slot bins + 1 -> +inf
        (one RuntimeWarning), else lo + ((b - 1) + (k - cum[b - 1] - 0.5) / c[b]) / scale.  n == 0 -> NaN."""
        p = np.atleast_1d(np.asarray(probs, dtype=np.float64))
        if p.ndim != 1 or not np.all((p >= 0.0) & (p <= 1.0)):
            raise ValueError("quantile requires probabilities in [0, 1]")
        B = self.bins
        c = self._host_counts(group)[:, :B + 2]
        cum = np.cumsum(c, axis=1)
        n = cum[:, -1]
        rows = np.arange(c.shape[0])
        out = np.full((p.size, c.shape[0]), np.nan)
        off = np.zeros(c.shape[0], dtype=bool)
        for i, pi in enumerate(p):
            k = np.minimum(np.maximum(np.ceil(pi * n.astype(np.float64)).astype(np.int64), 1), n)
            b = (cum < k[:, None]).sum(axis=1)  # the first slot with cum >= k (n == 0: meaningless, masked below)
            b = np.minimum(b, B + 1)
            before = np.where(b > 0, cum[rows, np.maximum(b - 1, 0)], 0)
            cb = np.maximum(c[rows, b], 1)
            q = self._lo_h + ((b - 1) + (k - before - 0.5) / cb) / self._scale_h
            q = np.where(b == 0, -np.inf, np.where(b == B + 1, np.inf, q))
            out[i] = np.where(n > 0, q, np.nan)
            off |= (n > 0) & ((b == 0) | (b == B + 1))
        if off.any():
            import warnings

            warnings.warn(f"RunningHistogram.quantile: a requested quantile of {int(off.sum())} of {off.size} coordinates "
                          "lies off the grid (-inf / +inf returned; see coverage())", RuntimeWarning, stacklevel=2)
        return out

    def median(self, group=None) -> np.ndarray:
        return self.quantile([0.5], group)[0]

    def interval(self, mass: float = 0.9, group=None):
        """The equal-tailed interval of probability ``mass``: (lower, upper), [D] each."""
        mass = float(mass)
        if not 0.0 < mass < 1.0:
            raise ValueError(f"interval requires 0 < mass < 1, but mass = {mass}")
        q = self.quantile([0.5 * (1.0 - mass), 1.0 - 0.5 * (1.0 - mass)], group)
        return q[0], q[1]

    def reset(self) -> None:
        """Forget every draw; the grid stays."""
        self._counts.zero_()
        self.n = 0

    # checkpoint / resume: the grid, the bin count, n and the counts; restored, the updates continue to the same integers
    def state_dict(self):
        return {"lo": torch.from_numpy(self._lo_h.copy()), "hi": torch.from_numpy(self._hi_h.copy()), "bins": self.bins,
                "n": self.n, "counts": self._counts.detach().cpu().clone()}

    def load_state_dict(self, sd):
        lo, hi = np.asarray(sd["lo"], dtype=np.float64), np.asarray(sd["hi"], dtype=np.float64)
        if int(sd["bins"]) != self.bins or lo.shape != self._lo_h.shape or not (
                np.array_equal(lo, self._lo_h) and np.array_equal(hi, self._hi_h)):
            raise ValueError("checkpoint holds a histogram on another grid (lo, hi and bins must equal this one's)")
        if tuple(sd["counts"].shape) != tuple(self._counts.shape):
            raise ValueError(f"checkpoint holds counts of shape {tuple(sd['counts'].shape)}, expected "
                             f"{tuple(self._counts.shape)}")
        self._counts.copy_(sd["counts"].to(self._counts.device))
        self.n = int(sd["n"])


class EnergyDiagnostics:
    """Divergent transitions and E-BFMI of an HMC run, tracked on the device: per-chain running statistics of the energy
    error and of the selected energy, and a fixed store of the states divergent trajectories STARTED from.  No draw is kept
    and nothing is read back per draw.

    ``update`` takes the five vectors the HMC accept test reads (``bk_mh_accept(BK_ACCEPT_HMC)``: lp_cur, kin0, lp_prop,
    kin1, log_u) BEFORE that test runs, and launches ``bk_energy_update`` -- the energy error ``d = (lp_prop - kin1) -
    (lp_cur - kin0)`` in the accept test's own roundings, divergent where d is NaN or ``d < -threshold``, and the energy
    ``E = -(selected joint log density)``, minus what ``sample()`` returns as logp -- then ``bk_divergence_capture``, which
    appends the columns of ``theta`` of the divergent chains to the store: in call order, by ascending chain within a call,
    the earliest ``capture`` entries kept and the rest counted (``seen``).  ``HMCDiag.track_energy()`` attaches one to a
    sampler.

    E-BFMI (Betancourt 2016) per chain is ``mean(diff(E)**2) / var(E)`` (ArviZ's estimator) over the chain's finite
    energies; ``ebfmi_pooled`` pools the chains, for runs of many short chains.  A non-finite energy is counted
    (``nonfinite_energies``) and skipped: the successive difference then spans the gap."""

    _VECTORS = ("mean_E", "m2_E", "last_E", "ssd", "trans", "cnt", "ndiv", "div_mask", "err")
    _STORE = ("theta_div", "chain", "draw", "err_store")

    def __init__(self, C: int, D=None, threshold: float = 1000.0, capture: int = 1024, chain_id0: int = 0, ops=None):
        self._ops = _ops(ops)
        dev = self._ops.device
        C, capture = int(C), int(capture)
        threshold = float(threshold)
        if C < 1:
            raise ValueError(f"EnergyDiagnostics requires C >= 1 chains, but C = {C}")
        if D is not None and int(D) < 1:
            raise ValueError(f"EnergyDiagnostics requires D >= 1 (or None: no states are captured), but D = {D}")
        if not (np.isfinite(threshold) and threshold > 0.0):
            raise ValueError(f"EnergyDiagnostics requires a finite threshold > 0, but threshold = {threshold}")
        if capture < 0:
            raise ValueError(f"EnergyDiagnostics requires capture >= 0, but capture = {capture}")
        self.C, self.D, self.threshold, self.chain_id0 = C, None if D is None else int(D), threshold, int(chain_id0)
        self.capture = capture if D is not None else 0
        f64, i64 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int64, device=dev)
        self.mean_E, self.m2_E, self.last_E, self.ssd, self.err = (torch.zeros(C, **f64) for _ in range(5))
        self.trans, self.cnt, self.ndiv = (torch.zeros(C, **i64) for _ in range(3))
        self.div_mask = torch.zeros(C, dtype=torch.uint8, device=dev)
        self._totals = torch.zeros(4, **i64)  # {transitions, divergent, NaN energy errors, non-finite energies}
        self._fill = torch.zeros(2, **i64)    # {stored, seen}
        cap = self.capture
        self.theta_div = torch.zeros((self.D, cap), **f64) if cap else None
        self.chain, self.draw = torch.zeros(cap, **i64), torch.zeros(cap, **i64)
        self.err_store = torch.zeros(cap, **f64)
        self._work = torch.zeros(self._ops.divergence_capture_work_elems(C), **i64)

    def update(self, lp_cur, kin0, lp_prop, kin1, log_u, theta=None, chain0=None) -> None:
        """One transition of every chain -- or, with ``chain0``, of the n = len(lp_cur) chains whose ids start at chain0
        (a column slice: the tile-major schedule).  theta: the [D, n] state the trajectories start from (None: divergences
        are counted, no state is captured).  Two entry points, three launches; no host read."""
        n = lp_cur.shape[0]
        c0 = 0 if chain0 is None else int(chain0) - self.chain_id0
        if c0 < 0 or c0 + n > self.C or (chain0 is None and n != self.C):
            raise ValueError(f"update: {n} chains from chain {self.chain_id0 + c0} do not lie inside this tracker's "
                             f"{self.C} chains from {self.chain_id0}")
        if theta is not None and self.theta_div is not None and tuple(theta.shape) != (self.D, n):
            raise ValueError(f"update: theta must be the [D, n] = ({self.D}, {n}) start state, got {tuple(theta.shape)}")
        sl = slice(c0, c0 + n)
        ops = self._ops
        ops.energy_update(lp_cur, kin0, lp_prop, kin1, log_u, self.threshold, self.mean_E[sl], self.m2_E[sl],
                          self.last_E[sl], self.ssd[sl], self.trans[sl], self.cnt[sl], self.ndiv[sl], self.div_mask[sl],
                          self.err[sl], self._totals)
        ops.divergence_capture(self.div_mask[sl], self.err[sl], self.trans[sl], theta, self.chain_id0 + c0, self.theta_div,
                               self.chain, self.draw, self.err_store, self._fill, self._work)

    # -- read-outs (none runs per draw) --------------------------------------------------------------------------------
    def _tot(self, group):
        return _gather_sum(self._totals, group).cpu()

    @property
    def transitions(self) -> int:
        """Transitions seen so far, over this rank's chains."""
        return int(self._totals[0].item())

    def divergences(self, group=None) -> int:
        return int(self._tot(group)[1])

    def divergence_rate(self, group=None) -> float:
        t = self._tot(group)
        return float(t[1]) / float(t[0]) if int(t[0]) else float("nan")

    def nan_transitions(self, group=None) -> int:
        """Transitions whose energy error was NaN (all of them are counted divergent)."""
        return int(self._tot(group)[2])

    def nonfinite_energies(self, group=None) -> int:
        """Transitions whose selected energy was not finite (left out of the energy statistics)."""
        return int(self._tot(group)[3])

    @property
    def divergences_per_chain(self) -> torch.Tensor:
        return self.ndiv.clone()

    @property
    def last_divergent(self) -> torch.Tensor:
        return self.div_mask.bool()

    @property
    def last_energy_error(self) -> torch.Tensor:
        return self.err.clone()

    def energy_mean(self) -> torch.Tensor:
        """[C]: the mean of each chain's finite energies (NaN where it has none)."""
        return torch.where(self.cnt > 0, self.mean_E, torch.full_like(self.mean_E, float("nan")))

    def energy_var(self) -> torch.Tensor:
        """[C]: their variance, ddof = 0 as in ``np.var`` (NaN where the chain has none)."""
        n = self.cnt.to(torch.float64)
        return torch.where(self.cnt > 0, self.m2_E / n.clamp(min=1.0), torch.full_like(self.m2_E, float("nan")))

    def ebfmi(self) -> torch.Tensor:
        """[C]: (ssd / (cnt - 1)) / (m2 / cnt) = mean(diff(E)**2) / var(E); NaN where cnt < 2 or m2 == 0."""
        n = self.cnt.to(torch.float64)
        ok = (self.cnt >= 2) & (self.m2_E != 0.0)
        num = self.ssd / (n - 1.0).clamp(min=1.0)
        den = torch.where(ok, self.m2_E / n.clamp(min=1.0), torch.ones_like(n))
        return torch.where(ok, num / den, torch.full_like(num, float("nan")))

    def ebfmi_pooled(self, group=None) -> float:
        """sum_c ssd / sum_c (cnt - 1) over the variance of ALL energies pooled, (sum_c m2 + sum_c cnt (mean_c - grand)^2) /
        sum_c cnt, over the chains of all ranks of ``group`` (two gathers: the sums, then the spread around the grand
        mean).  NaN with fewer than one successive difference or a pooled variance of zero."""
        n = self.cnt.to(torch.float64)
        pairs = (self.cnt - 1).clamp(min=0).to(torch.float64)
        mean = torch.where(self.cnt > 0, self.mean_E, torch.zeros_like(self.mean_E))
        s = _gather_sum(torch.stack([self.ssd.sum(), pairs.sum(), self.m2_E.sum(), n.sum(), (n * mean).sum()]), group)
        if float(s[1]) <= 0.0 or float(s[3]) <= 0.0:
            return float("nan")
        grand = s[4] / s[3]
        dev = mean - grand
        between = _gather_sum((n * dev * dev).sum().reshape(1), group)
        var = (float(s[2]) + float(between[0])) / float(s[3])
        return (float(s[0]) / float(s[1])) / var if var > 0.0 else float("nan")

    def divergent_states(self) -> dict:
        """The captured entries, oldest first: ``theta`` [n, D] (the states divergent trajectories started from), ``chain``
        (global chain ids), ``draw`` (the chain's transition number, 1-based), ``energy_error``; ``stored`` = n and ``seen``,
        the divergent transitions met (those past the capacity are counted only).  This rank's chains."""
        stored, seen = (int(v) for v in self._fill.cpu())
        th = None if self.theta_div is None else self.theta_div[:, :stored].t().contiguous()
        return {"theta": th, "chain": self.chain[:stored].clone(), "draw": self.draw[:stored].clone(),
                "energy_error": self.err_store[:stored].clone(), "stored": stored, "seen": seen}

    def _tensors(self):
        names = self._VECTORS + ("_totals", "_fill") + (self._STORE if self.theta_div is not None else self._STORE[1:])
        return {k.lstrip("_"): getattr(self, k) for k in names}

    def reset(self) -> None:
        """Forget every transition and empty the store; threshold and capacity stay."""
        for t in self._tensors().values():
            t.zero_()

    # checkpoint / resume: every tensor above; restored, the updates continue bit for bit
    def state_dict(self):
        sd = {k: t.detach().cpu().clone() for k, t in self._tensors().items()}
        sd["meta"] = {"C": self.C, "D": self.D, "threshold": self.threshold, "capture": self.capture,
                      "chain_id0": self.chain_id0}
        return sd

    def load_state_dict(self, sd):
        meta = sd["meta"]
        mine = {"C": self.C, "D": self.D, "threshold": self.threshold, "capture": self.capture, "chain_id0": self.chain_id0}
        for k, v in mine.items():
            if meta.get(k) != v:
                raise ValueError(f"checkpoint holds an energy tracker with {k} = {meta.get(k)!r}, this one has {k} = {v!r}")
        mine_t = self._tensors()
        for k, t in mine_t.items():
            if k not in sd or tuple(sd[k].shape) != tuple(t.shape) or sd[k].dtype != t.dtype:
                raise ValueError(f"checkpoint holds no {k!r} of shape {tuple(t.shape)} and dtype {t.dtype}")
        for k, t in mine_t.items():
            t.copy_(sd[k].to(t.device))


class DrawRecorder:
    """Draw storage for post-processing: the full series of a few tracked
    coordinates (and the returned log density) as ``[K, N, C]`` -- draw-major, chain-contiguous,
    the layout ``ess`` / ``rhat`` consume directly -- filled one draw at a time on the device.
    Storing every coordinate of every draw is rarely wanted at 65,536 chains x 1024 dims
    (512 MiB per draw); ``RunningMoments`` covers all coordinates in O(1) memory."""

    def __init__(self, dims: Sequence[int], capacity: int, chains: int, with_logp: bool = True, ops=None):
        self._ops = _ops(ops)
        self.dims = [int(d) for d in dims]
        self.with_logp = bool(with_logp)
        K = len(self.dims) + (1 if with_logp else 0)
        self.series = torch.empty((K, int(capacity), int(chains)), dtype=torch.float64, device=self._ops.device)
        self._dims_dev = torch.tensor(self.dims, dtype=torch.int32, device=self._ops.device)
        self.n = 0

    def _check_dims(self, D: int) -> None:
        """Tracked coordinates against the draw's D: negative indices count from the end (as ``theta[:, d]`` did),
        anything outside [-D, D) raises IndexError -- the kernel reads theta[dims[k] * ld + c] unchecked."""
        if getattr(self, "_dims_D", None) == D:
            return
        norm = []
        for d in self.dims:
            if not -D <= d < D:
                raise IndexError(f"tracked coordinate {d} is out of range for draws with {D} dimensions")
            norm.append(d + D if d < 0 else d)
        self._dims_dev = torch.tensor(norm, dtype=torch.int32, device=self._ops.device)
        self._dims_norm, self._dims_D = norm, D

    def record(self, theta, logp=None, layout=None) -> None:
        """theta: the (C, D) draw returned by ``sample()`` or the [D, C] buffer behind it (told apart by shape, a
        square draw by its strides or by ``layout`` = "cd" / "dc": diagnostics._as_dc); logp: its (C,) log density.
        One launch (bk_record_series) for all tracked series."""
        if self.n >= self.series.shape[1]:
            raise IndexError("DrawRecorder is full")
        C = self.series.shape[2]
        if theta.dim() != 2:
            raise ValueError(f"expected a 2-D draw, got shape {tuple(theta.shape)}")
        if layout == "dc" or (layout is None and theta.shape[1] == C and theta.shape[0] != C):
            D = theta.shape[0]
        else:
            D = theta.shape[1]
        t = _as_dc(theta, D, C, layout)
        self._check_dims(D)
        lp = None
        if self.with_logp:
            lp = logp if (logp.dtype == torch.float64 and logp.is_contiguous()) else logp.to(torch.float64).contiguous()
        if (C == 1 or t.stride(1) == 1) and t.dtype == torch.float64:
            self._ops.record_series(t, self._dims_dev, lp, self.series, self.n)
        else:  # a draw in some other layout / dtype: one strided copy per series
            for k, d in enumerate(self._dims_norm):
                self.series[k, self.n].copy_(t[d])
            if self.with_logp:
                self.series[-1, self.n].copy_(logp)
        self.n += 1

    def _record_dev(self, theta_dc, logp, row_dev, row_offset) -> None:
        """record() as a part of a sampler's draw (DrGhmcDiag.attach): row = row_dev[0] - row_offset, read on the
        device; the caller keeps self.n in step."""
        self._check_dims(theta_dc.shape[0])
        self._ops.record_series_dev(theta_dc, self._dims_dev, logp if self.with_logp else None, self.series, row_dev,
                                    row_offset)

    def _record_job(self, D, logp, row_offset):
        """_record_dev(...) as the tracked-series part of a job the NEXT draw's generator launch carries along."""
        self._check_dims(D)
        return (self._dims_dev, logp if self.with_logp else None, self.series, row_offset)

    def names(self):
        return [f"theta[{d}]" for d in self.dims] + (["logp"] if self.with_logp else [])

    def view(self, k: int) -> torch.Tensor:
        """[n, C] series of tracked quantity k."""
        return self.series[k, : self.n]

    def ess(self) -> torch.Tensor:
        """[K, C] effective sample sizes (ess.py:52-69) of every tracked series of every chain."""
        return torch.stack([ess(self.view(k), ops=self._ops) for k in range(self.series.shape[0])])

    def rhat(self, group=None) -> np.ndarray:
        """R-hat (rhat.py:111-171) of every tracked quantity over all chains (and ranks)."""
        return np.array([rhat(self.view(k), ops=self._ops, group=group) for k in range(self.series.shape[0])])

    def nested_rhat(self, chains_per_superchain: int, group=None) -> np.ndarray:
        """Nested R-hat of every tracked quantity over superchains of ``chains_per_superchain`` consecutive chains (of
        all ranks), from the stored series; works from one recorded draw on."""
        if self.n < 1:
            raise ValueError("nested_rhat requires len(chain) >= 1 for every chain in chains")
        series = [self.view(k) for k in range(self.series.shape[0])]
        return _nested_rhat_of_series(series, int(chains_per_superchain), self._ops, group)

    def summary(self, group=None) -> dict:
        """Per tracked quantity (arrays in ``names()`` order): ``name``, ``mean`` and ``sd`` (ddof = 1) of the split set,
        ``mcse_mean``, ``ess_bulk``, ``ess_tail`` and ``rhat`` (= ``rank_normalized_rhat(view(k))``), over all chains of
        all ranks.  Each value equals the standalone function's.  For an even number of draws the pooled draws of a
        quantity are sorted once, for bulk ESS, the quantiles of tail ESS and R-hat alike."""
        K = self.series.shape[0]
        cols = {f: np.empty(K) for f in ("mean", "sd", "mcse_mean", "ess_bulk", "ess_tail", "rhat")}
        for k in range(K):
            for f, v in _multi_summary(self.view(k), self._ops, group).items():
                cols[f][k] = v
        return {"name": self.names(), **cols}

    def state_dict(self):
        return {"series": self.series[:, : self.n].cpu().clone(), "dims": self.dims, "with_logp": self.with_logp,
                "n": self.n}

    def load_state_dict(self, sd):
        if list(sd["dims"]) != self.dims or bool(sd["with_logp"]) != self.with_logp:
            raise ValueError(f"checkpoint tracks dims {sd['dims']} (logp: {sd['with_logp']}), this recorder {self.dims} "
                             f"(logp: {self.with_logp})")
        ser = sd["series"]
        if ser.shape[0] != self.series.shape[0] or ser.shape[2] != self.series.shape[2] or ser.shape[1] > self.series.shape[1]:
            raise ValueError(f"checkpoint series {tuple(ser.shape)} does not fit the recorder {tuple(self.series.shape)}")
        self.n = int(ser.shape[1])
        self.series[:, : self.n].copy_(ser.to(self.series.device))


class DrawStore:
    """Chunked draw storage: every coordinate of every draw of this rank's chains, as
    fixed-size chunks ``[draws, D, C]`` -- draw-major, chain-contiguous: the series of coordinate d
    of a chunk is the strided view ``chunk[:, d, :]`` (``[n, C]``, chains contiguous), which ``ess`` /
    ``rhat`` / ``autocorr`` consume as it is, no reshaping.  Draws are staged in a device buffer and
    written one ``chunk_#####.npy`` file per full chunk (plus ``meta.json``); one directory per rank.

        store = DrawStore.create(path, D, C, chunk=64)        # writer
        store.append(theta)  ...  store.close()
        store = DrawStore.open(path)                           # reader
        x = store.series(d)        # [N, C] device tensor      r = rhat(x); e = ess(x)

    A store can be re-opened for appending (``DrawStore.create(..., resume=True)``): with the
    sampler's ``state_dict`` this makes a run restartable at any chunk boundary or in between (the
    partial chunk is kept in ``state_dict()`` of the store).
    """

    def __init__(self, path, D, C, chunk, ops, chunks):
        import os

        self.path, self.D, self.C, self.chunk = str(path), int(D), int(C), int(chunk)
        self._ops = _ops(ops)
        self._os = os
        self._chunks = list(chunks)  # draws per completed chunk file
        self._buf_t = None           # [chunk, D, C] device staging buffer: allocated by the first append()
        self._fill = 0

    @property
    def _buf(self):
        # a reader (DrawStore.open) never appends and never pays for the staging buffer: at config-3
        # size and chunk = 64 it would be 34 GB of HBM
        if self._buf_t is None:
            self._buf_t = torch.empty((self.chunk, self.D, self.C), dtype=torch.float64, device=self._ops.device)
        return self._buf_t

    # -- writer -----------------------------------------------------------------------------------
    @classmethod
    def create(cls, path, D, C, chunk=64, ops=None, resume=False):
        import json
        import os

        os.makedirs(path, exist_ok=True)
        meta = os.path.join(path, "meta.json")
        chunks = []
        if os.path.exists(meta):
            if not resume:
                raise FileExistsError(f"{path} already holds a draw store (pass resume=True to append)")
            with open(meta) as f:
                m = json.load(f)
            if (m["D"], m["C"], m["chunk"]) != (int(D), int(C), int(chunk)):
                raise ValueError(f"{path} holds a store of D={m['D']}, C={m['C']}, chunk={m['chunk']}")
            chunks = m["chunks"]
        st = cls(path, D, C, chunk, ops, chunks)
        st._write_meta()
        return st

    def _write_meta(self):
        import json

        with open(self._os.path.join(self.path, "meta.json"), "w") as f:
            json.dump({"D": self.D, "C": self.C, "chunk": self.chunk, "chunks": self._chunks, "dtype": "float64",
                       "layout": "[draw, D, C], C contiguous"}, f)

    def append(self, theta, layout=None) -> None:
        """theta: the sampler's draw -- the (C, D) view returned by ``sample()`` or a [D, C] buffer (told
        apart by shape; for C == D by strides, or say ``layout="cd"`` / ``"dc"``)."""
        t = _as_dc(theta, self.D, self.C, layout)
        self._buf[self._fill].copy_(t)
        self._fill += 1
        if self._fill == self.chunk:
            self._flush()

    def _flush(self):
        if self._fill == 0:
            return
        arr = self._buf[: self._fill].cpu().numpy()
        np.save(self._os.path.join(self.path, "chunk_%05d.npy" % len(self._chunks)), arr)
        self._chunks.append(int(self._fill))
        self._fill = 0
        self._write_meta()

    def close(self):
        self._flush()

    def state_dict(self):
        """The not yet written part of the current chunk (what a checkpoint must carry besides the files)."""
        part = self._buf[: self._fill].cpu().clone() if self._fill else torch.empty((0, self.D, self.C), dtype=torch.float64)
        return {"chunks": list(self._chunks), "partial": part}

    def load_state_dict(self, sd, truncate=False):
        """Rewind the store to a checkpoint.  Chunk files written AFTER the checkpoint belong to draws the
        resumed run will produce again: with ``truncate=True`` they are deleted, otherwise they are kept on
        disk under ``superseded_<k>_chunk_#####.npy`` (never read again by this store) -- nothing is removed
        unless asked for."""
        if len(sd["chunks"]) > len(self._chunks) or sd["chunks"] != self._chunks[: len(sd["chunks"])]:
            raise ValueError("the checkpoint refers to chunk files this store does not hold")
        for k in range(len(sd["chunks"]), len(self._chunks)):
            f = self._os.path.join(self.path, "chunk_%05d.npy" % k)
            if truncate:
                self._os.remove(f)
            else:
                gen = 0
                while self._os.path.exists(self._os.path.join(self.path, "superseded_%d_chunk_%05d.npy" % (gen, k))):
                    gen += 1
                self._os.replace(f, self._os.path.join(self.path, "superseded_%d_chunk_%05d.npy" % (gen, k)))
        self._chunks = list(sd["chunks"])
        part = sd["partial"]
        self._fill = int(part.shape[0])
        if self._fill:
            self._buf[: self._fill].copy_(part.to(self._ops.device))
        self._write_meta()

    # -- reader -----------------------------------------------------------------------------------
    @classmethod
    def open(cls, path, ops=None):
        import json
        import os

        with open(os.path.join(path, "meta.json")) as f:
            m = json.load(f)
        return cls(path, m["D"], m["C"], m["chunk"], ops, m["chunks"])

    @property
    def draws(self) -> int:
        return sum(self._chunks) + self._fill

    def chunk_array(self, k) -> np.ndarray:
        """Chunk k as a memory-mapped [n, D, C] array."""
        return np.load(self._os.path.join(self.path, "chunk_%05d.npy" % k), mmap_mode="r")

    def series(self, d: int) -> torch.Tensor:
        """All draws of coordinate d: [N, C] device tensor (each chunk contributes its [n, C] slice; only
        that slice is read from disk)."""
        N = self.draws
        out = torch.empty((N, self.C), dtype=torch.float64, device=self._ops.device)
        pos = 0
        for k, n in enumerate(self._chunks):
            out[pos:pos + n].copy_(torch.from_numpy(np.ascontiguousarray(self.chunk_array(k)[:, d, :])))
            pos += n
        if self._fill:
            out[pos:pos + self._fill].copy_(self._buf[: self._fill, d, :])
        return out

    def rhat(self, dims=None, group=None) -> np.ndarray:
        dims = range(self.D) if dims is None else dims
        return np.array([rhat(self.series(d), ops=self._ops, group=group) for d in dims])

    def ess(self, dims=None) -> torch.Tensor:
        dims = range(self.D) if dims is None else dims
        return torch.stack([ess(self.series(d), ops=self._ops) for d in dims])


# ---------------------------------------------------------------------------------------------
# helpers for the reference-style inputs
# ---------------------------------------------------------------------------------------------
def _is_matrix(x) -> bool:
    return isinstance(x, torch.Tensor) and x.dim() == 2


def _pack_chains(chains: Sequence, ops):
    """Sequence of (possibly ragged) 1-D chains -> ([Nmax, M] device tensor, lengths)."""
    arrs = [np.asarray(c, dtype=np.float64).reshape(-1) for c in chains]
    lens = np.array([a.shape[0] for a in arrs], dtype=np.int32)
    nmax = int(lens.max()) if len(arrs) else 0
    host = np.zeros((max(nmax, 1), len(arrs)), dtype=np.float64)
    for j, a in enumerate(arrs):
        host[: a.shape[0], j] = a
    return torch.from_numpy(host).to(ops.device), lens


def _rhat_of_columns(x, lens, ops, group=None):
    """R-hat of the chains stored as columns of x (lens None = all rows)."""
    N, M = x.shape
    dev = x.device
    mean = torch.empty((1, M), dtype=torch.float64, device=dev)
    var = torch.empty((1, M), dtype=torch.float64, device=dev)
    lt = None if lens is None else torch.from_numpy(np.asarray(lens, dtype=np.int32)).to(dev)
    ops.chain_mean_var(x, lt, mean[0], var[0])
    # reuse the per-dimension partial-sum kernel with D = 1 (n = 2 makes M2/(n-1) = var)
    part = torch.zeros(4, dtype=torch.float64, device=dev)
    ops.rhat_partials(mean, var, 2, None, part)
    part[3] = float(M)
    len_sum = torch.tensor([float(N * M) if lens is None else float(np.sum(lens))], dtype=torch.float64, device=dev)
    tot = _gather_sum(torch.cat([part, len_sum]), group)
    Mt = float(tot[3].item())
    if Mt < 2:  # rhat.py:159-160, over all ranks' chains
        raise ValueError(f"rhat requires len(chains) >= 2, but len(chains) = {int(Mt)}")
    centre = (tot[0:1] / Mt).contiguous()
    part2 = torch.zeros(4, dtype=torch.float64, device=dev)
    ops.rhat_partials(mean, var, 2, centre, part2)
    tot2 = _gather_sum(part2, group)
    nbar = float(tot[4].item()) / Mt
    var_means = float(tot2[2].item()) / (Mt - 1.0)
    mean_vars = float(tot[1].item()) / Mt
    return np.float64(np.sqrt((nbar - 1.0) / nbar + var_means / mean_vars))


# ---------------------------------------------------------------------------------------------
# rhat.py
# ---------------------------------------------------------------------------------------------
def rhat(chains, *, ops=None, group=None):
    """Potential scale reduction factor, bayes_kit/rhat.py:111-171.

    ``chains``: a sequence of 1-D chains (ragged allowed) or a device tensor [N, C].  With a
    process group, ``chains`` is this rank's shard and the statistic is over all ranks.
    """
    ops = _ops(ops)
    world = dist.get_world_size(group) if (dist.is_available() and dist.is_initialized()) else 1
    if _is_matrix(chains):
        N, M = chains.shape
        if world == 1 and M < 2:
            raise ValueError(f"rhat requires len(chains) >= 2, but len(chains) = {M}")
        if N < 2:
            raise ValueError("rhat requires len(chain) >= 2 for every chain in chains")
        x = chains if chains.stride(1) == 1 else chains.contiguous()
        return _rhat_of_columns(x, None, ops, group)
    if world == 1 and len(chains) < 2:
        raise ValueError(f"rhat requires len(chains) >= 2, but {len(chains) = }")
    if not all(len(chain) >= 2 for chain in chains):
        raise ValueError("rhat requires len(chain) >= 2 for every chain in chains")
    x, lens = _pack_chains(chains, ops)
    return _rhat_of_columns(x, lens, ops, group)


def split_chains(chains):
    """bayes_kit/rhat.py:9-24 (host-side index arithmetic only: no numerics involved)."""
    return [arr for chain in chains for arr in np.array_split(chain, 2)]


def split_rhat(chains, *, ops=None, group=None):
    """bayes_kit/rhat.py:174-202: R-hat of the chains split in half (first half one longer
    for odd lengths)."""
    ops = _ops(ops)
    if _is_matrix(chains):
        N, M = chains.shape
        x = chains if chains.stride(1) == 1 else chains.contiguous()
        h = (N + 1) // 2
        if N - h < 2:
            raise ValueError("rhat requires len(chain) >= 2 for every chain in chains")
        halves = torch.zeros((h, 2 * M), dtype=torch.float64, device=x.device)
        halves[:, :M] = x[:h]
        halves[: N - h, M:] = x[h:]
        lens = np.concatenate([np.full(M, h), np.full(M, N - h)]).astype(np.int32)
        return _rhat_of_columns(halves, lens, ops, group)
    return rhat(split_chains(chains), ops=ops, group=group)


def _canonical_keys(flat: torch.Tensor) -> torch.Tensor:
    """Sort keys whose RADIX order (the order of the raw bit patterns, which is what bk_sort_by_key and the
    splitter search see) is numpy's comparison order (rhat.py:51-52): -0.0 becomes +0.0, so that the two
    zeros tie and rank in pooled order, and every NaN becomes the positive quiet NaN, which sorts last
    as in ``np.argsort`` (a sign-bit NaN would sort first)."""
    flat = flat + 0.0  # (-0.0) + (+0.0) = +0.0 in round-to-nearest; every other value unchanged
    return torch.where(torch.isnan(flat), torch.full_like(flat, float("nan")), flat)


def _ranks_pooled(flat: torch.Tensor, ops) -> torch.Tensor:
    """Ascending 1-based ranks of the pooled draws (rhat.py:51-52: argsort().argsort() + 1).
    Ties get distinct consecutive ranks; numpy leaves their order to its sort, here it is the
    order of appearance (stable sort).  bk_sort_by_key + bk_scatter_ranks."""
    n = flat.numel()
    idx = torch.arange(n, dtype=torch.int64, device=flat.device)
    _, payload = ops.sort_by_key(_canonical_keys(flat).contiguous(), idx)
    ranks = torch.empty_like(flat)
    ops.scatter_ranks(payload, 0.0, ranks)
    return ranks


SAMPLES_PER_RANK = 64  # regular samples each rank contributes per destination bucket


def _ranks_pooled_across_ranks(x: torch.Tensor, ops, group=None) -> torch.Tensor:
    """Global pooled ranks of this rank's [N, C_local] shard WITHOUT replicating the draws: a sample
    sort.  Pooled order = chain-major over all ranks' chains in rank order (what rank_chains sees
    when handed every chain); equal values rank in that order.

      1. local stable sort of (value, global flat index)                       bk_sort_by_key
      2. 64*world regular samples per rank -> all_gather -> world-1 splitters
      3. bucket boundaries by binary search (bk_count_below); bucket k belongs to rank k
      4. all_to_all of the buckets (values + indices): S_local*16 bytes sent per rank, over RCCL/xGMI,
         instead of S_total*8 bytes RECEIVED by every rank
      5. owner: stable sort of what arrived (sorted runs in source-rank order: ties stay in global
         order); rank of position j = (sizes of the lower buckets) + j + 1      bk_scatter_ranks
      6. ranks travel back to the elements' home ranks (all_to_all)
    Returns the ranks as doubles, shaped like x."""
    world, me = dist.get_world_size(group), dist.get_rank(group)
    N, C = x.shape
    dev = x.device
    flat = _canonical_keys(x.t().contiguous().reshape(-1))
    S_local = flat.numel()
    sizes = _all_gather_counts(S_local, dev, group)
    ends = torch.cumsum(torch.tensor(sizes, dtype=torch.int64, device=dev), 0)
    first = int(ends[me].item()) - S_local
    gidx = torch.arange(S_local, dtype=torch.int64, device=dev) + first
    keys, pay = ops.sort_by_key(flat, gidx)
    # 2. splitters
    s = SAMPLES_PER_RANK * world
    samp = torch.full((s,), float("inf"), dtype=torch.float64, device=dev)
    if S_local > 0:
        k = min(s, S_local)
        pos = ((torch.arange(k, dtype=torch.float64, device=dev) + 0.5) * (S_local / k)).to(torch.int64).clamp_(max=S_local - 1)
        samp[:k] = keys[pos]
    parts = _bkdist.all_gather(samp, group)
    cat = torch.cat(parts)                                  # world*s values: tiny
    allsamp, _ = ops.sort_by_key(cat, torch.arange(cat.numel(), dtype=torch.int64, device=dev))
    nreal = int(torch.isfinite(allsamp).sum().item())
    cut_pos = [(nreal * (r + 1)) // world for r in range(world - 1)]
    splitters = allsamp[torch.tensor(cut_pos, dtype=torch.int64, device=dev).clamp_(max=max(nreal - 1, 0))]
    # 3. buckets (values equal to a splitter go to the bucket above it, on every rank alike)
    cuts = ops.count_below(keys, splitters.contiguous()) if world > 1 else torch.empty(0, dtype=torch.int64, device=dev)
    bounds = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), cuts, torch.tensor([S_local], dtype=torch.int64, device=dev)])
    bounds = torch.cummax(bounds, 0).values                # (monotone even if splitters repeat)
    send_counts = (bounds[1:] - bounds[:-1])
    recv_counts = torch.empty_like(send_counts)
    _bkdist.all_to_all_single(recv_counts, send_counts, group=group)
    sc, rc = send_counts.tolist(), recv_counts.tolist()
    # 4. the buckets travel
    R = sum(rc)
    rk = torch.empty(R, dtype=torch.float64, device=dev)
    rp = torch.empty(R, dtype=torch.int64, device=dev)
    _bkdist.all_to_all_single(rk, keys, rc, sc, group=group)
    _bkdist.all_to_all_single(rp, pay, rc, sc, group=group)
    # 5. ranks inside my bucket
    _, ps = ops.sort_by_key(rk, rp)
    bsz = _all_gather_counts(R, dev, group)
    my_base = float(sum(bsz[:me]))
    # 6. back home: group the sorted positions by the rank that owns the element
    owner = torch.searchsorted(ends, ps, right=True)
    _, order = ops.sort_by_key(owner.to(torch.float64), torch.arange(R, dtype=torch.int64, device=dev))
    back_idx = ps[order].contiguous()
    back_rank = (my_base + (order + 1).to(torch.float64)).contiguous()
    hi = torch.empty(S_local, dtype=torch.int64, device=dev)
    hr = torch.empty(S_local, dtype=torch.float64, device=dev)
    _bkdist.all_to_all_single(hi, back_idx, sc, rc, group=group)
    _bkdist.all_to_all_single(hr, back_rank, sc, rc, group=group)
    ranks = torch.empty(S_local, dtype=torch.float64, device=dev)
    ranks[hi - first] = hr
    return ranks.reshape(C, N).t()


def _pooled(chains, ops):
    """-> (flat chain-major device vector, list of lengths)."""
    if _is_matrix(chains):
        N, M = chains.shape
        return chains.t().contiguous().reshape(-1), [N] * M
    arrs = [np.asarray(c, dtype=np.float64).reshape(-1) for c in chains]
    flat = np.concatenate(arrs) if arrs else np.zeros(0)
    return torch.from_numpy(flat).to(ops.device), [a.shape[0] for a in arrs]


def rank_chains(chains, *, ops=None):
    """bayes_kit/rhat.py:27-59: chains with every value replaced by its pooled rank."""
    if len(chains) == 0:
        return chains
    ops = _ops(ops)
    flat, lens = _pooled(chains, ops)
    ranks = _ranks_pooled(flat, ops)
    if _is_matrix(chains):
        return ranks.reshape(len(lens), lens[0]).t()
    out, pos = [], 0
    r = ranks.cpu().numpy()
    for n in lens:
        out.append(r[pos:pos + n])
        pos += n
    return out


def rank_normalize_chains(chains, *, ops=None):
    """bayes_kit/rhat.py:62-108: Phi^-1((rank - 0.325) / (S - 0.25)) (the offset the reference
    actually uses, not the 3/8 of its docstring)."""
    ops = _ops(ops)
    flat, lens = _pooled(chains, ops)
    S = flat.numel()
    z = torch.empty_like(flat)
    ops.rank_normalize(_ranks_pooled(flat, ops), float(S), z)
    if _is_matrix(chains):
        return z.reshape(len(lens), lens[0]).t().contiguous()
    out, pos = [], 0
    zz = z.cpu().numpy()
    for n in lens:
        out.append(zz[pos:pos + n])
        pos += n
    return out


def _all_gather_counts(n: int, device, group=None):
    """Every rank's value of the integer n, in rank order (dist.shard hands the remainder of an
    uneven split to the first ranks, so shard widths may differ by one)."""
    world = dist.get_world_size(group)
    mine = torch.tensor([int(n)], dtype=torch.int64, device=device)
    return [int(p.item()) for p in _bkdist.all_gather(mine, group)]


def _all_gather_columns(x: torch.Tensor, group=None):
    """[N, C_local] on every rank -> ([N, C_total] in rank order, first column of this rank).
    C_local may differ between ranks: shards are padded to the widest for the collective and
    the padding is dropped afterwards."""
    world = dist.get_world_size(group)
    counts = _all_gather_counts(x.shape[1], x.device, group)
    cmax = max(counts)
    send = x.contiguous()
    if x.shape[1] != cmax:
        send = torch.zeros((x.shape[0], cmax), dtype=x.dtype, device=x.device)
        send[:, : x.shape[1]] = x
    parts = _bkdist.all_gather(send, group)
    full = torch.cat([p[:, :c] for p, c in zip(parts, counts)], dim=1)
    return full, sum(counts[: dist.get_rank(group)])


def rank_normalized_rhat(chains, *, ops=None, group=None):
    """bayes_kit/rhat.py:205-236: split R-hat of the rank-normalised chains.

    Across ranks (an [N, C_local] shard per rank) the ranks are global: they come from a sample
    sort over the process group (_ranks_pooled_across_ranks: each rank sends and receives its own
    share of the draws once, nothing is replicated); every rank then turns its own chains' ranks
    into normal scores and joins the usual cross-rank split R-hat."""
    multi = _bkdist.collectives_active(group)
    if not multi:
        return split_rhat(rank_normalize_chains(chains, ops=ops), ops=ops, group=group)  # (a one-rank group stays local)
    if not _is_matrix(chains):
        raise ValueError("across ranks rank_normalized_rhat takes this rank's [N, C_local] device tensor")
    ops = _ops(ops)
    ranks = _ranks_pooled_across_ranks(chains, ops, group).contiguous()
    S = float(sum(_all_gather_counts(chains.numel(), chains.device, group)))
    z = torch.empty_like(ranks)
    ops.rank_normalize(ranks, S, z)
    return split_rhat(z, ops=ops, group=group)


# ---------------------------------------------------------------------------------------------
# autocorr.py / iat.py / ess.py
# ---------------------------------------------------------------------------------------------
def _series(chain, ops):
    """-> ([N, C] device tensor, was_1d)."""
    if _is_matrix(chain):
        return (chain if chain.stride(1) == 1 else chain.contiguous()), False
    a = np.asarray(chain, dtype=np.float64).reshape(-1)
    return torch.from_numpy(a.copy()).to(ops.device).reshape(-1, 1), True


def _len(chain) -> int:
    return chain.shape[0] if _is_matrix(chain) else len(chain)


# Chains up to FFT_MIN_DRAWS draws: series staged in LDS, direct lag sums (N steps per 64 lags, only the lags the
# Geyer truncation needs).  Longer chains: the reference's own FFT formulation (autocorr.py:26-32), O(N log N)
# per chain, by the library's Stockham passes over the [N, C] layout (bk_autocorr_fft: one lane per pair of
# chains, two real series per complex transform), followed by the scan kernel (bk_iat_from_acor) -- the direct
# sums are O(N^2 / 64) for ALL lags.
FFT_MIN_DRAWS = 16384
# autocorr() wants ALL lags, which the direct sums pay O(N^2 / 64) for: the FFT is ahead from 256 draws on (4,096 chains:
# 0.10 vs 0.13 ms at 256 draws, 0.40 vs 0.66 at 2,048, 0.55 vs 3.2 at 8,192; tools/attic/autocorr_crossover.py)
AUTOCORR_FFT_MIN_DRAWS = 256
_FFT_SCRATCH_BYTES = 2 << 30  # chains per FFT batch are chosen to keep the two complex scratch arrays below this


def _fft_batch(N: int, C: int, ops) -> int:
    """Chains per bk_autocorr_fft call for chains of N draws."""
    size = 1 << int(np.ceil(np.log2(2 * N - 1)))
    block = max(128, (_FFT_SCRATCH_BYTES // (size * 16)) // 128 * 128)  # (2 buffers x size x block/2 x 16 B)
    need = getattr(ops, "autocorr_fft_work_bytes", None)
    while need is not None and block > 128 and need(N, min(block, C)) > 2 * _FFT_SCRATCH_BYTES:
        block = max(128, block // 2 // 128 * 128)  # (the plan pads its rows: size the batch by what it will really take)
    return block


def _autocorr_fft(x: torch.Tensor, ops) -> torch.Tensor:
    """autocorr.py:23-33 for every column of x [N, C]."""
    N, C = x.shape
    block = _fft_batch(N, C, ops)
    out = torch.empty_like(x)
    for c0 in range(0, C, block):
        ops.autocorr_fft(x[:, c0:c0 + block], out[:, c0:c0 + block])
    return out


def autocorr(chain, *, ops=None):
    """Autocorrelation at all lags, bayes_kit/autocorr.py:6-33."""
    if _len(chain) < 2:
        raise ValueError(f"autocorr requires len(chain) >= 2, but {len(chain)=}")
    ops = _ops(ops)
    x, one = _series(chain, ops)
    if x.shape[0] >= AUTOCORR_FFT_MIN_DRAWS:
        out = _autocorr_fft(x, ops)
    else:
        out = torch.empty_like(x)
        ops.autocorr(x, out)
    return out[:, 0].cpu().numpy() if one else out


def _iat_ess(chain, estimator, want, ops):
    ops = _ops(ops)
    x, one = _series(chain, ops)
    N, C = x.shape
    ess_out = torch.empty(C, dtype=torch.float64, device=x.device)
    iat_out = torch.empty(C, dtype=torch.float64, device=x.device)
    if N >= FFT_MIN_DRAWS:
        ops.iat_from_acor(_autocorr_fft(x, ops), estimator, ess_out, iat_out)
    else:
        ops.ess(x, estimator, ess_out, iat_out)
    r = ess_out if want == "ess" else iat_out
    return np.float64(r[0].item()) if one else r


def iat_ipse(chain, *, ops=None):
    """bayes_kit/iat.py:46-92."""
    if _len(chain) < 4:
        raise ValueError(f"ess requires len(chains) >= 4, but {len(chain)=}")
    return _iat_ess(chain, 1, "iat", ops)


def iat_imse(chain, *, ops=None):
    """bayes_kit/iat.py:95-135."""
    if _len(chain) < 4:
        raise ValueError(f"iat requires len(chains) >=4, but {len(chain) = }")
    return _iat_ess(chain, 0, "iat", ops)


def iat(chain, *, ops=None):
    """bayes_kit/iat.py:138-156."""
    return iat_imse(chain, ops=ops)


def ess_ipse(chain, *, ops=None):
    """bayes_kit/ess.py:5-21."""
    if _len(chain) < 4:
        raise ValueError(f"ess_ipse(chain) requires len(chain) >= 4, but {len(chain)=}")
    return _iat_ess(chain, 1, "ess", ops)


def ess_imse(chain, *, ops=None):
    """bayes_kit/ess.py:24-49."""
    if _len(chain) < 4:
        raise ValueError(f"ess_imse(chain) requires len(chain) >=4, but {len(chain) = }")
    return _iat_ess(chain, 0, "ess", ops)


def ess(chain, *, ops=None):
    """bayes_kit/ess.py:52-69."""
    if _len(chain) < 4:
        raise ValueError(f"ess(chain) requires len(chain) >=4, but {len(chain) = }")
    return _iat_ess(chain, 0, "ess", ops)


# ---------------------------------------------------------------------------------------------
# multi-chain ESS: bulk / tail / quantile / mean ESS and the MCSE of the mean
# ---------------------------------------------------------------------------------------------
# Vehtari, Gelman, Simpson, Carpenter and Buerkner (2021), "Rank-normalization, folding, and localization: an improved
# R-hat for assessing convergence of MCMC", Bayesian Analysis 16(2), sec. 3.2, eqs. 10-11, with Geyer's initial monotone
# sequence: the estimator of Stan's compute_effective_sample_size and posterior's ess_rfun.  Where those two differ in
# scaling or edge cases, the text below rules.
#
# Split set: n = N // 2; column c gives the chains x[:n, c] and x[N - n:, c] (views; an odd N drops its middle row),
# M = 2 * C_total.  Per split chain m: xbar_m, gamma_{m,t} = (1/n) sum_{i < n - t} (x_{m,i} - xbar_m)(x_{m,i+t} - xbar_m).
#   W = mean_m(gamma_{m,0}) * n / (n - 1),  var_plus = W (n - 1) / n + var_m(xbar_m, ddof=1),
#   Gamma_t = mean_m(gamma_{m,t}),  rho(t) = 1 - (W - Gamma_t) / var_plus,
# then _geyer_tau below, ESS = M n / tau.
#
# The device computes the moments (bk_ess_split_moments, bk_ess_between_sq) and Gamma in lag rounds (bk_ess_lag_sums:
# the first 64 lags, then doubling, until the scan stops; halves too long for LDS: bk_autocorr_fft + bk_ess_acov_sums,
# all lags in one round); each round is one small device-to-host copy and, across ranks, one gather_sum.
ESS_FIRST_LAGS = 64


def _geyer_tau(Gamma, W, var_plus, M, n):
    """(tau, max_t) of the multi-chain estimator from Gamma[t] = mean over the split chains of gamma_{m,t}, t < len(Gamma);
    None when the scan needs a lag beyond len(Gamma) (len(Gamma) >= n - 2 always suffices).  tau has the floor
    1 / log10(M n) (antithetic chains)."""
    G = np.asarray(Gamma, dtype=np.float64)
    rho = np.zeros(n)
    rho[0] = 1.0
    r_even = 1.0
    r_odd = 1.0 - (W - G[1]) / var_plus
    rho[1] = r_odd
    t = 0
    while t < n - 5 and not np.isnan(r_even + r_odd) and r_even + r_odd > 0:
        t += 2
        if t + 1 >= G.shape[0]:
            return None
        r_even = 1.0 - (W - G[t]) / var_plus
        r_odd = 1.0 - (W - G[t + 1]) / var_plus
        if r_even + r_odd >= 0:
            rho[t] = r_even
            rho[t + 1] = r_odd
    max_t = t
    if r_even > 0:
        rho[max_t] = r_even
    t = 0
    while t <= max_t - 4:  # Geyer's initial monotone sequence
        t += 2
        if rho[t] + rho[t + 1] > rho[t - 2] + rho[t - 1]:
            rho[t] = rho[t + 1] = (rho[t - 2] + rho[t - 1]) / 2
    tau = max(-1.0 + 2.0 * float(np.sum(rho[0:max_t])) + float(rho[max_t]), 1.0 / np.log10(M * n))
    return tau, max_t


def _quantile_indices(S: int, prob: float):
    """np.quantile(a, prob) of S sorted values, method "linear": (virtual index, lower index, upper index)."""
    vi = (S - 1) * float(prob)
    if vi >= S - 1:
        return vi, S - 1, S - 1
    i0 = int(np.floor(vi))
    return vi, i0, i0 + 1


def _quantile_lerp(a: float, b: float, vi: float, i0: int) -> float:
    """NumPy's _lerp(a, b, vi - i0), its t >= 0.5 branch included: bit for bit np.quantile's value."""
    t = vi - i0
    diff = b - a
    r = a + diff * t
    if t >= 0.5:
        r = b - diff * (1 - t)
    return r


def _split_quantiles(order_stats, S: int, probs):
    """np.quantile(split_pooled, p) for p in probs; order_stats(list of 0-based sorted positions) -> their values."""
    idx = [_quantile_indices(S, p) for p in probs]
    vals = np.asarray(order_stats([i for _, i0, i1 in idx for i in (i0, i1)]), dtype=np.float64)
    return [_quantile_lerp(float(vals[2 * j]), float(vals[2 * j + 1]), vi, i0) for j, (vi, i0, _) in enumerate(idx)]


def _multi_input(chains, ops, name, group):
    """-> ([N, C_local] float64 device tensor with unit column stride, C_total).  Ranks with different N raise on every
    rank before any other collective."""
    if _is_matrix(chains):
        x = chains if chains.dtype == torch.float64 else chains.to(torch.float64)
        if x.shape[1] > 1 and x.stride(1) != 1:
            x = x.contiguous()
    else:
        arrs = [np.asarray(c, dtype=np.float64).reshape(-1) for c in chains]
        lens = [a.shape[0] for a in arrs]
        if len(set(lens)) > 1:
            raise ValueError(f"{name} requires chains of equal length, got lengths {lens}")
        host = np.stack(arrs, axis=1) if arrs else np.zeros((0, 0))
        x = torch.from_numpy(host).to(ops.device)
    N, C = x.shape
    C_total = C
    if _bkdist.collectives_active(group):
        parts = _bkdist.all_gather(torch.tensor([N, C], dtype=torch.int64, device=x.device), group)
        Ns = [int(p[0].item()) for p in parts]
        if len(set(Ns)) > 1:
            raise ValueError(f"{name} requires the same number of draws on every rank, got N = {Ns}")
        C_total = sum(int(p[1].item()) for p in parts)
    if C_total < 1:
        raise ValueError(f"{name} requires at least one chain")
    if N < 8:
        raise ValueError(f"{name} requires at least 8 draws per chain (4 per split half), got {N}")
    return x, C_total


def _split_set(x):
    """The split set's rows of x [N, C]: x itself for even N, else x without its middle row."""
    N = x.shape[0]
    n = N // 2
    return x if N == 2 * n else torch.cat([x[:n], x[N - n:]])


class _SplitSort:
    """One pooled sort of a split set xs [2n, C_local] over all ranks of `group`: the normal scores of its ranks
    (``z``, [2n, C_local] chain-contiguous: bulk ESS and rank-normalised R-hat) and its order statistics (the quantiles of
    tail ESS).  Ranks as rank_chains: ordinal, stable, chain-major pooled order with chains in global order; for even N
    ``z`` is bit for bit ``rank_normalize_chains(x)``.  (posterior averages tied ranks and uses Blom's 3/8; this
    follows the library's rank_normalize_chains, the reference's (r - 0.325) / (S - 0.25).)"""

    def __init__(self, xs, ops, group):
        self._ops, self._group = ops, group
        self._multi = _bkdist.collectives_active(group)
        n2, C = xs.shape
        dev = xs.device
        if self._multi:
            ranks = _ranks_pooled_across_ranks(xs, ops, group)       # [2n, C] view of chain-major ranks
            self.S = sum(_all_gather_counts(xs.numel(), dev, group))
            self._ranks_t = ranks.t().contiguous().reshape(-1)
            self._values = xs.t().contiguous().reshape(-1)
        else:
            self._values = xs.t().contiguous().reshape(-1)
            self.S = self._values.numel()
            idx = torch.arange(self.S, dtype=torch.int64, device=dev)
            _, self._payload = ops.sort_by_key(_canonical_keys(self._values).contiguous(), idx)
            self._ranks_t = None
        self._shape = (C, n2)
        self._z = None

    @property
    def _ranks(self):
        if self._ranks_t is None:
            self._ranks_t = torch.empty_like(self._values)
            self._ops.scatter_ranks(self._payload, 0.0, self._ranks_t)
        return self._ranks_t

    @property
    def z(self):
        """The normal scores (computed on first use: tail ESS needs the order statistics alone)."""
        if self._z is None:
            z = torch.empty_like(self._ranks)
            self._ops.rank_normalize(self._ranks, float(self.S), z)
            self._z = z.reshape(*self._shape).t().contiguous()
        return self._z

    def order_stats(self, positions):
        """Values at the given 0-based positions of the pooled sorted split set (host array)."""
        dev = self._values.device
        if not self._multi:
            sel = self._payload[torch.tensor(positions, dtype=torch.int64, device=dev)]
            return self._values[sel].cpu().numpy()
        out = []
        for j in range(0, len(positions), 8):  # (bk_select_ranks takes up to 8 ranks per call)
            chunk = positions[j:j + 8]
            o = torch.zeros(len(chunk), dtype=torch.float64, device=dev)
            self._ops.select_ranks(self._ranks, self._values,
                                   torch.tensor([p + 1.0 for p in chunk], dtype=torch.float64, device=dev), o)
            out.append(_gather_sum(o, self._group).cpu().numpy())
        return np.concatenate(out)


def _lag_sums_fft(x, q, chain_g0, ops):
    """sum_m gamma_{m,t} for all t < n, for halves too long for the LDS tile: bk_autocorr_fft on the half views in chain
    batches (the indicator chains materialised one batch at a time), then bk_ess_acov_sums."""
    N, C = x.shape
    n = N // 2
    block = _fft_batch(n, C, ops)
    out = torch.zeros(n, dtype=torch.float64, device=x.device)
    for h, rows in ((0, x[:n]), (1, x[N - n:])):
        for c0 in range(0, C, block):
            v = rows[:, c0:c0 + block]
            if q is not None:
                ind = torch.empty((n, v.shape[1]), dtype=torch.float64, device=x.device)
                ops.ess_indicator(v, q, ind)
                v = ind
            acor = torch.empty((n, v.shape[1]), dtype=torch.float64, device=x.device)
            ops.autocorr_fft(v, acor)
            out += ops.ess_acov_sums(acor, chain_g0[h * C + c0:h * C + c0 + v.shape[1]], 0, n)
    return out


def _ess_split(x, q, ops, group, C_total):
    """(ESS, pooled sd, pooled mean) of the split chains of x [N, C_local] (q: None = the draws, else the indicator x <= q), over all
    ranks' chains.  NaN for a non-finite draw or var_plus == 0."""
    N, C = x.shape
    n = N // 2
    M = 2 * C_total
    dev = x.device
    chain_mean = torch.empty(2 * C, dtype=torch.float64, device=dev)
    chain_g0 = torch.empty(2 * C, dtype=torch.float64, device=dev)
    if C:
        mom = ops.ess_split_moments(x, q, chain_mean, chain_g0)
    else:
        mom = torch.zeros(3, dtype=torch.float64, device=dev)
    tot = _gather_sum(mom, group)
    centre = (tot[0:1] / M).contiguous()
    between = ops.ess_between_sq(chain_mean, centre) if C else torch.zeros(1, dtype=torch.float64, device=dev)
    h = torch.cat([tot, _gather_sum(between, group)]).cpu().numpy()
    sum_g0, bad, bsq = float(h[1]), float(h[2]), float(h[3])
    if bad > 0:
        return np.nan, np.nan, np.nan
    mean = float(h[0]) / M
    sd = float(np.sqrt((n * sum_g0 + n * bsq) / (M * n - 1)))
    W = sum_g0 / M * n / (n - 1)
    var_plus = W * (n - 1) / n + bsq / (M - 1)
    if var_plus == 0 or not np.isfinite(var_plus):
        return np.nan, sd, mean
    fft = n > ops.ess_lag_sums_max_half()
    Gamma = np.zeros(0)
    L, nxt = 0, (n if fft else min(ESS_FIRST_LAGS, n))
    while True:
        if not C:
            part = torch.zeros(nxt - L, dtype=torch.float64, device=dev)
        elif fft:
            part = _lag_sums_fft(x, q, chain_g0, ops)
        else:
            part = ops.ess_lag_sums(x, q, chain_mean, L, nxt - L)
        Gamma = np.concatenate([Gamma, _gather_sum(part, group).cpu().numpy() / M])
        L = nxt
        r = _geyer_tau(Gamma, W, var_plus, M, n)
        if r is not None:
            return M * n / r[0], sd, mean
        nxt = min(2 * L, n)


def _check_prob(prob):
    if not 0.0 < float(prob) < 1.0:
        raise ValueError(f"ess_quantile requires 0 < prob < 1, got {prob}")


def _bulk(x, ops, group, C_total, srt):
    ends = srt.order_stats([0, srt.S - 1])  # (non-finite draws sort to the ends)
    if not np.all(np.isfinite(ends)):
        return np.nan
    return _ess_split(srt.z, None, ops, group, C_total)[0]


def _tail_min(values):
    """The smaller of the two quantile ESS values, NaN if either is NaN (a degenerate indicator; R's min gives NA)."""
    return float(np.min(values))


def _quantile_ess(x, ops, group, C_total, srt, probs):
    qs = _split_quantiles(srt.order_stats, srt.S, probs)
    return [_ess_split(x, q, ops, group, C_total)[0] for q in qs]


def ess_bulk(chains, *, ops=None, group=None):
    """Bulk effective sample size over all chains (Vehtari et al. 2021, sec. 3.2): the multi-chain ESS of the
    rank-normalised split chains.

    ``chains``: an [N, C] float64 device tensor (draw-major, unit column stride, any row stride: ``DrawRecorder.view(k)``,
    ``DrawStore.series(d)``) or a sequence of equal-length 1-D chains; with a process group, this rank's [N, C_local]
    shard, and the value is over all ranks' chains (the same on every rank).  N >= 8.

    With thousands of short chains (this library's normal use) the estimate runs below the truth for strongly correlated
    draws: rho(t) keeps a small positive bias beyond lag ~ n / tau that the noise of a few chains would end the scan on,
    so the scan runs to its bound (t < n - 5).  At 2,048 chains of 1,000 draws of an AR(1) with phi = 0.9 it gives
    0.85-0.91 of the true ESS (0.99 at 4,000 draws).  Such data needs every lag."""
    ops = _ops(ops)
    x, C_total = _multi_input(chains, ops, "ess_bulk", group)
    return np.float64(_bulk(x, ops, group, C_total, _SplitSort(_split_set(x), ops, group)))


def ess_quantile(chains, prob, *, ops=None, group=None):
    """Multi-chain ESS of the split indicator chains I = (x <= q_prob), q_prob = np.quantile(split pooled draws, prob)
    (method "linear", bit for bit).  Inputs as ``ess_bulk``; 0 < prob < 1."""
    _check_prob(prob)
    ops = _ops(ops)
    x, C_total = _multi_input(chains, ops, "ess_quantile", group)
    srt = _SplitSort(_split_set(x), ops, group)
    return np.float64(_quantile_ess(x, ops, group, C_total, srt, [prob])[0])


def ess_tail(chains, *, ops=None, group=None):
    """Tail effective sample size: min(ess_quantile(chains, 0.05), ess_quantile(chains, 0.95)), from one sort; NaN when
    either is NaN (e.g. 5 % or more of the draws tie at the maximum: the 0.95 indicator is all 1).  Inputs as
    ``ess_bulk``."""
    ops = _ops(ops)
    x, C_total = _multi_input(chains, ops, "ess_tail", group)
    srt = _SplitSort(_split_set(x), ops, group)
    return np.float64(_tail_min(_quantile_ess(x, ops, group, C_total, srt, [0.05, 0.95])))


def ess_mean(chains, *, ops=None, group=None):
    """Multi-chain ESS of the raw split chains (the ESS that goes with the posterior mean).  Inputs as ``ess_bulk``."""
    ops = _ops(ops)
    x, C_total = _multi_input(chains, ops, "ess_mean", group)
    return np.float64(_ess_split(x, None, ops, group, C_total)[0])


def mcse_mean(chains, *, ops=None, group=None):
    """Monte Carlo standard error of the mean: sd / sqrt(ess_mean), sd the pooled standard deviation (ddof = 1) of the
    split set, from the same moments.  Inputs as ``ess_bulk``."""
    ops = _ops(ops)
    x, C_total = _multi_input(chains, ops, "mcse_mean", group)
    e, sd, _ = _ess_split(x, None, ops, group, C_total)
    return np.float64(sd / np.sqrt(e))


def _multi_summary(x, ops, group):
    """DrawRecorder.summary() of one [N, C_local] series."""
    x, C_total = _multi_input(x, ops, "summary", group)
    N = x.shape[0]
    e_mean, sd, mean = _ess_split(x, None, ops, group, C_total)
    srt = _SplitSort(_split_set(x), ops, group)
    tail = _tail_min(_quantile_ess(x, ops, group, C_total, srt, [0.05, 0.95]))
    bulk = _bulk(x, ops, group, C_total, srt)
    # R-hat from the same ranks (even N: srt.z is rank_normalize_chains(x)); an odd N has no middle row in srt
    rh = split_rhat(srt.z, ops=ops, group=group) if N % 2 == 0 else rank_normalized_rhat(x, ops=ops, group=group)
    return {"mean": mean, "sd": sd, "mcse_mean": sd / np.sqrt(e_mean), "ess_bulk": bulk, "ess_tail": tail,
            "rhat": float(rh)}
