"""Host side of the cross-chain warmup (HMCDiag.warmup, MALA.warmup): the window schedule, the dual-averaging controller of
the step size, the shrinkage of a window's estimate, and the jitter and the controller of the trajectory length.  The loop
that drives them is ManyChainSampler._warmup_loop (_engine.py); a sampler supplies how a warmup draw is launched, where its
step size lives, a metric estimator (update after a draw, install at a window's end) and, for ChEES, an observer of the totals.

Pure Python on a handful of doubles per draw; everything that touches [D, C] arrays stays on the device
(bk_accept_stat, bk_welford_update, bk_rhat_partials, bk_chees_sums, bk_chees_stat).  The window schedule's and dual
averaging's constants are Stan's.
"""
from __future__ import annotations

import math


def warmup_windows(draws: int, init: int = 75, term: int = 50, base: int = 25):
    """-> (init, term, ends): `init` draws of step-size adaptation alone, metric windows that start after them, double
    in length and END after the draws listed in `ends` (1-based counts), `term` closing draws of step-size adaptation.
    Fewer than 20 draws: no window (only the step size adapts).  A schedule that does not fit is scaled to 15 % / 10 % of
    the draws; the last window is stretched to draws - term when the next one would not fit."""
    if draws < 20:
        return 0, draws, []
    if init + term + base > draws:
        init = int(0.15 * draws)
        term = int(0.1 * draws)
        base = draws - init - term
    ends, start, w, slow_end = [], init, base, draws - term
    while start < slow_end:
        end = start + w
        if end + 2 * w > slow_end:
            end = slow_end
        ends.append(end)
        start, w = end, 2 * w
    return init, term, ends


def shrink_estimate(estimate, n_eff):
    """A window's variances [D] or covariance [D, D] from n_eff points, shrunk towards 1e-3 times the unit metric (Stan's
    regularisation): n/(n+5) * estimate + 1e-3 * 5/(n+5), for a matrix added to the diagonal (in place, of the product).
    The order of the operations is part of the result: dual averaging amplifies one ulp of it to percents."""
    shrunk = n_eff / (n_eff + 5.0) * estimate
    floor = 1e-3 * 5.0 / (n_eff + 5.0)
    if shrunk.ndim == 2:
        shrunk.diagonal().add_(floor)
        return shrunk
    return shrunk + floor


class DualAveraging:
    """Nesterov dual averaging on x = log(eps) towards a mean acceptance statistic `target` (Hoffman & Gelman 2014,
    algorithm 5): gamma = 0.05, t0 = 10, kappa = 0.75, mu = log(10 * eps)."""

    def __init__(self, eps: float, target: float = 0.8, gamma: float = 0.05, t0: float = 10.0, kappa: float = 0.75):
        self.target, self.gamma, self.t0, self.kappa = float(target), float(gamma), float(t0), float(kappa)
        self.restart(eps)

    def restart(self, eps: float) -> None:
        self.mu = math.log(10.0 * eps)
        self.t = 0
        self.hbar = 0.0
        self.xbar = 0.0

    def step(self, alpha: float) -> float:
        """Feed one draw's mean acceptance statistic; -> the step size of the next draw, exp(x)."""
        self.t += 1
        eta = 1.0 / (self.t + self.t0)
        self.hbar = (1.0 - eta) * self.hbar + eta * (self.target - alpha)
        x = self.mu - math.sqrt(self.t) / self.gamma * self.hbar
        w = self.t ** (-self.kappa)
        self.xbar = w * x + (1.0 - w) * self.xbar
        return math.exp(x)

    def final(self) -> float:
        """The averaged iterate, exp(xbar): the step size to keep."""
        return math.exp(self.xbar)


def radical_inverse2(n: int) -> float:
    """The base-2 radical inverse of n >= 1 (van der Corput): 1/2, 1/4, 3/4, 1/8, 5/8, ...; exact in a double."""
    h, f, n = 0.0, 0.5, int(n)
    while n:
        if n & 1:
            h += f
        n >>= 1
        f *= 0.5
    return h


def jitter_steps(n: int, T: float, eps: float, max_steps: int) -> int:
    """Leapfrog steps of jittered draw n = 1, 2, ...: min(max_steps, max(1, ceil(h_n T / eps))), h_n = radical_inverse2(n)."""
    return int(min(int(max_steps), max(1, math.ceil(radical_inverse2(n) * float(T) / float(eps)))))


class TrajectoryAdam:
    """Gradient ascent on x = log(T) of the ChEES criterion (Hoffman, Radul, Sountsov 2021), the gradient taken across
    chains (bk_chees_stat): Adam with beta1 = 0, beta2 = 0.95, learning rate 0.025, and DualAveraging's averaging of the
    iterates (weight k^-0.75).  The constants are this project's choice after the paper."""

    BETA2, RATE, TINY, KAPPA = 0.95, 0.025, 1e-8, 0.75

    def __init__(self, T: float):
        self.x = math.log(float(T))
        self.restart()

    def restart(self) -> None:
        """Keep x, forget the second moment, the update count and the averaged iterate (the geometry has changed)."""
        self.v = 0.0
        self.k = 0
        self.xbar = 0.0

    def step(self, S_wg: float, S_w: float, t: float, eps: float, max_steps: int) -> float:
        """Feed one draw: S_wg = sum_c w_c g_c and S_w = sum_c w_c over all chains, t = L eps the time that draw integrated;
        x is kept inside [log eps, log(eps max_steps)].  A draw without weight or with a non-finite sum is skipped.
        -> the trajectory length of the next draw, exp(x)."""
        if S_w > 0.0 and math.isfinite(S_wg):
            g = t * S_wg / S_w
            self.k += 1
            self.v = self.BETA2 * self.v + (1.0 - self.BETA2) * g * g
            self.x += self.RATE * g / (math.sqrt(self.v / (1.0 - self.BETA2 ** self.k)) + self.TINY)
            self.x = min(max(self.x, math.log(eps)), math.log(eps * max_steps))
            w = self.k ** (-self.KAPPA)
            self.xbar = w * self.x + (1.0 - w) * self.xbar
        return math.exp(self.x)

    def final(self) -> float:
        """exp of the averaged iterate: the trajectory length to keep (exp(x) when no draw was fed)."""
        return math.exp(self.xbar if self.k > 0 else self.x)
