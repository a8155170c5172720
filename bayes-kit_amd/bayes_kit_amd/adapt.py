"""Host side of the cross-chain warmup (HMCDiag.warmup): the window schedule and the dual-averaging controller.

Pure Python on a handful of doubles per draw; everything that touches [D, C] arrays stays on the device
(bk_accept_stat, bk_welford_update, bk_rhat_partials).  The constants are Stan's.
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
