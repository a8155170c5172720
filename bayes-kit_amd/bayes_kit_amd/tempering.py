"""``TemperedStretcher``: parallel tempering (replica exchange) on top of the ensemble sampler, for posteriors with
separated modes.

A ladder of ``T`` inverse temperatures ``betas[0] > betas[1] > ...`` gives ``T`` rungs; a walker on rung ``t`` targets
``lp0(theta) + betas[t] * ll(theta)``.  For a batched model with ``log_prior`` and ``log_likelihood`` (the
``LogPriorLikelihoodModel`` ``TemperedLikelihoodSMC`` takes) ``lp0`` is the prior and ``ll`` the likelihood, ``beta = 0`` is
allowed (the prior itself) and the ladder yields the model evidence; for any other model the whole ``log_density`` is
tempered, ``lp0`` is absent and every ``beta`` must be positive.

Every rung is an ensemble of ``Stretcher``: ``ensembles = replicas * T``, ensemble ``e = r * T + t`` with the rung ``t``
fastest, in ``Stretcher``'s column layout (walker ``i`` of half ``s`` of ensemble ``e`` is column ``s * C/2 + e * H + i``).
The rungs ``t`` and ``t + 1`` of one replica are therefore columns ``c`` and ``c + H`` of the same half: two adjacent
contiguous slices, which is all ``bk_replica_swap`` knows about (include/bkhip.h).

A draw is ``Stretcher``'s two half-updates with the tempered accept test (``bk_tempered_accept``; the ``z^(D-1)`` term
belongs to the proposal and is not tempered).  After draw number ``n = 1, 2, ...`` with ``n % swap_every == 0`` comes swap
round ``k = n / swap_every``: every pair ``(t, t + 1)`` with ``t % 2 == k % 2`` of every replica and both halves, walker
``i`` of rung ``t`` against walker ``i`` of rung ``t + 1`` (deterministic even-odd scheme).

Streams: an active walker draws ``u_j``, ``u_z``, ``u_a`` from its own stream as in ``Stretcher``; in a swap round the walker
on the LOWER rung index of each pair draws one more uniform from its own stream, and nobody else draws: where a stream
stands is a function of the draw count, the walker's rung and the parity alone.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from .ensemble import Stretcher


def geometric_ladder(T: int, beta_min: float, zero: bool = False) -> np.ndarray:
    """``T`` inverse temperatures from 1 down to ``beta_min`` in equal ratios, optionally followed by 0 (the prior; then
    ``T + 1`` rungs in all)."""
    if isinstance(T, bool) or not isinstance(T, (int, np.integer)) or T < 1:
        raise ValueError(f"T must be a strictly positive integer; found {T=}")
    if T > 1 and not 0.0 < beta_min < 1.0:
        raise ValueError(f"beta_min must lie inside (0, 1); found {beta_min=}")
    b = np.geomspace(1.0, float(beta_min), int(T)) if T > 1 else np.ones(1)
    b[0] = 1.0
    return np.concatenate([b, [0.0]]) if zero else b


def _positive_int(x) -> bool:
    return not isinstance(x, bool) and isinstance(x, (int, np.integer)) and x > 0


class TemperedStretcher(Stretcher):
    """``betas``: strictly decreasing, finite, >= 0 (0 only for a model with a prior / likelihood split); ``replicas``:
    independent ladders side by side (whole replicas per rank: shard with ``chain_id0``); ``swap_every``: draws between swap
    rounds; ``walkers``: walkers per rung; ``init``: (replicas * T * walkers, D).  ``sample()`` returns every walker's
    ``theta`` and its UNTEMPERED log density; ``cold_rows()`` are the rows that sample the target itself (rung 0)."""

    def __init__(self, model, betas, a: float = 2.0, walkers: Optional[int] = None, init=None, *, seed=None,
                 replicas: int = 1, swap_every: int = 1, chain_id0: int = 0, ops=None):
        b = np.asarray(betas, dtype=np.float64)
        if b.ndim != 1 or b.shape[0] < 1 or not np.isfinite(b).all() or (b < 0.0).any() or (np.diff(b) >= 0.0).any():
            raise ValueError(f"betas must be a strictly decreasing sequence of finite values >= 0; found {betas=}")
        if not _positive_int(replicas):
            raise ValueError(f"replicas must be a strictly positive integer; found {replicas=}")
        if not _positive_int(swap_every):
            raise ValueError(f"swap_every must be a strictly positive integer; found {swap_every=}")
        self._split = (getattr(model, "batched", False) is True and callable(getattr(model, "log_prior", None))
                       and callable(getattr(model, "log_likelihood", None)))
        if not self._split and b[-1] <= 0.0:
            raise ValueError("beta = 0 needs a batched model with log_prior and log_likelihood: without that split the "
                             "whole log density is tempered and every beta must be > 0")
        self._betas = b
        self._T, self._replicas, self._swap_every = int(b.shape[0]), int(replicas), int(swap_every)
        super().__init__(model, a, walkers, init, seed=seed, ensembles=self._replicas * self._T, chain_id0=chain_id0,
                         ops=ops)

    # -- the tempered target ---------------------------------------------------------------------------------------------
    def _init_cache(self):
        C, E, H, T, dev = self._C, self._ensembles, self._H, self._T, self._ops.device
        f64 = dict(dtype=torch.float64, device=dev)
        self._ll, self._ll_p = self._lp, self._lp_p  # (the base class's cache and scratch, under the names used here)
        self._lp0 = torch.zeros(C, **f64) if self._split else None
        self._lp0_p = torch.zeros(C, **f64) if self._split else None
        rung = self.rung_index()
        self._beta_col = torch.as_tensor(self._betas, **f64)[rung].contiguous()
        self._lower = []  # per parity: the walkers on the lower rung index of a pair (they draw the swap's uniform)
        for p in (0, 1):
            low = ((rung % 2 == p) & (rung + 1 < T)).to(torch.uint8).contiguous()
            self._lower.append(low if bool(low.any()) else None)
        self._swapped = torch.zeros(C, dtype=torch.uint8, device=dev)
        self._swap_ran = False
        # statistics, all on the device; block g = s * E + e of H columns is half s of ensemble e
        self._rung_acc = torch.zeros(E, dtype=torch.int32, device=dev)
        self._swap_prop = torch.zeros(2 * E, dtype=torch.int32, device=dev)
        self._swap_acc = torch.zeros(2 * E, dtype=torch.int32, device=dev)
        self._ll_sum = torch.zeros(E, **f64)
        self._lse = torch.full((E,), -math.inf, **f64)
        self._stat_n = torch.zeros(1, dtype=torch.int64)  # (host: draws the statistics cover)
        # (beta_{t-1} - beta_t) of every ensemble's rung t; 0.0 for rung 0, whose entry of `_lse` is never read
        db = np.concatenate([[0.0], self._betas[:-1] - self._betas[1:]])
        self._dbeta_e = torch.as_tensor(np.tile(db, self._replicas), **f64)
        self._eval_target(self._theta_dc, self._lp0, self._ll)

    def _eval_target(self, theta_dc, lp0_out, ll_out):
        if self._split:
            m = self._model
            lp0_out.copy_(m.log_prior(theta_dc.t()))
            ll_out.copy_(m.log_likelihood(theta_dc.t()))
        else:
            self._eval_logp(theta_dc, ll_out)

    def _accept(self, act):
        sp = self._split
        self._eval_target(self._theta_p[:, act], self._lp0_p[act] if sp else None, self._ll_p[act])
        # log(u_a) < ((lp0* - lp0) + beta (ll* - ll)) + zterm; accepted moves are counted per ensemble
        self._ops.tempered_accept(self._ll[act], self._lp0[act] if sp else None, self._ll_p[act],
                                  self._lp0_p[act] if sp else None, self._beta_col[act], self._zterm[act], self._logu[act],
                                  self._mask[act], self._rung_acc, self._H)

    def _end_draw(self, out):
        self._swap_ran = False
        if self._draws % self._swap_every == 0:
            low = self._lower[(self._draws // self._swap_every) % 2]
            if low is not None:
                ops = self._ops
                ops.log_uniform(self._rng_kind, self._rng_state, self._logu, low)
                # the state and the copy of it that this draw returns change places alike
                ops.replica_swap(self._theta_dc, out, self._ll, self._lp0, self._beta_col, self._logu, low, self._swapped,
                                 self._swap_prop, self._swap_acc, self._H)
                self._swap_ran = True
        self._accumulate()

    def _accumulate(self):
        """This draw's share of the running statistics: per ensemble the sum of ll, and the log-sum-exp of
        (beta_{t-1} - beta_t) ll over the walkers of rung t (the stepping stone from rung t to rung t - 1)."""
        E, H = self._ensembles, self._H
        ll = self._ll.view(2, E, H)
        self._ll_sum += ll.sum(dim=(0, 2))
        w = (ll * self._dbeta_e[None, :, None]).permute(1, 0, 2).reshape(E, 2 * H)
        torch.logaddexp(self._lse, torch.logsumexp(w, dim=1), out=self._lse)
        self._stat_n += 1

    def _logp_out(self):
        return self._lp0 + self._ll if self._split else self._ll

    # -- state -------------------------------------------------------------------------------------------------------
    def _state_tensors(self):
        st = {"theta": self._theta_dc, "ll": self._ll, "rung_accepted": self._rung_acc, "swap_proposed": self._swap_prop,
              "swap_accepted": self._swap_acc, "ll_sum": self._ll_sum, "lse": self._lse, "stat_draws": self._stat_n}
        if self._split:
            st["lp0"] = self._lp0
        return st

    def _state_extra(self):
        return {"a": self._a, "walkers": self._walkers, "ensembles": self._ensembles,
                "betas": [float(b) for b in self._betas], "replicas": self._replicas, "swap_every": self._swap_every}

    def load_state_dict(self, sd):
        self._load_extra(sd["meta"].get("extra", {}))  # another ladder is refused before anything is overwritten
        super().load_state_dict(sd)

    @property
    def betas(self) -> np.ndarray:
        return self._betas.copy()

    @property
    def replicas(self) -> int:
        return self._replicas

    @property
    def swap_every(self) -> int:
        return self._swap_every

    @property
    def last_swapped(self):
        """Whether a walker changed places with walker i of the next rung in the last draw's swap round (bool, length C;
        set at the walker on the lower rung index of the pair)."""
        return self._swapped.bool() if self._swap_ran else torch.zeros_like(self._swapped).bool()

    def rung_index(self):
        """The rung of every row of a draw (length C): ensemble e = r * T + t is rung t of replica r."""
        return self.ensemble_index() % self._T

    def replica_index(self):
        """The replica of every row of a draw (length C)."""
        return self.ensemble_index() // self._T

    def cold_rows(self):
        """The rows of a draw on rung 0: the walkers that sample the target at betas[0]."""
        return torch.nonzero(self.rung_index() == 0).reshape(-1)

    # -- statistics: read only when asked ------------------------------------------------------------------------------
    def _stat_draws(self) -> int:
        return int(self._stat_n.item())

    def reset_statistics(self):
        """Forget the counters and the running statistics gathered so far (a burn-in)."""
        for t in (self._rung_acc, self._swap_prop, self._swap_acc, self._ll_sum, self._stat_n):
            t.zero_()
        self._lse.fill_(-math.inf)

    def accept_rate(self) -> float:
        n = self._stat_draws() * self._C
        return float(self._rung_acc.sum().item()) / n if n else float("nan")

    def rung_accept_rate(self) -> np.ndarray:
        """Accepted stretch moves per proposed one, per rung -> [T]."""
        n = self._stat_draws() * self._replicas * self._walkers
        acc = self._rung_acc.view(self._replicas, self._T).sum(dim=0).cpu().numpy().astype(np.float64)
        return acc / n if n else np.full(self._T, np.nan)

    def swap_rate(self) -> np.ndarray:
        """Accepted swaps per proposed one, per pair (t, t + 1) -> [T - 1] (NaN for a pair that never proposed)."""
        shape = (2, self._replicas, self._T)
        prop = self._swap_prop.view(shape).sum(dim=(0, 1)).cpu().numpy().astype(np.float64)[:self._T - 1]
        acc = self._swap_acc.view(shape).sum(dim=(0, 1)).cpu().numpy().astype(np.float64)[:self._T - 1]
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(prop > 0, acc / prop, np.nan)

    def mean_log_likelihood(self) -> np.ndarray:
        """The mean of ll over the walkers of every rung and the draws since the last reset -> [replicas, T] (the integrand
        of thermodynamic integration)."""
        n = self._stat_draws() * self._walkers
        s = self._ll_sum.view(self._replicas, self._T).cpu().numpy()
        return s / n if n else np.full(s.shape, np.nan)

    def log_evidence(self) -> np.ndarray:
        """The stepping-stone estimate of the log evidence, sum_t log mean_{rung t+1} exp((beta_t - beta_{t+1}) ll), per
        replica -> [replicas].  Needs the prior / likelihood split and a ladder from 1 down to 0."""
        if not self._split:
            raise ValueError("log_evidence needs a model with log_prior and log_likelihood: the base measure of a tempered "
                             "log_density is improper")
        if self._betas[0] != 1.0 or self._betas[-1] != 0.0:
            raise ValueError(f"log_evidence needs betas[0] == 1 and betas[-1] == 0; found {self._betas[0]} and "
                             f"{self._betas[-1]}")
        n = self._stat_draws() * self._walkers
        if not n:
            return np.full(self._replicas, np.nan)
        lse = self._lse.view(self._replicas, self._T).cpu().numpy()
        return (lse[:, 1:] - math.log(n)).sum(axis=1)
