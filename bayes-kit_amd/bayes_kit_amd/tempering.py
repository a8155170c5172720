"""Parallel tempering (replica exchange), for posteriors with separated modes: ``ReplicaLadder``, everything the tempered
samplers share, and ``TemperedStretcher``, the ladder on top of the ensemble sampler.

A ladder of ``T`` inverse temperatures ``betas[0] > betas[1] > ...`` gives ``T`` rungs; a chain (a walker) on rung ``t``
targets ``lp0(theta) + betas[t] * ll(theta)``.  For a split model ``lp0`` is the prior and ``ll`` the likelihood, ``beta = 0``
is allowed (the prior itself) and the ladder yields the model evidence; for any other model the whole log density is
tempered, ``lp0`` is absent and every ``beta`` must be positive.  Which methods make a model split is the sampler's business
(``_SPLIT_METHODS``): ``log_prior`` and ``log_likelihood`` on a batched model here (the ``LogPriorLikelihoodModel``
``TemperedLikelihoodSMC`` takes), their gradient forms in ``tempered_hmc.TemperedHMC``.

``ReplicaLadder`` owns what concerns the ladder and nothing else: the check of ``betas``, ``replicas`` and ``swap_every``, the
per-column tables, the swap round, the statistics on the device with their read-outs, the index helpers, and the ladder's
share of a checkpoint.  The layout it knows is blocks of ``H`` columns, block ``e = r * T + t`` for rung ``t`` of replica ``r``
(the rung fastest), in one row of ``E = replicas * T`` blocks (``TemperedHMC``) or in two halves of ``E`` blocks each
(``Stretcher``'s column layout: walker ``i`` of half ``s`` of ensemble ``e`` is column ``s * C/2 + e * H + i``).  Either way the
rungs ``t`` and ``t + 1`` of one replica are columns ``c`` and ``c + H``: two adjacent contiguous slices, which is all
``bk_replica_swap`` knows about (include/bkhip.h).  A sampler keeps its target, its move and its own settings.

After draw number ``n = 1, 2, ...`` with ``n % swap_every == 0`` comes swap round ``k = n / swap_every``: every pair
``(t, t + 1)`` with ``t % 2 == k % 2`` of every replica (and both halves), column ``i`` of rung ``t`` against column ``i`` of
rung ``t + 1`` (deterministic even-odd scheme).

``TemperedStretcher``: every rung is an ensemble of ``Stretcher``, ``ensembles = replicas * T``.  A draw is ``Stretcher``'s two
half-updates with the tempered accept test (``bk_tempered_accept``; the ``z^(D-1)`` term belongs to the proposal and is not
tempered), then the swap round.

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


class ReplicaLadder:
    """The replica ladder of a tempered sampler (mix in BEFORE the ``ManyChainSampler`` it tempers).  The sampler calls
    ``_ladder_args`` before its base class is set up and ``_init_ladder`` once the device and ``C`` are known, ends every draw
    with ``_swap_round`` and ``_accumulate``, and provides the caches the swap exchanges with the state: ``_ll`` and ``_lp0``
    (None without the split), and ``_logu``."""

    _SPLIT_METHODS: tuple = ()  # the two methods of a batched model that make it a prior / likelihood split for this sampler

    def _ladder_args(self, model, betas, replicas, swap_every):
        """Validates and keeps the ladder's settings; decides whether the model is split."""
        b = np.asarray(betas, dtype=np.float64)
        if b.ndim != 1 or b.shape[0] < 1 or not np.isfinite(b).all() or (b < 0.0).any() or (np.diff(b) >= 0.0).any():
            raise ValueError(f"betas must be a strictly decreasing sequence of finite values >= 0; found {betas=}")
        if not _positive_int(replicas):
            raise ValueError(f"replicas must be a strictly positive integer; found {replicas=}")
        if not _positive_int(swap_every):
            raise ValueError(f"swap_every must be a strictly positive integer; found {swap_every=}")
        self._split = (getattr(model, "batched", False) is True
                       and all(callable(getattr(model, name, None)) for name in self._SPLIT_METHODS))
        if not self._split and b[-1] <= 0.0:
            raise ValueError(f"beta = 0 needs a batched model with {' and '.join(self._SPLIT_METHODS)}: without that split "
                             "the whole log density is tempered and every beta must be > 0")
        self._betas = b
        self._T, self._replicas, self._swap_every = int(b.shape[0]), int(replicas), int(swap_every)

    def _init_ladder(self, H, halves):
        """The per-column tables and the statistics, for blocks of `H` columns in `halves` (2: the ensemble layout, 1: one
        row of blocks)."""
        T, dev = self._T, self._ops.device
        E = self._replicas * T
        f64 = dict(dtype=torch.float64, device=dev)
        self._blocks = (halves, E, H)
        self._per_rung = halves * H  # columns of one rung of one replica
        rung = self.rung_index()
        self._beta_col = torch.as_tensor(self._betas, **f64)[rung].contiguous()
        self._lower = []  # per parity: the columns on the lower rung index of a pair (they draw the swap's uniform)
        for p in (0, 1):
            low = ((rung % 2 == p) & (rung + 1 < T)).to(torch.uint8).contiguous()
            self._lower.append(low if bool(low.any()) else None)
        self._swapped = torch.zeros(self._C, dtype=torch.uint8, device=dev)
        self._swap_ran = False
        # statistics, all on the device; block g = s * E + e of H columns is half s of block e
        self._rung_acc = torch.zeros(E, dtype=torch.int32, device=dev)
        self._swap_prop = torch.zeros(halves * E, dtype=torch.int32, device=dev)
        self._swap_acc = torch.zeros(halves * E, dtype=torch.int32, device=dev)
        self._ll_sum = torch.zeros(E, **f64)
        self._lse = torch.full((E,), -math.inf, **f64)
        self._stat_n = torch.zeros(1, dtype=torch.int64)  # (host: draws the statistics cover)
        # (beta_{t-1} - beta_t) of every block's rung t; 0.0 for rung 0, whose entry of `_lse` is never read
        db = np.concatenate([[0.0], self._betas[:-1] - self._betas[1:]])
        self._dbeta_e = torch.as_tensor(np.tile(db, self._replicas), **f64)

    # -- the end of a draw -------------------------------------------------------------------------------------------------
    def _swap_round(self, out) -> bool:
        """The swap round after draw `_draws`, if one is due and its parity has a pair -> whether it ran.  `out` is the copy
        of the state that the draw returns: it and the state change places alike.  The decision overwrites `_ll` (and
        `_lp0`); whatever else a sampler caches per column follows by `_swapped`."""
        self._swap_ran = False
        if self._draws % self._swap_every == 0:
            low = self._lower[(self._draws // self._swap_every) % 2]
            if low is not None:
                ops = self._ops
                ops.log_uniform(self._rng_kind, self._rng_state, self._logu, low)
                ops.replica_swap(self._theta_dc, out, self._ll, self._lp0, self._beta_col, self._logu, low, self._swapped,
                                 self._swap_prop, self._swap_acc, self._blocks[2])
                self._swap_ran = True
        return self._swap_ran

    def _accumulate(self):
        """This draw's share of the running statistics: per block the sum of ll, and the log-sum-exp of
        (beta_{t-1} - beta_t) ll over the columns of rung t (the stepping stone from rung t to rung t - 1).  (Each layout
        keeps its own reduction: the sums are compared bit for bit across checkpoints.)"""
        halves, E, H = self._blocks
        if halves == 2:
            ll = self._ll.view(2, E, H)
            self._ll_sum += ll.sum(dim=(0, 2))
            w = (ll * self._dbeta_e[None, :, None]).permute(1, 0, 2).reshape(E, 2 * H)
        else:
            ll = self._ll.view(E, H)
            self._ll_sum += ll.sum(dim=1)
            w = ll * self._dbeta_e[:, None]
        torch.logaddexp(self._lse, torch.logsumexp(w, dim=1), out=self._lse)
        self._stat_n += 1

    # -- checkpoints -------------------------------------------------------------------------------------------------------
    def _state_tensors(self):
        st = {"theta": self._theta_dc, "ll": self._ll, "rung_accepted": self._rung_acc, "swap_proposed": self._swap_prop,
              "swap_accepted": self._swap_acc, "ll_sum": self._ll_sum, "lse": self._lse, "stat_draws": self._stat_n}
        if self._split:
            st["lp0"] = self._lp0
        return st

    def _state_extra(self):
        return dict(super()._state_extra(), betas=[float(b) for b in self._betas], replicas=self._replicas,
                    swap_every=self._swap_every)

    def load_state_dict(self, sd):
        self._load_extra(sd["meta"].get("extra", {}))  # another ladder is refused before anything is overwritten
        super().load_state_dict(sd)
        self._swap_ran = False

    # -- surface -----------------------------------------------------------------------------------------------------------
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
        """Whether a column changed places with column i of the next rung in the last draw's swap round (bool, length C;
        set at the column on the lower rung index of the pair)."""
        return self._swapped.bool() if self._swap_ran else torch.zeros_like(self._swapped).bool()

    def _block_index(self):
        """The block e = r * T + t of every row of a draw (length C), the same in either half."""
        _, E, H = self._blocks
        return (torch.arange(self._C, dtype=torch.int64, device=self._ops.device) % (E * H)) // H

    def rung_index(self):
        """The rung of every row of a draw (length C): block e = r * T + t is rung t of replica r."""
        return self._block_index() % self._T

    def replica_index(self):
        """The replica of every row of a draw (length C)."""
        return self._block_index() // self._T

    def cold_rows(self):
        """The rows of a draw on rung 0: the ones that sample the target at betas[0]."""
        return torch.nonzero(self.rung_index() == 0).reshape(-1)

    # -- statistics: read only when asked ----------------------------------------------------------------------------------
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
        """Accepted proposals per proposed one, per rung -> [T]."""
        n = self._stat_draws() * self._replicas * self._per_rung
        acc = self._rung_acc.view(self._replicas, self._T).sum(dim=0).cpu().numpy().astype(np.float64)
        return acc / n if n else np.full(self._T, np.nan)

    def swap_rate(self) -> np.ndarray:
        """Accepted swaps per proposed one, per pair (t, t + 1) -> [T - 1] (NaN for a pair that never proposed)."""
        prop, acc = (c.view(-1, self._T).sum(dim=0).cpu().numpy().astype(np.float64)[:self._T - 1]
                     for c in (self._swap_prop, self._swap_acc))  # (summed over replicas and halves)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(prop > 0, acc / prop, np.nan)

    def mean_log_likelihood(self) -> np.ndarray:
        """The mean of ll over the columns of every rung and the draws since the last reset -> [replicas, T] (the integrand
        of thermodynamic integration)."""
        n = self._stat_draws() * self._per_rung
        s = self._ll_sum.view(self._replicas, self._T).cpu().numpy()
        return s / n if n else np.full(s.shape, np.nan)

    def log_evidence(self) -> np.ndarray:
        """The stepping-stone estimate of the log evidence, sum_t log mean_{rung t+1} exp((beta_t - beta_{t+1}) ll), per
        replica -> [replicas].  Needs the prior / likelihood split and a ladder from 1 down to 0."""
        if not self._split:
            raise ValueError(f"log_evidence needs the prior / likelihood split (a batched model with "
                             f"{' and '.join(self._SPLIT_METHODS)}): the base measure of a tempered log_density is improper")
        if self._betas[0] != 1.0 or self._betas[-1] != 0.0:
            raise ValueError(f"log_evidence needs betas[0] == 1 and betas[-1] == 0; found {self._betas[0]} and "
                             f"{self._betas[-1]}")
        n = self._stat_draws() * self._per_rung
        if not n:
            return np.full(self._replicas, np.nan)
        lse = self._lse.view(self._replicas, self._T).cpu().numpy()
        return (lse[:, 1:] - math.log(n)).sum(axis=1)


class TemperedStretcher(ReplicaLadder, Stretcher):
    """``betas``: strictly decreasing, finite, >= 0 (0 only for a model with a prior / likelihood split); ``replicas``:
    independent ladders side by side (whole replicas per rank: shard with ``chain_id0``); ``swap_every``: draws between swap
    rounds; ``walkers``: walkers per rung; ``init``: (replicas * T * walkers, D).  ``sample()`` returns every walker's
    ``theta`` and its UNTEMPERED log density; ``cold_rows()`` are the rows that sample the target itself (rung 0)."""

    _SPLIT_METHODS = ("log_prior", "log_likelihood")

    def __init__(self, model, betas, a: float = 2.0, walkers: Optional[int] = None, init=None, *, seed=None,
                 replicas: int = 1, swap_every: int = 1, chain_id0: int = 0, ops=None):
        self._ladder_args(model, betas, replicas, swap_every)
        super().__init__(model, a, walkers, init, seed=seed, ensembles=self._replicas * self._T, chain_id0=chain_id0,
                         ops=ops)

    # -- the tempered target ---------------------------------------------------------------------------------------------
    def _init_cache(self):
        f64 = dict(dtype=torch.float64, device=self._ops.device)
        self._ll, self._ll_p = self._lp, self._lp_p  # (the base class's cache and scratch, under the names used here)
        self._lp0 = torch.zeros(self._C, **f64) if self._split else None
        self._lp0_p = torch.zeros(self._C, **f64) if self._split else None
        self._init_ladder(self._H, 2)
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
        self._swap_round(out)
        self._accumulate()

    def _logp_out(self):
        return self._lp0 + self._ll if self._split else self._ll
