"""``DifferentialEvolution``: the differential-evolution move (ter Braak 2006, DE-MC; Nelson et al. 2013; emcee's
``DEMove``) on ``Stretcher``'s two half-updates, and ``TemperedDifferentialEvolution``, the same move on the ladder of
``TemperedStretcher``.

Every walker ``k`` of the active half proposes from an ordered pair of DIFFERENT walkers ``j1 != j2`` drawn from the other
half of its own ensemble,

    theta* = theta_k + g (theta_j1 - theta_j2),      g = gamma0 (1 + sigma z),   z ~ N(0, 1)

The proposal is symmetric (the pair ``(j2, j1)`` is as likely and ``z`` is symmetric), so the accept test is
``min(1, p(theta*) / p(theta))`` with no Jacobian term; it is as affine invariant as the stretch move, its steps span every
direction the other half spans instead of one line, and with ``gamma0 = 1`` a walker lands where ``theta_j1`` is relative
to ``theta_j2``: in the other mode, if the two sit in different ones.  ``jump_every = m > 0`` makes every ``m``-th draw such
a mode-jumping draw (ter Braak's ``gamma = 1`` step); all other draws use ``gamma``, by default ``2.38 / sqrt(2 D)``.

The column layout, the caches, the accept step, the column select, the streams and the checkpoints are ``Stretcher``'s; only
``_propose`` differs; the tempered one takes its ladder (swap rounds, statistics, the ladder's share of a checkpoint) from
``TemperedStretcher``, that is from ``tempering.ReplicaLadder``, unchanged.  Each active walker draws from ITS OWN stream,
in this order: uniform ``u_1``, uniform ``u_2``, one standard normal (``Generator.standard_normal()``, bit for bit:
``bk_momentum_refresh`` on one masked row), the accept uniform; inactive walkers draw nothing.  The proposal is the
``bk_de_propose`` kernel (include/bkhip.h).

``sigma`` perturbs the SCALAR ``gamma`` only, so the moves of a walker stay inside the span of the other half's
differences: with ``H = walkers / 2 <= D`` that span has fewer than ``D`` directions and the sampler is not ergodic.  The
default is therefore ``walkers = max(4, 4 D)`` (``H = 2 D``), and explicit ``walkers`` with ``walkers // 2 <= D`` warn.
"""
from __future__ import annotations

import math
import warnings
from typing import Optional

import numpy as np
import torch

from .ensemble import Stretcher
from .tempering import TemperedStretcher


class _DEMove:
    """The differential-evolution ``_propose`` for a ``Stretcher`` (mix in BEFORE it)."""

    def _de_args(self, model, gamma, sigma, walkers, jump_every) -> int:
        """Validates and keeps the move's settings -> walkers (the default filled in)."""
        D = int(model.dims())
        if gamma is None:
            gamma = 2.38 / math.sqrt(2.0 * D)
        if isinstance(gamma, bool) or not isinstance(gamma, (int, float, np.integer, np.floating)) \
                or not math.isfinite(gamma) or not gamma > 0:
            raise ValueError(f"gamma must be finite and strictly positive; found {gamma=}")
        if isinstance(sigma, bool) or not isinstance(sigma, (int, float, np.integer, np.floating)) \
                or not math.isfinite(sigma) or not sigma >= 0:
            raise ValueError(f"sigma must be finite and greater than or equal to 0; found {sigma=}")
        if isinstance(jump_every, bool) or not isinstance(jump_every, (int, np.integer)) or jump_every < 0:
            raise ValueError(f"jump_every must be an integer greater than or equal to 0; found {jump_every=}")
        if walkers is None:
            walkers = max(4, 4 * D)
        elif isinstance(walkers, bool) or not isinstance(walkers, (int, np.integer)) or walkers < 4 or walkers % 2 != 0:
            raise ValueError(f"walkers must be an even integer greater than or equal to 4 (a pair of different walkers "
                             f"from each half); found {walkers=}")
        elif walkers // 2 <= D:
            warnings.warn(f"walkers // 2 = {walkers // 2} <= D = {D}: the differences of one half span fewer than D "
                          "directions and sigma perturbs the scalar gamma only, so the sampler is not ergodic; use more than "
                          f"{2 * D} walkers (the default is max(4, 4 D))", UserWarning, stacklevel=3)
        self._gamma, self._sigma, self._jump_every = float(gamma), float(sigma), int(jump_every)
        return int(walkers)

    def _de_buffers(self):
        C, dev = self._C, self._ops.device
        self._z = torch.zeros(1, C, dtype=torch.float64, device=dev)  # (one row of normals: bk_momentum_refresh's layout)
        self._partners = torch.zeros(2, C, dtype=torch.int32, device=dev)
        self._gamma_used = torch.zeros(C, dtype=torch.float64, device=dev)

    def _gamma0(self) -> float:
        """gamma of the draw in progress, number `_draws + 1`: 1.0 on every jump_every-th one."""
        return 1.0 if self._jump_every > 0 and (self._draws + 1) % self._jump_every == 0 else self._gamma

    def _propose(self, s, act):
        ops, n = self._ops, self._n
        kind, st, active = self._rng_kind, self._rng_state, self._active[s]
        ops.uniform(kind, st, self._u_j, active)
        ops.uniform(kind, st, self._u_z, active)
        ops.momentum_refresh(kind, st, None, 0.0, 1.0, self._z, None, None, active=active)
        ops.log_uniform(kind, st, self._logu, active)
        # (`_zterm` stays the zeros it was made as: the proposal is symmetric)
        ops.de_propose(self._theta_dc, s * n, (1 - s) * n, n, self._H, self._u_j[act], self._u_z[act], self._z[0, act],
                       self._gamma0(), self._sigma, self._theta_p[:, act], self._partners[0, act], self._partners[1, act],
                       self._gamma_used[act])

    def _state_extra(self):
        extra = super()._state_extra()
        del extra["a"]  # (the stretch bound is not a setting of this move)
        return dict(gamma=self._gamma, sigma=self._sigma, jump_every=self._jump_every, **extra)

    @property
    def gamma(self) -> float:
        return self._gamma

    @property
    def sigma(self) -> float:
        return self._sigma

    @property
    def jump_every(self) -> int:
        return self._jump_every

    @property
    def last_partner(self):
        raise AttributeError("a differential-evolution move has two partners: see last_partners")

    @property
    def last_partners(self):
        """The columns (j1, j2) each walker's step was taken from in the last draw (int32, [2, C])."""
        return self._partners.clone()

    @property
    def last_gamma(self):
        """The step g = gamma0 (1 + sigma z) of each walker in the last draw (float64, length C)."""
        return self._gamma_used.clone()


class DifferentialEvolution(_DEMove, Stretcher):
    """``gamma``: step along the difference of the pair (finite, > 0; default 2.38 / sqrt(2 D)); ``sigma``: relative spread
    of gamma per walker and half-update (finite, >= 0); ``walkers``: walkers per ensemble (even, >= 4; default
    max(4, 4 D)); ``jump_every``: every how many draws gamma is 1.0 (0: never); ``init``: (C, D); ``ensembles``: independent
    ensembles side by side (shard whole ensembles with ``chain_id0``)."""

    def __init__(self, model, gamma: Optional[float] = None, sigma: float = 1e-5, walkers: Optional[int] = None, init=None,
                 *, seed=None, ensembles: int = 1, jump_every: int = 0, chain_id0: int = 0, ops=None):
        walkers = self._de_args(model, gamma, sigma, walkers, jump_every)
        Stretcher.__init__(self, model, 2.0, walkers, init, seed=seed, ensembles=ensembles, chain_id0=chain_id0, ops=ops)
        self._de_buffers()


class TemperedDifferentialEvolution(_DEMove, TemperedStretcher):
    """``TemperedStretcher``'s ladder, tempered accept test, swap rounds and statistics on the differential-evolution
    move: ``betas``, ``replicas``, ``swap_every`` as there, ``gamma``, ``sigma``, ``walkers`` (per rung), ``jump_every`` as in
    ``DifferentialEvolution``.  One rung with ``betas = [1.0]`` is ``DifferentialEvolution``, bit for bit."""

    def __init__(self, model, betas, gamma: Optional[float] = None, sigma: float = 1e-5, walkers: Optional[int] = None,
                 init=None, *, seed=None, replicas: int = 1, swap_every: int = 1, jump_every: int = 0, chain_id0: int = 0,
                 ops=None):
        walkers = self._de_args(model, gamma, sigma, walkers, jump_every)
        TemperedStretcher.__init__(self, model, betas, 2.0, walkers, init, seed=seed, replicas=replicas,
                                   swap_every=swap_every, chain_id0=chain_id0, ops=ops)
        self._de_buffers()
