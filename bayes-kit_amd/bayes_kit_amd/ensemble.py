"""``Stretcher``: the affine-invariant ensemble sampler of Goodman & Weare (2010), for many walkers on the device.

The reference keeps its implementation in comments (``bayes_kit/ensemble.py:16-69``); this follows that intent: walkers in
two halves, every walker of the active half stretched along the line through a walker drawn (with replacement) from the
other half, ``z = square(uniform(1/sqrt(a), sqrt(a)))``, accepted with probability ``min(1, z^(D-1) p(theta*) / p(theta))``.
It needs only ``log_density`` and is invariant under any affine map of the parameters.

Walkers are chains along the lanes of the ``[D, C]`` state, ``C = ensembles * walkers``.  Column layout, with
``H = walkers / 2``: walker ``i`` of half ``s`` of ensemble ``e`` is column ``s * (C/2) + e * H + i``, so the active half of
EVERY ensemble is one contiguous column slice ``[s * C/2, (s + 1) * C/2)``: the model's log density op, ``bk_mh_accept`` and
``bk_select_columns`` run on ``[D, C/2]`` views with the state's pitch, the active half is written and the other only read.

One ``sample()`` is two half-updates, ``s = 0`` then ``s = 1``.  Each active walker draws three uniforms from ITS OWN
stream (``numpy.random.Philox(key=[seed, chain_id0 + column])``), in the order ``u_j`` (partner), ``u_z`` (stretch), ``u_a``
(accept); inactive walkers draw nothing, so after ``n`` draws every stream stands ``3 n`` uniforms further.  The proposal is
the ``bk_stretch_propose`` kernel (include/bkhip.h).  The log density of every walker is cached (the reference's
``TODO(carpenter)``).  ``tempering.TemperedStretcher`` runs the same draw on a ladder of tempered targets: it overrides the
accept step, the end of a draw and the cached density (``_accept``, ``_end_draw``, ``_init_cache``, ``_logp_out``), and
``tempering.ReplicaLadder``, mixed in before this class, the checkpoint's content and the acceptance read-out
(``_state_tensors``, ``_state_extra``, ``load_state_dict``, ``accept_rate``);
``differential_evolution.DifferentialEvolution`` runs another move in the same two half-updates: it overrides the draws and
the proposal of one half-update (``_propose``).
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._engine import ManyChainSampler


class _WalkerwiseModel:
    """A reference-style single-point model served walker by walker on the host: for small checks, not speed."""

    batched = True

    def __init__(self, model, device):
        self._model = model
        self._device = device

    def dims(self) -> int:
        return int(self._model.dims())

    def log_density(self, Theta):
        rows = Theta.detach().cpu().numpy()
        lp = [float(self._model.log_density(np.array(row))) for row in rows]
        return torch.tensor(lp, dtype=torch.float64, device=self._device)


class Stretcher(ManyChainSampler):
    """ensemble.py:9-69.  ``a``: stretch bound (>= 1); ``walkers``: walkers per ensemble (positive, even; default 2 D);
    ``init``: (C, D); ``ensembles``: independent ensembles side by side (all walkers of an ensemble live on one rank: shard
    whole ensembles with ``chain_id0``)."""

    def __init__(self, model, a: float = 2.0, walkers: Optional[int] = None, init=None, *, seed=None, ensembles: int = 1,
                 chain_id0: int = 0, ops=None):
        if a is None or not a >= 1:
            raise ValueError(f"stretch bound must be greater than or equal to 1; found {a=}")
        D = int(model.dims())
        if walkers is None:
            walkers = 2 * D
        if isinstance(walkers, bool) or not isinstance(walkers, (int, np.integer)) or walkers <= 0 or walkers % 2 != 0:
            raise ValueError(f"walkers must be strictly positive, even integer; found {walkers=}")
        if isinstance(ensembles, bool) or not isinstance(ensembles, (int, np.integer)) or ensembles <= 0:
            raise ValueError(f"ensembles must be a strictly positive integer; found {ensembles=}")
        self._a = float(a)
        self._sqrt_a = math.sqrt(self._a)
        self._inv_sqrt_a = 1 / self._sqrt_a
        self._walkers, self._ensembles = int(walkers), int(ensembles)
        self._H = self._walkers // 2
        C = self._ensembles * self._walkers
        if init is not None and tuple(np.shape(init)) != (C, D):
            raise ValueError(f"init must be shape of draw {(C, D)}; found {tuple(np.shape(init))}")
        ops = ops if ops is not None else _lib.default_ops()
        if getattr(model, "batched", False) is not True:
            model = _WalkerwiseModel(model, ops.device)
        self._setup(model, None, init, seed, C, chain_id0, ops)
        self._init_graph(False)
        dev = ops.device
        f64 = dict(dtype=torch.float64, device=dev)
        n = self._n = C // 2
        self._theta_p = self._new_state()  # (the state's shape and pitch: bk_select_columns shares one pitch)
        self._lp = torch.empty(C, **f64)
        self._lp_p = torch.empty(C, **f64)
        self._u_j = torch.zeros(C, **f64)
        self._u_z = torch.zeros(C, **f64)
        self._logu = torch.zeros(C, **f64)
        self._zterm = torch.zeros(C, **f64)
        self._partner = torch.zeros(C, dtype=torch.int32, device=dev)
        self._mask = torch.zeros(C, dtype=torch.uint8, device=dev)
        self._accepted = torch.zeros(1, dtype=torch.int32, device=dev)
        self._active = []  # per half: which walkers draw
        for s in (0, 1):
            act = torch.zeros(C, dtype=torch.uint8, device=dev)
            act[s * n:(s + 1) * n] = 1
            self._active.append(act)
        self._draws = 0
        self._init_cache()

    # -- the target: what a subclass with another one overrides (TemperedStretcher) ------------------------------------
    def _init_cache(self):
        """The cached log density of every walker at the start."""
        self._eval_logp(self._theta_dc, self._lp)

    def _accept(self, act):
        """The density of the proposals of the active slice `act`, and the accept test: the mask, the cache and the counter."""
        self._eval_logp(self._theta_p[:, act], self._lp_p[act])
        # log(u_a) < (lp* - lp) + (zterm - 0.0); on acceptance the kernel moves lp* into lp   (ensemble.py:54-57)
        self._ops.mh_accept(_lib.ACCEPT_MALA, self._lp[act], None, self._lp_p[act], self._zterm[act], self._logu[act],
                            self._mask[act], None, self._accepted)

    def _end_draw(self, out):
        """After both half-updates (`_draws` counts this draw); `out` is the copy of the state that sample() returns."""

    def _logp_out(self):
        return self._lp

    # -- state ------------------------------------------------------------------------------------------------------
    def _state_tensors(self):
        return {"theta": self._theta_dc, "lp": self._lp, "accepted": self._accepted}

    def _state_extra(self):
        return {"a": self._a, "walkers": self._walkers, "ensembles": self._ensembles}

    def _load_extra(self, extra):
        mine = self._state_extra()
        if extra and any(extra.get(k, v) != v for k, v in mine.items()):
            raise ValueError(f"checkpoint is for a {type(self).__name__} with {extra}, this one has {mine}")

    @property
    def walkers(self) -> int:
        return self._walkers

    @property
    def ensembles(self) -> int:
        return self._ensembles

    @property
    def last_accept(self):
        return self._mask.bool()

    @property
    def last_partner(self):
        """The column each walker was stretched against in the last draw (int32, length C)."""
        return self._partner.clone()

    def accept_rate(self) -> float:
        n = self._draws * self._C
        return float(self._accepted.item()) / n if n else float("nan")

    def ensemble_index(self):
        """The ensemble of every row of a draw (length C): row c is walker (c mod C/2) mod H of ensemble (c mod C/2) // H."""
        c = torch.arange(self._C, dtype=torch.int64, device=self._ops.device)
        return (c % self._n) // self._H

    # -- the move: what a subclass with another one overrides (differential_evolution) ------------------------------------
    def _propose(self, s, act):
        """The draws of the walkers of half `s` from their streams, and their proposals into the slice `act` of `_theta_p`
        (with `_zterm`, the proposal's term of the accept test, and `_logu`)."""
        ops, n = self._ops, self._n
        for u in (self._u_j, self._u_z):
            ops.uniform(self._rng_kind, self._rng_state, u, self._active[s])
        ops.log_uniform(self._rng_kind, self._rng_state, self._logu, self._active[s])
        ops.stretch_propose(self._theta_dc, s * n, (1 - s) * n, n, self._H, self._u_j[act], self._u_z[act],
                            self._inv_sqrt_a, self._sqrt_a, self._theta_p[:, act], self._zterm[act], self._partner[act])

    # -- one draw for every walker --------------------------------------------------------------------------------
    def sample(self):
        ops, n = self._ops, self._n
        th, thp = self._theta_dc, self._theta_p
        out = self._new_state()
        for s in (0, 1):
            act = slice(s * n, s * n + n)
            self._propose(s, act)
            self._accept(act)
            # this half stays as it is now for the rest of the draw: its columns of the returned array in the same pass
            ops.select_columns(self._mask[act], th[:, act], thp[:, act], None, None, out[:, act])
        self._draws += 1
        self._end_draw(out)
        self._out = out
        return self._draw_out(th, self._logp_out())
