"""``TemperedHMC``: parallel tempering (replica exchange) for HMC, with one step size per rung, for high-dimensional
posteriors with separated modes.

A ladder of ``T`` inverse temperatures ``betas[0] > betas[1] > ...`` gives ``T`` rungs; a chain on rung ``t`` targets
``lp0(theta) + betas[t] * ll(theta)``.  A batched model with ``log_prior_gradient(Theta) -> (lp0, g0)`` and
``log_likelihood_gradient(Theta) -> (ll, gl)`` (``TorchPriorLikelihoodModel`` has both) is split: ``lp0`` is the prior, ``ll``
the likelihood, ``beta = 0`` is allowed and the ladder yields the evidence.  Any other batched model goes through the
engine's gradient bridge (``bk_eval``, ``bk_gradient``, ``log_density_gradient``): the whole log density is tempered, ``lp0``
is absent and every ``beta`` must be positive.

The ladder itself is ``tempering.ReplicaLadder``'s, shared with ``TemperedStretcher``: the check of ``betas``, ``replicas`` and
``swap_every``, the per-column tables, the swap round, the statistics and their read-outs, the index helpers and the
ladder's share of a checkpoint.  This module keeps what is HMC's: the step size of every rung, the cached gradients (which
it exchanges after a swap round), the draw and ``warmup()``.

Layout: ``C = replicas * T * chains`` columns, column ``c = (r * T + t) * H + i`` for chain ``i`` of rung ``t`` of replica
``r`` (``H = chains``, the rung fastest), so rungs ``t`` and ``t + 1`` of a replica are columns ``c`` and ``c + H``: the two
adjacent slices ``bk_replica_swap`` exchanges.  Every column carries its inverse temperature and its step size (and half of
it, and minus half of it) in ``[C]`` device vectors: the integrator kernels ``bk_tempered_kick_drift`` /
``bk_tempered_finish`` read them per column, because a hot rung is wider by about ``1 / sqrt(beta)`` and one step size for the
ladder either rejects on the cold rung or crawls on the hot ones.

A draw is ``HMCDiag``'s model-opaque draw: momentum (D normals) and its kinetic energy, the accept uniform, ``steps``
leapfrog steps with the gradient as a separate op between the kick+drift launches, the final half kick with the proposal's
kinetic energy, ``bk_tempered_hmc_accept``, ``bk_select_columns`` on the state and the cached gradients.  ``ll``, ``lp0`` and
their gradients are cached per column between draws.  After draw ``n = 1, 2, ...`` with ``n % swap_every == 0`` comes swap
round ``k = n / swap_every``: every pair ``(t, t + 1)`` with ``t % 2 == k % 2`` of every replica, chain ``i`` of rung ``t``
against chain ``i`` of rung ``t + 1`` (``TemperedStretcher``'s deterministic even-odd scheme).

Streams: every chain draws D normals and one uniform per draw from its own stream; in a swap round the chain on the LOWER
rung index of each pair draws one more uniform, and nobody else draws.

``warmup()`` tunes one step size per rung in this process: ranks that shard replicas (``chain_id0``) each adapt their own
step sizes from their own replicas, and nothing is exchanged between them.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._engine import ManyChainSampler
from .adapt import DualAveraging
from .tempering import ReplicaLadder, _positive_int


class TemperedHMC(ReplicaLadder, ManyChainSampler):
    """``betas``: strictly decreasing, finite, >= 0 (0 only for a split model); ``stepsize``: a scalar or one entry per rung;
    ``steps``: leapfrog steps (>= 1); ``chains``: chains per rung; ``replicas``: independent ladders side by side (whole
    replicas per rank: shard with ``chain_id0``); ``swap_every``: draws between swap rounds; ``init``: (replicas * T * chains,
    D).  ``sample()`` returns every chain's ``theta`` after the swap round and its UNTEMPERED log density; ``cold_rows()`` are
    the rows that sample the target itself (rung 0)."""

    _SPLIT_METHODS = ("log_prior_gradient", "log_likelihood_gradient")

    def __init__(self, model, betas, stepsize, steps, metric_diag=None, init=None, *, seed=None, chains=None,
                 replicas: int = 1, swap_every: int = 1, chain_id0: int = 0, ops=None):
        if getattr(model, "batched", False) is not True:
            raise ValueError("TemperedHMC needs a batched device model")
        self._ladder_args(model, betas, replicas, swap_every)
        if not _positive_int(steps):
            raise ValueError(f"steps must be a strictly positive integer; found {steps=}")
        E = self._replicas * self._T
        if chains is None and init is not None and np.ndim(init) == 2 and np.shape(init)[0] % E == 0:
            chains = int(np.shape(init)[0]) // E
        if not _positive_int(chains):
            raise ValueError(f"chains (per rung) must be a strictly positive integer; found {chains=}")
        self._H, self._steps = int(chains), int(steps)
        C, D = E * self._H, int(model.dims())
        eps = self._check_stepsizes(stepsize)
        if init is not None and tuple(np.shape(init)) != (C, D):
            raise ValueError(f"init must be shape of draw {(C, D)}; found {tuple(np.shape(init))}")
        ops = ops if ops is not None else _lib.default_ops()
        self._setup(model, metric_diag, init, seed, C, chain_id0, ops)
        self._init_graph(False)
        dev = ops.device
        f64 = dict(dtype=torch.float64, device=dev)
        self._thp, self._rho = self._new_state(), self._new_state()
        self._g_ll, self._gp_ll = self._new_state(), self._new_state()
        self._g_lp0 = self._new_state() if self._split else None
        self._gp_lp0 = self._new_state() if self._split else None
        self._ll, self._ll_p = torch.zeros(C, **f64), torch.zeros(C, **f64)
        self._lp0 = torch.zeros(C, **f64) if self._split else None
        self._lp0_p = torch.zeros(C, **f64) if self._split else None
        self._kin0, self._kin1, self._logu = (torch.zeros(C, **f64) for _ in range(3))
        self._mask = torch.zeros(C, dtype=torch.uint8, device=dev)
        self._init_ladder(self._H, 1)
        self._rung_host = self.rung_index().cpu().numpy()
        self._eps_col, self._half_col, self._neg_half_col = (torch.zeros(C, **f64) for _ in range(3))
        self._install_stepsizes(eps)
        self._draws = 0
        self._grad_parts(self._theta_dc, self._g_ll, self._g_lp0, self._ll, self._lp0)

    # -- step sizes ------------------------------------------------------------------------------------------------------
    def _check_stepsizes(self, stepsize) -> np.ndarray:
        e = np.asarray(stepsize, dtype=np.float64)
        if e.ndim == 0:
            e = np.full(self._T, float(e))
        if e.shape != (self._T,):
            raise ValueError(f"stepsize must be a scalar or one entry per rung ({self._T}); found shape {e.shape}")
        if not (np.isfinite(e).all() and (e > 0.0).all()):
            raise ValueError(f"stepsize must be finite and positive; found {stepsize=}")
        return e

    def _install_stepsizes(self, eps: np.ndarray):
        """eps, 0.5 * eps and -(0.5 * eps) of every column's rung, in place (the kernels keep reading these vectors)."""
        self._eps = eps.copy()
        col = eps[self._rung_host]
        half = 0.5 * col
        dev = self._ops.device
        self._eps_col.copy_(torch.from_numpy(col).to(dev))
        self._half_col.copy_(torch.from_numpy(half).to(dev))
        self._neg_half_col.copy_(torch.from_numpy(-half).to(dev))

    @property
    def stepsizes(self) -> np.ndarray:
        """The step size of every rung -> [T]."""
        return self._eps.copy()

    def set_stepsizes(self, stepsize):
        self._install_stepsizes(self._check_stepsizes(stepsize))

    # -- the target --------------------------------------------------------------------------------------------------------
    def _to_dc(self, g, out):
        """A model's (n, D) gradient into the chain-contiguous [D, n] array `out`."""
        n = out.shape[1]
        if g.dtype != torch.float64 or g.device != out.device:
            g = g.to(device=out.device, dtype=torch.float64)  # the kernels read raw fp64 pointers
        if tuple(g.shape) != (n, self._dim):
            raise ValueError(f"a gradient must have shape ({n}, {self._dim}), got {tuple(g.shape)}")
        self._ops.relayout(g.t(), out)

    def _grad_parts(self, theta_dc, gl_out, g0_out, ll_out, lp0_out):
        """The gradients of ll (and lp0) at theta_dc into the chain-contiguous arrays, and, where ll_out is given, the values."""
        if not self._split:
            self._materialize(self._eval_grad(theta_dc, gl_out, ll_out), gl_out)
            return
        self._grad_calls += 1
        m, Th = self._model, theta_dc.t()
        lp0, g0 = m.log_prior_gradient(Th)
        ll, gl = m.log_likelihood_gradient(Th)
        self._to_dc(g0, g0_out)
        self._to_dc(gl, gl_out)
        if ll_out is not None:
            lp0_out.copy_(lp0.reshape(-1))
            ll_out.copy_(ll.reshape(-1))

    # -- one draw for every chain, then the swap round ---------------------------------------------------------------------
    def sample(self):
        ops, H, L, m = self._ops, self._H, self._steps, self._metric_dev
        th, thp, rho = self._theta_dc, self._thp, self._rho
        beta, eps, half = self._beta_col, self._eps_col, self._half_col
        ops.momentum_refresh(self._rng_kind, self._rng_state, None, 0.0, 1.0, rho, m, self._kin0, None, self._rng_work)
        ops.log_uniform(self._rng_kind, self._rng_state, self._logu)
        for n in range(L):
            if n == 0:  # rho - eps/2 t + eps t: HMCDiag's first step, operation for operation
                ops.tempered_kick_drift(th, thp, rho, rho, self._g_ll, self._g_lp0, m, beta, eps, self._neg_half_col, eps)
            else:
                ops.tempered_kick_drift(thp, thp, rho, rho, self._gp_ll, self._gp_lp0, m, beta, eps, None, eps)
            last = n == L - 1
            self._grad_parts(thp, self._gp_ll, self._gp_lp0, self._ll_p if last else None, self._lp0_p if last else None)
        ops.tempered_finish(rho, None, self._gp_ll, self._gp_lp0, m, beta, half, self._kin1)
        ops.tempered_hmc_accept(self._ll, self._lp0, self._kin0, self._ll_p, self._lp0_p, self._kin1, beta, self._logu,
                                self._mask, self._rung_acc, H)
        out = self._new_state()
        ops.select_columns(self._mask, th, thp, self._g_ll, self._gp_ll, out)
        if self._split:
            ops.select_columns(self._mask, self._g_lp0, self._gp_lp0)
        self._draws += 1
        if self._swap_round(out):  # (the decision overwrote ll: the cached gradients follow by the exchange pass alone)
            ops.exchange_columns(self._g_ll, self._swapped, H)
            if self._split:
                ops.exchange_columns(self._g_lp0, self._swapped, H)
        self._accumulate()
        self._out = out
        return self._draw_out(th, self._lp0 + self._ll if self._split else self._ll)

    # -- warmup: one step size per rung ------------------------------------------------------------------------------------
    def warmup(self, draws, target_accept=0.8):
        """`draws` draws (swap rounds included) that tune every rung's step size: after each draw the exact number of
        accepted columns of every rung, divided by replicas * chains, feeds that rung's ``DualAveraging``; the averaged
        iterates are installed at the end and the statistics are reset.  One host read of T counters per draw.  The
        statistic is made of integers: the same report on every device.  Per process: a rank adapts from its own replicas.
        -> {"stepsizes": [T], "eps": [draws][T] (the step sizes each draw ran with), "alpha": [draws][T]}"""
        draws = self._check_warmup(draws, target_accept)
        R, T = self._replicas, self._T
        das = [DualAveraging(float(e), float(target_accept)) for e in self._eps]
        per_rung = float(R * self._H)
        seen = self._rung_acc.view(R, T).sum(dim=0).cpu().numpy().astype(np.int64)
        eps_hist, alpha_hist = [], []
        for it in range(draws):
            eps_hist.append([float(e) for e in self._eps])
            self.sample()
            now = self._rung_acc.view(R, T).sum(dim=0).cpu().numpy().astype(np.int64)  # the warmup draw's one host read
            alpha = [float(a) / per_rung for a in (now - seen)]
            seen = now
            alpha_hist.append(alpha)
            nxt = [da.step(a) for da, a in zip(das, alpha)]
            if it + 1 == draws:
                nxt = [da.final() for da in das]
            self._install_stepsizes(np.asarray(nxt, dtype=np.float64))
        self.reset_statistics()
        return {"stepsizes": [float(e) for e in self._eps], "eps": eps_hist, "alpha": alpha_hist}

    # -- state -------------------------------------------------------------------------------------------------------------
    def _state_tensors(self):
        st = super()._state_tensors()
        st["grad_ll"] = self._g_ll
        if self._split:
            st["grad_lp0"] = self._g_lp0
        return st

    def _state_extra(self):
        return dict(super()._state_extra(), chains_per_rung=self._H, steps=self._steps, split=self._split,
                    stepsizes=[float(e) for e in self._eps])

    def _load_extra(self, extra):
        """Refuses a checkpoint of other settings than this sampler's; the step sizes are the checkpoint's own."""
        mine = self._state_extra()
        del mine["stepsizes"]
        if any(extra.get(k) != v for k, v in mine.items()):
            raise ValueError(f"checkpoint is for a TemperedHMC with {extra}, this one has {mine}")
        self._check_stepsizes(extra["stepsizes"])

    def load_state_dict(self, sd):
        super().load_state_dict(sd)  # (`_load_extra` first: another ladder is refused before anything is overwritten)
        self._install_stepsizes(self._check_stepsizes(sd["meta"]["extra"]["stepsizes"]))

    # -- surface -----------------------------------------------------------------------------------------------------------
    @property
    def steps(self) -> int:
        return self._steps

    @property
    def chains_per_rung(self) -> int:
        return self._H

    @property
    def last_accept(self):
        return self._mask.bool()
