"""``TemperedHMC``: parallel tempering (replica exchange) for HMC, with one step size per rung, for high-dimensional
posteriors with separated modes.

A ladder of ``T`` inverse temperatures ``betas[0] > betas[1] > ...`` gives ``T`` rungs; a chain on rung ``t`` targets
``lp0(theta) + betas[t] * ll(theta)``.  A batched model with ``log_prior_gradient(Theta) -> (lp0, g0)`` and
``log_likelihood_gradient(Theta) -> (ll, gl)`` (``TorchPriorLikelihoodModel`` has both) is split: ``lp0`` is the prior, ``ll``
the likelihood, ``beta = 0`` is allowed and the ladder yields the evidence.  Any other batched model goes through the
engine's gradient bridge (``bk_eval``, ``bk_gradient``, ``log_density_gradient``): the whole log density is tempered, ``lp0``
is absent and every ``beta`` must be positive.

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

import math

import numpy as np
import torch

from . import _lib
from ._engine import ManyChainSampler
from .adapt import DualAveraging
from .tempering import _positive_int


class TemperedHMC(ManyChainSampler):
    """``betas``: strictly decreasing, finite, >= 0 (0 only for a split model); ``stepsize``: a scalar or one entry per rung;
    ``steps``: leapfrog steps (>= 1); ``chains``: chains per rung; ``replicas``: independent ladders side by side (whole
    replicas per rank: shard with ``chain_id0``); ``swap_every``: draws between swap rounds; ``init``: (replicas * T * chains,
    D).  ``sample()`` returns every chain's ``theta`` after the swap round and its UNTEMPERED log density; ``cold_rows()`` are
    the rows that sample the target itself (rung 0)."""

    def __init__(self, model, betas, stepsize, steps, metric_diag=None, init=None, *, seed=None, chains=None,
                 replicas: int = 1, swap_every: int = 1, chain_id0: int = 0, ops=None):
        if getattr(model, "batched", False) is not True:
            raise ValueError("TemperedHMC needs a batched device model")
        b = np.asarray(betas, dtype=np.float64)
        if b.ndim != 1 or b.shape[0] < 1 or not np.isfinite(b).all() or (b < 0.0).any() or (np.diff(b) >= 0.0).any():
            raise ValueError(f"betas must be a strictly decreasing sequence of finite values >= 0; found {betas=}")
        if not _positive_int(replicas):
            raise ValueError(f"replicas must be a strictly positive integer; found {replicas=}")
        if not _positive_int(swap_every):
            raise ValueError(f"swap_every must be a strictly positive integer; found {swap_every=}")
        if not _positive_int(steps):
            raise ValueError(f"steps must be a strictly positive integer; found {steps=}")
        T = int(b.shape[0])
        if chains is None and init is not None and np.ndim(init) == 2 and np.shape(init)[0] % (int(replicas) * T) == 0:
            chains = int(np.shape(init)[0]) // (int(replicas) * T)
        if not _positive_int(chains):
            raise ValueError(f"chains (per rung) must be a strictly positive integer; found {chains=}")
        self._split = (callable(getattr(model, "log_prior_gradient", None))
                       and callable(getattr(model, "log_likelihood_gradient", None)))
        if not self._split and b[-1] <= 0.0:
            raise ValueError("beta = 0 needs a batched model with log_prior_gradient and log_likelihood_gradient: without "
                             "that split the whole log density is tempered and every beta must be > 0")
        self._betas = b
        self._T, self._replicas, self._swap_every = T, int(replicas), int(swap_every)
        self._H, self._steps = int(chains), int(steps)
        self._E = self._replicas * T
        C, D = self._E * self._H, int(model.dims())
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
        self._swapped = torch.zeros(C, dtype=torch.uint8, device=dev)
        self._swap_ran = False
        rung = self.rung_index()
        self._rung_host = rung.cpu().numpy()
        self._beta_col = torch.as_tensor(b, **f64)[rung].contiguous()
        self._eps_col, self._half_col, self._neg_half_col = (torch.zeros(C, **f64) for _ in range(3))
        self._install_stepsizes(eps)
        self._lower = []  # per parity: the chains on the lower rung index of a pair (they draw the swap's uniform)
        for p in (0, 1):
            low = ((rung % 2 == p) & (rung + 1 < T)).to(torch.uint8).contiguous()
            self._lower.append(low if bool(low.any()) else None)
        # statistics, all on the device; block e = r * T + t of H columns is rung t of replica r
        E = self._E
        self._rung_acc = torch.zeros(E, dtype=torch.int32, device=dev)
        self._swap_prop = torch.zeros(E, dtype=torch.int32, device=dev)
        self._swap_acc = torch.zeros(E, dtype=torch.int32, device=dev)
        self._ll_sum = torch.zeros(E, **f64)
        self._lse = torch.full((E,), -math.inf, **f64)
        self._stat_n = torch.zeros(1, dtype=torch.int64)  # (host: draws the statistics cover)
        # (beta_{t-1} - beta_t) of every block's rung t; 0.0 for rung 0, whose entry of `_lse` is never read
        db = np.concatenate([[0.0], b[:-1] - b[1:]])
        self._dbeta_e = torch.as_tensor(np.tile(db, self._replicas), **f64)
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
        self._swap_ran = False
        if self._draws % self._swap_every == 0:
            low = self._lower[(self._draws // self._swap_every) % 2]
            if low is not None:
                ops.log_uniform(self._rng_kind, self._rng_state, self._logu, low)
                # the state and the copy of it that this draw returns change places alike; the decision overwrites ll, so the
                # cached gradients follow by the exchange pass alone
                ops.replica_swap(th, out, self._ll, self._lp0, beta, self._logu, low, self._swapped, self._swap_prop,
                                 self._swap_acc, H)
                ops.exchange_columns(self._g_ll, self._swapped, H)
                if self._split:
                    ops.exchange_columns(self._g_lp0, self._swapped, H)
                self._swap_ran = True
        self._accumulate()
        self._out = out
        return self._draw_out(th, self._lp0 + self._ll if self._split else self._ll)

    def _accumulate(self):
        """This draw's share of the running statistics: per block the sum of ll, and the log-sum-exp of
        (beta_{t-1} - beta_t) ll over the chains of rung t (the stepping stone from rung t to rung t - 1)."""
        ll = self._ll.view(self._E, self._H)
        self._ll_sum += ll.sum(dim=1)
        torch.logaddexp(self._lse, torch.logsumexp(ll * self._dbeta_e[:, None], dim=1), out=self._lse)
        self._stat_n += 1

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
        st = {"theta": self._theta_dc, "ll": self._ll, "grad_ll": self._g_ll, "rung_accepted": self._rung_acc,
              "swap_proposed": self._swap_prop, "swap_accepted": self._swap_acc, "ll_sum": self._ll_sum, "lse": self._lse,
              "stat_draws": self._stat_n}
        if self._split:
            st["lp0"] = self._lp0
            st["grad_lp0"] = self._g_lp0
        return st

    def _ladder(self):
        return {"betas": [float(b) for b in self._betas], "chains_per_rung": self._H, "replicas": self._replicas,
                "swap_every": self._swap_every, "steps": self._steps, "split": self._split}

    def _state_extra(self):
        return dict(self._ladder(), stepsizes=[float(e) for e in self._eps])

    def _check_ladder(self, extra):
        mine = self._ladder()
        if any(extra.get(k) != v for k, v in mine.items()):
            raise ValueError(f"checkpoint is for a TemperedHMC with {extra}, this one has {mine}")
        return self._check_stepsizes(extra["stepsizes"])

    def load_state_dict(self, sd):
        eps = self._check_ladder(sd["meta"].get("extra", {}))  # another ladder is refused before anything is overwritten
        super().load_state_dict(sd)
        self._install_stepsizes(eps)
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
    def steps(self) -> int:
        return self._steps

    @property
    def chains_per_rung(self) -> int:
        return self._H

    @property
    def last_accept(self):
        return self._mask.bool()

    @property
    def last_swapped(self):
        """Whether a chain changed places with chain i of the next rung in the last draw's swap round (bool, length C; set
        at the chain on the lower rung index of the pair)."""
        return self._swapped.bool() if self._swap_ran else torch.zeros_like(self._swapped).bool()

    def _block_index(self):
        return torch.arange(self._C, dtype=torch.int64, device=self._ops.device) // self._H

    def rung_index(self):
        """The rung of every row of a draw (length C): block e = r * T + t of H rows is rung t of replica r."""
        return self._block_index() % self._T

    def replica_index(self):
        """The replica of every row of a draw (length C)."""
        return self._block_index() // self._T

    def cold_rows(self):
        """The rows of a draw on rung 0: the chains that sample the target at betas[0]."""
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
        """Accepted proposals per draw and chain, per rung -> [T]."""
        n = self._stat_draws() * self._replicas * self._H
        acc = self._rung_acc.view(self._replicas, self._T).sum(dim=0).cpu().numpy().astype(np.float64)
        return acc / n if n else np.full(self._T, np.nan)

    def swap_rate(self) -> np.ndarray:
        """Accepted swaps per proposed one, per pair (t, t + 1) -> [T - 1] (NaN for a pair that never proposed)."""
        shape = (self._replicas, self._T)
        prop = self._swap_prop.view(shape).sum(dim=0).cpu().numpy().astype(np.float64)[:self._T - 1]
        acc = self._swap_acc.view(shape).sum(dim=0).cpu().numpy().astype(np.float64)[:self._T - 1]
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(prop > 0, acc / prop, np.nan)

    def mean_log_likelihood(self) -> np.ndarray:
        """The mean of ll over the chains of every rung and the draws since the last reset -> [replicas, T] (the integrand
        of thermodynamic integration)."""
        n = self._stat_draws() * self._H
        s = self._ll_sum.view(self._replicas, self._T).cpu().numpy()
        return s / n if n else np.full(s.shape, np.nan)

    def log_evidence(self) -> np.ndarray:
        """The stepping-stone estimate of the log evidence, sum_t log mean_{rung t+1} exp((beta_t - beta_{t+1}) ll), per
        replica -> [replicas].  Needs the prior / likelihood split and a ladder from 1 down to 0."""
        if not self._split:
            raise ValueError("log_evidence needs a model with the prior / likelihood split: the base measure of a tempered "
                             "log_density is improper")
        if self._betas[0] != 1.0 or self._betas[-1] != 0.0:
            raise ValueError(f"log_evidence needs betas[0] == 1 and betas[-1] == 0; found {self._betas[0]} and "
                             f"{self._betas[-1]}")
        n = self._stat_draws() * self._H
        if not n:
            return np.full(self._replicas, np.nan)
        lse = self._lse.view(self._replicas, self._T).cpu().numpy()
        return (lse[:, 1:] - math.log(n)).sum(axis=1)
