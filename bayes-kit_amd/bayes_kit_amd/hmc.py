"""Many-chain static-trajectory HMC on the GPU: drop-in for ``bayes_kit/hmc.py:8-63``.

Same constructor signature and ``sample() -> (theta, logp)`` / iterator protocol as the
reference's ``HMCDiag``; the momentum draw, leapfrog integrator, Metropolis accept and the
per-chain random streams are HIP kernels behind the C ABI of include/bkhip.h.

Per draw and chain (reference lines in brackets):
  rho ~ N(0, I) from the chain's stream, kin0 = 1/2 rho.(m*rho)            [hmc.py:56, :37]
  back half-step + L x (kick, drift, gradient) + forward half-step       [hmc.py:40-53]
  accept iff log(u) < (lp1 - kin1) - (lp0 - kin0), u always drawn        [hmc.py:57-63]
and the JOINT log density is returned (hmc.py:62-63).

Model calls.  With a reference-style single-chain model the call pattern of the reference is
kept exactly (2 ``log_density`` + ``steps+1`` ``log_density_gradient`` per draw,
test/test_hmc.py:22-35).  With a batched device model the sampler keeps (logp, grad) of the
current point across draws and uses the logp returned with the last gradient of the
trajectory: ``steps`` model calls per draw, bitwise the same results for any model whose
``log_density`` equals the first output of ``log_density_gradient``.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _lib
from ._engine import LookAhead, ManyChainSampler
from .adapt import TrajectoryAdam, jitter_steps, shrink_estimate
from .diagnostics import EnergyDiagnostics, RunningCovariance, _gather_sum


class TrajectoryObserver:
    """warmup(adapt_trajectory=True): feeds adapt.TrajectoryAdam with every draw's trajectory statistic (_stat[3:5]), assigns
    the sampler's trajectory length for the next draw and keeps the report's histories."""

    def __init__(self, sampler):
        self._s, self._ta = sampler, TrajectoryAdam(sampler._T)
        self._T_hist, self._steps_hist, self._nonfinite = [], [], 0

    def after_draw(self, tot, eps, window_end, last):
        s = self._s
        self._T_hist.append(float(s._T))
        self._steps_hist.append(int(s._steps))
        self._nonfinite += int(tot[4])
        s._T = self._ta.step(float(tot[3]), float(tot[0]), s._steps * eps, eps, s._max_steps)
        if window_end:
            self._ta.restart()  # (the geometry changes with the metric installed next)
        if last:
            s._T = self._ta.final()

    def report(self):
        return dict(trajectory_length=float(self._s._T), T=self._T_hist, steps=self._steps_hist,
                    nonfinite_chains=self._nonfinite)


class HMCDiag(ManyChainSampler):
    TUNING = ("graph", "prefetch_rng", "tune_placement", "chain_tile")
    _STEP_SIZE = "_stepsize"

    def __init__(
        self,
        model,
        stepsize: float,
        steps: int,
        metric_diag=None,
        init=None,
        seed=None,
        *,
        chains: Optional[int] = None,
        chain_id0: int = 0,
        path: str = "auto",
        metric_dense=None,
        precond_diag=None,
        trajectory_length: Optional[float] = None,
        max_steps: int = 1024,
        tuning: Optional[dict] = None,
        ops=None,
        **knobs,
    ):
        """The reference's arguments (hmc.py:9-17), then the engine's (ManyChainSampler: chains, chain_id0, path, tuning,
        ops) and ``metric_dense`` (extension: a dense velocity covariance, fp64 MFMA GEMMs).  Tuning knobs (none changes a
        result): ``graph`` (replay a draw as one hipGraph; default: small launch-bound shapes), ``prefetch_rng`` (the next
        draw's randomness on a side stream; default on, except that the tile-major loop generates each tile's in line
        unless True is given explicitly), ``tune_placement`` (time which allocation plays which role), ``chain_tile`` (chains per Infinity-Cache tile).

        ``precond_diag`` (extension; exclusive with metric_diag and metric_dense): a length-D vector v of velocity variances,
        ideally the posterior variances -- the proper diagonal preconditioner, ``oracle.samplers.HMCDense`` with M = diag(v)
        at the cost of the elementwise kernels: rho = 0.0 + sqrt(v)*z, kick rho += eps*(v*grad), kinetic energy
        1/2 rho.(rho/v).  Every path supports it and gives the same draws bit for bit: the built-in Gaussians and
        stay on the whole-draw kernel (its preconditioned instantiation), "step" and "opaque" use the preconditioned refresh
        and finish launches around the unchanged kick/drift kernels.  Two kinds of model fall back to one launch per leapfrog
        step while a preconditioner is set: a lane-spread density (bk_hmc_proposal sums the kinetic energy inside its
        launch), and an elementwise from_source / traced density (the whole-draw kernel compiled with it has no
        preconditioned export; it is HBM-bound there instead of register-resident).  ``set_precond_diag`` replaces it between draws,
        ``warmup`` estimates it.

        ``trajectory_length`` (extension): an integration TIME T instead of a fixed number of steps, jittered from draw to
        draw -- jittered draw n = 1, 2, ... takes L_n = min(max_steps, max(1, ceil(h_n T / eps))) leapfrog steps, h_n the
        base-2 radical inverse of n (1/2, 1/4, 3/4, 1/8, ...) and eps the step size of that draw; ``steps`` is then assigned
        L_n before every draw.  The jitter consumes no random numbers: stream positions are those of a fixed ``steps``.  A
        captured draw bakes ``steps`` in, so a graph chosen by default is switched off and an explicit ``graph=True`` is
        refused.  ``set_trajectory_length`` changes it between draws (None: back to a fixed ``steps``),
        ``warmup(adapt_trajectory=True)`` learns it."""
        fuse_builtin, fuse_steps = self._resolve_path(path)
        tn = self._resolve_tuning(tuning, knobs)
        chain_tile, graph = tn.get("chain_tile"), tn.get("graph")
        prefetch_rng, tune_placement = tn.get("prefetch_rng"), tn.get("tune_placement")
        self._stepsize = stepsize
        self._steps = steps
        self._chees = None     # warmup(adapt_trajectory=True): the scratch of the trajectory statistic (bk_chees_*)
        # prefetch_rng (decided below); per slot the stream table before that slot's normals were generated
        self._prefetch, self._snap = False, None
        self._T, self._jitter_n, self._last_steps = None, 0, None
        self._max_steps = self._check_max_steps(max_steps)
        self._graph_explicit = graph is True
        if trajectory_length is not None:
            self._T, self._steps_fixed = self._check_T(trajectory_length), steps
            if self._graph_explicit:
                raise ValueError("graph=True cannot be combined with trajectory_length: a captured draw bakes `steps` in")
            graph = False
        if precond_diag is not None and (metric_diag is not None or metric_dense is not None):
            raise ValueError("give precond_diag or metric_diag / metric_dense, not both")
        self._setup(model, metric_diag, init, seed, chains, chain_id0, ops)
        # Dense metric (extension; the reference only has metric_diag, and its literal
        # semantics -- rho ~ N(0, I), kick with m*grad, kinetic rho.(m*rho) -- leave the target
        # invariant only for m = 1).  The dense form is the proper
        # preconditioned HMC in the same (theta, velocity) variables: M = velocity covariance
        # (the inverse mass matrix; ideally ~ the posterior covariance),
        #     rho = chol(M) @ z,  z ~ N(0, I) from the chain's stream
        #     kick  rho += eps * (M @ grad),  drift  theta += eps * rho   [hmc.py:46-52 shape]
        #     kinetic energy 1/2 rho . (M^-1 @ rho)
        # and it reduces to the reference path exactly for M = I.  Every `matrix @ all chains`
        # is one fp64 MFMA GEMM (bk_dense_metric_apply).
        self._M = None
        if metric_dense is not None:
            if metric_diag is not None:
                raise ValueError("give metric_diag or metric_dense, not both")
            if not self._batched:
                raise ValueError("metric_dense needs a batched device model")
            self._install_metric_dense(metric_dense)
            fuse_builtin = False
        if precond_diag is not None:
            self._install_precond(precond_diag)
        self._init_graph(graph, prefetch_rng)
        self._graph_built = self._use_graph  # (what set_trajectory_length(None) goes back to)
        # built-in separable targets (and separable densities compiled from source) run the whole draw in
        # registers (bk_hmc_draw_gaussian): generator, ONE pass over the state (trajectory + kin0 + kin1 +
        # end-point log density), accept, select; results are bit-identical to the step-by-step path.  With
        # Philox streams the momentum is consumed chain-major, straight from the wavefront-per-chain
        # generator: no transpose, no kinetic-energy pass.
        self._fused_draw = (bool(fuse_builtin) and self._batched and self._M is None and hasattr(model, "bk_hmc_draw"))
        # ... with a preconditioner only where the model has the preconditioned form of that kernel (bk_hmc_draw_precond:
        # the built-in Gaussians); a density compiled from source (CTarget.from_source, TorchModel(compile=True)) then runs
        # step by step -- one launch per leapfrog step with its density inlined -- with the same draws bit for bit
        if self._pd is not None and not hasattr(model, "bk_hmc_draw_precond"):
            self._fused_draw = False
        self._fused = self._fused_draw  # whole-trajectory kernels in use: the whole draw is the only such path
        # ... a lane-spread density (bk.Funnel, CTarget.from_source(form="lanes")) runs the whole trajectory -- gradient
        # inlined, theta / rho register-resident, the proposal's gradient, log density and kinetic energy out -- as ONE launch
        # (bk_hmc_proposal: the delayed-rejection proposal kernel with hmc.py's first kick); the step-by-step path otherwise
        # issues ONE launch per leapfrog step where the model has bk_leapfrog_step
        self._lanes_traj = (bool(fuse_builtin) and self._batched and self._M is None and hasattr(model, "bk_hmc_proposal"))
        self._step_hook = (bool(fuse_steps) and self._batched and self._M is None and hasattr(model, "bk_leapfrog_step"))
        # ... and ONE launch per trajectory where it has bk_leapfrog_trajectory (a per-chain density compiled from source:
        # theta in registers, rho in LDS through all L steps), followed by the library's finish launch
        self._traj_hook = (bool(fuse_builtin) and self._step_hook and hasattr(model, "bk_leapfrog_trajectory"))
        self._chain_tile = self._pick_tile(chain_tile)
        self._fused_zt = self._fused_draw and self._rng_kind == _lib.RNG_PHILOX and self._dim >= 32
        D, C, dev = self._dim, self._C, self._ops.device
        f64 = dict(dtype=torch.float64, device=dev)
        # The tile-major schedule refreshes each tile's momentum into the tile's own workspace (_draw_tile_major): a sampler
        # that can take it owns no full-width momentum and no full-size generator scratch until a path that needs them
        # runs (_rho_full: the untiled loop, a ChEES warm-up, L = 0); a replayed hipGraph allocates up front.  An EXPLICIT
        # prefetch_rng=True is honoured as what it asks for -- the whole next draw's randomness generated ahead at full width
        # on the side stream, the tiles' first steps reading their columns of it, the schedule before the per-tile refresh --
        # while the default leaves the choice to the sampler, which on this loop generates in line (33.85 -> 33.25 ms per draw
        # at 65,536 x 1,024, profiles/cache_tiles.md section 9).
        self._tile_ahead = prefetch_rng is True and self._batched and not self._use_graph
        lazy = self._tile_rng and not self._use_graph and not self._tile_ahead
        self._work_dropped = lazy and self._rng_work is not None
        if lazy:
            self._rng_work = None  # (the engine's full-size scratch drew the initial state; _rho_full brings it back)
        self._rho_bufs = [None if (self._fused_zt or lazy) else torch.empty((D, C), **f64)]
        self._theta_p = torch.empty((D, C), **f64)
        self._grad = torch.empty((D, C), **f64)      # gradient at the current point
        self._grad_p = torch.empty((D, C), **f64)    # gradient along / at the end of the trajectory
        self._lp = torch.empty(C, **f64)
        self._lp_p = torch.empty(C, **f64)
        self._kin0_bufs = [torch.empty(C, **f64)]
        self._kin1 = torch.empty(C, **f64)
        self._logu_bufs = [torch.empty(C, **f64)]
        self._ret = torch.empty(C, **f64)
        self._mask = torch.empty(C, dtype=torch.uint8, device=dev)
        # tile-major schedule: the momentum of the tile in flight, [D, T] contiguous, and the generator's scratch for its T
        # chains (_tile_workspace; allocated below: never inside a capture)
        self._rho_tile, self._tile_work = None, None
        self._accepted = torch.zeros(1, dtype=torch.int32, device=dev)
        if self._fused_draw:
            self._part = torch.empty(12 * C, **f64)    # quarter partials of the three per-chain sums
        if self._fused_zt:
            dp = (D + 7) // 8 * 8
            self._zt_bufs = [torch.empty((C, dp), **f64)]  # (the momentum never exists in the state layout)
        if self._M is not None:
            self._mv = torch.empty((D, C), **f64)      # M @ grad along the trajectory
            self._mv_rng = torch.empty((D, C), **f64)  # M @ rho of the (possibly prefetched) momentum
        self._have_cache = False
        self._draws = 0
        # `self._theta = theta_prop` (hmc.py:61) as a REBIND: with a batched model and eager launches the
        # blend of state and proposal is written to a fresh array that becomes the state and is what sample()
        # returns (never written again): one array written instead of the in-place select's two
        # (bk_blend_columns).  A replayed hipGraph needs fixed addresses and keeps the in-place select.
        self._rebind = self._batched and not self._use_graph
        # Randomness of draw n+1 (momentum, its kinetic energy, the accept uniform) does not
        # depend on draw n, and the reference consumes it in a fixed order (D normals, then one
        # uniform: hmc.py:56,60).  With prefetch_rng it is generated on a second HIP stream
        # while draw n's trajectory streams through HBM on the main one: the RNG kernels are
        # integer bound and a small fraction of a draw, so they hide under the HBM-bound kernels.
        # A hipGraph replay is launch-free already and its graph stays linear (ManyChainSampler: a forked
        # capture is slower and unsafe on this ROCm): with graph=True the randomness is generated in line,
        # whatever prefetch_rng says -- the draws are bit-identical either way.
        if prefetch_rng is None:
            prefetch_rng = self._batched and self._ops.device.type == "cuda"
        self._prefetch = bool(prefetch_rng) and self._batched and not self._use_graph
        self._pf_kin_stale = False
        if self._prefetch:
            if self._fused_zt:
                self._zt_bufs.append(torch.empty_like(self._zt_bufs[0]))
                self._rho_bufs.append(None)
            else:
                self._rho_bufs.append(None if lazy else torch.empty((D, C), **f64))
            self._kin0_bufs.append(torch.empty(C, **f64))
            self._logu_bufs.append(torch.empty(C, **f64))
            self._ahead = LookAhead(dev)
            if self._fused_zt:
                self._snap = [torch.empty_like(self._rng_state) for _ in range(2)]
            else:
                self._rng_logical = self._rng_state.clone()  # stream position after the last finished draw
        if self._tile_rng:
            self._tile_workspace()
        self.placement = None
        if self._wants_placement_tuning(tune_placement) and not self._fused and self._M is None:
            self._tune_placement()

    def _install_metric_dense(self, metric_dense):
        if isinstance(metric_dense, torch.Tensor) and metric_dense.dim() == 1 and self._M is not None:
            # a DIAGONAL metric given by its entries (the SMC's per-temperature adaptation): factor and inverse are
            # elementwise, formed on the device -- no host round trip, no Cholesky of a D x D matrix
            v = metric_dense.to(device=self._ops.device, dtype=torch.float64)
            if v.shape[0] != self._dim:
                raise ValueError(f"a diagonal metric needs {self._dim} entries")
            self._M.copy_(torch.diag(v))
            self._M_chol.copy_(torch.diag(torch.sqrt(v)))
            self._M_inv.copy_(torch.diag(1.0 / v))
            return
        Mt = torch.as_tensor(metric_dense, dtype=torch.float64).cpu()
        if tuple(Mt.shape) != (self._dim, self._dim):
            raise ValueError(f"metric_dense must be ({self._dim}, {self._dim})")
        Mt = 0.5 * (Mt + Mt.t())
        dev_ = self._ops.device
        chol = torch.linalg.cholesky(Mt)   # host-side set-up
        inv = torch.linalg.inv(Mt)
        inv = 0.5 * (inv + inv.t())
        if self._M is None:
            self._M, self._M_chol, self._M_inv = (x.to(dev_).contiguous() for x in (Mt, chol, inv))
        else:  # in place: launches already queued (or captured) keep pointing at these buffers
            self._M.copy_(Mt)
            self._M_chol.copy_(chol)
            self._M_inv.copy_(inv)

    def set_metric_dense(self, metric_dense):
        """Replace the dense metric of a sampler that was built with one (an adaptation between draws: e.g. the
        tempered SMC re-estimates it from its particles at every temperature); a 1-D tensor = the entries of a diagonal one.  Momenta generated ahead with the old
        metric (prefetch_rng) are discarded: build such samplers with prefetch_rng=False to keep the stream order."""
        if self._M is None:
            raise ValueError("this sampler was built without metric_dense")
        self._install_metric_dense(metric_dense)
        self._drop_ahead(rewind=False)

    @property
    def metric_dense(self):
        """The dense metric as a host array (None when the sampler was built without one)."""
        return None if self._M is None else self._M.cpu().numpy().copy()

    # -- randomness generated ahead: the two places that know where it leaves the stream ----------------------
    def _stream_position(self):
        """The tensor that holds the logical stream position (a sampler's without prefetch_rng): the table -- while the next
        draw's randomness is generated ahead, the table as it was when that generation began, which is snap[slot], written
        by the chain-major generator itself, or else _rng_logical, a copy queued in front of the generator."""
        if self._prefetch and self._ahead.ahead:
            return self._rng_logical if self._snap is None else self._snap[self._ahead.slot]
        return self._rng_state

    def _drop_ahead(self, rewind):
        """Between two draws: drop the randomness generated ahead, once its generator has finished (a GPU-side wait);
        rewind: and take the stream back to where its generation began, for the next draw to generate it again."""
        if self._prefetch and self._ahead.ahead:
            position = self._stream_position()
            self._ahead.drop(wait=True)
            if rewind:
                self._rng_state.copy_(position)

    # -- the proper diagonal preconditioner -----------------------------------------------------------
    def _install_precond(self, v):
        """The preconditioner v, packed (_pack_precond); the kick kernels see its first row as their metric."""
        if self._M is not None or (self._pd is None and self._metric_dev is not None):
            raise ValueError("precond_diag cannot be combined with metric_diag / metric_dense")
        if self._pack_precond(v):
            self._metric_dev, self._metric_identity = self._pd[0], False
            self._drop_graphs()  # the captured launches had no preconditioner: capture again

    def set_precond_diag(self, v):
        """Set or replace the diagonal preconditioner between draws (see ``precond_diag``).  Changes no stream position:
        the chain-major generator keeps raw normals, which only their consumer scales; a momentum generated ahead in the
        state layout (prefetch_rng) carries the old scale, so it is dropped and regenerated from the stream position it
        started at."""
        self._install_precond(v)
        if self._fused_draw and not hasattr(self._model, "bk_hmc_draw_precond"):
            self._leave_whole_draw()
        if not self._fused_zt:
            self._drop_ahead(rewind=True)

    def _leave_whole_draw(self):
        """From the whole-draw kernel to the step-by-step path between two draws (a preconditioner was set on a model whose
        whole-draw hook has no preconditioned form): the stream goes back to where the next draw's randomness began, the
        momentum gets its state-layout buffers, and the cached gradient is evaluated again (the whole-draw path keeps the
        log density only; the same kernel gives the same value)."""
        self._drop_ahead(rewind=True)
        self._fused_draw = self._fused = self._fused_zt = False
        self._rho_bufs = [r if r is not None else torch.empty_like(self._thp_raw) for r in self._rho_bufs]
        if self._prefetch and self._snap is not None:
            self._snap, self._rng_logical = None, self._rng_state.clone()
        self._have_cache = False
        self._drop_graphs()

    # -- a jittered trajectory length ------------------------------------------------------------------
    @staticmethod
    def _check_T(T):
        try:
            Tf = float(T)
        except (TypeError, ValueError):
            raise ValueError(f"trajectory_length must be a finite, positive number, got {T!r}") from None
        if not (np.isfinite(Tf) and Tf > 0.0):
            raise ValueError(f"trajectory_length must be a finite, positive number, got {T!r}")
        return Tf

    @staticmethod
    def _check_max_steps(n):
        if isinstance(n, bool) or int(n) != n or int(n) < 1:
            raise ValueError(f"max_steps must be an integer >= 1, got {n!r}")
        return int(n)

    def set_trajectory_length(self, T):
        """Jitter the trajectory around the integration time T from the next draw on (see ``trajectory_length``); None goes
        back to the fixed ``steps`` it had before.  The jitter counter is kept."""
        if T is None:
            if self._T is not None:
                self._steps = self._steps_fixed
            self._T = None
            if self._graph_built and not self._use_graph:
                self._use_graph = True
                self._drop_graphs()
            return
        T = self._check_T(T)
        if self._use_graph:
            if self._graph_explicit:
                raise ValueError("graph=True cannot be combined with trajectory_length: a captured draw bakes `steps` in")
            self._use_graph = False  # (a graph chosen by default; the eager launches keep its in-place select)
            self._drop_graphs()
        if self._T is None:
            self._steps_fixed = self._steps
        self._T = T

    @property
    def trajectory_length(self):
        """The integration time the draws are jittered around (None: a fixed ``steps``)."""
        return self._T

    @property
    def max_steps(self):
        return self._max_steps

    @property
    def last_steps(self):
        """Leapfrog steps of the most recent draw (None before the first)."""
        return self._last_steps

    def _next_steps(self):
        """Assign ``steps`` for the draw about to run: L_n of the next jittered draw, or what it is."""
        if self._T is not None:
            self._jitter_n += 1
            self._steps = jitter_steps(self._jitter_n, self._T, float(self._stepsize), self._max_steps)
        self._last_steps = int(self._steps)

    def _enter_whole_draw(self):
        """The mirror of _leave_whole_draw, between two draws: the stream goes back to the logical position (a momentum
        generated ahead in the state layout is dropped), the chain-major normals and the stream snapshots come back, graphs
        are dropped.  The whole-draw kernel needs the current log density only, which the step-by-step path kept."""
        self._drop_ahead(rewind=True)
        D, C, dev = self._dim, self._C, self._ops.device
        self._fused_draw = self._fused = True
        self._fused_zt = self._rng_kind == _lib.RNG_PHILOX and D >= 32
        n_slots = 2 if self._prefetch else 1
        if getattr(self, "_part", None) is None:
            self._part = torch.empty(12 * C, dtype=torch.float64, device=dev)
        if self._fused_zt:
            zt = list(getattr(self, "_zt_bufs", []))
            while len(zt) < n_slots:
                zt.append(torch.empty((C, (D + 7) // 8 * 8), dtype=torch.float64, device=dev))
            self._zt_bufs = zt
            self._rho_bufs = [None] * n_slots  # (the momentum never exists in the state layout)
            if self._prefetch:
                self._snap = [torch.empty_like(self._rng_state) for _ in range(2)]
        self._pf_kin_stale = False
        self._drop_graphs()

    def _tune_placement(self):
        """Roles (theta', grad', rho of each slot, grad): see ManyChainSampler._tune_roles."""
        ops, m, eps = self._ops, self._metric_dev, float(self._stepsize)
        # (a sampler on the tile-major schedule owns no full-width momentum: the cached gradient, the third full-width
        # array of its first steps and selects, then stands in as the step's third array)
        owned = [r for r in self._rho_bufs if r is not None]
        n_rho = len(owned)

        builtin = hasattr(self._model, "bk_eval")  # the library's own gradient op: safe to time as well

        def cost(a):
            tp, gp, rhos = a[0], a[1], a[2:2 + n_rho] or [a[2]]
            ms = sum(self._time_ms(lambda r=r: ops.kick_drift(tp, tp, r, r, gp, m, eps, False, 0.0, True, eps))
                     for r in rhos) / len(rhos)
            if builtin:
                ms += self._time_ms(lambda: self._model.bk_eval(tp, gp, None))
            return ms

        chosen, rep = self._tune_roles([self._thp_raw, self._gp_raw] + owned + [self._grad], cost)
        self._theta_p, self._grad_p = chosen[0], chosen[1]
        placed = iter(chosen[2:2 + n_rho])
        self._rho_bufs = [None if r is None else next(placed) for r in self._rho_bufs]
        self._grad = chosen[2 + n_rho]
        key = "step_ms" if builtin else "kick_drift_ms"
        self.placement = {key + "_as_allocated": rep["ms_as_allocated"], key + "_chosen": rep["ms_chosen"],
                          "assignments_tried": rep["assignments_tried"]}

    # -- tile-major scratch ------------------------------------------------------------------------
    # The tiled model-opaque loop keeps theta' and the trajectory gradient TILE-MAJOR: the block of tile k (chains
    # [c0, c1), c0 = k*T) is a contiguous [D, c1 - c0] array at element offset D*c0 of the same D*C doubles -- the 63
    # in-place steps of a tile then walk rows 8*T bytes apart instead of 8*C (profiles/cache_tiles.md, section 6).  Only the
    # sampler reads those two arrays; whoever else asks (`_theta_p`, `_grad_p`: tests, bench.py --full) gets a [D, C] tensor,
    # assembled from the blocks when the last draw left them tile-major.
    _tm_last = False  # the last draw wrote _thp_raw / _gp_raw tile-major

    @staticmethod
    def tile_major_blocks(C, D, T):
        """[(c0, c1, offset)]: tile k holds chains [c0, c1) as a contiguous [D, c1 - c0] block `offset` elements into the
        D*C-element store; every tile but the last has T chains, so offset = D*c0 also when C is ragged."""
        return [(c0, min(C, c0 + T), D * c0) for c0 in range(0, C, T)]

    def _tm_assemble(self, raw):
        D, C = self._dim, self._C
        flat, out = raw.view(-1), torch.empty((D, C), dtype=raw.dtype, device=raw.device)
        for c0, c1, off in self.tile_major_blocks(C, D, self._chain_tile):
            out[:, c0:c1].copy_(flat[off:off + D * (c1 - c0)].view(D, c1 - c0))
        return out

    @property
    def _theta_p(self):
        """The proposal of every chain as a [D, C] tensor (the last draw's; a copy while the store is tile-major)."""
        return self._tm_assemble(self._thp_raw) if self._tm_last else self._thp_raw

    @_theta_p.setter
    def _theta_p(self, a):
        self._thp_raw = a

    @property
    def _grad_p(self):
        """The gradient at the proposal, as `_theta_p`."""
        return self._tm_assemble(self._gp_raw) if self._tm_last else self._gp_raw

    @_grad_p.setter
    def _grad_p(self, a):
        self._gp_raw = a

    def _tm_flat(self, name):
        """The D*C doubles behind `name` as a flat tensor (a store with padded rows is replaced by a dense one)."""
        a = getattr(self, name)
        if not a.is_contiguous() or a.numel() != self._dim * self._C:
            a = torch.empty((self._dim, self._C), dtype=a.dtype, device=a.device)
            setattr(self, name, a)
        return a.view(-1)

    def _draw_tile_major(self, th, rho, kin0, logu, g, m, eps, half, L):
        """The momentum refresh, the L steps, the finish, the accept test, the blend into the new state and the select into
        the cached gradient, tile by tile: a tile's momentum is generated into the tile's own workspace, and everything its
        end needs (rho, theta', the proposal's gradient) is still in the cache when it runs.  Values, chains and stream
        positions are those of the untiled schedule, bit for bit.

        rho None (the default): every tile's randomness is generated IN LINE at the tile's start -- the tile it pushes out of
        the cache is dead by then, while a generator one tile ahead on the side stream slows the resident steps beside it by
        as much as it hides (profiles/cache_tiles.md, section 9) -- so nothing is ahead between two draws.  rho given (an
        explicit prefetch_rng=True): the draw's full-width momentum, generated ahead with kin0 and logu; the first step of a
        tile reads its columns."""
        ops, D, C, T = self._ops, self._dim, self._C, self._chain_tile
        thp_f, gp_f = self._tm_flat("_thp_raw"), self._tm_flat("_gp_raw")
        self._tile_workspace()
        lp0 = self._lp.clone() if self._stat is not None else None  # (warmup: the statistic sees the log density as it was)
        # the accepted chains take their proposal: a blend into a fresh state array, or (a replayed hipGraph needs fixed
        # addresses) a select in place -- _take()'s two forms
        self._out = torch.empty_like(th) if self._rebind else None
        for c0, c1, off in self.tile_major_blocks(C, D, T):
            n, sl = c1 - c0, slice(c0, c1)
            thp_k, gp_k = thp_f[off:off + D * n].view(D, n), gp_f[off:off + D * n].view(D, n)
            rho_k = self._rho_tile[:D * n].view(D, n)
            if rho is None:
                self._tile_randomness(rho_k, kin0[sl], logu[sl], m, sl)
            gl = None
            for s in range(L):
                if s == 0:  # full-width state and gradient columns in, the tile's own arrays out; the momentum in place
                    ops.kick_drift_ld(th[:, sl], thp_k, rho_k if rho is None else rho[:, sl], rho_k, g[:, sl], m, eps, True,
                                      -half, True, eps)
                else:
                    ops.kick_drift(thp_k, thp_k, rho_k, rho_k, gl, m, eps, False, 0.0, True, eps)
                gl = self._eval_grad(thp_k, gp_k, self._lp_p[sl] if s == L - 1 else None)
            gl = self._materialize(gl, gp_k)
            # forward half-step + kinetic energy of the proposal [hmc.py:52, :37], accept [hmc.py:60-63], take [hmc.py:61]
            if self._pd is not None:
                ops.leapfrog_finish_precond(rho_k, None, gl, self._pd, half, False, self._kin1[sl])
            else:
                ops.leapfrog_finish(rho_k, None, gl, m, half, False, self._kin1[sl])
            if self._energy is not None:  # (this tile's log density and state columns are still the start's: no clone)
                self._energy.update(self._lp[sl], kin0[sl], self._lp_p[sl], self._kin1[sl], logu[sl], th[:, sl],
                                    chain0=self._chain_id0 + c0)
            ops.mh_accept(_lib.ACCEPT_HMC, self._lp[sl], kin0[sl], self._lp_p[sl], self._kin1[sl], logu[sl],
                          self._mask[sl], self._ret[sl], self._accepted)
            if self._rebind:
                ops.blend_columns_ld(self._mask[sl], th[:, sl], thp_k, self._out[:, sl])
            else:
                ops.select_columns_ld(self._mask[sl], th[:, sl], thp_k)
            ops.select_columns_ld(self._mask[sl], self._grad[:, sl], gp_k)
        if lp0 is not None:
            ops.accept_stat(lp0, kin0, self._lp_p, self._kin1, self._stat, self._stat_work)
        if self._rebind:
            self._theta_dc = self._out
        self._tm_last = True

    # -- optional cache blocking ----------------------------------------------------------------
    # chain_tile=T runs the L steps tile by tile over blocks of T chains (chains are
    # independent, so this is only a schedule).  The idea: keep a tile's three arrays inside
    # the 256 MiB Infinity Cache: theta, rho and the gradient of T chains, the arrays the in-place
    # steady-state step touches (the library's own rule for "fits", bk_streams_past_llc of
    # csrc/bk_common.hpp, is LLC_BYTES).  Inside the cache kick+drift and the gradient op take their
    # plain variants and a tile-step costs less than an eighth of the full-size step
    # (profiles/cache_tiles.md).  The default tiles where that applies and pays:
    #   * only the step-by-step loop with a separate gradient op (a whole-draw, whole-trajectory or
    #     one-launch-per-step kernel keeps its state on chip or streams it once per step anyway),
    #   * only when the three arrays are at least TWICE the threshold (two full tiles): just past it most of an untiled
    #     step still hits the cache and the ragged second tile loses -- 12,288 x 1,024 tiled as 8,192 + 4,096 takes 7.15 ms
    #     per draw against 6.90 untiled, while 16,384 gains 6 % and 65,538 (eight tiles and one of two chains) 4-5 %,
    #   * the largest even tile whose three arrays fit (8,192 chains at D = 1,024),
    #   * and not below MIN_TILE chains: at D = 1,024 tiles of 4,096 and 2,048 chains are SLOWER than no tiling
    #     (40.7 and 40.0 ms per draw against 38.8; 8,192: 37.8 -- the sweep in the same file): their launches are too
    #     short to run at the cache's rate.  A larger D would give the fitting tile fewer chains; nobody has measured that.
    # All of this was measured with the built-in diagonal Gaussian at D = 1,024 and 8,192 to 65,538 chains only: a smaller D
    # (longer rows, the same bytes per tile) and heavier gradient ops follow the same rule unmeasured.
    # An explicit chain_tile wins; chain_tile <= 0 means no tiling.
    # The tiled loop keeps its scratch tile-major and finishes each tile while it is resident (_draw_tile_major): that took the
    # 65,536-chain draw from 37.8 to 36.0 ms and 16,384 / 32,768 chains from 9.23 / 18.61 to 9.00 / 18.09; MIN_TILE and the
    # C >= 2 T rule were not measured again (the new schedule only makes a tile cheaper; the ragged cases above were not rerun).
    # The loop also refreshes each tile's momentum itself, in line at the tile's start, into the tile's [D, T] workspace through a
    # scratch chunk for T chains (64 MiB each at 8,192 x 1,024, dead before the tile's second step): 33.85 -> 33.25 ms per draw at
    # 65,536 chains, 8.48 -> 8.31 and 17.11 -> 16.64 at 16,384 / 32,768, and no full-width momentum or full-size scratch
    # (profiles/cache_tiles.md, section 9).  The footprint rule above still counts the three arrays of the steady-state step.
    LLC_BYTES = 192 << 20
    MIN_TILE = 8192

    @classmethod
    def default_chain_tile(cls, C, D):
        """Chains per tile for C chains of D dimensions on the step-by-step loop; C itself: no tiling."""
        t = cls.LLC_BYTES // (3 * 8 * D)
        t -= t % 2
        return t if t >= cls.MIN_TILE and C >= 2 * t else C

    def _pick_tile(self, chain_tile):
        C = self._C
        if chain_tile is None:
            # (bk_eval: a gradient op that writes the tile's gradient array itself; what a PyTorch model allocates on
            # the way is not among the three arrays, and a dense metric's products are whole-array GEMMs)
            opaque_loop = (self._batched and self._M is None and hasattr(self._model, "bk_eval")
                           and not self._fused_draw and not self._lanes_traj and not self._step_hook)
            return self.default_chain_tile(C, self._dim) if opaque_loop else C
        t = int(chain_tile)
        return C if t <= 0 or t >= C else max(2, t - t % 2)

    # -- statistics ---------------------------------------------------------------------------
    def accept_rate(self) -> float:
        """Fraction of accepted proposals so far (device counter, ballot/popcount sums)."""
        n = self._draws * self._C
        return float(self._accepted.item()) / n if n else float("nan")

    @property
    def last_accept(self):
        return self._mask.bool() if self._batched else bool(self._mask[0].item())

    # -- energy diagnostics ------------------------------------------------------------------------
    _energy = None  # track_energy(): the diagnostics.EnergyDiagnostics fed before every accept test

    def track_energy(self, threshold: float = 1000.0, capture: int = 1024) -> EnergyDiagnostics:
        """Track divergent transitions (energy error NaN or below -threshold) and the energy statistics of E-BFMI from the
        next draw on, and keep the states up to ``capture`` divergent trajectories started from; -> the tracker
        (diagnostics.EnergyDiagnostics, also ``self.energy``), which owns all of its state in device memory and
        checkpoints itself (``state_dict()`` of the sampler does not carry it).

        Tracking changes no bit of theta, logp, the accept counter or the streams on any path.  The tracker's two entry
        points run right before the accept test, on the five vectors that test reads and on the start state: three small
        launches per draw (per tile on the tile-major schedule), no host read, nothing allocated -- a captured draw
        (graph=True) replays them; graphs are captured again after this call.  Cost: the whole-draw kernel leaves its
        accept test to a launch of its own while a tracker is attached (as during warmup()): one more launch.
        warmup() works with a tracker attached and reports what it reports without one."""
        self._energy = EnergyDiagnostics(self._C, self._dim, threshold, capture, self._chain_id0, self._ops)
        self._drop_graphs()
        return self._energy

    def untrack_energy(self) -> None:
        """Detach the tracker (it keeps its state): the draws go back to the launches of an untracked sampler."""
        self._energy = None
        self._drop_graphs()

    @property
    def energy(self):
        """The attached EnergyDiagnostics (None: not tracking)."""
        return self._energy

    def _set_metric(self, m):
        if self._pd is not None:
            raise ValueError("metric_diag cannot be combined with precond_diag")
        super()._set_metric(m)
        self._pf_kin_stale = True  # a prefetched kinetic energy was computed with the old metric

    def _state_tensors(self):
        return {"theta": self._theta_dc, "grad": self._grad, "lp": self._lp, "accepted": self._accepted}

    def _logical_rng(self):
        if self._prefetch and self._ahead.ahead:
            self._ahead.synchronize()
        return self._stream_position()

    def load_state_dict(self, sd):
        if self._prefetch and self._ahead.ahead:
            torch.cuda.synchronize()  # (the generator queued ahead has finished before its bookkeeping goes)
        self._drop_ahead(rewind=False)
        if self._rebind:
            # the state array is the last draw handed out (see _draw): restore into a fresh one
            self._theta_dc = torch.empty_like(self._theta_dc)
        super().load_state_dict(sd)

    def _state_extra(self):
        return {"stepsize": float(self._stepsize), "precond_diag": self._precond_extra(),
                "trajectory_length": self._T, "max_steps": self._max_steps, "jitter_n": self._jitter_n,
                "metric_dense": None if self._M is None else self._M.cpu().clone()}

    def _load_extra(self, extra):
        # (checkpoints written before the step size and the preconditioner were carried hold neither: nothing changes)
        if "stepsize" in extra:
            self._stepsize = extra["stepsize"]
        if "trajectory_length" in extra:  # (older checkpoints: the sampler keeps what it was built with)
            self._max_steps = self._check_max_steps(extra["max_steps"])
            self.set_trajectory_length(extra["trajectory_length"])
            self._jitter_n = int(extra["jitter_n"])
        pv = self._precond_from_extra(extra)
        if pv is not None:
            self.set_precond_diag(pv)  # (randomness generated ahead was dropped by load_state_dict: the stream stays put)
        Md = extra.get("metric_dense")  # (older checkpoints carry none: the sampler keeps what it was built with)
        if Md is not None:
            if self._M is None:
                raise ValueError("checkpoint holds metric_dense, this sampler was built without one (build it with "
                                 "metric_dense=np.eye(D))")
            self._install_metric_dense(Md)

    def _after_load(self):
        # drop any randomness generated ahead: it is regenerated from the restored stream
        if self._prefetch:
            self._ahead.reset()
        self._pf_kin_stale = False

    def _rho_full(self, slot):
        """The full-width momentum of a slot and the full-size generator scratch, which a sampler on the tile-major
        schedule allocates only here: when a draw leaves that schedule (the untiled loop, a ChEES warm-up, L = 0)."""
        if self._rho_bufs[slot] is None:
            self._rho_bufs[slot] = torch.empty((self._dim, self._C), dtype=torch.float64, device=self._ops.device)
        if self._work_dropped:
            self._rng_work, self._work_dropped = self._ops.refresh_work(self._C, self._dim), False

    def _tile_workspace(self):
        """The tile-major schedule's workspace: a tile's [D, T] momentum and the generator's scratch for T chains (None
        where the generator takes none: _setup's rule)."""
        D, T, ops = self._dim, self._chain_tile, self._ops
        if self._rho_tile is None or self._rho_tile.numel() != D * T:
            self._rho_tile = torch.empty(D * T, dtype=torch.float64, device=ops.device)
            self._tile_work = ops.refresh_work(T, D) if self._rng_kind == _lib.RNG_PHILOX and D >= 32 else None

    def _tile_randomness(self, rho_k, kin0, logu, m, sl):
        """Momentum (into the tile's workspace), kinetic energy and accept uniform of the chains `sl` [hmc.py:56, :37, :60].
        Each chain's normals, then its uniform: its stream order is that of _randomness, whatever the order of the tiles."""
        ops, state = self._ops, self._rng_state[:, sl]
        if self._pd is not None:
            ops.momentum_refresh_precond(self._rng_kind, state, rho_k, self._pd, kin0, self._tile_work)
        else:
            ops.momentum_refresh(self._rng_kind, state, None, 0.0, 1.0, rho_k, m, kin0, None, self._tile_work)
        ops.log_uniform(self._rng_kind, state, logu)

    def _randomness(self, slot):
        """Momentum, kinetic energy and accept uniform of one draw [hmc.py:56, :37, :60]."""
        ops = self._ops
        if self._fused_zt:
            # D normals, chain-major; their kinetic energy is summed by the draw kernel itself
            # (with prefetch the generator also leaves the table as it found it -- the logical stream
            # position while this slot is the one generated ahead -- in snap[slot])
            ops.normals_chain_major(self._rng_kind, self._rng_state, self._zt_bufs[slot], self._dim,
                                    None if self._snap is None else self._snap[slot])
        elif self._pd is not None:
            ops.momentum_refresh_precond(self._rng_kind, self._rng_state, self._rho_bufs[slot], self._pd,
                                         self._kin0_bufs[slot], self._rng_work)
        elif self._M is None:
            ops.momentum_refresh(self._rng_kind, self._rng_state, None, 0.0, 1.0, self._rho_bufs[slot],
                                 self._metric_dev, None if self._fused_draw else self._kin0_bufs[slot], None,
                                 self._rng_work)
        else:
            ops.momentum_refresh(self._rng_kind, self._rng_state, None, 0.0, 1.0, self._mv_rng, None, None,
                                 None, self._rng_work)
            ops.dense_metric_apply(self._M_chol, self._mv_rng, self._rho_bufs[slot])  # rho = chol(M) @ z
            self._dense_kinetic(self._rho_bufs[slot], self._kin0_bufs[slot], self._mv_rng)
        ops.log_uniform(self._rng_kind, self._rng_state, self._logu_bufs[slot])

    def _dense_kinetic(self, rho, kin_out, scratch):
        """kin = 1/2 rho . (M^-1 @ rho)"""
        self._ops.dense_metric_apply(self._M_inv, rho, scratch)
        self._ops.dot_columns(rho, scratch, 0.5, kin_out)

    def _mg(self, g):
        """Gradient as the kick sees it: M @ grad with a dense metric, grad itself otherwise."""
        if self._M is None:
            return g
        self._ops.dense_metric_apply(self._M, self._materialize_dense(g), self._mv)
        return self._mv

    def _materialize_dense(self, g):
        if g.dim() == 2 and g.stride(1) == 1:
            return g
        self._ops.relayout(g, self._gp_raw)
        return self._gp_raw

    # The side-stream generator (prefetch_rng) runs ONE draw ahead: at the start of draw n the generator
    # of draw n+1 is queued (_engine.LookAhead).  _stream_position() is where the reference's generator would be between
    # two sample() calls.
    # For the one-pass draw (bk_hmc_draw), which is fp64-VALU bound like the generator, two other
    # schedules were measured at 65,536 x 1024 on one box (tools/fused_hmc_profile_run.py): queueing the
    # generator of draw n+2 right after draw n's accept test, so that it starts under the HBM-bound
    # blend -- 1.37 ms per draw, the generator then takes the ALUs from the next draw's trajectories
    # (1.0-1.1 ms instead of 0.78) -- and no side stream at all, 1.38 ms; one ahead gives 1.29 ms: the
    # trajectories keep the ALUs, the generator takes what they leave and finishes under the blend.
    def _current_randomness(self):
        """Buffers holding this draw's randomness; with prefetch_rng it was generated ahead, and the next draw's generator is
        queued on the side stream, where it hides under this draw's launches."""
        cur = 0
        if not self._fused_zt:
            for slot in range(len(self._rho_bufs)):  # (on the current stream, not where the generator runs)
                self._rho_full(slot)
        if not self._prefetch:
            self._randomness(0)
        else:
            ahead = self._ahead.ahead
            cur = self._ahead.take(self._randomness)
            if self._pf_kin_stale and ahead and not self._fused_draw:
                # (the kinetic energy generated ahead was computed with a metric that has been replaced since)
                self._ops.leapfrog_finish(self._rho_bufs[cur], None, None, self._metric_dev, 0.0, False, self._kin0_bufs[cur])
            self._pf_kin_stale = False
            self._ahead.start_next(self._randomness, None if self._snap is not None else (self._rng_logical, self._rng_state))
        self._zt_slot = cur
        return self._rho_bufs[cur], self._kin0_bufs[cur], self._logu_bufs[cur]

    @property
    def _tile_rng(self):
        """Whether this sampler's draws can take the tile-major loop (what does not change from draw to draw)."""
        return (self._chain_tile < self._C and self._batched and self._M is None and not self._step_hook
                and not self._fused_draw and not self._lanes_traj and hasattr(self._ops, "kick_drift_ld"))

    def _tile_major_draw(self):
        """Whether the draw about to run takes the tile-major loop: _draw's own conditions, in its order."""
        return self._tile_rng and self._chees is None and int(self._steps) >= 1

    def _tile_major_randomness(self):
        """The tile-major loop's randomness: the kinetic energies and the accept uniforms of all chains in slot 0's vectors,
        filled tile by tile, and no full-width momentum.  Randomness that a draw on another schedule generated ahead (a
        ChEES warm-up, L = 0) is dropped and its stream taken back: the tiles generate the same values again."""
        self._drop_ahead(rewind=True)
        self._pf_kin_stale = False
        self._zt_slot = 0
        return None, self._kin0_bufs[0], self._logu_bufs[0]

    def _graph_key(self):
        return (float(self._stepsize), int(self._steps))

    # -- warmup -------------------------------------------------------------------------------------
    def _dense_estimator(self, group):
        """warmup(adapt_metric="dense")'s estimate of metric_dense: as _diag_estimator, with diagnostics.RunningCovariance."""
        cov = RunningCovariance(self._dim, self._ops)

        def install(chains_total):
            Mn = shrink_estimate(cov.covariance(group), float(cov.n // self._C) * chains_total)
            self._drop_ahead(rewind=True)  # (the momentum generated ahead carries the old metric: generate it again)
            self.set_metric_dense(Mn)
            cov.reset()

        return (lambda: cov.update(self._theta_dc, layout="dc", group=group)), install

    def warmup(self, draws, target_accept=0.8, adapt_metric=True, group=None, *, adapt_trajectory=False, max_steps=None):
        """Run `draws` draws that tune the step size and (adapt_metric) the diagonal preconditioner from ALL chains of all
        ranks, then keep the tuned values: afterwards the sampler samples with them.  -> report dict: ``stepsize``,
        ``precond_diag`` (host copy, None if none is set), per-draw ``eps`` and ``alpha`` histories, ``window_ends``,
        ``nan_chains`` (total count of chains whose energy difference was NaN).

        Step size: dual averaging on log(eps) towards a mean acceptance statistic of `target_accept`
        (adapt.DualAveraging), fed once per draw with mean_c min(1, exp(min(0, h1 - h0))) over every chain
        (bk_accept_stat; a NaN difference counts 0).  Metric: Welford moments of the state after every draw inside a window
        of adapt.warmup_windows; at a window's end v = N/(N+5) * pooled variance + 1e-3 * 5/(N+5), N = draws in the window
        x chains, becomes the preconditioner (set_precond_diag), the moments are reset and the step size restarts from
        its averaged iterate.

        Dense metric (adapt_metric="dense"; accepted only on a sampler built with ``metric_dense=``, np.eye(D) being the
        natural start): the same windows and the same step-size schedule, with the D x D covariance of the state of ALL
        chains pooled in place of the variances -- diagnostics.RunningCovariance, one bk_cov_accumulate per draw inside a
        window (an fp64 MFMA pass of D^2 C flop: half of one of the 2L + 2 matrix applications a dense draw pays) around
        the first draw's cross-chain mean, common to all ranks.  At a window's end
        M = N/(N+5) * cov + 1e-3 * 5/(N+5) * I is installed with set_metric_dense (Cholesky factor and inverse on the host,
        as at construction: three times per warmup) and the accumulator is reset.  A momentum generated ahead with the old
        metric (prefetch_rng) is generated again from the stream position it started at, so the stream ends where a
        sampler without prefetch_rng leaves it.  The report gains ``metric_dense`` (host copy); ``precond_diag`` stays None.
        Meant for D up to a few hundred, or for modest chain counts: at 1,024 x 65,536 chains an update is of the order of
        a second, and so is every leapfrog step of a dense draw.  Non-finite chain states poison the estimate exactly as
        they do the diagonal one; they are not filtered.  Cannot be combined with adapt_trajectory.

        Trajectory length (adapt_trajectory=True; `steps` is not adapted otherwise): ChEES-HMC (Hoffman, Radul, Sountsov
        2021).  Every warmup draw is jittered around the integration time T (see ``trajectory_length``; it starts from the
        sampler's, or steps * stepsize), and adapt.TrajectoryAdam ascends log T along the gradient of
        1/4 E[(|theta' - E theta'|^2 - |theta - E theta|^2)^2] taken across all chains of all ranks
        (bk_chees_sums, bk_chees_stat: one more pair of passes over the state, the proposal and its velocity per draw; its
        two outputs travel in the same vector and the same host read as the acceptance statistic).  At a metric window's
        end the controller restarts from its current T.  Afterwards ``trajectory_length`` stays set to the averaged iterate,
        so sample() keeps jittering (and replays no captured graph).  The statistic needs the proposal's velocity in memory:
        for the duration of the warmup the whole-draw kernel is left for the step-by-step path (and entered again
        afterwards), the lane-spread one-launch trajectory and the tile-major schedule are not taken -- all of them give the
        same draws bit for bit, so the report does not depend on the path.  Needs a batched model and refuses metric_dense
        (the dense velocity is not what the kick and drift kernels hold); ``max_steps`` replaces the sampler's bound.  The
        report gains ``trajectory_length``, per-draw ``T`` and ``steps`` and ``nonfinite_chains`` (chains with weight whose
        gradient term was not finite, left out of the sum).

        Cost: the statistic kernel, ONE host read of three doubles (summed over ranks in rank order, dist.gather_sum) and,
        inside windows, a Welford update per draw; two more [D, C] arrays for the window moments, freed at the end.  The
        draws are launched eagerly (the step size changes every draw); captured graphs are dropped once at the end.  On
        launch-bound shapes (a draw of tens of microseconds) the host read dominates a warmup draw: at 128 x 4,096 chains a
        warmup draw takes 0.10 ms against 0.056 for a replayed plain draw, at 1,024 x 65,536 1.6-1.7 ms against 1.2
        (profiles/warmup_adapt.md).  A model without the preconditioned whole-draw hook (an elementwise from_source or traced
        density) leaves the whole-draw kernel for one launch per leapfrog step when its first window ends.
        All ranks reach identical eps and v, and a given (seed, chains, world size) reproduces them bit for bit on every path.
        Across world sizes the sums are grouped differently and agree to rounding only -- and dual averaging is not a
        contraction (after a restart it swings the step size across the stability limit and back), so that rounding grows: two
        world sizes end at different, equally valid adaptations (observed: eps 0.647 against 0.675, v within 3 % of each
        other and of the truth)."""
        dense = isinstance(adapt_metric, str)
        if dense:
            if adapt_metric != "dense":
                raise ValueError(f"warmup: adapt_metric must be True, False or 'dense', got {adapt_metric!r}")
            if self._M is None:
                raise ValueError("warmup: adapt_metric='dense' estimates metric_dense and is accepted only on a sampler "
                                 "built with metric_dense= (np.eye(D) is the natural start)")
        elif adapt_metric and (self._M is not None or (self._pd is None and self._metric_dev is not None)):
            raise ValueError("warmup: adapt_metric=True estimates precond_diag, which cannot be combined with "
                             "metric_diag / metric_dense (pass adapt_metric=False to tune the step size alone)")
        if adapt_trajectory:
            if not self._batched:
                raise ValueError("warmup: adapt_trajectory=True needs a batched device model (the gradient is taken across "
                                 "chains)")
            if self._M is not None:
                raise ValueError("warmup: adapt_trajectory=True cannot be combined with metric_dense (the dense velocity is "
                                 "not what the kick and drift kernels hold)")
            if self._graph_explicit:
                raise ValueError("warmup: adapt_trajectory=True jitters every draw, which graph=True cannot replay")
            if max_steps is not None:
                max_steps = self._check_max_steps(max_steps)
        elif max_steps is not None:
            raise ValueError("warmup: max_steps bounds the adapted trajectory, pass it with adapt_trajectory=True")
        draws = self._check_warmup(draws, target_accept)
        observer, was_fused = None, False
        if adapt_trajectory:
            ops, dev, C, D = self._ops, self._ops.device, self._C, self._dim
            if max_steps is not None:
                self._max_steps = max_steps
            self.set_trajectory_length(self._T if self._T is not None else float(self._steps) * float(self._stepsize))
            observer = TrajectoryObserver(self)
            was_fused = self._fused_draw
            if was_fused:
                self._leave_whole_draw()
            sums = torch.zeros(2 * D + 1, dtype=torch.float64, device=dev)  # {sum theta, sum theta', chains}
            sums[2 * D] = float(C)
            self._chees = (sums, torch.empty(ops.chees_work_elems(C), dtype=torch.float64, device=dev), group)

        def draw():
            self._next_steps()
            self._draw()
            self._join_ahead()

        metric = (self._dense_estimator if dense else self._diag_estimator) if adapt_metric else None
        try:
            rep = self._warmup_loop(draws, target_accept, group, draw, metric, observer)
        finally:
            self._chees, self._rho_cur = None, None
            self._drop_graphs()
            if was_fused and (self._pd is None or hasattr(self._model, "bk_hmc_draw_precond")):
                self._enter_whole_draw()
        if dense:
            rep["metric_dense"] = self._M.cpu().numpy().copy()
        return rep

    # -- one draw for every chain ------------------------------------------------------------------
    def sample(self):
        self._next_steps()
        self._run_draw(self._draw)
        self._join_ahead()
        self._draws += 1
        return self._draw_out(self._theta_dc, self._ret)

    def _draw(self):
        ops = self._ops
        eps, L, m = float(self._stepsize), int(self._steps), self._metric_dev
        half = 0.5 * eps
        th, thp, gp_raw = self._theta_dc, self._thp_raw, self._gp_raw
        mirror = not self._batched
        self._tm_last = False  # (every path but the tile-major one leaves theta' and its gradient as [D, C] arrays)

        # momentum + kinetic energy + accept uniform [hmc.py:56, :37, :60]; the uniform is drawn
        # right after the D normals -- the same stream order as the reference, whose uniform is
        # the next value of the stream whatever happens in between
        # (the tile-major loop generates them tile by tile, into each tile's workspace)
        tiled = self._tile_major_draw()
        in_line = tiled and not self._tile_ahead
        rho, kin0, logu = self._tile_major_randomness() if in_line else self._current_randomness()
        # warmup(adapt_trajectory=True): the trajectory statistic reads the proposal's velocity, so the finish launch stores
        # it (in place) and the paths that keep it on chip or in a tile's scratch are not taken
        chees = self._chees is not None
        self._rho_cur = rho if chees else None

        if self._fused_draw:
            if not self._have_cache:
                self._eval_logp(th, self._lp)
                self._have_cache = True
            zt = self._zt_bufs[self._zt_slot] if self._fused_zt else None
            # (fp64-VALU bound: a metric of ones is not multiplied in -- x * 1.0 is x, bit for bit)
            m_draw = None if (m is None or self._metric_identity) else m
            accept = (self._lp, logu, self._mask, self._ret, self._accepted)
            in_launch = accept if (self._stat is None and self._energy is None) else None
            if self._pd is not None:
                self._model.bk_hmc_draw_precond(th, thp, rho, zt, self._pd, eps, L, self._part, kin0, self._kin1, self._lp_p,
                                                accept=in_launch)
            else:
                self._model.bk_hmc_draw(th, thp, rho, zt, m_draw, eps, L, self._part, kin0, self._kin1, self._lp_p,
                                        accept=in_launch)  # [hmc.py:56-63]
            if in_launch is None:  # warmup / track_energy: their passes first, then the same accept arithmetic as its own launch
                self._accept(kin0, logu)
            self._take(th, thp)
            return

        if self._lanes_traj and L >= 1 and self._pd is None and not chees:
            if not self._have_cache:
                self._materialize(self._eval_grad(th, self._grad, self._lp), self._grad)
                self._have_cache = True
            # [hmc.py:40-53, :59] in one launch; the proposal's gradient is kept for the chains that accept
            if self._model.bk_hmc_proposal(th, rho, self._grad, thp, gp_raw, self._lp_p, self._kin1, m, eps, L):
                self._accept(kin0, logu)                                                 # [hmc.py:60-63]
                self._take(th, thp, self._grad, gp_raw)
                return

        if mirror:
            self._eval_logp(th, self._lp)                  # joint_logp(theta, rho)      [hmc.py:57]
            g = self._eval_grad(th, self._grad, None)       # leapfrog's first gradient   [hmc.py:45]
        else:
            if not self._have_cache:
                self._materialize(self._eval_grad(th, self._grad, self._lp), self._grad)
                self._have_cache = True
            g = self._grad

        if self._M is not None:
            m = None  # the metric is applied by _mg()
        if L == 0:
            # rho_mid = rho - c*t ; rho1 = rho_mid + c*t ; theta unchanged [hmc.py:46,52]
            ops.kick_drift(th, thp, rho, rho, self._mg(g), m, 0.0, True, -half, False, 0.0)
            g_last = g
            if not mirror:
                self._lp_p.copy_(self._lp)
        elif (self._traj_hook and not mirror and self._chain_tile >= self._C
              and self._model.bk_leapfrog_trajectory(th, rho, g, None, thp, rho, gp_raw, self._lp_p, m, eps, L,
                                                     hmc_first=True)):
            self._grad_calls += L   # [hmc.py:45-50] in one launch: L gradients of the model's density
            g_last = gp_raw
        elif tiled:
            # the tiled model-opaque loop: tile-major scratch, each tile refreshed, stepped and finished while it is resident
            # (an ops layer without the per-pitch entry points keeps the loop below on column slices of [D, C] arrays, and
            # so does a lane-spread model whose one-launch trajectory declines: the same draws)
            self._draw_tile_major(th, rho, kin0, logu, g, m, eps, half, L)
            return
        else:
            g_last = None
            T = self._chain_tile
            for c0 in range(0, self._C, T):
                c1 = min(self._C, c0 + T)
                tile = (c0, c1) != (0, self._C)
                v = (lambda a: a[:, c0:c1]) if tile else (lambda a: a)
                th_t, thp_t, rho_t, gp_t, g_t = v(th), v(thp), v(rho), v(gp_raw), v(g)
                lp_t = self._lp_p[c0:c1] if tile else self._lp_p
                gl = None
                for n in range(L):
                    last = n == L - 1
                    if n == 0:
                        ops.kick_drift(th_t, thp_t, rho_t, rho_t, self._mg(g_t), m, eps, True, -half, True, eps)
                    elif self._step_hook and not mirror:
                        # {gradient at the point reached, kick, drift} of step n as ONE launch (the gradient op of step
                        # n - 1 and this step's kick+drift, fused: the model's density inside the library's step kernel)
                        self._grad_calls += 1
                        self._model.bk_leapfrog_step(thp_t, rho_t, m, eps)
                    else:
                        ops.kick_drift(thp_t, thp_t, rho_t, rho_t, self._mg(gl), m, eps, False, 0.0, True, eps)
                    if self._step_hook and not mirror and not last:
                        continue  # (the next step's launch evaluates the gradient itself)
                    want_lp = lp_t if (last and not mirror) else None
                    gl = self._eval_grad(thp_t, gp_t, want_lp)
                if tile:
                    self._materialize(gl, gp_t)
                    g_last = gp_raw
                else:
                    g_last = gl
        # forward half-step + kinetic energy of the proposal [hmc.py:52, :37]
        if self._pd is not None:
            ops.leapfrog_finish_precond(rho, rho if chees else None, g_last, self._pd, half, False, self._kin1)
        elif self._M is None:
            ops.leapfrog_finish(rho, rho if chees else None, g_last, m, half, False, self._kin1)
        else:
            ops.leapfrog_finish(rho, rho, self._mg(g_last), None, half, False, None)
            self._dense_kinetic(rho, self._kin1, self._mv)
        if mirror:
            self._eval_logp(thp, self._lp_p)                # joint_logp(theta_prop, rho_prop) [hmc.py:59]
        self._accept(kin0, logu)  # [hmc.py:60-63]
        if mirror:
            self._select(self._mask, th, thp)
        else:
            gp = self._materialize(g_last, gp_raw) if L > 0 else None
            self._take(th, thp, self._grad if gp is not None else None, gp)

    def _accept(self, kin0, logu):
        """The accept test [hmc.py:60-63]; during warmup() preceded by the acceptance statistic of the same energies
        (bk_accept_stat, before the test overwrites the current log density), and with track_energy() by the energy
        diagnostics of the same five vectors and the capture of the divergent chains' start state."""
        if self._stat is not None:
            self._ops.accept_stat(self._lp, kin0, self._lp_p, self._kin1, self._stat, self._stat_work)
        if self._energy is not None:
            self._energy.update(self._lp, kin0, self._lp_p, self._kin1, logu, self._theta_dc)
        if self._chees is not None:
            self._chees_launch(kin0)
        self._ops.mh_accept(_lib.ACCEPT_HMC, self._lp, kin0, self._lp_p, self._kin1, logu,
                            self._mask, self._ret, self._accepted)

    def _chees_launch(self, kin0):
        """The trajectory statistic of this draw into _stat[3:5] (state, log density and proposal are still intact): sums
        over this rank's chains, all ranks' sums in rank order, the means (divided by the chain count as a TENSOR: the same
        doubles on every device, see diagnostics._cross_chain_moments), then the weighted gradient."""
        ops, D = self._ops, self._dim
        sums, work, group = self._chees
        ops.chees_sums(self._theta_dc, self._thp_raw, sums)
        tot = _gather_sum(sums, group)
        mean = (tot[0:2 * D] / tot[2 * D:2 * D + 1]).contiguous()
        ops.chees_stat(self._theta_dc, self._thp_raw, self._rho_cur, mean, self._lp, kin0, self._lp_p, self._kin1,
                       self._stat[3:5], work)

    def _take(self, th, thp, g=None, gp=None):
        """The accepted chains take their proposal [hmc.py:61] (and its cached gradient)."""
        if not self._rebind:
            self._select(self._mask, th, thp, g, gp)
            return
        self._out = torch.empty_like(th)
        self._ops.blend_columns(self._mask, th, thp, self._out)
        self._theta_dc = self._out
        if gp is not None:
            self._ops.select_columns(self._mask, g, gp)
