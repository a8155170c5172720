"""Many-chain Metropolis-adjusted Langevin on the GPU: drop-in for ``bayes_kit/mala.py:14-79``.

Per draw and chain: theta' = (theta + eps*grad) + sqrt(2 eps) z   [mala.py:41-45];
one gradient call at theta' [:46-48]; forward / reverse proposal densities [:50-53,68-79];
Metropolis-Hastings accept with strict ``<`` [metropolis.py:70-76]; (logp, grad) of the
current point are cached [mala.py:31-32,62-64]; the MODEL log density is returned [:66].

Two ways through the device:

* **two-pass** (many chains, Philox streams, 32 <= D <= 1024): a draw is the model's gradient op
  plus ONE kernel (``bk_mala_step``) that keeps a block of 16 chains x all dimensions on chip
  between the per-chain sums and the select, and also writes the NEXT draw's proposal from
  normals generated ahead on a side stream -- 88*D bytes of HBM traffic per chain-draw.  The
  state array is rebound every draw, as the reference rebinds ``_theta`` (mala.py:62): the
  tensor ``sample()`` returns IS the new state and is never written again.
  For a model that is a SEPARABLE density the library can inline (``bk_mala_step``: the built-in Gaussians, an elementwise
  ``CTarget.from_source`` / traced ``TorchModel``) the step kernel recomputes both gradients from theta and theta' and stores
  none: the model's launch is its log density alone and a draw moves 56*D bytes; the same draws bit for bit
  (``path="opaque"`` keeps the model-opaque pair of launches).
* **step by step** (everything else: a single-chain host model, PCG64 streams, odd shapes):
  proposal, gradient, proposal densities, accept and select as separate kernels.

Both consume each chain's stream in the reference's order (D normals, then one uniform) and give
the same draws bit for bit.

``precond_diag=v`` (extension) is plain MALA on theta / sqrt(v): theta' = (theta + eps*(v*grad)) + sqrt(2 eps)*(sqrt(v)*z),
proposal densities with x = .. - eps*(v*grad) and the sum of (x*x)*(1/v).  ``warmup`` estimates v and tunes eps from all chains.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._engine import LookAhead, ManyChainSampler


class MALA(ManyChainSampler):
    # 65,536 chains: 512-KiB rows.  The one-pass step kernel keeps 16 chains x all dims on a CU (1,024 row pieces of 128
    # bytes, all at the same offset of a 4-KiB-aligned pitch) and the gradient + log density op walks down the rows too:
    # 1.39 -> 1.27 ms per draw with the rows 1,152 bytes further apart (1.57 -> 1.38 on a box whose allocations sit
    # worse; pads 48..400 columns within 2 % of each other, 0 / 8 / 32 / 528 are the bad ones).
    STATE_PAD_COLUMNS = 144
    SINGLE_LAUNCH_MAX_DIMS = 4096  # (one lane walks the coordinates: the single-chain mode is for small models)

    TUNING = ("graph", "prefetch_rng", "tune_placement", "two_pass", "single_launch")
    _STEP_SIZE = "_epsilon"

    def __init__(self, model, epsilon: float, init=None, seed=None, *, chains: Optional[int] = None,
                 chain_id0: int = 0, path: str = "auto", precond_diag=None, tuning: Optional[dict] = None, ops=None,
                 **knobs):
        """The reference's arguments (mala.py:15-21), then the engine's (ManyChainSampler: chains, chain_id0, path, tuning,
        ops; path "step" and "opaque" both keep the model-opaque pair {gradient op, step kernel}).  Tuning knobs (none
        changes a result): ``graph``, ``prefetch_rng``, ``tune_placement``, ``two_pass`` (gradient op + ONE step kernel
        per draw; default where the shape allows), ``single_launch`` (one chain: one launch per draw).

        ``precond_diag`` (extension; needs a batched device model): a length-D vector v of variances, ideally the posterior
        variances -- the sampler is then plain MALA on theta / sqrt(v), at the cost of three more multiplies per element.
        Every path supports it and gives the same draws bit for bit: two-pass shapes use the preconditioned step kernel
        (bk_mala_step_precond), the built-in Gaussians their inlined one; an elementwise from_source / traced density, whose
        compiled step kernel has no preconditioned form, falls back to the model-opaque pair of launches while a
        preconditioner is set.  ``set_precond_diag`` replaces it between draws, ``warmup`` estimates it."""
        fuse_builtin, _ = self._resolve_path(path)
        tn = self._resolve_tuning(tuning, knobs)
        graph, prefetch_rng, tune_placement = tn.get("graph"), tn.get("prefetch_rng"), tn.get("tune_placement")
        two_pass, single_launch = tn.get("two_pass"), tn.get("single_launch")
        self._epsilon = epsilon
        self._setup(model, None, init, seed, chains, chain_id0, ops)
        if precond_diag is not None:
            self._pack_precond(precond_diag)
        self._init_graph(graph, prefetch_rng)
        D, C, dev = self._dim, self._C, self._ops.device
        f64 = dict(dtype=torch.float64, device=dev)
        self._theta_p = self._new_state()
        self._grad = self._new_state()
        self._grad_p = self._new_state()
        self._lp = torch.empty(C, **f64)
        self._lp_p = torch.empty(C, **f64)
        self._fwd = torch.empty(C, **f64)
        self._rev = torch.empty(C, **f64)
        self._logu = torch.empty(C, **f64)
        self._ret = torch.empty(C, **f64)
        self._mask = torch.empty(C, dtype=torch.uint8, device=dev)
        self._accepted = torch.zeros(1, dtype=torch.int32, device=dev)
        self._draws = 0
        # As in HMCDiag: the D proposal normals and the accept uniform of draw n+1 do not depend
        # on draw n and are consumed in a fixed order (mala.py:44 then metropolis.py:74), so they
        # are generated on a second HIP stream under draw n's HBM-bound kernels.
        # With graph=True the randomness is generated in line (a captured draw stays a linear graph,
        # see ManyChainSampler), whatever prefetch_rng says; the draws are bit-identical either way.
        if prefetch_rng is None:
            prefetch_rng = self._batched and dev.type == "cuda"
        self._prefetch = bool(prefetch_rng) and self._batched and not self._use_graph
        # Philox streams: the normals come from the wavefront-per-chain generator, chain-major
        # (zt[c, d]); the consuming kernel turns them through LDS.  Otherwise (PCG64 host-seeded
        # single chains, tiny D): one lane per chain, normals in the state layout.
        self._chain_major = self._rng_kind == _lib.RNG_PHILOX and D >= 32
        ld = self._theta_dc.stride(0) if D > 1 else C
        can_two_pass = self._batched and self._chain_major and self._ops.mala_step_supported(C, D, ld)
        if two_pass and not can_two_pass:
            raise ValueError("two_pass=True needs a batched model, Philox streams, 32 <= D <= 1024 and an even number "
                             "of chains")
        self._two_pass = can_two_pass if two_pass is None else bool(two_pass)
        # a separable density the library can inline: the step kernel recomputes the gradients (none is stored between draws;
        # _grad is brought up to date when somebody asks for it) -- with a preconditioner only where the model's hook has
        # the preconditioned form (the built-in Gaussians)
        self._sep_capable = (bool(fuse_builtin) and self._two_pass and hasattr(model, "bk_mala_step")
                             and hasattr(model, "bk_eval"))
        self._sep_step = False
        self._grad_stale = False
        self._route()
        nbuf = 2 if self._prefetch else 1
        if self._chain_major:
            dp = (D + 7) // 8 * 8
            self._zt_bufs = [torch.empty((C, dp), **f64) for _ in range(nbuf)]
            self._z_bufs = [zt[:, :D].t() for zt in self._zt_bufs]
        elif self._prefetch:
            self._z_bufs = [self._new_state() for _ in range(2)]
        if self._prefetch or self._two_pass:
            self._logu_bufs = [torch.empty(C, **f64) for _ in range(nbuf)]
        if self._prefetch:
            self._ahead = LookAhead(dev)
            self._rng_logical = self._rng_state.clone()  # step by step: the table in front of the generator queued ahead
        # two-pass pipeline: theta_p holds the proposal of the NEXT draw (made by the previous
        # draw's kernel from normals generated one draw ahead).  A generation unit is
        # (U_n, Z_{n+1}): the accept uniform of draw n, then the D normals of draw n+1 -- stream
        # order.  The LOGICAL stream position after draw n lies inside unit n (after U_n): it is
        # snapshotted there, per double-buffer slot.
        self._pipe_valid = False   # theta_p is the proposal of the next draw
        if self._two_pass:
            self._snap = [torch.empty_like(self._rng_state) for _ in range(nbuf)]
        # ONE chain driven by a reference-style host model (the README example, config 1): after the model call a draw is
        # ONE launch (bk_mala_single_draw: proposal densities, accept test, select AND the next draw's proposal), the
        # model's outputs go in and the draw comes out through pinned host memory the device addresses directly, and
        # the host waits on a sequence word instead of synchronising the stream: 1 launch + 1 model call per draw
        # (the step-by-step path: 6 launches, 2 device-to-host and 1 host-to-device copies, 121 us per draw).
        can_single = (not self._batched) and dev.type == "cuda" and D <= self.SINGLE_LAUNCH_MAX_DIMS
        if single_launch and not can_single:
            raise ValueError("single_launch=True needs a single-chain host model on a GPU and at most "
                             f"{self.SINGLE_LAUNCH_MAX_DIMS} dimensions")
        self._single = can_single if single_launch is None else bool(single_launch)
        if self._single:
            self.path = "single chain, one launch per draw (bk_mala_single_draw)"
            self._h_in = torch.zeros(D + 1, dtype=torch.float64).pin_memory()
            self._h_out = torch.zeros(2 * D + 3, dtype=torch.float64).pin_memory()
            self._h_in_np, self._h_out_np = self._h_in.numpy(), self._h_out.numpy()
            self._snap1 = self._rng_state.clone()  # (a generator's store() leaves the key words alone)
            self._seq = 0.0
            self._single_fn = self._ops.lib.bk_mala_single_draw
        self.placement = None
        if self._wants_placement_tuning(tune_placement) and not self._two_pass:
            self._tune_placement()
        # mala.py:31-32: (logp, grad) at theta0
        self._materialize(self._eval_grad(self._theta_dc, self._grad, self._lp), self._grad)

    # -- the diagonal preconditioner ------------------------------------------------------------------------------
    def _pack_precond(self, v):
        if not self._batched:
            raise ValueError("precond_diag needs a batched device model (the one-launch single-chain mode is not "
                             "preconditioned)")
        return super()._pack_precond(v)

    def _route(self):
        """Which step kernel a two-pass draw uses, and `path`."""
        sep = self._sep_capable and (self._pd is None or getattr(self._model, "bk_mala_step_precond", False) is True)
        if self._sep_step and not sep:
            self._fresh_grad()  # the model-opaque step kernel selects between stored gradients
        self._sep_step = sep
        pc = self._pd is not None
        if getattr(self, "_single", False):
            return
        if sep:
            self.path = "two-pass, gradients recomputed in the step kernel (model.bk_mala_step)"
        elif self._two_pass and pc and self._sep_capable:
            self.path = ("two-pass (bk_mala_step_precond): the model's inlined step kernel has no preconditioned form, "
                         "model-opaque pair of launches")
        elif self._two_pass:
            self.path = "two-pass (bk_mala_step_precond)" if pc else "two-pass (bk_mala_step)"
        else:
            self.path = "step-by-step"

    def set_precond_diag(self, v):
        """Set or replace the diagonal preconditioner between draws (see ``precond_diag``).  Changes no logical stream
        position: a proposal made ahead with the old v is discarded and its normals are drawn again, same values (as
        ``refresh_cache``); captured graphs are dropped."""
        self._pack_precond(v)
        self._invalidate_pipe(restore_stream=True)
        self._route()

    def _propose(self, th, g, z, thp, eps):
        """theta' from drawn normals z (either layout) [mala.py:41-45]."""
        if self._pd is None:
            self._ops.mala_propose_from_normals(th, g, z, thp, eps, math.sqrt(2 * eps))
        else:
            self._ops.mala_propose_from_normals_precond(th, g, z, self._pd, thp, eps, math.sqrt(2 * eps))

    def _logq(self, th, g, thp, gp, eps):
        """Forward / reverse proposal densities [mala.py:50-53, 68-79]."""
        if self._pd is None:
            self._ops.mala_logq(th, g, thp, gp, eps, self._fwd, self._rev)
        else:
            self._ops.mala_logq_precond(th, g, thp, gp, self._pd, eps, self._fwd, self._rev)

    def _state_layout_normals(self):
        """D normals per chain in the state layout from the chain's stream (PCG64 streams or D < 32: one lane per chain,
        the values bk_mala_propose draws inside its kernel)."""
        if getattr(self, "_z_state", None) is None:
            self._z_state = self._new_state()
        self._ops.momentum_refresh(self._rng_kind, self._rng_state, None, 0.0, 1.0, self._z_state, None, None)
        return self._z_state

    def _fresh_grad(self):
        """The cached gradient of the current point; the separable step kernel does not keep it (recomputed on demand)."""
        if self._grad_stale:
            self._materialize(self._eval_grad(self._theta_dc, self._grad, None), self._grad)
            self._grad_stale = False
        return self._grad

    def refresh_cache(self):
        """Recompute the cached (logp, grad) of the current point (mala.py:31-32) after ``_theta`` was
        assigned or edited from outside, as the reference's constructor does for ``init``; a proposal
        made ahead from the old point is discarded (its normals are drawn again, same values)."""
        self._invalidate_pipe(restore_stream=True)
        self._materialize(self._eval_grad(self._theta_dc, self._grad, self._lp), self._grad)
        self._grad_stale = False

    def _drop_ahead(self):
        """Step by step with prefetch_rng, between two draws: drop the randomness generated ahead and take the stream back to
        where that began (the draw that queued the generator has joined it: LookAhead.join)."""
        if self._prefetch and not self._two_pass and self._ahead.ahead:
            self._rng_state.copy_(self._rng_logical)
            self._ahead.drop(wait=False)

    def _invalidate_pipe(self, restore_stream):
        """Between two draws (the last one has joined the generator queued ahead): the proposal made ahead is discarded,
        and with it, two-pass, the unit generated ahead; step by step the randomness generated ahead stays valid."""
        if (self._two_pass or getattr(self, "_single", False)) and self._pipe_valid and restore_stream:
            self._rng_state.copy_(self._logical_rng())  # un-consume what was generated ahead
        self._pipe_valid = False
        if self._prefetch and self._two_pass:
            self._ahead.drop(wait=False)
        elif self._prefetch:
            self._ahead.already_joined()
        self._drop_graphs()

    def _tune_placement(self):
        """Roles (theta', grad, grad') for the proposal, proposal-density and select kernels, which
        stream four to five arrays at equal offsets: see ManyChainSampler._tune_roles."""
        ops, th, eps = self._ops, self._theta_dc, float(self._epsilon)
        z = self._z_bufs[0] if hasattr(self, "_z_bufs") else None
        out = self._new_state()
        self._mask.fill_(1)

        def cost(a):
            thp, g, gp = a
            ms = self._time_ms(lambda: ops.mala_logq(th, g, thp, gp, eps, self._fwd, self._rev))
            ms += self._time_ms(lambda: ops.select_columns(self._mask, th, thp, g, gp, out))
            if z is not None:
                ms += self._time_ms(lambda: ops.mala_propose_from_normals(th, g, z, thp, eps, math.sqrt(2 * eps)))
            return ms

        keep = th.clone()  # the select kernel writes theta: restore the initial state afterwards
        (self._theta_p, self._grad, self._grad_p), rep = self._tune_roles([self._theta_p, self._grad, self._grad_p],
                                                                          cost)
        th.copy_(keep)
        self.placement = {"draw_kernels_ms_as_allocated": rep["ms_as_allocated"],
                          "draw_kernels_ms_chosen": rep["ms_chosen"], "assignments_tried": rep["assignments_tried"]}

    def _state_tensors(self):
        return {"theta": self._theta_dc, "grad": self._fresh_grad(), "lp": self._lp, "accepted": self._accepted}

    def _logical_rng(self):
        if getattr(self, "_single", False):
            if not self._pipe_valid:
                return self._rng_state
            torch.cuda.synchronize()
            return self._snap1  # (the next draw's normals are already consumed: the position after this draw's uniform)
        if self._two_pass:
            if not self._pipe_valid:
                return self._rng_state
            if self._ops.device.type == "cuda":
                torch.cuda.synchronize()
            return self._snap[self._ahead.consumed if self._prefetch else 0]  # (inside the unit the last draw consumed)
        if self._prefetch and self._ahead.ahead:
            self._ahead.synchronize()
            return self._rng_logical
        return self._rng_state

    def load_state_dict(self, sd):
        if self._two_pass:
            # draws handed out earlier alias past state arrays: restore into a fresh one
            self._theta_dc = self._new_state()
        super().load_state_dict(sd)

    def _state_extra(self):
        return {"epsilon": float(self._epsilon), "precond_diag": self._precond_extra()}

    def _load_extra(self, extra):
        # (checkpoints written before the step size and the preconditioner were carried hold neither: nothing changes)
        if "epsilon" in extra:
            self._epsilon = extra["epsilon"]
        pv = self._precond_from_extra(extra)
        if pv is not None:
            self._pack_precond(pv)
            self._grad_stale = False  # (the gradient of the restored point came with it)
            self._route()

    def _after_load(self):
        self._grad_stale = False  # (the gradient of the restored point came with it)
        if self._prefetch:
            self._ahead.reset()
        self._invalidate_pipe(restore_stream=False)  # the stream was just restored to its logical position

    def _gen(self, slot):
        if self._chain_major:
            self._ops.normals_chain_major(self._rng_kind, self._rng_state, self._zt_bufs[slot], self._dim)
        else:
            self._ops.momentum_refresh(self._rng_kind, self._rng_state, None, 0.0, 1.0, self._z_bufs[slot],
                                       None, None)
        self._ops.log_uniform(self._rng_kind, self._rng_state, self._logu_bufs[slot])

    def _take_randomness(self):
        cur = self._ahead.take(self._gen)
        self._ahead.start_next(self._gen, (self._rng_logical, self._rng_state))
        return self._z_bufs[cur], self._logu_bufs[cur]

    # -- two-pass: generation units (U_n, Z_{n+1}) ------------------------------------------------------
    def _gen_unit(self, slot):
        ops = self._ops
        ops.log_uniform(self._rng_kind, self._rng_state, self._logu_bufs[slot])     # U_n   [metropolis.py:74]
        # Z_{n+1} [mala.py:44]; the generator leaves the table as it found it -- the position after draw n
        # -- in snap[slot]
        ops.normals_chain_major(self._rng_kind, self._rng_state, self._zt_bufs[slot], self._dim, self._snap[slot])

    # The schedule is fixed: the generator of the next unit is queued on the side stream with the model's launch, on its
    # own grid, and the step kernel does not wait for it.  Rounds 2-5 serialized the two -- the generator needed 169
    # registers per lane, could not sit beside a step workgroup (192 x 512 threads per CU), and they only slowed each other
    # down (1.52 against 1.3 ms per draw).  Round 6's generator needs 93 and finishes in 0.26-0.29 ms: letting its tail run
    # under the step kernel is the fastest of the 32 schedules measured (65,536 x 1024, one box: model-opaque 1.124 ms
    # against 1.152 serialized, density inlined 0.802 against 0.876; starting it with the step kernel instead, or on a
    # grid bounded to one to four workgroups per CU, lost too: profiles/r6_mala.md).  Results never depended on it (events order the data).
    def _take_unit(self):
        """(log u of this draw, chain-major normals of the next); with prefetch also starts the
        unit after that on the side stream."""
        cur = 0
        if not self._prefetch:
            self._gen_unit(0)
        else:
            cur = self._ahead.take(self._gen_unit)
            self._ahead.start_next(self._gen_unit)
        return self._logu_bufs[cur], self._zt_bufs[cur]

    def accept_rate(self) -> float:
        n = self._draws * self._C
        return float(self._accepted.item()) / n if n else float("nan")

    @property
    def last_accept(self):
        return self._mask.bool() if self._batched else bool(self._mask[0].item())

    @property
    def _log_p_theta(self):
        return self._lp if self._batched else float(self._lp[0].item())

    @property
    def _log_p_grad_theta(self):
        return self._fresh_grad().t() if self._batched else self._grad[:, 0].cpu().numpy()

    def _graph_key(self):
        return float(self._epsilon)

    # -- one chain, one launch per draw ---------------------------------------------------------------------------
    def _launch_single(self, have_prop):
        self._seq += 1.0
        eps = float(self._epsilon)
        rc = self._single_fn(self._rng_kind, self._rng_state.data_ptr(), self._rng_state.stride(0),
                             self._theta_dc.data_ptr(), self._grad.data_ptr(), self._lp.data_ptr(), self._theta_p.data_ptr(),
                             self._h_in.data_ptr(), self._h_out.data_ptr(), self._snap1.data_ptr(), self._snap1.stride(0),
                             self._mask.data_ptr(), self._accepted.data_ptr(), eps, math.sqrt(2 * eps), self._dim,
                             int(have_prop), self._seq, torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "bk_mala_single_draw")
        # wait for the launch's last store (the sequence word, released at system scope behind everything else)
        flag, i, want = self._h_out_np, 2 * self._dim + 2, self._seq
        for _ in range(200000):
            if flag[i] == want:
                return
        torch.cuda.current_stream().synchronize()  # (a slow box, or an error that the synchronisation reports)
        if flag[i] != want:
            raise _lib.BkHipError("bk_mala_single_draw did not complete")

    def _sample_single(self):
        D = self._dim
        if not self._pipe_valid:
            self._launch_single(0)  # this draw's proposal from the stream's next D normals (mala.py:41-45)
            self._pipe_valid = True
        hin, hout = self._h_in_np, self._h_out_np
        self._grad_calls += 1
        lp, g = self._model.log_density_gradient(np.array(hout[D + 2:2 * D + 2]))             # mala.py:46-48
        hin[1:] = np.broadcast_to(np.asarray(g, dtype=np.float64), (D,))  # array-likes allowed (mala.py:32)
        hin[0] = float(lp)
        self._launch_single(1)                                                                 # mala.py:50-66, then :41-45
        self._draws += 1
        return np.array(hout[:D]), np.float64(hout[D])

    def sample(self):
        if self._single:
            return self._sample_single()
        if self._two_pass and self._pipe_valid and self._pipe_eps != float(self._epsilon):
            # epsilon was assigned between draws (mala.py:23 is a plain attribute): the proposal made ahead used the old one
            self._invalidate_pipe(restore_stream=True)
        self._run_draw(self._draw2 if self._two_pass else self._draw)
        if self._sep_step:
            self._grad_stale = True  # (here, not in _draw2: a replayed hipGraph does not run the Python of the draw)
        self._join_ahead()
        self._draws += 1
        if self._two_pass and not self._use_graph:
            return self._theta_dc.t(), self._ret.clone()  # the new state array itself (never written again)
        return self._draw_out(self._theta_dc, self._ret)

    def _draw2(self):
        ops = self._ops
        eps = float(self._epsilon)
        s2 = math.sqrt(2 * eps)
        th, thp = self._theta_dc, self._theta_p
        if not self._pipe_valid:
            # this draw's proposal from the stream's next D normals (mala.py:41-45); later draws'
            # proposals are written by the previous draw's kernel
            ops.normals_chain_major(self._rng_kind, self._rng_state, self._zt_bufs[0], self._dim)
            self._propose(th, self._fresh_grad(), self._z_bufs[0], thp, eps)
            self._pipe_valid, self._pipe_eps = True, eps
        logu, zt_next = self._take_unit()
        if self._sep_step:
            self._eval_logp(thp, self._lp_p)                                                   # mala.py:46-48, log density
            self._grad_calls += 1   # (the gradient of the same call is evaluated inside the step kernel)
            gp = None
        else:
            gp = self._materialize(self._eval_grad(thp, self._grad_p, self._lp_p), self._grad_p)   # mala.py:46-48
        out = th if self._use_graph else self._new_state()
        if self._sep_step and self._pd is not None:
            self._model.bk_mala_step(th, out, thp, self._lp, self._lp_p, logu, zt_next, eps, s2,
                                     self._mask, self._ret, self._accepted, precond=self._pd)
        elif self._sep_step:
            self._model.bk_mala_step(th, out, thp, self._lp, self._lp_p, logu, zt_next, eps, s2,
                                     self._mask, self._ret, self._accepted)                    # mala.py:50-66
        elif self._pd is not None:
            ops.mala_step_precond(th, out, self._grad, thp, gp, self._pd, self._lp, self._lp_p, logu, zt_next, eps, s2,
                                  self._mask, self._ret, self._accepted)
        else:
            ops.mala_step(th, out, self._grad, thp, gp, self._lp, self._lp_p, logu, zt_next, eps, s2,
                          self._mask, self._ret, self._accepted)                               # mala.py:50-66
        self._theta_dc = out

    def _draw(self):
        ops = self._ops
        eps = float(self._epsilon)
        th, thp = self._theta_dc, self._theta_p
        if self._prefetch:
            z, logu = self._take_randomness()
            self._propose(th, self._grad, z, thp, eps)
        elif self._chain_major:
            logu = self._logu
            ops.normals_chain_major(self._rng_kind, self._rng_state, self._zt_bufs[0], self._dim)
            ops.log_uniform(self._rng_kind, self._rng_state, logu)  # right after the normals: same stream order
            self._propose(th, self._grad, self._z_bufs[0], thp, eps)
        elif self._pd is not None:
            # (bk_mala_propose draws its normals inside the kernel and has no preconditioned form: the same normals from
            # the generator, then the uniform -- the same stream order)
            logu = self._logu
            z = self._state_layout_normals()
            ops.log_uniform(self._rng_kind, self._rng_state, logu)
            self._propose(th, self._grad, z, thp, eps)
        else:
            logu = self._logu
            ops.mala_propose(self._rng_kind, self._rng_state, th, self._grad, thp, eps, math.sqrt(2 * eps))
            ops.log_uniform(self._rng_kind, self._rng_state, logu)  # right after the normals: same stream order
        gp = self._materialize(self._eval_grad(thp, self._grad_p, self._lp_p), self._grad_p)
        self._logq(th, self._grad, thp, gp, eps)
        ops.mh_accept(_lib.ACCEPT_MALA, self._lp, self._fwd, self._lp_p, self._rev, logu,
                      self._mask, self._ret, self._accepted)
        self._select(self._mask, th, thp, self._grad, gp)

    # -- warmup -------------------------------------------------------------------------------------
    def _warmup_draw(self, zero, ratio):
        """One draw as the step-by-step composition, whatever the sampler's own path: generator, proposal from the drawn
        normals, the model's gradient op, proposal densities, the acceptance statistic, accept, select."""
        ops = self._ops
        eps = float(self._epsilon)
        th, thp, logu = self._theta_dc, self._theta_p, self._logu
        if self._chain_major:
            ops.normals_chain_major(self._rng_kind, self._rng_state, self._zt_bufs[0], self._dim)
            z = self._z_bufs[0]
        else:
            z = self._state_layout_normals()
        ops.log_uniform(self._rng_kind, self._rng_state, logu)  # right after the normals: same stream order
        self._propose(th, self._grad, z, thp, eps)
        gp = self._materialize(self._eval_grad(thp, self._grad_p, self._lp_p), self._grad_p)
        self._logq(th, self._grad, thp, gp, eps)
        # the log acceptance ratio in bk_mh_accept's association, before the test overwrites lp; bk_accept_stat then takes
        # (ratio - 0) - (0 - 0), which is exact
        torch.sub(self._lp_p, self._lp, out=ratio)
        torch.sub(self._rev, self._fwd, out=self._ret)
        ratio.add_(self._ret)
        ops.accept_stat(zero, None, ratio, None, self._stat, self._stat_work)
        ops.mh_accept(_lib.ACCEPT_MALA, self._lp, self._fwd, self._lp_p, self._rev, logu,
                      self._mask, self._ret, self._accepted)
        self._select(self._mask, th, thp, self._grad, gp)

    def warmup(self, draws, target_accept=0.574, adapt_metric=True, group=None):
        """Run `draws` draws that tune epsilon and (adapt_metric) the diagonal preconditioner from ALL chains of all ranks,
        then keep the tuned values: afterwards the sampler samples with them.  -> the report dict of ``HMCDiag.warmup``:
        ``stepsize`` (the tuned epsilon), ``precond_diag`` (host copy, None if none is set), per-draw ``eps`` and ``alpha``
        histories, ``window_ends``, ``nan_chains``.

        The schedule, the shrinkage of the pooled window variance, the restart rule and the sum over ranks are
        ``HMCDiag.warmup``'s; the default target 0.574 is the asymptotically optimal acceptance of MALA (Roberts & Rosenthal
        1998).  The statistic of a draw is mean_c min(1, exp(min(0, r_c))) of the log acceptance ratio
        r = (lp' - lp) + (rev - fwd) (bk_accept_stat; a NaN ratio counts 0).

        Warmup draws run step by step on every configuration, with nothing generated or proposed ahead: the two-pass kernel
        writes draw n+1's proposal with draw n's epsilon, which dual averaging changes after every draw, and one kernel
        sequence makes the report identical bit for bit whatever ``two_pass``, ``path``, ``prefetch_rng`` and ``graph`` say.
        A proposal made ahead before the call is discarded (its normals are drawn again); afterwards graphs are dropped
        and the next ``sample()`` makes its proposal with the final epsilon and v."""
        draws = self._check_warmup(draws, target_accept)
        # pipeline off: back to the logical stream position, nothing made or generated ahead
        self._invalidate_pipe(restore_stream=True)
        self._drop_ahead()
        self._fresh_grad()
        if self._two_pass and not self._use_graph:
            # (the state array is the last draw handed out: the in-place select below must not write into it)
            keep = self._theta_dc
            self._theta_dc = self._new_state()
            self._theta_dc.copy_(keep)
        f64 = dict(dtype=torch.float64, device=self._ops.device)
        zero, ratio = torch.zeros(self._C, **f64), torch.empty(self._C, **f64)
        try:
            return self._warmup_loop(draws, target_accept, group, lambda: self._warmup_draw(zero, ratio),
                                     self._diag_estimator if adapt_metric else None)
        finally:
            self._grad_stale = False  # (the select above kept the stored gradient current)
            self._invalidate_pipe(restore_stream=False)
