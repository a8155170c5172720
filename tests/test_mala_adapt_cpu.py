"""The preconditioned MALA and MALA.warmup without a GPU: the sampler's host logic on the NumPy stand-in
(tests/fake_ops_mala_adapt.py), the stand-in's summation orders against plain sums, argument checks of the C ABI, and two
gloo ranks."""
import ctypes
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import bayes_kit_amd as bk
from tests import mala_adapt_parity as mp
from tests.fake_ops import FakeOps
from tests.fake_ops_mala_adapt import MalaAdaptFakeOps, step_slots, step_sum

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
# (the stand-in has neither a side stream nor hipGraphs: prefetch_rng and graph are varied in tests/test_gpu_mala_adapt.py)
VARIANTS = [dict(two_pass=False), dict(path="opaque"), dict(path="auto")]


# ---- the stand-in itself -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 32, 33, 128, 129, 257, 513, 1000, 1024])
def test_step_sum_is_a_sum_in_another_order(D):
    x = np.random.default_rng(D).normal(size=(D, 5)) ** 2
    np.testing.assert_allclose(step_sum(x), x.sum(axis=0), rtol=1e-13)
    assert step_slots(D) * 64 >= D
    one = np.zeros((D, 1))
    one[D - 1] = 3.0  # (the last row alone: exact in any order)
    assert step_sum(one)[0] == 3.0


def test_stand_in_with_ones_is_the_parent_stand_in():
    """The preconditioned restatements with v = 1 against tests/fake_ops.py's plain ones (sequential sums: the decisions and
    every elementwise output are the same, the densities agree to rounding)."""
    g = np.random.default_rng(1)
    D, C, eps = 40, 12, 0.05
    s2 = float(np.sqrt(2 * eps))
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x))  # noqa: E731
    th, gr, z = g.normal(size=(D, C)), g.normal(size=(D, C)), g.normal(size=(D, C))
    new, old = MalaAdaptFakeOps(), FakeOps()
    pd = torch.empty((3, D), dtype=torch.float64)
    new.precond_pack(torch.ones(D, dtype=torch.float64), pd)
    a, b = torch.empty(D, C, dtype=torch.float64), torch.empty(D, C, dtype=torch.float64)
    new.mala_propose_from_normals_precond(t(th), t(gr), t(z), pd, a, eps, s2)
    old.mala_propose_from_normals(t(th), t(gr), t(z), b, eps, s2)
    assert torch.equal(a, b)
    thp, gp = a.numpy(), g.normal(size=(D, C))
    f1, r1, f0, r0 = (torch.empty(C, dtype=torch.float64) for _ in range(4))
    new.mala_logq_precond(t(th), t(gr), t(thp), t(gp), pd, eps, f1, r1)
    old.mala_logq(t(th), t(gr), t(thp), t(gp), eps, f0, r0)
    np.testing.assert_allclose(f1.numpy(), f0.numpy(), rtol=1e-13)
    np.testing.assert_allclose(r1.numpy(), r0.numpy(), rtol=1e-13)
    new.mala_logq(t(th), t(gr), t(thp), t(gp), eps, f0, r0)
    assert torch.equal(f1, f0) and torch.equal(r1, r0)


# ---- 1. against the oracle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["auto", "opaque"])
@pytest.mark.parametrize("C,D", [(20, 48), (10, 130), (9, 6)])
def test_precond_diag_equals_the_oracle_on_the_rescaled_target(C, D, path):
    ops = MalaAdaptFakeOps()
    s = mp.check_vs_oracle(ops, C, D, path)
    if D == 6:
        assert s.path == "step-by-step" and ops.calls["mala_propose_from_normals_precond"] == 6
        assert ops.calls["mala_logq_precond"] == 6 and "mala_propose" not in ops.calls
    elif path == "auto":
        assert ops.calls["mala_step_gaussian_precond"] == 6 and "mala_step_precond" not in ops.calls
    else:
        assert ops.calls["mala_step_precond"] == 6 and "mala_step_gaussian_precond" not in ops.calls


# ---- 2. ones --------------------------------------------------------------------------------------------------------
def test_precond_of_ones_is_the_plain_sampler():
    mp.check_identity(MalaAdaptFakeOps(), 20, 48, [dict(), dict(two_pass=False), dict(path="opaque")])
    mp.check_identity(MalaAdaptFakeOps(), 9, 6)


# ---- 3. paths ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,D", [(2, 32), (34, 33), (146, 40), (130, 129), (16, 257), (18, 1000), (32, 1024)])
def test_paths_agree_and_the_preconditioner_may_change_between_draws(C, D):
    mp.check_paths_agree(MalaAdaptFakeOps(), C, D, VARIANTS)


# ---- 5. a model without the preconditioned step kernel ----------------------------------------------------------------
class _NoPrecondStep(bk.DiagGaussian):
    """A model with the inlined step kernel but no preconditioned form of it (what CTarget.from_source(form="elementwise")
    and traced densities are)."""

    bk_mala_step_precond = False

    def bk_mala_step(self, theta, theta_out, theta_prop, lp, lp_prop, log_u, zt_next, eps, sqrt2eps, mask, ret, count):
        super().bk_mala_step(theta, theta_out, theta_prop, lp, lp_prop, log_u, zt_next, eps, sqrt2eps, mask, ret, count)


def test_a_model_without_the_preconditioned_step_kernel_falls_back_to_the_opaque_pair():
    """... at construction, between draws (set_precond_diag), through a checkpoint and through warmup: the same draws as
    the built-in model on its inlined preconditioned kernel, and `path` says so."""
    D, C = 48, 12
    lam = np.logspace(0, 1, D)
    v = mp.perturbed_variances(lam)
    oa, ob = MalaAdaptFakeOps(), MalaAdaptFakeOps()
    a = mp.make(oa, C, D, v, model=_NoPrecondStep(lam, ops=oa))
    b = mp.make(ob, C, D, v)
    assert "model-opaque pair" in a.path and "no preconditioned form" in a.path and "model.bk_mala_step" in b.path
    for x, y in zip(mp.run_draws(a, 3), mp.run_draws(b, 3)):
        assert np.array_equal(x, y)
    assert oa.calls["mala_step_precond"] == 3 and "mala_step_gaussian_precond" not in oa.calls
    assert ob.calls["mala_step_gaussian_precond"] == 3
    # later: two draws on the inlined kernel, then the preconditioner
    a, b = mp.make(oa, C, D, model=_NoPrecondStep(lam, ops=oa)), mp.make(ob, C, D)
    assert "model.bk_mala_step" in a.path
    mp.run_draws(a, 2), mp.run_draws(b, 2)
    a.set_precond_diag(v), b.set_precond_diag(v)
    assert "model-opaque pair" in a.path
    for x, y in zip(mp.run_draws(a, 3), mp.run_draws(b, 3)):
        assert np.array_equal(x, y)
    assert np.array_equal(a.rng_state(), b.rng_state())
    # a checkpoint with a preconditioner into a sampler on the inlined kernel
    oc = MalaAdaptFakeOps()
    c = mp.make(oc, C, D, model=_NoPrecondStep(lam, ops=oc))
    mp.run_draws(c, 1)
    c.load_state_dict(b.state_dict())
    assert "model-opaque pair" in c.path
    assert np.array_equal(mp.run_draws(c, 2)[0], mp.run_draws(b, 2)[0])
    # warmup
    a, b = mp.make(oa, C, D, eps=0.01, model=_NoPrecondStep(lam, ops=oa)), mp.make(ob, C, D, eps=0.01)
    assert mp.reports_equal(a.warmup(60), b.warmup(60))
    assert np.array_equal(mp.run_draws(a, 2)[0], mp.run_draws(b, 2)[0])


# ---- 6. checkpoint ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,D,kw", [(20, 48, dict()), (20, 48, dict(path="opaque")), (9, 6, dict())])
def test_checkpoint_carries_preconditioner_and_epsilon(C, D, kw):
    mp.check_checkpoint(MalaAdaptFakeOps(), C, D, **kw)


# ---- 8. / 9. warmup -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [11, 3])
def test_warmup_end_to_end_on_the_stand_in(seed):
    """lam = logspace(0, 4, 32), 512 chains from N(0, I), epsilon = 1e-5, warmup(300): the conditions of
    mala_adapt_parity.check_warmup_report, whose docstring and profiles/mala_warmup.md hold the stand-in's eight-seed ranges.
    Seed 11 is also the run that tests/test_gpu_mala_adapt.py compares the HIP library with: the recorded report and the
    two draws that follow are still what the stand-in produces."""
    if seed == 11:
        rec = mp.warmup_record(MalaAdaptFakeOps(), 300)
        assert rec == mp.golden_record(300)
        rep, lam = mp.as_report(rec), np.logspace(0, 4, 32)
    else:
        s, rep, lam = mp.run_warmup(MalaAdaptFakeOps(), seed)
        assert s._epsilon == rep["stepsize"] and isinstance(s._epsilon, float)
        assert np.array_equal(s.precond_diag, rep["precond_diag"])
        th, lp = s.sample()  # ... and samples on with the adapted values
        assert np.isfinite(np.asarray(th)).all()
    mp.check_warmup_report(rep, lam)
    e = rep["window_ends"][0]
    assert 1e-5 < rep["eps"][e - 1] < 1e-3  # bounded by the stiffest direction (lam = 1e4) until the first window ends
    assert rep["stepsize"] > 1000.0 * rep["eps"][e - 1]  # ... three orders of magnitude more once every direction has unit scale


def test_warmup_with_one_window_is_the_recorded_run():
    """warmup(110): one window, ending after draw 99 (tests/test_gpu_mala_adapt.py compares its v with the HIP library's)."""
    rec = mp.warmup_record(MalaAdaptFakeOps(), 110)
    assert rec["window_ends"] == [99] and rec == mp.golden_record(110)


def test_warmup_is_reproducible_whatever_the_path_and_knobs():
    reps, after = [], []
    for kw in (dict(), dict(), dict(two_pass=False), dict(path="opaque"), dict(before=2), dict(before=2, two_pass=False)):
        s, rep, _ = mp.run_warmup(MalaAdaptFakeOps(), 3, draws=60, C=96, **kw)
        reps.append(rep)
        after.append(mp.run_draws(s, 3)[0])
    assert reps[0]["window_ends"] == [54] and reps[0]["stepsize"] > 1e-5 and reps[0]["precond_diag"] is not None
    for i in (1, 2, 3):
        assert mp.reports_equal(reps[0], reps[i]) and np.array_equal(after[0], after[i]), i
    # two pipelined draws before warmup: the proposal made ahead is discarded, as if nothing had been made ahead
    assert mp.reports_equal(reps[4], reps[5]) and np.array_equal(after[4], after[5])


def test_warmup_runs_the_step_by_step_composition_on_every_configuration():
    ops = MalaAdaptFakeOps()
    s, rep, _ = mp.run_warmup(ops, 5, draws=30, C=16)
    assert "model.bk_mala_step" in s.path and rep["window_ends"] == [27]
    assert "mala_step_gaussian" not in ops.calls and "mala_step" not in ops.calls and "mala_propose" not in ops.calls
    assert ops.calls["accept_stat"] == 30 and ops.calls["mh_accept"] == 30
    assert ops.calls["mala_logq"] == 27 and ops.calls["mala_logq_precond"] == 3
    mp.run_draws(s, 2)
    assert ops.calls["mala_step_gaussian_precond"] == 2  # back on its own path, with the adapted values
    s2, rep2, _ = mp.run_warmup(MalaAdaptFakeOps(), 5, draws=15, C=16)
    assert rep2["window_ends"] == [] and rep2["precond_diag"] is None  # fewer than 20 draws: the step size alone
    s3 = mp.make(MalaAdaptFakeOps(), 8, 40, np.full(40, 0.5))
    rep3 = s3.warmup(30, adapt_metric=False)
    assert rep3["window_ends"] == [] and np.array_equal(rep3["precond_diag"], np.full(40, 0.5))


# ---- 10. two ranks ------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_rank_warmup():
    """Two gloo ranks x 256 chains: both ranks end with the same epsilon and v bit for bit (they see the same gathered sums
    in rank order), and the 2 x 256-chain run meets the end-to-end conditions."""
    port = _free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "mala_adapt_dist_worker.py")], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(out)
    reps = []
    for p, out in zip(procs, outs):
        assert p.returncode == 0, out
        reps.append(json.loads([l for l in out.splitlines() if l.startswith("{")][-1]))
    assert reps[0]["stepsize"] == reps[1]["stepsize"] and reps[0]["precond_diag"] == reps[1]["precond_diag"]
    assert reps[0] == reps[1]
    mp.check_warmup_report(dict(reps[0], precond_diag=np.array(reps[0]["precond_diag"])), np.logspace(0, 4, 32))


# ---- 11. validation ---------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument():
    ops = MalaAdaptFakeOps()
    lam = np.array([1.0, 2.0, 3.0])

    def make(**kw):
        return bk.MALA(bk.DiagGaussian(lam, ops=ops), 0.1, chains=4, seed=1, ops=ops, **kw)

    with pytest.raises(TypeError):
        bk.MALA(bk.DiagGaussian(lam, ops=ops), 0.1, None, 1, np.ones(3))  # keyword-only
    with pytest.raises(ValueError, match="precond_diag has 2 entries"):
        make(precond_diag=np.ones(2))
    with pytest.raises(ValueError, match="precond_diag has 4 entries"):
        make().set_precond_diag(np.ones(4))
    for bad in ([1.0, 0.0, 1.0], [1.0, -2.0, 1.0], [1.0, np.nan, 1.0], [1.0, np.inf, 1.0]):
        with pytest.raises(ValueError, match="precond_diag must hold finite, positive"):
            make(precond_diag=np.array(bad))
        s = make(precond_diag=np.ones(3))
        with pytest.raises(ValueError, match="precond_diag must hold finite, positive"):
            s.set_precond_diag(np.array(bad))
        assert np.array_equal(s.precond_diag, np.ones(3))  # (a refused v leaves the old one)
    assert make().precond_diag is None
    with pytest.raises(ValueError, match="draws"):
        make().warmup(0)
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="target_accept"):
            make().warmup(10, target_accept=bad)

    # a single-chain host model: no preconditioner, no warmup
    from oracle import models as om

    with pytest.raises(ValueError, match="precond_diag needs a batched device model"):
        bk.MALA(om.DiagGaussian(lam), 0.1, seed=1, precond_diag=np.ones(3), ops=ops)
    h = bk.MALA(om.DiagGaussian(lam), 0.1, seed=1, ops=ops)
    with pytest.raises(ValueError, match="precond_diag needs a batched device model"):
        h.set_precond_diag(np.ones(3))
    with pytest.raises(ValueError, match="warmup needs a batched device model"):
        h.warmup(10)


def test_argument_errors_of_the_new_entry_points_without_a_gpu():
    """BK_E_ARG on null required pointers, BK_E_ALIGN where bk_mala_step returns it, C == 0 or D == 0 is BK_OK: all decided
    before any HIP call."""
    from bayes_kit_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    E_ARG, E_ALIGN, OK = -1, -2, 0
    step = lib.bk_mala_step_precond
    args = lambda **kw: [kw.get(k, d) for k, d in (("th", p), ("out", p), ("g", p), ("thp", p), ("gp", p), ("ld", 4), ("pc", p),  # noqa: E731
                                                  ("lp", p), ("lpp", p), ("logu", p), ("zt", None), ("ldz", 0), ("eps", 0.1),
                                                  ("s", 0.4), ("mask", None), ("ret", None), ("cnt", None), ("C", 4), ("D", 2),
                                                  ("stream", None))]
    for k in ("th", "out", "g", "thp", "gp", "pc", "lp", "lpp", "logu"):
        assert step(*args(**{k: None})) == E_ARG, k
    assert step(*args(C=-1)) == E_ARG and step(*args(D=-1)) == E_ARG
    assert step(*args(C=0)) == OK and step(*args(D=0)) == OK
    assert step(*args(C=3)) == E_ALIGN and step(*args(ld=5)) == E_ALIGN and step(*args(ld=2)) == E_ALIGN
    assert step(*args(D=1025)) == E_ALIGN and step(*args(th=p + 8)) == E_ALIGN
    assert step(*args(zt=p, ldz=1)) == E_ALIGN and step(*args(zt=p + 8, ldz=2)) == E_ALIGN
    assert lib.bk_mala_step(*[a for i, a in enumerate(args(C=3)) if i != 6]) == E_ALIGN  # (the neighbour's answers)

    gs = lib.bk_mala_step_gaussian_precond
    gargs = lambda **kw: [kw.get(k, d) for k, d in (("th", p), ("out", p), ("thp", p), ("ld", 4), ("lam", p), ("pc", p), ("lp", p),  # noqa: E731
                                                   ("lpp", p), ("logu", p), ("zt", None), ("ldz", 0), ("eps", 0.1), ("s", 0.4),
                                                   ("mask", None), ("ret", None), ("cnt", None), ("C", 4), ("D", 2),
                                                   ("stream", None))]
    for k in ("th", "out", "thp", "pc", "lp", "lpp", "logu"):
        assert gs(*gargs(**{k: None})) == E_ARG, k
    assert gs(*gargs(C=0)) == OK and gs(*gargs(D=0)) == OK and gs(*gargs(C=0, lam=None)) == OK
    assert gs(*gargs(C=3)) == E_ALIGN and gs(*gargs(th=p + 8)) == E_ALIGN

    pr = lib.bk_mala_propose_from_normals_precond
    pargs = lambda **kw: [kw.get(k, d) for k, d in (("th", p), ("g", p), ("z", p), ("zsd", 4), ("zsc", 1), ("pc", p), ("thp", p),  # noqa: E731
                                                   ("ld", 4), ("eps", 0.1), ("s", 0.4), ("C", 4), ("D", 2), ("stream", None))]
    for k in ("th", "g", "z", "pc", "thp"):
        assert pr(*pargs(**{k: None})) == E_ARG, k
    assert pr(*pargs(C=-1)) == E_ARG and pr(*pargs(ld=3)) == E_ALIGN and pr(*pargs(zsd=3, zsc=3)) == E_ALIGN
    assert pr(*pargs(C=0)) == OK and pr(*pargs(D=0)) == OK

    lq = lib.bk_mala_logq_precond
    largs = lambda **kw: [kw.get(k, d) for k, d in (("th", p), ("g", p), ("thp", p), ("gp", p), ("ld", 4), ("pc", p), ("eps", 0.1),  # noqa: E731
                                                   ("f", p), ("r", p), ("C", 4), ("D", 2), ("stream", None))]
    for k in ("th", "g", "thp", "gp", "pc", "f", "r"):
        assert lq(*largs(**{k: None})) == E_ARG, k
    assert lq(*largs(D=-1)) == E_ARG and lq(*largs(ld=3)) == E_ALIGN
    assert lq(*largs(C=0)) == OK and lq(*largs(D=0)) == OK
