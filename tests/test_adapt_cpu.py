"""The diagonal preconditioner, the adaptation statistics and HMCDiag.warmup without a GPU: the host controller alone,
the samplers' host logic on the NumPy stand-in (tests/fake_ops_adapt.py), argument checks of the C ABI, and two gloo ranks."""
import ctypes
import json
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import bayes_kit_amd as bk
from bayes_kit_amd.adapt import DualAveraging, warmup_windows
from tests import adapt_parity as ap
from tests.fake_ops_adapt import AdaptFakeOps, accept_stat_ref

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


# ---- the preconditioner --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ap.PATHS)
def test_precond_diag_equals_the_oracle_dense_sampler(path):
    ap.check_precond_vs_oracle(AdaptFakeOps(), 8, 6, path)
    ap.check_precond_vs_oracle(AdaptFakeOps(), 6, 40, path)  # (D >= 32: chain-major normals on the whole-draw path)


def test_paths_agree_bit_for_bit_and_the_metric_may_change_between_draws():
    ap.check_paths_agree(AdaptFakeOps(), 6, 6, [dict()])
    ap.check_paths_agree(AdaptFakeOps(), 5, 40, [dict()])


def test_the_whole_draw_path_is_taken_with_a_preconditioner():
    ops = AdaptFakeOps()
    ap.precond_driver(ops, 6, 40, "auto")
    assert ops.calls["hmc_draw_gaussian_precond"] == 4 and "leapfrog_finish_precond" not in ops.calls
    ops = AdaptFakeOps()
    ap.precond_driver(ops, 6, 40, "opaque")
    assert ops.calls["momentum_refresh_precond"] == 4 and ops.calls["leapfrog_finish_precond"] == 4
    assert "hmc_draw_gaussian_precond" not in ops.calls


def test_precond_of_ones_is_the_plain_sampler():
    ap.check_identity(AdaptFakeOps(), 6, 6)
    ap.check_identity(AdaptFakeOps(), 5, 40)


@pytest.mark.parametrize("path", ap.PATHS)
def test_checkpoint_carries_preconditioner_and_step_size(path):
    ap.check_checkpoint(AdaptFakeOps(), 6, 6, path)
    ap.check_checkpoint(AdaptFakeOps(), 6, 36, path)


def test_a_lane_spread_density_falls_back_to_the_step_path():
    """bk.Funnel offers bk_hmc_proposal (kinetic energy summed inside its launch): with a preconditioner the sampler
    issues one launch per leapfrog step instead, same draws as the opaque path."""
    outs = []
    for path in ("auto", "opaque"):
        ops = AdaptFakeOps()
        s = bk.HMCDiag(bk.Funnel(5, ops=ops), 0.05, 4, chains=6, seed=2, precond_diag=np.linspace(0.5, 2.0, 5), path=path,
                       ops=ops)
        outs.append(ap.run_draws(s, 3)[0])
        assert "hmc_trajectory_funnel" not in ops.calls and ops.calls["leapfrog_finish_precond"] == 3
    assert np.array_equal(outs[0], outs[1])


class _NoPrecondDraw(bk.DiagGaussian):
    """A model with the whole-draw hook but no preconditioned form of it (what CTarget.from_source(form="elementwise") and
    traced densities are): bk_hmc_draw_precond is hidden."""

    def __getattribute__(self, name):
        if name == "bk_hmc_draw_precond":
            raise AttributeError(name)
        return super().__getattribute__(name)


@pytest.mark.parametrize("D", [6, 40])
def test_a_model_without_the_preconditioned_whole_draw_falls_back_to_the_step_path(D):
    """... at construction, and between draws when the preconditioner arrives later (set_precond_diag, warmup, a
    checkpoint): the same draws as the built-in model on its whole-draw kernel."""
    lam = np.logspace(0, 1, D)
    v = ap.perturbed_variances(lam)
    mk = lambda cls, ops, **kw: bk.HMCDiag(cls(lam, ops=ops), 0.05, 7, chains=6, seed=8, ops=ops, **kw)  # noqa: E731
    assert not hasattr(_NoPrecondDraw(lam), "bk_hmc_draw_precond") and hasattr(_NoPrecondDraw(lam), "bk_hmc_draw")
    oa, ob = AdaptFakeOps(), AdaptFakeOps()
    a, b = mk(_NoPrecondDraw, oa, precond_diag=v), mk(bk.DiagGaussian, ob, precond_diag=v)
    assert not a._fused_draw and b._fused_draw
    assert np.array_equal(ap.run_draws(a, 3)[0], ap.run_draws(b, 3)[0])
    assert "hmc_draw_gaussian_precond" not in oa.calls and ob.calls["hmc_draw_gaussian_precond"] == 3
    # later: two draws on the whole-draw kernel, then the preconditioner
    a, b = mk(_NoPrecondDraw, oa), mk(bk.DiagGaussian, ob)
    assert a._fused_draw
    ap.run_draws(a, 2), ap.run_draws(b, 2)
    a.set_precond_diag(v), b.set_precond_diag(v)
    assert not a._fused_draw and b._fused_draw
    ta, la = ap.run_draws(a, 3)
    tb, lb = ap.run_draws(b, 3)
    assert np.array_equal(ta, tb) and np.array_equal(la, lb) and np.array_equal(a.rng_state(), b.rng_state())
    # a checkpoint with a preconditioner into a sampler on the whole-draw kernel
    c = mk(_NoPrecondDraw, AdaptFakeOps())
    c.load_state_dict(b.state_dict())
    assert not c._fused_draw
    assert np.array_equal(ap.run_draws(c, 2)[0], ap.run_draws(b, 2)[0])


# ---- statistics ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [0, 1, 63, 64, 65, 700])
def test_accept_stat_restatement_against_the_plain_formula(C):
    lp0, a0, lp1, a1 = ap.accept_stat_inputs(C)
    s, n = accept_stat_ref(lp0, a0, lp1, a1)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (lp1 - a1) - (lp0 - a0)
        want = np.where(np.isnan(d), 0.0, np.minimum(1.0, np.exp(np.minimum(0.0, d))))
    assert n == float(np.isnan(d).sum())
    assert abs(s - want.sum()) <= 1e-12 * max(1.0, want.sum())
    if C >= 8:
        assert n >= 2.0
    ops = AdaptFakeOps()
    out = torch.full((2,), -1.0, dtype=torch.float64)
    ops.accept_stat(*(torch.from_numpy(x) for x in (lp0, a0, lp1, a1)), out)
    assert out[0].item() == s and out[1].item() == n


def test_accept_stat_argument_errors_without_a_gpu():
    """bk_accept_stat decides BK_E_ARG before any HIP call (as tests/test_abi.py checks for its neighbours); an empty
    problem launches the combine alone (out = {0, 0}), which needs a device: tests/test_gpu_adapt.py."""
    from bayes_kit_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    E_ARG = -1
    assert lib.bk_accept_stat(None, p, p, p, 4, p, p, None) == E_ARG
    assert lib.bk_accept_stat(p, p, None, p, 4, p, p, None) == E_ARG
    assert lib.bk_accept_stat(p, p, p, p, 4, None, p, None) == E_ARG
    assert lib.bk_accept_stat(p, p, p, p, 4, p, None, None) == E_ARG   # scratch required
    assert lib.bk_accept_stat(p, p, p, p, -1, p, p, None) == E_ARG
    assert lib.bk_precond_pack(None, p, 4, None) == E_ARG and lib.bk_precond_pack(p, None, 4, None) == E_ARG
    assert lib.bk_precond_pack(p, p, -1, None) == E_ARG and lib.bk_precond_pack(p, p, 0, None) == 0
    assert lib.bk_momentum_refresh_precond(0, p, 4, p, 4, None, p, 4, 8, None, 0, None) == E_ARG   # precond required
    assert lib.bk_momentum_refresh_precond(0, p, 4, p, 4, p, None, 4, 8, None, 0, None) == E_ARG   # kin_out required
    assert lib.bk_momentum_refresh_precond(0, p, 0, p, 0, p, p, 0, 8, None, 0, None) == 0          # no chains
    assert lib.bk_leapfrog_finish_precond(p, None, 4, p, 4, 1, None, 0.1, 0, p, 4, 8, None) == E_ARG
    assert lib.bk_leapfrog_finish_precond(p, None, 0, p, 0, 1, p, 0.1, 0, p, 0, 8, None) == 0
    assert lib.bk_hmc_draw_gaussian_precond(p, p, 4, p, None, 0, p, None, 0.1, 3, p, p, p, p, None, None, None, None, None,
                                            4, 8, None) == E_ARG
    assert lib.bk_hmc_draw_gaussian_precond(p, p, 0, p, None, 0, p, p, 0.1, 3, p, p, p, p, None, None, None, None, None,
                                            0, 8, None) == 0


def test_pooled_variance_and_reset():
    ap.check_pooled_variance(AdaptFakeOps())


# ---- the host controller -------------------------------------------------------------------------------------------
def test_window_schedule_table():
    table = {
        10: (0, 10, []),
        19: (0, 19, []),
        20: (3, 2, [18]),
        100: (15, 10, [90]),
        150: (75, 50, [100]),
        300: (75, 50, [100, 150, 250]),
        1000: (75, 50, [100, 150, 250, 450, 950]),
    }
    for draws, want in table.items():
        assert warmup_windows(draws) == want, draws


def test_dual_averaging_reproduces_a_literal_sequence():
    """eps0 = 0.1, target 0.8, alpha = 1.0, 0.5, 0.9, 0.2: the formulas of the issue by hand --
    t = 1: eta = 1/11, Hbar = -0.2/11, x = log(1) + (1/0.05) * 0.2/11 = 4/11; ..."""
    da = DualAveraging(0.1, 0.8)
    got = [da.step(a) for a in (1.0, 0.5, 0.9, 0.2)]
    mu, g = math.log(1.0), 0.05
    h1 = (1 - 1 / 11) * 0.0 + (1 / 11) * (0.8 - 1.0)
    h2 = (1 - 1 / 12) * h1 + (1 / 12) * (0.8 - 0.5)
    h3 = (1 - 1 / 13) * h2 + (1 / 13) * (0.8 - 0.9)
    h4 = (1 - 1 / 14) * h3 + (1 / 14) * (0.8 - 0.2)
    xs = [mu - math.sqrt(t) / g * h for t, h in ((1, h1), (2, h2), (3, h3), (4, h4))]
    assert got == [math.exp(x) for x in xs]
    literal = [1.4385510095776777, 0.7900158579283462, 0.9999999999999998, 0.18009231214795227]
    np.testing.assert_allclose(got, literal, rtol=1e-14)
    xbar = 0.0
    for t, x in enumerate(xs, 1):
        w = t ** -0.75
        xbar = w * x + (1 - w) * xbar
    assert da.final() == math.exp(xbar)
    da.restart(da.final())
    assert (da.t, da.hbar, da.xbar) == (0, 0.0, 0.0) and da.mu == math.log(10 * math.exp(xbar))


# ---- warmup end to end ----------------------------------------------------------------------------------------------
def test_warmup_end_to_end_on_the_stand_in():
    """lam = logspace(0, 4, 32), 512 chains, eps0 = 0.006, L = 16, warmup(300).  Observed here (seed 11):
    max|v lam - 1| = 0.040, eps = 0.654, mean alpha of the last 20 draws 0.788 -- inside the conditions, the first two just
    outside the prototype's eight-seed ranges [0.021-0.036] and [0.66-0.74] (another random stream)."""
    s, rep, lam = ap.run_warmup(AdaptFakeOps(), 11)
    ap.check_warmup_report(rep, lam)
    assert s._stepsize == rep["stepsize"] and isinstance(s._stepsize, float)
    assert np.array_equal(s.precond_diag, rep["precond_diag"])
    th, lp = s.sample()  # ... and samples on with the adapted values
    assert np.isfinite(np.asarray(th)).all()


def test_warmup_is_reproducible_and_path_independent():
    reps, after = [], []
    for path in ("auto", "auto", "step", "opaque"):
        s, rep, _ = ap.run_warmup(AdaptFakeOps(), 3, path=path, draws=60, C=96)
        reps.append(rep)
        after.append(ap.run_draws(s, 2)[0])
    assert reps[0]["window_ends"] == [54] and reps[0]["stepsize"] > 0.006
    for rep, th in zip(reps[1:], after[1:]):
        assert ap.reports_equal(reps[0], rep)
        assert np.array_equal(after[0], th)


def test_warmup_step_size_only():
    ops = AdaptFakeOps()
    s = bk.HMCDiag(bk.DiagGaussian(np.array([1.0, 4.0, 0.25]), ops=ops), 0.01, 4, chains=64, seed=1, ops=ops)
    rep = s.warmup(15)  # fewer than 20 draws: no window
    assert rep["window_ends"] == [] and rep["precond_diag"] is None and rep["stepsize"] > 0.01
    m = bk.HMCDiag(bk.DiagGaussian(np.array([1.0, 4.0, 0.25]), ops=ops), 0.01, 4, np.ones(3), chains=64, seed=1, ops=ops)
    rep2 = m.warmup(15, adapt_metric=False)  # metric_diag keeps its meaning; the step size adapts
    assert rep2["precond_diag"] is None and rep2["eps"] == rep["eps"]


@pytest.mark.parametrize("case", ap.WARMUP_CASES)
def test_warmup_is_the_recorded_run(case):
    """Every kind of warmup on the stand-ins against its record (tests/golden/hmc_warmup_standin.json): the whole report,
    its keys in their order, the two draws that follow and the stream position after them, all with ==."""
    rec, want = ap.warmup_record(case), ap.golden_record(case)
    assert list(rec) == list(want)
    assert rec == want


# ---- refusals -------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument():
    ops = AdaptFakeOps()
    lam = np.array([1.0, 2.0, 3.0])

    def make(**kw):
        return bk.HMCDiag(bk.DiagGaussian(lam, ops=ops), 0.1, 3, kw.pop("metric_diag", None), chains=4, seed=1, ops=ops, **kw)

    with pytest.raises(ValueError, match="precond_diag.*metric_diag"):
        make(metric_diag=np.ones(3), precond_diag=np.ones(3))
    with pytest.raises(ValueError, match="precond_diag.*metric_dense"):
        make(metric_dense=np.eye(3), precond_diag=np.ones(3))
    with pytest.raises(ValueError, match="precond_diag has 2 entries"):
        make(precond_diag=np.ones(2))
    for bad in ([1.0, 0.0, 1.0], [1.0, -2.0, 1.0], [1.0, np.nan, 1.0], [1.0, np.inf, 1.0]):
        with pytest.raises(ValueError, match="precond_diag must hold finite, positive"):
            make(precond_diag=np.array(bad))
    with pytest.raises(ValueError, match="precond_diag"):
        make(metric_diag=np.ones(3)).set_precond_diag(np.ones(3))
    with pytest.raises(ValueError, match="precond_diag"):
        make(precond_diag=np.ones(3))._metric = np.ones(3)
    with pytest.raises(ValueError, match="adapt_metric"):
        make(metric_diag=np.ones(3)).warmup(30)
    with pytest.raises(ValueError, match="adapt_metric"):
        make(metric_dense=np.eye(3)).warmup(30)
    with pytest.raises(ValueError, match="draws"):
        make().warmup(0)
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="target_accept"):
            make().warmup(10, target_accept=bad)


# ---- two ranks ------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_rank_warmup_agrees_with_one_process():
    """Two gloo ranks x 256 chains against one process x 512.  Both ranks report identical eps and v (bit for bit: they
    see the same gathered sums in rank order), and the first draw's statistic agrees with the one-process run to rel 1e-12
    (another grouping of the same sum).

    The final v was expected to agree to 1e-6 "unless it does not hold: then record the observed value and the reason".
    It does not hold.  Observed: final v rel 3.0e-2, eps 0.6473 (two ranks) against 0.6751 (one process).  Reason: dual
    averaging is not a contraction -- after every restart it swings the step size across the stability limit and back, a
    map that amplifies a difference by about 1e4 per eight draws (measured on the stand-in: a one-ulp change of sqrt(v) in
    two dimensions gives 4e-12 in alpha after 10 draws, 4e-8 after 18, 1e-2 after 26).  The two groupings of the pooled
    variance differ in the last bits of the first v, and 200 draws later the two runs are two different, equally valid,
    adaptations.  (With np.sum in place of the device's tree the two groupings happened to give the same doubles and the
    1e-6 held, by luck.)  What can be asserted is what both runs must satisfy: each v within 10 % of 1 / lam (the
    end-to-end condition), hence within 1.1 / 0.9 - 1 of each other, and step sizes that both pass that condition."""
    port = _free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "adapt_dist_worker.py")], env=env,
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
    assert reps[0] == reps[1]
    _, one, lam = ap.run_warmup(AdaptFakeOps(), 21)
    a2, a1 = reps[0]["alpha"][0], one["alpha"][0]
    assert abs(a2 - a1) <= 1e-12 * abs(a1)
    v2, v1 = np.array(reps[0]["precond_diag"]), one["precond_diag"]
    rel = float(np.abs(v2 / v1 - 1.0).max())
    first = next((i for i, (x, y) in enumerate(zip(reps[0]["alpha"], one["alpha"])) if x != y), None)
    print(f"two ranks vs one process: first different alpha at draw {first}; final v rel {rel:.3e}, "
          f"eps {reps[0]['stepsize']!r} vs {one['stepsize']!r}")
    assert first is None or first >= reps[0]["window_ends"][0]  # (one 512-chain tree = the two ranks' trees added)
    two = dict(reps[0], precond_diag=v2)
    ap.check_warmup_report(two, lam)
    ap.check_warmup_report(one, lam)
    assert rel <= 1.1 / 0.9 - 1.0
