"""The jittered trajectory length, the trajectory statistic and HMCDiag.warmup(adapt_trajectory=True) without a GPU: the host
controller alone, the sampler's host logic on the NumPy stand-in (tests/fake_ops_chees.py), argument checks of the C ABI, and
two gloo ranks."""
import ctypes
import hashlib
import json
import math
import os
import socket
import subprocess
import sys
from unittest import mock

import numpy as np
import pytest
import torch

import bayes_kit_amd as bk
from bayes_kit_amd.adapt import TrajectoryAdam, jitter_steps, radical_inverse2
from tests import adapt_parity as ap
from tests import chees_parity as cp
from tests.fake_ops_adapt import AdaptFakeOps
from tests.fake_ops_chees import CheesFakeOps, chees_stat_ref, chees_sums_ref

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


# ---- jitter ---------------------------------------------------------------------------------------------------------
def test_radical_inverse_and_the_clamps_of_the_step_count():
    assert [radical_inverse2(n) for n in range(1, 9)] == [0.5, 0.25, 0.75, 0.125, 0.625, 0.375, 0.875, 0.0625]
    assert jitter_steps(1, 2.0, 0.1, 1024) == 10 and jitter_steps(3, 2.0, 0.1, 1024) == 15
    assert jitter_steps(2, 2.0, 0.3, 1024) == 2        # ceil(0.5 / 0.3)
    assert jitter_steps(8, 0.1, 0.5, 1024) == 1        # clamps at 1
    assert jitter_steps(3, 100.0, 0.01, 1024) == 1024  # ... and at max_steps
    assert jitter_steps(3, 100.0, 0.01, 7) == 7
    ops = CheesFakeOps()
    s = bk.HMCDiag(bk.IsoGaussian(3, ops=ops), 0.1, 5, chains=4, seed=1, trajectory_length=2.0, max_steps=12, ops=ops)
    assert s.trajectory_length == 2.0 and s.max_steps == 12 and s.last_steps is None
    got = []
    for _ in range(4):
        s.sample()
        got.append((s.last_steps, s._steps))
    assert got == [(10, 10), (5, 5), (12, 12), (3, 3)]
    s.set_trajectory_length(None)  # back to the fixed steps
    s.sample()
    assert s.trajectory_length is None and s.last_steps == 5 and s._jitter_n == 4
    s.set_trajectory_length(1.0)
    s.sample()
    assert s.last_steps == jitter_steps(5, 1.0, 0.1, 12) == 7


@pytest.mark.parametrize("path", ap.PATHS)
def test_jittered_draws_equal_the_oracle_with_the_same_step_counts(path):
    cp.check_jitter_vs_oracle(CheesFakeOps(), 8, 6, path)
    cp.check_jitter_vs_oracle(CheesFakeOps(), 6, 40, path)  # (D >= 32: chain-major normals on the whole-draw path)
    cp.check_jitter_vs_oracle(CheesFakeOps(), 4, 6, path, T=2.0, max_steps=9)  # (the upper clamp in use)


def test_jittered_draws_do_not_depend_on_the_path_and_consume_no_randomness():
    cp.check_jitter_paths_agree(CheesFakeOps(), 6, 6, [dict()])
    cp.check_jitter_paths_agree(CheesFakeOps(), 5, 40, [dict()])


@pytest.mark.parametrize("path", ap.PATHS)
def test_checkpoint_carries_trajectory_length_and_the_jitter_counter(path):
    cp.check_checkpoint(CheesFakeOps(), 6, 6, path)
    cp.check_checkpoint(CheesFakeOps(), 6, 36, path)


# ---- the statistic --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,D", cp.SHAPES)
def test_statistic_restatements_against_the_plain_formula(C, D):
    x = cp.chees_inputs(C, D)
    sums, w = cp.chees_plain(x)
    got = chees_sums_ref(x["theta"], x["theta_p"])
    fin = np.isfinite(sums)
    np.testing.assert_allclose(got[fin], sums[fin], rtol=1e-12, atol=1e-12 * np.abs(x["theta"]).sum(axis=1).max())
    assert np.array_equal(got[~fin], sums[~fin])  # (the planted inf: the same inf)
    mean = cp.finite_mean(x)
    s, n = chees_stat_ref(x["theta"], x["theta_p"], x["rho_p"], mean, x["lp_cur"], x["a_cur"], x["lp_prop"], x["a_prop"])
    want_s, want_n, g = cp.chees_plain_stat(x, mean, w)
    scale = float(np.abs(w * np.where(np.isfinite(g), g, 0.0)).sum())
    assert math.isfinite(s) and abs(s - want_s) <= 1e-12 * max(scale, 1e-300)
    assert n == want_n
    pl = x["planted"]
    if pl:
        assert w[pl["nan"]] == 0.0 and w[pl["zero_weight_inf"]] == 0.0 and not np.isfinite(g[pl["zero_weight_inf"]])
        assert w[pl["inf_g"]] > 0.0 and np.isinf(g[pl["inf_g"]]) and n == 1.0
    else:
        assert n == 0.0
    # ... and through the ops layer of the stand-in, with and without the kinetic energies
    ops = CheesFakeOps()
    so, out = cp.run_chees_ops(ops, x, mean)
    assert np.array_equal(so, got) and out[0] == s and out[1] == n
    out2 = torch.empty(2, dtype=torch.float64)
    t = lambda k: torch.from_numpy(x[k])  # noqa: E731
    ops.chees_stat(t("theta"), t("theta_p"), t("rho_p"), torch.from_numpy(mean), t("lp_cur"), None, t("lp_prop"), None, out2)
    s0, n0 = chees_stat_ref(x["theta"], x["theta_p"], x["rho_p"], mean, x["lp_cur"], None, x["lp_prop"], None)
    assert out2[0].item() == s0 and out2[1].item() == n0


def test_chees_entry_points_decide_argument_errors_without_a_gpu():
    from bayes_kit_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_double * 256)()
    p = ctypes.addressof(buf)
    E_ARG, E_ALIGN = -1, -2
    assert lib.bk_chees_sums(None, 4, p, 4, p, 4, 2, None) == E_ARG
    assert lib.bk_chees_sums(p, 4, None, 4, p, 4, 2, None) == E_ARG
    assert lib.bk_chees_sums(p, 4, p, 4, None, 4, 2, None) == E_ARG
    assert lib.bk_chees_sums(p, 4, p, 4, p, -1, 2, None) == E_ARG
    assert lib.bk_chees_sums(p, 4, p, 4, p, 4, -2, None) == E_ARG
    assert lib.bk_chees_sums(p, 4, p, 4, p, 4, 0, None) == 0          # no dimensions
    assert lib.bk_chees_sums(p, 3, p, 4, p, 4, 2, None) == E_ALIGN
    assert lib.bk_chees_sums(p, 4, p, 3, p, 4, 2, None) == E_ALIGN
    ok = (p, 4, p, 4, p, 4, p, p, p, p, p, p, p, 4, 2, None)

    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.bk_chees_stat(*a)

    for i in (0, 2, 4, 6, 7, 9, 11, 12):  # theta, theta_p, rho_p, mean, lp_cur, lp_prop, out, work
        assert call(**{f"a{i}": None}) == E_ARG, i
    assert call(a13=-1) == E_ARG and call(a14=-1) == E_ARG
    for i in (1, 3, 5):
        assert call(**{f"a{i}": 3}) == E_ALIGN, i


# ---- the controller -------------------------------------------------------------------------------------------------
def test_trajectory_adam_reproduces_a_sequence_computed_by_hand():
    """T0 = 0.5, eps = 0.1, max_steps = 1024; draws (S_wg, S_w, t) = (6, 3, 0.5), (-2, 4, 0.25), (1, 2, 0.75)."""
    ta = TrajectoryAdam(0.5)
    x0 = math.log(0.5)
    assert (ta.x, ta.v, ta.k, ta.xbar) == (x0, 0.0, 0, 0.0) and ta.final() == 0.5
    got = [ta.step(6.0, 3.0, 0.5, 0.1, 1024), ta.step(-2.0, 4.0, 0.25, 0.1, 1024), ta.step(1.0, 2.0, 0.75, 0.1, 1024)]
    g1, g2, g3 = 0.5 * 6.0 / 3.0, 0.25 * -2.0 / 4.0, 0.75 * 1.0 / 2.0
    v1 = 0.95 * 0.0 + 0.05 * g1 * g1
    x1 = x0 + 0.025 * g1 / (math.sqrt(v1 / (1 - 0.95)) + 1e-8)           # = x0 + 0.025 (first Adam step: g / |g|)
    v2 = 0.95 * v1 + 0.05 * g2 * g2
    x2 = x1 + 0.025 * g2 / (math.sqrt(v2 / (1 - 0.95 ** 2)) + 1e-8)
    v3 = 0.95 * v2 + 0.05 * g3 * g3
    x3 = x2 + 0.025 * g3 / (math.sqrt(v3 / (1 - 0.95 ** 3)) + 1e-8)
    assert got == [math.exp(x1), math.exp(x2), math.exp(x3)]
    np.testing.assert_allclose(x1 - x0, 0.025, rtol=1e-6)
    np.testing.assert_allclose(got, [0.5126575601340501, 0.5103859882628836, 0.5183035861700189], rtol=1e-14)
    xb = 0.0
    for k, x in enumerate((x1, x2, x3), 1):
        xb = k ** -0.75 * x + (1 - k ** -0.75) * xb
    assert ta.final() == math.exp(xb) and ta.k == 3
    # a draw without weight or with a non-finite sum is skipped
    before = (ta.x, ta.v, ta.k, ta.xbar)
    for bad in ((1.0, 0.0), (float("nan"), 2.0), (float("inf"), 2.0), (1.0, -1.0)):
        assert ta.step(bad[0], bad[1], 0.5, 0.1, 1024) == math.exp(x3)
    assert (ta.x, ta.v, ta.k, ta.xbar) == before
    # restart keeps x and clears the rest; final() is exp(x) until the next update
    ta.restart()
    assert (ta.x, ta.v, ta.k, ta.xbar) == (x3, 0.0, 0, 0.0) and ta.final() == math.exp(x3)
    # the clip: x stays inside [log eps, log(eps max_steps)]
    hi = TrajectoryAdam(0.79)
    assert hi.step(5.0, 1.0, 1.0, 0.1, 8) == math.exp(math.log(0.1 * 8)) and hi.x == math.log(0.1 * 8)
    lo = TrajectoryAdam(0.101)
    assert lo.step(-5.0, 1.0, 1.0, 0.1, 8) == math.exp(math.log(0.1)) and lo.x == math.log(0.1)


# ---- warmup end to end ------------------------------------------------------------------------------------------------
_ISO = {}


def _iso_run():
    """IsoGaussian(32), 512 chains, eps0 = 0.006, steps = 16, warmup(300, adapt_metric=False, adapt_trajectory=True), seed
    21, on the default path -- shared by the end-to-end and the two-rank test."""
    if not _ISO:
        ops = CheesFakeOps()
        s, rep = cp.run_chees_warmup(ops, bk.IsoGaussian(32, ops=ops), 21)
        _ISO.update(s=s, rep=rep, ops=ops)
    return _ISO


def test_warmup_finds_the_trajectory_length_of_a_unit_gaussian():
    """For a unit Gaussian ChEES(t) = D sin^2 t; with uniform jitter its mean is maximal where tan 2T = 2T, T = 2.247 as
    eps -> 0, pulled down by about eps by the ceil: the band [1.6, 2.4] (a NumPy prototype of the recipe: 1.87-1.93).
    Observed here (seed 21): see the printed line."""
    r = _iso_run()
    s, rep, ops = r["s"], r["rep"], r["ops"]
    cp.check_chees_report(rep)
    assert rep["T"][0] == 16 * 0.006 and rep["steps"][0] == jitter_steps(1, 16 * 0.006, 0.006, 1024) == 8
    assert s.trajectory_length == rep["trajectory_length"] and s._stepsize == rep["stepsize"]
    assert rep["window_ends"] == [] and rep["precond_diag"] is None
    # one host read per draw: the two outputs travelled with the acceptance statistic
    assert ops.calls["chees_sums"] == 300 and ops.calls["chees_stat"] == 300 and ops.calls["accept_stat"] == 300
    # sampling goes on jittered, on the whole-draw kernel again
    assert s._fused_draw and "hmc_draw_gaussian" not in ops.calls
    cp.check_pooled_variance_after(s)
    assert ops.calls["hmc_draw_gaussian"] == 100 and s._jitter_n == 400


def test_warmup_on_an_anisotropic_gaussian_without_metric_adaptation():
    """DiagGaussian(logspace(0, 2, 8)): the band again (prototype 1.99-2.05)."""
    ops = CheesFakeOps()
    s, rep = cp.run_chees_warmup(ops, bk.DiagGaussian(np.logspace(0, 2, 8), ops=ops), 21)
    cp.check_chees_report(rep, eps_min=None)


def test_warmup_report_does_not_depend_on_the_path_or_on_generating_ahead():
    lam = np.logspace(0, 1, 32)
    runs = []
    for kw in (dict(path="auto"), dict(path="auto"), dict(path="step"), dict(path="opaque"),
               dict(path="auto", prefetch_rng=False), dict(path="opaque", prefetch_rng=False)):
        ops = CheesFakeOps()
        s, rep = cp.run_chees_warmup(ops, bk.DiagGaussian(lam, ops=ops), 3, C=96, draws=60, warm=dict(), **kw)
        assert "hmc_draw_gaussian" not in ops.calls and "hmc_draw_gaussian_precond" not in ops.calls
        after = ap.run_draws(s, 5)
        if kw["path"] == "auto":  # the whole-draw kernel again (its preconditioned form: a window ended)
            assert ops.calls["hmc_draw_gaussian_precond"] == 5
        runs.append((rep, after, s.rng_state().copy()))
    assert runs[0][0]["window_ends"] == [54] and len(set(runs[0][0]["steps"])) > 1
    for rep, after, rng in runs[1:]:
        assert cp.chees_reports_equal(runs[0][0], rep)
        assert np.array_equal(after[0], runs[0][1][0]) and np.array_equal(after[1], runs[0][1][1])
        assert np.array_equal(rng, runs[0][2])


@pytest.mark.parametrize("path", ["auto", "opaque"])
def test_a_fresh_sampler_with_the_tuned_values_continues_bit_for_bit(path):
    lam = np.logspace(0, 1, 32)
    ops = CheesFakeOps()
    s, rep = cp.run_chees_warmup(ops, bk.DiagGaussian(lam, ops=ops), 4, C=48, draws=40, warm=dict(), path=path)
    sd = s.state_dict()
    want = ap.run_draws(s, 5)
    f = bk.HMCDiag(bk.DiagGaussian(lam, ops=ops), rep["stepsize"], 16, chains=48, seed=999, path=path,
                   precond_diag=rep["precond_diag"], trajectory_length=rep["trajectory_length"], ops=ops)
    f.load_state_dict(sd)
    assert f._jitter_n == 40 and f._fused_draw == s._fused_draw
    got = ap.run_draws(f, 5)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(f.rng_state(), s.rng_state())


def test_warmup_without_the_flag_is_what_it_was():
    """ap.run_warmup(seed 5, 96 chains, 300 draws) on the stand-in against the report of the commit before this feature,
    recorded there: every history bit for bit (SHA-256 of the doubles), and the report has no new keys."""
    s, rep, lam = ap.run_warmup(AdaptFakeOps(), 5, C=96)
    h = lambda a: hashlib.sha256(np.asarray(a, dtype=np.float64).tobytes()).hexdigest()  # noqa: E731
    assert sorted(rep) == ["alpha", "eps", "nan_chains", "precond_diag", "stepsize", "window_ends"]
    parent = dict(stepsize=0.6885284798713329, window_ends=[100, 150, 250], nan_chains=0, eps150=0.7064125158964891,
                  alpha299=0.9248619202129561, v31=0.00010327871286940769,
                  eps="5615032f65b84d90480a643d60d2e8b9b300c3cf627487ba4f706145773dd930",
                  alpha="b2cb7febff5ab066bdc6624595ad167a012b817bf3bbf553c4717bc535d79500",
                  v="85f870c35a65fa30ce8afb90c9df3e144560c6cf5a2bfda13751fbb69fd36f46")
    assert rep["stepsize"] == parent["stepsize"] and rep["window_ends"] == parent["window_ends"]
    assert rep["nan_chains"] == parent["nan_chains"]
    assert rep["eps"][150] == parent["eps150"] and rep["alpha"][299] == parent["alpha299"]
    assert rep["precond_diag"][31] == parent["v31"]
    assert h(rep["eps"]) == parent["eps"] and h(rep["alpha"]) == parent["alpha"] and h(rep["precond_diag"]) == parent["v"]
    assert s.trajectory_length is None and s._steps == 16 and s.last_steps == 16


# ---- refusals -------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument():
    ops = CheesFakeOps()
    lam = np.array([1.0, 2.0, 3.0])

    def make(**kw):
        return bk.HMCDiag(bk.DiagGaussian(lam, ops=ops), 0.1, 3, chains=4, seed=1, ops=ops, **kw)

    with pytest.raises(ValueError, match="graph"):
        make(trajectory_length=1.0, graph=True)
    with pytest.raises(ValueError, match="graph"):
        make(graph=True).set_trajectory_length(1.0)
    with pytest.raises(ValueError, match="graph"):
        make(graph=True).warmup(10, adapt_trajectory=True)
    with pytest.raises(ValueError, match="metric_dense"):
        make(metric_dense=np.eye(3)).warmup(10, adapt_metric=False, adapt_trajectory=True)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "long"):
        with pytest.raises(ValueError, match="trajectory_length"):
            make(trajectory_length=bad)
        with pytest.raises(ValueError, match="trajectory_length"):
            make().set_trajectory_length(bad)
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match="max_steps"):
            make(max_steps=bad)
        with pytest.raises(ValueError, match="max_steps"):
            make().warmup(10, adapt_trajectory=True, max_steps=bad)
    with pytest.raises(ValueError, match="max_steps"):
        make().warmup(10, max_steps=5)  # (bounds the adapted trajectory only)
    # a reference-style single-chain model
    single = mock.Mock()
    single.dims.return_value = 3
    single.batched = False
    s = bk.HMCDiag(single, 0.1, 3, seed=1, ops=ops)
    with pytest.raises(ValueError, match="adapt_trajectory"):
        s.warmup(10, adapt_trajectory=True)
    # a graph chosen by default is switched off, not refused
    d = make()
    d._use_graph = d._graph_built = True
    d.set_trajectory_length(1.0)
    assert not d._use_graph
    d.set_trajectory_length(None)
    assert d._use_graph and d._steps == 3


def test_warmup_max_steps_bounds_every_draw():
    ops = CheesFakeOps()
    s = bk.HMCDiag(bk.IsoGaussian(4, ops=ops), 0.01, 16, chains=32, seed=2, ops=ops)
    rep = s.warmup(25, adapt_metric=False, adapt_trajectory=True, max_steps=3)
    assert max(rep["steps"]) <= 3 and s.max_steps == 3 and 3 in rep["steps"]


# ---- two ranks ------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_rank_warmup_agrees_with_one_process():
    """Two gloo ranks x 256 chains against one process x 512 (the end-to-end run above).  Both ranks report identical T and
    eps (bit for bit: they see the same gathered sums in rank order).  Against one process the sums are grouped differently
    and agree to rounding only, which the controllers amplify (as documented for eps in HMCDiag.warmup): the first draw's
    statistic agrees to rel 1e-12, and both runs satisfy the same band."""
    port = _free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "chees_dist_worker.py")], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    one = _iso_run()["rep"]  # (while the workers run)
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
    two = reps[0]
    assert two["steps"][0] == one["steps"][0] and two["T"][0] == one["T"][0]
    assert abs(two["alpha"][0] - one["alpha"][0]) <= 1e-12 * abs(one["alpha"][0])
    assert abs(two["T"][1] - one["T"][1]) <= 1e-12 * one["T"][1]
    first = next((i for i, (x, y) in enumerate(zip(two["T"], one["T"])) if x != y), None)
    print(f"two ranks vs one process: first different T at draw {first}; final T {two['trajectory_length']!r} vs "
          f"{one['trajectory_length']!r}, eps {two['stepsize']!r} vs {one['stepsize']!r}")
    cp.check_chees_report(two)
    cp.check_chees_report(one)
