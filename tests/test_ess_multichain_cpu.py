"""Multi-chain bulk / tail / mean ESS and MCSE of the mean (no GPU): the estimator's known answers on the NumPy
restatement, the Geyer scan's branches, the library's host logic through a FakeOps subclass, input validation, the
quantile threshold, and two gloo ranks."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import bayes_kit_amd as bk
from bayes_kit_amd import diagnostics as dg
from tests import multichain_ess_ref as ref

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _ratio(x):
    n = x.shape[0] // 2
    e, max_t = ref.ess_split_chains(ref.split(x))
    return e / (2 * x.shape[1] * n), max_t


# ---- known answers of the estimator (restatement) ---------------------------------------------------------------------
def test_known_answers_2048_chains_of_1000():
    rng = np.random.default_rng(11)
    r, _ = _ratio(ref.ar1(rng, 1000, 2048, 0.0))
    assert 0.95 <= r <= 1.05
    r, _ = _ratio(ref.ar1(rng, 1000, 2048, 0.5))
    assert abs(r / (0.5 / 1.5) - 1) < 0.05
    off = np.where(np.arange(2048) % 2 == 0, 0.0, 5.0)
    x = ref.ar1(rng, 1000, 2048, 0.0, offset=off)
    r, max_t = _ratio(x)
    assert r < 0.01 and max_t == 500 - 4


def test_known_answer_phi_09_long_chains():
    rng = np.random.default_rng(12)
    r, _ = _ratio(ref.ar1(rng, 4000, 512, 0.9))
    assert abs(r / (0.1 / 1.9) - 1) < 0.10


# ---- the scan's branches through the library's _geyer_tau -------------------------------------------------------------
def _scan_inputs(x):
    ch = ref.split(x)
    n, M = ch.shape
    g = ref.autocov(ch)
    W = np.mean(g[0]) * n / (n - 1)
    vp = W * (n - 1) / n + np.var(ch.mean(axis=0), ddof=1)
    return g.mean(axis=1), W, vp, M, n


def test_geyer_tau_antithetic_floor():
    x = ref.ar1(np.random.default_rng(3), 1000, 64, -0.9)
    G, W, vp, M, n = _scan_inputs(x)
    tau, _ = dg._geyer_tau(G, W, vp, M, n)
    assert tau == 1 / np.log10(M * n)
    e = bk.ess_mean(torch.from_numpy(x), ops=ref.MultiEssFakeOps())
    assert e == M * n / (1 / np.log10(M * n))
    assert e == pytest.approx(M * n * np.log10(M * n), rel=1e-15)


@pytest.mark.parametrize("N", [8, 9])
def test_geyer_tau_shortest_chains_give_the_floor(N):
    x = ref.ar1(np.random.default_rng(N), N, 6, 0.3)
    G, W, vp, M, n = _scan_inputs(x)
    assert n == 4
    tau, max_t = dg._geyer_tau(G, W, vp, M, n)
    assert max_t == 0 and tau == 1 / np.log10(M * n)
    assert bk.ess_mean(torch.from_numpy(x), ops=ref.MultiEssFakeOps()) == M * n / tau


def test_geyer_tau_hand_built_sequences():
    n, M, W, vp = 20, 8, 1.0, 1.0
    # rho(t) = 1 - (W - Gamma_t) / var_plus = Gamma_t: slowly decaying, positive -> the scan reaches its bound
    G = np.linspace(1.0, 0.5, n)
    tau, max_t = dg._geyer_tau(G, W, vp, M, n)
    assert max_t == n - 4
    assert (tau, max_t) == ref.scan(G, W, vp, M, n)
    # a NaN ends the scan at its pair
    G2 = G.copy()
    G2[6] = np.nan
    tau2, max_t2 = dg._geyer_tau(G2, W, vp, M, n)
    assert max_t2 == 6 and np.isfinite(tau2)
    assert (tau2, max_t2) == ref.scan(G2, W, vp, M, n)
    # too few lags for the scan: asks for more
    assert dg._geyer_tau(G[:5], W, vp, M, n) is None


# ---- the library (host logic + FakeOps) against the restatement --------------------------------------------------------
FUNCS = ["ess_bulk", "ess_tail", "ess_mean", "mcse_mean"]


@pytest.mark.parametrize("N", [40, 41, 300])
@pytest.mark.parametrize("as_list", [False, True])
def test_library_equals_restatement(N, as_list):
    rng = np.random.default_rng(N)
    x = ref.ar1(rng, N, 7, 0.8)
    inp = [x[:, c] for c in range(x.shape[1])] if as_list else torch.from_numpy(x)
    ops = ref.MultiEssFakeOps()
    for f in FUNCS:
        assert getattr(bk, f)(inp, ops=ops) == pytest.approx(getattr(ref, f)(x), rel=1e-12), f
    assert bk.ess_quantile(inp, 0.37, ops=ops) == pytest.approx(ref.ess_quantile(x, 0.37), rel=1e-12)


def test_library_long_half_route_equals_restatement_and_constant_chain():
    rng = np.random.default_rng(5)
    x = ref.ar1(rng, 120, 5, 0.6)
    x[:, 2] = 1.5  # a stuck chain: gamma = 0 on both routes, its 0/0 autocorrelation never reaches Gamma
    t = torch.from_numpy(x)
    fft, lds = ref.MultiEssFakeOps(max_half=10), ref.MultiEssFakeOps()
    for f in ["ess_mean", "ess_tail", "ess_bulk"]:
        a, b = getattr(bk, f)(t, ops=fft), getattr(bk, f)(t, ops=lds)
        assert np.isfinite(a) and a == pytest.approx(b, rel=1e-12) and a == pytest.approx(getattr(ref, f)(x), rel=1e-12)
    assert fft.calls.get("ess_acov_sums") and not fft.calls.get("ess_lag_sums")


def test_lag_rounds_double_until_the_scan_stops():
    x = ref.ar1(np.random.default_rng(9), 1000, 8, 0.99)
    ops = ref.MultiEssFakeOps()
    bk.ess_mean(torch.from_numpy(x), ops=ops)
    assert ops.calls["ess_lag_sums"] >= 3  # 64, 128, 256, ... lags


def test_summary_matches_standalone_functions():
    x = ref.ar1(np.random.default_rng(2), 60, 6, 0.5)
    ops = ref.MultiEssFakeOps()
    rec = bk.DrawRecorder([0], 60, 6, with_logp=False, ops=ops)
    rec.series[0].copy_(torch.from_numpy(x))
    rec.n = 60
    s = rec.summary()
    assert s["name"] == ["theta[0]"]
    v = rec.view(0)
    assert s["ess_bulk"][0] == bk.ess_bulk(v, ops=ops)
    assert s["ess_tail"][0] == bk.ess_tail(v, ops=ops)
    assert s["mcse_mean"][0] == bk.mcse_mean(v, ops=ops)
    assert s["rhat"][0] == bk.rank_normalized_rhat(v, ops=ops)
    assert s["mean"][0] == pytest.approx(x.mean(), rel=1e-12)
    assert s["sd"][0] == pytest.approx(np.std(x, ddof=1), rel=1e-12)


# ---- validation and NaN ------------------------------------------------------------------------------------------------
def test_validation_errors():
    ops = ref.MultiEssFakeOps()
    with pytest.raises(ValueError, match=r"\[10, 11\]"):
        bk.ess_bulk([np.zeros(10), np.zeros(11)], ops=ops)
    for f in FUNCS:
        with pytest.raises(ValueError, match="8 draws"):
            getattr(bk, f)(torch.zeros((7, 4), dtype=torch.float64), ops=ops)
    for p in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="prob"):
            bk.ess_quantile(torch.zeros((20, 4), dtype=torch.float64), p, ops=ops)


def test_nan_cases():
    ops = ref.MultiEssFakeOps()
    rng = np.random.default_rng(4)
    x = rng.standard_normal((30, 4))
    for bad in (np.nan, np.inf):
        y = x.copy()
        y[3, 1] = bad
        for f in FUNCS + ["ess_quantile"]:
            args = (0.5,) if f == "ess_quantile" else ()
            assert np.isnan(getattr(bk, f)(torch.from_numpy(y), *args, ops=ops)), (f, bad)
    # var_plus == 0: constant draws, and an indicator that is all 1 (every draw equal to the quantile)
    const = torch.full((30, 4), 2.0, dtype=torch.float64)
    for f in ["ess_mean", "mcse_mean", "ess_tail"]:
        assert np.isnan(getattr(bk, f)(const, ops=ops)), f
    assert np.isnan(bk.ess_quantile(const, 0.5, ops=ops))


def test_tail_is_nan_when_one_quantile_indicator_is_degenerate():
    # 10 % of the draws tie at the maximum: the 0.95 quantile is that maximum and its indicator is all 1 (var_plus = 0),
    # while the 0.05 indicator is an ordinary one: the minimum of the two is NaN (Python's min(finite, nan) is finite)
    ops = ref.MultiEssFakeOps()
    x = np.random.default_rng(6).standard_normal((40, 6))
    x[::10] = 9.0
    t = torch.from_numpy(x)
    assert np.isfinite(bk.ess_quantile(t, 0.05, ops=ops)) and np.isnan(bk.ess_quantile(t, 0.95, ops=ops))
    assert np.isnan(bk.ess_tail(t, ops=ops)) and np.isnan(ref.ess_tail(x))
    rec = bk.DrawRecorder([0], 40, 6, with_logp=False, ops=ops)
    rec.series[0].copy_(t)
    rec.n = 40
    assert np.isnan(rec.summary()["ess_tail"][0])


# ---- the quantile threshold is np.quantile bit for bit ------------------------------------------------------------------
def test_quantile_threshold_bit_identical():
    rng = np.random.default_rng(8)
    datas = [rng.standard_normal(1001), np.round(rng.standard_normal(2000), 1), rng.integers(0, 5, 77).astype(float),
             rng.standard_normal(21), np.arange(101.0)]
    probs = [0.05, 0.95, 0.5, 0.25, 0.1, 0.3, 0.7, 0.123456789, 1e-9, 1 - 1e-9]
    for d in datas:
        srt = np.sort(d)
        for p in probs:
            got = dg._split_quantiles(lambda idx: srt[idx], d.size, [p])[0]
            want = np.quantile(d, p)
            assert np.float64(got).tobytes() == np.float64(want).tobytes(), (d.size, p)
    # probabilities that land exactly on an order statistic (S - 1 = 100: p = k / 100 for some k)
    d = rng.standard_normal(101)
    srt = np.sort(d)
    for k in (5, 25, 50, 95):
        p = k / 100
        assert dg._split_quantiles(lambda idx: srt[idx], 101, [p])[0] == np.quantile(d, p)


# ---- two gloo ranks -----------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _run_two_ranks(mode):
    port = _free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "ess_multichain_worker.py"), mode],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=240)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(out)
    for rank, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, out
        assert f"rank {rank} ok" in out, out


def test_two_gloo_ranks_equal_one_process():
    _run_two_ranks("values")


def test_two_gloo_ranks_mismatched_draws_raise_on_both():
    _run_two_ranks("mismatch")
