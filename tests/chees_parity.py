"""Checks of the jittered trajectory length (HMCDiag(trajectory_length=T)), the trajectory statistic (bk_chees_sums,
bk_chees_stat) and HMCDiag.warmup(adapt_trajectory=True) that take the kernel library as an argument:
tests/test_chees_cpu.py runs them on the NumPy stand-in (tests/fake_ops_chees.py), tests/test_gpu_chees.py on the HIP
library."""
import math

import numpy as np
import torch

import bayes_kit_amd as bk
from bayes_kit_amd.adapt import jitter_steps
from tests.adapt_parity import PATHS, _np, run_draws
from tests.sampler_parity import LOGP_RTOL

SHAPES = [(1, 1), (63, 3), (64, 4), (65, 5), (257, 33), (700, 130)]  # (C, D)
T_BAND = (1.6, 2.4)


# ---- jitter ---------------------------------------------------------------------------------------------------------
def check_jitter_vs_oracle(ops, C, D, path, T=0.4, eps=0.05, draws=6, max_steps=1024):
    """Six jittered draws against oracle.samplers.HMCDiag with o._steps = L_n assigned before each sample(): theta bit for
    bit, the log density to the tolerance of tests/sampler_parity.py (an elementwise-gradient target)."""
    from oracle import models as om
    from oracle import samplers as osamp

    lam = np.logspace(0, 1, D)
    s = bk.HMCDiag(bk.DiagGaussian(lam, ops=ops), eps, 7, chains=C, seed=31, trajectory_length=T, max_steps=max_steps,
                   path=path, ops=ops)
    th, lp, Ls = [], [], []
    for _ in range(draws):
        t, l = s.sample()
        th.append(_np(t).copy()), lp.append(_np(l).copy()), Ls.append(s.last_steps)
    want = [jitter_steps(n, T, eps, max_steps) for n in range(1, draws + 1)]
    assert Ls == want and len(set(want)) > 1, (Ls, want)
    for c in range(0, C, max(1, C // 8)):
        o = osamp.HMCDiag(om.DiagGaussian(lam), eps, 7, seed=np.random.Philox(key=[31, c]))
        for n in range(draws):
            o._steps = want[n]
            oth, olp = o.sample()
            assert np.array_equal(th[n][c], oth), (path, c, n)
            np.testing.assert_allclose(lp[n][c], olp, rtol=LOGP_RTOL, atol=1e-12)


def check_jitter_paths_agree(ops, C, D, knobs_list, T=0.4, eps=0.05, draws=6):
    """array_equal draws across the paths, and the stream positions of a fixed-`steps` sampler after as many draws."""
    lam = np.logspace(0, 1, D)
    mk = lambda path, **kw: bk.HMCDiag(bk.DiagGaussian(lam, ops=ops), eps, 7, chains=C, seed=77, path=path, ops=ops,  # noqa: E731
                                       **kw)
    fixed = mk("opaque")
    run_draws(fixed, draws)
    ref = None
    for knobs in knobs_list:
        for path in PATHS:
            s = mk(path, trajectory_length=T, **knobs)
            th, lp = run_draws(s, draws)
            ref = (th, lp) if ref is None else ref
            assert np.array_equal(th, ref[0]) and np.array_equal(lp, ref[1]), (path, knobs)
            assert np.array_equal(s.rng_state(), fixed.rng_state()), (path, knobs)


# ---- the statistic --------------------------------------------------------------------------------------------------
def chees_inputs(C, D, seed=0):
    """State, proposal, velocity and energies with planted cases (as far as C allows): a NaN energy difference; a chain
    of weight 0 (d = -inf) whose proposal is inf -- contributes 0, not NaN; a chain with weight whose g is infinite --
    counted; an underflowing weight."""
    g = np.random.default_rng(100 * C + D + seed)
    th, thp, rho = (g.normal(size=(D, C)) * s for s in (1.0, 1.5, 0.7))
    th += 0.3
    lp0, a0, lp1, a1 = (g.normal(size=C) * s for s in (3.0, 2.0, 3.0, 2.0))
    a0, a1 = np.abs(a0), np.abs(a1)
    planted = {}
    if C >= 8:
        lp1[1] = np.nan
        planted["nan"] = 1
        lp1[2] = -np.inf
        thp[0, 2] = np.inf
        planted["zero_weight_inf"] = 2
        thp[D - 1, 4] = 1e200   # A overflows: g = inf * P
        planted["inf_g"] = 4
        lp1[5] = lp0[5] + 5.0 + (a1[5] - a0[5])  # d > 0: weight 1
    if C >= 64:
        lp1[C - 1] = -800.0  # exp underflows: weight 0
        lp0[C // 2], lp1[C // 2] = np.inf, np.inf  # inf - inf: NaN
    return dict(theta=th, theta_p=thp, rho_p=rho, lp_cur=lp0, a_cur=a0, lp_prop=lp1, a_prop=a1, planted=planted)


def chees_plain(x):
    """The plain NumPy formulas: (sums [2 D], weights [C])."""
    th, thp = x["theta"], x["theta_p"]
    with np.errstate(invalid="ignore", over="ignore"):
        sums = np.concatenate([th.sum(axis=1), thp.sum(axis=1)])
        d = (x["lp_prop"] - x["a_prop"]) - (x["lp_cur"] - x["a_cur"])
        w = np.where(np.isnan(d), 0.0, np.minimum(1.0, np.exp(np.minimum(0.0, d))))
    return sums, w


def chees_plain_stat(x, mean, w):
    th, thp, rho = x["theta"], x["theta_p"], x["rho_p"]
    D = th.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        dp, dc = thp - mean[D:, None], th - mean[:D, None]
        g = ((dp * dp).sum(axis=0) - (dc * dc).sum(axis=0)) * (dp * rho).sum(axis=0)
    ok = (w > 0.0) & np.isfinite(g)
    return float((w[ok] * g[ok]).sum()), float(((w > 0.0) & ~np.isfinite(g)).sum()), g


def finite_mean(x):
    """Means for the statistic that do not depend on the planted inf (which would make every chain's dp NaN): the sums
    of the chains whose proposal is finite, divided by C."""
    th, thp = x["theta"], x["theta_p"]
    C = th.shape[1]
    cols = np.isfinite(thp).all(axis=0) & (np.abs(thp) < 1e100).all(axis=0)
    return np.concatenate([th.sum(axis=1), thp[:, cols].sum(axis=1)]) / float(C)


def run_chees_ops(ops, x, mean, ld=None):
    """The two ops calls on `ops`' device -> (sums [2 D], out [2]); ld: a row pitch > C for all three arrays."""
    dev = ops.device
    D, C = x["theta"].shape

    def put(a):
        if ld is None:
            return torch.from_numpy(a).to(dev)
        buf = torch.full((D, ld), float("nan"), dtype=torch.float64, device=dev)
        buf[:, :C] = torch.from_numpy(a).to(dev)
        return buf[:, :C]

    th, thp, rho = put(x["theta"]), put(x["theta_p"]), put(x["rho_p"])
    v = lambda k: torch.from_numpy(x[k]).to(dev)  # noqa: E731
    sums = torch.full((2 * D + 1,), -1.0, dtype=torch.float64, device=dev)
    ops.chees_sums(th, thp, sums)
    out = torch.full((2,), -1.0, dtype=torch.float64, device=dev)
    ops.chees_stat(th, thp, rho, torch.from_numpy(mean).to(dev), v("lp_cur"), v("a_cur"), v("lp_prop"), v("a_prop"), out)
    s = _np(sums)
    assert s[2 * D] == -1.0  # (nothing written past the 2 D sums)
    return s[:2 * D].copy(), _np(out).copy()


# ---- warmup ---------------------------------------------------------------------------------------------------------
def run_chees_warmup(ops, model, seed, C=512, draws=300, eps0=0.006, steps=16, path="auto", warm=None, **kw):
    warm = dict(adapt_metric=False) if warm is None else warm
    s = bk.HMCDiag(model, eps0, steps, chains=C, seed=seed, path=path, ops=ops, **kw)
    return s, s.warmup(draws, adapt_trajectory=True, **warm)


def check_chees_report(rep, draws=300, eps_min=0.4):
    T, eps = rep["trajectory_length"], rep["stepsize"]
    print(f"chees warmup: T = {T:.4f}  eps = {eps:.4f}  max steps {max(rep['steps'])}  nonfinite {rep['nonfinite_chains']}")
    assert len(rep["T"]) == draws and len(rep["steps"]) == draws and rep["nonfinite_chains"] >= 0
    assert all(1 <= L <= 1024 for L in rep["steps"])
    assert T_BAND[0] <= T <= T_BAND[1]
    if eps_min is not None:
        assert eps >= eps_min


def check_pooled_variance_after(s, draws=100, tol=0.10):
    """Every dimension's variance over the pooled draws of all chains within `tol` of 1 (a unit Gaussian target)."""
    x = np.stack([_np(s.sample()[0]).copy() for _ in range(draws)])  # [draws, C, D]
    var = x.reshape(-1, x.shape[2]).var(axis=0, ddof=1)
    print(f"pooled variance after warmup: min {var.min():.4f} max {var.max():.4f}")
    assert np.abs(var - 1.0).max() <= tol


def chees_reports_equal(a, b):
    from tests.adapt_parity import reports_equal

    return (reports_equal(a, b) and a["trajectory_length"] == b["trajectory_length"] and a["T"] == b["T"]
            and a["steps"] == b["steps"] and a["nonfinite_chains"] == b["nonfinite_chains"])


def check_checkpoint(ops, C, D, path):
    """trajectory_length, max_steps and the jitter counter travel: draws 4-6 of a fresh sampler built without any of them
    equal the original's."""
    lam = np.logspace(0, 1, D)
    a = bk.HMCDiag(bk.DiagGaussian(lam, ops=ops), 0.05, 7, chains=C, seed=9, trajectory_length=0.5, max_steps=9, path=path,
                   ops=ops)
    run_draws(a, 3)
    sd = a.state_dict()
    ta, la = run_draws(a, 3)
    b = bk.HMCDiag(bk.DiagGaussian(lam, ops=ops), 0.05, 7, chains=C, seed=1234, path=path, ops=ops)
    b.load_state_dict(sd)
    assert b.trajectory_length == 0.5 and b.max_steps == 9 and b._jitter_n == 3
    tb, lb = run_draws(b, 3)
    assert np.array_equal(ta, tb) and np.array_equal(la, lb)
    assert b.last_steps == a.last_steps == jitter_steps(6, 0.5, 0.05, 9)
    # an older checkpoint (no such keys) leaves the sampler as it was built
    for k in ("trajectory_length", "max_steps", "jitter_n"):
        sd["meta"]["extra"].pop(k)
    c = bk.HMCDiag(bk.DiagGaussian(lam, ops=ops), 0.05, 7, chains=C, seed=1234, trajectory_length=0.3, path=path, ops=ops)
    c.load_state_dict(sd)
    assert c.trajectory_length == 0.3 and c.max_steps == 1024 and math.isfinite(c._stepsize)
