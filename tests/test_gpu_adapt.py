"""The diagonal preconditioner, the adaptation statistics and HMCDiag.warmup on the MI355X: the checks of
tests/adapt_parity.py on the HIP library, the kernels against their NumPy restatement (tests/fake_ops_adapt.py), and the
statistical validity of the preconditioned sampler."""
import numpy as np
import pytest
import torch

import bayes_kit_amd as bk
from tests import adapt_parity as ap
from tests.fake_ops_adapt import AdaptFakeOps, accept_stat_ref
from tests.test_gpu_providers import DIAG_SRC  # (the config-3 density as a bk_term)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    return bk._lib.default_ops()


# ---- the preconditioner --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ap.PATHS)
@pytest.mark.parametrize("C,D", [(300, 48), (130, 130)])
def test_precond_diag_equals_the_oracle_dense_sampler(ops, C, D, path):
    ap.check_precond_vs_oracle(ops, C, D, path)


@pytest.mark.parametrize("C,D", [(300, 48), (129, 6)])
def test_paths_agree_bit_for_bit_whatever_the_knobs(ops, C, D):
    """(48 dims: chain-major normals on the whole-draw path, only their consumer sees sqrt(v); 6 dims: the momentum is
    generated in the state layout, a prefetched one is dropped and regenerated when v changes)"""
    ap.check_paths_agree(ops, C, D, [dict(prefetch_rng=True), dict(prefetch_rng=False), dict(graph=True)])


def test_precond_of_ones_is_the_plain_sampler(ops):
    ap.check_identity(ops, 300, 48)
    ap.check_identity(ops, 129, 6)


@pytest.mark.parametrize("D", [48, 5])
def test_from_source_density_equals_the_builtin_bit_for_bit(ops, D):
    """An elementwise from_source density has the whole-draw kernel but no preconditioned export of it: with precond_diag
    it runs one launch per leapfrog step (its density inlined).  Its draws equal the built-in DiagGaussian's, which stays
    on the whole-draw kernel -- built with the preconditioner, given it between draws (prefetch on and off), and through
    warmup."""
    lam = np.logspace(0, 1, D)
    v = ap.perturbed_variances(lam)
    C = 200
    src = lambda: bk.CTarget.from_source(DIAG_SRC, D, params=torch.as_tensor(lam).cuda())  # noqa: E731
    a = bk.HMCDiag(src(), 0.05, 7, chains=C, seed=77, precond_diag=v)
    b = bk.HMCDiag(bk.DiagGaussian(lam), 0.05, 7, chains=C, seed=77, precond_diag=v)
    assert not a._fused_draw and a._step_hook and b._fused_draw
    ta, la = ap.run_draws(a, 6)
    tb, lb = ap.run_draws(b, 6)
    assert np.array_equal(ta, tb) and np.array_equal(la, lb)
    assert np.array_equal(a.rng_state(), b.rng_state())
    for pf in (True, False):
        a = bk.HMCDiag(src(), 0.05, 7, chains=C, seed=78, prefetch_rng=pf)
        b = bk.HMCDiag(bk.DiagGaussian(lam), 0.05, 7, chains=C, seed=78, prefetch_rng=pf)
        assert a._fused_draw
        ap.run_draws(a, 2), ap.run_draws(b, 2)
        a.set_precond_diag(v), b.set_precond_diag(v)
        assert not a._fused_draw and b._fused_draw
        ta, la = ap.run_draws(a, 3)
        tb, lb = ap.run_draws(b, 3)
        assert np.array_equal(ta, tb) and np.array_equal(la, lb)
        assert np.array_equal(a.rng_state(), b.rng_state())
    a = bk.HMCDiag(src(), 0.02, 7, chains=C, seed=79)
    b = bk.HMCDiag(bk.DiagGaussian(lam), 0.02, 7, chains=C, seed=79)
    assert ap.reports_equal(a.warmup(60), b.warmup(60))
    assert np.array_equal(ap.run_draws(a, 2)[0], ap.run_draws(b, 2)[0])


@pytest.mark.parametrize("C,D", [(64, 40), (258, 130), (65, 40)])
@pytest.mark.parametrize("path", ["auto", "opaque"])
def test_gpu_equals_the_numpy_stand_in(ops, C, D, path):
    tg, lg = ap.precond_driver(ops, C, D, path)
    tc, lc = ap.precond_driver(AdaptFakeOps(), C, D, path)
    assert np.array_equal(tg, tc)
    np.testing.assert_allclose(lg, lc, rtol=1e-12)


@pytest.mark.parametrize("path", ap.PATHS)
def test_checkpoint_carries_preconditioner_and_step_size(ops, path):
    ap.check_checkpoint(ops, 129, 6, path)
    ap.check_checkpoint(ops, 300, 48, path)


def test_preconditioned_sampler_leaves_the_target_invariant(ops):
    """lam = [1, 4, 0.25, 100], precond_diag = 1/lam, eps = 0.5, L = 3 (eps L close to a quarter period), 8,192 chains,
    discard 20 draws, pool 30.  A NumPy run of exactly this gives 0.004, 0.003 and an acceptance of 0.95."""
    lam = np.array([1.0, 4.0, 0.25, 100.0])
    for path in ("auto", "step"):
        s = bk.HMCDiag(bk.DiagGaussian(lam), 0.5, 3, chains=8192, seed=12, precond_diag=1.0 / lam, path=path)
        acc = []
        for n in range(50):
            th, _ = s.sample()
            if n >= 20:
                acc.append(th.clone())
        x = torch.stack(acc).reshape(-1, 4).cpu().numpy()
        m, q = np.abs(x.mean(axis=0)) * np.sqrt(lam), np.abs(x.var(axis=0) * lam - 1.0)
        print(f"{path}: |mean| sqrt(lam) max {m.max():.4f}  |var lam - 1| max {q.max():.4f}  accept {s.accept_rate():.4f}")
        assert (m <= 0.02).all()
        assert (q <= 0.03).all()
        assert s.accept_rate() > 0.9


# ---- statistics ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [0, 1, 63, 64, 65, 4097, 65536])
def test_accept_stat_equals_its_restatement_bit_for_bit(ops, C):
    lp0, a0, lp1, a1 = ap.accept_stat_inputs(C)
    dev = [torch.from_numpy(x).cuda() for x in (lp0, a0, lp1, a1)]
    outs = []
    for _ in range(2):
        out = torch.full((2,), -1.0, dtype=torch.float64, device="cuda")
        ops.accept_stat(*dev, out)
        outs.append(out.cpu().numpy())
    assert np.array_equal(outs[0], outs[1])  # the same bits on every run
    if C == 0:
        assert outs[0][0] == 0.0 and outs[0][1] == 0.0
        return
    # (the library's host build of bk_exp is the same double as oracle.rng.exp_bk: tests/test_abi.py; it is the faster)
    lib = bk._lib.load()
    s, n = accept_stat_ref(lp0, a0, lp1, a1, exp=lib.bk_host_exp if C > 4096 else None)
    assert outs[0][0] == s and outs[0][1] == n
    if C >= 8:
        assert n >= 2.0
    # ... and without the kinetic energies (NULL = zeros)
    out = torch.empty(2, dtype=torch.float64, device="cuda")
    ops.accept_stat(dev[0], None, dev[2], None, out)
    s0, n0 = accept_stat_ref(lp0, None, lp1, None, exp=lib.bk_host_exp)
    assert out[0].item() == s0 and out[1].item() == n0


def test_precond_pack_is_ieee_sqrt_and_division(ops):
    g = np.random.default_rng(1)
    v = np.concatenate([g.random(100000) * 100.0, 10.0 ** g.uniform(-300, 300, 20000), [1.0, 4.0, 2.0, 1e-310]])
    pd = torch.empty((3, v.shape[0]), dtype=torch.float64, device="cuda")
    ops.precond_pack(torch.from_numpy(v).cuda(), pd)
    p = pd.cpu().numpy()
    with np.errstate(over="ignore"):
        assert np.array_equal(p[0], v) and np.array_equal(p[1], np.sqrt(v)) and np.array_equal(p[2], 1.0 / v)


def test_pooled_variance_and_reset(ops):
    ap.check_pooled_variance(ops)
    ap.check_pooled_variance(ops, C=1030, D=7, n=12)


# ---- warmup ---------------------------------------------------------------------------------------------------------
def _first_difference(a, b):
    return next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None)


def test_warmup_end_to_end_and_against_the_stand_in(ops):
    """The issue's conditions on the GPU; and against the NumPy stand-in on the same inputs.  Up to the first window's end
    the alpha and eps histories are equal bit for bit (the statistic is restated in the device's order, bk_exp is the same
    double).  Behind it agreement "to rounding" is not a usable condition: after a restart dual averaging swings the step
    size across the stability limit and back, and that map amplifies any difference -- on the stand-in a one-ulp change of
    sqrt(v) in 2 of 32 dimensions after the first window grows to 4e-12 in alpha 10 draws later, 4e-8 after 18, 1e-2 after
    26, and ends at another eps (0.654 against 0.660) and a v that differs by 3 %.  So the stand-in restates the pooled
    variance in the device's order too (AdaptFakeOps.rhat_partials) and EVERYTHING is compared bit for bit."""
    s, rep, lam = ap.run_warmup(ops, 11)
    ap.check_warmup_report(rep, lam)
    assert s._stepsize == rep["stepsize"] and isinstance(s._stepsize, float)
    sc, rc, _ = ap.run_warmup(AdaptFakeOps(), 11)
    e = rep["window_ends"][0]
    print(f"GPU vs stand-in: first difference in alpha at draw {_first_difference(rep['alpha'], rc['alpha'])}, in eps at "
          f"{_first_difference(rep['eps'], rc['eps'])}; final v rel {float(np.abs(rep['precond_diag'] / rc['precond_diag'] - 1).max()):.3e}, "
          f"eps {rep['stepsize']!r} vs {rc['stepsize']!r}")
    assert rep["alpha"][:e] == rc["alpha"][:e]
    assert rep["eps"][:e] == rc["eps"][:e]
    assert ap.reports_equal(rep, rc)
    assert np.array_equal(ap.run_draws(s, 2)[0], ap.run_draws(sc, 2)[0])


def test_first_adapted_metric_against_the_stand_in(ops):
    """warmup(110) has one window (draws 17..99): the final v is that window's.  Expected: rel 1e-12 against the stand-in;
    with the pooled variance restated in the device's order it is the same double."""
    _, rep, _ = ap.run_warmup(ops, 11, draws=110)
    _, rc, _ = ap.run_warmup(AdaptFakeOps(), 11, draws=110)
    assert rep["window_ends"] == [99] and rep["alpha"][:99] == rc["alpha"][:99]
    print(f"first v, GPU vs stand-in: rel {float(np.abs(rep['precond_diag'] / rc['precond_diag'] - 1).max()):.3e}")
    np.testing.assert_allclose(rep["precond_diag"], rc["precond_diag"], rtol=1e-12)
    assert np.array_equal(rep["precond_diag"], rc["precond_diag"])


def test_warmup_is_reproducible_whatever_the_path_and_knobs(ops):
    reps, after = [], []
    for kw in (dict(), dict(), dict(prefetch_rng=False), dict(path="step"), dict(path="opaque"), dict(graph=True),
               dict(path="opaque", prefetch_rng=False)):
        s, rep, _ = ap.run_warmup(ops, 3, **kw)
        reps.append(rep)
        after.append(ap.run_draws(s, 3)[0])
    for rep, th in zip(reps[1:], after[1:]):
        assert ap.reports_equal(reps[0], rep)
        assert np.array_equal(after[0], th)


def test_warmup_moves_a_state_layout_momentum_generated_ahead(ops):
    """D < 32: the momentum is generated in the state layout, one draw ahead (prefetch_rng); the one generated with the old v
    is dropped when a window ends.  Same report and draws as without generating ahead."""
    lam = np.array([1.0, 4.0, 0.25, 100.0, 30.0])
    outs = []
    for pf in (True, False):
        s = bk.HMCDiag(bk.DiagGaussian(lam), 0.01, 8, chains=1000, seed=4, prefetch_rng=pf)
        rep = s.warmup(120)
        outs.append((rep, ap.run_draws(s, 3)[0], s.rng_state().copy()))
    assert ap.reports_equal(outs[0][0], outs[1][0])
    assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2])
