"""bk.TemperedHMC without a GPU: the four symbols and their status codes, argument validation, the sampler on the NumPy
stand-in (tests/fake_ops_temper_hmc.py) against an independent chain-by-chain loop, one rung against bk.HMCDiag, checkpoints,
warmup, the statistics, and the kernel harness on the restatements themselves."""
import ctypes

import numpy as np
import pytest

import bayes_kit_amd as bk
from tests import temper_hmc_parity as hp
from tests.fake_ops_temper_hmc import TemperHmcFakeOps

B3 = [1.0, 0.4, 0.1]
E3 = [0.05, 0.08, 0.16]
NAMES = ("bk_tempered_kick_drift", "bk_tempered_finish", "bk_tempered_hmc_accept", "bk_exchange_columns")


@pytest.fixture()
def ops():
    return TemperHmcFakeOps()


def test_the_four_symbols_are_declared_exported_and_bound():
    from tests.test_abi import declared_symbols

    lib = bk._lib.load()
    for name in NAMES:
        assert name in declared_symbols() and name in bk._lib.SIGNATURES and hasattr(lib, name)
    assert bk.TemperedHMC.__name__ in bk.__all__
    for method in ("tempered_kick_drift", "tempered_finish", "tempered_hmc_accept", "exchange_columns"):
        assert callable(getattr(bk._lib.Ops, method)) and callable(getattr(TemperHmcFakeOps, method))


def test_status_codes_without_a_gpu():
    """BK_E_ARG / BK_E_ALIGN / BK_OK of the four entry points are decided before any HIP call (dummy pointers are never
    read)."""
    lib = bk._lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    OK, E_ARG, E_ALIGN = 0, -1, -2

    def kd(theta_in=p, theta_out=p, rho_in=p, rho_out=p, ld=8, grad_ll=p, grad_lp0=p, ldg=8, metric=p, beta=p, eps=p, pre=p,
           kick=p, C=8, D=3):
        return lib.bk_tempered_kick_drift(theta_in, theta_out, rho_in, rho_out, ld, grad_ll, grad_lp0, ldg, metric, beta, eps,
                                          pre, kick, C, D, None)

    for name in ("theta_in", "theta_out", "rho_in", "rho_out", "grad_ll", "beta", "eps"):
        assert kd(**{name: None}) == E_ARG, name
        assert kd(**{name: None}, C=0) == E_ARG, name
    assert kd(C=-1) == E_ARG and kd(D=-1) == E_ARG and kd(D=262_141) == E_ARG
    assert kd(ld=7) == E_ALIGN and kd(ldg=7) == E_ALIGN and kd(ld=7, C=8, D=0) == E_ALIGN
    assert kd(C=0) == OK and kd(D=0) == OK and kd(C=0, ld=0, ldg=0) == OK
    assert kd(C=0, grad_lp0=None, metric=None, pre=None, kick=None) == OK

    def fin(rho_in=p, rho_out=p, ld=8, grad_ll=p, grad_lp0=p, ldg=8, metric=p, beta=p, half=p, kin_out=p, C=8, D=3):
        return lib.bk_tempered_finish(rho_in, rho_out, ld, grad_ll, grad_lp0, ldg, metric, beta, half, kin_out, C, D, None)

    assert fin(rho_in=None) == E_ARG and fin(rho_in=None, C=0) == E_ARG
    assert fin(beta=None) == E_ARG and fin(half=None) == E_ARG  # (required with a gradient)
    assert fin(C=-1) == E_ARG and fin(D=-2) == E_ARG
    assert fin(ld=7) == E_ALIGN and fin(ldg=7) == E_ALIGN
    assert fin(C=0) == OK and fin(D=0) == OK
    assert fin(C=0, rho_out=None, grad_ll=None, grad_lp0=None, ldg=0, metric=None, beta=None, half=None, kin_out=None) == OK

    def acc(ll=p, lp0=p, kin0=p, ll_prop=p, lp0_prop=p, kin1=p, beta=p, log_u=p, mask=p, counts=p, n=4, H=2):
        return lib.bk_tempered_hmc_accept(ll, lp0, kin0, ll_prop, lp0_prop, kin1, beta, log_u, mask, counts, n, H, None)

    for name in ("ll", "kin0", "ll_prop", "kin1", "beta", "log_u", "mask"):
        assert acc(**{name: None}) == E_ARG, name
        assert acc(**{name: None}, n=0) == E_ARG, name
    assert acc(lp0_prop=None) == E_ARG
    assert acc(n=-2) == E_ARG and acc(H=0) == E_ARG and acc(H=-1) == E_ARG and acc(H=3) == E_ARG and acc(n=0, H=0) == E_ARG
    assert acc(n=0) == OK and acc(n=0, lp0=None, lp0_prop=None, counts=None) == OK

    def exch(x=p, ld=8, swapped=p, C=8, H=2, D=3):
        return lib.bk_exchange_columns(x, ld, swapped, C, H, D, None)

    assert exch(x=None) == E_ARG and exch(swapped=None) == E_ARG and exch(x=None, C=0) == E_ARG
    assert exch(C=-8) == E_ARG and exch(D=-1) == E_ARG and exch(H=0) == E_ARG and exch(H=3) == E_ARG
    assert exch(D=262_141) == E_ARG
    assert exch(ld=7) == E_ALIGN
    assert exch(C=0) == OK and exch(D=0) == OK and exch(C=8, H=8) == OK  # (one block: no column has a partner)


def test_argument_validation(ops):
    m = hp.HandModel(hp.lam_of(3), ops.device, False)
    sm = hp.HandModel(hp.lam_of(3), ops.device, True)
    kw = dict(chains=2, seed=1, ops=ops)
    for betas in ([0.5, 1.0], [1.0, 1.0], [1.0, 0.5, 0.5], [1.0, -0.1], [float("inf"), 1.0], [1.0, float("nan")], [],
                  [[1.0, 0.5]]):
        for model in (m, sm):
            with pytest.raises(ValueError, match="betas"):
                bk.TemperedHMC(model, betas, 0.1, 2, **kw)
    for betas in ([1.0, 0.0], [0.0]):
        with pytest.raises(ValueError, match="beta = 0"):
            bk.TemperedHMC(m, betas, 0.1, 2, **kw)
    bk.TemperedHMC(sm, [1.0, 0.0], 0.1, 2, **kw)  # (with the split the prior is a rung like any other)
    for eps in ([0.1, 0.2], [0.1] * 4, [[0.1, 0.2, 0.3]], 0.0, -0.1, [0.1, 0.2, float("nan")], float("inf")):
        with pytest.raises(ValueError, match="stepsize"):
            bk.TemperedHMC(m, B3, eps, 2, **kw)
    for steps in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="steps"):
            bk.TemperedHMC(m, B3, 0.1, steps, **kw)
    for chains in (0, -2, 1.5, True, None):
        with pytest.raises(ValueError, match="chains"):
            bk.TemperedHMC(m, B3, 0.1, 2, chains=chains, seed=1, ops=ops)
    for r in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="replicas"):
            bk.TemperedHMC(m, B3, 0.1, 2, replicas=r, **kw)
    for k in (0, -2, 2.0, True):
        with pytest.raises(ValueError, match="swap_every"):
            bk.TemperedHMC(m, B3, 0.1, 2, swap_every=k, **kw)
    for shape in ((3,), (4, 3), (6, 3), (12, 2), (3, 12)):
        with pytest.raises(ValueError, match="init"):
            bk.TemperedHMC(m, B3, 0.1, 2, replicas=2, init=np.zeros(shape), **kw)
    with pytest.raises(ValueError, match="metric_diag"):
        bk.TemperedHMC(m, B3, 0.1, 2, metric_diag=np.ones(2), **kw)

    class Single:
        def dims(self):
            return 3

    with pytest.raises(ValueError, match="batched"):
        bk.TemperedHMC(Single(), B3, 0.1, 2, **kw)
    s = bk.TemperedHMC(m, B3, E3, 2, replicas=2, init=np.zeros((12, 3)), seed=1, ops=ops)  # (chains from the init)
    assert s.chains == 12 and s.chains_per_rung == 2 and s.replicas == 2 and s.swap_every == 1 and s.steps == 2
    assert np.array_equal(s.betas, B3) and np.array_equal(s.stepsizes, E3)
    s.set_stepsizes(0.25)
    assert np.array_equal(s.stepsizes, [0.25] * 3) and np.all(s._half_col.numpy() == 0.125)
    with pytest.raises(ValueError, match="stepsize"):
        s.set_stepsizes([0.1, 0.2])


def test_layout_rungs_step_sizes_and_cold_rows(ops):
    s = hp.make(ops, B3, 2, 2, 3, stepsize=E3)
    H, T, R = 2, 3, 2
    blk = np.repeat(np.arange(R * T), H)
    assert np.array_equal(s.rung_index().numpy(), blk % T) and np.array_equal(s.replica_index().numpy(), blk // T)
    assert np.array_equal(s.cold_rows().numpy(), np.flatnonzero(blk % T == 0))
    assert np.array_equal(s._beta_col.numpy(), np.asarray(B3)[blk % T])
    e = np.asarray(E3)[blk % T]
    assert np.array_equal(s._eps_col.numpy(), e) and np.array_equal(s._half_col.numpy(), 0.5 * e)
    assert np.array_equal(s._neg_half_col.numpy(), -(0.5 * e))
    for p in (0, 1):  # the partner of a swap is H columns on, in the same replica, one rung up
        low = np.flatnonzero(s._lower[p].numpy()) if s._lower[p] is not None else np.zeros(0, dtype=int)
        assert np.array_equal(blk[low] % T % 2, np.full(len(low), p))
        assert np.array_equal(blk[low + H], blk[low] + 1) and np.array_equal(blk[low + H] // T, blk[low] // T)


@pytest.mark.parametrize("swap_every", [1, 2])
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("betas,eps", [([1.0], 0.05), (B3, E3)])
def test_sampler_equals_a_plain_chain_by_chain_loop_bit_for_bit(ops, betas, eps, split, swap_every):
    s = hp.check_sampler_vs_loop(ops, betas, 3, 2, 3, draws=7, split=split, swap_every=swap_every, stepsize=eps, steps=3)
    rounds = 7 // swap_every if len(betas) > 1 else 0
    assert ops.calls["tempered_kick_drift"] == 21 and ops.calls["tempered_finish"] == 7
    assert ops.calls["tempered_hmc_accept"] == 7 and ops.calls.get("replica_swap", 0) == rounds
    assert ops.calls.get("exchange_columns", 0) == rounds * (2 if split else 1)
    assert ops.calls["log_uniform"] == 7 + rounds and "mh_accept" not in ops.calls and "kick_drift" not in ops.calls
    assert len(betas) == 1 or np.all(s.swap_rate() > 0)


@pytest.mark.parametrize("split", [False, True])
def test_streams_follow_the_global_chain_id_and_the_metric_is_applied(ops, split):
    hp.check_sampler_vs_loop(ops, B3, 2, 2, 4, draws=7, seed=5, split=split, chain_id0=1000, stepsize=E3,
                             metric=[0.5, 1.0, 2.0, 1.5])


@pytest.mark.parametrize("C,D", [(6, 3), (5, 9)])
def test_one_rung_is_hmc_bit_for_bit(ops, C, D):
    hp.check_one_rung_is_hmc(ops, C, D, draws=7, stepsize=0.17)
    assert ops.calls["mh_accept"] == 7 and ops.calls["tempered_hmc_accept"] == 7 and "replica_swap" not in ops.calls


def test_draws_that_were_returned_stay_and_logp_is_untempered(ops):
    s = hp.make(ops, B3, 2, 2, 3, split=True, stepsize=E3)
    m = hp.HandModel(hp.lam_of(3), ops.device, True)
    th, lp = s.sample()
    keep = th.numpy().copy()
    assert hp.same(lp.numpy(), (m.log_prior(th) + m.log_likelihood(th)).numpy())
    assert hp.same(th.numpy(), s._theta.numpy())  # (the returned draw is the state after the swap round)
    s.sample()
    assert np.array_equal(th.numpy(), keep)


def test_torch_prior_likelihood_model_is_split_through_autograd(ops):
    """TorchPriorLikelihoodModel's two gradient methods: the values of its parts and their autograd gradients; TemperedHMC
    takes it as a split model (beta = 0 allowed)."""
    import torch

    from tests.temper_parity import split_model

    m = split_model(3, ops.device)
    Th = torch.from_numpy(np.random.default_rng(0).normal(size=(5, 3)))
    (p, g0), (l, gl) = m.log_prior_gradient(Th), m.log_likelihood_gradient(Th)
    assert hp.same(p.numpy(), m.log_prior(Th).numpy()) and hp.same(l.numpy(), m.log_likelihood(Th).numpy())
    np.testing.assert_allclose(g0.numpy(), hp.C1 * Th.numpy(), rtol=1e-14)
    np.testing.assert_allclose(gl.numpy(), -(hp.lam_of(3) * (Th.numpy() - hp.LIK_MEAN)), rtol=1e-14)
    assert not g0.requires_grad and not p.requires_grad
    s = bk.TemperedHMC(m, [1.0, 0.3, 0.0], 0.05, 2, chains=2, seed=1, ops=ops)
    s.sample()
    assert s._split and np.isfinite(s.log_evidence()).all()


@pytest.mark.parametrize("split", [False, True])
def test_state_dict_round_trip_continues_bit_for_bit(ops, split):
    sd = hp.check_state_round_trip(ops, B3, 4, 2, 3, split=split)
    ex = sd["meta"]["extra"]
    assert sd["meta"]["draws"] == 3 and ex["betas"] == B3 and ex["swap_every"] == 2 and len(ex["stepsizes"]) == 3
    assert ("lp0" in sd) == split and ("grad_lp0" in sd) == split and "grad_ll" in sd and "lse" in sd


def test_checkpoint_of_another_ladder_is_refused_before_anything_is_overwritten(ops):
    sd = hp.make(ops, B3, 4, 2, 3).state_dict()
    for betas, chains, replicas, kw in (([1.0, 0.5, 0.1], 4, 2, {}), (B3, 8, 1, {}), (B3, 4, 2, {"swap_every": 2}),
                                        (B3, 4, 2, {"steps": 4}), (B3, 4, 2, {"split": True})):
        r = hp.make(ops, betas, chains, replicas, 3, seed=2, **kw)  # (as many chains in all each time)
        before = (r._theta.numpy().copy(), r.rng_state().copy())
        with pytest.raises(ValueError):
            r.load_state_dict(sd)
        assert hp.same(r._theta.numpy(), before[0]) and np.array_equal(r.rng_state(), before[1])
    hp.make(ops, B3, 4, 2, 3, seed=3, stepsize=0.3).load_state_dict(sd)


def test_warmup_gives_the_same_report_twice_and_a_checkpoint_after_it_continues(ops):
    rep = hp.check_warmup_repeats_and_continues(ops, B3, 8, 2, 3, draws=12)
    assert ops.calls["replica_swap"] >= 2 * 12  # (swap rounds go on during warmup)
    s = hp.make(ops, B3, 2, 1, 3)
    for bad in ((0, 0.8), (5, 0.0), (5, 1.0)):
        with pytest.raises(ValueError, match="warmup"):
            s.warmup(*bad)
    # the step sizes moved the right way: a rung that accepted everything got a larger step size
    first = np.asarray(rep["alpha"][0])
    assert np.all(np.asarray(rep["eps"][1])[first == 1.0] > 0.3)


def test_statistics_and_reset(ops):
    """mean_log_likelihood and log_evidence against their definitions from the returned draws; reset drops the past."""
    betas = [1.0, 0.3, 0.0]
    s = hp.make(ops, betas, 4, 2, 3, split=True, stepsize=[0.05, 0.1, 0.4])
    m = hp.HandModel(hp.lam_of(3), ops.device, True)
    with pytest.raises(ValueError, match="split"):
        hp.make(ops, B3, 2, 1, 3).log_evidence()
    assert np.isnan(s.log_evidence()).all() and s.log_evidence().shape == (2,)  # (nothing drawn yet)
    hp.run_draws(s, 3)
    s.reset_statistics()
    assert np.isnan(s.accept_rate()) and np.isnan(s.rung_accept_rate()).all() and np.isnan(s.swap_rate()).all()
    rung, rep = s.rung_index().numpy(), s.replica_index().numpy()
    lls, acc = [], 0
    for _ in range(4):
        th, _ = s.sample()
        lls.append(m.log_likelihood(th).numpy())
        acc += int(s.last_accept.sum())
    lls = np.stack(lls)  # [draws, C]
    assert s.accept_rate() == acc / (4 * 24)
    mean = np.array([[lls[:, (rep == r) & (rung == t)].mean() for t in range(3)] for r in range(2)])
    np.testing.assert_allclose(s.mean_log_likelihood(), mean, rtol=1e-13)
    db = -np.diff(betas)
    logz = np.array([sum(np.log(np.mean(np.exp(db[t] * lls[:, (rep == r) & (rung == t + 1)]))) for t in range(2))
                     for r in range(2)])
    np.testing.assert_allclose(s.log_evidence(), logz, rtol=1e-12)
    assert s.rung_accept_rate().shape == (3,) and s.swap_rate().shape == (2,)
    with pytest.raises(ValueError, match="betas"):
        hp.make(ops, [1.0, 0.5], 2, 1, 3, split=True).log_evidence()


@pytest.mark.parametrize("H,T", [(1, 2), (2, 3), (65, 3)])
def test_kernel_checks_pass_on_the_restatements_themselves(ops, H, T):
    """(the harness the GPU tests run on the device, rehearsed on the stand-in)"""
    hp.check_kernels(ops, H, T)
    for pad in (0, 5):
        hp.check_exchange_kernel(ops, H, T, 2, 5, pad=pad)


def test_the_scheme_in_numpy_runs(ops):
    """(the vectorised run the statistical GPU tests took their bounds from, at a size that takes no time)"""
    mean_err, var_err = hp.scheme_rung_moments(1, chains=64)
    assert mean_err < 0.2 and var_err < 0.2
    acc, eps = hp.scheme_warmup_band(1, chains=64)
    assert np.all(np.abs(acc - 0.8) < 0.15) and np.all(np.diff(eps) > 0)
