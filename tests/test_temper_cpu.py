"""bk.TemperedStretcher without a GPU: argument validation, the sampler on the NumPy stand-in (tests/fake_ops_temper.py)
against an independent per-walker loop, one rung against bk.Stretcher, checkpoints, the statistics, the kernel harness on
the restatements themselves, and the status codes of bk_tempered_accept and bk_replica_swap."""
import ctypes

import numpy as np
import pytest

import bayes_kit_amd as bk
from tests import temper_parity as tp
from tests.fake_ops_temper import TemperFakeOps

B3 = [1.0, 0.4, 0.1]


@pytest.fixture()
def ops():
    return TemperFakeOps()


def test_argument_validation(ops):
    m = bk.DiagGaussian(tp.lam_of(3), ops=ops)
    sm = tp.split_model(3, ops.device)
    for betas in ([0.5, 1.0], [1.0, 1.0], [1.0, 0.5, 0.5], [1.0, -0.1], [float("inf"), 1.0], [1.0, float("nan")], [],
                  [[1.0, 0.5]]):
        for model in (m, sm):
            with pytest.raises(ValueError, match="betas"):
                bk.TemperedStretcher(model, betas, walkers=4, seed=1, ops=ops)
    with pytest.raises(ValueError, match="beta = 0"):
        bk.TemperedStretcher(m, [1.0, 0.0], walkers=4, seed=1, ops=ops)
    with pytest.raises(ValueError, match="beta = 0"):
        bk.TemperedStretcher(m, [0.0], walkers=4, seed=1, ops=ops)
    bk.TemperedStretcher(sm, [1.0, 0.0], walkers=4, seed=1, ops=ops)  # (with the split the prior is a rung like any other)
    for r in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="replicas"):
            bk.TemperedStretcher(m, B3, walkers=4, replicas=r, seed=1, ops=ops)
    for k in (0, -2, 2.0, True):
        with pytest.raises(ValueError, match="swap_every"):
            bk.TemperedStretcher(m, B3, walkers=4, swap_every=k, seed=1, ops=ops)
    for shape in ((3,), (4, 3), (12, 3), (24, 2), (3, 24), (0,)):
        with pytest.raises(ValueError, match="init"):
            bk.TemperedStretcher(m, B3, walkers=4, replicas=2, init=np.zeros(shape), seed=1, ops=ops)
    with pytest.raises(ValueError, match="walkers"):
        bk.TemperedStretcher(m, B3, walkers=3, seed=1, ops=ops)
    s = bk.TemperedStretcher(m, B3, walkers=4, replicas=2, init=np.zeros((24, 3)), seed=1, ops=ops)
    assert s.chains == 24 and s.ensembles == 6 and s.replicas == 2 and s.walkers == 4 and s.swap_every == 1
    assert np.array_equal(s.betas, B3)


def test_log_evidence_needs_the_split_and_both_end_rungs(ops):
    m = bk.DiagGaussian(tp.lam_of(3), ops=ops)
    sm = tp.split_model(3, ops.device)
    with pytest.raises(ValueError, match="log_prior"):
        bk.TemperedStretcher(m, B3, walkers=4, seed=1, ops=ops).log_evidence()
    for betas in ([1.0, 0.5], [0.9, 0.0], [0.9, 0.3]):
        with pytest.raises(ValueError, match="betas"):
            bk.TemperedStretcher(sm, betas, walkers=4, seed=1, ops=ops).log_evidence()
    s = bk.TemperedStretcher(sm, [1.0, 0.3, 0.0], walkers=4, replicas=2, seed=1, ops=ops)
    assert np.isnan(s.log_evidence()).all() and s.log_evidence().shape == (2,)  # (nothing drawn yet)
    s.sample()
    assert np.isfinite(s.log_evidence()).all()


def test_geometric_ladder():
    assert np.array_equal(bk.geometric_ladder(1, 0.5), [1.0])
    assert np.array_equal(bk.geometric_ladder(5, 1e-2), np.geomspace(1, 1e-2, 5))
    z = bk.geometric_ladder(5, 1e-2, zero=True)
    assert z.shape == (6,) and z[0] == 1.0 and z[-1] == 0.0 and np.all(np.diff(z) < 0)
    for T, bmin in ((0, 0.5), (-1, 0.5), (2.5, 0.5), (3, 0.0), (3, 1.0), (3, -1.0), (3, float("nan"))):
        with pytest.raises(ValueError):
            bk.geometric_ladder(T, bmin)


def test_layout_rungs_and_cold_rows(ops):
    s = tp.make(ops, B3, 4, 2, 3)
    H, T, R = 2, 3, 2
    ens = np.tile(np.repeat(np.arange(R * T), H), 2)
    assert np.array_equal(s.ensemble_index().numpy(), ens)
    assert np.array_equal(s.rung_index().numpy(), ens % T) and np.array_equal(s.replica_index().numpy(), ens // T)
    assert np.array_equal(s.cold_rows().numpy(), np.flatnonzero(ens % T == 0))
    assert np.array_equal(s._beta_col.numpy(), np.asarray(B3)[ens % T])
    # the partner of a swap is H columns on, in the same half and replica, one rung up
    for p in (0, 1):
        low = np.flatnonzero(s._lower[p].numpy()) if s._lower[p] is not None else np.zeros(0, dtype=int)
        assert np.array_equal(ens[low] % T % 2, np.full(len(low), p))
        assert np.array_equal(ens[low + H], ens[low] + 1) and np.array_equal(ens[low + H] // T, ens[low] // T)
        assert np.array_equal((low + H) // 12, low // 12)


@pytest.mark.parametrize("D", [3])
def test_one_rung_is_stretcher_bit_for_bit(ops, D):
    tp.check_one_rung_is_stretcher(ops, 6, 1, D, draws=6)
    assert "mh_accept" in ops.calls and ops.calls["tempered_accept"] == 12 and "replica_swap" not in ops.calls
    assert ops.calls["stretch_propose"] == 24 and ops.calls["select_columns"] == 24  # (both samplers, 6 draws each)


@pytest.mark.parametrize("swap_every", [1, 2])
@pytest.mark.parametrize("split", [False, True])
def test_sampler_equals_a_plain_per_walker_loop_bit_for_bit(ops, swap_every, split):
    s = tp.check_sampler_vs_loop(ops, B3, 4, 2, 3, draws=7, split=split, swap_every=swap_every)
    assert ops.calls["tempered_accept"] == 14 and ops.calls["replica_swap"] == 7 // swap_every
    assert ops.calls["stretch_propose"] == 14 and ops.calls["select_columns"] == 14 and "mh_accept" not in ops.calls
    assert np.all(s.swap_rate() > 0)


@pytest.mark.parametrize("split", [False, True])
def test_streams_follow_the_global_walker_id(ops, split):
    tp.check_sampler_vs_loop(ops, B3, 4, 2, 3, draws=7, seed=5, split=split, chain_id0=1000)


def test_whole_replicas_shard_with_chain_id0(ops):
    """No communication between replicas: replica 0 of a two-replica run, given the start and the streams of a one-replica
    run, draws what that run draws, whatever stands beside it."""
    one = tp.make(ops, B3, 4, 1, 3, seed=9, split=True)
    init = one._theta.numpy().copy()
    two = tp.make(ops, B3, 4, 2, 3, seed=9, split=True)
    rows = np.flatnonzero(two.replica_index().numpy() == 0)  # (in the order of the one-replica run's columns)
    gens = [np.random.Generator(np.random.Philox(key=[9, c])) for c in range(12)]
    seeds = [gens[np.flatnonzero(rows == c)[0]] if c in rows else np.random.Generator(np.random.Philox(key=[1, c]))
             for c in range(24)]
    init2 = two._theta.numpy().copy()
    init2[rows] = init
    two = bk.TemperedStretcher(tp.split_model(3, ops.device), B3, walkers=4, replicas=2, init=init2, seed=seeds, ops=ops)
    one = bk.TemperedStretcher(tp.split_model(3, ops.device), B3, walkers=4, replicas=1, init=init, seed=gens, ops=ops)
    for _ in range(5):
        (a, la), (b, lb) = one.sample(), two.sample()
        assert tp.same(a.numpy(), b.numpy()[rows]) and tp.same(la.numpy(), lb.numpy()[rows])


def test_draws_that_were_returned_stay_and_logp_is_untempered(ops):
    s = tp.make(ops, B3, 4, 2, 3, split=True)
    m = tp.split_model(3, ops.device)
    th, lp = s.sample()
    keep = th.numpy().copy()
    assert tp.same(lp.numpy(), m.log_density(th).numpy())
    assert tp.same(th.numpy(), s._theta.numpy())  # (the returned draw is the state after the swap round)
    s.sample()
    assert np.array_equal(th.numpy(), keep)
    t = tp.make(ops, B3, 4, 2, 3, split=False)
    th, lp = t.sample()
    np.testing.assert_allclose(lp.numpy(), -0.5 * (tp.lam_of(3) * th.numpy() ** 2).sum(axis=1), rtol=1e-14)


def test_reference_style_single_point_model_runs(ops):
    """A model with log_density(theta [D]) only: served walker by walker on the host, the whole density tempered."""
    class StdNormal:
        def dims(self):
            return 2

        def log_density(self, theta):
            assert theta.shape == (2,)
            return -0.5 * float(theta @ theta)

    s = bk.TemperedStretcher(StdNormal(), B3, walkers=6, seed=4, ops=ops)
    t = bk.TemperedStretcher(bk.IsoGaussian(2, ops=ops), B3, walkers=6, seed=4, ops=ops)
    for _ in range(4):
        (a, la), (b, lb) = s.sample(), t.sample()
        np.testing.assert_allclose(la.numpy(), lb.numpy(), rtol=1e-14)
        assert np.array_equal(a.numpy(), b.numpy())
    with pytest.raises(ValueError, match="beta = 0"):
        bk.TemperedStretcher(StdNormal(), [1.0, 0.0], walkers=6, seed=4, ops=ops)


def test_two_rungs_swap_only_in_even_rounds(ops):
    s = tp.make(ops, [1.0, 0.3], 6, 1, 3, split=True)
    before = s.rng_state().copy()
    _, _, _, _, sw = tp.run_draws(s, 4)
    assert not sw[0].any() and not sw[2].any()  # rounds 1 and 3: pairs (t, t + 1) with t odd -- there are none
    assert ops.calls["replica_swap"] == 2 and ops.calls["log_uniform"] == 8 + 2
    assert np.array_equal(sw[1].nonzero()[0] // 3 % 2, np.zeros(sw[1].sum(), dtype=int))  # (set at rung 0's walkers)
    assert not np.array_equal(before, s.rng_state())


@pytest.mark.parametrize("split", [False, True])
def test_state_dict_round_trip_continues_bit_for_bit(ops, split):
    sd = tp.check_state_round_trip(ops, B3, 4, 2, 3, split=split)
    assert sd["meta"]["draws"] == 3 and sd["meta"]["extra"]["betas"] == B3 and sd["meta"]["extra"]["swap_every"] == 2
    assert ("lp0" in sd) == split and "ll" in sd and "lse" in sd and "swap_accepted" in sd


def test_checkpoint_of_another_ladder_is_refused(ops):
    sd = tp.make(ops, B3, 4, 2, 3).state_dict()
    for betas, walkers, replicas, kw in (([1.0, 0.5, 0.1], 4, 2, {}), (B3, 8, 1, {}), (B3, 4, 2, {"swap_every": 2})):
        with pytest.raises(ValueError):  # (as many walkers in all each time)
            tp.make(ops, betas, walkers, replicas, 3, **kw).load_state_dict(sd)
    with pytest.raises(ValueError):  # a Stretcher of the same shape is another class
        bk.Stretcher(bk.DiagGaussian(tp.lam_of(3), ops=ops), walkers=4, ensembles=6, seed=1, ops=ops).load_state_dict(sd)
    tp.make(ops, B3, 4, 2, 3, seed=3).load_state_dict(sd)


def test_statistics_and_reset(ops):
    """mean_log_likelihood and log_evidence against their definitions from the returned draws; reset drops the past."""
    betas = [1.0, 0.3, 0.0]
    s = tp.make(ops, betas, 4, 2, 3, split=True)
    m = tp.split_model(3, ops.device)
    tp.run_draws(s, 3)
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


@pytest.mark.parametrize("H,T", [(1, 2), (2, 3), (65, 3)])
def test_kernel_checks_pass_on_the_restatements_themselves(ops, H, T):
    """(the harness the GPU tests run on the device, rehearsed on the stand-in)"""
    tp.check_kernels(ops, H, T)


def test_status_codes_without_a_gpu():
    """BK_E_ARG / BK_OK of bk_tempered_accept and bk_replica_swap are decided before any HIP call (dummy pointers are never
    read)."""
    lib = bk._lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    OK, E_ARG = 0, -1

    def accept(ll=p, lp0=p, ll_prop=p, lp0_prop=p, beta=p, zterm=p, log_u=p, mask=p, counts=p, n=4, H=2):
        return lib.bk_tempered_accept(ll, lp0, ll_prop, lp0_prop, beta, zterm, log_u, mask, counts, n, H, None)

    for name in ("ll", "ll_prop", "beta", "zterm", "log_u", "mask"):
        assert accept(**{name: None}, n=0) == E_ARG, name
        assert accept(**{name: None}) == E_ARG, name
    assert accept(lp0_prop=None) == E_ARG                       # lp0 without its proposal
    assert accept(n=-2) == E_ARG and accept(n=-2, H=1) == E_ARG
    assert accept(H=0) == E_ARG and accept(H=-1) == E_ARG and accept(n=0, H=0) == E_ARG
    assert accept(H=3) == E_ARG                                 # n % H != 0
    assert accept(n=0) == OK and accept(n=0, lp0=None, lp0_prop=None, counts=None) == OK

    def swap(theta=p, theta2=p, ld=8, ll=p, lp0=p, beta=p, log_u=p, lower=p, swapped=p, proposed=p, accepted=p, C=8, H=2,
             D=3):
        return lib.bk_replica_swap(theta, theta2, ld, ll, lp0, beta, log_u, lower, swapped, proposed, accepted, C, H, D,
                                   None)

    for name in ("theta", "ll", "beta", "log_u", "lower", "swapped"):
        assert swap(**{name: None}, C=0) == E_ARG, name
        assert swap(**{name: None}) == E_ARG, name
    assert swap(C=-8) == E_ARG and swap(D=-1) == E_ARG
    assert swap(H=0) == E_ARG and swap(H=-2) == E_ARG and swap(C=0, H=0) == E_ARG
    assert swap(H=3) == E_ARG                                   # C % H != 0
    assert swap(ld=7) == E_ARG                                  # ld < C
    assert swap(D=262_141) == E_ARG                             # more row blocks than a grid has
    assert swap(C=0) == OK and swap(C=0, ld=0, D=0) == OK
    assert swap(C=0, theta2=None, lp0=None, proposed=None, accepted=None) == OK
