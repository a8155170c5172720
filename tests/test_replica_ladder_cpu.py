"""The replica ladder that bk.TemperedStretcher, bk.TemperedDifferentialEvolution and bk.TemperedHMC share
(bayes_kit_amd/tempering.py's ReplicaLadder), without a GPU, on each sampler's NumPy stand-in: the checkpoint format, the layout
of the swap counters, the read-outs against their definitions from the returned draws and the raw counters, and the refusal of
another ladder's checkpoint before anything is overwritten.  Ladders of one, two and three rungs: no pair at all, pairs in one
parity only, pairs in both."""
import numpy as np
import pytest

import bayes_kit_amd as bk
from tests import de_parity as dp
from tests import temper_hmc_parity as hp
from tests import temper_parity as tp
from tests.fake_ops_de import TemperDEFakeOps
from tests.fake_ops_temper import TemperFakeOps
from tests.fake_ops_temper_hmc import TemperHmcFakeOps

D, R = 3, 2
LADDERS = ([1.0], [1.0, 0.5], [1.0, 0.5, 0.0])
# per sampler: its stand-in, the halves of its layout, the columns of a rung (walkers, or chains), log_uniform calls per draw
KINDS = {"stretcher": (TemperFakeOps, 2, 4, 2), "de": (TemperDEFakeOps, 2, 8, 2), "hmc": (TemperHmcFakeOps, 1, 2, 1)}
LADDER_TENSORS = ["rung_accepted", "swap_proposed", "swap_accepted", "ll_sum", "lse", "stat_draws"]
TENSORS = {"stretcher": ["theta", "ll", "lp0", "rng_state"] + LADDER_TENSORS,
           "de": ["theta", "ll", "lp0", "rng_state"] + LADDER_TENSORS,
           "hmc": ["theta", "ll", "lp0", "grad_ll", "grad_lp0", "rng_state"] + LADDER_TENSORS}
UNSPLIT_ONLY = {"lp0", "grad_lp0"}  # (absent where the whole log density is tempered)
EXTRA = {"stretcher": ["a", "walkers", "ensembles", "betas", "replicas", "swap_every"],
         "de": ["gamma", "sigma", "jump_every", "walkers", "ensembles", "betas", "replicas", "swap_every"],
         "hmc": ["betas", "chains_per_rung", "replicas", "swap_every", "steps", "split", "stepsizes"]}

cases = pytest.mark.parametrize("betas", LADDERS, ids=lambda b: f"T{len(b)}")
kinds = pytest.mark.parametrize("kind", list(KINDS))


def build(kind, betas, replicas=R, per_rung=None, split=True, seed=11, swap_every=2):
    """-> the sampler and its stand-in"""
    ops = KINDS[kind][0]()
    n = KINDS[kind][2] if per_rung is None else per_rung
    make = {"stretcher": tp.make, "de": dp.make_tempered, "hmc": hp.make}[kind]
    return make(ops, betas, n, replicas, D, seed=seed, split=split, swap_every=swap_every), ops


def log_likelihood(kind, ops, th):
    m = hp.HandModel(hp.lam_of(D), ops.device, True) if kind == "hmc" else tp.split_model(D, ops.device)
    return m.log_likelihood(th).numpy()


@kinds
@cases
def test_checkpoint_format_and_counter_layout(kind, betas):
    _, halves, n, _ = KINDS[kind]
    T = len(betas)
    s, _ = build(kind, betas)
    s.sample()
    sd = s.state_dict()
    assert set(sd) - {"meta"} == set(TENSORS[kind]) and set(sd["meta"]["extra"]) == set(EXTRA[kind])
    ex = sd["meta"]["extra"]
    assert ex["betas"] == betas and ex["replicas"] == R and ex["swap_every"] == 2
    assert len(s._swap_prop) == len(s._swap_acc) == halves * R * T
    assert len(s._rung_acc) == len(s._lse) == R * T and sd["stat_draws"].tolist() == [1]
    assert s.chains == R * T * n and np.array_equal(s.betas, betas) and s.replicas == R and s.swap_every == 2
    # which parity has a pair is decided once, here: none with one rung, the even one alone with two
    assert [low is not None for low in s._lower] == [T >= 2, T >= 3]
    rung = s.rung_index().numpy()
    for p, low in enumerate(s._lower):
        if low is not None:
            assert np.array_equal(low.numpy() != 0, (rung % 2 == p) & (rung + 1 < T))
    assert np.array_equal(s._beta_col.numpy(), np.asarray(betas)[rung])
    assert np.array_equal(s.cold_rows().numpy(), np.flatnonzero(rung == 0))
    assert np.array_equal(np.bincount(s.replica_index().numpy() * T + rung), np.full(R * T, n))


@kinds
def test_checkpoint_format_without_the_split(kind):
    s, _ = build(kind, [1.0, 0.5], split=False)
    sd = s.state_dict()
    assert set(sd) - {"meta"} == set(TENSORS[kind]) - UNSPLIT_ONLY and set(sd["meta"]["extra"]) == set(EXTRA[kind])
    with pytest.raises(ValueError, match="split.*log_prior"):  # (one wording, named in both samplers' own tests)
        s.log_evidence()


@kinds
@cases
def test_read_outs_equal_their_definitions(kind, betas):
    _, halves, n, per_draw = KINDS[kind]
    T, draws = len(betas), 5
    s, ops = build(kind, betas)
    rung, rep = s.rung_index().numpy(), s.replica_index().numpy()
    lls, acc, swp = [], np.zeros(T), np.zeros(T)
    for _ in range(draws):
        th, _ = s.sample()
        lls.append(log_likelihood(kind, ops, th))
        acc += np.bincount(rung[s.last_accept.numpy()], minlength=T)
        swp += np.bincount(rung[s.last_swapped.numpy()], minlength=T)
    lls = np.stack(lls)  # [draws, C]
    # swap rounds 1 and 2 came after draws 2 and 4: round k proposes the pairs (t, t + 1) with t % 2 == k % 2, every column
    # of their lower rung once; a round without a pair draws nothing
    rounds = [k for k in (1, 2) if any(t % 2 == k % 2 for t in range(T - 1))]
    prop = np.array([R * n * sum(t % 2 == k % 2 for k in rounds) for t in range(T - 1)], dtype=np.float64)
    assert ops.calls.get("replica_swap", 0) == len(rounds) and ops.calls["log_uniform"] == per_draw * draws + len(rounds)
    raw = [c.numpy().reshape(halves, R, T).sum(axis=(0, 1)) for c in (s._swap_prop, s._swap_acc)]
    assert np.array_equal(raw[0][:T - 1], prop) and np.array_equal(raw[1], swp) and raw[0][T - 1:] == 0
    assert s.swap_rate().shape == (T - 1,) and np.array_equal(s.swap_rate(), swp[:T - 1] / prop)
    assert np.array_equal(s._rung_acc.numpy().reshape(R, T).sum(axis=0), acc)
    assert np.array_equal(s.rung_accept_rate(), acc / (draws * R * n)) and s.accept_rate() == acc.sum() / (draws * R * T * n)
    mean = np.array([[lls[:, (rep == r) & (rung == t)].mean() for t in range(T)] for r in range(R)])
    np.testing.assert_allclose(s.mean_log_likelihood(), mean, rtol=1e-13)
    if betas[-1] == 0.0:
        db = -np.diff(betas)
        logz = np.array([sum(np.log(np.mean(np.exp(db[t] * lls[:, (rep == r) & (rung == t + 1)]))) for t in range(T - 1))
                         for r in range(R)])
        np.testing.assert_allclose(s.log_evidence(), logz, rtol=1e-12)
    else:
        with pytest.raises(ValueError, match="betas"):
            s.log_evidence()
    s.reset_statistics()
    assert np.isnan(s.accept_rate()) and np.isnan(s.rung_accept_rate()).all() and s.rung_accept_rate().shape == (T,)
    assert np.isnan(s.swap_rate()).all() and s.swap_rate().shape == (T - 1,)
    assert np.isnan(s.mean_log_likelihood()).all() and s.mean_log_likelihood().shape == (R, T)
    assert betas[-1] != 0.0 or (np.isnan(s.log_evidence()).all() and s.log_evidence().shape == (R,))
    assert np.all(np.isneginf(s._lse.numpy())) and not s._ll_sum.numpy().any() and not s._swap_prop.numpy().any()


@kinds
@cases
def test_another_ladders_checkpoint_is_refused_and_nothing_is_overwritten(kind, betas):
    n = KINDS[kind][2]
    other = [0.9] if len(betas) == 1 else [betas[0], 0.4] + betas[2:]
    r, _ = build(kind, betas)
    for _ in range(4):  # (the last of them ends in a swap round)
        r.sample()

    def state():
        tensors = (r._theta, r._ll, r._lp0, r._lse, r._ll_sum, r._rung_acc, r._swap_prop, r._swap_acc, r._stat_n)
        return [t.numpy().copy() for t in tensors] + [r.rng_state().copy()]

    before = state()
    # (as many columns in all each time: it is the ladder that differs)
    for kw in (dict(betas=other), dict(replicas=1, per_rung=2 * n), dict(swap_every=3)):
        foreign, _ = build(kind, **{"betas": betas, "seed": 5, **kw})
        foreign.sample()
        with pytest.raises(ValueError):
            r.load_state_dict(foreign.state_dict())
        assert all(tp.same(a, b) for a, b in zip(before, state()))
    twin, _ = build(kind, betas, seed=5)
    twin.sample()
    r.load_state_dict(twin.state_dict())
    assert tp.same(r._lse.numpy(), twin._lse.numpy()) and not tp.same(before[0], r._theta.numpy())
    assert not r.last_swapped.any()
