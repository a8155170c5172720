"""bk.DifferentialEvolution and bk.TemperedDifferentialEvolution without a GPU: argument validation, the samplers on the
NumPy stand-in (tests/fake_ops_de.py) against independent per-walker loops, sharding, partners, checkpoints, and
bk_de_propose's status codes."""
import ctypes
import warnings

import numpy as np
import pytest

import bayes_kit_amd as bk
from tests import de_parity as dp
from tests import stretch_parity as sp
from tests.fake_ops_de import DEFakeOps, TemperDEFakeOps, de_propose_ref


@pytest.fixture()
def ops():
    return DEFakeOps()


def _model(ops, D=3):
    return bk.DiagGaussian(sp.lam_of(D), ops=ops)


def test_argument_validation(ops):
    m = _model(ops, 1)
    for g in (0.0, -1.0, float("nan"), float("inf"), True, "1"):
        with pytest.raises(ValueError, match="gamma"):
            bk.DifferentialEvolution(m, gamma=g, seed=1, ops=ops)
    for s in (-1e-9, float("nan"), float("inf"), None, False):
        with pytest.raises(ValueError, match="sigma"):
            bk.DifferentialEvolution(m, sigma=s, seed=1, ops=ops)
    for w in (5, 7, 2, 0, -4, True, 4.0):
        with pytest.raises(ValueError, match="walkers"):
            bk.DifferentialEvolution(m, walkers=w, seed=1, ops=ops)
    for j in (-1, 1.0, 2.5, True, None):
        with pytest.raises(ValueError, match="jump_every"):
            bk.DifferentialEvolution(m, jump_every=j, seed=1, ops=ops)
    for e in (0, -1, 1.5):
        with pytest.raises(ValueError, match="ensembles"):
            bk.DifferentialEvolution(m, ensembles=e, seed=1, ops=ops)
    with pytest.raises(ValueError, match="init"):
        bk.DifferentialEvolution(m, walkers=4, init=np.zeros((3, 1)), seed=1, ops=ops)
    s = bk.DifferentialEvolution(m, gamma=0.5, sigma=0.0, walkers=4, init=np.zeros((8, 1)), ensembles=2, jump_every=0,
                                 seed=1, ops=ops)  # the bounds themselves are fine
    assert (s.gamma, s.sigma, s.jump_every, s.walkers, s.ensembles) == (0.5, 0.0, 0, 4, 2)
    with pytest.raises(AttributeError, match="last_partners"):
        s.last_partner


def test_too_few_walkers_per_half_warn(ops):
    for D, w in ((2, 4), (3, 6), (5, 10), (5, 4)):
        with pytest.warns(UserWarning, match="not ergodic"):
            bk.DifferentialEvolution(_model(ops, D), walkers=w, seed=1, ops=ops)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        bk.DifferentialEvolution(_model(ops, 2), walkers=6, seed=1, ops=ops)
        bk.DifferentialEvolution(_model(ops, 2), seed=1, ops=ops)
        bk.TemperedDifferentialEvolution(_model(ops, 2), [1.0, 0.5], seed=1, ops=TemperDEFakeOps())


def test_defaults(ops):
    for D in (1, 2, 3, 5):
        s = bk.DifferentialEvolution(_model(ops, D), seed=2, ops=ops)
        assert s.walkers == max(4, 4 * D) and s.chains == s.walkers
        assert s.gamma == 2.38 / np.sqrt(2 * D) and s.sigma == 1e-5 and s.jump_every == 0
        th, lp = s.sample()
        assert tuple(th.shape) == (s.walkers, D) and tuple(lp.shape) == (s.walkers,)
        assert tuple(s.last_partners.shape) == (2, s.walkers) and tuple(s.last_gamma.shape) == (s.walkers,)
    s = bk.DifferentialEvolution(_model(ops, 3), seed=2, ensembles=4, ops=ops)
    assert s.chains == 48 and s.ensembles == 4
    assert isinstance(s, bk.Stretcher)


@pytest.mark.parametrize("jump_every", [0, 2])
@pytest.mark.parametrize("walkers,E,D", [(4, 1, 1), (6, 2, 2), (10, 3, 3)])
def test_sampler_equals_a_plain_per_walker_loop_bit_for_bit(ops, walkers, E, D, jump_every):
    dp.check_sampler_vs_loop(ops, walkers, E, D, draws=5, jump_every=jump_every)
    assert ops.calls["de_propose"] == 10 and ops.calls["mh_accept"] == 10 and ops.calls["select_columns"] == 10
    assert ops.calls["momentum_refresh"] == 10 + 1 and "stretch_propose" not in ops.calls  # (+ 1: the default init)


def test_streams_follow_the_global_walker_id(ops):
    dp.check_sampler_vs_loop(ops, 6, 2, 2, draws=3, seed=5, jump_every=2, chain_id0=1000)


def test_a_wide_sigma_is_the_same_scheme(ops):
    s = dp.check_sampler_vs_loop(ops, 6, 2, 2, draws=3, sigma=0.3)
    g = s.last_gamma.numpy()
    assert np.unique(g).size == g.size  # (every walker its own step)


def test_two_shards_of_whole_ensembles_equal_the_one_run(ops):
    """No communication between ensembles: two shards of two ensembles each, made with chain_id0 = 0 and 2 * walkers, draw
    what the one run of four ensembles draws whose walkers carry the same global ids (its column s * C/2 + e * H + i is
    column s * C/4 + (e % 2) * H + i of shard e // 2)."""
    walkers, D, draws, seed = 6, 2, 5, 9
    H, Cs = walkers // 2, 2 * walkers
    shards = [dp.make(ops, walkers, 2, D, seed=seed, jump_every=2, chain_id0=r * Cs) for r in (0, 1)]
    where = [(e // 2, s * (Cs // 2) + (e % 2) * H + i) for s in (0, 1) for e in range(4) for i in range(H)]
    gens = [np.random.Generator(np.random.Philox(key=[seed, r * Cs + c])) for r, c in where]
    init = np.stack([shards[r]._theta.numpy()[c] for r, c in where])
    for g in gens:  # (a shard's walker has drawn its start from its stream)
        g.normal(size=D)
    one = bk.DifferentialEvolution(_model(ops, D), walkers=walkers, ensembles=4, init=init, seed=gens, jump_every=2, ops=ops)
    a = dp.run_draws(one, draws)
    b = [dp.run_draws(s, draws) for s in shards]
    for x, y0, y1 in zip(a, *b):  # theta, logp, partners (columns: compared below), gamma, accepted
        if x.ndim == 3 and x.shape[1] == 2:
            continue
        got = np.stack([(y0, y1)[r][:, c] for r, c in where], axis=1)
        assert dp.same(x, got)
    col = {rc: k for k, rc in enumerate(where)}
    for k, (r, c) in enumerate(where):
        for t in range(draws):
            assert [col[(r, int(j))] for j in b[r][2][t, :, c]] == a[2][t, :, k].tolist()
    assert a[4].any() and one.accept_rate() == (shards[0].accept_rate() + shards[1].accept_rate()) / 2


@pytest.mark.parametrize("walkers,E,D", [(4, 1, 1), (6, 2, 2), (10, 3, 3)])
def test_partners_differ_and_lie_in_the_other_half_of_the_same_ensemble(ops, walkers, E, D):
    dp.check_partners(ops, walkers, E, D, draws=6)


def test_every_jump_every_th_draw_takes_gamma_one(ops):
    ga = dp.check_partners(ops, 6, 2, 2, draws=7, jump_every=3)
    jump = np.arange(1, 8) % 3 == 0
    assert np.all(np.abs(ga[jump] - 1.0) < 1e-3) and np.all(np.abs(ga[~jump] - dp.default_gamma(2)) < 1e-3)
    s = dp.make(ops, 6, 1, 2, sigma=0.0, jump_every=1)
    s.sample()
    assert np.all(s.last_gamma.numpy() == 1.0)


@pytest.mark.parametrize("walkers,E,D", [(6, 2, 2), (10, 3, 3)])
def test_state_dict_round_trip_continues_bit_for_bit(ops, walkers, E, D):
    dp.check_state_round_trip(ops, walkers, E, D, jump_every=3, before=4)


def test_checkpoint_of_another_setting_is_refused(ops):
    sd = dp.make(ops, 6, 2, 2, jump_every=3).state_dict()
    for kw in (dict(gamma=0.9), dict(sigma=1e-4), dict(jump_every=2), dict(jump_every=0)):
        other = dict(jump_every=3)
        other.update(kw)
        with pytest.raises(ValueError, match="checkpoint"):
            dp.make(ops, 6, 2, 2, **other).load_state_dict(sd)
    with pytest.raises(ValueError):
        dp.make(ops, 4, 3, 2, jump_every=3).load_state_dict(sd)  # (as many walkers in all, other ensembles)
    with pytest.raises(ValueError):
        sp.make(ops, 6, 2, 2).load_state_dict(sd)  # (a Stretcher)
    dp.make(ops, 6, 2, 2, jump_every=3).load_state_dict(sd)


# ---- the tempered class ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jump_every", [0, 2])
def test_one_rung_is_differential_evolution(jump_every):
    dp.check_one_rung_is_de(TemperDEFakeOps(), 6, 2, 2, jump_every=jump_every)


def test_tempered_sampler_equals_its_per_walker_loop_through_swap_rounds_of_both_parities():
    ops = TemperDEFakeOps()
    s, sw = dp.check_tempered_vs_loop(ops, [1.0, 0.5, 0.1], 6, 2, 2, draws=4, split=True, jump_every=2)
    assert ops.calls["replica_swap"] == 4 and ops.calls["de_propose"] == 8 and ops.calls["tempered_accept"] == 8
    rung = s.rung_index().numpy()
    lower_of_round = [np.unique(rung[row]) for row in sw]  # round k swaps the pairs (t, t + 1) with t % 2 == k % 2
    assert any(r.tolist() == [0] for r in lower_of_round[1::2]) and any(r.tolist() == [1] for r in lower_of_round[0::2])
    assert isinstance(s, bk.TemperedStretcher) and s.jump_every == 2


def test_tempered_checkpoint_of_another_setting_is_refused():
    ops = TemperDEFakeOps()
    sd = dp.make_tempered(ops, [1.0, 0.5], 6, 1, 2, jump_every=3).state_dict()
    for kw in (dict(gamma=0.9), dict(sigma=1e-4), dict(jump_every=2), dict(swap_every=2)):
        other = dict(jump_every=3)
        other.update(kw)
        with pytest.raises(ValueError, match="checkpoint"):
            dp.make_tempered(ops, [1.0, 0.5], 6, 1, 2, **other).load_state_dict(sd)
    with pytest.raises(ValueError, match="checkpoint"):
        dp.make_tempered(ops, [1.0, 0.4], 6, 1, 2, jump_every=3).load_state_dict(sd)
    r = dp.make_tempered(ops, [1.0, 0.5], 6, 1, 2, seed=3, jump_every=3)
    r.load_state_dict(sd)


# ---- Stretcher is what it was ----------------------------------------------------------------------------------------------
def test_stretcher_still_equals_its_loop(ops):
    sp.check_sampler_vs_loop(ops, 6, 2, 3, draws=4)
    assert ops.calls["stretch_propose"] == 8 and "de_propose" not in ops.calls


# ---- the kernel's harness and status codes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("H,E,D", [(2, 1, 1), (3, 3, 5), (65, 3, 2)])
def test_kernel_check_passes_on_the_restatement_itself(ops, H, E, D):
    """(the harness the GPU tests run on the device, rehearsed on the stand-in)"""
    for half in (0, 1):
        for inject in dp.INJECTS:
            dp.check_kernel(ops, H, E, D, half, pad=5 * half, inject=inject)
        dp.check_kernel_any_uniforms(ops, H, E, D, half)


def test_pairs_are_uniform_over_the_ordered_pairs():
    """Every one of the H (H - 1) ordered pairs of different walkers has the same probability: exact on a grid of
    uniforms whose side is a multiple of H and of H - 1."""
    H, m = 5, 5 * 4 * 7
    u = (np.arange(m) + 0.5) / m
    u_1, u_2 = (v.ravel() for v in np.meshgrid(u, u, indexing="ij"))
    n = u_1.size  # (n / H ensembles, one grid point per active walker)
    _, j1, j2, _ = de_propose_ref(np.zeros((1, 2 * n)), 0, n, n, H, u_1, u_2, np.zeros(n), 1.0, 0.0)
    base = n + (np.arange(n) // H) * H
    counts = np.zeros((H, H), dtype=np.int64)
    np.add.at(counts, (j1 - base, j2 - base), 1)
    assert np.array_equal(counts, (m // H) * (m // (H - 1)) * (1 - np.eye(H, dtype=np.int64)))


def test_de_propose_status_codes_without_a_gpu():
    """BK_E_ARG / BK_OK of bk_de_propose are decided before any HIP call (dummy pointers are never read)."""
    lib = bk._lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    OK, E_ARG = 0, -1

    def call(theta=p, ld=8, col_act=0, col_oth=4, n=4, H=2, u_1=p, u_2=p, z=p, prop=p, ldp=4, partner1=p, partner2=p,
             gamma=p, D=3):
        return lib.bk_de_propose(theta, ld, col_act, col_oth, n, H, u_1, u_2, z, 0.7, 1e-5, prop, ldp, partner1, partner2,
                                 gamma, D, None)

    for name in ("theta", "u_1", "u_2", "z", "prop", "partner1", "partner2", "gamma"):
        assert call(**{name: None}) == E_ARG, name
    assert call(H=1) == E_ARG and call(H=0) == E_ARG and call(H=-2) == E_ARG   # a pair needs two walkers per half
    assert call(H=3) == E_ARG               # n % H != 0
    assert call(ld=7) == E_ARG              # ld < columns (4 + 4)
    assert call(col_act=4, col_oth=0, ld=7) == E_ARG
    assert call(ldp=3) == E_ARG
    assert call(n=-2) == E_ARG and call(D=-1) == E_ARG and call(col_oth=-4) == E_ARG and call(col_act=-1) == E_ARG
    big = 2 ** 31
    assert call(n=big, H=2, ld=2 * big, col_oth=big, ldp=big) == E_ARG      # more columns than INT32_MAX
    assert call(D=262_144) == E_ARG
    assert call(n=0) == OK and call(n=0, ld=0, col_oth=0, ldp=0) == OK
    assert call(D=0) == OK
    assert call(n=0, H=1) == E_ARG          # (an empty launch still has to be a well-formed one)
