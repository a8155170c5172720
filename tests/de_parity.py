"""Checks of bk.DifferentialEvolution, bk.TemperedDifferentialEvolution and bk_de_propose shared by the CPU tests (on
tests/fake_ops_de.py) and the GPU tests (on the HIP library): the drivers, independent per-walker loops, the kernel against
its restatement, the checkpoint round trip, the statistical runs."""
import warnings

import numpy as np
import torch

import bayes_kit_amd as bk
from tests.fake_ops_de import DEFakeOps, TemperDEFakeOps, de_propose_ref
from tests.helpers import rng_state_words
from tests.stretch_parity import U_MAX, lam_of
from tests.temper_parity import LIK_MEAN, PRIOR_SCALE, same, split_model, two_mode_model

LAM4 = np.array([1.0, 4.0, 0.25, 100.0])


def default_gamma(D):
    return 2.38 / np.sqrt(2.0 * D)


def make(ops, walkers, E, D, seed=11, **kw):
    with warnings.catch_warnings():  # (shapes with walkers // 2 <= D are checked for their bits, not for what they sample)
        warnings.simplefilter("ignore", UserWarning)
        return bk.DifferentialEvolution(bk.DiagGaussian(lam_of(D), ops=ops), walkers=walkers, ensembles=E, seed=seed,
                                        ops=ops, **kw)


def make_tempered(ops, betas, walkers, replicas, D, seed=11, split=False, **kw):
    model = split_model(D, ops.device) if split else bk.DiagGaussian(lam_of(D), ops=ops)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        return bk.TemperedDifferentialEvolution(model, betas, walkers=walkers, replicas=replicas, seed=seed, ops=ops, **kw)


def run_draws(s, n):
    """-> theta [n, C, D], logp [n, C], partners [n, 2, C], gamma [n, C], accepted [n, C], swapped [n, C] (zeros for a
    sampler without rungs)"""
    th, lp, pa, ga, ac, sw = [], [], [], [], [], []
    for _ in range(n):
        t, l = s.sample()
        th.append(t.cpu().numpy().copy())
        lp.append(l.cpu().numpy().copy())
        pa.append(s.last_partners.cpu().numpy().copy())
        ga.append(s.last_gamma.cpu().numpy().copy())
        ac.append(s.last_accept.cpu().numpy().copy())
        sw.append(s.last_swapped.cpu().numpy().copy() if hasattr(s, "last_swapped") else np.zeros_like(ac[-1]))
    return np.stack(th), np.stack(lp), np.stack(pa), np.stack(ga), np.stack(ac), np.stack(sw)


# ---- the scheme, written plainly: one numpy Generator per walker, walkers updated one after the other --------------------
def _pair(u_1, u_2, H):
    i1 = min(int(u_1 * H), H - 1)
    i2 = min(int(u_2 * (H - 1)), H - 2)
    return i1, i2 + (1 if i2 >= i1 else 0)


def de_loop(lam, walkers, E, draws, seed, gamma=None, sigma=1e-5, jump_every=0, chain_id0=0):
    """-> theta [draws, C, D], logp [draws, C], the walkers' generators, accepted moves.  Column of walker i of half s of
    ensemble e: s * (C/2) + e * H + i."""
    lam = np.asarray(lam, dtype=np.float64)
    D, H, C = len(lam), walkers // 2, E * walkers
    n = C // 2
    gamma = default_gamma(D) if gamma is None else gamma

    def logp(x):  # -1/2 sum lam x^2, summed in d order
        t = 0.0
        for d in range(D):
            t = t + x[d] * (lam[d] * x[d])
        return -0.5 * t

    gens = [np.random.Generator(np.random.Philox(key=[seed, chain_id0 + c])) for c in range(C)]
    theta = [g.normal(size=D) for g in gens]
    lp = [logp(x) for x in theta]
    out_th, out_lp, accepted = [], [], 0
    for it in range(1, draws + 1):
        gamma0 = 1.0 if jump_every > 0 and it % jump_every == 0 else gamma
        for s in (0, 1):
            for e in range(E):
                for i in range(H):
                    k = s * n + e * H + i
                    g = gens[k]
                    u_1, u_2, z, u_a = g.uniform(), g.uniform(), g.standard_normal(), g.uniform()
                    i1, i2 = _pair(u_1, u_2, H)
                    j1, j2 = (1 - s) * n + e * H + i1, (1 - s) * n + e * H + i2
                    step = gamma0 * (1.0 + sigma * z)
                    star = theta[k] + step * (theta[j1] - theta[j2])
                    lp_star = logp(star)
                    with np.errstate(divide="ignore"):
                        if np.log(u_a) < (lp_star - lp[k]) + (0.0 - 0.0):
                            theta[k], lp[k] = star, lp_star
                            accepted += 1
        out_th.append(np.stack(theta))
        out_lp.append(np.array(lp))
    return np.stack(out_th), np.stack(out_lp), gens, accepted


def check_sampler_vs_loop(ops, walkers, E, D, draws=5, seed=11, jump_every=0, chain_id0=0, sigma=1e-5):
    s = make(ops, walkers, E, D, seed=seed, jump_every=jump_every, chain_id0=chain_id0, sigma=sigma)
    th, lp, _, _, _, _ = run_draws(s, draws)
    rth, rlp, gens, accepted = de_loop(lam_of(D), walkers, E, draws, seed, sigma=sigma, jump_every=jump_every,
                                       chain_id0=chain_id0)
    assert same(th, rth) and same(lp, rlp)
    assert np.array_equal(s.rng_state(), np.stack([rng_state_words(g) for g in gens], axis=1))
    assert s.accept_rate() == accepted / (draws * E * walkers)
    return s


def tempered_de_loop(betas, walkers, replicas, D, draws, seed, split, swap_every=1, gamma=None, sigma=1e-5, jump_every=0,
                     chain_id0=0):
    """temper_parity.temper_loop with the differential-evolution move -> theta [draws, C, D], logp [draws, C] (untempered),
    final ll [C], final lp0 [C] or None, the walkers' generators, accepted moves per rung, proposed and accepted swaps per
    pair."""
    betas = np.asarray(betas, dtype=np.float64)
    lam = lam_of(D)
    T = len(betas)
    E, H = replicas * T, walkers // 2
    C = E * walkers
    n = C // 2
    c0 = -0.5 * (1.0 / (PRIOR_SCALE * PRIOR_SCALE))
    gamma = default_gamma(D) if gamma is None else gamma

    def parts(x):  # -> (lp0, ll)
        if not split:
            t = 0.0
            for d in range(D):
                t = t + x[d] * (lam[d] * x[d])
            return 0.0, -0.5 * t
        t = x[0] * x[0]
        for d in range(1, D):
            t = t + x[d] * x[d]
        r = x[0] - LIK_MEAN
        u = lam[0] * (r * r)
        for d in range(1, D):
            r = x[d] - LIK_MEAN
            u = u + lam[d] * (r * r)
        return c0 * t, -0.5 * u

    gens = [np.random.Generator(np.random.Philox(key=[seed, chain_id0 + c])) for c in range(C)]
    theta = [g.normal(size=D) for g in gens]
    lp0, ll = (list(v) for v in zip(*[parts(x) for x in theta]))
    acc = np.zeros(T, dtype=np.int64)
    prop, swp = np.zeros(max(T - 1, 0), dtype=np.int64), np.zeros(max(T - 1, 0), dtype=np.int64)
    out_th, out_lp = [], []
    for it in range(1, draws + 1):
        gamma0 = 1.0 if jump_every > 0 and it % jump_every == 0 else gamma
        for s in (0, 1):
            for e in range(E):
                t = e % T
                for i in range(H):
                    k = s * n + e * H + i
                    g = gens[k]
                    u_1, u_2, z, u_a = g.uniform(), g.uniform(), g.standard_normal(), g.uniform()
                    i1, i2 = _pair(u_1, u_2, H)
                    j1, j2 = (1 - s) * n + e * H + i1, (1 - s) * n + e * H + i2
                    step = gamma0 * (1.0 + sigma * z)
                    star = theta[k] + step * (theta[j1] - theta[j2])
                    p_star, l_star = parts(star)
                    dp = (p_star - lp0[k]) if split else 0.0
                    with np.errstate(divide="ignore"):
                        if np.log(u_a) < (dp + betas[t] * (l_star - ll[k])) + 0.0:
                            theta[k], lp0[k], ll[k] = star, p_star, l_star
                            acc[t] += 1
        if it % swap_every == 0:
            par = (it // swap_every) % 2
            for s in (0, 1):
                for r_ in range(replicas):
                    for t in range(T - 1):
                        if t % 2 != par:
                            continue
                        for i in range(H):
                            c = s * n + (r_ * T + t) * H + i
                            d = c + H
                            u = gens[c].uniform()
                            prop[t] += 1
                            with np.errstate(divide="ignore"):
                                if np.log(u) < (betas[t] - betas[t + 1]) * (ll[d] - ll[c]):
                                    theta[c], theta[d] = theta[d], theta[c]
                                    ll[c], ll[d] = ll[d], ll[c]
                                    lp0[c], lp0[d] = lp0[d], lp0[c]
                                    swp[t] += 1
        out_th.append(np.stack(theta))
        out_lp.append(np.array(lp0) + np.array(ll) if split else np.array(ll))
    return (np.stack(out_th), np.stack(out_lp), np.array(ll), np.array(lp0) if split else None, gens, acc, prop, swp)


def counters(s):
    R, T = s.replicas, len(s.betas)
    acc = s._rung_acc.cpu().numpy().reshape(R, T).sum(axis=0)
    prop = s._swap_prop.cpu().numpy().reshape(2, R, T).sum(axis=(0, 1))
    swp = s._swap_acc.cpu().numpy().reshape(2, R, T).sum(axis=(0, 1))
    return acc, prop[:T - 1], swp[:T - 1]


def check_tempered_vs_loop(ops, betas, walkers, replicas, D, draws=4, seed=11, split=True, swap_every=1, jump_every=0):
    s = make_tempered(ops, betas, walkers, replicas, D, seed=seed, split=split, swap_every=swap_every,
                      jump_every=jump_every)
    th, lp, _, _, _, sw = run_draws(s, draws)
    rth, rlp, rll, rlp0, gens, acc, prop, swp = tempered_de_loop(betas, walkers, replicas, D, draws, seed, split,
                                                                 swap_every=swap_every, jump_every=jump_every)
    assert same(th, rth) and same(lp, rlp)
    assert same(s._ll.cpu().numpy(), rll)
    assert (s._lp0 is None) if not split else same(s._lp0.cpu().numpy(), rlp0)
    assert np.array_equal(s.rng_state(), np.stack([rng_state_words(g) for g in gens], axis=1))
    got = counters(s)
    assert np.array_equal(got[0], acc) and np.array_equal(got[1], prop) and np.array_equal(got[2], swp)
    return s, sw


def check_one_rung_is_de(ops, walkers, replicas, D, draws=5, seed=11, jump_every=0):
    """TemperedDifferentialEvolution(m, [1.0]) == DifferentialEvolution(m, ensembles=replicas), bit for bit."""
    t = make_tempered(ops, [1.0], walkers, replicas, D, seed=seed, jump_every=jump_every)
    s = make(ops, walkers, replicas, D, seed=seed, jump_every=jump_every)
    for _ in range(draws):
        (a, la), (b, lb) = t.sample(), s.sample()
        assert same(a.cpu().numpy(), b.cpu().numpy()) and same(la.cpu().numpy(), lb.cpu().numpy())
        assert np.array_equal(t.last_partners.cpu().numpy(), s.last_partners.cpu().numpy())
        assert same(t.last_gamma.cpu().numpy(), s.last_gamma.cpu().numpy())
        assert np.array_equal(t.last_accept.cpu().numpy(), s.last_accept.cpu().numpy())
        assert not t.last_swapped.any()
    assert np.array_equal(t.rng_state(), s.rng_state())
    assert t.accept_rate() == s.accept_rate()


def check_partners(ops, walkers, E, D, draws=4, jump_every=0):
    """j1 != j2, and both lie in the OTHER half of the walker's own ensemble."""
    s = make(ops, walkers, E, D, jump_every=jump_every)
    n = E * walkers // 2
    ens = s.ensemble_index().cpu().numpy()
    half = np.arange(E * walkers) // n
    _, _, pa, ga, _, _ = run_draws(s, draws)
    assert pa.shape == (draws, 2, E * walkers) and pa.dtype == np.int32 and ga.dtype == np.float64
    for p in pa:
        assert np.all(p[0] != p[1])
        for j in p:
            assert np.array_equal(ens[j], ens) and np.array_equal(half[j], 1 - half)
    return ga


def check_sampler_vs_stand_in(ops, walkers, E, D, draws=6, seed=11, jump_every=0):
    """The sampler on `ops` against the sampler on the NumPy stand-in: partners, gamma, accepts and theta bit for bit, logp
    to 1e-12 (the device sums the density's terms in another order), the same streams and acceptance."""
    s = make(ops, walkers, E, D, seed=seed, jump_every=jump_every)
    f = make(DEFakeOps(), walkers, E, D, seed=seed, jump_every=jump_every)
    assert same(s._theta.cpu().numpy(), f._theta.numpy())
    th, lp, pa, ga, ac, _ = run_draws(s, draws)
    fth, flp, fpa, fga, fac, _ = run_draws(f, draws)
    assert np.array_equal(pa, fpa) and same(ga, fga) and np.array_equal(ac, fac)
    assert same(th, fth)
    np.testing.assert_allclose(lp, flp, rtol=1e-12, atol=0.0)
    assert np.array_equal(s.rng_state(), f.rng_state())
    assert s.accept_rate() == f.accept_rate()
    assert ac.any() and not ac.all()
    if jump_every:  # the mode-jumping draws took gamma0 = 1, the others gamma: sigma = 1e-5 keeps the two apart
        jump = (np.arange(1, draws + 1) % jump_every == 0)
        assert np.all(np.abs(ga[jump] - 1.0) < 1e-3) and np.all(np.abs(ga[~jump] - default_gamma(D)) < 1e-3)


def check_tempered_vs_stand_in(ops, betas, walkers, replicas, D, draws=6, seed=11, split=True, jump_every=0):
    s = make_tempered(ops, betas, walkers, replicas, D, seed=seed, split=split, jump_every=jump_every)
    f = make_tempered(TemperDEFakeOps(), betas, walkers, replicas, D, seed=seed, split=split, jump_every=jump_every)
    assert same(s._theta.cpu().numpy(), f._theta.numpy())
    th, lp, pa, ga, ac, sw = run_draws(s, draws)
    fth, flp, fpa, fga, fac, fsw = run_draws(f, draws)
    assert np.array_equal(pa, fpa) and same(ga, fga) and np.array_equal(ac, fac) and np.array_equal(sw, fsw)
    assert same(th, fth)
    np.testing.assert_allclose(lp, flp, rtol=1e-12, atol=0.0)
    assert np.array_equal(s.rng_state(), f.rng_state())
    for a, b in zip(counters(s), counters(f)):
        assert np.array_equal(a, b)
    assert s.accept_rate() == f.accept_rate()
    assert sw.any() and not sw.all()


def check_state_round_trip(ops, walkers, E, D, seed=11, jump_every=3, before=4, after=5):
    """A checkpoint taken after `before` draws (no multiple of jump_every) continues bit for bit, the phase of the
    mode-jumping draws included, in a sampler that was built with other streams."""
    assert before % jump_every != 0
    s = make(ops, walkers, E, D, seed=seed, jump_every=jump_every)
    run_draws(s, before)
    sd = s.state_dict()
    rate = s.accept_rate()
    a = run_draws(s, after)
    r = make(ops, walkers, E, D, seed=seed + 1, jump_every=jump_every)
    r.load_state_dict(sd)
    assert r.accept_rate() == rate
    b = run_draws(r, after)
    for x, y in zip(a, b):
        assert same(x, y)
    jump = (np.arange(before + 1, before + after + 1) % jump_every == 0)
    assert jump.any() and np.all(np.abs(b[3][jump] - 1.0) < 1e-3) and np.all(np.abs(b[3][~jump] - 1.0) > 1e-3)
    assert np.array_equal(s.rng_state(), r.rng_state()) and s.accept_rate() == r.accept_rate()
    return sd


# ---- the kernel alone -------------------------------------------------------------------------------------------------
INJECTS = (None, "u1_0", "u1_1", "u2_0", "u2_1", "both_0", "both_1", "z0", "sigma0")


def kernel_inputs(H, E, D, pad, inject, seed=0):
    """A state [D, C + pad] whose padding is NaN, and the active half's uniforms and normals; inject: a whole vector at an
    end of [0, 1) (INJECTS), z = 0, or sigma = 0.  -> theta, u_1, u_2, z, sigma"""
    g = np.random.default_rng([seed, H, E, D])
    n = H * E
    theta = np.full((D, 2 * n + pad), np.nan)
    theta[:, :2 * n] = g.normal(size=(D, 2 * n))
    u_1, u_2, z = g.uniform(size=n), g.uniform(size=n), g.normal(size=n)
    sigma = 0.05
    if inject is None and n >= 2:  # a few lanes at the ends either way
        u_1[0], u_1[n - 1], u_2[n // 2], u_2[(n - 1) // 2] = 0.0, U_MAX, 0.0, U_MAX
    if inject in ("u1_0", "both_0"):
        u_1[:] = 0.0
    if inject in ("u1_1", "both_1"):
        u_1[:] = U_MAX
    if inject in ("u2_0", "both_0"):
        u_2[:] = 0.0
    if inject in ("u2_1", "both_1"):
        u_2[:] = U_MAX
    if inject == "z0":
        z[:] = 0.0
    if inject == "sigma0":
        sigma = 0.0
    return theta, u_1, u_2, z, sigma


def _launch(ops, theta, n, H, half, pad, u_1, u_2, z, gamma0, sigma):
    """ops.de_propose on device copies with guards -> (theta_prop with its padding, partner1, partner2, gamma with one
    guard element each, the state as the device holds it afterwards)"""
    D = theta.shape[0]
    dev = ops.device
    col_act, col_oth = half * n, (1 - half) * n
    t_theta = torch.from_numpy(theta.copy()).to(dev)
    t_theta = t_theta[:, :2 * n] if pad else t_theta
    t_u1, t_u2, t_z = (torch.from_numpy(v).to(dev) for v in (u_1, u_2, z))
    ppad = pad - 2 if pad else 0  # (the proposal's own pitch: even with an even pad, odd with an odd one)
    t_prop_full = torch.full((D, n + ppad), np.nan, dtype=torch.float64, device=dev)
    t_prop = t_prop_full[:, :n] if ppad else t_prop_full
    t_p1 = torch.full((n + 1,), -7, dtype=torch.int32, device=dev)
    t_p2 = torch.full((n + 1,), -7, dtype=torch.int32, device=dev)
    t_g = torch.full((n + 1,), np.nan, dtype=torch.float64, device=dev)
    ops.de_propose(t_theta, col_act, col_oth, n, H, t_u1, t_u2, t_z, gamma0, sigma, t_prop, t_p1[:n], t_p2[:n], t_g[:n])
    return (t_prop_full.cpu().numpy(), t_p1.cpu().numpy(), t_p2.cpu().numpy(), t_g.cpu().numpy(), t_theta.cpu().numpy())


def _check_pairs(p1, p2, n, H, col_oth):
    """Two different columns of the other half of the walker's own ensemble."""
    e = np.arange(n) // H
    assert np.all(p1 != p2)
    for p in (p1, p2):
        assert np.all((p >= col_oth) & (p < col_oth + n)) and np.array_equal((p - col_oth) // H, e)


def check_kernel(ops, H, E, D, half, pad=0, inject=None, gamma0=0.7):
    """ops.de_propose against de_propose_ref: theta_prop, both partner arrays and gamma bit for bit, nothing written
    outside the outputs' n columns, the state untouched."""
    n = H * E
    theta, u_1, u_2, z, sigma = kernel_inputs(H, E, D, pad, inject)
    col_act, col_oth = half * n, (1 - half) * n
    prop, p1, p2, g = de_propose_ref(theta, col_act, col_oth, n, H, u_1, u_2, z, gamma0, sigma)
    got_prop, got_p1, got_p2, got_g, back = _launch(ops, theta, n, H, half, pad, u_1, u_2, z, gamma0, sigma)
    assert np.array_equal(got_p1[:n], p1) and got_p1[n] == -7
    assert np.array_equal(got_p2[:n], p2) and got_p2[n] == -7
    _check_pairs(got_p1[:n], got_p2[:n], n, H, col_oth)
    assert same(got_g[:n], g) and np.isnan(got_g[n])
    assert same(got_prop[:, :n], prop)
    assert np.isnan(got_prop[:, n:]).all()
    assert same(back, theta[:, :2 * n])
    first = col_oth + (np.arange(n) // H) * H
    if H == 2:  # the smallest half: the second partner is the other walker
        assert np.array_equal(got_p1[:n] + got_p2[:n], 2 * first + 1)
    if inject in ("u1_0", "both_0"):
        assert np.array_equal(got_p1[:n], first)
    if inject in ("u1_1", "both_1"):
        assert np.array_equal(got_p1[:n], first + H - 1)
    if inject == "u2_0":
        assert np.array_equal(got_p2[:n], first + (got_p1[:n] == first))
    if inject == "u2_1":
        assert np.array_equal(got_p2[:n], first + H - 1 - (got_p1[:n] == first + H - 1))
    if inject == "both_0":
        assert np.array_equal(got_p2[:n], first + 1)
    if inject == "both_1":
        assert np.array_equal(got_p2[:n], first + H - 2)
    if inject in ("z0", "sigma0"):
        assert np.all(got_g[:n] == gamma0)


def check_kernel_any_uniforms(ops, H, E, D, half):
    """NaN, infinities, negative values and values >= 1 in u_1 and u_2 still give two different columns of the other half
    of the walker's own ensemble (which ones is not specified), and finite proposals."""
    n = H * E
    theta, u_1, u_2, z, sigma = kernel_inputs(H, E, D, 0, None)
    odd = np.array([np.nan, -np.nan, np.inf, -np.inf, -1e-300, -0.5, -3.0, 1.0, 1.5, 2.0 ** 40, -2.0 ** 40, 1e300, -1e300,
                    2.0 ** 63, -2.0 ** 63, 2.0 ** 64])
    g = np.random.default_rng([5, H, E])
    u_1[:] = odd[g.integers(len(odd), size=n)]
    u_2[:] = odd[g.integers(len(odd), size=n)]
    u_2[::3] = g.uniform(size=len(u_2[::3]))  # (some ordinary ones beside a wild partner)
    got_prop, got_p1, got_p2, got_g, back = _launch(ops, theta, n, H, half, 0, u_1, u_2, z, 0.7, sigma)
    _check_pairs(got_p1[:n], got_p2[:n], n, H, (1 - half) * n)
    assert got_p1[n] == -7 and got_p2[n] == -7
    assert np.isfinite(got_prop).all() and np.isfinite(got_g[:n]).all()
    assert same(back, theta)


# ---- statistical runs (the GPU tests; the stand-in's figures at the same seeds are in their docstrings) ---------------------
def run_invariance(ops, seed):
    """DiagGaussian([1, 4, 0.25, 100]), 4096 walkers, default gamma, sigma and init, 150 draws discarded, 50 pooled.
    -> (max |mean| sqrt(lam), max |var lam - 1|, acceptance over all 200 draws)"""
    s = bk.DifferentialEvolution(bk.DiagGaussian(LAM4, ops=ops), walkers=4096, seed=seed, ops=ops)
    for _ in range(150):
        s.sample()
    pool = torch.cat([s.sample()[0] for _ in range(50)]).cpu().numpy()
    mean = np.abs(pool.mean(axis=0)) * np.sqrt(LAM4)
    var = np.abs(pool.var(axis=0) * LAM4 - 1.0)
    return float(mean.max()), float(var.max()), s.accept_rate()


def two_mode_init(seed, walkers=512):
    """Odd and even rows started at (3, 3) and (-3, -3) + 0.3 N(0, I)."""
    init = 0.3 * np.random.default_rng(seed).normal(size=(walkers, 2))
    init[0::2] += -3.0
    init[1::2] += 3.0
    return init


def run_two_modes(ops, seed=2025, walkers=512, draws=400, jump_every=10):
    """temper_parity.two_mode_model(), `walkers` walkers from two_mode_init, `draws` draws.  -> (share of the walkers of the
    last draws // 2 draws with theta[0] > 0 under DifferentialEvolution, the same under a Stretcher from the same start)"""
    model = two_mode_model()
    init = two_mode_init(seed, walkers)
    out = []
    for s in (bk.DifferentialEvolution(model, walkers=walkers, init=init, seed=seed, jump_every=jump_every, ops=ops),
              bk.Stretcher(model, walkers=walkers, init=init, seed=seed, ops=ops)):
        for _ in range(draws // 2):
            s.sample()
        out.append(float(torch.stack([s.sample()[0][:, 0] > 0 for _ in range(draws - draws // 2)]).double().mean().item()))
    return tuple(out)
