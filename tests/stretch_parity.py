"""Checks of bk.Stretcher and bk_stretch_propose shared by the CPU tests (on tests/fake_ops_stretch.py) and the GPU tests
(on the HIP library): the drivers, an independent per-walker loop, the kernel against its restatement, the checkpoint
round trip."""
import numpy as np
import torch

import bayes_kit_amd as bk
from tests.fake_ops_stretch import StretchFakeOps, stretch_propose_ref
from tests.helpers import rng_state_words

U_MAX = 1.0 - 2.0 ** -53  # the largest double a generator's uniform() returns


def lam_of(D):
    return np.logspace(0, 2, D)


def make(ops, walkers, E, D, seed=11, **kw):
    return bk.Stretcher(bk.DiagGaussian(lam_of(D), ops=ops), walkers=walkers, ensembles=E, seed=seed, ops=ops, **kw)


def run_draws(s, n):
    """-> theta [n, C, D], logp [n, C], partner [n, C], accepted [n, C]"""
    th, lp, pa, ac = [], [], [], []
    for _ in range(n):
        t, l = s.sample()
        th.append(t.cpu().numpy().copy())
        lp.append(l.cpu().numpy().copy())
        pa.append(s.last_partner.cpu().numpy().copy())
        ac.append(s.last_accept.cpu().numpy().copy())
    return np.stack(th), np.stack(lp), np.stack(pa), np.stack(ac)


# ---- the scheme, written plainly: one numpy Generator per walker, walkers updated one after the other --------------------
def stretch_loop(lam, walkers, E, draws, seed, a=2.0, chain_id0=0):
    """-> theta [draws, C, D], logp [draws, C], the walkers' generators, accepted moves.  Column of walker i of half s of
    ensemble e: s * (C/2) + e * H + i."""
    lam = np.asarray(lam, dtype=np.float64)
    D, H, C = len(lam), walkers // 2, E * walkers
    n = C // 2

    def logp(x):  # -1/2 sum lam x^2, summed in d order
        t = 0.0
        for d in range(D):
            t = t + x[d] * (lam[d] * x[d])
        return -0.5 * t

    gens = [np.random.Generator(np.random.Philox(key=[seed, chain_id0 + c])) for c in range(C)]
    theta = [g.normal(size=D) for g in gens]
    lp = [logp(x) for x in theta]
    lo, hi = 1 / np.sqrt(a), np.sqrt(a)
    out_th, out_lp, accepted = [], [], 0
    for _ in range(draws):
        for s in (0, 1):
            for e in range(E):
                for i in range(H):
                    k = s * n + e * H + i
                    g = gens[k]
                    u_j, u_z, u_a = g.uniform(), g.uniform(), g.uniform()
                    j = (1 - s) * n + e * H + min(int(np.floor(u_j * H)), H - 1)
                    r = lo + (hi - lo) * u_z
                    z = r * r
                    star = theta[j] + z * (theta[k] - theta[j])
                    lp_star = logp(star)
                    with np.errstate(divide="ignore"):
                        if np.log(u_a) < (lp_star - lp[k]) + ((D - 1) * np.log(z) - 0.0):
                            theta[k], lp[k] = star, lp_star
                            accepted += 1
        out_th.append(np.stack(theta))
        out_lp.append(np.array(lp))
    return np.stack(out_th), np.stack(out_lp), gens, accepted


def check_sampler_vs_loop(ops, walkers, E, D, draws=5, seed=11, chain_id0=0):
    s = make(ops, walkers, E, D, seed=seed, chain_id0=chain_id0)
    th, lp, _, _ = run_draws(s, draws)
    rth, rlp, gens, accepted = stretch_loop(lam_of(D), walkers, E, draws, seed, chain_id0=chain_id0)
    assert np.array_equal(th, rth) and np.array_equal(lp, rlp)
    assert np.array_equal(s.rng_state(), np.stack([rng_state_words(g) for g in gens], axis=1))
    assert s.accept_rate() == accepted / (draws * E * walkers)


def check_sampler_vs_stand_in(ops, walkers, E, D, draws=6, seed=11):
    """The sampler on `ops` against the sampler on the NumPy stand-in: theta bit for bit, logp to 1e-12 (the device sums
    the density's terms in another order), the streams where the stand-in's are, the same acceptance."""
    s, f = make(ops, walkers, E, D, seed=seed), make(StretchFakeOps(), walkers, E, D, seed=seed)
    assert np.array_equal(s._theta.cpu().numpy(), f._theta.numpy())
    th, lp, pa, ac = run_draws(s, draws)
    fth, flp, fpa, fac = run_draws(f, draws)
    assert np.array_equal(pa, fpa) and np.array_equal(ac, fac)
    assert np.array_equal(th, fth)
    np.testing.assert_allclose(lp, flp, rtol=1e-12, atol=0.0)
    assert np.array_equal(s.rng_state(), f.rng_state())
    assert s.accept_rate() == f.accept_rate()


def check_partners(ops, walkers, E, D, draws=3):
    """Every walker's partner lies in the OTHER half of its own ensemble; ensemble_index() says which that is."""
    s = make(ops, walkers, E, D)
    H, n = walkers // 2, E * walkers // 2
    ens = s.ensemble_index().cpu().numpy()
    assert ens.shape == (E * walkers,)
    assert np.array_equal(ens, np.tile(np.repeat(np.arange(E), H), 2))
    _, _, pa, _ = run_draws(s, draws)
    half = np.arange(E * walkers) // n
    for p in pa:
        assert np.array_equal(ens[p], ens) and np.array_equal(half[p], 1 - half)


def check_state_round_trip(ops, walkers, E, D, seed=11):
    """A checkpoint taken mid-run continues bit for bit in a sampler that was built with other streams."""
    s = make(ops, walkers, E, D, seed=seed)
    run_draws(s, 3)
    sd = s.state_dict()
    rate = s.accept_rate()
    a = run_draws(s, 3)
    r = make(ops, walkers, E, D, seed=seed + 1)
    r.load_state_dict(sd)
    assert r.accept_rate() == rate
    b = run_draws(r, 3)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert np.array_equal(s.rng_state(), r.rng_state()) and s.accept_rate() == r.accept_rate()


# ---- the kernel alone -------------------------------------------------------------------------------------------------
def kernel_inputs(H, E, D, pad, inject, seed=0):
    """A state [D, C + pad] whose padding is NaN, and the active half's uniforms; inject: None or one of "uj0", "uj1",
    "uz0", "uz1" (a whole vector at an end of [0, 1))."""
    g = np.random.default_rng([seed, H, E, D])
    n = H * E
    theta = np.full((D, 2 * n + pad), np.nan)
    theta[:, :2 * n] = g.normal(size=(D, 2 * n))
    u_j, u_z = g.uniform(size=n), g.uniform(size=n)
    if inject is None and n >= 2:  # a few lanes at the ends either way
        u_j[0], u_j[n - 1], u_z[n // 2], u_z[(n - 1) // 2] = 0.0, U_MAX, 0.0, U_MAX
    if inject == "uj0":
        u_j[:] = 0.0
    if inject == "uj1":
        u_j[:] = U_MAX
    if inject == "uz0":
        u_z[:] = 0.0
    if inject == "uz1":
        u_z[:] = U_MAX
    return theta, u_j, u_z


def check_kernel(ops, H, E, D, half, pad=0, inject=None, a=2.0):
    """ops.stretch_propose against stretch_propose_ref: theta_prop and partner bit for bit, zterm to 1e-15 (the device's
    log), nothing written outside the outputs' n columns, the state untouched."""
    n = H * E
    theta, u_j, u_z = kernel_inputs(H, E, D, pad, inject)
    lo, hi = 1 / np.sqrt(a), np.sqrt(a)
    col_act, col_oth = half * n, (1 - half) * n
    prop, zterm, partner = stretch_propose_ref(theta, col_act, col_oth, n, H, u_j, u_z, lo, hi)
    dev = ops.device
    t_theta = torch.from_numpy(theta.copy()).to(dev)
    t_theta = t_theta[:, :2 * n] if pad else t_theta
    t_uj, t_uz = torch.from_numpy(u_j).to(dev), torch.from_numpy(u_z).to(dev)
    ppad = pad - 2 if pad else 0  # (the proposal's own pitch: even with an even pad, odd with an odd one)
    t_prop_full = torch.full((D, n + ppad), np.nan, dtype=torch.float64, device=dev)
    t_prop = t_prop_full[:, :n] if ppad else t_prop_full
    t_z = torch.full((n + 1,), np.nan, dtype=torch.float64, device=dev)
    t_p = torch.full((n + 1,), -7, dtype=torch.int32, device=dev)
    ops.stretch_propose(t_theta, col_act, col_oth, n, H, t_uj, t_uz, lo, hi, t_prop, t_z[:n], t_p[:n])
    got_prop, got_z, got_p = t_prop_full.cpu().numpy(), t_z.cpu().numpy(), t_p.cpu().numpy()
    assert np.array_equal(got_p[:n], partner) and got_p[n] == -7
    assert np.all((partner >= col_oth) & (partner < col_oth + n))
    assert np.array_equal((partner - col_oth) // H, np.arange(n) // H)
    assert np.array_equal(got_prop[:, :n], prop)
    assert np.isnan(got_prop[:, n:]).all() and np.isnan(got_z[n])
    np.testing.assert_allclose(got_z[:n], zterm, rtol=1e-15, atol=0.0)
    if D == 1:
        assert np.all(got_z[:n] == 0.0)
    if inject == "uj0":
        assert np.array_equal(partner, col_oth + (np.arange(n) // H) * H)
    if inject == "uj1":
        assert np.array_equal(partner, col_oth + (np.arange(n) // H) * H + H - 1)
    if inject in ("uz0", "uz1"):  # one z for every walker: (1/sqrt a)^2 or just below a
        assert np.all(got_z[:n] == got_z[0])
    back = t_theta.cpu().numpy()
    assert np.array_equal(back, theta[:, :2 * n])
