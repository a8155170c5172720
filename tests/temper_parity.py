"""Checks of bk.TemperedStretcher, bk_tempered_accept and bk_replica_swap shared by the CPU tests (on
tests/fake_ops_temper.py) and the GPU tests (on the HIP library): the drivers, an independent per-walker loop, the kernels
against their restatements, the checkpoint round trip."""
import numpy as np
import torch

import bayes_kit_amd as bk
from tests.fake_ops_temper import TemperFakeOps, replica_swap_ref, tempered_accept_ref
from tests.helpers import rng_state_words
from tests.stretch_parity import lam_of

PRIOR_SCALE, LIK_MEAN = 1.5, 0.5  # the split model of these checks: prior N(0, 1.5^2 I), ll = -1/2 sum lam_d (x_d - 0.5)^2


def bits(x):
    """An array's bytes: equality that tells NaN payloads and signed zeros apart."""
    return np.ascontiguousarray(x).view(np.uint8)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def split_model(D, device):
    """A batched prior / likelihood model whose two parts are sums IN d ORDER of elementwise operations: the same doubles
    from PyTorch on either device and from the per-walker loop below."""
    lam = torch.as_tensor(lam_of(D), dtype=torch.float64, device=device)
    c0 = -0.5 * (1.0 / (PRIOR_SCALE * PRIOR_SCALE))

    def log_prior(Th):
        t = Th[:, 0] * Th[:, 0]
        for d in range(1, D):
            t = t + Th[:, d] * Th[:, d]
        return c0 * t

    def log_likelihood(Th):
        r = Th[:, 0] - LIK_MEAN
        t = lam[0] * (r * r)
        for d in range(1, D):
            r = Th[:, d] - LIK_MEAN
            t = t + lam[d] * (r * r)
        return -0.5 * t

    return bk.TorchPriorLikelihoodModel(log_prior, log_likelihood, D)


def make(ops, betas, walkers, replicas, D, seed=11, split=False, **kw):
    model = split_model(D, ops.device) if split else bk.DiagGaussian(lam_of(D), ops=ops)
    return bk.TemperedStretcher(model, betas, walkers=walkers, replicas=replicas, seed=seed, ops=ops, **kw)


def run_draws(s, n):
    """-> theta [n, C, D], logp [n, C], partner [n, C], accepted [n, C], swapped [n, C]"""
    th, lp, pa, ac, sw = [], [], [], [], []
    for _ in range(n):
        t, l = s.sample()
        th.append(t.cpu().numpy().copy())
        lp.append(l.cpu().numpy().copy())
        pa.append(s.last_partner.cpu().numpy().copy())
        ac.append(s.last_accept.cpu().numpy().copy())
        sw.append(s.last_swapped.cpu().numpy().copy())
    return np.stack(th), np.stack(lp), np.stack(pa), np.stack(ac), np.stack(sw)


def counters(s):
    """-> accepted moves per rung [T], proposed and accepted swaps per pair [T - 1] (the device counters, summed over
    replicas and halves)."""
    R, T = s.replicas, len(s.betas)
    acc = s._rung_acc.cpu().numpy().reshape(R, T).sum(axis=0)
    prop = s._swap_prop.cpu().numpy().reshape(2, R, T).sum(axis=(0, 1))
    swp = s._swap_acc.cpu().numpy().reshape(2, R, T).sum(axis=(0, 1))
    assert prop[T - 1] == 0 and swp[T - 1] == 0  # the last rung is nobody's lower one
    return acc, prop[:T - 1], swp[:T - 1]


# ---- the scheme, written plainly: one numpy Generator per walker, walkers and pairs visited one after the other ---------
def temper_loop(betas, walkers, replicas, D, draws, seed, split, swap_every=1, a=2.0, chain_id0=0):
    """-> theta [draws, C, D], logp [draws, C] (untempered), final ll [C], final lp0 [C] or None, the walkers' generators,
    accepted moves per rung, proposed and accepted swaps per pair."""
    betas = np.asarray(betas, dtype=np.float64)
    lam = lam_of(D)
    T = len(betas)
    E, H = replicas * T, walkers // 2
    C = E * walkers
    n = C // 2
    c0 = -0.5 * (1.0 / (PRIOR_SCALE * PRIOR_SCALE))

    def parts(x):  # -> (lp0, ll)
        if not split:  # DiagGaussian: -1/2 sum lam x^2, summed in d order
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
    lo, hi = 1 / np.sqrt(a), np.sqrt(a)
    acc = np.zeros(T, dtype=np.int64)
    prop, swp = np.zeros(max(T - 1, 0), dtype=np.int64), np.zeros(max(T - 1, 0), dtype=np.int64)
    out_th, out_lp = [], []
    for it in range(1, draws + 1):
        for s in (0, 1):
            for e in range(E):
                t = e % T
                for i in range(H):
                    k = s * n + e * H + i
                    g = gens[k]
                    u_j, u_z, u_a = g.uniform(), g.uniform(), g.uniform()
                    j = (1 - s) * n + e * H + min(int(np.floor(u_j * H)), H - 1)
                    r = lo + (hi - lo) * u_z
                    z = r * r
                    star = theta[j] + z * (theta[k] - theta[j])
                    p_star, l_star = parts(star)
                    dp = (p_star - lp0[k]) if split else 0.0
                    with np.errstate(divide="ignore"):
                        if np.log(u_a) < (dp + betas[t] * (l_star - ll[k])) + (D - 1) * np.log(z):
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


def check_sampler_vs_loop(ops, betas, walkers, replicas, D, draws=7, seed=11, split=False, swap_every=1, chain_id0=0):
    s = make(ops, betas, walkers, replicas, D, seed=seed, split=split, swap_every=swap_every, chain_id0=chain_id0)
    th, lp, _, _, _ = run_draws(s, draws)
    rth, rlp, rll, rlp0, gens, acc, prop, swp = temper_loop(betas, walkers, replicas, D, draws, seed, split,
                                                            swap_every=swap_every, chain_id0=chain_id0)
    assert same(th, rth) and same(lp, rlp)
    assert same(s._ll.cpu().numpy(), rll)
    assert (s._lp0 is None) if not split else same(s._lp0.cpu().numpy(), rlp0)
    assert np.array_equal(s.rng_state(), np.stack([rng_state_words(g) for g in gens], axis=1))
    got = counters(s)
    assert np.array_equal(got[0], acc) and np.array_equal(got[1], prop) and np.array_equal(got[2], swp)
    T = len(betas)
    assert np.array_equal(s.rung_accept_rate(), acc / (draws * replicas * walkers))
    assert s.accept_rate() == acc.sum() / (draws * replicas * T * walkers)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(s.swap_rate(), np.where(prop > 0, swp / np.maximum(prop, 1), np.nan), equal_nan=True)
    return s


def check_one_rung_is_stretcher(ops, walkers, replicas, D, draws=6, seed=11):
    """TemperedStretcher(m, [1.0]) == Stretcher(m, ensembles=replicas): theta, logp, partners, masks, streams, acceptance."""
    t = make(ops, [1.0], walkers, replicas, D, seed=seed)
    s = bk.Stretcher(bk.DiagGaussian(lam_of(D), ops=ops), walkers=walkers, ensembles=replicas, seed=seed, ops=ops)
    for _ in range(draws):
        (a, la), (b, lb) = t.sample(), s.sample()
        assert same(a.cpu().numpy(), b.cpu().numpy()) and same(la.cpu().numpy(), lb.cpu().numpy())
        assert np.array_equal(t.last_partner.cpu().numpy(), s.last_partner.cpu().numpy())
        assert np.array_equal(t.last_accept.cpu().numpy(), s.last_accept.cpu().numpy())
        assert not t.last_swapped.any()
    assert np.array_equal(t.rng_state(), s.rng_state())
    assert t.accept_rate() == s.accept_rate() and t.rung_accept_rate()[0] == s.accept_rate()
    assert t.swap_rate().shape == (0,)


def check_sampler_vs_stand_in(ops, betas, walkers, replicas, D, draws=6, seed=11, split=False, swap_every=1):
    """The sampler on `ops` against the sampler on the NumPy stand-in: theta, masks, swaps and streams bit for bit, ll to
    1e-12 (the device sums a built-in density's terms in another order)."""
    s = make(ops, betas, walkers, replicas, D, seed=seed, split=split, swap_every=swap_every)
    f = make(TemperFakeOps(), betas, walkers, replicas, D, seed=seed, split=split, swap_every=swap_every)
    assert same(s._theta.cpu().numpy(), f._theta.numpy())
    th, lp, pa, ac, sw = run_draws(s, draws)
    fth, flp, fpa, fac, fsw = run_draws(f, draws)
    assert np.array_equal(pa, fpa) and np.array_equal(ac, fac) and np.array_equal(sw, fsw)
    assert same(th, fth)
    np.testing.assert_allclose(lp, flp, rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(s._ll.cpu().numpy(), f._ll.numpy(), rtol=1e-12, atol=0.0)
    assert np.array_equal(s.rng_state(), f.rng_state())
    for a, b in zip(counters(s), counters(f)):
        assert np.array_equal(a, b)
    assert s.accept_rate() == f.accept_rate()
    np.testing.assert_allclose(s.mean_log_likelihood(), f.mean_log_likelihood(), rtol=1e-11)
    assert sw.any() and not sw.all()  # (the shapes of this check do swap, and do refuse)


def check_state_round_trip(ops, betas, walkers, replicas, D, seed=11, split=True):
    """A checkpoint taken after 3 draws with swap_every = 2 continues bit for bit, the parity of the next swap round
    included, in a sampler that was built with other streams; the statistics travel with it."""
    s = make(ops, betas, walkers, replicas, D, seed=seed, split=split, swap_every=2)
    run_draws(s, 3)
    sd = s.state_dict()
    a = run_draws(s, 5)
    r = make(ops, betas, walkers, replicas, D, seed=seed + 1, split=split, swap_every=2)
    r.load_state_dict(sd)
    b = run_draws(r, 5)
    for x, y in zip(a, b):
        assert same(x, y)
    assert a[4][0].any() != a[4][1].any()  # (swap rounds after draws 4, 6, 8: every other one of the continued draws)
    assert np.array_equal(s.rng_state(), r.rng_state())
    for x, y in zip(counters(s), counters(r)):
        assert np.array_equal(x, y)
    assert s.accept_rate() == r.accept_rate()
    assert same(s.mean_log_likelihood(), r.mean_log_likelihood())
    assert same(s._lse.cpu().numpy(), r._lse.cpu().numpy())
    return sd


# ---- statistical runs (the GPU tests; the stand-in's figures at the same seeds are in their docstrings) ---------------------
def _sq_dist(Th, mu):
    """|theta - mu|^2 per row, summed in d order (elementwise operations only: the same doubles on either device)."""
    r = Th[:, 0] - mu
    t = r * r
    for d in range(1, Th.shape[1]):
        r = Th[:, d] - mu
        t = t + r * r
    return t


def run_rung_moments(ops, seed=2025):
    """D = 3, prior N(0, 2^2 I), ll = -1/2 |theta - 2|^2 / 0.25, betas = geomspace(1, 1e-2, 5) then 0, 256 walkers per rung,
    default init, 300 draws, the first 100 dropped.  Rung t is N(4 beta_t 2 / p_t, 1 / p_t) with p_t = 1/4 + 4 beta_t.
    -> (max_t |mean error| / sd, max_t |var ratio - 1|, the sampler)"""
    D = 3
    model = bk.TorchPriorLikelihoodModel(lambda Th: -0.125 * _sq_dist(Th, 0.0), lambda Th: -2.0 * _sq_dist(Th, 2.0), D)
    betas = bk.geometric_ladder(5, 1e-2, zero=True)
    s = bk.TemperedStretcher(model, betas, walkers=256, seed=seed, ops=ops)
    for _ in range(100):
        s.sample()
    pool = torch.stack([s.sample()[0] for _ in range(200)]).cpu().numpy()  # [200, C, D]
    rung = s.rung_index().cpu().numpy()
    mean_err, var_err = 0.0, 0.0
    for t, b in enumerate(betas):
        prec = 0.25 + 4.0 * b
        x = pool[:, rung == t, :].reshape(-1, D)
        mean_err = max(mean_err, np.abs(x.mean(axis=0) - 4.0 * b * 2.0 / prec).max() * np.sqrt(prec))
        var_err = max(var_err, np.abs(x.var(axis=0) * prec - 1.0).max())
    return mean_err, var_err, s


LOG_Z_TWO_MODES = -np.log(2.0 * np.pi * 16.25) - 18.0 / (2.0 * 16.25)  # log N((3, 3); 0, 16.25 I) = -5.1798


def two_mode_model():
    """D = 2, prior N(0, 4^2 I), likelihood 0.3 N(theta; (-3, -3), 0.5^2 I) + 0.7 N(theta; (3, 3), 0.5^2 I), both
    normalised: the evidence is 0.3 N((-3, -3); 0, 16.25 I) + 0.7 N((3, 3); 0, 16.25 I) = N((3, 3); 0, 16.25 I)."""
    c_prior, c_lik = float(-np.log(2.0 * np.pi * 16.0)), float(-np.log(2.0 * np.pi * 0.25))
    c_minor, c_major = float(np.log(0.3)) + c_lik, float(np.log(0.7)) + c_lik

    def log_prior(Th):
        return c_prior - _sq_dist(Th, 0.0) / 32.0

    def log_likelihood(Th):
        return torch.logaddexp(c_minor - 2.0 * _sq_dist(Th, -3.0), c_major - 2.0 * _sq_dist(Th, 3.0))

    return bk.TorchPriorLikelihoodModel(log_prior, log_likelihood, 2)


def run_two_modes(ops, seed=2025, walkers=256, draws=400):
    """betas = geomspace(1, 1e-3, 11) then 0, every walker started at (-3, -3) + 0.3 N(0, I) (the minor mode), `draws`
    draws, reset_statistics() after half of them.  -> (share of the cold walkers of the second half's draws with
    theta[0] > 0, log_evidence() of the one replica, swap_rate(), the same share for a plain Stretcher from the cold
    walkers' start)"""
    model = two_mode_model()
    betas = bk.geometric_ladder(11, 1e-3, zero=True)
    C = len(betas) * walkers
    init = -3.0 + 0.3 * np.random.default_rng(seed).normal(size=(C, 2))
    s = bk.TemperedStretcher(model, betas, a=2.0, walkers=walkers, init=init, seed=seed, ops=ops)
    cold = s.cold_rows()
    for _ in range(draws // 2):
        s.sample()
    s.reset_statistics()
    share = float(torch.stack([s.sample()[0][cold, 0] > 0 for _ in range(draws - draws // 2)]).double().mean().item())
    p = bk.Stretcher(model, a=2.0, walkers=walkers, init=init[cold.cpu().numpy()], seed=seed, ops=ops)
    for _ in range(draws // 2):
        p.sample()
    plain = float(torch.stack([p.sample()[0][:, 0] > 0 for _ in range(draws - draws // 2)]).double().mean().item())
    return share, float(s.log_evidence()[0]), s.swap_rate(), plain


# ---- the kernels alone -------------------------------------------------------------------------------------------------
LOG_U_MODES = ("random", "-inf", "0")


def ladder(T, zero=False):
    b = np.linspace(1.0, 0.2, T)
    if zero:
        b[-1] = 0.0
    return b


def column_rungs(H, T, replicas):
    """The rung of every column in the sampler's layout: two halves of replicas * T blocks of H columns."""
    return np.tile(np.repeat(np.arange(replicas * T) % T, H), 2)


def kernel_log_u(g, n, mode):
    if mode == "random":
        return np.log(g.uniform(size=n))
    return np.full(n, -np.inf if mode == "-inf" else 0.0)


def _dev(x, dev, guard, fill):
    """x on the device followed by `guard` elements of `fill` -> (the whole tensor, its view of x)."""
    full = np.concatenate([x, np.full(guard, fill, dtype=x.dtype)])
    t = torch.from_numpy(full).to(dev)
    return t, t[:len(x)]


def check_swap_kernel(ops, H, T, replicas, parity, D, pad=0, mode="random", special=False):
    """ops.replica_swap against replica_swap_ref, bit for bit: theta (its NaN padding included), a second array, ll, lp0,
    swapped and the counters; nothing written behind the C columns of any vector; columns of pairs that took no part or
    did not swap untouched; two all-swap rounds of one parity give the original back."""
    C = 2 * replicas * T * H
    g = np.random.default_rng([7, H, T, replicas, parity, D, pad, LOG_U_MODES.index(mode), int(special)])
    rung = column_rungs(H, T, replicas)
    beta = ladder(T, zero=special)[rung]
    lower = ((rung % 2 == parity) & (rung + 1 < T)).astype(np.uint8)
    theta = np.full((D, C + pad), np.nan)
    theta[:, :C] = g.normal(size=(D, C))
    theta2 = np.full((D, C + pad), np.nan)
    theta2[:, :C] = g.normal(size=(D, C))
    use_lp0, use_theta2 = (D + parity) % 2 == 0, D in (2, 33)
    ll, lp0 = 3.0 * g.normal(size=C), g.normal(size=C)
    if special:
        ll[g.uniform(size=C) < 0.2] = -np.inf
        ll[g.uniform(size=C) < 0.1] = np.nan
        ll[g.uniform(size=C) < 0.05] = np.inf
    log_u = kernel_log_u(g, C, mode)
    r_th, r_ll, r_lp0, r_sw, r_prop, r_acc = replica_swap_ref(theta, ll, lp0 if use_lp0 else None, beta, log_u, lower, H)
    r_th2 = replica_swap_ref(theta2, ll, None, beta, log_u, lower, H)[0]

    dev = ops.device
    t_th_full, t_th2_full = torch.from_numpy(theta.copy()).to(dev), torch.from_numpy(theta2.copy()).to(dev)
    t_th, t_th2 = (t_th_full[:, :C], t_th2_full[:, :C]) if pad else (t_th_full, t_th2_full)
    t_ll_full, t_ll = _dev(ll, dev, 1, 123.0)
    t_lp0_full, t_lp0 = _dev(lp0, dev, 1, 123.0)
    t_sw_full, t_sw = _dev(np.full(C, 9, dtype=np.uint8), dev, 1, 9)
    t_prop = torch.full((C // H + 1,), 5, dtype=torch.int32, device=dev)
    t_acc = torch.full((C // H + 1,), 5, dtype=torch.int32, device=dev)
    t_beta, t_logu, t_lower = (torch.from_numpy(v).to(dev) for v in (beta, log_u, lower))

    def launch():
        ops.replica_swap(t_th, t_th2 if use_theta2 else None, t_ll, t_lp0 if use_lp0 else None, t_beta, t_logu, t_lower,
                         t_sw, t_prop[:C // H], t_acc[:C // H], H)

    launch()
    got_th, got_th2 = t_th_full.cpu().numpy(), t_th2_full.cpu().numpy()
    got_ll, got_lp0, got_sw = t_ll_full.cpu().numpy(), t_lp0_full.cpu().numpy(), t_sw_full.cpu().numpy()
    assert same(got_th, r_th)
    assert same(got_th2, r_th2 if use_theta2 else theta2)
    assert same(got_ll[:C], r_ll) and got_ll[C] == 123.0
    assert same(got_lp0[:C], r_lp0 if use_lp0 else lp0) and got_lp0[C] == 123.0
    assert np.array_equal(got_sw[:C], r_sw) and got_sw[C] == 9
    prop, acc = t_prop.cpu().numpy(), t_acc.cpu().numpy()
    assert np.array_equal(prop[:-1], 5 + r_prop.astype(np.int64)) and prop[-1] == 5
    assert np.array_equal(acc[:-1], 5 + r_acc.astype(np.int64)) and acc[-1] == 5
    assert r_prop.sum() == lower.sum() and np.all(r_sw <= lower)
    # what did not swap is what it was; what swapped is its partner's
    a = np.flatnonzero(r_sw)
    still = np.ones(C, dtype=bool)
    still[a] = still[a + H] = False
    assert same(got_th[:, :C][:, still], theta[:, :C][:, still]) and same(got_ll[:C][still], ll[still])
    assert same(got_th[:, a], theta[:, a + H]) and same(got_th[:, a + H], theta[:, a])
    if mode == "-inf" and not special:
        assert np.array_equal(r_sw, lower)  # every pair swaps ...
        launch()                            # ... and swaps back
        assert same(t_th_full.cpu().numpy(), theta) and same(t_ll_full.cpu().numpy()[:C], ll)
        assert same(t_th2_full.cpu().numpy(), theta2)
        assert same(t_lp0_full.cpu().numpy()[:C], lp0)
        assert np.array_equal(t_acc.cpu().numpy()[:-1], 5 + 2 * r_acc.astype(np.int64))
    if mode == "0":  # log u = 0: exactly the pairs whose ratio exceeds one swap (strict `<`)
        lo = np.flatnonzero(lower)
        with np.errstate(invalid="ignore"):
            assert np.array_equal(r_sw[lo] != 0, (beta[lo] - beta[lo + H]) * (ll[lo + H] - ll[lo]) > 0.0)


def check_swap_kernel_refuses_everything(ops, H, T, replicas, parity, D, pad=0):
    """log u = +inf (and, on another run, NaN): no pair swaps, no byte of the state changes."""
    C = 2 * replicas * T * H
    g = np.random.default_rng([8, H, T, D])
    rung = column_rungs(H, T, replicas)
    beta = ladder(T)[rung]
    lower = ((rung % 2 == parity) & (rung + 1 < T)).astype(np.uint8)
    theta = np.full((D, C + pad), np.nan)
    theta[:, :C] = g.normal(size=(D, C))
    ll = g.normal(size=C)
    dev = ops.device
    for fill in (np.inf, np.nan):
        t_full = torch.from_numpy(theta.copy()).to(dev)
        t_th = t_full[:, :C] if pad else t_full
        t_ll, t_sw = torch.from_numpy(ll.copy()).to(dev), torch.full((C,), 9, dtype=torch.uint8, device=dev)
        t_prop, t_acc = (torch.zeros(C // H, dtype=torch.int32, device=dev) for _ in range(2))
        ops.replica_swap(t_th, None, t_ll, None, torch.from_numpy(beta).to(dev), torch.full((C,), fill, dtype=torch.float64,
                                                                                         device=dev),
                         torch.from_numpy(lower).to(dev), t_sw, t_prop, t_acc, H)
        assert same(t_full.cpu().numpy(), theta) and same(t_ll.cpu().numpy(), ll)
        assert not t_sw.cpu().numpy().any() and not t_acc.cpu().numpy().any()
        assert t_prop.cpu().numpy().sum() == lower.sum()


def check_accept_kernel(ops, H, T, replicas, half, mode="random", special=False, use_lp0=True):
    """ops.tempered_accept on the slice of one half (for half = 1 a slice that is 8-byte aligned only) against
    tempered_accept_ref: mask, ll, lp0 and the per-ensemble counts exact; nothing written outside the slice."""
    E = replicas * T
    n = E * H
    g = np.random.default_rng([9, H, T, replicas, half, LOG_U_MODES.index(mode), int(special), int(use_lp0)])
    beta = ladder(T, zero=special)[np.repeat(np.arange(E) % T, H)]
    ll, llp, lp0, lp0p = (2.0 * g.normal(size=n) for _ in range(4))
    zterm = g.normal(size=n)
    if special:
        for v in (ll, llp, lp0p):
            v[g.uniform(size=n) < 0.15] = -np.inf
            v[g.uniform(size=n) < 0.08] = np.nan
        llp[g.uniform(size=n) < 0.05] = np.inf
    log_u = kernel_log_u(g, n, mode)
    r_mask, r_ll, r_lp0, r_cnt = tempered_accept_ref(ll, lp0 if use_lp0 else None, llp, lp0p if use_lp0 else None, beta,
                                                     zterm, log_u, H)
    dev, off = ops.device, half

    def put(x, fill):
        full = np.concatenate([np.full(off, fill, dtype=x.dtype), x, np.full(1, fill, dtype=x.dtype)])
        t = torch.from_numpy(full).to(dev)
        return t, t[off:off + n]

    f_ll, t_ll = put(ll, 77.0)
    f_lp0, t_lp0 = put(lp0, 77.0)
    f_mask, t_mask = put(np.full(n, 9, dtype=np.uint8), 9)
    _, t_llp = put(llp, 0.0)
    _, t_lp0p = put(lp0p, 0.0)
    _, t_beta = put(beta, 0.0)
    _, t_z = put(zterm, 0.0)
    _, t_u = put(log_u, 0.0)
    t_cnt = torch.full((E + 1,), 3, dtype=torch.int32, device=dev)
    ops.tempered_accept(t_ll, t_lp0 if use_lp0 else None, t_llp, t_lp0p if use_lp0 else None, t_beta, t_z, t_u, t_mask,
                        t_cnt[:E], H)
    g_ll, g_lp0, g_mask, cnt = (v.cpu().numpy() for v in (f_ll, f_lp0, f_mask, t_cnt))
    assert np.array_equal(g_mask[off:off + n], r_mask) and np.all(g_mask[:off] == 9) and g_mask[off + n] == 9
    assert same(g_ll[off:off + n], r_ll) and np.all(g_ll[:off] == 77.0) and g_ll[off + n] == 77.0
    assert same(g_lp0[off:off + n], r_lp0 if use_lp0 else lp0) and g_lp0[off + n] == 77.0
    assert np.array_equal(cnt[:E], 3 + r_cnt.astype(np.int64)) and cnt[E] == 3
    assert r_cnt.sum() == r_mask.sum()
    if mode == "-inf" and not special:
        assert r_mask.all()
    if not use_lp0 and not special:  # without lp0 and at beta = 1 the test is bk_mh_accept(BK_ACCEPT_MALA)'s
        one = beta == 1.0
        with np.errstate(invalid="ignore"):
            assert np.array_equal(r_mask[one] != 0, (log_u < (llp - ll) + (zterm - 0.0))[one])


def check_kernels(ops, H, T):
    """The grid of the kernel checks for one (H, T): replicas 1 and 2, both parities and halves, D in (1, 2, 5, 33), row
    pads 0, 6 and 5, the three kinds of log u; one run each with -inf, +inf and NaN in ll and a beta = 0 rung."""
    for replicas in (1, 2):
        for parity in (0, 1):
            for D in (1, 2, 5, 33):
                for pad in (0, 6, 5):
                    for mode in LOG_U_MODES:
                        check_swap_kernel(ops, H, T, replicas, parity, D, pad=pad, mode=mode)
            check_swap_kernel(ops, H, T, replicas, parity, 5, pad=6, special=True)
            check_swap_kernel(ops, H, T, replicas, parity, 2, pad=5, mode="-inf", special=True)
            check_swap_kernel_refuses_everything(ops, H, T, replicas, parity, 5, pad=6 * parity)
        for half in (0, 1):
            for mode in LOG_U_MODES:
                for use_lp0 in (True, False):
                    check_accept_kernel(ops, H, T, replicas, half, mode=mode, use_lp0=use_lp0)
            check_accept_kernel(ops, H, T, replicas, half, special=True)
            check_accept_kernel(ops, H, T, replicas, half, mode="-inf", special=True, use_lp0=False)
