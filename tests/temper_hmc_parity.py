"""Checks of bk.TemperedHMC and its four entry points shared by the CPU tests (on tests/fake_ops_temper_hmc.py) and the GPU
tests (on the HIP library): the drivers, an independent chain-by-chain loop, the kernels against their restatements, the
checkpoint round trip, and the statistical runs with a vectorised NumPy run of the same scheme for their bounds."""
import numpy as np
import torch

import bayes_kit_amd as bk
from tests.fake_ops_temper_hmc import (TemperHmcFakeOps, exchange_columns_ref, tempered_finish_ref, tempered_hmc_accept_ref,
                                       tempered_kick_drift_ref)
from tests.helpers import rng_state_words
from tests.stretch_parity import lam_of
from tests.temper_parity import LOG_Z_TWO_MODES, bits, same, two_mode_model  # noqa: F401

PRIOR_SCALE, LIK_MEAN = 1.5, 0.5  # prior N(0, 1.5^2 I), ll = -1/2 sum lam_d (x_d - 0.5)^2 (tests/temper_parity.py's model)
C1 = -(1.0 / (PRIOR_SCALE * PRIOR_SCALE))
C0 = 0.5 * C1


class HandModel:
    """A batched model whose values are sums IN d ORDER of elementwise operations and whose gradients are written by hand,
    elementwise: the same doubles from PyTorch on either device and from the chain-by-chain loop below.  split: the prior /
    likelihood pair; otherwise log_density_gradient alone (the sum of the two parts)."""

    batched = True

    def __init__(self, lam, device, split, prior_coef=C0, mean=LIK_MEAN):
        self._D = len(lam)
        self._lam = torch.as_tensor(np.asarray(lam, dtype=np.float64), device=device)
        self._c0, self._c1, self._mean = float(prior_coef), float(2.0 * prior_coef), float(mean)
        if split:
            self.log_prior_gradient, self.log_likelihood_gradient = self._prior, self._lik
            self.log_prior = lambda Th: self._prior(Th)[0]
            self.log_likelihood = lambda Th: self._lik(Th)[0]

    def dims(self):
        return self._D

    def _prior(self, Th):
        t = Th[:, 0] * Th[:, 0]
        for d in range(1, self._D):
            t = t + Th[:, d] * Th[:, d]
        return self._c0 * t, self._c1 * Th

    def _lik(self, Th):
        R = Th - self._mean
        t = self._lam[0] * (R[:, 0] * R[:, 0])
        for d in range(1, self._D):
            t = t + self._lam[d] * (R[:, d] * R[:, d])
        return -0.5 * t, -(self._lam[None, :] * R)

    def log_density_gradient(self, Th):
        (p, g0), (l, gl) = self._prior(Th), self._lik(Th)
        return p + l, g0 + gl

    def log_density(self, Th):
        return self.log_density_gradient(Th)[0]


def hand_parts(x, lam, c0=C0, mean=LIK_MEAN):
    """HandModel at one point in NumPy -> (lp0, g0, ll, gl), the same operations in the same order."""
    t = x[0] * x[0]
    for d in range(1, len(x)):
        t = t + x[d] * x[d]
    r = x - mean
    u = lam[0] * (r[0] * r[0])
    for d in range(1, len(x)):
        u = u + lam[d] * (r[d] * r[d])
    return c0 * t, (2.0 * c0) * x, -0.5 * u, -(lam * r)


def make(ops, betas, chains, replicas, D, seed=11, split=False, stepsize=0.05, steps=3, **kw):
    return bk.TemperedHMC(HandModel(lam_of(D), ops.device, split), betas, stepsize, steps, chains=chains, replicas=replicas,
                          seed=seed, ops=ops, **kw)


def run_draws(s, n):
    """-> theta [n, C, D], logp [n, C], accepted [n, C], swapped [n, C]"""
    th, lp, ac, sw = [], [], [], []
    for _ in range(n):
        t, l = s.sample()
        th.append(t.cpu().numpy().copy())
        lp.append(l.cpu().numpy().copy())
        ac.append(s.last_accept.cpu().numpy().copy())
        sw.append(s.last_swapped.cpu().numpy().copy())
    return np.stack(th), np.stack(lp), np.stack(ac), np.stack(sw)


def counters(s):
    """-> accepted proposals per rung [T], proposed and accepted swaps per pair [T - 1] (summed over replicas)."""
    R, T = s.replicas, len(s.betas)
    acc = s._rung_acc.cpu().numpy().reshape(R, T).sum(axis=0)
    prop = s._swap_prop.cpu().numpy().reshape(R, T).sum(axis=0)
    swp = s._swap_acc.cpu().numpy().reshape(R, T).sum(axis=0)
    assert prop[T - 1] == 0 and swp[T - 1] == 0  # the last rung is nobody's lower one
    return acc, prop[:T - 1], swp[:T - 1]


# ---- the scheme, written plainly: one numpy Generator per chain, chains and pairs visited one after the other -------------
def hmc_loop(betas, chains, replicas, D, draws, seed, split, stepsize, steps, swap_every=1, chain_id0=0, metric=None):
    """-> theta [draws, C, D], logp [draws, C] (untempered), final ll [C], final lp0 [C] or None, the chains' generators,
    accepted proposals per rung, proposed and accepted swaps per pair.  Not split: HandModel's log_density_gradient, the sum
    of the two parts, tempered as a whole."""
    betas = np.asarray(betas, dtype=np.float64)
    lam = lam_of(D)
    T, H = len(betas), chains
    C = replicas * T * H
    eps_t = np.full(T, float(stepsize)) if np.ndim(stepsize) == 0 else np.asarray(stepsize, dtype=np.float64)
    m = None if metric is None else np.asarray(metric, dtype=np.float64)

    def parts(x):  # -> (lp0, g0, ll, gl); not split: lp0 = 0.0, g0 = None
        p, g0, l, gl = hand_parts(x, lam)
        return (p, g0, l, gl) if split else (0.0, None, p + l, g0 + gl)

    def force(b, g0, gl):
        f = b * gl
        if g0 is not None:
            f = g0 + f
        return f if m is None else m * f

    def seq_kin(v):  # (the stand-in's momentum refresh sums in d order)
        mv, k = (v if m is None else m * v), 0.0
        for d in range(D):
            k = k + v[d] * mv[d]
        return 0.5 * k

    def quarter_kin(v):
        mv, Dq, p = (v if m is None else m * v), (D + 3) // 4, []
        for w in range(4):
            k = 0.0
            for d in range(w * Dq, min((w + 1) * Dq, D)):
                k = k + v[d] * mv[d]
            p.append(k)
        return 0.5 * (((p[0] + p[1]) + p[2]) + p[3])

    gens = [np.random.Generator(np.random.Philox(key=[seed, chain_id0 + c])) for c in range(C)]
    theta = [g.normal(size=D) for g in gens]
    cache = [parts(x) for x in theta]
    acc = np.zeros(T, dtype=np.int64)
    prop, swp = np.zeros(max(T - 1, 0), dtype=np.int64), np.zeros(max(T - 1, 0), dtype=np.int64)
    out_th, out_lp = [], []
    for it in range(1, draws + 1):
        for c in range(C):
            t = (c // H) % T
            b, eps = betas[t], eps_t[t]
            half = 0.5 * eps
            g = gens[c]
            rho = g.standard_normal(D)
            kin0 = seq_kin(rho)
            with np.errstate(divide="ignore"):
                logu = np.log(g.uniform())
            p0, g0, l0, gl = cache[c]
            f = force(b, g0, gl)
            r = rho + (-half) * f
            r = r + eps * f
            x = theta[c] + eps * r
            new = parts(x)
            for _ in range(steps - 1):
                r = r + eps * force(b, new[1], new[3])
                x = x + eps * r
                new = parts(x)
            r = r + half * force(b, new[1], new[3])
            kin1 = quarter_kin(r)
            h0 = ((p0 + b * l0) if split else b * l0) - kin0
            h1 = ((new[0] + b * new[2]) if split else b * new[2]) - kin1
            if logu < h1 - h0:
                theta[c], cache[c] = x, new
                acc[t] += 1
        if it % swap_every == 0:
            par = (it // swap_every) % 2
            for r_ in range(replicas):
                for t in range(T - 1):
                    if t % 2 != par:
                        continue
                    for i in range(H):
                        c = (r_ * T + t) * H + i
                        d = c + H
                        u = gens[c].uniform()
                        prop[t] += 1
                        with np.errstate(divide="ignore"):
                            if np.log(u) < (betas[t] - betas[t + 1]) * (cache[d][2] - cache[c][2]):
                                theta[c], theta[d] = theta[d], theta[c]
                                cache[c], cache[d] = cache[d], cache[c]
                                swp[t] += 1
        out_th.append(np.stack(theta))
        out_lp.append(np.array([v[0] + v[2] if split else v[2] for v in cache]))
    ll, lp0 = np.array([v[2] for v in cache]), np.array([v[0] for v in cache])
    return np.stack(out_th), np.stack(out_lp), ll, lp0 if split else None, gens, acc, prop, swp


def check_sampler_vs_loop(ops, betas, chains, replicas, D, draws=7, seed=11, split=False, swap_every=1, chain_id0=0,
                          stepsize=0.05, steps=3, metric=None):
    s = make(ops, betas, chains, replicas, D, seed=seed, split=split, swap_every=swap_every, chain_id0=chain_id0,
             stepsize=stepsize, steps=steps, metric_diag=metric)
    th, lp, _, sw = run_draws(s, draws)
    rth, rlp, rll, rlp0, gens, acc, prop, swp = hmc_loop(betas, chains, replicas, D, draws, seed, split, stepsize, steps,
                                                         swap_every=swap_every, chain_id0=chain_id0, metric=metric)
    assert same(th, rth) and same(lp, rlp)
    assert same(s._ll.cpu().numpy(), rll)
    assert (s._lp0 is None) if not split else same(s._lp0.cpu().numpy(), rlp0)
    assert np.array_equal(s.rng_state(), np.stack([rng_state_words(g) for g in gens], axis=1))
    got = counters(s)
    assert np.array_equal(got[0], acc) and np.array_equal(got[1], prop) and np.array_equal(got[2], swp)
    T = len(betas)
    assert np.array_equal(s.rung_accept_rate(), acc / (draws * replicas * chains))
    assert s.accept_rate() == acc.sum() / (draws * replicas * T * chains)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(s.swap_rate(), np.where(prop > 0, swp / np.maximum(prop, 1), np.nan), equal_nan=True)
    # the cached gradients followed the state through accepts and swaps
    m = HandModel(lam_of(D), ops.device, split)
    if split:
        assert same(s._g_ll.cpu().numpy(), m._lik(s._theta)[1].t().cpu().numpy())
        assert same(s._g_lp0.cpu().numpy(), m._prior(s._theta)[1].t().cpu().numpy())
    else:
        assert same(s._g_ll.cpu().numpy(), m.log_density_gradient(s._theta)[1].t().cpu().numpy())
    return s


def check_one_rung_is_hmc(ops, C, D, draws=6, seed=11, stepsize=0.02, steps=3):
    """TemperedHMC(m, [1.0], eps) == HMCDiag(m, eps, path="opaque"): theta of every draw and the accept masks."""
    t = bk.TemperedHMC(bk.DiagGaussian(lam_of(D), ops=ops), [1.0], stepsize, steps, chains=C, seed=seed, ops=ops)
    h = bk.HMCDiag(bk.DiagGaussian(lam_of(D), ops=ops), stepsize, steps, seed=seed, chains=C, path="opaque", ops=ops)
    seen = 0
    for _ in range(draws):
        (a, _), (b, _) = t.sample(), h.sample()
        assert same(a.cpu().numpy(), b.cpu().numpy())
        assert np.array_equal(t.last_accept.cpu().numpy(), h.last_accept.cpu().numpy())
        assert not t.last_swapped.any()
        seen += int(t.last_accept.sum())
    assert np.array_equal(t.rng_state(), h.rng_state())
    assert 0 < seen < draws * C  # (the step size of this check accepts and refuses)
    assert t.swap_rate().shape == (0,)


def check_sampler_vs_stand_in(ops, chains, T, replicas, D, draws=6, seed=11, split=False, warm=30):
    """The sampler on `ops` against the sampler on the NumPy stand-in, bit for bit: the warmup reports, then theta, logp, ll,
    masks, swaps, streams and counters of `draws` draws."""
    betas = np.geomspace(1.0, 0.05, T)
    eps = 0.05 / np.sqrt(betas)
    s = make(ops, betas, chains, replicas, D, seed=seed, split=split, stepsize=eps, steps=3)
    f = make(TemperHmcFakeOps(), betas, chains, replicas, D, seed=seed, split=split, stepsize=eps, steps=3)
    assert same(s._theta.cpu().numpy(), f._theta.numpy())
    if warm:
        ra, rb = s.warmup(warm), f.warmup(warm)
        assert ra == rb
        assert same(s.stepsizes, f.stepsizes) and not np.array_equal(s.stepsizes, eps)
    th, lp, ac, sw = run_draws(s, draws)
    fth, flp, fac, fsw = run_draws(f, draws)
    assert np.array_equal(ac, fac) and np.array_equal(sw, fsw)
    assert same(th, fth) and same(lp, flp)
    assert same(s._ll.cpu().numpy(), f._ll.numpy())
    assert np.array_equal(s.rng_state(), f.rng_state())
    for a, b in zip(counters(s), counters(f)):
        assert np.array_equal(a, b)
    assert s.accept_rate() == f.accept_rate()
    np.testing.assert_allclose(s.mean_log_likelihood(), f.mean_log_likelihood(), rtol=1e-11)
    assert sw.any() and not sw.all() and ac.any() and not ac.all()  # (these shapes swap and refuse, accept and refuse)


def check_state_round_trip(ops, betas, chains, replicas, D, seed=11, split=True):
    """A checkpoint taken after 3 draws with swap_every = 2 continues bit for bit, the parity of the next swap round
    included, in a sampler built with other streams and other step sizes; the statistics travel with it."""
    eps = 0.05 / np.sqrt(np.asarray(betas))
    s = make(ops, betas, chains, replicas, D, seed=seed, split=split, swap_every=2, stepsize=eps)
    run_draws(s, 3)
    sd = s.state_dict()
    a = run_draws(s, 5)
    r = make(ops, betas, chains, replicas, D, seed=seed + 1, split=split, swap_every=2, stepsize=0.5)
    r.load_state_dict(sd)
    assert same(r.stepsizes, eps)
    b = run_draws(r, 5)
    for x, y in zip(a, b):
        assert same(x, y)
    assert a[3][0].any() != a[3][1].any()  # (swap rounds after draws 4, 6, 8: every other one of the continued draws)
    assert np.array_equal(s.rng_state(), r.rng_state())
    for x, y in zip(counters(s), counters(r)):
        assert np.array_equal(x, y)
    assert s.accept_rate() == r.accept_rate()
    assert same(s.mean_log_likelihood(), r.mean_log_likelihood())
    assert same(s._lse.cpu().numpy(), r._lse.cpu().numpy())
    return sd


def check_warmup_repeats_and_continues(ops, betas, chains, replicas, D, draws=12, seed=11, split=True):
    """warmup gives the same report twice (two samplers of the same seed), changes every rung's step size, resets the
    statistics, and a checkpoint taken after it continues bit for bit."""
    a = make(ops, betas, chains, replicas, D, seed=seed, split=split, stepsize=0.3)
    b = make(ops, betas, chains, replicas, D, seed=seed, split=split, stepsize=0.3)
    ra, rb = a.warmup(draws), b.warmup(draws)
    assert ra == rb and len(ra["eps"]) == draws and len(ra["alpha"]) == draws and len(ra["stepsizes"]) == len(betas)
    assert np.array_equal(a.stepsizes, ra["stepsizes"]) and np.all(a.stepsizes != 0.3)
    assert all(0.0 <= x <= 1.0 and (x * replicas * chains) == round(x * replicas * chains) for row in ra["alpha"] for x in row)
    assert np.isnan(a.accept_rate()) and a._draws == draws
    sd = a.state_dict()
    c = make(ops, betas, chains, replicas, D, seed=seed + 3, split=split, stepsize=0.3)
    c.load_state_dict(sd)
    for x, y in zip(run_draws(a, 4), run_draws(c, 4)):
        assert same(x, y)
    return ra


# ---- the kernels alone -------------------------------------------------------------------------------------------------
def ladder(T, zero=False):
    b = np.linspace(1.0, 0.2, T)
    if zero:
        b[-1] = 0.0
    return b


def column_rungs(H, T, replicas):
    return np.repeat(np.arange(replicas * T) % T, H)


def _array(g, D, C, pad, off, dev):
    """A [D, C] array of normals as a view of a NaN-filled [D, off + C + pad] device array (off = 1: 8-byte aligned only)
    -> (host array [D, C], the whole device tensor, the view)."""
    x = g.normal(size=(D, C))
    full = np.full((D, off + C + pad), np.nan)
    full[:, off:off + C] = x
    t = torch.from_numpy(full).to(dev)
    return x, t, (t[:, off:off + C] if (pad or off) else t)


def _vector(x, dev, fill=123.0):
    """x on the device between two guard elements -> (the whole tensor, its view of x)."""
    full = np.concatenate([np.full(2, fill, dtype=x.dtype), x, np.full(2, fill, dtype=x.dtype)])
    t = torch.from_numpy(full).to(dev)
    return t, t[2:2 + len(x)]


def _padding_untouched(full, C, off):
    a = full.cpu().numpy()
    return np.isnan(a[:, :off]).all() and np.isnan(a[:, off + C:]).all()


def check_integrator_kernels(ops, H, T, replicas, D, pad=0, off=0, use_lp0=True, use_metric=True, use_pre=True,
                             use_kick=True, in_place=False, zero_times_inf=False):
    """ops.tempered_kick_drift and ops.tempered_finish against their restatements, bit for bit; the NaN pitch padding and
    the vectors' guards untouched; inputs of an out-of-place call untouched."""
    C = replicas * T * H
    g = np.random.default_rng([11, H, T, replicas, D, pad, off, int(use_lp0), int(use_metric), int(use_pre), int(use_kick),
                               int(in_place), int(zero_times_inf)])
    dev = ops.device
    rung = column_rungs(H, T, replicas)
    beta = ladder(T, zero=zero_times_inf)[rung]
    eps = 0.05 + 0.01 * rung + 0.001 * g.uniform(size=C)  # (a step size per column: the kernels know no rungs)
    th, th_full, t_th = _array(g, D, C, pad, off, dev)
    rho, rho_full, t_rho = _array(g, D, C, pad, off, dev)
    gl, gl_full, t_gl = _array(g, D, C, pad + 2, off, dev)  # (the gradients have a pitch of their own)
    g0, g0_full, t_g0 = _array(g, D, C, pad + 2, off, dev)
    if zero_times_inf:  # beta = 0 against an infinite gradient entry: 0 * inf, IEEE decides
        hot = np.flatnonzero(beta == 0.0)
        gl[0, hot[0]] = np.inf
        gl[D - 1, hot[-1]] = -np.inf
        t_gl.copy_(torch.from_numpy(gl).to(dev))
    metric = 0.5 + g.uniform(size=D)
    f_beta, t_beta = _vector(beta, dev)
    f_eps, t_eps = _vector(eps, dev)
    f_pre, t_pre = _vector(-(0.5 * eps), dev)
    f_half, t_half = _vector(0.5 * eps, dev)
    if off:  # the vectors 8-byte aligned only, like the arrays
        f_beta, f_eps, f_pre, f_half = (torch.cat([v[:1], v]) for v in (f_beta, f_eps, f_pre, f_half))
        t_beta, t_eps, t_pre, t_half = (v[3:3 + C] for v in (f_beta, f_eps, f_pre, f_half))
    t_m = torch.from_numpy(metric).to(dev) if use_metric else None
    a_g0, a_m = (g0 if use_lp0 else None), (metric if use_metric else None)
    a_pre, a_kick = (-(0.5 * eps) if use_pre else None), (eps if use_kick else None)

    r_th, r_rho = tempered_kick_drift_ref(th, rho, gl, a_g0, a_m, beta, eps, a_pre, a_kick)
    if in_place:
        o_th_full, o_th, o_rho_full, o_rho = th_full, t_th, rho_full, t_rho
    else:
        _, o_th_full, o_th = _array(g, D, C, pad, off, dev)
        _, o_rho_full, o_rho = _array(g, D, C, pad, off, dev)
    ops.tempered_kick_drift(t_th, o_th, t_rho, o_rho, t_gl, t_g0 if use_lp0 else None, t_m, t_beta, t_eps,
                            t_pre if use_pre else None, t_eps if use_kick else None)
    assert same(o_th.cpu().numpy(), r_th) and same(o_rho.cpu().numpy(), r_rho)
    for full in (o_th_full, o_rho_full, th_full, rho_full):
        assert _padding_untouched(full, C, off)
    if not in_place:
        assert same(t_th.cpu().numpy(), th) and same(t_rho.cpu().numpy(), rho)
    assert same(t_gl.cpu().numpy(), gl) and same(t_g0.cpu().numpy(), g0)
    if zero_times_inf:
        assert np.isnan(r_rho[0, hot[0]]) and np.isnan(r_rho[D - 1, hot[-1]]) and np.isfinite(r_rho[:, beta > 0]).all()

    # finish: from the same inputs (rho as it was), with and without rho_out; grad_ll None: the kinetic energy alone
    if in_place:
        t_rho.copy_(torch.from_numpy(rho).to(dev))
    src = t_rho
    f_kin, t_kin = _vector(np.full(C, 7.0), dev)
    if off:
        f_kin = torch.cat([f_kin[:1], f_kin])
        t_kin = f_kin[3:3 + C]
    r_r, r_kin = tempered_finish_ref(rho, gl, a_g0, a_m, beta, 0.5 * eps)
    _, out_full, out = _array(g, D, C, pad, off, dev)
    want_out = (D + H) % 2 == 0
    ops.tempered_finish(src, out if want_out else None, t_gl, t_g0 if use_lp0 else None, t_m, t_beta, t_half, t_kin)
    assert same(t_kin.cpu().numpy(), r_kin)
    if want_out:
        assert same(out.cpu().numpy(), r_r)
    assert _padding_untouched(out_full, C, off) and same(src.cpu().numpy(), rho)
    guards = f_kin.cpu().numpy()
    assert np.all(guards[:len(guards) - C - 2] == 123.0) and np.all(guards[-2:] == 123.0)
    _, k_kin = tempered_finish_ref(rho, None, None, a_m, None, None)
    ops.tempered_finish(src, None, None, None, t_m, None, None, t_kin)
    assert same(t_kin.cpu().numpy(), k_kin)
    for v, x in ((f_beta, beta), (f_eps, eps)):
        h = v.cpu().numpy()
        assert same(h[len(h) - C - 2:-2], x) and np.all(h[-2:] == 123.0)


def check_degenerate_equality(ops, C, D):
    """beta = 1, uniform vectors, no lp0: bk_tempered_kick_drift and bk_tempered_finish equal ops.kick_drift and
    ops.leapfrog_finish bit for bit (first step, later step, with and without a metric, in place and not)."""
    g = np.random.default_rng([12, C, D])
    dev = ops.device
    eps, half = 0.037, 0.5 * 0.037
    one, e, h, nh = (torch.full((C,), v, dtype=torch.float64, device=dev) for v in (1.0, eps, half, -half))
    th, rho, gr = (torch.from_numpy(g.normal(size=(D, C))).to(dev) for _ in range(3))
    metric = torch.from_numpy(0.5 + g.uniform(size=D)).to(dev)
    for m in (None, metric):
        for first in (True, False):
            a_th, a_rho, b_th, b_rho = th.clone(), rho.clone(), th.clone(), rho.clone()
            ops.kick_drift(a_th, a_th, a_rho, a_rho, gr, m, eps, first, -half, True, eps)
            ops.tempered_kick_drift(b_th, b_th, b_rho, b_rho, gr, None, m, one, e, nh if first else None, e)
            assert same(a_th.cpu().numpy(), b_th.cpu().numpy()) and same(a_rho.cpu().numpy(), b_rho.cpu().numpy())
            o_th, o_rho, p_th, p_rho = (torch.empty_like(th) for _ in range(4))
            ops.kick_drift(th, o_th, rho, o_rho, gr, m, eps, first, -half, True, eps)
            ops.tempered_kick_drift(th, p_th, rho, p_rho, gr, None, m, one, e, nh if first else None, e)
            assert same(o_th.cpu().numpy(), p_th.cpu().numpy()) and same(o_rho.cpu().numpy(), p_rho.cpu().numpy())
        k0, k1 = torch.zeros(C, dtype=torch.float64, device=dev), torch.zeros(C, dtype=torch.float64, device=dev)
        r0, r1 = torch.empty_like(rho), torch.empty_like(rho)
        ops.leapfrog_finish(rho, r0, gr, m, half, False, k0)
        ops.tempered_finish(rho, r1, gr, None, m, one, h, k1)
        assert same(k0.cpu().numpy(), k1.cpu().numpy()) and same(r0.cpu().numpy(), r1.cpu().numpy())
        ops.leapfrog_finish(rho, None, None, m, 0.0, False, k0)
        ops.tempered_finish(rho, None, None, None, m, None, None, k1)
        assert same(k0.cpu().numpy(), k1.cpu().numpy())


LOG_U_MODES = ("random", "-inf", "0", "+inf", "nan")


def check_accept_kernel(ops, H, T, replicas, off=0, mode="random", special=False, use_lp0=True):
    """ops.tempered_hmc_accept against tempered_hmc_accept_ref: mask, ll, lp0 and the per-block counts exact; nothing
    written outside the n columns.  special: -inf, +inf and NaN in ll with a beta = 0 rung."""
    E = replicas * T
    n = E * H
    g = np.random.default_rng([13, H, T, replicas, off, LOG_U_MODES.index(mode), int(special), int(use_lp0)])
    beta = ladder(T, zero=special)[np.repeat(np.arange(E) % T, H)]
    ll, llp, lp0, lp0p = (2.0 * g.normal(size=n) for _ in range(4))
    kin0, kin1 = g.chisquare(3, size=n), g.chisquare(3, size=n)
    if special:
        for v in (ll, llp):
            v[g.uniform(size=n) < 0.15] = -np.inf
            v[g.uniform(size=n) < 0.08] = np.nan
            v[g.uniform(size=n) < 0.08] = np.inf
        ll[n - 1] = np.inf  # (the last block is the beta = 0 rung)
    log_u = {"random": np.log(g.uniform(size=n)), "-inf": np.full(n, -np.inf), "0": np.zeros(n), "+inf": np.full(n, np.inf),
             "nan": np.full(n, np.nan)}[mode]
    r_mask, r_ll, r_lp0, r_cnt = tempered_hmc_accept_ref(ll, lp0 if use_lp0 else None, kin0, llp, lp0p if use_lp0 else None,
                                                         kin1, beta, log_u, H)
    dev = ops.device

    def put(x, fill):
        full = np.concatenate([np.full(off, fill, dtype=x.dtype), x, np.full(1, fill, dtype=x.dtype)])
        t = torch.from_numpy(full).to(dev)
        return t, t[off:off + n]

    f_ll, t_ll = put(ll, 77.0)
    f_lp0, t_lp0 = put(lp0, 77.0)
    f_mask, t_mask = put(np.full(n, 9, dtype=np.uint8), 9)
    t_llp, t_lp0p, t_beta, t_k0, t_k1, t_u = (put(v, 0.0)[1] for v in (llp, lp0p, beta, kin0, kin1, log_u))
    t_cnt = torch.full((E + 1,), 3, dtype=torch.int32, device=dev)
    ops.tempered_hmc_accept(t_ll, t_lp0 if use_lp0 else None, t_k0, t_llp, t_lp0p if use_lp0 else None, t_k1, t_beta, t_u,
                            t_mask, t_cnt[:E], H)
    g_ll, g_lp0, g_mask, cnt = (v.cpu().numpy() for v in (f_ll, f_lp0, f_mask, t_cnt))
    assert np.array_equal(g_mask[off:off + n], r_mask) and np.all(g_mask[:off] == 9) and g_mask[off + n] == 9
    assert same(g_ll[off:off + n], r_ll) and np.all(g_ll[:off] == 77.0) and g_ll[off + n] == 77.0
    assert same(g_lp0[off:off + n], r_lp0 if use_lp0 else lp0) and g_lp0[off + n] == 77.0
    assert np.array_equal(cnt[:E], 3 + r_cnt.astype(np.int64)) and cnt[E] == 3
    assert r_cnt.sum() == r_mask.sum()
    if mode == "-inf" and not special:
        assert r_mask.all()
    if mode in ("+inf", "nan"):
        assert not r_mask.any()
    if special:  # a beta = 0 rung with an infinite ll: 0 * inf is NaN, refused whatever log u is
        bad = (beta == 0.0) & (np.isinf(ll) | np.isinf(llp) | np.isnan(ll) | np.isnan(llp))
        assert bad[n - 1] and not r_mask[bad].any()
    if not use_lp0 and not special:  # at beta = 1 without lp0 the test is bk_mh_accept(BK_ACCEPT_HMC)'s
        one = beta == 1.0
        with np.errstate(invalid="ignore"):
            assert np.array_equal(r_mask[one] != 0, (log_u < (llp - kin1) - (ll - kin0))[one])


def check_exchange_kernel(ops, H, T, replicas, D, pad=0):
    """ops.exchange_columns on an array against what ops.replica_swap did to theta2 under the same `swapped`, and against
    exchange_columns_ref; the NaN padding untouched; a second application gives the original back."""
    C = replicas * T * H
    g = np.random.default_rng([14, H, T, replicas, D, pad])
    dev = ops.device
    rung = column_rungs(H, T, replicas)
    beta = torch.from_numpy(ladder(T)[rung]).to(dev)
    lower = torch.from_numpy(((rung % 2 == 0) & (rung + 1 < T)).astype(np.uint8)).to(dev)
    _, th_full, t_th = _array(g, D, C, pad, 0, dev)
    x, x_full, t_x = _array(g, D, C, pad, 0, dev)
    _, y_full, t_y = _array(g, D, C, pad, 0, dev)
    t_y.copy_(t_x)
    ll = torch.from_numpy(3.0 * g.normal(size=C)).to(dev)
    log_u = torch.from_numpy(np.log(g.uniform(size=C))).to(dev)
    swapped = torch.full((C,), 9, dtype=torch.uint8, device=dev)
    ops.replica_swap(t_th, t_x, ll, None, beta, log_u, lower, swapped, None, None, H)
    sw = swapped.cpu().numpy()
    assert C < 128 or (sw.any() and not sw[lower.cpu().numpy() != 0].all())
    ops.exchange_columns(t_y, swapped, H)
    assert same(t_y.cpu().numpy(), t_x.cpu().numpy()) and same(t_y.cpu().numpy(), exchange_columns_ref(x, sw, H))
    assert _padding_untouched(y_full, C, 0)
    ops.exchange_columns(t_y, swapped, H)
    assert same(t_y.cpu().numpy(), x)


def check_kernels(ops, H, T):
    """The grid of the kernel checks for one (H, T): replicas 1 and 2; D in (1, 3, 4, 5, 33): ragged row blocks and empty
    quarters of the kinetic sum; pitch pads 0 and 6 (even) and 5 (odd) and a view that is 8-byte aligned only, so that both
    forms run (with odd H the two columns of a 16-byte lane lie on different rungs); grad_lp0, metric, pre and kick each
    present and NULL; in place and out of place; 0 * inf; the accept test with every kind of log u and of ll."""
    for replicas in (1, 2):
        for D in (1, 3, 4, 5, 33):
            for pad, off in ((0, 0), (6, 0), (5, 0), (6, 1)):
                k = D + pad + off
                check_integrator_kernels(ops, H, T, replicas, D, pad=pad, off=off, use_lp0=k % 2 == 0, use_metric=k % 3 != 0,
                                         in_place=(k // 2) % 2 == 0)
        for flags in ((True, False), (False, True), (False, False)):
            check_integrator_kernels(ops, H, T, replicas, 5, pad=6, use_pre=flags[0], use_kick=flags[1])
        for lp0, metric, in_place in ((True, True, True), (False, False, False), (True, False, False), (False, True, True)):
            check_integrator_kernels(ops, H, T, replicas, 33, use_lp0=lp0, use_metric=metric, in_place=in_place)
        check_integrator_kernels(ops, H, T, replicas, 5, pad=6, zero_times_inf=True)
        check_integrator_kernels(ops, H, T, replicas, 4, pad=5, zero_times_inf=True, use_lp0=False)
        for off in (0, 1):
            for mode in LOG_U_MODES:
                for use_lp0 in (True, False):
                    check_accept_kernel(ops, H, T, replicas, off, mode=mode, use_lp0=use_lp0)
            check_accept_kernel(ops, H, T, replicas, off, special=True)
            check_accept_kernel(ops, H, T, replicas, off, mode="-inf", special=True, use_lp0=False)


# ---- statistical runs ----------------------------------------------------------------------------------------------------
RUNG_BETAS = bk.geometric_ladder(5, 1e-2, zero=True)
RUNG_STEPS = 5


def rung_precisions(betas=RUNG_BETAS):
    """The conjugate Gaussian of tests/temper_parity.py::run_rung_moments: D = 3, prior N(0, 2^2 I), ll = -1/2 |theta - 2|^2
    / 0.25; rung t is N(4 beta_t 2 / p_t, 1 / p_t) with p_t = 1/4 + 4 beta_t."""
    return 0.25 + 4.0 * np.asarray(betas)


def rung_model(device):
    """That model with hand-written gradients: prior coefficient -1/8, lam = 4, mean 2."""
    return HandModel(np.full(3, 4.0), device, True, prior_coef=-0.125, mean=2.0)


def rung_parts_np(X):
    """rung_model on a NumPy [n, 3] batch -> (lp0, g0, ll, gl)."""
    R = X - 2.0
    return -0.125 * (X * X).sum(axis=1), -0.25 * X, -2.0 * (R * R).sum(axis=1), -4.0 * R


def two_mode_parts_np(X):
    """tests/temper_parity.py::two_mode_model on a NumPy [n, 2] batch -> (lp0, g0, ll, gl)."""
    c_prior, c_lik = -np.log(2.0 * np.pi * 16.0), -np.log(2.0 * np.pi * 0.25)
    a = np.log(0.3) + c_lik - 2.0 * ((X + 3.0) ** 2).sum(axis=1)
    b = np.log(0.7) + c_lik - 2.0 * ((X - 3.0) ** 2).sum(axis=1)
    ll = np.logaddexp(a, b)
    wa, wb = np.exp(a - ll), np.exp(b - ll)
    gl = wa[:, None] * (-4.0 * (X + 3.0)) + wb[:, None] * (-4.0 * (X - 3.0))
    return c_prior - (X * X).sum(axis=1) / 32.0, -X / 16.0, ll, gl


def two_mode_stepsizes(betas):
    """0.45 standard deviations of a mode of rung t: local precision 4 beta_t + 1/16."""
    return 0.45 / np.sqrt(4.0 * np.asarray(betas) + 1.0 / 16.0)


class SchemeNumpy:
    """The scheme of TemperedHMC for one replica, vectorised over the chains with ONE NumPy generator: the same moves and
    tests in the same order, other random numbers.  What the bounds of the statistical GPU tests were derived from."""

    def __init__(self, parts, betas, H, eps, steps, init, seed, target_accept=0.8):
        self.parts, self.betas, self.H, self.steps = parts, np.asarray(betas, dtype=np.float64), H, steps
        self.T = len(self.betas)
        self.g = np.random.default_rng(seed)
        self.rung = np.repeat(np.arange(self.T), H)
        self.beta = self.betas[self.rung]
        self.set_eps(eps)
        self.x = np.array(init, dtype=np.float64)
        self.cache = self.parts(self.x)
        self.n = 0
        self.reset()

    def set_eps(self, eps):
        self.eps_t = np.full(self.T, float(eps)) if np.ndim(eps) == 0 else np.asarray(eps, dtype=np.float64)
        self.eps = self.eps_t[self.rung][:, None]

    def reset(self):
        self.acc = np.zeros(self.T)
        self.prop, self.swp = np.zeros(self.T - 1), np.zeros(self.T - 1)
        self.lse = np.full(self.T, -np.inf)
        self.stat_n = 0

    def force(self, c):
        return c[1] + self.beta[:, None] * c[3]

    def draw(self):
        C, D = self.x.shape
        rho = self.g.standard_normal((C, D))
        kin0 = 0.5 * (rho * rho).sum(axis=1)
        logu = np.log(self.g.uniform(size=C))
        p0, _, l0, _ = self.cache
        r = rho + 0.5 * self.eps * self.force(self.cache)
        x = self.x + self.eps * r
        new = self.parts(x)
        for _ in range(self.steps - 1):
            r = r + self.eps * self.force(new)
            x = x + self.eps * r
            new = self.parts(x)
        r = r + 0.5 * self.eps * self.force(new)
        kin1 = 0.5 * (r * r).sum(axis=1)
        with np.errstate(invalid="ignore"):
            ok = logu < ((new[0] + self.beta * new[2]) - kin1) - ((p0 + self.beta * l0) - kin0)
        self.x = np.where(ok[:, None], x, self.x)
        self.cache = tuple(np.where(ok[:, None] if a.ndim == 2 else ok, a, b) for a, b in zip(new, self.cache))
        counts = ok.reshape(self.T, self.H).sum(axis=1)
        self.acc += counts
        self.n += 1
        par, H = self.n % 2, self.H
        ll = self.cache[2]
        for t in range(par, self.T - 1, 2):
            lo = np.arange(t * H, (t + 1) * H)
            hi = lo + H
            with np.errstate(invalid="ignore"):
                sw = np.log(self.g.uniform(size=H)) < (self.betas[t] - self.betas[t + 1]) * (ll[hi] - ll[lo])
            a, b = lo[sw], hi[sw]
            self.x[a], self.x[b] = self.x[b].copy(), self.x[a].copy()
            self.cache = tuple(self._swap(v, a, b) for v in self.cache)
            ll = self.cache[2]
            self.prop[t] += H
            self.swp[t] += sw.sum()
        db = np.concatenate([[0.0], self.betas[:-1] - self.betas[1:]])
        w = (self.cache[2] * db[self.rung]).reshape(self.T, H)
        mx = w.max(axis=1)
        self.lse = np.logaddexp(self.lse, mx + np.log(np.exp(w - mx[:, None]).sum(axis=1)))
        self.stat_n += 1
        return counts

    @staticmethod
    def _swap(v, a, b):
        v = v.copy()
        v[a], v[b] = v[b].copy(), v[a].copy()
        return v

    def warmup(self, draws, target=0.8):
        das = [bk.adapt.DualAveraging(float(e), target) for e in self.eps_t]
        for it in range(draws):
            counts = self.draw()
            nxt = [da.step(float(c) / self.H) for da, c in zip(das, counts)]
            if it + 1 == draws:
                nxt = [da.final() for da in das]
            self.set_eps(nxt)
        self.reset()

    def log_evidence(self):
        return float((self.lse[1:] - np.log(self.stat_n * self.H)).sum())


def rung_errors(pool, rung, betas=RUNG_BETAS):
    """pool [draws, C, 3] -> (max_t |mean error| / sd, max_t |var ratio - 1|)"""
    mean_err, var_err = 0.0, 0.0
    for t, b in enumerate(betas):
        prec = 0.25 + 4.0 * b
        x = pool[:, rung == t, :].reshape(-1, pool.shape[2])
        mean_err = max(mean_err, np.abs(x.mean(axis=0) - 4.0 * b * 2.0 / prec).max() * np.sqrt(prec))
        var_err = max(var_err, np.abs(x.var(axis=0) * prec - 1.0).max())
    return mean_err, var_err


def run_rung_moments(ops, seed=2025, chains=256):
    """The conjugate Gaussian, betas = geomspace(1, 1e-2, 5) then 0, `chains` chains per rung, default init, step size 0.35
    standard deviations of each rung, 5 steps, 300 draws, the first 100 dropped -> (max_t |mean error| / sd, max_t |var
    ratio - 1|, the sampler)"""
    eps = 0.35 / np.sqrt(rung_precisions())
    s = bk.TemperedHMC(rung_model(ops.device), RUNG_BETAS, eps, RUNG_STEPS, chains=chains, seed=seed, ops=ops)
    for _ in range(100):
        s.sample()
    pool = torch.stack([s.sample()[0] for _ in range(200)]).cpu().numpy()
    mean_err, var_err = rung_errors(pool, s.rung_index().cpu().numpy())
    return mean_err, var_err, s


def scheme_rung_moments(seed, chains=256):
    eps = 0.35 / np.sqrt(rung_precisions())
    T = len(RUNG_BETAS)
    sc = SchemeNumpy(rung_parts_np, RUNG_BETAS, chains, eps, RUNG_STEPS, np.random.default_rng([seed, 1]).normal(
        size=(T * chains, 3)), seed)
    for _ in range(100):
        sc.draw()
    pool = []
    for _ in range(200):
        sc.draw()
        pool.append(sc.x.copy())
    return rung_errors(np.stack(pool), sc.rung)


TWO_MODE_BETAS = bk.geometric_ladder(11, 1e-3, zero=True)
TWO_MODE_STEPS = 4


def run_two_modes(ops, seed=2025, chains=256, draws=400):
    """12 rungs (geomspace(1, 1e-3, 11) then 0) of `chains` chains, every chain started at (-3, -3) + 0.3 N(0, I) (the minor
    mode), `draws` draws, reset_statistics() after half of them -> (share of the cold chains of the second half's draws with
    theta[0] > 0, log_evidence() of the one replica, swap_rate(), the same share for a plain HMCDiag from the cold chains'
    start with the cold rung's step size)"""
    model = two_mode_model()
    betas = TWO_MODE_BETAS
    eps = two_mode_stepsizes(betas)
    C = len(betas) * chains
    init = -3.0 + 0.3 * np.random.default_rng(seed).normal(size=(C, 2))
    s = bk.TemperedHMC(model, betas, eps, TWO_MODE_STEPS, init=init, chains=chains, seed=seed, ops=ops)
    cold = s.cold_rows()
    for _ in range(draws // 2):
        s.sample()
    s.reset_statistics()
    share = float(torch.stack([s.sample()[0][cold, 0] > 0 for _ in range(draws - draws // 2)]).double().mean().item())
    p = bk.HMCDiag(model, float(eps[0]), TWO_MODE_STEPS, init=init[cold.cpu().numpy()], seed=seed, chains=chains,
                   path="opaque", ops=ops)
    for _ in range(draws // 2):
        p.sample()
    plain = float(torch.stack([p.sample()[0][:, 0] > 0 for _ in range(draws - draws // 2)]).double().mean().item())
    return share, float(s.log_evidence()[0]), s.swap_rate(), plain


def scheme_two_modes(seed, chains=256, draws=400):
    betas = TWO_MODE_BETAS
    C = len(betas) * chains
    init = -3.0 + 0.3 * np.random.default_rng(seed).normal(size=(C, 2))
    sc = SchemeNumpy(two_mode_parts_np, betas, chains, two_mode_stepsizes(betas), TWO_MODE_STEPS, init, [seed, 2])
    for _ in range(draws // 2):
        sc.draw()
    sc.reset()
    hits = []
    for _ in range(draws - draws // 2):
        sc.draw()
        hits.append(sc.x[:chains, 0] > 0)
    return float(np.mean(hits)), sc.log_evidence(), sc.swp / sc.prop


WARMUP_STEPS = 1  # (one frequency per rung: with more steps the energy error of a trajectory vanishes at resonant step sizes,
#                    the acceptance is not monotone in the step size and the averaged iterate is not where the last ones are)


def run_warmup_band(ops, seed=2025, chains=256, target=0.8):
    """warmup(150) on the conjugate Gaussian with one leapfrog step from a step size of 0.35 standard deviations, then 100
    draws -> (every rung's acceptance over those, the sampler)"""
    eps = 0.35 / np.sqrt(rung_precisions())
    s = bk.TemperedHMC(rung_model(ops.device), RUNG_BETAS, eps, WARMUP_STEPS, chains=chains, seed=seed, ops=ops)
    s.warmup(150, target_accept=target)
    for _ in range(100):
        s.sample()
    return s.rung_accept_rate(), s


def scheme_warmup_band(seed, chains=256, target=0.8):
    eps = 0.35 / np.sqrt(rung_precisions())
    T = len(RUNG_BETAS)
    sc = SchemeNumpy(rung_parts_np, RUNG_BETAS, chains, eps, WARMUP_STEPS, np.random.default_rng([seed, 1]).normal(
        size=(T * chains, 3)), [seed, 3])
    sc.warmup(150, target)
    for _ in range(100):
        sc.draw()
    return sc.acc / (100 * chains), sc.eps_t
