"""The diagnostic kernels of csrc/bk_diag.hip at their launch seams and fallbacks -- shared test bodies (GPU:
tests/test_gpu_diag_kernels.py on the HIP library; CPU: tests/test_diag_kernels_cpu.py on tests/fake_ops.FakeOps, which
exercises these bodies, their references and their bounds without a device).

Every body calls the ``ops.*`` entry point itself.  Every output is a view of a wider / longer buffer pre-filled with NaN,
and whatever the contract leaves alone must still be NaN afterwards.  References are exact (math.fsum, fractions.Fraction,
Python integers), mpmath at 50 digits, or oracle/diagnostics.py at the tolerances the project already holds these kernels
to; every other bound is derived from the number of rounded operations (u = 2^-53), never from what a device returned.
Each check prints the largest err / bound it saw (``pytest -s``; the largest per check: profiles/diag_kernel_edges.md)."""
import math
import time
from fractions import Fraction

import numpy as np
import torch

import bayes_kit_amd as bk
from oracle import diagnostics as od

U = 2.0 ** -53
NAN = float("nan")
F64 = torch.float64
POISON = 1e300  # behind a chain's length / beside an input's columns: a read past the end cannot hide


def say(what, value, unit="max err/bound"):
    print(f"[diag-kernels] {what}: {unit} = {value:.3g}" if isinstance(value, float) else f"[diag-kernels] {what}: {value}")


def ratio_of(err, bound, what):
    """max err / bound, asserting err <= bound componentwise (a zero bound asks for a zero error)."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert np.all(np.isfinite(err)), (what, "non-finite error")
    bad = err > bound
    assert not bad.any(), (what, "worst err / bound", float(np.max(err[bad] / np.maximum(bound[bad], 1e-320))),
                           "cells over", int(bad.sum()), "first", tuple(np.argwhere(bad)[0]))
    pos = bound > 0
    return float(np.max(err[pos] / bound[pos])) if pos.any() else 0.0


def dev(a, ops, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(ops.device)


class Slack:
    """A [R, C] view -- `off` columns in, R of R + extra rows -- of a [R + extra, off + C + pad] buffer filled with `fill`."""

    def __init__(self, ops, R, C, pad=3, extra=1, off=0, fill=NAN, data=None):
        self.buf = torch.full((R + extra, off + C + pad), fill, dtype=F64, device=ops.device)
        self.t = self.buf[:R, off:off + C]
        self.R, self.C, self.off, self.fill = R, C, off, fill
        if data is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(data, dtype=np.float64)))

    def take(self, what=""):
        """The view's values; asserts that every cell outside the view still holds the fill."""
        out = self.t.cpu().numpy().copy()
        probe = self.buf.clone()
        probe[:self.R, self.off:self.off + self.C] = self.fill
        same = torch.isnan(probe) if self.fill != self.fill else probe == self.fill
        assert bool(same.all()), f"a write outside the [R, C] view ({what})"
        return out


class SlackVec:
    """The first n entries of a NaN-filled vector of n + 3."""

    def __init__(self, ops, n, dtype=F64):
        self.n = n
        if dtype == F64:
            self.buf = torch.full((n + 3,), NAN, dtype=F64, device=ops.device)
        else:
            self.buf = torch.full((n + 3,), -77, dtype=dtype, device=ops.device)
        self.t = self.buf[:n]

    def take(self, what=""):
        tail = self.buf[self.n:]
        ok = torch.isnan(tail).all() if self.buf.dtype == F64 else (tail == -77).all()
        assert bool(ok), f"a write behind the vector ({what})"
        return self.t.cpu().numpy().copy()


# =====================================================================================================================
# 1. ops.ess / ops.autocorr: group seams, the 64 KiB branch, the one-lane fallback
# =====================================================================================================================
# ess_tile_launch's constants, restated
ET_RT_MIN_DRAWS, ET_RT_TAIL = 288, 72         # register tiles from 288 draws on, followed by 72 zeros in LDS
ET_CAP = (160 * 1024 - 512) // 8              # doubles of LDS one workgroup may take: 20,416
ET_CAP2 = 78 * 1024 // 8                      # ... when two workgroups are to share a CU: 9,984
ET_OPT_IN = 64 * 1024                         # tiles above this need hipFuncSetAttribute
PC_BLOCK = 64                                 # workgroup of the one-lane-per-chain kernels
GROUPS = (16, 8, 4, 2, 1)
PHIS = (-0.6, 0.0, 0.5, 0.9, 0.98, 0.999)


def ess_pitch(N):
    return ((N + ET_RT_TAIL) if N >= ET_RT_MIN_DRAWS else N) | 1


def ess_group(N):
    """(G, LDS bytes) ess_tile_launch stages N draws with; (0, 0): the one-lane-per-chain kernels serve."""
    p = ess_pitch(N)
    for cap in (ET_CAP2, ET_CAP):
        for g in GROUPS:
            if g * p <= cap:
                return g, g * p * 8
    return 0, 0


def _last_n(limit):
    return max(N for N in range(ET_RT_MIN_DRAWS, 2 * ET_CAP) if ess_pitch(N) <= limit)


def _band_mid(g):
    band = [N for N in range(4, ET_CAP2) if ess_group(N)[0] == g and ess_group(N)[1] > ET_OPT_IN]
    return band[len(band) // 2]


ESS_SEAMS = []
for _g in GROUPS:
    _n = _last_n(ET_CAP2 // _g)   # the last N whose G = _g tile leaves room for a second workgroup on the CU
    ESS_SEAMS += [_n, _n + 1]
ESS_SEAM_WIDE = _last_n(ET_CAP // 2)      # the last N that runs G = 2 with the CU to itself (from 9,912 on); then G = 1
ESS_BANDS = [_band_mid(_g) for _g in GROUPS]  # one N per G whose tile is over 64 KiB (the opt-in branch, per instance)
ESS_LAST_TILE = _last_n(ET_CAP)           # the last N one chain of which fits: 20,343; from 20,344 on k_ess / k_autocorr
ESS_FALLBACK = [ESS_LAST_TILE + 1, 40_000]
ESS_N = sorted(set(ESS_SEAMS + [ESS_SEAM_WIDE, ESS_SEAM_WIDE + 1] + ESS_BANDS + [ESS_LAST_TILE] + ESS_FALLBACK))
AUTOCORR_N = [n for n in ESS_N if n != 40_000]  # (k_autocorr is O(N^2) per lane: one fallback size)

# a changed constant shows up here, not as a silently moved seam
assert ESS_SEAMS == [551, 552, 1175, 1176, 2423, 2424, 4919, 4920, 9911, 9912], ESS_SEAMS
assert (ESS_LAST_TILE, ESS_FALLBACK[0]) == (20_343, 20_344)
assert [ess_group(n)[0] for n in ESS_SEAMS] == [16, 8, 8, 4, 4, 2, 2, 1, 1, 2]
assert [ess_group(n)[0] for n in (ESS_SEAM_WIDE, ESS_SEAM_WIDE + 1, 20_343, 20_344)] == [2, 1, 1, 0]
assert all(lo <= n <= hi for n, (lo, hi) in zip(ESS_BANDS, ((440, 551), (952, 1175), (1976, 2423), (4024, 4919), (8120, 9911))))
assert all(ess_group(n) == (g, g * ess_pitch(n) * 8) and g * ess_pitch(n) * 8 > ET_OPT_IN for n, g in zip(ESS_BANDS, GROUPS))
assert ess_group(9912)[1] > ET_OPT_IN and ess_group(20_343)[1] > ET_OPT_IN and ess_group(551)[1] > ET_OPT_IN


def ess_chain_counts(N):
    """1, G - 1, G + 1 and a ragged last workgroup; the one-lane kernels: 1, 3 and one lane past a PC_BLOCK workgroup.
    G = 1 also gets 7 chains: chain 5 is the first with phi = 0.999, whose lag loop runs over the most blocks."""
    G = ess_group(N)[0]
    if G == 0:
        return [1, 3, PC_BLOCK + 1]
    return sorted(({1, G - 1, G + 1, 2 * G + 3} | ({len(PHIS) + 1} if G == 1 else set())) - {0})


ESS_CASES = [(N, C) for N in ESS_N for C in ess_chain_counts(N)]
# k_autocorr is O(N^2) per lane (2.07e8 terms at N = 20,344) whatever the chain count: its measured time at 1 and at 65
# chains is in profiles/diag_kernel_edges.md, and all three chain counts of the one-lane launch stay
AUTOCORR_CASES = [(N, C) for N in AUTOCORR_N for C in ess_chain_counts(N)]
# seeds replaced because a chain's truncation pair sat on a near-zero sum: {(N, C): seed}
ESS_REPLACED_SEEDS = {}
PAIR_MARGIN = 1e-9


def ar1_series(N, C, seed=0):
    """[N, C] AR(1) series, chain c with persistence PHIS[c % 6] (the inputs of test_lds_staged_ess_and_autocorr_vs_oracle)."""
    from scipy.signal import lfilter

    rng = np.random.default_rng([N, C, ESS_REPLACED_SEEDS.get((N, C), seed)])
    x = np.empty((N, C))
    for c in range(C):
        x[:, c] = lfilter([1.0], [1.0, -PHIS[c % len(PHIS)]], rng.normal(size=N))
    return x


def scan_margin(acor):
    """Smallest |pair sum| over the pairs the Geyer scan tests up to and including the one it stops at: a sum within
    rounding of zero could stop one formulation a pair earlier than the other."""
    N = len(acor)
    n, m = 0, np.inf
    while n + 1 < N:
        p = acor[n] + acor[n + 1]
        m = min(m, abs(p))
        if p < 0:
            break
        n += 2
    return m


def direct_pair_sum_ld(x, n):
    """acor[n] + acor[n + 1] by direct lag sums in long double (autocorr.py:23-33 without the FFT)."""
    x = np.asarray(x, dtype=np.longdouble)
    N = len(x)
    xc = x - x.sum() / N
    q = (xc * xc).sum()
    return float(((xc[:N - n] * xc[n:]).sum() + (xc[:N - n - 1] * xc[n + 1:]).sum()) / q)


def check_ess(ops, N, C):
    """ops.ess, both estimators, ess_out and iat_out, on a [:, :C] view of a wider buffer, against the oracle."""
    x = ar1_series(N, C)
    xs = Slack(ops, N, C, fill=POISON, data=x)
    acor = [od.autocorr(x[:, c]) for c in range(C)]
    margin = min(scan_margin(a) for a in acor)
    assert margin > PAIR_MARGIN, ("a truncation pair within 1e-9 of zero: replace the seed (ESS_REPLACED_SEEDS)", N, C, margin)
    worst = 0.0
    for est, oiat in ((0, od.iat_imse), (1, od.iat_ipse)):
        e, i = SlackVec(ops, C), SlackVec(ops, C)
        ops.ess(xs.t, est, e.t, i.t)
        got_e, got_i = e.take("ess_out"), i.take("iat_out")
        want_i = np.array([oiat(x[:, c]) for c in range(C)])
        want_e = N / want_i
        np.testing.assert_allclose(got_i, want_i, rtol=1e-9, err_msg=f"iat, estimator {est}")
        np.testing.assert_allclose(got_e, want_e, rtol=1e-9, err_msg=f"ess, estimator {est}")
        worst = max(worst, float(np.max(np.abs(got_i / want_i - 1.0))), float(np.max(np.abs(got_e / want_e - 1.0))))
        e2 = SlackVec(ops, C)
        ops.ess(xs.t, est, e2.t, None)  # iat_out is optional
        assert np.array_equal(e2.take("ess_out alone"), got_e)
    say(f"ess N={N} C={C} G={ess_group(N)[0]}", worst / 1e-9)
    return worst / 1e-9


def check_autocorr(ops, N, C, timed=False):
    """ops.autocorr (all lags) into a [:N, :C] view of a wider, taller NaN buffer, against the oracle at atol 1e-12."""
    x = ar1_series(N, C)
    xs = Slack(ops, N, C, fill=POISON, data=x)
    out = Slack(ops, N, C, pad=5, extra=2)
    t0 = time.perf_counter()
    ops.autocorr(xs.t, out.t)
    got = out.take("autocorr")
    dt = time.perf_counter() - t0
    worst = 0.0
    for c in range(C):
        want = od.autocorr(x[:, c])
        np.testing.assert_allclose(got[:, c], want, rtol=0, atol=1e-12, err_msg=f"chain {c}")
        worst = max(worst, float(np.max(np.abs(got[:, c] - want))))
    say(f"autocorr N={N} C={C} G={ess_group(N)[0]}", worst / 1e-12)
    if timed:
        say(f"autocorr N={N} C={C} launch to host copy", dt, "seconds")
    return worst / 1e-12


def check_hand_over(ops, C=3):
    """The tile kernel at N = 20,343 and the one-lane kernel at N = 20,344 on series that share their first 20,343 draws:
    autocorrelations at lags 0..63 within 2e-12 of each other (both are held to the oracle at 1e-12).  The extra draw of
    the longer series is the mean of the first 20,343: its centred value is zero (to rounding), so every lag sum and the
    sum of squares are those of the shorter series, and acor = a / (q / N) / N does not depend on N but for roundings.
    (Any other last draw moves every autocorrelation by O(1 / N) = 5e-5 and the two kernels could not be compared.)"""
    N1 = ESS_LAST_TILE
    assert ess_group(N1)[0] == 1 and ess_group(N1 + 1)[0] == 0
    x = np.empty((N1 + 1, C))
    x[:N1] = ar1_series(N1, C, seed=5)
    x[N1] = [math.fsum(x[:N1, c]) / N1 for c in range(C)]
    a = Slack(ops, N1, C, fill=POISON, data=x[:N1])
    b = Slack(ops, N1 + 1, C, fill=POISON, data=x)
    oa, ob = Slack(ops, N1, C), Slack(ops, N1 + 1, C)
    ops.autocorr(a.t, oa.t)
    ops.autocorr(b.t, ob.t)
    ga, gb = oa.take("tile"), ob.take("one lane")
    d = float(np.max(np.abs(ga[:64] - gb[:64])))
    say("tile (N=20343) against one-lane (N=20344) autocorrelation, lags 0..63", d / 2e-12)
    assert d <= 2e-12, d
    return d / 2e-12


# =====================================================================================================================
# 2. ops.chain_mean_var
# =====================================================================================================================
CMV_N = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 1000, 4001)
CMV_C = (1, 63, 64, 65, 130, 4097)
CMV_LARGE = (1000, 65_536)
CMV_DATA = ("normal", "offset", "scales")
CMV_EXACT_CELLS = 70_000  # above this many draws the exact reference takes a subset of the chains (edges + a random few)


def cmv_data(kind, N, C, seed=0):
    rng = np.random.default_rng([N, C, seed, CMV_DATA.index(kind)])
    z = rng.normal(size=(N, C))
    if kind == "offset":    # a mean that is large against the spread
        z += 1e6 * (1.0 + rng.uniform(size=C))
    elif kind == "scales":  # 1e-150 and 1e150 side by side in adjacent chains
        z *= np.where(np.arange(C) % 2 == 0, 1e-150, 1e150)
    return z


def cmv_lengths(N, C, need_var, seed=1):
    """Per chain one of {2, 3, N, N - 1, ceil(N / 2)}, at least 2 wherever the variance is requested, never above N."""
    rng = np.random.default_rng([N, C, seed])
    lo = 2 if need_var else 1
    choices = np.clip(np.array([2, 3, N, N - 1, -(-N // 2)]), min(lo, N), N)
    return choices[rng.integers(0, 5, size=C)].astype(np.int32)


def exact_int_scaled(col):
    """Python integers m_i and an exponent e with col[i] = m_i * 2**e exactly."""
    mant, ex = np.frexp(col)
    m = (mant * 2.0 ** 53).astype(np.int64)
    e0 = int(ex.min())
    return [int(a) << (int(b) - e0) for a, b in zip(m, ex)], e0 - 53


def exact_mean_var(col):
    """(mean, sum (x - mean)^2 / (n - 1)) of a float64 column as Fractions (variance None for n = 1); the sum of the
    draws also through math.fsum, which must round the same integer sum."""
    n = len(col)
    ints, e = exact_int_scaled(np.asarray(col, dtype=np.float64))
    scale = Fraction(2) ** e
    S = sum(ints)
    assert float(S * scale) == math.fsum(col)
    mean = Fraction(S, n) * scale
    if n < 2:
        return mean, None
    Q = Fraction(sum(v * v for v in ints)) - Fraction(S * S, n)  # sum (x - mean)^2 = sum x^2 - S^2 / n, exactly
    return mean, Q * scale * scale / (n - 1)


def cmv_bounds(n, sum_abs, var_exact):
    """|mean - exact| <= delta = k u sum|x| / n and |var - exact| <= (k + 6) u exact + n / (n - 1) delta^2, with
    k = ceil(n / 4) + 4, from k_chain_mean_var operation by operation:
      ceil(n / 4)  a lane-wave's sequential sum of its every-fourth draws (one rounding per addition, first order);
      + 3          the three combining additions ((p0 + p1) + p2) + p3;
      + 1          the division by n (mean) or n - 1 (variance);
    and for the variance, per term, + 2 for the subtraction x - mu (its relative error enters the square twice), + 1 for
    the square, with 3 to spare for the second order: (k + 6) u.  The mean the second pass centres on is off by at most
    delta, and sum (x - m)^2 = sum (x - mu)^2 + n (mu - m)^2: hence n / (n - 1) delta^2."""
    k = -(-n // 4) + 4
    delta = k * U * sum_abs / n
    if n < 2:
        return delta, None
    return delta, (k + 6) * U * var_exact + n / (n - 1.0) * delta * delta


def cmv_reference(x, lengths, chains):
    """Exact mean / variance of chains `chains` (their first lengths[c] draws) and the bounds: float64 arrays
    (mean, var, mean_bound, var_bound), var entries NaN where n = 1."""
    out = np.full((4, len(chains)), np.nan)
    for j, c in enumerate(chains):
        col = x[:lengths[c], c]
        mu, var = exact_mean_var(col)
        db, vb = cmv_bounds(len(col), math.fsum(np.abs(col)), float(var) if var is not None else None)
        out[0, j], out[2, j] = float(mu), db
        if var is not None:
            out[1, j], out[3, j] = float(var), vb
        # (float(Fraction) rounds once: half an ulp of the reference, against bounds of five ulps and more)
    return out


def cmv_chains(N, C, seed=2):
    if N * C <= CMV_EXACT_CELLS:
        return np.arange(C)
    edge = [c for c in (0, 1, 62, 63, 64, 65, 127, 128, C - 65, C - 64, C - 2, C - 1) if 0 <= c < C]
    rnd = np.random.default_rng([N, C, seed]).integers(0, C, size=24)
    return np.unique(np.concatenate([edge, rnd]))


def cmv_longdouble(x, lengths):
    """Mean and variance of every chain in long double (pairwise sums: error (log2 n + 2) 2^-64 of sum|x|), for the
    chains the exact reference does not visit; -> (mean, var, sum|x|) as float64."""
    N, C = x.shape
    mean, var, sabs = np.empty(C), np.empty(C), np.empty(C)
    for c0 in range(0, C, 4096):
        blk = x[:, c0:c0 + 4096].astype(np.longdouble)
        n = lengths[c0:c0 + 4096].astype(np.longdouble)
        live = np.arange(N)[:, None] < lengths[None, c0:c0 + 4096]
        blk = np.where(live, blk, np.longdouble(0))
        mu = blk.sum(axis=0) / n
        d = np.where(live, blk - mu, np.longdouble(0))
        mean[c0:c0 + 4096] = mu
        with np.errstate(invalid="ignore", divide="ignore"):
            var[c0:c0 + 4096] = (d * d).sum(axis=0) / (n - 1)
        sabs[c0:c0 + 4096] = np.abs(blk).sum(axis=0)
    return mean, var, sabs


def check_chain_mean_var(ops, N, C, kinds=CMV_DATA, ragged_modes=(False, True)):
    worst_m = worst_v = 0.0
    need_var = N >= 2
    for kind in kinds:
        x = cmv_data(kind, N, C)
        for ragged in ragged_modes:
            lengths = cmv_lengths(N, C, need_var) if ragged else np.full(C, N, dtype=np.int32)
            xp = x.copy()
            xp[np.arange(N)[:, None] >= lengths[None, :]] = POISON  # rows past a chain's length
            xs = Slack(ops, N, C, fill=POISON, data=xp)
            mean, var = SlackVec(ops, C), SlackVec(ops, C)
            ops.chain_mean_var(xs.t, dev(lengths, ops, np.int32) if ragged else None, mean.t, var.t if need_var else None)
            gm = mean.take("mean")
            gv = var.take("var") if need_var else None
            if not need_var:
                assert bool(torch.isnan(var.buf).all()), "var=None, yet something was written"
            chains = cmv_chains(N, C)
            ref = cmv_reference(xp, lengths, chains)
            what = f"N={N} C={C} {kind} ragged={ragged}"
            worst_m = max(worst_m, ratio_of(np.abs(gm[chains] - ref[0]), ref[2], "mean " + what))
            if need_var:
                worst_v = max(worst_v, ratio_of(np.abs(gv[chains] - ref[1]), ref[3], "var " + what))
            if len(chains) < C:
                # every chain, against long double: the same bounds plus the long-double sums' own error
                lm, lv, sabs = cmv_longdouble(xp, lengths)
                n = lengths.astype(np.float64)
                rerr = (np.log2(n) + 2.0) * 2.0 ** -64
                bm, bv = np.empty(C), np.empty(C)
                for c in range(C):
                    bm[c], bv[c] = cmv_bounds(int(lengths[c]), sabs[c], lv[c])
                worst_m = max(worst_m, ratio_of(np.abs(gm - lm), bm + rerr * sabs / n, "mean, all chains " + what))
                worst_v = max(worst_v, ratio_of(np.abs(gv - lv), bv + 8 * rerr * lv, "var, all chains " + what))
    say(f"chain_mean_var N={N} C={C} mean", worst_m)
    say(f"chain_mean_var N={N} C={C} var", worst_v)
    return worst_m, worst_v


# =====================================================================================================================
# 3. ops.rhat_partials
# =====================================================================================================================
RP_D = (1, 3, 130)
RP_C = (1, 2, 255, 256, 257, 1000, 65_537)
RP_N = (2, 1000)


def two_square(d):
    """(hi, lo) with hi + lo = d * d exactly (Dekker's split; no overflow or underflow at these magnitudes)."""
    hi = d * d
    s = d * 134217729.0
    a = s - (s - d)
    b = d - a
    lo = ((a * a - hi) + 2.0 * a * b) + b * b
    return hi, lo


def rp_inputs(D, C, n, seed=0):
    """Per-chain means with a common offset of 1e6 against a between-chain sd of 1e-3 (where the centred second pass
    matters) and M2 of chains whose own sd is about 1e-3, so that neither term of R-hat drowns the other."""
    rng = np.random.default_rng([D, C, n, seed])
    mean = 1e6 + 1e-3 * rng.normal(size=(D, C))
    m2 = (n - 1) * 1e-6 * (1.0 + 0.1 * rng.normal(size=(D, C))) ** 2
    return mean, m2


def rp_bound(C, sum_abs):
    """(ceil(C / 256) + 8 + 3) u sum|term|: a thread's sequential additions of its every-256th chain, the eight levels of
    the LDS tree, and the per-term roundings (division or subtraction, square, and one to spare)."""
    return (-(-C // 256) + 8 + 3) * U * sum_abs


def check_rhat_partials(ops, D, C, n):
    mean, m2 = rp_inputs(D, C, n)
    ms, qs = Slack(ops, D, C, fill=POISON, data=mean), Slack(ops, D, C, fill=POISON, data=m2)
    centre = np.array([math.fsum(mean[d]) / C for d in range(D)])
    term1 = m2 / float(n - 1)  # rounded once, as the kernel divides before it adds
    dv = mean - centre[:, None]
    assert np.array_equal(dv.astype(np.longdouble), mean.astype(np.longdouble) - centre[:, None].astype(np.longdouble))
    hi, lo = two_square(dv)   # (mu - centre)^2 exactly: the difference is exact (asserted), the square split in two
    want = np.empty((3, D))
    bound = np.empty((3, D))
    for d in range(D):
        want[0, d], bound[0, d] = math.fsum(mean[d]), rp_bound(C, math.fsum(np.abs(mean[d])))
        want[1, d], bound[1, d] = math.fsum(term1[d]), rp_bound(C, math.fsum(term1[d]))
        want[2, d] = math.fsum(np.concatenate([hi[d], lo[d]]))
        bound[2, d] = rp_bound(C, want[2, d])
    worst = 0.0
    for with_centre in (False, True):
        out = SlackVec(ops, 3 * D + 1)
        ops.rhat_partials(ms.t, qs.t, n, dev(centre, ops) if with_centre else None, out.t)
        got = out.take("rhat_partials")
        assert np.isnan(got[3 * D]), "out[3D] belongs to the caller"
        rows = 3 if with_centre else 2
        if not with_centre:
            assert np.isnan(got[2 * D:3 * D]).all(), "out[2D:3D] is written only with a centre"
        worst = max(worst, ratio_of(np.abs(got[:rows * D].reshape(rows, D) - want[:rows]), bound[:rows],
                                    f"rhat_partials D={D} C={C} n={n} centre={with_centre}"))
    ms.take("mean"), qs.take("m2")
    say(f"rhat_partials D={D} C={C} n={n}", worst)
    if C >= 2:
        # rhat.py:163-171 and the pooled variance from the same moments, in Fractions
        rhat = bk.diagnostics.rhat_from_moments(ms.t, qs.t, n, ops)
        pooled = bk.diagnostics.pooled_variance_from_moments(ms.t, qs.t, n, ops).cpu().numpy()
        for d in range(D):
            mu = [Fraction(v) for v in mean[d]] if C <= 1000 else None
            if mu is not None:
                gm = sum(mu) / C
                vm = sum((v - gm) ** 2 for v in mu) / (C - 1)
                mv = sum(Fraction(v) for v in m2[d]) / (n - 1) / C
            else:  # (65,537 chains: the same sums through fsum, correctly rounded, about the rounded centre)
                shift = Fraction(math.fsum(mean[d])) / C - Fraction(centre[d])  # (exact to half an ulp of the sum)
                vm = (Fraction(want[2, d]) - C * shift * shift) / (C - 1)
                mv = Fraction(math.fsum(m2[d])) / (n - 1) / C
            want_r = math.sqrt(Fraction(n - 1, n) + vm / mv)
            want_p = float(Fraction(n - 1, n) * mv + vm)
            np.testing.assert_allclose(rhat[d], want_r, rtol=1e-12, err_msg=f"rhat d={d}")
            np.testing.assert_allclose(pooled[d], want_p, rtol=1e-12, err_msg=f"pooled variance d={d}")
    return worst


# =====================================================================================================================
# 4. ops.welford_update / ops.welford_update_dev
# =====================================================================================================================
WF_STEPS = 40
WF_BASE_C = 4097  # the draws of chain c are built from column c % 4097 of a [D, 4097] table per step
WF_SHAPES = {
    # name: (C, D, column offset of the moment views, theta's extra pitch, through the device count)
    "even": (4096, 7, 0, 0, False),          # (i)   two chains per lane, D % 4 = 3
    "odd": (4097, 5, 0, 0, False),           # (ii)  odd C: scalar
    "misaligned": (4096, 7, 1, 0, False),    # (iii) buf[:, 1:1+C]: pointers off 16 bytes: scalar
    "theta_pitch": (4096, 6, 0, 5, False),   # (iv)  theta with its own larger, odd row pitch: scalar
    "past_llc": (65_536, 132, 0, 0, False),  # (v)   3 C D 8 = 207.6 MB > 192 MiB: two chains per lane, non-temporal
    "even_dev": (4096, 7, 0, 0, True),       # (vi)  (i) with the count in a device int64 and a nonzero offset
    "odd_dev": (4097, 5, 0, 0, True),        #       (ii) likewise
}
WF_BRANCH = {"even": "v2", "odd": "scalar", "misaligned": "scalar", "theta_pitch": "scalar", "past_llc": "v2_nt",
             "even_dev": "v2", "odd_dev": "scalar"}
WF_DEV_OFFSET = 7


def _aligned16(t):
    return t.data_ptr() % 16 == 0


def _pitch(t):
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def welford_branch(mean, m2, theta):
    """welford_launch's choice, restated: bkw::v2_applies (csrc/bk_welford.hpp) and bk_streams_past_llc (bk_common.hpp)."""
    D, C = theta.shape
    v2 = (C % 2 == 0 and _pitch(mean) % 2 == 0 and _pitch(theta) % 2 == 0 and _aligned16(mean) and _aligned16(m2)
          and _aligned16(theta))
    if not v2:
        return "scalar"
    return "v2_nt" if 3 * C * D * 8 > (192 << 20) else "v2"


def wf_tables(C, D, seed=0):
    rng = np.random.default_rng([seed, 99])
    off = 1e6 * rng.uniform(-1.0, 1.0, size=65_536)[:C]      # per-chain offsets up to 1e6
    scale = 0.5 + 1.5 * rng.uniform(size=65_536)[:C]
    return off, scale, np.arange(C) % WF_BASE_C


def wf_draw(t, C, D, tables, seed=0):
    """Draw t of every shape: chain c, row d holds the same double in every shape that has them."""
    off, scale, idx = tables
    z = np.random.default_rng([seed, 100, t]).normal(size=(132, WF_BASE_C))[:D]
    return z[:, idx] * scale + off


def wf_exact(xs):
    """xs [n, ...] -> exact (mean, M2) as float64 arrays rounded once from Fractions."""
    n = xs.shape[0]
    flat = xs.reshape(n, -1)
    mean, m2 = np.empty(flat.shape[1]), np.empty(flat.shape[1])
    for j in range(flat.shape[1]):
        mu, var = exact_mean_var(flat[:, j])
        mean[j], m2[j] = float(mu), float(var * (n - 1))
    return mean.reshape(xs.shape[1:]), m2.reshape(xs.shape[1:])


def wf_subset(C):
    edge = [c for c in (0, 1, 2, 3, 254, 255, 256, 257, 510, 511, 512, 513, 4094, 4095, 4096, C - 2, C - 1) if c < C]
    return np.unique(np.concatenate([edge, np.random.default_rng(C).integers(0, C, size=16)]))


def run_welford(ops, name, steps=WF_STEPS):
    """-> (mean, m2, numpy recurrence mean, m2, exact mean, m2 on the chain subset, subset, max|x| per cell)"""
    C, D, coff, th_pad, on_dev = WF_SHAPES[name]
    pad = 2  # (the moments' pitch stays even: only the shape's own feature sends it to the scalar kernel)
    mean, m2 = Slack(ops, D, C, pad=pad - coff, extra=2, off=coff), Slack(ops, D, C, pad=pad - coff, extra=2, off=coff)
    theta = Slack(ops, D, C, pad=pad - coff + th_pad, extra=1, off=coff, fill=POISON)
    mean.t.zero_(), m2.t.zero_()
    assert welford_branch(mean.t, m2.t, theta.t) == WF_BRANCH[name], (name, welford_branch(mean.t, m2.t, theta.t))
    tables = wf_tables(C, D)
    sub = wf_subset(C)
    kept = np.empty((steps, D, len(sub)))
    mu, q, big = np.zeros((D, C)), np.zeros((D, C)), np.zeros((D, C))
    n_dev = torch.zeros(1, dtype=torch.int64, device=ops.device)
    for t in range(steps):
        x = wf_draw(t, C, D, tables)
        kept[t] = x[:, sub]
        theta.t.copy_(torch.from_numpy(x))
        if on_dev:
            n_dev.fill_(t + 1 + WF_DEV_OFFSET)
            ops.welford_update_dev(mean.t, m2.t, theta.t, n_dev, WF_DEV_OFFSET)
        else:
            ops.welford_update(mean.t, m2.t, theta.t, t + 1)
        delta = x - mu                      # welford_elem, csrc/bk_welford.hpp
        mu = mu + delta / float(t + 1)
        q = q + delta * (x - mu)
        np.maximum(big, np.abs(x), out=big)
    theta.take("theta")
    return mean.take(name + " mean"), m2.take(name + " m2"), mu, q, *wf_exact(kept), sub, big


def check_welford(ops, name, steps=WF_STEPS):
    gm, gq, mu, q, em, eq, sub, big = run_welford(ops, name, steps)
    # the float64 restatement, at the tolerances of test_cfg4_spec_length_sequence_vs_oracle
    tol_m, tol_q = 1e-13 * big, 1e-13 * steps * big * big
    r1 = ratio_of(np.abs(gm - mu), tol_m, name + ": mean against the float64 recurrence")
    r2 = ratio_of(np.abs(gq - q), tol_q, name + ": M2 against the float64 recurrence")
    # against the exact moments: four times the recurrence's own error (each of its roundings may move under an fma
    # contraction) plus the tolerances above
    np_m, np_q = np.abs(mu[:, sub] - em), np.abs(q[:, sub] - eq)
    r3 = ratio_of(np.abs(gm[:, sub] - em), 4 * np_m.max() + tol_m[:, sub], name + ": mean against the exact mean")
    r4 = ratio_of(np.abs(gq[:, sub] - eq), 4 * np_q.max() + tol_q[:, sub], name + ": M2 against the exact M2")
    say(f"welford {name} [{WF_BRANCH[name]}] against the recurrence (mean, M2)", max(r1, r2))
    say(f"welford {name} against the exact moments (mean, M2)", max(r3, r4))
    say(f"welford {name} recurrence's own error: mean {np_m.max():.3g} (of |x| {float((np_m / big[:, sub]).max()):.3g}), "
        f"M2 {np_q.max():.3g} (of n |x|^2 {float((np_q / (steps * big[:, sub] ** 2)).max()):.3g})", "")
    return gm, gq, mu, q


def ulp_distance(a, b):
    """Largest distance in units in the last place between two float64 arrays of one sign pattern."""
    ia, ib = np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64)
    return int(np.max(np.abs(ia - ib))) if a.size else 0


def check_welford_three_kernels(ops, steps=WF_STEPS):
    """Shapes (i), (iii) and (v) -- two chains per lane, scalar, non-temporal -- run the same arithmetic on the same data
    on the chains and rows they share.  The library is built with -ffp-contract=off and none of the three kernels holds a
    contracted multiply-add (the only v_fma_f64 in their disassembly belong to the division's expansion, the same in all
    three), so the results must be the same bits -- and those of the float64 NumPy recurrence."""
    res = {name: check_welford(ops, name, steps) for name in ("even", "misaligned", "past_llc")}
    C, D = WF_SHAPES["even"][:2]
    worst = 0
    for name in ("misaligned", "past_llc"):
        for k, what in ((0, "mean"), (1, "M2")):
            a, b = res["even"][k], res[name][k][:D, :C]
            d = ulp_distance(a, b)
            worst = max(worst, d)
            say(f"welford even against {name}, {what}", "bit-identical" if d == 0 else f"largest distance {d} ulp")
    d_np = max(ulp_distance(res["even"][0], res["even"][2]), ulp_distance(res["even"][1], res["even"][3]))
    say("welford even against the float64 recurrence", "bit-identical" if d_np == 0 else f"largest distance {d_np} ulp")
    assert worst == 0, f"the three Welford kernels differ by up to {worst} ulp on the same data"
    return worst, d_np


# =====================================================================================================================
# 5. ops.rank_normalize
# =====================================================================================================================
RN_S = (2.0, 7.0, 4096.0, 1e7, 1e15, 4e15)
EXPM2 = 0.13533528323661269189  # bk_ndtri's branch constant


def rn_p(rank, S):
    """The double the kernel forms (rhat.py:104-107; 0.325 as implemented there)."""
    with np.errstate(invalid="ignore"):
        return (np.asarray(rank, dtype=np.float64) - 0.325) / (S - 0.25)


def _ranks_around(S, p_target, steps=6):
    """Ranks (fractional) whose p lies within a few ulps of p_target on both sides, and the integer ranks either side."""
    r0 = p_target * (S - 0.25) + 0.325
    out = [math.floor(r0), math.floor(r0) + 1.0]
    lo = hi = r0
    for _ in range(steps):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [float(lo), float(hi)]
    return out + [float(r0)]


def rn_inputs():
    """-> list of (S, ranks array): the five ranks per S, both sides of both branch boundaries, deep-tail ranks, a
    10,000-point sweep at S = 1e7 and the specials p = 0, p = 1, NaN."""
    cases = []
    for S in RN_S:
        r = [1.0, 2.0, float(S // 2), S - 1.0, S]
        if S >= 7:
            r += _ranks_around(S, EXPM2) + _ranks_around(S, 1.0 - EXPM2)
        if S == 4e15:
            r += [0.325 + 2.0 ** -k for k in (10, 30, 53)]      # p down to 1.4e-32: sqrt(-2 ln p) = 12
        # p = 0 -> -inf; p = 1 -> +inf (the rank next to S + 0.075 whose p is exactly one); NaN -> NaN
        one = S + 0.075
        near = [float(one)]
        for _ in range(4):
            near += [float(np.nextafter(min(near), -np.inf)), float(np.nextafter(max(near), np.inf))]
        ones = [v for v in near if rn_p(v, S) == 1.0]
        r += [0.325, NAN] + ones[:1]
        if S == 1e7:
            r += list(np.arange(1.0, 2501.0)) + list(S - np.arange(0.0, 2500.0)) + list(np.round(np.linspace(2501, S - 2500, 5000)))
        r = np.array(r)
        p = rn_p(r, S)
        keep = ~(p > 1.0) & ~(p < 0.0)  # (bayes_kit never forms a p outside [0, 1])
        cases.append((S, r[keep]))
    return cases


def rn_reference(p):
    """sqrt(2) erfinv(2 p - 1) at 50 digits for every double p, rounded once; -inf, +inf and NaN at p = 0, p = 1, NaN."""
    import mpmath as mp

    mp.mp.dps = 50
    out = np.empty(len(p))
    for i, v in enumerate(p):
        if v != v:
            out[i] = NAN
        elif v <= 0.0:
            out[i] = -np.inf
        elif v >= 1.0:
            out[i] = np.inf
        else:
            out[i] = float(mp.sqrt(2) * mp.erfinv(2 * mp.mpf(float(v)) - 1))
    return out


def rn_branch(p):
    """0: central rational, 1: tail with sqrt(-2 ln p) < 8, 2: tail with sqrt(-2 ln p) >= 8, -1: special."""
    with np.errstate(invalid="ignore", divide="ignore"):
        y = np.where(p > 1.0 - EXPM2, 1.0 - p, p)
        x = np.sqrt(-2.0 * np.log(y))
        b = np.where(y > EXPM2, 0, np.where(x < 8.0, 1, 2))
    return np.where((p > 0.0) & (p < 1.0), b, -1)


def rn_rel_err(got, want):
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.abs(got - want) / np.abs(want)
    e[(got == want) | (np.isnan(got) & np.isnan(want))] = 0.0
    return e


_RN_CACHE = {}


def rn_problem():
    """All inputs, their p, the 50-digit reference, SciPy's ndtri error against it, and the kernel's bound."""
    if not _RN_CACHE:
        import scipy.special

        cases = rn_inputs()
        p = np.concatenate([rn_p(r, S) for S, r in cases])
        want = rn_reference(p)
        with np.errstate(invalid="ignore"):
            sp_err = rn_rel_err(scipy.special.ndtri(p), want)
        br = rn_branch(p)
        assert (br == 2).sum() >= 8 and (br == 1).sum() >= 1000 and (br == 0).sum() >= 1000
        assert ((p > 0) & (np.sqrt(-2 * np.log(np.where(p > 0, p, 1.0))) >= 8.0)).any()       # the x >= 8 branch, below
        assert ((p < 1) & (np.sqrt(-2 * np.log1p(-np.where(p < 1, p, 0.0))) >= 8.0)).any()    # ... and above
        assert (p == 0).any() and (p == 1).any() and np.isnan(p).any()
        for e in (EXPM2, 1.0 - EXPM2):  # both sides of both boundaries, and the boundary itself
            assert (p == e).any() and (p == np.nextafter(e, 0)).any() and (p == np.nextafter(e, 1)).any(), e
        _RN_CACHE.update(cases=cases, want=want, sp_err=sp_err, branch=br, p=p)
    return _RN_CACHE


def check_rank_normalize(ops):
    """The kernel's bound: four times SciPy's largest relative error against mpmath on these very inputs, plus 4 u (the
    device's log and sqrt are not libm's, and the tail branches are differences of two terms)."""
    pb = rn_problem()
    sp_max = float(pb["sp_err"].max())
    assert sp_max < 1e-15, sp_max  # the inputs sit where the reference implementation itself is good
    bound = 4 * sp_max + 4 * U
    got = []
    for S, r in pb["cases"]:
        out = SlackVec(ops, len(r))
        ops.rank_normalize(dev(r, ops), S, out.t)
        got.append(out.take(f"rank_normalize S={S}"))
    got = np.concatenate(got)
    want, br = pb["want"], pb["branch"]
    special = br < 0
    assert np.array_equal(got[special], want[special], equal_nan=True), (got[special], want[special])
    err = rn_rel_err(got, want)
    for b, name in ((0, "central"), (1, "tail x < 8"), (2, "tail x >= 8")):
        say(f"rank_normalize {name}: {int((br == b).sum())} points, SciPy ndtri max rel err {pb['sp_err'][br == b].max():.3g}, "
            f"kernel max rel err {err[br == b].max():.3g}", "")
    worst = ratio_of(err[~special], np.full((~special).sum(), bound), "rank_normalize against mpmath")
    say(f"rank_normalize (bound {bound:.3g} = 4 x {sp_max:.3g} + 4 u)", worst)
    # n across a workgroup of 256: the first n points of the S = 1e7 sweep
    S, r = next(c for c in pb["cases"] if c[0] == 1e7)
    first = sum(len(c[1]) for c in pb["cases"][:RN_S.index(1e7)])
    for n in (255, 256, 257):
        out = SlackVec(ops, n)
        ops.rank_normalize(dev(r[:n], ops), S, out.t)
        assert np.array_equal(out.take(f"rank_normalize n={n}"), got[first:first + n], equal_nan=True), n
    return worst


def check_rank_normalize_six_values(ops):
    """The regression guard of tests/test_gpu_kernels.py, kept: rtol 1e-14 against scipy.stats.norm.ppf at six values."""
    import scipy.stats

    S = 1000.0
    r = np.array([1.0, 10.0, 500.0, 501.0, 990.0, 1000.0])
    out = SlackVec(ops, 6)
    ops.rank_normalize(dev(r, ops), S, out.t)
    np.testing.assert_allclose(out.take(), scipy.stats.norm.ppf((r - 0.325) / (S - 0.25)), rtol=1e-14)


# =====================================================================================================================
# 6. ops.iat_from_acor, ops.end_pos_pairs
# =====================================================================================================================
PAIRS_C = (1, 63, 64, 65, 255, 256, 257, 1000)
PAIRS_N = (12, 13, 200, 201)
PAIR_KINDS = ("first_negative", "all_positive", "minus_zero", "plus_zero", "nan_in_pair", "down_then_up", "stops_late")


def pairs_acor(N, C, seed=0):
    """[N, C] crafted autocorrelations, chain c of kind PAIR_KINDS[c % 7].  First pair >= 1 and every later positive pair
    >= 0.5 (the bound of pairs_reference rests on it); for odd N the last, unpaired row holds -1e300."""
    rng = np.random.default_rng([N, C, seed])
    a = 0.25 + 0.5 * rng.uniform(size=(N, C))  # pairs in [0.5, 1.5)
    a[0] = 1.0
    for c in range(C):
        kind = PAIR_KINDS[c % len(PAIR_KINDS)]
        if kind == "first_negative":
            a[1, c] = -1.5
        elif kind == "minus_zero":      # -0.0 is not < 0: the scan goes on to the negative pair behind it
            a[2, c] = a[3, c] = -0.0
            a[6:8, c] = [0.25, -0.75]
        elif kind == "plus_zero":
            a[2:4, c] = [0.5, -0.5]
            a[8:10, c] = [-1.0, 0.5]
        elif kind == "nan_in_pair":     # NaN is not < 0 either
            a[4 + c % 2, c] = NAN
            a[8:10, c] = [0.125, -0.25]
        elif kind == "down_then_up":    # the running minimum of the monotone estimator
            k = np.arange(N // 2)
            a[0:2 * len(k):2, c] = a[1:2 * len(k):2, c] = 0.5 + 0.25 * np.abs(k - min(3, len(k) - 1))
            a[0, c] += 0.5
        elif kind == "stops_late" and N >= 12:
            a[10:12, c] = [0.5, -0.5 - 2.0 ** -52]
    if N % 2:
        a[N - 1] = -POISON
    return a


def pairs_reference(a, estimator):
    """iat.py:7-43 and :95-135 (estimator 0) / :46-92 (estimator 1) in Python: the pair sums in float64 as the reference
    forms them, the totals in Fractions -> (stop index, iat, ess, pairs added) per chain; NaN where a NaN entered."""
    N, C = a.shape
    stop, iat, ess, cnt = np.empty(C, dtype=np.int64), np.empty(C), np.empty(C), np.empty(C)
    for c in range(C):
        n, pairs = 0, []
        while n + 1 < N:
            pk = float(a[n, c] + a[n + 1, c])
            pairs.append(pk)
            if pk < 0:
                break
            n += 2
        stop[c] = n
        before = [p for p in pairs if not p < 0]  # the pairs before the stop: acor[0:n]
        if estimator == 0:
            run, terms = pairs[0], [pairs[0]]  # (the first pair always enters, even when negative: iat.py:127-128)
            for pk in before[1:] if not pairs[0] < 0 else []:
                run = min(run, pk)  # iat.py:132 -- Python's min keeps the running minimum when the pair is NaN
                terms.append(run)
        else:
            terms = before  # iat.py:91: 2 * acor[0:n].sum() - 1
        cnt[c] = len(terms)
        if any(t != t for t in terms):
            iat[c] = ess[c] = NAN
        else:
            it = 2 * sum((Fraction(t) for t in terms), Fraction(0)) - 1
            iat[c], ess[c] = float(it), float(N / it)
    return stop, iat, ess, cnt


def check_pairs(ops, N, C):
    """Stop indices exact; IAT and ESS within (pairs + 2) u relative: the sequential sum of `pairs` terms, all positive
    once the first is in, is within (pairs - 1) u of its value T; 2 T - 1 adds one rounding and amplifies the relative
    error by 2 T / (2 T - 1) <= 1 + 1 / pairs (first pair >= 1, later ones >= 0.5), which the second spare u covers to
    first order; N / iat adds the last."""
    a = pairs_acor(N, C)
    xs = Slack(ops, N, C, fill=-POISON, data=a)  # a pair read from the padding would be negative
    out = SlackVec(ops, C, dtype=torch.int64)
    ops.end_pos_pairs(xs.t, out.t)
    worst = 0.0
    for est in (0, 1):
        stop, iat, ess, cnt = pairs_reference(a, est)
        assert np.array_equal(out.take("end_pos_pairs"), stop)
        e, i = SlackVec(ops, C), SlackVec(ops, C)
        ops.iat_from_acor(xs.t, est, e.t, i.t)
        ge, gi = e.take("ess_out"), i.take("iat_out")
        assert np.array_equal(np.isnan(gi), np.isnan(iat)), ("NaN chains (iat)", est, np.flatnonzero(np.isnan(gi) != np.isnan(iat))[:8])
        assert np.array_equal(np.isnan(ge), np.isnan(ess)), ("NaN chains (ess)", est)
        ok = ~np.isnan(iat)
        bound = (cnt[ok] + 2) * U
        worst = max(worst, ratio_of(np.abs(gi[ok] / iat[ok] - 1.0), bound, f"iat N={N} C={C} estimator {est}"),
                    ratio_of(np.abs(ge[ok] / ess[ok] - 1.0), bound, f"ess N={N} C={C} estimator {est}"))
        e2 = SlackVec(ops, C)
        ops.iat_from_acor(xs.t, est, e2.t, None)
        assert np.array_equal(e2.take(), ge, equal_nan=True)
    xs.take("acor")
    say(f"iat_from_acor / end_pos_pairs N={N} C={C}", worst)
    return worst


# =====================================================================================================================
# 7. ops.record_series / ops.record_series_dev
# =====================================================================================================================
REC_C = (1, 255, 256, 257, 5000)
REC_DIMS = ((), (2,), (4, 0, 4))  # K = 0, 1, 3: repeated and unordered
REC_CAP, REC_D, REC_OFFSET = 5, 5, 3


def check_record_series(ops, C, dims, with_logp, on_dev):
    """Rows 0 and 4 of a recorder of capacity 5: every recorded value bit-equal, every other row and the slack behind the
    series still NaN.  on_dev: the row is row_dev - 3 with row_dev - 3 = -1, 0, 4, 5; only 0 and 4 write anything."""
    rng = np.random.default_rng([C, len(dims), with_logp])
    K = len(dims)
    rows = max(K + (1 if with_logp else 0), 1)  # (K = 0 without logp: nothing to write into the one row given)
    flat = torch.full((rows * REC_CAP * C + 16,), NAN, dtype=F64, device=ops.device)
    series = flat[:rows * REC_CAP * C].view(rows, REC_CAP, C)
    theta = Slack(ops, REC_D, C, fill=POISON)
    dims_t = torch.tensor(dims, dtype=torch.int32, device=ops.device) if K else None
    row_dev = torch.zeros(1, dtype=torch.int64, device=ops.device)
    want = np.full((rows, REC_CAP, C), NAN)
    for row in ((-1, 0, 4, 5) if on_dev else (0, 4)):
        th, lp = rng.normal(size=(REC_D, C)), rng.normal(size=C)
        theta.t.copy_(torch.from_numpy(th))
        logp = dev(lp, ops) if with_logp else None
        if on_dev:
            row_dev.fill_(row + REC_OFFSET)
            ops.record_series_dev(theta.t, dims_t, logp, series, row_dev, REC_OFFSET)
        else:
            ops.record_series(theta.t, dims_t, logp, series, row)
        if 0 <= row < REC_CAP:
            for k, d in enumerate(dims):
                want[k, row] = th[d]
            if with_logp:
                want[K, row] = lp
        got = series.cpu().numpy()
        assert np.array_equal(got, want, equal_nan=True), (C, dims, with_logp, on_dev, row)
    assert bool(torch.isnan(flat[rows * REC_CAP * C:]).all()), "a write behind the series"
    theta.take("theta")
