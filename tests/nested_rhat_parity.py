"""Nested R-hat (bk_superchain_moments and the functions built on it) -- shared test bodies (GPU: tests/test_gpu_nested_rhat.py
on the HIP library; CPU: tests/test_nested_rhat_cpu.py on tests/fake_ops_nested.NestedFakeOps, which restates the kernel's
summation orders in NumPy).

The reference has no nested R-hat: the yardstick is the definition (Margossian et al.), evaluated EXACTLY here -- every
double is an integer times a power of two, the sums are Python integers, the quotients Fractions -- and the M = 1 identity
nested R-hat^2 = R-hat^2 + 1/n that ties it to the reference-pinned ``bk.rhat``.  Bounds are derived from the summation
order the kernel states for each M (u = 2^-53), never from what a device returned.  Outputs are views of wider NaN-filled
buffers, inputs views of wider buffers filled with 1e300.  Each check prints the largest err / bound it saw (``pytest -s``).
"""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import bayes_kit_amd as bk
from tests.diag_kernel_parity import POISON, U, Slack, SlackVec, dev, ratio_of, two_square  # noqa: F401

NAN = float("nan")


def say(what, value, unit="max err/bound"):
    print(f"[nested-rhat] {what}: {unit} = {value:.3g}" if isinstance(value, float) else f"[nested-rhat] {what}: {value}")


# =====================================================================================================================
# 1. the kernel: ops.superchain_moments
# =====================================================================================================================
SC_M = (1, 2, 3, 4, 32, 64, 65, 96, 128, 256, 257, 1000)
SC_K = (2, 3, 5)
SC_D = (1, 3, 130)
SC_N = (1, 2, 1000)
SC_WIDE = (1, 32_769, 2, 2)  # 65,538 chains: 257 workgroups of 256 lanes along the row, the last one ragged


def _cases():
    """Every M with every n; D and K rotate through their values (each meets every launch shape); 130 rows only up to
    M = 256, to keep the exact reference quick."""
    out = []
    for i, M in enumerate(SC_M):
        for j, n in enumerate(SC_N):
            D = SC_D[(i + j) % 3]
            if M > 256 and D == 130:
                D = 3
            out.append((D, SC_K[(i + 2 * j) % 3], M, n))
    return out


SC_CASES = _cases()
assert {c[2] for c in SC_CASES} == set(SC_M) and {c[1] for c in SC_CASES} == set(SC_K)
assert {c[0] for c in SC_CASES} == set(SC_D) and {c[3] for c in SC_CASES} == set(SC_N)
END_TO_END_CASES = [c for c in SC_CASES if c[1] * c[2] <= 1000 and not (c[2] == 1 and c[3] == 1)]


def regime(M):
    """The launch shape bk_superchain_moments picks (csrc/bk_diag.hip), restated."""
    if M <= 64 and M & (M - 1) == 0:
        return "seg"
    return "wg" if M > 64 else "lane"


assert [regime(M) for M in SC_M] == ["seg", "seg", "lane", "seg", "seg", "seg", "wg", "wg", "wg", "wg", "wg", "wg"]


def sc_adds(M):
    """Rounded additions on the longest path of one superchain's sum, from the order the kernel states:
    seg  (M = 2^j <= 64): the xor butterfly, one addition per level: log2 M;
    wg   (M > 64): a thread's ceil(M / 256) sequential additions (the first, to 0.0, is exact, and counted all the same),
         then the eight levels of the LDS tree;
    lane (any other M): M - 1 sequential additions."""
    r = regime(M)
    if r == "seg":
        return M.bit_length() - 1
    return -(-M // 256) + 8 if r == "wg" else M - 1


def sc_bounds(M, sum_abs_mu, w_exact):
    """|s - exact| <= delta = (a + 2) u sum|mu| / M  and  |w - exact| <= (a + 6) u w + M / (M - 1) delta^2,  a = sc_adds(M):
      s:  a roundings on the longest path of the sum (first order: each at most u times a partial sum <= sum|mu|), + 1 for
          the division by M, + 1 to spare for the second order;
      Wt: + 1 per term for M2 / (n - 1), a for the sum, + 1 for the division by M:                       (a + 2) u Wt;
      Bt: per term + 2 for the subtraction mu - s (its relative error enters the square twice) and + 1 for the square, a
          for the sum, + 1 for the division by M - 1:                                                    (a + 4) u Bt';
      + 1 for the final addition Bt + Wt and + 1 to spare: (a + 6) u (Bt' + Wt).  Bt' is centred on the ROUNDED s, off by
      at most delta, and sum (mu - s')^2 = sum (mu - s)^2 + M (s' - s)^2 exactly: hence M / (M - 1) delta^2 (M = 1: Bt = 0)."""
    a = sc_adds(M)
    delta = (a + 2) * U * sum_abs_mu / M
    bw = (a + 6) * U * w_exact + (M / (M - 1.0) * delta * delta if M > 1 else 0.0)
    return delta, bw


def sc_inputs(D, K, M, n, seed=0, offset=1e6):
    """rp_inputs-style: per-chain means with a common offset of 1e6 against a within-superchain sd of 1e-3 (where the
    centred form matters), superchain k shifted by a planted +-0.01 (k + 1), and M2 of chains whose own sd is about 1e-3."""
    rng = np.random.default_rng([D, K, M, n, seed])
    shift = 0.01 * (np.arange(K) + 1.0) * (-1.0) ** np.arange(K)
    mean = offset + 1e-3 * rng.normal(size=(D, K * M)) + np.repeat(shift, M)[None, :]
    m2 = (n - 1) * 1e-6 * (1.0 + 0.1 * rng.normal(size=(D, K * M))) ** 2
    return mean, m2


def _ints(a):
    """Python integers v_i and an exponent e with a[i] = v_i * 2**e exactly (a: 1-D float64, finite)."""
    mant, ex = np.frexp(a)
    m = (mant * 2.0 ** 53).astype(np.int64)
    e0 = int(ex.min())
    return [int(p) << (int(q) - e0) for p, q in zip(m, ex)], e0 - 53


_EXACT = {}


def sc_exact(mean, m2, n, M, key=None):
    """Per (d, k), as Fractions: s = sum mu / M and w = sum (mu - s)^2 / (M - 1) + sum M2 / (n - 1) / M; and float sum|mu|.
    sum (mu - s)^2 = sum mu^2 - (sum mu)^2 / M exactly, in integers."""
    if key is not None and key in _EXACT:
        return _EXACT[key]
    D, C = mean.shape
    K = C // M
    s = [[None] * K for _ in range(D)]
    w = [[None] * K for _ in range(D)]
    sabs = np.empty((D, K))
    for d in range(D):
        vi, ve = _ints(mean[d])
        qi, qe = _ints(m2[d]) if n > 1 else (None, 0)
        sc, sq = Fraction(2) ** ve, Fraction(2) ** qe
        for k in range(K):
            seg = vi[k * M:(k + 1) * M]
            S = sum(seg)
            s[d][k] = Fraction(S, M) * sc
            bt = Fraction(M * sum(v * v for v in seg) - S * S, M * (M - 1)) * sc * sc if M > 1 else Fraction(0)
            wt = Fraction(sum(qi[k * M:(k + 1) * M]), (n - 1) * M) * sq if n > 1 else Fraction(0)
            w[d][k] = bt + wt
            sabs[d, k] = float(sum(abs(v) for v in seg) * sc)
    if key is not None:
        _EXACT[key] = (s, w, sabs)
    return s, w, sabs


def exact_nested_rhat(s, w):
    """sqrt(1 + B / W) per row from the exact per-superchain values, B = var_k(s_k, ddof=1), W = mean_k(w_k)."""
    out = []
    for sd, wd in zip(s, w):
        K = len(sd)
        sbar = sum(sd) / K
        B = sum((v - sbar) ** 2 for v in sd) / (K - 1)
        W = sum(wd) / K
        out.append(math.sqrt(1 + B / W))
    return np.array(out)


def run_superchain_moments(ops, mean, m2, n, M, pad=3, nan_m2=False):
    """ops.superchain_moments on [:, :C] views of wider buffers (ld > C) into [:, :K] views of NaN buffers (ldk > K).
    -> (s, w) after checking that nothing beside the views was written and the inputs were left alone."""
    D, C = mean.shape
    ms = Slack(ops, D, C, pad=pad, fill=POISON, data=mean)
    qs = Slack(ops, D, C, pad=pad, fill=NAN if nan_m2 else POISON, data=np.full((D, C), NAN) if nan_m2 else m2)
    so, wo = Slack(ops, D, C // M), Slack(ops, D, C // M)
    ops.superchain_moments(ms.t, qs.t, n, M, so.t, wo.t)
    s, w = so.take("s_out"), wo.take("w_out")
    assert np.array_equal(ms.take("mean"), mean), "mean was overwritten"
    return s, w


def check_superchain_moments(ops, D, K, M, n):
    mean, m2 = sc_inputs(D, K, M, n)
    # n = 1: M2 must not be read -- it is handed over NaN-filled and w must come out finite
    s, w = run_superchain_moments(ops, mean, m2, n, M, nan_m2=(n == 1))
    assert np.isfinite(s).all() and np.isfinite(w).all(), "non-finite output (n = 1: was m2 read?)"
    es, ew, sabs = sc_exact(mean, m2, n, M, key=(D, K, M, n))
    err_s, err_w, bs, bw = (np.empty((D, K)) for _ in range(4))
    for d in range(D):
        for k in range(K):
            err_s[d, k] = abs(Fraction(float(s[d, k])) - es[d][k])
            err_w[d, k] = abs(Fraction(float(w[d, k])) - ew[d][k])
            bs[d, k], bw[d, k] = sc_bounds(M, sabs[d, k], float(ew[d][k]))
    rs = ratio_of(err_s, bs, f"superchain_moments s D={D} K={K} M={M} n={n}")
    rw = ratio_of(err_w, bw, f"superchain_moments w D={D} K={K} M={M} n={n}")
    say(f"superchain_moments D={D} K={K} M={M} n={n} ({regime(M)}) s", rs)
    say(f"superchain_moments D={D} K={K} M={M} n={n} ({regime(M)}) w", rw)
    if M == 1:  # one chain per superchain: nothing is summed
        assert np.array_equal(s, mean), "M = 1: s is the chain's mean, bit for bit"
        assert np.array_equal(w, m2 / float(n - 1) if n > 1 else np.zeros_like(mean)), "M = 1: w is M2 / (n - 1), bit for bit"
    return rs, rw


def check_position_independence(ops, D, K, M, n):
    """Superchain k of the [D, K M] input == superchain 0 of the view that starts at column k M (first, middle, last k);
    the same bits at another row pitch and on a second run."""
    mean, m2 = sc_inputs(D, K, M, n, seed=1)
    C = K * M
    ms, qs = Slack(ops, D, C, fill=POISON, data=mean), Slack(ops, D, C, fill=POISON, data=m2)
    so, wo = Slack(ops, D, K), Slack(ops, D, K)
    ops.superchain_moments(ms.t, qs.t, n, M, so.t, wo.t)
    s, w = so.take("s_out"), wo.take("w_out")
    for k in sorted({0, K // 2, K - 1}):
        s1, w1 = Slack(ops, D, 1), Slack(ops, D, 1)
        ops.superchain_moments(ms.t[:, k * M:(k + 1) * M], qs.t[:, k * M:(k + 1) * M], n, M, s1.t, w1.t)
        assert np.array_equal(s1.take("s_out of a view")[:, 0], s[:, k]), ("s depends on the position", M, k)
        assert np.array_equal(w1.take("w_out of a view")[:, 0], w[:, k]), ("w depends on the position", M, k)
    s2, w2 = run_superchain_moments(ops, mean, m2, n, M, pad=11)
    assert np.array_equal(s2, s) and np.array_equal(w2, w), ("the row pitch changes the bits", M)
    s3, w3 = run_superchain_moments(ops, mean, m2, n, M)
    assert np.array_equal(s3, s) and np.array_equal(w3, w), ("two runs differ", M)


# =====================================================================================================================
# 2. end-to-end values
# =====================================================================================================================
def check_from_moments_against_fractions(ops, D, K, M, n):
    """nested_rhat_from_moments against the exact evaluation at rel 1e-12.

    Inputs: sc_inputs WITHOUT the common offset of 1e6.  The interface hands the superchain means on as doubles, and
    B = var_k(s_k) is first order in their rounding: with |s_k| = 1e6 and planted shifts of 0.01 an error of half an ulp
    of s_k (5.8e-11) alone moves s_k - mean(s) by 6e-9 of itself, so 1e-12 is not a property any double-valued s_out can
    have there; that data is what the kernel's own bound (check_superchain_moments) is for.  Around zero the same
    roundings are (a + 2) u of values of the size of the shifts themselves."""
    mean, m2 = sc_inputs(D, K, M, n, seed=2, offset=0.0)
    ms, qs = Slack(ops, D, K * M, fill=POISON, data=mean), Slack(ops, D, K * M, fill=POISON, data=m2)
    got = bk.nested_rhat_from_moments(ms.t, qs.t if n > 1 else None, n, M, ops=ops)
    es, ew, _ = sc_exact(mean, m2, n, M)
    want = exact_nested_rhat(es, ew)
    assert got.shape == (D,)
    rel = float(np.max(np.abs(got / want - 1.0)))
    say(f"nested_rhat_from_moments D={D} K={K} M={M} n={n}", rel / 1e-12, "max rel err / 1e-12")
    np.testing.assert_allclose(got, want, rtol=1e-12)
    return rel


def check_m1_identity(ops):
    """nested R-hat^2 - R-hat^2 = 1/n for M = 1, to rel 1e-12 of 1/n, on [50, 64] draws."""
    x = np.random.default_rng(7).normal(size=(50, 64))
    xt = dev(x, ops)
    nr = float(bk.nested_rhat(xt, 1, ops=ops))
    r = float(bk.rhat(xt, ops=ops))
    diff = nr * nr - r * r
    say("M = 1 identity: (nR^2 - R^2) n - 1", abs(diff * 50 - 1.0), "")
    assert abs(diff - 1.0 / 50) <= 1e-12 * (1.0 / 50), (nr, r, diff)


def check_three_entry_points(ops, M=4, K=6, N=12, D=3):
    """The same draws as one [N, C] tensor per coordinate, fed draw by draw to a RunningMoments, and to a DrawRecorder."""
    C = K * M
    x = np.random.default_rng(11).normal(size=(N, D, C)) + np.repeat(0.3 * np.arange(K), M)[None, None, :]
    xt = dev(x, ops)
    rm = bk.RunningMoments(D, C, ops=ops)
    rec = bk.DrawRecorder(list(range(D)), N, C, with_logp=False, ops=ops)
    for t in range(N):
        rm.update(xt[t], layout="dc")
        rec.record(xt[t], layout="dc")
        if t == 0:  # defined from the first draw on, on all three
            first = [float(bk.nested_rhat(xt[:1, d, :], M, ops=ops)) for d in range(D)]
            assert np.array_equal(rec.nested_rhat(M), np.array(first))
            np.testing.assert_allclose(rm.nested_rhat(M), first, rtol=1e-10)
    tensor = np.array([float(bk.nested_rhat(xt[:, d, :].contiguous(), M, ops=ops)) for d in range(D)])
    recorder = rec.nested_rhat(M)
    assert recorder.shape == (D,) and np.array_equal(tensor, recorder), (tensor, recorder)
    np.testing.assert_allclose(rm.nested_rhat(M), tensor, rtol=1e-10)
    seq = float(bk.nested_rhat([x[:, 0, c] for c in range(C)], M, ops=ops))  # the sequence form: the same chains
    assert seq == tensor[0]
    if hasattr(ops, "ess_split_moments"):  # (the device; the base stand-in has no multi-chain ESS): summary gains no entry
        assert set(rec.summary()) == {"name", "mean", "sd", "mcse_mean", "ess_bulk", "ess_tail", "rhat"}


# =====================================================================================================================
# 3. behaviour
# =====================================================================================================================
BEHAVIOUR_SEEDS = range(5)
BK_K, BK_M = 16, 32


def numpy_nested_rhat(x, M):
    """The definition in plain NumPy on [n, C] draws."""
    n, C = x.shape
    K = C // M
    mu = x.mean(axis=0).reshape(K, M)
    var = x.var(axis=0, ddof=1).reshape(K, M) if n > 1 else np.zeros((K, M))
    s = mu.mean(axis=1)
    bt = mu.var(axis=1, ddof=1) if M > 1 else np.zeros(K)
    return np.sqrt(1.0 + s.var(ddof=1) / np.mean(bt + var.mean(axis=1)))


def check_behaviour(ops, seed):
    K, M = BK_K, BK_M
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(50, K * M))
    f = lambda a: float(bk.nested_rhat(dev(a, ops), M, ops=ops))  # noqa: E731
    iid = f(x)
    shifted = f(x + np.repeat(np.arange(K, dtype=np.float64), M)[None, :])
    one = f(rng.normal(size=(1, K * M)))
    starts = rng.normal(size=K)
    stuck_x = (np.repeat(starts, M) + 1e-3 * rng.uniform(-1.0, 1.0, size=K * M))[None, :]
    stuck = f(stuck_x)
    say(f"seed {seed}: iid n=50 / shifted / iid n=1 / stuck n=1", f"{iid:.5f} {shifted:.3f} {one:.4f} {stuck:.0f}")
    np.testing.assert_allclose([iid, stuck], [numpy_nested_rhat(x, M), numpy_nested_rhat(stuck_x, M)], rtol=1e-9)
    assert iid < 1.005
    assert shifted > 3
    assert math.isfinite(one) and one < 1.1
    assert stuck > 100


# =====================================================================================================================
# 4. errors
# =====================================================================================================================
def check_errors(ops):
    x = dev(np.random.default_rng(0).normal(size=(5, 8)), ops)
    with pytest.raises(ValueError, match="superchains"):
        bk.nested_rhat(x, 8, ops=ops)                      # K = 1
    with pytest.raises(ValueError, match="both are 1"):
        bk.nested_rhat(x[:1], 1, ops=ops)                  # M = 1 with n = 1
    with pytest.raises(ValueError, match="multiple of chains_per_superchain"):
        bk.nested_rhat(x, 3, ops=ops)                      # C % M != 0
    with pytest.raises(ValueError, match="equal length"):
        bk.nested_rhat([np.zeros(4), np.zeros(4), np.zeros(3), np.zeros(4)], 2, ops=ops)
    with pytest.raises(ValueError, match="chains_per_superchain >= 1"):
        bk.nested_rhat(x, 0, ops=ops)
    rm = bk.RunningMoments(2, 8, ops=ops)
    with pytest.raises(ValueError, match="len\\(chain\\) >= 1"):
        rm.nested_rhat(2)                                  # no draw yet
    rm.update(dev(np.random.default_rng(1).normal(size=(2, 8)), ops), layout="dc")
    assert np.isfinite(rm.nested_rhat(2)).all()            # ... and from the first draw on
    with pytest.raises(ValueError, match="both are 1"):
        rm.nested_rhat(1)
    with pytest.raises(ValueError, match="superchains"):
        rm.nested_rhat(8)
    # NaN and W = 0 propagate as IEEE arithmetic gives them
    const = dev(np.repeat([1.0, 2.0, 4.0], 2)[None, :], ops)  # every subchain AT its superchain's start: W = 0 < B
    assert bk.nested_rhat(const, 2, ops=ops) == np.inf
    bad = np.random.default_rng(2).normal(size=(5, 8))
    bad[3, 5] = NAN
    assert math.isnan(bk.nested_rhat(dev(bad, ops), 2, ops=ops))


def check_superchain_init():
    pts = np.arange(6.0).reshape(3, 2)
    init = bk.superchain_init(pts, 4)
    assert init.shape == (12, 2)
    for c in range(12):
        assert np.array_equal(init[c], pts[c // 4])  # the c -> c // M convention
    t = bk.superchain_init(torch.from_numpy(pts), 4)
    assert isinstance(t, torch.Tensor) and np.array_equal(t.numpy(), init)
    with pytest.raises(ValueError):
        bk.superchain_init(pts, 0)
    with pytest.raises(ValueError):
        bk.superchain_init(np.zeros(3), 2)


# =====================================================================================================================
# 5. a sampler run
# =====================================================================================================================
RUN_K, RUN_M, RUN_D, RUN_EPS, RUN_STEPS = 16, 32, 4, 0.3, 8
RUN_SEED, RUN_DRAWS = 20, 2  # (RUN_DRAWS: see check_sampler_run)


def run_starts(seed=RUN_SEED):
    return 10.0 * np.random.default_rng([seed, 1]).normal(size=(RUN_K, RUN_D))


def check_sampler_run(ops, draws=None):
    """HMCDiag on IsoGaussian(4) from 16 start points 10 N(0, 1), 32 subchains each, feeding a RunningMoments:
    max_d nested R-hat(32) is above 3 after the first draw and below 1.05 after RUN_DRAWS draws.

    RUN_DRAWS = 2 is the smallest N at which the same configuration run through oracle.samplers.HMCDiag (one NumPy chain
    per Philox key (RUN_SEED, c), Welford moments, the definition in NumPy) is below 1.02: 18.92078 after the first draw,
    1.00586 after the second.  (The trajectory of 2.4 time units takes a start x to about -0.74 x: two draws of a chain
    straddle the mode, so their within-chain variance, about 80, swamps what is left between the superchain means.)"""
    draws = RUN_DRAWS if draws is None else draws
    C = RUN_K * RUN_M
    s = bk.HMCDiag(bk.IsoGaussian(RUN_D, ops=ops), RUN_EPS, RUN_STEPS, init=bk.superchain_init(run_starts(), RUN_M), chains=C,
                   seed=RUN_SEED, ops=ops)
    rm = bk.RunningMoments(RUN_D, C, ops=ops)
    hist = []
    for t in range(draws):
        th, _ = s.sample()
        rm.update(th)
        if t == 0 or t == draws - 1:
            hist.append(float(np.max(rm.nested_rhat(RUN_M))))
    say(f"sampler run: max_d nested R-hat after 1 and {draws} draws", f"{hist[0]:.3f} {hist[-1]:.4f}")
    assert hist[0] > 3, hist
    assert hist[-1] < 1.05, hist
    return hist
