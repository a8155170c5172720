"""The multi-chain ESS kernels of csrc/bk_ess_multi.hip (and bk_autocorr_fft as that route calls it) at their group, tile
and launch seams -- shared test bodies (GPU: tests/test_gpu_ess_multi_kernels.py on the HIP library; CPU:
tests/test_ess_multi_kernels_cpu.py on tests/multichain_ess_ref.MultiEssFakeOps, which exercises these bodies, their
references and their bounds without a device).

Every input is a ``[:, off:off + C]`` view of a wider, longer buffer filled with POISON; chain_mean / chain_g0 are the
leading 2C entries of NaN-filled vectors, and whatever the contract leaves alone must still be NaN afterwards.  The
references are long double (lag sums), exact (math.fsum of exact products, Fractions) or the project's own NumPy
restatement at the tolerance it already holds; every other bound is the number of rounded operations on the deepest path of
the kernel's summation shape (u = 2^-53) times the sum of |terms|, never something a device returned.  Each body prints and
returns the largest err / bound it saw (``pytest -s``; kept in profiles/ess_multi_edges.md)."""
import functools
import math
from fractions import Fraction

import numpy as np
import torch

import bayes_kit_amd as bk
from bayes_kit_amd import diagnostics as dg
from tests import multichain_ess_ref as ref
from tests.diag_kernel_parity import (CMV_DATA, F64, NAN, PHIS, POISON, U, Slack, SlackVec, ar1_series, cmv_bounds,
                                      cmv_data, dev, exact_mean_var, ratio_of, two_square)
from tests.diag_kernel_parity import say as _say

BK_OK, BK_E_ARG, BK_E_ALIGN = 0, -1, -2  # include/bkhip.h


def say(what, value, unit="max err/bound"):
    _say("ess-multi " + what, value, unit)


def cdiv(a, b):
    return -(-a // b)


def has_abi(ops):
    """The HIP library (a C ABI to call with caller-owned buffers); the NumPy stand-in has none."""
    return hasattr(ops, "lib") and hasattr(ops, "_call")


def status_of(ops, name, *args):
    """Return code of a C entry called exactly as the wrappers call it (ops._call raises with the code in its text)."""
    from bayes_kit_amd._lib import BkHipError

    try:
        ops._call(name, *args)
    except BkHipError as e:
        return int(str(e).rsplit(" ", 1)[1])
    return BK_OK


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _stream(ops):
    return ops._s()


# =====================================================================================================================
# The launch plan of bk_ess_multi.hip, restated (lag_plan, lag_chunk, bk_ess_multi_work_bytes)
# =====================================================================================================================
EM_BLOCK, EM_WAVE = 256, 64
EM_RT_MIN, EM_RT_TAIL = 288, 72              # register tiles from this half length on, followed by 72 zeros in LDS
EM_RED = 4 * 64                              # doubles behind the chains for the four wavefronts' sums
EM_CAP = (160 * 1024 - 512) // 8 - EM_RED    # doubles of chains one workgroup may stage: 20,160
EM_CAP2 = 78 * 1024 // 8 - EM_RED            # ... when two workgroups are to share a CU: 9,728
EM_OPT_IN = 64 * 1024                        # above this many bytes of LDS: hipFuncSetAttribute, once per instance
EM_PART_BYTES = 256 << 20                    # partials of one k_lag_sums launch
GROUPS = (16, 8, 4, 2, 1)
MAX_HALF = 20_087


def lag_plan(n):
    """(G, pitch, register tiles, LDS bytes) of k_lag_sums for half length n; G = 0: the FFT route serves."""
    rt = n >= EM_RT_MIN
    pitch = ((n + EM_RT_TAIL) if rt else (n + 1)) | 1
    for cap in (EM_CAP2, EM_CAP):
        for g in GROUPS:
            if g * pitch <= cap:
                return g, pitch, rt, (g * pitch + EM_RED) * 8
    return 0, pitch, rt, 0


def lag_chunk(C, G, nlags):
    cap = EM_PART_BYTES // 8 // (2 * cdiv(C, G)) // EM_WAVE * EM_WAVE
    return min(nlags, max(cap, EM_WAVE))


def work_bytes(n, C, nlags):
    G = lag_plan(n)[0]
    B = max(2 * cdiv(C, EM_WAVE) * 3, cdiv(2 * C, EM_BLOCK))
    bl = 2 * cdiv(C, G) * lag_chunk(C, G, nlags) if G else cdiv(C, EM_BLOCK) * nlags
    return 8 * max(B, bl, 1)


def _seams():
    out, prev = [], None
    for n in range(1, MAX_HALF + 200):
        g = lag_plan(n)[0]
        if g != prev:
            out.append((n, g))
            prev = g
    return out


EM_SEAMS = _seams()  # (first half length, G) of every stretch
# a changed constant shows up here, not as a silently moved seam
assert EM_SEAMS == [(1, 16), (536, 8), (1144, 4), (2360, 2), (4792, 1), (9656, 2), (10_008, 1), (20_088, 0)], EM_SEAMS
assert [lag_plan(n)[1] for n in (4, 287, 288, 535)] == [5, 289, 361, 607]  # (n + 1) | 1 below 288, then (n + 72) | 1
# the lower side of a seam is that instance's over-64-KiB launch, the upper side the next instance's plain launch
# (9,655 / 9,656 / 10,007 / 10,008 / 20,087 have the CU to themselves: all opt-in)
assert [lag_plan(n)[3] > EM_OPT_IN for n in (535, 536, 1143, 1144, 2359, 2360, 4791, 4792)] == [True, False] * 4
assert all(lag_plan(n)[3] > EM_OPT_IN for n in (9655, 9656, 10_007, 10_008, MAX_HALF))
assert [min(n for n in range(1, 9656) if lag_plan(n)[0] == g and lag_plan(n)[3] > EM_OPT_IN) for g in GROUPS] == \
    [424, 920, 1912, 3896, 7864]
assert lag_plan(MAX_HALF)[3] == 160 * 1024 - 520 and lag_chunk(4096, 1, 5000) == 4096

LS_N = (4, 63, 64, 65, 287, 288, 289, 535, 536, 1143, 1144, 2359, 2360, 4791, 4792, 9655, 9656, 10_007, 10_008, MAX_HALF)
LS_ODD_N = (288, 536, 2360, 9656)  # N = 2n + 1: the second half starts at row n + 1
LS_INDICATOR_N = (65, 535, 1143, 2359, 4791, 9655)  # one per instance: <16, false>, then <16 / 8 / 4 / 2 / 1, true>
LS_ALL_LAGS_UP_TO = 2360
LS_CONST = 24
"""The stated constant of the lag-sum bound: 6 levels of the register tiles' butterfly, 3 additions of the four wavefronts'
sums, 6 + 3 of k_sum_rows' wave sum and tree, 2 for the factor 1 / n (its own rounding and the product), 1 for a term's
rounded product (the one-accumulator kernel below 288 draws; the register tiles use fma), 1 for rounding the reference to
float64, 2 to spare for the second order."""


def ls_chain_counts(n):
    G = lag_plan(n)[0]
    return sorted({1, G - 1, G + 1, 2 * G + 3} - {0})


LS_CASES = [(n, 0, C) for n in LS_N for C in ls_chain_counts(n)] + [(n, 1, C) for n in LS_ODD_N for C in ls_chain_counts(n)]
LS_INDICATOR_CASES = [(n, 0, 2 * lag_plan(n)[0] + 3) for n in LS_INDICATOR_N]
assert [lag_plan(n)[0] for n in LS_INDICATOR_N] == [16, 16, 8, 4, 2, 1] and not lag_plan(65)[2]


def ls_requests(n):
    """The driver's own rounds, an unaligned request, requests whose later blocks of a pass start at or beyond lag_end
    (G <= 2), the last lags (lanes that stop early, the nl < n guard) and all lags in one call."""
    req = [(0, min(64, n)), (64, 64), (128, 128), (37, 100), (0, 65), (0, 129), (0, 193), (n - 70, 70), (n - 1, 1), (0, n)]
    out = []
    for a, b in req:
        if a >= 0 and b >= 1 and a + b <= n and (a, b) not in out:
            out.append((a, b))
    return out


def ls_compared(n, lag0, nlags):
    """Positions of a request's output that are compared: every lag, or for (0, n) above 2,360 the first 320, the last 130
    and 256 seeded random ones (every returned value must be finite all the same)."""
    if not (lag0 == 0 and nlags == n and n > LS_ALL_LAGS_UP_TO):
        return np.arange(nlags)
    rnd = np.random.default_rng([n, 17]).integers(320, n - 130, size=256)
    return np.unique(np.concatenate([np.arange(320), np.arange(n - 130, n), rnd]))


def ls_depth(n, k, G, rt, B):
    """Rounded operations on the deepest path to lag k's sum: the longest sequential chain of additions (a register-tile
    accumulator takes 9 terms per 576-draw chunk; the one-accumulator kernel all n - k), the chains of a workgroup, a
    k_sum_rows thread's partials, and LS_CONST."""
    seq = 9 * cdiv(n - k, 9 * EM_WAVE) if rt else n - k
    return seq + G + cdiv(B, EM_BLOCK) + LS_CONST


def ls_longdouble_error(n, M, rows=0):
    """Relative to sum |terms|: a long-double product (2^-64) and NumPy's pairwise sum of n M of them; with `rows`, each
    chain's `rows` terms are added one after the other instead (ls_reference's large inputs) and the chains pairwise."""
    return ((rows + math.log2(max(M, 2)) if rows else math.log2(max(n * M, 2))) + 3.0) * 2.0 ** -64


LS_WHOLE_CELLS = 1 << 24


def ls_reference(d, lags):
    """d [n, M]: the centred split chains exactly as the kernel stages them.  -> (sum_m gamma_{m,k}, sum |terms| / n, the
    long-double sums' own error relative to sum |terms|) for k in lags: products and sums in long double; sum |terms| in
    float64, rounded up (it only scales a bound).  Above 2^24 cells only the rows the lags need are converted, each chain's
    terms are added in sequence (no temporary) and the lags are spread over eight threads."""
    n, M = d.shape
    lags = [int(k) for k in lags]
    if d.size <= LS_WHOLE_CELLS:
        whole = d.astype(np.longdouble)
        want = np.array([float((whole[:n - k] * whole[k:]).sum() / n) for k in lags])
        sabs = np.array([float(np.abs(d[:n - k] * d[k:]).sum()) for k in lags]) / n * (1.0 + 1e-9)
        return want, sabs, np.full(len(lags), ls_longdouble_error(n, M))
    from concurrent.futures import ThreadPoolExecutor

    kmin = min(lags)
    head, tail = d[:n - kmin].astype(np.longdouble), d[kmin:].astype(np.longdouble)

    def one(k):
        w = np.einsum("tm,tm->m", head[:n - k], tail[k - kmin:]).sum() / n
        return float(w), float(np.einsum("tm,tm->", np.abs(d[:n - k]), np.abs(d[k:]))) / n * (1.0 + 1e-9)

    with ThreadPoolExecutor(8) as pool:
        res = list(pool.map(one, lags))
    return (np.array([r[0] for r in res]), np.array([r[1] for r in res]),
            np.array([ls_longdouble_error(n, M, rows=n - k) for k in lags]))


def ls_inputs(ops, n, odd, C, seed=0):
    """-> (x [N, C] host, Slack view): AR(1) chains with persistence PHIS[c % 6]; the middle row of an odd N is POISON."""
    N = 2 * n + odd
    x = ar1_series(N, C, seed)
    if odd:
        x[n] = POISON
    return x, Slack(ops, N, C, pad=3, extra=1, off=2, fill=POISON, data=x)


def ls_moments(ops, xs, q, C):
    """chain_mean / chain_g0 from the entry point itself, as the leading 2C entries of NaN-filled vectors."""
    cm, g0 = SlackVec(ops, 2 * C), SlackVec(ops, 2 * C)
    tot = ops.ess_split_moments(xs.t, q, cm.t, g0.t)
    return cm, g0, tot.cpu().numpy()


def check_lag_sums(ops, n, odd, C, indicator=False, requests=None, compared=None):
    """ops.ess_lag_sums at one half length, chain count and parity of N, every request of ls_requests (or `requests`),
    against the long-double sums of the very doubles the kernel stages, d = fl(x - chain_mean[m])."""
    G, pitch, rt, lds = lag_plan(n)
    x, xs = ls_inputs(ops, n, odd, C)
    q = float(x[n // 3, 0]) if indicator else None  # (ties a draw exactly)
    cm, _, _ = ls_moments(ops, xs, q, C)
    mean = cm.take("chain_mean")
    s = ref.split(x)
    if indicator:
        assert (s == q).any()
        s = (s <= q).astype(np.float64)
    d = s - mean  # float64, one rounding per draw: what k_lag_sums writes to LDS
    B = 2 * cdiv(C, G)
    requests = ls_requests(n) if requests is None else requests
    pick = {r: (ls_compared(n, *r) if compared is None else np.asarray(compared[r])) for r in requests}
    lags = np.unique(np.concatenate([r[0] + pick[r] for r in requests]))
    want, sabs, ld_err = ls_reference(d, lags)
    depth = np.array([ls_depth(n, int(k), G, rt, B) for k in lags])
    bound = depth * U * sabs + ld_err * sabs
    worst = 0.0
    for lag0, nlags in requests:
        got = ops.ess_lag_sums(xs.t, q, cm.t, lag0, nlags)
        again = ops.ess_lag_sums(xs.t, q, cm.t, lag0, nlags)
        assert got.shape == (nlags,) and bool(torch.isfinite(got).all()), ("a non-finite lag sum", n, C, lag0, nlags)
        assert torch.equal(got, again), ("two identical calls differ", n, C, lag0, nlags)
        g = got.cpu().numpy()[pick[(lag0, nlags)]]
        idx = np.searchsorted(lags, lag0 + pick[(lag0, nlags)])
        worst = max(worst, ratio_of(np.abs(g - want[idx]), bound[idx],
                                    f"lag sums n={n} N={2 * n + odd} C={C} G={G} request=({lag0}, {nlags})"))
    xs.take("x"), cm.take("chain_mean")
    say(f"lag sums n={n} N={2 * n + odd} C={C} G={G} pitch={pitch} lds={lds} indicator={indicator}", worst)
    return worst


# one dropped or doubled term: |d d| / n against a bound of depth u sum|d d| / n <= depth u n M max|d d| / n; with
# |d d| of order one the term stands depth u n M below... i.e. 1 / (depth u n M) above the bound: at the largest case
# (n = 20,087, M = 10, depth 350) a factor 1.3e8, and more at every smaller one.
LS_TERM_OVER_BOUND_LARGEST = 1.0 / (ls_depth(MAX_HALF, 0, 1, True, 10) * U * MAX_HALF * 10)
assert LS_TERM_OVER_BOUND_LARGEST > 1e8

CHUNKED = (5000, 4096)


def check_lag_sums_chunked(ops, n=CHUNKED[0], C=CHUNKED[1]):
    """All lags of 5,000-draw halves of 4,096 chains in one call: lag_chunk = 4,096 < n, two launches share the partials.
    Compared: lags 4,032 .. 4,160 (both sides of the chunk edge) and the last 64."""
    if (n, C) == CHUNKED:
        assert lag_plan(n)[0] == 1 and lag_chunk(C, 1, n) == 4096 < n
    lags = np.concatenate([np.arange(4032, 4161), np.arange(n - 64, n)])
    return check_lag_sums(ops, n, 0, C, requests=[(0, n)], compared={(0, n): lags})


def check_lag_sums_abi(ops):
    """Caller-owned out and work: `out` NaN-guarded, `work` exactly bk_ess_multi_work_bytes long with NaN guards behind it
    in the same allocation; the return codes of the host-side checks (no kernel runs for any of them)."""
    assert has_abi(ops)
    from bayes_kit_amd._lib import _ld

    lib = ops.lib
    assert int(lib.bk_ess_lag_sums_max_half()) == ops.ess_lag_sums_max_half() == MAX_HALF
    for n in (1, 4, 287, 288, 535, 536, 4791, 4792, 9656, MAX_HALF, MAX_HALF + 1, 66_000):
        for C in (1, 3, 63, 64, 65, 4096, 65_600):
            for nlags in (1, 64, n):
                assert int(lib.bk_ess_multi_work_bytes(n, C, nlags)) == work_bytes(n, C, nlags), (n, C, nlags)
    n, C, nlags = 600, 11, 193
    x, xs = ls_inputs(ops, n, 1, C)
    cm, _, _ = ls_moments(ops, xs, None, C)
    want = ops.ess_lag_sums(xs.t, None, cm.t, 7, nlags)
    wb = work_bytes(n, C, nlags)
    work = torch.full((wb // 8 + 4,), NAN, dtype=F64, device=ops.device)
    out = SlackVec(ops, nlags)

    def call(N=2 * n + 1, ld=_ld(xs.t), C_=C, lag0=7, nl=nlags, wbytes=wb, xt=xs.t):
        return status_of(ops, "bk_ess_lag_sums", _ptr(xt), ld, N, C_, 0, 0.0, _ptr(cm.t), lag0, nl, _ptr(out.t), _ptr(work),
                         wbytes, _stream(ops))

    assert call() == BK_OK
    assert np.array_equal(out.take("out"), want.cpu().numpy())
    assert bool(torch.isnan(work[wb // 8:]).all()), "a write behind the work buffer"
    assert call(wbytes=wb - 8) == BK_E_ARG
    assert call(lag0=n - nlags + 1) == BK_E_ARG and call(lag0=n - nlags) == BK_OK
    assert call(ld=C - 1) == BK_E_ALIGN
    long_x = torch.zeros((2 * (MAX_HALF + 1), 1), dtype=F64, device=ops.device)  # (real rows: nothing here may be read)
    one = SlackVec(ops, 2)
    one.t.zero_()
    big = torch.empty(work_bytes(MAX_HALF, 1, 1) // 8 + 64, dtype=F64, device=ops.device)
    args = (_ptr(one.t), 0, 1, _ptr(out.t), _ptr(big), big.numel() * 8, _stream(ops))
    assert status_of(ops, "bk_ess_lag_sums", _ptr(long_x), 1, 2 * (MAX_HALF + 1), 1, 0, 0.0, *args) == BK_E_ARG
    assert status_of(ops, "bk_ess_lag_sums", _ptr(long_x), 1, 2 * MAX_HALF, 1, 0, 0.0, *args) == BK_OK
    # the moments and the between-chain pass with their own exact work sizes
    mom = SlackVec(ops, 3)
    c2, g2 = SlackVec(ops, 2 * C), SlackVec(ops, 2 * C)
    wb = work_bytes(n, C, 1)
    work = torch.full((wb // 8 + 4,), NAN, dtype=F64, device=ops.device)
    margs = (_ptr(c2.t), _ptr(g2.t), _ptr(mom.t), _ptr(work))
    assert status_of(ops, "bk_ess_split_moments", _ptr(xs.t), _ld(xs.t), 2 * n + 1, C, 0, 0.0, *margs, wb, _stream(ops)) == BK_OK
    assert np.array_equal(c2.take(), cm.take()) and bool(torch.isnan(work[wb // 8:]).all())
    mom.take("moments out")
    assert status_of(ops, "bk_ess_split_moments", _ptr(xs.t), C - 1, 2 * n + 1, C, 0, 0.0, *margs, wb, _stream(ops)) == BK_E_ALIGN
    assert status_of(ops, "bk_ess_split_moments", _ptr(xs.t), _ld(xs.t), 2 * n + 1, C, 0, 0.0, *margs, 8 * 3 * 2 - 8,
                     _stream(ops)) == BK_E_ARG
    assert status_of(ops, "bk_ess_split_moments", _ptr(xs.t), _ld(xs.t), 1, C, 0, 0.0, *margs, wb, _stream(ops)) == BK_E_ARG
    return True


# =====================================================================================================================
# 2. ops.ess_split_moments, ops.ess_between_sq
# =====================================================================================================================
SM_N = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 1000)
SM_C = (1, 63, 64, 65, 130)
SM_WIDE = (5, 8200)  # 2 * cdiv(8200, 64) = 258 > 256 partials per row of k_sum_rows
BSQ_M = (2, 255, 256, 257, 1000, 65_540)


def sum_rows_bound(B, sum_abs, terms=64):
    """Totals of per-workgroup partials: a wave sum over `terms` lanes (6 levels) inside the workgroup, then k_sum_rows --
    a thread's ceil(B / 256) sequential additions, the 6 levels of its wave sum, 3 for the four wavefronts -- and one to
    spare."""
    return (math.ceil(math.log2(max(terms, 2))) + cdiv(B, EM_BLOCK) + 6 + 3 + 1) * U * sum_abs


def sm_exact(s):
    """Exact mean and gamma_0 = sum (x - mean)^2 / n of every column of s [n, M], and the bounds of cmv_bounds carried
    over to the divisor n: |mean - exact| <= delta = k u sum|x| / n, |g0 - exact| <= (k + 6) u exact + delta^2 with
    k = ceil(n / 4) + 4 (four wavefronts of sequential sums, their three additions, the division)."""
    n, M = s.shape
    out = np.empty((4, M))
    for m in range(M):
        mu, var = exact_mean_var(s[:, m])
        g0 = float(var * (n - 1) / n) if var is not None else 0.0
        delta, _ = cmv_bounds(n, math.fsum(np.abs(s[:, m])), None if n < 2 else g0)
        k = cdiv(n, 4) + 4
        out[:, m] = float(mu), g0, delta, (k + 6) * U * g0 + delta * delta
    return out


def check_split_moments(ops, n, C, kinds=CMV_DATA, odds=(0, 1)):
    worst = [0.0, 0.0, 0.0]
    for kind in kinds:
        for odd in odds:
            N = 2 * n + odd
            x = cmv_data(kind, N, C)
            if odd:
                x[n] = POISON
            xs = Slack(ops, N, C, pad=3, extra=1, off=1, fill=POISON, data=x)
            cm, g0, tot = ls_moments(ops, xs, None, C)
            gm, gg = cm.take("chain_mean"), g0.take("chain_g0")
            ex = sm_exact(ref.split(x))
            what = f"n={n} N={N} C={C} {kind}"
            worst[0] = max(worst[0], ratio_of(np.abs(gm - ex[0]), ex[2], "chain_mean " + what))
            worst[1] = max(worst[1], ratio_of(np.abs(gg - ex[1]), ex[3], "chain_g0 " + what))
            B = 2 * cdiv(C, EM_WAVE)
            for j, v in ((0, gm), (1, gg)):  # the totals of the values the entry point itself wrote
                worst[2] = max(worst[2], ratio_of(abs(tot[j] - math.fsum(v)), sum_rows_bound(B, math.fsum(np.abs(v))),
                                                  f"out[{j}] " + what))
            assert tot[2] == 0.0, ("out[2]: no draw of the split set is non-finite", what, tot[2])
            xs.take("x")
    say(f"split moments n={n} C={C} mean", worst[0])
    say(f"split moments n={n} C={C} gamma_0", worst[1])
    say(f"split moments n={n} C={C} totals", worst[2])
    return worst


def sm_indicator_data(N, C, seed=0):
    """Draws on a grid of tenths (ties with q, -0.0 next to +0.0) with +inf and -inf among them."""
    rng = np.random.default_rng([N, C, seed, 5])
    x = np.round(rng.normal(size=(N, C)), 1)
    x[rng.uniform(size=(N, C)) < 0.05] = -0.0
    x[rng.uniform(size=(N, C)) < 0.02] = np.inf
    x[rng.uniform(size=(N, C)) < 0.02] = -np.inf
    return x


def check_split_moments_indicator(ops, n, C, odd):
    """Indicator mode: the sums are integers, so chain_mean is count / n bit for bit; gamma_0 = p (1 - p) within
    (k + 6) u gamma_0 + (u p)^2; out[2] counts the infinities of the split set.  q = 0.0 ties +0.0 and -0.0, q = 0.3 a
    grid value."""
    N = 2 * n + odd
    x = sm_indicator_data(N, C)
    if odd:
        x[n] = NAN  # (not a row of the split set: must not count)
    xs = Slack(ops, N, C, pad=2, extra=2, off=3, fill=POISON, data=x)
    s = ref.split(x)
    worst = 0.0
    for q in (0.0, 0.3):
        assert (s == q).any() or n * C < 40
        cm, g0, tot = ls_moments(ops, xs, q, C)
        cnt = (s <= q).sum(axis=0)
        assert np.array_equal(cm.take("chain_mean"), cnt / float(n)), ("indicator mean", n, C, odd, q)
        p = [Fraction(int(c), n) for c in cnt]
        exact = np.array([float(v * (1 - v)) for v in p])
        k = cdiv(n, 4) + 4
        bound = (k + 6) * U * exact + (U * cnt / n) ** 2
        worst = max(worst, ratio_of(np.abs(g0.take("chain_g0") - exact), bound, f"indicator gamma_0 n={n} C={C} q={q}"))
        assert tot[2] == float(np.sum(~np.isfinite(s))), ("out[2] in indicator mode", n, C, odd, q, tot[2])
        assert tot[0] == math.fsum(cnt / float(n)) or abs(tot[0] - math.fsum(cnt / float(n))) <= \
            sum_rows_bound(2 * cdiv(C, EM_WAVE), float(np.sum(cnt)) / n)
    say(f"split moments, indicator n={n} N={N} C={C} gamma_0", worst)
    return worst


BAD_VALUES = (NAN, np.inf, -np.inf)


def check_bad_count(ops, n=33, C=130):
    """out[2] is the exact number of non-finite draws of the split set, raw and in indicator mode: one NaN / +inf / -inf
    at a time in rows 0, n - 1, N - n, N - 1, in chain 64 (second workgroup) and the last chain of the ragged third; several
    at once; for odd N a NaN in the dropped middle row counts 0 and changes no output bit."""
    assert C > 128 and C % 64
    seen = 0
    for odd in (0, 1):
        N = 2 * n + odd
        x = np.random.default_rng([n, C, odd]).normal(size=(N, C))
        cells = [(r, c) for r in (0, n - 1, N - n, N - 1) for c in (0, 64, C - 1)]
        xs = Slack(ops, N, C, pad=3, extra=1, off=2, fill=POISON, data=x)
        base = {}
        for q in (None, 0.1):
            cm, g0, tot = ls_moments(ops, xs, q, C)
            assert tot[2] == 0.0
            base[q] = (cm.take(), g0.take(), tot)
        for i, (r, c) in enumerate(cells):
            for q in (None, 0.1):
                v = BAD_VALUES[(i + (q is not None)) % 3]
                xs.t[r, c] = v
                cm, g0, tot = ls_moments(ops, xs, q, C)
                assert tot[2] == 1.0, ("one non-finite draw", v, "row", r, "chain", c, "N", N, "q", q, "counted", tot[2])
                m = cm.take()
                h = 0 if r < n else 1
                keep = np.ones(2 * C, dtype=bool)
                keep[h * C + c] = False
                assert np.array_equal(m[keep], base[q][0][keep]), "a non-finite draw reached another chain's mean"
                xs.t[r, c] = float(x[r, c])
                seen += 1
        for q in (None, 0.1):  # several at once, two of them in one chain
            for j, (r, c) in enumerate(cells + [(1, 64), (N - 2, C - 1)]):
                xs.t[r, c] = BAD_VALUES[j % 3]
            _, _, tot = ls_moments(ops, xs, q, C)
            assert tot[2] == float(len(cells) + 2), ("several non-finite draws", N, q, tot[2])
            xs.t.copy_(torch.from_numpy(x))
        if odd:
            for q in (None, 0.1):
                xs.t[n, :] = NAN
                cm, g0, tot = ls_moments(ops, xs, q, C)
                assert tot[2] == 0.0, ("the dropped middle row was counted", q, tot[2])
                assert np.array_equal(cm.take(), base[q][0]) and np.array_equal(g0.take(), base[q][1])
                assert np.array_equal(tot, base[q][2])
                xs.t[n, :] = torch.from_numpy(x[n])
        xs.take("x")
    say("out[2] non-finite counts", f"{seen} single placements, exact")
    return seen


def bsq_inputs(M, seed=0):
    """Means with a common offset of 1e6 against a spread of 1e-3 (where the centred second pass matters)."""
    mean = 1e6 + 1e-3 * np.random.default_rng([M, seed, 3]).normal(size=M)
    return mean, math.fsum(mean) / M


def check_between_sq(ops, M):
    mean, centre = bsq_inputs(M)
    d = mean - centre
    assert np.array_equal(d.astype(np.longdouble), mean.astype(np.longdouble) - np.longdouble(centre))  # (exact)
    hi, lo = two_square(d)
    want = math.fsum(np.concatenate([hi, lo]))
    buf = torch.full((M + 5,), POISON, dtype=F64, device=ops.device)
    buf[2:2 + M] = dev(mean, ops)
    got = ops.ess_between_sq(buf[2:2 + M], dev(np.array([centre, POISON]), ops)[:1])
    assert got.shape == (1,)
    # per term the subtraction and the square, the wave sum and tree of k_between_sq (6 + 3), then k_sum_rows
    bound = 2 * U * want + sum_rows_bound(cdiv(M, EM_BLOCK), want) + 3 * U * want
    r = ratio_of(abs(float(got[0]) - want), bound, f"between_sq M={M}")
    say(f"between_sq M={M}", r)
    return r


# =====================================================================================================================
# 3. ops.ess_acov_sums, ops.ess_indicator, ops.select_ranks
# =====================================================================================================================
ACOV_CASES = ((1, 9, 0, 9), (255, 9, 2, 5), (256, 9, 2, 5), (257, 9, 2, 5), (700, 70, 5, 65), (65_600, 5, 1, 3))
ACOV_LONG = (3, 66_000, (0, 65_534, 65_535, 65_536, 65_999))


def two_prod(a, b):
    """(hi, lo) with hi + lo = a * b exactly (Veltkamp / Dekker; magnitudes of order one)."""
    hi = a * b

    def split_(v):
        s = v * 134217729.0
        h = s - (s - v)
        return h, v - h

    a1, a2 = split_(a)
    b1, b2 = split_(b)
    return hi, a2 * b2 - (((hi - a1 * b1) - a2 * b1) - a1 * b2)


def acov_bound(C, sum_abs):
    """One rounded product per chain, k_acov_sums' wave sum and tree over 256 chains (8 levels in all, as rp_bound), then
    k_sum_rows over the cdiv(C, 256) partials, and one to spare."""
    return (1 + 8 + cdiv(cdiv(C, EM_BLOCK), EM_BLOCK) + 6 + 3 + 1) * U * sum_abs


def check_acov_sums(ops, C, rows, lag0, nlags, check_lags=None, seed=0):
    """A synthetic autocorrelation in a wider buffer; chains 1 and C - 2 have gamma_0 = 0 and an all-NaN column: they must
    contribute exactly 0."""
    rng = np.random.default_rng([C, rows, seed, 11])
    acor = rng.uniform(-1.0, 1.0, size=(rows, C))
    g0 = rng.uniform(0.5, 2.0, size=C) * 10.0 ** rng.integers(-3, 4, size=C)
    for c in ((1, C - 2) if C >= 3 else ()):
        g0[c] = 0.0
        acor[:, c] = NAN
    a = Slack(ops, rows, C, pad=3, extra=2, off=1, fill=POISON, data=acor)
    gv = torch.full((C + 3,), POISON, dtype=F64, device=ops.device)
    gv[:C] = dev(g0, ops)
    got = ops.ess_acov_sums(a.t, gv[:C], lag0, nlags)
    assert got.shape == (nlags,)
    got = got.cpu().numpy()
    live = g0 != 0.0
    ks = np.arange(nlags) if check_lags is None else np.asarray(check_lags) - lag0
    err, bound = np.empty(len(ks)), np.empty(len(ks))
    for i, k in enumerate(ks):
        hi, lo = two_prod(acor[lag0 + k, live], g0[live])
        want = math.fsum(np.concatenate([hi, lo]))
        err[i] = abs(got[k] - want)
        bound[i] = acov_bound(C, math.fsum(np.abs(hi))) + U * abs(want)
    assert np.all(np.isfinite(got)), "a NaN autocorrelation of a constant chain reached the sum"
    r = ratio_of(err, bound, f"acov_sums C={C} rows={rows} lag0={lag0} nlags={nlags}")
    a.take("acor")
    say(f"acov_sums C={C} rows={rows} lag0={lag0} nlags={nlags}", r)
    return r


IND_N = (1, 4095, 4096, 4097, 9000)
IND_C = (1, 255, 256, 257)


def check_indicator(ops, n, C):
    """out bit-equal to (x <= q) on strided input and output views: ties, -0.0 against q = 0.0, NaN (gives 0), +-inf."""
    x = sm_indicator_data(n, C, seed=1)
    x[np.random.default_rng([n, C, 9]).uniform(size=(n, C)) < 0.02] = NAN
    if n * C >= 8:
        x.reshape(-1)[:4] = [0.3, -0.0, NAN, np.inf]
    xs = Slack(ops, n, C, pad=3, extra=1, off=2, fill=POISON, data=x)
    for q in (0.0, 0.3):
        out = Slack(ops, n, C, pad=5, extra=2, off=1)
        ops.ess_indicator(xs.t, q, out.t)
        with np.errstate(invalid="ignore"):
            want = (x <= q).astype(np.float64)
        got = out.take("indicator")
        assert np.array_equal(got, want), ("indicator", n, C, q, "first cell", tuple(np.argwhere(got != want)[0]))
    xs.take("x")
    return True


def check_select_ranks(ops):
    """n = 0 (nothing runs), 256, 257; 8 targets; targets nobody holds leave `out` alone; 9 targets are refused."""
    rng = np.random.default_rng(21)
    for n in (0, 256, 257):
        ranks = torch.full((n + 4,), POISON, dtype=F64, device=ops.device)
        vals = torch.full((n + 4,), POISON, dtype=F64, device=ops.device)
        r, v = rng.permutation(n) + 1.0, rng.normal(size=n)
        ranks[:n], vals[:n] = dev(r, ops), dev(v, ops)
        targets = np.array([1.0, float(n), float(n // 2), 2.0, n + 1.0, 0.0, 0.5, 1e300])  # the last four: nobody's (1e300: behind the view)
        out = SlackVec(ops, 8)
        ops.select_ranks(ranks[:n], vals[:n], dev(targets, ops), out.t)
        got = out.take("select_ranks")
        for j, t in enumerate(targets):
            hit = np.nonzero(r == t)[0]
            if hit.size:
                assert got[j] == v[hit[0]], (n, j, t)
            else:
                assert np.isnan(got[j]), ("a target nobody holds was written", n, j, t)
    # a rank without chains: torch hands an empty tensor over as a null pointer, and n = 0 must still be a no-op
    empty, out = torch.empty(0, dtype=F64, device=ops.device), SlackVec(ops, 8)
    ops.select_ranks(empty, empty, dev(targets, ops), out.t)
    assert np.isnan(out.take("select_ranks, empty rank")).all()
    out = SlackVec(ops, 9)
    nine = dev(np.arange(1.0, 10.0), ops)
    if has_abi(ops):
        assert status_of(ops, "bk_select_ranks", _ptr(ranks), _ptr(vals), 257, _ptr(nine), 9, _ptr(out.t), _stream(ops)) == BK_E_ARG
    else:
        try:
            ops.select_ranks(ranks[:257], vals[:257], nine, out.t)
        except ValueError:
            pass
        else:
            raise AssertionError("nine targets were accepted")
    assert np.isnan(out.take()).all()
    return True


# =====================================================================================================================
# 4. The FFT hand-over at max_half, and ops.autocorr_fft as this route calls it
# =====================================================================================================================
FFT_ATOL = 2e-12  # test_autocorr_fft_against_numpy's
HAND_OVER_C = 3


def hand_over_lags(n):
    rnd = np.random.default_rng([n, 23]).integers(128, n - 64, size=64)
    return np.unique(np.concatenate([np.arange(128), np.arange(n - 64, n), rnd]))


def check_fft_hand_over(ops, n1=MAX_HALF, C=HAND_OVER_C):
    """ess_lag_sums at n = 20,087 and the FFT route (_lag_sums_fft) at n = 20,088 on series whose halves share their first
    20,087 draws; the extra draw of each half is that half's mean (check_hand_over's construction), so its centred value
    is zero to rounding and n Gamma_t is the same sum on both sides.  Each side against the long-double reference of its
    own staged data -- the lag sums at their bound, the FFT route at 2e-12 sum gamma_0 (the atol its autocorrelations are
    held to) plus the acov_sums bound -- and n Gamma_t of the two within twice the larger."""
    if n1 == MAX_HALF:
        assert lag_plan(n1)[0] == 1 and lag_plan(n1 + 1)[0] == 0
    base = ar1_series(2 * n1, C, seed=5)
    x2 = np.empty((2 * n1 + 2, C))
    for h, rows in ((0, base[:n1]), (1, base[n1:])):
        x2[h * (n1 + 1):h * (n1 + 1) + n1] = rows
        x2[h * (n1 + 1) + n1] = [math.fsum(rows[:, c]) / n1 for c in range(C)]
    lags = hand_over_lags(n1)
    sides = []
    for x, n, fft in ((base, n1, False), (x2, n1 + 1, True)):
        xs = Slack(ops, 2 * n, C, pad=3, extra=1, off=2, fill=POISON, data=x)
        cm, g0, _ = ls_moments(ops, xs, None, C)
        mean, gam0 = cm.take(), g0.take()
        d = ref.split(x) - mean
        want, sabs, ld_err = ls_reference(d, lags)
        if fft:
            got = dg._lag_sums_fft(xs.t, None, g0.t, ops).cpu().numpy()[lags]
            tol = FFT_ATOL * math.fsum(gam0) + acov_bound(C, sabs) + 2 * ld_err * sabs
        else:
            got = ops.ess_lag_sums(xs.t, None, cm.t, 0, n).cpu().numpy()[lags]
            tol = np.array([ls_depth(n, int(k), 1, True, 2 * C) for k in lags]) * U * sabs + ld_err * sabs
        r = ratio_of(np.abs(got - want), tol, "fft route" if fft else "lag sums" + f" at n={n}")
        say(f"hand-over: {'fft route' if fft else 'lag sums'} at n={n} against long double", r)
        sides.append((got * n, np.broadcast_to(tol, got.shape) * n, r))
        xs.take("x")
    pair = 2 * np.maximum(sides[0][1], sides[1][1])
    r = ratio_of(np.abs(sides[0][0] - sides[1][0]), pair, "lag sums against the fft route")
    say(f"hand-over: n Gamma_t of the two routes, {len(lags)} lags", r)
    return sides[0][2], sides[1][2], r


WIDE_FFT = [(N, C) for N in (33, 257) for C in (2047, 2048, 2049)]


def fft_series(N, C, seed=0):
    """test_autocorr_fft_against_numpy's inputs: AR(1) of four persistences, scales 1e-6 .. 1e6 and offsets side by side."""
    from scipy.signal import lfilter

    rng = np.random.default_rng([N, C, seed, 31])
    e = rng.normal(size=(N, C))
    x = np.empty((N, C))
    for j, phi in enumerate((0.0, 0.5, 0.95, 0.999)):
        x[:, j::4] = lfilter([1.0], [1.0, -phi], e[:, j::4], axis=0)
    c = np.arange(C)
    return (x + 10.0 * (c % 3)) * 10.0 ** (3 * (c % 5) - 6)


def fft_reference(x):
    """autocorr.py:23-33 with numpy.fft for every column."""
    N = x.shape[0]
    size = 1 << int(np.ceil(np.log2(2 * N - 1)))
    nd = x - x.mean(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.fft.ifft(np.abs(np.fft.fft(nd, size, axis=0)) ** 2, axis=0).real[:N] / np.var(x, axis=0) / N


def check_autocorr_fft_wide(ops, N, C):
    """1,024 and more complex columns take the 256-column row pitch (ldc = Cp + 36 off a multiple of 256) and 17 column
    blocks; 2,047 chains stay on the other side."""
    x = fft_series(N, C)
    xs = Slack(ops, N, C, pad=3, extra=1, off=0, fill=POISON, data=x)
    out = Slack(ops, N, C, pad=1, extra=1)
    ops.autocorr_fft(xs.t, out.t)
    got = out.take("autocorr_fft")
    err = np.abs(got - fft_reference(x))
    r = ratio_of(err, np.full(err.shape, FFT_ATOL), f"autocorr_fft N={N} C={C}")
    assert np.allclose(got[0], 1.0, rtol=0, atol=1e-13)
    say(f"autocorr_fft N={N} C={C} Cp={(C + 1) // 2}", r, "max err / 2e-12")
    return r


def check_autocorr_fft_non_finite(ops, N=33, C=7):
    """One NaN, then one +inf, in one column: that column comes back all NaN, every other column -- its partner in the
    complex pair first of all -- stays within 2e-12 of its own reference.  The bad column even, odd, and the last,
    unpaired column of an odd C."""
    assert C % 2 == 1
    x = fft_series(N, C, seed=1)
    want = fft_reference(x)
    worst = 0.0
    for bad_col in (2, 3, C - 1):
        for v in (NAN, np.inf):
            xb = x.copy()
            xb[N // 2, bad_col] = v
            xs = Slack(ops, N, C, pad=3, extra=1, off=1, fill=POISON, data=xb)
            out = Slack(ops, N, C, pad=2, extra=1, off=1)
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                ops.autocorr_fft(xs.t, out.t)
            got = out.take("autocorr_fft")
            assert np.isnan(got[:, bad_col]).all(), ("the column holding", v, "is not all NaN", bad_col)
            rest = np.arange(C) != bad_col
            err = np.abs(got[:, rest] - want[:, rest])
            worst = max(worst, ratio_of(err, np.full(err.shape, FFT_ATOL), f"autocorr_fft C={C} bad column {bad_col} ({v})"))
    say(f"autocorr_fft N={N} C={C}, a NaN / +inf column beside finite ones", worst, "max err / 2e-12")
    return worst


# =====================================================================================================================
# 5. End to end, one case per instance
# =====================================================================================================================
E2E_N = (535, 1143, 2359, 4791, 9655, 10_007, MAX_HALF)
E2E_FUNCS = ("ess_mean", "ess_bulk", "ess_tail", "ess_quantile", "mcse_mean")
E2E_REL = 1e-9
E2E_PAIR_MARGIN = 1e-9
# seeds replaced because a pair sum the reference scan tests sat within 1e-9 of zero: {n: seed}
E2E_REPLACED_SEEDS = {}


def e2e_series(n):
    return ar1_series(2 * n, 2 * lag_plan(n)[0] + 3, E2E_REPLACED_SEEDS.get(n, 0))


def scan_pairs(ch):
    """(smallest |r_even + r_odd| over the pairs ref.scan tests, max_t) for split chains ch [n, M]."""
    n, M = ch.shape
    g = ref.autocov(ch)
    W = np.mean(g[0]) * n / (n - 1)
    vp = W * (n - 1) / n + np.var(ch.mean(axis=0), ddof=1)
    rho = 1 - (W - g.mean(axis=1)) / vp
    t, pair, margin = 0, 1.0 + rho[1], abs(1.0 + rho[1])
    while t < n - 5 and pair > 0:
        t += 2
        pair = rho[t] + rho[t + 1]
        margin = min(margin, abs(pair))
    assert t == ref.scan(g.mean(axis=1), W, vp, M, n)[1]
    return margin, t


@functools.lru_cache(maxsize=None)
def e2e_reference(n):
    """The five values of tests/multichain_ess_ref.py, the smallest pair sum any of their scans tested and the largest
    max_t (computed once per process, shared by every test that needs it, never changed)."""
    x = e2e_series(n)
    s = ref.split_rows(x)
    chains = [ref.split(x), ref.split(ref.z_scores(x))]
    chains += [ref.split((s <= np.quantile(s, p)).astype(np.float64)) for p in (0.05, 0.95, 0.3)]
    pairs = [scan_pairs(ch) for ch in chains]
    want = {"ess_mean": ref.ess_mean(x), "ess_bulk": ref.ess_bulk(x), "ess_tail": ref.ess_tail(x),
            "ess_quantile": ref.ess_quantile(x, 0.3), "mcse_mean": ref.mcse_mean(x)}
    return want, min(p[0] for p in pairs), max(p[1] for p in pairs)


def check_end_to_end(ops, n):
    want, margin, max_t = e2e_reference(n)
    assert margin > E2E_PAIR_MARGIN, ("a tested pair within 1e-9 of zero: replace the seed (E2E_REPLACED_SEEDS)", n, margin)
    assert max_t >= 64, ("no second lag round", n, max_t)
    x = e2e_series(n)
    xs = Slack(ops, x.shape[0], x.shape[1], pad=3, extra=1, off=2, fill=POISON, data=x)
    worst = 0.0
    for f in E2E_FUNCS:
        got = getattr(bk, f)(xs.t, 0.3, ops=ops) if f == "ess_quantile" else getattr(bk, f)(xs.t, ops=ops)
        rel = abs(float(got) / want[f] - 1.0)
        assert rel <= E2E_REL, (f, n, float(got), want[f], rel)
        worst = max(worst, rel)
    xs.take("x")
    say(f"end to end n={n} C={x.shape[1]} G={lag_plan(n)[0]} (reference max_t {max_t})", worst / E2E_REL, "max rel err / 1e-9")
    return worst / E2E_REL


def _five(ops, t):
    return [float(bk.ess_mean(t, ops=ops)), float(bk.ess_bulk(t, ops=ops)), float(bk.ess_tail(t, ops=ops)),
            float(bk.ess_quantile(t, 0.3, ops=ops)), float(bk.mcse_mean(t, ops=ops))]


def check_non_finite_end_to_end(ops, n=300, C=5):
    """A NaN or an infinity in a row of the split set: all five functions give NaN.  A NaN only in the dropped middle row
    of an odd N: the values of the same data with that cell finite, bit for bit."""
    N = 2 * n + 1
    x = ar1_series(N, C, seed=3)
    xs = Slack(ops, N, C, pad=3, extra=1, off=2, fill=POISON, data=x)
    base = _five(ops, xs.t)
    assert all(np.isfinite(base))
    for (r, c), v in (((0, 0), NAN), ((n - 1, C - 1), np.inf), ((N - n, 2), -np.inf), ((N - 1, 1), NAN)):
        xs.t[r, c] = v
        got = _five(ops, xs.t)
        assert all(np.isnan(got)), ("a non-finite draw in row", r, "gave", got)
        xs.t[r, c] = float(x[r, c])
    xs.t[n, 3] = NAN
    got = _five(ops, xs.t)
    assert got == base, ("a NaN in the dropped middle row changed a value", got, base)
    xs.t[n, 3] = float(x[n, 3])
    assert _five(ops, xs.t) == base
    xs.take("x")
    return True
