"""CPU side of the multi-chain ESS kernels' edge work: the references of tests/ess_multi_parity.py against each other, the
restated launch plan against the text of csrc/bk_ess_multi.hip, the restatement's split-set rule, and the shared bodies
run on the NumPy stand-in (tests/multichain_ess_ref.MultiEssFakeOps) -- which checks the bodies, their bounds and the
stand-in; the kernels themselves are held to them in tests/test_gpu_ess_multi_kernels.py.  Each body is also shown to notice
a wrong kernel: the ``*_notices_a_planted_defect`` cases run it on a stand-in with one defect planted."""
import math
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import bayes_kit_amd as bk
from tests import ess_multi_parity as ep
from tests import multichain_ess_ref as ref
from tests.multichain_ess_ref import MultiEssFakeOps

CSRC = os.path.join(os.path.dirname(__file__), "..", "bayes-kit_amd", "csrc")


@pytest.fixture(scope="module")
def ops():
    return MultiEssFakeOps(max_half=ep.MAX_HALF)


# ---- the references -----------------------------------------------------------------------------------------------------------
def test_long_double_lag_sums_against_fsum_of_exact_products():
    """The long-double sums the lag-sum bound stands on, against math.fsum of exact (two_prod) products: within the stated
    (log2(n M) + 3) 2^-64 sum |terms| plus the rounding of the reference to float64 -- a hundredth of u sum |terms|, which
    LS_CONST's spare covers."""
    rng = np.random.default_rng(1)
    d = rng.normal(size=(301, 6)) * np.array([1e-3, 1.0, 1e3, 1.0, 7.0, 0.1])
    lags = np.array([0, 1, 63, 64, 65, 200, 299, 300])
    for cells in (ep.LS_WHOLE_CELLS, 100):  # the whole-array route, and the row-slice route of the large inputs
        monkey = ep.LS_WHOLE_CELLS
        ep.LS_WHOLE_CELLS = cells
        try:
            want, sabs, ld_err = ep.ls_reference(d, lags)
        finally:
            ep.LS_WHOLE_CELLS = monkey
        for k, w, s, e in zip(lags, want, sabs, ld_err):
            hi, lo = ep.two_prod(d[:301 - k].reshape(-1), d[k:].reshape(-1))
            exact = Fraction(math.fsum(np.concatenate([hi, lo]))) / 301
            assert abs(Fraction(w) - exact) <= Fraction(e * s) + Fraction(ep.U * abs(w)) * 2
            assert s >= math.fsum(np.abs(hi)) / 301
    assert ep.ls_longdouble_error(ep.MAX_HALF, 10) < 0.011 * ep.U
    assert ep.ls_longdouble_error(5000, 8192, rows=968) < 0.5 * ep.U  # (the chunked case: against a depth of 75 u)


def test_two_prod_is_exact():
    rng = np.random.default_rng(0)
    a, b = rng.uniform(-1, 1, size=500), rng.uniform(0.5, 2.0, size=500) * 10.0 ** rng.integers(-3, 4, size=500)
    hi, lo = ep.two_prod(a, b)
    for x, y, h, l in zip(a, b, hi, lo):
        assert Fraction(x) * Fraction(y) == Fraction(h) + Fraction(l)


def test_exact_split_moments_against_long_double():
    x = ep.cmv_data("offset", 130, 4)
    s = ref.split(x)
    ex = ep.sm_exact(s)
    ld = s.astype(np.longdouble)
    mu = ld.sum(axis=0) / 65
    g0 = ((ld - mu) ** 2).sum(axis=0) / 65
    assert np.all(np.abs(ex[0] - mu.astype(np.float64)) <= 2 * ep.U * np.abs(ex[0]))
    assert np.all(np.abs(ex[1] - g0.astype(np.float64)) <= 1e-12 * ex[1])
    one = ep.sm_exact(np.array([[3.0, -2.0]]))
    assert one[0].tolist() == [3.0, -2.0] and one[1].tolist() == [0.0, 0.0] and one[3].tolist()[0] < 1e-29


def test_fft_reference_is_the_direct_autocorrelation():
    x = ep.fft_series(33, 9)
    want = ep.fft_reference(x)
    d = x - x.mean(axis=0)
    direct = np.array([(d[:33 - k] * d[k:]).sum(axis=0) for k in range(33)]) / (d * d).sum(axis=0)
    np.testing.assert_allclose(want, direct, rtol=0, atol=1e-13)


# ---- the restated plan against csrc/ ------------------------------------------------------------------------------------------
def test_the_restated_constants_are_the_ones_in_the_source():
    """Matches the source lines literally: meant to trip on any edit of them, so that whoever changes a launch constant looks
    at the restatement in tests/ess_multi_parity.py."""
    src = open(os.path.join(CSRC, "bk_ess_multi.hip")).read()
    assert "constexpr int EM_BLOCK = 256, EM_WAVES = EM_BLOCK / BK_WAVE;" in src and ep.EM_BLOCK == 256
    assert f"constexpr int EM_RT_MIN = {ep.EM_RT_MIN}, EM_RT_TAIL = {ep.EM_RT_TAIL};" in src
    assert "p.pitch = (int)((p.rt ? n + EM_RT_TAIL : n + 1) | 1);" in src
    assert "const i64 red = EM_WAVES * BK_WAVE;" in src and ep.EM_RED == 256
    assert "const i64 cap = (i64)(160 * 1024 - 512) / 8 - red, cap2 = (i64)(78 * 1024) / 8 - red;" in src
    assert (ep.EM_CAP, ep.EM_CAP2) == (20_160, 9_728)
    assert src.count("for (int g : {16, 8, 4, 2, 1})") == 2 and "if ((i64)g * p.pitch <= cap2)" in src
    assert "p.bytes = ((size_t)p.G * p.pitch + red) * 8;" in src and "if (p.bytes > 64 * 1024)" in src
    assert "constexpr i64 EM_PART_BYTES = (i64)256 << 20;" in src
    assert "const i64 cap = EM_PART_BYTES / 8 / lag_blocks(C, G) / BK_WAVE * BK_WAVE;" in src
    assert "i64 lag_blocks(i64 C, int G) { return 2 * bk_cdiv(C, G); }" in src
    assert "i64 B = 2 * bk_cdiv(C, BK_WAVE) * 3;" in src and "bk_cdiv(2 * C, EM_BLOCK)" in src
    assert "p.G ? lag_blocks(C, p.G) * lag_chunk(C, p.G, nlags) : bk_cdiv(C, EM_BLOCK) * nlags;" in src
    assert "(unsigned)(nlags < 65535 ? nlags : 65535)" in src and "(unsigned)(n < 4096 ? n : 4096)" in src
    assert "k < 1 || k > 8" in src


def test_lag_plan_restatement():
    assert [g for _, g in ep.EM_SEAMS] == [16, 8, 4, 2, 1, 2, 1, 0]
    assert ep.lag_plan(4) == (16, 5, False, (16 * 5 + 256) * 8) and ep.lag_plan(287)[1] == 289
    assert ep.lag_plan(ep.MAX_HALF) == (1, 20_159, True, 163_320) and ep.lag_plan(ep.MAX_HALF + 1)[0] == 0
    assert ep.lag_plan(9655)[:2] == (1, 9727) and ep.lag_plan(9656)[:2] == (2, 9729) and ep.lag_plan(10_007)[0] == 2
    assert ep.work_bytes(5000, 4096, 5000) == 8 * 8192 * 4096 == 256 << 20
    assert ep.work_bytes(1, 1, 1) == 8 * 6 and ep.work_bytes(66_000, 3, 66_000) == 8 * 66_000
    for n, odd, C in ep.LS_CASES:
        G = ep.lag_plan(n)[0]
        assert C in (1, G - 1, G + 1, 2 * G + 3) and odd in (0, 1)
    assert {n for n, _, _ in ep.LS_CASES} == set(ep.LS_N)
    for n in ep.LS_N:  # requests whose later blocks of a pass start at or beyond lag_end exist wherever G <= 2
        if n >= 193:
            assert {(0, 65), (0, 129), (0, 193), (n - 70, 70), (n - 1, 1), (0, n), (37, 100)} <= set(ep.ls_requests(n))
    assert ep.ls_requests(4) == [(0, 4), (3, 1)]
    assert len(ep.ls_compared(ep.MAX_HALF, 0, ep.MAX_HALF)) > 650 and len(ep.ls_compared(2360, 0, 2360)) == 2360


def test_select_ranks_takes_an_empty_rank_whose_arrays_are_null():
    """bk_select_ranks' host side (no device needed: it returns before any launch): n = 0 is a no-op whatever rank and
    values point to -- torch hands an empty tensor over as a null pointer -- while n > 0 with null arrays, and more than
    eight targets, are still refused."""
    import __graft_entry__ as ge

    ge.build()
    from bayes_kit_amd import _lib

    lib = _lib.load()
    targets, out = np.arange(1.0, 10.0), np.full(9, np.nan)
    assert lib.bk_select_ranks(0, 0, 0, targets.ctypes.data, 8, out.ctypes.data, 0) == ep.BK_OK
    assert np.isnan(out).all()
    assert lib.bk_select_ranks(0, 0, 1, targets.ctypes.data, 8, out.ctypes.data, 0) == ep.BK_E_ARG
    assert lib.bk_select_ranks(0, 0, 0, targets.ctypes.data, 9, out.ctypes.data, 0) == ep.BK_E_ARG
    assert lib.bk_select_ranks(0, 0, 0, 0, 8, out.ctypes.data, 0) == ep.BK_E_ARG


# ---- the restatement's split-set rule -------------------------------------------------------------------------------------
def test_bulk_ess_of_the_restatement_looks_at_the_split_set_only(ops):
    """A NaN in the dropped middle row of an odd N is not a draw of the estimator: ref.ess_bulk gives the value of the split
    set (as ref.ess_mean, ref.ess_tail, ref.ess_quantile and the library do), and NaN for a NaN in any other row."""
    x = ref.ar1(np.random.default_rng(9), 201, 4, 0.5)
    clean = {f: getattr(ref, f)(x) for f in ("ess_bulk", "ess_mean", "ess_tail", "mcse_mean")}
    y = x.copy()
    y[100, 2] = np.nan
    for f, v in clean.items():
        assert np.isfinite(v) and getattr(ref, f)(y) == v, f
    assert ref.ess_quantile(y, 0.3) == ref.ess_quantile(x, 0.3)
    t = torch.from_numpy(y)
    assert bk.ess_bulk(t, ops=ops) == pytest.approx(clean["ess_bulk"], rel=1e-9)
    assert bk.ess_mean(t, ops=ops) == pytest.approx(clean["ess_mean"], rel=1e-9)
    for row in (0, 99, 101, 200):
        z = x.copy()
        z[row, 1] = np.nan
        assert np.isnan(ref.ess_bulk(z)) and np.isnan(ref.ess_mean(z)) and np.isnan(bk.ess_bulk(torch.from_numpy(z), ops=ops))


# ---- end to end: the seeds ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ep.E2E_N)
def test_end_to_end_seeds_keep_clear_of_zero_pairs_and_need_a_second_lag_round(n):
    want, margin, max_t = ep.e2e_reference(n)
    ep.say(f"end to end n={n}: smallest tested pair sum {margin:.3g}, largest max_t {max_t}", "")
    assert margin > ep.E2E_PAIR_MARGIN and max_t >= 64 and all(np.isfinite(v) for v in want.values())


# ---- the shared bodies on the stand-in -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,odd,C", ep.LS_CASES)
def test_lag_sums_body_on_the_stand_in(ops, n, odd, C):
    ep.check_lag_sums(ops, n, odd, C)


@pytest.mark.parametrize("n,odd,C", ep.LS_INDICATOR_CASES)
def test_lag_sums_indicator_body_on_the_stand_in(ops, n, odd, C):
    ep.check_lag_sums(ops, n, odd, C, indicator=True)


def test_chunked_lag_sums_body_on_the_stand_in_with_few_chains(ops):
    """(The stand-in has no launches to chunk and pays O(n^2 C): the body, its lag choice and its bound at 16 chains.)"""
    ep.check_lag_sums_chunked(ops, ep.CHUNKED[0], 16)


@pytest.mark.parametrize("C", ep.SM_C)
@pytest.mark.parametrize("n", ep.SM_N)
def test_split_moments_body_on_the_stand_in(ops, n, C):
    ep.check_split_moments(ops, n, C)


def test_split_moments_body_on_the_stand_in_with_258_partials(ops):
    ep.check_split_moments(ops, *ep.SM_WIDE, kinds=("offset",))


@pytest.mark.parametrize("odd", [0, 1])
@pytest.mark.parametrize("n,C", [(1, 1), (4, 65), (33, 130), (64, 63), (1000, 64)])
def test_split_moments_indicator_body_on_the_stand_in(ops, n, C, odd):
    ep.check_split_moments_indicator(ops, n, C, odd)


def test_bad_count_body_on_the_stand_in(ops):
    ep.check_bad_count(ops)


@pytest.mark.parametrize("M", ep.BSQ_M)
def test_between_sq_body_on_the_stand_in(ops, M):
    ep.check_between_sq(ops, M)


@pytest.mark.parametrize("C,rows,lag0,nlags", ep.ACOV_CASES)
def test_acov_sums_body_on_the_stand_in(ops, C, rows, lag0, nlags):
    ep.check_acov_sums(ops, C, rows, lag0, nlags)


def test_acov_sums_body_on_the_stand_in_beyond_65535_lags(ops):
    C, rows, lags = ep.ACOV_LONG
    ep.check_acov_sums(ops, C, rows, 0, rows, check_lags=lags)


@pytest.mark.parametrize("C", ep.IND_C)
@pytest.mark.parametrize("n", ep.IND_N)
def test_indicator_body_on_the_stand_in(ops, n, C):
    ep.check_indicator(ops, n, C)


def test_select_ranks_body_on_the_stand_in(ops):
    ep.check_select_ranks(ops)


def test_fft_hand_over_body_on_the_stand_in(ops):
    ep.check_fft_hand_over(ops)


@pytest.mark.parametrize("N,C", ep.WIDE_FFT)
def test_wide_autocorr_fft_body_on_the_stand_in(ops, N, C):
    ep.check_autocorr_fft_wide(ops, N, C)


def test_non_finite_autocorr_fft_body_on_the_stand_in(ops):
    ep.check_autocorr_fft_non_finite(ops)
    ep.check_autocorr_fft_non_finite(ops, 33, 2049)


@pytest.mark.parametrize("n", ep.E2E_N)
def test_end_to_end_body_on_the_stand_in(ops, n):
    ep.check_end_to_end(ops, n)


def test_non_finite_end_to_end_body_on_the_stand_in(ops):
    ep.check_non_finite_end_to_end(ops)


# ---- each body notices a wrong kernel -----------------------------------------------------------------------------------------
class DropsOneLastTerm(MultiEssFakeOps):
    """The last term of chain 1 at lag 70 is missing."""

    def ess_lag_sums(self, x, q, chain_mean, lag0, nlags):
        out = super().ess_lag_sums(x, q, chain_mean, lag0, nlags)
        if lag0 <= 70 < lag0 + nlags:
            _, s = self._split(x, q)
            n = s.shape[0]
            d = s[:, 1] - chain_mean.numpy()[1]
            out[70 - lag0] -= d[n - 71] * d[n - 1] / n
        return out


class SecondHalfFromRowN(MultiEssFakeOps):
    """Rows [n, 2n) for the second half whatever the parity of N."""

    def ess_lag_sums(self, x, q, chain_mean, lag0, nlags):
        n = x.shape[0] // 2
        return super().ess_lag_sums(x[:2 * n], q, chain_mean, lag0, nlags)


class CountsTheFirstHalfOnly(MultiEssFakeOps):
    def ess_split_moments(self, x, q, chain_mean, chain_g0):
        out = super().ess_split_moments(x, q, chain_mean, chain_g0)
        out[2] = float(np.sum(~np.isfinite(x.numpy()[:x.shape[0] // 2])))
        return out


class MultipliesTheNaNColumn(MultiEssFakeOps):
    def ess_acov_sums(self, acor, chain_g0, lag0, nlags):
        return torch.from_numpy((acor.numpy()[lag0:lag0 + nlags] * chain_g0.numpy()).sum(axis=1))


class StrictlyBelow(MultiEssFakeOps):
    def ess_indicator(self, x, q, out):
        with np.errstate(invalid="ignore"):
            out.numpy()[...] = (x.numpy() < q).astype(np.float64)


def test_lag_sums_body_notices_a_planted_defect():
    ep.check_lag_sums(DropsOneLastTerm(), 65, 0, 3)  # (nothing at lag 70: the planted defect alone changes nothing)
    with pytest.raises(AssertionError, match="lag sums"):
        ep.check_lag_sums(DropsOneLastTerm(), 289, 0, 3)
    with pytest.raises(AssertionError, match="lag sums"):
        ep.check_lag_sums(DropsOneLastTerm(), 2360, 0, 3)
    ep.check_lag_sums(SecondHalfFromRowN(), 288, 0, 3)
    with pytest.raises(AssertionError, match="lag sums|non-finite"):
        ep.check_lag_sums(SecondHalfFromRowN(), 288, 1, 3)


def test_split_moments_body_notices_a_planted_defect():
    with pytest.raises(AssertionError, match="one non-finite draw"):
        ep.check_bad_count(CountsTheFirstHalfOnly())
    with pytest.raises(AssertionError, match=r"out\[2\] in indicator mode"):
        ep.check_split_moments_indicator(CountsTheFirstHalfOnly(), 33, 130, 0)


def test_acov_sums_body_notices_a_planted_defect():
    ep.check_acov_sums(MultipliesTheNaNColumn(), 1, 9, 0, 9)  # (one chain: no NaN column)
    with pytest.raises(AssertionError, match="NaN autocorrelation|non-finite"):
        ep.check_acov_sums(MultipliesTheNaNColumn(), 257, 9, 2, 5)


def test_indicator_body_notices_a_planted_defect():
    with pytest.raises(AssertionError, match="indicator"):
        ep.check_indicator(StrictlyBelow(), 4097, 1)
