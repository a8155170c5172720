"""CPU side of the diagnostic kernels' edge work: the exact references of tests/diag_kernel_parity.py against mpmath, NumPy's
own mean / variance inside the derived bounds, the restated launch decisions against the constants in csrc/, and the shared
bodies run on the NumPy stand-in (tests/fake_ops.FakeOps) -- which checks the bodies, their bounds and the stand-in; the
kernels themselves are held to them in tests/test_gpu_diag_kernels.py.  Each body is also shown to notice a wrong kernel:
the ``*_body_notices_a_planted_defect`` cases run it on a stand-in with one defect planted."""
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from oracle import diagnostics as od
from tests import diag_kernel_parity as dk
from tests.fake_ops import FakeOps

CSRC = os.path.join(os.path.dirname(__file__), "..", "bayes-kit_amd", "csrc")


@pytest.fixture(scope="module")
def ops():
    return FakeOps()


# ---- the references ---------------------------------------------------------------------------------------------------------
def test_exact_mean_and_variance_against_mpmath_at_50_digits():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    for kind in dk.CMV_DATA:
        x = dk.cmv_data(kind, 33, 4)
        for c in range(4):
            col = [mp.mpf(float(v)) for v in x[:, c]]
            mu = mp.fsum(col) / 33
            var = mp.fsum((v - mu) ** 2 for v in col) / 32
            em, ev = dk.exact_mean_var(x[:, c])
            assert abs(mp.mpf(em.numerator) / em.denominator - mu) <= mp.mpf(10) ** -45 * abs(mu), (kind, c)
            assert abs(mp.mpf(ev.numerator) / ev.denominator - var) <= mp.mpf(10) ** -45 * var, (kind, c)
    assert dk.exact_mean_var(np.array([3.0])) == (Fraction(3), None)
    assert dk.exact_mean_var(np.array([1.0, 2.0, 4.0])) == (Fraction(7, 3), Fraction(7, 3))


def test_long_double_moments_agree_with_the_exact_ones_within_their_stated_error():
    x = dk.cmv_data("offset", 1000, 8)
    lengths = dk.cmv_lengths(1000, 8, True)
    lm, lv, sabs = dk.cmv_longdouble(x, lengths)
    ref = dk.cmv_reference(x, lengths, np.arange(8))
    rerr = (np.log2(lengths) + 2.0) * 2.0 ** -64
    assert np.all(np.abs(lm - ref[0]) <= rerr * sabs / lengths + dk.U * np.abs(ref[0]))  # (+ the rounding to float64)
    assert np.all(np.abs(lv - ref[1]) <= 8 * rerr * ref[1] + dk.U * ref[1])


def test_two_square_is_exact():
    d = np.random.default_rng(0).normal(size=1000) * 1e-3
    hi, lo = dk.two_square(d)
    for v, h, l in zip(d, hi, lo):
        assert Fraction(v) ** 2 == Fraction(h) + Fraction(l)


def test_numpy_mean_and_variance_are_what_the_stand_in_returns(ops):
    """FakeOps.chain_mean_var is np.mean / np.var(ddof=1): the body passing on it (below, on every input) is NumPy's own
    mean and variance sitting inside the derived bounds, which therefore stand on the exact reference alone."""
    x = dk.cmv_data("offset", 65, 5)
    m, v = torch.empty(5, dtype=torch.float64), torch.empty(5, dtype=torch.float64)
    ops.chain_mean_var(torch.from_numpy(x), None, m, v)
    assert m.tolist() == [np.mean(x[:, c]) for c in range(5)] and v.tolist() == [np.var(x[:, c], ddof=1) for c in range(5)]


def test_scipy_ndtri_is_within_1e_15_of_mpmath_on_the_rank_normalize_inputs():
    pytest.importorskip("mpmath")
    pb = dk.rn_problem()
    for b, name in ((0, "central"), (1, "tail x < 8"), (2, "tail x >= 8")):
        dk.say(f"scipy.special.ndtri {name}, {int((pb['branch'] == b).sum())} points: max rel err", float(pb["sp_err"][pb["branch"] == b].max()), "")
    assert pb["sp_err"].max() < 1e-15
    # the double the kernel forms reaches both tails' deep branch and the specials
    assert (pb["branch"] == 2).sum() >= 8 and (pb["branch"] == -1).sum() >= 3


def test_pairs_reference_is_the_oracle_on_real_autocorrelations():
    x = dk.ar1_series(400, 6)
    a = np.stack([od.autocorr(x[:, c]) for c in range(6)], axis=1)
    for est, fn in ((0, od.iat_imse), (1, od.iat_ipse)):
        stop, iat, ess, _ = dk.pairs_reference(a, est)
        assert stop.tolist() == [od._end_pos_pairs(a[:, c]) for c in range(6)]
        np.testing.assert_allclose(iat, [fn(x[:, c]) for c in range(6)], rtol=1e-13)
        np.testing.assert_allclose(ess, [400 / fn(x[:, c]) for c in range(6)], rtol=1e-13)


def test_the_truncation_pairs_of_the_most_persistent_chains_are_clear_of_zero():
    """phi = 0.999: long-double direct lag sums agree with the oracle's FFT pair sum at the pair the scan stops at, and that
    sum is farther than 1e-9 from zero -- no chain of the ESS cases owes its result to the sign of a rounding error."""
    seen = 0
    for N, C in dk.ESS_CASES:
        if C < 6 or N > 5000:  # (chain 5 is the first with phi = 0.999; the long-double sums are O(N) per pair)
            continue
        x = dk.ar1_series(N, C)
        for c in range(5, C, 6 * 4):
            a = od.autocorr(x[:, c])
            n = od._end_pos_pairs(a)
            if n + 1 >= N:
                continue
            pair = dk.direct_pair_sum_ld(x[:, c], n)
            assert abs(pair - (a[n] + a[n + 1])) < 1e-12 and pair < -dk.PAIR_MARGIN, (N, C, c, pair)
            seen += 1
    assert seen >= 8


# ---- the restated launch decisions against csrc/ -------------------------------------------------------------------------------
def _src(name):
    return open(os.path.join(CSRC, name)).read()


def test_the_restated_constants_are_the_ones_in_the_sources():
    """Matches the source lines literally, spacing and casts included: it is meant to trip on any edit of them, so that
    whoever changes a launch constant (or only reformats it) looks at the restatement in tests/diag_kernel_parity.py."""
    diag, common, wf = _src("bk_diag.hip"), _src("bk_common.hpp"), _src("bk_welford.hpp")
    assert f"ET_RT_MIN_DRAWS = {dk.ET_RT_MIN_DRAWS}, ET_RT_TAIL = {dk.ET_RT_TAIL}" in diag
    assert "const i64 cap = (i64)(160 * 1024 - 512) / 8;" in diag and dk.ET_CAP == 20_416
    assert "const i64 cap2 = (i64)(78 * 1024) / 8;" in diag and dk.ET_CAP2 == 9_984
    assert "if (bytes > 64 * 1024)" in diag and "for (int g : {16, 8, 4, 2, 1})" in diag
    assert "(rt ? N + ET_RT_TAIL : N) | 1" in diag
    assert f"constexpr int PC_BLOCK = {dk.PC_BLOCK};" in diag
    assert "return elems * 8 > ((i64)192 << 20);" in common and "bk_streams_past_llc(3 * C * D)" in diag
    assert re.search(r"C % 2 == 0 && ld % 2 == 0 && ld_th % 2 == 0 && bk_aligned16\(mean\) && bk_aligned16\(m2\) && "
                     r"bk_aligned16\(theta\)", wf)


def test_ess_group_restatement():
    assert [dk.ess_group(n) for n in (4, 287, 288)] == [(16, 16 * 5 * 8), (16, 16 * 287 * 8), (16, 16 * 361 * 8)]
    assert dk.ess_pitch(551) == 623 and 16 * 623 <= dk.ET_CAP2 < 16 * dk.ess_pitch(552)
    assert [dk.ess_group(n)[0] for n in (439, 440, 951, 952, 1975, 1976, 4023, 4024, 8119, 8120)] == [16, 16, 8, 8, 4, 4, 2, 2, 1, 1]
    assert [dk.ess_group(n)[1] > dk.ET_OPT_IN for n in (439, 440, 951, 952, 1975, 1976, 4023, 4024, 8119, 8120)] == [False, True] * 5
    assert dk.ess_group(20_343) == (1, 20_415 * 8) and dk.ess_group(20_344) == (0, 0) and dk.ess_group(40_000) == (0, 0)
    for N, C in dk.ESS_CASES:
        G = dk.ess_group(N)[0]
        assert C == 1 or (G == 0 and C in (3, 65)) or C in (G - 1, G + 1, 2 * G + 3) or (G == 1 and C == 7)
    assert all((N, 7) in dk.ESS_CASES and (N, 7) in dk.AUTOCORR_CASES for N in dk.ESS_N if dk.ess_group(N)[0] == 1)
    assert {N for N, _ in dk.AUTOCORR_CASES} == set(dk.ESS_N) - {40_000}
    assert all((20_344, C) in dk.AUTOCORR_CASES and (20_344, C) in dk.ESS_CASES for C in (1, 3, 65))


def test_welford_branch_restatement():
    base = torch.zeros(8 * 10 + 2, dtype=torch.float64)
    assert base.data_ptr() % 16 == 0
    a = base[:80].view(8, 10)
    even, shifted, odd_c = a[:, :6], a[:, 1:7], a[:, :5]
    b11 = torch.zeros(8 * 11, dtype=torch.float64).view(8, 11)[:, :6]  # odd pitch
    assert dk.welford_branch(even, even, even) == "v2"
    assert dk.welford_branch(shifted, even, even) == dk.welford_branch(even, shifted, even) == "scalar"
    assert dk.welford_branch(even, even, shifted) == "scalar"
    assert dk.welford_branch(odd_c, odd_c, odd_c) == "scalar"
    assert dk.welford_branch(even, even, b11) == dk.welford_branch(b11, b11, even) == "scalar"
    # the sizes: shape (v) streams past the cache, config 4's 32,768 x 101 does not
    assert 3 * 65_536 * 132 * 8 == 207_618_048 > (192 << 20) == 201_326_592 > 3 * 32_768 * 101 * 8
    for name, (C, D, coff, th_pad, _) in dk.WF_SHAPES.items():
        want = "scalar" if (C % 2 or coff or th_pad % 2) else ("v2_nt" if 3 * C * D * 8 > (192 << 20) else "v2")
        assert dk.WF_BRANCH[name] == want, name
    assert set(dk.WF_BRANCH.values()) == {"scalar", "v2", "v2_nt"}


# ---- the shared bodies on the stand-in ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,C", dk.ESS_CASES)
def test_ess_body_on_the_stand_in(ops, N, C):
    dk.check_ess(ops, N, C)


@pytest.mark.parametrize("N,C", dk.AUTOCORR_CASES)
def test_autocorr_body_on_the_stand_in(ops, N, C):
    dk.check_autocorr(ops, N, C)


def test_hand_over_body_on_the_stand_in(ops):
    dk.check_hand_over(ops)


@pytest.mark.parametrize("C", dk.CMV_C)
@pytest.mark.parametrize("N", dk.CMV_N)
def test_chain_mean_var_body_on_the_stand_in(ops, N, C):
    dk.check_chain_mean_var(ops, N, C)


def test_chain_mean_var_body_on_the_stand_in_at_65536_chains(ops):
    dk.check_chain_mean_var(ops, *dk.CMV_LARGE, kinds=("offset",))


@pytest.mark.parametrize("n", dk.RP_N)
@pytest.mark.parametrize("C", dk.RP_C)
@pytest.mark.parametrize("D", dk.RP_D)
def test_rhat_partials_body_on_the_stand_in(ops, D, C, n):
    dk.check_rhat_partials(ops, D, C, n)


@pytest.mark.parametrize("name", ["odd", "theta_pitch", "even_dev", "odd_dev"])
def test_welford_body_on_the_stand_in(ops, name):
    dk.check_welford(ops, name)


def test_welford_three_kernel_body_on_the_stand_in(ops):
    dk.check_welford_three_kernels(ops)


def test_rank_normalize_body_on_the_stand_in(ops):
    pytest.importorskip("mpmath")
    dk.check_rank_normalize(ops)
    dk.check_rank_normalize_six_values(ops)


@pytest.mark.parametrize("C", dk.PAIRS_C)
@pytest.mark.parametrize("N", dk.PAIRS_N)
def test_pairs_body_on_the_stand_in(ops, N, C):
    dk.check_pairs(ops, N, C)


@pytest.mark.parametrize("on_dev", [False, True])
@pytest.mark.parametrize("with_logp", [False, True])
@pytest.mark.parametrize("dims", dk.REC_DIMS)
@pytest.mark.parametrize("C", dk.REC_C)
def test_record_series_body_on_the_stand_in(ops, C, dims, with_logp, on_dev):
    dk.check_record_series(ops, C, dims, with_logp, on_dev)


# ---- each body notices a wrong kernel -----------------------------------------------------------------------------------------
class DropsTheLastDraw(FakeOps):
    def chain_mean_var(self, x, lengths, mean, var):
        n = torch.full((x.shape[1],), x.shape[0], dtype=torch.int32) if lengths is None else lengths
        super().chain_mean_var(x, n - 1, mean, var)


class SkipsChainsFrom256(FakeOps):
    def rhat_partials(self, mean, m2, n, center, out):
        super().rhat_partials(mean[:, :256], m2[:, :256], n, center, out)


class CountsOneTooMany(FakeOps):
    def welford_update(self, mean, m2, theta, n):
        super().welford_update(mean, m2, theta, n + 1)


class TailPolynomialOfTheNearBranch(FakeOps):
    """bk_ndtri with the x >= 8 tail evaluated by the 2 <= x < 8 rational (Cephes ndtri.c's P1 / Q1)."""

    P1 = (4.05544892305962419923E0, 3.15251094599893866154E1, 5.71628192246421288162E1, 4.40805073893200834700E1,
          1.46849561928858024014E1, 2.18663306850790267539E0, -1.40256079171354495875E-1, -3.50424626827848203418E-2,
          -8.57456785154685413611E-4)
    Q1 = (1.0, 1.57799883256466749731E1, 4.53907635128879210584E1, 4.13172038254672030440E1, 1.50425385692907503408E1,
          2.50464946208309415979E0, -1.42182922854787788574E-1, -3.80806407691578277194E-2, -9.33259480895457427372E-4)

    def rank_normalize(self, rank, S, out):
        super().rank_normalize(rank, S, out)
        p = dk.rn_p(rank.numpy().reshape(-1), S)
        o = out.numpy().reshape(-1)
        for i in np.flatnonzero(dk.rn_branch(p) == 2):
            y = min(p[i], 1.0 - p[i])
            x = math.sqrt(-2.0 * math.log(y))
            z = 1.0 / x
            x1 = z * np.polyval(self.P1, z) / np.polyval(self.Q1, z)
            o[i] = math.copysign((x - math.log(x) / x) - x1, p[i] - 0.5)


class StopsAtAZeroPair(FakeOps):
    """`<=` instead of `<` at the pair test."""

    def end_pos_pairs(self, acor, out):
        a = acor.numpy()
        for c in range(a.shape[1]):
            n = 0
            while n + 1 < a.shape[0] and not (a[n, c] + a[n + 1, c] <= 0):
                n += 2
            out[c] = n

    def iat_from_acor(self, acor, estimator, ess_out, iat_out=None):
        a = acor.numpy().copy()
        for c in range(a.shape[1]):  # (cut the chain where the wrong test stops it: the scan then ends by itself)
            for n in range(2, a.shape[0] - 1, 2):
                if a[n, c] + a[n + 1, c] <= 0:
                    a[n:, c] = -1.0
                    break
        super().iat_from_acor(torch.from_numpy(a), estimator, ess_out, iat_out)


class RunningMinimumTakesTheNaN(FakeOps):
    """prev_min < pk ? prev_min : pk -- a NaN pair replaces the running minimum; iat.py:132's min() keeps it."""

    def iat_from_acor(self, acor, estimator, ess_out, iat_out=None):
        super().iat_from_acor(acor, estimator, ess_out, iat_out)
        if estimator == 0:
            a = acor.numpy()
            stop, _, _, _ = dk.pairs_reference(a, 0)
            for c in range(a.shape[1]):
                if np.isnan(a[:stop[c], c]).any():
                    ess_out[c] = dk.NAN
                    if iat_out is not None:
                        iat_out[c] = dk.NAN


def test_chain_mean_var_body_notices_a_planted_defect():
    with pytest.raises(AssertionError, match="mean"):
        dk.check_chain_mean_var(DropsTheLastDraw(), 64, 65, kinds=("normal",))
    with pytest.raises(AssertionError):
        dk.check_chain_mean_var(DropsTheLastDraw(), 4001, 63, kinds=("offset",), ragged_modes=(False,))


def test_rhat_partials_body_notices_a_planted_defect():
    dk.check_rhat_partials(SkipsChainsFrom256(), 3, 256, 2)  # (nothing to skip: the planted defect alone changes nothing)
    with pytest.raises(AssertionError, match="rhat_partials"):
        dk.check_rhat_partials(SkipsChainsFrom256(), 3, 257, 2)


def test_welford_body_notices_a_planted_defect():
    with pytest.raises(AssertionError, match="recurrence"):
        dk.check_welford(CountsOneTooMany(), "odd", steps=8)


def test_rank_normalize_body_notices_a_planted_defect():
    pytest.importorskip("mpmath")
    with pytest.raises(AssertionError, match="rank_normalize against mpmath"):
        dk.check_rank_normalize(TailPolynomialOfTheNearBranch())


def test_pairs_body_notices_a_planted_defect():
    with pytest.raises(AssertionError):
        dk.check_pairs(StopsAtAZeroPair(), 12, 65)
    ops = StopsAtAZeroPair()
    ops.end_pos_pairs = FakeOps().end_pos_pairs  # (the scan kernel alone wrong)
    with pytest.raises(AssertionError, match="iat|ess|NaN"):
        dk.check_pairs(ops, 200, 64)
    with pytest.raises(AssertionError, match="NaN chains"):
        dk.check_pairs(RunningMinimumTakesTheNaN(), 13, 63)
