"""Nested R-hat without a GPU: the shared bodies of tests/nested_rhat_parity.py on the NumPy stand-in
(tests/fake_ops_nested.NestedFakeOps, the kernel's summation orders restated), the exact reference against a 50-digit
evaluation, the bodies shown to notice planted defects, and the C ABI's argument checks (decided before any launch)."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

from tests import nested_rhat_parity as nr
from tests.fake_ops_nested import NestedFakeOps, sequential_sum, superchain_moments_ref


@pytest.fixture(scope="module")
def ops():
    return NestedFakeOps()


# ---- the reference ------------------------------------------------------------------------------------------------------
def test_exact_superchain_moments_against_mpmath_at_50_digits():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    D, K, M, n = 2, 3, 5, 7
    mean, m2 = nr.sc_inputs(D, K, M, n)
    s, w, sabs = nr.sc_exact(mean, m2, n, M)
    for d in range(D):
        for k in range(K):
            mu = [mp.mpf(float(v)) for v in mean[d, k * M:(k + 1) * M]]
            q = [mp.mpf(float(v)) for v in m2[d, k * M:(k + 1) * M]]
            sk = mp.fsum(mu) / M
            wk = mp.fsum((v - sk) ** 2 for v in mu) / (M - 1) + mp.fsum(q) / (n - 1) / M
            assert abs(mp.mpf(s[d][k].numerator) / s[d][k].denominator - sk) <= mp.mpf(10) ** -44 * abs(sk)
            assert abs(mp.mpf(w[d][k].numerator) / w[d][k].denominator - wk) <= mp.mpf(10) ** -40 * wk
            assert sabs[d, k] == pytest.approx(float(mp.fsum(abs(v) for v in mu)), rel=1e-15)
    assert nr.sc_exact(np.array([[1.0, 2.0, 4.0, 8.0]]), np.array([[3.0, 1.0, 2.0, 2.0]]), 3, 2)[:2] == (
        [[Fraction(3, 2), Fraction(6)]], [[Fraction(1, 2) + Fraction(1), Fraction(8) + Fraction(1)]])


def test_the_restated_launch_choice_matches_the_host_code():
    import os
    import re

    src = open(os.path.join(os.path.dirname(__file__), "..", "bayes-kit_amd", "csrc", "bk_diag.hip")).read()
    body = src[src.index("int bk_superchain_moments("):]
    body = body[:body.index("BK_RETURN_LAUNCH_STATUS")]
    assert re.search(r"if \(M <= BK_WAVE && \(M & \(M - 1\)\) == 0\)", body) and "} else if (M > BK_WAVE) {" in body
    assert [body.index(k) for k in ("k_superchain_seg<<<", "k_superchain_wg<<<", "k_superchain_lane<<<")] == sorted(
        body.index(k) for k in ("k_superchain_seg<<<", "k_superchain_wg<<<", "k_superchain_lane<<<"))
    assert "#define BK_WAVE 64" in open(os.path.join(os.path.dirname(__file__), "..", "bayes-kit_amd", "csrc", "bk_common.hpp")).read()


# ---- the bodies on the stand-in -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,K,M,n", nr.SC_CASES + [nr.SC_WIDE])
def test_superchain_moments_body_on_the_stand_in(ops, D, K, M, n):
    nr.check_superchain_moments(ops, D, K, M, n)


@pytest.mark.parametrize("M", nr.SC_M)
def test_position_independence_body_on_the_stand_in(ops, M):
    nr.check_position_independence(ops, 3, 5, M, 2)


@pytest.mark.parametrize("D,K,M,n", nr.END_TO_END_CASES)
def test_from_moments_against_the_fraction_evaluation_on_the_stand_in(ops, D, K, M, n):
    nr.check_from_moments_against_fractions(ops, D, K, M, n)


def test_m1_identity_with_rhat_on_the_stand_in(ops):
    nr.check_m1_identity(ops)


def test_tensor_running_moments_and_recorder_agree_on_the_stand_in(ops):
    nr.check_three_entry_points(ops)


@pytest.mark.parametrize("seed", nr.BEHAVIOUR_SEEDS)
def test_behaviour_on_the_stand_in(ops, seed):
    nr.check_behaviour(ops, seed)


def test_errors_on_the_stand_in(ops):
    nr.check_errors(ops)


def test_superchain_init_repeats_each_start_contiguously():
    nr.check_superchain_init()


def test_sampler_run_on_the_stand_in(ops):
    nr.check_sampler_run(ops)


# ---- planted defects: each body must reject a wrong kernel --------------------------------------------------------------
class _Defect(NestedFakeOps):
    def superchain_moments(self, mean, m2, n, M, s_out, w_out):
        s, w = self.wrong(mean.numpy(), None if n == 1 else m2.numpy(), n, M)
        s_out.numpy()[...] = s
        w_out.numpy()[...] = w


class Uncentred(_Defect):
    """Bt from sum mu^2 - M s^2."""

    def wrong(self, mean, m2, n, M):
        s, w = superchain_moments_ref(mean, m2, n, M)
        x = mean.reshape(mean.shape[0], -1, M)
        good_bt = sequential_sum((x - s[..., None]) ** 2) / (M - 1.0)
        bad_bt = (sequential_sum(x * x) - M * s * s) / (M - 1.0)
        return s, w - good_bt + bad_bt


class Ddof0(_Defect):
    """Bt divided by M."""

    def wrong(self, mean, m2, n, M):
        s, w = superchain_moments_ref(mean, m2, n, M)
        x = mean.reshape(mean.shape[0], -1, M)
        bt = sequential_sum((x - s[..., None]) ** 2)
        return s, w - bt / (M - 1.0) + bt / M


class DropsLast(_Defect):
    """The last subchain of each superchain is left out."""

    def wrong(self, mean, m2, n, M):
        D, C = mean.shape
        keep = np.arange(C) % M != M - 1
        return superchain_moments_ref(mean[:, keep], None if m2 is None else m2[:, keep], n, M - 1)


class ShiftedByOne(_Defect):
    """Superchain k takes chains k M + 1 .. k M + M."""

    def wrong(self, mean, m2, n, M):
        return superchain_moments_ref(np.roll(mean, -1, axis=1), None if m2 is None else np.roll(m2, -1, axis=1), n, M)


@pytest.mark.parametrize("defect", [Uncentred, Ddof0, DropsLast, ShiftedByOne])
@pytest.mark.parametrize("M", [4, 96, 1000])
def test_kernel_body_notices_a_planted_defect(defect, M):
    with pytest.raises(AssertionError):
        nr.check_superchain_moments(defect(), 3, 3, M, 2)


@pytest.mark.parametrize("defect", [Ddof0, DropsLast, ShiftedByOne])
def test_end_to_end_body_notices_a_planted_defect(defect):
    with pytest.raises(AssertionError):
        nr.check_from_moments_against_fractions(defect(), 3, 5, 4, 2)


def test_position_body_notices_a_kernel_whose_order_depends_on_the_position():
    class ByPosition(NestedFakeOps):
        """Sums the first superchain of an array from its first chain on, every other one from its last."""

        def superchain_moments(self, mean, m2, n, M, s_out, w_out):
            s, w = superchain_moments_ref(mean.numpy(), m2.numpy(), n, M, total=sequential_sum)
            s1, w1 = superchain_moments_ref(mean.numpy(), m2.numpy(), n, M, total=lambda x: sequential_sum(x[..., ::-1]))
            s[:, 1:], w[:, 1:] = s1[:, 1:], w1[:, 1:]
            s_out.numpy()[...] = s
            w_out.numpy()[...] = w

    with pytest.raises(AssertionError):
        nr.check_position_independence(ByPosition(), 3, 5, 3, 2)


# ---- the C ABI's argument checks (no GPU: decided before any HIP call) --------------------------------------------------
def test_error_behaviour_of_bk_superchain_moments_without_a_gpu():
    from bayes_kit_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    OK, E_ARG, E_ALIGN = 0, -1, -2
    f = lib.bk_superchain_moments  # (mean, m2, ld, n, M, s_out, w_out, ldk, C, D, stream)
    assert f(p, p, 8, 2, 0, p, p, 4, 8, 1, None) == E_ARG        # M = 0
    assert f(p, p, 8, 2, 3, p, p, 4, 8, 1, None) == E_ARG        # C % M != 0
    assert f(None, p, 8, 2, 2, p, p, 4, 8, 1, None) == E_ARG     # a null mean
    assert f(p, p, 8, 2, 2, None, p, 4, 8, 1, None) == E_ARG
    assert f(p, p, 8, 2, 2, p, None, 4, 8, 1, None) == E_ARG
    assert f(p, None, 8, 2, 2, p, p, 4, 8, 1, None) == E_ARG     # m2 is needed from n = 2 on
    assert f(p, p, 8, 0, 2, p, p, 4, 8, 1, None) == E_ARG        # n < 1
    assert f(p, p, 7, 2, 2, p, p, 4, 8, 1, None) == E_ALIGN      # ld < C
    assert f(p, p, 8, 2, 2, p, p, 3, 8, 1, None) == E_ALIGN      # ldk < K
    assert f(p, p, 0, 2, 2, p, p, 0, 0, 8, None) == OK           # C = 0
    assert f(p, None, 8, 1, 2, p, p, 4, 8, 0, None) == OK        # D = 0 (and m2 may be NULL for n = 1)
    assert "bk_superchain_moments" in _lib.SIGNATURES
