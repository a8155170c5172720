"""The multi-chain ESS kernels of csrc/bk_ess_multi.hip on the MI355X, called by name where their launch code changes
path: k_lag_sums on both sides of every chain-group seam of lag_plan (the lower side of each is that instance's
over-64-KiB launch), with odd N, in indicator mode and across a chunked launch, against long-double sums of the doubles
the kernel stages; the split moments, their totals and the count of non-finite draws against exact references;
bk_ess_between_sq, bk_ess_acov_sums beyond 65,535 lags, bk_ess_indicator beyond 4,096 rows, bk_select_ranks; the hand-over
to the FFT route at bk_ess_lag_sums_max_half and bk_autocorr_fft with 1,024 and more complex columns and with non-finite
columns; the five user-facing functions once per instance.  The bodies and their derived bounds:
tests/ess_multi_parity.py.  Run with ``-s`` for the per-check err / bound ratios (the largest per check are kept in
profiles/ess_multi_edges.md)."""
import pytest

import bayes_kit_amd as bk
from tests import ess_multi_parity as ep

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    return bk._lib.default_ops()


# ---- 1. bk_ess_lag_sums -------------------------------------------------------------------------------------------------------
def test_the_restated_plan_is_the_librarys_and_the_host_side_checks_refuse(ops):
    ep.check_lag_sums_abi(ops)


@pytest.mark.parametrize("n,odd,C", ep.LS_CASES)
def test_lag_sums_at_the_group_seams_and_in_the_opt_in_launches(ops, n, odd, C):
    ep.check_lag_sums(ops, n, odd, C)


@pytest.mark.parametrize("n,odd,C", ep.LS_INDICATOR_CASES)
def test_lag_sums_in_indicator_mode_once_per_instance(ops, n, odd, C):
    ep.check_lag_sums(ops, n, odd, C, indicator=True)


def test_lag_sums_across_a_chunked_launch(ops):
    ep.check_lag_sums_chunked(ops)


# ---- 2. bk_ess_split_moments / bk_ess_between_sq ----------------------------------------------------------------------------------
@pytest.mark.parametrize("C", ep.SM_C)
@pytest.mark.parametrize("n", ep.SM_N)
def test_split_moments_against_the_exact_moments(ops, n, C):
    ep.check_split_moments(ops, n, C)


def test_split_moments_with_more_than_256_partials_per_row(ops):
    ep.check_split_moments(ops, *ep.SM_WIDE, kinds=("offset",))


@pytest.mark.parametrize("odd", [0, 1])
@pytest.mark.parametrize("n,C", [(1, 1), (4, 65), (33, 130), (64, 63), (1000, 64)])
def test_split_moments_in_indicator_mode(ops, n, C, odd):
    ep.check_split_moments_indicator(ops, n, C, odd)


def test_the_count_of_non_finite_draws_is_exact(ops):
    ep.check_bad_count(ops)


@pytest.mark.parametrize("M", ep.BSQ_M)
def test_between_sq_against_fsum_of_exact_squares(ops, M):
    ep.check_between_sq(ops, M)


# ---- 3. bk_ess_acov_sums / bk_ess_indicator / bk_select_ranks -----------------------------------------------------------------------
@pytest.mark.parametrize("C,rows,lag0,nlags", ep.ACOV_CASES)
def test_acov_sums_against_fsum_of_exact_products(ops, C, rows, lag0, nlags):
    ep.check_acov_sums(ops, C, rows, lag0, nlags)


def test_acov_sums_beyond_65535_lags(ops):
    C, rows, lags = ep.ACOV_LONG
    ep.check_acov_sums(ops, C, rows, 0, rows, check_lags=lags)


@pytest.mark.parametrize("C", ep.IND_C)
@pytest.mark.parametrize("n", ep.IND_N)
def test_indicator_is_bit_equal_on_strided_views(ops, n, C):
    ep.check_indicator(ops, n, C)


def test_select_ranks_sizes_and_targets_nobody_holds(ops):
    ep.check_select_ranks(ops)


# ---- 4. the FFT hand-over, bk_autocorr_fft as this route calls it ---------------------------------------------------------------------
def test_lag_sums_and_the_fft_route_agree_at_the_hand_over(ops):
    ep.check_fft_hand_over(ops)


@pytest.mark.parametrize("N,C", ep.WIDE_FFT)
def test_autocorr_fft_with_1024_and_more_complex_columns(ops, N, C):
    ep.check_autocorr_fft_wide(ops, N, C)


def test_autocorr_fft_keeps_a_non_finite_column_from_its_partner(ops):
    ep.check_autocorr_fft_non_finite(ops)
    ep.check_autocorr_fft_non_finite(ops, 33, 2049)


# ---- 5. end to end --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ep.E2E_N)
def test_the_five_functions_once_per_instance(ops, n):
    ep.check_end_to_end(ops, n)


def test_non_finite_draws_end_to_end(ops):
    ep.check_non_finite_end_to_end(ops)
