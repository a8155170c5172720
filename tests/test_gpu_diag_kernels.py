"""The diagnostic kernels of csrc/bk_diag.hip on the MI355X, called by name at the sizes where their launch code changes
path: the LDS-staged ESS / autocorrelation on both sides of every chain-group seam, inside every over-64-KiB band and at
the hand-over to the one-lane-per-chain kernels; bk_chain_mean_var, bk_rhat_partials and the three Welford kernels
against exact references; every branch of the Cephes ndtri port against mpmath; the Geyer scans on crafted pairs; the
recorder's row rules.  The bodies and their derived bounds: tests/diag_kernel_parity.py.  Run with ``-s`` for the per-check
err / bound ratios (the largest per check are kept in profiles/diag_kernel_edges.md)."""
import pytest

import bayes_kit_amd as bk
from tests import diag_kernel_parity as dk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    return bk._lib.default_ops()


# ---- 1. bk_ess / bk_autocorr ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,C", dk.ESS_CASES)
def test_ess_at_the_group_seams_the_opt_in_bands_and_the_one_lane_fallback(ops, N, C):
    dk.check_ess(ops, N, C)


@pytest.mark.parametrize("N,C", dk.AUTOCORR_CASES)
def test_autocorr_at_the_group_seams_the_opt_in_bands_and_the_one_lane_fallback(ops, N, C):
    dk.check_autocorr(ops, N, C, timed=N == dk.ESS_FALLBACK[0])


def test_tile_and_one_lane_autocorr_agree_at_the_hand_over(ops):
    dk.check_hand_over(ops)


# ---- 2. bk_chain_mean_var ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", dk.CMV_C)
@pytest.mark.parametrize("N", dk.CMV_N)
def test_chain_mean_var_against_the_exact_moments(ops, N, C):
    dk.check_chain_mean_var(ops, N, C)


def test_chain_mean_var_1000_draws_of_65536_chains(ops):
    dk.check_chain_mean_var(ops, *dk.CMV_LARGE, kinds=("offset",))


# ---- 3. bk_rhat_partials ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", dk.RP_N)
@pytest.mark.parametrize("C", dk.RP_C)
@pytest.mark.parametrize("D", dk.RP_D)
def test_rhat_partials_sums_write_contracts_and_rhat_end_to_end(ops, D, C, n):
    dk.check_rhat_partials(ops, D, C, n)


# ---- 4. bk_welford_update / bk_welford_update_dev -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["odd", "theta_pitch", "even_dev", "odd_dev"])
def test_welford_launch_shapes(ops, name):
    dk.check_welford(ops, name)


def test_welford_scalar_paired_and_non_temporal_kernels_give_the_same_bits(ops):
    dk.check_welford_three_kernels(ops)


# ---- 5. bk_rank_normalize ---------------------------------------------------------------------------------------------------
def test_rank_normalize_every_branch_against_mpmath(ops):
    dk.check_rank_normalize(ops)


def test_rank_normalize_six_values_against_scipy(ops):
    dk.check_rank_normalize_six_values(ops)


# ---- 6. bk_iat_from_acor / bk_end_pos_pairs -----------------------------------------------------------------------------------
@pytest.mark.parametrize("C", dk.PAIRS_C)
@pytest.mark.parametrize("N", dk.PAIRS_N)
def test_geyer_scans_on_crafted_pairs(ops, N, C):
    dk.check_pairs(ops, N, C)


# ---- 7. bk_record_series / bk_record_series_dev -------------------------------------------------------------------------------
@pytest.mark.parametrize("on_dev", [False, True])
@pytest.mark.parametrize("with_logp", [False, True])
@pytest.mark.parametrize("dims", dk.REC_DIMS)
@pytest.mark.parametrize("C", dk.REC_C)
def test_record_series_rows_and_the_out_of_range_rule(ops, C, dims, with_logp, on_dev):
    dk.check_record_series(ops, C, dims, with_logp, on_dev)
