"""The logistic-regression target on the MI355X: the fp64 MFMA GEMM, its fused residual epilogue, bk_logistic_residual,
bk_logistic_finish and bk.LogisticRegression as a whole against the long-double reference of tests/logistic_ref.py, at the
shapes and inputs where such kernels go wrong (the bodies and their derived bounds: tests/logistic_parity.py).  Run with
``-s`` for the per-shape err / bound ratios (the largest per check are kept in profiles/logistic_parity.md)."""
import pytest

import bayes_kit_amd as bk
from tests import logistic_parity as lp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    return bk._lib.default_ops()


# ---- the GEMM: bk_gemm_chains with and without work, bk_gemm_chains_logistic ---------------------------------------------
@pytest.mark.parametrize("kind", ["chains", "chains_work", "logistic"])
@pytest.mark.parametrize("R,K,C", lp.GEMM_SHAPES)
def test_gemm_exact_on_integers_and_within_the_rounding_bound(ops, R, K, C, kind):
    lp.check_gemm(ops, kind, R, K, C)


@pytest.mark.parametrize("D,C", lp.METRIC_SHAPES)
def test_dense_metric_apply_exact_on_integers_and_within_the_rounding_bound(ops, D, C):
    lp.check_gemm(ops, "metric", D, D, C)


@pytest.mark.parametrize("kind", ["chains", "chains_work", "metric", "logistic"])
@pytest.mark.parametrize("variant", lp.VARIANTS[1:])
def test_a_broken_precondition_of_the_unchecked_kernel_changes_no_bit(ops, variant, kind):
    if kind == "metric":
        lp.check_broken_precondition(ops, kind, variant, 256, 256, 256)
    else:
        lp.check_broken_precondition(ops, kind, variant)


def test_gemm_degenerate_sizes(ops):
    lp.check_gemm_degenerate(ops)


# ---- bk_logistic_residual -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", lp.RESIDUAL_C)
@pytest.mark.parametrize("N,segments", lp.RESIDUAL_CASES[:-1])
def test_logistic_residual_edges(ops, N, segments, C):
    lp.check_residual(ops, N, segments, C)


def test_logistic_residual_with_65535_segments(ops):
    lp.check_residual(ops, *lp.RESIDUAL_CASES[-1], 63)


def test_logistic_residual_non_finite_logits(ops):
    lp.check_residual_nonfinite(ops)


# ---- bk_logistic_finish -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("segments", [1, 256])
@pytest.mark.parametrize("C", [1, 64, 65, 1000])
@pytest.mark.parametrize("D", [1, 2, 40, 513])
def test_logistic_finish_bits_null_combinations_and_refusals(ops, D, C, segments):
    lp.check_finish(ops, D, C, segments)


# ---- the target as a whole ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", lp.THETA_SCALES)
@pytest.mark.parametrize("N,D,C", lp.TARGET_SHAPES)
def test_target_every_chain_against_the_long_double_reference(ops, N, D, C, scale):
    lp.check_target(ops, N, D, C, scale)


def test_a_chain_does_not_depend_on_the_chains_it_shares_an_evaluation_with(ops):
    lp.check_sharing_invariance(ops)


# ---- fixtures run by the reference itself ---------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["auto", "opaque"])
@pytest.mark.parametrize("name", ["hmc_logistic16", "hmc_logistic40"])
def test_hmc_on_the_logistic_target_against_the_reference_run(ops, name, path):
    lp.check_logistic_fixture(ops, name, path=path)


@pytest.mark.parametrize("name", ["mala_logistic16", "mala_logistic40"])
def test_mala_on_the_logistic_target_against_the_reference_run(ops, name):
    lp.check_logistic_fixture(ops, name)


def test_tempered_smc_on_the_logistic_target_against_the_reference_run(ops):
    lp.check_logistic_smc_fixture(ops)
