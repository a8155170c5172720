"""bk.GLM on the MI355X: the GLM epilogue of the fp64 MFMA GEMM (bk_gemm_chains_glm), the stand-alone pass
(bk_glm_residual) and the target as a whole against the long-double reference of tests/glm_ref.py, bit for bit against the
logistic entry points where the family is Bernoulli, and under the samplers (the bodies and their derived bounds:
tests/glm_parity.py).  Run with ``-s`` for the per-case err / bound ratios (the largest per check: profiles/glm.md)."""
import pytest

import bayes_kit_amd as bk
from tests import glm_parity as gp

pytestmark = pytest.mark.gpu

FAM_OFF = [(f, o) for f in gp.FAMILIES for o in (False, True)]


@pytest.fixture(scope="module")
def ops():
    return bk._lib.default_ops()


@pytest.mark.parametrize("family,offset", FAM_OFF)
@pytest.mark.parametrize("R,K,C", gp.EPILOGUE_SHAPES)
def test_epilogue_equals_the_stand_alone_pass_bit_for_bit(ops, R, K, C, family, offset):
    gp.check_epilogue_equals_pass(ops, family, offset, R, K, C)


@pytest.mark.parametrize("variant", ["lda_odd", "ldx_odd", "a_off", "x_off"])
@pytest.mark.parametrize("family,offset", FAM_OFF)
def test_a_broken_precondition_of_the_unchecked_kernel_changes_no_bit(ops, family, offset, variant):
    gp.check_broken_precondition(ops, family, offset, variant)


@pytest.mark.parametrize("R,K,C", gp.EPILOGUE_SHAPES)
def test_bernoulli_without_offset_is_the_logistic_entry_points_bit_for_bit(ops, R, K, C):
    gp.check_bernoulli_is_logistic(ops, R, K, C)


@pytest.mark.parametrize("C", gp.RESIDUAL_C)
@pytest.mark.parametrize("N,segments", gp.RESIDUAL_CASES)
@pytest.mark.parametrize("family,offset", FAM_OFF)
def test_cells_against_the_long_double_of_the_same_z(ops, family, offset, N, segments, C):
    gp.check_cells(ops, family, offset, N, segments, C)


@pytest.mark.parametrize("family,offset", FAM_OFF)
def test_non_finite_eta_follows_the_header_table(ops, family, offset):
    gp.check_nonfinite(ops, family, offset)


def test_argument_checks(ops):
    gp.check_arguments(ops)


@pytest.mark.parametrize("family,offset", FAM_OFF)
@pytest.mark.parametrize("N,D,C", gp.TARGET_SHAPES)
def test_whole_target_against_the_long_double_reference(ops, N, D, C, family, offset):
    gp.check_target(ops, family, offset, N, D, C)


@pytest.mark.parametrize("offset", [False, True])
def test_gaussian_log_likelihood_is_the_closed_form(ops, offset):
    gp.check_gaussian_closed_form(ops, offset)


@pytest.mark.parametrize("family", gp.FAMILIES)
def test_a_non_finite_chain_changes_no_other_chain(ops, family):
    gp.check_nonfinite_chain(ops, family)


@pytest.mark.parametrize("family", gp.FAMILIES)
def test_a_chain_does_not_depend_on_the_chains_it_shares_a_call_with(ops, family):
    gp.check_sharing_invariance(ops, family)


@pytest.mark.parametrize("kind", ["hmc", "hmc_opaque", "mala", "smc"])
def test_bernoulli_glm_is_a_drop_in_for_logistic_regression(ops, kind):
    gp.check_drop_in(ops, kind)


@pytest.mark.parametrize("family", ["binomial", "poisson", "gaussian"])
def test_the_constant_survives_evaluations_at_other_widths(ops, family):
    gp.check_constant_survives_other_widths(ops, family)


@pytest.mark.parametrize("family", ["poisson", "gaussian"])
def test_two_graph_replayed_samplers_of_different_widths_on_one_model(ops, family):
    gp.check_two_samplers_on_one_model(ops, family)


def test_hmc_leaves_the_closed_form_gaussian_posterior_invariant(ops):
    gp.check_invariance_hmc(ops)


def test_tempered_hmc_treats_glm_as_a_split_model_with_a_beta_zero_rung(ops):
    gp.check_invariance_tempered(ops)
