"""Nested R-hat on the MI355X: bk_superchain_moments in its three launch shapes (segmented butterfly, workgroup per
superchain, lane per superchain) against the exact per-superchain values inside bounds derived from the stated summation
orders, its write contracts and position independence, and the functions built on it -- against the exact evaluation, the
M = 1 identity with ``bk.rhat``, each other, the behaviour table and a sampler run.  The bodies and their bounds:
tests/nested_rhat_parity.py.  Run with ``-s`` for the per-check err / bound ratios."""
import pytest

import bayes_kit_amd as bk
from tests import nested_rhat_parity as nr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    return bk._lib.default_ops()


@pytest.mark.parametrize("D,K,M,n", nr.SC_CASES + [nr.SC_WIDE])
def test_superchain_moments_against_the_exact_values_and_write_contracts(ops, D, K, M, n):
    nr.check_superchain_moments(ops, D, K, M, n)


@pytest.mark.parametrize("M", nr.SC_M)
def test_superchain_moments_do_not_depend_on_position_pitch_or_run(ops, M):
    nr.check_position_independence(ops, 3, 5, M, 2)


@pytest.mark.parametrize("D,K,M,n", nr.END_TO_END_CASES)
def test_nested_rhat_from_moments_against_the_fraction_evaluation(ops, D, K, M, n):
    nr.check_from_moments_against_fractions(ops, D, K, M, n)


def test_m1_identity_with_rhat(ops):
    nr.check_m1_identity(ops)


def test_tensor_running_moments_and_recorder_agree(ops):
    nr.check_three_entry_points(ops)


@pytest.mark.parametrize("seed", nr.BEHAVIOUR_SEEDS)
def test_behaviour(ops, seed):
    nr.check_behaviour(ops, seed)


def test_errors(ops):
    nr.check_errors(ops)


def test_sampler_run_from_superchain_starts(ops):
    nr.check_sampler_run(ops)
