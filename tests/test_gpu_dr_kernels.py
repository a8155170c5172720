"""The delayed-rejection stage kernels of csrc/bk_dr.hip and the two counted single-step kernels on the MI355X, at their lane
and list seams: the checks of tests/dr_kernel_parity.py on the HIP library, against the NumPy statement of every entry point
(tests/fake_ops.py).  tests/test_dr_kernels_cpu.py asserts, for the same parametrisations, that the inputs reach every
branch and that no retry decision sits within a last-bit difference of its threshold."""
import pytest

import bayes_kit_amd as bk
from tests import dr_kernel_parity as dk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    return bk._lib.default_ops()


@pytest.mark.parametrize("kind", dk.KINDS)
@pytest.mark.parametrize("C", dk.STAGE_CHAINS)
def test_stage_scalars(ops, C, kind):
    dk.check_stage_scalars(ops, C, kind)


@pytest.mark.parametrize("case", dk.accept_cases(), ids=dk.case_id)
def test_accept_forms(ops, case):
    dk.check_accept_forms(ops, case)


@pytest.mark.parametrize("case", dk.ghost_cases(), ids=dk.case_id)
def test_ghost_forms(ops, case):
    dk.check_ghost_forms(ops, case)


@pytest.mark.parametrize("n", dk.COMPACT_SIZES)
def test_compaction(ops, n):
    dk.check_compaction(ops, n)


@pytest.mark.parametrize("D", dk.SCATTER_DIMS)
@pytest.mark.parametrize("n", dk.SCATTER_LANES)
def test_scatter(ops, n, D):
    dk.check_scatter(ops, n, D)


@pytest.mark.parametrize("target", ("gaussian", "funnel"))
@pytest.mark.parametrize("C,D", dk.STEP_SHAPES)
def test_single_step(ops, C, D, target):
    dk.check_single_step(ops, C, D, target)
