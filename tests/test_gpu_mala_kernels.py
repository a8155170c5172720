"""tests/mala_kernel_parity.py on the HIP library: the MALA kernels alone at their slot, block, pitch and offset seams (the figures
of a run are kept in profiles/mala_kernels.md)."""
import pytest

import bayes_kit_amd as bk
from tests import mala_kernel_parity as mk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    return bk._lib.default_ops()


@pytest.mark.parametrize("kind", mk.KINDS)
def test_planted_thresholds(ops, kind):
    worst = 0.0
    for D in mk.PLANT_D:
        for C in mk.PLANT_C + (mk.PLANT_C_AT_65 if D == 65 else ()):
            worst = max(worst, mk.check_planted(ops, kind, C, D))
    mk.say(f"planted thresholds, {kind}", worst)


@pytest.mark.parametrize("kind", mk.KINDS)
def test_layouts_and_guard_cells(ops, kind):
    for D in mk.LAYOUT_D:
        for C in mk.LAYOUT_C:
            mk.check_layouts(ops, kind, C, D)


@pytest.mark.parametrize("kind", mk.KINDS)
def test_nonfinite_values_and_the_pair_partner(ops, kind):
    for C, D in mk.NONFINITE_SHAPES:
        mk.check_nonfinite(ops, kind, C, D)


@pytest.mark.parametrize("kind,C,D,streams", mk.SEAMS)
def test_cache_size_seam(ops, kind, C, D, streams):
    mk.say(f"seam {kind} {C} x {D} ({'non-temporal' if streams else 'resident'})", mk.check_seam(ops, kind, C, D, streams))


def test_logq(ops):
    worst = max(mk.check_logq(ops, C, D) for D in mk.LOGQ_D for C in mk.LOGQ_C)
    mk.say("bk_mala_logq", worst)
    mk.check_logq_no_dims(ops)


def test_propose_from_normals(ops):
    for C, D in mk.PROPOSE_Z_SHAPES:
        mk.check_propose_from_normals(ops, C, D)


def test_propose(ops):
    for C, D in mk.PROPOSE_SHAPES:
        mk.check_propose(ops, C, D)
