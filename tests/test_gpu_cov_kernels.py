"""bk_cov_accumulate on the MI355X at its tile-block, slab and chunk seams: the checks of tests/cov_parity.py on the HIP
library (exact products on integer data; determinism, whole-tile == checked and the long-double bound on real data), and the
restated plan against the library's own, so that a change of the plan fails here instead of moving the shapes off their
seams.  Figures: profiles/cov_edges.md."""
import pytest

import bayes_kit_amd as bk
from tests import cov_parity as cp

pytestmark = pytest.mark.gpu

_WHOLE_IDS = [f"{s.D}x{s.C}" for s in cp.WHOLE_SHAPES]
_BOUND_IDS = [f"{s.D}x{s.C}" for s in cp.BOUND_SHAPES]


@pytest.fixture(scope="module")
def ops():
    return bk._lib.default_ops()


def test_k_chunk_is_the_restated_one(ops):
    got = [ops.cov_k_chunk(D) for D in range(1, 4097)]
    assert got == [cp.k_chunk(D) for D in range(1, 4097)]


@pytest.mark.parametrize("sh", cp.SHAPES, ids=cp.SHAPE_IDS)
def test_work_elems_are_the_restated_ones_and_the_shape_hits_its_seam(ops, sh):
    cp.assert_shape_hits_its_seam(sh)
    assert int(ops.lib.bk_cov_accumulate_work_elems(sh.D, sh.C)) == cp.plan(sh.D, sh.C).work_elems
    assert ops.cov_work(sh.D, sh.C).numel() == cp.plan(sh.D, sh.C).work_elems


@pytest.mark.parametrize("sh", cp.SHAPES, ids=cp.SHAPE_IDS)
def test_exact(ops, sh):
    cp.check_exact(ops, sh)


@pytest.mark.parametrize("sh", cp.SHAPES, ids=cp.SHAPE_IDS)
def test_real_data_is_deterministic(ops, sh):
    cp.check_deterministic(ops, sh)


@pytest.mark.parametrize("sh", cp.WHOLE_SHAPES, ids=_WHOLE_IDS)
def test_whole_tile_equals_checked(ops, sh):
    cp.check_whole_tile_equals_checked(ops, sh)


@pytest.mark.parametrize("sh", cp.BOUND_SHAPES, ids=_BOUND_IDS)
def test_long_double_bound(ops, sh):
    cp.check_long_double_bound(ops, sh)


def test_nan_poisons_one_row_and_column(ops):
    cp.check_nan_poisons_one_row_and_column(ops)


def test_running_covariance_across_tile_blocks(ops):
    cp.check_running_covariance_across_tile_blocks(ops)
