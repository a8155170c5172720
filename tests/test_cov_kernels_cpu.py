"""tests/cov_parity.py without a GPU: every listed shape still hits the seam it is listed for; the checks pass on the NumPy
stand-in that walks bk_cov_accumulate's plan; and each of the stand-in's planted faults -- one broken seam each -- makes the
exact check fail at the shape named for that seam, which is the evidence that the same checks would notice such a kernel."""
import numpy as np
import pytest

from tests import cov_parity as cp
from tests.fake_ops_dense_adapt import DenseAdaptFakeOps


@pytest.fixture(scope="module")
def ops():
    return cp.PlanFollowingCov()


@pytest.mark.parametrize("sh", cp.SHAPES, ids=cp.SHAPE_IDS)
def test_shape_hits_its_seam(sh):
    cp.assert_shape_hits_its_seam(sh)


def test_the_listed_shapes_are_the_issue_s():
    assert [(s.D, s.C) for s in cp.SHAPES] == [(257, 37), (300, 300), (5, 1025), (130, 1025), (130, 2049), (1921, 1025),
                                                (2049, 225), (256, 32), (384, 16), (384, 48), (128, 1040), (256, 512),
                                                (2176, 1024), (897, 145)]  # (the last one added to the issue's thirteen)
    assert [s.kernel for s in cp.SHAPES] == [cp.CHECKED] * 7 + [cp.WHOLE] * 6 + [cp.CHECKED]
    assert [(s.D, s.C) for s in cp.BOUND_SHAPES] == [(257, 37), (300, 300), (5, 1025), (130, 1025), (130, 2049), (256, 32),
                                                      (384, 16), (384, 48), (128, 1040), (256, 512)]
    assert set(cp.FAULTS.values()) <= {(s.D, s.C) for s in cp.SHAPES}


def test_plan_restatement_at_known_values():
    """k_chunk is a multiple of 16 within the L2 budget (tests/test_dense_adapt_cpu.py asks the library the same), 128 while
    four times the tile count stays below it (asserted up to D = 768), capped by the budget at the listed D = 1921, 2049
    and at 4096, and the decode walks the triangle row by row."""
    for D in range(1, 4097):
        k = cp.k_chunk(D)
        assert k % 16 == 0 and k >= 16 and (k == 16 or D * k * 8 <= 2 << 20)
    assert {cp.k_chunk(D) for D in range(1, 769)} == {128} and cp.k_chunk(1921) == 128 and cp.plan(1921, 1).k == 544
    assert cp.k_chunk(2048) == 128 and cp.k_chunk(2049) == 112 and cp.k_chunk(4096) == 64
    tiles = [cp.decode(t) for t in range(10)]
    assert tiles == [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2), (3, 0), (3, 1), (3, 2), (3, 3)]


def test_float64_product_of_integer_data_is_the_int64_product():
    x, c = cp.integer_data(300, 300)
    assert x.min() == -15.0 and x.max() == 15.0 and (x != 0.0).all() and np.abs(c).max() <= 16.0
    for cc in (None, c):
        S, s = cp.exact_product(x, cc)
        xi = x.astype(np.int64) - (0 if cc is None else cc.astype(np.int64)[:, None])
        assert np.array_equal(S, (xi @ xi.T).astype(np.float64)) and np.array_equal(s, xi.sum(axis=1).astype(np.float64))


# ---- the checks on the fault-free stand-in -------------------------------------------------------------------------------------
@pytest.mark.parametrize("sh", cp.SHAPES, ids=cp.SHAPE_IDS)
def test_exact(ops, sh):
    cp.check_exact(ops, sh)


@pytest.mark.parametrize("sh", cp.SHAPES, ids=cp.SHAPE_IDS)
def test_real_data_is_deterministic(ops, sh):
    cp.check_deterministic(ops, sh)


@pytest.mark.parametrize("sh", cp.WHOLE_SHAPES, ids=[f"{s.D}x{s.C}" for s in cp.WHOLE_SHAPES])
def test_whole_tile_equals_checked(ops, sh):
    cp.check_whole_tile_equals_checked(ops, sh)


@pytest.mark.parametrize("sh", cp.BOUND_SHAPES, ids=[f"{s.D}x{s.C}" for s in cp.BOUND_SHAPES])
def test_long_double_bound(ops, sh):
    cp.check_long_double_bound(ops, sh)


def test_nan_poisons_one_row_and_column(ops):
    cp.check_nan_poisons_one_row_and_column(ops)


def test_running_covariance_across_tile_blocks():
    cp.check_running_covariance_across_tile_blocks(DenseAdaptFakeOps())


def test_running_covariance_across_tile_blocks_on_the_plan_following_stand_in(ops):
    class Both(DenseAdaptFakeOps):  # (the plan-following accumulation under RunningCovariance's other entry points)
        cov_k_chunk = staticmethod(cp.k_chunk)
        cov_work = ops.cov_work
        cov_accumulate = ops.cov_accumulate

    cp.check_running_covariance_across_tile_blocks(Both())


# ---- each planted fault is noticed ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fault", sorted(cp.FAULTS))
def test_fault_is_noticed_by_the_exact_check(fault):
    sh = cp.shape(*cp.FAULTS[fault])
    what = "s differs from the exact row sums" if fault == "row_sums" else "S differs from the exact product"
    with pytest.raises(AssertionError, match=what) as e:
        cp.check_exact(cp.PlanFollowingCov(fault), sh)
    print(fault, sh.D, sh.C, e.value)
