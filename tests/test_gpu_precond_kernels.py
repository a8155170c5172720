"""The preconditioned HMC kernels on the MI355X at their row, tile and size seams: the checks of tests/precond_kernel_parity.py on
the HIP library -- bk_leapfrog_finish_precond (k_finish<true>, bkt::k_finish_t<8, 8, 0, true>, k_finish_v2<true>),
bk_momentum_refresh_precond (k_refresh<Philox | Pcg64, true>, k_refresh_apply_kin_rows<false, true>,
k_refresh_apply_kin<false, true, false | true>) and bk_hmc_draw_gaussian_precond (k_traj_q<.., PD = true> in 64- and 256-thread
workgroups).  tests/test_precond_kernels_cpu.py asserts that every listed shape reaches the form named here and that each
layer of the references notices a planted defect."""
import pytest

import bayes_kit_amd as bk
from tests import precond_kernel_parity as pk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    return bk._lib.default_ops()


# ---- A. bk_leapfrog_finish_precond -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", pk.FINISH_D)
def test_finish_small_shapes(ops, D):
    for C in pk.FINISH_C:
        assert pk.check_finish_small(ops, C, D) < 1.0


@pytest.mark.parametrize("C,D,arrays,form", pk.FINISH_SEAMS)
def test_finish_size_seams(ops, C, D, arrays, form):
    assert pk.check_finish_seam(ops, C, D, arrays, negate=arrays == "inplace") < 1.0


# ---- B. bk_momentum_refresh_precond -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_work", [True, False])
@pytest.mark.parametrize("D", pk.REFRESH_LANES_D)
def test_refresh_lane_per_chain(ops, D, use_work):
    for C in pk.REFRESH_LANES_C:
        assert pk.check_refresh(ops, C, D, use_work=use_work) < 1.0


def test_refresh_lane_per_chain_in_64_thread_workgroups(ops):
    assert pk.check_refresh(ops, *pk.REFRESH_LANES_BIG) < 1.0


@pytest.mark.parametrize("C,D", pk.REFRESH_PCG)
def test_refresh_pcg64(ops, C, D):
    assert pk.check_refresh(ops, C, D, pcg=True) < 1.0


@pytest.mark.parametrize("D", pk.REFRESH_ROWS_D)
def test_refresh_rows_kernel(ops, D):
    for C in pk.REFRESH_ROWS_C:
        assert pk.check_refresh(ops, C, D) < 1.0


@pytest.mark.parametrize("D", pk.REFRESH_PLAIN_D)
def test_refresh_past_the_rows_kernel(ops, D):
    for C in pk.REFRESH_PLAIN_C:
        assert pk.check_refresh(ops, C, D) < 1.0


@pytest.mark.parametrize("C,D", [pk.REFRESH_PLAIN_BIG, pk.REFRESH_NT], ids=["resident", "non_temporal"])
def test_refresh_at_the_cache_size(ops, C, D):
    assert pk.check_refresh(ops, C, D) < 1.0


# ---- C. bk_hmc_draw_gaussian_precond ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", pk.DRAW_C)
@pytest.mark.parametrize("D", pk.DRAW_D)
def test_whole_draw(ops, D, C):
    assert pk.check_draw(ops, C, D) < 1.0
