"""bk.TemperedHMC and its four entry points on the MI355X: the kernels against their NumPy restatements and against the
plain integrator's kernels, the sampler against the sampler on the stand-in (tests/fake_ops_temper_hmc.py), one rung against
bk.HMCDiag, checkpoints, every rung's own target, a two-mode posterior with its evidence, and the per-rung warmup."""
import numpy as np
import pytest

import bayes_kit_amd as bk
from tests import temper_hmc_parity as hp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    return bk._lib.default_ops()


@pytest.mark.parametrize("H,T", [(H, T) for H in (1, 2, 63, 64, 65, 257) for T in (2, 3)])
def test_kernels_equal_their_restatements(ops, H, T):
    """bk_tempered_kick_drift, bk_tempered_finish and bk_tempered_hmc_accept, bit for bit, counters exact.  replicas 1 and 2;
    D in (1, 3, 4, 5, 33): ragged row blocks, empty quarters of the kinetic sum; pitch pads 0 and 6 with even C: two columns
    per lane on 16-byte words (with odd H on different rungs); pad 5, odd C or a view that is 8-byte aligned only: one column
    per lane; grad_lp0, metric, pre and kick present and NULL; in place and out of place; beta = 0 against an infinite
    gradient entry; log u random, -inf, 0.0, +inf and NaN; -inf, +inf and NaN in ll with a beta = 0 rung; H = 63, 65, 257:
    wavefronts that straddle blocks of H columns count per lane."""
    hp.check_kernels(ops, H, T)


@pytest.mark.parametrize("C", [130, 129])
def test_degenerate_case_equals_the_plain_integrator_bit_for_bit(ops, C):
    """beta = 1, uniform vectors, no lp0: bk_leapfrog_kick_drift and bk_leapfrog_finish; C = 130 the 16-byte forms, 129 the
    8-byte ones."""
    hp.check_degenerate_equality(ops, C, 33)


@pytest.mark.parametrize("H", [1, 64, 65])
@pytest.mark.parametrize("pad", [0, 5])
def test_exchange_columns_is_the_exchange_pass_of_replica_swap(ops, H, pad):
    for T, replicas, D in ((2, 1, 5), (3, 2, 33)):
        hp.check_exchange_kernel(ops, H, T, replicas, D, pad=pad)


@pytest.mark.parametrize("C,D,eps", [(130, 5, 0.17), (258, 130, 0.09)])
def test_one_rung_is_hmc_bit_for_bit(ops, C, D, eps):
    hp.check_one_rung_is_hmc(ops, C, D, draws=6, stepsize=eps)


@pytest.mark.parametrize("chains,T,replicas,D", [(130, 3, 1, 5), (64, 4, 2, 33)])
@pytest.mark.parametrize("split", [False, True])
def test_sampler_equals_the_sampler_on_the_stand_in(ops, chains, T, replicas, D, split):
    """warmup(30) (equal reports) and 6 draws, bit for bit."""
    hp.check_sampler_vs_stand_in(ops, chains, T, replicas, D, draws=6, split=split, warm=30)


@pytest.mark.parametrize("split", [False, True])
def test_state_dict_round_trip_continues_bit_for_bit(ops, split):
    sd = hp.check_state_round_trip(ops, [1.0, 0.4, 0.1], 130, 1, 5, split=split)
    with pytest.raises(ValueError):
        hp.make(ops, [1.0, 0.5, 0.1], 130, 1, 5, split=split, swap_every=2).load_state_dict(sd)


def test_every_rung_samples_its_own_target(ops):
    """tests/temper_hmc_parity.py::run_rung_moments.  The vectorised NumPy run of the scheme (SchemeNumpy) gave over 20 seeds
    max_t |mean error| / sd <= 0.0128 and max_t |var ratio - 1| <= 0.0208; bounded here by twice that, 0.026 and 0.042.  The
    stand-in (tests/fake_ops_temper_hmc.py) at this test's seed: 0.0108 and 0.0156 (acceptance per rung
    0.980-0.981, swap rates 0.374, 0.413, 0.532, 0.737, 0.838)."""
    mean_err, var_err, s = hp.run_rung_moments(ops)
    print(f"tempered HMC rungs: max |mean error| / sd = {mean_err:.4f}, max |var ratio - 1| = {var_err:.4f}, "
          f"acceptance per rung = {np.round(s.rung_accept_rate(), 3)}, swap rates = {np.round(s.swap_rate(), 3)}")
    assert mean_err <= 0.026
    assert var_err <= 0.042


def test_modes_are_found_and_the_evidence_is_right(ops):
    """tests/temper_hmc_parity.py::run_two_modes: all chains start in the minor mode (0.3 of the mass), 12 rungs of 256
    chains.  The NumPy run of the scheme gave over 20 seeds a share of 0.690-0.710 of the cold chains in the major mode, the
    stepping-stone log Z within 0.0124 of the closed form -5.1798 and swap rates of 0.643-0.980; bounded here by twice the
    worst deviations, 0.02 and 0.025.  The stand-in at this test's seed: share 0.7009, log Z -5.1773, swap rates 0.651-0.980, plain HMCDiag
    0.0000."""
    share, log_z, swap, plain = hp.run_two_modes(ops)
    print(f"two modes: share in the major mode = {share:.4f} (plain HMCDiag {plain:.4f}), log Z = {log_z:.4f} "
          f"(closed form {hp.LOG_Z_TWO_MODES:.4f}), swap rates = {np.round(swap, 3)}")
    assert abs(share - 0.7) <= 0.02
    assert abs(log_z - hp.LOG_Z_TWO_MODES) <= 0.025
    assert np.all((swap > 0.0) & (swap < 1.0))
    assert plain <= 0.01


def test_warmup_brings_every_rung_to_the_target_acceptance(ops):
    """tests/temper_hmc_parity.py::run_warmup_band: warmup(150) towards 0.8, then 100 draws.  The NumPy run of the scheme
    gave over 20 seeds every rung's acceptance within 0.0089 of 0.8 (final step sizes 0.527 ... 2.19 from cold to hot);
    bounded here by 0.02.  The stand-in at this test's seed: acceptance 0.8004, 0.7956, 0.7948, 0.8055, 0.7982,
    0.8014 with step sizes 0.525, 0.885, 1.346, 1.757, 2.016, 2.156."""
    acc, s = hp.run_warmup_band(ops)
    print(f"warmup: acceptance per rung = {np.round(acc, 4)}, step sizes = {np.round(s.stepsizes, 4)}")
    assert np.all(np.abs(acc - 0.8) <= 0.02)
    assert np.all(np.diff(s.stepsizes) > 0)  # (a hotter rung is wider)
