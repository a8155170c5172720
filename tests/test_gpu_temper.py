"""bk.TemperedStretcher, bk_tempered_accept and bk_replica_swap on the MI355X: the kernels against their NumPy restatements,
the sampler against the sampler on the stand-in (tests/fake_ops_temper.py), one rung against bk.Stretcher, checkpoints,
every rung's own target, and a two-mode posterior with its evidence."""
import numpy as np
import pytest

import bayes_kit_amd as bk
from tests import temper_parity as tp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    return bk._lib.default_ops()


@pytest.mark.parametrize("H,T", [(H, T) for H in (1, 2, 63, 64, 65, 257) for T in (2, 3)])
def test_kernels_equal_their_restatements(ops, H, T):
    """bk_replica_swap and bk_tempered_accept, bit for bit, counters exact.  replicas 1 and 2, both parities; D = 33: nine row
    blocks, the last one ragged; row pads 0 and 6 with even H: two pairs per lane on 16-byte words; pad 5 or odd H: one pair
    per lane; H = 63, 65, 257: wavefronts that straddle blocks of H columns count per lane, H = 64: every wavefront inside
    one block; log u random, all -inf (every pair swaps, twice: the original is back), all 0.0 (the pairs whose ratio exceeds
    one swap) and all +inf / NaN (nothing moves); -inf, +inf and NaN in ll with a beta = 0 rung."""
    tp.check_kernels(ops, H, T)


@pytest.mark.parametrize("walkers,replicas,D", [(130, 1, 5), (258, 2, 130)])
def test_one_rung_is_stretcher_bit_for_bit(ops, walkers, replicas, D):
    tp.check_one_rung_is_stretcher(ops, walkers, replicas, D, draws=6)


@pytest.mark.parametrize("walkers,T,replicas,D,split", [(130, 3, 1, 5, False), (64, 4, 2, 33, False), (130, 3, 1, 5, True)])
def test_sampler_equals_the_sampler_on_the_stand_in(ops, walkers, T, replicas, D, split):
    tp.check_sampler_vs_stand_in(ops, np.geomspace(1.0, 0.05, T), walkers, replicas, D, draws=6, split=split)


@pytest.mark.parametrize("split", [False, True])
def test_state_dict_round_trip_continues_bit_for_bit(ops, split):
    sd = tp.check_state_round_trip(ops, [1.0, 0.4, 0.1], 130, 1, 5, split=split)
    with pytest.raises(ValueError):
        tp.make(ops, [1.0, 0.5, 0.1], 130, 1, 5, split=split, swap_every=2).load_state_dict(sd)


def test_every_rung_samples_its_own_target(ops):
    """tests/temper_parity.py::run_rung_moments.  A NumPy run of the scheme gave over 20 seeds max_t |mean error| / sd <=
    0.023 and max_t |var ratio - 1| <= 0.022; both are bounded by 0.06 here.  The stand-in (tests/fake_ops_temper.py) at
    this test's seed: 0.0123 and 0.0363 (acceptance per rung 0.641-0.651, swap rates 0.368, 0.403, 0.529, 0.732, 0.840)."""
    mean_err, var_err, s = tp.run_rung_moments(ops)
    print(f"tempered rungs: max |mean error| / sd = {mean_err:.4f}, max |var ratio - 1| = {var_err:.4f}, "
          f"acceptance per rung = {np.round(s.rung_accept_rate(), 3)}, swap rates = {np.round(s.swap_rate(), 3)}")
    assert mean_err <= 0.06
    assert var_err <= 0.06


def test_modes_are_found_and_the_evidence_is_right(ops):
    """tests/temper_parity.py::run_two_modes: all walkers start in the minor mode (0.3 of the mass).  A NumPy run of the
    scheme gave over 20 seeds a share of 0.683-0.713 of the cold walkers in the major mode (sd 0.008), the stepping-stone
    log Z within 0.031 of the closed form -5.1798 (sd 0.012) and a smallest swap rate of 0.65; a plain Stretcher left 0.000
    there.  The stand-in at this test's seed: share 0.7065, log Z -5.1766, swap rates 0.649-0.979, plain Stretcher 0.0000."""
    share, log_z, swap, plain = tp.run_two_modes(ops)
    print(f"two modes: share in the major mode = {share:.4f} (plain Stretcher {plain:.4f}), log Z = {log_z:.4f} "
          f"(closed form {tp.LOG_Z_TWO_MODES:.4f}), swap rates = {np.round(swap, 3)}")
    assert abs(share - 0.7) <= 0.04
    assert abs(log_z - (-5.1798)) <= 0.06
    assert np.all((swap > 0.4) & (swap < 1.0))
    assert plain <= 0.01
