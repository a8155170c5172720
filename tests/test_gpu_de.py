"""bk.DifferentialEvolution, bk.TemperedDifferentialEvolution and bk_de_propose on the MI355X: the kernel against its
NumPy restatement, the samplers against the samplers on the stand-in (tests/fake_ops_de.py), the target's moments, two
modes, checkpoints."""
import pytest

import bayes_kit_amd as bk
from tests import de_parity as dp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    return bk._lib.default_ops()


@pytest.mark.parametrize("H,E", [(H, E) for H in (2, 3, 63, 64, 65, 257) for E in (1, 3)] + [(257, 4)])
def test_kernel_equals_its_restatement(ops, H, E):
    """theta_prop, both partner arrays and gamma bit for bit.  H = 2: the smallest half, the second partner is the other
    walker; H * E odd: the one-walker-per-lane form, and a second half whose base is 8-byte aligned only; H * E even: two
    walkers per lane; 257 * 3 walkers: four workgroups of the first form, the last one ragged; 257 * 4: three of the second;
    D = 33: nine row blocks, the last one ragged, dealt in groups of eight; pad: rows further apart than C with NaN between
    them, and a proposal pitch of its own (6: even pitches, 5: odd ones -- the one-walker form on an even count); whole
    vectors of u_1 and u_2 at the ends of [0, 1), alone and together, z = 0 and sigma = 0; and uniforms that are none."""
    for D in (1, 2, 5, 33):
        for half in (0, 1):
            for pad in (0, 6, 5):
                dp.check_kernel(ops, H, E, D, half, pad=pad)
        for inject in dp.INJECTS[1:]:
            dp.check_kernel(ops, H, E, D, 1, pad=0, inject=inject)
            dp.check_kernel(ops, H, E, D, 0, pad=6, inject=inject)
        for half in (0, 1):
            dp.check_kernel_any_uniforms(ops, H, E, D, half)


def test_kernel_partner_clamp_at_a_million_walkers_per_half(ops):
    """H = 2^20 + 1, D = 1: u_1 and u_2 at 1 - 2^-53 give the last walkers of the other half, never the column behind it, and
    at 0 the first ones, never the column before it; the two always differ; an odd count, so the second half is the
    unaligned one."""
    H = 2 ** 20 + 1
    for half in (0, 1):
        dp.check_kernel(ops, H, 1, 1, half, inject="both_1")
        dp.check_kernel(ops, H, 1, 1, half, inject="both_0")
    dp.check_kernel(ops, H, 1, 1, 1, inject="u1_1")
    dp.check_kernel(ops, H, 1, 1, 0, inject="u2_1")
    dp.check_kernel(ops, H, 1, 1, 1, inject="u2_0")
    dp.check_kernel(ops, H, 1, 1, 0)


@pytest.mark.parametrize("jump_every", [0, 2])
@pytest.mark.parametrize("walkers,E,D", [(130, 1, 5), (64, 3, 33), (258, 2, 130)])
def test_sampler_equals_the_sampler_on_the_stand_in(ops, walkers, E, D, jump_every):
    dp.check_sampler_vs_stand_in(ops, walkers, E, D, draws=6, jump_every=jump_every)


def test_tempered_sampler_equals_the_sampler_on_the_stand_in(ops):
    dp.check_tempered_vs_stand_in(ops, [1.0, 0.5, 0.2], 66, 2, 5, draws=6, split=True, jump_every=2)


def test_one_rung_is_differential_evolution(ops):
    dp.check_one_rung_is_de(ops, 66, 2, 5, jump_every=2)


def test_target_is_invariant(ops):
    """DiagGaussian([1, 4, 0.25, 100]), 4096 walkers, default gamma = 2.38 / sqrt(8), sigma = 1e-5 and init, 150 draws
    discarded, 50 pooled.  The stand-in (tests/fake_ops_de.py) on the CPU at this test's seed and six further ones gave
    (max |mean| sqrt(lam), max |var lam - 1|, acceptance):
        seed 2024: 0.0190, 0.0072, 0.2870      seed 2025: 0.0259, 0.0114, 0.2878      seed 2026: 0.0107, 0.0082, 0.2867
        seed 2027: 0.0058, 0.0158, 0.2872      seed 2028: 0.0062, 0.0165, 0.2876      seed 2029: 0.0171, 0.0071, 0.2863
        seed 2030: 0.0079, 0.0194, 0.2865
    The bounds on the two moments are 2.3 times the worst of the seven (the margin test_gpu_stretch.py gives the same pooled,
    correlated draws): 2.3 * 0.0259 and 2.3 * 0.0194; the acceptance a band of 0.03 either side of their range 0.2863-0.2878
    (it counts the 150 discarded draws too)."""
    mean, var, rate = dp.run_invariance(ops, seed=2024)
    print(f"differential evolution invariance: max |mean| sqrt(lam) = {mean:.4f}, max |var lam - 1| = {var:.4f}, "
          f"acceptance = {rate:.4f}")
    assert mean <= 0.0596
    assert var <= 0.0446
    assert 0.2563 <= rate <= 0.3178


def test_walkers_cross_between_two_modes(ops):
    """temper_parity.two_mode_model(): 0.3 of the mass at (-3, -3), 0.7 at (3, 3).  512 walkers, every second one started in
    each mode, 400 draws, jump_every = 10: the share of theta[0] > 0 over the last 200 draws is 0.7 within 4 sd.
    A vectorised NumPy run of this scheme from this start gave over 20 seeds a share of 0.688-0.718, mean 0.7005, sd 0.0074
    (with jump_every = 0: 0.682-0.717, sd 0.0104); the stand-in (tests/fake_ops_de.py) at this test's seed: 0.7134.
    A Stretcher from the same start never leaves 0.500: a stretch move does not land in the partner's mode."""
    share, plain = dp.run_two_modes(ops, seed=2025, walkers=512, draws=400, jump_every=10)
    print(f"two modes: share of theta[0] > 0: differential evolution {share:.4f}, stretch move {plain:.4f}")
    assert abs(share - 0.7) <= 4 * 0.0074
    assert abs(plain - 0.5) <= 0.01


def test_state_dict_round_trip_continues_bit_for_bit(ops):
    dp.check_state_round_trip(ops, 130, 1, 5, jump_every=3, before=4)
