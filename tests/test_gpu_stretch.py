"""bk.Stretcher and bk_stretch_propose on the MI355X: the kernel against its NumPy restatement, the sampler against the
sampler on the stand-in (tests/fake_ops_stretch.py), the target's moments, checkpoints, and affine invariance in practice."""
import numpy as np
import pytest
import torch

import bayes_kit_amd as bk
from tests import stretch_parity as sp

pytestmark = pytest.mark.gpu

LAM4 = np.array([1.0, 4.0, 0.25, 100.0])


@pytest.fixture(scope="module")
def ops():
    return bk._lib.default_ops()


@pytest.mark.parametrize("H,E", [(H, E) for H in (1, 2, 63, 64, 65, 257) for E in (1, 3)] + [(257, 4)])
def test_kernel_equals_its_restatement(ops, H, E):
    """theta_prop and partner bit for bit, zterm to 1e-15.  H * E odd: the one-walker-per-lane form, and a second half whose
    base is 8-byte aligned only; H * E even: two walkers per lane; 257 * 3 walkers: four workgroups of the first form, the last
    one ragged; 257 * 4: three of the second; D = 33:
    nine row blocks, the last one ragged, dealt in groups of eight; pad: rows further apart than C with NaN between them,
    and a proposal pitch of its own (6: even pitches, 5: odd ones -- the one-walker form on an even count)."""
    for D in (1, 2, 5, 33):
        for half in (0, 1):
            for pad in (0, 6, 5):
                sp.check_kernel(ops, H, E, D, half, pad=pad)
        for inject in ("uj0", "uj1", "uz0", "uz1"):
            sp.check_kernel(ops, H, E, D, 1, pad=0, inject=inject)
            sp.check_kernel(ops, H, E, D, 0, pad=6, inject=inject)


def test_kernel_partner_clamp_at_a_million_walkers_per_half(ops):
    """H = 2^20 + 1, D = 1: u_j = 1 - 2^-53 gives the last walker of the other half, never the column behind it; an odd
    count, so the second half is the unaligned one."""
    H = 2 ** 20 + 1
    for half in (0, 1):
        sp.check_kernel(ops, H, 1, 1, half, inject="uj1")
    sp.check_kernel(ops, H, 1, 1, 1, inject="uj0")
    sp.check_kernel(ops, H, 1, 1, 0)


@pytest.mark.parametrize("walkers,E,D", [(130, 1, 5), (64, 3, 33), (258, 2, 130)])
def test_sampler_equals_the_sampler_on_the_stand_in(ops, walkers, E, D):
    sp.check_sampler_vs_stand_in(ops, walkers, E, D, draws=6)


def test_target_is_invariant(ops):
    """DiagGaussian([1, 4, 0.25, 100]), 4096 walkers, a = 2, default init, 150 draws discarded, 50 pooled.  A NumPy run of
    this scheme gave over six seeds max |mean| sqrt(lam) <= 0.025, max |var lam - 1| <= 0.026, acceptance 0.593-0.597;
    the bounds are about 2.3 times that (the pooled draws of one ensemble are strongly correlated).  The stand-in
    (tests/fake_ops_stretch.py) at this test's seed: 0.0304, 0.0274 and 0.5856 (the acceptance counts the 150 discarded
    draws too, the first of them from an N(0, I) start that is far too wide for lam = 100)."""
    s = bk.Stretcher(bk.DiagGaussian(LAM4), a=2.0, walkers=4096, seed=2024)
    for _ in range(150):
        s.sample()
    pool = torch.cat([s.sample()[0] for _ in range(50)]).cpu().numpy()
    mean = np.abs(pool.mean(axis=0)) * np.sqrt(LAM4)
    var = np.abs(pool.var(axis=0) * LAM4 - 1.0)
    rate = s.accept_rate()
    print(f"stretcher invariance: max |mean| sqrt(lam) = {mean.max():.4f}, max |var lam - 1| = {var.max():.4f}, "
          f"acceptance = {rate:.4f}")
    assert mean.max() <= 0.06
    assert var.max() <= 0.06
    assert 0.56 <= rate <= 0.63


def test_state_dict_round_trip_continues_bit_for_bit(ops):
    sp.check_state_round_trip(ops, 130, 1, 5)


def test_acceptance_does_not_depend_on_the_scaling_of_the_target(ops):
    """Affine invariance in practice: the badly scaled Gaussian started from the isotropic run's walkers divided by
    sqrt(lam) is the same problem in other units, so the two runs accept alike (equal up to rounding of the map)."""
    init = np.random.default_rng(7).normal(size=(4096, 4))
    iso = bk.Stretcher(bk.IsoGaussian(4), walkers=4096, init=init, seed=31)
    diag = bk.Stretcher(bk.DiagGaussian(LAM4), walkers=4096, init=init / np.sqrt(LAM4), seed=31)
    for _ in range(30):
        iso.sample()
        diag.sample()
    print(f"stretcher acceptance: iso {iso.accept_rate():.4f}, scaled {diag.accept_rate():.4f}")
    assert abs(iso.accept_rate() - diag.accept_rate()) <= 0.01
    assert 0.4 < iso.accept_rate() < 0.8
