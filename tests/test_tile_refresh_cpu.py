"""The tile-major HMC loop with each tile's momentum refreshed into the tile's own workspace, without a GPU: on the NumPy
stand-in that has the per-pitch entry points, the tiled sampler gives the untiled sampler's draws and leaves every chain's
stream where the untiled one leaves it.  (The stand-in has no second stream: the in-line schedule only.)"""
import numpy as np
import pytest
import torch

import bayes_kit_amd as bk
from tests.fake_ops_energy import EnergyFakeOps

D_S, L_S = 5, 3
LAM_S = np.logspace(0, 1, D_S)


def _sampler(ops, C, tile):
    s = bk.HMCDiag(bk.DiagGaussian(LAM_S, ops=ops), 0.1, L_S, chains=C, seed=11, path="opaque", chain_tile=tile, ops=ops)
    s._theta_dc.mul_(torch.as_tensor(1.0 / np.sqrt(LAM_S))[:, None])
    return s


def _draws(s, n):
    out = []
    for _ in range(n):
        th, lp = s.sample()
        out.append((th.clone(), lp.clone(), s._mask.clone(), torch.as_tensor(s.rng_state().view(np.int64).copy())))
    return out


def _same(ra, rb):
    assert len(ra) == len(rb)
    for n, (x, y) in enumerate(zip(ra, rb)):
        for what, u, v in zip(("theta", "logp", "mask", "rng state"), x, y):
            assert torch.equal(u, v), (what, n)


@pytest.mark.parametrize("C", [96, 80])  # T = 32: three full tiles; two and a ragged third of 16 chains
def test_per_tile_refresh_draws_equal_untiled(C):
    ops = EnergyFakeOps()
    a, b = _sampler(ops, C, 0), _sampler(ops, C, 32)
    assert not b._prefetch and b._chain_tile == 32
    ra = _draws(a, 5)
    n0 = ops.calls["momentum_refresh"]
    rb = _draws(b, 2)
    assert ops.calls["momentum_refresh"] - n0 == 2 * 3  # one refresh per tile and draw
    sd = b.state_dict()
    rb += _draws(b, 3)
    _same(ra, rb)
    assert b._tm_last and 0.0 < b.accept_rate() < 1.0
    assert all(r is None for r in b._rho_bufs) and b._rho_tile.numel() == D_S * 32
    c = _sampler(ops, C, 32)
    c.load_state_dict(sd)
    _same(ra[2:], _draws(c, 3))


def test_a_draw_without_steps_leaves_the_tiles_and_comes_back():
    ops = EnergyFakeOps()
    a, b = _sampler(ops, 80, 0), _sampler(ops, 80, 32)
    ra, rb = _draws(a, 1), _draws(b, 1)
    a._steps = b._steps = 0
    ra += _draws(a, 1)
    rb += _draws(b, 1)
    assert b._rho_bufs[0] is not None and not b._tm_last  # the plain path got its full-width momentum
    a._steps = b._steps = L_S
    ra += _draws(a, 2)
    rb += _draws(b, 2)
    assert b._tm_last
    _same(ra, rb)
