"""Cache-resident chain tiles on the GPU: a tiled draw equals the untiled one bit for bit, and kick+drift and the Gaussian
gradient op give the separately rounded result on both sides of the size at which they change variant."""
import numpy as np
import pytest
import torch

import bayes_kit_amd as bk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    return bk._lib.default_ops()


# -- tiled == untiled --------------------------------------------------------------------------------------------------
def _run(C, D, L, tile, draws=3, **kw):
    lam = np.logspace(0, 2, D)
    s = bk.HMCDiag(bk.DiagGaussian(lam), 0.05, L, chains=C, seed=11, path="opaque", chain_tile=tile, **kw)
    # start at the target's own widths: from there a draw accepts some proposals and rejects others, with metric_diag too
    # (acceptance 0.86-0.95 in the four settings below), so the compared state is what the trajectories produced
    s._theta_dc.mul_(torch.as_tensor(1.0 / np.sqrt(lam), device=s._theta_dc.device)[:, None])
    out = []
    for _ in range(draws):
        th, lp = s.sample()
        out.append((th.clone(), lp.clone(), s._mask.clone(), s._rng_state.clone(),
                    s._theta_p.clone(), s._lp_p.clone(), s._kin1.clone(), s._grad_p.clone()))
    return s, out


WHAT = ("theta", "logp", "mask", "rng state", "proposal", "proposal's logp", "proposal's kinetic energy", "proposal's gradient")


@pytest.mark.parametrize("C,tile", [(1026, 512), (130, 64)])  # tiles of 512, 512 and 2 chains; of 64, 64 and 2
@pytest.mark.parametrize("prefetch_rng", [True, False])
@pytest.mark.parametrize("metric", [False, True])
def test_tiled_draws_equal_untiled_bit_for_bit(C, tile, prefetch_rng, metric):
    D, L = 33, 3
    kw = dict(prefetch_rng=prefetch_rng)
    if metric:
        kw["metric_diag"] = np.linspace(0.9, 1.1, D)
    a, ra = _run(C, D, L, 0, **kw)
    b, rb = _run(C, D, L, tile, **kw)
    assert a._chain_tile == C and b._chain_tile == tile
    assert not (b._fused_draw or b._step_hook or b._traj_hook or b._lanes_traj)
    for n, (x, y) in enumerate(zip(ra, rb)):
        for what, u, v in zip(WHAT, x, y):
            assert torch.equal(u, v), (what, n)
    assert a.accept_rate() == b.accept_rate()
    assert 0.0 < a.accept_rate() < 1.0  # both branches of the select took part


# -- the variant seam --------------------------------------------------------------------------------------------------
# D = 1024: three arrays of 8,192 chains are 192 MiB, the largest footprint that counts as cache resident; 8,194 chains are
# just past it.  Every product and sum of the torch expressions below is a kernel of its own, hence rounded separately.
D_SEAM = 1024
EPS = 0.0123


@pytest.fixture(scope="module")
def seam_inputs(ops):
    g = torch.Generator(device=ops.device)
    g.manual_seed(5)
    th, rho, gr = (torch.randn((D_SEAM, 8194), dtype=torch.float64, device=ops.device, generator=g) for _ in range(3))
    m = torch.linspace(0.5, 1.5, D_SEAM, dtype=torch.float64, device=ops.device)
    lam = torch.logspace(0, 4, D_SEAM, dtype=torch.float64, device=ops.device)
    return th, rho, gr, m, lam


def _expect(th, rho, gr, m, use_pre, pre, use_kick, kick):
    t = m[:, None] * gr
    r = rho
    if use_pre:
        r = r + pre * t
    if use_kick:
        r = r + kick * t
    return th + EPS * r, r


@pytest.mark.parametrize("C", [8192, 8194])
def test_kick_drift_in_place_on_both_sides_of_the_cache_threshold(ops, seam_inputs, C):
    th, rho, gr, m, _ = (x[:, :C].clone() if x.dim() == 2 else x for x in seam_inputs)  # (the inputs are shared)
    assert (3 * 8 * C * D_SEAM <= bk.HMCDiag.LLC_BYTES) == (C == 8192)
    want_th, want_rho = _expect(th, rho, gr, m, False, 0.0, True, EPS)
    ops.kick_drift(th, th, rho, rho, gr, m, EPS, False, 0.0, True, EPS)  # the steady-state step: three arrays
    assert torch.equal(th, want_th) and torch.equal(rho, want_rho)


def test_kick_drift_out_of_place_at_the_resident_size(ops, seam_inputs):
    """The first step of a tile: theta -> theta', rho in place; four arrays of 64 MiB are past the threshold."""
    C = 8192
    th, rho, gr, m, _ = (x[:, :C].clone() if x.dim() == 2 else x for x in seam_inputs)
    tho = torch.full_like(th, float("nan"))
    want_th, want_rho = _expect(th, rho, gr, m, True, -0.5 * EPS, True, EPS)
    th0 = th.clone()
    ops.kick_drift(th, tho, rho, rho, gr, m, EPS, True, -0.5 * EPS, True, EPS)
    assert torch.equal(tho, want_th) and torch.equal(rho, want_rho) and torch.equal(th, th0)


@pytest.mark.parametrize("C", [8192, 8194, 12288, 12290])  # (12,288: the op's own two arrays reach 192 MiB)
def test_gaussian_gradient_op_on_both_sides_of_the_cache_threshold(ops, seam_inputs, C):
    th, _, _, _, lam = seam_inputs
    th = th[:, :C].contiguous() if C <= th.shape[1] else torch.cat([th, th[:, : C - th.shape[1]] * 0.5], dim=1).contiguous()
    assert th.shape == (D_SEAM, C)
    grad = torch.full_like(th, float("nan"))
    bk.DiagGaussian(lam).bk_eval(th, grad, None)
    assert torch.equal(grad, -(lam[:, None] * th))


def test_a_resident_tile_of_a_larger_state(ops, seam_inputs):
    """What the tiled loop launches: columns [c0, c0 + T) of arrays with a longer leading dimension."""
    th, rho, gr, m, lam = seam_inputs
    big = [torch.cat([x, x * 0.25], dim=1).contiguous() for x in (th, rho, gr)]  # [1024, 16388]
    c0, T = 4098, 8192
    tv, rv, gv = (x[:, c0:c0 + T] for x in big)
    keep = [x.clone() for x in big]
    want_th, want_rho = _expect(tv, rv, gv, m, False, 0.0, True, EPS)
    ops.kick_drift(tv, tv, rv, rv, gv, m, EPS, False, 0.0, True, EPS)
    assert torch.equal(tv, want_th) and torch.equal(rv, want_rho)
    bk.DiagGaussian(lam).bk_eval(tv, gv, None)
    assert torch.equal(gv, -(lam[:, None] * want_th))
    for x, k in zip(big, keep):  # nothing outside the tile's columns was written
        assert torch.equal(x[:, :c0], k[:, :c0]) and torch.equal(x[:, c0 + T:], k[:, c0 + T:])
