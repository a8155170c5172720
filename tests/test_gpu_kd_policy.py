"""The in-place step of a cache-resident tile with a cache policy per access (bk_tile_kernels.hpp: k_kick_drift_tile,
k_gauss_grad_tile, reached from bk_leapfrog_kick_drift and the separable Gaussians' gradient-only op when the call is in
place on three different arrays / inside the cache and gridDim.x is a multiple of 8).  A policy decides where a line lives,
never what it holds: every output is the same double as the separately rounded torch expression
    t = m * g;  r = rho (+ pre * t) + kick * t;  theta' = theta + eps * r            grad = -(lam * theta)
every element of the [D, C] views is written exactly once and nothing outside them is touched -- the new kernels address a
row through a buffer resource of the row's own size, so pitch padding and extra rows, pre-filled with NaN, stay NaN.  The
calls that keep the old kernels (other grids, out of place) are pinned to the same expression.

Shapes (C, D, pitch): the smallest at which the routing or the addressing can go wrong.
    (4096, 1, 4096)     gridDim.x = 8, the smallest grid that routes to the new kernels; one row
    (4096, 5, 4098)     gridDim.x = 8; odd D, padded pitch
    (8192, 3, 8192)     gridDim.x = 16
    (4094, 3, 4094)     gridDim.x = 8 with the last column block ragged
    (2, 1, 2), (2048, 5, 2048), (4098, 3, 4098)     gridDim.x = 1, 4, 9: the old kernel
    (4096, 5, 4096) out of place                    the old kernel, inputs untouched
"""
import numpy as np
import pytest
import torch

import bayes_kit_amd as bk

pytestmark = pytest.mark.gpu

EXTRA = 2  # rows past D in every buffer


@pytest.fixture(scope="module")
def ops():
    return bk._lib.default_ops()


def _padded(D, C, ld, fill):
    """A [D, C] view with row pitch ld inside a buffer of D + EXTRA rows; returns (whole buffer [D + EXTRA, ld], view)."""
    whole = torch.empty((D + EXTRA) * ld, dtype=torch.float64, device="cuda").view(D + EXTRA, ld)
    whole.fill_(fill)
    return whole, whole[:D, :C]


def _bits(t):
    return t.contiguous().view(torch.int64)


def _nan_outside(whole, D, C):
    return bool(torch.isnan(whole[:D, C:]).all()) and bool(torch.isnan(whole[D:]).all())


def _inputs(C, D, ld, seed):
    """theta, rho, g as [D, C] views of NaN-filled padded buffers, their values, and a metric."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    bufs, views, vals = [], [], []
    for _ in range(3):
        whole, view = _padded(D, C, ld, float("nan"))
        val = torch.randn(D, C, dtype=torch.float64, device="cuda", generator=gen)
        view.copy_(val)
        bufs.append(whole), views.append(view), vals.append(val)
    metric = torch.as_tensor(np.logspace(-0.5, 0.5, D), dtype=torch.float64, device="cuda")
    return bufs, views, vals, metric


EPS, PRE, KICK = 0.0625 + 1e-3, 0.03125 + 1e-4, 0.07 + 1e-5  # (no powers of two: every product rounds)


def _expected(theta, rho, g, metric, use_pre):
    t = metric[:, None] * g if metric is not None else g
    r = rho
    if use_pre:
        r = r + PRE * t
    r = r + KICK * t
    return theta + EPS * r, r


KD_CASES = [
    # C, D, ld
    (4096, 1, 4096),
    (4096, 5, 4098),
    (8192, 3, 8192),
    (4094, 3, 4094),
    (2, 1, 2),
    (2048, 5, 2048),
    (4098, 3, 4098),
]


@pytest.mark.parametrize("use_pre", [False, True], ids=["kick", "pre+kick"])
@pytest.mark.parametrize("with_metric", [False, True], ids=["unit", "metric"])
@pytest.mark.parametrize("C,D,ld", KD_CASES, ids=[f"{c[0]}x{c[1]}-ld{c[2]}" for c in KD_CASES])
def test_in_place_kick_drift_bits_and_bounds(ops, C, D, ld, with_metric, use_pre):
    bufs, (theta, rho, g), (t0, r0, g0), metric = _inputs(C, D, ld, 1000 * C + D)
    metric = metric if with_metric else None
    assert theta.stride(0) == rho.stride(0) == g.stride(0) == ld
    assert len({theta.data_ptr(), rho.data_ptr(), g.data_ptr()}) == 3
    ops.kick_drift(theta, theta, rho, rho, g, metric, EPS, use_pre, PRE, True, KICK)
    torch.cuda.synchronize()
    want_theta, want_rho = _expected(t0, r0, g0, metric, use_pre)
    assert torch.equal(_bits(theta), _bits(want_theta))
    assert torch.equal(_bits(rho), _bits(want_rho))
    assert torch.equal(_bits(g), _bits(g0)), "gradient written"
    for whole in bufs:
        assert _nan_outside(whole, D, C), "pitch padding or rows past D written"


@pytest.mark.parametrize("use_pre", [False, True], ids=["kick", "pre+kick"])
@pytest.mark.parametrize("with_metric", [False, True], ids=["unit", "metric"])
def test_out_of_place_kick_drift_bits_and_bounds(ops, with_metric, use_pre):
    C, D, ld = 4096, 5, 4096
    bufs, (theta, rho, g), (t0, r0, g0), metric = _inputs(C, D, ld, 77)
    metric = metric if with_metric else None
    whole_t, theta_out = _padded(D, C, ld, float("nan"))
    whole_r, rho_out = _padded(D, C, ld, float("nan"))
    ops.kick_drift(theta, theta_out, rho, rho_out, g, metric, EPS, use_pre, PRE, True, KICK)
    torch.cuda.synchronize()
    want_theta, want_rho = _expected(t0, r0, g0, metric, use_pre)
    assert torch.equal(_bits(theta_out), _bits(want_theta))
    assert torch.equal(_bits(rho_out), _bits(want_rho))
    for view, val in ((theta, t0), (rho, r0), (g, g0)):
        assert torch.equal(_bits(view), _bits(val)), "input written"
    for whole in bufs + [whole_t, whole_r]:
        assert _nan_outside(whole, D, C), "rows past D written"


GRAD_CASES = [(4096, 5, 4098), (8192, 3, 8192)]


@pytest.mark.parametrize("kind", ["diag_gaussian", "iso_gaussian"])
@pytest.mark.parametrize("C,D,ld", GRAD_CASES, ids=[f"{c[0]}x{c[1]}-ld{c[2]}" for c in GRAD_CASES])
def test_gradient_only_bits_and_bounds(ops, kind, C, D, ld):
    gen = torch.Generator(device="cuda").manual_seed(1000 * C + D)
    whole_t, theta = _padded(D, C, ld, float("nan"))
    t0 = torch.randn(D, C, dtype=torch.float64, device="cuda", generator=gen)
    theta.copy_(t0)
    whole, out = _padded(D, C, ld, float("nan"))
    lam = None
    if kind == "diag_gaussian":
        lam = torch.as_tensor(np.logspace(-1, 1, D), dtype=torch.float64, device="cuda")
    ops.target_grad(kind, lam, theta, out, None)
    torch.cuda.synchronize()
    want = -t0 if lam is None else -(lam[:, None] * t0)
    assert torch.equal(_bits(out), _bits(want))
    assert torch.equal(_bits(theta), _bits(t0)), "theta written"
    assert _nan_outside(whole, D, C) and _nan_outside(whole_t, D, C), "pitch padding or rows past D written"


def test_tiled_opaque_draws_equal_untiled():
    """HMCDiag on DiagGaussian through the model-opaque loop, 8,192 chains x 3, L = 3: two tiles of 4,096 chains (gridDim.x =
    8: every in-place step of a tile takes the new kernels) against no tiling (gridDim.x = 16, the new kernels on the whole
    state): state, log density and accept mask bit-equal over two draws."""
    lam = np.logspace(0, 1, 3)
    a = bk.HMCDiag(bk.DiagGaussian(lam), 0.05, 3, chains=8192, seed=11, path="opaque", chain_tile=0)
    b = bk.HMCDiag(bk.DiagGaussian(lam), 0.05, 3, chains=8192, seed=11, path="opaque", chain_tile=4096)
    assert a._chain_tile == 8192 and b._chain_tile == 4096
    for _ in range(2):
        ta, la = a.sample()
        tb, lb = b.sample()
        assert torch.equal(_bits(ta), _bits(tb)) and torch.equal(_bits(la), _bits(lb))
        assert torch.equal(a.last_accept, b.last_accept)
