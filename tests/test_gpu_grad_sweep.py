"""Row sweep of the separable Gaussians' gradient-only kernels (bk_targets.hip: k_gauss_grad_v2<1, false>, <1, true>,
<2, false> and k_gauss_grad_s).  The kernels map blockIdx.y to row groups from the last to the first when the grid keeps a
column block on one XCD (gridDim.x a multiple of 8) and ascending otherwise; they are elementwise, so under either map
every output is the same double as the torch expression, every element of the [D, C] view is written exactly once and
nothing outside it is touched: pitch padding and extra rows, pre-filled with NaN, stay NaN.

Shapes: the smallest at which the block-to-row map can go wrong, once in each direction of the sweep.
    (2, 1)                          one row group, one block
    (2, 3), (514, 5)                two column blocks, odd D
    (4096, 5)                       the same kernel with gridDim.x = 8: descending
    (3, 4 | 5 | 7), odd pitch       k_gauss_grad_s, its last row group of 4 ragged at D = 5 and D = 7
    (4, 5 | 7), view offset 8 B     k_gauss_grad_s through the alignment rule
    (2048, 5 | 7), odd pitch        k_gauss_grad_s with gridDim.x = 8: descending, ragged
    (2, 65537)                      two rows per thread (D > 65,535), last row group half empty
    (4096, 65537)                   the same with gridDim.x = 8: descending (one launch over 2 GiB)
    (8192, 2048), distinct arrays   2 x 128 MiB, past the streaming threshold: the non-temporal variant, descending
"""
import numpy as np
import pytest
import torch

import bayes_kit_amd as bk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    return bk._lib.default_ops()


def _padded(D, C, ld, extra, offset, fill):
    """A [D, C] view with row pitch ld inside a buffer of D + extra rows that starts `offset` doubles into its allocation;
    returns (whole buffer as [D + extra, ld], view)."""
    flat = torch.empty((D + extra) * ld + offset, dtype=torch.float64, device="cuda")
    whole = flat[offset:].view(D + extra, ld)
    whole.fill_(fill)
    return whole, whole[:D, :C]


def _bits(t):
    return t.contiguous().view(torch.int64)


CASES = [
    # C, D, ld, extra rows, offset in doubles
    (2, 1, 4, 2, 0),
    (2, 3, 4, 2, 0),
    (514, 5, 516, 3, 0),
    (4096, 5, 4098, 3, 0),
    (3, 4, 5, 2, 0),
    (3, 5, 5, 2, 0),
    (3, 7, 5, 2, 0),
    (4, 5, 6, 2, 1),
    (4, 7, 6, 2, 1),
    (2048, 5, 2051, 2, 0),
    (2048, 7, 2051, 2, 0),
    (2, 65537, 4, 1, 0),
    (4096, 65537, 4098, 1, 0),
    (8192, 2048, 8194, 1, 0),
]


@pytest.mark.parametrize("kind", ["diag_gaussian", "iso_gaussian"])
@pytest.mark.parametrize("C,D,ld,extra,offset", CASES, ids=[f"{c[0]}x{c[1]}-ld{c[2]}-off{c[4]}" for c in CASES])
def test_gradient_only_bits_and_bounds(ops, kind, C, D, ld, extra, offset):
    g = torch.Generator(device="cuda").manual_seed(1000 * C + D)
    _, theta = _padded(D, C, ld, extra, offset, 0.0)
    theta.copy_(torch.randn(D, C, dtype=torch.float64, device="cuda", generator=g))
    whole, out = _padded(D, C, ld, extra, offset, float("nan"))
    assert theta.data_ptr() != out.data_ptr() and theta.stride(0) == out.stride(0) == ld
    assert (theta.data_ptr() % 16 == 0) == (offset % 2 == 0)
    lam = None
    if kind == "diag_gaussian":
        lam = torch.as_tensor(np.logspace(-1, 1, D), dtype=torch.float64, device="cuda")
    ops.target_grad(kind, lam, theta, out, None)
    torch.cuda.synchronize()
    want = -theta if lam is None else -(lam[:, None] * theta)
    assert torch.equal(_bits(out), _bits(want))
    del want
    assert bool(torch.isnan(whole[:D, C:]).all()), "pitch padding written"
    assert bool(torch.isnan(whole[D:]).all()), "rows past D written"


def test_tiled_opaque_draws_equal_untiled(ops):
    """HMCDiag on DiagGaussian through the model-opaque loop (one kick+drift and one gradient op per step), two tiles of 4
    chains against no tiling: state, log density and accept mask bit-equal over two draws."""
    lam = np.logspace(0, 1, 3)
    a = bk.HMCDiag(bk.DiagGaussian(lam), 0.05, 3, chains=8, seed=11, path="opaque", chain_tile=0)
    b = bk.HMCDiag(bk.DiagGaussian(lam), 0.05, 3, chains=8, seed=11, path="opaque", chain_tile=4)
    assert a._chain_tile == 8 and b._chain_tile == 4
    for _ in range(2):
        ta, la = a.sample()
        tb, lb = b.sample()
        assert torch.equal(_bits(ta), _bits(tb)) and torch.equal(_bits(la), _bits(lb))
        assert torch.equal(a.last_accept, b.last_accept)
