"""The tile-major store of the tiled HMC schedule without a GPU: where tile k's block lies for a ragged chain count, and
that `_theta_p` / `_grad_p` hand back [D, C] arrays assembled from the blocks."""
import pytest
import torch

from bayes_kit_amd.hmc import HMCDiag


@pytest.mark.parametrize("C,D,T", [(1026, 33, 512), (130, 33, 64), (131, 5, 64), (64, 7, 64), (65536, 1024, 8192), (3, 2, 2)])
def test_blocks_partition_the_store(C, D, T):
    blocks = HMCDiag.tile_major_blocks(C, D, T)
    assert [b[0] for b in blocks] == list(range(0, C, T))
    end = 0
    for k, (c0, c1, off) in enumerate(blocks):
        assert c1 - c0 == (T if k < len(blocks) - 1 else C - c0) and 0 < c1 - c0 <= T
        assert off == end == D * c0          # blocks are dense and in tile order: nothing between them
        end = off + D * (c1 - c0)
    assert end == D * C and blocks[-1][1] == C
    if T % 2 == 0:
        assert all(off % 2 == 0 for _, _, off in blocks)  # every block starts 16-byte aligned in an aligned store


def _bare(C, D, T):
    s = HMCDiag.__new__(HMCDiag)  # (no device: only what the two properties read)
    s._C, s._dim, s._chain_tile = C, D, T
    return s


@pytest.mark.parametrize("C,D,T", [(130, 33, 64), (131, 5, 64), (10, 3, 4)])
def test_assembled_proposal_and_gradient(C, D, T):
    s = _bare(C, D, T)
    want_t = torch.arange(D * C, dtype=torch.float64).reshape(D, C)
    want_g = -2.0 * want_t
    for name, want in (("_thp_raw", want_t), ("_gp_raw", want_g)):
        store = torch.full((D * C,), float("nan"), dtype=torch.float64)
        for c0, c1, off in HMCDiag.tile_major_blocks(C, D, T):
            store[off:off + D * (c1 - c0)] = want[:, c0:c1].reshape(-1)  # element (d, c) of tile k at off + d*(c1-c0) + (c-c0)
        setattr(s, name, store.view(D, C))
    s._tm_last = True
    assert s._theta_p.shape == (D, C) and s._grad_p.shape == (D, C)
    assert torch.equal(s._theta_p, want_t) and torch.equal(s._grad_p, want_g)
    s._tm_last = False  # a draw of any other schedule leaves plain [D, C] arrays: handed back as they are
    assert s._theta_p is s._thp_raw and s._grad_p is s._gp_raw
    s._theta_p = want_t  # the setter replaces the store (placement tuning assigns through it)
    assert s._thp_raw is want_t
