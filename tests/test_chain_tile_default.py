"""The default chain tile of HMCDiag's step-by-step loop (HMCDiag.default_chain_tile / _pick_tile): host logic only."""
import numpy as np

import bayes_kit_amd as bk
from tests.fake_ops import FakeOps

pick = bk.HMCDiag.default_chain_tile


def test_default_tile_is_the_largest_even_tile_whose_three_arrays_fit():
    assert pick(65536, 1024) == 8192            # 3 x 64 MiB = 192 MiB: the library's own threshold, met exactly
    assert 3 * 8 * 8192 * 1024 == bk.HMCDiag.LLC_BYTES
    assert pick(8192, 1024) == 8192             # the three arrays fit: no tiling
    assert pick(65536, 128) == 65536            # ... here too (3 x 64 MiB)
    assert pick(8194, 1024) == 8194 and pick(12288, 1024) == 12288   # fewer than two full tiles: untiled (12,288 measured)
    assert pick(16382, 1024) == 16382 and pick(16384, 1024) == 8192 and pick(16386, 1024) == 8192
    t = pick(65536, 1000)                       # a tile that does not divide C: even, fits, and the next even one does not
    assert t % 2 == 0 and 3 * 8 * t * 1000 <= bk.HMCDiag.LLC_BYTES < 3 * 8 * (t + 2) * 1000
    assert 65536 % t != 0


def test_odd_chain_count_gets_an_even_tile_and_a_ragged_last_tile():
    C = 65537
    t = pick(C, 1024)
    assert t == 8192 and t % 2 == 0
    tiles = [(c0, min(C, c0 + t)) for c0 in range(0, C, t)]
    assert tiles[-1] == (65536, 65537) and all(b - a == t for a, b in tiles[:-1])


def test_no_tile_below_the_minimum_tile_size():
    D = 3 * 1024
    t = bk.HMCDiag.LLC_BYTES // (3 * 8 * D)
    assert t < bk.HMCDiag.MIN_TILE and pick(65536, D) == 65536
    d_min = bk.HMCDiag.LLC_BYTES // (3 * 8 * bk.HMCDiag.MIN_TILE)   # the largest D that still tiles
    assert pick(1 << 20, d_min) == bk.HMCDiag.MIN_TILE and pick(1 << 20, d_min + 1) == 1 << 20


def test_explicit_chain_tile_wins_and_nonpositive_means_untiled():
    ops = FakeOps()
    lam = np.logspace(0, 1, 6)

    def make(**kw):
        return bk.HMCDiag(bk.DiagGaussian(lam, ops=ops), 0.05, 3, chains=11, seed=5, path="opaque", ops=ops, **kw)

    assert make()._chain_tile == 11                  # small: the default does not tile
    assert make(chain_tile=4)._chain_tile == 4
    assert make(chain_tile=5)._chain_tile == 4       # (made even)
    assert make(chain_tile=0)._chain_tile == 11 and make(chain_tile=-3)._chain_tile == 11
    assert make(chain_tile=64)._chain_tile == 11
    assert make(tuning={"chain_tile": 6})._chain_tile == 6


def test_default_tiles_only_the_loop_with_a_separate_gradient_op(monkeypatch):
    """With the threshold lowered to this test's sizes: path="opaque" tiles by default, the whole-draw and one-launch-per-step
    paths do not, and the tiled default gives the untiled draws bit for bit."""
    ops = FakeOps()
    lam = np.logspace(0, 1, 6)
    monkeypatch.setattr(bk.HMCDiag, "LLC_BYTES", 3 * 8 * 6 * 4)   # three arrays of 4 chains x 6 dimensions
    monkeypatch.setattr(bk.HMCDiag, "MIN_TILE", 2)

    def make(path, **kw):
        return bk.HMCDiag(bk.DiagGaussian(lam, ops=ops), 0.05, 3, chains=11, seed=5, path=path, ops=ops, **kw)

    a, b = make("opaque"), make("opaque", chain_tile=0)
    assert a._chain_tile == 4 and b._chain_tile == 11
    assert make("step")._chain_tile == 11 and make("auto")._chain_tile == 11
    for _ in range(3):
        ta, la = a.sample()
        tb, lb = b.sample()
        assert np.array_equal(ta.numpy(), tb.numpy()) and np.array_equal(la.numpy(), lb.numpy())
