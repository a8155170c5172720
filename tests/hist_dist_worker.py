"""World-size-2 worker for tests/test_hist_dist_cpu.py (gloo, CPU, the NumPy stand-in): RunningHistogram over chains split
2,051 / 2,048 across ranks equals the single-process result on the concatenation exactly, at one all_gather per read."""
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bayes-kit_amd")]

import numpy as np
import torch
import torch.distributed as dist

import bayes_kit_amd as bk
from tests import hist_parity as hp
from tests.fake_ops_hist import HistFakeOps, counts_ref


def _gathers(fn):
    before = dict(bk.dist.collective_calls)
    out = fn()
    spent = {k: bk.dist.collective_calls[k] - before[k] for k in before}
    return out, spent


def main():
    rank, _, world = bk.dist.init_from_env(backend="gloo")
    assert world == 2 and dist.get_backend() == "gloo"
    ops = HistFakeOps()
    solo = [dist.new_group(ranks=[r]) for r in range(world)][rank]  # (a single-process run must not see the 2-rank group)
    D, B, C = 5, 37, 2051 + 2048
    first, n = (0, 2051) if rank == 0 else (2051, 2048)   # (not dist.shard's even split: the ranks' slab seams differ)
    lo, hi, scale = hp.grid("nondyadic", D, B)
    draws = [hp.data("nondyadic", D, C, B)] + [hp.finite_data(D, C, seed) for seed in (1, 2)]
    one = {"all_gather": 1, "all_reduce": 0, "all_to_all": 0}
    # 1) counts and quantiles
    mine, full = bk.RunningHistogram(lo, hi, bins=B, ops=ops), bk.RunningHistogram(lo, hi, bins=B, ops=ops)
    for x in draws:
        mine.update(torch.from_numpy(np.array(x[:, first:first + n])), layout="dc")
        full.update(torch.from_numpy(np.array(x)), layout="dc")
    assert mine.n == 3 * n and full.n == 3 * C
    got, spent = _gathers(lambda: mine.counts())
    assert spent == one, spent
    want = full.counts(group=solo)
    assert got.dtype == torch.int64 and torch.equal(got, want)
    assert np.array_equal(want.numpy(), counts_ref(np.concatenate(draws, axis=1), lo, scale, B))
    assert not torch.equal(mine.counts(group=solo), want)       # (a rank's own counts are a part only)
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)        # (the special values put the extreme quantiles off the grid)
        q, spent = _gathers(lambda: mine.quantile(hp.PROBS))
        assert spent == one, spent
        assert np.array_equal(q, full.quantile(hp.PROBS, group=solo), equal_nan=True)
        assert np.array_equal(mine.median(), full.median(group=solo))
        for a, b in zip(mine.interval(0.9), full.interval(0.9, group=solo)):
            assert np.array_equal(a, b)
    cov, spent = _gathers(lambda: mine.coverage())
    assert spent == one and np.array_equal(cov, full.coverage(group=solo))
    # 2) the grid from moments over both ranks' chains.  Two draws of integer values whose chain means cancel in pairs: every
    #    per-chain moment is a multiple of 1/4, the cross-chain centre is exactly 0 and every sum is exact in any order, so the
    #    two-rank grid must be the single-process grid bit for bit
    g = np.random.default_rng(5)
    half = g.integers(1, 16, size=(2, D, C // 2)).astype(np.float64) * g.choice([-1.0, 1.0], size=(2, D, C // 2))
    ints = np.concatenate([half, -half, np.stack([np.full((D, 1), 3.0), np.full((D, 1), -3.0)])], axis=2)[:, :, g.permutation(C)]
    rm, rm_all = bk.RunningMoments(D, n, ops=ops), bk.RunningMoments(D, C, ops=ops)
    for x in ints:
        rm.update(torch.from_numpy(np.array(x[:, first:first + n])), layout="dc")
        rm_all.update(torch.from_numpy(np.array(x)), layout="dc")
    (h, spent), h_all = _gathers(lambda: bk.RunningHistogram.from_moments(rm)), bk.RunningHistogram.from_moments(rm_all, group=solo)
    assert spent == {"all_gather": 3, "all_reduce": 0, "all_to_all": 0}, spent   # the mean: one; the variance: two passes
    assert np.array_equal(h._lo_h, h_all._lo_h) and np.array_equal(h._hi_h, h_all._hi_h) and np.array_equal(h._scale_h, h_all._scale_h)
    assert np.array_equal(0.5 * (h._lo_h + h._hi_h), np.zeros(D)) and (h._hi_h > 8.0).all()
    #    ... and on real-valued draws, where the sums over chains take another order, to rounding; every rank holds ONE grid
    rm, rm_all = bk.RunningMoments(D, n, ops=ops), bk.RunningMoments(D, C, ops=ops)
    for x in draws[1:] + [hp.finite_data(D, C, 3)]:
        rm.update(torch.from_numpy(np.array(x[:, first:first + n])), layout="dc")
        rm_all.update(torch.from_numpy(np.array(x)), layout="dc")
    h = bk.RunningHistogram.from_moments(rm, bins=64, width=6.0)
    h_all = bk.RunningHistogram.from_moments(rm_all, bins=64, width=6.0, group=solo)
    # (sums over chains in another order: the grids agree to rounding, and every rank holds the SAME grid)
    np.testing.assert_allclose(h._lo_h, h_all._lo_h, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(h._hi_h, h_all._hi_h, rtol=1e-12, atol=1e-13)
    grids = bk.dist.all_gather(torch.from_numpy(np.concatenate([h._lo_h, h._hi_h, h._scale_h])))
    assert torch.equal(grids[0], grids[1])
    dist.barrier()
    dist.destroy_process_group()
    print("rank", rank, "ok")


if __name__ == "__main__":
    main()
