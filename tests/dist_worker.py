"""World-size-2 worker for tests/test_dist_cpu.py (gloo, CPU, fake ops): the N>1 path of
chain sharding and of the cross-rank R-hat combine."""
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bayes-kit_amd")]

import numpy as np
import torch
import torch.distributed as dist

import bayes_kit_amd as bk
from tests.fake_ops import FakeOps


def main():
    rank, local_rank, world = bk.dist.init_from_env(backend="gloo")
    assert world == 2 and dist.get_backend() == "gloo"
    ops = FakeOps()
    z = np.load(os.path.join(ROOT, "tests", "golden", "diagnostics.npz"))
    chains = z["rhat_chains"]  # (64 chains, 200 draws)
    M = chains.shape[0]
    first, n = bk.dist.shard(M)
    assert (first, n) == (rank * 32, 32)
    # 1) R-hat of a sharded [N, C] series == the reference's value on all chains
    x = torch.from_numpy(np.ascontiguousarray(chains[first:first + n].T))
    r = bk.rhat(x, ops=ops)
    np.testing.assert_allclose(r, z["rhat"], rtol=1e-12)
    sr = bk.split_rhat(x, ops=ops)
    np.testing.assert_allclose(sr, z["split_rhat"], rtol=1e-12)
    # 2) streaming moments over a sharded many-chain sampler; every rank gets the same R-hat
    C, D = 10, 3
    first, n = bk.dist.shard(C)  # 5 + 5
    s = bk.HMCDiag(bk.IsoGaussian(D, ops=ops), 0.3, 4, chains=n, chain_id0=first, seed=99, ops=ops)
    mom = bk.RunningMoments(D, n, ops=ops)
    draws = []
    for _ in range(30):
        th, _ = s.sample()
        mom.update(th)
        draws.append(th.numpy().copy())
    rh = mom.rhat()
    draws = np.stack(draws)  # (30, n, D)
    gathered = [None, None]
    dist.all_gather_object(gathered, draws)
    full = np.concatenate(gathered, axis=1)  # (30, C, D)
    from oracle import diagnostics as od

    want = np.array([od.rhat([full[:, c, d] for c in range(C)]) for d in range(D)])
    np.testing.assert_allclose(rh, want, rtol=1e-10)
    # 3) sharding invariance: the union of the shards == one process running all chains
    if rank == 0:
        ref = bk.HMCDiag(bk.IsoGaussian(D, ops=ops), 0.3, 4, chains=C, seed=99, ops=ops)
        for i in range(30):
            th, _ = ref.sample()
            assert np.array_equal(th.numpy(), full[i])
    # 4) rank-normalised R-hat across ranks == the reference's value on all chains
    rk = z["rank_chains"]  # (8 chains, 100 draws)
    f4, n4 = bk.dist.shard(rk.shape[0])
    xr = torch.from_numpy(np.ascontiguousarray(rk[f4:f4 + n4].T))
    np.testing.assert_allclose(bk.rank_normalized_rhat(xr, ops=ops), z["rank_normalized_rhat"], rtol=1e-12)
    # 5) tempered SMC with global resampling: the two shards == one process holding all particles
    lp_fn = lambda Th: -0.5 * (Th * Th).sum(dim=1)
    ll_fn = lambda Th: -2.0 * ((Th - 1.0) ** 2).sum(dim=1)
    M_total, Dp = 12, 2
    init = np.random.default_rng(4).normal(size=(M_total, Dp))
    f5, n5 = bk.dist.shard(M_total)
    smc = bk.TemperedLikelihoodSMC(bk.TorchPriorLikelihoodModel(lp_fn, ll_fn, Dp), n5, 5, init[f5:f5 + n5],
                                   bk.metropolis_kernel(0.4), seed=21, slot_id0=f5, ops=ops)
    smc.run()
    parts = [None, None]
    dist.all_gather_object(parts, smc.thetas.numpy().copy())
    # a single-process reference run must not see the 2-rank group: give it a 1-rank subgroup
    # (new_group is collective: every rank creates both groups, in the same order)
    solo_groups = [dist.new_group(ranks=[r]) for r in range(world)]
    solo_group = solo_groups[rank]
    solo = bk.TemperedLikelihoodSMC(bk.TorchPriorLikelihoodModel(lp_fn, ll_fn, Dp), M_total, 5, init,
                                    bk.metropolis_kernel(0.4), seed=21, group=solo_group, ops=ops)
    solo.run()
    assert np.array_equal(np.concatenate(parts, axis=0), solo.thetas.numpy())
    # 6) uneven shards (dist.shard gives the remainder to the first ranks): 7 chains = 4 + 3,
    #    11 particles = 6 + 5; the collectives must not assume equal widths
    f6, n6 = bk.dist.shard(7)
    assert (f6, n6) == ((0, 4) if rank == 0 else (4, 3))
    x7 = torch.from_numpy(np.ascontiguousarray(rk[f6:f6 + n6].T))
    want7 = od.rank_normalized_rhat([rk[c] for c in range(7)])
    np.testing.assert_allclose(bk.rank_normalized_rhat(x7, ops=ops), want7, rtol=1e-12)
    np.testing.assert_allclose(bk.rhat(x7, ops=ops), od.rhat([rk[c] for c in range(7)]), rtol=1e-12)
    M_odd = 11
    init_o = np.random.default_rng(5).normal(size=(M_odd, Dp))
    f7, n7 = bk.dist.shard(M_odd)
    smc_o = bk.TemperedLikelihoodSMC(bk.TorchPriorLikelihoodModel(lp_fn, ll_fn, Dp), n7, 4, init_o[f7:f7 + n7],
                                     bk.metropolis_kernel(0.4), seed=22, slot_id0=f7, ops=ops)
    smc_o.run()
    parts_o = [None, None]
    dist.all_gather_object(parts_o, smc_o.thetas.numpy().copy())
    solo_o = bk.TemperedLikelihoodSMC(bk.TorchPriorLikelihoodModel(lp_fn, ll_fn, Dp), M_odd, 4, init_o,
                                      bk.metropolis_kernel(0.4), seed=22, group=solo_group, ops=ops)
    solo_o.run()
    assert np.array_equal(np.concatenate(parts_o, axis=0), solo_o.thetas.numpy())
    # 6b) the ADAPTIVE ladder across ranks: the next temperature is found on the log likelihoods of ALL ranks'
    #     particles (gathered), the HMC move's metric from the particles of all ranks -- same ladder, same particles
    ll_big = lambda Th: -400.0 * ((Th - 0.3) ** 2).sum(dim=1)
    mk = lambda m, init_, **kw: bk.TemperedLikelihoodSMC(bk.TorchPriorLikelihoodModel(lp_fn, ll_big, Dp), m, 3, init_,  # noqa: E731
                                                         bk.hmc_kernel(0.6, 2, adapt_metric=True), seed=23, ops=ops,
                                                         adaptive=0.6, **kw)
    M_ad = 41
    init_a = np.random.default_rng(6).normal(size=(M_ad, Dp))
    f8, n8 = bk.dist.shard(M_ad)
    smc_a = mk(n8, init_a[f8:f8 + n8], slot_id0=f8)
    smc_a.run()
    parts_a = [None, None]
    dist.all_gather_object(parts_a, (smc_a.thetas.numpy().copy(), list(smc_a.temperatures), list(smc_a.ess_history)))
    solo_a = mk(M_ad, init_a, group=solo_group)
    solo_a.run()
    assert parts_a[0][1] == parts_a[1][1] and len(solo_a.temperatures) > 3   # (the ranks agree exactly; one process sums
    np.testing.assert_allclose(parts_a[0][1], solo_a.temperatures, rtol=1e-9)  #  the particle moments in another order)
    np.testing.assert_allclose(parts_a[0][2], solo_a.ess_history, rtol=1e-9)
    np.testing.assert_allclose(np.concatenate([parts_a[0][0], parts_a[1][0]], axis=0), solo_a.thetas.numpy(), rtol=1e-9, atol=1e-12)
    # 7) the sample sort behind the cross-rank rank normalisation: global ranks of a sharded series ==
    #    ranks of the pooled series in one process, including ties (resolved by pooled order) and a
    #    heavily skewed split of the value range between the ranks
    from bayes_kit_amd import diagnostics as dg

    rs = np.random.default_rng(11)
    neg_nan = np.copysign(np.nan, -1.0)

    def with_specials(x):  # NaNs of both signs, both infinities and both zeros over a fifth of the draws
        spots = rs.permutation(x.size)[:x.size // 5]
        x.reshape(-1)[spots] = np.array([np.nan, neg_nan, np.inf, -np.inf, 0.0, -0.0])[rs.integers(0, 6, size=len(spots))]
        return x

    def split_range(sign):  # every draw of rank 0 (chains 0, 1) below (sign = 1) or above every draw of rank 1
        x = rs.normal(size=(25, 4))
        x[:, :2] -= sign * 100.0
        x[:, 2:] += sign * 100.0
        return x

    for C_tot, N_t, make in ((7, 50, lambda: rs.integers(0, 9, size=(50, 7)).astype(np.float64)),
                             (6, 40, lambda: np.sort(rs.normal(size=(40 * 6))).reshape(6, 40).T.copy()),
                             (9, 31, lambda: rs.normal(size=(31, 9))),
                             # every value equal: every splitter repeats, one bucket is empty
                             (4, 20, lambda: np.full((20, 4), 2.5)),
                             (5, 30, lambda: rs.integers(0, 2, size=(30, 5)).astype(np.float64)),   # two distinct values
                             (6, 40, lambda: with_specials(rs.normal(size=(40, 6)))),
                             (6, 200, lambda: with_specials(np.round(rs.normal(size=(200, 6)), 1))),  # ... more draws than samples
                             (4, 10, lambda: np.where(rs.integers(0, 2, size=(10, 4)) == 0, np.nan, neg_nan)),  # every draw NaN
                             (2, 3, lambda: rs.normal(size=(3, 2))),        # a shard smaller than its 128 samples
                             (1, 5, lambda: rs.normal(size=(5, 1))),        # rank 1 holds an [N, 0] shard
                             (4, 25, lambda: split_range(1.0)),
                             (4, 25, lambda: split_range(-1.0))):
        full_np = make()
        shared = [full_np if rank == 0 else None]
        dist.broadcast_object_list(shared, src=0)
        full_np = shared[0]
        f8, n8 = bk.dist.shard(C_tot)
        mine = torch.from_numpy(np.ascontiguousarray(full_np[:, f8:f8 + n8]))
        assert full_np.shape == (N_t, C_tot) and mine.shape == (N_t, n8)
        got = dg._ranks_pooled_across_ranks(mine, ops)
        want = dg.rank_chains(torch.from_numpy(full_np), ops=ops)[:, f8:f8 + n8]
        assert got.shape == want.shape and torch.equal(got, want), (C_tot, N_t)
        # ... and rank_chains of the pooled series is NumPy's stable ranking (rhat.py:51-52), on this input too
        flat_np = full_np.T.reshape(-1)
        assert np.array_equal(want.numpy(), (flat_np.argsort(kind="stable").argsort() + 1).reshape(C_tot, N_t).T[:, f8:f8 + n8])
    total = bk.dist.sum_over_ranks(float(n))
    assert total == C
    dist.barrier()
    dist.destroy_process_group()
    print("rank", rank, "ok")


if __name__ == "__main__":
    main()
