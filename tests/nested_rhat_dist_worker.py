"""World-size-2 worker for tests/test_nested_rhat_dist_cpu.py (gloo, CPU, the NumPy stand-in): nested R-hat over superchains
sharded across ranks."""
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bayes-kit_amd")]

import numpy as np
import torch
import torch.distributed as dist

import bayes_kit_amd as bk
from tests.fake_ops_nested import NestedFakeOps


def main():
    rank, _, world = bk.dist.init_from_env(backend="gloo")
    assert world == 2 and dist.get_backend() == "gloo"
    ops = NestedFakeOps()
    solo = [dist.new_group(ranks=[r]) for r in range(world)][rank]  # (a single-process run must not see the 2-rank group)
    K, M, N, D = 8, 4, 6, 3
    C = K * M
    x = np.random.default_rng(3).normal(size=(N, D, C)) + np.repeat(0.5 * np.arange(K), M)[None, None, :]
    first, n = bk.dist.shard(C)  # 4 superchains of 4 chains on each rank
    assert (first, n) == (rank * 16, 16)
    mine = torch.from_numpy(np.ascontiguousarray(x[:, :, first:first + n]))
    full = torch.from_numpy(x)
    # 1) one [N, C_local] tensor per rank == one process holding all chains; exactly two all_gathers
    want = float(bk.nested_rhat(full[:, 0, :].contiguous(), M, ops=ops, group=solo))
    before = dict(bk.dist.collective_calls)
    got = float(bk.nested_rhat(mine[:, 0, :].contiguous(), M, ops=ops))
    spent = {k: bk.dist.collective_calls[k] - before[k] for k in before}
    assert spent == {"all_gather": 2, "all_reduce": 0, "all_to_all": 0}, spent
    np.testing.assert_allclose(got, want, rtol=1e-12)
    # 2) streaming moments and a recorder, every coordinate at once: the same cost, the same values
    rm, rm_all = bk.RunningMoments(D, n, ops=ops), bk.RunningMoments(D, C, ops=ops)
    rec = bk.DrawRecorder([0, 1, 2], N, n, with_logp=False, ops=ops)
    for t in range(N):
        rm.update(mine[t], layout="dc")
        rm_all.update(full[t], layout="dc")
        rec.record(mine[t], layout="dc")
        if t == 0:  # from the first draw on, across ranks too
            np.testing.assert_allclose(rm.nested_rhat(M), rm_all.nested_rhat(M, group=solo), rtol=1e-12)
    before = dict(bk.dist.collective_calls)
    got_rm = rm.nested_rhat(M)
    assert bk.dist.collective_calls["all_gather"] - before["all_gather"] == 2
    np.testing.assert_allclose(got_rm, rm_all.nested_rhat(M, group=solo), rtol=1e-12)
    before = dict(bk.dist.collective_calls)
    got_rec = rec.nested_rhat(M)
    assert bk.dist.collective_calls["all_gather"] - before["all_gather"] == 2
    np.testing.assert_allclose(got_rec, got_rm, rtol=1e-10)
    assert got_rec[0] == got  # (the tensor and the recorder go through bk_chain_mean_var alike)
    # 3) a superchain that straddles the ranks: rank 1 holds 14 chains, no multiple of 4 -- EVERY rank raises
    width = 16 if rank == 0 else 14
    try:
        bk.nested_rhat(mine[:, 0, :width].contiguous(), M, ops=ops)
    except ValueError as e:
        assert "multiple of chains_per_superchain" in str(e) and "every rank" in str(e), e
    else:
        raise AssertionError(f"rank {rank} did not raise")
    # 4) one superchain per rank is enough: K counts all ranks (and K = 1 in all raises everywhere)
    assert np.isfinite(bk.nested_rhat(mine[:, 0, :4].contiguous(), M, ops=ops))
    try:
        bk.nested_rhat(mine[:, 0, :4 if rank == 0 else 0].contiguous(), M, ops=ops)
    except ValueError as e:
        assert "superchains" in str(e), e
    else:
        raise AssertionError(f"rank {rank} did not raise for one superchain in all")
    dist.barrier()
    dist.destroy_process_group()
    print("rank", rank, "ok")


if __name__ == "__main__":
    main()
