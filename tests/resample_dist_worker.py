"""World-size-2 worker for tests/test_resample_schemes.py (gloo, CPU, stand-in ops): tempered SMC with systematic and
stratified resampling over the particles of both ranks == one process holding all particles, bit for bit."""
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bayes-kit_amd")]

import numpy as np
import torch.distributed as dist

import bayes_kit_amd as bk
from tests.fake_ops_resample import ResampleFakeOps


def main():
    rank, local_rank, world = bk.dist.init_from_env(backend="gloo")
    assert world == 2 and dist.get_backend() == "gloo"
    ops = ResampleFakeOps()
    lp_fn = lambda Th: -0.5 * (Th * Th).sum(dim=1)           # noqa: E731
    ll_fn = lambda Th: -2.0 * ((Th - 1.0) ** 2).sum(dim=1)   # noqa: E731
    M_total, Dp, N = 13, 2, 4                                 # an odd total: 7 + 6
    init = np.random.default_rng(8).normal(size=(M_total, Dp))
    first, n = bk.dist.shard(M_total)
    assert n == (7, 6)[rank]
    # a single-process reference run must not see the 2-rank group: give it a 1-rank subgroup (new_group is collective)
    solo_group = [dist.new_group(ranks=[r]) for r in range(world)][rank]
    for scheme in ("systematic", "stratified"):
        mk = lambda m, init_, **kw: bk.TemperedLikelihoodSMC(bk.TorchPriorLikelihoodModel(lp_fn, ll_fn, Dp), m, N, init_,  # noqa: E731
                                                             bk.metropolis_kernel(0.4), seed=31, ops=ops, resampling=scheme, **kw)
        smc = mk(n, init[first:first + n], slot_id0=first)
        solo = mk(M_total, init, group=solo_group)
        for k in range(1, N + 1):
            smc.transition(k)
            solo.transition(k)
            parts = [None, None]
            dist.all_gather_object(parts, (smc.thetas.numpy().copy(), smc._idx.numpy().copy(), smc.last_ess))
            assert np.array_equal(np.concatenate([p[1] for p in parts]), solo._idx.numpy()), (scheme, k)
            assert np.array_equal(np.concatenate([p[0] for p in parts], axis=0), solo.thetas.numpy()), (scheme, k)
            assert np.all(np.diff(solo._idx.numpy()) >= 0), (scheme, k)
        assert ops.calls["resample_ordered"] == 2 * N * (1 + ("systematic", "stratified").index(scheme))
    dist.barrier()
    dist.destroy_process_group()
    print("rank", rank, "ok")


if __name__ == "__main__":
    main()
