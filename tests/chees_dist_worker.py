"""World-size-2 worker for tests/test_chees_cpu.py (gloo, CPU, the NumPy stand-in): HMCDiag.warmup(adapt_trajectory=True)
over sharded chains.  Prints the report as one JSON line."""
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bayes-kit_amd")]

import torch.distributed as dist

import bayes_kit_amd as bk
from tests.fake_ops_chees import CheesFakeOps


def main():
    rank, local_rank, world = bk.dist.init_from_env(backend="gloo")
    assert world == 2
    ops = CheesFakeOps()
    first, n = bk.dist.shard(512)
    s = bk.HMCDiag(bk.IsoGaussian(32, ops=ops), 0.006, 16, chains=n, chain_id0=first, seed=21, ops=ops)
    rep = s.warmup(300, adapt_metric=False, adapt_trajectory=True)
    rep["precond_diag"] = None
    print(json.dumps(rep))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
