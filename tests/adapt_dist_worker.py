"""World-size-2 worker for tests/test_adapt_cpu.py (gloo, CPU, the NumPy stand-in): HMCDiag.warmup over sharded chains.
Prints the report as one JSON line."""
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bayes-kit_amd")]

import numpy as np
import torch.distributed as dist

import bayes_kit_amd as bk
from tests.fake_ops_adapt import AdaptFakeOps


def main():
    rank, local_rank, world = bk.dist.init_from_env(backend="gloo")
    assert world == 2
    ops = AdaptFakeOps()
    lam = np.logspace(0, 4, 32)
    first, n = bk.dist.shard(512)
    s = bk.HMCDiag(bk.DiagGaussian(lam, ops=ops), 0.006, 16, chains=n, chain_id0=first, seed=21, ops=ops)
    rep = s.warmup(300)
    rep["precond_diag"] = [float(x) for x in rep["precond_diag"]]
    print(json.dumps(rep))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
