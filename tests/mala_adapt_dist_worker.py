"""World-size-2 worker for tests/test_mala_adapt_cpu.py (gloo, CPU, the NumPy stand-in): MALA.warmup over sharded chains.
Prints the report as one JSON line."""
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bayes-kit_amd")]

import torch.distributed as dist

import bayes_kit_amd as bk
from tests import mala_adapt_parity as mp
from tests.fake_ops_mala_adapt import MalaAdaptFakeOps


def main():
    rank, local_rank, world = bk.dist.init_from_env(backend="gloo")
    assert world == 2
    first, n = bk.dist.shard(512)
    _, rep, _ = mp.run_warmup(MalaAdaptFakeOps(), 21, C=n, chain_id0=first)
    rep["precond_diag"] = [float(x) for x in rep["precond_diag"]]
    print(json.dumps(rep))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
