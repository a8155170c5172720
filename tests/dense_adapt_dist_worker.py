"""World-size-2 worker for tests/test_dense_adapt_cpu.py (gloo, CPU, the NumPy stand-in):
HMCDiag.warmup(adapt_metric="dense") over 2 x 256 sharded chains.  Prints the report as one JSON line."""
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bayes-kit_amd")]

import torch.distributed as dist

import bayes_kit_amd as bk
from tests import dense_adapt_parity as dp
from tests.fake_ops_dense_adapt import DenseAdaptFakeOps


def main():
    rank, local_rank, world = bk.dist.init_from_env(backend="gloo")
    assert world == 2
    ops = DenseAdaptFakeOps()
    first, n = bk.dist.shard(dp.CHAINS)
    s = dp.make_sampler(ops, int(os.environ["BK_TEST_SEED"]), C=n, chain_id0=first)
    rep = dp.warmup_recording(s, 300)
    rep["metric_dense"] = rep["metric_dense"].tolist()
    rep["installed"] = [m.tolist() for m in rep["installed"]]
    print(json.dumps(rep))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
