"""World-size-2 worker for tests/test_ess_multichain_cpu.py (gloo, CPU, fake ops): multi-chain ESS over uneven shards
equals the one-process value; ranks with different numbers of draws raise on both ranks."""
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bayes-kit_amd")]

import numpy as np
import pytest
import torch
import torch.distributed as dist

import bayes_kit_amd as bk
from tests import multichain_ess_ref as ref


def main():
    rank, _, world = bk.dist.init_from_env(backend="gloo")
    assert world == 2
    ops = ref.MultiEssFakeOps()
    if sys.argv[1] == "values":
        for N in (60, 61):
            x = ref.ar1(np.random.default_rng(N), N, 9, 0.7)
            lo, hi = (0, 4) if rank == 0 else (4, 9)  # uneven shards
            mine = torch.from_numpy(np.ascontiguousarray(x[:, lo:hi]))
            for f in ("ess_bulk", "ess_tail", "ess_mean", "mcse_mean"):
                got = getattr(bk, f)(mine, ops=ops)
                assert got == pytest.approx(getattr(ref, f)(x), rel=1e-12), (f, N)
            assert bk.ess_quantile(mine, 0.2, ops=ops) == pytest.approx(ref.ess_quantile(x, 0.2), rel=1e-12)
    else:
        N = 40 if rank == 0 else 41
        x = torch.from_numpy(np.random.default_rng(rank).standard_normal((N, 3)))
        with pytest.raises(ValueError, match=r"\[40, 41\]"):
            bk.ess_bulk(x, ops=ops)
        dist.barrier()
    print(f"rank {rank} ok", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
