"""World-size-2 worker for tests/test_energy_cpu.py (gloo, CPU, the NumPy stand-in): the funnel run of tests/energy_parity.py
as two shards of 128 chains, each with its own tracker, against one process with all 256 chains -- divergence counts equal,
the pooled E-BFMI to rel 1e-12, the captured chain ids global."""
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bayes-kit_amd")]

import numpy as np
import torch
import torch.distributed as dist

import bayes_kit_amd as bk
from tests import energy_parity as ep
from tests.fake_ops_energy import EnergyFakeOps


def main():
    rank, _, world = bk.dist.init_from_env(backend="gloo")
    assert world == 2 and dist.get_backend() == "gloo"
    ops = EnergyFakeOps()
    solo = [dist.new_group(ranks=[r]) for r in range(world)][rank]  # (a single-process run must not see the 2-rank group)
    first, n = 128 * rank, 128
    mine = ep.funnel_sampler(bk, ops, ops, chains=n, chain_id0=first, path="opaque")
    full = ep.funnel_sampler(bk, ops, ops, chains=256, path="opaque")
    em, ef = mine.track_energy(), full.track_energy()
    for _ in range(40):
        (tm, _), (tf, _) = mine.sample(), full.sample()
        assert torch.equal(tm, tf[first:first + n])
    before = dict(bk.dist.collective_calls)
    got = (em.divergences(), em.nan_transitions(), em.nonfinite_energies())
    assert bk.dist.collective_calls["all_gather"] - before["all_gather"] == 3
    want = (ef.divergences(group=solo), ef.nan_transitions(group=solo), ef.nonfinite_energies(group=solo))
    assert got == want and got[0] > 0, (got, want)
    assert em.divergence_rate() == ef.divergence_rate(group=solo)
    np.testing.assert_allclose(em.ebfmi_pooled(), ef.ebfmi_pooled(group=solo), rtol=1e-12)
    assert em.ebfmi_pooled(group=solo) != ef.ebfmi_pooled(group=solo)          # (128 chains are not 256)
    # the captured chain ids are global: this rank's entries are the full run's entries of its chains, in the same order
    dm, df = em.divergent_states(), ef.divergent_states()
    assert df["stored"] == df["seen"] == got[0]
    sel = (df["chain"] >= first) & (df["chain"] < first + n)
    assert dm["stored"] == int(sel.sum()) == em.divergences(group=solo)
    for k in ("chain", "draw", "energy_error", "theta"):
        assert np.array_equal(dm[k].numpy(), df[k][sel].numpy(), equal_nan=True), k
    dist.barrier()
    dist.destroy_process_group()
    print("rank", rank, "ok")


if __name__ == "__main__":
    main()
