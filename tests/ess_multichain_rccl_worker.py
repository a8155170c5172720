"""A ONE-rank `nccl` (= RCCL) process group on the GPU with the collectives forced through it (bayes_kit_amd.dist
.force_collectives): the cross-rank path of the multi-chain ESS -- the shape check's all_gather, the sample sort's
all_to_all_singles, the order statistics selected by global rank (bk_select_ranks) and every gathered partial sum, on
device tensors -- must give the no-group answers.  Started as a child process by tests/test_gpu_ess_multichain.py."""
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bayes-kit_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import bayes_kit_amd as bk  # noqa: E402


def values(x, rec):
    out = {f: float(getattr(bk, f)(x)) for f in ("ess_bulk", "ess_tail", "ess_mean", "mcse_mean")}
    out["ess_quantile"] = float(bk.ess_quantile(x, 0.3))
    s = rec.summary()
    for k in ("mean", "sd", "mcse_mean", "ess_bulk", "ess_tail", "rhat"):
        out["summary_" + k] = [float(v) for v in s[k]]
    return out


def main():
    import faulthandler

    faulthandler.dump_traceback_later(float(os.environ.get("BK_TEST_WATCHDOG", "240")), exit=True)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    assert dist.get_backend() == "nccl" and dist.get_world_size() == 1
    g = torch.Generator().manual_seed(3)
    results = {}
    for N in (300, 301):
        x = torch.randn((N, 70), dtype=torch.float64, generator=g)
        x[:, 5] += 0.5
        x[::7, 9] = torch.round(x[::7, 9])  # some ties
        x = x.to(dev)
        rec = bk.DrawRecorder([0], N, 70, with_logp=False)
        rec.series[0].copy_(x)
        rec.n = N
        bk.dist.force_collectives = False
        want = values(x, rec)
        calls0 = dict(bk.dist.collective_calls)
        bk.dist.force_collectives = True
        got = values(x, rec)
        bk.dist.force_collectives = False
        calls = {k: bk.dist.collective_calls[k] - calls0[k] for k in calls0}
        assert calls["all_gather"] > 0 and calls["all_to_all"] > 0, calls
        for k in want:
            np.testing.assert_allclose(got[k], want[k], rtol=1e-12, err_msg=f"{k} N={N}")
        results[N] = calls
    dist.barrier()
    dist.destroy_process_group()
    print(json.dumps({"ok": True, "collectives": results}), flush=True)


if __name__ == "__main__":
    main()
