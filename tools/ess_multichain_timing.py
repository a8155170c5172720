"""Timing breakdown of the multi-chain ESS (bk.ess_bulk / ess_tail / ess_mean) at [N, C] = [1000, 65536] on one GPU, for
iid normal draws (one lag round) and AR(1) phi = 0.9 draws (every lag): the pooled sort, rank normalisation, the moments
passes, each lag round, the order-statistic selects and the host syncs, beside bk.ess and one bk_sort_by_key of the same
data timed in the same process.  Prints one JSON object (and writes it with --out).

    python tools/ess_multichain_timing.py [--draws 1000] [--chains 65536] [--reps 5] [--out profiles/...json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bayes-kit_amd")]

import numpy as np
import torch

import bayes_kit_amd as bk
from bayes_kit_amd import _lib
from bench_config import FP64_VECTOR_PEAK_TFLOPS


def _ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def _ar1(N, C, phi, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    x = torch.empty((N, C), dtype=torch.float64, device="cuda")
    x[0] = torch.randn(C, dtype=torch.float64, device="cuda", generator=g)
    s = float(np.sqrt(1 - phi * phi))
    for t in range(1, N):
        x[t] = phi * x[t - 1] + s * torch.randn(C, dtype=torch.float64, device="cuda", generator=g)
    return x


class _Timed:
    """Wraps the ops object: per entry point, the device time of every call (events) and the number of calls."""

    def __init__(self, ops):
        self.ops, self.rec = ops, {}

    def __getattr__(self, name):
        fn = getattr(self.ops, name)
        if not callable(fn) or name in ("ess_lag_sums_max_half", "autocorr_fft_work_bytes"):
            return fn

        def call(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*a, **k)
            e1.record()
            label = name
            if name == "ess_lag_sums":
                label = f"ess_lag_sums[{a[3]}:{a[3] + a[4]}]"
            self.rec.setdefault(label, []).append((e0, e1))
            return r

        return call

    def table(self):
        torch.cuda.synchronize()
        return {k: {"calls": len(v), "ms": round(sum(a.elapsed_time(b) for a, b in v), 4)} for k, v in self.rec.items()}


def _breakdown(x, reps):
    ops = _lib.default_ops()
    res = {}
    ess_out = torch.empty(x.shape[1], dtype=torch.float64, device="cuda")
    res["bk.ess_ms"] = _ms(lambda: ops.ess(x, 0, ess_out), reps)
    flat = x.t().contiguous().reshape(-1)
    idx = torch.arange(flat.numel(), dtype=torch.int64, device="cuda")
    res["sort_by_key_ms"] = _ms(lambda: ops.sort_by_key(flat, idx), reps)
    for f in ("ess_mean", "ess_bulk", "ess_tail"):
        res[f + "_ms"] = _ms(lambda f=f: getattr(bk, f)(x), reps)
    res["ess_bulk_plus_tail_ms"] = res["ess_bulk_ms"] + res["ess_tail_ms"]
    # first lag round alone (64 lags), the bar against bk.ess
    n = x.shape[0] // 2
    cm = torch.empty(2 * x.shape[1], dtype=torch.float64, device="cuda")
    g0 = torch.empty_like(cm)
    ops.ess_split_moments(x, None, cm, g0)
    res["first_lag_round_ms"] = _ms(lambda: ops.ess_lag_sums(x, None, cm, 0, min(64, n)), reps)
    # per-stage device times of one ess_bulk + ess_tail, and the host syncs (device-to-host reads)
    timed = _Timed(ops)
    syncs = [0]
    orig_cpu = torch.Tensor.cpu

    def counting_cpu(t, *a, **k):
        syncs[0] += 1
        return orig_cpu(t, *a, **k)

    torch.Tensor.cpu = counting_cpu
    try:
        vals = {"ess_bulk": float(bk.ess_bulk(x, ops=timed)), "ess_tail": float(bk.ess_tail(x, ops=timed))}
    finally:
        torch.Tensor.cpu = orig_cpu
    res["stages_bulk_plus_tail"] = timed.table()
    res["host_reads_bulk_plus_tail"] = syncs[0]
    res["values"] = vals
    res["ratio_first_round_to_bk_ess"] = res["first_lag_round_ms"] / res["bk.ess_ms"]
    res["ratio_bulk_plus_tail_to_sort"] = res["ess_bulk_plus_tail_ms"] / res["sort_by_key_ms"]
    return res


def lag_rate(stages, n, C):
    """Achieved fp64 rate of the lag rounds: a round of lags [l0, l1) costs sum_t (n - t) multiply-adds (2 FLOP) per split
    chain, 2 C chains per call (all lags of all rounds: n^2 / 2 per chain)."""
    flops = ms = 0.0
    for k, v in stages.items():
        if k.startswith("ess_lag_sums["):
            l0, l1 = (int(a) for a in k[len("ess_lag_sums["):-1].split(":"))
            flops += v["calls"] * 2 * C * 2 * sum(n - t for t in range(l0, l1))
            ms += v["ms"]
    tf = flops / (ms * 1e-3) / 1e12 if ms else None
    return {"lag_kernel_tflops": tf, "lag_kernel_fraction_of_fp64_vector_peak": tf / FP64_VECTOR_PEAK_TFLOPS if tf else None}


def cfg3_bulk_ess_per_sec(draws, chains):
    """Config 3 (bench.py's sampler, the headline's model-opaque path) for `draws` draws with the tracked series of bench.py
    --full recorded; bulk ESS of each series over the sampling time (informative: not part of the bench line)."""
    from bench import make_cfg3_sampler

    s = make_cfg3_sampler(chains, 0, torch.device("cuda", torch.cuda.current_device()))
    D = s._theta_dc.shape[0]
    rec = bk.DrawRecorder([0, D // 2, D - 1], draws, chains)
    for _ in range(2):
        s.sample()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(draws):
        th, lp = s.sample()
        rec.record(th, lp)
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    t1 = time.perf_counter()
    sm = rec.summary()
    torch.cuda.synchronize()
    bulk = [float(v) for v in sm["ess_bulk"]]
    return {"draws": draws, "chains": chains, "tracked": sm["name"], "sampling_s": sec, "summary_s": time.perf_counter() - t1,
            "ess_bulk": bulk, "ess_tail": [float(v) for v in sm["ess_tail"]], "rhat": [float(v) for v in sm["rhat"]],
            "bulk_ess_per_sec": [b / sec for b in bulk], "min_bulk_ess_per_sec": min(bulk) / sec}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cfg3-draws", type=int, default=200, help="draws of config 3 for the bulk ESS/sec figure (0 = skip)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    N, C = a.draws, a.chains
    out = {"N": N, "C": C, "device": torch.cuda.get_device_name(0)}
    x = torch.randn((N, C), dtype=torch.float64, device="cuda")
    out["iid"] = _breakdown(x, a.reps)
    del x
    x = _ar1(N, C, 0.9, 7)
    r = _breakdown(x, max(1, a.reps // 2))
    r.update(lag_rate(r["stages_bulk_plus_tail"], N // 2, C))
    out["ar1_phi_0.9"] = r
    del x
    if a.cfg3_draws > 0:
        out["cfg3_tracked_bulk_ess"] = cfg3_bulk_ess_per_sec(a.cfg3_draws, C)
    print(json.dumps(out, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
