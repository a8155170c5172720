#!/usr/bin/env python3
"""The dense-metric adaptation on one GPU (profiles/dense_adapt.md).

    python tools/dense_adapt_timing.py [--small] [--kernels-only] [--no-warmup] [--out FILE.json]

  kernels   bk_cov_accumulate beside bk_dense_metric_apply at the same (D, C): 512 x 2,048 chains (config 5's shape) and
            1,024 x 16,384, launch blocks between device events, the two alternated over the repeats; a second, interleaved
            series of the SAME cov launch gives the A/A spread.  Useful flops: D^2 C (1 + 128 / D) for the lower tile
            blocks of the scatter matrix, 2 D^2 C for the GEMM.  The bar: one covariance update takes no longer than one
            metric application.
  warmup    logistic regression, D = 64, N = 20,000, 2,048 chains: warmup(300, adapt_metric="dense") on a metric_dense = I
            sampler against the diagonal warmup on a plain one -- warmup wall time, final eps, ms per draw, bulk ESS per
            second of the worst coordinate over 200 draws.
--small rehearses the script at toy sizes (its numbers are overheads); --kernels-only runs a few launches of the kernels and
nothing else (the program of a `rocprofv3 --kernel-trace` or a counters-only `--pmc` pass)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bayes-kit_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bayes_kit_amd as bk  # noqa: E402


def events_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "repeats": [round(x, 5) for x in xs]}


def cov_flops(D, C):
    return D * D * C * (1.0 + 128.0 / D)


def gemm_flops(D, C):
    return 2.0 * D * D * C


def time_kernels(ops, shapes, reps, repeats):
    out = {}
    for D, C in shapes:
        dev = ops.device
        g = torch.Generator(device=dev)
        g.manual_seed(D + C)
        X = torch.randn((D, C), dtype=torch.float64, device=dev, generator=g)
        Y = torch.empty_like(X)
        M = torch.randn((D, D), dtype=torch.float64, device=dev, generator=g)
        S = torch.zeros((D, D), dtype=torch.float64, device=dev)
        s = torch.zeros(D, dtype=torch.float64, device=dev)
        c = X.mean(dim=1).contiguous()
        work = ops.cov_work(D, C)
        cov = lambda: ops.cov_accumulate(X, c, S, s, work)  # noqa: E731
        gemm = lambda: ops.dense_metric_apply(M, X, Y)      # noqa: E731
        for f in (cov, gemm):
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        ms = {"cov": [], "cov_again": [], "gemm": []}
        for _ in range(repeats):  # alternated
            ms["cov"].append(events_ms(cov, reps))
            ms["gemm"].append(events_ms(gemm, reps))
            ms["cov_again"].append(events_ms(cov, reps))
        r = {k: spread(v) for k, v in ms.items()}
        r["cov_tflops_useful"] = cov_flops(D, C) / (r["cov"]["median"] * 1e-3) / 1e12
        r["gemm_tflops"] = gemm_flops(D, C) / (r["gemm"]["median"] * 1e-3) / 1e12
        r["cov_over_gemm_time"] = r["cov"]["median"] / r["gemm"]["median"]
        r["aa_spread"] = abs(r["cov"]["median"] - r["cov_again"]["median"]) / r["cov"]["median"]
        r["k_chunk"] = ops.cov_k_chunk(D)
        r["work_MB"] = work.numel() * 8 / 1e6
        out[f"{D}x{C}"] = r
        print(f"{D} x {C}: cov {r['cov']['median']:.4f} ms ({r['cov_tflops_useful']:.1f} TFLOP/s useful)  gemm "
              f"{r['gemm']['median']:.4f} ms ({r['gemm_tflops']:.1f} TFLOP/s)  cov/gemm {r['cov_over_gemm_time']:.3f}  "
              f"A/A {100 * r['aa_spread']:.2f} %", flush=True)
    return out


def logistic_problem(N, D, dev, seed=7):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    X = torch.randn((N, D), dtype=torch.float64, device=dev, generator=g) / D ** 0.5
    beta = torch.randn(D, dtype=torch.float64, device=dev, generator=g)
    y = (torch.rand(N, dtype=torch.float64, device=dev, generator=g) < torch.sigmoid(X @ beta)).to(torch.float64)
    return X, y


def time_warmup(ops, N, D, C, warm, draws):
    dev = ops.device
    X, y = logistic_problem(N, D, dev)
    out = {}
    for name in ("diag", "dense"):
        model = bk.LogisticRegression(X, y, prior_scale=1.0)
        kw = dict(metric_dense=np.eye(D)) if name == "dense" else {}
        s = bk.HMCDiag(model, 0.01, 8, chains=C, seed=5, **kw)
        s.sample()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rep = s.warmup(warm, adapt_metric="dense" if name == "dense" else True)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        for _ in range(3):
            s.sample()
        torch.cuda.synchronize()
        keep = torch.empty((draws, D, C), dtype=torch.float64, device=dev)
        t0 = time.perf_counter()
        for n in range(draws):
            th, _ = s.sample()
            keep[n].copy_(th.t())
        torch.cuda.synchronize()
        per_draw = (time.perf_counter() - t0) / draws
        ess = [float(bk.ess_bulk(keep[:, d, :].contiguous())) for d in range(D)]
        out[name] = {"warmup_s": wall, "eps": rep["stepsize"], "mean_alpha_last20": float(np.mean(rep["alpha"][-20:])),
                     "ms_per_draw": 1e3 * per_draw, "accept_rate": s.accept_rate(), "min_bulk_ess": min(ess),
                     "min_bulk_ess_per_s": min(ess) / (per_draw * draws)}
        print(name, json.dumps(out[name]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--no-warmup", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dense_adapt_timing.py measures on a GPU; none is visible")
    ops = bk._lib.default_ops()
    shapes = [(128, 256), (130, 300)] if a.small else [(512, 2048), (1024, 16384)]
    res = {"device": torch.cuda.get_device_name(0)}
    if a.kernels_only:
        res["kernels"] = time_kernels(ops, shapes, 3, 1)
    else:
        res["kernels"] = time_kernels(ops, shapes, 4 if a.small else 50, 3 if a.small else 9)
        if not a.no_warmup:
            res["warmup"] = time_warmup(ops, *((500, 8, 128, 30, 20) if a.small else (20_000, 64, 2048, 300, 200)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "kernels"}))


if __name__ == "__main__":
    main()
