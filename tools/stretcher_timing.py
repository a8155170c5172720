#!/usr/bin/env python3
"""bk.Stretcher on one GPU: ms per draw and per launch, and the rate of the proposal kernel on its algorithmic bytes beside
bk_leapfrog_kick_drift's in the same process (profiles/stretcher.md).

    python tools/stretcher_timing.py [--small] [--kernels-only] [--out FILE.json]

  draws     DiagGaussian(logspace(0, 2, D)), D = 1,024: 65,536 walkers in one ensemble; 64 ensembles of 2 D walkers; and a
            small shape (64 ensembles of 32 walkers at D = 16), where a draw is its 14 launches.  Every shape warmed up,
            then the shapes alternated over the repeats; the spread of one shape over its repeats is the A/A spread.
  kernels   bk_stretch_propose at 32,768 and at 65,536 active walkers x 1,024 (24 D bytes per active walker: its own column
            read, the partner's gathered, the proposal written) and bk_leapfrog_kick_drift in place at 65,536 x 1,024
            (40 bytes per element), alternated launch blocks between device events.
--small rehearses the script at toy sizes (its numbers are overheads); --kernels-only runs a few launches of the kernels
section and nothing else (the program of a counters-only `rocprofv3 --pmc` pass)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bayes-kit_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bayes_kit_amd as bk  # noqa: E402

LAUNCHES_PER_DRAW = 14  # per half: two uniforms, log uniform, proposal, log density, accept, select


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


def time_draws(shapes, draws, repeats):
    samplers = {}
    for name, (walkers, E, D) in shapes.items():
        s = bk.Stretcher(bk.DiagGaussian(np.logspace(0, 2, D)), walkers=walkers, ensembles=E, seed=1)
        for _ in range(3):
            s.sample()
        samplers[name] = s
    torch.cuda.synchronize()
    ms = {name: [] for name in shapes}
    for _ in range(repeats):
        for name, s in samplers.items():  # alternated
            ms[name].append(events_ms(s.sample, draws))
    out = {}
    for name, (walkers, E, D) in shapes.items():
        r = spread(ms[name])
        r.update(walkers=walkers, ensembles=E, D=D, chains=walkers * E, accept_rate=samplers[name].accept_rate(),
                 ms_per_launch=r["median"] / LAUNCHES_PER_DRAW)
        out[name] = r
    return out


def time_kernels(C, D, halves, reps, repeats):
    ops = bk._lib.default_ops()
    dev = ops.device
    g = torch.Generator(device=dev).manual_seed(3)
    jobs = {}
    for n, H in halves:
        theta = torch.randn((D, 2 * n), dtype=torch.float64, device=dev, generator=g)
        prop = torch.empty((D, n), dtype=torch.float64, device=dev)
        u_j = torch.rand(n, dtype=torch.float64, device=dev, generator=g)
        u_z = torch.rand(n, dtype=torch.float64, device=dev, generator=g)
        zt = torch.empty(n, dtype=torch.float64, device=dev)
        pa = torch.empty(n, dtype=torch.int32, device=dev)
        lo, hi = 1 / np.sqrt(2.0), np.sqrt(2.0)

        def propose(theta=theta, prop=prop, u_j=u_j, u_z=u_z, zt=zt, pa=pa, n=n, H=H):
            ops.stretch_propose(theta, n, 0, n, H, u_j, u_z, lo, hi, prop, zt, pa)  # (the second half active)

        jobs[f"stretch_propose n={n} H={H}"] = (propose, 24.0 * D * n)
    th, rho, grad = (torch.randn((D, C), dtype=torch.float64, device=dev, generator=g) * 1e-3 for _ in range(3))

    def kick_drift():
        ops.kick_drift(th, th, rho, rho, grad, None, 1e-3, False, 0.0, True, 1e-3)

    jobs[f"kick_drift C={C}"] = (kick_drift, 40.0 * D * C)
    for fn, _ in jobs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in jobs}
    for _ in range(repeats):
        for name, (fn, _) in jobs.items():  # alternated
            ms[name].append(events_ms(fn, reps))
    out = {}
    for name, (_, nbytes) in jobs.items():
        r = spread(ms[name])
        r.update(bytes=nbytes, TB_per_s=nbytes / (r["median"] * 1e-3) / 1e12,
                 TB_per_s_range=[nbytes / (r["max"] * 1e-3) / 1e12, nbytes / (r["min"] * 1e-3) / 1e12])
        out[name] = r
    kd = out[f"kick_drift C={C}"]["TB_per_s"]
    for name, r in out.items():
        r["rate_over_kick_drift"] = r["TB_per_s"] / kd
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.kernels_only:
        res = {"draws": {}, "kernels": time_kernels(65536, 1024, [(32768, 32768), (65536, 1024)], 2, 1)}
    elif args.small:
        shapes = {"one ensemble": (256, 1, 16), "64 ensembles of 2 D": (32, 64, 16), "small": (32, 4, 16)}
        res = {"draws": time_draws(shapes, 3, 2), "kernels": time_kernels(512, 16, [(256, 256), (512, 8)], 3, 2)}
    else:
        shapes = {"one ensemble": (65536, 1, 1024), "64 ensembles of 2 D": (2048, 64, 1024), "small": (32, 64, 16)}
        res = {"draws": time_draws(shapes, 10, 5),
               "kernels": time_kernels(65536, 1024, [(32768, 32768), (65536, 1024)], 20, 7)}
    res["device"] = torch.cuda.get_device_name(0)
    for name, r in res["draws"].items():
        print(f"draw  {name:22s} {r['chains']:7d} x {r['D']:5d}: {r['median']:9.4f} ms per draw "
              f"[{r['min']:.4f}, {r['max']:.4f}], {1e3 * r['ms_per_launch']:8.2f} us per launch, accept {r['accept_rate']:.3f}")
    for name, r in res["kernels"].items():
        print(f"kernel {name:34s}: {r['median']:8.4f} ms [{r['min']:.4f}, {r['max']:.4f}] = {r['TB_per_s']:.2f} TB/s "
              f"on {r['bytes'] / 1e6:.0f} MB, {r['rate_over_kick_drift']:.2f} x kick+drift")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
