#!/usr/bin/env python3
"""bk.DifferentialEvolution on one GPU beside bk.Stretcher: the proposal kernels, the whole draw, and the acceptance
(profiles/differential_evolution.md).

    python tools/de_timing.py [--small] [--out FILE.json]

  kernels   bk_de_propose (32 D bytes per active walker: its own column read, two partners gathered, the proposal written)
            beside bk_stretch_propose (24 D bytes) on the same state, at 65,536 active walkers x 1,024 in 64 ensembles
            (1,024 walkers per half: a row's partners are 8 KB, served from the CU's cache) and at 32,768 active walkers x
            1,024 in one ensemble (32,768 per half: a row's partners are 256 KB).  Launch blocks between device events,
            alternated; the stretch kernel runs under two names, and the gap between the two is the A/A spread.  The aim at
            1,024 per half: time(de) / time(stretch) <= 32 / 24 plus the A/A spread.  No bar at 32,768 per half.
  draws     DiagGaussian(logspace(0, 2, D)), D = 1,024, at the same two shapes: ms per draw of both samplers, alternated.
  accept    IsoGaussian(D) from its own draws, default settings of both samplers (2 D and 4 D walkers), 64 ensembles, at
            D = 16 and D = 256: accepted moves per proposed one.
--small rehearses the script at toy sizes (its numbers are overheads)."""
import argparse
import json
import os
import statistics
import sys
import warnings

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


def alternate(jobs, reps, repeats):
    for fn in jobs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in jobs}
    for _ in range(repeats):
        for name, fn in jobs.items():
            ms[name].append(events_ms(fn, reps))
    return {name: spread(v) for name, v in ms.items()}


def time_kernels(D, n, H, reps, repeats, bar=True):
    ops = bk._lib.default_ops()
    dev = ops.device
    g = torch.Generator(device=dev).manual_seed(3)
    theta = torch.randn((D, 2 * n), dtype=torch.float64, device=dev, generator=g)
    prop = torch.empty((D, n), dtype=torch.float64, device=dev)
    u_1, u_2 = (torch.rand(n, dtype=torch.float64, device=dev, generator=g) for _ in range(2))
    z = torch.randn(n, dtype=torch.float64, device=dev, generator=g)
    zt, ga = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(2))
    p1, p2 = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
    lo, hi = 1 / np.sqrt(2.0), np.sqrt(2.0)
    gamma0 = 2.38 / np.sqrt(2.0 * D)

    def stretch():
        ops.stretch_propose(theta, n, 0, n, H, u_1, u_2, lo, hi, prop, zt, p1)  # (the second half active)

    def de():
        ops.de_propose(theta, n, 0, n, H, u_1, u_2, z, gamma0, 1e-5, prop, p1, p2, ga)

    r = alternate({"stretch A": stretch, "de": de, "stretch B": lambda: stretch()}, reps, repeats)
    a, b, d = r["stretch A"]["median"], r["stretch B"]["median"], r["de"]["median"]
    st = 0.5 * (a + b)
    aa = abs(a - b) / st
    out = {"n": n, "H": H, "D": D, "stretch_A": r["stretch A"], "stretch_B": r["stretch B"], "de": r["de"],
           "stretch_TB_per_s": 24.0 * D * n / (st * 1e-3) / 1e12, "de_TB_per_s": 32.0 * D * n / (d * 1e-3) / 1e12,
           "de_over_stretch": d / st, "aa_spread": aa, "aim": 32.0 / 24.0 * (1.0 + aa)}
    out["verdict"] = ("met" if out["de_over_stretch"] <= out["aim"] else "MISSED") if bar else "no bar"
    return out


def time_draws(walkers, E, D, draws, repeats):
    model = bk.DiagGaussian(np.logspace(0, 2, D))
    s = bk.Stretcher(model, walkers=walkers, ensembles=E, seed=1)
    with warnings.catch_warnings():  # (2 D walkers as the Stretcher's shape: timed here, not sampled from)
        warnings.simplefilter("ignore", UserWarning)
        d = bk.DifferentialEvolution(model, walkers=walkers, ensembles=E, seed=1)
    r = alternate({"stretcher": s.sample, "differential evolution": d.sample}, draws, repeats)
    return {"walkers": walkers, "ensembles": E, "D": D, "chains": walkers * E, "stretcher": r["stretcher"],
            "de": r["differential evolution"],
            "de_over_stretcher": r["differential evolution"]["median"] / r["stretcher"]["median"]}


def acceptance(D, E, draws):
    model = bk.IsoGaussian(D)
    out = {"D": D, "ensembles": E, "draws": draws}
    for name, s in (("stretcher", bk.Stretcher(model, ensembles=E, seed=2)),
                    ("de", bk.DifferentialEvolution(model, ensembles=E, seed=2))):
        for _ in range(draws):
            s.sample()
        out[name] = {"walkers": s.walkers, "accept_rate": s.accept_rate()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.small:
        res = {"kernels": {"cache": time_kernels(16, 512, 8, 3, 2), "one ensemble": time_kernels(16, 256, 256, 3, 2, bar=False)},
               "draws": {"cache": time_draws(16, 32, 16, 3, 2), "one ensemble": time_draws(512, 1, 16, 3, 2)},
               "accept": [acceptance(D, 2, 5) for D in (4, 16)]}
    else:
        res = {"kernels": {"1,024 per half": time_kernels(1024, 65536, 1024, 20, 7),
                           "32,768 per half": time_kernels(1024, 32768, 32768, 20, 7, bar=False)},
               "draws": {"1,024 per half": time_draws(2048, 64, 1024, 5, 5),
                         "32,768 per half": time_draws(65536, 1, 1024, 10, 5)},
               "accept": [acceptance(D, 64, 200) for D in (16, 256)]}
    res["device"] = torch.cuda.get_device_name(0)
    for name, r in res["kernels"].items():
        print(f"kernel {name:16s} n={r['n']:6d} D={r['D']:5d}: de {r['de']['median']:.4f} ms = {r['de_TB_per_s']:.2f} TB/s, "
              f"stretch {r['stretch_A']['median']:.4f} / {r['stretch_B']['median']:.4f} ms = {r['stretch_TB_per_s']:.2f} TB/s, "
              f"de / stretch = {r['de_over_stretch']:.3f}, A/A spread {r['aa_spread']:.3f}, aim <= {r['aim']:.3f}: "
              f"{r['verdict']}")
    for name, r in res["draws"].items():
        print(f"draw   {name:16s} {r['chains']:7d} x {r['D']:5d}: differential evolution {r['de']['median']:.4f} ms "
              f"[{r['de']['min']:.4f}, {r['de']['max']:.4f}], stretcher {r['stretcher']['median']:.4f} ms "
              f"[{r['stretcher']['min']:.4f}, {r['stretcher']['max']:.4f}], ratio {r['de_over_stretcher']:.3f}")
    for r in res["accept"]:
        print(f"accept N(0, I) D={r['D']:4d}: differential evolution ({r['de']['walkers']} walkers) "
              f"{r['de']['accept_rate']:.4f}, stretcher ({r['stretcher']['walkers']} walkers) "
              f"{r['stretcher']['accept_rate']:.4f}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
