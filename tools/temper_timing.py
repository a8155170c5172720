#!/usr/bin/env python3
"""bk.TemperedStretcher on one GPU: what the tempered accept and a swap round cost beside bk.Stretcher's draw, and the rate of
bk_replica_swap on its algorithmic bytes beside bk_leapfrog_kick_drift's in the same process (profiles/tempered_stretcher.md).

    python tools/temper_timing.py [--small] [--out FILE.json]

  draws     DiagGaussian(logspace(0, 2, D)), D = 1,024, 64 ensembles of 1,024 walkers: as Stretcher(ensembles=64), twice (the
            A/A pair), as TemperedStretcher with 16 rungs x 4 replicas whose swap round never comes (swap_every past the
            run: the tempered accept and the running statistics alone), and the same with swap_every = 1.  Every sampler
            warmed up, then alternated over the repeats, device events around a block of draws.
  kernels   bk_replica_swap at 65,536 columns x 1,024, H = 512, the even pairs of 16 rungs (32,768 pairs) with log u =
            -inf, so that every pair swaps: 32 D bytes per swapped pair and array plus the scalars of the decision pass,
            with one array and with two (the state and the copy a draw returns); the same with log u = +inf (nothing swaps:
            the decision pass and the `swapped` bytes alone) and with a random log u that swaps a scattered part of the pairs
            (its bytes from the `accepted` counter); bk_leapfrog_kick_drift in place at 65,536 x 1,024 (40 bytes per
            element).  Alternated launch blocks between device events.
--small rehearses the script at toy sizes (its numbers are overheads)."""
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


def time_draws(walkers, T, replicas, D, draws, repeats):
    model = bk.DiagGaussian(np.logspace(0, 2, D))
    # a ladder dense enough that neighbours swap at this D (ll has sd sqrt(D / 2) / beta): steps of 0.7 / sqrt(D)
    betas = 1.0 - (0.7 / np.sqrt(D)) * np.arange(T)
    never = 10 ** 9
    samplers = {
        "Stretcher A": bk.Stretcher(model, walkers=walkers, ensembles=T * replicas, seed=1),
        "Stretcher A'": bk.Stretcher(model, walkers=walkers, ensembles=T * replicas, seed=1),
        "Tempered, no swap round": bk.TemperedStretcher(model, betas, walkers=walkers, replicas=replicas, seed=1,
                                                        swap_every=never),
        "Tempered, swap_every=1": bk.TemperedStretcher(model, betas, walkers=walkers, replicas=replicas, seed=1),
    }
    for s in samplers.values():
        for _ in range(4):
            s.sample()
    torch.cuda.synchronize()
    ms = {name: [] for name in samplers}
    for _ in range(repeats):
        for name, s in samplers.items():  # alternated
            ms[name].append(events_ms(s.sample, draws))
    out = {}
    for name, s in samplers.items():
        r = spread(ms[name])
        r.update(walkers=walkers, ensembles=T * replicas, D=D, chains=s.chains, accept_rate=s.accept_rate())
        if isinstance(s, bk.TemperedStretcher) and s.swap_every == 1:
            r["swap_rate"] = [round(float(x), 4) for x in s.swap_rate()]
        out[name] = r
    a, a2 = out["Stretcher A"]["median"], out["Stretcher A'"]["median"]
    out["summary"] = {
        "AA_spread": abs(a - a2) / a,
        "AA_repeat_range": max((r["max"] - r["min"]) / r["median"] for r in (out["Stretcher A"], out["Stretcher A'"])),
        "tempered_accept_over_stretcher": out["Tempered, no swap round"]["median"] / a,
        "swap_round_ms": out["Tempered, swap_every=1"]["median"] - out["Tempered, no swap round"]["median"],
    }
    return out


def time_kernels(H, T, replicas, D, reps, repeats):
    ops = bk._lib.default_ops()
    dev = ops.device
    C = 2 * replicas * T * H
    g = torch.Generator(device=dev).manual_seed(3)
    theta, theta2 = (torch.randn((D, C), dtype=torch.float64, device=dev, generator=g) for _ in range(2))
    ll = torch.randn(C, dtype=torch.float64, device=dev, generator=g)
    rung = (torch.arange(C, device=dev) % (C // 2)) // H % T
    beta = torch.linspace(1.0, 0.5, T, dtype=torch.float64, device=dev)[rung].contiguous()
    lower = ((rung % 2 == 0) & (rung + 1 < T)).to(torch.uint8).contiguous()
    pairs = int(lower.sum().item())
    swapped = torch.zeros(C, dtype=torch.uint8, device=dev)
    prop, acc = (torch.zeros(C // H, dtype=torch.int32, device=dev) for _ in range(2))
    all_swap = torch.full((C,), -np.inf, dtype=torch.float64, device=dev)
    none_swap = torch.full((C,), np.inf, dtype=torch.float64, device=dev)

    def swap(log_u, second):
        def fn():
            ops.replica_swap(theta, theta2 if second else None, ll, None, beta, log_u, lower, swapped, prop, acc, H)
        return fn

    # the decision pass: lower and swapped (1 byte each) for every column; log u, two beta and two ll read and two ll written
    # per pair; the exchange pass reads `swapped` for the C - H columns with a partner, once per row block and array
    scalars = 2.0 * C + 56.0 * pairs
    flags = (C - H) * np.ceil(D / 4)
    jobs = {
        "replica_swap, every pair, 1 array": (swap(all_swap, False), 32.0 * D * pairs + scalars + flags),
        "replica_swap, every pair, 2 arrays": (swap(all_swap, True), 64.0 * D * pairs + scalars + 2 * flags),
        "replica_swap, no pair, 1 array": (swap(none_swap, False), 2.0 * C + 40.0 * pairs + flags),
    }
    # about half of the pairs, scattered: ll of its own with a spread that makes (beta_t - beta_{t+1}) (ll' - ll) of order one;
    # every call swaps other pairs (a swap turns its pair's sign), so the bytes come from the `accepted` counter
    ll_half = ll * (1.0 / (0.5 / max(T - 1, 1)))
    some_swap = torch.log(torch.rand(C, dtype=torch.float64, device=dev, generator=g))
    acc_half = torch.zeros(C // H, dtype=torch.int32, device=dev)

    def swap_half():
        ops.replica_swap(theta, theta2, ll_half, None, beta, some_swap, lower, swapped, prop, acc_half, H)

    jobs["replica_swap, some pairs, 2 arrays"] = (swap_half, None)
    th, rho, grad = (torch.randn((D, C), dtype=torch.float64, device=dev, generator=g) * 1e-3 for _ in range(3))

    def kick_drift():
        ops.kick_drift(th, th, rho, rho, grad, None, 1e-3, False, 0.0, True, 1e-3)

    jobs[f"kick_drift C={C}"] = (kick_drift, 40.0 * D * C)
    for fn, _ in jobs.values():
        for _ in range(4):  # (an even count: the all-swap jobs leave the state as it was)
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in jobs}
    for _ in range(repeats):
        for name, (fn, _) in jobs.items():  # alternated
            ms[name].append(events_ms(fn, reps))
    calls_half = 4 + reps * repeats
    pairs_half = float(acc_half.sum().item()) / calls_half  # swapped pairs per call, averaged over every call made
    jobs["replica_swap, some pairs, 2 arrays"] = (swap_half, 64.0 * D * pairs_half + scalars + 2 * flags)
    out = {}
    for name, (_, nbytes) in jobs.items():
        r = spread(ms[name])
        r.update(bytes=nbytes, pairs=pairs, TB_per_s=nbytes / (r["median"] * 1e-3) / 1e12,
                 TB_per_s_range=[nbytes / (r["max"] * 1e-3) / 1e12, nbytes / (r["min"] * 1e-3) / 1e12])
        out[name] = r
    out["replica_swap, some pairs, 2 arrays"]["swapped_pairs_per_call"] = pairs_half
    kd = out[f"kick_drift C={C}"]["TB_per_s"]
    for r in out.values():
        r["rate_over_kick_drift"] = r["TB_per_s"] / kd
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.small:
        res = {"draws": time_draws(32, 4, 2, 16, 3, 2), "kernels": time_kernels(16, 4, 2, 16, 4, 2)}
    else:
        res = {"draws": time_draws(1024, 16, 4, 1024, 10, 7), "kernels": time_kernels(512, 16, 4, 1024, 20, 7)}
    res["device"] = torch.cuda.get_device_name(0)
    for name, r in res["draws"].items():
        if name == "summary":
            continue
        print(f"draw  {name:26s} {r['chains']:7d} x {r['D']:5d}: {r['median']:9.4f} ms per draw "
              f"[{r['min']:.4f}, {r['max']:.4f}], accept {r['accept_rate']:.3f}" +
              (f", swap rates {min(r['swap_rate']):.3f}-{max(r['swap_rate']):.3f}" if "swap_rate" in r else ""))
    s = res["draws"]["summary"]
    print(f"A/A: medians differ by {100 * s['AA_spread']:.2f} %, repeats range over {100 * s['AA_repeat_range']:.2f} %; "
          f"tempered draw without a swap round = {s['tempered_accept_over_stretcher']:.4f} x Stretcher's; "
          f"a swap round adds {s['swap_round_ms']:.4f} ms")
    for name, r in res["kernels"].items():
        print(f"kernel {name:36s}: {r['median']:8.4f} ms [{r['min']:.4f}, {r['max']:.4f}] = {r['TB_per_s']:.2f} TB/s "
              f"on {r['bytes'] / 1e6:.0f} MB, {r['rate_over_kick_drift']:.2f} x kick+drift")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
