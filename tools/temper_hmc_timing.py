#!/usr/bin/env python3
"""bk.TemperedHMC on one GPU: its integrator kernels beside the plain ones, its draw beside bk.HMCDiag's, and cold-rung ESS per
second beside bk.TemperedStretcher's (profiles/tempered_hmc.md).

    python tools/temper_hmc_timing.py [--small] [--skip-ess] [--out FILE.json]

  A kernels  bk_tempered_kick_drift in place at 65,536 x 1,024 with 16 rungs (a step size per rung, kick = eps: the
             steady-state step), with and without grad_lp0, beside bk_leapfrog_kick_drift on the same arrays, which is
             launched under two names (the A/A pair); the same for bk_tempered_finish beside bk_leapfrog_finish.  Alternated
             launch blocks between device events.  Bytes: 40 D C (48 with grad_lp0) and 16 D C (24) plus the vectors.
  B draws    DiagGaussian(logspace(0, 2, D)): HMCDiag(path="opaque") twice (A/A), TemperedHMC with 16 rungs whose swap round
             never comes, and with swap_every = 1; same C, D and steps.
  C ess      N(0, I) at D = 16 and 256, 8 rungs, 512 cold chains: bulk ESS of the cold rows' first coordinate per second of
             sampling, TemperedHMC (step sizes from warmup(100), 8 steps) beside TemperedStretcher (a = 2).
--small rehearses the script at toy sizes (its numbers are overheads)."""
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


def alternate(jobs, reps, repeats, warm=3):
    for fn in jobs.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in jobs}
    for _ in range(repeats):
        for name, fn in jobs.items():
            ms[name].append(events_ms(fn, reps))
    return {name: spread(v) for name, v in ms.items()}


def time_kernels(H, T, replicas, D, reps, repeats):
    ops = bk._lib.default_ops()
    dev = ops.device
    C = replicas * T * H
    g = torch.Generator(device=dev).manual_seed(3)
    th, rho, grad, grad0 = (torch.randn((D, C), dtype=torch.float64, device=dev, generator=g) * 1e-3 for _ in range(4))
    rung = (torch.arange(C, device=dev) // H) % T
    beta = torch.linspace(1.0, 0.5, T, dtype=torch.float64, device=dev)[rung].contiguous()
    eps = (1e-3 / torch.sqrt(beta)).contiguous()
    half = (0.5 * eps).contiguous()
    kin = torch.zeros(C, dtype=torch.float64, device=dev)

    def kd():
        ops.kick_drift(th, th, rho, rho, grad, None, 1e-3, False, 0.0, True, 1e-3)

    def fin():
        ops.leapfrog_finish(rho, None, grad, None, 5e-4, False, kin)

    jobs = {
        "leapfrog_kick_drift A": kd, "leapfrog_kick_drift A'": lambda: kd(),
        "tempered_kick_drift": lambda: ops.tempered_kick_drift(th, th, rho, rho, grad, None, None, beta, eps, None, eps),
        "tempered_kick_drift + grad_lp0": lambda: ops.tempered_kick_drift(th, th, rho, rho, grad, grad0, None, beta, eps, None,
                                                                          eps),
        "leapfrog_finish A": fin, "leapfrog_finish A'": lambda: fin(),
        "tempered_finish": lambda: ops.tempered_finish(rho, None, grad, None, None, beta, half, kin),
        "tempered_finish + grad_lp0": lambda: ops.tempered_finish(rho, None, grad, grad0, None, beta, half, kin),
    }
    nbytes = {"leapfrog_kick_drift A": 40.0 * D * C, "leapfrog_kick_drift A'": 40.0 * D * C,
              "tempered_kick_drift": 40.0 * D * C + 24.0 * C, "tempered_kick_drift + grad_lp0": 48.0 * D * C + 24.0 * C,
              "leapfrog_finish A": 16.0 * D * C + 8.0 * C, "leapfrog_finish A'": 16.0 * D * C + 8.0 * C,
              "tempered_finish": 16.0 * D * C + 24.0 * C, "tempered_finish + grad_lp0": 24.0 * D * C + 24.0 * C}
    out = alternate(jobs, reps, repeats)
    for name, r in out.items():
        r.update(bytes=nbytes[name], TB_per_s=nbytes[name] / (r["median"] * 1e-3) / 1e12)
    summary = {}
    for fam, base in (("kick_drift", 40.0), ("finish", 16.0)):
        a, a2 = out[f"leapfrog_{fam} A"], out[f"leapfrog_{fam} A'"]
        aa = abs(a["median"] - a2["median"]) / a["median"]
        rng = max((r["max"] - r["min"]) / r["median"] for r in (a, a2))
        # the per-column vectors' bytes from HBM as a share of the stream's: 8 C bytes per vector (kick+drift: beta, eps,
        # kick; finish: beta, half); their repeated reads (once per 4 rows / per quarter of the rows) are cache hits
        extra = (24.0 if fam == "kick_drift" else 16.0) / (base * D)
        t = out[f"tempered_{fam}"]
        ratio = t["median"] / min(a["median"], a2["median"])
        allowed = 1.0 + max(aa, rng) + extra
        summary[fam] = {"AA_median_difference": aa, "AA_repeat_range": rng, "vector_request_share": extra,
                        "tempered_time_over_yardstick": ratio, "allowed": allowed, "aim": "hit" if ratio <= allowed else "MISSED",
                        "with_grad_lp0_rate_over_yardstick": out[f"tempered_{fam} + grad_lp0"]["TB_per_s"] / a["TB_per_s"]}
    out["summary"] = summary
    out["shape"] = {"C": C, "D": D, "H": H, "T": T, "replicas": replicas}
    return out


def time_draws(H, T, replicas, D, steps, draws, repeats):
    model = bk.DiagGaussian(np.logspace(0, 2, D))
    C = replicas * T * H
    betas = (1.0 - 0.7 / np.sqrt(D)) ** np.arange(T)  # (dense enough that neighbours swap at this D)
    eps = 0.01 / np.sqrt(betas)
    samplers = {
        "HMCDiag opaque A": bk.HMCDiag(model, 0.01, steps, seed=1, chains=C, path="opaque"),
        "HMCDiag opaque A'": bk.HMCDiag(model, 0.01, steps, seed=1, chains=C, path="opaque"),
        "TemperedHMC, no swap round": bk.TemperedHMC(model, betas, eps, steps, chains=H, replicas=replicas, seed=1,
                                                     swap_every=10 ** 9),
        "TemperedHMC, swap_every=1": bk.TemperedHMC(model, betas, eps, steps, chains=H, replicas=replicas, seed=1),
    }
    out = alternate({k: s.sample for k, s in samplers.items()}, draws, repeats)
    for name, s in samplers.items():
        out[name].update(chains=s.chains, D=D, steps=steps, accept_rate=float(s.accept_rate()))
    sw = samplers["TemperedHMC, swap_every=1"]
    out["TemperedHMC, swap_every=1"]["swap_rate"] = [round(float(x), 4) for x in sw.swap_rate()]
    a, a2 = out["HMCDiag opaque A"]["median"], out["HMCDiag opaque A'"]["median"]
    out["summary"] = {"AA_median_difference": abs(a - a2) / a,
                      "tempered_draw_over_hmc": out["TemperedHMC, no swap round"]["median"] / min(a, a2),
                      "swap_round_ms": out["TemperedHMC, swap_every=1"]["median"] - out["TemperedHMC, no swap round"]["median"]}
    return out


def ess_per_second(D, T, cold, burn, draws, steps):
    model = bk.IsoGaussian(D)
    betas = (1.0 - 0.7 / np.sqrt(D)) ** np.arange(T)  # (dense enough that neighbours swap at this D)
    out = {}
    for name in ("TemperedHMC", "TemperedStretcher"):
        if name == "TemperedHMC":
            s = bk.TemperedHMC(model, betas, 0.5 * D ** -0.25 / np.sqrt(betas), steps, chains=cold, seed=1)
            s.warmup(burn)
        else:
            s = bk.TemperedStretcher(model, betas, walkers=cold, seed=1)
            for _ in range(burn):
                s.sample()
        rows = s.cold_rows()
        series = torch.empty((draws, rows.numel()), dtype=torch.float64, device=rows.device)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for n in range(draws):
            series[n] = s.sample()[0][rows, 0]
        torch.cuda.synchronize()
        sec = time.perf_counter() - t0
        ess = float(bk.ess_bulk(series))
        out[name] = {"D": D, "rungs": T, "cold_chains": int(rows.numel()), "draws": draws, "seconds": sec, "ess_bulk": ess,
                     "ess_per_second": ess / sec, "ess_per_draw_and_chain": ess / (draws * rows.numel()),
                     "swap_rate": [round(float(x), 3) for x in s.swap_rate()],
                     "cold_accept_rate": float(s.rung_accept_rate()[0])}
        if name == "TemperedHMC":
            out[name]["stepsizes"] = [round(float(e), 4) for e in s.stepsizes]
    out["hmc_over_stretcher"] = out["TemperedHMC"]["ess_per_second"] / out["TemperedStretcher"]["ess_per_second"]
    return out


def print_kernels(k):
    for name, r in k.items():
        if name in ("summary", "shape"):
            continue
        print(f"kernel {name:32s}: {r['median']:8.4f} ms [{r['min']:.4f}, {r['max']:.4f}] = {r['TB_per_s']:.2f} TB/s on "
              f"{r['bytes'] / 1e6:.0f} MB")
    for fam, s in k["summary"].items():
        print(f"A {fam}: tempered / yardstick = {s['tempered_time_over_yardstick']:.4f}, allowed {s['allowed']:.4f} (A/A medians "
              f"{100 * s['AA_median_difference']:.2f} %, repeats {100 * s['AA_repeat_range']:.2f} %, vectors "
              f"{100 * s['vector_request_share']:.2f} %): {s['aim']}; with grad_lp0 {s['with_grad_lp0_rate_over_yardstick']:.3f} x "
              f"the yardstick's rate", flush=True)


def print_draws(d):
    for name, r in d.items():
        if name == "summary":
            continue
        print(f"draw  {name:28s} {r['chains']:7d} x {r['D']:5d}, {r['steps']} steps: {r['median']:9.4f} ms per draw "
              f"[{r['min']:.4f}, {r['max']:.4f}], accept {r['accept_rate']:.3f}")
    s = d["summary"]
    print(f"B: A/A medians differ by {100 * s['AA_median_difference']:.2f} %; TemperedHMC draw without a swap round = "
          f"{s['tempered_draw_over_hmc']:.4f} x HMCDiag's; a swap round adds {s['swap_round_ms']:.4f} ms", flush=True)


def print_ess(e):
    for name in ("TemperedHMC", "TemperedStretcher"):
        r = e[name]
        print(f"C D={r['D']:4d} {name:18s}: bulk ESS {r['ess_bulk']:10.0f} of {r['draws']} x {r['cold_chains']} in "
              f"{r['seconds']:.3f} s = {r['ess_per_second']:.0f} / s; cold acceptance {r['cold_accept_rate']:.3f}, swap rates "
              f"{min(r['swap_rate']):.3f}-{max(r['swap_rate']):.3f}")
    print(f"C D={e['TemperedHMC']['D']:4d}: TemperedHMC / TemperedStretcher = {e['hmc_over_stretcher']:.2f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--skip-ess", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    small = args.small
    res = {"device": torch.cuda.get_device_name(0)}
    res["kernels"] = time_kernels(16, 4, 2, 16, 4, 2) if small else time_kernels(1024, 16, 4, 1024, 20, 7)
    print_kernels(res["kernels"])
    res["draws"] = time_draws(16, 4, 2, 16, 3, 3, 2) if small else time_draws(1024, 16, 4, 1024, 4, 5, 5)
    print_draws(res["draws"])
    if not args.skip_ess:
        res["ess"] = []
        for shape in (((4, 3, 16, 10, 40, 3),) if small else ((16, 8, 512, 100, 400, 8), (256, 8, 512, 100, 400, 8))):
            res["ess"].append(ess_per_second(*shape))
            print_ess(res["ess"][-1])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
