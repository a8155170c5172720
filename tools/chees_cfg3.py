"""What HMCDiag.warmup(adapt_trajectory=True) finds and costs on one MI355X; writes profiles/chees_adapt.md and
profiles/chees_adapt.json.

One process; every section runs under its own time limit (a watchdog ends the process when it is exceeded) and an error in
one ends the run -- nothing is started on the GPU after a failure.  Host clock around a device synchronise, every shape
warmed first, the variants of a comparison alternated round by round, one A/A pair per comparison to show the spread.

  user_gain      config-3 target (lam = logspace(0, 4, 1024)) at 16,384 chains, from eps = 0.006 and L = 16: warmup(300)
                 against warmup(300, adapt_trajectory=True); then 1,000 draws each: the adapted T and eps, ms per draw, bulk ESS
                 per second of theta[0] and of the worst of 16 spread dimensions; ms per warmup draw of both
  stat_launches  bk_chees_sums and bk_chees_stat at the same shape (and at 65,536 chains) against the 40 D C bytes they read

    python tools/chees_cfg3.py [--small] [--warmup-lines FILE] [--out profiles/chees_adapt]

--small: tiny shapes, a rehearsal of the script itself (its numbers mean nothing).  --warmup-lines: a file of
"label<TAB>JSON" rows, each printed by `python tools/chees_cfg3.py --warmup-only` in a tree of its own (this commit and its
parent, alternated, same box), rendered as the "a warmup draw costs what it did" table.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bayes-kit_amd")]

import numpy as np
import torch

import bayes_kit_amd as bk
from bench_config import D_CFG3, EPS_CFG3, SEED_CFG3
from tools.warmup_cfg3 import alternate, section, spread


def _warmup(s, draws, **kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rep = s.warmup(draws, **kw)
    torch.cuda.synchronize()
    return rep, time.perf_counter() - t0


def warmup_only(C, D, draws, rounds):
    """ms per warmup draw of the plain warmup (no trajectory adaptation: what the parent commit has too), `rounds` fresh
    samplers after one that warms the shape."""
    lam = torch.logspace(0, 4, D, dtype=torch.float64)
    ms = []
    for r in range(rounds + 1):
        s = bk.HMCDiag(bk.DiagGaussian(lam), EPS_CFG3, 16, chains=C, seed=SEED_CFG3)
        _, el = _warmup(s, draws)
        if r:
            ms.append(round(1e3 * el / draws, 4))
        del s
        torch.cuda.empty_cache()
    return {"chains": C, "D": D, "draws": draws, "warmup_ms_per_draw": ms}


def user_gain(C, D, draws, warm_draws):
    lam = torch.logspace(0, 4, D, dtype=torch.float64)
    dims = [0] + [int(round(x)) for x in np.linspace(0, D - 1, 16)]  # theta[0], then 16 spread dimensions (0 .. D-1)
    dims_t = torch.tensor(dims, device="cuda")
    rows = []
    for label, kw in (("warmup(%d)" % warm_draws, dict()), ("warmup(%d) (A/A)" % warm_draws, dict()),
                      ("warmup(%d, adapt_trajectory=True)" % warm_draws, dict(adapt_trajectory=True))):
        s = bk.HMCDiag(bk.DiagGaussian(lam), EPS_CFG3, 16, chains=C, seed=SEED_CFG3)
        rep, el = _warmup(s, warm_draws, **kw)
        row = {"variant": label, "warmup_ms_per_draw": round(1e3 * el / warm_draws, 4), "eps": float(s._stepsize),
               "T": rep.get("trajectory_length"), "steps_fixed": None if kw else int(s._steps),
               "max_abs_v_lam_minus_1": round(float(np.abs(rep["precond_diag"] * lam.numpy() - 1.0).max()), 4),
               "alpha_last_20": round(float(np.mean(rep["alpha"][-20:])), 4),
               "nonfinite_chains": rep.get("nonfinite_chains"),
               "warmup_leapfrog_steps": int(sum(rep["steps"])) if kw else 16 * warm_draws}
        assert s._fused_draw  # (sampling runs on the whole-draw kernel again)
        series = torch.empty((len(dims), draws, C), dtype=torch.float64, device="cuda")
        acc0, steps = float(s._accepted.item()), 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for n in range(draws):
            th, _ = s.sample()
            steps += s.last_steps
            series[:, n] = th[:, dims_t].t()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        row["ms_per_draw"] = round(1e3 * el / draws, 4)
        row["mean_steps_per_draw"] = round(steps / draws, 2)
        row["accept_rate"] = round((float(s._accepted.item()) - acc0) / (draws * C), 4)
        bulk = [float(bk.ess_bulk(series[k])) for k in range(len(dims))]
        row["ess_bulk_theta0"], row["ess_bulk_min_16"] = round(bulk[0], 1), round(min(bulk[1:]), 1)
        row["ess_bulk_theta0_per_sec"] = round(bulk[0] / el, 1)
        row["ess_bulk_min_16_per_sec"] = round(min(bulk[1:]) / el, 1)
        rows.append(row)
        del s, series
        torch.cuda.empty_cache()
    return {"chains": C, "D": D, "draws": draws, "dims": dims, "rows": rows}


def stat_launches(shapes, n, rounds):
    ops = bk._lib.default_ops()
    out = []
    for C, D in shapes:
        g = torch.Generator(device="cuda").manual_seed(1)
        th, thp, rho = (torch.randn((D, C), dtype=torch.float64, device="cuda", generator=g) for _ in range(3))
        lp0, k0, lp1, k1 = (torch.randn(C, dtype=torch.float64, device="cuda", generator=g) for _ in range(4))
        sums = torch.zeros(2 * D + 1, dtype=torch.float64, device="cuda")
        stat = torch.zeros(2, dtype=torch.float64, device="cuda")
        work = torch.empty(ops.chees_work_elems(C), dtype=torch.float64, device="cuda")
        ops.chees_sums(th, thp, sums)
        mean = (sums[:2 * D] / float(C)).contiguous()
        launches = {
            "chees_sums": lambda: ops.chees_sums(th, thp, sums),
            "chees_sums (A/A)": lambda: ops.chees_sums(th, thp, sums),
            "chees_stat": lambda: ops.chees_stat(th, thp, rho, mean, lp0, k0, lp1, k1, stat, work),
            "chees_stat (A/A)": lambda: ops.chees_stat(th, thp, rho, mean, lp0, k0, lp1, k1, stat, work),
        }
        res = alternate(launches, n, rounds)
        both = res["chees_sums"]["ms"] + res["chees_stat"]["ms"]
        out.append({"shape": [D, C], "launches_per_round": n, "ms": res, "bytes_read": 40 * D * C,
                    "both_ms": round(both, 4), "GB_per_s_both": round(40 * D * C / (both * 1e-3) / 1e9, 1),
                    "GB_per_s_sums": round(16 * D * C / (res["chees_sums"]["ms"] * 1e-3) / 1e9, 1),
                    "GB_per_s_stat": round(24 * D * C / (res["chees_stat"]["ms"] * 1e-3) / 1e9, 1),
                    "aa_spread_percent": {"chees_sums": spread(res, "chees_sums (A/A)", "chees_sums"),
                                          "chees_stat": spread(res, "chees_stat (A/A)", "chees_stat")}})
        del th, thp, rho, work
        torch.cuda.empty_cache()
    return out


def render(res):
    L = ["# Trajectory-length adaptation (ChEES) on the MI355X", "",
         f"Written by `tools/chees_cfg3.py` ({res['device']}, one process, {res['date']}).  Times: host clock around a device",
         "synchronise after warming every shape; the variants of a launch comparison alternated round by round, median of the",
         "rounds; an A/A pair is the same variant built twice.", ""]
    ug = res["user_gain"]
    L += [f"## What a user gains (config-3 target, {ug['chains']} chains, from eps = 0.006 and L = 16; {ug['draws']} draws after "
          "the warmup)", "",
          "| variant | adapted T | adapted eps | mean steps per draw | ms per draw | accept | ess_bulk theta[0] | ess_bulk min of 16 | "
          "ESS/s theta[0] (bulk) | ESS/s min of 16 (bulk) | ms per warmup draw | leapfrog steps in the warmup |",
          "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in ug["rows"]:
        T = "(L = %d)" % r["steps_fixed"] if r["T"] is None else "%.4g" % r["T"]
        L.append(f"| {r['variant']} | {T} | {r['eps']:.4g} | {r['mean_steps_per_draw']} | {r['ms_per_draw']} | {r['accept_rate']} | "
                 f"{r['ess_bulk_theta0']} | {r['ess_bulk_min_16']} | {r['ess_bulk_theta0_per_sec']:.4g} | "
                 f"{r['ess_bulk_min_16_per_sec']:.4g} | {r['warmup_ms_per_draw']} | {r['warmup_leapfrog_steps']} |")
    L += ["", "Beside these, measured earlier on another box (README): 4.9e7 ESS/s of theta[0] with L = 16 after warmup, 1.6e7 with "
              "the hand-tuned eps = 0.006, L = 384.  A warmup draw that adapts the trajectory runs the step-by-step path with a "
              "jittered number of steps, so its cost per draw is not comparable step for step: the last column counts them.", ""]
    if res.get("warmup_lines"):
        L += ["## A warmup draw without the flag costs what it did: this commit and its parent, same box, alternated", "",
              "| run | ms per warmup draw (fresh samplers) |", "|---|---|"]
        for lab, j in res["warmup_lines"]:
            L.append(f"| {lab} | {j.get('warmup_ms_per_draw')} |")
        L.append("")
    L += ["## The two statistic launches against the bytes they read", "",
          "| D x C | bk_chees_sums ms (A/A) | bk_chees_stat ms (A/A) | both ms | bytes read (40 D C) | GB/s both | GB/s sums (16 D C) | "
          "GB/s stat (24 D C) |", "|---|---|---|---|---|---|---|---|"]
    for r in res["stat_launches"]:
        m = r["ms"]
        L.append(f"| {r['shape'][0]} x {r['shape'][1]} | {m['chees_sums']['ms']} ({m['chees_sums (A/A)']['ms']}) | "
                 f"{m['chees_stat']['ms']} ({m['chees_stat (A/A)']['ms']}) | {r['both_ms']} | {r['bytes_read']} | {r['GB_per_s_both']} | "
                 f"{r['GB_per_s_sums']} | {r['GB_per_s_stat']} |")
    L += ["", "(bk_chees_stat also writes and reads back 12 C doubles of quarter partials, which the byte count leaves out.)", "",
          f"Section wall times (s): {res['section_seconds']}", ""]
    return "\n".join(L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--warmup-only", action="store_true")
    ap.add_argument("--warmup-lines")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chees_adapt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/chees_cfg3.py measures on a GPU"
    small = a.small
    C, D = (512, 64) if small else (16384, D_CFG3)
    if a.warmup_only:
        with section("warmup_only", 240):
            print(json.dumps(warmup_only(C, D, 40 if small else 300, 2)))
        return
    res = {"device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "small": small}
    if a.warmup_lines:
        res["warmup_lines"] = []
        for line in open(a.warmup_lines):
            if "\t" in line:
                lab, js = line.rstrip("\n").split("\t", 1)
                res["warmup_lines"].append((lab, json.loads(js)))
    with section("user_gain", 420):
        res["user_gain"] = user_gain(C, D, 40 if small else 1000, 40 if small else 300)
    with section("stat_launches", 120):
        res["stat_launches"] = stat_launches([(C, D)] if small else [(16384, D_CFG3), (65536, D_CFG3)], 5 if small else 20,
                                             2 if small else 5)
    res["section_seconds"] = section.times
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out + ".json", "w") as f:
        json.dump(res, f, indent=1)
    with open(a.out + ".md", "w") as f:
        f.write(render(res))
    print(json.dumps({"wrote": [a.out + ".md", a.out + ".json"]}))


if __name__ == "__main__":
    main()
