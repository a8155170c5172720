"""Cost and gain of MALA's diagonal preconditioner and of MALA.warmup on one MI355X; writes profiles/mala_warmup.md and
profiles/mala_warmup.json.

One process; every section runs under its own time limit (a watchdog ends the process when it is exceeded) and an error in
one ends the run -- nothing is started on the GPU after a failure.  Host clock around a device synchronise, every shape
warmed first, the variants of a comparison alternated round by round, one A/A pair per comparison to show the spread.

  kernel_cost    config-3 target at 16,384 chains x D = 1,024, two-pass draws: the preconditioned step kernels
                 (bk_mala_step_precond with the model's gradient op; bk_mala_step_gaussian_precond with its log-density
                 launch) against the unpreconditioned ones.  With --parent-lib the unpreconditioned side is the PARENT
                 commit's library, loaded beside this one and driven by the same Python, its A/A pair included; without it,
                 this commit's flag-off instantiations (instruction for instruction the parent's, see the note).
  overhead       a warmup draw (step-by-step composition + statistic kernel + one host read, + Welford update inside a
                 window) against a plain draw of the same sampler and against a plain step-by-step draw
  user_gain      warmup(300) from epsilon = 1e-5, then 1,000 draws, against a hand scan of epsilon without a preconditioner
                 (each started inside the target); bulk ESS per second of theta[0] and of the worst of 16 spread dimensions

    python tools/mala_warmup_cfg3.py [--small] [--parent-lib PATH] [--bench-lines FILE] [--out profiles/mala_warmup]

The note's text in front of its "## Measured on the GPU" heading is kept; everything from that heading on is rewritten.
--small: tiny shapes, a rehearsal of the script itself (its numbers mean nothing).  --bench-lines: a file of
"label<TAB>bench.py JSON line" rows (`bench.py --only mala` on this commit and on its parent, alternated, same box).
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bayes-kit_amd"), os.path.join(ROOT, "tools")]

import numpy as np
import torch

import bayes_kit_amd as bk
from bench_config import D_CFG3, SEED_CFG3
from warmup_cfg3 import alternate, section, spread, timed

EPS_HAND = 1e-4  # (timing only: inside the stability limit 2 / lam_max of the unpreconditioned sampler)


def parent_ops(path):
    """An Ops object whose library is another build of libbkhip.so (the parent commit's), loaded beside this one."""
    lib = ctypes.CDLL(os.path.abspath(path))
    for name, argtypes in bk._lib.SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:  # (entry points this commit adds are not in it)
            fn.argtypes = argtypes
            fn.restype = bk._lib._RESTYPE.get(name, ctypes.c_int)
    ops = bk._lib.Ops()
    ops.lib = lib
    return ops


def kernel_cost(C, D, n, rounds, parent):
    lam = torch.logspace(0, 4, D, dtype=torch.float64)
    v = torch.linspace(0.9, 1.1, D, dtype=torch.float64)  # (timing only: any vector takes the preconditioned kernels)
    out = {"shape": [D, C], "draws_per_round": n, "unpreconditioned_side": "parent library" if parent else "this library"}
    for path, key in (("opaque", "model_opaque_ms_per_draw"), ("auto", "inlined_ms_per_draw")):
        def mk(ops=None, **kw):
            kw = dict(kw, ops=ops) if ops is not None else kw
            model = bk.DiagGaussian(lam, ops=ops) if ops is not None else bk.DiagGaussian(lam)
            return bk.MALA(model, EPS_HAND, chains=C, seed=SEED_CFG3, path=path, **kw)

        ss = {"plain": mk(parent), "plain (A/A)": mk(parent), "precond_diag": mk(precond_diag=v)}
        if parent is not None:
            ss["plain, this library"] = mk()
        assert all(s._two_pass and s._prefetch for s in ss.values())
        assert ss["precond_diag"]._sep_step == (path == "auto")
        w = alternate({k: s.sample for k, s in ss.items()}, n, rounds)
        w["aa_spread_percent"] = spread(w, "plain (A/A)", "plain")
        w["precond_over_plain_percent"] = round((w["precond_diag"]["ms"] / w["plain"]["ms"] - 1.0) * 100.0, 2)
        w["target_percent"] = round(w["aa_spread_percent"] + 5.0, 2)
        w["target_met"] = bool(w["precond_over_plain_percent"] <= w["target_percent"])
        out[key] = w
        del ss
        torch.cuda.empty_cache()
    return out


def overhead(C, D, n):
    lam = torch.logspace(0, 4, D, dtype=torch.float64)
    row = {"shape": f"{D} x {C}"}
    for label, kw in (("two-pass (default)", dict()), ("step by step", dict(two_pass=False))):
        s = bk.MALA(bk.DiagGaussian(lam), EPS_HAND, chains=C, seed=SEED_CFG3, **kw)
        for _ in range(5):
            s.sample()
        row[f"plain_ms_per_draw, {label}"] = round(1e3 * timed(s.sample, n), 4)
        row[f"plain_ms_per_draw, {label} (A/A)"] = round(1e3 * timed(s.sample, n), 4)
        row[f"graph, {label}"] = bool(s._use_graph)
        del s
        torch.cuda.empty_cache()
    b = bk.MALA(bk.DiagGaussian(lam), EPS_HAND, chains=C, seed=SEED_CFG3)
    for _ in range(5):
        b.sample()
    k = min(n, 19)
    torch.cuda.synchronize()
    t = time.perf_counter()
    b.warmup(k)  # fewer than 20 draws: statistic + host read, no window
    torch.cuda.synchronize()
    row["warmup_ms_per_draw_step_size_only"] = round(1e3 * (time.perf_counter() - t) / k, 4)
    t = time.perf_counter()
    b.warmup(2 * n)  # a schedule of 2 n draws spends 75 % of them inside its window: + the Welford update
    torch.cuda.synchronize()
    row["warmup_ms_per_draw_75pc_in_window"] = round(1e3 * (time.perf_counter() - t) / (2 * n), 4)
    return row


def user_gain(C, D, draws, warm_draws, scan):
    lam = torch.logspace(0, 4, D, dtype=torch.float64)
    dims = [0] + [int(round(x)) for x in np.linspace(0, D - 1, 16)]  # theta[0], then 16 spread dimensions (0 .. D-1)
    dims_t = torch.tensor(dims, device="cuda")
    rows = []
    for eps in list(scan) + [None]:
        s = bk.MALA(bk.DiagGaussian(lam), 1e-5 if eps is None else eps, chains=C, seed=SEED_CFG3)
        row = {"variant": f"epsilon = {eps:g}, no preconditioner" if eps is not None else f"warmup({warm_draws}) from epsilon = 1e-5"}
        if eps is None:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rep = s.warmup(warm_draws)
            torch.cuda.synchronize()
            row["warmup_wall_s"] = round(time.perf_counter() - t0, 3)
            row["max_abs_v_lam_minus_1"] = round(float(np.abs(rep["precond_diag"] * lam.numpy() - 1.0).max()), 4)
            row["alpha_last_20"] = round(float(np.mean(rep["alpha"][-20:])), 4)
            row["epsilon_at_first_window_end"] = rep["eps"][rep["window_ends"][0] - 1] if rep["window_ends"] else None
        else:
            # the hand-tuned rows start inside the target: their small steps would otherwise spend the timed draws on the
            # transient
            s._theta_dc.mul_((1.0 / torch.sqrt(lam)).to(s._theta_dc.device)[:, None])
            s.refresh_cache()
            for _ in range(5):
                s.sample()
        row["epsilon"] = float(s._epsilon)
        series = torch.empty((len(dims), draws, C), dtype=torch.float64, device="cuda")
        acc0 = float(s._accepted.item())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for n in range(draws):
            th, _ = s.sample()
            series[:, n] = th[:, dims_t].t()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        row["ms_per_draw"] = round(1e3 * el / draws, 4)
        row["accept_rate"] = round((float(s._accepted.item()) - acc0) / (draws * C), 4)
        bulk = [float(bk.ess_bulk(series[k])) for k in range(len(dims))]
        row["ess_bulk_theta0"], row["ess_bulk_min_16"] = round(bulk[0], 1), round(min(bulk[1:]), 1)
        row["ess_bulk_theta0_per_sec"] = round(bulk[0] / el, 1)
        row["ess_bulk_min_16_per_sec"] = round(min(bulk[1:]) / el, 1)
        rows.append(row)
        del s, series
        torch.cuda.empty_cache()
    hand = rows[:-1]
    best0 = max(r["ess_bulk_theta0_per_sec"] for r in hand)
    bestw = max(r["ess_bulk_min_16_per_sec"] for r in hand)
    return {"chains": C, "D": D, "draws": draws, "dims": dims, "rows": rows,
            "theta0_warmup_over_best_hand": round(rows[-1]["ess_bulk_theta0_per_sec"] / best0, 2) if best0 > 0 else None,
            "worst_of_16_warmup_over_best_hand": round(rows[-1]["ess_bulk_min_16_per_sec"] / bestw, 2) if bestw > 0 else None}


MARKER = "## Measured on the GPU"


def render(res, head):
    """`head`: the part of the note that is not measured here (stand-in ranges, resource table, disassembly diff) -- what
    the existing note holds in front of MARKER is kept, everything from MARKER on is rewritten."""
    L = [head.rstrip("\n"), "", MARKER, "",
         f"Written by `tools/mala_warmup_cfg3.py` ({res['device']}, one process, {res['date']}).  Times: host clock around a",
         "device synchronise after warming every shape; variants alternated round by round, median of the rounds; the A/A pair",
         "of a comparison is the same variant built twice.", ""]
    if res.get("bench_lines"):
        L += ["### Unpreconditioned paths: `bench.py --only mala` on this commit and on its parent, same box, alternated", "",
              "| run | value | result line |", "|---|---|---|"]
        for lab, j in res["bench_lines"]:
            L.append(f"| {lab} | {j.get('value')} | `{json.dumps(j)[:300]}` |")
        L.append("")
    kc = res["kernel_cost"]
    L += [f"### Cost of the preconditioned two-pass kernels ({kc['shape'][0]} x {kc['shape'][1]}; unpreconditioned side: "
          f"{kc['unpreconditioned_side']})", ""]
    for key, title in (("model_opaque_ms_per_draw", "model-opaque pair: gradient op + `bk_mala_step[_precond]`"),
                       ("inlined_ms_per_draw", "inlined: log-density launch + `bk_mala_step_gaussian[_precond]`")):
        w = kc[key]
        L += [f"**{title}**", "", "| variant | ms per draw (median) | rounds |", "|---|---|---|"]
        for k, r in w.items():
            if isinstance(r, dict):
                L.append(f"| {k} | {r['ms']} | {r['rounds']} |")
        L += ["", f"precond_diag over plain: {w['precond_over_plain_percent']:+.2f} %; A/A spread {w['aa_spread_percent']} %; target "
                  f"A/A + 5 % = {w['target_percent']} %: {'met' if w['target_met'] else 'MISSED'}.", ""]
    o = res["overhead"]
    L += [f"### Overhead of a warmup draw ({o['shape']})", "", "| quantity | ms per draw |", "|---|---|"]
    for k, x in o.items():
        if k != "shape":
            L.append(f"| {k} | {x} |")
    ug = res["user_gain"]
    L += ["", f"### What a user gains (config-3 target, {ug['chains']} chains, {ug['draws']} draws after the set-up; reported, not gated)",
          "", "| variant | epsilon | ms per draw | accept | ess_bulk theta[0] | ess_bulk worst of 16 | ESS/s theta[0] | ESS/s worst of 16 | "
          "warmup wall s |", "|---|---|---|---|---|---|---|---|---|"]
    for r in ug["rows"]:
        L.append(f"| {r['variant']} | {r['epsilon']:.4g} | {r['ms_per_draw']} | {r['accept_rate']} | {r['ess_bulk_theta0']} | "
                 f"{r['ess_bulk_min_16']} | {r['ess_bulk_theta0_per_sec']:.4g} | {r['ess_bulk_min_16_per_sec']:.4g} | "
                 f"{r.get('warmup_wall_s', '')} |")
    wr = ug["rows"][-1]
    L += ["", f"Adapted: max |v lam - 1| = {wr.get('max_abs_v_lam_minus_1')}, mean alpha of the last 20 warmup draws "
              f"{wr.get('alpha_last_20')}, epsilon when the first window ends {wr.get('epsilon_at_first_window_end')}.  ESS per second, "
              f"warmup row over the best hand-tuned row: theta[0] **{ug['theta0_warmup_over_best_hand']} x**, worst of 16 "
              f"**{ug['worst_of_16_warmup_over_best_hand']} x**.", "",
          f"Section wall times (s): {res['section_seconds']}", ""]
    return "\n".join(L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--parent-lib")
    ap.add_argument("--bench-lines")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mala_warmup"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/mala_warmup_cfg3.py measures on a GPU"
    small = a.small
    C, D = (1024, 64) if small else (16384, D_CFG3)
    res = {"device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "small": small}
    if a.bench_lines:
        res["bench_lines"] = []
        for line in open(a.bench_lines):
            if "\t" in line:
                lab, js = line.rstrip("\n").split("\t", 1)
                res["bench_lines"].append((lab, json.loads(js)))
    with section("kernel_cost", 240):
        res["kernel_cost"] = kernel_cost(C, D, 5 if small else 30, 2 if small else 7,
                                         parent_ops(a.parent_lib) if a.parent_lib else None)
    with section("overhead", 180):
        res["overhead"] = overhead(C, D, 10 if small else 40)
    with section("user_gain", 420):
        res["user_gain"] = user_gain(C, D, 40 if small else 1000, 40 if small else 300,
                                     (1e-4,) if small else (5e-5, 1e-4, 1.5e-4, 1.9e-4))
    res["section_seconds"] = section.times
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    head = "# MALA: diagonal preconditioner and cross-chain warmup\n"
    if os.path.exists(a.out + ".md"):
        head = open(a.out + ".md").read().split(MARKER)[0]
    with open(a.out + ".json", "w") as f:
        json.dump(res, f, indent=1)
    with open(a.out + ".md", "w") as f:
        f.write(render(res, head))
    print(json.dumps({"wrote": [a.out + ".md", a.out + ".json"], "kernel_cost": {k: v.get("precond_over_plain_percent")
                                                                                 for k, v in res["kernel_cost"].items() if isinstance(v, dict)}}))


if __name__ == "__main__":
    main()
