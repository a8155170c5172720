"""Cost and gain of the diagonal preconditioner and of HMCDiag.warmup on one MI355X; writes profiles/warmup_adapt.md and
profiles/warmup_adapt.json.

One process; every section runs under its own time limit (a watchdog ends the process when it is exceeded) and an error in
one ends the run -- nothing is started on the GPU after a failure.  Host clock around a device synchronise, every shape
warmed first, the variants of a comparison alternated round by round, one A/A pair per comparison to show the spread.

  precond_cost   config-3 shape (1,024 x 65,536, L = 64, eps = 0.006): the whole-draw kernel with precond_diag against the
                 same kernel with metric_diag (its HM = true instantiation), and the opaque path's refresh and finish
                 launches with and without the preconditioner
  user_gain      config-3 target at 16,384 chains: eps = 0.006 with L = 64 and L = 384 against warmup(300) from
                 eps = 0.006 with L = 16; 1,000 draws each; ESS of theta[0] and the minimum over 16 spread dimensions
  overhead       a warmup draw (statistic kernel + one host read, + Welford update inside a window) against a plain draw,
                 config 3 and config 2 (128 x 4,096, L = 32)

    python tools/warmup_cfg3.py [--small] [--bench-lines FILE] [--out profiles/warmup_adapt]

--small: tiny shapes, a rehearsal of the script itself (its numbers mean nothing).  --bench-lines: a file of
"label<TAB>bench.py JSON line" rows (this commit and its parent, alternated, same box) rendered as the "no cost when unused"
table.
"""
import argparse
import json
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bayes-kit_amd")]

import numpy as np
import torch

import bayes_kit_amd as bk
from bench_config import C_CFG3, D_CFG3, EPS_CFG3, L_CFG3, SEED_CFG3


class section:
    """`with section(name, seconds):` -- the section's wall time is recorded; past its limit the process ends."""

    times = {}

    def __init__(self, name, limit):
        self.name, self.limit = name, int(limit)

    def _expired(self, *_):
        sys.stderr.write(f"section {self.name!r} exceeded its limit of {self.limit} s: ending the run\n")
        sys.stderr.flush()
        os._exit(124)

    def __enter__(self):
        signal.signal(signal.SIGALRM, self._expired)
        signal.alarm(self.limit)
        self.t0 = time.perf_counter()
        print(f"[{self.name}] ...", flush=True)

    def __exit__(self, et, ev, tb):
        signal.alarm(0)
        torch.cuda.synchronize()
        section.times[self.name] = round(time.perf_counter() - self.t0, 2)
        print(f"[{self.name}] {section.times[self.name]} s", flush=True)
        return False  # an exception ends the run


def timed(fn, n):
    """Seconds per call of fn over n calls, host clock around a device synchronise."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def alternate(variants, n, rounds, warm=3):
    """variants: {label: fn}.  Every fn warmed, then `rounds` rounds of n calls each, the variants in turn.
    -> {label: {"ms": median, "rounds": [...]}}."""
    for fn in variants.values():
        for _ in range(warm):
            fn()
    res = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            res[k].append(1e3 * timed(fn, n))
    return {k: {"ms": round(statistics.median(v), 4), "rounds": [round(x, 4) for x in v]} for k, v in res.items()}


def spread(res, a, b):
    return round(abs(res[a]["ms"] / res[b]["ms"] - 1.0) * 100.0, 2)


def precond_cost(C, D, L, n, rounds):
    lam = torch.logspace(0, 4, D, dtype=torch.float64)
    v = torch.linspace(0.9, 1.1, D, dtype=torch.float64)  # (timing only: any non-trivial vector takes the HM / PD kernels)
    mk = lambda **kw: bk.HMCDiag(bk.DiagGaussian(lam), EPS_CFG3, L, chains=C, seed=SEED_CFG3, **kw)  # noqa: E731
    ss = {"metric_diag": mk(metric_diag=v), "metric_diag (A/A)": mk(metric_diag=v), "precond_diag": mk(precond_diag=v)}
    assert all(s._fused_draw and s._fused_zt for s in ss.values())
    out = {"shape": [D, C], "L": L, "draws_per_round": n,
           "whole_draw_ms_per_draw": alternate({k: s.sample for k, s in ss.items()}, n, rounds)}
    w = out["whole_draw_ms_per_draw"]
    w["aa_spread_percent"] = spread(w, "metric_diag (A/A)", "metric_diag")
    w["precond_over_metric_percent"] = round((w["precond_diag"]["ms"] / w["metric_diag"]["ms"] - 1.0) * 100.0, 2)
    del ss
    torch.cuda.empty_cache()
    # the opaque path's launches that differ: momentum refresh (+ kinetic energy) and the finish
    ops = bk._lib.default_ops()
    s = mk(precond_diag=v, path="opaque", prefetch_rng=False, tune_placement=False)
    rho, kin, g = s._rho_bufs[0], s._kin0_bufs[0], s._grad
    g.zero_()
    pd, m = s._pd, s._pd[0]
    kind, st, work = s._rng_kind, s._rng_state, s._rng_work
    launches = {
        "refresh metric": lambda: ops.momentum_refresh(kind, st, None, 0.0, 1.0, rho, m, kin, None, work),
        "refresh metric (A/A)": lambda: ops.momentum_refresh(kind, st, None, 0.0, 1.0, rho, m, kin, None, work),
        "refresh precond": lambda: ops.momentum_refresh_precond(kind, st, rho, pd, kin, work),
        "finish metric": lambda: ops.leapfrog_finish(rho, None, g, m, 0.003, False, kin),
        "finish metric (A/A)": lambda: ops.leapfrog_finish(rho, None, g, m, 0.003, False, kin),
        "finish precond": lambda: ops.leapfrog_finish_precond(rho, None, g, pd, 0.003, False, kin),
    }
    out["opaque_launch_ms"] = alternate(launches, n, rounds)
    return out


def user_gain(C, D, draws, warm_draws):
    lam = torch.logspace(0, 4, D, dtype=torch.float64)
    dims = [0] + [int(round(x)) for x in np.linspace(0, D - 1, 16)]  # theta[0], then 16 spread dimensions (0 .. D-1)
    dims_t = torch.tensor(dims, device="cuda")
    rows = []
    for label, L, adapt in (("eps = 0.006, L = 64", 64, False), ("eps = 0.006, L = 384", 384, False),
                            ("warmup(%d) from eps = 0.006, L = 16" % warm_draws, 16, True)):
        s = bk.HMCDiag(bk.DiagGaussian(lam), EPS_CFG3, L, chains=C, seed=SEED_CFG3)
        row = {"variant": label, "L": L}
        if adapt:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rep = s.warmup(warm_draws)
            torch.cuda.synchronize()
            row["warmup_wall_s"] = round(time.perf_counter() - t0, 3)
            row["max_abs_v_lam_minus_1"] = round(float(np.abs(rep["precond_diag"] * lam.numpy() - 1.0).max()), 4)
            row["alpha_last_20"] = round(float(np.mean(rep["alpha"][-20:])), 4)
        else:
            # the fixed-settings rows start in the stationary distribution (as tools/cfg3_trajectory_length.py does):
            # their small eps L would otherwise spend the timed draws on the transient
            s._theta_dc.mul_((1.0 / torch.sqrt(lam)).to(s._theta_dc.device)[:, None])
            for _ in range(5):
                s.sample()
        row["eps"] = float(s._stepsize)
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
        per_chain = [float(bk.ess(series[k]).clamp(min=0.0, max=float(draws)).sum()) for k in range(len(dims))]
        row["ess_bulk_theta0"], row["ess_bulk_min_16"] = round(bulk[0], 1), round(min(bulk[1:]), 1)
        row["bk_ess_theta0"], row["bk_ess_min_16"] = round(per_chain[0], 1), round(min(per_chain[1:]), 1)
        row["ess_bulk_theta0_per_100_draws_per_chain"] = round(100.0 * bulk[0] / (draws * C), 2)
        row["ess_bulk_theta0_per_sec"] = round(bulk[0] / el, 1)
        row["ess_bulk_min_16_per_sec"] = round(min(bulk[1:]) / el, 1)
        row["bk_ess_theta0_per_sec"] = round(per_chain[0] / el, 1)
        rows.append(row)
        del s, series
        torch.cuda.empty_cache()
    gain = rows[2]["ess_bulk_theta0_per_sec"] / rows[1]["ess_bulk_theta0_per_sec"]
    return {"chains": C, "D": D, "draws": draws, "dims": dims, "rows": rows,
            "ess_bulk_theta0_per_sec_warmup_over_L384": round(gain, 2), "bar_met": bool(gain >= 1.0)}


def overhead(shapes, n):
    out = []
    for name, model, C, eps, L in shapes:
        mk = lambda: bk.HMCDiag(model(), eps, L, chains=C, seed=SEED_CFG3)  # noqa: E731
        a = mk()
        for _ in range(5):
            a.sample()
        plain = 1e3 * timed(a.sample, n)
        plain2 = 1e3 * timed(a.sample, n)
        del a
        b = mk()
        for _ in range(5):
            b.sample()
        t = time.perf_counter()
        b.warmup(min(n, 19), target_accept=0.8)  # fewer than 20 draws: statistic + host read, no window
        torch.cuda.synchronize()
        stat_only = 1e3 * (time.perf_counter() - t) / min(n, 19)
        # a schedule of 2 n draws spends 75 % of them inside its window: statistic + host read + Welford update
        t = time.perf_counter()
        b.warmup(2 * n)
        torch.cuda.synchronize()
        windowed = 1e3 * (time.perf_counter() - t) / (2 * n)
        out.append({"shape": name, "plain_ms_per_draw": round(plain, 4), "plain_ms_per_draw (A/A)": round(plain2, 4),
                    "warmup_ms_per_draw_step_size_only": round(stat_only, 4),
                    "warmup_ms_per_draw_75pc_in_window": round(windowed, 4), "graph_for_plain_draws": bool(b._use_graph)})
        del b
        torch.cuda.empty_cache()
    return out


def render(res):
    L = ["# Cross-chain warmup and the diagonal preconditioner on the MI355X", "",
         f"Written by `tools/warmup_cfg3.py` ({res['device']}, one process, {res['date']}).  Times: host clock around a device",
         "synchronise after warming every shape; variants alternated round by round, median of the rounds; the A/A pair of a",
         "comparison is the same variant built twice.", ""]
    if res.get("bench_lines"):
        L += ["## No cost when unused: `bench.py --gpus 1` on this commit and on its parent, same box, alternated", "",
              "| run | value (steps/s) | ms per step |", "|---|---|---|"]
        for lab, j in res["bench_lines"]:
            L.append(f"| {lab} | {j.get('value')} | {j.get('ms_per_step')} |")
        L.append("")
    pc = res["precond_cost"]
    w = pc["whole_draw_ms_per_draw"]
    L += [f"## Cost of the preconditioned whole-draw kernel ({pc['shape'][0]} x {pc['shape'][1]}, L = {pc['L']})", "",
          "| variant | ms per draw (median) | rounds |", "|---|---|---|"]
    for k in ("metric_diag", "metric_diag (A/A)", "precond_diag"):
        L.append(f"| {k} | {w[k]['ms']} | {w[k]['rounds']} |")
    L += ["", f"precond_diag over metric_diag: {w['precond_over_metric_percent']:+.2f} %; A/A spread {w['aa_spread_percent']} %.",
          "", "The opaque path's launches that differ (ms per launch):", "", "| launch | ms (median) | rounds |", "|---|---|---|"]
    for k, r in pc["opaque_launch_ms"].items():
        L.append(f"| {k} | {r['ms']} | {r['rounds']} |")
    L += ["", res.get("registers_note", ""), ""]
    ug = res["user_gain"]
    L += [f"## What a user gains (config-3 target, {ug['chains']} chains, {ug['draws']} draws after the set-up)", "",
          "| variant | eps | ms per draw | accept | ess_bulk theta[0] (per 100 draws of a chain) | ess_bulk min of 16 | bk.ess theta[0] | "
          "ESS/s theta[0] (bulk) | ESS/s min of 16 (bulk) | warmup wall s |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in ug["rows"]:
        L.append(f"| {r['variant']} | {r['eps']:.4g} | {r['ms_per_draw']} | {r['accept_rate']} | {r['ess_bulk_theta0']} "
                 f"({r['ess_bulk_theta0_per_100_draws_per_chain']}) | {r['ess_bulk_min_16']} | {r['bk_ess_theta0']} | "
                 f"{r['ess_bulk_theta0_per_sec']:.4g} | {r['ess_bulk_min_16_per_sec']:.4g} | {r.get('warmup_wall_s', '')} |")
    wr = ug["rows"][2]
    L += ["", f"Adapted: max |v lam - 1| = {wr.get('max_abs_v_lam_minus_1')}, mean alpha of the last 20 warmup draws "
              f"{wr.get('alpha_last_20')}.  ESS per second of theta[0], warmup row over the L = 384 row: "
              f"**{ug['ess_bulk_theta0_per_sec_warmup_over_L384']} x** (bar: >= 1; {'met' if ug['bar_met'] else 'MISSED'}).", ""]
    L += ["## Overhead of a warmup draw", "",
          "| shape | plain draw ms | plain (A/A) | warmup draw, step size only | warmup draw, 75 % inside a window | plain draws replay a graph |",
          "|---|---|---|---|---|---|"]
    for r in res["overhead"]:
        L.append(f"| {r['shape']} | {r['plain_ms_per_draw']} | {r['plain_ms_per_draw (A/A)']} | {r['warmup_ms_per_draw_step_size_only']} | "
                 f"{r['warmup_ms_per_draw_75pc_in_window']} | {r['graph_for_plain_draws']} |")
    L += ["", f"Section wall times (s): {res['section_seconds']}", ""]
    return "\n".join(L)


REGISTERS_NOTE = ("Compiler report (`-Rpass-analysis=kernel-resource-usage`, gfx950) for `k_traj_q<GaussTerm<true>, HM, ZT, PD>`: "
                  "HM = true: 117 VGPRs (chain-major normals) / 114 (state-layout momentum), occupancy 4, no scratch; "
                  "PD = true: 114 / 110 VGPRs, occupancy 4, no scratch (1/v is read where the kinetic energies are summed, "
                  "not held through the trajectory loop).  The PD = false instantiations, `k_finish`, `k_finish_v2` and the "
                  "refresh kernels are instruction for instruction the parent commit's.")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--bench-lines")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warmup_adapt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/warmup_cfg3.py measures on a GPU"
    small = a.small
    res = {"device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "small": small,
           "registers_note": REGISTERS_NOTE}
    if a.bench_lines:
        res["bench_lines"] = []
        for line in open(a.bench_lines):
            if "\t" in line:
                lab, js = line.rstrip("\n").split("\t", 1)
                res["bench_lines"].append((lab, json.loads(js)))
    with section("precond_cost", 240):
        res["precond_cost"] = precond_cost(4096 if small else C_CFG3, 64 if small else D_CFG3, L_CFG3, 5 if small else 20,
                                           2 if small else 5)
    with section("user_gain", 420):
        res["user_gain"] = user_gain(512 if small else 16384, 64 if small else D_CFG3, 40 if small else 1000,
                                     40 if small else 300)
    with section("overhead", 240):
        lam3 = torch.logspace(0, 4, D_CFG3, dtype=torch.float64)
        shapes = [("config 3: 1024 x 65536, L = 64", lambda: bk.DiagGaussian(lam3), 2048 if small else C_CFG3, EPS_CFG3, L_CFG3),
                  ("config 2: 128 x 4096, L = 32", lambda: bk.IsoGaussian(128), 4096, 0.05, 32)]
        res["overhead"] = overhead(shapes, 10 if small else 40)
    res["section_seconds"] = section.times
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out + ".json", "w") as f:
        json.dump(res, f, indent=1)
    with open(a.out + ".md", "w") as f:
        f.write(render(res))
    print(json.dumps({"wrote": [a.out + ".md", a.out + ".json"], "gain": res["user_gain"]["ess_bulk_theta0_per_sec_warmup_over_L384"]}))


if __name__ == "__main__":
    main()
