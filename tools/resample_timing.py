#!/usr/bin/env python3
"""Whole calls of bk_resample_ordered (systematic, stratified) beside bk_resample_indices (multinomial: numpy's choice, one
wavefront whose lane 0 runs the cumulative sum; csrc/bk_smc.hip, unchanged) on one GPU (profiles/resample_ordered.md).

    python tools/resample_timing.py [--small] [--out FILE.json] [--md FILE.md]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/resample_timing.py --launches      (per-launch times, a run of its own)
    python tools/resample_timing.py --stats DIR/.../*_kernel_stats.csv --out FILE.json --md FILE.md   (adds them to the report)

n = m = 2,048, 65,536 and 1,048,576 random weights, one process, the four jobs alternated between device events:
bk_resample_indices under two names (the A/A pair), bk_resample_ordered in both modes.  The condition: at 65,536 and at
1,048,576 each ordered call is faster than the multinomial one; at 2,048 the times are recorded and no bar is set.  For
information: bk_leapfrog_kick_drift's rate in place at 65,536 x 256 (40 D C bytes), against which the scan launches' compulsory
bytes per second are set -- max 8 n, tile sums 8 n, carries 16 n / 2,048, tile scan 16 n, search 8 n + 12 m.
--small rehearses the script at toy sizes (its numbers are overheads)."""
import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bayes-kit_amd")]

import torch  # noqa: E402

import bayes_kit_amd as bk  # noqa: E402

TILE = 2048
LAUNCH_BYTES = {"k_ro_max": lambda n, m: 8.0 * n, "k_ro_tile": lambda n, m: 8.0 * n + 8.0 * n / TILE,
                "k_ro_carry": lambda n, m: 16.0 * n / TILE, "k_ro_scan": lambda n, m: 16.0 * n + 8.0 * n / TILE,
                "k_ro_search": lambda n, m: 8.0 * n + 12.0 * m}


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


def problem(ops, n):
    dev = ops.device
    g = torch.Generator(device=dev).manual_seed(n)
    w = torch.rand(n, dtype=torch.float64, device=dev, generator=g) ** 3 + 1e-6
    u = torch.rand(n, dtype=torch.float64, device=dev, generator=g)
    cdf = torch.empty(n, dtype=torch.float64, device=dev)
    work = torch.empty(ops.resample_ordered_work_bytes(n), dtype=torch.uint8, device=dev)
    idx = torch.empty(n, dtype=torch.int32, device=dev)
    lib = bk._lib
    return {"multinomial A": lambda: ops.resample_indices(w, u, cdf, idx),
            "multinomial A'": lambda: ops.resample_indices(w, u, cdf, idx),
            "systematic": lambda: ops.resample_ordered(w, u, lib.BK_RESAMPLE_SYSTEMATIC, 0, n, work, idx),
            "stratified": lambda: ops.resample_ordered(w, u, lib.BK_RESAMPLE_STRATIFIED, 0, n, work, idx)}


def time_calls(ops, n, repeats):
    jobs = problem(ops, n)
    reps = max(3, min(200, (1 << 22) // n))   # (the multinomial call takes ~8 ns per particle: ~30 ms per timed block at least)
    out = alternate(jobs, reps, repeats)
    a, a2 = out["multinomial A"]["median"], out["multinomial A'"]["median"]
    base = min(a, a2)
    out["summary"] = {"n": n, "reps_per_block": reps, "AA_median_difference": abs(a - a2) / a,
                      "multinomial_over_systematic": base / out["systematic"]["median"],
                      "multinomial_over_stratified": base / out["stratified"]["median"]}
    if n >= 65536:
        ok = max(out["systematic"]["median"], out["stratified"]["median"]) < base
        out["summary"]["condition"] = "hit" if ok else "MISSED"
    return out


def kick_drift_rate(ops, C, D, reps, repeats):
    dev = ops.device
    th, rho, grad = (torch.zeros((D, C), dtype=torch.float64, device=dev) for _ in range(3))
    out = alternate({"kick_drift": lambda: ops.kick_drift(th, th, rho, rho, grad, None, 1e-3, False, 0.0, True, 1e-3)}, reps, repeats)
    r = out["kick_drift"]
    r.update(C=C, D=D, bytes=40.0 * D * C, TB_per_s=40.0 * D * C / (r["median"] * 1e-3) / 1e12)
    return r


def read_stats(path, n, m):
    """rocprofv3's *_kernel_stats.csv of a --launches run -> {launch: {calls, mean_us, bytes, GB_per_s}}."""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            for k, nbytes in LAUNCH_BYTES.items():
                if k + "<" in name or k + "(" in name or name.endswith(k):
                    calls = int(row["Calls"])
                    mean_us = float(row["TotalDurationNs"]) / calls / 1e3
                    e = out.setdefault(k, {"calls": 0, "total_us": 0.0})
                    e["calls"] += calls
                    e["total_us"] += mean_us * calls
    for k, e in out.items():
        e["mean_us"] = e.pop("total_us") / e["calls"]
        e["bytes"] = LAUNCH_BYTES[k](n, m)
        e["GB_per_s"] = e["bytes"] / (e["mean_us"] * 1e-6) / 1e9
    return out


def markdown(res):
    L = ["| n = m | multinomial (`bk_resample_indices`) | systematic | stratified | multinomial / systematic | multinomial / stratified | A/A | condition |",
         "|---|---|---|---|---|---|---|---|"]
    for c in res["calls"]:
        s = c["summary"]
        mn = min(c["multinomial A"]["median"], c["multinomial A'"]["median"])
        L.append(f"| {s['n']:,} | {mn * 1e3:.1f} us | {c['systematic']['median'] * 1e3:.1f} us | {c['stratified']['median'] * 1e3:.1f} us | "
                 f"{s['multinomial_over_systematic']:.2f} x | {s['multinomial_over_stratified']:.2f} x | "
                 f"{100 * s['AA_median_difference']:.2f} % | {s.get('condition', 'no bar')} |")
    if "kick_drift" in res:
        k = res["kick_drift"]
        L += ["", f"`bk_leapfrog_kick_drift` in place at {k['C']:,} x {k['D']}: {k['median']:.4f} ms = {k['TB_per_s']:.2f} TB/s."]
    if "launches" in res:
        L += ["", f"Per launch at n = m = {res['launches_n']:,} (kernel trace, a run of its own):", "",
              "| launch | mean | compulsory bytes | rate | of kick+drift's |", "|---|---|---|---|---|"]
        for k, e in res["launches"].items():
            share = f"{e['GB_per_s'] / (res['kick_drift']['TB_per_s'] * 1e3):.3f}" if "kick_drift" in res else "-"
            L.append(f"| `{k}` | {e['mean_us']:.2f} us | {e['bytes'] / 1e6:.2f} MB | {e['GB_per_s']:.0f} GB/s | {share} |")
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--launches", action="store_true", help="only run the ordered calls at the largest size (for a kernel trace)")
    ap.add_argument("--stats", default=None, help="a kernel-stats CSV of a --launches run: no GPU work, merged into --out")
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    sizes = (256, 4099) if args.small else (2048, 65536, 1048576)
    if args.stats:
        res = json.load(open(args.out))
        res["launches_n"] = sizes[-1]
        res["launches"] = read_stats(args.stats, sizes[-1], sizes[-1])
    else:
        ops = bk._lib.default_ops()
        if args.launches:
            jobs = problem(ops, sizes[-1])
            for _ in range(50):
                jobs["systematic"]()
                jobs["stratified"]()
            torch.cuda.synchronize()
            return
        res = {"device": torch.cuda.get_device_name(0), "calls": []}
        for n in sizes:
            res["calls"].append(time_calls(ops, n, 3 if args.small else 7))
            s = res["calls"][-1]["summary"]
            print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in s.items()}), flush=True)
        res["kick_drift"] = kick_drift_rate(ops, 1024, 16, 3, 2) if args.small else kick_drift_rate(ops, 65536, 256, 20, 7)
    text = markdown(res)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    if args.md:
        with open(args.md, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
