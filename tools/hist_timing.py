#!/usr/bin/env python3
"""bk.RunningHistogram.update beside bk.RunningMoments.update on one GPU (profiles/running_histogram.md).

    python tools/hist_timing.py [--small] [--out FILE.md]

Whole calls between device events, alternated in one process, medians of the repeats; the histogram runs under two names and
the gap between the two is the A/A spread.  Shape 1,024 x 65,536 (config 3), fp64.
  bins      512 (the default: all slots in one LDS window) and bk_hist_lds_bins() + 1 (two windows: the slab is read twice).
  data      N(0, 1) draws on the default grid of from_moments (-/+ 8 sd), and ALL CHAINS EQUAL (every lane of every
            wavefront on one counter: what the run merge in front of the LDS add is for).
  the bar   an update costs no more than RunningMoments.update at the same shape (which moves 40 D C bytes against the
            histogram's 8 D C + 8 D (B + 3)), plus the A/A spread -- on the N(0, 1) data.  The all-equal time is recorded
            with its ratio to the N(0, 1) time and has no bar.
  the rate  bk_hist_accumulate alone on its 8 D C + 8 D (B + 3) bytes, beside bk_leapfrog_kick_drift in place on its
            40 D C bytes in the same run: TB/s and the fraction of kick+drift's rate.
Before it times anything the tool checks the counts of every (bins, data) pair against the slot rule written in torch
ops on the device.  --small rehearses the script at toy sizes (its numbers are
overheads)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bayes-kit_amd")]

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


def alternate(jobs, reps, repeats):
    for fn in jobs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in jobs}
    for _ in range(repeats):
        for name, fn in jobs.items():
            ms[name].append(events_ms(fn, reps))
    return ms


def slots_on_device(x, lo, scale, B):
    """The slot rule in torch ops on the device: (x - lo) * scale as two rounded fp64 operations (no fused form exists in
    eager torch), row by row to bound the scratch."""
    out = torch.zeros((x.shape[0], B + 3), dtype=torch.int64, device=x.device)
    for d in range(x.shape[0]):
        t = (x[d] - lo[d]) * scale[d]
        s = torch.where(torch.isnan(x[d]), B + 2, torch.where(t < 0.0, 0, torch.where(t >= float(B), B + 1,
                                                                                        1 + t.clamp(0.0, float(B)).to(torch.int64))))
        out[d] = torch.bincount(s, minlength=B + 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("hist_timing.py measures on a GPU; none is visible")
    ops = bk._lib.default_ops()
    dev = ops.device
    D, C = (64, 4096) if a.small else (1024, 65536)
    reps, repeats = (3, 3) if a.small else (10, 7)
    L = ops.hist_lds_bins()
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    normal = torch.randn((D, C), dtype=torch.float64, device=dev, generator=g)
    equal = torch.full((D, C), 0.123, dtype=torch.float64, device=dev)
    rm = bk.RunningMoments(D, C, ops=ops)
    rho, grad = torch.randn_like(normal), torch.randn_like(normal)
    th = normal.clone()

    def moments():
        rm.update(normal, layout="dc")

    def kick_drift():
        ops.kick_drift(th, th, rho, rho, grad, None, 1e-3, False, 0.0, True, 1e-3)

    lines = [f"device: {torch.cuda.get_device_name(0)}; D = {D}, C = {C}; {repeats} repeats of {reps} calls, alternated, "
             f"medians; bk_hist_lds_bins() = {L}, slab = {ops.hist_slab_chains(C, D, 512)} chains at 512 bins and "
             f"{ops.hist_slab_chains(C, D, L + 1)} at {L + 1}; one box, one run", "",
             "| bins | data | histogram update ms (A / A') | A/A spread | moments update ms | histogram / moments | bar "
             "(<= 1 + A/A) | kernel ms | bytes | TB/s | kick+drift TB/s | of kick+drift |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    times = {}
    for B in (512, L + 1):
        for name, x in (("N(0, 1)", normal), ("all equal", equal)):
            h = bk.RunningHistogram(torch.full((D,), -8.0), torch.full((D,), 8.0), bins=B, ops=ops)
            h.update(x, layout="dc")
            want = slots_on_device(x, h.lo, h.scale, B)
            assert torch.equal(h.counts(), want), (B, name, "counts differ from the slot rule")
            counts = torch.zeros((D, B + 3), dtype=torch.int64, device=dev)
            jobs = {"hist A": lambda: h.update(x, layout="dc"), "moments": moments, "hist A2": lambda: h.update(x, layout="dc"),
                    "kernel": lambda: ops.hist_accumulate(x, h.lo, h.scale, B, counts), "kick_drift": kick_drift}
            ms = alternate(jobs, reps, repeats)
            med = {k: statistics.median(v) for k, v in ms.items()}
            hist = 0.5 * (med["hist A"] + med["hist A2"])
            aa = abs(med["hist A"] - med["hist A2"]) / hist
            ratio = hist / med["moments"]
            nbytes = 8 * D * C + 8 * D * (B + 3)
            tbs = nbytes / (med["kernel"] * 1e-3) / 1e12
            kd = 40.0 * D * C / (med["kick_drift"] * 1e-3) / 1e12
            verdict = ("met" if ratio <= 1.0 + aa else "MISSED") if name == "N(0, 1)" else "no bar"
            times[(B, name)] = hist
            lines.append(f"| {B} | {name} | {med['hist A']:.4f} / {med['hist A2']:.4f} | {100 * aa:.2f} % | {med['moments']:.4f} | "
                         f"{ratio:.3f} | {verdict} | {med['kernel']:.4f} | {nbytes / 1e6:.0f} MB | {tbs:.2f} | {kd:.2f} | "
                         f"{tbs / kd:.2f} |")
            print(lines[-1], flush=True)
            print("  repeats (ms): " + "; ".join(f"{k} {[round(v, 4) for v in vs]}" for k, vs in ms.items()), flush=True)
    lines.append("")
    for B in (512, L + 1):
        lines.append(f"all equal / N(0, 1) at {B} bins: {times[(B, 'all equal')] / times[(B, 'N(0, 1)')]:.3f}")
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
