#!/usr/bin/env python3
"""Nested R-hat beside R-hat on the same moments, one GPU, one process (profiles/nested_rhat.md).

    python tools/nested_rhat_timing.py [--small] [--out FILE.md]

Moments of D = 1,024 x C = 65,536 chains (1 GiB of mean and M2: past the Infinity Cache), n = 30 draws.  Per
M in {2, 64, 1,024}: whole calls of ``RunningMoments.nested_rhat(M)`` (A) and ``RunningMoments.rhat()`` (B) between HIP
events, warm, alternated A/B/A/B over the repeats, and a second interleaved series of A for the A/A spread; then
``bk_superchain_moments`` alone, its rate on the 24 D C + 16 D K bytes it moves (16 D C + 16 D K at n = 1) in TB/s and as a
fraction of the kick+drift kernel's rate the README quotes.  The bar: nested_rhat no slower than rhat() at each M beyond
the A/A spread.  --small rehearses the script at a toy size (its numbers are overheads)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bayes-kit_amd")]

import torch  # noqa: E402

import bayes_kit_amd as bk  # noqa: E402

KICK_DRIFT_TBS = (6.2, 6.5)  # README: the kick+drift kernel at config 3


def events_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("nested_rhat_timing.py measures on a GPU; none is visible")
    ops = bk._lib.default_ops()
    D, C, n = (64, 4096, 30) if a.small else (1024, 65536, 30)
    reps, repeats = (3, 3) if a.small else (10, 7)
    g = torch.Generator(device=ops.device)
    g.manual_seed(1)
    rm = bk.RunningMoments(D, C, ops=ops)
    rm.mean.copy_(torch.randn((D, C), dtype=torch.float64, device=ops.device, generator=g))
    rm.m2.copy_(torch.rand((D, C), dtype=torch.float64, device=ops.device, generator=g) * (n - 1))
    rm.n = n
    lines = [f"device: {torch.cuda.get_device_name(0)}; D = {D}, C = {C}, n = {n}; {repeats} repeats of {reps} calls, "
             "medians; one box, one run", "",
             "| M | launch | nested_rhat ms | rhat ms | nested / rhat | A/A spread | kernel ms | bytes | TB/s | of kick+drift |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for M in (2, 64, 1024):
        K = C // M
        A = lambda: rm.nested_rhat(M)  # noqa: E731
        B = lambda: rm.rhat()          # noqa: E731
        s = torch.empty((D, K), dtype=torch.float64, device=ops.device)
        w = torch.empty_like(s)
        kern = lambda: ops.superchain_moments(rm.mean, rm.m2, n, M, s, w)  # noqa: E731
        for f in (A, B, kern):
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        ms = {"A": [], "B": [], "A2": [], "k": []}
        for _ in range(repeats):
            ms["A"].append(events_ms(A, reps))
            ms["B"].append(events_ms(B, reps))
            ms["A2"].append(events_ms(A, reps))
            ms["k"].append(events_ms(kern, reps))
        med = {k: statistics.median(v) for k, v in ms.items()}
        aa = abs(med["A"] - med["A2"]) / med["A"]
        nbytes = 24 * D * C + 16 * D * K
        tbs = nbytes / (med["k"] * 1e-3) / 1e12
        launch = "butterfly" if M <= 64 else "workgroup"
        lines.append(f"| {M} | {launch} | {med['A']:.4f} | {med['B']:.4f} | {med['A'] / med['B']:.3f} | {100 * aa:.2f} % | "
                     f"{med['k']:.4f} | {nbytes / 1e6:.0f} MB | {tbs:.2f} | {tbs / KICK_DRIFT_TBS[1]:.2f}-{tbs / KICK_DRIFT_TBS[0]:.2f} |")
        print(lines[-1], flush=True)
        print(f"  repeats (ms): nested {[round(x, 4) for x in ms['A']]} rhat {[round(x, 4) for x in ms['B']]} "
              f"kernel {[round(x, 4) for x in ms['k']]}", flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
