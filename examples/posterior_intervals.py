"""Medians and 90 % credible intervals of EVERY coordinate without storing a draw: HMC warmup, moments during a short window,
a histogram grid from the moments, then one fixed-memory histogram per coordinate fed after every draw.  The target is a
diagonal Gaussian, so the closed form is printed next to the estimate.
Run on an MI355X:  python examples/posterior_intervals.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "bayes-kit_amd")]

import numpy as np
import torch

import bayes_kit_amd as bk

D, chains, window, draws = 256, 16384, 20, 100
lam = torch.logspace(0, 2, D, dtype=torch.float64)             # precisions: posterior sd from 1 down to 0.1
sampler = bk.HMCDiag(bk.DiagGaussian(lam), 0.05, 16, chains=chains, seed=1)
sampler.warmup(200)                                            # step size + diagonal preconditioner from all chains

moments = bk.RunningMoments(D, chains)                         # a short window: where the posterior is, and how wide
for _ in range(window):
    theta, _ = sampler.sample()
    moments.update(theta)
hist = bk.RunningHistogram.from_moments(moments)               # mean -/+ 8 sd in 512 bins: a bin is 1/32 sd

for _ in range(draws):                                         # D x 515 counters, whatever chains x draws is
    theta, _ = sampler.sample()
    hist.update(theta)

median = hist.median()
lower, upper = hist.interval(0.9)
sd = 1.0 / np.sqrt(lam.numpy())
width = np.diff(hist.edges()[:, :2], axis=1)[:, 0]
print(f"{hist.n} values per coordinate, {hist.bins} bins, on the grid: {hist.coverage().min():.6f} at least")
print("   d      sd |  median (0) |   5 %    closed form |  95 %    closed form | bin width")
for d in list(range(0, D, D // 8)) + [D - 1]:
    print(f"{d:4d} {sd[d]:7.4f} | {median[d]:+11.5f} | {lower[d]:+8.4f} {-1.6449 * sd[d]:+8.4f}     | "
          f"{upper[d]:+8.4f} {1.6449 * sd[d]:+8.4f}     | {width[d]:.5f}")
err = np.maximum(np.abs(lower + 1.6449 * sd), np.abs(upper - 1.6449 * sd)) / sd
print(f"largest error of an interval end over all {D} coordinates: {err.max():.4f} posterior sd")
