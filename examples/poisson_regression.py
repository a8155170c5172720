"""Poisson regression with an exposure offset on the library's own kernels: counts y_n ~ Poisson(exposure_n * exp(x_n . theta)),
theta ~ N(0, 2^2 I).  bk.GLM's gradient for ALL chains is two fp64 MFMA GEMMs with the Poisson cell rule between them; HMC
warmup tunes the step size and a diagonal preconditioner from all chains, then every coefficient's median and 90 % interval
come from a fixed-memory histogram fed after every draw (no draw is stored).
Run on an MI355X:  python examples/poisson_regression.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "bayes-kit_amd")]

import numpy as np

import bayes_kit_amd as bk

N, D, chains, window, draws = 20_000, 12, 2048, 20, 100
g = np.random.default_rng(3)
X = np.column_stack([np.ones(N), g.normal(size=(N, D - 1)) / 2])   # an intercept and eleven covariates
theta_true = np.concatenate([[-1.0], g.normal(size=D - 1) / 2])
exposure = g.uniform(0.5, 20.0, size=N)                            # e.g. person-years at risk
y = g.poisson(exposure * np.exp(X @ theta_true))

model = bk.GLM(X, y, "poisson", prior_scale=2.0, offset=np.log(exposure))   # eta = x . theta + log exposure
sampler = bk.HMCDiag(model, 0.01, 16, chains=chains, seed=1)
report = sampler.warmup(200)                                       # step size + diagonal preconditioner from all chains
print(f"warmup: step size {report['stepsize']:.4f}")

moments = bk.RunningMoments(D, chains)                             # a short window: where the posterior is, and how wide
for _ in range(window):
    theta, _ = sampler.sample()
    moments.update(theta)
hist = bk.RunningHistogram.from_moments(moments)

for _ in range(draws):
    theta, logp = sampler.sample()
    hist.update(theta)

median = hist.median()
lower, upper = hist.interval(0.9)
print(f"{hist.n} values per coefficient; log density of the last draw: mean {float(logp.mean()):.1f} (normalised likelihood)")
print("   d    truth |  median |     5 %     95 % | inside")
for d in range(D):
    inside = lower[d] <= theta_true[d] <= upper[d]
    print(f"{d:4d} {theta_true[d]:+8.4f} | {median[d]:+7.4f} | {lower[d]:+8.4f} {upper[d]:+8.4f} | {'yes' if inside else 'no'}")
