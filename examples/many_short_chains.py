"""Many short chains: K superchains of M chains each, started from K over-dispersed points, and nested R-hat (Margossian
et al., "Nested R-hat: assessing the convergence of Markov chain Monte Carlo when running many short chains") telling when the
run has forgotten its starts -- after a handful of draws per chain, where R-hat has nothing to say yet.
Run on an MI355X:  python examples/many_short_chains.py"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "bayes-kit_amd")]

import numpy as np
import torch

import bayes_kit_amd as bk

D, K, M, L, max_draws = 64, 128, 128, 4, 200                    # 16,384 chains
starts = 5.0 * np.random.default_rng(0).normal(size=(K, D))  # K start points, far wider than the target
init = bk.superchain_init(starts, M)                       # chain c starts at starts[c // M]; subchains differ by their streams
model = bk.DiagGaussian(torch.logspace(0, 2, D, dtype=torch.float64))
pilot = bk.HMCDiag(model, 0.02, L, init=init, chains=K * M, seed=1)
report = pilot.warmup(150)                                 # step size + diagonal preconditioner from all chains
# the run proper: the tuned settings, the K starts again (the pilot's chains have long left them), fresh streams
sampler = bk.HMCDiag(model, report["stepsize"], L, precond_diag=report["precond_diag"], init=init, chains=K * M, seed=2)

# The paper's reading of the statistic: with stationary, independent subchains the superchain means differ by no more than
# Monte-Carlo noise, B / W is about 1 / (M * ESS per chain), so nested R-hat sits below sqrt(1 + 1 / M) from the very first
# draw; a threshold sqrt(1 + 1 / M + eps) allows a squared bias of eps posterior variances on top.  It tightens as M grows
# -- more chains per superchain buy a sharper test, not more draws per chain.
eps = 0.01
threshold = math.sqrt(1.0 + 1.0 / M + eps)
print(f"eps {report['stepsize']:.3f} after warmup; threshold sqrt(1 + 1/M + {eps}) = {threshold:.4f} for M = {M} "
      f"(M = 8: {math.sqrt(1 + 1 / 8 + eps):.4f}, M = 1,024: {math.sqrt(1 + 1 / 1024 + eps):.4f})")
# The moments cover the latest `window` draws only: the question is whether the chains' CURRENT distribution still knows its
# start, and a mean over the transient would answer another one (here a trajectory takes theta to about -theta, so the mean of
# two consecutive draws nearly cancels the start while the state itself still carries it).
window = 1
moments = bk.RunningMoments(D, K * M)
for draw in range(1, max_draws + 1):
    theta, _ = sampler.sample()
    if (draw - 1) % window == 0:
        moments.reset()
    moments.update(theta)
    if draw % window:
        continue
    worst = float(np.max(moments.nested_rhat(M)))          # defined from the first draw on
    if draw <= 5 or draw % 10 == 0 or worst < threshold:
        print(f"draw {draw:3d}: max_d nested R-hat = {worst:.4f}")
    if worst < threshold:
        print(f"below the threshold after {draw} draws per chain ({draw * K * M:,} draws in all)")
        break
else:
    print(f"still above the threshold after {max_draws} draws")
