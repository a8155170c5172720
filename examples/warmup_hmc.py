"""Cross-chain warmup: an ill-conditioned Gaussian (condition number 1e4) started from a step size that is 100 x too
small; warmup tunes the step size and a diagonal preconditioner from all chains, then the sampler samples with them.
Run on an MI355X:  python examples/warmup_hmc.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "bayes-kit_amd")]

import torch

import bayes_kit_amd as bk

D, chains, draws = 1024, 16384, 200
sampler = bk.HMCDiag(bk.DiagGaussian(torch.logspace(0, 4, D, dtype=torch.float64)), 0.006, 16, chains=chains, seed=1)
report = sampler.warmup(300)                               # step size + velocity variances, on the device
recorder = bk.DrawRecorder([0, D // 2, D - 1], draws, chains)
for _ in range(draws):
    theta, logp = sampler.sample()
    recorder.record(theta, logp)
print(f"eps {report['stepsize']:.3f} (from 0.006), accept rate {sampler.accept_rate():.2f}")
for k, v in recorder.summary().items():                    # mean, sd, MCSE, bulk / tail ESS, R-hat over all chains
    print(k, v)
