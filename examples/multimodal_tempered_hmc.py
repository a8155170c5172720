"""Tempered HMC on a posterior with two separated modes: 0.3 of the mass at (-3, -3), 0.7 at (3, 3), every chain started in the
minor one.  Plain HMC never leaves it; the coldest of 12 tempered rungs finds the 0.3 / 0.7 split, and the ladder gives the
model evidence on the way.  Every rung integrates with its own step size, tuned by warmup() from that rung's acceptance.
Run on an MI355X:  python examples/multimodal_tempered_hmc.py"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "bayes-kit_amd")]

import numpy as np
import torch

import bayes_kit_amd as bk

chains, draws, steps, seed = 256, 400, 4, 2025
c_prior = -math.log(2 * math.pi * 16.0)  # prior N(0, 4^2 I), normalised (the evidence needs the constants)
c_lik = -math.log(2 * math.pi * 0.25)    # the likelihood's two components: N(., 0.5^2 I)


def sq_dist(Theta, mu):
    return ((Theta - mu) ** 2).sum(dim=1)


# the two parts are tempered separately: their gradients come from autograd (log_prior_gradient, log_likelihood_gradient)
model = bk.TorchPriorLikelihoodModel(
    lambda Theta: c_prior - sq_dist(Theta, 0.0) / 32.0,
    lambda Theta: torch.logaddexp(math.log(0.3) + c_lik - 2.0 * sq_dist(Theta, -3.0),
                                  math.log(0.7) + c_lik - 2.0 * sq_dist(Theta, 3.0)), 2)
# Z = 0.3 N((-3, -3); 0, 16.25 I) + 0.7 N((3, 3); 0, 16.25 I) = N((3, 3); 0, 16.25 I)
log_z = -math.log(2 * math.pi * 16.25) - 18.0 / (2 * 16.25)

betas = bk.geometric_ladder(11, 1e-3, zero=True)  # 1 ... 1e-3 in equal ratios, then 0: the prior itself
init = -3.0 + 0.3 * np.random.default_rng(seed).normal(size=(len(betas) * chains, 2))
# a first guess: 0.45 standard deviations of a mode at every rung (a mode of rung t has precision 4 beta_t + 1/16)
eps = 0.45 / np.sqrt(4.0 * betas + 1.0 / 16.0)
tempered = bk.TemperedHMC(model, betas, eps, steps, init=init, chains=chains, seed=seed)
cold = tempered.cold_rows()  # the rows of a draw that sample the posterior itself
plain = bk.HMCDiag(model, float(eps[0]), steps, init=init[cold.cpu().numpy()], seed=seed, chains=chains)

report = tempered.warmup(draws // 2, target_accept=0.8)  # burn-in that tunes every rung's step size; swaps go on
for _ in range(draws // 2):
    plain.sample()
print("step sizes per rung after warmup:", np.round(report["stepsizes"], 3))
share_t, share_p = [], []
for _ in range(draws // 2):
    share_t.append((tempered.sample()[0][cold, 0] > 0).double().mean())
    share_p.append((plain.sample()[0][:, 0] > 0).double().mean())
print(f"share of chains in the major mode (0.7 of the mass): plain HMCDiag {float(torch.stack(share_p).mean()):.3f}, "
      f"coldest rung of TemperedHMC {float(torch.stack(share_t).mean()):.3f}")
print("acceptance per rung:", np.round(tempered.rung_accept_rate(), 3))
print("swap rates per pair:", np.round(tempered.swap_rate(), 3))
print(f"log evidence (stepping stones): {tempered.log_evidence()[0]:.4f}; closed form {log_z:.4f}")
