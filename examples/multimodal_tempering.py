"""Parallel tempering on a posterior with two separated modes: 0.3 of the mass at (-3, -3), 0.7 at (3, 3), every walker started
in the minor one.  The plain ensemble sampler never leaves it, and every convergence diagnostic then agrees on the wrong
answer; the coldest of 12 tempered rungs finds the 0.3 / 0.7 split, and the ladder gives the model evidence on the way.
Run on an MI355X:  python examples/multimodal_tempering.py"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "bayes-kit_amd")]

import numpy as np
import torch

import bayes_kit_amd as bk

walkers, draws, seed = 256, 400, 2025
c_prior = -math.log(2 * math.pi * 16.0)  # prior N(0, 4^2 I), normalised (the evidence needs the constants)
c_lik = -math.log(2 * math.pi * 0.25)    # the likelihood's two components: N(., 0.5^2 I)


def sq_dist(Theta, mu):
    return ((Theta - mu) ** 2).sum(dim=1)


model = bk.TorchPriorLikelihoodModel(
    lambda Theta: c_prior - sq_dist(Theta, 0.0) / 32.0,
    lambda Theta: torch.logaddexp(math.log(0.3) + c_lik - 2.0 * sq_dist(Theta, -3.0),
                                  math.log(0.7) + c_lik - 2.0 * sq_dist(Theta, 3.0)), 2)
# Z = 0.3 N((-3, -3); 0, 16.25 I) + 0.7 N((3, 3); 0, 16.25 I) = N((3, 3); 0, 16.25 I)
log_z = -math.log(2 * math.pi * 16.25) - 18.0 / (2 * 16.25)

betas = bk.geometric_ladder(11, 1e-3, zero=True)  # 1 ... 1e-3 in equal ratios, then 0: the prior itself
init = -3.0 + 0.3 * np.random.default_rng(seed).normal(size=(len(betas) * walkers, 2))
tempered = bk.TemperedStretcher(model, betas, walkers=walkers, init=init, seed=seed)
cold = tempered.cold_rows()  # the rows of a draw that sample the posterior itself
plain = bk.Stretcher(model, walkers=walkers, init=init[cold.cpu().numpy()], seed=seed)

for _ in range(draws // 2):  # burn-in
    tempered.sample()
    plain.sample()
tempered.reset_statistics()
share_t, share_p = [], []
for _ in range(draws // 2):
    share_t.append((tempered.sample()[0][cold, 0] > 0).double().mean())
    share_p.append((plain.sample()[0][:, 0] > 0).double().mean())
print(f"share of walkers in the major mode (0.7 of the mass): plain Stretcher {float(torch.stack(share_p).mean()):.3f}, "
      f"coldest rung of TemperedStretcher {float(torch.stack(share_t).mean()):.3f}")
print("acceptance per rung:", np.round(tempered.rung_accept_rate(), 3))
print("swap rates per pair:", np.round(tempered.swap_rate(), 3))
print(f"log evidence (stepping stones): {tempered.log_evidence()[0]:.4f}; closed form {log_z:.4f}")
ml, b = tempered.mean_log_likelihood()[0], tempered.betas
print(f"thermodynamic integration over the same rungs (trapezoid): {float(np.sum(0.5 * (ml[:-1] + ml[1:]) * (b[:-1] - b[1:]))):.4f}")
