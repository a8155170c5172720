"""The differential-evolution move on a posterior with two separated modes: 0.3 of the mass at (-3, -3), 0.7 at (3, 3), every
second walker started in each.  The stretch move keeps every walker in the mode it started in, so the ensemble reports the
0.5 / 0.5 split of its start for ever; a differential-evolution step along the difference of two walkers that sit in
different modes carries a third one across, most often on the draws with gamma = 1 (jump_every), and the ensemble finds
0.3 / 0.7 without a temperature ladder.  (Both modes have to be populated: a mode no walker has found is found by
bk.TemperedDifferentialEvolution or bk.TemperedStretcher, not by this.)
Run on an MI355X:  python examples/multimodal_differential_evolution.py"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "bayes-kit_amd")]

import numpy as np
import torch

import bayes_kit_amd as bk

walkers, draws, seed = 512, 400, 2025
c_prior = -math.log(2 * math.pi * 16.0)  # prior N(0, 4^2 I)
c_lik = -math.log(2 * math.pi * 0.25)    # the likelihood's two components: N(., 0.5^2 I)


def sq_dist(Theta, mu):
    return ((Theta - mu) ** 2).sum(dim=1)


model = bk.TorchPriorLikelihoodModel(
    lambda Theta: c_prior - sq_dist(Theta, 0.0) / 32.0,
    lambda Theta: torch.logaddexp(math.log(0.3) + c_lik - 2.0 * sq_dist(Theta, -3.0),
                                  math.log(0.7) + c_lik - 2.0 * sq_dist(Theta, 3.0)), 2)

init = 0.3 * np.random.default_rng(seed).normal(size=(walkers, 2))
init[0::2] -= 3.0
init[1::2] += 3.0
de = bk.DifferentialEvolution(model, walkers=walkers, init=init, seed=seed, jump_every=10)
plain = bk.Stretcher(model, walkers=walkers, init=init, seed=seed)

for _ in range(draws // 2):  # burn-in
    de.sample()
    plain.sample()
share_d, share_p = [], []
for _ in range(draws // 2):
    share_d.append((de.sample()[0][:, 0] > 0).double().mean())
    share_p.append((plain.sample()[0][:, 0] > 0).double().mean())
print(f"share of walkers in the major mode (0.7 of the mass): Stretcher {float(torch.stack(share_p).mean()):.3f}, "
      f"DifferentialEvolution {float(torch.stack(share_d).mean()):.3f}")
print(f"acceptance: Stretcher {plain.accept_rate():.3f}, DifferentialEvolution {de.accept_rate():.3f} "
      f"(gamma = {de.gamma:.3f}, 1.0 on every {de.jump_every}th draw)")
