"""Divergent transitions and E-BFMI of HMC on Neal's funnel, tracked on the GPU without keeping a draw.  A step size of 0.5
accepts 60 % of its proposals and looks healthy; the tracker shows trajectories blowing up, where they start (deep in the
neck, v << 0) and how little of the energy distribution a transition explores.  Then the same after warmup().
Run on an MI355X:  python examples/funnel_divergences.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "bayes-kit_amd")]

import numpy as np
import torch

import bayes_kit_amd as bk

chains, draws = 256, 40


def report(sampler, title, stepsize):
    energy = sampler.track_energy(threshold=1000.0, capture=1024)   # from the next draw on; nothing is read back per draw
    v_sum = 0.0
    for _ in range(draws):
        theta, _ = sampler.sample()
        v_sum += float(theta[:, 0].mean())
    states = energy.divergent_states()
    per_chain = energy.divergences_per_chain.cpu().numpy()
    ebfmi = energy.ebfmi().cpu().numpy()
    print(f"-- {title}: step size {stepsize:.4f}, accept rate {sampler.accept_rate():.3f}")
    print(f"   {energy.divergences()} divergent of {energy.transitions} transitions ({100 * energy.divergence_rate():.2f} %), "
          f"{energy.nan_transitions()} with a NaN energy error; from {int((per_chain > 0).sum())} chains, "
          f"one of them {int(per_chain.max())} times")
    if states["stored"]:
        v = states["theta"][:, 0].cpu().numpy()
        print(f"   they start at v = {v.mean():+.2f} on average (min {v.min():+.2f}, max {v.max():+.2f}); "
              f"all states of the run: {v_sum / draws:+.2f}")
        first = ", ".join(f"chain {int(c)} draw {int(d)} (dH {e:.3g})" for c, d, e in
                          zip(states["chain"][:4], states["draw"][:4], states["energy_error"][:4]))
        print(f"   the first of {states['stored']} kept: {first}")
    print(f"   E-BFMI pooled over the chains {energy.ebfmi_pooled():.3f}; per chain: median {np.nanmedian(ebfmi):.3f}, "
          f"below 0.3 in {int((ebfmi < 0.3).sum())} of {chains} chains")
    sampler.untrack_energy()


sampler = bk.HMCDiag(bk.Funnel(11), 0.5, 8, chains=chains, seed=5, path="opaque")
report(sampler, "as configured", 0.5)

rep = sampler.warmup(300)                                           # step size and preconditioner from all chains
print(f"warmup: step size {rep['stepsize']:.4f}, {rep['nan_chains']} NaN energy errors on the way")
report(sampler, "after warmup", rep["stepsize"])
