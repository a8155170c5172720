"""ms per DRGHMC draw of the AR(1) state-space model (examples/state_space_model.py) at D = 101 x 32,768 chains, three ways on one
box, alternated round by round: the traced PyTorch function (form="chain", one launch per trajectory), the neighbour lanes source
(examples/state_space_neighbour_lanes.py: one launch per proposal) and the same source with path="opaque" (gradient op per
leapfrog step).  Two sampler settings: the example's and config 4's.  Prints one JSON object (and writes it with --out).

    python tools/ssm_neighbour_timing.py [--chains 32768] [--rounds 5] [--draws 40] [--out profiles/...json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "bayes-kit_amd"), os.path.join(ROOT, "examples")]

import torch

import bayes_kit_amd as bk
from state_space_neighbour_lanes import EXAMPLE_ARGS, ms_per_draw, problem

CFG4_ARGS = (3, [0.2, 0.05, 0.0125], [10, 40, 160], 0.1)  # bench_secondary.py: config 4's sampler


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=32768)
    ap.add_argument("--T", type=int, default=99)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--draws", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    _, log_density, neighbour_model, init = problem(a.T, dev)
    D = a.T + 2
    traced = bk.TorchModel(log_density, D, compile=True)
    assert traced.compiled_form == "chain", traced.compile_note
    nb = neighbour_model()
    res = dict(D=D, chains=a.chains, rounds=a.rounds, draws_per_round=a.draws, device=torch.cuda.get_device_name(dev),
               settings={})
    for name, args in (("example", EXAMPLE_ARGS), ("config4", CFG4_ARGS)):
        th0 = init(a.chains)
        s = {"chain": bk.DrGhmcDiag(traced, *args, chains=a.chains, seed=7, init=th0),
             "lanes_one_launch": bk.DrGhmcDiag(nb, *args, chains=a.chains, seed=7, init=th0),
             "lanes_opaque": bk.DrGhmcDiag(nb, *args, chains=a.chains, seed=7, init=th0, path="opaque")}
        assert s["lanes_one_launch"]._one_launch and not s["lanes_opaque"]._one_launch and not s["lanes_opaque"]._step_hook
        assert s["chain"]._traj_hook
        for x in s.values():
            x.advance(a.warmup)
        times = {k: [] for k in s}
        for _ in range(a.rounds):
            for k, x in s.items():
                times[k].append(ms_per_draw(x, a.draws))
        fin = {k: bool(torch.isfinite(x._theta_dc).all()) for k, x in s.items()}
        res["settings"][name] = dict(args=[args[0], list(args[1]), list(args[2]), args[3]],
                                     ms_per_draw_median={k: round(statistics.median(v), 4) for k, v in times.items()},
                                     ms_per_draw_all={k: [round(t, 4) for t in v] for k, v in times.items()},
                                     finite_state=fin,
                                     accept_rate={k: round(float(x.accept_rate()), 4) if hasattr(x, "accept_rate") else None
                                                  for k, x in s.items()})
        del s
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
