#!/usr/bin/env python3
"""Gradient-only evaluations of bk.GLM's families beside bk.LogisticRegression's, one process, alternated (profiles/glm.md).

    python tools/glm_timing.py [--n 1000000 --d 512 --c 2048] [--rounds 9] [--inner 3] [--parent-lib PATH] [--out FILE]

A gradient-only evaluation is the three launches bk_eval sends for a leapfrog step: the first GEMM with the residual in its
epilogue (bk_gemm_chains_logistic, or bk_gemm_chains_glm for a family), the second GEMM X^T r split over the observations
(bk_gemm_chains with work), and bk_logistic_finish.  They are sent here through the C ABI on ONE set of buffers (the shape
of config 5 holds 24 GB per model otherwise), timed with device events around `inner` evaluations, the variants taken in
turn for `rounds` rounds after a warm-up round; the figure of a variant is the median of its rounds.

The baseline runs TWICE in every round, as two variants: the difference of their medians is the A/A spread that every
comparison is read against.  --parent-lib: a libbkhip.so built from the parent commit; its logistic evaluation is one more
variant (measurement (a): nothing the logistic target runs changed).  Prints one JSON document; needs a GPU."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "bayes-kit_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bayes_kit_amd import _lib  # noqa: E402


def load_parent(path):
    lib = ctypes.CDLL(path)
    for name in ("bk_gemm_chains_logistic", "bk_gemm_chains", "bk_logistic_finish", "bk_gemm_chains_work_elems"):
        fn = getattr(lib, name)
        fn.argtypes = _lib.SIGNATURES[name]
        fn.restype = _lib._RESTYPE.get(name, ctypes.c_int)
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--c", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ops = _lib.default_ops()
    dev, N, D, C = ops.device, a.n, a.d, a.c
    g = torch.Generator(device=dev).manual_seed(1)
    f64 = dict(dtype=torch.float64, device=dev)
    X = torch.randn((N, D), generator=g, **f64) / D ** 0.5
    Xt = X.t().contiguous()
    theta = 0.5 * torch.randn((D, C), generator=g, **f64)   # |eta| stays a few units: every family's mean is finite
    y01 = (torch.rand(N, generator=g, **f64) < 0.5).to(torch.float64)
    trials = torch.floor(1.0 + 9.0 * torch.rand(N, generator=g, **f64))
    rows = {"bernoulli": (y01, None), "binomial": (torch.floor(trials * 0.5), trials),
            "poisson": (torch.floor(4.0 * torch.rand(N, generator=g, **f64)), None),
            "gaussian": (torch.randn(N, generator=g, **f64), 0.5 + torch.rand(N, generator=g, **f64))}
    off = 0.1 * torch.randn(N, generator=g, **f64)
    Z, G, grad = torch.empty((N, C), **f64), torch.empty((D, C), **f64), torch.empty((D, C), **f64)
    work = ops.gemm_chains_work(D, N, C)
    st, p = ops._s(), _lib.ptr
    wn = 0 if work is None else work.numel()

    def tail(lib):
        _lib.check(lib.bk_gemm_chains(p(Xt), N, D, N, p(Z), C, p(G), C, C, p(work), wn, st), "bk_gemm_chains")
        _lib.check(lib.bk_logistic_finish(p(G), p(theta), C, 0, 1, 0.25, 1.0, p(grad), 0, 0, C, D, st), "bk_logistic_finish")

    def logistic(lib):
        def run():
            _lib.check(lib.bk_gemm_chains_logistic(p(X), D, N, D, p(theta), C, p(Z), C, C, p(y01), st), "bk_gemm_chains_logistic")
            tail(lib)
        return run

    def glm(family, with_offset):
        yv, aux = rows[family]
        fam = _lib.GLM_FAMILIES.index(family)

        def run():
            _lib.check(ops.lib.bk_gemm_chains_glm(p(X), D, N, D, p(theta), C, p(Z), C, C, fam, p(yv), p(aux),
                                                  p(off) if with_offset else 0, st), "bk_gemm_chains_glm")
            tail(ops.lib)
        return run

    variants = {"logistic A": logistic(ops.lib), "logistic A'": logistic(ops.lib)}
    if a.parent_lib:
        variants["logistic parent"] = logistic(load_parent(a.parent_lib))
    for fam in _lib.GLM_FAMILIES:
        for wo in (False, True):
            variants[f"glm {fam}{' +offset' if wo else ''}"] = glm(fam, wo)
    times = {k: [] for k in variants}
    sums = {}
    for rnd in range(a.rounds + 1):  # (round 0 warms every variant up)
        for name, run in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                run()
            e1.record()
            e1.synchronize()
            if rnd:
                times[name].append(e0.elapsed_time(e1) / a.inner)
            else:
                sums[name] = float(grad.abs().sum().item())  # (finite, and the same for the variants that must agree)
    med = {k: statistics.median(v) for k, v in times.items()}
    base = med["logistic A"]
    flop = 2.0 * 2.0 * N * D * C  # two GEMMs
    out = {"shape": {"N": N, "D": D, "C": C}, "rounds": a.rounds, "inner": a.inner, "device": torch.cuda.get_device_name(0),
           "aa_spread": abs(med["logistic A'"] - base) / base,
           "variants": {k: {"median_ms": med[k], "min_ms": min(times[k]), "max_ms": max(times[k]), "vs_logistic": med[k] / base,
                            "tflops": flop / (med[k] * 1e-3) / 1e12, "grad_abs_sum": sums[k]} for k in variants}}
    assert all(np.isfinite(v["grad_abs_sum"]) for v in out["variants"].values())
    assert sums["glm bernoulli"] == sums["logistic A"], "the Bernoulli family must be the logistic target bit for bit"
    if a.parent_lib:
        assert sums["logistic parent"] == sums["logistic A"], "the parent's logistic evaluation differs"
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
