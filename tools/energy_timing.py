#!/usr/bin/env python3
"""What HMCDiag.track_energy costs, and that an untracked sampler costs what it did before (profiles/energy_diagnostics.md).

    python tools/energy_timing.py [--small] [--parent DIR] [--out FILE.md]

Whole draws between device events, alternated in one process, medians of the repeats.  Shape 1,024 x 65,536 (config 3:
DiagGaussian(logspace(0, 4, D)), eps 0.006, 64 steps), fp64, on the two paths bench.py times: path="opaque" (the headline:
the gradient a separate op per step, the tile-major schedule) and the whole-draw kernel.
  --parent DIR   a checkout of the PARENT commit with its library built (python bayes-kit_amd/build.py there).  Its package
                 is imported beside this one under another name, and per path the jobs are
                     parent A | commit (untracked) | parent A' | commit tracked
                 A and A' are the same parent sampler under two names: their gap is the A/A spread of the run.
  the bar        the untracked commit draw costs no more than the parent draw plus the A/A spread.  It is the only bar; without
                 --parent the tool times commit A / A' / tracked and evaluates none.
  tracked        reported beside untracked, no bar: three more small launches per draw (per tile on the tile-major schedule),
                 and on the whole-draw path the accept test as a launch of its own.
  kernels        bk_energy_update and bk_divergence_capture alone at C = 65,536, D = 1,024 with 0, 1 % and 100 % of the
                 chains flagged; the capture into an empty store (its fill level zeroed before every call: one more tiny
                 launch inside the timed window) and into a full one.
Before anything is timed the tool checks, at the timed size, that tracked and untracked samplers of this commit and the
parent's sampler hold the same state after three draws.  --small rehearses the script at toy sizes (its numbers are
overheads)."""
import argparse
import importlib.util
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bayes-kit_amd")]

import torch  # noqa: E402

import bayes_kit_amd as bk  # noqa: E402


def load_package(root, name):
    """The bayes_kit_amd package of another checkout, imported under `name` (it loads that checkout's own library)."""
    path = os.path.join(os.path.abspath(root), "bayes-kit_amd", "bayes_kit_amd")
    spec = importlib.util.spec_from_file_location(name, os.path.join(path, "__init__.py"), submodule_search_locations=[path])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def events_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(jobs, reps, repeats, warm=3):
    for fn in jobs.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in jobs}
    for _ in range(repeats):
        for name, fn in jobs.items():
            ms[name].append(events_ms(fn, reps))
    return {k: statistics.median(v) for k, v in ms.items()}, ms


def cfg3_sampler(pkg, D, C, L, fused):
    """bench.py's config-3 sampler (make_cfg3_sampler), without the placement tuning: every sampler of a comparison keeps
    its arrays as allocated."""
    lam = torch.logspace(0, 4, D, dtype=torch.float64)
    s = pkg.HMCDiag(pkg.DiagGaussian(lam), 0.006, L, metric_diag=torch.ones(D, dtype=torch.float64), seed=20241, chains=C,
                    path="auto" if fused else "opaque", tune_placement=False, graph=False)
    s._theta_dc.mul_((1.0 / torch.sqrt(lam)).to(s._theta_dc.device)[:, None])
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--parent")
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("energy_timing.py measures on a GPU; none is visible")
    ops = bk._lib.default_ops()
    dev = ops.device
    D, C, L = (64, 4096, 8) if a.small else (1024, 65536, 64)
    parent = load_package(a.parent, "bayes_kit_amd_parent") if a.parent else None
    lines = [f"device: {torch.cuda.get_device_name(0)}; D = {D}, C = {C}, {L} steps; alternated, medians; one box, one run; "
             + ("parent: the checkout given with --parent" if parent else "NO parent checkout: the bar is not evaluated"), "",
             "| path | " + ("parent A / A' ms" if parent else "commit A / A' ms") + " | A/A spread | commit untracked ms | "
             "untracked / parent | bar (<= 1 + A/A) | tracked ms | tracked - untracked | tracked / untracked |",
             "|---|---|---|---|---|---|---|---|---|"]
    for fused in (False, True):
        name = "whole-draw kernel" if fused else 'path="opaque"'
        reps, repeats = ((3, 3) if a.small else ((40, 7) if fused else (4, 7)))
        base = cfg3_sampler(parent if parent else bk, D, C, L, fused)
        plain, tracked = cfg3_sampler(bk, D, C, L, fused), cfg3_sampler(bk, D, C, L, fused)
        assert plain._fused_draw == fused and (fused or plain._chain_tile < C or a.small)
        e = tracked.track_energy()
        for _ in range(3):
            base.sample(), plain.sample(), tracked.sample()
        assert torch.equal(plain._theta_dc, tracked._theta_dc) and torch.equal(plain._theta_dc, base._theta_dc), name
        assert e.transitions == 3 * C
        jobs = {"A": base.sample, "plain": plain.sample, "A2": base.sample, "tracked": tracked.sample}
        med, ms = alternate(jobs, reps, repeats, warm=2)
        ref = 0.5 * (med["A"] + med["A2"])
        aa = abs(med["A"] - med["A2"]) / ref
        ratio = med["plain"] / ref
        verdict = ("met" if ratio <= 1.0 + aa else "MISSED") if parent else "not evaluated"
        lines.append(f"| {name} | {med['A']:.4f} / {med['A2']:.4f} | {100 * aa:.2f} % | {med['plain']:.4f} | {ratio:.4f} | "
                     f"{verdict} | {med['tracked']:.4f} | {1e3 * (med['tracked'] - med['plain']):.1f} us | "
                     f"{med['tracked'] / med['plain']:.4f} |")
        print(lines[-1], flush=True)
        print("  repeats (ms): " + "; ".join(f"{k} {[round(v, 4) for v in vs]}" for k, vs in ms.items()), flush=True)
        print(f"  tracker after the run: {e.transitions} transitions, {e.divergences()} divergences, pooled E-BFMI "
              f"{e.ebfmi_pooled():.3f}", flush=True)
        del base, plain, tracked, jobs
        torch.cuda.empty_cache()
    # the two entry points alone
    lines += ["", "| flagged | bk_energy_update ms | bytes | TB/s | capture, empty store ms | capture, full store ms |",
              "|---|---|---|---|---|---|"]
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    rn = lambda *s: torch.randn(s, dtype=torch.float64, device=dev, generator=g)  # noqa: E731
    theta = rn(D, C)
    lp, k0, k1 = rn(C) - 20.0, rn(C) ** 2, rn(C) ** 2
    logu = torch.log(torch.rand(C, dtype=torch.float64, device=dev, generator=g))
    for frac in (0.0, 0.01, 1.0):
        lp_p = lp + 0.1 * rn(C)
        n_flag = int(round(frac * C))
        if n_flag:
            lp_p[torch.randperm(C, device=dev, generator=g)[:n_flag]] -= 5000.0
        e = bk.EnergyDiagnostics(C, D, ops=ops)
        e.update(lp, k0, lp_p, k1, logu, theta)
        assert int(e.div_mask.sum()) == n_flag == e.divergent_states()["seen"]

        def update():
            ops.energy_update(lp, k0, lp_p, k1, logu, e.threshold, e.mean_E, e.m2_E, e.last_E, e.ssd, e.trans, e.cnt, e.ndiv,
                              e.div_mask, e.err, e._totals)

        def capture():
            ops.divergence_capture(e.div_mask, e.err, e.trans, theta, 0, e.theta_div, e.chain, e.draw, e.err_store, e._fill,
                                   e._work)

        def capture_empty():
            e._fill.zero_()
            capture()

        e._fill.fill_(e.capture)
        med_full, _ = alternate({"update": update, "capture": capture}, 3 if a.small else 50, 3 if a.small else 7)
        med_empty, _ = alternate({"capture": capture_empty}, 3 if a.small else 50, 3 if a.small else 7)
        nbytes = C * (5 * 8 + 2 * (4 * 8 + 3 * 8) + 8 + 1)
        lines.append(f"| {100 * frac:g} % | {med_full['update']:.4f} | {nbytes / 1e6:.1f} MB | "
                     f"{nbytes / (med_full['update'] * 1e-3) / 1e12:.2f} | {med_empty['capture']:.4f} | "
                     f"{med_full['capture']:.4f} |")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
