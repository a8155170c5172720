"""The configurations bench.py and bench_secondary.py time, at the size they are timed, against the oracle.

The goldens have 2-8 chains; the branches that only switch on at bench size (placement tuning from 128 MiB per array,
padded row pitch from 4,096 chains, the RNG prefetch on a side stream, the whole-draw kernel with chain-major normals,
per-workgroup list appends over hundreds of workgroups, advance(n) graphs with the diagnostics riding on the generator
launch) are held here to the oracle's standard on a scattered set of chains: theta bit for bit at every draw, logp to
1e-12, stream state (and DRGHMC's momentum) exact at the end.  Each oracle chain draws its own theta0 from its stream
(init=None), as the device does; where the bench rescales theta0 the oracle gets the same float64 factor.

Every sampler is built through the bench's own constructor or with its exact arguments (bench.make_cfg3_sampler,
bench_secondary.bench_cfg2 / bench_mala / bench_cfg4_spec_length), one full-size sampler alive at a time."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bayes_kit_amd as bk
from oracle import models as om
from oracle import samplers as osamp
from tests.helpers import rng_state_words
from tests.sampler_parity import LOGP_RTOL

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

EDGES = (0, 1, 63, 64, 255, 256, 4095, 4096)


@pytest.fixture(scope="module")
def ops():
    return bk._lib.default_ops()


@pytest.fixture(autouse=True)
def _release_memory():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def scattered_chains(C, n=48, seed=0, extra=()):
    """Ascending chain ids: the fixed edges {0, 1, 63, 64, 255, 256, 4095, 4096, C//2, C-2, C-1} (and `extra`) below
    C, topped up to n with a seeded sample of the rest."""
    picked = {c for c in (*EDGES, C // 2, C - 2, C - 1, *extra) if 0 <= c < C}
    rest = np.setdiff1d(np.arange(C), sorted(picked))
    k = max(0, min(n - len(picked), rest.size))
    picked.update(int(c) for c in np.random.default_rng(seed).choice(rest, size=k, replace=False))
    return np.array(sorted(picked), dtype=np.int64)


def _rows(x, chains):
    """x[chains] of a device tensor (C, ...) as a host array."""
    return x.index_select(0, torch.as_tensor(chains, device=x.device)).cpu().numpy()


def check_theta0(s, oracles, chains):
    th0 = _rows(s._theta, chains)
    for j, c in enumerate(chains):
        assert np.array_equal(th0[j], oracles[j]._theta), ("theta0", int(c))


def check_draws(s, oracles, chains, draws):
    """`draws` sample() calls of the device sampler against the per-chain oracles: theta bit for bit, logp to 1e-12
    at every draw; the stream state of every checked chain exact at the end."""
    for n in range(draws):
        th, lp = s.sample()
        th, lp = _rows(th, chains), _rows(lp, chains)
        for j, c in enumerate(chains):
            oth, olp = oracles[j].sample()
            assert np.array_equal(th[j], oth), (int(c), n, float(np.abs(th[j] - oth).max()))
            np.testing.assert_allclose(lp[j], olp, rtol=LOGP_RTOL, atol=1e-12, err_msg=f"chain {c} draw {n}")
    st = s.rng_state()
    for j, c in enumerate(chains):
        np.testing.assert_array_equal(st[:, c], rng_state_words(oracles[j]._rng), err_msg=f"stream of chain {c}")


def assert_model_opaque(s):
    """The gradient a separate op per leapfrog step: none of the fused / one-launch hooks."""
    assert not (s._fused or s._fused_draw or s._step_hook or s._traj_hook or s._lanes_traj)


# ---------------------------------------------------------------------------------------------------------------------
# config 3 (bench.py's headline)
# ---------------------------------------------------------------------------------------------------------------------
def cfg3_oracles(chains, chain_id0=0):
    """Oracle HMC chains of make_cfg3_sampler, theta0 rescaled by the bench's own float64 factor 1/sqrt(lam)."""
    from bench import D_CFG3, EPS_CFG3, L_CFG3, SEED_CFG3

    lam_t = torch.logspace(0, 4, D_CFG3, dtype=torch.float64)  # (the bench's values: np.logspace may differ)
    lam, scale = lam_t.numpy(), (1.0 / torch.sqrt(lam_t)).numpy()
    out = []
    for c in chains:
        o = osamp.HMCDiag(om.DiagGaussian(lam), EPS_CFG3, L_CFG3, metric_diag=np.ones(D_CFG3),
                          seed=np.random.Philox(key=[SEED_CFG3, chain_id0 + int(c)]))
        o._theta = o._theta * scale
        out.append(o)
    return out


@pytest.mark.parametrize("fused", [False, True])
def test_cfg3_bench_sampler_at_full_size_vs_oracle(ops, fused):
    """make_cfg3_sampler(65,536 chains) as bench.py builds it: fused=False is the headline (model-opaque: one
    kick+drift and one gradient op per leapfrog step, placement tuned, RNG prefetched on a side stream); fused=True the
    whole-draw kernel with chain-major normals.  3 draws against the oracle."""
    from bench import C_CFG3, make_cfg3_sampler

    C = C_CFG3
    s = make_cfg3_sampler(C, 0, ops.device, fused=fused)
    assert s._C == C == 65536
    if fused:
        assert s._fused_draw and s._fused_zt
    else:
        assert_model_opaque(s)
        assert s.placement is not None  # placement tuning ran (>= 128 MiB per array)
        assert s._prefetch and not s._use_graph
    pad = bk.HMCDiag.STATE_PAD_COLUMNS if (C * 8) % 4096 == 0 else 0
    assert s._state_pad == pad and s._theta_dc.stride(0) == C + pad
    chains = scattered_chains(C, n=64, seed=3)
    oracles = cfg3_oracles(chains)
    check_theta0(s, oracles, chains)
    check_draws(s, oracles, chains, 3)
    del s


def test_bench_py_headline_run_outputs_vs_oracle(tmp_path):
    """bench.py itself, as a child process (--steps 2 --warmup 1 --dump-outputs): the dumped outputs of the process whose
    time is the headline equal the oracle's 3rd draw -- theta bit for bit on a subset of the dumped rows, logp to
    1e-12 there, every chain's logp finite."""
    from bench import C_CFG3, DUMP_ROWS, SEED_CFG3

    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.strip()][-1])
    assert line.get("dump_outputs"), line
    assert line["steps"] == 2 and line["warmup"] == 1 and line["config"]["chains_per_gpu"] == C_CFG3
    theta, logp = np.load(out / "theta.npy"), np.load(out / "logp.npy")
    rows = np.sort(np.random.default_rng(SEED_CFG3).choice(C_CFG3, size=min(C_CFG3, DUMP_ROWS), replace=False))
    assert theta.shape == (rows.size, 1024) and logp.shape == (C_CFG3,)
    assert np.isfinite(logp).all()
    pos = np.unique(np.concatenate([[0, 1, rows.size - 2, rows.size - 1],
                                    np.random.default_rng(11).choice(rows.size, size=20, replace=False)]))
    chains = rows[pos]
    for o, p, c in zip(cfg3_oracles(chains), pos, chains):
        for _ in range(3):  # warmup + steps: the dump is the last timed draw
            oth, olp = o.sample()
        assert np.array_equal(theta[p], oth), (int(c), float(np.abs(theta[p] - oth).max()))
        np.testing.assert_allclose(logp[c], olp, rtol=LOGP_RTOL, atol=1e-12, err_msg=f"chain {c}")


# ---------------------------------------------------------------------------------------------------------------------
# MALA at config-3 shape (bench_secondary.bench_mala)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["step", "auto"])
def test_mala_bench_sampler_at_full_size_vs_oracle(ops, path):
    """bench_mala's two samplers at 65,536 chains (padded row pitch): path="step" is the model-opaque pair (the
    gradient a separate op), the default inlines the separable density into the step kernel.  theta0 rescaled as the
    bench does, then refresh_cache(); 3 draws against the oracle."""
    from bench import C_CFG3, D_CFG3

    C, D, eps, seed = C_CFG3, D_CFG3, 5e-5, 7
    lam = torch.logspace(0, 4, D, dtype=torch.float64)
    kw = dict(path="step") if path == "step" else {}
    s = bk.MALA(bk.DiagGaussian(lam), eps, chains=C, chain_id0=0, seed=seed, **kw)
    s._theta_dc.mul_((1.0 / torch.sqrt(lam)).to(ops.device)[:, None])
    s.refresh_cache()
    assert s.path == ("two-pass (bk_mala_step)" if path == "step" else
                      "two-pass, gradients recomputed in the step kernel (model.bk_mala_step)")
    assert s._state_pad == bk.MALA.STATE_PAD_COLUMNS > 0 and s._theta_dc.stride(0) == C + s._state_pad
    assert s._prefetch
    chains = scattered_chains(C, n=64, seed=5)
    scale = (1.0 / torch.sqrt(lam)).numpy()
    oracles = []
    for c in chains:
        o = osamp.MALA(om.DiagGaussian(lam.numpy()), eps, seed=np.random.Philox(key=[seed, int(c)]))
        o._theta = o._theta * scale
        lp, g = o._model.log_density_gradient(o._theta)  # (refresh_cache())
        o._lp, o._grad = lp, np.asanyarray(g)
        oracles.append(o)
    check_theta0(s, oracles, chains)
    check_draws(s, oracles, chains, 3)
    del s


# ---------------------------------------------------------------------------------------------------------------------
# config 2 (bench_secondary.bench_cfg2)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["opaque", "step", "auto"])
def test_cfg2_bench_samplers_vs_oracle(ops, path):
    """bench_cfg2's three samplers (iso-Gaussian D=128, L=32, eps 0.05, 4,096 chains, seed 20240, metric of ones),
    each replayed as a hipGraph at this size; 3 draws against the oracle."""
    C, D, L, eps, seed = 4096, 128, 32, 0.05, 20240
    s = bk.HMCDiag(bk.IsoGaussian(D), eps, L, metric_diag=torch.ones(D, dtype=torch.float64), seed=seed, chains=C,
                   chain_id0=0, path=path)
    assert s._use_graph
    if path == "opaque":
        assert_model_opaque(s)
    elif path == "step":
        assert s._step_hook and not s._fused
    else:
        assert s._fused_draw
    chains = scattered_chains(C, n=64, seed=2)
    oracles = [osamp.HMCDiag(om.IsoGaussian(D), eps, L, metric_diag=np.ones(D),
                             seed=np.random.Philox(key=[seed, int(c)])) for c in chains]
    check_theta0(s, oracles, chains)
    check_draws(s, oracles, chains, 3)
    del s


# ---------------------------------------------------------------------------------------------------------------------
# config 4 (bench_secondary.bench_cfg4_spec_length)
# ---------------------------------------------------------------------------------------------------------------------
def test_cfg4_spec_length_sequence_vs_oracle(ops):
    """Config 4 as bench_cfg4_spec_length runs it (32,768 funnel chains, D=101, K=3, one-launch proposals, hipGraph):
    eager / single-draw-graph draws, then attach(RunningMoments, DrawRecorder([0, 1, 100])), advance(2 + per) and
    advance(per) twice -- graphs of `per` draws whose moments update and series record ride on the next draw's
    generator launch.  Against the canonical-order oracle (oracle.models.FunnelCanonical) on chains on both sides of
    256-lane workgroup edges: every recorded series value bit for bit, recorded logp to 1e-12, the final theta,
    momentum and stream state exact, and the moments equal to a NumPy Welford over the oracle's draws."""
    from bench_secondary import CFG4_ARGS

    C, D, seed, pre_attach = 32768, 101, 20242, 3
    s = bk.DrGhmcDiag(bk.Funnel(D), *CFG4_ARGS, chains=C, chain_id0=0, seed=seed)
    assert s._one_launch and s._use_graph and s.host_syncs_per_draw == 0
    per = int(s.DRAWS_PER_GRAPH)
    for _ in range(pre_attach):
        s.advance()
    dims, recorded = [0, 1, D - 1], 2 + 3 * per
    mom = bk.RunningMoments(D, C)
    rec = bk.DrawRecorder(dims, recorded, C)
    s.attach(moments=mom, recorder=rec)
    s.advance(2 + per)
    s.advance(per)
    s.advance(per)
    assert per in s._graph_many  # the multi-draw graph ran
    assert mom.n == recorded and rec.n == recorded
    chains = scattered_chains(C, n=40, seed=4, extra=(511, 512, 16383, 16640, 32511, 32512))
    idx = torch.as_tensor(chains, device=ops.device)
    series = rec.series.index_select(2, idx).cpu().numpy()          # [4, recorded, n]
    mean = mom.mean.index_select(1, idx).cpu().numpy()              # [D, n]
    m2 = mom.m2.index_select(1, idx).cpu().numpy()
    theta = s._theta_dc.index_select(1, idx).cpu().numpy()
    rho = _rows(s._rho, chains)
    st = s.rng_state()
    for j, c in enumerate(chains):
        o = osamp.DrGhmcDiag(om.FunnelCanonical(D), *CFG4_ARGS, seed=np.random.Philox(key=[seed, int(c)]))
        for _ in range(pre_attach):
            o.sample()
        xs = np.empty((recorded, D))
        for n in range(recorded):
            oth, olp = o.sample()
            xs[n] = oth
            assert np.array_equal(series[:3, n, j], oth[dims]), (int(c), n)
            np.testing.assert_allclose(series[3, n, j], olp, rtol=LOGP_RTOL, atol=1e-12, err_msg=f"chain {c} draw {n}")
        assert np.array_equal(theta[:, j], o._theta), int(c)
        assert np.array_equal(rho[j], o._rho), int(c)
        np.testing.assert_array_equal(st[:, c], rng_state_words(o._rng), err_msg=f"stream of chain {c}")
        # Welford as csrc/bk_welford.hpp states it; 1e-13 rather than bit for bit: hipcc may contract into an fma
        mu, q = np.zeros(D), np.zeros(D)
        for n in range(recorded):
            delta = xs[n] - mu
            mu = mu + delta / (n + 1)
            q = q + delta * (xs[n] - mu)
        # (relative to the size of the terms summed, per dimension: a mean near zero is a difference of large draws)
        big = np.abs(xs).max(axis=0)
        assert (np.abs(mean[:, j] - mu) <= 1e-13 * big).all(), ("mean", int(c), float(np.abs(mean[:, j] - mu).max()))
        assert (np.abs(m2[:, j] - q) <= 1e-13 * recorded * big * big).all(), ("m2", int(c))
    del s, mom, rec
