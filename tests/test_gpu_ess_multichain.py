"""Multi-chain bulk / tail / mean ESS and MCSE of the mean on the MI355X (csrc/bk_ess_multi.hip) against the NumPy
restatement of tests/multichain_ess_ref.py."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import bayes_kit_amd as bk
from bayes_kit_amd import diagnostics as dg
from tests import multichain_ess_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

FUNCS = ["ess_bulk", "ess_tail", "ess_mean", "mcse_mean"]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _check_all(x, t, rel=1e-9):
    for f in FUNCS:
        assert getattr(bk, f)(t) == pytest.approx(getattr(ref, f)(x), rel=rel), f
    assert bk.ess_quantile(t, 0.3) == pytest.approx(ref.ess_quantile(x, 0.3), rel=rel)


@pytest.mark.parametrize("n", [287, 288, 289, 575, 576, 577, 1151, 1153])
@pytest.mark.parametrize("odd", [0, 1])
def test_register_tile_seams(n, odd):
    x = ref.ar1(np.random.default_rng(n + odd), 2 * n + odd, 17, 0.6)
    _check_all(x, _dev(x))


@pytest.mark.parametrize("C", [1, 2, 17, 64, 65, 100])
def test_chain_counts(C):
    x = ref.ar1(np.random.default_rng(C), 301, C, 0.4)
    _check_all(x, _dev(x))


def test_strided_view_and_antithetic():
    x = ref.ar1(np.random.default_rng(1), 200, 40, 0.5)
    big = torch.zeros((200, 57), dtype=torch.float64, device="cuda")
    big[:, 3:43] = _dev(x)
    v = big[:, 3:43]
    assert v.stride(0) == 57
    _check_all(x, v)
    a = ref.ar1(np.random.default_rng(2), 400, 30, -0.9)
    _check_all(a, _dev(a))


@pytest.mark.parametrize("phi", [0.9, 0.99, 0.999])
def test_strong_correlation_several_lag_rounds(phi):
    x = ref.ar1(np.random.default_rng(int(phi * 1000)), 1000, 24, phi)
    _check_all(x, _dev(x))


def test_lag_sums_entry_point_against_numpy_and_bit_identical():
    x = ref.ar1(np.random.default_rng(5), 999, 70, 0.7)
    t = _dev(x)
    ops = dg._ops(None)
    cm = torch.empty(140, dtype=torch.float64, device="cuda")
    g0 = torch.empty_like(cm)
    ops.ess_split_moments(t, None, cm, g0)
    a = ops.ess_lag_sums(t, None, cm, 0, 499)
    b = ops.ess_lag_sums(t, None, cm, 0, 499)
    assert torch.equal(a, b)
    want = ref.autocov_direct(ref.split(x)).sum(axis=1)
    np.testing.assert_allclose(a.cpu().numpy(), want, rtol=1e-9, atol=1e-9 * want[0])
    c = ops.ess_lag_sums(t, 0.1, cm * 0 + 0.5, 64, 128)  # indicator mode against the materialised indicator
    ind = (ref.split(x) <= 0.1).astype(np.float64) - 0.5
    want = np.array([(ind[: 499 - k] * ind[k:]).sum(axis=0).sum() / 499 for k in range(64, 192)])
    np.testing.assert_allclose(c.cpu().numpy(), want, rtol=1e-12, atol=1e-12)


def test_fft_route_and_switch_over():
    ops = dg._ops(None)
    n = ops.ess_lag_sums_max_half()
    x = ref.ar1(np.random.default_rng(6), 2 * n, 3, 0.95)
    x[:, 1] = 0.25  # a stuck chain among moving ones
    t = _dev(x)
    cm = torch.empty(6, dtype=torch.float64, device="cuda")
    g0 = torch.empty_like(cm)
    ops.ess_split_moments(t, None, cm, g0)
    lds = ops.ess_lag_sums(t, None, cm, 0, n)
    fft = dg._lag_sums_fft(t, None, g0, ops)
    np.testing.assert_allclose(fft.cpu().numpy(), lds.cpu().numpy(), rtol=1e-9, atol=1e-9 * float(lds[0]))
    e = bk.ess_mean(t)
    assert np.isfinite(e) and e == pytest.approx(ref.ess_mean(x), rel=1e-9)
    y = ref.ar1(np.random.default_rng(7), 2 * n + 3, 3, 0.95)  # the FFT route (halves one longer than the tile)
    y[:, 2] = -1.0
    _check_all(y, _dev(y))


def test_long_halves_few_chains_per_workgroup_and_chunked_lags():
    """Halves of 3,000 draws (two chains per workgroup: the other two wavefronts take the next lag block) and of 5,000
    (one chain per workgroup) with 4,096 chains: every lag in one request needs more partials than one launch holds, so
    bk_ess_lag_sums runs it as several launches.  Both against the FFT route."""
    ops = dg._ops(None)
    for n, C in ((3000, 8), (5000, 4096)):
        x = _gen_ar1(2 * n, C, 0.9, n)
        cm = torch.empty(2 * C, dtype=torch.float64, device="cuda")
        g0 = torch.empty_like(cm)
        ops.ess_split_moments(x, None, cm, g0)
        lds = ops.ess_lag_sums(x, None, cm, 0, n)
        fft = dg._lag_sums_fft(x, None, g0, ops)
        np.testing.assert_allclose(lds.cpu().numpy(), fft.cpu().numpy(), rtol=1e-9, atol=1e-9 * float(lds[0]))
        part = ops.ess_lag_sums(x, None, cm, 1000, 37)
        np.testing.assert_allclose(part.cpu().numpy(), lds[1000:1037].cpu().numpy(), rtol=1e-12, atol=1e-12 * float(lds[0]))
    y = ref.ar1(np.random.default_rng(30), 6001, 8, 0.95)
    _check_all(y, _dev(y))


def test_select_ranks_entry_point():
    ops = dg._ops(None)
    rng = np.random.default_rng(4)
    vals = rng.standard_normal(10007)
    ranks = rng.permutation(10007) + 1.0
    targets = np.array([1.0, 10007.0, 5000.0, 17.0, 9999.0, 2.0, 3.0, 4.0])
    out = torch.full((8,), -1.0, dtype=torch.float64, device="cuda")
    ops.select_ranks(_dev(ranks), _dev(vals), _dev(targets), out)
    want = np.array([vals[np.nonzero(ranks == t)[0][0]] for t in targets])
    assert np.array_equal(out.cpu().numpy(), want)
    out = torch.zeros(2, dtype=torch.float64, device="cuda")
    ops.select_ranks(_dev(ranks[:100]), _dev(vals[:100]), _dev(np.array([1e9, 0.5])), out)  # (no element holds them)
    assert np.array_equal(out.cpu().numpy(), [0.0, 0.0])


def test_one_rank_rccl_group_gives_the_no_group_answer():
    """The cross-rank path on the real collective library (following test_sample_sort_and_rhat_collectives_run_on_rccl and
    tests/single_rank_group_worker.py): all five functions and DrawRecorder.summary() under a one-rank `nccl` group with
    the collectives forced through it -- the sample sort, bk_select_ranks and the gathered partial sums -- equal the
    no-group values.  A child process (this one has touched the GPU)."""
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port),
                "HSA_ENABLE_IPC_MODE_LEGACY": os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0")})
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ess_multichain_rccl_worker.py")], env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    r = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert r["ok"] and all(c["all_to_all"] >= 4 for c in r["collectives"].values())


def test_constant_columns_among_moving_ones():
    x = ref.ar1(np.random.default_rng(8), 700, 20, 0.5)
    x[:, [3, 11]] = 2.0
    _check_all(x, _dev(x))


def _gen_ar1(N, C, phi, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    e = torch.randn((N, C), dtype=torch.float64, device="cuda", generator=g) * float(np.sqrt(1 - phi * phi))
    x = torch.empty_like(e)
    x[0] = torch.randn(C, dtype=torch.float64, device="cuda", generator=g)
    for t in range(1, N):
        x[t] = phi * x[t - 1] + e[t]
    return x


def test_full_size_known_answers():
    N, C = 1000, 65536
    Mn = 2 * C * (N // 2)
    x = _gen_ar1(N, C, 0.0, 1)
    assert abs(bk.ess_mean(x) / Mn - 1) < 0.05
    assert abs(bk.ess_bulk(x) / Mn - 1) < 0.05
    x = _gen_ar1(N, C, 0.5, 2)
    assert abs(bk.ess_mean(x) / Mn / (0.5 / 1.5) - 1) < 0.05
    x = torch.randn((N, C), dtype=torch.float64, device="cuda")
    x[:, 1::2] += 5.0
    assert bk.ess_mean(x) / Mn < 0.01


def test_summary_after_hmc_run_and_one_sort_per_quantity():
    C, D = 256, 4
    s = bk.HMCDiag(bk.DiagGaussian(np.logspace(0, 1, D)), 0.2, 8, chains=C, seed=3)
    rec = bk.DrawRecorder([0, 3], 100, C)
    for _ in range(100):
        th, lp = s.sample()
        rec.record(th, lp)
    ops = rec._ops
    calls = []
    orig = ops.sort_by_key

    def counted(*a, **k):
        calls.append(1)
        return orig(*a, **k)

    ops.sort_by_key = counted
    try:
        sm = rec.summary()
    finally:
        del ops.sort_by_key
    assert len(calls) == 3  # one per tracked quantity (theta[0], theta[3], logp)
    assert sm["name"] == rec.names()
    for k in range(3):
        v = rec.view(k)
        assert sm["ess_bulk"][k] == bk.ess_bulk(v)
        assert sm["ess_tail"][k] == bk.ess_tail(v)
        assert sm["mcse_mean"][k] == bk.mcse_mean(v)
        assert sm["rhat"][k] == bk.rank_normalized_rhat(v)
        assert sm["ess_bulk"][k] == pytest.approx(ref.ess_bulk(v.cpu().numpy()), rel=1e-9)
