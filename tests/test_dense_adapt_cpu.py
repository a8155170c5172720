"""The dense-metric adaptation without a GPU: bk.RunningCovariance, HMCDiag.warmup(adapt_metric="dense"), the checkpoint and
the SMC kernel on the NumPy stand-in (tests/fake_ops_dense_adapt.py), argument checks of the C ABI, refusals, and two gloo
ranks."""
import ctypes
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import bayes_kit_amd as bk
from tests import dense_adapt_parity as dp
from tests.fake_ops_dense_adapt import DenseAdaptFakeOps

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SEED = 1


@pytest.fixture(scope="module")
def ops():
    return DenseAdaptFakeOps()


# ---- the kernel's C ABI: decided before any HIP call ------------------------------------------------------------------------
def test_cov_accumulate_argument_errors_without_a_gpu():
    from bayes_kit_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_double * 4096)()
    p = ctypes.addressof(buf)
    E_ARG = -1
    D, C = 5, 37
    need = lib.bk_cov_accumulate_work_elems(D, C)
    assert need >= 128 * 128 + 128 and lib.bk_cov_accumulate_work_elems(0, C) == 0 == lib.bk_cov_accumulate_work_elems(D, 0)
    assert lib.bk_cov_k_chunk(D) >= 16 and lib.bk_cov_k_chunk(D) % 16 == 0 and lib.bk_cov_k_chunk(0) == 0
    for Dk in (1, 16, 130, 512, 1024, 5000):  # a chunk of D x k_chunk doubles fits half of an XCD's 4 MiB L2
        k = lib.bk_cov_k_chunk(Dk)
        assert k % 16 == 0 and (k == 16 or Dk * k * 8 <= 2 << 20), (Dk, k)
    assert lib.bk_cov_accumulate(None, C, C, D, None, p, D, p, p, need, None) == E_ARG
    assert lib.bk_cov_accumulate(p, C, C, D, None, None, D, p, p, need, None) == E_ARG
    assert lib.bk_cov_accumulate(p, C, C, D, None, p, D, None, p, need, None) == E_ARG
    assert lib.bk_cov_accumulate(p, C - 1, C, D, None, p, D, p, p, need, None) == E_ARG   # ld < C
    assert lib.bk_cov_accumulate(p, C, C, D, None, p, D - 1, p, p, need, None) == E_ARG   # lds < D
    assert lib.bk_cov_accumulate(p, C, C, D, None, p, D, p, None, need, None) == E_ARG    # scratch required
    assert lib.bk_cov_accumulate(p, C, C, D, None, p, D, p, p, need - 1, None) == E_ARG   # ... and large enough
    assert lib.bk_cov_accumulate(p, C, -1, D, None, p, D, p, p, need, None) == E_ARG
    assert lib.bk_cov_accumulate(p, C, C, -1, None, p, D, p, p, need, None) == E_ARG
    assert lib.bk_cov_accumulate(p, 0, 0, D, None, p, D, p, None, 0, None) == 0           # no chains: nothing to add
    assert lib.bk_cov_accumulate(p, C, C, 0, None, p, 0, p, None, 0, None) == 0


# ---- RunningCovariance --------------------------------------------------------------------------------------------------
def test_running_covariance(ops):
    dp.check_running_covariance(ops)


def test_running_covariance_refuses_what_it_cannot_use(ops):
    import torch

    rc = bk.RunningCovariance(5, ops=ops)
    with pytest.raises(ValueError, match="covariance"):
        rc.covariance()
    with pytest.raises(ValueError):
        rc.update(torch.zeros((4, 7), dtype=torch.float64))
    with pytest.raises(ValueError, match="layout"):
        rc.update(torch.zeros((5, 7), dtype=torch.float64), layout="xx")
    with pytest.raises(ValueError, match="shape"):
        rc.load_state_dict(bk.RunningCovariance(4, ops=ops).state_dict())


# ---- warmup -------------------------------------------------------------------------------------------------------------
def test_dense_warmup_reaches_the_statistic_and_installs_a_metric(ops):
    dp.check_statistic_is_reached(ops)


def test_identity_metric_is_the_plain_sampler(ops):
    dp.check_identity_start_is_the_plain_path(ops)


def test_dense_warmup_end_to_end_on_the_stand_in(ops):
    s, rep = dp.warmed(ops, SEED)
    dp.check_dense_warmup_report(rep)
    assert s._stepsize == rep["stepsize"] and np.array_equal(s.metric_dense, rep["metric_dense"])
    assert len(rep["installed"]) == 3 and np.array_equal(rep["installed"][-1], rep["metric_dense"])


def test_the_diagonal_warmup_ends_with_at_most_half_the_step_size(ops):
    dp.check_step_size_against_diagonal(ops, SEED)


def test_sampling_after_the_dense_warmup(ops):
    dp.check_sampling_after_warmup(ops, SEED)


def test_checkpoint_carries_the_dense_metric(ops):
    dp.check_checkpoint(ops)


def test_warmup_with_and_without_prefetch_rng(ops):
    dp.check_prefetch_independent(ops)


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_refusals(ops):
    with pytest.raises(ValueError, match="only on a sampler built with metric_dense"):
        dp.make_sampler(ops, 1, dense=False, C=8).warmup(30, adapt_metric="dense")
    with pytest.raises(ValueError, match="adapt_trajectory=True cannot be combined with metric_dense"):
        dp.make_sampler(ops, 1, C=8).warmup(30, adapt_metric="dense", adapt_trajectory=True)
    with pytest.raises(ValueError, match="adapt_metric must be True, False or 'dense'"):
        dp.make_sampler(ops, 1, C=8).warmup(30, adapt_metric="diag")
    with pytest.raises(ValueError, match="adapt_metric must be True, False or 'dense'"):
        bk.hmc_kernel(0.3, 4, adapt_metric="full")
    a = dp.make_sampler(ops, 1, C=8)
    a.sample()
    with pytest.raises(ValueError, match="checkpoint holds metric_dense"):
        dp.make_sampler(ops, 2, dense=False, C=8).load_state_dict(a.state_dict())
    # a checkpoint written without one loads into a sampler that has one, which keeps its own (as older checkpoints do)
    b = dp.make_sampler(ops, 2, dense=False, C=8)
    b.sample()
    c = dp.make_sampler(ops, 3, C=8)
    c.load_state_dict(b.state_dict())
    assert np.array_equal(c.metric_dense, np.eye(dp.D_TARGET))


# ---- SMC ----------------------------------------------------------------------------------------------------------------
def test_smc_hmc_kernel_with_the_particles_full_covariance(ops):
    dp.check_smc_dense(ops)


# ---- two ranks ------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_rank_dense_warmup_agrees_with_one_process(ops):
    """Two gloo ranks x 256 chains against one process x 512 (the end-to-end test's run).  Both ranks report array_equal
    metric_dense and eps (they see the same gathered sums in rank order and shift by the same gathered centre).  Up to the
    first window's end the two runs make the same draws (the acceptance statistic of 512 chains is the two ranks' trees
    added), so the first installed metric differs by the grouping of the sums alone: rel 1e-11 (of sqrt(M_ii M_jj)).
    After it dual averaging amplifies that rounding (tests/test_adapt_cpu.py): both runs must pass the end-to-end bars."""
    port = _free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), OMP_NUM_THREADS="1", BK_TEST_SEED=str(SEED))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dense_adapt_dist_worker.py")], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(out)
    reps = []
    for p, out in zip(procs, outs):
        assert p.returncode == 0, out
        reps.append(json.loads([l for l in out.splitlines() if l.startswith("{")][-1]))
    assert reps[0]["eps"] == reps[1]["eps"] and reps[0]["stepsize"] == reps[1]["stepsize"]
    assert np.array_equal(np.array(reps[0]["metric_dense"]), np.array(reps[1]["metric_dense"]))
    assert reps[0] == reps[1]
    _, one = dp.warmed(ops, SEED)
    m2, m1 = np.array(reps[0]["installed"][0]), one["installed"][0]
    d = np.sqrt(np.diag(m1))
    rel = float((np.abs(m2 - m1) / (d[:, None] * d[None, :])).max())  # (the scale of dp.assert_cov_close)
    print(f"two ranks vs one process: first window's metric rel {rel:.3e}; eps {reps[0]['stepsize']!r} vs {one['stepsize']!r}")
    assert reps[0]["alpha"][:100] == one["alpha"][:100]
    assert rel <= 1e-11
    two = dict(reps[0], metric_dense=np.array(reps[0]["metric_dense"]), precond_diag=None)
    dp.check_dense_warmup_report(two)
