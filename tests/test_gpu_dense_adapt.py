"""The dense-metric adaptation on the MI355X: bk_cov_accumulate against a long-double reference at its tile, K-step and slab
seams, and the checks of tests/dense_adapt_parity.py on the HIP library (bars, not equality with the stand-in: the MFMA
summation order is not restated)."""
import ctypes

import numpy as np
import pytest
import torch

import bayes_kit_amd as bk
from tests import dense_adapt_parity as dp

pytestmark = pytest.mark.gpu

SEED = 11  # (see test_sampling_after_the_dense_warmup)
U = 2.0 ** -53


@pytest.fixture(scope="module")
def ops():
    return bk._lib.default_ops()


def _np(t):
    return np.asarray(t.cpu())


def _shapes(ops):
    return [(1, 1), (5, 37), (16, 16), (17, 15), (127, 130), (129, 257), (130, ops.cov_k_chunk(130) + 1), (128, 256)]


def _reference(x, c):
    """Xc Xc^T, rowsum(Xc) and the entrywise bounds 4 C u (|Xc| |Xc|^T), 4 C u rowsum(|Xc|) in np.longdouble; Xc itself
    is formed in double, as the kernel forms it (one rounding per element, the same one)."""
    xc = (x if c is None else x - c[:, None]).astype(np.longdouble)
    C = x.shape[1]
    a = np.abs(xc)
    return xc @ xc.T, xc.sum(axis=1), 4.0 * C * U * (a @ a.T), 4.0 * C * U * a.sum(axis=1)


def _call(ops, X, c, S, s):
    ops.cov_accumulate(X, c, S, s, ops.cov_work(X.shape[0], X.shape[1]))


@pytest.mark.parametrize("centred", [False, True])
@pytest.mark.parametrize("case", range(8))
def test_cov_accumulate_against_long_double(ops, case, centred):
    """Shapes at the MFMA tile edge (16), the workgroup tile edge (128), the K-step edge and the slab seam
    (k_chunk + 1 chains), plus one whole-tile shape (128, 256) that takes the unchecked kernel; X a column slice of a wider
    tensor (padded pitch; an odd pitch or offset keeps the checked kernel, (128, 256) is given an aligned one).  The
    error bound is the dot product's: 4 C u (|Xc| |Xc|^T)_ij, and 4 C u rowsum|Xc| for s.  S and s are pre-filled by a call on
    the first half of the chains; the call on the second half must land within the bound of the whole.  Then exact
    symmetry, a non-negative diagonal, and a repeated call on zeroed outputs with array_equal results."""
    D, C = _shapes(ops)[case]
    dev = ops.device
    g = np.random.default_rng(100 + case)
    x = g.normal(size=(D, C)) * np.logspace(0, 1, D)[:, None]
    c = None
    if centred:
        c = 1e3 * (1.0 + g.random(D))      # a centre of order 1e3 under data of order 1e3: cancellation would show
        x = x + c[:, None] + 0.1 * g.normal(size=(D, 1))
    aligned = (D, C) == (128, 256)
    pad, off = (8, 4) if aligned else (7, 3)
    wide = torch.zeros((D, C + pad), dtype=torch.float64, device=dev)
    wide[:, off:off + C] = torch.from_numpy(x).to(dev)
    wide[:, :off] = float("nan")           # (whatever lies outside the slice must not be read into a sum)
    wide[:, off + C:] = float("nan")
    X = wide[:, off:off + C]
    ct = None if c is None else torch.from_numpy(c).to(dev)
    want_S, want_s, tol_S, tol_s = _reference(x, c)

    def run(S, s):
        h = C // 2
        if h:
            _call(ops, X[:, :h], ct, S, s)      # pre-fill: a previous call's result
        _call(ops, X[:, h:], ct, S, s)
        return _np(S), _np(s)

    Sbig = torch.zeros((D, D + 3), dtype=torch.float64, device=dev)   # (a padded pitch for S as well)
    S1, s1 = run(Sbig[:, :D], torch.zeros(D, dtype=torch.float64, device=dev))
    assert not _np(Sbig[:, D:]).any()
    errS = np.abs(S1.astype(np.longdouble) - want_S)
    errs = np.abs(s1.astype(np.longdouble) - want_s)
    print(f"D={D} C={C} centred={centred}: max err/bound S {float((errS / tol_S).max()):.3f}  s "
          f"{float((errs / tol_s).max()):.3f}")
    assert (errS <= tol_S).all() and (errs <= tol_s).all()
    assert np.array_equal(S1, S1.T) and (np.diag(S1) >= 0.0).all()
    S2, s2 = run(torch.zeros((D, D), dtype=torch.float64, device=dev), torch.zeros(D, dtype=torch.float64, device=dev))
    assert np.array_equal(S1, S2) and np.array_equal(s1, s2)
    # one call on all chains: within the same bound
    S3 = torch.zeros((D, D), dtype=torch.float64, device=dev)
    s3 = torch.zeros(D, dtype=torch.float64, device=dev)
    _call(ops, X, ct, S3, s3)
    assert (np.abs(_np(S3).astype(np.longdouble) - want_S) <= tol_S).all()
    assert (np.abs(_np(s3).astype(np.longdouble) - want_s) <= tol_s).all()
    assert np.array_equal(_np(S3), _np(S3).T)


def test_cov_accumulate_argument_errors_launch_nothing(ops):
    lib, dev = ops.lib, ops.device
    D, C = 5, 37
    X = torch.ones((D, C), dtype=torch.float64, device=dev)
    S = torch.full((D, D), 7.0, dtype=torch.float64, device=dev)
    s = torch.full((D,), 7.0, dtype=torch.float64, device=dev)
    work = ops.cov_work(D, C)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = work.numel()
    assert lib.bk_cov_accumulate(p(X), C - 1, C, D, None, p(S), D, p(s), p(work), n, st) == -1
    assert lib.bk_cov_accumulate(p(X), C, C, D, None, p(S), D - 1, p(s), p(work), n, st) == -1
    assert lib.bk_cov_accumulate(p(X), C, C, D, None, p(S), D, p(s), p(work), n - 1, st) == -1
    assert lib.bk_cov_accumulate(p(X), C, C, D, None, p(S), D, p(s), None, 0, st) == -1
    assert lib.bk_cov_accumulate(p(X), C, 0, D, None, p(S), D, p(s), None, 0, st) == 0
    torch.cuda.synchronize()
    assert (_np(S) == 7.0).all() and (_np(s) == 7.0).all()


# ---- RunningCovariance, warmup, checkpoint, SMC: the shared checks on the library -----------------------------------------
def test_running_covariance(ops):
    dp.check_running_covariance(ops)


def test_dense_warmup_reaches_the_statistic_and_installs_a_metric(ops):
    dp.check_statistic_is_reached(ops)


def test_identity_metric_is_the_plain_sampler(ops):
    dp.check_identity_start_is_the_plain_path(ops)


def test_dense_warmup_end_to_end(ops):
    """Observed on the MI355X: seed 11 cond(W) = 1.112, eps = 0.823, mean alpha of the last 20 draws 0.793; seed 1
    1.150 / 0.781 / 0.790 (the stand-in's nine seeds: dp.check_dense_warmup_report)."""
    s, rep = dp.warmed(ops, SEED)
    dp.check_dense_warmup_report(rep)
    assert s._stepsize == rep["stepsize"] and np.array_equal(s.metric_dense, rep["metric_dense"])


def test_the_diagonal_warmup_ends_with_at_most_half_the_step_size(ops):
    """Observed on the MI355X: seed 11 eps 0.823 against 0.2275 (ratio 3.62); seed 1 0.781 against 0.230 (3.39)."""
    dp.check_step_size_against_diagonal(ops, SEED)


def test_sampling_after_the_dense_warmup(ops):
    """Observed on the MI355X: seed 11 eigenvalues 0.914 .. 1.060; seed 1 0.823 .. 1.211 -- inside the bar, but its warmup
    ends at eps = 0.781, where the issue's fixed L = 8 makes a trajectory of 6.245 time units, 0.04 short of the period
    2 pi (dp.check_sampling_after_warmup: on the stand-in seed 7 of nine misses the lower bar for that reason).  The
    library's sums are grouped differently from the stand-in's, so a seed's warmup here is another, equally valid
    adaptation than there; this file uses seed 11, whose step size lies away from the resonance on the device, the CPU file
    seed 1, whose does there."""
    dp.check_sampling_after_warmup(ops, SEED)


def test_checkpoint_carries_the_dense_metric(ops):
    dp.check_checkpoint(ops)


def test_warmup_with_and_without_prefetch_rng(ops):
    dp.check_prefetch_independent(ops)


def test_smc_hmc_kernel_with_the_particles_full_covariance(ops):
    dp.check_smc_dense(ops)
