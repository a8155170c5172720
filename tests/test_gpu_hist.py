"""tests/hist_parity.py on the HIP library (bk_hist_accumulate on the MI355X), and one end-to-end run: HMC warmup, moments,
a grid from the moments, medians and 90 % intervals of every coordinate from the histogram."""
import numpy as np
import pytest
import torch

import bayes_kit_amd as bk
from bayes_kit_amd import _lib
from tests import fake_ops_hist as fh
from tests import hist_parity as hp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    return _lib.default_ops()


def _ids(cases):
    return [hp.case_id(c) for c in cases]


def test_the_stand_in_restates_the_library_s_plan(ops):
    """The seam cases below are built from the stand-in's slab and window (collection needs no device): they are the
    library's."""
    assert ops.hist_lds_bins() == fh.LDS_BINS
    assert hp.slab_cases(ops) == hp.slab_cases(fh.HistFakeOps()) and hp.window_cases(ops) == hp.window_cases(fh.HistFakeOps())


@pytest.mark.parametrize("c", hp.BASE_CASES, ids=_ids(hp.BASE_CASES))
def test_exact(ops, c):
    hp.check_exact(ops, c)


@pytest.mark.parametrize("c", hp.BIN_CASES, ids=_ids(hp.BIN_CASES))
def test_exact_bin_counts(ops, c):
    hp.check_exact(ops, c)


_SLAB_CASES = hp.slab_cases(fh.HistFakeOps())
_WINDOW_CASES = hp.window_cases(fh.HistFakeOps())


@pytest.mark.parametrize("c", _SLAB_CASES, ids=_ids(_SLAB_CASES))
def test_exact_at_the_slab_seam(ops, c):
    hp.check_exact(ops, c)


@pytest.mark.parametrize("c", _WINDOW_CASES, ids=_ids(_WINDOW_CASES))
def test_exact_at_the_lds_window_seam(ops, c):
    hp.check_exact(ops, c)


def test_edges_land_in_their_bins(ops):
    hp.check_edges_land_in_their_bins(ops)


@pytest.mark.parametrize("kind,B", [("dyadic", 64), ("nondyadic", 37)])
def test_all_equal_rows(ops, kind, B):
    hp.check_all_equal_rows(ops, kind, B)


def test_accumulation(ops):
    hp.check_accumulation(ops)


@pytest.mark.parametrize("c", [hp.Case("nondyadic", 5, hp.SEAM_C, 37, 1), hp.Case("nondyadic", 2, hp.SEAM_C, fh.LDS_BINS + 1, 1)],
                         ids=["one-window", "two-windows"])
def test_deterministic(ops, c):
    hp.check_deterministic(ops, c)


def test_quantile_bound(ops):
    assert hp.check_quantile_bound(ops, bk) <= 1.0


def test_running_histogram_counts(ops):
    hp.check_running_histogram_counts(ops, bk)


def test_hmc_medians_and_intervals_end_to_end(ops):
    """HMCDiag on DiagGaussian([1, 4, 0.25, 100]), 2,048 chains: warmup(100), 20 draws into RunningMoments, from_moments, 50
    draws into the histogram.  coverage == 1 to 1e-3; the counts equal the stand-in's on the same draws; median and the ends
    of interval(0.9) within one bin width + 5 MCSE of 0 and -/+1.6449 / sqrt(lam), MCSE = sd / sqrt(ess) with ess taken as
    the number of chains (independent chains: a lower bound on the effective draws)."""
    lam = np.array([1.0, 4.0, 0.25, 100.0])
    D, C = 4, 2048
    s = bk.HMCDiag(bk.DiagGaussian(torch.from_numpy(lam)), 0.1, 8, chains=C, seed=20)
    s.warmup(100)
    rm = bk.RunningMoments(D, C)
    for _ in range(20):
        theta, _ = s.sample()
        rm.update(theta)
    h = bk.RunningHistogram.from_moments(rm)
    host = bk.RunningHistogram(h._lo_h, h._hi_h, bins=h.bins, ops=fh.HistFakeOps())
    for _ in range(50):
        theta, _ = s.sample()
        h.update(theta)
        host.update(theta.cpu())
    assert h.n == 50 * C
    cov = h.coverage()
    print("coverage", cov)
    assert (np.abs(cov - 1.0) <= 1e-3).all()
    assert np.array_equal(h.counts().cpu().numpy(), host.counts().numpy())
    sd = 1.0 / np.sqrt(lam)
    width = 1.0 / h._scale_h
    tol = width + 5.0 * sd / np.sqrt(C)
    med = h.median()
    lower, upper = h.interval(0.9)
    for name, got, want in (("median", med, 0.0 * sd), ("lower", lower, -1.6449 * sd), ("upper", upper, 1.6449 * sd)):
        print(name, got, "want", want, "err / tol", np.abs(got - want) / tol)
        assert (np.abs(got - want) <= tol).all(), name
