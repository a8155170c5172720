"""tests/energy_parity.py on the HIP library (bk_energy_update and bk_divergence_capture on the MI355X), and
HMCDiag.track_energy on every path the funnel and the diagonal Gaussian offer, a replayed hipGraph included."""
import numpy as np
import pytest
import torch

import bayes_kit_amd as bk
from bayes_kit_amd import _lib
from tests import energy_parity as ep
from tests.fake_ops_energy import EnergyFakeOps

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    return _lib.default_ops()


# ---- the kernels -----------------------------------------------------------------------------------------------------------------
def test_the_stand_in_restates_the_library_s_scratch_rule(ops):
    for C in (1, 255, 256, 257, 65536):
        assert ops.divergence_capture_work_elems(C) == EnergyFakeOps.divergence_capture_work_elems(C)


@pytest.mark.parametrize("C", ep.UPDATE_CHAINS)
def test_update_exact(ops, C):
    ep.check_update(ops, C)


@pytest.mark.parametrize("C", (65, 1000))
def test_update_with_null_a(ops, C):
    ep.check_update(ops, C, null=True)


@pytest.mark.parametrize("C,off", ((64, 1), (257, 3), (1000, 1)))
def test_update_on_odd_slices(ops, C, off):
    ep.check_update(ops, C, off=off)


@pytest.mark.parametrize("c", ep.CAPTURE_CASES, ids=[ep.capture_id(c) for c in ep.CAPTURE_CASES])
def test_capture_exact(ops, c):
    ep.check_capture(ops, c)


def test_capture_is_deterministic(ops):
    c = ep.CAPTURE_CASES[7]
    a, b = ep.check_capture(ops, c), ep.check_capture(ops, c)
    assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


# ---- the sampler -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def funnel(ops):
    """The issue's run on the opaque path, shared: (sampler, recorder, restated state, restated store)."""
    return ep.check_funnel_run(bk, ops, path="opaque")


def test_funnel_run_opaque(funnel):
    assert len(funnel[1].records) == 40


@pytest.mark.parametrize("kw", ({"path": "step"}, {}, {"path": "opaque", "chain_tile": 64}),
                         ids=("step", "default", "tile-major"))
def test_funnel_run_on_the_other_paths(ops, kw):
    a, rec, ref, store = ep.check_funnel_run(bk, ops, **kw)
    if "chain_tile" in kw:
        assert len(rec.records) == 4 * 40 and a._tm_last   # four tiles a draw, each with its own update and capture


def test_funnel_run_replayed_as_a_graph(ops):
    """graph=True: nothing can be recorded inside a capture, so the tracker is compared with the eager tracked run's."""
    eager, _, _ = ep.run_tracked(bk, ops)
    g, twin = ep.funnel_sampler(bk, ops, graph=True), ep.funnel_sampler(bk, ops, graph=True)
    e = g.track_energy()
    for n in range(40):
        og, ot = g.sample(), twin.sample()
        ep.assert_same_draw(g, twin, og, ot, f"draw {n}: ")
    assert g._graph is not None, "the tracked draws were replayed"
    ep.assert_same_end(g, twin)
    want, got = ep.tracker_host(eager.energy), ep.tracker_host(e)
    for k in want:
        ep._eq(got[k], want[k], "graph against eager: " + k)
    assert e.divergences() > 0


def test_whole_draw_kernel_tracked_against_untracked(ops):
    ep.check_whole_draw(bk, ops)


def test_capacity(ops, funnel):
    ep.check_capacity(bk, ops, funnel[3], path="opaque")


def test_nan_energy_errors(ops):
    ep.check_nan_errors(bk, ops, path="opaque")


def test_readouts(ops, funnel):
    a, rec, ref, store = funnel
    _, _, energies = ep.replay_records(rec.records, 256, 11, 1024)
    pooled = ep.check_readouts(a.energy, energies)
    eb = a.energy.ebfmi().cpu().numpy()
    print("E-BFMI pooled", pooled, "per chain: min", np.nanmin(eb), "median", np.nanmedian(eb))


def test_lifecycle(ops):
    ep.check_lifecycle(bk, ops, path="opaque")


def test_warmup_report_is_unchanged_by_a_tracker(ops):
    ep.check_warmup_report(bk, ops)
