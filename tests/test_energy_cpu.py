"""tests/energy_parity.py without a GPU: the checks pass on the NumPy stand-in that walks the launches of bk_energy_update and
bk_divergence_capture; each of the stand-in's planted faults -- one broken seam each -- makes a check fail; the library's
argument checks (no device needed); HMCDiag.track_energy on every path the stand-in supports; EnergyDiagnostics' host logic;
and two gloo ranks against one process."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import bayes_kit_amd as bk
from tests import energy_parity as ep
from tests import fake_ops_energy as fe
from tests.fake_ops_energy import EnergyAdaptFakeOps, EnergyFakeOps

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def ops():
    return EnergyFakeOps()


# ---- the kernel checks on the fault-free stand-in ------------------------------------------------------------------------------
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


def test_capture_cases_cover_what_they_claim():
    mid = ep.CAPTURE_CASES[7]
    assert int(ep.flags("random", mid.C, 0).sum()) > mid.cap
    assert int(ep.flags("edges", 1000).sum()) == ep.CAPTURE_CASES[4].cap == 6
    assert {c.D for c in ep.CAPTURE_CASES} == {1, 3, 130}


# ---- each planted fault is noticed -----------------------------------------------------------------------------------------------
FAULT_CHECKS = {
    "le": lambda o: ep.check_update(o, 256),
    "nan_ok": lambda o: ep.check_update(o, 256),
    "e_h1": lambda o: ep.check_update(o, 65),
    "nonfinite_welford": lambda o: ep.check_update(o, 65, null=True),
    "ssd_first": lambda o: ep.check_update(o, 1),
    "delta_sq": lambda o: ep.check_update(o, 63, off=1),
    "arrival": lambda o: ep.check_capture(o, ep.CAPTURE_CASES[0]),
    "overrun": lambda o: ep.check_capture(o, ep.CAPTURE_CASES[3]),
    "chain0": lambda o: ep.check_capture(o, ep.CAPTURE_CASES[1]),
    "pitch": lambda o: ep.check_capture(o, ep.CAPTURE_CASES[2]),
}


def test_every_fault_has_a_check():
    assert sorted(FAULT_CHECKS) == sorted(fe.FAULTS)


@pytest.mark.parametrize("fault", sorted(FAULT_CHECKS))
def test_fault_is_noticed_by_a_kernel_check(fault):
    with pytest.raises(AssertionError, match="differs from the NumPy restatement") as e:
        FAULT_CHECKS[fault](EnergyFakeOps(fault))
    print(fault, e.value)


@pytest.mark.parametrize("fault", ("overrun", "arrival"))
def test_capture_faults_are_noticed_where_the_store_fills(fault):
    with pytest.raises(AssertionError, match="differs from the NumPy restatement"):
        ep.check_capture(EnergyFakeOps(fault), ep.CAPTURE_CASES[7])


# ---- the library without a device ------------------------------------------------------------------------------------------------
def test_c_abi_argument_checks():
    from bayes_kit_amd import _lib

    ep.check_abi_errors(_lib.load())
    assert EnergyFakeOps.divergence_capture_work_elems(65536) == _lib.load().bk_divergence_capture_work_elems(65536)


# ---- the sampler on the stand-in -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def funnel(ops):
    """The issue's run on the opaque path, shared: (sampler, recorder, restated state, restated store)."""
    return ep.check_funnel_run(bk, ops, model_ops=ops, path="opaque")


def test_funnel_run_opaque(funnel):
    a, rec, ref, store = funnel
    assert len(rec.records) == 40


@pytest.mark.parametrize("kw", ({"path": "step"}, {}, {"path": "opaque", "chain_tile": 64}),
                         ids=("step", "default", "tile-major"))
def test_funnel_run_on_the_other_paths(ops, funnel, kw):
    a, rec, ref, store = ep.check_funnel_run(bk, ops, model_ops=ops, **kw)
    if "chain_tile" in kw:
        assert len(rec.records) == 4 * 40 and a._tm_last   # four tiles a draw, each with its own update and capture
    # every path gives the same draws, so the same tracker
    for k in ref:
        ep._eq(ref[k], funnel[2][k], k)
    for k in store:
        ep._eq(store[k], funnel[3][k], k)


def test_whole_draw_kernel_tracked_against_untracked(ops):
    ep.check_whole_draw(bk, ops, model_ops=ops)


def test_single_chain_host_model_goes_through_the_same_accept(ops):
    class Model:
        def dims(self):
            return 3

        def log_density(self, th):
            return float(-0.5 * np.dot(th, th))

        def log_density_gradient(self, th):
            return self.log_density(th), -np.asarray(th)

    rec = ep.RecordingOps(ops)
    a, b = (bk.HMCDiag(Model(), 0.4, 5, seed=3, ops=o) for o in (rec, ops))
    rec.sampler = a
    e = a.track_energy(threshold=1.0)
    for _ in range(20):
        (ta, la), (tb, lb) = a.sample(), b.sample()
        assert np.array_equal(ta, tb) and la == lb
    ref, store, energies = ep.replay_records(rec.records, 1, 3, e.capture, threshold=1.0)
    ep.assert_tracker_equals(e, ref, store)
    assert e.transitions == 20
    ep.check_readouts(e, energies)


def test_capacity(ops, funnel):
    ep.check_capacity(bk, ops, funnel[3], model_ops=ops, path="opaque")


def test_nan_energy_errors(ops):
    ep.check_nan_errors(bk, ops, model_ops=ops, path="opaque")


def test_readouts(ops, funnel):
    a, rec, ref, store = funnel
    _, _, energies = ep.replay_records(rec.records, 256, 11, 1024)
    pooled = ep.check_readouts(a.energy, energies)
    e = a.energy
    print("E-BFMI pooled", pooled, "per chain: min", np.nanmin(e.ebfmi().numpy()), "median", np.nanmedian(e.ebfmi().numpy()))
    assert np.array_equal(e.divergences_per_chain.numpy(), ref["ndiv"])
    assert np.array_equal(e.last_divergent.numpy(), ref["div_mask"].astype(bool))
    assert np.array_equal(e.last_energy_error.numpy(), ref["err"], equal_nan=True)
    assert e.divergence_rate() == ref["totals"][1] / ref["totals"][0]
    assert e.nan_transitions() == ref["totals"][2] and e.nonfinite_energies() == ref["totals"][3]
    ds = e.divergent_states()
    assert sorted(ds) == ["chain", "draw", "energy_error", "seen", "stored", "theta"]
    assert (ds["draw"].numpy() >= 1).all() and (ds["draw"].numpy() <= 40).all()
    assert np.array_equal(np.sort(ds["draw"].numpy()), ds["draw"].numpy())          # call order
    for d in np.unique(ds["draw"].numpy()):                                         # ascending chains within a call
        ch = ds["chain"].numpy()[ds["draw"].numpy() == d]
        assert (np.diff(ch) > 0).all()
    err = ds["energy_error"].numpy()
    assert (np.isnan(err) | (err < -1000.0)).all()


def test_sampler_level_checks_notice_faults(ops, funnel):
    """The sampler checks have teeth as well: the tracker-against-restatement comparison, the capacity check and the NaN
    check each fail on a stand-in with a planted fault."""
    with pytest.raises(AssertionError, match="differs from the NumPy restatement"):
        ep.check_funnel_run(bk, EnergyFakeOps("e_h1"), model_ops=ops, path="opaque")
    with pytest.raises(AssertionError):
        ep.check_capacity(bk, EnergyFakeOps("overrun"), funnel[3], model_ops=ops, path="opaque")
    with pytest.raises(AssertionError):
        ep.check_nan_errors(bk, EnergyFakeOps("nan_ok"), model_ops=ops, path="opaque")
    a, rec, _ = ep.run_tracked(bk, EnergyFakeOps("delta_sq"), draws=10, model_ops=ops, path="opaque")
    _, _, energies = ep.replay_records(rec.records, 256, 11, 1024)
    with pytest.raises(AssertionError):
        ep.check_readouts(a.energy, energies)


def test_lifecycle(ops):
    ep.check_lifecycle(bk, ops, model_ops=ops, path="opaque")


def test_warmup_report_is_unchanged_by_a_tracker():
    o = EnergyAdaptFakeOps()
    rep, e = ep.check_warmup_report(bk, o, model_ops=o)
    assert "nan_chains" in rep and e.divergences() >= 0


def test_tracking_drops_captured_graphs_and_allocates_nothing_per_draw(ops):
    s = ep.funnel_sampler(bk, ops, ops, path="opaque")
    s._graph, s._graph_warm = object(), 1
    e = s.track_energy()
    assert s._graph is None and s._graph_warm == 0
    ptrs = {k: t.data_ptr() for k, t in e._tensors().items()}
    s.sample(), s.sample()
    assert ptrs == {k: t.data_ptr() for k, t in e._tensors().items()}
    s._graph, s._graph_warm = object(), 1
    s.untrack_energy()
    assert s._graph is None and s.energy is None


# ---- EnergyDiagnostics on its own ---------------------------------------------------------------------------------------------
def test_constructor_and_update_errors(ops):
    for kw in (dict(C=0), dict(C=4, D=0), dict(C=4, threshold=0.0), dict(C=4, threshold=float("inf")),
               dict(C=4, threshold=float("nan")), dict(C=4, D=2, capture=-1)):
        with pytest.raises(ValueError):
            bk.EnergyDiagnostics(ops=ops, **kw)
    e = bk.EnergyDiagnostics(8, 2, chain_id0=100, ops=ops)
    z = torch.zeros(8, dtype=torch.float64)
    with pytest.raises(ValueError, match="do not lie inside"):
        e.update(z[:4], z[:4], z[:4], z[:4], z[:4])                       # a part without chain0
    with pytest.raises(ValueError, match="do not lie inside"):
        e.update(z[:4], z[:4], z[:4], z[:4], z[:4], chain0=106)          # runs past the end
    with pytest.raises(ValueError, match="start state"):
        e.update(z, z, z, z, z, theta=torch.zeros((3, 8), dtype=torch.float64))
    e.update(z[:4], z[:4], z[:4], z[:4], z[:4] - 1.0, chain0=104)
    assert e.transitions == 4 and e.trans.tolist() == [0, 0, 0, 0, 1, 1, 1, 1] and e.divergences() == 0
    assert np.isnan(e.ebfmi().numpy()).all() and np.isnan(e.ebfmi_pooled())
    assert np.isnan(e.energy_mean().numpy()[:4]).all() and (e.energy_mean().numpy()[4:] == 0.0).all()
    # without D no state is kept; divergences are still counted and seen
    n = bk.EnergyDiagnostics(8, ops=ops)
    n.update(z, z, z - 5000.0, z, z - 1.0)
    ds = n.divergent_states()
    assert n.divergences() == 8 and ds["stored"] == 0 and ds["seen"] == 8 and ds["theta"] is None


def test_standalone_updates_match_the_restatement(ops):
    C, D = 300, 3
    e = bk.EnergyDiagnostics(C, D, threshold=ep.THRESHOLD, capture=16, chain_id0=9, ops=ops)
    ref, store = fe.new_state(C), fe.new_store(D, 16)
    for step in range(3):
        v = ep.update_inputs(C, step)
        theta = np.random.default_rng(step).normal(size=(D, C))
        e.update(*(torch.from_numpy(v[k]) for k in ("lp_cur", "a_cur", "lp_prop", "a_prop", "log_u")),
                 theta=torch.from_numpy(theta))
        fe.energy_ref(ref, v["lp_cur"], v["a_cur"], v["lp_prop"], v["a_prop"], v["log_u"], ep.THRESHOLD)
        fe.capture_ref(store, ref["div_mask"], ref["err"], ref["trans"], theta, 9)
    ep.assert_tracker_equals(e, ref, store)
    ds = e.divergent_states()
    assert ds["stored"] == 16 < ds["seen"] and (ds["chain"].numpy() >= 9).all()


# ---- two ranks -----------------------------------------------------------------------------------------------------------------
def test_two_rank_gloo_divergences_and_pooled_ebfmi():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "energy_dist_worker.py")], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=240)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(out)
    for rank, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, out
        assert f"rank {rank} ok" in out
