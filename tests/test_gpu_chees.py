"""The jittered trajectory length, the trajectory statistic and HMCDiag.warmup(adapt_trajectory=True) on the MI355X: the
checks of tests/chees_parity.py on the HIP library, the two kernels against their NumPy restatement
(tests/fake_ops_chees.py) bit for bit, and the warmup report against the stand-in's."""
import ctypes

import numpy as np
import pytest
import torch

import bayes_kit_amd as bk
from tests import adapt_parity as ap
from tests import chees_parity as cp
from tests.fake_ops_chees import CheesFakeOps, chees_stat_ref, chees_sums_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    return bk._lib.default_ops()


def _stand_in():
    """The stand-in with the library's host build of bk_exp (the same double as oracle.rng.exp_bk, and faster)."""
    fake = CheesFakeOps()
    fake.exp = bk._lib.load().bk_host_exp
    return fake


# ---- jitter ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ap.PATHS)
def test_jittered_draws_equal_the_oracle_with_the_same_step_counts(ops, path):
    cp.check_jitter_vs_oracle(ops, 300, 48, path)
    cp.check_jitter_vs_oracle(ops, 129, 6, path, T=2.0, max_steps=9)


def test_jittered_draws_do_not_depend_on_the_path_or_the_knobs(ops):
    cp.check_jitter_paths_agree(ops, 300, 48, [dict(), dict(prefetch_rng=True), dict(prefetch_rng=False)])
    cp.check_jitter_paths_agree(ops, 129, 6, [dict(), dict(prefetch_rng=True)])


def test_a_graph_chosen_by_default_is_switched_off_by_the_jitter(ops):
    lam = np.logspace(0, 1, 6)
    s = bk.HMCDiag(bk.DiagGaussian(lam), 0.05, 7, chains=64, seed=1)
    assert s._use_graph
    a = ap.run_draws(s, 3)[0]  # (eager, capture, replay)
    s.set_trajectory_length(0.4)
    assert not s._use_graph
    b = ap.run_draws(s, 3)[0]
    r = bk.HMCDiag(bk.DiagGaussian(lam), 0.05, 7, chains=64, seed=1, graph=False)
    ra = ap.run_draws(r, 3)[0]
    r.set_trajectory_length(0.4)
    rb = ap.run_draws(r, 3)[0]
    assert np.array_equal(a, ra) and np.array_equal(b, rb)
    with pytest.raises(ValueError, match="graph"):
        bk.HMCDiag(bk.DiagGaussian(lam), 0.05, 7, chains=64, seed=1, graph=True, trajectory_length=0.4)


@pytest.mark.parametrize("path", ap.PATHS)
def test_checkpoint_carries_trajectory_length_and_the_jitter_counter(ops, path):
    cp.check_checkpoint(ops, 129, 6, path)
    cp.check_checkpoint(ops, 300, 48, path)


# ---- the kernels ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,D,ld", [(C, D, None) for C, D in cp.SHAPES] + [(4097, 6, None), (65, 5, 72), (257, 33, 300)])
def test_kernels_equal_their_restatement_bit_for_bit(ops, C, D, ld):
    """(4097 chains: 17 workgroups of partials, one of them ragged, for the single-workgroup combine, and 17 terms per thread
    in the per-dimension sums; ld > C: padded rows full of NaN that must not be read)"""
    x = cp.chees_inputs(C, D)
    mean = cp.finite_mean(x)
    outs = [cp.run_chees_ops(ops, x, mean, ld) for _ in range(2)]
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])  # the same bits on every run
    sums, out = outs[0]
    assert np.array_equal(sums, chees_sums_ref(x["theta"], x["theta_p"]))
    exp = bk._lib.load().bk_host_exp
    s, n = chees_stat_ref(x["theta"], x["theta_p"], x["rho_p"], mean, x["lp_cur"], x["a_cur"], x["lp_prop"], x["a_prop"],
                          exp=exp)
    print(f"C = {C} D = {D}: statistic {out[0]!r} (restatement {s!r}), non-finite {out[1]} ({n})")
    assert out[0] == s and out[1] == n and np.isfinite(out[0])
    assert n == (1.0 if x["planted"] else 0.0)
    # ... and without the kinetic energies (NULL = zeros)
    dev = lambda k: torch.from_numpy(x[k]).cuda()  # noqa: E731
    out2 = torch.empty(2, dtype=torch.float64, device="cuda")
    ops.chees_stat(dev("theta"), dev("theta_p"), dev("rho_p"), torch.from_numpy(mean).cuda(), dev("lp_cur"), None,
                   dev("lp_prop"), None, out2)
    s0, n0 = chees_stat_ref(x["theta"], x["theta_p"], x["rho_p"], mean, x["lp_cur"], None, x["lp_prop"], None, exp=exp)
    assert out2[0].item() == s0 and out2[1].item() == n0


def test_no_chains_give_zeros(ops):
    lib = bk._lib.load()
    out = torch.full((2,), -1.0, dtype=torch.float64, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.bk_chees_stat(None, 0, None, 0, None, 0, None, None, None, None, None, out.data_ptr(), None, 0, 3, stream) == 0
    assert out.cpu().tolist() == [0.0, 0.0]


# ---- warmup ---------------------------------------------------------------------------------------------------------
_STAND_IN = {}


def _stand_in_run(C, D):
    if (C, D) not in _STAND_IN:
        fake = _stand_in()
        s, rep = cp.run_chees_warmup(fake, bk.DiagGaussian(np.logspace(0, 1, D), ops=fake), 3, C=C, draws=60, warm=dict())
        _STAND_IN[(C, D)] = (rep, ap.run_draws(s, 2)[0])
    return _STAND_IN[(C, D)]


@pytest.mark.parametrize("path", ["auto", "opaque"])
@pytest.mark.parametrize("C,D", [(258, 40), (65, 130)])
def test_warmup_report_equals_the_numpy_stand_in(ops, C, D, path):
    """warmup(60, adapt_trajectory=True), step size, preconditioner (one window) and trajectory length adapting: every
    history of the report bit for bit, and the two draws that follow."""
    want, after = _stand_in_run(C, D)
    s, rep = cp.run_chees_warmup(ops, bk.DiagGaussian(np.logspace(0, 1, D)), 3, C=C, draws=60, warm=dict(), path=path)
    first = next((i for i, (a, b) in enumerate(zip(rep["T"], want["T"])) if a != b), None)
    print(f"GPU vs stand-in ({C} x {D}, {path}): first difference in T at draw {first}; T {rep['trajectory_length']!r} vs "
          f"{want['trajectory_length']!r}, eps {rep['stepsize']!r} vs {want['stepsize']!r}")
    assert rep["window_ends"] == [54] and len(set(rep["steps"])) > 1
    assert cp.chees_reports_equal(rep, want)
    assert s._fused_draw == (path == "auto")
    assert np.array_equal(ap.run_draws(s, 2)[0], after)


def test_warmup_finds_the_trajectory_length_of_a_unit_gaussian(ops):
    """IsoGaussian(32), 512 chains, from eps = 0.006 and 16 steps: T inside [1.6, 2.4], eps >= 0.4, then 100 draws whose
    pooled variances are within 10 % of 1 (see tests/test_chees_cpu.py for the basis of the band)."""
    s, rep = cp.run_chees_warmup(ops, bk.IsoGaussian(32), 21)
    cp.check_chees_report(rep)
    assert s.trajectory_length == rep["trajectory_length"] and s._fused_draw and not s._use_graph
    cp.check_pooled_variance_after(s)


def test_warmup_report_does_not_depend_on_the_path_the_knobs_or_the_tile(ops):
    """... among them an explicit chain_tile below the chain count on the opaque path: while adapting the tile-major schedule
    (whose velocity lives in a tile's scratch) gives way to column slices of the full arrays."""
    lam = np.logspace(0, 1, 40)
    runs = []
    for kw in (dict(), dict(), dict(prefetch_rng=True), dict(prefetch_rng=False), dict(path="step"), dict(path="opaque"),
               dict(path="opaque", chain_tile=64), dict(path="opaque", chain_tile=64, prefetch_rng=True)):
        s, rep = cp.run_chees_warmup(ops, bk.DiagGaussian(lam), 5, C=258, draws=60, warm=dict(), **kw)
        if "chain_tile" in kw:
            assert s._chain_tile == 64
        sd = s.state_dict()
        after = ap.run_draws(s, 5)
        # a fresh sampler with the tuned values and the warmed one's state continues bit for bit
        f = bk.HMCDiag(bk.DiagGaussian(lam), rep["stepsize"], 16, chains=258, seed=77, precond_diag=rep["precond_diag"],
                       trajectory_length=rep["trajectory_length"], **kw)
        f.load_state_dict(sd)
        again = ap.run_draws(f, 5)
        assert np.array_equal(after[0], again[0]) and np.array_equal(after[1], again[1]), kw
        runs.append((rep, after))
    for (rep, after), kw in zip(runs[1:], "abcdefg"):
        assert cp.chees_reports_equal(runs[0][0], rep), kw
        assert np.array_equal(after[0], runs[0][1][0]) and np.array_equal(after[1], runs[0][1][1]), kw
