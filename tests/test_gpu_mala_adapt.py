"""The preconditioned MALA and MALA.warmup on the MI355X: the checks of tests/mala_adapt_parity.py on the HIP library, the
new kernels against their NumPy restatement (tests/fake_ops_mala_adapt.py), the statistical validity of the preconditioned
sampler, and warmup against the stand-in's recorded reports."""
import hashlib

import numpy as np
import pytest
import torch

import bayes_kit_amd as bk
from tests import mala_adapt_parity as mp
from tests.fake_ops_mala_adapt import MalaAdaptFakeOps

pytestmark = pytest.mark.gpu

# two_pass off / the model-opaque pair / the inlined step kernel, each with the generator on a side stream, in line, and as
# a replayed hipGraph
BASES = [dict(two_pass=False), dict(path="opaque"), dict(path="auto")]
KNOBS = [dict(prefetch_rng=True), dict(prefetch_rng=False), dict(graph=True)]
VARIANTS = [dict(b, **k) for b in BASES for k in KNOBS]


@pytest.fixture(scope="module")
def ops():
    return bk._lib.default_ops()


# ---- 1. against the oracle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["auto", "opaque"])
@pytest.mark.parametrize("C,D", [(300, 48), (130, 130), (129, 6)])
def test_precond_diag_equals_the_oracle_on_the_rescaled_target(ops, C, D, path):
    """(300, 48): two-pass; (130, 130): two-pass with E = 4; (129, 6): step by step, normals in the state layout."""
    s = mp.check_vs_oracle(ops, C, D, path)
    assert ("two-pass" in s.path) == (D >= 32)


# ---- 2. ones --------------------------------------------------------------------------------------------------------
def test_precond_of_ones_is_the_plain_sampler(ops):
    mp.check_identity(ops, 300, 48, [dict(), dict(two_pass=False), dict(path="opaque"), dict(graph=False)])
    mp.check_identity(ops, 129, 6, [dict(), dict(graph=False)])


# ---- 3. paths and knobs -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,D", [(2, 32), (34, 33), (146, 40), (130, 129), (16, 257), (18, 1000), (32, 1024)])
def test_paths_and_knobs_agree_and_the_preconditioner_may_change_between_draws(ops, C, D):
    """The kernel's seams: one pair with rows >= D in slot 0; a ragged last block; 10 workgroups (the XCD-aware walk has a
    remainder); the E 2 -> 4 seam; E = 8; E = 16, the register-heaviest instantiation, ragged and full."""
    mp.check_paths_agree(ops, C, D, VARIANTS)


def test_non_temporal_instantiations_equal_the_step_by_step_path(ops):
    """8,192 x 1,024: the smallest power-of-two shape at which both step kernels take their non-temporal instantiation."""
    C, D = 8192, 1024
    v = mp.perturbed_variances(np.logspace(0, 1, D))
    ref = mp.run_draws(mp.make(ops, C, D, v, two_pass=False, graph=False), 3)
    assert 0 < ref[2].sum() < ref[2].size
    for kw in (dict(path="opaque"), dict(path="auto")):
        got = mp.run_draws(mp.make(ops, C, D, v, graph=False, **kw), 3)
        for x, y in zip(got, ref):
            assert np.array_equal(x, y), kw


# ---- 4. the kernels alone -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gaussian", [False, True])
def test_step_kernels_against_their_cpu_statement(ops, gaussian):
    mp.check_step_kernels(ops, MalaAdaptFakeOps(), gaussian)


def test_propose_and_logq_kernels_against_their_cpu_statement(ops):
    mp.check_propose_kernel(ops, MalaAdaptFakeOps())
    mp.check_logq_kernel(ops, MalaAdaptFakeOps())


# ---- 5. a from-source density -------------------------------------------------------------------------------------------
def test_from_source_density_falls_back_and_equals_the_builtin(ops):
    """An elementwise from_source density has the inlined step kernel but no preconditioned export of it: with precond_diag
    it runs the model-opaque pair, and `path` says so.  Its draws equal the built-in DiagGaussian's on the inlined
    preconditioned kernel -- built with v, given v between draws, and through warmup."""
    from tests.test_gpu_providers import DIAG_SRC  # (the config-3 density as a bk_term)

    C, D = 200, 48
    lam = np.logspace(0, 1, D)
    v = mp.perturbed_variances(lam)
    src = lambda: bk.CTarget.from_source(DIAG_SRC, D, params=torch.as_tensor(lam).cuda())  # noqa: E731
    a, b = mp.make(ops, C, D, v, model=src()), mp.make(ops, C, D, v)
    assert "model-opaque pair" in a.path and "model.bk_mala_step" in b.path
    for x, y in zip(mp.run_draws(a, 6), mp.run_draws(b, 6)):
        assert np.array_equal(x, y)
    assert np.array_equal(a.rng_state(), b.rng_state())
    for pf in (True, False):
        a, b = mp.make(ops, C, D, model=src(), prefetch_rng=pf), mp.make(ops, C, D, prefetch_rng=pf)
        assert "model.bk_mala_step" in a.path
        mp.run_draws(a, 2), mp.run_draws(b, 2)
        a.set_precond_diag(v), b.set_precond_diag(v)
        assert "model-opaque pair" in a.path
        for x, y in zip(mp.run_draws(a, 3), mp.run_draws(b, 3)):
            assert np.array_equal(x, y)
        assert np.array_equal(a.rng_state(), b.rng_state())
    a, b = mp.make(ops, C, D, eps=0.01, model=src()), mp.make(ops, C, D, eps=0.01)
    assert mp.reports_equal(a.warmup(60), b.warmup(60))
    assert np.array_equal(mp.run_draws(a, 2)[0], mp.run_draws(b, 2)[0])


# ---- 6. checkpoint ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,D,kw", [(300, 48, dict()), (300, 48, dict(path="opaque", prefetch_rng=True)), (129, 6, dict())])
def test_checkpoint_carries_preconditioner_and_epsilon(ops, C, D, kw):
    mp.check_checkpoint(ops, C, D, **kw)


# ---- 7. invariance ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(path="auto"), dict(two_pass=False)])
def test_preconditioned_sampler_leaves_the_target_invariant(ops, kw):
    """lam = logspace(0, 2, 32), precond_diag = 1/lam, epsilon = 0.4, 8,192 chains drawn from the target, discard 10 draws,
    pool 30.  A NumPy run of exactly this over six seeds gave max |mean| sqrt(lam) 0.010-0.012, max |var lam - 1|
    0.009-0.014 and an acceptance of 0.615-0.617; with the 1/v weight dropped from the densities the second figure is 0.37,
    with v in place of sqrt(v) on the noise 0.99."""
    lam = np.logspace(0, 2, 32)
    C = 8192
    init = np.random.default_rng(12).normal(size=(C, 32)) / np.sqrt(lam)
    s = bk.MALA(bk.DiagGaussian(lam), 0.4, init=init, seed=12, precond_diag=1.0 / lam, **kw)
    acc = []
    for n in range(40):
        th, _ = s.sample()
        if n >= 10:
            acc.append(th.clone())
    x = torch.stack(acc).reshape(-1, 32).cpu().numpy()
    m, q = np.abs(x.mean(axis=0)) * np.sqrt(lam), np.abs(x.var(axis=0) * lam - 1.0)
    print(f"{kw}: |mean| sqrt(lam) max {m.max():.4f}  |var lam - 1| max {q.max():.4f}  accept {s.accept_rate():.4f}")
    assert m.max() <= 0.03
    assert q.max() <= 0.04
    assert 0.55 <= s.accept_rate() <= 0.68


# ---- 8. / 9. warmup -----------------------------------------------------------------------------------------------------
def _first_difference(a, b):
    return next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None)


def _sha(theta):
    return hashlib.sha256(np.ascontiguousarray(theta).tobytes()).hexdigest()


def test_warmup_end_to_end_and_against_the_stand_in(ops):
    """The end-to-end conditions on the GPU, and the whole report and the two draws that follow against the NumPy stand-in
    (its recorded run, which tests/test_mala_adapt_cpu.py keeps equal to the stand-in): bit for bit."""
    s, rep, lam = mp.run_warmup(ops, 11)
    mp.check_warmup_report(rep, lam)
    assert s._epsilon == rep["stepsize"] and isinstance(s._epsilon, float)
    rec = mp.golden_record(300)
    rc = mp.as_report(rec)
    print(f"GPU vs stand-in: first difference in alpha at draw {_first_difference(rep['alpha'], rc['alpha'])}, in eps at "
          f"{_first_difference(rep['eps'], rc['eps'])}; final v rel "
          f"{float(np.abs(rep['precond_diag'] / rc['precond_diag'] - 1).max()):.3e}, eps {rep['stepsize']!r} vs {rc['stepsize']!r}")
    assert mp.reports_equal(rep, rc)
    assert _sha(mp.run_draws(s, 2)[0]) == rec["after_sha256"]


def test_first_adapted_preconditioner_against_the_stand_in(ops):
    """warmup(110) has one window (draws 17..99): the final v is that window's, the same doubles as the stand-in's."""
    _, rep, _ = mp.run_warmup(ops, 11, draws=110)
    rc = mp.as_report(mp.golden_record(110))
    assert rep["window_ends"] == [99] and rep["alpha"][:99] == rc["alpha"][:99]
    assert np.array_equal(rep["precond_diag"], rc["precond_diag"])


def test_warmup_is_reproducible_whatever_the_path_and_knobs(ops):
    reps, after = [], []
    for kw in (dict(), dict(), dict(prefetch_rng=False), dict(two_pass=False), dict(path="opaque"), dict(graph=True),
               dict(two_pass=False, prefetch_rng=True)):
        s, rep, _ = mp.run_warmup(ops, 3, **kw)
        reps.append(rep)
        after.append(mp.run_draws(s, 3)[0])
    for kw_i, (rep, th) in enumerate(zip(reps[1:], after[1:]), 1):
        assert mp.reports_equal(reps[0], rep), kw_i
        assert np.array_equal(after[0], th), kw_i
    # two pipelined draws before warmup: the proposal made ahead is discarded -- as one run with two_pass=False throughout
    outs = []
    for kw in (dict(prefetch_rng=True), dict(prefetch_rng=False), dict(two_pass=False, prefetch_rng=False)):
        s, rep, _ = mp.run_warmup(ops, 3, draws=60, before=2, **kw)
        outs.append((rep, mp.run_draws(s, 3)[0], s.rng_state().copy()))
    for rep, th, rng in outs[:2]:
        assert mp.reports_equal(rep, outs[2][0]) and np.array_equal(th, outs[2][1]) and np.array_equal(rng, outs[2][2])
