"""CPU side of bk.GLM: the shared bodies of tests/glm_parity.py run on the NumPy stand-in (tests/fake_ops_glm.FakeOpsGLM) --
which checks the bodies, their bounds and the stand-in; every fault the stand-in can plant is shown caught by the body
named for it; and the host logic of bk.GLM (validation, the constant, the buffers).  The kernels themselves are held to
the same bodies in tests/test_gpu_glm.py."""
import math

import numpy as np
import pytest
import torch

import bayes_kit_amd as bk
from tests import glm_parity as gp
from tests import glm_ref as ref
from tests.fake_ops_glm import FAULTS, FakeOpsGLM, GLMFakeMixin
from tests.fake_ops_temper_hmc import TemperHmcFakeOps

FAM_OFF = [(f, o) for f in gp.FAMILIES for o in (False, True)]


@pytest.fixture(scope="module")
def ops():
    return FakeOpsGLM()


# ---- the shared bodies on the stand-in -----------------------------------------------------------------------------------
@pytest.mark.parametrize("family,offset", FAM_OFF)
@pytest.mark.parametrize("R,K,C", gp.EPILOGUE_SHAPES)
def test_epilogue_equals_pass_on_the_stand_in(ops, R, K, C, family, offset):
    gp.check_epilogue_equals_pass(ops, family, offset, R, K, C)


@pytest.mark.parametrize("variant", ["lda_odd", "ldx_odd", "a_off", "x_off"])
@pytest.mark.parametrize("family,offset", FAM_OFF)
def test_broken_precondition_on_the_stand_in(ops, family, offset, variant):
    gp.check_broken_precondition(ops, family, offset, variant)


@pytest.mark.parametrize("R,K,C", gp.EPILOGUE_SHAPES)
def test_bernoulli_is_the_logistic_entry_points_on_the_stand_in(ops, R, K, C):
    gp.check_bernoulli_is_logistic(ops, R, K, C)


@pytest.mark.parametrize("C", gp.RESIDUAL_C)
@pytest.mark.parametrize("N,segments", gp.RESIDUAL_CASES)
@pytest.mark.parametrize("family,offset", FAM_OFF)
def test_cells_on_the_stand_in(ops, family, offset, N, segments, C):
    gp.check_cells(ops, family, offset, N, segments, C)


@pytest.mark.parametrize("family,offset", FAM_OFF)
def test_non_finite_cells_on_the_stand_in(ops, family, offset):
    gp.check_nonfinite(ops, family, offset)


def test_argument_checks_on_the_stand_in(ops):
    gp.check_arguments(ops)


@pytest.mark.parametrize("family,offset", FAM_OFF)
@pytest.mark.parametrize("N,D,C", gp.TARGET_SHAPES)
def test_target_on_the_stand_in(ops, N, D, C, family, offset):
    gp.check_target(ops, family, offset, N, D, C)


@pytest.mark.parametrize("offset", [False, True])
def test_gaussian_closed_form_on_the_stand_in(ops, offset):
    gp.check_gaussian_closed_form(ops, offset)


@pytest.mark.parametrize("family", gp.FAMILIES)
def test_non_finite_chain_on_the_stand_in(ops, family):
    gp.check_nonfinite_chain(ops, family)


@pytest.mark.parametrize("family", ["poisson", "gaussian"])
def test_sharing_invariance_on_the_stand_in(ops, family):
    gp.check_sharing_invariance(ops, family, N=300, D=5, C=600)


@pytest.mark.parametrize("kind", ["hmc", "hmc_opaque", "mala", "smc"])
def test_bernoulli_drop_in_on_the_stand_in(ops, kind):
    gp.check_drop_in(ops, kind)


@pytest.mark.parametrize("family", ["binomial", "poisson", "gaussian"])
def test_constant_survives_evaluations_at_other_widths_on_the_stand_in(ops, family):
    gp.check_constant_survives_other_widths(ops, family)


def test_two_samplers_of_different_widths_on_one_model_on_the_stand_in(ops):
    gp.check_two_samplers_on_one_model(ops)


def test_invariance_hmc_on_the_stand_in(ops):
    gp.check_invariance_hmc(ops)


def test_invariance_tempered_on_the_stand_in():
    class Ops(GLMFakeMixin, TemperHmcFakeOps):
        pass

    gp.check_invariance_tempered(Ops())


# ---- every planted fault is caught at the case named for it ----------------------------------------------------------------
CAUGHT_BY = {
    "aux_not_advanced": lambda o: gp.check_epilogue_equals_pass(o, "binomial", False, 1000, 512, 256),
    "offset_not_advanced": lambda o: gp.check_epilogue_equals_pass(o, "poisson", True, 1000, 512, 256),
    "offset_after_exp": lambda o: gp.check_cells(o, "poisson", True, 9, 2, 63),
    "binomial_m_not_in_term": lambda o: gp.check_cells(o, "binomial", False, 9, 2, 63),
    "gaussian_precision_dropped_from_r": lambda o: gp.check_cells(o, "gaussian", False, 9, 2, 63),
    "poisson_term_from_yz": lambda o: gp.check_cells(o, "poisson", True, 9, 2, 63),
    "const_per_segment": lambda o: gp.check_target(o, "poisson", False, 130, 1, 1),
    "const_left_out_of_loglik": lambda o: gp.check_target(o, "gaussian", True, 130, 1, 1),
    "null_part_changes_r": lambda o: gp.check_cells(o, "bernoulli", False, 9, 2, 63),
}


def test_every_fault_has_its_case():
    assert sorted(CAUGHT_BY) == sorted(FAULTS)


@pytest.mark.parametrize("fault", FAULTS)
def test_planted_fault_is_caught(fault):
    CAUGHT_BY[fault](FakeOpsGLM())  # (the case passes on the faultless stand-in ...)
    with pytest.raises(AssertionError):
        CAUGHT_BY[fault](FakeOpsGLM(fault))


def test_seam_faults_are_invisible_away_from_the_seam():
    """... and an all-FULL shape has no second launch: the not-advanced pointers are only seen where R_full < R."""
    for fault in ("aux_not_advanced", "offset_not_advanced"):
        gp.check_epilogue_equals_pass(FakeOpsGLM(fault), "binomial", True, 256, 64, 256)


# ---- host logic ------------------------------------------------------------------------------------------------------------
def _data(N=12, D=3):
    g = np.random.default_rng(0)
    return g.normal(size=(N, D)), g


def test_validation_errors(ops):
    X, g = _data()
    N = X.shape[0]
    y01, cnt, m = (g.uniform(size=N) < 0.5) * 1.0, g.poisson(3.0, size=N) * 1.0, np.full(N, 20.0)
    bad = lambda v, i, x: np.where(np.arange(N) == i, x, v)  # noqa: E731
    ok = lambda **kw: bk.GLM(X, kw.pop("y"), kw.pop("family"), ops=ops, **kw)  # noqa: E731
    ok(y=y01, family="bernoulli")
    ok(y=np.full(N, 0.25), family="bernoulli")  # fractions stay allowed
    ok(y=cnt, family="binomial", trials=m)
    ok(y=cnt, family="poisson", offset=np.zeros(N))
    ok(y=cnt, family="gaussian", noise_sd=0.5)
    ok(y=cnt, family="gaussian", noise_sd=np.full(N, 0.5))
    cases = [
        dict(y=y01, family="probit"),
        dict(y=bad(y01, 2, 1.5), family="bernoulli"), dict(y=bad(y01, 2, -0.1), family="bernoulli"),
        dict(y=bad(y01, 0, np.nan), family="bernoulli"),
        dict(y=cnt, family="binomial"),                                    # trials required
        dict(y=bad(cnt, 1, 21.0), family="binomial", trials=m), dict(y=bad(cnt, 1, -1.0), family="binomial", trials=m),
        dict(y=cnt, family="binomial", trials=bad(m, 3, np.inf)), dict(y=cnt, family="binomial", trials=m[:-1]),
        dict(y=bad(cnt, 4, -1.0), family="poisson"), dict(y=bad(cnt, 4, np.inf), family="poisson"),
        dict(y=cnt, family="gaussian"),                                    # noise_sd required
        dict(y=cnt, family="gaussian", noise_sd=0.0), dict(y=cnt, family="gaussian", noise_sd=-1.0),
        dict(y=cnt, family="gaussian", noise_sd=np.inf), dict(y=cnt, family="gaussian", noise_sd=bad(m, 0, np.nan)),
        dict(y=cnt, family="gaussian", noise_sd=np.ones(N + 1)),
        dict(y=cnt, family="poisson", offset=bad(m, 5, np.inf)), dict(y=cnt, family="poisson", offset=np.zeros(N - 1)),
        dict(y=cnt[:-1], family="poisson"),
        # an argument that does not belong to the family
        dict(y=y01, family="bernoulli", trials=m), dict(y=cnt, family="poisson", trials=m),
        dict(y=cnt, family="gaussian", noise_sd=1.0, trials=m), dict(y=y01, family="bernoulli", noise_sd=1.0),
        dict(y=cnt, family="binomial", trials=m, noise_sd=1.0), dict(y=cnt, family="poisson", noise_sd=1.0),
    ]
    for kw in cases:
        with pytest.raises(ValueError):
            ok(**dict(kw))


def test_constant_is_the_double_nearest_the_exact_sum(ops):
    X, g = _data(N=500)
    N = X.shape[0]
    m = 1.0 + g.integers(0, 40, size=N)
    yb = np.floor(g.uniform(size=N) * (m + 1))
    yp = g.poisson(30.0, size=N) * 1.0
    sd = g.uniform(0.1, 3.0, size=N)
    assert bk.GLM(X, (yb > 0) * 1.0, "bernoulli", ops=ops)._ll_const == 0.0
    assert bk.GLM(X, yb, "binomial", trials=m, ops=ops)._ll_const == math.fsum(
        math.lgamma(a + 1) - math.lgamma(b + 1) - math.lgamma(a - b + 1) for a, b in zip(m.tolist(), yb.tolist()))
    assert bk.GLM(X, yp, "poisson", ops=ops)._ll_const == math.fsum(-math.lgamma(v + 1) for v in yp.tolist())
    w = 1.0 / (sd * sd)
    assert bk.GLM(X, yp, "gaussian", noise_sd=sd, ops=ops)._ll_const == math.fsum(
        0.5 * (math.log(v) - math.log(2 * math.pi)) for v in w.tolist())
    assert bk.GLM(X, yp, "gaussian", noise_sd=2.0, ops=ops)._ll_const == math.fsum(
        [0.5 * (math.log(1.0 / (2.0 * 2.0)) - math.log(2 * math.pi))] * N)
    assert gp.fsum_constant("poisson", yp, None) == bk.GLM(X, yp, "poisson", ops=ops)._ll_const


def test_log_likelihood_includes_the_constant_once_and_the_split_adds_up(ops):
    """Poisson, small enough to write out: loglik = sum (y eta - e^eta - log y!), at every width the buffers are used at."""
    X, g = _data(N=40, D=3)
    y = g.poisson(2.0, size=40) * 1.0
    off = g.normal(size=40) * 0.1
    m = bk.GLM(X, y, "poisson", 1.5, offset=off, ops=ops)
    assert m.dims() == 3 and m.family == "poisson"
    for C in (7, 3, 7, 9):
        Th = torch.from_numpy(g.normal(size=(C, 3)) * 0.3)
        eta = X @ Th.numpy().T + off[:, None]
        want = (y[:, None] * eta - np.exp(eta)).sum(axis=0) - sum(math.lgamma(v + 1) for v in y)
        np.testing.assert_allclose(m.log_likelihood(Th).numpy(), want, rtol=1e-13)
        np.testing.assert_allclose(m.log_density(Th).numpy(), want + m.log_prior(Th).numpy(), rtol=1e-13)
        ll, gl = m.log_likelihood_gradient(Th)
        lp0, g0 = m.log_prior_gradient(Th)
        lpd, gd = m.log_density_gradient(Th)
        np.testing.assert_allclose((ll + lp0).numpy(), lpd.numpy(), rtol=1e-13)
        np.testing.assert_allclose((gl + g0).numpy(), gd.numpy(), rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(gl.numpy(), ((y[:, None] - np.exp(eta)).T @ X), rtol=1e-12, atol=1e-13)


def test_logistic_regression_keeps_its_sequence_of_ops_calls(ops):
    """The shared base changes nothing LogisticRegression sends to the kernel library: the same calls, in the same order."""
    X, g = _data(N=30, D=3)
    y = (g.uniform(size=30) < 0.5) * 1.0
    calls = []

    spied = ("gemm_chains", "gemm_chains_logistic", "logistic_residual", "logistic_finish", "gemm_chains_glm", "glm_residual")
    depth = [0]

    def spy(name, fn):
        def wrapper(*a, **kw):
            if depth[0] == 0:  # (the stand-in's own nested calls are not the target's)
                calls.append(name)
            depth[0] += 1
            try:
                return fn(*a, **kw)
            finally:
                depth[0] -= 1
        return wrapper

    sops = FakeOpsGLM()
    for name in spied:
        setattr(sops, name, spy(name, getattr(sops, name)))
    m = bk.LogisticRegression(X, y, ops=sops)
    th = torch.from_numpy(g.normal(size=(3, 5)))
    gr, lpv = torch.empty((3, 5), dtype=torch.float64), torch.empty(5, dtype=torch.float64)
    m.bk_eval(th, gr, None)
    assert calls == ["gemm_chains_logistic", "gemm_chains", "logistic_finish"]
    del calls[:]
    m.bk_eval(th, gr, lpv)
    assert calls == ["gemm_chains", "logistic_residual", "gemm_chains", "logistic_finish"]
    del calls[:]
    m.bk_eval(th, None, lpv)
    assert calls == ["gemm_chains", "logistic_residual", "logistic_finish"]
    assert ref.TERM_OPS["bernoulli"] == 8
