"""CPU side of the logistic target's parity work: the long-double reference (tests/logistic_ref.py) against mpmath at 50
digits, and the shared bodies of tests/logistic_parity.py run on the NumPy stand-in (tests/fake_ops.FakeOps) -- which
checks the bodies, their bounds and the stand-in; the kernels themselves are held to them in tests/test_gpu_logistic.py."""
import numpy as np
import pytest

from tests import logistic_parity as lp
from tests import logistic_ref as ref
from tests.fake_ops import FakeOps


@pytest.fixture(scope="module")
def ops():
    return FakeOps()


def test_reference_against_mpmath_at_50_digits():
    """The long-double forms at a handful of points, extreme |z| included, and one small model end to end: within
    8 long-double epsilons (relative; absolute below the smallest normal double) of the 50-digit value."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    eps = float(np.finfo(np.longdouble).eps)
    zs = [0.0, 1e-300, -1e-300, 0.3, -0.3, 5.0, -5.0, 36.7, -36.7, 37.0, -37.0, 709.0, -709.0, 745.2, -745.2, 800.0, -800.0]
    p, sp = ref.sigmoid_softplus_ld(np.array(zs))
    for z, pi, si in zip(zs, p, sp):
        mz = mp.mpf(z)
        wp, ws = 1 / (1 + mp.exp(-mz)), mp.log1p(mp.exp(mz)) if z < 700 else mz + mp.log1p(mp.exp(-mz))
        assert abs(mp.mpf(float(pi)) + mp.mpf(float(pi - np.longdouble(float(pi)))) - wp) <= 8 * eps * wp + mp.mpf(2) ** -1074, z
        assert abs(mp.mpf(float(si)) + mp.mpf(float(si - np.longdouble(float(si)))) - ws) <= 8 * eps * ws + mp.mpf(2) ** -1074, z
    g = np.random.default_rng(1)
    N, D = 9, 3
    X, th = g.normal(size=(N, D)), 40.0 * g.normal(size=(D, 2))
    y = (g.uniform(size=N) < 0.5).astype(np.float64)
    e = ref.LogisticRef(X, y, prior_scale=2.0).evaluate(th, 0.3)
    inv = mp.mpf(1.0 / 2.0 ** 2)
    for c in range(2):
        z = [mp.fsum(mp.mpf(X[n, d]) * mp.mpf(th[d, c]) for d in range(D)) for n in range(N)]
        sig = [1 / (1 + mp.exp(-v)) for v in z]
        ll = mp.fsum(mp.mpf(y[n]) * z[n] - (z[n] + mp.log1p(mp.exp(-z[n])) if z[n] > 0 else mp.log1p(mp.exp(z[n])))
                     for n in range(N))
        lp_ = mp.mpf(0.3) * ll - inv * mp.fsum(mp.mpf(v) ** 2 for v in th[:, c]) / 2
        assert abs(mp.mpf(e["loglik"][c]) - ll) <= 2.0 ** -52 * abs(ll)
        assert abs(mp.mpf(e["logp"][c]) - lp_) <= 2.0 ** -52 * abs(lp_)
        for n in range(N):
            assert abs(mp.mpf(e["z"][n, c]) - z[n]) <= 2.0 ** -52 * abs(z[n])
            assert abs(mp.mpf(e["r"][n, c]) - (mp.mpf(y[n]) - sig[n])) <= 2.0 ** -52
        for d in range(D):
            G = mp.fsum(mp.mpf(X[n, d]) * (mp.mpf(y[n]) - sig[n]) for n in range(N))
            gd = mp.mpf(0.3) * G - inv * mp.mpf(th[d, c])
            assert abs(mp.mpf(e["G"][d, c]) - G) <= 2.0 ** -52 * abs(G) + 2.0 ** -60
            assert abs(mp.mpf(e["grad"][d, c]) - gd) <= 2.0 ** -52 * abs(gd) + 2.0 ** -60


def test_reference_magnitudes_and_segments():
    g = np.random.default_rng(2)
    z, y = g.normal(size=(9, 4)), np.array([0, 1, 1, 0, 1, 0, 0, 1, 0.25])
    part, pmag, rows = ref.segment_sums(z, y, 2)
    assert rows == 5 and part.shape == (2, 4)
    term = y[:, None] * z - np.logaddexp(0.0, z)
    np.testing.assert_allclose(part, [term[:5].sum(axis=0), term[5:].sum(axis=0)], rtol=1e-14)
    assert np.all(pmag >= np.abs(part))
    part, pmag, rows = ref.segment_sums(z[:5], y[:5], 256)
    assert rows == 1 and np.array_equal(part[5:], np.zeros((251, 4))) and np.array_equal(pmag[5:], np.zeros((251, 4)))
    Y, mag = ref.gemm(z, z.T)
    np.testing.assert_allclose(Y, z @ z.T, rtol=1e-14, atol=1e-15)
    assert np.all(mag >= np.abs(Y))
    # the one-chain model of the fixture generator is the same evaluation, and the oracle's density up to rounding
    from oracle.models import LogisticRegression

    X, th = g.normal(size=(9, 4)), g.normal(size=4)
    m, o = ref.LongDoubleLogistic(X, y, 2.0), LogisticRegression(X, y, 2.0)
    e = ref.LogisticRef(X, y, 2.0).evaluate(th[:, None])
    lp_, gr = m.log_density_gradient(th)
    np.testing.assert_allclose([lp_, m.log_density(th)], e["logp"][0], rtol=2e-16)
    np.testing.assert_allclose(gr, e["grad"][:, 0], rtol=1e-15, atol=1e-16)
    np.testing.assert_allclose(m.log_likelihood(th) + m.log_prior(th), e["logp"][0], rtol=1e-15)
    olp, og = o.log_density_gradient(th)
    np.testing.assert_allclose(lp_, olp, rtol=1e-14)
    np.testing.assert_allclose(gr, og, rtol=1e-13, atol=1e-15)


# ---- the shared bodies on the stand-in -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["chains", "chains_work", "logistic"])
@pytest.mark.parametrize("R,K,C", lp.GEMM_SHAPES)
def test_gemm_bodies_on_the_stand_in(ops, R, K, C, kind):
    lp.check_gemm(ops, kind, R, K, C)


@pytest.mark.parametrize("D,C", lp.METRIC_SHAPES)
def test_dense_metric_body_on_the_stand_in(ops, D, C):
    lp.check_gemm(ops, "metric", D, D, C)


@pytest.mark.parametrize("kind", ["chains", "metric", "logistic"])
@pytest.mark.parametrize("variant", lp.VARIANTS[1:])
def test_broken_precondition_body_on_the_stand_in(ops, variant, kind):
    lp.check_broken_precondition(ops, kind, variant, 256, 256 if kind == "metric" else 64, 256)


def test_gemm_degenerate_sizes_on_the_stand_in(ops):
    lp.check_gemm_degenerate(ops)


@pytest.mark.parametrize("C", lp.RESIDUAL_C)
@pytest.mark.parametrize("N,segments", lp.RESIDUAL_CASES[:-1])
def test_residual_body_on_the_stand_in(ops, N, segments, C):
    lp.check_residual(ops, N, segments, C)


def test_residual_body_with_65535_segments_on_the_stand_in(ops):
    lp.check_residual(ops, *lp.RESIDUAL_CASES[-1], 63)


def test_residual_non_finite_body_on_the_stand_in(ops):
    lp.check_residual_nonfinite(ops)


@pytest.mark.parametrize("segments", [1, 256])
@pytest.mark.parametrize("D,C", [(1, 1), (2, 65), (40, 64), (513, 1000), (1, 1000), (513, 1)])
def test_finish_body_on_the_stand_in(ops, D, C, segments):
    lp.check_finish(ops, D, C, segments)


@pytest.mark.parametrize("scale", lp.THETA_SCALES)
@pytest.mark.parametrize("N,D,C", lp.TARGET_SHAPES[:-1])
def test_target_body_on_the_stand_in(ops, N, D, C, scale):
    lp.check_target(ops, N, D, C, scale)


def test_target_body_on_the_stand_in_at_2049_chains(ops):
    # (one scale: the long-double reference of 5,000 x 2,049 cells is most of a minute of this suite per scale)
    lp.check_target(ops, *lp.TARGET_SHAPES[-1], 1.0)


def test_sharing_invariance_body_on_the_stand_in(ops):
    lp.check_sharing_invariance(ops, N=300, D=5, C=600)


# ---- fixtures run by the reference itself, through the stand-in ------------------------------------------------------------
@pytest.mark.parametrize("name,path", [("hmc_logistic16", "auto"), ("hmc_logistic16", "opaque"), ("hmc_logistic40", "auto")])
def test_hmc_fixture_body_on_the_stand_in(ops, name, path):
    lp.check_logistic_fixture(ops, name, path=path)


@pytest.mark.parametrize("name", ["mala_logistic16", "mala_logistic40"])
def test_mala_fixture_body_on_the_stand_in(ops, name):
    lp.check_logistic_fixture(ops, name)


def test_smc_fixture_body_on_the_stand_in(ops):
    lp.check_logistic_smc_fixture(ops)
