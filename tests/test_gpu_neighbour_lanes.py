"""Neighbour-coupled densities on the lane-spread kernels: CTarget.from_source(form="lanes", neighbour=True), c.sum_pair and
c.grad_pair (csrc/bk_lanes.hpp).  The gradient op against a NumPy restatement in the canonical class order, bit for bit; the
state-space model against autograd and the traced per-chain form; every sampler path against every other and against the oracle
samplers; a Gaussian AR(1) prior's stationary moments."""
import numpy as np
import pytest
import torch

import bayes_kit_amd as bk
from tests import provider_parity as pp
from tests.neighbour_models import SSM_SRC, Ar1Canonical, ar1_params, ar1_src, ssm_torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    return bk._lib.default_ops()


def ar1_target(D, head, device, contract=False):
    return bk.CTarget.from_source(ar1_src(head), D, params=ar1_params(D, device), form="lanes", head=head, neighbour=True,
                                  contract=contract)


def _same_state(a, b):
    return (torch.equal(a._theta_dc, b._theta_dc) and torch.equal(a._rho_dc, b._rho_dc)
            and torch.equal(a._rng_state, b._rng_state) and torch.equal(a._lp, b._lp))


def test_gradient_op_is_the_canonical_order_numpy_model_bit_for_bit(ops):
    """An AR(1) with observations built from + - x only (contract=False): logp and gradient of the op equal the NumPy statement
    in the canonical class order with g_d = dx(d) + dxp(d+1), for 1..8 slots per class and rows walked in memory, every chain
    count (host- and device-counted)."""
    dev = ops.device
    g = torch.Generator(device="cpu").manual_seed(5)
    for head, D in ((0, 1), (1, 2), (2, 17), (0, 16), (1, 18), (2, 101), (0, 128), (1, 129), (2, 131), (0, 300), (2, 302)):
        t = ar1_target(D, head, dev)
        assert t.source_neighbour and hasattr(t, "bk_leapfrog_step") == (D - head <= 128)
        host = Ar1Canonical(D, head)
        for n in (1, 63, 4608, 12293):
            th = torch.randn((D, n), generator=g, dtype=torch.float64).to(dev)
            gr = torch.zeros_like(th)
            lp = torch.zeros(n, dtype=torch.float64, device=dev)
            t.bk_eval(th, gr, lp)
            want_lp, want_g = host.batch(th.cpu().numpy())
            np.testing.assert_array_equal(lp.cpu().numpy(), want_lp, err_msg=f"logp head={head} D={D} n={n}")
            np.testing.assert_array_equal(gr.cpu().numpy(), want_g, err_msg=f"grad head={head} D={D} n={n}")
            # device-counted: chains past *n_dev untouched
            m = max(1, n - 3)
            gn = torch.zeros_like(th)
            t.bk_eval(th, gn, None, n_dev=torch.tensor([m], dtype=torch.int32, device=dev))
            np.testing.assert_array_equal(gn[:, :m].cpu().numpy(), want_g[:, :m])
            assert not gn[:, m:].any()


def test_state_space_source_is_the_pytorch_function(ops):
    """The state-space model as a neighbour lanes source (head = 2): logp and gradient equal torch autograd of the example's
    PyTorch function and the traced form="chain" model on random points, to rel 1e-12."""
    dev = ops.device
    T = 99
    D = T + 2
    fn, y = ssm_torch(T, dev)
    src = bk.CTarget.from_source(SSM_SRC, D, params=torch.cat([torch.zeros(2, dtype=torch.float64, device=dev), y]),
                                 form="lanes", head=2, neighbour=True)
    traced = bk.TorchModel(fn, D, compile=True)
    assert traced.compiled_form == "chain"
    g = torch.Generator(device="cpu").manual_seed(9)
    for n in (1, 70, 5000):
        Th = torch.empty((n, D), dtype=torch.float64)
        Th[:, 0] = 0.5 + 0.3 * torch.randn(n, generator=g, dtype=torch.float64)
        Th[:, 1] = -1.0 + 0.3 * torch.randn(n, generator=g, dtype=torch.float64)
        Th[:, 2:] = y.cpu() + 0.4 * torch.randn((n, T), generator=g, dtype=torch.float64)
        Th = Th.to(dev)
        x = Th.clone().requires_grad_(True)
        lp_a = fn(x)
        (g_a,) = torch.autograd.grad(lp_a.sum(), x)
        lp_s, g_s = src.log_density_gradient(Th)
        lp_t, g_t = traced.log_density_gradient(Th)
        for lp_, g_ in ((lp_s, g_s), (lp_t, g_t)):
            torch.testing.assert_close(lp_, lp_a.detach(), rtol=1e-12, atol=1e-12)
            torch.testing.assert_close(g_, g_a, rtol=1e-12, atol=1e-11)


def test_every_sampler_path_agrees_bit_for_bit(ops):
    """DrGhmcDiag: the one-launch proposals == path="step" (one launch per leapfrog step) == path="opaque" (gradient op + the
    library's kick + drift) == host-counted, with and without a metric, K = 1..4, over chain counts that pick each geometry;
    HMCDiag's one-launch trajectory == its opaque path; the first 64 chains of a 20,000-chain run == a 64-chain run."""
    dev = ops.device
    T = 40
    D = T + 2
    fn, y = ssm_torch(T, dev, seed=4)
    yp = torch.cat([torch.zeros(2, dtype=torch.float64, device=dev), y])
    mk = lambda: bk.CTarget.from_source(SSM_SRC, D, params=yp, form="lanes", head=2, neighbour=True)  # noqa: E731
    init = lambda C: torch.cat([torch.full((C, 1), 0.5, dtype=torch.float64), torch.full((C, 1), -1.0, dtype=torch.float64),  # noqa: E731
                                y.cpu().expand(C, T) + 0.1 * torch.randn((C, T), generator=torch.Generator().manual_seed(C),
                                                                         dtype=torch.float64)], 1)
    cases = [(1, [0.03], [6], 1.0, None, 700),
             (2, [0.04, 0.015], [4, 10], 0.5, "m", 5000),
             (3, [0.05, 0.02, 0.008], [8, 16, 32], 0.2, None, 13000),
             (4, [0.05, 0.025, 0.012, 0.006], [3, 6, 12, 24], 0.3, "m", 300)]
    for K, sizes, counts, damping, metric, C in cases:
        m = None if metric is None else np.linspace(0.6, 1.5, D)
        kw = dict(metric_diag=m, chains=C, seed=13, init=init(C))
        f = bk.DrGhmcDiag(mk(), K, sizes, counts, damping, **kw)
        s = bk.DrGhmcDiag(mk(), K, sizes, counts, damping, path="step", **kw)
        o = bk.DrGhmcDiag(mk(), K, sizes, counts, damping, path="opaque", **kw)
        h = bk.DrGhmcDiag(mk(), K, sizes, counts, damping, device_counts=False, **kw)
        assert f._one_launch and f._dev_counts and s._step_hook and not s._one_launch and not o._step_hook and not h._dev_counts
        for n in range(5):
            tf, Hf = f.sample()
            for x in (s, o, h):
                tx, Hx = x.sample()
                assert torch.equal(tf, tx), (K, C, n)
                # (the returned joint H: the one-launch kernel sums the kinetic energy in its lanes' order)
                torch.testing.assert_close(Hf, Hx, rtol=1e-12, atol=1e-12)
        assert _same_state(f, s) and _same_state(f, o) and _same_state(f, h), K
    # HMC: one launch per trajectory == gradient op per step
    for metric, C in ((None, 3000), ("m", 20000)):
        m = None if metric is None else np.linspace(0.7, 1.3, D)
        a = bk.HMCDiag(mk(), 0.02, 9, metric_diag=m, chains=C, seed=41, init=init(C))
        b = bk.HMCDiag(mk(), 0.02, 9, path="opaque", metric_diag=m, chains=C, seed=41, init=init(C))
        assert a._lanes_traj and not b._lanes_traj and not b._step_hook
        for n in range(5):
            ta, _ = a.sample()
            tb, _ = b.sample()
            assert torch.equal(ta, tb), (C, n)
        np.testing.assert_array_equal(a.rng_state(), b.rng_state())
    # another geometry: the first 64 chains of 20,000 (4 lanes per chain) are a 64-chain run (16 lanes per chain)
    args = (3, [0.05, 0.02, 0.008], [8, 16, 32], 0.2)
    big = bk.DrGhmcDiag(mk(), *args, chains=20000, seed=3, init=init(20000))
    small = bk.DrGhmcDiag(mk(), *args, chains=64, seed=3, init=init(20000)[:64])
    for n in range(5):
        tb, lb = big.sample()
        ts, ls = small.sample()
        assert torch.equal(tb[:64], ts) and torch.equal(lb[:64], ls), n
    np.testing.assert_array_equal(big.rng_state()[:, :64], small.rng_state())


def test_oracle_samplers_on_the_numpy_model(ops):
    """oracle.samplers.DrGhmcDiag and HMCDiag driven by the canonical-order NumPy model give the device samplers' theta bit for
    bit (the one-launch paths of a neighbour build), chain by chain."""
    from oracle import samplers as osamp

    for head, D, C in ((0, 24, 257), (2, 40, 300), (1, 60, 13000)):  # (13,000 chains: 4 lanes per chain in the first stage)
        host = lambda: Ar1Canonical(D, head)  # noqa: E731
        s = bk.DrGhmcDiag(ar1_target(D, head, ops.device), *pp.DR3, chains=C, seed=4601 + head, ops=ops)
        assert s._one_launch
        pp.compare_with_oracle(s, lambda sd: osamp.DrGhmcDiag(host(), *pp.DR3, seed=sd), 6, pp._watch(C), 4601 + head, True)
        h = bk.HMCDiag(ar1_target(D, head, ops.device), 0.05, 7, chains=C, seed=4701 + head, ops=ops)
        assert h._lanes_traj
        pp.compare_with_oracle(h, lambda sd: osamp.HMCDiag(host(), 0.05, 7, seed=sd), 6, pp._watch(C), 4701 + head, True)


GAUSS_AR1_SRC = """
// zero-mean Gaussian AR(1), x_0 at its stationary variance: x_0 ~ N(0, s2 / (1 - phi^2)), x_d ~ N(phi x_{d-1}, s2)
template <class L> __device__ double bk_lanes_density(L& c, const double* p) {
  const double phi = p[0], is2 = p[1], w0 = (1.0 - phi * phi) * is2;
  const double s = c.sum_pair([=](double xp, double x, i64 d) {
    if (d == 0) return (-0.5 * w0) * (x * x);
    const double r = x - phi * xp;
    return (-0.5 * is2) * (r * r);
  });
  c.grad_pair([=](double xp, double x, i64 d) {
    if (d == 0) return bk_pair{0.0, -(w0 * x)};
    const double r = x - phi * xp;
    return bk_pair{(phi * is2) * r, -(is2 * r)};
  });
  return s;
}
"""


def test_gaussian_ar1_stationary_moments(ops):
    """A wrong gradient that is wrong the same way on every path passes the parity tests: the sampled marginal variances and
    lag-1 correlations of a Gaussian AR(1) (head = 0) match s^2 / (1 - phi^2) and phi within Monte-Carlo error."""
    dev = ops.device
    D, C, phi, s2 = 36, 8192, 0.7, 0.5
    t = bk.CTarget.from_source(GAUSS_AR1_SRC, D, params=torch.tensor([phi, 1.0 / s2], dtype=torch.float64, device=dev),
                               form="lanes", head=0, neighbour=True)
    # (trajectory length 1.0 in both stages: a length L reflects the mode of frequency pi / L on every draw, which then never
    # mixes -- at 1.8 that is the period-4 pattern along d -- and pi / 1.0 lies above this prior's spectrum, 2.4 at most)
    dr = bk.DrGhmcDiag(t, 2, [0.25, 0.1], [4, 10], 0.5, chains=C, seed=17)
    assert dr._one_launch
    dr.advance(400)
    var, corr = [], []
    for _ in range(40):
        dr.advance(5)
        th, _ = dr.sample()
        x = th.double()
        x = x - x.mean(0)
        v = (x * x).mean(0)
        var.append(v)
        corr.append((x[:, 1:] * x[:, :-1]).mean(0) / torch.sqrt(v[1:] * v[:-1]))
    var = torch.stack(var).mean(0).cpu().numpy()
    corr = torch.stack(corr).mean(0).cpu().numpy()
    v_true = s2 / (1 - phi * phi)
    # per coordinate: 40 snapshots of 8192 chains (correlated snapshots: count them as ~8 independent ones)
    se_v = v_true * np.sqrt(2.0 / (8 * C))
    se_c = (1 - phi * phi) / np.sqrt(8 * C)
    assert np.all(np.abs(var - v_true) < 6 * se_v), (var.min(), var.max(), v_true)
    assert np.all(np.abs(corr - phi) < 6 * se_c), (corr.min(), corr.max(), phi)
    assert abs(var.mean() - v_true) < 3 * se_v and abs(corr.mean() - phi) < 3 * se_c
