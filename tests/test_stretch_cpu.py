"""bk.Stretcher without a GPU: argument validation, the sampler on the NumPy stand-in (tests/fake_ops_stretch.py) against an
independent per-walker loop, partners, checkpoints, a reference-style model, and bk_stretch_propose's status codes."""
import ctypes

import numpy as np
import pytest

import bayes_kit_amd as bk
from tests import stretch_parity as sp
from tests.fake_ops_stretch import StretchFakeOps


@pytest.fixture()
def ops():
    return StretchFakeOps()


def _model(ops, D=3):
    return bk.DiagGaussian(sp.lam_of(D), ops=ops)


def test_argument_validation(ops):
    m = _model(ops)
    for a in (0.999, 0.0, -2.0, float("nan")):
        with pytest.raises(ValueError, match="stretch bound"):
            bk.Stretcher(m, a=a, seed=1, ops=ops)
    for w in (0, -2, 3, 7, 4.0):
        with pytest.raises(ValueError, match="walkers"):
            bk.Stretcher(m, walkers=w, seed=1, ops=ops)
    for e in (0, -1, 1.5):
        with pytest.raises(ValueError, match="ensembles"):
            bk.Stretcher(m, walkers=4, ensembles=e, seed=1, ops=ops)
    for shape in ((3,), (4, 2), (3, 4), (8, 3), (0,)):
        with pytest.raises(ValueError, match="init"):
            bk.Stretcher(m, walkers=4, init=np.zeros(shape), seed=1, ops=ops)
    bk.Stretcher(m, a=1.0, walkers=4, init=np.zeros((8, 3)), ensembles=2, seed=1, ops=ops)  # the bounds themselves are fine


def test_walkers_default_to_twice_the_dimension(ops):
    for D in (1, 3, 5):
        s = bk.Stretcher(_model(ops, D), seed=2, ops=ops)
        assert s.walkers == 2 * D and s.chains == 2 * D
        th, lp = s.sample()
        assert tuple(th.shape) == (2 * D, D) and tuple(lp.shape) == (2 * D,)
    s = bk.Stretcher(_model(ops, 3), seed=2, ensembles=4, ops=ops)
    assert s.chains == 24 and s.ensembles == 4


@pytest.mark.parametrize("walkers,E,D", [(6, 1, 3), (4, 3, 5)])
def test_sampler_equals_a_plain_per_walker_loop_bit_for_bit(ops, walkers, E, D):
    sp.check_sampler_vs_loop(ops, walkers, E, D, draws=5)
    assert ops.calls["stretch_propose"] == 10 and ops.calls["mh_accept"] == 10 and ops.calls["select_columns"] == 10


def test_streams_follow_the_global_walker_id(ops):
    sp.check_sampler_vs_loop(ops, 4, 2, 3, draws=2, seed=5, chain_id0=1000)


def test_init_is_used_and_the_iterator_protocol_draws(ops):
    init = np.random.default_rng(0).normal(size=(8, 3))
    s = bk.Stretcher(_model(ops), walkers=4, ensembles=2, init=init, seed=3, ops=ops)
    assert np.array_equal(s._theta.numpy(), init)
    assert iter(s) is s
    th, lp = next(s)
    moved = s.last_accept.numpy()
    assert moved.shape == (8,) and np.array_equal(th.numpy()[~moved], init[~moved])
    assert s.accept_rate() == moved.sum() / 8
    # a draw that is returned stays what it was
    keep = th.numpy().copy()
    s.sample()
    assert np.array_equal(th.numpy(), keep)


@pytest.mark.parametrize("walkers,E,D", [(6, 1, 3), (4, 3, 5), (2, 2, 2)])
def test_partners_lie_in_the_other_half_of_the_same_ensemble(ops, walkers, E, D):
    sp.check_partners(ops, walkers, E, D)


@pytest.mark.parametrize("walkers,E,D", [(6, 1, 3), (4, 3, 5)])
def test_state_dict_round_trip_continues_bit_for_bit(ops, walkers, E, D):
    sp.check_state_round_trip(ops, walkers, E, D)


def test_checkpoint_of_another_shape_is_refused(ops):
    sd = sp.make(ops, 4, 3, 5).state_dict()
    with pytest.raises(ValueError):
        sp.make(ops, 6, 2, 5).load_state_dict(sd)  # (as many walkers in all, other ensembles)
    with pytest.raises(ValueError):
        sp.make(ops, 4, 2, 5).load_state_dict(sd)


def test_reference_style_single_point_model_runs(ops):
    """A model with log_density(theta [D]) only, as the reference's own: served walker by walker on the host."""
    class StdNormal:
        def dims(self):
            return 2

        def log_density(self, theta):
            assert theta.shape == (2,)
            return -0.5 * float(theta @ theta)

    s = bk.Stretcher(StdNormal(), walkers=6, seed=4, ops=ops)
    t = bk.Stretcher(bk.IsoGaussian(2, ops=ops), walkers=6, seed=4, ops=ops)
    for _ in range(4):
        (a, la), (b, lb) = s.sample(), t.sample()
        np.testing.assert_allclose(la.numpy(), lb.numpy(), rtol=1e-14)
        assert np.array_equal(a.numpy(), b.numpy())
    assert 0.0 < s.accept_rate() <= 1.0


@pytest.mark.parametrize("H,E,D", [(1, 1, 1), (2, 3, 5), (65, 3, 2)])
def test_kernel_check_passes_on_the_restatement_itself(ops, H, E, D):
    """(the harness the GPU tests run on the device, rehearsed on the stand-in)"""
    for half in (0, 1):
        for inject in (None, "uj0", "uj1", "uz0", "uz1"):
            sp.check_kernel(ops, H, E, D, half, pad=5 * half, inject=inject)


def test_stretch_propose_status_codes_without_a_gpu():
    """BK_E_ARG / BK_OK of bk_stretch_propose are decided before any HIP call (dummy pointers are never read)."""
    lib = bk._lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    OK, E_ARG = 0, -1

    def call(theta=p, ld=8, col_act=0, col_oth=4, n=4, H=2, u_j=p, u_z=p, prop=p, ldp=4, zterm=p, partner=p, D=3):
        return lib.bk_stretch_propose(theta, ld, col_act, col_oth, n, H, u_j, u_z, 0.5, 2.0, prop, ldp, zterm, partner, D, None)

    for name in ("theta", "u_j", "u_z", "prop", "zterm", "partner"):
        assert call(**{name: None}) == E_ARG, name
    assert call(H=0) == E_ARG and call(H=-1) == E_ARG
    assert call(H=3) == E_ARG               # n % H != 0
    assert call(ld=7) == E_ARG              # ld < columns (4 + 4)
    assert call(col_act=4, col_oth=0, ld=7) == E_ARG
    assert call(ldp=3) == E_ARG
    assert call(n=-2) == E_ARG and call(D=-1) == E_ARG and call(col_oth=-4) == E_ARG
    assert call(n=0) == OK and call(n=0, ld=0, col_oth=0, ldp=0) == OK
    assert call(D=0) == OK
    assert call(n=0, H=0) == E_ARG          # (an empty launch still has to be a well-formed one)
