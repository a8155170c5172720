"""HMCDiag's and MALA's randomness generated ahead (prefetch_rng) at the operations that have to drop it between two draws: a sampler
that generates ahead and one that does not stay equal bit for bit -- stream position, draws, log densities -- across each
of them.  130 chains (a ragged third wavefront, just past a 128-chain tile); D = 8 generates the momentum ahead in the state
layout (the logical position is a copy queued in front of the generator), D = 40 chain-major normals (the generator's own
snapshot).  MALA: D = 8 runs step by step (the logical position is the copy in front of the generator), D = 40 two-pass (the
snapshot inside the unit the last draw consumed)."""
import numpy as np
import pytest
import torch

import bayes_kit_amd as bk
from tests import adapt_parity as ap
from tests import mala_adapt_parity as mp
from tests.test_gpu_providers import DIAG_SRC  # (the diagonal Gaussian as an elementwise bk_term)

pytestmark = pytest.mark.gpu

C = 130


def _lam(D):
    return np.logspace(0, 1, D)


def _builtin(D):
    return bk.DiagGaussian(_lam(D))


def _from_source(D):
    return bk.CTarget.from_source(DIAG_SRC, D, params=torch.as_tensor(_lam(D)).cuda())


def _precond(s):
    s.set_precond_diag(ap.perturbed_variances(_lam(s._dim)))


# name -> (model, constructor keywords, the operation, whole-draw kernel in use before it, after it)
SEAMS = {
    "set_precond_diag, stays on the whole-draw kernel": (_builtin, {}, _precond, True, True),
    "set_precond_diag, leaves the whole-draw kernel": (_from_source, {}, _precond, True, False),
    "warmup(adapt_trajectory=True) leaves and re-enters the whole-draw kernel":
        (_builtin, {}, lambda s: s.warmup(25, adapt_trajectory=True), True, True),
    "warmup(adapt_metric='dense')":
        (_builtin, dict(metric_dense="eye"), lambda s: s.warmup(25, adapt_metric="dense"), False, False),
    "load_state_dict(state_dict())": (_builtin, {}, lambda s: s.load_state_dict(s.state_dict()), True, True),
}


def _pair(model, D, **kw):
    """The same sampler generating ahead and not (eager launches for both: a replayed graph generates in line anyway)."""
    if kw.get("metric_dense") == "eye":
        kw["metric_dense"] = np.eye(D)
    pair = [bk.HMCDiag(model(D), 0.05, 7, chains=C, seed=19, prefetch_rng=pf, graph=False, **kw) for pf in (True, False)]
    assert pair[0]._prefetch and not pair[1]._prefetch
    return pair


def _assert_equal_draws(a, b, n, what):
    (ta, la), (tb, lb) = ap.run_draws(a, n), ap.run_draws(b, n)
    assert np.array_equal(ta, tb) and np.array_equal(la, lb), what
    assert np.array_equal(a.rng_state(), b.rng_state()), what


@pytest.mark.parametrize("D", [8, 40])
@pytest.mark.parametrize("seam", list(SEAMS))
def test_generating_ahead_changes_nothing_across(seam, D):
    model, kw, op, fused_before, fused_after = SEAMS[seam]
    a, b = _pair(model, D, **kw)
    assert a._fused_draw == b._fused_draw == fused_before
    assert (a._snap is not None) == (fused_before and D >= 32)
    _assert_equal_draws(a, b, 2, "before")
    assert a._ahead.ahead  # (something was generated ahead for the operation to drop)
    op(a), op(b)
    assert a._fused_draw == b._fused_draw == fused_after
    assert np.array_equal(a.rng_state(), b.rng_state())
    _assert_equal_draws(a, b, 2, "after")


@pytest.mark.parametrize("D", [8, 40])
def test_set_metric_dense_drops_the_momentum_ahead_without_a_rewind(D):
    """As documented ("build such samplers with prefetch_rng=False to keep the stream order"): the momentum generated ahead
    with the old metric is dropped and the stream stays where its generation ended, one draw's randomness ahead of the
    sampler that generates in line."""
    a, b = _pair(_builtin, D, metric_dense="eye")
    _assert_equal_draws(a, b, 2, "before")
    M = np.diag(ap.perturbed_variances(_lam(D))) + 0.01
    a.set_metric_dense(M), b.set_metric_dense(M)
    torch.cuda.synchronize()
    assert not a._ahead.ahead
    assert np.array_equal(a.rng_state(), a._rng_state.cpu().numpy().view(np.uint64))  # (the raw table: nothing rewound)
    assert not np.array_equal(a.rng_state(), b.rng_state())
    b.sample()
    assert np.array_equal(a.rng_state(), b.rng_state())
    ap.run_draws(a, 2), ap.run_draws(b, 2)
    assert np.array_equal(a.rng_state(), b.rng_state())


# ---- MALA ------------------------------------------------------------------------------------------------------------------
MALA_SEAMS = {
    "refresh_cache()": lambda s: s.refresh_cache(),
    "epsilon assigned": lambda s: setattr(s, "_epsilon", 0.8 * s._epsilon),
    "set_precond_diag": _precond,
    "load_state_dict(state_dict())": lambda s: s.load_state_dict(s.state_dict()),
    "warmup(25)": lambda s: s.warmup(25),
}


@pytest.mark.parametrize("D", [8, 40])
@pytest.mark.parametrize("seam", list(MALA_SEAMS))
def test_mala_generating_ahead_changes_nothing_across(seam, D):
    a, b = (mp.make(None, C, D, seed=19, prefetch_rng=pf, graph=False) for pf in (True, False))
    assert a._prefetch and not b._prefetch
    assert a._two_pass == b._two_pass == (D == 40)
    _assert_equal_draws(a, b, 2, "before")
    assert a._ahead.ahead  # (something was generated ahead for the operation to drop or keep)
    MALA_SEAMS[seam](a), MALA_SEAMS[seam](b)
    assert np.array_equal(a.rng_state(), b.rng_state())
    _assert_equal_draws(a, b, 2, "after")
