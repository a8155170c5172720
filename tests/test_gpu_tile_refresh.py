"""The tile-rate momentum refresh on the GPU: the row-spread shape (bkt::k_refresh_apply_kin_t) against the kernels every
other call takes, both reached through bk_momentum_refresh with the routing forced by the shape of the output (an even pitch
and 16-byte alignment: the new shape; an odd pitch: today's kernels), on the same normals; and the tile-major sampler, which
refreshes each tile's momentum into the tile's workspace, against the untiled one: by default (the sampler owns a side stream
for the draws that leave the tile-major loop, the tiles generate in line), with prefetch_rng=False, and with an explicit
prefetch_rng=True, which keeps the full-width look-ahead."""
import numpy as np
import pytest
import torch

import bayes_kit_amd as bk
from bayes_kit_amd import _lib
from bayes_kit_amd._engine import make_streams

pytestmark = pytest.mark.gpu

SEED = 2024
SCALE = 0.75
LOC_MUL = 0.5


@pytest.fixture(scope="module")
def ops():
    return _lib.default_ops()


def _fixed_order(terms):
    """Four contiguous quarters of the rows, each summed in increasing d, added ((0+1)+2)+3 (terms: [D, C] NumPy)."""
    D = terms.shape[0]
    Dq = (D + 3) // 4
    parts = []
    for w in range(4):
        s = np.zeros(terms.shape[1])
        for d in range(w * Dq, min((w + 1) * Dq, D)):
            s = s + terms[d]
        parts.append(s)
    return ((parts[0] + parts[1]) + parts[2]) + parts[3]


def _normals(C, D):
    """z[d][c]: chain c's first D normals, from the stream the library continues (Philox keyed (seed, chain))."""
    return np.stack([np.random.Generator(np.random.Philox(key=[SEED, c])).standard_normal(D) for c in range(C)], axis=1)


def _padded(ops, D, C, extra):
    """A NaN-filled [D + 2, C + extra] array and its [D, C] window one row and two columns in: with extra = 6 the pitch is
    even and the window 16-byte aligned, with extra = 7 the pitch is odd."""
    full = torch.full((D + 2, C + extra), float("nan"), dtype=torch.float64, device=ops.device)
    return full, full[1:1 + D, 2:2 + C]


def _untouched(full, D, C):
    pad = torch.ones_like(full, dtype=torch.bool)
    pad[1:1 + D, 2:2 + C] = False
    return bool(torch.isnan(full[pad]).all())


def _refresh(ops, C, D, extra, metric, loc, precond):
    kind, state = make_streams(SEED, C, 0, False, ops.device)
    assert kind == _lib.RNG_PHILOX
    full, out = _padded(ops, D, C, extra)
    kin = torch.full((C + 2,), float("nan"), dtype=torch.float64, device=ops.device)
    work = ops.refresh_work(C, D)   # zt[C][dp], dp = D rounded up to 8: padded rows for every D of this file
    loc_v = None
    if loc is not None:
        loc_full, loc_v = _padded(ops, D, C, extra)
        loc_v.copy_(loc)
    if precond is not None:
        ops.momentum_refresh_precond(kind, state, out, precond, kin[:C], work)
    else:
        ops.momentum_refresh(kind, state, loc_v, LOC_MUL, SCALE, out, metric, kin[:C], None, work)
    assert _untouched(full, D, C) and bool(torch.isnan(kin[C:]).all())
    return out.clone(), kin[:C].clone(), state


# C: below, at and just past one group of 16 chains, and not a multiple of it; D: fewer rows than quarters, a ragged last
# quarter, not a multiple of the 16-dimension piece (3 and 5 take the generator of short rows: the launches agree there too)
@pytest.mark.parametrize("C", [2, 16, 18, 130])
@pytest.mark.parametrize("D", [3, 5, 33, 130])
@pytest.mark.parametrize("metric", [False, True])
def test_tile_shape_equals_todays_kernel(ops, C, D, metric):
    assert (D + 7) // 8 * 8 != D  # the scratch rows are padded
    m = torch.linspace(0.5, 1.5, D, dtype=torch.float64, device=ops.device) if metric else None
    new, kin_new, st_new = _refresh(ops, C, D, 6, m, None, None)
    old, kin_old, st_old = _refresh(ops, C, D, 7, m, None, None)
    assert torch.equal(new, old) and torch.equal(kin_new, kin_old) and torch.equal(st_new, st_old)
    # ... and what both are specified to be: 0.0 + scale * z, the kinetic energy in the fixed order
    v = 0.0 + SCALE * _normals(C, D)
    mv = m.cpu().numpy()[:, None] * v if metric else v
    assert np.array_equal(new.cpu().numpy(), v)
    assert np.array_equal(kin_new.cpu().numpy(), 0.5 * _fixed_order(v * mv))


@pytest.mark.parametrize("C,D", [(18, 33), (130, 130)])
def test_tile_shape_with_a_location_and_with_a_preconditioner(ops, C, D):
    g = torch.Generator(device=ops.device)
    g.manual_seed(3)
    loc = torch.randn((D, C), dtype=torch.float64, device=ops.device, generator=g)
    new, kin_new, _ = _refresh(ops, C, D, 6, None, loc, None)
    old, kin_old, _ = _refresh(ops, C, D, 7, None, loc, None)
    assert torch.equal(new, old) and torch.equal(kin_new, kin_old)
    z = _normals(C, D)
    assert np.array_equal(new.cpu().numpy(), loc.cpu().numpy() * LOC_MUL + SCALE * z)
    v = torch.linspace(0.25, 4.0, D, dtype=torch.float64, device=ops.device)
    pd = torch.stack([v, torch.sqrt(v), 1.0 / v]).contiguous()
    new, kin_new, _ = _refresh(ops, C, D, 6, None, None, pd)
    old, kin_old, _ = _refresh(ops, C, D, 7, None, None, pd)
    assert torch.equal(new, old) and torch.equal(kin_new, kin_old)
    pn = pd.cpu().numpy()
    rho = 0.0 + pn[1][:, None] * z
    assert np.array_equal(new.cpu().numpy(), rho)
    assert np.array_equal(kin_new.cpu().numpy(), 0.5 * _fixed_order(rho * (pn[2][:, None] * rho)))


# -- the sampler: each tile's momentum refreshed into the tile's workspace ---------------------------------------------
D_S, L_S = 33, 3
LAM_S = np.logspace(0, 2, D_S)


def _sampler(C, tile, **kw):
    # (graph=False: eager launches, also where prefetch_rng is off -- a replayed graph at these sizes would allocate up front)
    s = bk.HMCDiag(bk.DiagGaussian(LAM_S), 0.05, L_S, chains=C, seed=11, path="opaque", chain_tile=tile, graph=False, **kw)
    # start at the target's own widths, so that a draw accepts some proposals and rejects others
    s._theta_dc.mul_(torch.as_tensor(1.0 / np.sqrt(LAM_S), device=s._theta_dc.device)[:, None])
    return s


def _draws(s, n):
    out = []
    for _ in range(n):
        th, lp = s.sample()
        out.append((th.clone(), lp.clone(), s._mask.clone(), torch.as_tensor(s.rng_state().view(np.int64).copy())))
    return out


def _same(ra, rb):
    for n, (x, y) in enumerate(zip(ra, rb)):
        for what, u, v in zip(("theta", "logp", "mask", "rng state"), x, y):
            assert torch.equal(u, v), (what, n)


@pytest.fixture(scope="module")
def untiled():
    """The untiled sampler's five draws, per chain count (read-only)."""
    return {C: _draws(_sampler(C, 0), 5) for C in (96, 80)}


@pytest.mark.parametrize("C", [96, 80])  # T = 32: three full tiles; two and a ragged third of 16 chains
@pytest.mark.parametrize("prefetch_rng", [None, False, True], ids=["default", "off", "explicit"])
def test_per_tile_refresh_draws_equal_untiled(untiled, C, prefetch_rng):
    b = _sampler(C, 32, prefetch_rng=prefetch_rng)
    assert b._prefetch == (prefetch_rng is not False) and b._chain_tile == 32 and b._tile_ahead == (prefetch_rng is True)
    rb = _draws(b, 2)
    sd = b.state_dict()   # mid-run: nothing is ahead between two draws, the table is the logical position
    rb += _draws(b, 3)
    _same(untiled[C], rb)
    assert b._tm_last and 0.0 < b.accept_rate() < 1.0
    if prefetch_rng is True:  # the full-width look-ahead, as asked for
        assert all(r is not None for r in b._rho_bufs) and b._rng_work is not None
    else:  # no full-width momentum and no full-size scratch: the tile's workspace instead
        assert all(r is None for r in b._rho_bufs) and b._rng_work is None
        assert b._rho_tile.numel() == D_S * 32 and b._tile_work.numel() == 32 * 40
    c = _sampler(C, 32, prefetch_rng=prefetch_rng)
    c.load_state_dict(sd)
    _same(untiled[C][2:], _draws(c, 3))


def test_a_draw_that_leaves_the_tile_major_loop_gets_its_full_width_momentum():
    """L = 0 takes the plain path: the full-width buffers appear then, and the tiles take over again afterwards."""
    a, b = _sampler(96, 0), _sampler(96, 32)  # (by default both own the side stream; b's tiles generate in line)
    assert a._prefetch and b._prefetch and not b._tile_ahead
    ra, rb = _draws(a, 1), _draws(b, 1)
    a._steps = b._steps = 0
    ra += _draws(a, 2)
    rb += _draws(b, 2)
    assert b._rho_bufs[0] is not None and not b._tm_last
    a._steps = b._steps = L_S
    ra += _draws(a, 2)   # (the first of them drops what the L = 0 draw generated ahead and takes its stream back)
    rb += _draws(b, 2)
    assert b._tm_last
    _same(ra, rb)
