"""The tile-major HMC schedule on the GPU: kick+drift, blend and select with one row pitch per array, the per-chain
reductions at tile size against the scalar kernels and a NumPy restatement of their fixed order, and the tiled sampler
against the untiled one.  Every product and sum of an expected value is a torch (or NumPy) op of its own, hence rounded
separately, as the library's are (-ffp-contract=off)."""
import numpy as np
import pytest
import torch

import bayes_kit_amd as bk

pytestmark = pytest.mark.gpu

EPS = 0.0123
SENTINEL = 777.0


@pytest.fixture(scope="module")
def ops():
    return bk._lib.default_ops()


def _randn(ops, shape, seed):
    g = torch.Generator(device=ops.device)
    g.manual_seed(seed)
    return torch.randn(shape, dtype=torch.float64, device=ops.device, generator=g)


# -- 1. kick+drift, different input and output pitches -----------------------------------------------------------------
def _kd_expect(th, rho, gr, m, use_pre, pre, kick):
    t = m[:, None] * gr if m is not None else gr
    r = rho
    if use_pre:
        r = r + pre * t
    r = r + kick * t
    return th + EPS * r, r


@pytest.mark.parametrize("off,C", [(2, 130), (3, 130), (2, 131)])  # 16-byte form; odd offset and odd C: the 8-byte form
@pytest.mark.parametrize("metric", [False, True])
@pytest.mark.parametrize("use_pre", [False, True])
@pytest.mark.parametrize("rho_in_place", [False, True])
def test_kick_drift_with_one_pitch_per_array(ops, off, C, metric, use_pre, rho_in_place):
    D, W = 33, 262
    th, rho, gr = (_randn(ops, (D, W), s) for s in (1, 2, 3))
    m = torch.linspace(0.5, 1.5, D, dtype=torch.float64, device=ops.device) if metric else None
    keep = [x.clone() for x in (th, rho, gr)]
    tv, rv, gv = (x[:, off:off + C] for x in (th, rho, gr))
    want_th, want_rho = _kd_expect(tv, rv, gv, m, use_pre, -0.5 * EPS, EPS)
    th_out = torch.full((D, C), SENTINEL, dtype=torch.float64, device=ops.device)
    rho_out = rv if rho_in_place else torch.full((D, C), SENTINEL, dtype=torch.float64, device=ops.device)
    ops.kick_drift_ld(tv, th_out, rv, rho_out, gv, m, EPS, use_pre, -0.5 * EPS, True, EPS)
    assert torch.equal(th_out, want_th) and torch.equal(rho_out, want_rho)
    # the inputs and every column outside the slice are as they were
    assert torch.equal(th, keep[0]) and torch.equal(gr, keep[2])
    if rho_in_place:
        assert torch.equal(rho[:, :off], keep[1][:, :off]) and torch.equal(rho[:, off + C:], keep[1][:, off + C:])
    else:
        assert torch.equal(rho, keep[1])


# -- 2. blend and select, a different pitch per array ------------------------------------------------------------------
def _masks(C, device):
    pairs = torch.tensor([0, 0, 0, 1, 1, 0, 1, 1], dtype=torch.uint8, device=device)  # (m0, m1) = 00, 01, 10, 11
    mixed = pairs.repeat((C + 7) // 8)[:C].contiguous()
    return {"mixed": mixed, "all": torch.ones_like(mixed), "none": torch.zeros_like(mixed)}


@pytest.mark.parametrize("off,C", [(2, 130), (3, 130), (2, 131)])  # the vector path; the unaligned and the odd fallback
@pytest.mark.parametrize("which", ["mixed", "all", "none"])
def test_blend_and_select_with_one_pitch_per_array(ops, off, C, which):
    D = 5  # an odd row count for the two-row kernels
    mask = _masks(C, ops.device)[which]
    if which == "mixed":
        got = {(int(mask[2 * i]), int(mask[2 * i + 1])) for i in range(C // 2)}
        assert got == {(0, 0), (0, 1), (1, 0), (1, 1)}
    a = _randn(ops, (D, 262), 4)       # the state: pitch 262
    b = _randn(ops, (D, C), 5)         # the tile's proposal: contiguous
    out = torch.full((D, 300), SENTINEL, dtype=torch.float64, device=ops.device)  # the new state: another pitch
    a0, b0 = a.clone(), b.clone()
    av, ov = a[:, off:off + C], out[:, off + 2:off + 2 + C]
    want = torch.where(mask.bool()[None, :], b, av)
    ops.blend_columns_ld(mask, av, b, ov)
    assert torch.equal(ov, want)
    assert torch.equal(a, a0) and torch.equal(b, b0)
    assert bool((out[:, :off + 2] == SENTINEL).all()) and bool((out[:, off + 2 + C:] == SENTINEL).all())

    dst = _randn(ops, (D, 262), 6)     # the cached gradient: pitch 262
    src = _randn(ops, (D, C), 7)       # the tile's gradient: contiguous
    dst0, src0 = dst.clone(), src.clone()
    dv = dst[:, off:off + C]
    want = torch.where(mask.bool()[None, :], src, dv)
    ops.select_columns_ld(mask, dv, src)
    assert torch.equal(dv, want) and torch.equal(src, src0)
    assert torch.equal(dst[:, :off], dst0[:, :off]) and torch.equal(dst[:, off + C:], dst0[:, off + C:])


# -- 3. the reduction kernels at tile size -----------------------------------------------------------------------------
T_TILE = 8192
HALF = 0.5 * EPS


def _fixed_order(terms):
    """Four contiguous quarters of the rows, each summed in increasing d, added 0+1+2+3 (terms: [D, C] NumPy)."""
    D = terms.shape[0]
    Dq = (D + 3) // 4
    parts = []
    for w in range(4):
        s = np.zeros(terms.shape[1])
        for d in range(w * Dq, min((w + 1) * Dq, D)):
            s = s + terms[d]
        parts.append(s)
    return ((parts[0] + parts[1]) + parts[2]) + parts[3]


@pytest.fixture(scope="module")
def tile_inputs(ops):
    # columns 1 .. 8192 of arrays two columns wider: an UNALIGNED view, which takes the scalar kernels
    wide = [_randn(ops, (1024, T_TILE + 2), s) for s in (8, 9, 10)]
    lam = torch.logspace(0, 2, 1024, dtype=torch.float64, device=ops.device)
    m = torch.linspace(0.5, 1.5, 1024, dtype=torch.float64, device=ops.device)
    return wide, lam, m


@pytest.mark.parametrize("D", [1024, 1023])  # 1023: quarters of 256, 256, 256 and 255 rows
def test_log_density_and_gradient_at_tile_size(ops, tile_inputs, D):
    (th_w, _, _), lam, _ = tile_inputs
    lam = lam[:D].contiguous()
    view = th_w[:D, 1:1 + T_TILE]
    assert view.data_ptr() % 16 != 0
    th = view.contiguous()             # what a tile is: even, aligned, resident -> the tile-size kernel
    assert 2 * 8 * D * T_TILE <= bk.HMCDiag.LLC_BYTES and D * T_TILE >= 1 << 22
    model = bk.DiagGaussian(lam)
    g_s, lp_s = torch.full_like(th_w[:D], SENTINEL)[:, 1:1 + T_TILE], torch.empty(T_TILE, dtype=torch.float64, device=ops.device)
    model.bk_eval(view, g_s, lp_s)
    g_t, lp_t = torch.full_like(th, SENTINEL), torch.empty_like(lp_s)
    model.bk_eval(th, g_t, lp_t)
    lt = lam[:, None] * th
    want_lp = -0.5 * _fixed_order((th * lt).cpu().numpy())
    assert torch.equal(g_t, -lt) and torch.equal(g_t, g_s)
    assert torch.equal(lp_t, lp_s)
    assert np.array_equal(lp_t.cpu().numpy(), want_lp)


@pytest.mark.parametrize("D,metric", [(1024, True), (1023, False)])
def test_finish_at_tile_size(ops, tile_inputs, D, metric):
    (_, rho_w, gr_w), _, m = tile_inputs
    m = m[:D].contiguous() if metric else None
    rv, gv = rho_w[:D, 1:1 + T_TILE], gr_w[:D, 1:1 + T_TILE]
    rho, gr = rv.contiguous(), gv.contiguous()
    kin_s, kin_t = (torch.empty(T_TILE, dtype=torch.float64, device=ops.device) for _ in range(2))
    out_s = torch.full_like(rho_w[:D], SENTINEL)[:, 1:1 + T_TILE]
    out_t = torch.full_like(rho, SENTINEL)
    ops.leapfrog_finish(rv, out_s if metric else None, gv, m, HALF, False, kin_s)      # unaligned: the scalar kernel
    ops.leapfrog_finish(rho, out_t if metric else None, gr, m, HALF, False, kin_t)     # the tile-size kernel
    t = m[:, None] * gr if metric else gr
    v = rho + HALF * t
    mv = m[:, None] * v if metric else v
    want = 0.5 * _fixed_order((v * mv).cpu().numpy())
    assert torch.equal(kin_t, kin_s)
    assert np.array_equal(kin_t.cpu().numpy(), want)
    if metric:
        assert torch.equal(out_t, v) and torch.equal(out_t, out_s)


# -- 4. the sampler: tiled (tile-major) against untiled ----------------------------------------------------------------
D_S, L_S = 33, 3
LAM_S = np.logspace(0, 2, D_S)


def _sampler(C, tile, **kw):
    s = bk.HMCDiag(bk.DiagGaussian(LAM_S), 0.05, L_S, chains=C, seed=11, path="opaque", chain_tile=tile, **kw)
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


@pytest.mark.parametrize("C,tile", [(1026, 512), (130, 64)])  # ragged: tiles of 512, 512 and 2 chains; of 64, 64 and 2
@pytest.mark.parametrize("prefetch_rng", [True, False])
def test_tile_major_draws_equal_untiled(C, tile, prefetch_rng):
    a, b = _sampler(C, 0, prefetch_rng=prefetch_rng), _sampler(C, tile, prefetch_rng=prefetch_rng)
    ra, rb = _draws(a, 5), _draws(b, 5)
    assert a._chain_tile == C and not a._tm_last
    assert b._chain_tile == tile and b._tm_last  # the tiled sampler really ran tile-major
    _same(ra, rb)
    # the proposal and its gradient, assembled from the tile-major store, are the untiled sampler's arrays
    assert b._theta_p.shape == (D_S, C) and torch.equal(a._theta_p, b._theta_p) and torch.equal(a._grad_p, b._grad_p)
    assert a.accept_rate() == b.accept_rate()
    assert 0.0 < b.accept_rate() < 1.0


@pytest.mark.parametrize("C,tile", [(1026, 512), (130, 64)])
def test_tile_major_warmup_equals_untiled(C, tile):
    a, b = _sampler(C, 0), _sampler(C, tile)
    rep_a, rep_b = a.warmup(24), b.warmup(24)  # one metric window (ends after draw 22), then draws with the preconditioner
    assert b._tm_last and rep_a["window_ends"] == rep_b["window_ends"] and len(rep_a["window_ends"]) == 1
    assert rep_a["eps"] == rep_b["eps"] and rep_a["alpha"] == rep_b["alpha"]
    assert rep_a["stepsize"] == rep_b["stepsize"]
    assert np.array_equal(rep_a["precond_diag"], rep_b["precond_diag"])
    _same(_draws(a, 2), _draws(b, 2))
    assert a.accept_rate() == b.accept_rate()


def test_tile_major_state_dict_round_trip():
    C, tile = 130, 64
    a, b = _sampler(C, 0), _sampler(C, tile)
    _same(_draws(a, 2), _draws(b, 2))
    sd = b.state_dict()
    c = _sampler(C, tile)
    c.load_state_dict(sd)
    ra = _draws(a, 3)
    _same(ra, _draws(b, 3))
    _same(ra, _draws(c, 3))
    assert c._tm_last and 0.0 < c.accept_rate() < 1.0
