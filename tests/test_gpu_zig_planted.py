"""The word-parallel normal generator (k_zig_parallel / k_zig_parallel_side of csrc/bk_rng.hip) at PLANTED stream events:
tests/golden/zig_planted.json puts a wedge, a tail, a rejected wedge, neighbouring exceptions, a counter carry, ... at a
stated position of the generator's first window (tests/zig_planted.py; tests/test_zig_planted_cpu.py proves the claims
without a GPU).  Everything here is bit for bit: planted chains against numpy.random.Generator started from the same
state, all chains against the one-lane kernel, the stream table and the snapshot.  The planted chains sit in the first,
inner and last segments of wavefronts between int-seeded neighbours, so the segments of one wavefront advance by
different amounts and finish in different passes."""
import math

import numpy as np
import pytest
import torch

from tests import zig_planted as zp

pytestmark = pytest.mark.gpu

PHILOX, PCG64 = 0, 1


@pytest.fixture(scope="module")
def ops():
    from bayes_kit_amd import _lib

    return _lib.default_ops()


def _f64(ops, *shape, fill=None):
    if fill is None:
        return torch.empty(shape, dtype=torch.float64, device=ops.device)
    return torch.full(shape, fill, dtype=torch.float64, device=ops.device)


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _groups(lpc, multi=None, min_D=1):
    """[(C, D, entries)] of the fixture for one window size; multi: only / never the launches of more than one pass."""
    out = []
    for (l, C, D), es in zp.groups_by_shape().items():
        if l != lpc or D < min_D:
            continue
        is_multi = (C, D) == zp.MULTI[lpc]
        if multi is None or multi == is_multi:
            out.append((C, D, es))
    assert out
    return out


def _tables(ops, C, D, es, lpc):
    assert ops.normals_lanes_per_chain(C, D) == lpc, (C, D)
    words, where = zp.build_table(es, C)
    assert len(where) == len(es)
    return zp.to_device(words, ops.device), zp.to_device(words, ops.device), where


def _one_lane(ops, st, C, D):
    z = _f64(ops, D, C)
    ops.momentum_refresh(PHILOX, st, None, 0.0, 1.0, z, None, None)
    return z


@pytest.mark.parametrize("lpc", [16, 32, 64])
@pytest.mark.parametrize("multi", [False, True], ids=["one_pass", "multi_pass"])
def test_chain_major_normals_at_planted_events(ops, lpc, multi):
    """bk_normals_chain_major, plain and as a background launch of fewer workgroups than chain groups, against the
    one-lane kernel (all chains) and numpy (planted chains): normals, stream table, snapshot.  D in 1..31 is reached
    through this entry point only."""
    for C, D, es in _groups(lpc, multi):
        st_a, st_b, where = _tables(ops, C, D, es, lpc)
        st_c = st_a.clone()
        before = st_a.clone()
        dp = (D + 7) // 8 * 8
        zt, zc = _f64(ops, C, dp, fill=np.nan), _f64(ops, C, dp, fill=np.nan)
        snap, snap_c = torch.zeros_like(st_a), torch.zeros_like(st_a)
        ops.normals_chain_major(PHILOX, st_a, zt, D, snap)
        n_groups = -(-C // (4 * (64 // lpc)))
        ops.normals_chain_major(PHILOX, st_c, zc, D, snap_c, max_workgroups=max(1, n_groups // 3))
        z = _one_lane(ops, st_b, C, D)
        tag = (lpc, C, D, [e["name"] for e in es])
        assert torch.equal(zt[:, :D].t(), z) and torch.equal(st_a, st_b), tag
        assert torch.equal(zc[:, :D], zt[:, :D]) and torch.equal(st_c, st_a), tag
        assert torch.equal(snap, before) and torch.equal(snap_c, before), tag
        assert bool(torch.isnan(zt[:, D:]).all()), tag  # (nothing written past a chain's D normals)
        zp.assert_planted_equal_numpy(where, D, zt.cpu().numpy(), z.cpu().numpy(), _u64(st_a))


@pytest.mark.parametrize("lpc", [16, 32, 64])
def test_momentum_refresh_entry_points_at_planted_events(ops, lpc):
    """bk_momentum_refresh and bk_momentum_refresh_precond with scratch (the word-parallel path) against the same calls
    without (one lane per chain) and against numpy; bk_mala_propose (one lane) on the same tables."""
    for C, D, es in _groups(lpc, min_D=32):
        st_a, st_b, where = _tables(ops, C, D, es, lpc)
        work = ops.refresh_work(C, D)
        a, b, ka, kb = _f64(ops, D, C), _f64(ops, D, C), _f64(ops, C), _f64(ops, C)
        ops.momentum_refresh(PHILOX, st_a, None, 0.0, 1.0, a, None, ka, None, work)
        ops.momentum_refresh(PHILOX, st_b, None, 0.0, 1.0, b, None, kb, None, None)
        tag = (lpc, C, D, [e["name"] for e in es])
        assert torch.equal(a, b) and torch.equal(ka, kb) and torch.equal(st_a, st_b), tag
        zp.assert_planted_equal_numpy(where, D, None, a.cpu().numpy(), _u64(st_a))
        zp.assert_planted_equal_numpy(where, D, None, b.cpu().numpy(), _u64(st_b))
        # preconditioned: out = 0.0 + sqrt(v)[d] * z
        st_a, st_b, where = _tables(ops, C, D, es, lpc)
        v = np.linspace(0.5, 1.5, D)
        pc = torch.as_tensor(np.stack([v, np.sqrt(v), 1.0 / v])).to(ops.device)
        ops.momentum_refresh_precond(PHILOX, st_a, a, pc, ka, work)
        ops.momentum_refresh_precond(PHILOX, st_b, b, pc, kb, None)
        assert torch.equal(a, b) and torch.equal(ka, kb) and torch.equal(st_a, st_b), tag
        got, table = a.cpu().numpy(), _u64(st_a)
        for col, e in where.items():
            z, w = zp.expected(e, D)
            assert np.array_equal(got[:, col], 0.0 + np.sqrt(v) * z) and np.array_equal(table[:, col], w), (e["name"], lpc)
        # the MALA proposal of the one-lane kernel: (theta + eps grad) + s z
        st_a, _, where = _tables(ops, C, D, es, lpc)
        rng = np.random.default_rng(D)
        th, gr = rng.normal(size=(D, C)), rng.normal(size=(D, C))
        prop = _f64(ops, D, C)
        ops.mala_propose(PHILOX, st_a, torch.as_tensor(th).to(ops.device), torch.as_tensor(gr).to(ops.device), prop, 0.03,
                         math.sqrt(0.06))
        got, table = prop.cpu().numpy(), _u64(st_a)
        for col, e in where.items():
            z, w = zp.expected(e, D)
            assert np.array_equal(got[:, col], (th[:, col] + 0.03 * gr[:, col]) + math.sqrt(0.06) * z), (e["name"], lpc)
            assert np.array_equal(table[:, col], w), (e["name"], lpc)


def _dr_outs(ops, C):
    return dict(kin=_f64(ops, C), H=_f64(ops, C), h=_f64(ops, C), rej=_f64(ops, C),
                alive=torch.empty(C, dtype=torch.uint8, device=ops.device),
                counters=torch.full((5,), 9, dtype=torch.int32, device=ops.device),
                draws=torch.full((1,), 3, dtype=torch.int64, device=ops.device))


def _dr_refresh_begin(ops, st, rho, work, logp, o, side=None):
    ops.dr_refresh_begin(PHILOX, st, None, 0.0, 1.0, rho, None, o["kin"], work, logp, o["H"], o["h"], o["rej"], o["alive"], 1.0,
                         o["counters"], o["draws"], side=side)


def _assert_dr_equal(x, y, tag):
    for k in x:
        assert torch.equal(x[k], y[k]), (k, tag)


def _expected_after_uniform(e, D):
    """numpy's normals, the retry uniform that follows them, and the table column after both."""
    g = zp.numpy_generator(e)
    z = g.normal(size=D)
    u = g.uniform()
    st = g.bit_generator.state
    w = zp.state_words(e)
    w[2:6], w[6:10], w[10] = st["state"]["counter"], st["buffer"], st["buffer_pos"]
    return z, u, w


@pytest.mark.parametrize("lpc", [16, 32, 64])
def test_dr_refresh_begin_at_planted_events(ops, lpc):
    """bk_dr_refresh_begin (generator launch + transpose / energy / start of the draw, whose retry uniform is the word
    right after the chain's last normal) against bk_momentum_refresh with one lane per chain + bk_dr_begin_retry, and
    against numpy."""
    for C, D, es in _groups(lpc, min_D=32):
        st_a, st_b, where = _tables(ops, C, D, es, lpc)
        work = ops.refresh_work(C, D)
        logp = torch.as_tensor(np.random.default_rng(C + D).normal(size=C)).to(ops.device)
        ra, rb, oa, ob = _f64(ops, D, C), _f64(ops, D, C), _dr_outs(ops, C), _dr_outs(ops, C)
        _dr_refresh_begin(ops, st_a, ra, work, logp, oa)
        ops.momentum_refresh(PHILOX, st_b, None, 0.0, 1.0, rb, None, ob["kin"], None, None)
        ops.dr_begin_retry(PHILOX, st_b, logp, ob["kin"], ob["H"], ob["h"], ob["rej"], ob["alive"], 1.0, ob["counters"], ob["draws"])
        tag = (lpc, C, D, [e["name"] for e in es])
        assert torch.equal(ra, rb) and torch.equal(st_a, st_b), tag
        _assert_dr_equal(oa, ob, tag)
        got, table, alive = ra.cpu().numpy(), _u64(st_a), oa["alive"].cpu().numpy()
        for col, e in where.items():
            z, u, w = _expected_after_uniform(e, D)
            assert np.array_equal(got[:, col].view(np.uint64), (0.0 + 1.0 * z).view(np.uint64)), (e["name"], lpc)
            assert np.array_equal(table[:, col], w), (e["name"], lpc)
            assert alive[col] == (1 if np.log(u) < 0.0 else 0), (e["name"], lpc)


# generator shape (lanes per chain, one pass or more), side job: Welford theta [Dw, Cw] and / or K tracked dimensions + logp
# of a theta with Cr chains.  n_wg = generator workgroups, units = side units (256 lanes x 2 chains x 4 dims of the Welford
# update; 256 chains of one tracked series), period = max(2, (n_wg + units) // units).
SIDE_CASES = [
    # lpc, multi, welford (Cw, Dw), record (Cr, K, with logp),  n_wg, units, period, grid
    (16, False, (64, 40), None, 5, 10, 2, 20),          # side units outnumber the generator's workgroups: period 2, grid extended
    (64, False, None, (70, 1, True), 18, 2, 10, 20),    # a larger period that divides the grid
    (32, False, (64, 8), None, 9, 2, 5, 11),            # ... that does not divide the grid
    (32, False, (600, 9), (600, 2, True), 9, 15, 2, 30),  # both parts in one job
    (16, True, (64, 40), (64, 3, False), 2048, 13, 158, 2061),  # a grid of many generator workgroups
]


@pytest.mark.parametrize("lpc,multi,welford,record,n_wg,units,period,grid", SIDE_CASES)
def test_side_job_launch_at_planted_events(ops, lpc, multi, welford, record, n_wg, units, period, grid):
    """k_zig_parallel_side: the generator's workgroups interleaved with side-job workgroups.  The normals, energies, draw
    start and stream table equal the launch without a side job; the side job's result equals bk_welford_update_dev /
    bk_record_series_dev called alone."""
    C, D, es = sorted(_groups(lpc, multi, min_D=32), key=lambda g: -len(g[2]))[0]
    # the launch geometry this case is about, restated from zig_parallel_side_launch
    chains_per_wg = 4 * (64 // lpc)
    u = 0
    if welford:
        u += -(-(welford[0] // 2) // 256) * -(-welford[1] // 4)
    if record:
        u += -(-record[0] // 256) * (record[1] + (1 if record[2] else 0))
    total = -(-C // chains_per_wg) + u
    assert (-(-C // chains_per_wg), u, max(2, total // u)) == (n_wg, units, period)
    assert max(total, (u - 1) * period + period) == grid
    st_a, st_b, where = _tables(ops, C, D, es, lpc)
    work = ops.refresh_work(C, D)
    g = np.random.default_rng(grid)
    logp = torch.as_tensor(g.normal(size=C)).to(ops.device)
    n_dev = torch.full((1,), 7, dtype=torch.int64, device=ops.device)
    kw_job = {}
    Cs, Ds = (welford[0], welford[1]) if welford else (record[0], 6)  # (one job describes one theta)
    assert not (welford and record) or record[0] == welford[0]
    # (what lets the generator's launch carry the Welford part itself instead of a launch of its own: an even chain count,
    # contiguous 16-byte aligned arrays, a footprint inside the last-level cache)
    assert not welford or (Cs % 2 == 0 and 3 * Cs * Ds * 8 < (192 << 20))
    theta = torch.as_tensor(g.normal(size=(Ds, Cs))).to(ops.device)
    if welford:
        mean, m2 = torch.as_tensor(g.normal(size=(Ds, Cs))).to(ops.device), torch.as_tensor(g.random(size=(Ds, Cs))).to(ops.device)
        mean_ref, m2_ref = mean.clone(), m2.clone()
        kw_job["welford"] = (mean, m2, 4)  # n = 7 - 4
    if record:
        Cr, K, with_logp = record
        dims = torch.as_tensor(np.arange(K, dtype=np.int32)[::-1].copy()).to(ops.device)
        slogp = torch.as_tensor(g.normal(size=Cr)).to(ops.device) if with_logp else None
        series = _f64(ops, K + (1 if with_logp else 0), 4, Cr, fill=np.nan)
        series_ref = series.clone()
        kw_job["record"] = (dims, slogp, series, 5)  # row = 7 - 5
    ra, rb, oa, ob = _f64(ops, D, C), _f64(ops, D, C), _dr_outs(ops, C), _dr_outs(ops, C)
    job = ops.diag_job(theta, n_dev, **kw_job)
    _dr_refresh_begin(ops, st_a, ra, work, logp, oa, side=job)
    _dr_refresh_begin(ops, st_b, rb, work, logp, ob)
    tag = (lpc, C, D)
    assert torch.equal(ra, rb) and torch.equal(st_a, st_b), tag
    _assert_dr_equal(oa, ob, tag)
    got, table = ra.cpu().numpy(), _u64(st_a)
    for col, e in where.items():
        z, _, w = _expected_after_uniform(e, D)
        assert np.array_equal(got[:, col].view(np.uint64), (0.0 + 1.0 * z).view(np.uint64)), (e["name"], lpc)
        assert np.array_equal(table[:, col], w), (e["name"], lpc)
    if welford:
        ops.welford_update_dev(mean_ref, m2_ref, theta, n_dev, 4)
        assert torch.equal(mean, mean_ref) and torch.equal(m2, m2_ref), tag
    if record:
        ops.record_series_dev(theta, dims, slogp, series_ref, n_dev, 5)
        assert torch.equal(series[:, 2], series_ref[:, 2]) and bool(torch.isnan(series[:, [0, 1, 3]]).all()), tag
        assert not bool(torch.isnan(series[:, 2]).any()), tag


def test_one_lane_kernels_on_planted_pcg64_streams(ops):
    """The PCG64 cases (a tail; a rejected wedge followed by an accepted one) through the one-lane kernels."""
    from bayes_kit_amd._engine import make_streams

    es = zp.entries("pcg64")
    assert len(es) == 2
    D = es[0]["D"]
    assert all(e["D"] == D for e in es)
    C = len(es)
    kind, st = make_streams([zp.numpy_generator(e) for e in es], C, 0, False, ops.device)
    assert kind == PCG64
    _, st2 = make_streams([zp.numpy_generator(e) for e in es], C, 0, False, ops.device)
    out = _f64(ops, D, C)
    ops.momentum_refresh(kind, st, None, 0.0, 1.0, out, None, None)
    rng = np.random.default_rng(1)
    th, gr = rng.normal(size=(D, C)), rng.normal(size=(D, C))
    prop = _f64(ops, D, C)
    ops.mala_propose(kind, st2, torch.as_tensor(th).to(ops.device), torch.as_tensor(gr).to(ops.device), prop, 0.03, math.sqrt(0.06))
    assert torch.equal(st, st2)
    got, gp, table = out.cpu().numpy(), prop.cpu().numpy(), _u64(st)
    for c, e in enumerate(es):
        g = zp.numpy_generator(e)
        z = g.normal(size=D)
        assert np.array_equal(got[:, c].view(np.uint64), (0.0 + 1.0 * z).view(np.uint64)), e["name"]
        assert np.array_equal(gp[:, c], (th[:, c] + 0.03 * gr[:, c]) + math.sqrt(0.06) * z), e["name"]
        s = g.bit_generator.state["state"]["state"]
        assert [int(table[0, c]), int(table[1, c])] == [s >> 64, s & ((1 << 64) - 1)], e["name"]
