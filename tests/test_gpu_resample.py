"""bk_resample_ordered on the MI355X: ancestor indices and the fixed-point cumulative weight against the NumPy restatement
(tests/fake_ops_resample.py), equal bit for bit at the seams of the five launches -- T = 2,048 elements per tile, W = 256 tile
sums per pass of the carry loop -- and TemperedLikelihoodSMC(resampling=...) end to end against the restatement fed the
device's own weights."""
import ctypes

import numpy as np
import pytest
import torch

import bayes_kit_amd as bk
from tests import fake_ops_resample as fr

pytestmark = pytest.mark.gpu

T, W = fr.TILE, fr.CARRY_W
SIZES = (1, 2, 7, T - 1, T, T + 1, 2 * T + 3, W * T - 1, W * T, W * T + 1, 2 ** 20 + 1)
MODES = {"systematic": fr.SYSTEMATIC, "stratified": fr.STRATIFIED}


@pytest.fixture(scope="module")
def ops():
    from bayes_kit_amd import _lib

    return _lib.default_ops()


def weight_sets(n, g):
    """The adversarial sets, their features laid across tile boundaries (and across the carry loop's pass boundary W * T)."""
    last_tile = ((n - 1) // T) * T                      # first element of the last tile
    sets = {"random": g.random(n) + 1e-3, "equal": np.full(n, 0.37), "only_first": np.r_[2.5, np.zeros(n - 1)],
            "only_last": np.r_[np.zeros(n - 1), 1e-7]}
    z = g.random(n) + 0.1
    for b in (T, 2 * T, W * T, 2 * W * T):              # runs of zeros across the boundaries
        if b + 7 <= n:
            z[b - 5:b + 7] = 0.0
    z[n // 4:n // 4 + max(0, min(n // 8, 3000))] = 0.0   # (longer than a tile where n allows)
    if last_tile > 0:
        z[last_tile + 1:] = 0.0                         # the last non-zero weight opens the last tile ...
    elif n > 2:
        z[n - max(1, n // 5):] = 0.0
    sets["zero_runs"] = z
    sp = np.logspace(-300, 0, n)[g.permutation(n)] if n > 1 else np.ones(1)
    if last_tile > 1:
        sp[last_tile:] = 0.0                            # ... or closes the tile before it
        sp[last_tile - 1] = 1e-3
        if sp.max() < 1.0:
            sp[0] = 1.0
    sets["span"] = sp
    assert all(np.isfinite(v).all() and (v >= 0).all() and v.max() > 0 for v in sets.values())
    return sets


@pytest.mark.parametrize("n", SIZES)
def test_kernel_equals_the_restatement_at_the_seams(ops, n):
    g = np.random.default_rng(1000 + n % 997)
    dev = ops.device
    nb = ops.resample_ordered_work_bytes(n)
    assert nb == fr.work_bytes(n)
    u_all = g.random(2 * n + 1)
    u_all[:2] = (0.0, fr_top())
    u_dev = torch.as_tensor(u_all).to(dev)
    for wname, w in weight_sets(n, g).items():
        w_dev = torch.as_tensor(w).to(dev)
        Q_ref = fr.cumulative(w)
        Q_dev = torch.as_tensor(Q_ref.view(np.uint8)).to(dev)
        work = torch.zeros(nb, dtype=torch.uint8, device=dev)
        checked_on_host = False
        for m in sorted({1, n, n // 2 + 1, 2 * n + 1}):
            for slot0 in sorted({0, m // 2}):
                m_local = m - slot0 if slot0 == 0 else min(m - slot0, m // 3 + 1)   # a middle shard ends before the last slot
                for mname, mode in MODES.items():
                    for u0 in ((0, 1, 2) if mode == fr.SYSTEMATIC and m == n else (2,)):
                        # stratified: the shard's own uniforms; systematic: one (u = 0 and u = 1 - 2^-53 as well at m = n)
                        u = u_dev[u0:u0 + 1] if mode == fr.SYSTEMATIC else u_dev[slot0:slot0 + m_local]
                        u_host = u_all[u0:u0 + 1] if mode == fr.SYSTEMATIC else u_all[slot0:slot0 + m_local]
                        idx = torch.full((m_local,), -7, dtype=torch.int32, device=dev)
                        work.zero_()
                        ops.resample_ordered(w_dev, u, mode, slot0, m, work, idx)
                        tag = (n, wname, m, slot0, mname, u0)
                        # Q: read back and compared once per weight set, after that compared where it lies (read back to report)
                        same = torch.equal(work[fr.Q_OFFSET:fr.Q_OFFSET + 8 * n], Q_dev)
                        if not (same and checked_on_host):
                            Q = work.cpu().numpy()[fr.Q_OFFSET:fr.Q_OFFSET + 8 * n].copy().view(np.int64)
                            checked_on_host = True
                            bad = np.flatnonzero(Q != Q_ref)
                            assert same and np.array_equal(Q, Q_ref), (tag, "Q differs at", bad[:4], Q[bad[:4]], Q_ref[bad[:4]], len(bad))
                        tau = fr.thresholds(Q_ref[-1], u_host, mode, m_local, slot0, m)
                        want = np.minimum(np.searchsorted(Q_ref, tau, side="right"), n - 1).astype(np.int32)
                        got = idx.cpu().numpy()
                        assert np.array_equal(got, want), tag
                        if wname == "only_first":
                            assert not got.any(), tag
                        if wname == "only_last":
                            assert (got == n - 1).all(), tag
                        if wname == "equal" and m == n and mode == fr.SYSTEMATIC and slot0 == 0:
                            assert np.array_equal(got, np.arange(n)), tag


def fr_top():
    return 1.0 - 2.0 ** -53


def test_an_unaligned_weight_view_takes_the_8_byte_loads(ops):
    g = np.random.default_rng(6)
    n = 2 * T + 3
    buf = torch.as_tensor(g.random(n + 1)).to(ops.device)
    w = buf[1:]
    assert w.data_ptr() % 16 == 8
    u = torch.as_tensor(g.random(n)).to(ops.device)
    work = torch.zeros(ops.resample_ordered_work_bytes(n), dtype=torch.uint8, device=ops.device)
    idx = torch.empty(n, dtype=torch.int32, device=ops.device)
    ops.resample_ordered(w, u, fr.STRATIFIED, 0, n, work, idx)
    want, Q = fr.resample_ordered_ref(w.cpu().numpy(), u.cpu().numpy(), fr.STRATIFIED, n, 0, n)
    assert np.array_equal(idx.cpu().numpy(), want)
    assert np.array_equal(work.cpu().numpy()[fr.Q_OFFSET:fr.Q_OFFSET + 8 * n].copy().view(np.int64), Q)


def test_argument_errors_and_the_empty_call_launch_nothing(ops):
    lib = ops.lib
    n = 100
    nb = lib.bk_resample_ordered_work_bytes(n)
    assert lib.bk_resample_ordered_work_bytes(0) == 0 and lib.bk_resample_ordered_work_bytes(2 ** 31) == -1
    w = torch.ones(n, dtype=torch.float64, device=ops.device)
    u = torch.zeros(n, dtype=torch.float64, device=ops.device)
    work = torch.full((nb + 16,), 0x5A, dtype=torch.uint8, device=ops.device)
    idx = torch.full((n,), -7, dtype=torch.int32, device=ops.device)
    P = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731

    def call(weights=w, n_=n, u_=u, m_local=n, slot0=0, m_total=n, mode=fr.STRATIFIED, work_=work, wb=nb, out=idx):
        return lib.bk_resample_ordered(None if weights is None else P(weights), n_, None if u_ is None else P(u_), m_local, slot0,
                                       m_total, mode, None if work_ is None else P(work_), wb, None if out is None else P(out), None)

    E_ARG = -1
    for kw in (dict(weights=None), dict(u_=None), dict(work_=None), dict(out=None), dict(n_=0), dict(m_total=0), dict(slot0=-1),
               dict(slot0=1), dict(m_local=n + 1), dict(n_=2 ** 31), dict(m_total=2 ** 31), dict(mode=2), dict(mode=-1),
               dict(wb=nb - 1), dict(work_=work[8:])):
        assert call(**kw) == E_ARG, kw
    assert call(m_local=0) == 0 and call(m_local=0, slot0=n) == 0
    torch.cuda.synchronize()
    assert (idx.cpu().numpy() == -7).all() and (work.cpu().numpy() == 0x5A).all()      # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(idx.cpu().numpy(), np.arange(n))


@pytest.mark.parametrize("scheme", sorted(MODES))
def test_smc_end_to_end_against_the_restatement(ops, scheme):
    M, D, N = 3 * T + 5, 3, 4
    g = np.random.default_rng(9)
    y = torch.as_tensor(g.normal(size=D), device=ops.device)
    init = g.normal(size=(M, D))
    model = bk.TorchPriorLikelihoodModel(lambda Th: -0.5 * (Th * Th).sum(dim=1), lambda Th: -3.0 * ((Th - y) ** 2).sum(dim=1), D)
    smc = bk.TemperedLikelihoodSMC(model, M, N, init, bk.metropolis_kernel(0.5), seed=17, ops=ops, resampling=scheme)
    assert smc.resampling == scheme
    for k in range(1, N + 1):
        seen = {}
        ordered, gather = ops.resample_ordered, ops.gather_columns

        def spy_ordered(weights, u, mode, slot0, m_total, work, idx_out, _s=seen, _f=ordered):
            _s.update(w=weights.cpu().numpy().copy(), u=u.cpu().numpy().copy(), args=(mode, slot0, m_total, idx_out.shape[0]))
            _f(weights, u, mode, slot0, m_total, work, idx_out)

        def spy_gather(index, src, dst, _s=seen, _f=gather):
            _s["moved"] = src.cpu().numpy().copy()
            _f(index, src, dst)

        ops.resample_ordered, ops.gather_columns = spy_ordered, spy_gather
        try:
            smc.transition(k)
        finally:
            del ops.resample_ordered, ops.gather_columns
        mode, slot0, m_total, m_local = seen["args"]
        assert (mode, slot0, m_total, m_local) == (MODES[scheme], 0, M, M)
        want, _ = fr.resample_ordered_ref(seen["w"], seen["u"], mode, m_local, slot0, m_total)
        idx = smc._idx.cpu().numpy()
        assert np.array_equal(idx, want), (scheme, k)
        assert np.all(np.diff(idx) >= 0) and len(np.unique(idx)) > M // 20, (scheme, k)
        assert np.array_equal(smc._theta_dc.cpu().numpy(), seen["moved"][:, idx]), (scheme, k)
    assert smc.t == 1.0
