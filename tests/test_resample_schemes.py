"""Systematic and stratified resampling (include/bkhip.h: bk_resample_ordered) on the CPU: the NumPy restatement of
tests/fake_ops_resample.py against the definition evaluated in Python integers, the properties that hold without any
tolerance, the offspring statistics, and TemperedLikelihoodSMC(resampling=...) on the stand-in ops (one and two ranks)."""
import bisect
import math
import os
import socket
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

import bayes_kit_amd as bk
from tests import fake_ops_resample as fr
from tests.fake_ops import FakeOps

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
MODES = {"systematic": fr.SYSTEMATIC, "stratified": fr.STRATIFIED}
U_TOP = 1.0 - 2.0 ** -53


# ---- the definition, in Python integers ---------------------------------------------------------------------------------
def exact_q(w):
    """q_i = round-half-even(fl(w_i / wmax) * 2^s) with the product and the rounding done on rationals."""
    w = [float(x) for x in w]
    wmax, s = max(w), 62 - (len(w) - 1).bit_length()
    return [round(Fraction(x / wmax) * 2 ** s) if x > 0.0 else 0 for x in w]


def exact_Q(w):
    Q, tot = [], 0
    for q in exact_q(w):
        tot += q
        Q.append(tot)
    return Q


def exact_points(Q, u, mode, m, slot0, m_local):
    """-> (tau_J, idx_J) of the slots slot0 .. slot0 + m_local - 1, Python ints."""
    total = Q[-1]
    a = total // m
    taus, idx = [], []
    for j in range(m_local):
        J = slot0 + j
        uj = float(u[0]) if mode == fr.SYSTEMATIC else float(u[j])
        o = min(a - 1, int(math.floor(uj * float(a))))
        assert 0 <= o <= a - 1
        tau = (J * total) // m + o
        taus.append(tau)
        idx.append(bisect.bisect_right(Q, tau))
    return taus, idx


def run_fake(w, u, mode, m_local, slot0, m_total):
    ops = fr.ResampleFakeOps()
    n = len(w)
    work = torch.zeros(ops.resample_ordered_work_bytes(n), dtype=torch.uint8)
    idx = torch.full((m_local,), -1, dtype=torch.int32)
    ops.resample_ordered(torch.as_tensor(np.asarray(w, dtype=np.float64)), torch.as_tensor(np.asarray(u, dtype=np.float64)),
                         mode, slot0, m_total, work, idx)
    Q = work.numpy()[fr.Q_OFFSET:fr.Q_OFFSET + 8 * n].copy().view(np.int64)
    return idx.numpy(), Q


def check_exact_properties(w, u, mode, m, tag):
    """Everything section "the arithmetic" promises, for the whole slot range; -> (idx, Q, q) as Python lists."""
    n = len(w)
    q, Q = exact_q(w), exact_Q(w)
    s = 62 - (n - 1).bit_length()
    assert n * 2 ** s <= 2 ** 62 and 2 ** 31 <= 2 ** s <= Q[-1] <= 2 ** 62 and Q[-1] > m, tag
    idx_f, Q_f = run_fake(w, u, mode, m, 0, m)
    assert [int(x) for x in Q_f] == Q, tag                                  # the restatement == the definition
    taus, idx = exact_points(Q, u, mode, m, 0, m)
    assert [int(x) for x in idx_f] == idx, tag
    assert all(0 <= i <= n - 1 for i in idx), tag
    assert all(b >= a for a, b in zip(idx, idx[1:])), tag                   # non-decreasing in J
    assert all(q[i] > 0 for i in idx), tag                                  # q_i = 0 is never chosen
    for J, tau in enumerate(taus):                                          # one point in every stratum
        assert (J * Q[-1]) // m <= tau < ((J + 1) * Q[-1]) // m, (tag, J)
    counts = [0] * n
    for i in idx:
        counts[i] += 1
    lo = [0] + Q[:-1]
    edges = [(J * Q[-1]) // m for J in range(m + 1)]
    for i in range(n):
        if mode == fr.SYSTEMATIC:                                           # floor(m q / Q) <= N_i <= ceil(m q / Q)
            assert (m * q[i]) // Q[-1] <= counts[i] <= -((-m * q[i]) // Q[-1]), (tag, i)
        # strata wholly inside [Q_{i-1}, Q_i) <= N_i <= strata meeting it (both schemes)
        j0, j1 = bisect.bisect_left(edges, lo[i]), bisect.bisect_right(edges, Q[i]) - 1   # first edge >= lo, last edge <= hi
        inside = max(0, j1 - j0)
        meeting = 0 if q[i] == 0 else (bisect.bisect_left(edges, Q[i]) - 1) - (bisect.bisect_right(edges, lo[i]) - 1) + 1
        assert inside <= counts[i] <= meeting, (tag, i, inside, counts[i], meeting)
    return idx, Q, q


def weight_sets(n, g):
    sets = {"random": g.random(n) + 1e-3, "span": np.logspace(-300, 0, n)[g.permutation(n)] if n > 1 else np.ones(1),
            "equal": np.full(n, 0.37), "only_first": np.r_[2.5, np.zeros(n - 1)], "only_last": np.r_[np.zeros(n - 1), 1e-7]}
    z = g.random(n) + 0.1
    z[n // 4:n // 2] = 0.0
    z[n - max(1, n // 5):] = 0.0
    if not z.any():
        z[0] = 1.0
    sets["zero_runs"] = z
    return sets


def uniform_sets(m, g):
    return {"random": g.random(m), "zero": np.zeros(m), "top": np.full(m, U_TOP), "mixed": np.where(g.random(m) < 0.5, 0.0, U_TOP)}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_exact_properties(mode):
    g = np.random.default_rng(11)
    for n in (1, 2, 7, 64, 301):
        for wname, w in weight_sets(n, g).items():
            for m in sorted({1, n, n // 2 + 1, 2 * n + 1}):
                for uname, u in uniform_sets(m, g).items():
                    tag = (mode, n, wname, m, uname)
                    idx, Q, q = check_exact_properties(w, u, MODES[mode], m, tag)
                    if wname == "only_first":
                        assert idx == [0] * m, tag
                    if wname == "only_last":
                        assert idx == [n - 1] * m, tag
                    if wname == "equal" and m == n and mode == "systematic":
                        assert idx == list(range(n)), tag                    # the identity


def test_the_clamp_keeps_the_top_of_a_stratum_inside_it():
    """o_J <= a - 1 whatever the product's rounding.  For u < 1 the rounded u * float(a) stays below a (it is at most the
    double before float(a), and a is at least half an ulp above that), so the clamp is a guard: u = 1 - 2^-53 gives a point
    in the stratum's top ulp, and u = 1.0 itself -- outside the contract -- is held at a - 1 by the clamp alone."""
    g = np.random.default_rng(13)
    for n, m in ((64, 64), (7, 3), (301, 77)):
        w = g.random(n) + 0.01 if n != 64 else np.full(64, 1.0)
        Q = exact_Q(w)
        a = Q[-1] // m
        assert a > 2 ** 53 and int(math.floor(U_TOP * float(a))) <= a - 1
        for u in (U_TOP, 1.0):
            taus, idx = exact_points(Q, [u], fr.SYSTEMATIC, m, 0, m)
            got, _ = run_fake(w, [u], fr.SYSTEMATIC, m, 0, m)
            assert [int(x) for x in got] == idx
            for J, tau in enumerate(taus):
                assert (J * Q[-1]) // m <= tau < ((J + 1) * Q[-1]) // m
                assert u < 1.0 or tau == (J * Q[-1]) // m + min(a - 1, int(float(a)))
        if n == 64:
            assert idx == list(range(64))


@pytest.mark.parametrize("mode", sorted(MODES))
def test_a_shard_draws_its_slice_of_the_whole(mode):
    g = np.random.default_rng(12)
    for n, m in ((50, 50), (50, 23), (9, 40)):
        w = weight_sets(n, g)["zero_runs"]
        u = g.random(m)
        whole, _ = run_fake(w, u, MODES[mode], m, 0, m)
        for slot0, m_local in ((0, m), (1, m - 1), (m // 3, m // 2), (m - 1, 1), (m, 0)):
            us = u[:1] if mode == "systematic" else u[slot0:slot0 + m_local]
            part, _ = run_fake(w, us if len(us) else np.zeros(1), MODES[mode], m_local, slot0, m)
            assert np.array_equal(part, whole[slot0:slot0 + m_local]), (mode, n, m, slot0)


def test_restatement_parts_are_the_stand_in_op():
    """tests/test_gpu_resample.py calls the restatement's parts (one Q per weight set); the stand-in op is those parts."""
    g = np.random.default_rng(5)
    w, u = g.random(300), g.random(77)
    for mode in MODES.values():
        idx, Q = fr.resample_ordered_ref(w, u[3:3 + 40], mode, 40, 30, 77)
        tau = fr.thresholds(fr.cumulative(w)[-1], u[3:3 + 40], mode, 40, 30, 77)
        assert np.array_equal(Q, fr.cumulative(w)) and np.array_equal(idx, np.searchsorted(Q, tau, side="right"))


def test_argument_errors_of_the_stand_in():
    ops = fr.ResampleFakeOps()
    w, u, idx = torch.ones(8, dtype=torch.float64), torch.zeros(8, dtype=torch.float64), torch.zeros(8, dtype=torch.int32)
    work = torch.zeros(ops.resample_ordered_work_bytes(8), dtype=torch.uint8)
    for bad in (dict(mode=2), dict(slot0=-1), dict(slot0=1), dict(m_total=0), dict(work=work[:-1])):
        kw = dict(mode=0, slot0=0, m_total=8, work=work)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.resample_ordered(w, u, kw["mode"], kw["slot0"], kw["m_total"], kw["work"], idx)
    assert fr.work_bytes(0) == 0 and fr.work_bytes(2 ** 31) == -1 and fr.work_bytes(2 ** 31 - 1) > 8 * (2 ** 31 - 1)


def test_c_abi_status_codes_are_decided_before_any_hip_call():
    """BK_E_ARG / BK_OK of bk_resample_ordered on a machine without a GPU (dummy pointers are never read), and the scratch size
    against the restatement's."""
    import ctypes

    from bayes_kit_amd import _lib

    lib = _lib.load()
    assert _lib.BK_RESAMPLE_SYSTEMATIC == fr.SYSTEMATIC and _lib.BK_RESAMPLE_STRATIFIED == fr.STRATIFIED
    for n in (-1, 0, 1, 2, 7, fr.TILE - 1, fr.TILE, fr.TILE + 1, fr.CARRY_W * fr.TILE + 1, 2 ** 20 + 1, 2 ** 31 - 1, 2 ** 31):
        assert lib.bk_resample_ordered_work_bytes(n) == fr.work_bytes(n), n
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    p += (-p) % 16
    n, nb = 4, lib.bk_resample_ordered_work_bytes(4)

    def call(w=p, n_=n, u=p, m_local=0, slot0=0, m_total=n, mode=fr.SYSTEMATIC, work=p, wb=nb, out=p):
        return lib.bk_resample_ordered(w, n_, u, m_local, slot0, m_total, mode, work, wb, out, None)

    assert call() == 0 and call(slot0=n) == 0 and call(mode=fr.STRATIFIED) == 0    # m_local == 0: BK_OK, nothing launched
    for kw in (dict(w=None), dict(u=None), dict(work=None), dict(out=None), dict(n_=0), dict(n_=-3), dict(m_total=0),
               dict(m_local=-1), dict(slot0=-1), dict(slot0=n + 1), dict(m_local=1, slot0=n), dict(m_local=n + 1),
               dict(n_=2 ** 31, wb=2 ** 40), dict(m_total=2 ** 31), dict(mode=2), dict(mode=-1), dict(wb=nb - 1), dict(work=p + 8)):
        assert call(**kw) == -1, kw


# ---- offspring statistics ---------------------------------------------------------------------------------------------------
N_STAT, R_STAT = 64, 4000


@pytest.fixture(scope="module")
def offspring():
    """Offspring counts [R, n] of the three schemes for one weight vector, n = m = 64, R = 4,000 draws of a fixed seed."""
    g = np.random.default_rng(2024)
    w = g.random(N_STAT) ** 3 + 1e-3
    Q = fr.cumulative(w)
    U = g.random((R_STAT, N_STAT))
    out = {"w": w, "q": np.diff(np.r_[0, Q]), "Q": int(Q[-1])}
    for name, mode in MODES.items():
        c = np.zeros((R_STAT, N_STAT), dtype=np.int64)
        for r in range(R_STAT):
            tau = fr.thresholds(Q[-1], U[r], mode, N_STAT, 0, N_STAT)
            c[r] = np.bincount(np.searchsorted(Q, tau, side="right"), minlength=N_STAT)
        out[name] = c
    fake = FakeOps()
    c = np.zeros((R_STAT, N_STAT), dtype=np.int64)
    wt, cdf, idx = torch.from_numpy(w), torch.empty(N_STAT, dtype=torch.float64), torch.empty(N_STAT, dtype=torch.int32)
    for r in range(R_STAT):
        fake.resample_indices(wt, torch.from_numpy(U[r]), cdf, idx)
        c[r] = np.bincount(idx.numpy(), minlength=N_STAT)
    out["multinomial"] = c
    return out


def test_systematic_is_unbiased(offspring):
    """N_i takes two adjacent values, so its variance is at most 1/4: the mean of R draws is within 6 * 0.5 / sqrt(R) of
    m q_i / Q for every i (six standard errors)."""
    expect = N_STAT * offspring["q"].astype(np.float64) / float(offspring["Q"])
    err = np.abs(offspring["systematic"].mean(axis=0) - expect)
    print("max |mean N_i - m q_i / Q| =", err.max(), "bound", 6 * 0.5 / math.sqrt(R_STAT))
    assert np.all(err <= 6 * 0.5 / math.sqrt(R_STAT))


def test_ordered_schemes_have_less_offspring_variance_than_multinomial(offspring):
    v = {k: float(offspring[k].var(axis=0, ddof=1).sum()) for k in ("systematic", "stratified", "multinomial")}
    print("summed offspring variance:", v)
    assert v["systematic"] < v["multinomial"] and v["stratified"] < v["multinomial"]


# ---- the sampler ----------------------------------------------------------------------------------------------------------------
def _gauss_smc(ops, M=37, N=5, seed=5, **kw):
    D = 2
    g = np.random.default_rng(3)
    y, init = torch.as_tensor(g.normal(size=D)), g.normal(size=(M, D))
    model = bk.TorchPriorLikelihoodModel(lambda T: -0.5 * (T * T).sum(dim=1), lambda T: -3.0 * ((T - y) ** 2).sum(dim=1), D)
    return bk.TemperedLikelihoodSMC(model, M, N, init, bk.metropolis_kernel(0.5), seed=seed, ops=ops, **kw)


def test_resampling_keyword_is_validated():
    ops = fr.ResampleFakeOps()
    assert _gauss_smc(ops).resampling == "multinomial"
    for scheme in MODES:
        assert _gauss_smc(ops, resampling=scheme).resampling == scheme
    with pytest.raises(ValueError):
        _gauss_smc(ops, resampling="residual")
    for scheme in MODES:
        for stream in (np.random, np.random.RandomState(3)):
            with pytest.raises(ValueError):
                _gauss_smc(ops, seed=stream, resampling=scheme)
    _gauss_smc(ops, seed=np.random.RandomState(3), resampling="multinomial")


def test_sampler_runs_each_scheme_on_the_same_streams():
    runs = {}
    for scheme in ("multinomial", "systematic", "stratified"):
        ops = fr.ResampleFakeOps()
        smc = _gauss_smc(ops, resampling=scheme)
        work = smc._rs_work
        for n in range(1, smc.N + 1):
            moved = {}
            gather = ops.gather_columns

            def spy(index, src, dst, _m=moved, _g=gather):
                _m["theta"] = src.numpy().copy()
                _g(index, src, dst)

            ops.gather_columns = spy
            try:
                smc.transition(n)
            finally:
                del ops.gather_columns
            idx = smc._idx.numpy()
            assert np.array_equal(smc._theta_dc.numpy(), moved["theta"][:, idx])
            if scheme != "multinomial":
                assert np.all(np.diff(idx) >= 0), (scheme, n)
        assert smc.t == 1.0 and smc._rs_work is work                      # (the scratch is allocated once)
        assert ops.calls.get("resample_ordered", 0) == (0 if scheme == "multinomial" else smc.N)
        runs[scheme] = (smc._rng_state.numpy().copy(), smc.thetas.numpy().copy())
    for scheme in MODES:
        assert np.array_equal(runs[scheme][0], runs["multinomial"][0]), scheme   # the RNG end state does not depend on the scheme
    plain = _gauss_smc(FakeOps())                                             # built without the keyword, on the plain stand-in
    plain.run()
    assert np.array_equal(plain.thetas.numpy(), runs["multinomial"][1])
    assert not np.array_equal(runs["systematic"][1], runs["multinomial"][1])


def test_systematic_uses_global_slot_zeros_uniform():
    ops = fr.ResampleFakeOps()
    smc = _gauss_smc(ops, resampling="systematic", N=1)
    seen = {}
    inner = ops.resample_ordered

    def spy(weights, u, mode, slot0, m_total, work, idx_out):
        seen.update(w=weights.numpy().copy(), u=u.numpy().copy(), args=(mode, slot0, m_total))
        inner(weights, u, mode, slot0, m_total, work, idx_out)

    ops.resample_ordered = spy
    smc.transition(1)
    assert seen["args"] == (fr.SYSTEMATIC, 0, smc.M) and len(seen["u"]) == smc.M
    want, _ = fr.resample_ordered_ref(seen["w"], seen["u"][:1], fr.SYSTEMATIC, smc.M, 0, smc.M)
    assert np.array_equal(smc._idx.numpy(), want)


def test_two_rank_gloo_resampling_equals_the_solo_run():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "resample_dist_worker.py")], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=240)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(out)
    for rank, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, out
        assert f"rank {rank} ok" in out
