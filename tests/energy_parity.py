"""bk_energy_update / bk_divergence_capture (csrc/bk_energy.hip), EnergyDiagnostics and HMCDiag.track_energy at their seams;
checks that take the kernel library as an argument.  tests/test_energy_cpu.py runs them on the NumPy stand-in of
tests/fake_ops_energy.py (and on its planted faults, one broken seam each, to show that the checks notice);
tests/test_gpu_energy.py on the HIP library.

The reference of the kernel checks is EXACT and has no tolerance: the contract is a fixed sequence of individually rounded
fp64 operations and integer counts (include/bkhip.h), which fake_ops_energy.energy_ref / capture_ref restate; everything the
two entry points write must be np.array_equal (NaN == NaN) to them, and what they may not write must come back unchanged."""
from collections import namedtuple

import numpy as np
import torch

from bayes_kit_amd import _lib
from tests.fake_ops_energy import STATE, capture_ref, energy_ref, new_state, new_store

THRESHOLD = 1000.0
UPDATE_CHAINS = (1, 63, 64, 65, 255, 256, 257, 1000, 4099)
GUARD = -77.0
INF, NAN = float("inf"), float("nan")


def _dev(ops, a):
    return torch.from_numpy(np.array(a)).to(ops.device)


def _eq(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    same = np.array_equal(got, want, equal_nan=True) if got.dtype.kind == "f" else np.array_equal(got, want)
    if not same:
        bad = np.flatnonzero(~((got == want) | ((got != got) & (want != want))).reshape(-1)) if got.shape == want.shape else []
        raise AssertionError(f"{what} differs from the NumPy restatement at {len(bad)} places, first {list(bad[:6])}: "
                             f"got {got.reshape(-1)[bad[:3]] if len(bad) else got.shape}, "
                             f"want {want.reshape(-1)[bad[:3]] if len(bad) else want.shape}")


# ---- bk_energy_update ----------------------------------------------------------------------------------------------------------
def _plant(v, i, kind):
    """One planted chain; a_cur / a_prop are zero there, so h0 = lp_cur and h1 = lp_prop exactly."""
    v["a_cur"][i] = v["a_prop"][i] = 0.0
    lc, lp, lu = v["lp_cur"], v["lp_prop"], v["log_u"]
    if kind == 0:    # d == -threshold exactly: not divergent
        lc[i], lp[i] = 0.0, -THRESHOLD
    elif kind == 1:  # one ulp below: divergent
        lc[i], lp[i] = 0.0, np.nextafter(-THRESHOLD, -INF)
    elif kind == 2:  # d = NaN from inf - inf; rejected, E = -inf
        lc[i], lp[i] = INF, INF
    elif kind == 3:  # d = +inf (h0 = -inf): accepted, not divergent, E = 3
        lc[i], lp[i] = -INF, -3.0
    elif kind == 4:  # d = -inf: divergent, rejected, E = 3
        lc[i], lp[i] = -3.0, -INF
    elif kind == 5:  # log_u = -inf accepts anything that is not NaN (here a large drop that is not divergent)
        lc[i], lp[i], lu[i] = -3.0, -900.0, -INF
    elif kind == 6:  # ... and not a NaN: rejected, E = -h0 finite
        lc[i], lp[i], lu[i] = -3.0, NAN, -INF
    elif kind == 7:  # E = +inf (h0 = h1 = -inf: d NaN, rejected)
        lc[i], lp[i] = -INF, -INF
    elif kind == 8:  # E = NaN
        lc[i], lp[i] = NAN, -2.0
    # kind 9: an ordinary chain


KINDS = 10


def update_inputs(C, step):
    """The five vectors of update `step` (0, 1, 2) for C chains: ordinary energies, 3 % of the chains with a drop of 2,000
    (divergent), and the planted chains -- position (5 + 11 k) % C holds kind (k + step) % KINDS, so that over the three
    updates every planted position sees finite and non-finite energies interleaved, and first energies at every update."""
    g = np.random.default_rng(1000 * C + step)
    v = {"lp_cur": g.normal(-20.0, 5.0, C), "a_cur": 0.5 * g.chisquare(4, C)}
    v["lp_prop"] = v["lp_cur"] + g.normal(0.0, 2.0, C)
    v["a_prop"] = v["a_cur"] + g.normal(0.0, 1.0, C)
    v["log_u"] = np.log(g.uniform(size=C))
    v["lp_prop"][g.uniform(size=C) < 0.03] -= 2000.0
    for k in range(KINDS):
        _plant(v, (5 + 11 * k) % C, (k + step) % KINDS)
    return v


class _State:
    """The per-chain state as views [off, off + C) of longer arrays of guard values, which must come back unchanged."""
    DTYPES = dict(mean_E=torch.float64, m2_E=torch.float64, last_E=torch.float64, ssd=torch.float64, trans=torch.int64,
                  cnt=torch.int64, ndiv=torch.int64, div_mask=torch.uint8, err=torch.float64)

    def __init__(self, ops, C, off):
        self.C, self.off = C, off
        self.big = {k: torch.full((C + off + 3,), 77 if dt == torch.uint8 else (GUARD if dt == torch.float64 else int(GUARD)),
                                  dtype=dt, device=ops.device)
                    for k, dt in self.DTYPES.items()}
        self.v = {k: b[off:off + C] for k, b in self.big.items()}
        for k, t in self.v.items():
            t.zero_()
        self.totals = torch.zeros(4, dtype=torch.int64, device=ops.device)

    def host(self):
        out = {}
        for k, b in self.big.items():
            h = b.cpu().numpy()
            guard = 77 if h.dtype == np.uint8 else GUARD
            assert (h[:self.off] == guard).all() and (h[self.off + self.C:] == guard).all(), f"{k}: written outside the slice"
            out[k] = h[self.off:self.off + self.C].copy()
        out["totals"] = self.totals.cpu().numpy()
        return out


def _slice_of(ops, a, off):
    big = torch.full((a.shape[0] + off + 3,), GUARD, dtype=torch.float64, device=ops.device)
    big[off:off + a.shape[0]] = _dev(ops, a)
    return big[off:off + a.shape[0]]


def check_update(ops, C, null=False, off=0):
    """Three successive updates of C chains from a zeroed state: after each, everything the call wrote equals energy_ref,
    and the guards around the slices are untouched.  null: a_cur / a_prop are NULL; off: every array is the slice
    [off, off + C) of a longer one (odd off: 8-byte alignment only)."""
    st, ref = _State(ops, C, off), new_state(C)
    for step in range(3):
        v = update_inputs(C, step)
        if null:
            v["a_cur"] = v["a_prop"] = None
        t = {k: None if a is None else _slice_of(ops, a, off) for k, a in v.items()}
        ops.energy_update(t["lp_cur"], t["a_cur"], t["lp_prop"], t["a_prop"], t["log_u"], THRESHOLD,
                          *(st.v[k] for k in STATE), st.v["div_mask"], st.v["err"], st.totals)
        energy_ref(ref, v["lp_cur"], v["a_cur"], v["lp_prop"], v["a_prop"], v["log_u"], THRESHOLD)
        got = st.host()
        for k in ref:
            _eq(got[k], ref[k], f"update {step}, C={C}: {k}")
        for k, a in v.items():  # (the inputs are read only)
            if a is not None:
                _eq(t[k].cpu().numpy(), a, f"input {k}")
    if C >= 63:  # the data holds what the contract's edges need
        assert ref["totals"][1] > ref["totals"][2] > 0 and ref["totals"][3] > 0
        assert (ref["cnt"] == 3).any() and (ref["cnt"] == 2).any() and (ref["cnt"] < 2).any()
    return ref


# ---- bk_divergence_capture -----------------------------------------------------------------------------------------------------
Capture = namedtuple("Capture", "C D cap calls")  # calls: ((flags, chain0), ...)

CAPTURE_CASES = [
    Capture(1000, 1, 1024, (("edges", 0),)),
    Capture(1000, 3, 1024, (("edges", 7), ("random", 5000))),        # two calls with different chain0
    Capture(1000, 130, 1024, (("edges", 0), ("random", 1000))),
    Capture(1000, 3, 1024, (("all", 0), ("all", 1000))),             # cap filled in the middle of the second call
    Capture(1000, 3, 6, (("edges", 0), ("random", 0))),              # cap filled exactly at the first call's end
    Capture(1000, 3, 0, (("random", 0),)),                           # cap = 0: counted only
    Capture(1000, 3, 1024, (("none", 0), ("edges", 0))),
    Capture(4099, 3, 1024, (("random", 3), ("edges", 9))),           # ~1,230 flags: the store fills mid-call
    Capture(1, 3, 4, (("all", 0), ("none", 0), ("all", 5))),
    Capture(257, 130, 300, (("all", 0), ("edges", 0))),
    Capture(65, 1, 1024, (("edges", 0), ("all", 100))),
]


def capture_id(c):
    return f"C{c.C}-D{c.D}-cap{c.cap}-" + "+".join(f"{k}@{c0}" for k, c0 in c.calls)


def flags(kind, C, seed=0):
    m = np.zeros(C, dtype=np.uint8)
    if kind == "edges":
        m[[c for c in (0, 63, 64, 255, 256, C - 1) if c < C]] = 1
    elif kind == "all":
        m[:] = 1
    elif kind == "random":
        m[np.random.default_rng(C + seed).uniform(size=C) < 0.3] = 1
    else:
        assert kind == "none"
    return m


def check_capture(ops, c, pitch=3, off=1):
    """The calls of case c on an empty store: after each, the store and its fill level equal capture_ref's.  theta has a row
    pitch of C + pitch; the mask, err and trans are slices that start `off` elements into longer arrays."""
    C, D, cap = c.C, c.D, c.cap
    dev = ops.device
    ref = new_store(D, cap)
    i64, f64 = dict(dtype=torch.int64, device=dev), dict(dtype=torch.float64, device=dev)
    th_div = torch.full((D, cap), GUARD, **f64) if cap else None
    chain, draw, err_s = torch.full((cap,), -7, **i64), torch.full((cap,), -7, **i64), torch.full((cap,), GUARD, **f64)
    ref["theta_div"][:], ref["chain"][:], ref["draw"][:], ref["err_store"][:] = GUARD, -7, -7, GUARD
    fill = torch.zeros(2, **i64)
    work = torch.full((ops.divergence_capture_work_elems(C),), -1, **i64)
    for n, (kind, chain0) in enumerate(c.calls):
        g = np.random.default_rng(17 * C + n)
        mask, err = flags(kind, C, n), g.normal(size=C) * 1e3
        trans = g.integers(1, 1 << 40, size=C)
        theta = (np.arange(D)[:, None] * 1e6 + np.arange(C)[None, :] + 0.25 * (n + 1)).astype(np.float64)
        wide = torch.full((D, C + pitch), NAN, **f64)
        wide[:, :C] = _dev(ops, theta)
        m_big = torch.full((C + off + 3,), 1, dtype=torch.uint8, device=dev)  # (flags beyond the slice must not be seen)
        m_big[off:off + C] = _dev(ops, mask)
        e_t, t_t = _slice_of(ops, err, off), torch.zeros(C + off, **i64)
        t_t[off:] = _dev(ops, trans)
        ops.divergence_capture(m_big[off:off + C], e_t, t_t[off:], wide[:, :C], chain0, th_div, chain, draw, err_s, fill, work)
        if cap:
            capture_ref(ref, mask, err, trans, theta, chain0)
        else:
            ref["fill"][1] += int(mask.sum())
        what = f"{capture_id(c)}, call {n}: "
        _eq(fill.cpu().numpy(), ref["fill"], what + "fill")
        if cap:
            _eq(th_div.cpu().numpy(), ref["theta_div"], what + "theta_div")
            _eq(chain.cpu().numpy(), ref["chain"], what + "chain")
            _eq(draw.cpu().numpy(), ref["draw"], what + "draw")
            _eq(err_s.cpu().numpy(), ref["err_store"], what + "err")
    return ref


def check_abi_errors(lib):
    """BK_E_ARG before any HIP call (no device needed; dummy pointers are never read), BK_OK for an empty problem."""
    import ctypes

    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    OK, E_ARG = 0, -1
    f = lib.bk_energy_update
    good = [p, p, p, p, p, 1000.0, p, p, p, p, p, p, p, p, p, p, 4, None]
    assert f(*(good[:16] + [0, None])) == OK
    for i in (0, 2, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15):  # every pointer but a_cur / a_prop
        bad = list(good)
        bad[i] = None
        assert f(*bad) == E_ARG, i
    for thr in (0.0, -1.0, INF, NAN):
        bad = list(good)
        bad[5] = thr
        assert f(*bad) == E_ARG, thr
    bad = list(good)
    bad[16] = -1
    assert f(*bad) == E_ARG
    w = lib.bk_divergence_capture_work_elems
    assert [w(C) for C in (-1, 0, 1, 256, 257, 65536)] == [0, 2, 3, 3, 4, 258]
    f = lib.bk_divergence_capture
    good = [p, p, p, p, 8, 4, 3, 0, p, p, p, p, 16, p, p, None]
    assert f(*(good[:5] + [0] + good[6:])) == OK                      # C == 0
    for i in (0, 13, 14):
        bad = list(good)
        bad[i] = None
        assert f(*bad) == E_ARG, i
    for i in (1, 2, 3, 9, 10, 11):                                    # with a store every array is needed
        bad = list(good)
        bad[i] = None
        assert f(*bad) == E_ARG, i
    for i, v in ((4, 3), (5, -1), (6, -1), (12, -1), (6, 1 << 21)):  # ld < C, C < 0, D < 0, cap < 0, too many row blocks
        bad = list(good)
        bad[i] = v
        assert f(*bad) == E_ARG, (i, v)


# ---- the sampler ---------------------------------------------------------------------------------------------------------------
class RecordingOps:
    """The sampler's ops with ops.mh_accept wrapped: before every accept test it keeps host copies of the five vectors the
    test reads, of the chains they belong to and of those chains' columns of the state (still the start state)."""

    def __init__(self, ops):
        self._inner, self.sampler, self.records = ops, None, []

    def __getattr__(self, name):
        return getattr(self._inner, name)

    def mh_accept(self, mode, lp_cur, a_cur, lp_prop, a_prop, log_u, mask, ret, count):
        s = self.sampler
        if s is not None:
            c0 = lp_cur.storage_offset() - s._lp.storage_offset()
            n = lp_cur.shape[0]
            h = lambda t: np.zeros(n) if t is None else t.detach().cpu().numpy().copy()  # noqa: E731  (NULL = zeros)
            self.records.append(dict(c0=c0, lp_cur=h(lp_cur), a_cur=h(a_cur), lp_prop=h(lp_prop), a_prop=h(a_prop),
                                     log_u=h(log_u), theta=h(s._theta_dc[:, c0:c0 + n])))
        self._inner.mh_accept(mode, lp_cur, a_cur, lp_prop, a_prop, log_u, mask, ret, count)


def funnel_sampler(bk, ops, model_ops=None, stepsize=0.5, chains=256, chain_id0=0, **kw):
    """The issue's run: HMCDiag(Funnel(11), 0.5, 8, chains=256, seed=5)."""
    model = bk.Funnel(11) if model_ops is None else bk.Funnel(11, ops=model_ops)
    return bk.HMCDiag(model, stepsize, 8, chains=chains, seed=5, chain_id0=chain_id0, ops=ops, **kw)


def gauss_sampler(bk, ops, model_ops=None, chains=256, **kw):
    """HMCDiag(DiagGaussian(logspace(0, 2, 16)), 0.3, 6): the whole-draw kernel, whose accept test a tracker takes out."""
    lam = torch.from_numpy(np.logspace(0, 2, 16))
    model = bk.DiagGaussian(lam) if model_ops is None else bk.DiagGaussian(lam, ops=model_ops)
    return bk.HMCDiag(model, 0.3, 6, chains=chains, seed=5, ops=ops, **kw)


def check_whole_draw(bk, ops, model_ops=None, draws=10, **kw):
    """The whole-draw path, tracked against untracked: equal draws; the tracker equals the restatement; the tracked sampler
    launches its accept test itself and goes back to the in-launch test once untracked."""
    a, rec, thetas = run_tracked(bk, ops, draws=draws, model_ops=model_ops, sampler=gauss_sampler, **kw)
    assert a._fused_draw
    e = a.energy
    ref, store, _ = replay_records(rec.records, e.C, e.D, e.capture)
    assert_tracker_equals(e, ref, store)
    assert e.transitions == draws * e.C and len(rec.records) == draws
    a.untrack_energy()
    a.sample()
    assert len(rec.records) == draws, "untracked: the accept test is back inside the whole-draw launch"
    return a


def tracker_host(e):
    """Everything a tracker holds, as host arrays."""
    out = {k: getattr(e, k).cpu().numpy().copy() for k in STATE + ("div_mask", "err")}
    out["totals"], out["fill"] = e._totals.cpu().numpy().copy(), e._fill.cpu().numpy().copy()
    for k in ("theta_div", "chain", "draw", "err_store"):
        if getattr(e, k) is not None:
            out[k] = getattr(e, k).cpu().numpy().copy()
    return out


def replay_records(records, C, D, cap, chain_id0=0, threshold=THRESHOLD):
    """energy_ref / capture_ref fed with the recorded accept tests -> (state, store, the energies [calls, C] or None)."""
    ref, store = new_state(C), new_store(D, cap)
    energies = []
    for r in records:
        c0, n = r["c0"], r["lp_cur"].shape[0]
        part = {k: (v[c0:c0 + n] if k != "totals" else v) for k, v in ref.items()}  # (views: updated in place)
        energy_ref(part, r["lp_cur"], r["a_cur"], r["lp_prop"], r["a_prop"], r["log_u"], threshold)
        if cap:
            capture_ref(store, part["div_mask"], part["err"], part["trans"], r["theta"], chain_id0 + c0)
        else:
            store["fill"][1] += int(part["div_mask"].sum())
        if n == C:
            with np.errstate(invalid="ignore"):
                h0, h1 = r["lp_cur"] - r["a_cur"], r["lp_prop"] - r["a_prop"]
                energies.append(-np.where(r["log_u"] < h1 - h0, h1, h0))
    return ref, store, (np.array(energies) if len(energies) == len(records) else None)


def assert_tracker_equals(e, ref, store, what=""):
    got = tracker_host(e)
    for k in ref:
        _eq(got[k], ref[k], what + k)
    for k in store:
        _eq(got[k], store[k], what + k)


def assert_same_draw(a, b, out_a, out_b, what=""):
    """theta, logp and last_accept of a tracked sampler and its untracked twin after one draw."""
    assert torch.equal(out_a[0], out_b[0]), what + "theta"
    assert np.array_equal(out_a[1].cpu().numpy(), out_b[1].cpu().numpy(), equal_nan=True), what + "logp"
    assert torch.equal(a.last_accept, b.last_accept), what + "last_accept"


def assert_same_end(a, b):
    assert torch.equal(a.state_dict()["rng_state"], b.state_dict()["rng_state"]), "rng_state"
    assert a.accept_rate() == b.accept_rate()


def run_tracked(bk, ops, draws=40, capture=1024, model_ops=None, sampler=funnel_sampler, threshold=THRESHOLD, **kw):
    """A tracked sampler on RecordingOps beside an untracked twin, compared after every draw -> (tracked sampler, recorder,
    the draws' theta [draws, C, D] on the host).  Eager launches: the recorder reads device memory, which a capture cannot."""
    kw.setdefault("graph", False)
    rec = RecordingOps(ops)
    a, b = sampler(bk, rec, model_ops, **kw), sampler(bk, ops, model_ops, **kw)
    rec.sampler = a
    e = a.track_energy(threshold=threshold, capture=capture)
    assert a.energy is e and b.energy is None
    thetas = []
    for n in range(draws):
        before = len(rec.records)
        oa, ob = a.sample(), b.sample()
        assert len(rec.records) > before, "a tracked draw calls ops.mh_accept"
        assert_same_draw(a, b, oa, ob, f"draw {n}: ")
        thetas.append(oa[0].cpu().numpy().copy())
    assert_same_end(a, b)
    return a, rec, np.array(thetas)


def check_funnel_run(bk, ops, model_ops=None, **kw):
    """The issue's funnel run on the path `kw` selects: draws equal the twin's, the tracker's whole state equals the
    restatement fed with the recorded accept tests, divergences are met, and they start deep in the neck."""
    a, rec, thetas = run_tracked(bk, ops, model_ops=model_ops, **kw)
    e = a.energy
    C, D = thetas.shape[1], thetas.shape[2]
    ref, store, _ = replay_records(rec.records, C, D, e.capture, chain_id0=kw.get("chain_id0", 0))
    assert_tracker_equals(e, ref, store)
    assert e.transitions == 40 * C and e.divergences() == int(ref["totals"][1]) and e.divergences() > 0
    ds = e.divergent_states()
    assert ds["stored"] == min(e.capture, ds["seen"]) and ds["seen"] == e.divergences()
    assert tuple(ds["theta"].shape) == (ds["stored"], D)
    v_div, v_all = float(ds["theta"][:, 0].mean()), float(thetas[:, :, 0].mean())
    print(f"funnel run {kw}: {e.divergences()} divergences in {int((ref['ndiv'] > 0).sum())} chains (most in one: "
          f"{int(ref['ndiv'].max())}); mean v at their start {v_div:.3f}, over the run {v_all:.3f}; "
          f"nan {e.nan_transitions()}, pooled E-BFMI {e.ebfmi_pooled():.4f}")
    assert v_div < v_all - 1.0
    return a, rec, ref, store


def check_readouts(e, energies):
    """ebfmi() against np.diff / np.var of the recorded energies, ebfmi_pooled() against the plain formula, rel 1e-12
    (chains with a non-finite energy are compared on their finite ones)."""
    C = energies.shape[1]
    want = np.full(C, np.nan)
    fin = [energies[np.isfinite(energies[:, c]), c] for c in range(C)]
    for c, x in enumerate(fin):
        if x.size >= 2 and x.var() > 0.0:
            want[c] = np.mean(np.diff(x) ** 2) / np.var(x)
    got = e.ebfmi().cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_allclose(got[~np.isnan(want)], want[~np.isnan(want)], rtol=1e-12)
    allx = np.concatenate(fin)
    pooled = (sum(float(np.sum(np.diff(x) ** 2)) for x in fin) / sum(max(x.size - 1, 0) for x in fin)) / np.var(allx)
    np.testing.assert_allclose(e.ebfmi_pooled(), pooled, rtol=1e-12)
    np.testing.assert_allclose(e.energy_mean().cpu().numpy(), [x.mean() if x.size else np.nan for x in fin], rtol=1e-12)
    np.testing.assert_allclose(e.energy_var().cpu().numpy(), [x.var() if x.size else np.nan for x in fin], rtol=1e-10,
                               atol=1e-12)
    return pooled


def check_capacity(bk, ops, big_store, model_ops=None, **kw):
    """capture=16 on the same run: stored == 16, seen == the divergence total, the first 16 entries of the large store."""
    a, rec, _ = run_tracked(bk, ops, capture=16, model_ops=model_ops, **kw)
    ds = a.energy.divergent_states()
    assert ds["stored"] == 16 and ds["seen"] == a.energy.divergences() == int(big_store["fill"][1])
    _eq(ds["theta"].cpu().numpy(), big_store["theta_div"][:, :16].T, "theta")
    _eq(ds["chain"].cpu().numpy(), big_store["chain"][:16], "chain")
    _eq(ds["draw"].cpu().numpy(), big_store["draw"][:16], "draw")
    _eq(ds["energy_error"].cpu().numpy(), big_store["err_store"][:16], "energy_error")


def check_nan_errors(bk, ops, model_ops=None, **kw):
    """stepsize = 2.0: NaN energy errors, every one counted divergent, the energy state finite where cnt > 0."""
    a, rec, _ = run_tracked(bk, ops, draws=12, model_ops=model_ops, stepsize=2.0, **kw)
    e = a.energy
    ref, store, _ = replay_records(rec.records, e.C, e.D, e.capture)
    assert_tracker_equals(e, ref, store)
    nan = sum(int(np.isnan((r["lp_prop"] - r["a_prop"]) - (r["lp_cur"] - r["a_cur"])).sum()) for r in rec.records)
    print(f"stepsize 2.0: {e.nan_transitions()} NaN energy errors, {e.divergences()} divergences, "
          f"{e.nonfinite_energies()} non-finite energies")
    assert e.nan_transitions() == nan > 0 and e.divergences() >= nan
    got = tracker_host(e)
    nan_per_chain = np.zeros(e.C, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for r in rec.records:
            is_nan = np.isnan((r["lp_prop"] - r["a_prop"]) - (r["lp_cur"] - r["a_cur"]))
            nan_per_chain[r["c0"]:r["c0"] + is_nan.shape[0]] += is_nan
    assert (got["ndiv"] >= nan_per_chain).all() and got["div_mask"][is_nan].all()  # every NaN is counted divergent
    live = got["cnt"] > 0
    for k in ("mean_E", "m2_E", "last_E", "ssd"):
        assert np.isfinite(got[k][live]).all(), k
    assert np.array_equal(got["ndiv"] >= 0, np.ones(e.C, dtype=bool)) and got["ndiv"].sum() == e.divergences()


def check_lifecycle(bk, ops, model_ops=None, **kw):
    """A state_dict round trip in the middle of the run continues to the same bits; reset(); untrack_energy() goes back to
    an untracked sampler's launches with draws still equal to the twin's."""
    a, b = funnel_sampler(bk, ops, model_ops, **kw), funnel_sampler(bk, ops, model_ops, **kw)
    twin = funnel_sampler(bk, ops, model_ops, **kw)
    ea, eb = a.track_energy(), b.track_energy()
    for _ in range(12):
        a.sample(), b.sample(), twin.sample()
    sd, sds = ea.state_dict(), a.state_dict()
    c = funnel_sampler(bk, ops, model_ops, **kw)
    c.load_state_dict(sds)
    ec = c.track_energy()
    ec.load_state_dict(sd)
    for _ in range(12):
        oa, oc = a.sample(), c.sample()
        assert torch.equal(oa[0], oc[0])
    ha, hc = tracker_host(ea), tracker_host(ec)
    for k in ha:
        _eq(hc[k], ha[k], "after the round trip: " + k)
    assert ea.divergences() > 0
    for other in (bk.EnergyDiagnostics(ea.C + 1, ea.D, ops=ops), bk.EnergyDiagnostics(ea.C, ea.D, threshold=10.0, ops=ops),
                  bk.EnergyDiagnostics(ea.C, ea.D, capture=8, ops=ops), bk.EnergyDiagnostics(ea.C, ea.D + 1, ops=ops)):
        try:
            other.load_state_dict(sd)
        except ValueError:
            continue
        raise AssertionError("a checkpoint of another shape, threshold or capacity was accepted")
    eb.reset()
    hb = tracker_host(eb)
    assert all(not np.any(v) for v in hb.values()) and eb.transitions == 0 and eb.divergent_states()["stored"] == 0
    assert np.isnan(eb.divergence_rate()) and np.isnan(eb.ebfmi_pooled())
    # untracked again: the twin's draws, and the tracker stands still
    for _ in range(12):
        twin.sample()
    a.untrack_energy()
    assert a.energy is None
    seen = ea.transitions
    for _ in range(3):
        oa, ot = a.sample(), twin.sample()
        assert_same_draw(a, twin, oa, ot)
    assert ea.transitions == seen
    assert_same_end(a, twin)


def check_warmup_report(bk, ops, model_ops=None, **kw):
    """warmup(30) with a tracker attached reports what it reports without one, and leaves the same sampler."""
    a, b = funnel_sampler(bk, ops, model_ops, **kw), funnel_sampler(bk, ops, model_ops, **kw)
    e = a.track_energy()
    ra, rb = a.warmup(30), b.warmup(30)
    assert sorted(ra) == sorted(rb)
    for k in ra:
        assert np.array_equal(np.asarray(ra[k], dtype=np.float64), np.asarray(rb[k], dtype=np.float64), equal_nan=True) \
            if ra[k] is not None else rb[k] is None, k
    assert e.transitions == 30 * a._C
    oa, ob = a.sample(), b.sample()
    assert_same_draw(a, b, oa, ob)
    assert_same_end(a, b)
    return ra, e
