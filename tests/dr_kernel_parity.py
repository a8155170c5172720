"""The delayed-rejection stage helpers (csrc/bk_dr.hip) and the two counted single-step kernels at their lane and list seams:
input builders and checks that take the kernel library as an argument.  Every check runs the same inputs through `ops` and
through a fresh tests.fake_ops.FakeOps() -- the NumPy statement of every entry point, which the CPU suite already holds the
samplers to -- and compares.  tests/test_dr_kernels_cpu.py runs them with ops = FakeOps() and asserts that the inputs reach
every branch; tests/test_gpu_dr_kernels.py runs them on the HIP library.

Comparison rules.  Everything is held to bit equality (any NaN equals any NaN: the sign of a NaN that an `inf - inf` makes is
the processor's; -0.0 differs from 0.0) except the three arrays that hold log1p(-exp(a)) -- rej, cur_h and a ghost's parent
h -- which are within rtol = 1e-14 of the stand-in where finite and identical where not: the allowance of
test_dr_scalar_kernels_vs_fake for the device's log1p / exp against libm.  The appended lists are compared as sets, their
counts exactly (tests/fake_ops.py builds them in reverse lane order: nothing may depend on the order).

Inputs.  A random draw of energies almost never retries, dies, or makes a ghost's probability exactly one, so the builders
PLACE lanes: they read the next two uniforms of every chain's stream from the stand-in's table and choose exp(a) on the side
of each threshold that the wanted class needs, half way into the interval, so that no decision sits on a last-bit difference
(accept_report's `margin`, asserted on the CPU).  Classes are interleaved by lane number, so every prefix of a lane set that a
device-side count cuts off holds them as well.  What is run where, and what it found: profiles/dr_kernel_edges.md."""
import functools
import itertools
from collections import namedtuple

import numpy as np
import torch

from bayes_kit_amd._engine import make_streams, numpy_generator_from_words
from tests.fake_ops import FakeOps

F_SENT, B_SENT, I_SENT = 7.0, 9, -1            # what every output holds before a launch
LANE_SIZES = (1, 63, 64, 65, 255, 256, 257, 700, 1025)
PAD = 37                                       # chains = lanes + PAD: an index is a true subset
KINDS = ("philox", "pcg64")
PROB_RETRY = (1.0, 0.0, 0.35)
N_DEV = ("none", "n", "n+5", "n-70", "0")
STAGE_CHAINS = (1, 63, 64, 65, 700)
N_COUNTERS = (0, 1, 5, 64)
COMPACT_SIZES = (1, 7, 8, 9, 8191, 8192, 8193, 16384, 16385)
DENSITIES = (0.0, 0.03, 0.5, 1.0)
FLAG_BYTES = (1, 2, 0x80, 0xFF)
SCATTER_DIMS = (0, 1, 7, 8, 9, 33)
SCATTER_LANES = (1, 63, 64, 65, 257)
STEP_SHAPES = ((2, 1), (64, 3), (65, 4), (130, 5), (258, 33))
STEP_PADS = (0, 5, 6)
RTOL = 1e-14                                   # log1p(-exp(a)): device vs libm
MARGIN = 1e-13                                 # no retry decision may lie within MARGIN * max(1, |pr * r|) of its threshold


def n_dev_value(n, which):
    return {"none": None, "n": n, "n+5": n + 5, "n-70": max(n - 70, 0), "0": 0}[which]


def lanes(n, which):
    """min(n, *n_dev): the lanes a launch of size n really has."""
    v = n_dev_value(n, which)
    return n if v is None else min(n, v)


# ---- tensors --------------------------------------------------------------------------------------------------------------------
def put(ops, a):
    return torch.from_numpy(np.array(a, copy=True)).to(ops.device)


def get(t):
    return t.detach().cpu().numpy().copy()


def full(ops, n, value, dtype):
    return torch.full((int(n),), value, dtype=dtype, device=ops.device)


def count_tensor(ops, v):
    return None if v is None else torch.tensor([v], dtype=torch.int32, device=ops.device)


def same(a, b):
    """Bit equality, any NaN equal to any NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.float64:
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))


def assert_same(got, want, what):
    assert same(got, want), f"{what}: differs from the stand-in at {np.flatnonzero(~_eq(got, want))[:8]}"


def _eq(a, b):
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    if a.dtype != np.float64:
        return a == b
    return (np.isnan(a) & np.isnan(b)) | (a.view(np.uint64) == b.view(np.uint64))


def assert_close(got, want, what):
    """Within RTOL where finite, identical where infinite or NaN."""
    got, want = np.asarray(got), np.asarray(want)
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(got)) and same(got[~fin], want[~fin]), f"{what}: non-finite entries differ"
    err = np.abs(got[fin] - want[fin])
    assert (err <= RTOL * np.abs(want[fin])).all(), f"{what}: {err.max():.3e} off, beyond rtol {RTOL}"


# ---- streams --------------------------------------------------------------------------------------------------------------------
def _fresh(kind_name, C, device):
    """Philox by an int seed; PCG64 as test_device_rng_pcg64_and_loc_scale seeds it."""
    seed = 31 if kind_name == "philox" else [np.random.default_rng(100 + c) for c in range(C)]
    return make_streams(seed, C, 0, False, device)


def _warm(ops, kind, st):
    """Chain c has made c % 4 earlier draws: fresh streams and every position inside a buffer, in one table."""
    C = st.shape[1]
    out = torch.empty(C, dtype=torch.float64, device=ops.device)
    for k in range(3):
        ops.uniform(kind, st, out, put(ops, (np.arange(C) % 4 > k).astype(np.uint8)))


@functools.lru_cache(maxsize=None)
def stream_table(kind_name, C):
    """(kind, the warmed table's words, the next two uniforms of every chain) by the stand-in."""
    fake = FakeOps()
    kind, st = _fresh(kind_name, C, fake.device)
    _warm(fake, kind, st)
    words = st.numpy().copy()
    u = np.empty((C, 2))
    for c in range(C):
        g = numpy_generator_from_words(kind, words.view(np.uint64)[:, c])
        u[c] = g.uniform(), g.uniform()
    words.setflags(write=False)
    u.setflags(write=False)
    return kind, words, u


def streams(ops, kind_name, C):
    """The warmed table on ops.device; it must stand where the stand-in's stands."""
    kind, words, _ = stream_table(kind_name, C)
    if isinstance(ops, FakeOps):  # (its own table: nothing to learn from warming it again)
        return kind, torch.from_numpy(words.copy())
    k2, st = _fresh(kind_name, C, ops.device)
    _warm(ops, k2, st)
    assert k2 == kind and np.array_equal(get(st), words), "ops.uniform left the streams elsewhere than the stand-in"
    return kind, st


# ---- the accept forms -----------------------------------------------------------------------------------------------------------
AcceptCase = namedtuple("AcceptCase", "n kind pr n_dev index")


def accept_cases():
    """Every lane-set size x generator x n_dev form; prob_retry rotates so that the three full-size forms (none, n, n + 5) of
    every size have the three values; index = None with C = n at one size."""
    out = [AcceptCase(n, kind, PROB_RETRY[(i + k) % 3], nd, True)
           for i, n in enumerate(LANE_SIZES) for kind in KINDS for k, nd in enumerate(N_DEV)]
    out += [AcceptCase(257, kind, pr, "none", False) for kind in KINDS for pr in PROB_RETRY]
    return out


def case_id(c):
    return "-".join(str(v) for v in c)


def _solve_H(frac, cur_H, h, cur_h, pr):
    """H with ((H - cur_H) + (h - cur_h)) + (pr * h - pr * cur_h) ~ frac (a few ulps of the operands off)."""
    return ((frac - (pr * h - pr * cur_h)) - (h - cur_h)) + cur_H


@functools.lru_cache(maxsize=None)
def accept_inputs(n, kind_name, pr, index):
    """Lane classes by lane number j: j % 10 == 3 not live (a = -inf); j % 10 == 7 frac >= 0 (every other one exactly 0);
    lanes 5, 6, 8 carry NaN, +inf, -inf in H; the rest are placed by their chain's next two uniforms u1, u2: accepted
    (exp(a) in (u1, 1)), rejected and retrying (exp(a) < u1 and < L), rejected and dying (L <= exp(a) < u1, where that
    interval exists), with L = 1 - u2^(1 / pr) the value of exp(a) at which log(u2) = pr * log1p(-exp(a))."""
    C = n + PAD if index else n
    rng = np.random.default_rng([n, KINDS.index(kind_name), int(pr * 100), int(index)])
    chain = rng.permutation(C)[:n].astype(np.int32) if index else np.arange(n, dtype=np.int32)
    u = stream_table(kind_name, C)[2][chain]
    u1, u2 = u[:, 0], u[:, 1]
    L = 1.0 - u2 ** (1.0 / pr) if pr > 0 else np.ones(n)   # (pr = 0: pr * r = 0 > log(u2): every rejected lane retries)
    cur_H, cur_h = rng.normal(size=C), -rng.uniform(0, 2, size=C)
    h = -rng.uniform(0, 2, size=n)
    H = np.empty(n)
    live = np.ones(n, dtype=np.uint8)
    a0 = np.full(n, F_SENT)
    general = dying = turn = 0
    for j in range(n):
        c = chain[j]
        if n >= 9 and j in (5, 6, 8):
            H[j] = {5: np.nan, 6: np.inf, 8: -np.inf}[j]
            continue
        if j % 10 == 3:
            live[j], a0[j], H[j] = 0, -np.inf, rng.normal()
            continue
        if j % 10 == 7:
            if (j // 10) % 2:
                h[j], H[j] = cur_h[c], cur_H[c]
            else:
                H[j] = _solve_H(rng.uniform(0.1, 2), cur_H[c], h[j], cur_h[c], pr)
            continue
        general += 1
        if L[j] < u1[j] - 1e-6 and dying < 0.3 * general + 1:
            dying += 1
            t = 0.5 * (L[j] + u1[j])
        elif turn % 2 == 0:
            turn += 1
            t = 0.5 * (u1[j] + 1.0)
        else:
            turn += 1
            t = max(0.5 * min(u1[j], L[j]), 1e-300)
        H[j] = _solve_H(np.log(t), cur_H[c], h[j], cur_h[c], pr)
    alive0 = np.full(C, B_SENT, dtype=np.uint8)
    alive0[chain] = 1
    out = dict(C=C, chain=chain, u=u, H=H, h=h, live=live, a=a0, cur_H=cur_H, cur_h=cur_h, alive=alive0)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def accept_run(ops, case, form):
    """One of `unfused` (dr_accept_prob, dr_accept_test), `fused` (dr_accept_prob_test), `next` (dr_accept_prob_test_next)."""
    inp = accept_inputs(case.n, case.kind, case.pr, case.index)
    n, C = case.n, inp["C"]
    kind, st = streams(ops, case.kind, C)
    t = {k: put(ops, inp[k]) for k in ("H", "h", "live", "a", "cur_H", "cur_h", "alive")}
    t["rej"] = full(ops, C, F_SENT, torch.float64)
    t["accepted"] = full(ops, n, B_SENT, torch.uint8)
    t["next_index"] = full(ops, n, I_SENT, torch.int32)
    t["next_count"] = full(ops, 1, 0, torch.int32)
    idx = put(ops, inp["chain"]) if case.index else None
    nd = count_tensor(ops, n_dev_value(n, case.n_dev))
    if form == "unfused":
        ops.dr_accept_prob(t["H"], t["cur_H"], t["h"], t["cur_h"], idx, case.pr, t["live"], t["a"], n, nd)
        ops.dr_accept_test(kind, st, idx, t["a"], t["H"], n, t["cur_H"], t["cur_h"], t["rej"], t["alive"], t["accepted"], nd)
    elif form == "fused":
        ops.dr_accept_prob_test(kind, st, idx, t["H"], t["h"], t["live"], t["a"], case.pr, n, t["cur_H"], t["cur_h"], t["rej"],
                                t["alive"], t["accepted"], nd)
    else:
        ops.dr_accept_prob_test_next(kind, st, idx, t["H"], t["h"], t["live"], t["a"], case.pr, n, t["cur_H"], t["cur_h"],
                                     t["rej"], t["alive"], t["accepted"], t["next_index"], t["next_count"], nd)
    out = {k: get(v) for k, v in t.items()}
    out["state"] = get(st)
    return out


@functools.lru_cache(maxsize=None)
def accept_reference(case):
    fake = FakeOps()
    return {form: accept_run(fake, case, form) for form in ("fused", "next")}


EXACT = ("accepted", "alive", "cur_H", "a", "state")
CLOSE = ("rej", "cur_h")


def _assert_list(got, want, what):
    k = int(want["next_count"][0])
    assert int(got["next_count"][0]) == k, f"{what}: count {int(got['next_count'][0])}, the stand-in's {k}"
    assert sorted(got["next_index"][:k].tolist()) == sorted(want["next_index"][:k].tolist()), f"{what}: another set"
    assert (got["next_index"][k:] == I_SENT).all(), f"{what}: entries past the count were written"


def check_accept_forms(ops, case):
    inp = accept_inputs(case.n, case.kind, case.pr, case.index)
    ref = accept_reference(case)
    eff = lanes(case.n, case.n_dev)
    words = stream_table(case.kind, inp["C"])[1]
    got = {form: accept_run(ops, case, form) for form in ("unfused", "fused", "next")}
    # what no launch may touch: lanes at and beyond the count, chains outside the index, their streams
    out_chain = np.ones(inp["C"], dtype=bool)
    out_chain[inp["chain"][:eff]] = False
    for form, g in got.items():
        assert (g["accepted"][eff:] == B_SENT).all() and same(g["a"][eff:], inp["a"][eff:]), (form, "lanes past the count")
        assert same(g["alive"][out_chain], inp["alive"][out_chain]) and (g["rej"][out_chain] == F_SENT).all(), form
        assert same(g["cur_H"][out_chain], inp["cur_H"][out_chain]) and same(g["cur_h"][out_chain], inp["cur_h"][out_chain]), form
        assert np.array_equal(g["state"][:, out_chain], words[:, out_chain]), (form, "streams of untouched chains")
        for k in ("H", "h", "live"):
            assert same(g[k], inp[k]), (form, k, "an input was written")
    assert (got["fused"]["next_index"] == I_SENT).all() and got["fused"]["next_count"][0] == 0
    # the fused launch is the two launches (the same device arithmetic: every array bit for bit)
    for k in EXACT + CLOSE:
        assert_same(got["fused"][k], got["unfused"][k], f"dr_accept_prob_test vs dr_accept_prob + dr_accept_test: {k}")
    # ... and the appending form decides as they do
    for k in ("accepted", "cur_H", "a", "rej", "cur_h"):
        assert_same(got["next"][k], got["fused"][k], f"dr_accept_prob_test_next vs dr_accept_prob_test: {k}")
    # both against the specification
    for form in ("fused", "next"):
        for k in EXACT:
            assert_same(got[form][k], ref[form][k], f"{form}: {k}")
        for k in CLOSE:
            assert_close(got[form][k], ref[form][k], f"{form}: {k}")
    _assert_list(got["next"], ref["next"], "the chains that propose again")


def accept_report(case):
    """The classes the stand-in's outputs put the effective lanes in, and the least margin of a retry decision."""
    inp = accept_inputs(case.n, case.kind, case.pr, case.index)
    ref = accept_reference(case)["next"]
    eff = lanes(case.n, case.n_dev)
    chain = inp["chain"][:eff]
    acc = ref["accepted"][:eff] == 1
    again = np.isin(chain, ref["next_index"][: int(ref["next_count"][0])])
    a = ref["a"][:eff]
    with np.errstate(invalid="ignore"):
        thr = case.pr * ref["rej"][chain]
    lu2 = np.log(inp["u"][:eff, 1])
    dec = ~acc & ~np.isnan(thr)
    margin = np.abs(lu2[dec] - thr[dec]) / np.maximum(1.0, np.abs(thr[dec]))
    assert (ref["alive"][chain] == again).all() and not (acc & again).any()
    return dict(eff=eff, accepted=int((acc & (a < 0)).sum()), retry=int(again.sum()), die=int((~acc & ~again).sum()),
                not_live=int((inp["live"][:eff] == 0).sum()), a_zero=int(((a == 0) & (inp["live"][:eff] == 1)).sum()),
                nan=int(np.isnan(inp["H"][:eff]).sum()), pinf=int((inp["H"][:eff] == np.inf).sum()),
                ninf=int((inp["H"][:eff] == -np.inf).sum()), margin=float(margin.min()) if margin.size else np.inf)


# ---- the ghost forms ------------------------------------------------------------------------------------------------------------
GhostCase = namedtuple("GhostCase", "n pr n_dev sub")


def ghost_cases():
    return [GhostCase(n, PROB_RETRY[(i + k + s) % 3], nd, bool(s))
            for i, n in enumerate(LANE_SIZES) for k, nd in enumerate(N_DEV) for s in (1, 0)]


@functools.lru_cache(maxsize=None)
def ghost_inputs(n, pr, sub):
    """Ghost lane j of parent lane p = sub_index[j].  j % 10 == 3: not live, a = -inf (the parent goes on, h unchanged);
    j % 10 == 7: frac >= 0 (a = 0 kills the parent), every other one exactly 0; j % 10 == 9: not live with a = -0.0 (j % 20
    == 9) or 0.0 (kills the parent); lanes 5, 6, 8: NaN, +inf (a = 0) and -inf in H; the rest frac < 0."""
    P = n + PAD if sub else n
    rng = np.random.default_rng([n, int(pr * 100), int(sub), 5])
    par = rng.permutation(P)[:n].astype(np.int32) if sub else np.arange(n, dtype=np.int32)
    par_H, par_h = rng.normal(size=P), -rng.uniform(0, 2, size=P)
    h = -rng.uniform(0, 2, size=n)
    H = np.empty(n)
    live = np.ones(n, dtype=np.uint8)
    a0 = np.full(n, F_SENT)
    for j in range(n):
        p = par[j]
        if n >= 9 and j in (5, 6, 8):
            H[j] = {5: np.nan, 6: np.inf, 8: -np.inf}[j]
        elif j % 10 == 3:
            live[j], a0[j], H[j] = 0, -np.inf, rng.normal()
        elif j % 10 == 9:
            live[j], a0[j], H[j] = 0, (-0.0 if j % 20 == 9 else 0.0), rng.normal()
        elif j % 10 == 7 and (j // 10) % 2:
            h[j], H[j] = par_h[p], par_H[p]
        else:
            frac = rng.uniform(0.1, 2) if j % 10 == 7 else -rng.uniform(0.01, 3)
            H[j] = _solve_H(frac, par_H[p], h[j], par_h[p], pr)
    par_live = np.full(P, B_SENT, dtype=np.uint8)
    par_live[par] = 1
    out = dict(P=P, par=par, H=H, h=h, live=live, a=a0, par_H=par_H, par_h=par_h, par_live=par_live)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def ghost_run(ops, case, form):
    inp = ghost_inputs(case.n, case.pr, case.sub)
    n, P = case.n, inp["P"]
    t = {k: put(ops, inp[k]) for k in ("H", "h", "live", "a", "par_H", "par_h", "par_live")}
    t["par_a"] = full(ops, P, F_SENT, torch.float64)
    t["next_index"] = full(ops, n, I_SENT, torch.int32)
    t["next_count"] = full(ops, 1, 0, torch.int32)
    sub = put(ops, inp["par"]) if case.sub else None
    nd = count_tensor(ops, n_dev_value(n, case.n_dev))
    if form == "unfused":
        ops.dr_accept_prob(t["H"], t["par_H"], t["h"], t["par_h"], sub, case.pr, t["live"], t["a"], n, nd)
        ops.dr_ghost_update(t["a"], sub, n, t["par_h"], t["par_live"], t["par_a"], nd)
    elif form == "fused":
        ops.dr_accept_prob_ghost(t["H"], t["par_H"], t["h"], t["par_h"], sub, case.pr, t["live"], t["a"], n, t["par_live"],
                                 t["par_a"], nd)
    else:
        ops.dr_accept_prob_ghost_next(t["H"], t["par_H"], t["h"], t["par_h"], sub, case.pr, t["live"], t["a"], n,
                                      t["par_live"], t["par_a"], t["next_index"], t["next_count"], nd)
    return {k: get(v) for k, v in t.items()}


@functools.lru_cache(maxsize=None)
def ghost_reference(case):
    fake = FakeOps()
    with np.errstate(divide="ignore", invalid="ignore"):
        return {form: ghost_run(fake, case, form) for form in ("fused", "next")}


def check_ghost_forms(ops, case):
    inp = ghost_inputs(case.n, case.pr, case.sub)
    ref = ghost_reference(case)
    eff = lanes(case.n, case.n_dev)
    with np.errstate(divide="ignore", invalid="ignore"):
        got = {form: ghost_run(ops, case, form) for form in ("unfused", "fused", "next")}
    out_par = np.ones(inp["P"], dtype=bool)
    out_par[inp["par"][:eff]] = False
    for form, g in got.items():
        assert same(g["a"][eff:], inp["a"][eff:]), (form, "lanes past the count")
        assert same(g["par_live"][out_par], inp["par_live"][out_par]) and (g["par_a"][out_par] == F_SENT).all(), form
        assert same(g["par_h"][out_par], inp["par_h"][out_par]), (form, "parents outside the set")
        for k in ("H", "h", "live", "par_H"):
            assert same(g[k], inp[k]), (form, k, "an input was written")
    assert (got["fused"]["next_index"] == I_SENT).all() and got["fused"]["next_count"][0] == 0
    for k in ("a", "par_live", "par_a", "par_h"):
        assert_same(got["fused"][k], got["unfused"][k], f"dr_accept_prob_ghost vs dr_accept_prob + dr_ghost_update: {k}")
        assert_same(got["next"][k], got["fused"][k], f"dr_accept_prob_ghost_next vs dr_accept_prob_ghost: {k}")
    for form in ("fused", "next"):
        for k in ("a", "par_live", "par_a"):
            assert_same(got[form][k], ref[form][k], f"{form}: {k}")
        assert_close(got[form]["par_h"], ref[form]["par_h"], f"{form}: par_h")
    _assert_list(got["next"], ref["next"], "the parents that go on")


def ghost_report(case):
    inp = ghost_inputs(case.n, case.pr, case.sub)
    ref = ghost_reference(case)["next"]
    eff = lanes(case.n, case.n_dev)
    par = inp["par"][:eff]
    a, live = ref["a"][:eff], inp["live"][:eff]
    killed = ref["par_live"][par] == 0
    assert int(ref["next_count"][0]) == int((~killed).sum()) and (np.isneginf(ref["par_a"][par]) == killed).all()
    return dict(eff=eff, goes_on=int((~killed & (live == 1)).sum()), a_zero=int((killed & (live == 1)).sum()),
                not_live=int(((live == 0) & np.isneginf(a)).sum()),
                neg_zero=int(((live == 0) & (a == 0) & np.signbit(a)).sum()),
                pos_zero=int(((live == 0) & (a == 0) & ~np.signbit(a)).sum()), nan=int(np.isnan(inp["H"][:eff]).sum()),
                pinf=int((inp["H"][:eff] == np.inf).sum()), ninf=int((inp["H"][:eff] == -np.inf).sum()))


# ---- the stage scalars ----------------------------------------------------------------------------------------------------------
def _energies(C, rng):
    """log p and kinetic energy with a NaN, +inf, -inf, an infinite kinetic energy and an inf - inf among them."""
    logp, kin = rng.normal(size=C), rng.uniform(0, 5, size=C)
    if C >= 9:
        logp[1], logp[2], logp[3], kin[4] = np.nan, np.inf, -np.inf, np.inf
        logp[5], kin[5] = np.inf, np.inf
    return logp, kin


@functools.lru_cache(maxsize=None)
def retry_inputs(C, kind_name):
    """dr_retry_test: rej = log(uniform), exactly 0 at c % 10 == 3, -inf at c % 10 == 7 (0 * -inf = NaN: the test fails);
    three chains in ten are not alive and must not draw."""
    rng = np.random.default_rng([C, KINDS.index(kind_name), 9])
    rej = np.log(rng.uniform(size=C))
    rej[np.arange(C) % 10 == 3] = 0.0
    rej[np.arange(C) % 10 == 7] = -np.inf
    alive = (rng.uniform(size=C) < 0.7).astype(np.uint8)
    if C == 1:
        alive[:] = 1
    return rej, alive


def retry_margin(C, kind_name):
    """Least |log(u) - pr * rej| / max(1, |pr * rej|) over the chains dr_retry_test decides, for every prob_retry."""
    rej, alive = retry_inputs(C, kind_name)
    lu = np.log(stream_table(kind_name, C + PAD)[2][:C, 0])
    least = np.inf
    for pr in PROB_RETRY:
        with np.errstate(invalid="ignore"):
            thr = pr * rej
        dec = (alive == 1) & ~np.isnan(thr) & np.isfinite(thr)
        if dec.any():
            least = min(least, float((np.abs(lu[dec] - thr[dec]) / np.maximum(1.0, np.abs(thr[dec]))).min()))
    return least


@np.errstate(invalid="ignore", divide="ignore")  # (the stand-in's inf - inf and 0 * inf: wanted here)
def check_stage_scalars(ops, C, kind_name):
    """dr_begin, dr_level_begin, dr_begin_retry, dr_retry_test and dr_accept_prob against the stand-in, bit for bit."""
    rng = np.random.default_rng([C, 77])
    logp, kin = _energies(C, rng)

    def outputs(o, n):
        return ([full(o, n, F_SENT, torch.float64) for _ in range(3)], full(o, n, B_SENT, torch.uint8))

    # dr_begin
    res = []
    for o in (ops, FakeOps()):
        (H, h, rej), alive = outputs(o, C)
        o.dr_begin(put(o, logp), put(o, kin), H, h, rej, alive)
        res.append([get(x) for x in (H, h, rej, alive)])
    for g, w, name in zip(res[0], res[1], ("H", "h", "rej", "alive")):
        assert_same(g, w, f"dr_begin: {name}")
    assert (res[0][1] == 0).all() and (res[0][2] == 0).all() and (res[0][3] == 1).all()
    # dr_level_begin: every n_dev form
    for which in N_DEV:
        eff, res = lanes(C, which), []
        for o in (ops, FakeOps()):
            (H, h, _), live = outputs(o, C)
            o.dr_level_begin(put(o, logp), put(o, kin), H, h, live, C, count_tensor(o, n_dev_value(C, which)))
            res.append([get(x) for x in (H, h, live)])
        for g, w, name in zip(res[0], res[1], ("H", "h", "live")):
            assert_same(g, w, f"dr_level_begin n_dev = {which}: {name}")
        assert (res[0][0][eff:] == F_SENT).all() and (res[0][1][eff:] == F_SENT).all() and (res[0][2][eff:] == B_SENT).all()
        assert (res[0][1][:eff] == 0).all() and (res[0][2][:eff] == 1).all()
    # dr_begin_retry on the first C chains of a wider table: counters zeroed, the draw counter one on (or absent)
    words = stream_table(kind_name, C + PAD)[1]
    for k, nc in enumerate(N_COUNTERS):
        pr, with_draws, res = PROB_RETRY[k % 3], k % 2 == 0, []
        for o in (ops, FakeOps()):
            kind, st = streams(o, kind_name, C + PAD)
            (H, h, rej), alive = outputs(o, C)
            buf = full(o, 70, B_SENT, torch.int32)
            draws = torch.tensor([41], dtype=torch.int64, device=o.device) if with_draws else None
            o.dr_begin_retry(kind, st[:, :C], put(o, logp), put(o, kin), H, h, rej, alive, pr, buf[:nc] if nc else None, draws)
            res.append([get(x) for x in (H, h, rej, alive, st, buf)] + [None if draws is None else int(draws.item())])
        for g, w, name in zip(res[0][:5], res[1][:5], ("H", "h", "rej", "alive", "state")):
            assert_same(g, w, f"dr_begin_retry n_counters = {nc}: {name}")
        assert (res[0][3] == 1).all(), "rej = 0: the first retry test passes for every chain"
        assert np.array_equal(res[0][4][:, C:], words[:, C:]), "streams of chains past C"
        assert (res[0][5][:nc] == 0).all() and (res[0][5][nc:] == B_SENT).all(), f"counters, n_counters = {nc}"
        assert res[0][6] == (42 if with_draws else None)
    # dr_retry_test
    rej_in, alive_in = retry_inputs(C, kind_name)
    for pr in PROB_RETRY:
        res = []
        for o in (ops, FakeOps()):
            kind, st = streams(o, kind_name, C + PAD)
            alive = put(o, alive_in)
            o.dr_retry_test(kind, st[:, :C], put(o, rej_in), pr, alive)
            res.append((get(alive), get(st)))
        assert_same(res[0][0], res[1][0], f"dr_retry_test prob_retry = {pr}: alive")
        assert_same(res[0][1], res[1][1], f"dr_retry_test prob_retry = {pr}: state")
        idle = np.ones(C + PAD, dtype=bool)
        idle[:C] = alive_in == 0
        assert np.array_equal(res[0][1][:, idle], words[:, idle]), "a chain that is not alive drew"
    # dr_accept_prob alone: C lanes of C + PAD chains, every n_dev form
    inp = accept_inputs(C, kind_name, 0.35, True)
    for which in N_DEV:
        res = []
        for o in (ops, FakeOps()):
            a = put(o, inp["a"])
            o.dr_accept_prob(put(o, inp["H"]), put(o, inp["cur_H"]), put(o, inp["h"]), put(o, inp["cur_h"]), put(o, inp["chain"]),
                             0.35, put(o, inp["live"]), a, C, count_tensor(o, n_dev_value(C, which)))
            res.append(get(a))
        assert_same(res[0], res[1], f"dr_accept_prob n_dev = {which}: a")
        assert same(res[0][lanes(C, which):], inp["a"][lanes(C, which):])


# ---- compaction -----------------------------------------------------------------------------------------------------------------
def compaction_flags(n, density, seed):
    rng = np.random.default_rng([n, int(density * 100), seed])
    flags = np.where(rng.uniform(size=n) < density, rng.choice(FLAG_BYTES, size=n), 0).astype(np.uint8)
    if density == 1.0:
        assert flags.all()
    return flags


def check_compaction(ops, n):
    """Every density x byte offset of the mask (0: the 8-bytes-per-load path; 1..7: one byte per load) x n_dev form.  The
    bytes around the mask are set, so a load past either end shows as an index."""
    for density, off, which in itertools.product(DENSITIES, range(8), N_DEV):
        flags = compaction_flags(n, density, off)
        host = np.full(n + 24, 0xFF, dtype=np.uint8)
        host[8 + off: 8 + off + n] = flags
        buf = put(ops, host)
        mask = buf[8 + off: 8 + off + n]
        assert (mask.data_ptr() - off) % 8 == 0 and mask.data_ptr() % 8 == off
        idx = full(ops, n, I_SENT, torch.int32)
        cnt = full(ops, 1, B_SENT, torch.int32)
        ops.compact_indices(mask, n, idx, cnt, count_tensor(ops, n_dev_value(n, which)))
        want = np.flatnonzero(flags[: lanes(n, which)])
        what = (n, density, off, which)
        assert int(cnt.item()) == len(want), (what, int(cnt.item()), len(want))
        got = get(idx)
        assert np.array_equal(got[: len(want)], want), what
        assert (got[len(want):] == I_SENT).all(), (what, "entries past the count were written")
        assert np.array_equal(get(buf), host), (what, "the mask was written")


# ---- scatter --------------------------------------------------------------------------------------------------------------------
class _NoRows:
    """A [0, w] array AT AN ADDRESS, which bk_scatter_columns asks for even when D = 0 (a torch tensor without elements
    has none): the first row of `t` seen as no rows at all."""

    def __init__(self, t):
        self._t, self.shape = t, (0, t.shape[1])

    def dim(self):
        return 2

    def stride(self, i=None):
        return self._t.stride() if i is None else self._t.stride(i)

    def data_ptr(self):
        return self._t.data_ptr()

    def numpy(self):
        return self._t.numpy()[:0]


def check_scatter(ops, n, D):
    """One to three arrays of D rows, with and without the scalar pair, with an index and without, every n_dev form, masks of
    zeros, ones and flag bytes; source and destination are views of wider buffers at different pitches, and the whole
    buffers are compared: a column that is not selected, and whatever lies beside the views, must not change."""
    rng = np.random.default_rng([n, D, 3])
    masks = {"zeros": np.zeros(n, dtype=np.uint8), "ones": np.ones(n, dtype=np.uint8), "flags": compaction_flags(n, 0.5, 1)}
    for arrays, scalars, with_index, which, mk in itertools.product((1, 2, 3), (False, True), (True, False), N_DEV, masks):
        C = n + PAD if with_index else n
        index = rng.permutation(C)[:n].astype(np.int32) if with_index else None
        src_h = [rng.normal(size=(D + 1, n + 11)) for _ in range(arrays)]
        dst_h = [rng.normal(size=(D + 1, C + 5)) for _ in range(arrays)]
        ssrc_h, sdst_h = rng.normal(size=n), rng.normal(size=C)
        res = []
        for o in (ops, FakeOps()):
            src_b, dst_b = [put(o, x) for x in src_h], [put(o, x) for x in dst_h]
            if D:
                srcs, dsts = [b[:D, 3: 3 + n] for b in src_b], [b[:D, 2: 2 + C] for b in dst_b]
            else:
                srcs, dsts = [_NoRows(b[:1, 3: 3 + n]) for b in src_b], [_NoRows(b[:1, 2: 2 + C]) for b in dst_b]
            assert dsts[0].data_ptr() != 0 and srcs[0].data_ptr() != 0
            sdst = put(o, sdst_h) if scalars else None
            o.scatter_columns(put(o, masks[mk]), None if index is None else put(o, index), n, dsts, srcs, sdst,
                              put(o, ssrc_h) if scalars else None, count_tensor(o, n_dev_value(n, which)))
            res.append([get(b) for b in dst_b] + [get(b) for b in src_b] + ([get(sdst)] if scalars else []))
        what = (arrays, scalars, with_index, which, mk)
        for g, w in zip(res[0], res[1]):
            assert_same(g, w, f"scatter_columns {what}")
        # ... and against the plain statement, so that the stand-in is not the only witness
        sel = np.flatnonzero(masks[mk][: lanes(n, which)])
        to = sel if index is None else index[sel]
        for k in range(arrays):
            want = dst_h[k].copy()
            want[:D, 2 + to] = src_h[k][:D, 3 + sel]
            assert same(res[0][k], want), what
        if scalars:
            want = sdst_h.copy()
            want[to] = ssrc_h[sel]
            assert same(res[0][-1], want), what


# ---- the counted single steps ---------------------------------------------------------------------------------------------------
def _step_view(o, host, D, C, ld, off):
    buf = put(o, host)
    return buf, torch.as_strided(buf, (D, C), (ld, 1), off)


def check_single_step(ops, C, D, target):
    """bk_leapfrog_step_gaussian / bk_leapfrog_step_funnel in place on a [D, C] view at pitch C + pad, from the buffer's start
    (16-byte aligned) and one column on (8-byte aligned only), with and without lam and the metric, every n_dev form.  The
    whole buffers are compared: the pad, and the columns beyond the count, keep what they held."""
    rng = np.random.default_rng([C, D, 11])
    h = 0.0625 + 0.01
    lam_h, metric_h = rng.uniform(0.5, 2.0, size=D), rng.uniform(0.5, 1.5, size=D)
    lams = (True, False) if target == "gaussian" else (False,)
    for pad, off, with_lam, with_metric, which in itertools.product(STEP_PADS, (0, 1), lams, (True, False), N_DEV):
        ld = C + pad
        size = D * ld + 1
        th_h, rho_h = rng.normal(size=size), rng.normal(size=size)
        at = (np.arange(D)[:, None] * ld + np.arange(C)[None, :] + off).ravel()   # the view's elements
        beside = np.ones(size, dtype=bool)
        beside[at] = False
        th_h[beside], rho_h[beside] = F_SENT, F_SENT
        eff = lanes(C, which)
        what = (target, C, D, pad, off, with_lam, with_metric, which)
        res = []
        for o, direct in ((ops, True), (ops if target == "funnel" else FakeOps(), False)):
            tb, th = _step_view(o, th_h, D, C, ld, off)
            rb, rho = _step_view(o, rho_h, D, C, ld, off)
            if direct:
                assert th.data_ptr() % 16 == 8 * off
            lam = put(o, lam_h) if with_lam else None
            metric = put(o, metric_h) if with_metric else None
            nd = count_tensor(o, n_dev_value(C, which))
            if target == "gaussian":
                o.leapfrog_step_gaussian(lam, th, rho, metric, h, nd)
            elif direct:
                o.leapfrog_step_funnel(th, rho, metric, h, nd)
            else:  # the gradient op and the kick + drift launch on the same device
                _, g = _step_view(o, np.zeros(size), D, C, ld, off)
                o.target_grad("funnel", None, th, g, None, nd)
                o.kick_drift(th, th, rho, rho, g, metric, h, False, 0.0, True, h, nd)
            res.append((get(tb), get(rb)))
        assert_same(res[0][0], res[1][0], f"theta {what}")
        assert_same(res[0][1], res[1][1], f"rho {what}")
        for g, start in zip(res[0], (th_h, rho_h)):
            assert (g[beside] == F_SENT).all(), (what, "written beside the view")
            keep = (np.arange(D)[:, None] * ld + np.arange(eff, C)[None, :] + off).ravel()
            assert same(g[keep], start[keep]), (what, "columns beyond the count")
            if eff and D:
                moved = (np.arange(D)[:, None] * ld + np.arange(eff)[None, :] + off).ravel()
                assert (g[moved] != start[moved]).all(), (what, "a column of the set did not move")
