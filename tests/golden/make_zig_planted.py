#!/usr/bin/env python3
"""Regenerates tests/golden/zig_planted.json: Philox (and two PCG64) states that put the rare events of NumPy's ziggurat
stream at chosen positions of the first window of the word-parallel generator (csrc/bk_rng.hip, zig_parallel_wave).

    python tests/golden/make_zig_planted.py            # ~2 minutes, no GPU; the output is byte-for-byte reproducible

The scan is deterministic: the streams np.random.Philox(key=[KEY0, j]), j = 0 .. N_KEYS-1, WORDS_PER_KEY words each,
classified word by word with the committed ziggurat tables (oracle.rng.ziggurat_tables).  A fresh Philox(key) stands at
counter 0 with buffer_pos 4, so its stream word s is word s % 4 of block s // 4 + 1; the state (counter = B,
buffer_pos = bp) therefore puts stream word s at window position s + 4 - 4 B and starts consuming at position bp.  For
every event class and window size the first scanned candidate whose walk shows the wanted facts -- and whose wedge
comparisons and tails stay clear of the limits tests/zig_planted.py states -- is taken; the chosen entry is then verified
with the sequential walker and numpy.random.Generator before it is written.  Classes with no candidate are listed in the
output's "not_found" (and so in profiles/zig_planted.md), never dropped silently.

The output holds keys, counters, buffer_pos, D, the window size / lanes per chain / chain count of the launch the entry
is meant for, and the claimed facts; nothing else.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.rng import ziggurat_tables  # noqa: E402
from tests import zig_planted as zp  # noqa: E402

KEY0 = 20261020
N_KEYS = 10
WORDS_PER_KEY = 1 << 22
PCG_SEEDS = (20261020, 20261021)
PCG_WORDS = 1 << 21
LPCS = (16, 32, 64)
ORD_D = {16: 57, 32: 100, 64: 121}      # one-pass launches for the ordering / carry-in / counter classes (121: the
                                        # smallest D that takes 64 lanes per chain at 70 chains)
ORD_P = {16: 20, 32: 40, 64: 80}        # window position (rounded up to the anchor's residue mod 4) of their events
LAST_P = {16: 44, 32: 100, 64: 200}     # ... of the last-dimension classes (D follows from the walk)
LATE_D = {16: 40, 32: 90, 64: 200}      # D of the classes whose events lie BEHIND the last dimension
M64 = (1 << 64) - 1

KI, WI, FI = (np.array(t) for t in ziggurat_tables())
KI = KI.astype(np.uint64)


class Scan:
    """One scanned stream: positional class of every word (0 fast, 1 wedge, 2 tail), wedge outcomes and margins,
    positional tail lengths."""

    def __init__(self, words, key=None):
        self.key = key
        self.w = words
        n = len(words)
        idx = (words & np.uint64(0xFF)).astype(np.intp)
        rabs = (words >> np.uint64(9)) & np.uint64(0x000FFFFFFFFFFFFF)
        fail = rabs >= KI[idx]
        self.cls = np.where(fail, np.where(idx == 0, 2, 1), 0).astype(np.uint8)
        wpos = np.flatnonzero(self.cls == 1)
        wpos = wpos[wpos + 1 < n]
        x = rabs[wpos].astype(np.float64) * WI[idx[wpos]]
        u = (words[wpos + 1] >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
        lhs = (FI[idx[wpos] - 1] - FI[idx[wpos]]) * u + FI[idx[wpos]]
        rhs = np.exp(-0.5 * x * x)
        self.wacc = np.zeros(n, dtype=bool)
        self.wacc[wpos] = lhs < rhs
        self.wmargin = np.full(n, np.inf)
        self.wmargin[wpos] = np.abs(lhs - rhs) / rhs
        self.tlen = {}
        for i in np.flatnonzero(self.cls == 2):
            i = int(i)
            self.tlen[i] = zp.tail_len([int(v) for v in words[i:i + 80]], 0)
        self.tl = np.zeros(n, dtype=np.int32)  # positional tail length as an array (0: not a tail start / ran out)
        for i, L in self.tlen.items():
            self.tl[i] = L or 0

    def walk(self, t, D):
        """Attempts (s, len, kind, emit, dim) of the D normals consumed from stream index t; (None, None) near the end."""
        i, d, att = t, 0, []
        cls, n = self.cls, len(self.w)
        while d < D:
            if i >= n - 128:
                return None, None
            c = cls[i]
            if c == 0:
                att.append((i, 1, "F", True, d))
                d += 1
                i += 1
            elif c == 1:
                e = bool(self.wacc[i])
                att.append((i, 2, "W", e, d if e else None))
                d += 1 if e else 0
                i += 2
            else:
                L = self.tlen[i]
                if not L:
                    return None, None
                att.append((i, L, "T", True, d))
                d += 1
                i += L
        return att, i


class Ctx:
    """A candidate placement: anchor s0 at window position p with buffer_pos bp."""

    def __init__(self, sc, s0, p, bp):
        self.sc, self.s0, self.p, self.bp = sc, s0, p, bp
        self.ok = (s0 - p) % 4 == 0 and (s0 + 4 - p) // 4 >= 1
        self.B = (s0 + 4 - p) // 4
        self.t = 4 * self.B + bp - 4  # stream index of the first word consumed

    def win(self, s):
        return s + 4 - 4 * self.B

    def run(self, D):
        self.D = D
        self.att, self.end = self.sc.walk(self.t, D)
        if self.att is None:
            return False
        self.starts = {a[0]: a for a in self.att}
        return True

    def cls(self, s):
        return "FWT"[int(self.sc.cls[s])]

    def f_class(self, s):
        return ["class", self.win(s), self.cls(s)]

    def f_attempt(self, s):
        a = self.starts[s]
        return ["attempt", self.win(s), a[1], a[2], a[3]]


def entry(c, name, lpc, C, facts):
    return dict(name=name, kind="philox", ww=4 * lpc, lpc=lpc, C=C, D=c.D, key=[int(c.sc.key[0]), int(c.sc.key[1])],
                counter=[int(c.B), 0, 0, 0], buffer_pos=c.bp, facts=facts)


def accept(e):
    """The slow, independent verification: walker + numpy + the safety limits."""
    try:
        _, normals, final, _ = zp.check_facts(e)
        zp.check_safety(e)
    except AssertionError:
        return False
    z, w = zp.expected(e, e["D"])
    return (np.array_equal(z.view(np.uint64), normals.view(np.uint64)) and [int(v) for v in w[2:6]] == final["counter"]
            and [int(v) for v in w[6:10]] == final["buffer"] and int(w[10]) == final["buffer_pos"])


def res_p(p0, s0):
    """The smallest window position >= p0 with the anchor's residue mod 4."""
    return p0 + ((s0 - p0) % 4)


def vary_bp(s0):
    return 1 + (s0 // 4) % 4


# ---- the event classes ----------------------------------------------------------------------------------------------
# each: name -> (anchors(sc) -> index array, make(sc, s0, lpc) -> entry or None)
def _fixed(name, shape, p_of, cond, bp_of=vary_bp):
    """A class with a fixed launch shape: shape(lpc) -> (C, D); p_of(ww, s0) -> window position of the anchor;
    cond(ctx) -> facts or None (the anchor must be the start of an attempt unless cond says otherwise)."""
    def make(sc, s0, lpc):
        C, D = shape(lpc)
        c = Ctx(sc, s0, p_of(4 * lpc, s0), bp_of(s0))
        if not c.ok or not c.run(D):
            return None
        facts = cond(c)
        return None if facts is None else entry(c, name, lpc, C, facts)
    return make


def _multi(lpc):
    return zp.MULTI[lpc]


def _small(lpc):
    return zp.SMALL_C, ORD_D[lpc]


def _late(lpc):
    return zp.SMALL_C, LATE_D[lpc]


def _started(extra=lambda c: []):
    def cond(c):
        if c.s0 not in c.starts:
            return None
        return [c.f_class(c.s0), c.f_attempt(c.s0)] + extra(c)
    return cond


def _idx(mask, lo=2048):
    i = np.flatnonzero(mask)
    return i[(i >= lo) & (i < len(mask) - 2048)]


def _sh(a, k):
    """a shifted so that out[s] = a[s + k]."""
    out = np.zeros_like(a)
    out[:len(a) - k] = a[k:]
    return out


CLASSES = {}


def add(name, anchors, make, lpcs=LPCS):
    CLASSES[name] = (anchors, make, lpcs)


def _passes2(c):
    return [["passes", 2]] if c.end > c.win(c.s0) else None


# window end: the event is consumed (the launch goes on into a second window)
def _end(extra=lambda c: []):
    def cond(c):
        base = _started(extra)(c)
        return None if base is None or c.win(c.end) <= c.p + 1 else base + [["passes", 2]]
    return cond


add("end_wedge_last", lambda sc: _idx(sc.cls == 1), _fixed("end_wedge_last", _multi, lambda ww, s: ww - 1, _end()))
add("end_tail_last", lambda sc: _idx(sc.cls == 2), _fixed("end_tail_last", _multi, lambda ww, s: ww - 1, _end()))
for acc in (True, False):
    for nxt_fail in (False, True):
        nm = "end_wedge_m2_%s_%s" % ("acc" if acc else "rej", "lastfails" if nxt_fail else "lastpasses")
        add(nm, (lambda acc, nxt_fail: lambda sc: _idx((sc.cls == 1) & (sc.wacc == acc) & ((_sh(sc.cls, 1) != 0) == nxt_fail)))(acc, nxt_fail),
            _fixed(nm, _multi, lambda ww, s: ww - 2, _end(lambda c: [c.f_class(c.s0 + 1), ["covered", c.win(c.s0 + 1)]])))
for L, off, nm in ((3, 3, "end_tail3_fits"), (3, 2, "end_tail3_runs_out"), (5, 5, "end_tail5_fits"), (5, 4, "end_tail5_runs_out")):
    add(nm, (lambda L: lambda sc: _idx(sc.tl == L))(L),
        _fixed(nm, _multi, (lambda off: lambda ww, s: ww - off)(off), _end(lambda c: [["taillen", c.win(c.s0), int(c.sc.tl[c.s0])]])))


# ordering
def _p_ord(ww, s):
    return res_p(ORD_P[ww // 4], s)


def _cov1(c):
    return [c.f_class(c.s0 + 1), ["covered", c.win(c.s0 + 1)]]


add("adj_in_lane", lambda sc: _idx((sc.cls == 1) & (_sh(sc.cls, 1) != 0) & (np.arange(len(sc.cls)) % 4 != 3)),
    _fixed("adj_in_lane", _small, _p_ord, _started(_cov1)))
add("adj_cross_lane", lambda sc: _idx((sc.cls == 1) & (_sh(sc.cls, 1) != 0) & (np.arange(len(sc.cls)) % 4 == 3)),
    _fixed("adj_cross_lane", _small, _p_ord, _started(_cov1)))


def _three(c):
    out = [c.f_class(c.s0 + 1), c.f_class(c.s0 + 2)]
    for s in (c.s0 + 1, c.s0 + 2):
        out.append(c.f_attempt(s) if s in c.starts else ["covered", c.win(s)])
    return out


add("three_in_row", lambda sc: _idx((sc.cls != 0) & (_sh(sc.cls, 1) != 0) & (_sh(sc.cls, 2) != 0)),
    _fixed("three_in_row", _small, _p_ord, _started(_three)))
add("fail_then_tail_word", lambda sc: _idx((sc.cls == 1) & (_sh(sc.cls, 1) == 2)),
    _fixed("fail_then_tail_word", _small, _p_ord, _started(_cov1)))
add("fail_then_tail_attempt", lambda sc: _idx((sc.cls == 1) & (_sh(sc.cls, 2) == 2)),
    _fixed("fail_then_tail_attempt", _small, _p_ord, _started(lambda c: [c.f_class(c.s0 + 2), c.f_attempt(c.s0 + 2)])))


def _anch_fail_in_tail(sc):
    out = [i for i, L in sc.tlen.items() if L and sc.cls[i + 1:i + L].any()]
    return _idx(np.isin(np.arange(len(sc.cls)), out))


def _fail_in_tail(c):
    L = c.starts[c.s0][1]
    out = [["taillen", c.win(c.s0), L]]
    for s in range(c.s0 + 1, c.s0 + L):
        if c.sc.cls[s]:
            out += [c.f_class(s), ["covered", c.win(s)]]
    return out


add("fail_in_tail_pairs", _anch_fail_in_tail, _fixed("fail_in_tail_pairs", _small, _p_ord, _started(_fail_in_tail)))
add("lane_k0_k2", lambda sc: _idx((sc.cls == 1) & (_sh(sc.cls, 2) != 0) & (np.arange(len(sc.cls)) % 4 == 0)),
    _fixed("lane_k0_k2", _small, _p_ord, _started(lambda c: [c.f_class(c.s0 + 2), c.f_attempt(c.s0 + 2)])))
add("rej_wedge_then_exception", lambda sc: _idx((sc.cls == 1) & ~sc.wacc & (_sh(sc.cls, 2) != 0)),
    _fixed("rej_wedge_then_exception", _small, _p_ord, _started(lambda c: [c.f_class(c.s0 + 2), c.f_attempt(c.s0 + 2)])))


def _anch_longest(sc):
    return _idx(sc.tl == LONGEST[0])


LONGEST = [0]
add("longest_tail", _anch_longest,
    _fixed("longest_tail", _small, _p_ord, _started(lambda c: [["taillen", c.win(c.s0), int(c.sc.tl[c.s0])]])))

# carry-in
for bp in (1, 2, 3, 4):
    add("carry_bp%d" % bp, lambda sc: _idx(sc.cls == 1),
        _fixed("carry_bp%d" % bp, _small, _p_ord, _started(lambda c: [["buffer_pos", c.bp]]), (lambda bp: lambda s: bp)(bp)))
add("carry_consumed_fail", lambda sc: _idx(sc.cls != 0),
    _fixed("carry_consumed_fail", _small, lambda ww, s: s % 4, lambda c: [c.f_class(c.s0), ["consumed_fail", c.p], ["buffer_pos", c.bp]],
           lambda s: s % 4 + 1))


# last dimension: D follows from the walk
def _last(name, p_of, pick, facts_of, d_range=None, bp_of=vary_bp):
    """pick(ctx) -> stream index of the attempt that must emit dimension D - 1 (walked with the largest D first)."""
    def make(sc, s0, lpc):
        lo, hi = d_range or zp.D_RANGE[lpc]
        c = Ctx(sc, s0, p_of(4 * lpc, s0), bp_of(s0))
        if not c.ok or not c.run(hi + 8):
            return None
        s_last = pick(c)
        if s_last is None or s_last not in c.starts or not c.starts[s_last][3]:
            return None
        D = c.starts[s_last][4] + 1
        if not lo <= D <= hi or not c.run(D):
            return None
        facts = [["dim", c.win(s_last), D - 1], c.f_attempt(s_last), ["end", c.win(c.end)]] + facts_of(c)
        return entry(c, name, lpc, zp.SMALL_C, facts)
    return make


def _p_last(ww, s):
    return res_p(LAST_P[ww // 4], s)


def _anch_fast_end(sc):
    n = len(sc.cls)
    cum = np.concatenate([[0], np.cumsum(sc.cls != 0)])
    near = cum[:n] - cum[np.maximum(np.arange(n) - 56, 0)]  # failing words among the 56 before
    return _idx((sc.cls == 0) & (np.arange(n) % 4 == 3) & (near >= 2))


add("last_fast_at_window_end", _anch_fast_end,
    _last("last_fast_at_window_end", lambda ww, s: ww - 1, lambda c: c.s0, lambda c: [], bp_of=lambda s: 4))
add("last_wedge_accepted", lambda sc: _idx((sc.cls == 1) & sc.wacc), _last("last_wedge_accepted", _p_last, lambda c: c.s0, lambda c: []))
add("last_tail", lambda sc: _idx(sc.cls == 2), _last("last_tail", _p_last, lambda c: c.s0, lambda c: []))
add("last_wedge_accepted_small_D", lambda sc: _idx((sc.cls == 1) & sc.wacc),
    _last("last_wedge_accepted_small_D", lambda ww, s: res_p(12, s), lambda c: c.s0, lambda c: [], d_range=(1, 31)), lpcs=(16,))
add("last_tail_small_D", lambda sc: _idx(sc.cls == 2),
    _last("last_tail_small_D", lambda ww, s: res_p(20, s), lambda c: c.s0, lambda c: [], d_range=(1, 31)), lpcs=(16,))


def _prev_emits(c, s):
    i = c.att.index(c.starts[s])
    return i > 0 and c.att[i - 1][3]


add("last_after_one_rejected_wedge", lambda sc: _idx((sc.cls == 1) & ~sc.wacc),
    _last("last_after_one_rejected_wedge", _p_last,
          lambda c: c.s0 + 2 if c.s0 in c.starts and _prev_emits(c, c.s0) else None, lambda c: [c.f_attempt(c.s0)]))
add("last_after_two_rejected_wedges", lambda sc: _idx((sc.cls == 1) & ~sc.wacc & (_sh(sc.cls, 2) == 1) & ~_sh(sc.wacc, 2)),
    _last("last_after_two_rejected_wedges", _p_last,
          lambda c: c.s0 + 4 if c.s0 in c.starts and _prev_emits(c, c.s0) else None,
          lambda c: [c.f_attempt(c.s0), c.f_attempt(c.s0 + 2)]))


def _ends_at(c):
    for a in c.att:
        if a[0] + a[1] == c.s0:
            return a[0] if a[3] else None
    return None


add("last_then_rejected_wedge", lambda sc: _idx((sc.cls == 1) & ~sc.wacc),
    _last("last_then_rejected_wedge", _p_last, _ends_at,
          lambda c: [c.f_class(c.s0), ["wedge", c.p, False], ["unconsumed", c.p]]))
add("last_then_tail_start", lambda sc: _idx(sc.cls == 2),
    _last("last_then_tail_start", _p_last, _ends_at, lambda c: [c.f_class(c.s0), ["unconsumed", c.p]]))


# behind the last dimension, in the same window: nothing of it may reach the written-back state
def _late_cond(extra=lambda c: []):
    def cond(c):
        if c.win(c.end) > c.p - 4:
            return None
        return [c.f_class(c.s0), ["unconsumed", c.p], ["end", c.win(c.end)], ["passes", 1]] + extra(c)
    return cond


add("late_tail_out_of_window", lambda sc: _idx(sc.tl >= 3),
    _fixed("late_tail_out_of_window", _late, lambda ww, s: ww - 2, _late_cond(lambda c: [["taillen", c.p, int(c.sc.tl[c.s0])]])))
add("late_failing_last_word", lambda sc: _idx(sc.cls != 0),
    _fixed("late_failing_last_word", _late, lambda ww, s: ww - 1, _late_cond()))
add("late_neighbouring_exceptions", lambda sc: _idx((sc.cls != 0) & (_sh(sc.cls, 1) != 0)),
    _fixed("late_neighbouring_exceptions", _late, lambda ww, s: res_p(ww - 12, s), _late_cond(lambda c: [c.f_class(c.s0 + 1)])))


# sequential pair logic (next_normal_pair(Philox&) of the one-lane kernels): the anchor is the first word of an even dimension
def _pair(name, facts_of, odd_last=False):
    def make(sc, s0, lpc):
        for back in (range(36, 48) if odd_last else range(24, 32)):
            t = s0 - back
            B, bp = (t // 4, 4) if t % 4 == 0 else (t // 4 + 1, t % 4)
            c = Ctx(sc, s0, s0 + 4 - 4 * B, bp)
            if not c.ok or not c.run(ORD_D[lpc]):
                continue
            first, d = {}, 0
            for a in c.att:
                first.setdefault(d, a[0])
                d += 1 if a[3] else 0
            dd = [k for k, v in first.items() if v == s0]
            if not dd:
                continue
            if odd_last:
                D = dd[0] + 1
                if D % 2 == 0 or D < 32 or not c.run(D):
                    continue
                return entry(c, name, lpc, zp.SMALL_C, [["odd_last", c.cls(s0)], ["dim", c.win(c.att[-1][0]), D - 1]])
            if dd[0] % 2 or dd[0] + 1 >= c.D:
                continue
            return entry(c, name, lpc, zp.SMALL_C, [["pair", dd[0], c.cls(s0), c.cls(s0 + 1)]] + facts_of(c, dd[0]))
        return None
    return make


add("pair_first_fails", lambda sc: _idx((sc.cls == 1) & (_sh(sc.cls, 1) == 0)), _pair("pair_first_fails", lambda c, d: []), lpcs=(16,))
add("pair_second_fails", lambda sc: _idx((sc.cls == 0) & (_sh(sc.cls, 1) != 0)), _pair("pair_second_fails", lambda c, d: []), lpcs=(16,))
add("pair_both_fail", lambda sc: _idx((sc.cls != 0) & (_sh(sc.cls, 1) != 0)), _pair("pair_both_fail", lambda c, d: []), lpcs=(16,))
add("pair_unget_crosses_refill", lambda sc: _idx((sc.cls == 1) & (np.arange(len(sc.cls)) % 4 == 3)),
    _pair("pair_unget_crosses_refill", lambda c, d: [["pair_r0_block_last", d]]), lpcs=(16,))
add("pair_tail_first", lambda sc: _idx(sc.cls == 2), _pair("pair_tail_first", lambda c, d: []), lpcs=(16,))
add("odd_D_ends_on_exception", lambda sc: _idx(sc.cls != 0), _pair("odd_D_ends_on_exception", None, odd_last=True), lpcs=(16,))


# ---- counter carries: no scan, any stream will do; the first key whose stream passes the safety limits -------------------
def counter_entries():
    out = []
    for lpc in LPCS:
        specs = [("ctr_carry_between_lanes", [M64 - lpc // 2 + 1, 0, 0, 0], 4, [["carry_lane", lpc // 2]]),
                 ("ctr_carry_between_lanes", [M64, 7, 0, 0], 2, [["carry_lane", 1]]),
                 ("ctr_carry_between_lanes", [M64 - lpc + 2, M64, 5, 0], 1, [["carry_lane", lpc - 1]]),
                 ("ctr_two_limbs_max", [M64, M64, 0, 0], 3, [["limbs_max"], ["carry_lane", 1]]),
                 ("ctr_two_limbs_max", [M64, M64, M64, 0], 4, [["limbs_max"], ["carry_lane", 1]]),
                 ("ctr_written_back_crosses", [M64 - 2, 0, 0, 0], 4, [["carry_lane", 3], ["final_crosses_carry"]])]
        for n, (name, ctr, bp, facts) in enumerate(specs):
            for j in range(1000, 1200):
                e = dict(name=name, kind="philox", ww=4 * lpc, lpc=lpc, C=zp.SMALL_C, D=ORD_D[lpc], key=[KEY0, j + 200 * n],
                         counter=ctr, buffer_pos=bp, facts=facts)
                if accept(e):
                    out.append(e)
                    break
            else:
                raise SystemExit(f"no stream for {name}")
    return out


# ---- PCG64 (one-lane kernels only) ---------------------------------------------------------------------------------------
def pcg_entries(stats):
    out = []
    scans = [Scan(np.random.PCG64(seed).random_raw(PCG_WORDS)) for seed in PCG_SEEDS]
    stats["pcg64_words"] = PCG_WORDS * len(PCG_SEEDS)
    wants = (("pcg_tail", lambda sc: _idx(sc.cls == 2, 64)),
             ("pcg_rejected_then_accepted_wedge", lambda sc: _idx((sc.cls == 1) & ~sc.wacc & (_sh(sc.cls, 2) == 1) & _sh(sc.wacc, 2), 64)))
    for (name, anch), sc, seed in zip(wants, scans, PCG_SEEDS):
        cands = anch(sc)
        stats["candidates"][name] = int(len(cands))
        for s0 in cands:
            s0 = int(s0)
            t = s0 - 21
            att, end = sc.walk(t, 40)
            if att is None or s0 not in {a[0] for a in att}:
                continue
            if min(sc.wmargin[a[0]] for a in att) <= zp.MARGIN:
                continue
            kinds = [a for a in att if a[0] >= s0][:1 if name == "pcg_tail" else 2]
            out.append(dict(name=name, kind="pcg64", ww=0, lpc=0, C=1, D=40, seed=seed, advance=t,
                            facts=[["attempt", a[0] - t, a[1], a[2], a[3]] for a in kinds]))
            break
    return out


def main():
    stats = {"keys": [[KEY0, j] for j in range(N_KEYS)], "words_per_key": WORDS_PER_KEY, "words": N_KEYS * WORDS_PER_KEY,
             "candidates": {}, "tail_lengths": {}, "wedges": 0, "rejected_wedges": 0}
    scans = []
    for j in range(N_KEYS):
        sc = Scan(np.random.Philox(key=[KEY0, j]).random_raw(WORDS_PER_KEY), key=(KEY0, j))
        scans.append(sc)
        for L in sc.tlen.values():
            k = str(L or "unfinished")
            stats["tail_lengths"][k] = stats["tail_lengths"].get(k, 0) + 1
        stats["wedges"] += int((sc.cls == 1).sum())
        stats["rejected_wedges"] += int(((sc.cls == 1) & ~sc.wacc).sum())
    LONGEST[0] = max(int(sc.tl.max()) for sc in scans)
    stats["longest_tail"] = LONGEST[0]
    out, not_found = [], []
    for name, (anchors, make, lpcs) in CLASSES.items():
        cands = [anchors(sc) for sc in scans]
        stats["candidates"][name] = int(sum(len(c) for c in cands))
        for lpc in lpcs:
            found = None
            tried = refused = 0
            for sc, cc in zip(scans, cands):
                for s0 in cc:
                    e = make(sc, int(s0), lpc)
                    tried += 1
                    if e is not None:
                        if accept(e):
                            found = e
                            break
                        refused += 1
                        if refused > 200:
                            raise SystemExit(f"{name}: 200 candidates refused by the verification")
                if found:
                    break
            if found:
                out.append(found)
            else:
                not_found.append({"name": name, "ww": 4 * lpc, "candidates_tried": tried, "words_scanned": stats["words"]})
            print(name, 4 * lpc, "ok" if found else "NOT FOUND", tried, flush=True)
    assert LONGEST[0] >= 7
    out += counter_entries()
    out += pcg_entries(stats)
    stats["tail_lengths"] = dict(sorted(stats["tail_lengths"].items(), key=lambda kv: (len(kv[0]), kv[0])))
    doc = {"scan": stats, "not_found": not_found, "entries": out}
    with open(zp.FIXTURE, "w") as f:
        f.write("{\n \"scan\": " + json.dumps(stats) + ",\n \"not_found\": " + json.dumps(not_found) + ",\n \"entries\": [\n")
        f.write(",\n".join("  " + json.dumps(e) for e in out))
        f.write("\n ]\n}\n")
    print(len(out), "entries;", len(not_found), "not found;", os.path.getsize(zp.FIXTURE), "bytes")
    return doc


if __name__ == "__main__":
    main()
