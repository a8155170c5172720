"""Planted stream events for the word-parallel normal generator (TEST INFRASTRUCTURE).

``tests/golden/zig_planted.json`` (written by ``tests/golden/make_zig_planted.py``) holds Philox states -- key, counter,
``buffer_pos`` -- chosen so that a rare event of NumPy's ziggurat stream (a wedge or tail attempt, a rejected wedge,
neighbouring exceptions, a counter carry, ...) lands at a stated position of the FIRST window the kernel
``zig_parallel_wave`` of ``csrc/bk_rng.hip`` evaluates.  Window coordinates: position ``q`` is word ``q % 4`` of block
``counter + q // 4``; the first ``buffer_pos`` positions are consumed already (a fresh ``np.random.Philox`` has
``buffer_pos = 4``: its first stream word is position 4).

Here: the fixture loader, a sequential walker on ``oracle.rng.PhiloxStream`` that reports every attempt (start
position, length, kind, emitted value), the checker of a fixture entry's claimed facts, the state-table builder and the
GPU check functions that ``tests/test_gpu_zig_planted.py`` shares between its cases.
"""
from __future__ import annotations

import json
import math
import os

import numpy as np

from oracle.rng import M64, ZIG_INV_R, ZIG_R, PhiloxStream, philox4x64_10, ziggurat_tables

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zig_planted.json")
MARGIN = 1e-12  # smallest relative margin of a wedge comparison a planted stream may contain
MAX_TAIL = 15   # longest positional tail (words) near a planted stream's consumed range

# window sizes and the (C, D) launches that select them (bk_normals_lanes_per_chain confirms every one)
SMALL_C = 70
D_RANGE = {16: (32, 57), 32: (58, 120), 64: (121, 247)}  # one pass at C = SMALL_C
MULTI = {16: (32768, 101), 32: (16384, 200), 64: (SMALL_C, 300)}  # more than one pass


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def entries(kind="philox"):
    return [e for e in load_fixture()["entries"] if e["kind"] == kind]


def ctr_add(counter, k):
    """The 256-bit counter (four 64-bit limbs, least significant first) plus k."""
    v = sum(int(c) << (64 * i) for i, c in enumerate(counter)) + int(k)
    return [(v >> (64 * i)) & M64 for i in range(4)]


def block_of(entry, b):
    """Block ``counter + b`` of the entry's stream."""
    return philox4x64_10(ctr_add(entry["counter"], b), [int(k) for k in entry["key"]])


def window_words(entry, n):
    """The words at window positions 0 .. n-1."""
    out = []
    for b in range((n + 3) // 4):
        out.extend(block_of(entry, b))
    return out[:n]


def state_words(entry) -> np.ndarray:
    """uint64[11]: key, counter, buffer (= the block the counter names, as NumPy holds it), buffer_pos."""
    w = np.zeros(11, dtype=np.uint64)
    w[0:2] = [int(k) for k in entry["key"]]
    w[2:6] = [int(c) for c in entry["counter"]]
    w[6:10] = block_of(entry, 0)
    w[10] = entry["buffer_pos"]
    return w


def numpy_generator(entry) -> np.random.Generator:
    """numpy's own generator standing exactly at the entry's state."""
    if entry["kind"] == "pcg64":
        bg = np.random.PCG64(int(entry["seed"]))
        bg.advance(int(entry["advance"]))
        return np.random.Generator(bg)
    bg = np.random.Philox(key=np.array([int(k) for k in entry["key"]], dtype=np.uint64))
    st = bg.state
    st["state"]["counter"] = np.array([int(c) for c in entry["counter"]], dtype=np.uint64)
    st["buffer"] = np.array(block_of(entry, 0), dtype=np.uint64)
    st["buffer_pos"] = int(entry["buffer_pos"])
    st["has_uint32"], st["uinteger"] = 0, 0
    bg.state = st
    return np.random.Generator(bg)


# ---- word classes (positional: what an attempt STARTING at the word would do) -------------------------------------
def word_class(w):
    """'F': passes the fast test; 'W': fails it, a wedge attempt (2 words); 'T': fails it with table index 0, a tail."""
    ki, _, _ = ziggurat_tables()
    idx = w & 0xFF
    rabs = (w >> 9) & 0x000FFFFFFFFFFFFF
    if rabs < ki[idx]:
        return "F"
    return "T" if idx == 0 else "W"


def wedge_test(w, w_next):
    """(accepted, relative margin of the comparison) of the wedge attempt that starts at w and reads w_next."""
    _, wi, fi = ziggurat_tables()
    idx = w & 0xFF
    rabs = (w >> 9) & 0x000FFFFFFFFFFFFF
    x = rabs * wi[idx]
    u = (w_next >> 11) * (1.0 / 9007199254740992.0)
    lhs = (fi[idx - 1] - fi[idx]) * u + fi[idx]
    rhs = math.exp(-0.5 * x * x)
    return lhs < rhs, abs(lhs - rhs) / rhs


def tail_len(words, i, limit=10 ** 9):
    """Words of the tail attempt that starts at words[i] (1 + 2 pairs tried); None if the list (or limit) runs out."""
    j = i + 1
    while j + 1 < len(words) and j + 2 - i <= limit:
        xx = -ZIG_INV_R * math.log1p(-((words[j] >> 11) * (1.0 / 9007199254740992.0)))
        yy = -math.log1p(-((words[j + 1] >> 11) * (1.0 / 9007199254740992.0)))
        if yy + yy > xx * xx:
            return j + 2 - i
        j += 2
    return None


# ---- the sequential walker ----------------------------------------------------------------------------------------
class _CountingStream(PhiloxStream):
    def __init__(self, entry):
        super().__init__(int(entry["key"][0]), int(entry["key"][1]))
        self.counter = [int(c) for c in entry["counter"]]
        self.buffer = block_of(entry, 0)
        self.buffer_pos = int(entry["buffer_pos"])
        self.pos = self.buffer_pos  # window position of the next word

    def next_u64(self):
        self.pos += 1
        return super().next_u64()


def walk(entry, D=None):
    """The entry's next D normals, one attempt at a time.  Returns ``(attempts, normals, final_state, end)``:
    ``attempts`` = list of ``(pos, length, kind, emit, dim, value)`` -- pos: window position of the attempt's first
    word; kind 'F' / 'W' / 'T'; emit False for a rejected wedge (dim, value None); ``normals`` the D values;
    ``final_state`` the dict ``PhiloxStream.state()`` gives; ``end`` the window position of the next unconsumed word."""
    ki, wi, fi = ziggurat_tables()
    D = entry["D"] if D is None else D
    s = _CountingStream(entry)
    attempts, normals = [], []
    while len(normals) < D:
        p0 = s.pos
        r = s.next_u64()
        idx = r & 0xFF
        sign = (r >> 8) & 1
        rabs = (r >> 9) & 0x000FFFFFFFFFFFFF
        x = rabs * wi[idx]
        if sign:
            x = -x
        if rabs < ki[idx]:
            kind, emit, val = "F", True, x
        elif idx == 0:
            kind, emit = "T", True
            while True:
                xx = -ZIG_INV_R * math.log1p(-s.next_double())
                yy = -math.log1p(-s.next_double())
                if yy + yy > xx * xx:
                    val = -(ZIG_R + xx) if (rabs >> 8) & 1 else ZIG_R + xx
                    break
        else:
            kind = "W"
            emit = (fi[idx - 1] - fi[idx]) * s.next_double() + fi[idx] < math.exp(-0.5 * x * x)
            val = x
        if emit:
            attempts.append((p0, s.pos - p0, kind, True, len(normals), val))
            normals.append(val)
        else:
            attempts.append((p0, s.pos - p0, kind, False, None, None))
    return attempts, np.array(normals, dtype=np.float64), s.state(), s.pos


def walk_words(words, D):
    """The same walk over a plain list of stream words (any bit generator): attempts ``(index, length, kind, emit, dim)``
    and the index of the next unconsumed word."""
    i, d, att = 0, 0, []
    while d < D:
        k = word_class(words[i])
        if k == "F":
            n, emit = 1, True
        elif k == "W":
            n, emit = 2, wedge_test(words[i], words[i + 1])[0]
        else:
            n, emit = tail_len(words, i), True
        att.append((i, n, k, emit, d if emit else None))
        d += 1 if emit else 0
        i += n
    return att, i


# ---- facts ----------------------------------------------------------------------------------------------------------
def check_facts(entry):
    """Every claimed fact of a Philox entry against the walker and the words themselves; returns the walk."""
    attempts, normals, final, end = walk(entry)
    starts = {a[0]: a for a in attempts}
    covered = set()
    for a in attempts:
        covered.update(range(a[0] + 1, a[0] + a[1]))
    n_words = max([end + 4] + [f[1] + 40 for f in entry["facts"] if f[0] in ("class", "taillen", "attempt")])
    words = window_words(entry, n_words)
    first_of_dim = {}  # dimension -> window position of the first word consumed for it (rejected attempts included)
    d = 0
    for a in attempts:
        first_of_dim.setdefault(d, a[0])
        if a[3]:
            d += 1
    for f in entry["facts"]:
        what = f[0]
        if what == "class":
            assert word_class(words[f[1]]) == f[2], (entry["name"], f)
        elif what == "attempt":
            a = starts.get(f[1])
            assert a is not None and [a[1], a[2], a[3]] == f[2:5], (entry["name"], f, a)
        elif what == "covered":
            assert f[1] in covered and f[1] not in starts, (entry["name"], f)
        elif what == "dim":
            a = starts.get(f[1])
            assert a is not None and a[3] and a[4] == f[2], (entry["name"], f, a)
        elif what == "end":
            assert end == f[1], (entry["name"], f, end)
        elif what == "unconsumed":
            assert f[1] >= end, (entry["name"], f, end)
        elif what == "taillen":
            assert word_class(words[f[1]]) == "T" and tail_len(words, f[1]) == f[2], (entry["name"], f)
        elif what == "wedge":  # positional wedge outcome
            assert word_class(words[f[1]]) == "W" and wedge_test(words[f[1]], words[f[1] + 1])[0] == f[2], (entry["name"], f)
        elif what == "pair":  # k_refresh's pair that starts dimension d: classes of the two words it pops
            p = first_of_dim[f[1]]
            assert f[1] % 2 == 0 and f[1] + 1 < entry["D"], (entry["name"], f)
            assert [word_class(words[p]), word_class(words[p + 1])] == f[2:4], (entry["name"], f)
        elif what == "pair_r0_block_last":
            assert first_of_dim[f[1]] % 4 == 3, (entry["name"], f)
        elif what == "odd_last":  # the single normal that ends an odd D starts on a word of this class
            assert entry["D"] % 2 == 1 and word_class(words[first_of_dim[entry["D"] - 1]]) == f[1], (entry["name"], f)
        elif what == "consumed_fail":  # a word of the current block, consumed before the state was taken, fails the fast test
            assert f[1] < entry["buffer_pos"] and word_class(words[f[1]]) != "F", (entry["name"], f)
        elif what == "buffer_pos":
            assert entry["buffer_pos"] == f[1], (entry["name"], f)
        elif what == "carry_lane":  # block `counter + m` is the first of the window whose low limb wrapped
            m = f[1]
            assert 0 < m < entry["lpc"], (entry["name"], f)
            assert ctr_add(entry["counter"], m - 1)[0] == M64 and ctr_add(entry["counter"], m)[0] == 0, (entry["name"], f)
        elif what == "limbs_max":  # counter[0] = counter[1] = 2^64 - 1
            assert [int(c) for c in entry["counter"][:2]] == [M64, M64], (entry["name"], f)
        elif what == "final_crosses_carry":
            assert int(entry["counter"][0]) > (1 << 63) and final["counter"][0] < (1 << 63), (entry["name"], f)
        elif what == "passes":  # the D normals need words beyond the first window
            assert (end > entry["ww"]) == (f[1] > 1), (entry["name"], f, end)
        else:
            raise AssertionError(f"unknown fact {f!r} in {entry['name']}")
    return attempts, normals, final, end


def check_safety(entry):
    """Wedge margins in the consumed range; no long positional tail anywhere a pass may look."""
    attempts, _, _, end = walk(entry)
    n = int(1.1 * entry["D"] + 2 * entry["ww"])
    words = window_words(entry, n + 2 * MAX_TAIL + 8)
    for a in attempts:
        if a[2] == "W":
            acc, margin = wedge_test(words[a[0]], words[a[0] + 1])
            assert acc == a[3] and margin > MARGIN, (entry["name"], a, margin)
    assert end <= n, (entry["name"], end, n)
    for q in range(n):
        if word_class(words[q]) == "T":
            L = tail_len(words, q, limit=MAX_TAIL + 2)
            assert L is not None and L <= MAX_TAIL, (entry["name"], q, L)


# ---- the window bookkeeping of zig_parallel_wave, restated for ONE chain ------------------------------------------------
# What the kernel does per pass with ballots, DPP scans and LDS, written as plain loops over the window's words: which
# words are left to the next pass, which start an attempt, where the next window begins, where the stream stands after
# dimension D - 1.  tests/test_zig_planted_cpu.py holds it to the sequential walker on every fixture entry, records which
# branch every entry takes in its first window, and plants faults in it (FAULTS) to show that the fixture notices each.
FAULTS = (
    "deferred_word_not_covered",     # the window's failing last word emits in this pass as well
    "carry_ignores_cover",           # an attempt reaching into the next window is forgotten (carry = stop - 4 adv)
    "carry_ignores_stop",            # the next window's carry comes from `cover` alone
    "always_shortcut",               # the ballot shortcut is taken whatever the exceptions look like
    "shortcut_misses_next_lane",     # ... and does not cover word 0 of the lane behind a failing word 3
    "short_tail_keeps_later_words",  # words behind a tail that ran out of window still emit
    "rejected_wedge_emits",
    "last_end_ignores_length",       # the written-back position ends one word after the START of dimension D - 1
    "last_end_from_later_words",     # ... or follows whatever the last pass covered
    "ordered_walk_ignores_cover",    # every exception starts an attempt in the ordered walk
    "counter_without_carry",         # the window's block counters wrap in the low limb only
)


def window_model(entry, fault=None):
    """Returns (dims, end, counter, passes): dims[d] = (window-0 position, words) of the attempt that emits dimension d;
    end = position of the first unconsumed word; counter = the written-back counter; passes = per pass, the set of
    branches taken ('defer', 'short', 'shortcut', 'ordered', 'tail', 'two_in_lane', 'covered_exception', 'neighbours',
    'cover_gt_stop')."""
    lpc, WW, D, v0 = entry["lpc"], entry["ww"], entry["D"], entry["buffer_pos"]
    key = [int(k) for k in entry["key"]]
    add = ctr_add
    if fault == "counter_without_carry":
        def add(c, k):
            return [(int(c[0]) + k) & M64] + [int(x) for x in c[1:]]
    base, carry, d_base = 0, v0, 0
    dims, passes = [], []
    last_end, last_base = -1, 0
    while d_base < D:
        assert len(passes) < 64
        br = set()
        words = []
        for lane in range(lpc):
            words.extend(philox4x64_10(add(entry["counter"], base + lane), key))
        cls = [word_class(w) for w in words]
        fail = [c != "F" for c in cls]
        cov = [q < carry for q in range(WW)]
        stop = WW
        if fail[WW - 1]:  # the window's last word cannot start an attempt here: left to the next pass
            fail[WW - 1] = False
            cov[WW - 1] = fault != "deferred_word_not_covered"
            stop = WW - 1
            br.add("defer")
        length, emit = [1] * WW, [True] * WW
        short_at, tail_here = WW, False
        for lane in range(lpc):
            if sum(fail[4 * lane:4 * lane + 4]) > 1:
                br.add("two_in_lane")
        for q in range(WW):
            if not fail[q]:
                continue
            if cls[q] == "T":
                tail_here = True
                br.add("tail")
                L = tail_len(words, q)  # (pairs inside the window only)
                if L is None:
                    short_at = min(short_at, q)
                else:
                    length[q] = L
            else:
                length[q] = 2
                emit[q] = wedge_test(words[q], words[q + 1])[0] or fault == "rejected_wedge_emits"
        if short_at < WW:  # a tail ran out of window: the pass stops in front of it
            br.add("short")
            stop = min(stop, short_at)
            for q in range(short_at, WW):
                if fault != "short_tail_keeps_later_words" or q == short_at:
                    fail[q] = False
                    cov[q] = True
        exc = [q for q in range(WW) if fail[q]]
        cover = carry
        covered_exc = any(cov[q] for q in exc)
        neighbours = any(q + 1 in exc for q in exc)
        if covered_exc:
            br.add("covered_exception")
        if neighbours:
            br.add("neighbours")
        if exc and (fault in ("always_shortcut", "shortcut_misses_next_lane") or not (tail_here or covered_exc or neighbours)):
            br.add("shortcut")
            for q in exc:
                if q + 1 < WW and not (fault == "shortcut_misses_next_lane" and q % 4 == 3):
                    cov[q + 1] = True
            cover = exc[-1] + 2
        elif exc:
            br.add("ordered")
            for q in exc:
                if q >= cover or fault == "ordered_walk_ignores_cover":
                    cover = q + length[q]
                    for j in range(q + 1, min(q + length[q], WW)):
                        cov[j] = True
        for q in range(WW):
            if not cov[q] and emit[q]:
                if d_base < D:
                    dims.append((4 * base + q, length[q]))
                if d_base == D - 1:
                    last_end = q + (1 if fault == "last_end_ignores_length" else length[q])
                    last_base = base
                d_base += 1
        if cover > stop:
            br.add("cover_gt_stop")
        adv = stop >> 2
        assert adv > 0
        if fault == "carry_ignores_cover":
            carry = stop - 4 * adv
        elif fault == "carry_ignores_stop":
            carry = max(cover - 4 * adv, 0)
        else:
            carry = max(cover, stop) - 4 * adv
        if fault == "last_end_from_later_words":
            last_end, last_base = max(cover, last_end if last_base == base else 0), base
        base += adv
        passes.append(br)
    end = 4 * last_base + last_end
    counter = [int(c) for c in entry["counter"]]
    if end > v0:
        counter = add(counter, (end - 1) // 4)
    return dims, end, counter, passes


def model_agrees(entry, fault=None):
    """The model's attempts, end of stream and written-back counter against the sequential walker's."""
    attempts, _, final, end = walk(entry)
    want = [(a[0], a[1]) for a in attempts if a[3]]
    try:
        dims, m_end, counter, _ = window_model(entry, fault)
    except (AssertionError, IndexError, TypeError):  # (a fault may send the model off the rails: that is "noticed")
        return False
    return dims == want and m_end == end and counter == final["counter"]


# ---- state tables and GPU checks --------------------------------------------------------------------------------------
def planted_columns(C, n, shift=0):
    """Columns for n planted chains: the first, inner and last segments of wavefronts, next to unplanted neighbours,
    the table's first and last chain included."""
    if n == 0:
        return []
    if n >= C:
        return list(range(C))
    if n < 4:  # (a launch with few planted chains: not always the table's first column)
        return sorted((1 + 3 * shift + i * (C // n)) % C for i in range(n))
    cols = sorted({int(round(i * (C - 1) / max(n - 1, 1))) for i in range(n)})
    c = 0
    while len(cols) < n:  # (rounding collisions)
        if c not in cols:
            cols.append(c)
        c += 1
    return sorted(cols)


def build_table(group, C, seed=20261020, chain0=3):
    """uint64[11, C]: the int-seed table (chain c = Philox(key=[seed, chain0 + c])) with the group's planted entries written
    over spread-out columns.  Returns (table, {column: entry})."""
    words = np.zeros((11, C), dtype=np.uint64)
    words[0, :] = seed
    words[1, :] = np.arange(C, dtype=np.uint64) + np.uint64(chain0)
    words[10, :] = 4
    cols = planted_columns(C, len(group), shift=group[0]["D"] if group else 0)
    where = {}
    for col, e in zip(cols, group):
        words[:, col] = state_words(e)
        where[col] = e
    return words, where


def to_device(words, device):
    import torch

    return torch.from_numpy(np.array(words, dtype=np.uint64).view(np.int64)).to(device)  # (a copy: never a view of `words`)


def expected(entry, D):
    """(normals, final table column) numpy gives from the entry's state."""
    g = numpy_generator(entry)
    z = g.normal(size=D)
    st = g.bit_generator.state
    w = state_words(entry)
    w[2:6] = st["state"]["counter"]
    w[6:10] = st["buffer"]
    w[10] = st["buffer_pos"]
    return z, w


def groups_by_shape(kind="philox", only=None):
    """{(lpc, C, D): [entries]} in fixture order."""
    out = {}
    for e in entries(kind):
        if only is not None and not only(e):
            continue
        out.setdefault((e["lpc"], e["C"], e["D"]), []).append(e)
    return out


def assert_planted_equal_numpy(where, D, zt_or_none, out_dc, table_after, scale=1.0):
    """Planted chains against numpy: normals (chain-major zt[c, :D] and / or [D, C] layout) and the stream table."""
    for col, e in where.items():
        z, w = expected(e, D)
        if zt_or_none is not None:
            assert np.array_equal(zt_or_none[col, :D].view(np.uint64), z.view(np.uint64)), (e["name"], e["ww"], "normals")
        if out_dc is not None:
            want = 0.0 + scale * z
            assert np.array_equal(out_dc[:, col].view(np.uint64), want.view(np.uint64)), (e["name"], e["ww"], "momenta")
        assert np.array_equal(table_after[:, col], w), (e["name"], e["ww"], "stream table", table_after[:, col], w)
