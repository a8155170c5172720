"""bk_hist_accumulate (csrc/bk_hist.hip) and RunningHistogram at their seams; checks that take the kernel library as an
argument.  tests/test_hist_cpu.py runs them on the NumPy stand-in of tests/fake_ops_hist.py (and on its planted faults, one
broken seam each, to show that the checks notice); tests/test_gpu_hist.py on the HIP library.

The reference of the count checks is EXACT and has no tolerance: the counters are integers and the slot of a value is one
rule of two rounded fp64 operations (include/bkhip.h), which fake_ops_hist.slots_ref restates; the counts must be
np.array_equal to a per-row np.bincount of those slots.

What makes the check bite is the data around the bin edges: every interior edge lo + b / scale and the values up to 4 ulps
on either side of it.  On the non-dyadic grid below (B = 37) these 324 values per row hold several at which the form
x * scale - lo * scale picks another bin than the contract's (x - lo) * scale; 2 M uniform values hold none.  The module
asserts, when it is imported, that its data holds at least one such value for that grid."""
import functools
from collections import namedtuple

import numpy as np
import torch

from tests.fake_ops_hist import counts_ref, slots_ref, slots_two_product

NAN = float("nan")
GUARD = -7
PAD = 4                     # counts are a [D, B + 3] view of a [D + 1, B + 3 + PAD] tensor of guards: ldc = B + 7
PROBS = (0.001, 0.05, 0.25, 0.5, 0.75, 0.95, 0.999)

DYADIC_LO = np.array([0.0, -4.0, -1.0, -4.0, -2.0])            # hi = lo + 8: with B a power of two every edge is exact
NONDYADIC_LO = np.array([-0.3, -8.0, -1e-3, 5.0, -100.0])
NONDYADIC_HI = np.array([0.7001, 8.0, 1e-3, 5.5, 300.0])


def grid(kind, D, B):
    """(lo, hi, scale), [D] each; scale = B / (hi - lo) as RunningHistogram computes it."""
    if kind == "dyadic":
        assert B & (B - 1) == 0
        lo, hi = DYADIC_LO[:D].copy(), DYADIC_LO[:D] + 8.0
    else:
        lo, hi = NONDYADIC_LO[:D].copy(), NONDYADIC_HI[:D].copy()
    return lo, hi, float(B) / (hi - lo)


def edge_neighbourhood(lo, scale, B):
    """Every interior edge lo + b / scale (b = 1 .. B - 1) and the values up to 4 ulps below and above it: 9 (B - 1)."""
    e = lo + np.arange(1, B, dtype=np.float64) / scale
    out = [e]
    dn, up = e.copy(), e.copy()
    for _ in range(4):
        dn, up = np.nextafter(dn, -np.inf), np.nextafter(up, np.inf)
        out += [dn.copy(), up.copy()]
    return np.concatenate(out)


def specials(lo, hi):
    return np.array([np.inf, -np.inf, NAN, -0.0, 5e-324, 1e308, -1e308, lo, hi, np.nextafter(lo, -np.inf),
                     np.nextafter(hi, -np.inf)])


@functools.lru_cache(maxsize=64)
def data(kind, D, C, B):
    """x [D, C]: normal draws centred on the grid with sd = range / 16, with a random half (at most) of the positions of
    every row overwritten by the special values and the edge neighbourhoods of that row (all of them where they fit)."""
    lo, hi, scale = grid(kind, D, B)
    g = np.random.default_rng([D, C, B, 0 if kind == "dyadic" else 1])
    x = 0.5 * (lo + hi)[:, None] + (hi - lo)[:, None] / 16.0 * g.normal(size=(D, C))
    for d in range(D):
        pool = np.concatenate([specials(lo[d], hi[d]), edge_neighbourhood(lo[d], scale[d], B)])
        k = min(len(pool), max(C // 2, 1))
        take = pool if k == len(pool) else pool[g.choice(len(pool), size=k, replace=False)]
        x[d, g.choice(C, size=k, replace=False)] = take
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=8)
def equal_data(kind, D, C, B):
    """Rows in which ALL chains hold one value: inside a bin, x == lo, x == hi, NaN; the last row normal draws."""
    assert D == 5
    lo, hi, _ = grid(kind, D, B)
    x = np.empty((D, C))
    x[0], x[1], x[2], x[3] = lo[0] + 0.37 * (hi[0] - lo[0]), lo[1], hi[2], NAN
    x[4] = data(kind, D, C, B)[4]
    x.setflags(write=False)
    return x


def two_product_differs(kind, D, C, B):
    """How many values of data(...) the two-product formula puts into another slot than the contract does."""
    lo, _, scale = grid(kind, D, B)
    x = data(kind, D, C, B)
    return int(sum((slots_ref(x[d], lo[d], scale[d], B) != slots_two_product(x[d], lo[d], scale[d], B)).sum()
                   for d in range(D)))


# ---- the cases, each the smallest at which a thing can go wrong -----------------------------------------------------------------
Case = namedtuple("Case", "kind D C B pitch")        # pitch: ld - C (1 only with odd C: misaligned row starts)


def case_id(c):
    return f"{c.kind}-D{c.D}-C{c.C}-B{c.B}" + ("-ld+1" if c.pitch else "")


SEAM_C = 4099               # = 2 s + 3 for the slab s = 2,048 of the small shapes; odd


def _pitches(C):
    return (0, 1) if C % 2 else (0,)


BASE_CASES = [Case(kind, D, C, B, p) for kind, B in (("dyadic", 64), ("nondyadic", 37)) for D in (1, 5)
              for C in (1, 2, 63, 64, 65, SEAM_C) for p in _pitches(C)]
BIN_CASES = ([Case("nondyadic", 5, SEAM_C, B, 1) for B in (1, 2, 37, 64, 512)] +
             [Case("dyadic", 5, SEAM_C, B, 1) for B in (1, 2, 64, 512)])


def slab_cases(ops):
    """C in {s - 1, s, s + 1, 2 s + 3} around the slab s the library reports for these shapes."""
    out = []
    for kind, B in (("dyadic", 64), ("nondyadic", 37)):
        for D in (1, 5):
            s = ops.hist_slab_chains(SEAM_C, D, B)
            assert s >= 2 and SEAM_C == 2 * s + 3, (s, "the seam shapes assume a slab of 2,048 chains")
            for C in (s - 1, s, s + 1, 2 * s + 3):
                assert ops.hist_slab_chains(C, D, B) == s
                out += [Case(kind, D, C, B, p) for p in _pitches(C)]
    return out


def window_cases(ops):
    """B in {L - 1, L, L + 1} around the largest bin count L of the one-window path, and the largest B of all."""
    L = ops.hist_lds_bins()
    assert 2 <= L < 65536
    return [Case("nondyadic", 2, SEAM_C, B, 1) for B in (L - 1, L, L + 1, 65536) if B <= 65536] + [
        Case("dyadic", 2, SEAM_C, 65536, 1)]


def view(ops, x, pitch):
    """x as the first C columns of a [D, C + pitch] tensor with NaN in the pitch elements (a NaN that is counted shows)."""
    D, C = x.shape
    wide = torch.full((D, C + pitch), NAN, dtype=torch.float64, device=ops.device)
    wide[:, :C] = torch.from_numpy(np.array(x, dtype=np.float64)).to(ops.device)
    return wide[:, :C]


def _dev(ops, a):
    return torch.from_numpy(np.array(a)).to(ops.device)


class Counts:
    """[D, B + 3] int64 counters as a view of a [D + 1, B + 3 + PAD] tensor of guard values: the padding of every row and
    the row after the last must come back unchanged (the write contract)."""

    def __init__(self, ops, D, B, preset=None):
        self.big = torch.full((D + 1, B + 3 + PAD), GUARD, dtype=torch.int64, device=ops.device)
        self.counts = self.big[:D, :B + 3]
        self.counts.copy_(torch.zeros((D, B + 3), dtype=torch.int64) if preset is None else torch.from_numpy(preset))
        self.D, self.B = D, B

    def host(self):
        big = self.big.cpu().numpy()
        assert (big[self.D] == GUARD).all() and (big[:, self.B + 3:] == GUARD).all(), "the call wrote outside its slots"
        return big[:self.D, :self.B + 3].copy()


def _accumulate(ops, c, x, out):
    lo, _, scale = grid(c.kind, c.D, c.B)
    X = view(ops, x, c.pitch)
    if c.D > 1:
        assert X.stride(0) == c.C + c.pitch
    ops.hist_accumulate(X, _dev(ops, lo), _dev(ops, scale), c.B, out.counts)


def _assert_equal(got, want, c, what="counts"):
    bad = np.argwhere(got != want)
    assert not len(bad), (f"{what} differ from the NumPy restatement at {len(bad)} slots of {case_id(c)}, first "
                          f"{[(int(d), int(s), int(got[d, s]), int(want[d, s])) for d, s in bad[:6]]} (row, slot, got, want)")


# ---- (a) exact counts ------------------------------------------------------------------------------------------------------------
def check_exact(ops, c):
    """Zeroed counters, one call: array_equal with the restatement, every value counted once, the guards untouched."""
    lo, _, scale = grid(c.kind, c.D, c.B)
    x = data(c.kind, c.D, c.C, c.B)
    out = Counts(ops, c.D, c.B)
    _accumulate(ops, c, x, out)
    got = out.host()
    _assert_equal(got, counts_ref(x, lo, scale, c.B), c)
    assert (got.sum(axis=1) == c.C).all()


def check_edges_land_in_their_bins(ops):
    """Dyadic grid, B = 64: x == edge b lands in bin b, nextafter(edge b, -inf) in bin b - 1, x == hi in "above", x == lo
    and -0.0 (lo = 0) in bin 0 -- written out, not through the restatement.
    Row 0 has lo = 0: x - lo is exact for every x, so the value just below EVERY edge is in the bin below.  Row 1 has
    lo = -4: x - lo is exact for x == edge (multiples of 1/8) and for the values just below the edges in [-4, -2]; nearer to
    zero the ulp of x is finer than that of x - lo, the subtraction rounds back onto the edge, and the rule -- which is the
    contract -- puts such a value into the edge's own bin.  Those are left to the restatement (check_exact)."""
    B, D = 64, 2
    lo, hi, scale = grid("dyadic", D, B)
    assert lo[0] == 0.0 and lo[1] == -4.0
    C = 2 * (B + 1) + 1
    x = np.empty((D, C))
    for d in range(D):
        e = lo[d] + np.arange(B + 1) / scale[d]
        assert e[-1] == hi[d] and np.array_equal(e, lo[d] + np.arange(B + 1) * (8.0 / B))
        if d == 0:
            x[d] = np.concatenate([e, np.nextafter(e, -np.inf), [-0.0]])
        else:
            x[d] = np.concatenate([e, np.nextafter(e[:17], -np.inf), np.full(C - (B + 1) - 17, lo[d])])
    want = np.zeros((D, B + 3), dtype=np.int64)
    want[:, 1:B + 1] = 1          # edge b in bin b
    want[:, B + 1] = 1            # x == hi
    want[:, 0] = 1                # just below lo
    want[0, 1:B + 1] += 1         # row 0: the value just below edge b + 1 in bin b
    want[0, 1] += 1               #        and -0.0 in bin 0
    want[1, 1:17] += 1            # row 1: the same for the edges up to -2
    want[1, 1] += C - (B + 1) - 17  #      and x == lo, many times
    c = Case("dyadic", D, C, B, 1)
    out = Counts(ops, D, B)
    _accumulate(ops, c, x, out)
    _assert_equal(out.host(), want, c)


def check_all_equal_rows(ops, kind, B):
    c = Case(kind, 5, SEAM_C, B, 1)
    lo, _, scale = grid(kind, 5, B)
    x = equal_data(kind, 5, SEAM_C, B)
    out = Counts(ops, 5, B)
    _accumulate(ops, c, x, out)
    got = out.host()
    _assert_equal(got, counts_ref(x, lo, scale, B), c)
    assert got[1, 1] == SEAM_C and got[3, B + 2] == SEAM_C and (got[:4].max(axis=1) == SEAM_C).all()
    if kind == "dyadic":
        assert got[2, B + 1] == SEAM_C


# ---- (b) accumulation ------------------------------------------------------------------------------------------------------------
ACC_CHAINS = (65, 2049, SEAM_C)


def check_accumulation(ops, kind="nondyadic", B=37, D=5):
    """Three calls with different C == one restatement of the concatenation; counters preset to a pattern come out as the
    pattern plus the restatement (the call adds)."""
    lo, _, scale = grid(kind, D, B)
    xs = [data(kind, D, C, B) for C in ACC_CHAINS]
    want = counts_ref(np.concatenate(xs, axis=1), lo, scale, B)
    pattern = (np.arange(D * (B + 3), dtype=np.int64).reshape(D, B + 3) * 1_000_003) % 97 + (1 << 40)
    for preset in (None, pattern):
        out = Counts(ops, D, B, preset)
        for C, x in zip(ACC_CHAINS, xs):
            _accumulate(ops, Case(kind, D, C, B, 1), x, out)
        _assert_equal(out.host(), want if preset is None else want + pattern, Case(kind, D, sum(ACC_CHAINS), B, 1),
                      "accumulated counts")


# ---- (c) determinism -------------------------------------------------------------------------------------------------------------
def check_deterministic(ops, c):
    x = data(c.kind, c.D, c.C, c.B)
    got = []
    for _ in range(2):
        out = Counts(ops, c.D, c.B)
        _accumulate(ops, c, x, out)
        got.append(out.host())
    assert np.array_equal(got[0], got[1])


# ---- (d) quantiles of data -------------------------------------------------------------------------------------------------------
def finite_data(D, C, seed):
    """Normal draws centred on the non-dyadic grid with sd = range / 16 (the grid is -/+ 8 sd: nothing falls off it)."""
    lo, hi, _ = grid("nondyadic", D, 37)
    g = np.random.default_rng([D, C, seed])
    return 0.5 * (lo + hi)[:, None] + (hi - lo)[:, None] / 16.0 * g.normal(size=(D, C))


def check_quantile_bound(ops, bk):
    """|quantile(p) - x_(k)| <= (1 + 1e-9) / scale against np.quantile(.., method="inverted_cdf") of everything fed: both
    values lie in the same bin, which is 1 / scale wide; the 1e-9 covers the rounding of the edge arithmetic.  Returns the
    largest error in bin widths."""
    D, B = 5, 37
    lo, hi, scale = grid("nondyadic", D, B)
    h = bk.RunningHistogram(lo, hi, bins=B, ops=ops)
    xs = [finite_data(D, C, 7) for C in (SEAM_C, 65, 2049)]
    for x in xs:
        h.update(_dev(ops, x), layout="dc")
    pooled = np.concatenate(xs, axis=1)
    assert h.n == pooled.shape[1] and (h.coverage() == 1.0).all()
    q = h.quantile(PROBS)
    worst = 0.0
    for i, p in enumerate(PROBS):
        want = np.quantile(pooled, p, axis=1, method="inverted_cdf")
        err = np.abs(q[i] - want) * scale
        print(f"p={p}: largest |quantile - x_(k)| = {err.max():.4f} bin widths")
        worst = max(worst, float(err.max()))
        assert (np.abs(q[i] - want) <= (1.0 + 1e-9) / scale).all(), (p, q[i], want)
    assert np.array_equal(h.median(), q[PROBS.index(0.5)])
    lower, upper = h.interval(0.9)
    assert np.array_equal(lower, q[PROBS.index(0.05)]) and np.array_equal(upper, q[PROBS.index(0.95)])
    return worst


def check_running_histogram_counts(ops, bk):
    """RunningHistogram.update through every input form == the restatement: (C, D) views, [D, C] buffers, a padded state."""
    D, B = 5, 37
    lo, hi, scale = grid("nondyadic", D, B)
    h = bk.RunningHistogram(lo, hi, bins=B, ops=ops)
    assert np.array_equal(h.scale.cpu().numpy(), scale)
    xs = [data("nondyadic", D, C, B) for C in ACC_CHAINS]
    h.update(_dev(ops, xs[0]))                                   # [D, C]
    h.update(_dev(ops, xs[1]).t())                               # sample()'s (C, D) view of a [D, C] buffer
    h.update(view(ops, xs[2], 1))                                # a state with a row pitch of its own
    want = counts_ref(np.concatenate(xs, axis=1), lo, scale, B)
    got = h.counts().cpu().numpy()
    _assert_equal(got, want, Case("nondyadic", D, sum(ACC_CHAINS), B, 0), "RunningHistogram.counts()")
    assert h.n == sum(ACC_CHAINS) and tuple(got.shape) == (D, B + 3)


# ---- module check: the data bites ------------------------------------------------------------------------------------------------
for _D in (1, 5):
    assert two_product_differs("nondyadic", _D, SEAM_C, 37) >= 1, "no value tells the two-product formula from the contract"
