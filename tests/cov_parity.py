"""bk_cov_accumulate (csrc/bk_cov.hip) at the seams of its tile decode, its slab split and its finish kernel; checks that take
the kernel library as an argument.  tests/test_cov_kernels_cpu.py runs them on PlanFollowingCov below (NumPy, walking the
same plan, with one seam broken at a time to show that the checks notice); tests/test_gpu_cov_kernels.py on the HIP library.

The reference of the seam checks is EXACT: for integer-valued X (entries in +-{1..15}) and an integer centre in [-16, 16]
every product and every partial sum of Xc Xc^T and rowsum(Xc) is an integer far below 2^53, so every summation order -- the
MFMA's, the slabs', the host BLAS's -- gives the same double, and the kernel must equal `xc @ xc.T` bit for bit.  No entry of
X is zero, so a dropped or doubled chain changes every diagonal entry.  Figures: profiles/cov_edges.md."""
import functools
from collections import namedtuple

import numpy as np
import torch

from tests import dense_adapt_parity as dp
from tests.test_gpu_dense_adapt import _reference  # the long-double reference and its bound, as that file holds it

BM, BK, XCDS = 128, 16, 8
TILE_ELEMS = BM * BM
NAN = float("nan")


def cdiv(a, b):
    return -(-a // b)


# ---- the plan, restated ------------------------------------------------------------------------------------------------------
def k_chunk(D):
    """cov_k_chunk: max(128, 4 tiles rounded up to 16), capped by what keeps D x k_chunk doubles within 2 MiB."""
    nb = cdiv(D, BM)
    tiles = nb * (nb + 1) // 2
    k = max(cdiv(4 * tiles, BK) * BK, 128)
    fit = max(((2 << 20) // (8 * D)) // BK * BK, BK)
    return min(k, fit)


Plan = namedtuple("Plan", "nb tiles k fit k_chunk per slab_chains slabs last rounds grid slab_elems work_elems col_blocks "
                          "whole k_steps_last")


def plan(D, C):
    """cov_plan and the launch geometry of bk_cov_accumulate for X[D, C].  `whole`: D and C are whole tiles and K-steps (the
    unchecked kernel then still needs a 16-byte-aligned base and an even pitch: whole_tile_view)."""
    nb = cdiv(D, BM)
    tiles = nb * (nb + 1) // 2
    k = max(cdiv(4 * tiles, BK) * BK, 128)
    fit = max(((2 << 20) // (8 * D)) // BK * BK, BK)
    kc = min(k, fit)
    assert kc == k_chunk(D)
    chunks = cdiv(C, kc)
    max_slabs = max(1024 // tiles, XCDS)
    per = cdiv(chunks, max_slabs)
    slab_chains = per * kc
    slabs = cdiv(C, slab_chains)
    last = C - (slabs - 1) * slab_chains
    slab_elems = tiles * TILE_ELEMS + nb * BM
    return Plan(nb=nb, tiles=tiles, k=k, fit=fit, k_chunk=kc, per=per, slab_chains=slab_chains, slabs=slabs, last=last,
                rounds=cdiv(slabs, XCDS), grid=cdiv(slabs, XCDS) * XCDS * tiles, slab_elems=slab_elems,
                work_elems=slabs * slab_elems, col_blocks=cdiv(D, 256), whole=(D % BM == 0 and C % BK == 0),
                k_steps_last=cdiv(last, BK))


def decode(tile):
    """tile -> (row block, column block <= row block), as k_cov_accumulate's loop."""
    rb = 0
    while (rb + 1) * (rb + 2) // 2 <= tile:
        rb += 1
    return rb, tile - rb * (rb + 1) // 2


def whole_tile_view(X):
    """Whether bk_cov_accumulate takes the unchecked kernel for this view."""
    D, C = X.shape
    ld = X.stride(0) if D > 1 else C
    return plan(D, C).whole and ld % 2 == 0 and X.data_ptr() % 16 == 0


# ---- the shapes, each named for a seam -------------------------------------------------------------------------------------------
CHECKED, WHOLE = "checked", "whole-tile"
Shape = namedtuple("Shape", "D C kernel seam expect")
SHAPES = [
    Shape(257, 37, CHECKED, "third row block: tile blocks (2,0) (2,1) (2,2); finish with a second column block of one column",
          dict(nb=3, tiles=6, slabs=1, col_blocks=2, k_chunk=128)),
    Shape(300, 300, CHECKED, "third row block with three slabs, the last of 44 chains; the real-data bound",
          dict(nb=3, tiles=6, slabs=3, last=44, per=1)),
    Shape(5, 1025, CHECKED, "second placement round on one tile block: nine slabs, the last of one chain, seven surplus workgroups",
          dict(tiles=1, slabs=9, last=1, grid=16, rounds=2)),
    Shape(130, 1025, CHECKED, "second placement round on three tile blocks: slot / tiles and slot % tiles",
          dict(tiles=3, slabs=9, last=1, grid=48, rounds=2)),
    Shape(130, 2049, CHECKED, "third placement round", dict(tiles=3, slabs=17, rounds=3, last=1)),
    Shape(1921, 1025, CHECKED, "fit decides k_chunk (k = 544 > fit = 128); slabs of two chunks; finish with 8 column blocks",
          dict(nb=16, tiles=136, k=544, fit=128, k_chunk=128, per=2, slab_chains=256, slabs=5, last=1, col_blocks=8)),
    Shape(2049, 225, CHECKED, "k_chunk = 112, no power of two; 17 row blocks",
          dict(nb=17, tiles=153, k_chunk=112, per=1, slabs=3, last=1, col_blocks=9)),
    Shape(256, 32, WHOLE, "the unchecked off-diagonal instantiation; two K-steps",
          dict(nb=2, tiles=3, slabs=1, k_steps_last=2)),
    Shape(384, 16, WHOLE, "unchecked, third row block, one K-step (no second panel)",
          dict(nb=3, tiles=6, slabs=1, k_steps_last=1)),
    Shape(384, 48, WHOLE, "unchecked, three K-steps: both LDS buffers reused", dict(nb=3, slabs=1, k_steps_last=3)),
    Shape(128, 1040, WHOLE, "unchecked, second placement round, last slab of 16 chains = one K-step",
          dict(tiles=1, slabs=9, last=16, k_steps_last=1, rounds=2)),
    Shape(256, 512, WHOLE, "unchecked, four whole slabs; the identity shape of whole-tile == checked",
          dict(tiles=3, slabs=4, last=128, per=1)),
    Shape(2176, 1024, WHOLE, "unchecked, k_chunk = 112, slabs of two chunks, last slab of 128 chains",
          dict(nb=17, k_chunk=112, per=2, slab_chains=224, slabs=5, last=128, col_blocks=9)),
    # found while restating the plan: four times the tile count passes 128 from D = 897 on, below the L2 cap
    Shape(897, 145, CHECKED, "k_chunk = 144 from the tile count (128 < k < fit); two slabs, the last of one chain",
          dict(nb=8, tiles=36, k=144, fit=288, k_chunk=144, per=1, slabs=2, last=1, col_blocks=4)),
]
SHAPE_IDS = [f"{s.D}x{s.C}" for s in SHAPES]
WHOLE_SHAPES = [s for s in SHAPES if s.kernel == WHOLE]
BOUND_SHAPES = [s for s in SHAPES if s.D * s.D * s.C <= 4e7]  # the long-double host reference stays well under a second


def shape(D, C):
    return next(s for s in SHAPES if (s.D, s.C) == (D, C))


def assert_shape_hits_its_seam(sh):
    """The plan values a shape is listed for, and the kernel it is listed under; a changed plan fails here, loudly, instead
    of moving the shape off its seam."""
    p = plan(sh.D, sh.C)
    for key, want in sh.expect.items():
        assert getattr(p, key) == want, (sh.D, sh.C, key, getattr(p, key), want)
    assert p.whole == (sh.kernel == WHOLE), (sh.D, sh.C)
    assert p.slab_chains == p.per * p.k_chunk and (p.slabs - 1) * p.slab_chains < sh.C <= p.slabs * p.slab_chains
    assert p.work_elems * 8 <= 100 << 20  # the scratch of a test shape stays below 100 MiB
    if "third row block" in sh.seam:
        assert p.tiles >= 6 and [decode(t) for t in (3, 4, 5)] == [(2, 0), (2, 1), (2, 2)]
    if "placement round" in sh.seam:
        assert p.slabs >= 9 and p.rounds >= 2
    if "fit decides" in sh.seam:
        assert p.k > p.fit
    if "two chunks" in sh.seam:
        assert p.per == 2
    if "k_chunk = 1" in sh.seam:  # (112 from the cap, 144 from the tile count: neither 128 nor a power of two)
        assert p.k_chunk & (p.k_chunk - 1) and p.k_chunk == (p.fit if p.k > p.fit else p.k)
    if "off-diagonal instantiation" in sh.seam:
        assert p.whole and p.nb >= 2


# ---- data ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def integer_data(D, C):
    """(x, centre): x in +-{1..15}, never zero; centre integer in [-16, 16].  Both float64."""
    g = np.random.default_rng([D, C, 1])
    x = g.integers(1, 16, size=(D, C)).astype(np.float64) * g.choice([-1.0, 1.0], size=(D, C))
    c = g.integers(-16, 17, size=D).astype(np.float64)
    return x, c


def exact_product(x, c):
    """Xc Xc^T and rowsum(Xc) in float64 on the host, exact; the magnitude condition asserted."""
    xc = x if c is None else x - c[:, None]
    assert np.array_equal(xc, np.rint(xc)) and np.isfinite(xc).all()
    m = float(np.abs(xc).max())
    assert 2.0 * x.shape[1] * m * m < 2.0 ** 53  # (twice: the `+=` check doubles the sums)
    return xc @ xc.T, xc.sum(axis=1)


@functools.lru_cache(maxsize=2)
def real_data(D, C):
    """The generator of tests/test_gpu_dense_adapt.py, centred variant: scales logspace(0, 1, D), a centre of order 1e3
    under data of order 1e3."""
    g = np.random.default_rng([D, C, 2])
    x = g.normal(size=(D, C)) * np.logspace(0, 1, D)[:, None]
    c = 1e3 * (1.0 + g.random(D))
    return x + c[:, None] + 0.1 * g.normal(size=(D, 1)), c


def view(ops, x, off, pad):
    """x as a column slice [off, off + C) of a [D, C + pad] tensor with NaN outside the slice."""
    D, C = x.shape
    wide = torch.full((D, C + pad), NAN, dtype=torch.float64, device=ops.device)
    wide[:, off:off + C] = torch.from_numpy(x).to(ops.device)
    return wide[:, off:off + C]


def listed_view(ops, x, sh):
    """Checked rows: offset 3, pad 7 (an 8-byte-aligned base).  Whole-tile rows: offset 4, pad 8 (16-byte-aligned, an
    even pitch)."""
    X = view(ops, x, 4, 8) if sh.kernel == WHOLE else view(ops, x, 3, 7)
    assert whole_tile_view(X) == (sh.kernel == WHOLE)
    return X


def _np(t):
    return np.asarray(t.cpu())


GUARD = 1024


class Outputs:
    """Zeroed S (a [D, D] slice of a [D, D + 3] tensor), zeroed s, and the scratch: ops.cov_work's size exactly, pre-filled
    with NaN (whatever the finish kernel reads, the call must have written), GUARD sentinel doubles behind it."""

    def __init__(self, ops, D, C):
        dev = ops.device
        self.Sbig = torch.zeros((D, D + 3), dtype=torch.float64, device=dev)
        self.S = self.Sbig[:, :D]
        self.s = torch.zeros(D, dtype=torch.float64, device=dev)
        n = ops.cov_work(D, C).numel()
        assert n == plan(D, C).work_elems
        self.buf = torch.full((n + GUARD,), -7.0, dtype=torch.float64, device=dev)
        self.work = self.buf[:n]
        self.ops = ops

    def call(self, X, ct):
        self.work.fill_(NAN)
        self.ops.cov_accumulate(X, ct, self.S, self.s, self.work)
        return self

    def host(self):
        assert (_np(self.buf[self.work.numel():]) == -7.0).all() and not _np(self.Sbig[:, self.S.shape[1]:]).any()
        return _np(self.S).copy(), _np(self.s).copy()


def _dev(ops, c):
    return None if c is None else torch.from_numpy(c).to(ops.device)


# ---- (a) exact -----------------------------------------------------------------------------------------------------------------
def check_exact(ops, sh):
    """Integer data, with and without a centre, into zeroed outputs: S and s array_equal with the host product, S exactly
    symmetric.  Then NaN in S's strict upper triangle and the same call again: exactly twice the product, in both triangles
    (`+=` reads the lower triangle only and rewrites both)."""
    D, C = sh.D, sh.C
    x, centre = integer_data(D, C)
    X = listed_view(ops, x, sh)
    upper = torch.ones((D, D), dtype=torch.bool, device=ops.device).triu(1)
    for c in (None, centre):
        want_S, want_s = exact_product(x, c)
        out = Outputs(ops, D, C)
        S1, s1 = out.call(X, _dev(ops, c)).host()
        bad = np.argwhere(S1 != want_S)
        assert not len(bad), f"S differs from the exact product at {len(bad)} entries of {(D, C)}, first {bad[:6].tolist()}"
        bad = np.flatnonzero(s1 != want_s)
        assert not len(bad), f"s differs from the exact row sums at {len(bad)} entries of {(D, C)}, first {bad[:6].tolist()}"
        assert np.array_equal(S1, S1.T)
        out.S.masked_fill_(upper, NAN)
        S2, s2 = out.call(X, _dev(ops, c)).host()
        assert np.array_equal(S2, 2.0 * want_S) and np.array_equal(s2, 2.0 * want_s)


# ---- (b) real data is deterministic ----------------------------------------------------------------------------------------------
def check_deterministic(ops, sh):
    x, c = real_data(sh.D, sh.C)
    X = listed_view(ops, x, sh)
    a = Outputs(ops, sh.D, sh.C).call(X, _dev(ops, c)).host()
    b = Outputs(ops, sh.D, sh.C).call(X, _dev(ops, c)).host()
    assert np.isfinite(a[0]).all() and np.isfinite(a[1]).all()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- (c) whole-tile == checked ---------------------------------------------------------------------------------------------------
def check_whole_tile_equals_checked(ops, sh):
    """Real data through the aligned view (the unchecked kernel), a view at offset 3 of the same even pitch (base not
    16-byte aligned) and a view of odd pitch: the plan is a function of (D, C) only and the masks are no-ops on whole tiles,
    so S and s are array_equal."""
    assert sh.kernel == WHOLE
    x, c = real_data(sh.D, sh.C)
    views = [view(ops, x, 4, 8), view(ops, x, 3, 8), view(ops, x, 4, 7)]
    assert [whole_tile_view(v) for v in views] == [True, False, False]
    assert views[1].stride(0) == views[0].stride(0) and views[2].stride(0) % 2 == 1
    outs = [Outputs(ops, sh.D, sh.C).call(v, _dev(ops, c)).host() for v in views]
    for S, s in outs[1:]:
        assert np.array_equal(S, outs[0][0]) and np.array_equal(s, outs[0][1])


# ---- (d) the long-double bound ---------------------------------------------------------------------------------------------------
def check_long_double_bound(ops, sh):
    """Real data, centred and not, one call: |S - S_ld| <= 4 C u |Xc| |Xc|^T, |s - s_ld| <= 4 C u rowsum |Xc|
    (tests/test_gpu_dense_adapt.py's reference and bound).  Returns the two largest err / bound."""
    assert sh.D * sh.D * sh.C <= 4e7
    x, centre = real_data(sh.D, sh.C)
    rS = rs = 0.0
    for c in (None, centre):
        want_S, want_s, tol_S, tol_s = _reference(x, c)
        S, s = Outputs(ops, sh.D, sh.C).call(listed_view(ops, x, sh), _dev(ops, c)).host()
        errS = np.abs(S.astype(np.longdouble) - want_S)
        errs = np.abs(s.astype(np.longdouble) - want_s)
        rS, rs = max(rS, float((errS / tol_S).max())), max(rs, float((errs / tol_s).max()))
        print(f"D={sh.D} C={sh.C} centred={c is not None}: max err/bound S {float((errS / tol_S).max()):.4f}  s "
              f"{float((errs / tol_s).max()):.4f}")
        assert (errS <= tol_S).all() and (errs <= tol_s).all()
        assert np.array_equal(S, S.T) and (np.diag(S) >= 0.0).all()
    return rS, rs


# ---- (e) non-finite values -------------------------------------------------------------------------------------------------------
NAN_SHAPE = (130, 1025)
NAN_PLACES = [(129, 1024), (0, 127)]  # the lone chain of the last slab, in the second row block; the first slab's last chain


def check_nan_poisons_one_row_and_column(ops):
    D, C = NAN_SHAPE
    sh = shape(D, C)
    p = plan(D, C)
    assert p.slabs == 9 and p.last == 1 and p.slab_chains == 128 and p.nb == 2
    x, c = integer_data(D, C)
    want_S, want_s = exact_product(x, c)
    for r, k in NAN_PLACES:
        y = x.copy()
        y[r, k] = NAN
        S, s = Outputs(ops, D, C).call(listed_view(ops, y, sh), _dev(ops, c)).host()
        assert np.isnan(S[r, :]).all() and np.isnan(S[:, r]).all() and np.isnan(s[r])
        keep = np.arange(D) != r
        assert np.array_equal(S[np.ix_(keep, keep)], want_S[np.ix_(keep, keep)]) and np.array_equal(s[keep], want_s[keep])


# ---- (f) RunningCovariance across tile blocks ----------------------------------------------------------------------------------------
def check_running_covariance_across_tile_blocks(ops):
    """dense_adapt_parity's check (bar 1e-11 through assert_cov_close) at 12 draws of (257, 130): three row blocks, two
    slabs."""
    p = plan(257, 130)
    assert p.nb == 3 and p.slabs == 2
    dp.check_running_covariance(ops, 12, 257, 130)


# ---- a stand-in that follows the plan ----------------------------------------------------------------------------------------------------
FAULTS = {
    # fault -> the shape named for the seam it breaks
    "tile_decode": (257, 37),
    "slab_round": (130, 1025),
    "last_chain": (5, 1025),
    "per": (1921, 1025),
    "finish_cols": (257, 37),
    "row_sums": (130, 1025),
}


class PlanFollowingCov:
    """cov_k_chunk, cov_work and cov_accumulate in NumPy -- TEST INFRASTRUCTURE ONLY.  Walks the launch grid of
    k_cov_accumulate workgroup by workgroup (placement, tile decode, slab range; one product per tile block, written to the
    slab's scratch where the kernel writes it, the idle quadrant of a diagonal block left alone) and finishes as k_cov_finish
    does (column blocks of 256, slabs added in increasing order, the lower triangle read and both written).  The order of
    the sums INSIDE a tile block is BLAS's, not the MFMA's: on real data this is a stand-in, on integer data it is exact.

    fault: None, or one of FAULTS -- one seam broken:
      tile_decode  tile blocks from the fourth on are computed for the column block mirrored within their row block
      slab_round   the placement forgets the round: slabs 8.. are never computed (their scratch holds zeros)
      last_chain   a slab that is not full loses its last chain
      per          slab_chains = k_chunk whatever `per` is
      finish_cols  the finish stops at column 256
      row_sums     the row sums of row blocks >= 1 are those of block 0"""
    name = "plan-following-cov"

    def __init__(self, fault=None):
        assert fault is None or fault in FAULTS
        self.fault = fault
        self.device = torch.device("cpu")
        self.calls = {}

    @staticmethod
    def cov_k_chunk(D):
        return k_chunk(D)

    def cov_work(self, D, C):
        return torch.empty(plan(D, C).work_elems, dtype=torch.float64)

    def cov_accumulate(self, X, center, S, s, work):
        self.calls["cov_accumulate"] = self.calls.get("cov_accumulate", 0) + 1
        D, C = X.shape
        assert S.shape == (D, D) and s.numel() == D
        if C == 0 or D == 0:
            return
        p = plan(D, C)
        assert work.numel() >= p.work_elems
        w = work.numpy()
        if self.fault == "slab_round":
            w[:p.work_elems] = 0.0
        slab_chains = p.k_chunk if self.fault == "per" else p.slab_chains
        xc = np.zeros((p.nb * BM, C))          # rows past D: zeros after centring
        xc[:D] = X.numpy() if center is None else X.numpy() - center.numpy()[:, None]
        for wg in range(p.grid):
            xcd, slot = wg % XCDS, wg // XCDS
            slab = xcd if self.fault == "slab_round" else (slot // p.tiles) * XCDS + xcd
            tile = slot % p.tiles
            if slab >= p.slabs:
                continue
            rb, cb = decode(tile)
            if self.fault == "tile_decode" and tile >= 3:
                cb = rb - cb
            k_lo = slab * slab_chains
            k_hi = min(k_lo + slab_chains, C)
            if self.fault == "last_chain" and k_hi - k_lo < slab_chains:
                k_hi -= 1
            out = w[slab * p.slab_elems:(slab + 1) * p.slab_elems]
            a = np.ascontiguousarray(xc[rb * BM:(rb + 1) * BM, k_lo:k_hi])
            b = a if rb == cb else np.ascontiguousarray(xc[cb * BM:(cb + 1) * BM, k_lo:k_hi])
            tp = out[tile * TILE_ELEMS:(tile + 1) * TILE_ELEMS].reshape(BM, BM)
            g = a @ b.T
            if rb == cb:
                tp[:64, :64], tp[64:, :] = g[:64, :64], g[64:, :]
                src = xc[:BM, k_lo:k_hi] if self.fault == "row_sums" else a
                out[p.tiles * TILE_ELEMS + rb * BM:p.tiles * TILE_ELEMS + (rb + 1) * BM] = src.sum(axis=1)
            else:
                tp[...] = g
        Sn, sn = S.numpy(), s.numpy()
        i = np.arange(D)[:, None]
        for cblk in range(1 if self.fault == "finish_cols" else p.col_blocks):
            j = cblk * 256 + np.arange(256)[None, :]
            ii, jj = np.nonzero((j <= i) & (i < D))
            jj = jj + cblk * 256
            rbi, cbi = ii // BM, jj // BM
            off = (rbi * (rbi + 1) // 2 + cbi) * TILE_ELEMS + (ii % BM) * BM + (jj % BM)
            acc = w[off]
            for q in range(1, p.slabs):
                acc = acc + w[q * p.slab_elems + off]
            v = Sn[ii, jj] + acc
            Sn[ii, jj] = v
            Sn[jj, ii] = v
        so = p.tiles * TILE_ELEMS + np.arange(D)
        acc = w[so]
        for q in range(1, p.slabs):
            acc = acc + w[q * p.slab_elems + so]
        sn[...] = sn + acc
