"""FakeOps with the fixed-grid histogram of RunningHistogram (include/bkhip.h: bk_hist_accumulate), restated in NumPy --
TEST INFRASTRUCTURE ONLY.

slots_ref is the contract's rule and counts_ref the restatement every exact check compares with: a per-row np.bincount of
the slots.  HistFakeOps.hist_accumulate walks the launch as the kernel does -- row by row, slab by slab, a head element
where the slab does not start on 16 bytes, pairs, a tail element, a flush of the slab's private counters that are not zero --
so that one seam at a time can be broken (``fault``) to show that the checks of tests/hist_parity.py notice."""
import numpy as np
import torch

from tests.fake_ops import FakeOps

LDS_BINS = 8189          # bk_hist_lds_bins(): 8,192 counters of one LDS window less the three extra slots
UNIT = 2048              # chains: 256 threads x four 16-byte loads
MIN_WORKGROUPS = 2048
MAX_SLAB = 1 << 30
MAX_BINS = 65536


def cdiv(a, b):
    return -(-a // b)


def slab_chains(C, D, B):
    """bk_hist_slab_chains."""
    if C < 1 or D < 1 or B < 1 or B > MAX_BINS:
        return 0
    slab = cdiv(cdiv(C, cdiv(MIN_WORKGROUPS, D)), UNIT) * UNIT
    floor_ = cdiv(2 * min(B + 3, LDS_BINS + 3), UNIT) * UNIT
    return min(max(slab, floor_), MAX_SLAB)


def slots_ref(x, lo, scale, B):
    """The slot of every x (any shape; lo and scale broadcast): the rule of include/bkhip.h in float64, one rounded
    subtraction and one rounded multiplication."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        t = (x - lo) * scale
    slot = np.empty(t.shape, dtype=np.int64)
    nan = np.isnan(x)
    below = ~nan & (t < 0.0)
    above = ~nan & (t >= float(B))
    mid = ~(nan | below | above)
    slot[nan] = B + 2
    slot[below] = 0
    slot[above] = B + 1
    slot[mid] = 1 + t[mid].astype(np.int64)
    return slot


def slots_two_product(x, lo, scale, B):
    """NOT the contract: t = x * scale - lo * scale (the form a compiler or a hurried author would write)."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        t = x * scale - lo * scale
    slot = np.where(np.isnan(x), B + 2, np.where(t < 0.0, 0, np.where(t >= float(B), B + 1, 0))).astype(np.int64)
    mid = ~np.isnan(x) & ~(t < 0.0) & ~(t >= float(B))
    slot[mid] = 1 + t[mid].astype(np.int64)
    return slot


def counts_ref(x, lo, scale, B):
    """[D, B + 3] int64: the counts of x [D, C] on the grid (lo [D], scale [D])."""
    x = np.asarray(x, dtype=np.float64)
    out = np.zeros((x.shape[0], B + 3), dtype=np.int64)
    for d in range(x.shape[0]):
        out[d] = np.bincount(slots_ref(x[d], lo[d], scale[d], B), minlength=B + 3)
    return out


FAULTS = ("two_product", "x_edges", "below_le", "above_gt", "nan_below", "odd_tail", "pitch", "slab_seam", "flush_zero")


class HistFakeOps(FakeOps):
    """fault: None, or one of FAULTS -- one seam broken:
      two_product  t = x * scale - lo * scale
      x_edges      the bin is found by comparing x with the edges lo + b / scale
      below_le     t <= 0 is "below" (x == lo and t == -0.0 leave bin 0)
      above_gt     only t > B is "above": the range is closed, t == B (x == hi on a dyadic grid) is counted in the last bin.
                   (With an unclamped 1 + (int64)t a literal `t > B` would still land in slot B + 1; the fault is planted
                   in the form in which a kernel can get it wrong, a bin index clamped to B - 1.)
      nan_below    NaN is counted as "below"
      odd_tail     the element after the last whole pair of a slab is dropped
      pitch        a row is ld elements long, not C
      slab_seam    every slab but the first starts one chain early
      flush_zero   the flush STORES the sum for every counter of the slab, and 0 where the slab's counter is zero"""
    name = "fake-cpu-hist"

    def __init__(self, fault=None):
        super().__init__()
        assert fault is None or fault in FAULTS
        self.fault = fault

    @staticmethod
    def hist_lds_bins():
        return LDS_BINS

    @staticmethod
    def hist_slab_chains(C, D, B):
        return slab_chains(int(C), int(D), int(B))

    def _slots(self, x, lo, scale, B):
        f = self.fault
        if f == "two_product":
            return slots_two_product(x, lo, scale, B)
        if f == "x_edges":
            edges = lo + np.arange(B + 1, dtype=np.float64) / scale
            s = np.searchsorted(edges, x, side="right").astype(np.int64)  # 0 below edge 0 .. B + 1 from edge B on
            return np.where(np.isnan(x), B + 2, s)
        s = slots_ref(x, lo, scale, B)
        with np.errstate(over="ignore", invalid="ignore"):
            t = (x - lo) * scale
        if f == "below_le":
            s = np.where(~np.isnan(x) & (t <= 0.0), 0, s)
        elif f == "above_gt":
            s = np.where(~np.isnan(x) & (t == float(B)), B, s)
        elif f == "nan_below":
            s = np.where(np.isnan(x), 0, s)
        return s

    def hist_accumulate(self, theta, lo, scale, B, counts):
        self._count("hist_accumulate")
        B = int(B)
        D, C = theta.shape
        if B < 1 or B > MAX_BINS or counts.shape[1] < B + 3 or counts.shape[0] != D:
            raise ValueError("bk_hist_accumulate: BK_E_ARG")
        assert counts.dtype == torch.int64 and theta.dtype == torch.float64
        assert C <= 1 or theta.stride(1) == 1
        if C == 0 or D == 0:
            return
        ld = theta.stride(0) if D > 1 else C
        lo_h, sc_h = lo.numpy(), scale.numpy()
        out = counts.numpy()  # (a view: the row pitch of `counts` is respected, only [:, :B + 3] is touched)
        rows = theta.numpy()
        if self.fault == "pitch" and ld > C and D > 1:  # rows d < D - 1 run on into their pitch elements
            wide = torch.as_strided(theta, (D - 1, ld), (ld, 1)).numpy()
        else:
            wide = None
        slab = slab_chains(C, D, B)
        first = theta.data_ptr() // 8
        for d in range(D):
            row = rows[d] if wide is None or d == D - 1 else wide[d]
            n_row = row.shape[0]
            for c0 in range(0, n_row, slab):
                a = c0 - 1 if (self.fault == "slab_seam" and c0 > 0) else c0
                n = min(c0 + slab, n_row) - a
                head = (first + d * ld + a) & 1
                n2 = (n - head) // 2
                tail = n - head - 2 * n2
                if self.fault == "odd_tail" and tail:
                    n -= 1
                h = np.bincount(self._slots(row[a:a + n], lo_h[d], sc_h[d], B), minlength=B + 3)[:B + 3]
                if self.fault == "flush_zero":
                    out[d, :B + 3] = np.where(h != 0, out[d, :B + 3] + h, 0)
                else:
                    nz = h != 0
                    out[d, :B + 3][nz] += h[nz]
