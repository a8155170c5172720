"""FakeOps with ordered resampling (include/bkhip.h: bk_resample_ordered), restated in NumPy -- TEST INFRASTRUCTURE ONLY.

The restatement knows nothing of the kernels' tiling: the cumulative weight is a sum of int64, which every order of
summation gives the same bits, and every slot position is an exact integer.

    wmax = max_i w_i,  s = 62 - bit_length(n - 1),  q_i = rint(ldexp(w_i / wmax, s))      (a weight that is not > 0: q_i = 0)
    Q_i  = cumsum(q)_i (int64),  Q = Q_{n-1},  a = Q // m,  r = Q % m
    tau_J = J * a + (J * r) // m + min(a - 1, floor(u * float(a))),   idx_J = searchsorted(Q, tau_J, side="right")
"""
import numpy as np

from tests.fake_ops import FakeOps

SYSTEMATIC, STRATIFIED = 0, 1
TILE = 2048      # RO_TILE of csrc/bk_resample.hip: elements per workgroup of the tile-sum and tile-scan launches
CARRY_W = 256    # RO_CARRY_W: tile sums per pass of the carry launch's loop
Q_OFFSET = 16    # Q starts at this byte of the work area


def shift(n):
    return 62 - (int(n) - 1).bit_length()


def work_bytes(n):
    """bk_resample_ordered_work_bytes."""
    if n <= 0:
        return 0
    if n > 2 ** 31 - 1:
        return -1
    return 16 + 8 * ((n + 1) & ~1) + 8 * (-(-n // TILE))


def quantise(w):
    """[n] float64 -> q [n] int64."""
    w = np.asarray(w, dtype=np.float64)
    wp = np.where(w > 0.0, w, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = wp / wp.max()
        pos = r > 0.0
        return np.where(pos, np.rint(np.ldexp(np.where(pos, r, 0.0), shift(len(w)))), 0.0).astype(np.int64)


def cumulative(w):
    return np.cumsum(quantise(w), dtype=np.int64)


def thresholds(Q_total, u, mode, m_local, slot0, m_total):
    """tau_J of the slots J = slot0 .. slot0 + m_local - 1 as int64."""
    a, r = int(Q_total) // int(m_total), int(Q_total) % int(m_total)
    J = np.arange(slot0, slot0 + m_local, dtype=np.int64)
    uj = np.asarray(u, dtype=np.float64).reshape(-1)[:1 if mode == SYSTEMATIC else m_local]   # (systematic: one, broadcast)
    o = np.minimum(np.int64(a - 1), np.floor(uj * float(a)).astype(np.int64))
    return J * np.int64(a) + (J * np.int64(r)) // np.int64(m_total) + o


def resample_ordered_ref(w, u, mode, m_local, slot0, m_total):
    """-> (idx [m_local] int32, Q [n] int64)."""
    Q = cumulative(w)
    tau = thresholds(Q[-1], u, mode, m_local, slot0, m_total)
    idx = np.searchsorted(Q, tau, side="right")
    return np.minimum(idx, len(Q) - 1).astype(np.int32), Q


class ResampleFakeOps(FakeOps):
    name = "fake-cpu-resample"

    def resample_ordered_work_bytes(self, n):
        nb = work_bytes(int(n))
        if nb < 0:
            raise ValueError("bk_resample_ordered_work_bytes failed")
        return nb

    def resample_ordered(self, weights, u, mode, slot0, m_total, work, idx_out):
        self._count("resample_ordered")
        n, m_local = int(weights.shape[0]), int(idx_out.shape[0])
        if (n < 1 or m_total < 1 or slot0 < 0 or slot0 + m_local > m_total or n > 2 ** 31 - 1 or m_total > 2 ** 31 - 1
                or mode not in (SYSTEMATIC, STRATIFIED) or work is None or work.numel() * work.element_size() < work_bytes(n)):
            raise ValueError("bk_resample_ordered: BK_E_ARG")
        if m_local == 0:
            return
        idx, Q = resample_ordered_ref(weights.numpy(), u.numpy(), mode, m_local, int(slot0), int(m_total))
        work.numpy().reshape(-1).view(np.uint8)[Q_OFFSET:Q_OFFSET + 8 * n] = Q.view(np.uint8)
        idx_out.numpy()[...] = idx
