"""AdaptFakeOps with the two entry points of the trajectory-length statistic (include/bkhip.h: bk_chees_sums,
bk_chees_stat), restated in NumPy in the DEVICE's summation order -- TEST INFRASTRUCTURE ONLY.

bk_chees_sums: per dimension, k_rhat_partials' tree over the chains (tests/fake_ops_adapt.tree256_sum).
bk_chees_stat: the three per-chain sums in the library's quarter order (quarter_sum), every product and sum rounded on its
own; the sums over chains in bk_accept_stat's tree (wave xor butterfly, ((w0+w1)+w2)+w3, single-workgroup combine).
"""
import numpy as np

from oracle.rng import exp_bk
from tests.fake_ops_adapt import AdaptFakeOps, accept_stat_ref, quarter_sum, tree256_sum


def accept_tree_sum(v):
    """sum over chains of v[c] in bk_accept_stat's order."""
    C = v.shape[0]
    if C == 0:
        return 0.0
    nb = (C + 255) // 256
    pad = np.zeros(nb * 256)
    pad[:C] = v
    w = pad.reshape(nb * 4, 64).copy()  # one row per wavefront
    lane = np.arange(64)
    for m in (1, 2, 4, 8, 16, 32):  # v = v + shfl_xor(v, m)
        w = w + w[:, lane ^ m]
    ws = w[:, 0].reshape(nb, 4)
    part = ((ws[:, 0] + ws[:, 1]) + ws[:, 2]) + ws[:, 3]  # work[b]
    red = np.zeros(256)
    for t in range(min(256, nb)):  # thread t: partials t, t + 256, ... in order
        s = 0.0
        for b in range(t, nb, 256):
            s = s + part[b]
        red[t] = s
    width = 128
    while width > 0:
        red[:width] = red[:width] + red[width:2 * width]
        width >>= 1
    return float(red[0])


def chees_sums_ref(theta, theta_p):
    """bk_chees_sums on NumPy [D, C] arrays -> [2 D]."""
    return np.concatenate([tree256_sum(theta), tree256_sum(theta_p)])


def chees_weights(lp_cur, a_cur, lp_prop, a_prop, exp=None):
    """w_c = 0 if d_c is NaN, else min(1, bk_exp(min(0, d_c))), d_c as in bk_accept_stat."""
    exp = exp_bk if exp is None else exp
    C = lp_cur.shape[0]
    a0 = np.zeros(C) if a_cur is None else a_cur
    a1 = np.zeros(C) if a_prop is None else a_prop
    with np.errstate(invalid="ignore"):
        d = (lp_prop - a1) - (lp_cur - a0)
    w = np.zeros(C)
    for c in range(C):
        if d[c] == d[c]:
            w[c] = min(1.0, exp(min(0.0, float(d[c]))))
    return w


def chees_stat_ref(theta, theta_p, rho_p, mean, lp_cur, a_cur, lp_prop, a_prop, exp=None):
    """bk_chees_stat on NumPy arrays -> (sum of w g, number of chains with w > 0 and a non-finite g)."""
    D, C = theta.shape
    if C == 0:
        return 0.0, 0.0
    w = chees_weights(lp_cur, a_cur, lp_prop, a_prop, exp)
    with np.errstate(invalid="ignore", over="ignore"):
        dp = theta_p - mean[D:2 * D, None]
        dc = theta - mean[0:D, None]
        A, B, P = quarter_sum(dp * dp), quarter_sum(dc * dc), quarter_sum(dp * rho_p)
        g = (A - B) * P
        ok = (w > 0.0) & np.isfinite(g)
        s = np.where(ok, w * np.where(ok, g, 0.0), 0.0)
    nn = ((w > 0.0) & ~np.isfinite(g)).astype(np.float64)
    return accept_tree_sum(s), accept_tree_sum(nn)


class CheesFakeOps(AdaptFakeOps):
    name = "fake-cpu-chees"

    def __init__(self):
        super().__init__()
        self._exp_memo = {}

    def exp(self, x):
        """oracle.rng.exp_bk, remembered: a warmup draw asks for the same exponentials twice (accept_stat, chees_stat)."""
        y = self._exp_memo.get(x)
        if y is None:
            if len(self._exp_memo) > 4096:
                self._exp_memo.clear()
            y = self._exp_memo[x] = exp_bk(x)
        return y

    def accept_stat(self, lp_cur, a_cur, lp_prop, a_prop, out, work=None):
        self._count("accept_stat")
        opt = lambda t: None if t is None else t.numpy()  # noqa: E731
        s, n = accept_stat_ref(lp_cur.numpy(), opt(a_cur), lp_prop.numpy(), opt(a_prop), exp=self.exp)
        out.numpy()[0] = s
        out.numpy()[1] = n

    @staticmethod
    def chees_work_elems(C):
        return max(2, 12 * C + 2 * ((C + 255) // 256))

    def chees_sums(self, theta, theta_p, out):
        self._count("chees_sums")
        D = theta.shape[0]
        out.numpy()[:2 * D] = chees_sums_ref(theta.numpy(), theta_p.numpy())

    def chees_stat(self, theta, theta_p, rho_p, mean, lp_cur, a_cur, lp_prop, a_prop, out, work=None):
        self._count("chees_stat")
        opt = lambda t: None if t is None else t.numpy()  # noqa: E731
        s, n = chees_stat_ref(theta.numpy(), theta_p.numpy(), rho_p.numpy(), mean.numpy(), lp_cur.numpy(), opt(a_cur),
                              lp_prop.numpy(), opt(a_prop), self.exp)
        out.numpy()[0] = s
        out.numpy()[1] = n
