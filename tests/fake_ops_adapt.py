"""FakeOps with the entry points of the diagonal preconditioner and the warmup statistics (include/bkhip.h:
bk_momentum_refresh_precond, bk_leapfrog_finish_precond, bk_hmc_draw_gaussian_precond, bk_accept_stat), restated in NumPy
in the DEVICE's summation order -- TEST INFRASTRUCTURE ONLY.

Per-chain sums over the dimensions run over four contiguous quarters, each sequential in d, combined ((p0+p1)+p2)+p3 (the
parent class sums sequentially, which is the same value to ~1e-16 only): with the device's order the acceptance statistic of
a warmup draw is the same double here and on the GPU.
"""
import numpy as np
import torch

from oracle.rng import exp_bk
from tests.fake_ops import FakeOps


def quarter_sum(x):
    """sum over d of x[d, c] as the kernels take it: quarters [q*Dq, (q+1)*Dq), Dq = ceil(D/4), sequential, then
    ((p0+p1)+p2)+p3."""
    D = x.shape[0]
    Dq = (D + 3) // 4
    parts = []
    for q in range(4):
        s = np.zeros(x.shape[1])
        for d in range(q * Dq, min(D, (q + 1) * Dq)):
            s = s + x[d]
        parts.append(s)
    return ((parts[0] + parts[1]) + parts[2]) + parts[3]


def tree256_sum(x):
    """sum over c of x[d, c] as k_rhat_partials takes it: thread t adds chains t, t + 256, ... in order, the 256 sums are
    halved 128, 64, .. 1."""
    D, C = x.shape
    nb = (C + 255) // 256
    pad = np.zeros((D, nb * 256))
    pad[:, :C] = x
    s = np.zeros((D, 256))
    for b in range(nb):
        s = s + pad[:, b * 256:(b + 1) * 256]
    w = 128
    while w > 0:
        s[:, :w] = s[:, :w] + s[:, w:2 * w]
        w >>= 1
    return s[:, 0].copy()


def accept_stat_ref(lp_cur, a_cur, lp_prop, a_prop, exp=None):
    """bk_accept_stat on NumPy vectors -> (sum of the statistic, number of NaN chains), in the kernel's tree order.
    exp: a stand-in for bk_exp that returns the same double (default: oracle.rng.exp_bk, exact but slow)."""
    exp = exp_bk if exp is None else exp
    C = lp_cur.shape[0]
    if C == 0:
        return 0.0, 0.0
    a0 = np.zeros(C) if a_cur is None else a_cur
    a1 = np.zeros(C) if a_prop is None else a_prop
    with np.errstate(invalid="ignore"):
        d = (lp_prop - a1) - (lp_cur - a0)
    nb = (C + 255) // 256
    a = np.zeros(nb * 256)
    nn = np.zeros(nb * 256)
    for c in range(C):
        if d[c] != d[c]:
            nn[c] = 1.0
        else:
            a[c] = min(1.0, exp(min(0.0, float(d[c]))))

    def tree(v):
        w = v.reshape(nb * 4, 64).copy()  # one row per wavefront
        lane = np.arange(64)
        for m in (1, 2, 4, 8, 16, 32):  # v = v + shfl_xor(v, m)
            w = w + w[:, lane ^ m]
        ws = w[:, 0].reshape(nb, 4)
        part = ((ws[:, 0] + ws[:, 1]) + ws[:, 2]) + ws[:, 3]  # work[b]
        red = np.zeros(256)
        for t in range(256):  # thread t: partials t, t + 256, ... in order
            s = 0.0
            for b in range(t, nb, 256):
                s = s + part[b]
            red[t] = s
        width = 128
        while width > 0:
            red[:width] = red[:width] + red[width:2 * width]
            width >>= 1
        return float(red[0])

    return tree(a), tree(nn)


class AdaptFakeOps(FakeOps):
    name = "fake-cpu-adapt"

    _quarter_sum = staticmethod(quarter_sum)  # (hmc_draw_gaussian's three per-chain sums, in the device's order)

    @staticmethod
    def _pd(precond):
        p = precond.numpy()
        return p[0], p[1], p[2]

    def target_grad(self, kind, params, theta, grad, logp, n_dev=None):
        if kind not in ("iso_gaussian", "diag_gaussian") or logp is None or n_dev is not None:
            return super().target_grad(kind, params, theta, grad, logp, n_dev)
        super().target_grad(kind, params, theta, grad, None, n_dev)
        th = theta.numpy()
        lt = th if kind == "iso_gaussian" else params.numpy()[:, None] * th
        logp.numpy()[...] = -0.5 * quarter_sum(th * lt)

    def momentum_refresh(self, kind, state, loc_in, loc_mul, scale, out, metric, kin_out, active=None, work=None):
        super().momentum_refresh(kind, state, loc_in, loc_mul, scale, out, metric, kin_out, active, work)
        if kin_out is not None and active is None:  # (the kinetic energy again, in the device's order)
            o = out.numpy()
            kin_out.numpy()[...] = 0.5 * quarter_sum(o * self._mt(metric, o))

    def leapfrog_finish(self, rho_in, rho_out, grad, metric, half, negate, kin_out, n_dev=None, level=None,
                        lanes_out=None, lanes_total=None):
        plain = n_dev is None and level is None and lanes_out is None and lanes_total is None
        if not plain or kin_out is None:
            return super().leapfrog_finish(rho_in, rho_out, grad, metric, half, negate, kin_out, n_dev, level, lanes_out,
                                           lanes_total)
        r = torch.empty_like(rho_in)
        super().leapfrog_finish(rho_in, r, grad, metric, half, negate, None)
        if rho_out is not None:
            rho_out.copy_(r)
        kin_out.numpy()[...] = 0.5 * quarter_sum(r.numpy() * self._mt(metric, r.numpy()))

    def rhat_partials(self, mean, m2, n, center, out):
        # (the device's order: the pooled variance of a warmup window is then the same double here and on the GPU, which
        # matters -- dual averaging amplifies a one-ulp difference in v to percents within some twenty draws)
        mu = mean.numpy()
        D = mu.shape[0]
        o = out.numpy().reshape(-1)
        o[0:D] = tree256_sum(mu)
        o[D:2 * D] = tree256_sum(m2.numpy() / float(n - 1))
        if center is not None:
            dv = mu - center.numpy()[:, None]
            o[2 * D:3 * D] = tree256_sum(dv * dv)

    def precond_pack(self, v, precond):
        p, x = precond.numpy(), v.numpy().copy()
        p[0], p[1], p[2] = x, np.sqrt(x), 1.0 / x  # (NumPy's sqrt is the IEEE one; torch's vectorised CPU sqrt is not)

    def momentum_refresh_precond(self, kind, state, out, precond, kin_out, work=None):
        self._count("momentum_refresh_precond")
        D, C = out.shape
        _, sd, vinv = self._pd(precond)
        o = out.numpy()
        for c in range(C):
            g = self._gen(kind, state, c)
            o[:, c] = 0.0 + sd * g.standard_normal(D)
            self._put(kind, state, c, g)
        kin_out.numpy()[...] = 0.5 * quarter_sum(o * (vinv[:, None] * o))

    def leapfrog_finish_precond(self, rho_in, rho_out, grad, precond, half, negate, kin_out):
        self._count("leapfrog_finish_precond")
        v, _, vinv = self._pd(precond)
        r = rho_in.numpy().copy() if grad is None else rho_in.numpy() + half * (v[:, None] * grad.numpy())
        if negate:
            r = -r
        if rho_out is not None:
            rho_out.numpy()[...] = r
        if kin_out is not None:
            kin_out.numpy()[...] = 0.5 * quarter_sum(r * (vinv[:, None] * r))

    def hmc_draw_gaussian(self, theta_in, theta_out, rho_in, zt, lam, metric, eps, steps, part, kin0, kin1, lp_out,
                          accept=None, precond=None):
        if precond is None:
            return super().hmc_draw_gaussian(theta_in, theta_out, rho_in, zt, lam, metric, eps, steps, part, kin0, kin1,
                                             lp_out, accept)
        self._count("hmc_draw_gaussian_precond")
        assert metric is None
        D = theta_in.shape[0]
        _, sd, vinv = self._pd(precond)
        r0 = torch.from_numpy(0.0 + sd[:, None] * zt.numpy()[:, :D].T) if zt is not None else rho_in
        r1 = torch.empty_like(theta_in)
        k0 = torch.from_numpy(0.5 * quarter_sum(r0.numpy() * (vinv[:, None] * r0.numpy())))
        if kin0 is not None:
            kin0.copy_(k0)
        self.hmc_trajectory_gaussian(theta_in, theta_out, r0, r1, lam, precond[0], eps, steps)
        kin1.numpy()[...] = 0.5 * quarter_sum(r1.numpy() * (vinv[:, None] * r1.numpy()))
        th = theta_out.numpy()
        lt = th if lam is None else lam.numpy()[:, None] * th
        lp_out.numpy()[...] = -0.5 * quarter_sum(th * lt)
        if accept is not None:
            lp_cur, log_u, mask, ret, count = accept
            self.mh_accept(0, lp_cur, k0, lp_out, kin1, log_u, mask, ret, count)

    def accept_stat(self, lp_cur, a_cur, lp_prop, a_prop, out, work=None):
        self._count("accept_stat")
        s, n = accept_stat_ref(lp_cur.numpy(), None if a_cur is None else a_cur.numpy(), lp_prop.numpy(),
                               None if a_prop is None else a_prop.numpy())
        out.numpy()[0] = s
        out.numpy()[1] = n
