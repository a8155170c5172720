"""AdaptFakeOps with the entry points of the preconditioned MALA (include/bkhip.h: bk_mala_step_precond,
bk_mala_step_gaussian_precond, bk_mala_propose_from_normals_precond, bk_mala_logq_precond) restated in NumPy in the DEVICE's
summation order -- TEST INFRASTRUCTURE ONLY.

The plain MALA ops are restated in the device's order as well (the parent classes sum sequentially over d, the same value to
~1e-16 only): a warmup draw's acceptance statistic is then the same double here and on the GPU before the first
preconditioner exists, and the preconditioned ops with v = 1 are the plain ones bit for bit.

* the step kernels (k_mala_step, k_mala_step_sep): thread row r = 0..63 adds its slots r, r + 64, ... r + 64 (E - 1) in
  sequence (E = 2, 4, 8, 16 for D <= 128, 256, 512, 1024; rows >= D add +0.0), a xor tree over each group of 8 consecutive
  rows, then the 8 groups in order;
* bk_mala_logq[_precond]: four contiguous quarters, ((p0+p1)+p2)+p3 (tests/fake_ops_adapt.quarter_sum).
"""
import numpy as np
import torch

from tests.fake_ops_adapt import AdaptFakeOps, quarter_sum


def step_slots(D):
    return 2 if D <= 128 else 4 if D <= 256 else 8 if D <= 512 else 16


def step_sum(x):
    """sum over d of x[d, c] in the step kernels' order."""
    D, C = x.shape
    E = step_slots(D)
    pad = np.zeros((64 * E, C))
    pad[:D] = x
    slots = pad.reshape(E, 64, C)
    s = np.zeros((64, C))
    for e in range(E):
        s = s + slots[e]
    g = s.reshape(8, 8, C)  # [group][row in the group]
    g = ((g[:, 0] + g[:, 1]) + (g[:, 2] + g[:, 3])) + ((g[:, 4] + g[:, 5]) + (g[:, 6] + g[:, 7]))
    t = g[0]
    for k in range(1, 8):
        t = t + g[k]
    return t


def _residuals(th, g, thp, gp, eps, pd):
    """-> the forward / reverse terms summed per chain: (x*x) plain, (x*x)*(1/v) with x = .. - eps*(v*grad) preconditioned."""
    with np.errstate(invalid="ignore", over="ignore"):  # (a non-finite input follows IEEE arithmetic, as on the device)
        if pd is None:
            xf = (thp - th) - eps * g
            xr = (th - thp) - eps * gp
            return xf * xf, xr * xr
        v, iv = pd[0][:, None], pd[2][:, None]
        xf = (thp - th) - eps * (v * g)
        xr = (th - thp) - eps * (v * gp)
        return (xf * xf) * iv, (xr * xr) * iv


class MalaAdaptFakeOps(AdaptFakeOps):
    name = "fake-cpu-mala-adapt"

    # -- proposal -----------------------------------------------------------------------------------------------------
    def mala_propose_from_normals_precond(self, theta, grad, z, precond, theta_prop, eps, sqrt2eps):
        self._count("mala_propose_from_normals_precond")
        v, sd, _ = self._pd(precond)
        theta_prop.numpy()[...] = ((theta.numpy() + eps * (v[:, None] * grad.numpy()))
                                   + sqrt2eps * (sd[:, None] * z.numpy()))

    # -- proposal densities ---------------------------------------------------------------------------------------------
    def _logq(self, theta, grad, theta_prop, grad_prop, eps, lp_forward, lp_reverse, pd):
        if theta.shape[0] == 0 or theta.shape[1] == 0:  # C == 0 or D == 0: BK_OK, nothing launched, nothing written
            return
        tf, tr = _residuals(theta.numpy(), grad.numpy(), theta_prop.numpy(), grad_prop.numpy(), eps, pd)
        k = -0.25 / eps
        lp_forward.numpy()[...] = k * quarter_sum(tf)
        lp_reverse.numpy()[...] = k * quarter_sum(tr)

    def mala_logq(self, theta, grad, theta_prop, grad_prop, eps, lp_forward, lp_reverse):
        self._count("mala_logq")
        self._logq(theta, grad, theta_prop, grad_prop, eps, lp_forward, lp_reverse, None)

    def mala_logq_precond(self, theta, grad, theta_prop, grad_prop, precond, eps, lp_forward, lp_reverse):
        self._count("mala_logq_precond")
        self._logq(theta, grad, theta_prop, grad_prop, eps, lp_forward, lp_reverse, self._pd(precond))

    # -- the step kernels -------------------------------------------------------------------------------------------------
    def _step(self, theta, theta_out, grad, theta_prop, grad_prop, lp, lp_prop, log_u, zt_next, eps, sqrt2eps, mask, ret,
              count, pd):
        th, g, thp, gp = theta.numpy(), grad.numpy(), theta_prop.numpy(), grad_prop.numpy()
        tf, tr = _residuals(th, g, thp, gp, eps, pd)
        k = -0.25 / eps
        l0, l1 = lp.numpy().copy(), lp_prop.numpy()
        with np.errstate(invalid="ignore"):
            acc = log_u.numpy() < (l1 - l0) + (k * step_sum(tr) - k * step_sum(tf))
        new_th = np.where(acc[None, :], thp, th)
        new_g = np.where(acc[None, :], gp, g)
        theta_out.numpy()[...] = new_th
        grad.numpy()[...] = new_g
        lp.numpy()[...] = np.where(acc, l1, l0)
        if ret is not None:
            ret.numpy()[...] = lp.numpy()
        if mask is not None:
            mask.numpy()[...] = acc
        if count is not None:
            count += int(acc.sum())
        if zt_next is not None:
            z = zt_next.numpy()[:, :th.shape[0]].T
            if pd is None:
                theta_prop.numpy()[...] = (new_th + eps * new_g) + sqrt2eps * z
            else:
                theta_prop.numpy()[...] = (new_th + eps * (pd[0][:, None] * new_g)) + sqrt2eps * (pd[1][:, None] * z)

    def mala_step(self, theta, theta_out, grad, theta_prop, grad_prop, lp, lp_prop, log_u, zt_next, eps, sqrt2eps, mask,
                  ret, count):
        self._count("mala_step")
        self._step(theta, theta_out, grad, theta_prop, grad_prop, lp, lp_prop, log_u, zt_next, eps, sqrt2eps, mask, ret,
                   count, None)

    def mala_step_precond(self, theta, theta_out, grad, theta_prop, grad_prop, precond, lp, lp_prop, log_u, zt_next, eps,
                          sqrt2eps, mask, ret, count):
        self._count("mala_step_precond")
        self._step(theta, theta_out, grad, theta_prop, grad_prop, lp, lp_prop, log_u, zt_next, eps, sqrt2eps, mask, ret,
                   count, self._pd(precond))

    def mala_step_gaussian(self, lam, theta, theta_out, theta_prop, lp, lp_prop, log_u, zt_next, eps, sqrt2eps, mask, ret,
                           count, precond=None):
        self._count("mala_step_gaussian" if precond is None else "mala_step_gaussian_precond")
        kind = "iso_gaussian" if lam is None else "diag_gaussian"
        g, gp = torch.zeros_like(theta), torch.zeros_like(theta_prop)  # both gradients recomputed, none stored
        self.target_grad(kind, lam, theta, g, None)
        self.target_grad(kind, lam, theta_prop, gp, None)
        self._step(theta, theta_out, g, theta_prop, gp, lp, lp_prop, log_u, zt_next, eps, sqrt2eps, mask, ret, count,
                   None if precond is None else self._pd(precond))
