"""TemperFakeOps with the four entry points of tempered HMC (include/bkhip.h: bk_tempered_kick_drift, bk_tempered_finish,
bk_tempered_hmc_accept, bk_exchange_columns), restated in NumPy with the same operations in the same order, each rounded on
its own -- TEST INFRASTRUCTURE ONLY."""
import numpy as np

from tests.fake_ops_temper import TemperFakeOps


def tempered_force_ref(grad_ll, grad_lp0, metric, beta):
    """t[d, c] = metric[d] * (grad_lp0[d, c] + beta[c] * grad_ll[d, c]); grad_lp0 / metric None: no such operation."""
    with np.errstate(invalid="ignore", over="ignore"):
        f = beta[None, :] * grad_ll
        if grad_lp0 is not None:
            f = grad_lp0 + f
        return metric[:, None] * f if metric is not None else f


def tempered_kick_drift_ref(theta, rho, grad_ll, grad_lp0, metric, beta, eps, pre, kick):
    """bk_tempered_kick_drift on NumPy [D, C] arrays and [C] vectors -> (theta_out, rho_out); inputs are not modified."""
    t = tempered_force_ref(grad_ll, grad_lp0, metric, beta)
    with np.errstate(invalid="ignore", over="ignore"):
        r = rho.copy()
        if pre is not None:
            r = r + pre[None, :] * t
        if kick is not None:
            r = r + kick[None, :] * t
        return theta + eps[None, :] * r, r


def quarter_sum(x):
    """sum over d of x[d, c] in the kernels' order: four contiguous quarters of ceil(D / 4) rows, sequential inside each
    from 0.0, combined as ((p0 + p1) + p2) + p3."""
    D = x.shape[0]
    Dq = (D + 3) // 4
    parts = []
    for w in range(4):
        p = np.zeros(x.shape[1])
        for d in range(w * Dq, min((w + 1) * Dq, D)):
            p = p + x[d]
        parts.append(p)
    return ((parts[0] + parts[1]) + parts[2]) + parts[3]


def tempered_finish_ref(rho, grad_ll, grad_lp0, metric, beta, half):
    """bk_tempered_finish -> (rho_out [D, C], kin [C]); grad_ll None: no kick."""
    with np.errstate(invalid="ignore", over="ignore"):
        r = rho.copy() if grad_ll is None else rho + half[None, :] * tempered_force_ref(grad_ll, grad_lp0, metric, beta)
        mv = metric[:, None] * r if metric is not None else r
        return r, 0.5 * quarter_sum(r * mv)


def tempered_hmc_accept_ref(ll, lp0, kin0, ll_prop, lp0_prop, kin1, beta, log_u, H):
    """bk_tempered_hmc_accept on NumPy vectors of n columns -> (mask [n] uint8, ll, lp0 (or None), counts [n / H] uint32)."""
    n = len(ll)
    with np.errstate(invalid="ignore", over="ignore"):
        e0, e1 = beta[:n] * ll, beta[:n] * ll_prop[:n]
        if lp0 is not None:
            e0, e1 = lp0 + e0, lp0_prop[:n] + e1
        h0, h1 = e0 - kin0[:n], e1 - kin1[:n]
        acc = log_u[:n] < h1 - h0
    new_ll = np.where(acc, ll_prop[:n], ll)
    new_lp0 = np.where(acc, lp0_prop[:n], lp0) if lp0 is not None else None
    counts = acc.reshape(n // H, H).sum(axis=1).astype(np.uint32)
    return acc.astype(np.uint8), new_ll, new_lp0, counts


def exchange_columns_ref(x, swapped, H):
    """bk_exchange_columns on a NumPy [D, >= C] array -> the array with columns c and c + H exchanged where swapped[c]."""
    C = len(swapped)
    a = np.flatnonzero(np.asarray(swapped[:max(C - H, 0)]) != 0)
    x = x.copy()
    x[:, a], x[:, a + H] = x[:, a + H].copy(), x[:, a].copy()
    return x


class TemperHmcFakeOps(TemperFakeOps):
    name = "fake-cpu-temper-hmc"

    @staticmethod
    def _opt(t, n=None):
        return None if t is None else (t.numpy() if n is None else t.numpy()[:n])

    def tempered_kick_drift(self, theta_in, theta_out, rho_in, rho_out, grad_ll, grad_lp0, metric, beta, eps, pre, kick):
        self._count("tempered_kick_drift")
        D, C = theta_out.shape
        if C == 0 or D == 0:
            return
        th, r = tempered_kick_drift_ref(theta_in.numpy(), rho_in.numpy(), grad_ll.numpy(), self._opt(grad_lp0),
                                        self._opt(metric), beta.numpy()[:C], eps.numpy()[:C], self._opt(pre, C),
                                        self._opt(kick, C))
        rho_out.numpy()[...] = r
        theta_out.numpy()[...] = th

    def tempered_finish(self, rho_in, rho_out, grad_ll, grad_lp0, metric, beta, half, kin_out):
        self._count("tempered_finish")
        D, C = rho_in.shape
        if C == 0 or D == 0:
            return
        r, kin = tempered_finish_ref(rho_in.numpy(), self._opt(grad_ll), self._opt(grad_lp0), self._opt(metric),
                                     self._opt(beta, C), self._opt(half, C))
        if rho_out is not None:
            rho_out.numpy()[...] = r
        if kin_out is not None:
            kin_out.numpy()[:C] = kin

    def tempered_hmc_accept(self, ll, lp0, kin0, ll_prop, lp0_prop, kin1, beta, log_u, mask, counts, H):
        self._count("tempered_hmc_accept")
        n = ll.shape[0]
        if H < 1 or n % H != 0 or (lp0 is None) != (lp0_prop is None):
            raise ValueError("bk_tempered_hmc_accept: BK_E_ARG")
        if n == 0:
            return
        m, new_ll, new_lp0, cnt = tempered_hmc_accept_ref(ll.numpy(), self._opt(lp0), kin0.numpy(), ll_prop.numpy(),
                                                          self._opt(lp0_prop), kin1.numpy(), beta.numpy(), log_u.numpy(), H)
        mask.numpy()[:n] = m
        ll.numpy()[...] = new_ll
        if lp0 is not None:
            lp0.numpy()[...] = new_lp0
        if counts is not None:
            counts.numpy().view(np.uint32)[:n // H] += cnt

    def exchange_columns(self, x, swapped, H):
        self._count("exchange_columns")
        D, C = x.shape
        if H < 1 or C % H != 0:
            raise ValueError("bk_exchange_columns: BK_E_ARG")
        if C == 0 or D == 0:
            return
        x.numpy()[...] = exchange_columns_ref(x.numpy(), swapped.numpy()[:C], H)
