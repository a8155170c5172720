"""The stand-ins with the differential-evolution move's entry point (include/bkhip.h: bk_de_propose), restated in NumPy
with the same operations in the same order, each rounded on its own -- TEST INFRASTRUCTURE ONLY."""
import numpy as np

from tests.fake_ops_stretch import StretchFakeOps
from tests.fake_ops_temper import TemperFakeOps


def _index(u, count, top):
    """clamp((int64)(u * count), 0, top): the cast truncates, and a value no int64 holds may come out as anything before
    the clamp."""
    with np.errstate(invalid="ignore", over="ignore"):
        i = np.trunc(np.asarray(u, dtype=np.float64) * float(count))
        i = np.where(np.isfinite(i) & (np.abs(i) < 2.0 ** 62), i, 0.0).astype(np.int64)
    return np.maximum(np.minimum(i, top), 0)


def de_propose_ref(theta, col_act, col_oth, n, H, u_1, u_2, z, gamma0, sigma):
    """bk_de_propose on a NumPy [D, >= columns] state -> (theta_prop [D, n], partner1 [n] int32, partner2 [n] int32,
    gamma [n]).  (For u outside [0, 1) only the clamp is specified, not which end it takes.)"""
    k = np.arange(n, dtype=np.int64)
    i1 = _index(u_1[:n], H, H - 1)
    i2 = _index(u_2[:n], H - 1, H - 2)
    i2 = i2 + (i2 >= i1)
    base = col_oth + (k // H) * H
    j1, j2 = base + i1, base + i2
    g = gamma0 * (1.0 + sigma * np.asarray(z[:n], dtype=np.float64))
    tk = theta[:, col_act:col_act + n]
    diff = theta[:, j1] - theta[:, j2]
    prop = tk + g[None, :] * diff
    return prop, j1.astype(np.int32), j2.astype(np.int32), g


class _DEOps:
    def de_propose(self, theta, col_act, col_oth, n, H, u_1, u_2, z, gamma0, sigma, theta_prop, partner1, partner2, gamma):
        self._count("de_propose")
        columns = max(col_act, col_oth) + n
        if H < 2 or n % H != 0 or theta.shape[1] < columns or tuple(theta_prop.shape) != (theta.shape[0], n):
            raise ValueError("bk_de_propose: BK_E_ARG")
        if n == 0:
            return
        prop, j1, j2, g = de_propose_ref(theta.numpy(), col_act, col_oth, n, H, u_1.numpy(), u_2.numpy(), z.numpy(),
                                         gamma0, sigma)
        theta_prop.numpy()[...] = prop
        partner1.numpy()[:n] = j1
        partner2.numpy()[:n] = j2
        gamma.numpy()[:n] = g


class DEFakeOps(_DEOps, StretchFakeOps):
    name = "fake-cpu-de"


class TemperDEFakeOps(_DEOps, TemperFakeOps):
    name = "fake-cpu-temper-de"
