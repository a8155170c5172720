"""FakeOps with the stretch move's entry point (include/bkhip.h: bk_stretch_propose), restated in NumPy with the same
operations in the same order, each rounded on its own -- TEST INFRASTRUCTURE ONLY."""
import numpy as np

from tests.fake_ops import FakeOps


def stretch_propose_ref(theta, col_act, col_oth, n, H, u_j, u_z, inv_sqrt_a, sqrt_a):
    """bk_stretch_propose on a NumPy [D, >= columns] state -> (theta_prop [D, n], zterm [n], partner [n] int32)."""
    D = theta.shape[0]
    k = np.arange(n, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        i = np.floor(np.asarray(u_j[:n], dtype=np.float64) * float(H)).astype(np.int64)
    i = np.maximum(np.minimum(i, H - 1), 0)
    j = col_oth + (k // H) * H + i
    r = inv_sqrt_a + (sqrt_a - inv_sqrt_a) * np.asarray(u_z[:n], dtype=np.float64)
    z = r * r
    tk = theta[:, col_act:col_act + n]
    tj = theta[:, j]
    diff = tk - tj
    prop = tj + z[None, :] * diff
    zterm = float(D - 1) * np.log(z)
    return prop, zterm, j.astype(np.int32)


class StretchFakeOps(FakeOps):
    name = "fake-cpu-stretch"

    def stretch_propose(self, theta, col_act, col_oth, n, H, u_j, u_z, inv_sqrt_a, sqrt_a, theta_prop, zterm, partner):
        self._count("stretch_propose")
        columns = max(col_act, col_oth) + n
        if H < 1 or n % H != 0 or theta.shape[1] < columns or tuple(theta_prop.shape) != (theta.shape[0], n):
            raise ValueError("bk_stretch_propose: BK_E_ARG")
        if n == 0:
            return
        prop, zt, j = stretch_propose_ref(theta.numpy(), col_act, col_oth, n, H, u_j.numpy(), u_z.numpy(), inv_sqrt_a,
                                          sqrt_a)
        theta_prop.numpy()[...] = prop
        zterm.numpy()[:n] = zt
        partner.numpy()[:n] = j
