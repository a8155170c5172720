"""StretchFakeOps with the two entry points of parallel tempering (include/bkhip.h: bk_tempered_accept, bk_replica_swap),
restated in NumPy with the same operations in the same order, each rounded on its own -- TEST INFRASTRUCTURE ONLY."""
import numpy as np

from tests.fake_ops_stretch import StretchFakeOps


def tempered_accept_ref(ll, lp0, ll_prop, lp0_prop, beta, zterm, log_u, H):
    """bk_tempered_accept on NumPy vectors of n columns -> (mask [n] uint8, ll, lp0 (or None), counts [n / H] uint32); the
    inputs are not modified."""
    n = len(ll)
    with np.errstate(invalid="ignore", over="ignore"):
        dp = (lp0_prop[:n] - lp0) if lp0 is not None else 0.0
        acc = log_u[:n] < (dp + beta[:n] * (ll_prop[:n] - ll)) + zterm[:n]
    new_ll = np.where(acc, ll_prop[:n], ll)
    new_lp0 = np.where(acc, lp0_prop[:n], lp0) if lp0 is not None else None
    counts = acc.reshape(n // H, H).sum(axis=1).astype(np.uint32)
    return acc.astype(np.uint8), new_ll, new_lp0, counts


def replica_swap_ref(theta, ll, lp0, beta, log_u, lower, H):
    """bk_replica_swap on a NumPy [D, >= C] state and [C] vectors -> (theta, ll, lp0 (or None), swapped [C] uint8,
    proposed [C / H] uint32, accepted [C / H] uint32); the inputs are not modified."""
    C = len(ll)
    c = np.arange(C)
    prop = (np.asarray(lower[:C]) != 0) & (c + H < C)
    lo = c[prop]
    hi = lo + H
    with np.errstate(invalid="ignore", over="ignore"):
        ok = log_u[lo] < (beta[lo] - beta[hi]) * (ll[hi] - ll[lo])
    a, b = lo[ok], hi[ok]
    theta, ll = theta.copy(), ll.copy()
    theta[:, a], theta[:, b] = theta[:, b].copy(), theta[:, a].copy()
    ll[a], ll[b] = ll[b].copy(), ll[a].copy()
    if lp0 is not None:
        lp0 = lp0.copy()
        lp0[a], lp0[b] = lp0[b].copy(), lp0[a].copy()
    swapped = np.zeros(C, dtype=np.uint8)
    swapped[a] = 1
    proposed = prop.reshape(C // H, H).sum(axis=1).astype(np.uint32)
    accepted = swapped.reshape(C // H, H).sum(axis=1).astype(np.uint32)
    return theta, ll, lp0, swapped, proposed, accepted


class TemperFakeOps(StretchFakeOps):
    name = "fake-cpu-temper"

    def tempered_accept(self, ll, lp0, ll_prop, lp0_prop, beta, zterm, log_u, mask, counts, H):
        self._count("tempered_accept")
        n = ll.shape[0]
        if H < 1 or n % H != 0 or (lp0 is None) != (lp0_prop is None):
            raise ValueError("bk_tempered_accept: BK_E_ARG")
        if n == 0:
            return
        m, new_ll, new_lp0, cnt = tempered_accept_ref(ll.numpy(), None if lp0 is None else lp0.numpy(), ll_prop.numpy(),
                                                      None if lp0 is None else lp0_prop.numpy(), beta.numpy(), zterm.numpy(),
                                                      log_u.numpy(), H)
        mask.numpy()[:n] = m
        ll.numpy()[...] = new_ll
        if lp0 is not None:
            lp0.numpy()[...] = new_lp0
        if counts is not None:
            counts.numpy().view(np.uint32)[:n // H] += cnt

    def replica_swap(self, theta, theta2, ll, lp0, beta, log_u, lower, swapped, proposed, accepted, H):
        self._count("replica_swap")
        D, C = theta.shape
        if H < 1 or C % H != 0:
            raise ValueError("bk_replica_swap: BK_E_ARG")
        if C == 0:
            return
        th, new_ll, new_lp0, sw, prop, acc = replica_swap_ref(theta.numpy(), ll.numpy()[:C],
                                                              None if lp0 is None else lp0.numpy()[:C], beta.numpy(),
                                                              log_u.numpy(), lower.numpy(), H)
        theta.numpy()[...] = th
        if theta2 is not None:
            t2 = theta2.numpy()
            a = np.flatnonzero(sw)
            t2[:, a], t2[:, a + H] = t2[:, a + H].copy(), t2[:, a].copy()
        ll.numpy()[:C] = new_ll
        if lp0 is not None:
            lp0.numpy()[:C] = new_lp0
        swapped.numpy()[:C] = sw
        if proposed is not None:
            proposed.numpy().view(np.uint32)[:C // H] += prop
        if accepted is not None:
            accepted.numpy().view(np.uint32)[:C // H] += acc
