"""FakeOps with the two entry points of the energy diagnostics (include/bkhip.h: bk_energy_update, bk_divergence_capture),
restated in NumPy -- TEST INFRASTRUCTURE ONLY.

energy_ref and capture_ref are the contract in a few lines, and what every exact check compares with.  The stand-in's ops
walk the launch as the kernels do -- workgroups of 256 chains, the exclusive scan of their flag counts, the gather over
(block of chains, block of 16 rows) with a chain's rank re-derived inside its block -- so that one seam at a time can be
broken (``fault``) to show that the checks of tests/energy_parity.py notice."""
import numpy as np
import torch

from tests.fake_ops import FakeOps
from tests.fake_ops_adapt import AdaptFakeOps

BLOCK = 256
GATHER_ROWS = 16
STATE = ("mean_E", "m2_E", "last_E", "ssd", "trans", "cnt", "ndiv")


def new_state(C):
    s = {k: np.zeros(C) for k in STATE[:4]}
    s.update({k: np.zeros(C, dtype=np.int64) for k in STATE[4:]})
    s.update(div_mask=np.zeros(C, dtype=np.uint8), err=np.zeros(C), totals=np.zeros(4, dtype=np.int64))
    return s


def new_store(D, cap):
    return dict(theta_div=np.zeros((D, cap)), chain=np.zeros(cap, dtype=np.int64), draw=np.zeros(cap, dtype=np.int64),
                err_store=np.zeros(cap), fill=np.zeros(2, dtype=np.int64))


def energy_ref(s, lp_cur, a_cur, lp_prop, a_prop, log_u, threshold):
    """One bk_energy_update on the state dict `s` (new_state), in place: the contract of include/bkhip.h."""
    a0 = 0.0 if a_cur is None else a_cur
    a1 = 0.0 if a_prop is None else a_prop
    with np.errstate(invalid="ignore", over="ignore"):
        h0, h1 = lp_cur - a0, lp_prop - a1
        d = h1 - h0
        acc = log_u < d
        div = np.isnan(d) | (d < -threshold)
        E = -np.where(acc, h1, h0)
        ok = np.isfinite(E)
        s["err"][:] = d
        s["div_mask"][:] = div
        s["trans"] += 1
        s["ndiv"] += div
        first = s["cnt"] == 0
        n1 = (s["cnt"] + 1).astype(np.float64)
        delta = E - s["mean_E"]
        mean = s["mean_E"] + delta / n1
        m2 = s["m2_E"] + delta * (E - mean)
        t = E - s["last_E"]
        ssd = s["ssd"] + t * t
    s["ssd"][:] = np.where(ok & ~first, ssd, s["ssd"])
    s["mean_E"][:] = np.where(ok, mean, s["mean_E"])
    s["m2_E"][:] = np.where(ok, m2, s["m2_E"])
    s["last_E"][:] = np.where(ok, E, s["last_E"])
    s["cnt"] += ok
    s["totals"] += np.array([d.shape[0], div.sum(), np.isnan(d).sum(), (~ok).sum()], dtype=np.int64)


def capture_ref(st, div_mask, err, trans, theta, chain0):
    """One bk_divergence_capture on the store dict `st` (new_store), in place: ascending chains, the earliest kept."""
    cap = st["chain"].shape[0]
    for c in np.flatnonzero(div_mask):
        p = int(st["fill"][0])
        if p < cap:
            st["theta_div"][:, p] = theta[:, c]
            st["chain"][p], st["draw"][p], st["err_store"][p] = chain0 + c, trans[c], err[c]
            st["fill"][0] += 1
        st["fill"][1] += 1


FAULTS = ("le", "nan_ok", "e_h1", "nonfinite_welford", "ssd_first", "delta_sq", "arrival", "overrun", "chain0", "pitch")


class EnergyOpsMixin:
    """fault: None, or one of FAULTS -- one seam broken:
      le                 d <= -threshold is divergent
      nan_ok             a NaN energy error is not divergent
      e_h1               E = -h1 whether the chain accepts or not
      nonfinite_welford  a non-finite E is fed to the Welford step
      ssd_first          the squared difference is added from the first finite energy on (against last = 0)
      delta_sq           m2 += delta * delta
      arrival            a block's place in the store is decided by the order blocks arrive in (here: last block first)
      overrun            entries past cap are stored as well (over the last slot) and counted as stored
      chain0             chain ids start at 0
      pitch              a row of theta is C elements long, not ld"""
    fault = None

    def energy_update(self, lp_cur, a_cur, lp_prop, a_prop, log_u, threshold, mean_E, m2_E, last_E, ssd, trans, cnt, ndiv,
                      div_mask, err, totals):
        self._count("energy_update")
        thr = float(threshold)
        if not (np.isfinite(thr) and thr > 0.0):
            raise ValueError("bk_energy_update: BK_E_ARG")
        f = self.fault
        n = lambda t: None if t is None else t.numpy()  # noqa: E731  (views: slices are written in place)
        l0, a0, l1, a1, lu = n(lp_cur), n(a_cur), n(lp_prop), n(a_prop), n(log_u)
        mu_, q_, last_, ssd_, tr_, cnt_, nd_, mk_, er_, tot = (n(x) for x in (mean_E, m2_E, last_E, ssd, trans, cnt, ndiv,
                                                                              div_mask, err, totals))
        C = l0.shape[0]
        with np.errstate(invalid="ignore", over="ignore"):
            for b0 in range(0, C, BLOCK):  # one workgroup
                sl = slice(b0, min(C, b0 + BLOCK))
                h0 = l0[sl] - (0.0 if a0 is None else a0[sl])
                h1 = l1[sl] - (0.0 if a1 is None else a1[sl])
                d = h1 - h0
                acc = lu[sl] < d
                nan = np.isnan(d)
                div = (d <= -thr) if f == "le" else (d < -thr)
                if f != "nan_ok":
                    div = div | nan
                er_[sl], mk_[sl] = d, div
                tr_[sl] += 1
                nd_[sl] += div
                E = -h1 if f == "e_h1" else -np.where(acc, h1, h0)
                fin = np.isfinite(E)
                ok = np.ones_like(fin) if f == "nonfinite_welford" else fin
                n0 = cnt_[sl].copy()
                n1 = (n0 + 1).astype(np.float64)
                delta = E - mu_[sl]
                mean = mu_[sl] + delta / n1
                m2 = q_[sl] + (delta * delta if f == "delta_sq" else delta * (E - mean))
                t = E - last_[sl]
                pair = ok if f == "ssd_first" else ok & (n0 > 0)
                ssd_[sl] = np.where(pair, ssd_[sl] + t * t, ssd_[sl])
                mu_[sl] = np.where(ok, mean, mu_[sl])
                q_[sl] = np.where(ok, m2, q_[sl])
                last_[sl] = np.where(ok, E, last_[sl])
                cnt_[sl] += ok
                tot[:4] += np.array([d.shape[0], div.sum(), nan.sum(), (~fin).sum()], dtype=np.int64)  # (the ballots)

    @staticmethod
    def divergence_capture_work_elems(C):
        return -(-int(C) // BLOCK) + 2

    def divergence_capture(self, div_mask, err, trans, theta, chain0, theta_div, chain, draw, err_store, fill, work):
        self._count("divergence_capture")
        f = self.fault
        mk, fl, wk = div_mask.numpy(), fill.numpy(), work.numpy()
        C = mk.shape[0]
        nb = -(-C // BLOCK)
        assert wk.shape[0] >= nb + 2
        store = theta is not None and theta_div is not None and theta_div.shape[1] > 0
        cap = theta_div.shape[1] if store else 0
        if C == 0:
            return
        # the scan (one workgroup): flags per block, their exclusive prefix, the fill level found, the new fill level
        counts = np.array([int((mk[b * BLOCK:(b + 1) * BLOCK] != 0).sum()) for b in range(nb)], dtype=np.int64)
        wk[:nb] = np.cumsum(counts) - counts
        wk[nb], wk[nb + 1] = counts.sum(), fl[0]
        fl[0] = fl[0] + (wk[nb] if f == "overrun" and cap else min(wk[nb], max(cap - fl[0], 0)))
        fl[1] += wk[nb]
        if not store:
            return
        D = theta_div.shape[0]
        th = theta.numpy()
        if f == "pitch" and D > 1 and theta.stride(0) > C:
            th = torch.as_strided(theta, (D, C), (C, 1)).numpy()
        td, ch, dr, es, er, tr = (x.numpy() for x in (theta_div, chain, draw, err_store, err, trans))
        base = int(wk[nb + 1])
        arrived = base  # ("arrival": an atomic counter takes the place of the scan)
        blocks = range(nb - 1, -1, -1) if f == "arrival" else range(nb)
        for b in blocks:  # one workgroup per (block of chains, block of rows)
            if counts[b] == 0:
                continue
            first = arrived if f == "arrival" else base + int(wk[b])
            arrived += int(counts[b])
            if first >= cap and f != "overrun":
                continue
            flags = mk[b * BLOCK:(b + 1) * BLOCK] != 0
            rank = np.cumsum(flags) - flags  # (wavefront counts before the chain's wavefront + the ballot below its lane)
            for t in np.flatnonzero(flags):
                c, pos = b * BLOCK + int(t), first + int(rank[t])
                if pos >= cap:
                    if f != "overrun":
                        continue
                    pos = cap - 1
                for d0 in range(0, D, GATHER_ROWS):
                    if d0 == 0:
                        ch[pos], dr[pos], es[pos] = (0 if f == "chain0" else int(chain0)) + c, tr[c], er[c]
                    td[d0:d0 + GATHER_ROWS, pos] = th[d0:d0 + GATHER_ROWS, c]


    # the per-pitch entry points of the tile-major schedule: the parent's restatements work on views of any pitch
    def kick_drift_ld(self, theta_in, theta_out, rho_in, rho_out, grad, metric, eps, use_pre, pre, use_kick, kick):
        self.kick_drift(theta_in, theta_out, rho_in, rho_out, grad, metric, eps, use_pre, pre, use_kick, kick)

    def blend_columns_ld(self, mask, a, b, out):
        self.blend_columns(mask, a, b, out)

    def select_columns_ld(self, mask, dst, src):
        self.select_columns(mask, dst, src)


class EnergyFakeOps(EnergyOpsMixin, FakeOps):
    name = "fake-cpu-energy"

    def __init__(self, fault=None):
        super().__init__()
        assert fault is None or fault in FAULTS
        self.fault = fault


class EnergyAdaptFakeOps(EnergyOpsMixin, AdaptFakeOps):
    """... on the stand-in that has warmup()'s statistics."""
    name = "fake-cpu-energy-adapt"
