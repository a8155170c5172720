"""Neighbour-coupled densities for the lanes form (CTarget.from_source(..., neighbour=True)) and their twins: an AR(1) with
observations written with + - x only, restated in NumPy in the library's canonical class order (bk_lanes.hpp), and the
state-space model of examples/state_space_model.py as a lanes source and as the example's PyTorch function."""
import numpy as np
import torch

AR1_PARAMS = (0.6, 1.25, 0.8)  # phi, 1 / s^2, 1 / (observation sd)^2


def ar1_src(head):
    """AR(1) rows with an observation y_d each (params = phi, 1/s^2, 1/o^2, y_0 .. y_{D-1}); head coordinates ~ N(0, 1)."""
    heads = "\n".join(f"  const double v{i} = c.head({i});\n  lh = lh + (-0.5 * (v{i} * v{i}));\n  c.grad_head({i}, -v{i});"
                      for i in range(head))
    return """
template <class L> __device__ double bk_lanes_density(L& c, const double* p) {
  const double phi = p[0], is2 = p[1], io2 = p[2];
  double lh = 0.0;
%s
  const double s = c.sum_pair([=](double xp, double x, i64 d) {
    const double r = x - phi * xp;
    const double e = x - p[3 + d];
    return (-0.5 * (r * r)) * is2 + (-0.5 * (e * e)) * io2;
  });
  c.grad_pair([=](double xp, double x, i64 d) {
    const double r = x - phi * xp;
    const double e = x - p[3 + d];
    return bk_pair{(phi * r) * is2, -(r * is2) - e * io2};
  });
  return lh + s;
}
""" % heads


def ar1_y(D):
    return np.sin(0.37 * np.arange(D)) * 1.5


def ar1_params(D, device):
    return torch.as_tensor(np.concatenate([AR1_PARAMS, ar1_y(D)]), dtype=torch.float64, device=device)


class Ar1Canonical:
    """ar1_src's density in NumPy, every operation as the kernels order it: the row terms summed per class c = (d - head) mod 16
    in slot order, classes into four group sums ((cs[g] + cs[g+4]) + cs[g+8]) + cs[g+12], those in order; g_d = dx(d) +
    dxp(d+1), the last row dx alone.  A single chain (the oracle samplers' Model protocol) or a batch [D, n]."""

    def __init__(self, D, head):
        self.D, self.head = D, head
        self.phi, self.is2, self.io2 = AR1_PARAMS
        self.y = ar1_y(D)

    def dims(self):
        return self.D

    def batch(self, th):
        D, H = self.D, self.head
        phi, is2, io2 = self.phi, self.is2, self.io2
        lh = np.zeros(th.shape[1])
        g = np.empty_like(th)
        for i in range(H):
            lh = lh + (-0.5 * (th[i] * th[i]))
            g[i] = -th[i]
        x = th[H:]
        xp = np.concatenate([np.zeros((1, th.shape[1])), th[H:-1]]) if D > H else x
        y = self.y[H:, None]
        r = x - phi * xp
        e = x - y
        term = (-0.5 * (r * r)) * is2 + (-0.5 * (e * e)) * io2
        dxp = (phi * r) * is2
        dx = -(r * is2) - e * io2
        rows = D - H
        cs = []
        for c in range(16):
            acc = np.zeros(th.shape[1])
            for k in range(c, rows, 16):
                acc = acc + term[k]
            cs.append(acc)
        q = [((cs[k] + cs[k + 4]) + cs[k + 8]) + cs[k + 12] for k in range(4)]
        s = ((q[0] + q[1]) + q[2]) + q[3]
        gx = dx.copy()
        gx[:-1] = dx[:-1] + dxp[1:]
        g[H:] = gx
        return lh + s, g

    def log_density(self, theta):
        return float(self.batch(np.asarray(theta, dtype=np.float64)[:, None])[0][0])

    def log_density_gradient(self, theta):
        lp, g = self.batch(np.asarray(theta, dtype=np.float64)[:, None])
        return float(lp[0]), g[:, 0]


SSM_SRC = """
// the state-space model of examples/state_space_model.py: theta = (a, log s, x_1 .. x_T), phi = tanh(a); params = y at rows 2..
template <class L> __device__ double bk_lanes_density(L& c, const double* y) {
  const double a = c.head(0), ls = c.head(1);
  const double phi = tanh(a), ch = cosh(a), ich2 = 1.0 / (ch * ch), prec = exp(-2.0 * ls);
  const double T = (double)(c.dims() - 2);
  // Q: the states' quadratic form times s^2 (x_1 at its stationary variance), B = -(1/2) dQ/dphi
  const double Q = c.sum_pair([=](double xp, double x, i64 d) {
    if (d == 2) return (x * x) * ich2;
    const double r = x - phi * xp;
    return r * r;
  });
  const double B = c.sum_pair([=](double xp, double x, i64 d) {
    if (d == 2) return phi * (x * x);
    return (x - phi * xp) * xp;
  });
  const double Sy = c.wants_logp() ? c.sum([y](double x, i64 d) { const double e = x - y[d]; return e * e; }) : 0.0;
  c.grad_head(0, (prec * B) * ich2 - phi - a);
  c.grad_head(1, prec * Q - T - 4.0 * (ls + 1.0));
  c.grad_pair([=](double xp, double x, i64 d) {
    const double e = 4.0 * (x - y[d]);
    if (d == 2) return bk_pair{0.0, -(prec * ich2) * x - e};
    const double r = x - phi * xp;
    return bk_pair{(prec * phi) * r, -(prec * r) - e};
  });
  return (((-0.5 * prec) * Q - T * ls) - log(ch) - 2.0 * Sy) - (0.5 * (a * a) + 2.0 * ((ls + 1.0) * (ls + 1.0)));
}
"""


def ssm_torch(T, device, seed=11):
    """The example's PyTorch function (observation sd 0.5) and its observations y (T values)."""
    phi_true, s_true, obs_sd = 0.8, 0.5, 0.5
    g = torch.Generator().manual_seed(seed)
    x_true = torch.zeros(T, dtype=torch.float64)
    x_true[0] = s_true / (1 - phi_true ** 2) ** 0.5 * torch.randn((), generator=g, dtype=torch.float64)
    for t in range(1, T):
        x_true[t] = phi_true * x_true[t - 1] + s_true * torch.randn((), generator=g, dtype=torch.float64)
    y = (x_true + obs_sd * torch.randn(T, generator=g, dtype=torch.float64)).to(device)

    def log_density(Th):
        a, ls, x = Th[:, 0], Th[:, 1], Th[:, 2:]
        phi = torch.tanh(a)
        inn = x[:, 1:] - phi[:, None] * x[:, :-1]
        prec = torch.exp(-2.0 * ls)
        ch = torch.cosh(a)
        lp_x = -0.5 * prec * (inn * inn).sum(-1) - (T - 1) * ls \
            - 0.5 * prec / (ch * ch) * x[:, 0] ** 2 - ls - torch.log(ch)
        lp_y = -0.5 * (((y - x) / obs_sd) ** 2).sum(-1)
        return lp_x + lp_y - 0.5 * a * a - 0.5 * ((ls + 1.0) / 0.5) ** 2

    return log_density, y
