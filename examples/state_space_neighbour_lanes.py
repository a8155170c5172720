"""The state-space model of examples/state_space_model.py written as a NEIGHBOUR lanes source: the library's lane-spread one-launch
kernels (a chain spread over 4 / 8 / 16 lanes of a wavefront, theta and rho in registers, row d - 1 fetched from the neighbouring
lane with DPP moves) instead of the per-chain form the traced PyTorch function gets.

    theta = (a, log s, x_1 .. x_T);   phi = tanh(a);   x_1 ~ N(0, s^2 / (1 - phi^2)),  x_t ~ N(phi x_{t-1}, s^2);
    y_t ~ N(x_t, 0.5^2) observed;   a ~ N(0, 1),  log s ~ N(-1, 0.5^2)

The two head coordinates (a, log s) are held by every lane of a chain; the states are the spread rows.  c.sum_pair sums a term of
(x_{t-1}, x_t) over the rows, c.grad_pair returns its two partials and the library adds them up (g_d = dx(d) + dxp(d+1)).

    python examples/state_space_neighbour_lanes.py          # one MI355X
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "bayes-kit_amd")]

import torch

import bayes_kit_amd as bk

SSM_SRC = """
// theta = (a, log s, x_1 .. x_T), phi = tanh(a); params: y_t at row t + 1 (rows 0 and 1 unused)
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
  // (the observations only make up the value: skipped where the kernel discards it)
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

EXAMPLE_ARGS = (3, [0.05, 0.02, 0.008], [8, 16, 32], 0.2)  # examples/state_space_model.py's DRGHMC settings


def problem(T, dev, seed=11):
    """Observations of a simulated AR(1) path, the PyTorch log density of examples/state_space_model.py, the neighbour source."""
    phi_true, s_true, obs_sd = 0.8, 0.5, 0.5
    g = torch.Generator().manual_seed(seed)
    x_true = torch.zeros(T, dtype=torch.float64)
    x_true[0] = s_true / (1 - phi_true ** 2) ** 0.5 * torch.randn((), generator=g, dtype=torch.float64)
    for t in range(1, T):
        x_true[t] = phi_true * x_true[t - 1] + s_true * torch.randn((), generator=g, dtype=torch.float64)
    y = (x_true + obs_sd * torch.randn(T, generator=g, dtype=torch.float64)).to(dev)

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

    def neighbour_model():
        yp = torch.cat([torch.zeros(2, dtype=torch.float64, device=dev), y])
        return bk.CTarget.from_source(SSM_SRC, T + 2, params=yp, form="lanes", head=2, neighbour=True)

    def init(chains, seed=3):
        g0 = torch.Generator().manual_seed(seed)
        th = torch.zeros((chains, T + 2), dtype=torch.float64)
        th[:, 0] = 0.5 + 0.2 * torch.randn(chains, generator=g0, dtype=torch.float64)
        th[:, 1] = -1.0 + 0.2 * torch.randn(chains, generator=g0, dtype=torch.float64)
        th[:, 2:] = y.cpu() + 0.3 * torch.randn((chains, T), generator=g0, dtype=torch.float64)
        return th

    return x_true, log_density, neighbour_model, init


def ms_per_draw(s, draws):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s.advance(draws)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / draws


def main():
    dev = torch.device("cuda", 0)
    T, chains, draws = 99, 8192, 400
    D = T + 2
    x_true, log_density, neighbour_model, init = problem(T, dev)
    model = neighbour_model()
    dr = bk.DrGhmcDiag(model, *EXAMPLE_ARGS, chains=chains, seed=7, init=init(chains))
    print("neighbour lanes source: one launch per proposal:", dr._one_launch, "| host syncs per draw:", dr.host_syncs_per_draw)
    dr.advance(draws)                                    # burn-in
    mom = bk.RunningMoments(D, chains)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(draws):
        theta, _ = dr.sample()
        mom.update(theta)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / draws
    rh = torch.as_tensor(mom.rhat())
    phi = torch.tanh(theta[:, 0])
    print(f"  {ms:.2f} ms per draw of {chains} chains incl. the moments update | chains with a non-finite state: "
          f"{int((~torch.isfinite(theta).all(1)).sum())}")
    print(f"  R-hat: a {float(rh[0]):.3f}  log s {float(rh[1]):.3f}  max over states {float(rh[2:].max()):.3f}")
    print(f"  posterior mean of phi {float(phi.mean()):.3f} (sd {float(phi.std()):.3f}; truth 0.8), "
          f"of s {float(theta[:, 1].exp().mean()):.3f} (truth 0.5)")
    rmse = float(((theta[:, 2:].mean(0).cpu() - x_true) ** 2).mean().sqrt())
    print(f"  rmse of the posterior mean path against the true states {rmse:.3f} (observation noise 0.5)")
    # the draws alone, next to the same model traced from PyTorch into the per-chain form
    traced = bk.TorchModel(log_density, D, compile=True)
    ch = bk.DrGhmcDiag(traced, *EXAMPLE_ARGS, chains=chains, seed=7, init=init(chains))
    ch.advance(50)
    dr.advance(50)
    print(f"  ms per draw: neighbour lanes {ms_per_draw(dr, 200):.3f} | traced form={traced.compiled_form!r} "
          f"{ms_per_draw(ch, 200):.3f}")


if __name__ == "__main__":
    main()
