"""Checks of the preconditioned MALA (MALA(precond_diag=v)) and MALA.warmup that take the kernel library as an argument:
tests/test_mala_adapt_cpu.py runs them on the NumPy stand-in (tests/fake_ops_mala_adapt.py), tests/test_gpu_mala_adapt.py on
the HIP library."""
import hashlib
import json
import os

import numpy as np
import torch

import bayes_kit_amd as bk
from tests.adapt_parity import perturbed_variances, reports_equal  # noqa: F401  (re-exported)

EPS = 0.6  # (the targets below have about unit scale after preconditioning: an acceptance of 0.65-0.8 at D = 6 .. 130)


def _np(t):
    return np.asarray(t.cpu())


def eps_for(D):
    """A step size with a middling acceptance on a unit-scale Gaussian in D dimensions (MALA: eps ~ D^(-1/3))."""
    return min(0.5, 1.5 * D ** (-1.0 / 3.0))


def run_draws(s, n):
    """n draws -> (theta [n, C, D], logp [n, C], accept masks [n, C])."""
    th, lp, acc = [], [], []
    for _ in range(n):
        t, l = s.sample()
        th.append(_np(t).copy())
        lp.append(_np(l).copy())
        acc.append(_np(s.last_accept).copy())
    return np.stack(th), np.stack(lp), np.stack(acc)


def theta0(C, D, seed=2):
    return np.random.default_rng(seed).normal(size=(C, D))


def make(ops, C, D, v=None, seed=77, eps=None, model=None, **kw):
    """MALA on N(0, 1/lam), lam = logspace(0, 1, D), started inside the target (in the transient phase every proposal of a
    small step is accepted and every one of a large step refused: nothing for a decision to get wrong)."""
    lam = np.logspace(0, 1, D)
    model = bk.DiagGaussian(lam, ops=ops) if model is None else model
    return bk.MALA(model, eps_for(D) if eps is None else eps, init=theta0(C, D) / np.sqrt(lam), chains=C, seed=seed,
                   precond_diag=v, ops=ops, **kw)


# ---- 1. against the oracle, by rescaling ------------------------------------------------------------------------------
def check_vs_oracle(ops, C, D, path, draws=6):
    """MALA with precond_diag = v on N(0, 1/lam) IS plain MALA on y = theta / sqrt(v), whose target is N(0, 1/(lam v)):
    oracle.samplers.MALA on oracle.models.DiagGaussian(lam * v) from theta0 / sqrt(v), same stream.  theta = sqrt(v) * y at
    rel 1e-10 / atol 1e-13, logp at atol 1e-12 (the project's bar for precond_diag), every accept decision equal."""
    from oracle import models as om
    from oracle import samplers as osamp

    lam = np.logspace(0, 1, D)
    v = perturbed_variances(lam)
    sd = np.sqrt(v)
    t0 = theta0(C, D)
    s = bk.MALA(bk.DiagGaussian(lam, ops=ops), EPS, init=t0, seed=31, precond_diag=v, path=path, ops=ops)
    th, lp, acc = run_draws(s, draws)
    chains = sorted(set(np.linspace(0, C - 1, 8).astype(int).tolist()))
    n_acc = 0
    for c in chains:
        o = osamp.MALA(om.DiagGaussian(lam * v), EPS, init=t0[c] / sd, seed=np.random.Philox(key=[31, c]))
        for n in range(draws):
            y, olp = o.sample()
            assert bool(acc[n][c]) == o.last_accept, (c, n)
            np.testing.assert_allclose(th[n][c], sd * y, rtol=1e-10, atol=1e-13)
            np.testing.assert_allclose(lp[n][c], olp, rtol=0.0, atol=1e-12)
            n_acc += o.last_accept
    assert 0 < n_acc < len(chains) * draws  # (both outcomes of the decision were compared)
    return s


# ---- 2. ones are the plain sampler ------------------------------------------------------------------------------------
def check_identity(ops, C, D, knobs_list=(dict(),)):
    """precond_diag = ones IS the sampler without it: every added factor is an exact multiplication by 1.0."""
    for kw in knobs_list:
        # (no preconditioning: the step size is bounded by the stiffest direction, lam = 10)
        a = make(ops, C, D, np.ones(D), seed=3, eps=0.05, **kw)
        b = make(ops, C, D, None, seed=3, eps=0.05, **kw)
        ra, rb = run_draws(a, 4), run_draws(b, 4)
        for x, y in zip(ra, rb):
            assert np.array_equal(x, y), kw
        assert np.array_equal(a.rng_state(), b.rng_state()), kw
        assert 0.0 < a.accept_rate() < 1.0


# ---- 3. paths and knobs agree -----------------------------------------------------------------------------------------
def six_draws(ops, C, D, v, v2=None, draws=6, **kw):
    """`draws` draws; v2: set_precond_diag(v2) between draws 3 and 4.  -> (theta, accept masks, final stream table)"""
    s = make(ops, C, D, v, **kw)
    th, _, acc = run_draws(s, 3)
    if v2 is not None:
        s.set_precond_diag(v2)
    th2, _, acc2 = run_draws(s, draws - 3)
    return np.concatenate([th, th2]), np.concatenate([acc, acc2]), s.rng_state().copy()


def check_paths_agree(ops, C, D, variants, draws=6):
    """Every variant gives array_equal draws, accept masks and final stream positions, with the preconditioner replaced
    between draws 3 and 4 and without.  The first variant is the reference."""
    lam = np.logspace(0, 1, D)
    v, v2 = perturbed_variances(lam), perturbed_variances(lam, seed=6)
    for change in (None, v2):
        ref = six_draws(ops, C, D, v, change, draws, **variants[0])
        assert 0 < ref[1].sum() < ref[1].size
        for kw in variants[1:]:
            got = six_draws(ops, C, D, v, change, draws, **kw)
            for k, (x, y) in enumerate(zip(got, ref)):
                assert np.array_equal(x, y), (kw, change is not None, ("theta", "accept", "rng")[k])


# ---- 4. the kernels alone against the stand-in --------------------------------------------------------------------------
STEP_SHAPES = [(34, 33, False, True), (16, 64, True, True), (50, 1000, False, False), (300, 257, True, True),
               (2, 1024, False, True), (16, 513, False, True)]


def _wide_v(D, g):
    """Variances spanning 1e-6 .. 1e6."""
    return 10.0 ** g.uniform(-6.0, 6.0, size=D)


def check_step_kernels(ops, fake, gaussian):
    """bk_mala_step_precond (gaussian: bk_mala_step_gaussian_precond with lam) alone on random inputs -- ragged last block,
    odd D, in-place theta_out, no next proposal, v over twelve decades -- against its NumPy statement: every output
    array_equal (the stand-in restates the device's summation order, so the sums are the same doubles)."""
    rng = np.random.default_rng(5)
    for C, D, inplace, with_z in STEP_SHAPES:
        eps = 0.01
        s2 = float(np.sqrt(2 * eps))
        v = _wide_v(D, rng)
        lam = rng.uniform(0.5, 2.0, size=D) / v
        th = rng.normal(size=(D, C)) * np.sqrt(v)[:, None]
        g = -th * lam[:, None]
        thp = th + eps * v[:, None] * g + s2 * np.sqrt(v)[:, None] * rng.normal(size=(D, C))
        gp = -thp * lam[:, None]
        lp, logu = rng.normal(size=C), np.log(rng.uniform(size=C))
        lpp = lp + 0.5 * rng.normal(size=C)
        dp = (D + 7) // 8 * 8
        zt = rng.normal(size=(C, dp))

        def run(o, dev):
            t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
            a = dict(th=t(th), g=t(g), thp=t(thp), gp=t(gp), lp=t(lp), lpp=t(lpp), logu=t(logu), zt=t(zt))
            pd = torch.empty((3, D), dtype=torch.float64, device=dev)
            o.precond_pack(t(v), pd)
            out = a["th"] if inplace else torch.full_like(a["th"], float("nan"))
            mask = torch.zeros(C, dtype=torch.uint8, device=dev)
            ret = torch.zeros(C, dtype=torch.float64, device=dev)
            cnt = torch.zeros(1, dtype=torch.int32, device=dev)
            z = a["zt"] if with_z else None
            if gaussian:
                o.mala_step_gaussian(t(lam), a["th"], out, a["thp"], a["lp"], a["lpp"], a["logu"], z, eps, s2, mask, ret, cnt,
                                     precond=pd)
                return [x.cpu().numpy() for x in (out, a["thp"], a["lp"], ret, mask, cnt)]
            o.mala_step_precond(a["th"], out, a["g"], a["thp"], a["gp"], pd, a["lp"], a["lpp"], a["logu"], z, eps, s2, mask,
                                ret, cnt)
            return [x.cpu().numpy() for x in (out, a["g"], a["thp"], a["lp"], ret, mask, cnt)]

        got, want = run(ops, ops.device), run(fake, "cpu")
        for k, (x, y) in enumerate(zip(got, want)):
            assert np.array_equal(x, y), (C, D, inplace, with_z, gaussian, k)
        assert 0 < int(got[-1][0]) < C or C <= 2, (C, D, int(got[-1][0]))


def check_propose_kernel(ops, fake):
    """bk_mala_propose_from_normals_precond in both layouts of z: array_equal."""
    rng = np.random.default_rng(6)
    for C, D in [(1, 1), (63, 3), (65, 33), (257, 64), (300, 130)]:
        v = _wide_v(D, rng)
        th, g, z = rng.normal(size=(D, C)), rng.normal(size=(D, C)), rng.normal(size=(D, C))
        dp = (D + 7) // 8 * 8
        zt = np.zeros((C, dp))
        zt[:, :D] = z.T

        def run(o, dev, chain_major):
            t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
            pd = torch.empty((3, D), dtype=torch.float64, device=dev)
            o.precond_pack(t(v), pd)
            out = torch.full((D, C), float("nan"), dtype=torch.float64, device=dev)
            zz = t(zt)[:, :D].t() if chain_major else t(z)
            o.mala_propose_from_normals_precond(t(th), t(g), zz, pd, out, 0.03, float(np.sqrt(0.06)))
            return out.cpu().numpy()

        for cm in (False, True):
            assert np.array_equal(run(ops, ops.device, cm), run(fake, "cpu", cm)), (C, D, cm)


def check_logq_kernel(ops, fake):
    """bk_mala_logq_precond: array_equal at the quarter seams."""
    rng = np.random.default_rng(7)
    for D in (1, 3, 4, 5, 33, 1024):
        for C in (1, 63, 65):
            v = _wide_v(D, rng)
            th, g, thp, gp = (rng.normal(size=(D, C)) for _ in range(4))

            def run(o, dev):
                t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
                pd = torch.empty((3, D), dtype=torch.float64, device=dev)
                o.precond_pack(t(v), pd)
                f = torch.full((C,), float("nan"), dtype=torch.float64, device=dev)
                r = torch.full((C,), float("nan"), dtype=torch.float64, device=dev)
                o.mala_logq_precond(t(th), t(g), t(thp), t(gp), pd, 0.02, f, r)
                return f.cpu().numpy(), r.cpu().numpy()

            (gf, gr), (wf, wr) = run(ops, ops.device), run(fake, "cpu")
            assert np.array_equal(gf, wf) and np.array_equal(gr, wr), (C, D)


# ---- 6. checkpoint ----------------------------------------------------------------------------------------------------
def check_checkpoint(ops, C, D, **kw):
    """state_dict after draw 3 (preconditioner and a changed epsilon inside), load into a fresh sampler built with neither
    and another seed, draws 4-6 array_equal."""
    lam = np.logspace(0, 1, D)
    v = perturbed_variances(lam)
    a = make(ops, C, D, v, seed=9, **kw)
    run_draws(a, 3)
    a._epsilon = 0.8 * a._epsilon
    sd = a.state_dict()
    ra = run_draws(a, 3)
    b = make(ops, C, D, None, seed=1234, **kw)
    run_draws(b, 1)
    b.load_state_dict(sd)
    assert b._epsilon == 0.8 * eps_for(D) and np.array_equal(b.precond_diag, v)
    rb = run_draws(b, 3)
    for x, y in zip(ra, rb):
        assert np.array_equal(x, y)
    assert np.array_equal(a.rng_state(), b.rng_state())
    # a checkpoint from before the step size and the preconditioner were carried changes nothing ...
    old = dict(sd, meta=dict(sd["meta"], extra={}))
    c = make(ops, C, D, v, seed=9, **kw)
    c.load_state_dict(old)
    assert c._epsilon == eps_for(D) and np.array_equal(c.precond_diag, v)
    # ... and one written explicitly without a preconditioner is refused by a sampler that has one
    none = dict(sd, meta=dict(sd["meta"], extra={"epsilon": 0.1, "precond_diag": None}))
    try:
        make(ops, C, D, v, seed=9, **kw).load_state_dict(none)
    except ValueError as e:
        assert "without precond_diag" in str(e)
    else:
        raise AssertionError("a checkpoint without precond_diag was accepted by a sampler that has one")


# ---- 8. / 9. warmup ---------------------------------------------------------------------------------------------------
def run_warmup(ops, seed, draws=300, C=512, chain_id0=0, before=0, **kw):
    """lam = logspace(0, 4, 32), C chains from N(0, I), epsilon = 1e-5; `before`: draws sampled before warmup()."""
    lam = np.logspace(0, 4, 32)
    s = bk.MALA(bk.DiagGaussian(lam, ops=ops), 1e-5, chains=C, chain_id0=chain_id0, seed=seed, ops=ops, **kw)
    if before:
        run_draws(s, before)
    return s, s.warmup(draws), lam


def warmup_figures(rep, lam):
    v = rep["precond_diag"]
    return float(np.abs(v * lam - 1.0).max()), float(rep["stepsize"]), float(np.mean(rep["alpha"][-20:]))


def check_warmup_report(rep, lam, draws=300):
    """The end-to-end conditions (a NumPy prototype's range over eight seeds / the stand-in's own over eight seeds, in
    brackets): max_d |v_d lam_d - 1| <= 0.10 [0.021-0.039 / 0.025-0.046]; final epsilon >= 0.2 [0.432-0.439 /
    0.434-0.442]; mean alpha of the last 20 draws in [0.50, 0.65] [0.567-0.570 / 0.567-0.571]."""
    dev, eps, last = warmup_figures(rep, lam)
    print(f"MALA warmup: max|v lam - 1| = {dev:.4f}  eps = {eps:.4f}  mean alpha (last 20) = {last:.4f}  "
          f"nan_chains = {rep['nan_chains']}")
    assert len(rep["eps"]) == draws and len(rep["alpha"]) == draws and rep["eps"][0] == 1e-5
    assert rep["window_ends"] == [100, 150, 250] and rep["nan_chains"] == 0
    assert dev <= 0.10
    assert eps >= 0.2
    assert 0.50 <= last <= 0.65


# ---- the stand-in's warmup, recorded -----------------------------------------------------------------------------------
# The NumPy stand-in needs half a minute for warmup(300) at 512 chains (a Python loop per chain and draw in its
# generator).  Its reports for seed 11 are kept in tests/golden/mala_warmup_standin.json: tests/test_mala_adapt_cpu.py checks
# that the stand-in still produces exactly them, tests/test_gpu_mala_adapt.py compares the HIP library with them.
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mala_warmup_standin.json")


def warmup_record(ops, draws, seed=11):
    """warmup(draws) and the two draws that follow -> a JSON-able record (doubles survive repr exactly; the draws as a digest
    of their bytes)."""
    s, rep, _ = run_warmup(ops, seed, draws=draws)
    after = np.ascontiguousarray(run_draws(s, 2)[0])
    rec = dict(rep, precond_diag=[float(x) for x in rep["precond_diag"]])
    rec["after_sha256"] = hashlib.sha256(after.tobytes()).hexdigest()
    return rec


def golden_record(draws):
    with open(GOLDEN) as f:
        return json.load(f)[str(draws)]


def as_report(rec):
    return dict(rec, precond_diag=np.array(rec["precond_diag"]))


if __name__ == "__main__":  # PYTHONPATH=.:bayes-kit_amd python -m tests.mala_adapt_parity: write the golden file from the stand-in
    from tests.fake_ops_mala_adapt import MalaAdaptFakeOps

    with open(GOLDEN, "w") as f:
        json.dump({str(d): warmup_record(MalaAdaptFakeOps(), d) for d in (300, 110)}, f, indent=0)
        f.write("\n")
