"""The three preconditioned HMC entry points (include/bkhip.h: bk_leapfrog_finish_precond, bk_momentum_refresh_precond,
bk_hmc_draw_gaussian_precond) alone, at their row, tile and size seams: input builders, the restated launch choices and checks
that take the kernel library as an argument.  tests/test_precond_kernels_cpu.py runs the checks on the NumPy stand-in
(tests/fake_ops_adapt.AdaptFakeOps) at the small shapes and on stand-ins with one defect planted; tests/test_gpu_precond_kernels.py
runs them on the HIP library.

Inputs.  The variances are v = 10 ** U(-6, 6) per row, packed {v, sqrt(v), 1/v} by ops.precond_pack: with v * lam far from one
a wrong slot of the pack or another association of the products is off by orders of magnitude, not by an ulp.  Momenta are
of order sqrt(v), gradients of order 1/sqrt(v), so that both sides of r = rho + half * (v * g) matter in every row.  State
arrays are [D, C] column views of wider buffers whose surroundings hold NaN (pad 7 / offset 3: never 16-byte aligned with an
even pitch; pad 8 / offset 4: aligned, and an even pitch for an even C) and must still hold NaN after the call.

References, in this order of independence (the assertion messages name the layer):
  1. elementwise outputs (rho_out, the refreshed momentum, theta_out): array_equal to the plain NumPy double expression, every
     product and sum rounded separately (the library is built with -ffp-contract=off);
  2. per-chain sums (kin, kin0, kin1, lp) against np.longdouble: ref = 1/2 sum_d r_d**2 / v_d with r the output checked under 1
     (-1/2 sum lam th**2 for the log density), |got - ref| <= (Dq + 8) * 2**-53 * ref with Dq = ceil(D/4).  Derived, not
     measured: the terms are non-negative, each carries three roundings (1/v and two products; lam*th and th*(..) for lp), a
     quarter's sequential sum adds at most Dq - 1, the three combining additions 3, the 0.5 is exact; 8 instead of 5 covers the
     second-order terms.  Each check prints the largest err / bound it saw (pytest -s);
  3. the same sums array_equal to AdaptFakeOps, which restates the device's order (quarters of Dq rows, each sequential in d,
     combined ((p0+p1)+p2)+p3);
  4. on the device, torch.equal across the forms of one operation (scalar / tile / streaming; rows / plain / non-temporal /
     lane per chain) on the same values, and a pack of ones against the non-preconditioned entry point."""
import numpy as np
import torch

from bayes_kit_amd import _lib
from bayes_kit_amd._engine import make_streams
from tests.fake_ops import FakeOps
from tests.fake_ops_adapt import AdaptFakeOps

U = 2.0 ** -53
NAN = float("nan")
HALF = 0.0275        # the half step of the finish checks
EPS = 0.11           # the step size of the whole-draw checks
LLC_BYTES = 192 << 20

# ---- the shapes ---------------------------------------------------------------------------------------------------------------
FINISH_D = (1, 2, 3, 4, 5, 7, 8, 9, 31, 33, 65, 129)   # empty quarters, ragged last quarter, FIN_UNROLL = 8 and a remainder of 1
FINISH_C = (1, 63, 64, 65, 130)
# (C, D, arrays, form): "distinct" rho / grad / rho_out, "inplace" rho_out is rho_in, "noout" rho_out = None
FINISH_SEAMS = (
    (16320, 257, "distinct", "scalar"),   # C * D = 4,194,240 < 2**22
    (16322, 257, "distinct", "tile"),     # 4,194,754; ragged: 16,322 = 16 * 1020 + 2
    (16610, 256, "distinct", "tile"),     # Dq = 64: exactly one chunk of 64 rows
    (16610, 253, "distinct", "tile"),     # last quarter 61 rows
    (32634, 257, "distinct", "tile"),     # 3 * 8,386,938 * 8 B < 192 MiB; Dq = 65: two chunks
    (32642, 257, "inplace", "tile"),      # two distinct arrays: resident
    (32642, 257, "noout", "tile"),
    (32642, 257, "distinct", "stream"),   # 3 * 8,388,994 * 8 B > 192 MiB
)
REFRESH_LANES_D = (1, 2, 3, 5, 31)        # the two-normals-per-pass loop and its odd tail
REFRESH_LANES_C = (1, 31, 33, 65, 130)
REFRESH_LANES_BIG = (32770, 5)            # rng_block 64 instead of 32
REFRESH_PCG = ((8, 5), (8, 257))
REFRESH_ROWS_D = (32, 33, 40, 63, 64, 65, 120)
REFRESH_ROWS_C = (1, 63, 65, 130)         # ragged nch, rows shorter than 64 double2
REFRESH_PLAIN_D = (121, 128, 129, 257)    # Dq = 31, 32, 33, 65 against the 16-row pieces
REFRESH_PLAIN_C = (63, 65, 130)
REFRESH_PLAIN_BIG = (48960, 257)          # 2 * 12,582,720 * 8 B < 192 MiB
REFRESH_NT = (48962, 257)                 # 2 * 12,583,234 * 8 B > 192 MiB
DRAW_D = (1, 3, 5, 8, 9, 33, 37)
DRAW_C = (1, 63, 65, 130, 16384, 16386)   # the last two on either side of C * 4 <= 256 * 256
DRAW_STEPS = (0, 1, 5)
PHILOX_SEED = 20_240


# ---- the launch choices, restated from csrc/ -------------------------------------------------------------------------------------
def streams_past_llc(elems):
    """bk_streams_past_llc (csrc/bk_common.hpp)."""
    return elems * 8 > LLC_BYTES


def finish_form(C, D, ld, arrays, aligned=True, grad_unit_chain_stride=True, ldg_d=None):
    """finish_level's choice (csrc/bk_integrator.hip) for a call without device-side counts: "scalar" (k_finish), "tile"
    (bkt::k_finish_t) or "stream" (k_finish_v2).  arrays: how many DIFFERENT arrays among rho_in, rho_out, grad;
    aligned: every array given starts on a 16-byte boundary; ldg_d: the gradient's row pitch (None: no gradient)."""
    vec = C % 2 == 0 and ld % 2 == 0 and C * D >= (1 << 22) and aligned
    if ldg_d is not None:
        vec = vec and grad_unit_chain_stride and ldg_d % 2 == 0
    if vec and not streams_past_llc(arrays * C * D):
        return "tile"
    return "stream" if vec else "scalar"


def refresh_form(C, D, philox=True, work_elems=None, arrays=2):
    """bk_momentum_refresh_precond's choice (csrc/bk_rng.hip, refresh_apply_kin_launch): "lanes" (k_refresh, a lane per chain),
    "rows" (k_refresh_apply_kin_rows), "plain" or "nt" (k_refresh_apply_kin<.., NT>).  arrays: the distinct arrays among the
    scratch and the output."""
    dp = (D + 7) // 8 * 8
    if not philox or work_elems is None or D < 32 or work_elems < C * dp:
        return "lanes"
    lds = (64 * (dp + 1) + 256) * 8
    if dp <= 128 and lds <= 65536:
        return "rows"
    return "nt" if streams_past_llc(arrays * C * D) else "plain"


def refresh_rng_block(C):
    """rng_block (csrc/bk_rng.hip): the workgroup of the lane-per-chain kernel."""
    return 32 if C <= 32768 else 64


def draw_block(C):
    """hmc_draw_launch's workgroup (csrc/bk_elementwise.hpp): one wavefront while C * 4 <= 256 * BLOCK, BLOCK = 256."""
    return 64 if C * 4 <= 256 * 256 else 256


# ---- tensors ---------------------------------------------------------------------------------------------------------------------
def say(what, value):
    print(f"[precond-kernels] {what}: max err/bound = {value:.3g}")


def put(ops, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ops.device)


def get(t):
    return t.detach().cpu().numpy().copy()


def nan_vec(ops, n):
    return torch.full((int(n),), NAN, dtype=torch.float64, device=ops.device)


def wide_v(D, rng):
    return 10.0 ** rng.uniform(-6.0, 6.0, size=D)


def pack(ops, v):
    pd = torch.empty((3, len(v)), dtype=torch.float64, device=ops.device)
    ops.precond_pack(put(ops, v), pd)
    return pd


class View:
    """A [D, C] column view `v` of a wider buffer whose surroundings hold NaN; values: what the view holds (default NaN too)."""

    def __init__(self, ops, D, C, aligned=False, values=None):
        pad, self.off = (8, 4) if aligned else (7, 3)
        self.C = C
        self.buf = torch.full((D, C + pad), NAN, dtype=torch.float64, device=ops.device)
        self.v = self.buf[:, self.off:self.off + C]
        if values is not None:
            self.v.copy_(values if torch.is_tensor(values) else put(ops, values))
        assert (self.v.data_ptr() % 16 == 0) == aligned

    def intact(self):
        return bool(torch.isnan(self.buf[:, :self.off]).all()) and bool(torch.isnan(self.buf[:, self.off + self.C:]).all())


def host_subset(C, full_below=1024):
    """The chains whose sums are recomputed on the host: all of them for small C; otherwise at least 512 with the first 16,
    the last 18 (the ragged group of both two-chains-per-lane forms) and both sides of every 128-chain boundary touched."""
    if C <= full_below:
        return np.arange(C)
    s = set(range(16)) | set(range(C - 18, C))
    for k in np.unique(np.linspace(1, (C - 1) // 128, 9).astype(np.int64)):
        s |= set(range(128 * int(k) - 32, min(C, 128 * int(k) + 32)))
    for c in list(s):
        if c % 128 == 127 and c + 1 < C:
            s.add(c + 1)
        if c % 128 == 0 and c > 0:
            s.add(c - 1)
    return np.array(sorted(s), dtype=np.int64)


def cols(t, idx):
    """columns idx of a device [D, C] tensor (a per-chain vector: entries idx), on the host."""
    i = torch.from_numpy(idx).to(t.device)
    return get(t.index_select(t.dim() - 1, i))


# ---- the layers -------------------------------------------------------------------------------------------------------------------
def kin_terms(r, v):
    rl = r.astype(np.longdouble)
    return rl * rl / v.astype(np.longdouble)[:, None]


def lp_terms(th, lam):
    tl = th.astype(np.longdouble)
    return tl * tl if lam is None else lam.astype(np.longdouble)[:, None] * tl * tl


def layer1(got, want, what):
    assert np.array_equal(got, want), f"layer 1 (elementwise, NumPy double): {what}"


def layer2(got, terms, what):
    """|got - ref| <= (Dq + 8) * 2**-53 * ref, ref = 1/2 sum of the non-negative long-double terms [D, n] -> max err / bound."""
    D = terms.shape[0]
    Dq = (D + 3) // 4
    ref = np.longdouble(0.5) * terms.sum(axis=0)
    assert np.all(np.isfinite(got)), f"layer 2 (long double): {what}: non-finite sum"
    err = np.abs(got.astype(np.longdouble) - ref)
    bound = (Dq + 8) * np.longdouble(U) * ref
    bad = err > bound
    worst = float(np.max(err[bad] / np.maximum(bound[bad], np.finfo(np.longdouble).tiny))) if bad.any() else 0.0
    assert not bad.any(), (f"layer 2 (long double, bound (Dq + 8) u): {what}: worst err / bound {worst:.3g}, "
                           f"{int(bad.sum())} chains over, first {int(np.flatnonzero(bad)[0])}")
    pos = bound > 0
    return float(np.max(err[pos] / bound[pos])) if pos.any() else 0.0


def layer3(got, want, what):
    assert np.array_equal(got, want), f"layer 3 (the stand-in's summation order): {what}"


def cpu_pack(v):
    pd = torch.empty((3, len(v)), dtype=torch.float64)
    AdaptFakeOps().precond_pack(torch.from_numpy(v.copy()), pd)
    return pd


# ---- A. bk_leapfrog_finish_precond -------------------------------------------------------------------------------------------------
def finish_inputs(C, D, rng):
    v = wide_v(D, rng)
    sd = np.sqrt(v)
    return v, rng.normal(size=(D, C)) * sd[:, None], rng.normal(size=(D, C)) / sd[:, None]


def finish_want(rho, g, v, negate):
    r = rho.copy() if g is None else rho + HALF * (v[:, None] * g)
    return -r if negate else r


def grad_layout(ops, g, layout):
    """The three gradient layouts of test_kick_drift_bit_exact: the state layout, a row-major (C, D) tensor seen transposed,
    arbitrary odd strides."""
    D, C = g.shape
    if layout == "chain":
        return View(ops, D, C, values=g).v
    if layout == "dim":
        return put(ops, g.T).t()
    big = torch.zeros((D * 2 + 1, C * 3 + 1), dtype=torch.float64, device=ops.device)
    gd = big[1::2, 1::3][:D, :C]
    gd.copy_(put(ops, g))
    return gd


def check_finish_small(ops, C, D):
    """Every argument form of the call at one small shape (the scalar kernel): layers 1 to 3, the guards, and a pack of ones
    against leapfrog_finish(metric=None) -> max err / bound of layer 2."""
    rng = np.random.default_rng(7000 + 131 * D + C)
    v, rho, g = finish_inputs(C, D, rng)
    pd, fake, pd_f = pack(ops, v), AdaptFakeOps(), cpu_pack(v)
    worst = 0.0
    for layout in ("chain", "dim", "odd", None):
        gd = None if layout is None else grad_layout(ops, g, layout)
        for negate in (False, True):
            want = finish_want(rho, None if layout is None else g, v, negate)
            kin_f = torch.empty(C, dtype=torch.float64)
            fake.leapfrog_finish_precond(torch.from_numpy(rho.copy()), None, None if layout is None else torch.from_numpy(g.copy()),
                                         pd_f, HALF, negate, kin_f)
            for out_mode in ("separate", "inplace", "none"):
                for with_kin in (True, False):
                    if out_mode == "none" and not with_kin:
                        continue
                    what = f"finish C={C} D={D} grad={layout} negate={negate} rho_out={out_mode} kin={with_kin}"
                    rin = View(ops, D, C, values=rho)
                    out = {"none": None, "separate": View(ops, D, C), "inplace": rin}[out_mode]
                    kin = nan_vec(ops, C) if with_kin else None
                    ops.leapfrog_finish_precond(rin.v, None if out is None else out.v, gd, pd, HALF, negate, kin)
                    assert rin.intact() and (out is None or out.intact()), f"guard: {what}"
                    if out_mode != "inplace":
                        assert np.array_equal(get(rin.v), rho), f"rho_in changed: {what}"
                    r = want if out is None else get(out.v)
                    layer1(r, want, what)
                    if with_kin:
                        worst = max(worst, layer2(get(kin), kin_terms(r, v), what))
                        layer3(get(kin), kin_f.numpy(), what)
    # a pack of ones is the non-preconditioned call
    ones = pack(ops, np.ones(D))
    for negate in (False, True):
        a, b = View(ops, D, C), View(ops, D, C)
        ka, kb = nan_vec(ops, C), nan_vec(ops, C)
        rin, gin = View(ops, D, C, values=rho), View(ops, D, C, values=g)
        ops.leapfrog_finish_precond(rin.v, a.v, gin.v, ones, HALF, negate, ka)
        ops.leapfrog_finish(rin.v, b.v, gin.v, None, HALF, negate, kb)
        assert torch.equal(a.v, b.v) and torch.equal(ka, kb), f"layer 4 (pack of ones): finish C={C} D={D} negate={negate}"
    say(f"finish C={C} D={D}", worst)
    return worst


def check_finish_seam(ops, C, D, arrays, negate=False):
    """One row of FINISH_SEAMS: the call on aligned arrays (the form the row names), on an unaligned view of the same values
    (the scalar kernel), with a pack of ones and through leapfrog_finish(metric=None) -- torch.equal for ALL chains on the
    device; layers 1 to 3 on the host for host_subset(C) -> max err / bound of layer 2."""
    rng = np.random.default_rng(9000 + D + C)
    v, rho, g = finish_inputs(C, D, rng)
    pd, ones = pack(ops, v), pack(ops, np.ones(D))
    what = f"finish seam C={C} D={D} arrays={arrays}"
    g_al = View(ops, D, C, aligned=True, values=g)
    g_un = View(ops, D, C, aligned=False, values=g_al.v)
    rho_d = put(ops, rho)

    def run(fn, aligned, gview):
        rin = View(ops, D, C, aligned=aligned, values=rho_d)
        out = {"distinct": View(ops, D, C, aligned=aligned), "inplace": rin, "noout": None}[arrays]
        kin = nan_vec(ops, C)
        fn(rin.v, None if out is None else out.v, gview.v, kin)
        assert rin.intact() and gview.intact() and (out is None or out.intact()), f"guard: {what} aligned={aligned}"
        return kin, (None if out is None else out.v)

    pre = lambda p: (lambda r, o, gg, k: ops.leapfrog_finish_precond(r, o, gg, p, HALF, negate, k))  # noqa: E731
    kin_a, r_a = run(pre(pd), True, g_al)
    kin_u, r_u = run(pre(pd), False, g_un)
    assert torch.equal(kin_a, kin_u), f"layer 4 (aligned against unaligned): kin: {what}"
    assert r_a is None or torch.equal(r_a, r_u), f"layer 4 (aligned against unaligned): rho_out: {what}"
    idx = host_subset(C)
    assert len(idx) >= min(C, 512)
    kin_h = cols(kin_a, idx)
    want = finish_want(rho[:, idx], g[:, idx], v, negate)
    r_h = want if r_a is None else cols(r_a, idx)
    del r_u, kin_u
    kin_1, r_1 = run(pre(ones), True, g_al)
    kin_0, r_0 = run(lambda r, o, gg, k: ops.leapfrog_finish(r, o, gg, None, HALF, negate, k), True, g_al)
    assert torch.equal(kin_1, kin_0), f"layer 4 (pack of ones): kin: {what}"
    assert r_1 is None or torch.equal(r_1, r_0), f"layer 4 (pack of ones): rho_out: {what}"
    layer1(r_h, want, what)
    worst = layer2(kin_h, kin_terms(r_h, v), what)
    kin_f = torch.empty(len(idx), dtype=torch.float64)
    AdaptFakeOps().leapfrog_finish_precond(torch.from_numpy(np.ascontiguousarray(rho[:, idx])), None,
                                           torch.from_numpy(np.ascontiguousarray(g[:, idx])), cpu_pack(v), HALF, negate, kin_f)
    layer3(kin_h, kin_f.numpy(), what)
    say(what, worst)
    return worst


# ---- B. bk_momentum_refresh_precond -------------------------------------------------------------------------------------------------
NAMED_CHAINS = (0, 1, 31, 32, 63, 64)


def refresh_streams(ops, C, D, pcg):
    """(kind, stream table, a function c -> fresh NumPy generator of chain c)."""
    if pcg:
        kind, st = make_streams([np.random.default_rng(100 + c) for c in range(C)], C, 0, False, ops.device)
        assert kind == _lib.RNG_PCG64
        return kind, st, lambda c: np.random.default_rng(100 + c)
    seed = PHILOX_SEED + D
    kind, st = make_streams(seed, C, 0, False, ops.device)
    return kind, st, lambda c: np.random.Generator(np.random.Philox(key=[seed, c]))


def check_refresh(ops, C, D, pcg=False, use_work=True):
    """One shape of the refresh: the normals are those of the plain ops.momentum_refresh on a clone of the stream table (pinned
    to NumPy bit for bit elsewhere), out == 0.0 + sqrt(v) * z for all chains on the device, the two tables equal afterwards;
    the named chains directly against NumPy's generators; the kinetic energy under layers 2 and 3; with scratch one element
    too short the lane-per-chain kernel gives the same bits -> max err / bound of layer 2."""
    rng = np.random.default_rng(11000 + 131 * D + C)
    v = wide_v(D, rng)
    sd = np.sqrt(v)
    pd = pack(ops, v)
    what = f"refresh C={C} D={D} {'pcg64' if pcg else 'philox'} work={use_work}"
    kind, st0, gen_of = refresh_streams(ops, C, D, pcg)
    work = ops.refresh_work(C, D) if use_work else None
    st, st_z = st0.clone(), st0.clone()
    out, z = View(ops, D, C), View(ops, D, C)
    kin = nan_vec(ops, C)
    ops.momentum_refresh_precond(kind, st, out.v, pd, kin, work)
    ops.momentum_refresh(kind, st_z, None, 0.0, 1.0, z.v, None, None, None, work)
    assert out.intact() and z.intact(), f"guard: {what}"
    assert torch.equal(out.v, pd[1][:, None] * z.v + 0.0), f"layer 1 (elementwise, all chains on the device): {what}"
    assert torch.equal(st, st_z) and not torch.equal(st, st0), f"stream tables: {what}"
    for c in sorted({c for c in NAMED_CHAINS + (C - 1,) if c < C}):
        layer1(get(out.v[:, c]), 0.0 + sd * gen_of(c).standard_normal(D), f"{what} chain {c} against NumPy's generator")
    idx = host_subset(C)
    o, k = cols(out.v, idx), cols(kin, idx)
    worst = layer2(k, kin_terms(o, v), what)
    fake = AdaptFakeOps()
    st_f = torch.from_numpy(np.ascontiguousarray(cols(st0, idx)))
    out_f, kin_f = torch.empty((D, len(idx)), dtype=torch.float64), torch.empty(len(idx), dtype=torch.float64)
    fake.momentum_refresh_precond(kind, st_f, out_f, cpu_pack(v), kin_f)
    layer1(o, out_f.numpy(), f"{what} against the stand-in's generators")
    layer3(k, kin_f.numpy(), what)
    assert np.array_equal(st_f.numpy(), cols(st, idx)), f"stream positions: {what}"
    if work is not None and D >= 32 and not pcg:
        # scratch one element too short: the lane-per-chain kernel, the same bits
        st2, out2, kin2 = st0.clone(), View(ops, D, C), nan_vec(ops, C)
        ops.momentum_refresh_precond(kind, st2, out2.v, pd, kin2, work[:work.numel() - 1])
        assert out2.intact() and torch.equal(out2.v, out.v) and torch.equal(kin2, kin) and torch.equal(st2, st), \
            f"layer 4 (scratch too short: lane per chain): {what}"
    say(what, worst)
    return worst


# ---- C. bk_hmc_draw_gaussian_precond ------------------------------------------------------------------------------------------------
def check_draw(ops, C, D, all_steps=DRAW_STEPS):
    """The whole-draw kernel at one shape, steps in DRAW_STEPS, lam given and None, momentum from rho_in and from chain-major
    normals: layers 1 to 3, the three sums torch.equal to leapfrog_finish_precond / target_grad on the same arrays, the folded
    accept test equal to mh_accept on those energies -> max err / bound of layer 2."""
    rng = np.random.default_rng(13000 + 131 * D + C)
    v = wide_v(D, rng)
    sd = np.sqrt(v)
    lam_np = rng.uniform(0.5, 2.0, size=D) / v
    th = rng.normal(size=(D, C)) * sd[:, None]
    rho = rng.normal(size=(D, C)) * sd[:, None]
    ldz = (D + 7) // 8 * 8
    zt_np = np.full((C, ldz), NAN)
    zt_np[:, :D] = rng.normal(size=(C, D))
    pd, pd_f, fake, plain = pack(ops, v), cpu_pack(v), AdaptFakeOps(), FakeOps()
    zt = put(ops, zt_np)
    f64 = dict(dtype=torch.float64, device=ops.device)
    worst = 0.0
    for steps in all_steps:
        for use_lam in (True, False):
            lam = lam_np if use_lam else None
            lam_d = put(ops, lam_np) if use_lam else None
            lam_f = torch.from_numpy(lam_np.copy()) if use_lam else None
            tkind = "diag_gaussian" if use_lam else "iso_gaussian"
            for use_zt in (True, False):
                what = f"draw C={C} D={D} steps={steps} lam={use_lam} zt={use_zt}"
                r0 = 0.0 + sd[:, None] * zt_np[:, :D].T if use_zt else rho
                th_ref, r1 = torch.empty((D, C), dtype=torch.float64), torch.empty((D, C), dtype=torch.float64)
                plain.hmc_trajectory_gaussian(torch.from_numpy(th.copy()), th_ref, torch.from_numpy(np.ascontiguousarray(r0)), r1,
                                              lam_f, torch.from_numpy(v.copy()), EPS, steps)
                th_ref, r1 = th_ref.numpy(), r1.numpy()
                tin, tout = View(ops, D, C, values=th), View(ops, D, C)
                rin = None if use_zt else View(ops, D, C, values=rho)
                part = torch.full((12 * C,), NAN, **f64)
                k0, k1, lp = (nan_vec(ops, C) for _ in range(3))
                args = (tin.v, tout.v, None if use_zt else rin.v, zt if use_zt else None, lam_d, None, EPS, steps, part)
                ops.hmc_draw_gaussian(*args, k0, k1, lp, precond=pd)
                assert tin.intact() and tout.intact() and (rin is None or rin.intact()), f"guard: {what}"
                assert np.array_equal(get(tin.v), th), f"theta_in changed: {what}"
                layer1(get(tout.v), th_ref, what)
                g0, g1, gl = get(k0), get(k1), get(lp)
                worst = max(worst, layer2(g0, kin_terms(r0, v), what + " kin0"), layer2(g1, kin_terms(r1, v), what + " kin1"),
                            layer2(-gl, lp_terms(th_ref, lam), what + " lp"))
                tf = torch.empty((D, C), dtype=torch.float64)
                f0, f1, fl = (torch.empty(C, dtype=torch.float64) for _ in range(3))
                fake.hmc_draw_gaussian(torch.from_numpy(th.copy()), tf, None if use_zt else torch.from_numpy(rho.copy()),
                                       torch.from_numpy(zt_np.copy()) if use_zt else None, lam_f, None, EPS, steps, None, f0, f1, fl,
                                       precond=pd_f)
                layer3(g0, f0.numpy(), what + " kin0")
                layer3(g1, f1.numpy(), what + " kin1")
                layer3(gl, fl.numpy(), what + " lp")
                # the reduction kernels on the same arrays
                q0, q1, ql = (nan_vec(ops, C) for _ in range(3))
                ops.leapfrog_finish_precond(put(ops, r0), None, None, pd, 0.0, False, q0)
                ops.leapfrog_finish_precond(put(ops, r1), None, None, pd, 0.0, False, q1)
                ops.target_grad(tkind, lam_d, tout.v, None, ql)
                assert torch.equal(k0, q0) and torch.equal(k1, q1) and torch.equal(lp, ql), \
                    f"layer 4 (the reduction kernels' values): {what}"
                # the folded accept test (kin0 = None) against mh_accept on those energies; energy errors of order one (of
                # order 1e-12 of the energies where the unstable iso trajectories make them astronomically large)
                mag = np.abs(gl) + np.abs(g0) + np.abs(g1)
                lp_cur = put(ops, ((gl - g1) + g0) + rng.normal(size=C) * np.maximum(1.0, 1e-12 * mag))
                logu = put(ops, np.log(rng.uniform(size=C)))
                la, lb = lp_cur.clone(), lp_cur.clone()
                ma, mb = (torch.zeros(C, dtype=torch.uint8, device=ops.device) for _ in range(2))
                ra, rb = nan_vec(ops, C), nan_vec(ops, C)
                na, nb = (torch.zeros(1, dtype=torch.int32, device=ops.device) for _ in range(2))
                ops.mh_accept(_lib.ACCEPT_HMC, la, k0, lp, k1, logu, ma, ra, na)
                k1b, lpb, tout2 = nan_vec(ops, C), nan_vec(ops, C), View(ops, D, C)
                args = (tin.v, tout2.v) + args[2:]
                ops.hmc_draw_gaussian(*args, None, k1b, lpb, accept=(lb, logu, mb, rb, nb), precond=pd)
                assert torch.equal(tout2.v, tout.v) and torch.equal(k1b, k1) and torch.equal(lpb, lp), f"kin0 = None: {what}"
                assert torch.equal(ma, mb) and torch.equal(ra, rb) and torch.equal(la, lb) and int(na) == int(nb), \
                    f"folded accept test: {what}"
                assert C < 63 or 0 < int(nb) < C, f"accept count {int(nb)} of {C}: {what}"
    say(f"draw C={C} D={D}", worst)
    return worst
