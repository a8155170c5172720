"""The plain and preconditioned MALA kernels alone (include/bkhip.h: bk_mala_step, bk_mala_step_precond, bk_mala_step_gaussian with and
without lam, bk_mala_step_gaussian_precond, bk_mala_logq, bk_mala_propose_from_normals, bk_mala_propose), at their slot, block,
pitch and offset seams: input builders, the launch choices restated from csrc/ and checks that take the kernel library as an
argument.  tests/test_mala_kernels_cpu.py runs the checks on the NumPy stand-in (tests/fake_ops_mala_adapt.MalaAdaptFakeOps, the
device's summation order) at the small shapes and on stand-ins with one defect planted; tests/test_gpu_mala_kernels.py runs
them on the HIP library.

Planted thresholds.  The per-chain sums tf, tr of the step kernels leave the kernel only as a decision
log_u < (lp' - lp) + (k tr - k tf).  Here the right-hand side T is computed in NumPy in the device's order (step_sum: a thread's
slots in sequence, a xor tree over each group of 8 rows, the 8 groups in order; products and sums rounded separately, the library
is built with -ffp-contract=off) and log_u is PLANTED on it: log_u = T on even chains (strict <: refused), nextafter(T, -inf) on
odd chains (accepted).  A sum that differs in its last bit flips about half of the chains it touches.

The restatement is held against np.longdouble: |T - T_long| <= (E + 12) 2**-53 (|k| (sum xr^2 + sum xf^2) + |lp' - lp|).  Derived:
the terms are non-negative; one rounding per product, E - 1 slot additions, 3 tree levels, 7 group additions, then k *, the two
differences and the final sum.  Each check prints the largest err / bound it saw (pytest -s).

Guard cells.  State arrays are [D, C] views (pitch ld = C + pad, a column offset; both even, so the views stay 16-byte aligned) of
flat buffers of 64 E + 1 rows -- every row a thread of the step kernel can form an address for -- whose cells outside the view
hold a NaN of a fixed payload and are compared as int64 after the call: a store that the range check should have dropped, or
that went to a pad column, lands in one of them."""
import numpy as np
import torch

from bayes_kit_amd import _lib
from bayes_kit_amd._engine import _bitgen_words, make_streams
from tests.fake_ops_adapt import quarter_sum
from tests.fake_ops_mala_adapt import step_slots, step_sum

U = 2.0 ** -53
LLC_BYTES = 192 << 20
SENT = np.int64(0x7FF8_0000_0BAD_CAFE)  # a quiet NaN with a payload nothing computes
KINDS = ("step", "step_precond", "gauss", "gauss_iso", "gauss_precond")

# ---- the shapes ---------------------------------------------------------------------------------------------------------------
PLANT_D = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024)   # the E seams and a single group
PLANT_C = (18, 130)                                    # 2 and 9 blocks, both ragged
PLANT_C_AT_65 = (2, 14, 16, 18, 112, 128, 130, 254, 258)   # 1, 1, 1, 2, 7, 8, 9, 16, 17 blocks; ragged last block and not
LAYOUT_D = (1, 33, 129, 1000)
LAYOUT_C = (2, 18, 130)
LAYOUTS = ((0, 0, 0), (2, 2, 1), (6, 0, 2), (0, 2, 2), (6, 2, 0))   # (pad, column offset, which ldz)
NONFINITE_SHAPES = ((18, 65), (34, 513))
# (kind, C, D, streams): on either side of 6 C D 8 > 192 MiB (4 C D 8 for the separable kernel), every E
SEAMS = tuple((k, C + 2 * s, D, bool(s)) for k, base in (("step", 4194304), ("gauss", 6291456))
              for D in (128, 256, 512, 1024) for C in (base // D,) for s in (0, 1))
LOGQ_D = (1, 3, 4, 5, 33, 1024)
LOGQ_C = (1, 63, 65)
PROPOSE_Z_SHAPES = ((1, 1), (63, 3), (65, 33), (257, 64), (300, 130))   # (C, D)
PROPOSE_SHAPES = ((1, 1), (33, 2), (65, 5), (130, 33))


# ---- the launch choices, restated from csrc/ ------------------------------------------------------------------------------------
def streams_past_llc(elems):
    """bk_streams_past_llc (csrc/bk_common.hpp)."""
    return elems * 8 > LLC_BYTES


def separable(kind):
    return kind.startswith("gauss")


def step_form(kind, C, D):
    """mala_step_launch / mala_step_sep_launch (csrc/bk_mala.hip, csrc/bk_mala_step.hpp) -> (E, blocks, nt)."""
    arrays = 4 if separable(kind) else 6
    return step_slots(D), -(-C // 16), streams_past_llc(arrays * C * D)


def xcd_map(blocks):
    """The chain block that workgroup b of a launch of `blocks` walks (k_mala_step: per = blocks / 8, the first 8 per
    workgroups are dealt round robin to contiguous ranges, the rest keep their index)."""
    per = blocks // 8
    return [(b % 8) * per + b // 8 if b < per * 8 else b for b in range(blocks)]


def step_offsets(C, D, ld, ldz=None):
    """Every byte offset the step kernels form for (C, D, ld[, ldz]) with the width of the access added, and the two
    num_records, as Python integers (csrc/bk_mala.hip: voff + e * slotb, woff = nbytes for a pair past C, zoff + 1024 k) ->
    the largest."""
    E = step_slots(D)
    nbytes = ((D - 1) * ld + C) * 8
    slotb = 64 * ld * 8
    voff = (63 * ld + (C - 2)) * 8            # r = 63, the last pair
    out = [nbytes, voff + (E - 1) * slotb + 16, nbytes + (E - 1) * slotb + 16]
    if ldz is not None:
        zoff = (C - 1) * ldz * 8 + 16 * 63
        out += [((C - 1) * ldz + D) * 8, zoff + 1024 * (E // 2 - 1) + 16]
    return max(out)


# ---- tensors ---------------------------------------------------------------------------------------------------------------------
def say(what, value):
    print(f"[mala-kernels] {what}: max err/bound = {value:.3g}")


def put(ops, a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(ops.device)   # (a copy on the CPU too: calls write in place)


def get(t):
    return t.detach().cpu().numpy().copy()


def bits(a):
    return np.ascontiguousarray(a).view(np.int64) if a.dtype == np.float64 else a


def same(a, b):
    """array_equal on the bits (a NaN equals itself, -0.0 is not 0.0)."""
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


class View:
    """A [D, C] view (pitch ld, column offset off) of a flat buffer of `rows` rows + off cells; every cell outside holds SENT."""

    def __init__(self, ops, values, ld, off, rows):
        D, C = values.shape
        n = rows * ld + off
        buf = np.full(n, SENT, dtype=np.int64).view(np.float64)
        self.inside = np.zeros(n, dtype=bool)
        for d in range(D):
            buf[off + d * ld: off + d * ld + C] = values[d]
            self.inside[off + d * ld: off + d * ld + C] = True
        self.buf = torch.from_numpy(buf).to(ops.device)
        self.v = self.buf.as_strided((D, C), (ld, 1), off)

    def guards_intact(self):
        return bool(np.all(get(self.buf).view(np.int64)[~self.inside] == SENT))


def ldz_choices(D):
    d8 = (D + 7) // 8 * 8
    return ((D + 1) // 2 * 2, d8, d8 + 6)


# ---- inputs and the NumPy statement of a step -----------------------------------------------------------------------------------
def make_inputs(kind, C, D, seed=0):
    """Inputs of a step as NumPy arrays.  v = 10 ** U(-6, 6) (preconditioned kinds), state of order sqrt(v), the gradients those of
    N(0, 1 / lam) -- what the separable kernels recompute -- with lam = U(0.5, 2) / v (1 for the isotropic kind), the
    proposal a MALA proposal from the state; eps = 0.3 / D."""
    g = np.random.default_rng([seed, C, D, KINDS.index(kind)])
    eps = 0.3 / D
    s2 = float(np.sqrt(2 * eps))
    v = 10.0 ** g.uniform(-6.0, 6.0, size=D) if kind.endswith("precond") else np.ones(D)
    lam = np.ones(D) if kind == "gauss_iso" else g.uniform(0.5, 2.0, size=D) / v
    th = g.normal(size=(D, C)) * np.sqrt(v)[:, None]
    gr = -(lam[:, None] * th)
    thp = (th + eps * (v[:, None] * gr)) + s2 * (np.sqrt(v)[:, None] * g.normal(size=(D, C)))
    lp = g.normal(size=C)
    return dict(kind=kind, C=C, D=D, eps=eps, s2=s2, v=v if kind.endswith("precond") else None,
                lam=None if kind == "gauss_iso" else lam, th=th, thp=thp, lp=lp, lpp=lp + 0.5 * g.normal(size=C),
                z=g.normal(size=(C, D)))


def grads(inp, th):
    """The gradient the separable kernels recompute (and the model's op would store): -(lam * th), -th without lam."""
    return -th if inp["lam"] is None else -(inp["lam"][:, None] * th)


def residual_terms(inp, pack, dtype=np.float64):
    """-> the forward / reverse terms [D, C] summed per chain; pack: {v, sqrt(v), 1/v} as the device packed it, or None.
    dtype = np.longdouble: the squares (and their weights) of the same double residuals in extended precision."""
    th, thp, eps = inp["th"], inp["thp"], inp["eps"]
    g, gp = inp.get("g", None), inp.get("gp", None)
    g = grads(inp, th) if g is None else g
    gp = grads(inp, thp) if gp is None else gp
    with np.errstate(invalid="ignore", over="ignore"):
        if pack is None:
            xf = ((thp - th) - eps * g).astype(dtype)
            xr = ((th - thp) - eps * gp).astype(dtype)
            return xf * xf, xr * xr
        v, iv = pack[0][:, None], pack[2][:, None].astype(dtype)
        xf = ((thp - th) - eps * (v * g)).astype(dtype)
        xr = ((th - thp) - eps * (v * gp)).astype(dtype)
        return (xf * xf) * iv, (xr * xr) * iv


def threshold(inp, pack):
    """T_c = (lp' - lp) + (k tr - k tf) in the device's order -> (T, err / bound against np.longdouble)."""
    k = -0.25 / inp["eps"]
    tf, tr = residual_terms(inp, pack)
    with np.errstate(invalid="ignore", over="ignore"):
        T = (inp["lpp"] - inp["lp"]) + (k * step_sum(tr) - k * step_sum(tf))
        lf, lr = residual_terms(inp, pack, np.longdouble)
        dl = inp["lpp"].astype(np.longdouble) - inp["lp"].astype(np.longdouble)
        ref = dl + np.longdouble(k) * (lr.sum(axis=0) - lf.sum(axis=0))
        scale = abs(k) * (lr.sum(axis=0) + lf.sum(axis=0)) + np.abs(dl)
        bound = (step_slots(inp["D"]) + 12) * U * scale
        ok = np.isfinite(T)
        ratio = float(np.max(np.abs(T[ok] - ref[ok]) / bound[ok])) if ok.any() else 0.0
    return T, ratio


def planted_log_u(T):
    lu = T.copy()
    lu[1::2] = np.nextafter(T[1::2], -np.inf)
    return lu


def expected(inp, pack, log_u, count0, with_z=True):
    """The NumPy statement of the step -> dict of what every output must hold."""
    T, _ = threshold(inp, pack)
    with np.errstate(invalid="ignore"):
        acc = log_u < T
    th, thp = inp["th"], inp["thp"]
    g = inp["g"] if "g" in inp else grads(inp, th)
    gp = inp["gp"] if "gp" in inp else grads(inp, thp)
    out = np.where(acc[None, :], thp, th)
    gn = np.where(acc[None, :], gp, g)
    lp = np.where(acc, inp["lpp"], inp["lp"])
    z = inp["z"].T
    with np.errstate(invalid="ignore", over="ignore"):
        if pack is None:
            nxt = (out + inp["eps"] * gn) + inp["s2"] * z
        else:
            nxt = (out + inp["eps"] * (pack[0][:, None] * gn)) + inp["s2"] * (pack[1][:, None] * z)
    return dict(out=out, g=gn, thp=nxt if with_z else thp, lp=lp, ret=lp, mask=acc.astype(np.uint8),
                count=np.array([count0 + int(acc.sum())], dtype=np.int32), acc=acc)


def device_pack(ops, inp):
    if inp["v"] is None:
        return None, None
    pd = torch.empty((3, inp["D"]), dtype=torch.float64, device=ops.device)
    ops.precond_pack(put(ops, inp["v"]), pd)
    return pd, get(pd)


def run_step(ops, inp, log_u, pd, layout=None, inplace=False, with_z=True, drop=(), count0=0, cols=None, bufs=None):
    """One call of the entry point of inp["kind"].  layout: None (contiguous arrays, zt [C, (D+7)//8*8]) or (pad, offset, which
    ldz) for guarded views.  drop: names among mask / ret / count passed as None.  cols = (lo, hi): the call on that column
    range of the buffers `bufs` of an earlier call.  -> (dict of outputs as NumPy arrays, the buffers)."""
    kind, C, D = inp["kind"], inp["C"], inp["D"]
    opaque = not separable(kind)
    if bufs is None:
        if layout is None:
            ld, off, rows, ldz, zrows = C, 0, D, (D + 7) // 8 * 8, C
        else:
            pad, off, zk = layout
            ld, rows, ldz, zrows = C + pad, 64 * step_slots(D) + 1, ldz_choices(D)[zk], C + 1
        arrays = dict(th=inp["th"], thp=inp["thp"])
        if opaque:
            arrays.update(g=inp["g"] if "g" in inp else grads(inp, inp["th"]),
                          gp=inp["gp"] if "gp" in inp else grads(inp, inp["thp"]))
        if not inplace:
            arrays["out"] = np.full((D, C), np.nan)
        bufs = {k: View(ops, a, ld, off, rows) for k, a in arrays.items()}
        zv = np.full(zrows * ldz, SENT, dtype=np.int64).view(np.float64).reshape(zrows, ldz)
        zv[:C, :D] = inp["z"]
        bufs["zt0"] = zv.copy()
        bufs["zt"] = put(ops, zv)
        bufs["lp"], bufs["lpp"], bufs["logu"] = put(ops, inp["lp"]), put(ops, inp["lpp"]), put(ops, log_u)
        bufs["mask"] = torch.full((C,), 9, dtype=torch.uint8, device=ops.device)
        bufs["ret"] = torch.full((C,), float("nan"), dtype=torch.float64, device=ops.device)
        bufs["count"] = torch.full((1,), count0, dtype=torch.int32, device=ops.device)
        bufs["lam"] = None if inp["lam"] is None else put(ops, inp["lam"])
    lo, hi = (0, C) if cols is None else cols
    a = {k: bufs[k].v[:, lo:hi] for k in ("th", "thp", "g", "gp", "out") if k in bufs}
    out = a["th"] if "out" not in a else a["out"]
    vec = {k: bufs[k][lo:hi] for k in ("lp", "lpp", "logu", "mask", "ret")}
    mask, ret = (None if k in drop else vec[k] for k in ("mask", "ret"))
    count = None if "count" in drop else bufs["count"]
    z = bufs["zt"][lo:hi] if with_z else None
    eps, s2 = inp["eps"], inp["s2"]
    if kind == "step":
        ops.mala_step(a["th"], out, a["g"], a["thp"], a["gp"], vec["lp"], vec["lpp"], vec["logu"], z, eps, s2, mask, ret, count)
    elif kind == "step_precond":
        ops.mala_step_precond(a["th"], out, a["g"], a["thp"], a["gp"], pd, vec["lp"], vec["lpp"], vec["logu"], z, eps, s2, mask,
                              ret, count)
    elif pd is None:
        ops.mala_step_gaussian(bufs["lam"], a["th"], out, a["thp"], vec["lp"], vec["lpp"], vec["logu"], z, eps, s2, mask, ret,
                               count)
    else:
        ops.mala_step_gaussian(bufs["lam"], a["th"], out, a["thp"], vec["lp"], vec["lpp"], vec["logu"], z, eps, s2, mask, ret,
                               count, precond=pd)
    return collect(bufs), bufs


def collect(bufs):
    res = dict(out=get(bufs["out"].v if "out" in bufs else bufs["th"].v), thp=get(bufs["thp"].v), lp=get(bufs["lp"]),
               ret=get(bufs["ret"]), mask=get(bufs["mask"]), count=get(bufs["count"]))
    if "g" in bufs:
        res["g"] = get(bufs["g"].v)
    return res


def guards_intact(bufs):
    for k in ("th", "thp", "g", "gp", "out"):
        if k in bufs and not bufs[k].guards_intact():
            return False, k
    return same(get(bufs["zt"]), bufs["zt0"]), "zt"


def assert_outputs(got, want, tag, skip=()):
    for k in ("mask", "ret", "lp", "count", "out", "g", "thp"):
        if k in got and k not in skip:
            assert same(got[k], want[k]), tag + (k,)


# ---- A. planted thresholds ---------------------------------------------------------------------------------------------------------
def check_planted(ops, kind, C, D):
    """Every chain's decision sits one ulp beside its threshold: mask, ret, lp, count, the selected state, the selected gradient
    and the next proposal array_equal to the NumPy statement.  -> err / bound of the statement against np.longdouble."""
    inp = make_inputs(kind, C, D)
    pd, pack = device_pack(ops, inp)
    T, ratio = threshold(inp, pack)
    assert np.all(np.isfinite(T)) and ratio <= 1.0, (kind, C, D, ratio)
    log_u = planted_log_u(T)
    want = expected(inp, pack, log_u, 0)
    assert np.array_equal(want["acc"], np.arange(C) % 2 == 1)
    got, _ = run_step(ops, inp, log_u, pd)
    assert_outputs(got, want, (kind, C, D))
    return ratio


# ---- B. pitch, offset and guard cells ----------------------------------------------------------------------------------------------
def check_layouts(ops, kind, C, D):
    """Guarded views at every layout: sentinels unchanged, no NaN in an output, the outputs those of the contiguous call bit for
    bit; then theta_out = theta, no next proposal, mask / ret / count = None in turn, count from 7."""
    inp = make_inputs(kind, C, D, seed=1)
    pd, pack = device_pack(ops, inp)
    log_u = planted_log_u(threshold(inp, pack)[0])
    flat, _ = run_step(ops, inp, log_u, pd)
    assert_outputs(flat, expected(inp, pack, log_u, 0), (kind, C, D, "contiguous"))
    variants = [dict(count0=7)] + [dict(inplace=True, count0=7), dict(with_z=False), dict(drop=("mask",)), dict(drop=("ret",)),
                                   dict(drop=("count",))]
    for n, layout in enumerate(LAYOUTS):
        for kw in (variants if n == 1 else variants[:1] if n else [dict()]):
            tag = (kind, C, D, layout, tuple(kw.items()))
            got, bufs = run_step(ops, inp, log_u, pd, layout=layout, **kw)
            ok, which = guards_intact(bufs)
            assert ok, tag + ("guard cells of " + which,)
            want = expected(inp, pack, log_u, kw.get("count0", 0), with_z=kw.get("with_z", True))
            drop = kw.get("drop", ())
            if "mask" in drop:
                want["mask"] = np.full(C, 9, dtype=np.uint8)
            if "ret" in drop:
                want["ret"] = np.full(C, np.nan)
            if "count" in drop:
                want["count"] = np.array([0], dtype=np.int32)
            assert_outputs(got, want, tag)
            for k in ("out", "g", "thp", "lp"):
                assert k not in got or not np.isnan(got[k]).any(), tag + (k, "NaN")
            if set(kw) <= {"count0"}:
                assert_outputs(got, flat, tag + ("vs contiguous",), skip=("count",) if kw else ())


# ---- C. non-finite values and the pair partner ---------------------------------------------------------------------------------------
NONFINITE = (("lpp", np.nan, False), ("lpp", np.inf, True), ("lpp", -np.inf, False), ("logu", -np.inf, True),
             ("logu", np.inf, False), ("logu", np.nan, False), ("thp", np.inf, False))


def check_nonfinite(ops, kind, C, D):
    """One chain of a pair made bad: its decision follows IEEE comparison, a refused chain keeps theta, grad and lp bit for bit,
    and every other chain -- its pair partner first -- is bit-identical to the run without the bad chain."""
    inp = make_inputs(kind, C, D, seed=2)
    if not separable(kind):
        inp["g"], inp["gp"] = grads(inp, inp["th"]), grads(inp, inp["thp"])
    pd, pack = device_pack(ops, inp)
    log_u = planted_log_u(threshold(inp, pack)[0])
    base, _ = run_step(ops, inp, log_u, pd)
    for what, value, accepted in NONFINITE:
        for b in (0, C - 1, 2 * (C // 4) + 1):   # an even chain (its partner is accepted), the last chain, an odd one inside
            bad, lu = dict(inp), log_u.copy()
            if what == "logu":
                lu[b] = value
            elif what == "lpp":
                bad["lpp"] = inp["lpp"].copy()
                bad["lpp"][b] = value
            else:
                bad["thp"] = inp["thp"].copy()
                bad["thp"][D // 2, b] = value
                if not separable(kind):   # (the model's gradient at an infinite coordinate)
                    bad["gp"] = grads(inp, bad["thp"])
            tag = (kind, C, D, what, value, b)
            got, _ = run_step(ops, bad, lu, pd)
            assert bool(got["mask"][b]) == accepted, tag + ("decision",)
            assert_outputs(got, expected(bad, pack, lu, 0), tag)
            others = np.arange(C) != b
            partner = b ^ 1
            for k in ("mask", "ret", "lp", "out", "g", "thp"):
                if k in got:
                    assert same(got[k][..., partner], base[k][..., partner]), tag + (k, "pair partner")
                    assert same(got[k][..., others], base[k][..., others]), tag + (k, "other chains")
            if not accepted:
                assert same(got["out"][:, b], inp["th"][:, b]) and got["lp"][b] == inp["lp"][b], tag + ("refused state",)
                assert "g" not in got or same(got["g"][:, b], inp["g"][:, b]), tag + ("refused gradient",)


# ---- D. the cache-size seam ----------------------------------------------------------------------------------------------------------
def check_seam(ops, kind, C, D, streams):
    """A shape on one side of the footprint rule: the planted-threshold outputs for all chains, and torch.equal to the same call
    made on the two column halves as pitched views of the same buffers (those take the resident form)."""
    assert step_form(kind, C, D)[2] == streams
    inp = make_inputs(kind, C, D, seed=3)
    T, ratio = threshold(inp, None)
    assert ratio <= 1.0, (kind, C, D, ratio)
    log_u = planted_log_u(T)
    got, _ = run_step(ops, inp, log_u, None)
    assert_outputs(got, expected(inp, None, log_u, 0), (kind, C, D))
    h = C // 4 * 2
    assert not step_form(kind, h, D)[2] and not step_form(kind, C - h, D)[2]
    _, bufs = run_step(ops, inp, log_u, None, cols=(0, h))
    halves, _ = run_step(ops, inp, log_u, None, cols=(h, C), bufs=bufs)
    assert_outputs(halves, got, (kind, C, D, "halves"))
    return ratio


# ---- E. the small kernels --------------------------------------------------------------------------------------------------------------
def check_logq(ops, C, D):
    """bk_mala_logq on guarded views: array_equal to the quarter sums, within (ceil(D/4) + 8) 2**-53 ref of np.longdouble."""
    g = np.random.default_rng([4, C, D])
    arr = [g.normal(size=(D, C)) for _ in range(4)]
    eps, k = 0.02, -0.25 / 0.02
    views = [View(ops, a, C + 3, 1, D + 1) for a in arr]
    f = torch.full((C,), float("nan"), dtype=torch.float64, device=ops.device)
    r = torch.full((C,), float("nan"), dtype=torch.float64, device=ops.device)
    ops.mala_logq(*[v.v for v in views], eps, f, r)
    th, gr, thp, gp = arr
    xf, xr = (thp - th) - eps * gr, (th - thp) - eps * gp
    worst = 0.0
    for got, x in ((get(f), xf), (get(r), xr)):
        assert same(got, k * quarter_sum(x * x)), (C, D)
        ref = np.longdouble(k) * (x.astype(np.longdouble) ** 2).sum(axis=0)
        bound = ((D + 3) // 4 + 8) * U * np.abs(ref)
        worst = max(worst, float(np.max(np.abs(got - ref) / bound)))
    assert worst <= 1.0, (C, D, worst)
    assert all(v.guards_intact() for v in views), (C, D)
    return worst


def check_logq_no_dims(ops):
    """D = 0: BK_OK, nothing launched, nothing written -- bk_mala_logq and bk_mala_logq_precond alike (include/bkhip.h)."""
    C = 5
    a = torch.zeros((1, C), dtype=torch.float64, device=ops.device)
    pd = torch.ones((3, 1), dtype=torch.float64, device=ops.device)
    p = _lib.ptr
    for pc in (False, True):
        f = torch.full((C,), float("nan"), dtype=torch.float64, device=ops.device)
        r = torch.full((C,), float("nan"), dtype=torch.float64, device=ops.device)
        if hasattr(ops, "lib"):   # (an empty tensor has no address: the C ABI itself, on arrays that exist)
            if pc:
                ops._call("bk_mala_logq_precond", p(a), p(a), p(a), p(a), C, p(pd), 0.02, p(f), p(r), C, 0, ops._s())
            else:
                ops._call("bk_mala_logq", p(a), p(a), p(a), p(a), C, 0.02, p(f), p(r), C, 0, ops._s())
        elif pc:
            ops.mala_logq_precond(a[:0], a[:0], a[:0], a[:0], pd[:, :0], 0.02, f, r)
        else:
            ops.mala_logq(a[:0], a[:0], a[:0], a[:0], 0.02, f, r)
        assert np.isnan(get(f)).all() and np.isnan(get(r)).all(), pc


def check_propose_from_normals(ops, C, D):
    """bk_mala_propose_from_normals, z in the state layout and chain-major with row pitch D and (D+7)//8*8 + 6: array_equal."""
    g = np.random.default_rng([5, C, D])
    th, gr, z = (g.normal(size=(D, C)) for _ in range(3))
    eps, s = 0.03, float(np.sqrt(0.06))
    want = (th + eps * gr) + s * z
    for ldz in (None, D, (D + 7) // 8 * 8 + 6):
        vs = [View(ops, a, C + 3, 1, D + 1) for a in (th, gr, np.full((D, C), np.nan))]
        if ldz is None:
            zz = View(ops, z, C + 3, 1, D + 1).v
        else:
            zt = np.full((C + 1) * ldz, SENT, dtype=np.int64).view(np.float64).reshape(C + 1, ldz)
            zt[:C, :D] = z.T
            zz = put(ops, zt)[:C, :D].t()
        ops.mala_propose_from_normals(vs[0].v, vs[1].v, zz, vs[2].v, eps, s)
        assert same(get(vs[2].v), want), (C, D, ldz)
        assert all(v.guards_intact() for v in vs), (C, D, ldz)


def check_propose(ops, C, D, seed=55):
    """bk_mala_propose against NumPy's Philox stream of every chain: the proposal array_equal, and the stream table after the
    call the one NumPy's generator is left in."""
    g = np.random.default_rng([6, C, D])
    th, gr = g.normal(size=(D, C)), g.normal(size=(D, C))
    eps, s = 0.07, float(np.sqrt(0.14))
    kind, st = make_streams(seed, C, 0, False, ops.device)
    assert kind == _lib.RNG_PHILOX
    vs = [View(ops, a, C + 3, 1, D + 1) for a in (th, gr, np.full((D, C), np.nan))]
    ops.mala_propose(kind, st, vs[0].v, vs[1].v, vs[2].v, eps, s)
    got, table = get(vs[2].v), get(st).view(np.uint64)
    for c in range(C):
        gen = np.random.Generator(np.random.Philox(key=[seed, c]))
        z = gen.normal(size=D)
        assert same(got[:, c], (th[:, c] + eps * gr[:, c]) + s * z), (C, D, c)
        assert np.array_equal(table[:, c], _bitgen_words(gen.bit_generator)[1]), (C, D, c, "stream table")
    assert all(v.guards_intact() for v in vs), (C, D)
