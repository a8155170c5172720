"""bk.GLM and its two entry points (bk_gemm_chains_glm, bk_glm_residual) at their edges -- shared test bodies (GPU:
tests/test_gpu_glm.py on the HIP library; CPU: tests/test_glm_cpu.py on tests/fake_ops_glm.FakeOpsGLM, which also shows
every planted fault caught by the body named for it).

Every comparison is with tests/glm_ref.py (long double, rounded once), with an exact integer product, or bit for bit with
another entry point; every bound is derived from the number of rounded operations (u = 2^-53), never from what a device
returned.  Each bounded check prints the largest err / bound it saw (``pytest -s``)."""
import functools
import math

import numpy as np
import torch

import bayes_kit_amd as bk
from bayes_kit_amd._lib import GLM_FAMILIES, BkHipError
from tests import glm_ref as ref
from tests import logistic_parity as lp
from tests import logistic_ref as lref
from tests.logistic_parity import F64, SENT, Pitched, dev, ratio_of

U = ref.U
FAMILIES = ref.FAMILIES
SLOPE_SLACK = 1.001  # an error of eta is carried through the map's derivative AT THE REFERENCE'S eta; over an interval of
#                      |d eta| < 1e-9 that derivative changes by a relative e^|d eta| - 1 < 1e-9: the factor covers it
TINY = 2.0 ** -1066  # 256 ulp of the subnormal range: exp's result there has an absolute, not a relative, error


def say(what, ratio):
    print(f"[glm-parity] {what}: max err/bound = {ratio:.3g}")


def fam_id(family):
    return GLM_FAMILIES.index(family)


# ---- per-row data: every row's y, aux and offset distinct, so that a shifted row is seen --------------------------------
def make_rows(g, family, R, offset, integer=False):
    """(y, aux or None, offset or None) for R rows.  integer: counts and trials as a model would hold them."""
    aux = None
    if family == "bernoulli":
        y = (g.uniform(size=R) < 0.5).astype(np.float64) if integer else g.uniform(0.0, 1.0, size=R)
    elif family == "binomial":
        aux = 1.0 + g.permutation(R).astype(np.float64) % 23 + (0.0 if integer else 1.0) * np.arange(R) / (4.0 * R)
        if integer:
            aux = np.floor(aux)
        y = np.floor(g.uniform(size=R) * (aux + 1.0)) if integer else g.uniform(size=R) * aux
    elif family == "poisson":
        y = g.poisson(3.0, size=R).astype(np.float64) if integer else g.uniform(0.0, 20.0, size=R)
    else:
        y = 2.0 * g.normal(size=R)
        aux = g.uniform(0.25, 4.0, size=R)
    off = 0.5 * g.normal(size=R) if offset else None
    return y, aux, off


def _opt(v, ops):
    return None if v is None else dev(v, ops)


# ---- the fused epilogue against the stand-alone pass ----------------------------------------------------------------------
EPILOGUE_SHAPES = [(256, 64, 256),     # all-FULL
                   (1000, 512, 256),   # FULL rows + a partial last row block: the R_full pointer seam
                   (130, 37, 129),     # partial tiles in every direction
                   (1, 1, 1),          # smallest shape
                   (128, 1, 128),      # short K
                   (128, 32, 1153)]    # empty XCD slots


def run_glm_gemm(ops, A, X, family, rows, variant=None):
    """bk_gemm_chains_glm on A [R, K] @ X [K, C] with pitched, sentinel-guarded operands (logistic_parity.run_gemm's
    pattern; `variant` breaks one FULL precondition); returns Y as NumPy."""
    R, K = A.shape
    C = X.shape[1]
    apad, aoff = {"lda_odd": (1, 0), "a_off": (2, 1)}.get(variant, (0, 0))
    if variant == "lda_odd" and K % 2:
        apad = 2
    xpad, xoff = {"ldx_odd": (1, 0), "x_off": (2, 1)}.get(variant, (0, 0))
    a, x, y = Pitched(ops, R, K, apad, aoff, A), Pitched(ops, K, C, xpad, xoff, X), Pitched(ops, R, C, 3, 0)
    yr, aux, off = rows
    ops.gemm_chains_glm(a.t, x.t, y.t, fam_id(family), dev(yr, ops), _opt(aux, ops), _opt(off, ops))
    assert np.array_equal(a.take(), A) and np.array_equal(x.take(), X), "an input changed"
    return y.take()


def standalone(ops, Z, family, rows, segments=None, with_part=False):
    """bk_glm_residual on a pitched copy of Z -> (r, part or None)."""
    N, C = Z.shape
    z = Pitched(ops, N, C, 5, 0, Z)
    yr, aux, off = rows
    part = torch.full((segments, C), SENT, dtype=F64, device=ops.device) if with_part else None
    ops.glm_residual(z.t, fam_id(family), dev(yr, ops), _opt(aux, ops), _opt(off, ops), part, segments)
    return z.take(), (None if part is None else part.cpu().numpy())


def cell_bounds(family, z, rows):
    """Componentwise bound on |r - rref|, rref the long-double residual OF THE SAME z (u = 2^-53, first order in u).

    Every family: with an offset eta = z + o is one rounding, |d eta| <= u |eta|, carried to r through |dr / d eta| (the
    map's derivative: a p (1 - p), mu, w); the reference's own rounding to double is u |r|.
      bernoulli (a = 1) / binomial (a = m): check_epilogue's count -- exp within 3 ulp of a value <= 1 (3 u), 1 + e (u), the
        division (u): |dp| <= 5 u; the product a p adds u (a p) and scales dp by a; y - a p and the reference's rounding are
        u |r| <= u a each: |dr| <= 7 u a + u (a p) <= 8 u a + u (a p), the last term absent for bernoulli.
      poisson: exp within 3 ulp, an ulp at most 2 u of the value: 6 u mu (plus an absolute floor where mu is subnormal);
        y - mu and the reference's rounding: 2 u |y - mu|.
      gaussian: d = y - eta, r = a d and the reference's rounding: three roundings, 3 u |r|."""
    y, aux, off = rows
    r, _, _, eta = ref.cells_ld(family, z, y, aux, off)
    absr, eta = np.abs(np.asarray(r, dtype=np.float64)), np.asarray(eta, dtype=np.float64)
    if family in ("bernoulli", "binomial"):
        p, _ = lref.sigmoid_softplus_ld(eta)
        p = np.asarray(p, dtype=np.float64)
        a = 1.0 if family == "bernoulli" else aux[:, None]
        b = 8 * U * a + (U * a * p if family == "binomial" else 0.0)
        slope = a * p * (1.0 - p)
    elif family == "poisson":
        with np.errstate(over="ignore", under="ignore"):
            mu = np.exp(eta)
        b = 6 * U * mu + 2 * U * absr + TINY
        slope = mu
    else:
        b = 3 * U * absr
        slope = aux[:, None]
    b = np.broadcast_to(b, z.shape).copy()
    if off is not None:
        b += SLOPE_SLACK * U * np.abs(eta) * slope
    return b


def check_epilogue_equals_pass(ops, family, offset, R, K, C):
    """bk_gemm_chains_glm(A, X) == bk_gemm_chains(A, X) then bk_glm_residual(part = NULL), BIT FOR BIT, with distinct y, aux
    and offset per row (a per-row pointer not advanced by R_full shifts the last row block's rows and is seen);
    exact-integer A, X: the epilogue of the exact Z equals the stand-alone pass of that Z; and r within cell_bounds of the
    long double of the same Z."""
    g = np.random.default_rng([31, R, K, C, fam_id(family), int(offset)])
    rows = make_rows(g, family, R, offset)
    A, X, Yint = lp.integer_case(R, K, C)
    got = run_glm_gemm(ops, A, X, family, rows)
    want, _ = standalone(ops, Yint, family, rows)
    assert np.array_equal(got, want, equal_nan=True), ("exact", family, offset, R, K, C)
    A, X, Yref, _ = lp.real_case(R, K, C)
    Xs = X * (3.0 / max(float(np.abs(Yref).max()), 1e-300))  # |z| <= 3: every family's mean stays finite
    Z, _ = lp.run_gemm(ops, "chains", A, Xs)
    r = run_glm_gemm(ops, A, Xs, family, rows)
    want, _ = standalone(ops, Z, family, rows)
    assert np.array_equal(r, want), ("epilogue != stand-alone pass", family, offset, R, K, C)
    rho = ratio_of(np.abs(r - ref.residual(family, Z, *rows)), cell_bounds(family, Z, rows), ("epilogue", family, R, K, C))
    say(f"epilogue {family} offset={offset} (R, K, C) = {(R, K, C)}", rho)
    return rho


def check_broken_precondition(ops, family, offset, variant, R=256, K=64, C=256):
    """On an all-FULL shape, one precondition of the unchecked kernel broken (odd lda, odd ldx, A or X 8-byte but not
    16-byte aligned): the checked kernel gives the aligned call's bits."""
    g = np.random.default_rng([37, R, K, C, fam_id(family), int(offset)])
    rows = make_rows(g, family, R, offset)
    A, X = g.normal(size=(R, K)) / 4, g.normal(size=(K, C)) / 4
    want = run_glm_gemm(ops, A, X, family, rows)
    got = run_glm_gemm(ops, A, X, family, rows, variant)
    assert np.array_equal(got, want), (family, offset, variant)


def check_bernoulli_is_logistic(ops, R, K, C):
    """BERNOULLI without an offset: bk_gemm_chains_glm == bk_gemm_chains_logistic and bk_glm_residual ==
    bk_logistic_residual (r and part), bit for bit."""
    g = np.random.default_rng([41, R, K, C])
    rows = make_rows(g, "bernoulli", R, False)
    A, X, Yref, _ = lp.real_case(R, K, C)
    for reach in (None, 40.0, 800.0):
        Xs = X if reach is None else X * (reach / max(float(np.abs(Yref).max()), 1e-300))
        want, _ = lp.run_gemm(ops, "logistic", A, Xs, rows[0])
        assert np.array_equal(run_glm_gemm(ops, A, Xs, "bernoulli", rows), want), ("gemm", R, K, C, reach)
        Z, _ = lp.run_gemm(ops, "chains", A, Xs)
        for segments in (1, 7):
            r0, p0 = lp.call_residual(ops, Z, rows[0], segments)
            r1, p1 = standalone(ops, Z, "bernoulli", rows, segments, with_part=True)
            assert np.array_equal(r1, r0) and np.array_equal(p1, p0), ("residual", R, K, C, reach, segments)


# ---- bk_glm_residual ------------------------------------------------------------------------------------------------------
RESIDUAL_CASES = [(1, 1), (9, 2), (257, 256), (1000, 7)]
RESIDUAL_C = (1, 63, 257)
LOGIT_SPECIALS = [0.0] + [s * v for v in (1e-300, 36.7, 709.0, 745.2) for s in (1.0, -1.0)]
OTHER_SPECIALS = [0.0] + [s * v for v in (1e-300, 36.7, 709.0) for s in (1.0, -1.0)]


def eta_with_specials(g, family, N, C, off):
    """z such that eta = z + o is ~N(0, 2^2) with the special values planted as eta (z = special - o; where that sum does
    not round back to the special the cell is simply another large value)."""
    sp = np.array(LOGIT_SPECIALS if family in ("bernoulli", "binomial") else OTHER_SPECIALS)
    z = 2.0 * g.normal(size=(N, C))
    g.shuffle(sp)
    reps = max(1, min(8, (N * C) // (4 * len(sp))))
    cells = g.choice(N * C, size=min(N * C, reps * len(sp)), replace=False)
    vals = np.resize(sp, len(cells))
    if family == "poisson":  # e^709 = 8e307: two of them in one segment sum overflow, so +709 is planted once, then +700
        vals[np.flatnonzero(vals == 709.0)[1:]] = 700.0
    if off is not None:
        vals = vals - off[cells // C]
    z.reshape(-1)[cells] = vals
    return z


def check_cells(ops, family, offset, N, segments, C):
    """bk_glm_residual against the long double of the same Z.  r within cell_bounds.  part[s] within
    u (rows_per_seg + k) * the segment's magnitude sum (glm_ref: the sum of the absolute values of the terms that are
    rounded) -- at most rows_per_seg roundings of the running sum, and k = glm_ref.TERM_OPS rounded operations per cell,
    counted as check_residual counts bernoulli's 8 (y eta 1, exp 3, log1p 2, max + log1p 1, the subtraction 1):
      binomial 9: one more product, a * softplus;
      poisson 8: y eta 1, exp 3 ulp of a value that may exceed 1 (an ulp is at most 2 u of it) 6, the subtraction 1;
      gaussian 4: d enters r d twice (2), r = a d (1), r d (1); the product with -0.5 is exact;
    with an offset plus u |eta| |r| per cell: d term / d eta = r (SLOPE_SLACK as in cell_bounds).  Segments past the data
    are exactly +0.0; part = NULL and another `segments` leave r's bits alone."""
    g = np.random.default_rng([43, N, segments, C, fam_id(family), int(offset)])
    rows = make_rows(g, family, N, offset, integer=True)
    y, aux, off = rows
    z = eta_with_specials(g, family, N, C, off)
    r, part = standalone(ops, z, family, rows, segments, with_part=True)
    rr, _, _, eta = ref.cells_ld(family, z, y, aux, off)
    rho_r = ratio_of(np.abs(r - np.asarray(rr, dtype=np.float64)), cell_bounds(family, z, rows), ("r", family, offset, N, segments, C))
    pref, pmag, nrows = ref.segment_sums(family, z, y, aux, off, segments)
    used = -(-N // nrows)
    assert np.array_equal(part[used:], np.zeros((segments - used, C))) and not np.signbit(part[used:]).any()
    bound = U * (nrows + ref.TERM_OPS[family]) * pmag + TINY
    if off is not None:
        carry = np.asarray(U * np.abs(eta) * np.abs(rr), dtype=np.float64)  # (u first: |eta| |r| alone can pass 1.8e308)
        for s in range(used):
            bound[s] += SLOPE_SLACK * carry[s * nrows:(s + 1) * nrows].sum(axis=0)
    rho_p = ratio_of(np.abs(part - pref), bound, ("part", family, offset, N, segments, C))
    r2, _ = standalone(ops, z, family, rows, segments, with_part=False)
    assert np.array_equal(r2, r), ("part = NULL changes r", family, offset, N, segments, C)
    for s2 in (1, 256):
        if s2 != segments:
            r3, _ = standalone(ops, z, family, rows, s2, with_part=(s2 == 1))
            assert np.array_equal(r3, r), ("segments changes r", family, N, segments, s2, C)
    say(f"cells r {family} offset={offset} (N, segments, C) = {(N, segments, C)}", rho_r)
    say(f"cells part {family} offset={offset} (N, segments, C) = {(N, segments, C)}", rho_p)
    return rho_r, rho_p


def nonfinite_table(family, v, y, a):
    """(r, term) of include/bkhip.h's table for eta = v (+-inf, NaN, or 710 for poisson), response y, aux a."""
    nan, inf = np.nan, np.inf
    if np.isnan(v):
        return nan, nan
    if family in ("bernoulli", "binomial"):
        a = 1.0 if family == "bernoulli" else a
        return (y - a, nan) if v > 0 else (y, nan if y == 0 else -inf)
    if family == "poisson":
        if v == inf:
            return -inf, nan
        if v > 0:  # finite, past exp's range
            return -inf, -inf
        return y, (nan if y == 0 else -inf)
    return (-inf if v > 0 else inf), -inf


def check_nonfinite(ops, family, offset, N=64, C=70, segments=8):
    """eta = +-inf, NaN (and 710 for poisson) in a few cells, with y = 0 and y > 0: the header's table holds cell by cell
    (r, and the segment sum the cell's term falls into: NaN with a NaN term, else -inf); every other cell of r and every
    segment sum without such a cell keep their bits."""
    g = np.random.default_rng([47, fam_id(family), int(offset)])
    rows = make_rows(g, family, N, offset, integer=True)
    y, aux, off = rows
    y[:8:2] = 0.0
    if family == "binomial":
        y[1:8:2] = np.maximum(1.0, np.floor(aux[1:8:2] / 2))
    elif family != "gaussian":
        y[1:8:2] = 1.0
    z0 = g.normal(size=(N, C))
    z = z0.copy()
    vals = [np.inf, -np.inf, np.nan] + ([710.0] if family == "poisson" else [])
    cells = [(2 * i + n, 5 * i + n, v) for i, v in enumerate(vals) for n in (0, 1)]  # rows with y = 0 and with y > 0
    cells += [(63, 69, -np.inf), (40, 33, np.nan)]
    for n, c, v in cells:
        z[n, c] = v
        if off is not None and np.isfinite(v):
            z[n, c] = v - off[n] + 1.0  # (eta stays past exp's range whatever the offset's rounding)
    hit = np.zeros(z.shape, dtype=bool)
    for n, c, _ in cells:
        hit[n, c] = True
    r0, part0 = standalone(ops, z0, family, rows, segments, with_part=True)
    r, part = standalone(ops, z, family, rows, segments, with_part=True)
    assert np.array_equal(r[~hit], r0[~hit])
    nrows = lref.rows_per_segment(N, segments)
    seg_nan, seg_inf = np.zeros((segments, C), dtype=bool), np.zeros((segments, C), dtype=bool)
    for n, c, v in cells:
        want_r, want_t = nonfinite_table(family, v, y[n], None if aux is None else aux[n])
        assert np.array_equal(r[n, c], want_r, equal_nan=True), (family, n, c, v, r[n, c], want_r)
        (seg_nan if np.isnan(want_t) else seg_inf)[n // nrows, c] = True
    touched = seg_nan | seg_inf
    assert np.array_equal(part[~touched], part0[~touched])
    assert np.isnan(part[seg_nan]).all()
    only_inf = seg_inf & ~seg_nan
    assert np.array_equal(part[only_inf], np.full(int(only_inf.sum()), -np.inf))


def check_arguments(ops):
    """BK_E_ARG before any launch: an unknown family, aux missing for binomial / gaussian, aux given for bernoulli /
    poisson, a null y, segments outside [1, 65535]; nothing is written."""
    f = dict(dtype=F64, device=ops.device)
    A, X = torch.ones((4, 3), **f), torch.ones((3, 5), **f)
    Y = Pitched(ops, 4, 5, 3)
    v = torch.ones(4, **f)
    refused = lp._refused
    for fam, aux in ((0, v), (2, v), (1, None), (3, None), (4, None), (-1, None), (7, v)):
        assert refused(lambda: ops.gemm_chains_glm(A, X, Y.t, fam, v, aux, None)), (fam, aux is None)
        assert refused(lambda: ops.glm_residual(Y.t, fam, v, aux, None, None, 4)), (fam, aux is None)
    for seg in (-1, 65536):
        assert refused(lambda: ops.glm_residual(Y.t, 0, v, None, None, None, seg)), seg
    assert refused(lambda: ops.glm_residual(Y.t, 0, v, None, None, torch.empty((0, 5), **f)))  # (segments = 0)
    assert bool((Y.buf == SENT).all())
    if hasattr(ops, "lib"):  # a null y reaches the C ABI only as a pointer
        st = ops._s()
        for fam in range(4):
            aux = v.data_ptr() if fam in (1, 3) else 0
            assert refused(lambda: ops._call("bk_gemm_chains_glm", A.data_ptr(), 3, 4, 3, X.data_ptr(), 5, Y.t.data_ptr(),
                                             Y.t.stride(0), 5, fam, 0, aux, 0, st))
            assert refused(lambda: ops._call("bk_glm_residual", Y.t.data_ptr(), Y.t.stride(0), fam, 0, aux, 0, 0, 4, 5, 4, st))
        assert refused(lambda: ops._call("bk_glm_residual", Y.t.data_ptr(), Y.t.stride(0), 0, v.data_ptr(), 0, 0, 0, 4, 5, 0, st))
        assert bool((Y.buf == SENT).all())


# ---- the target as a whole ---------------------------------------------------------------------------------------------
TARGET_SHAPES = [(1536, 16, 256), (2100, 40, 130), (130, 1, 1)]
TEMPERATURES = (1.0, 0.3)
PRIOR_SCALE = 2.0


@functools.lru_cache(maxsize=4)
def make_data(family, N, D, offset, seed=0):
    """(X, y, kwargs of bk.GLM, aux as the library holds it, offset, generator).  eta* = X theta* + o is ~N(0, 1)."""
    g = np.random.default_rng([53, N, D, fam_id(family), int(offset), seed])
    X = g.normal(size=(N, D)) / np.sqrt(D)
    off = g.uniform(-0.3, 0.3, size=N) if offset else None
    eta = X @ g.normal(size=D) + (0.0 if off is None else off)
    kw, aux = {}, None
    if family == "bernoulli":
        y = (g.uniform(size=N) < 1 / (1 + np.exp(-eta))).astype(np.float64)
    elif family == "binomial":
        aux = 1.0 + (np.arange(N) % 9).astype(np.float64)
        y = g.binomial(aux.astype(np.int64), 1 / (1 + np.exp(-eta))).astype(np.float64)
        kw["trials"] = aux
    elif family == "poisson":
        y = g.poisson(np.exp(eta)).astype(np.float64)
    else:
        sd = g.uniform(0.5, 2.0, size=N)
        y = eta + sd * g.normal(size=N)
        kw["noise_sd"] = sd
        aux = 1.0 / (sd * sd)  # (the model's own two roundings)
    if off is not None:
        kw["offset"] = off
    return X, y, kw, aux, off, g


def draw_theta(family, X, off, D, C, seed):
    """[D, C] chains; for poisson scaled so that |eta| <= 5 (the z error is carried through exp with factor mu)."""
    g = np.random.default_rng([59, D, C, seed])
    Th = g.normal(size=(D, C))
    if family == "poisson":
        Th *= 0.6
        eta = X @ Th + (0.0 if off is None else off[:, None])
        Th *= min(1.0, 4.9 / float(np.abs(eta).max()))
    return Th


def target_bounds(rf, e, Theta, t, N, D, segments, S2):
    """Componentwise bounds on bk.GLM's errors against the long-double evaluation `e`, derived like
    logistic_parity.target_bounds (u = 2^-53; first order in u; k = glm_ref.TERM_OPS):

      z = X Theta, one slab:             |dz| <= (D + 2) u |X||Theta|; with an offset eta = z + o adds u |eta|: together e_eta
      r:                                 |dr| <= cell_bounds' first part + slope e_eta, slope = |dr / d eta| at the reference
                                         (a p (1 - p), mu, w; SLOPE_SLACK for its change over the interval; poisson: the
                                         factor mu, with |eta| <= 5)
      G = X^T r over S2 slabs:           |dG| <= (N + S2 + 1) u |X^T||r| + |X^T| |dr|
      grad = t G + (-(inv theta)):       3 roundings on t |X^T||r| and |theta| inv:
                                         |dgrad| <= u (N + S2 + 4) t |X^T||r| + t |X^T| |dr| + 3 u |theta| inv
      loglik = (sum of part) + const:    a segment within u (rows + k) of its magnitude sum, `segments` additions and the
                                         constant's (segments + 1) u of the total magnitude llmag + |const|; const itself is
                                         the double nearest the exact sum: u |const| <= u cmag;  d term / d eta = r carries
                                         e_eta:  |dll| <= u (rows + k + segments + 1) (llmag + cmag) + u cmag + sum_n |r| e_eta
      prior:                             (D + 2) u |prior|
      logp = t ll + prior:               2 more roundings:
                                         |dlogp| <= u (rows + k + segments + D + 6) (t (llmag + cmag) + |prior|) + t sum_n |r| e_eta"""
    rows = lref.rows_per_segment(N, segments)
    k = ref.TERM_OPS[rf.family]
    absX = np.abs(rf.X)
    e_eta = (D + 2) * U * e["zmag"] + (U * np.abs(e["eta"]) if rf.offset is not None else 0.0)
    cb = cell_bounds(rf.family, e["z"], (rf.y, rf.aux, None if rf.offset is None else rf.offset))
    dr = cb + SLOPE_SLACK * e["slope"] * e_eta
    Gmag = absX.T @ e["absr"]
    gb = U * (N + S2 + 4) * t * Gmag + t * (absX.T @ dr) + 3 * U * np.abs(Theta) * rf.inv_s2
    carry = SLOPE_SLACK * (e["absr"] * e_eta).sum(axis=0)
    mag = e["llmag"] + rf.const_mag
    llb = U * (rows + k + segments + 2) * mag + carry
    lpb = U * (rows + k + segments + D + 6) * (t * mag + e["prior"]) + t * carry
    return gb, llb, lpb


def make_model(ops, family, N, D, offset, seed=0):
    X, y, kw, aux, off, _ = make_data(family, N, D, offset, seed)
    return bk.GLM(X, y, family, PRIOR_SCALE, ops=ops, **kw), ref.GLMRef(X, y, family, PRIOR_SCALE, aux, off)


def eval_target(model, Theta, t):
    """(logp, grad [D, C], loglik, gradient-only grad) at the columns of Theta."""
    ops = model._get_ops()
    D, C = Theta.shape
    th = dev(Theta, ops)
    lpv, g = model.log_density_gradient_tempered(th.t(), t)
    ll = model.log_likelihood(th.t())
    g_only = torch.full((D, C), SENT, dtype=F64, device=ops.device)
    model.bk_eval(th, g_only, None, t)  # (the leapfrog path: residual in the GEMM's epilogue)
    return lpv.cpu().numpy(), g.t().cpu().numpy().copy(), ll.cpu().numpy(), g_only.cpu().numpy()


def check_target(ops, family, offset, N, D, C):
    """bk.GLM's entry points against the long-double evaluation, EVERY chain, within target_bounds, at t = 1 and 0.3; the
    gradient-only evaluation (epilogue path) gives the full evaluation's gradient bit for bit; bk_retemper from the t = 1
    parts equals a fresh evaluation at 0.3 bit for bit; log_density(_gradient) is the t = 1 evaluation;
    log_likelihood_gradient / log_prior_gradient are its parts."""
    model, rf = make_model(ops, family, N, D, offset)
    Theta = draw_theta(family, rf.X, rf.offset, D, C, 1)
    segments = min(model.SEGMENTS, max(1, N))
    S2 = lp.slab_count(ops.gemm_chains_work(D, N, C), D, C)
    e = rf.evaluate(Theta, TEMPERATURES)
    if family == "poisson":
        assert np.abs(e["eta"]).max() <= 5.0
    got = [eval_target(model, Theta, t) for t in TEMPERATURES]
    worst = {}
    for i, (t, (lpv, grad, ll, g_only)) in enumerate(zip(TEMPERATURES, got)):
        assert np.array_equal(g_only, grad), ("gradient-only evaluation differs", family, offset, N, D, C, t)
        gb, llb, lpb = target_bounds(rf, e, Theta, t, N, D, segments, S2)
        what = (family, offset, N, D, C, t)
        worst[("grad", t)] = ratio_of(np.abs(grad - e["grad"][i]), gb, ("grad",) + what)
        worst[("loglik", t)] = ratio_of(np.abs(ll - e["loglik"]), llb, ("loglik",) + what)
        worst[("logp", t)] = ratio_of(np.abs(lpv - e["logp"][i]), lpb, ("logp",) + what)
    for (name, t), w in worst.items():
        say(f"target {name} {family} offset={offset} (N, D, C) = {(N, D, C)} t {t}", w)
    # bk_retemper: the t = 1 parts -> t = 0.3, against the fresh evaluation
    th = dev(Theta, ops)
    f = dict(dtype=F64, device=ops.device)
    g1, lp1, ll1, gll = torch.empty((D, C), **f), torch.empty(C, **f), torch.empty(C, **f), torch.empty((D, C), **f)
    model.bk_eval(th, g1, lp1, 1.0, ll1, gll)
    assert np.array_equal(lp1.cpu().numpy(), got[0][0]) and np.array_equal(g1.cpu().numpy(), got[0][1])
    assert np.array_equal(ll1.cpu().numpy(), got[0][2])
    g2, lp2 = torch.empty((D, C), **f), torch.empty(C, **f)
    model.bk_retemper(th, gll, ll1, 0.3, g2, lp2)
    assert np.array_equal(lp2.cpu().numpy(), got[1][0]) and np.array_equal(g2.cpu().numpy(), got[1][1]), "bk_retemper"
    # the plain protocol and the split
    lpd, gd = model.log_density_gradient(th.t())
    assert np.array_equal(lpd.cpu().numpy(), got[0][0]) and np.array_equal(gd.t().cpu().numpy(), got[0][1])
    assert np.array_equal(model.log_density(th.t()).cpu().numpy(), got[0][0])
    llg, gl = model.log_likelihood_gradient(th.t())
    assert np.array_equal(llg.cpu().numpy(), got[0][2]) and np.array_equal(gl.t().cpu().numpy(), gll.cpu().numpy())
    lp0, g0 = model.log_prior_gradient(th.t())
    np.testing.assert_allclose(lp0.cpu().numpy(), -e["prior"], rtol=(D + 4) * U, atol=0)
    assert np.array_equal(g0.cpu().numpy(), -(rf.inv_s2 * Theta.T))
    return worst


def check_gaussian_closed_form(ops, offset, N=2100, D=40, C=130):
    """log_likelihood includes the constant: for the gaussian family it is sum_n log N(y_n; eta_n, sd_n), here in long
    double from the sd the user passed (not from the rounded precision).  Bound: the residual pass's bound,
    u (rows + k + segments) llmag, with the z error it is handed carried through d term / d eta = r (the reference starts
    from X and Theta), plus u (N + 2) times the constant's magnitude sum cmag and nothing else.  That last term holds what
    is not the pass's: the constant's own rounding and its addition (2 u cmag at most), and w = 1 / (sd sd), two roundings,
    which moves each observation's constant by at most u (N u in all, and N <= cmag / 0.22 as |c_n| >= 0.22 for w in
    [0.25, 4]: at most 5 u cmag) and each term by 2 u of itself (2 u llmag).  Together 7 u cmag + 2 u llmag, which
    u (N + 2) cmag covers where 2 llmag <= (N - 5) cmag: asserted."""
    model, rf = make_model(ops, "gaussian", N, D, offset)
    X, y, kw, aux, off, _ = make_data("gaussian", N, D, offset)
    Theta = draw_theta("gaussian", X, off, D, C, 2)
    LD = lref.LD
    eta = lref.gemm_ld(X, Theta) + (0 if off is None else np.asarray(off, dtype=LD)[:, None])
    sd = np.asarray(kw["noise_sd"], dtype=LD)[:, None]
    d = (np.asarray(y, dtype=LD)[:, None] - eta) / sd
    want = (-LD(0.5) * np.log(2 * np.pi * sd * sd) - LD(0.5) * d * d).sum(axis=0).astype(np.float64)
    ll = model.log_likelihood(dev(Theta, ops).t()).cpu().numpy()
    e = rf.evaluate(Theta, (1.0,))
    segments = min(model.SEGMENTS, N)
    rows = lref.rows_per_segment(N, segments)
    e_eta = (D + 2) * U * e["zmag"] + (U * np.abs(e["eta"]) if off is not None else 0.0)
    carry = SLOPE_SLACK * (e["absr"] * e_eta).sum(axis=0)
    assert np.all(2 * e["llmag"] <= (N - 5) * rf.const_mag) and np.all(np.abs(ref.constants("gaussian", y, aux)) >= 0.22)
    bound = U * (rows + ref.TERM_OPS["gaussian"] + segments) * e["llmag"] + carry + U * (N + 2) * rf.const_mag
    rho = ratio_of(np.abs(ll - want), bound, ("gaussian closed form", offset))
    say(f"gaussian closed form offset={offset}", rho)
    return rho


def check_nonfinite_chain(ops, family, N=300, D=6, C=130):
    """A chain whose theta makes eta non-finite (a coordinate at +inf, at NaN, and -- poisson -- large enough for exp to
    overflow) changes no bit of any other chain's grad / logp / loglik, with and without the log likelihood."""
    model, rf = make_model(ops, family, N, D, True)
    Theta = draw_theta(family, rf.X, rf.offset, D, C, 3)
    bad = Theta.copy()
    hit = [3, 64, 129]
    bad[0, 3], bad[D - 1, 64], bad[:, 129] = np.inf, np.nan, 1e6
    good = np.setdiff1d(np.arange(C), hit)
    a, b = eval_target(model, Theta, 0.3), eval_target(model, bad, 0.3)
    for x, yv in zip(a, b):
        assert np.array_equal(x[..., good], yv[..., good])
    assert not np.isfinite(b[0][hit[:2]]).any()


def check_sharing_invariance(ops, family, N=700, D=24, C=2049):
    """A chain's logp, loglik and gradients are the same bits evaluated among 2,049 chains, among 256 of them (through the
    same model's buffers, narrower than they were made for -- the constant's row moves with the width -- and through a
    fresh model) or alone."""
    model, rf = make_model(ops, family, N, D, True)
    Theta = draw_theta(family, rf.X, rf.offset, D, C, 4)
    full = eval_target(model, Theta, 1.0)
    fresh = lambda: make_model(ops, family, N, D, True)[0]  # noqa: E731
    for mk in (lambda: model, fresh):
        for sl in (slice(256, 512), slice(C - 256, C)):
            part = eval_target(mk(), Theta[:, sl], 1.0)
            for x, yv in zip(full, part):
                assert np.array_equal(x[..., sl], yv), (family, sl)
        for c in (0, 127, 128, C - 1):
            one = eval_target(mk(), Theta[:, c:c + 1], 1.0)
            for x, yv in zip(full, one):
                assert np.array_equal(x[..., c:c + 1], yv), (family, c)
    again = eval_target(model, Theta, 1.0)  # (and back at the full width)
    for x, yv in zip(full, again):
        assert np.array_equal(x, yv)


# ---- samplers ------------------------------------------------------------------------------------------------------------
def _states(s):
    return s._theta.cpu().numpy().copy(), s.rng_state().copy()


def check_drop_in(ops, kind, N=2100, D=40, chains=130, draws=5):
    """bk.GLM(X, y, "bernoulli") against bk.LogisticRegression(X, y), same seed: theta, logp and the stream state are
    array_equal after every step.  kind: "hmc", "hmc_opaque", "mala", "smc" (TemperedLikelihoodSMC with hmc_kernel: the
    bk_retemper path, 3 temperatures)."""
    X, y, _ = lp.make_data(N, D, [61, N, D])
    models = [bk.LogisticRegression(X, y, 2.0, ops=ops), bk.GLM(X, y, "bernoulli", 2.0, ops=ops)]
    if kind == "smc":
        init = np.random.default_rng(5).normal(size=(chains, D))
        runs = [bk.TemperedLikelihoodSMC(m, chains, 3, init, bk.hmc_kernel(0.05, 4), seed=11, ops=ops) for m in models]
        for n in range(1, 4):
            for s in runs:
                s.transition(n)
            a, b = runs
            assert np.array_equal(np.asarray(torch.as_tensor(a.thetas).cpu()), np.asarray(torch.as_tensor(b.thetas).cpu())), n
            assert np.array_equal(np.asarray(a._idx.cpu()), np.asarray(b._idx.cpu())), n
            assert np.array_equal(np.asarray(a._rng_state.cpu()), np.asarray(b._rng_state.cpu())), n
            lls = [np.asarray(m.log_likelihood(torch.as_tensor(s.thetas)).cpu()) for m, s in zip(models, runs)]
            lps = [np.asarray(m.log_density(torch.as_tensor(s.thetas)).cpu()) for m, s in zip(models, runs)]
            assert np.array_equal(lls[0], lls[1]) and np.array_equal(lps[0], lps[1]), n
        return
    if kind == "mala":
        runs = [bk.MALA(m, 0.02, chains=chains, seed=7, ops=ops) for m in models]
    else:
        extra = {"path": "opaque"} if kind == "hmc_opaque" else {}
        runs = [bk.HMCDiag(m, 0.05, 6, chains=chains, seed=7, ops=ops, **extra) for m in models]
    moved = False
    th0 = runs[0]._theta.cpu().numpy().copy()
    for n in range(draws):
        outs = [s.sample() for s in runs]
        (tha, lpa), (thb, lpb) = [(th.cpu().numpy(), lpv.cpu().numpy()) for th, lpv in outs]
        assert np.array_equal(tha, thb) and np.array_equal(lpa, lpb), (kind, n)
        assert np.array_equal(runs[0].rng_state(), runs[1].rng_state()), (kind, n)
        moved = moved or bool((tha != th0).any())
    assert moved


def check_constant_survives_other_widths(ops, family="poisson", widths=(8, 4, 8, 300, 4)):
    """The constant's row of a width's part array is the one datum in the model's buffers that is not scratch: after
    evaluations at other widths, wider and narrower (and a growth of Z), every width's row still holds the constant, and an
    evaluation at a width gives the bits it gave the first time."""
    model, rf = make_model(ops, family, 300, 5, True)
    assert model._ll_const != 0.0
    first = {}
    for C in widths:
        Theta = draw_theta(family, rf.X, rf.offset, 5, C, 6)
        got = eval_target(model, Theta, 0.3)
        for x, yv in zip(first.setdefault(C, got), got):
            assert np.array_equal(x, yv), (family, C)
        S = model._dev["S"]
        for Cw, rows in model._dev["parts"].items():
            assert rows.shape == (S + 1, Cw)
            assert np.array_equal(rows[S].cpu().numpy(), np.full(Cw, model._ll_const)), (family, C, Cw)


def check_two_samplers_on_one_model(ops, family="poisson", widths=(64, 192), draws=6):
    """Two HMCDiag samplers with different chain counts on ONE model, their draws interleaved and an eager evaluation of a
    wider batch between them, each equal their single-sampler run on a model of their own bit for bit.  On the device every
    sampler replays its draw as a captured graph (asserted): a replay runs none of the model's host code, so the constant
    it reads must have survived the other sampler's evaluations."""
    N, D = 600, 12
    on_device = ops.device.type == "cuda"
    extra = {"graph": True} if on_device else {}
    mk = lambda m, C: bk.HMCDiag(m, 0.02, 5, chains=C, seed=29, ops=ops, **extra)  # noqa: E731
    shared, rf = make_model(ops, family, N, D, True)
    both = [mk(shared, C) for C in widths]
    solo = [mk(make_model(ops, family, N, D, True)[0], C) for C in widths]
    wide = dev(draw_theta(family, rf.X, rf.offset, D, 300, 8), ops).t()
    ll_wide = shared.log_likelihood(wide).cpu().numpy()
    for n in range(draws):
        for s, ref_s in zip(both, solo):
            (th, lpv), (th0, lp0) = s.sample(), ref_s.sample()
            assert np.array_equal(th.cpu().numpy(), th0.cpu().numpy()), (family, n, s._C)
            assert np.array_equal(lpv.cpu().numpy(), lp0.cpu().numpy()), (family, n, s._C)
            assert np.array_equal(shared.log_likelihood(wide).cpu().numpy(), ll_wide), (family, n)
    for s, ref_s in zip(both, solo):
        assert np.array_equal(s.rng_state(), ref_s.rng_state())
        if on_device:
            assert s._use_graph and s._graph is not None, "the draws were not replayed from a captured graph"
        assert 0.0 < float(s.accept_rate()) <= 1.0  # (proposals were accepted: logp decided something)


INV_N, INV_D, INV_CHAINS, INV_DRAWS = 400, 8, 4096, 5


@functools.lru_cache(maxsize=1)
def invariance_case():
    """The gaussian family's posterior in closed form: cov = (X^T W X + I / s^2)^-1, mean = cov X^T W (y - o)."""
    X, y, kw, aux, off, _ = make_data("gaussian", INV_N, INV_D, True, seed=9)
    W = aux  # the precision the model holds
    prec = X.T @ (W[:, None] * X) + np.eye(INV_D) / PRIOR_SCALE ** 2
    cov = np.linalg.inv(prec)
    mean = cov @ (X.T @ (W * (y - off)))
    return X, y, kw, mean, cov


def exact_draws(mean, cov, n, seed):
    g = np.random.default_rng(seed)
    return mean + g.normal(size=(n, len(mean))) @ np.linalg.cholesky(cov).T


def assert_invariant(theta, mean, cov, what):
    """Each coordinate's pooled mean within 6 sd_d / sqrt(n) of mean_d, its pooled variance within 6 var_d sqrt(2 / (n - 1))
    of var_d (the sampling distribution of n independent exact draws, which an invariant kernel maps to itself)."""
    n = theta.shape[0]
    var = np.diag(cov)
    assert np.all(np.abs(theta.mean(axis=0) - mean) <= 6 * np.sqrt(var / n)), (what, "mean")
    assert np.all(np.abs(theta.var(axis=0, ddof=1) - var) <= 6 * var * np.sqrt(2.0 / (n - 1))), (what, "variance")


def check_invariance_hmc(ops):
    """4,096 chains start from exact draws of the closed-form posterior; after 5 HMCDiag draws the pooled mean and variance
    of every coordinate are still the posterior's, and proposals were accepted."""
    X, y, kw, mean, cov = invariance_case()
    model = bk.GLM(X, y, "gaussian", PRIOR_SCALE, ops=ops, **kw)
    init = exact_draws(mean, cov, INV_CHAINS, 71)
    s = bk.HMCDiag(model, 0.03, 8, init=init, chains=INV_CHAINS, seed=13, ops=ops)
    accepted = 0
    prev = s._theta.cpu().numpy().copy()
    assert np.array_equal(prev, init)
    for _ in range(INV_DRAWS):
        th, _ = s.sample()
        th = th.cpu().numpy()
        accepted += int(np.any(th != prev, axis=1).sum())
        prev = th.copy()
    assert accepted > 0
    assert_invariant(prev, mean, cov, "HMCDiag")


def check_invariance_tempered(ops):
    """The same for the cold rows of a TemperedHMC with ladder [1, 0.3, 0]: bk.GLM is a split model (_split) and the
    beta = 0 rung runs (it samples the prior: its proposals are accepted and its chains move)."""
    X, y, kw, mean, cov = invariance_case()
    model = bk.GLM(X, y, "gaussian", PRIOR_SCALE, ops=ops, **kw)
    betas = [1.0, 0.3, 0.0]
    H = INV_CHAINS
    # every rung starts from exact draws of ITS tempered posterior (closed form as well), so a swap keeps rung 0 exact
    W = 1.0 / np.asarray(kw["noise_sd"]) ** 2
    init = []
    for b in betas:
        prec = b * (X.T @ (W[:, None] * X)) + np.eye(INV_D) / PRIOR_SCALE ** 2
        cb = np.linalg.inv(prec)
        init.append(exact_draws(cb @ (b * (X.T @ (W * (y - kw["offset"])))), cb, H, 73 + len(init)))
    s = bk.TemperedHMC(model, betas, [0.03, 0.05, 0.3], 8, init=np.concatenate(init), chains=H, seed=17, ops=ops)
    assert s._split is True
    cold = s.cold_rows()
    cold = cold.cpu().numpy() if hasattr(cold, "cpu") else np.asarray(cold)
    start = s._theta.cpu().numpy().copy()
    for _ in range(INV_DRAWS):
        th, _ = s.sample()
    th = th.cpu().numpy()
    rates = np.asarray(s.rung_accept_rate())
    assert rates.shape == (3,) and np.all(rates > 0), rates  # (every rung, the beta = 0 one included, ran and accepted)
    hot = np.setdiff1d(np.arange(th.shape[0]), cold)
    assert np.any(th[hot] != start[hot])
    assert_invariant(th[cold], mean, cov, "TemperedHMC cold rows")


def refuses(call):
    try:
        call()
    except (ValueError, BkHipError):
        return True
    return False


def fsum_constant(family, y, aux):
    return math.fsum(ref.constants(family, np.asarray(y, dtype=np.float64), None if aux is None else np.asarray(aux, dtype=np.float64)))
