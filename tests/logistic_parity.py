"""The logistic-regression target's kernels at their edges -- shared test bodies (GPU: tests/test_gpu_logistic.py on the
HIP library; CPU: tests/test_logistic_cpu.py on tests/fake_ops.FakeOps, which exercises these bodies without a device).

Every comparison is with tests/logistic_ref.py (long double, rounded once) or with an exact integer product; every bound is
derived from the number of rounded operations (u = 2^-53), never from what a device returned.  Each check prints the largest
err / bound it saw (``pytest -s``)."""
import functools

import numpy as np
import torch

import bayes_kit_amd as bk
from bayes_kit_amd._lib import BkHipError
from tests import logistic_ref as ref

U = ref.U
SENT = -7.25  # sentinel behind pitched rows and behind work_elems
F64 = torch.float64


def say(what, ratio):
    print(f"[logistic-parity] {what}: max err/bound = {ratio:.3g}")


def ratio_of(err, bound, what):
    """max err / bound, asserting err <= bound componentwise (a zero bound asks for a zero error)."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert np.all(np.isfinite(err)), what
    bad = err > bound
    assert not bad.any(), (what, "worst err / bound", float(np.max(err[bad] / np.maximum(bound[bad], 1e-320))),
                           "cells over", int(bad.sum()), "first", tuple(np.argwhere(bad)[0]))
    pos = bound > 0
    return float(np.max(err[pos] / bound[pos])) if pos.any() else 0.0


# ---- tensors with a pitch, an element offset and a sentinel around them -------------------------------------------------
class Pitched:
    """A [R, C] view (row pitch C + pad, `offset` elements into its buffer) of a 1-D buffer filled with SENT."""

    def __init__(self, ops, R, C, pad=0, offset=0, data=None):
        ld = C + pad
        self.buf = torch.full((offset + R * ld + 8,), SENT, dtype=F64, device=ops.device)
        self.t = self.buf[offset:offset + R * ld].view(R, ld)[:, :C]
        if data is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(data, dtype=np.float64)))

    def take(self):
        """The view's values; asserts that nothing outside the view changed."""
        out = self.t.cpu().numpy().copy()
        self.t.fill_(SENT)
        assert bool((self.buf == SENT).all()), "a write outside Y[:, :C]"
        self.t.copy_(torch.from_numpy(out))
        return out


def _refused(call):
    try:
        call()
    except BkHipError:
        return True
    return False


def dev(a, ops):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(ops.device)


# ---- the GEMM ----------------------------------------------------------------------------------------------------------
GEMM_KINDS = ("chains", "chains_work", "metric", "logistic")
VARIANTS = (None, "lda_odd", "ldx_odd", "a_off", "x_off")  # FULL preconditions broken one at a time

GEMM_SHAPES = (
    [(256, 64, 256)]                                                      # all-FULL
    + [(200, 64, 128), (1000, 512, 256)]                                  # FULL + a partial last row block
    + [(130, 37, 129), (1, 1, 1), (127, 15, 127), (129, 17, 129)]         # partial tile in every direction
    + [(128, k, 128) for k in (1, 3, 4, 5, 16, 18)]                       # short K
    + [(128, 32, 9 * 128), (128, 32, 9 * 128 + 1)]                        # empty XCD slots (cb_i >= chain_blocks)
    + [(16, 1024, 4), (40, 2100, 130), (40, 2100, 131), (24, 1536, 256)]  # split-K (131: odd C, padded slab pitch)
    + [(16, 40_016, 300)]                                                 # split-K, short last slab
    + [(40, 4100, 2049), (40, 4100, 4096 + 130)]                          # split-K, more than one column block
)
# bk_dense_metric_apply is square: the row counts above, and the short inner dimensions
METRIC_SHAPES = sorted({(R, C) for R, _, C in GEMM_SHAPES} | {(k, 128) for k in (1, 3, 4, 5, 16, 18)})


def slab_count(work, R, C):
    """S of the split the library makes with this scratch (bk_gemm_chains_work_elems = S * R * ldw)."""
    if work is None:
        return 1
    ldw = C + (C & 1) if C < 2048 else 2048
    assert work.numel() % (R * ldw) == 0
    return work.numel() // (R * ldw)


def run_gemm(ops, kind, A, X, y_rows=None, variant=None):
    """One call of the entry point `kind` on A [R, K] @ X [K, C] with a pitched, sentinel-guarded Y (and a sentinel behind
    work_elems); returns (Y as NumPy, slab count)."""
    R, K = A.shape
    C = X.shape[1]
    apad, aoff = {"lda_odd": (1, 0), "a_off": (2, 1)}.get(variant, (0, 0))
    if variant == "lda_odd" and K % 2:
        apad = 2
    xpad, xoff = {"ldx_odd": (1, 0), "x_off": (2, 1)}.get(variant, (0, 0))
    ypad, yoff = 3, 0
    if kind == "metric":  # (X and Y share one pitch there)
        if variant is None:
            xpad = 2
        ypad, yoff = xpad, xoff
    a, x, y = Pitched(ops, R, K, apad, aoff, A), Pitched(ops, K, C, xpad, xoff, X), Pitched(ops, R, C, ypad, yoff)
    S = 1
    if kind == "chains":
        ops.gemm_chains(a.t, x.t, y.t)
    elif kind == "chains_work":
        work = ops.gemm_chains_work(R, K, C)
        S = slab_count(work, R, C)
        if work is None:
            ops.gemm_chains(a.t, x.t, y.t, None)
        else:
            n = work.numel()
            wbuf = torch.full((n + 64,), SENT, dtype=F64, device=ops.device)
            ops.gemm_chains(a.t, x.t, y.t, wbuf[:n])
            assert bool((wbuf[n:] == SENT).all()), "a write behind work_elems"
    elif kind == "metric":
        assert R == K
        ops.dense_metric_apply(a.t, x.t, y.t)
    elif kind == "logistic":
        ops.gemm_chains_logistic(a.t, x.t, y.t, dev(y_rows, ops))
    else:
        raise ValueError(kind)
    assert np.array_equal(a.take(), A) and np.array_equal(x.take(), X), "an input changed"
    return y.take(), S


def standalone_residual(ops, Z, y_rows):
    """bk_logistic_residual(part = NULL) on a copy of Z."""
    z = Pitched(ops, Z.shape[0], Z.shape[1], 1, 0, Z)
    ops.logistic_residual(z.t, dev(y_rows, ops), None)
    return z.take()


@functools.lru_cache(maxsize=2)
def real_case(R, K, C):
    g = np.random.default_rng([R, K, C])
    A, X = g.normal(size=(R, K)), g.normal(size=(K, C))
    Y, mag = ref.gemm(A, X)
    return A, X, Y, mag


@functools.lru_cache(maxsize=2)
def integer_case(R, K, C):
    g = np.random.default_rng([7, R, K, C])
    A, X = g.integers(-3, 4, size=(R, K)), g.integers(-3, 4, size=(K, C))  # int64
    Y = A @ X
    assert np.abs(Y).max() < 2 ** 53
    return A.astype(np.float64), X.astype(np.float64), Y.astype(np.float64)


def check_gemm(ops, kind, R, K, C):
    """Two checks of one shape.

    EXACT: entries from {-3..3}, K <= 2^16: every product and every partial sum is an integer below 2^53, so Y equals
    the int64 product bit for bit whatever the order of summation or the split -- the check that catches indexing errors.
    (`logistic`: the epilogue of the exact Z equals bk_logistic_residual of that Z, bit for bit, with a distinct y per row.)

    BOUNDED: real inputs against the long-double product, componentwise |Y - Yref| <= (K + S + 1) u (|A||X|): one rounding
    per fused multiply-add, at most K + S - 1 roundings on any path from the products to an output whatever the order (K
    accumulations, S - 1 slab additions), (1 + u)^(K+S-1) - 1 <= (K + S) u for K + S < 2^26, and one more u for the
    reference, whose own error is 2^-11 of that.  (`logistic`: see check_epilogue.)"""
    assert K <= 2 ** 16
    A, X, Yint = integer_case(R, K, C)
    if kind == "logistic":
        y_rows = np.random.default_rng([8, R, K, C]).uniform(size=R)
        got, _ = run_gemm(ops, kind, A, X, y_rows)
        assert np.array_equal(got, standalone_residual(ops, Yint, y_rows)), ("exact", kind, R, K, C)
        return check_epilogue(ops, R, K, C)
    got, S = run_gemm(ops, kind, A, X)
    bad = np.argwhere(got != Yint)
    assert bad.size == 0, ("exact", kind, (R, K, C), "cells wrong", len(bad), "first", tuple(bad[0]))
    A, X, Yref, mag = real_case(R, K, C)
    got, S = run_gemm(ops, kind, A, X)
    rho = ratio_of(np.abs(got - Yref), (K + S + 1) * U * mag, ("bounded", kind, R, K, C))
    say(f"gemm {kind} (R, K, C) = {(R, K, C)} S = {S}", rho)
    return rho


def check_epilogue(ops, R, K, C):
    """bk_gemm_chains_logistic(A, X, Y, y) == bk_gemm_chains(A, X, Z) then bk_logistic_residual(Z, y, NULL), bit for bit
    (the build has -ffp-contract=off and one exp; the epilogue never splits K, so the comparison passes no work), and
    |r - rref| <= 8 u with rref the long-double residual OF THE SAME Z: p <= 1; exp within 3 ulp (OpenCL's fp64 limit,
    which the device library states it meets) of a value <= 1, carried to p with a factor <= 1; three correctly rounded
    operations (1 + e, the division, y - p) on values <= 2.  Logits as drawn, and scaled to reach +-40 and +-800."""
    A, X, Yref, _ = real_case(R, K, C)
    g = np.random.default_rng([9, R, K, C])
    worst = 0.0
    for reach in (None, 40.0, 800.0):
        f = 1.0 if reach is None else reach / max(float(np.abs(Yref).max()), 1e-300)
        Xs = X * f
        y_rows = (g.uniform(size=R) < 0.5).astype(np.float64)
        Z, _ = run_gemm(ops, "chains", A, Xs)
        if reach is not None:
            assert np.abs(Z).max() >= 0.99 * reach
        r, _ = run_gemm(ops, "logistic", A, Xs, y_rows)
        assert np.array_equal(r, standalone_residual(ops, Z, y_rows)), ("epilogue != stand-alone pass", R, K, C, reach)
        worst = max(worst, ratio_of(np.abs(r - ref.residual(Z, y_rows)), np.full(r.shape, 8 * U), ("epilogue", R, K, C, reach)))
    say(f"epilogue residual (R, K, C) = {(R, K, C)}", worst)
    return worst


def check_broken_precondition(ops, kind, variant, R=256, K=64, C=256):
    """On a shape that is otherwise all-FULL, one precondition of the unchecked kernel broken (odd lda, odd ldx, A or X
    8-byte but not 16-byte aligned): the checked kernel must give the aligned call's bits, and the exact product."""
    g = np.random.default_rng([11, R, K, C])
    y_rows = g.uniform(size=R) if kind == "logistic" else None
    A, X = g.normal(size=(R, K)), g.normal(size=(K, C))
    want, _ = run_gemm(ops, kind, A, X, y_rows)
    got, _ = run_gemm(ops, kind, A, X, y_rows, variant)
    assert np.array_equal(got, want), (kind, variant)
    Ai = g.integers(-3, 4, size=(R, K)).astype(np.float64)
    Xi = g.integers(-3, 4, size=(K, C)).astype(np.float64)
    got, _ = run_gemm(ops, "chains" if kind == "logistic" else kind, Ai, Xi, None, variant)
    assert np.array_equal(got, (Ai.astype(np.int64) @ Xi.astype(np.int64)).astype(np.float64)), (kind, variant)


def check_gemm_degenerate(ops):
    """The contract of a degenerate GEMM (include/bkhip.h): R = 0 and C = 0 return without touching Y; K = 0 is the empty
    sum, Y = 0 (y_rows - 0.5 with the epilogue), and reads neither A nor X; a null A, X or Y is BK_E_ARG.

    A tensor without elements has a null data pointer, whatever it is a view of, so through the tensor-level wrappers
    every degenerate size is a refusal (pinned first, on the library and on the stand-in).  The sizes themselves are
    reached through the C ABI with the pointers of the parent buffers -- A[:, :0] and X[:0] as C sees them -- so that
    even an implementation that loads a first panel before it looks at the panel count (the unchecked kernel did, at
    K = 0 with C % 128 = 0 and aligned pointers) reads inside an allocation."""
    f = dict(dtype=F64, device=ops.device)
    Abuf, Xbuf = torch.full((256, 16), 3.0, **f), torch.full((16, 256), 5.0, **f)
    assert Abuf[:, :0].data_ptr() == 0 and torch.empty((4, 0), **f).data_ptr() == 0
    y = Pitched(ops, 256, 256, 3)
    yr = torch.zeros(256, **f)
    for A, X, Y in [(Abuf[:, :0], Xbuf[:0], y.t), (Abuf[:0], Xbuf, y.t[:0]), (Abuf, Xbuf[:, :0], y.t[:, :0]),
                    (torch.empty((256, 0), **f), torch.empty((0, 256), **f), y.t)]:
        for call in (lambda: ops.gemm_chains(A, X, Y), lambda: ops.gemm_chains_logistic(A, X, Y, yr[:A.shape[0]]),
                     lambda: ops.gemm_chains(A, X, Y, torch.zeros(64, **f))):
            assert _refused(call), (A.shape, X.shape)
    assert _refused(lambda: ops.dense_metric_apply(Abuf[:0, :0], y.t[:0], y.t[:0]))
    assert bool((y.buf == SENT).all())
    if not hasattr(ops, "lib"):  # (the stand-in has no C ABI underneath)
        return
    g = np.random.default_rng(3)
    pa, px, st = Abuf.data_ptr(), Xbuf.data_ptr(), ops._s()
    for R, K, C in [(0, 16, 128), (128, 16, 0), (0, 5, 0), (0, 0, 7), (0, 0, 0)]:
        y = Pitched(ops, 256, 256, 3)
        ld = y.t.stride(0)
        ops._call("bk_gemm_chains", pa, 16, R, K, px, 256, y.t.data_ptr(), ld, C, 0, 0, st)
        ops._call("bk_gemm_chains_logistic", pa, 16, R, K, px, 256, y.t.data_ptr(), ld, C, yr.data_ptr(), st)
        ops._call("bk_dense_metric_apply", pa, 16, px, y.t.data_ptr(), ld, C, 0, st)
        assert bool((y.buf == SENT).all()), (R, K, C)
    for R, C in [(256, 256), (200, 128), (130, 129), (1, 1)]:
        y_rows = g.uniform(size=R)
        yd = dev(y_rows, ops)
        assert int(ops.lib.bk_gemm_chains_work_elems(R, 0, C)) == 0
        for kind in ("chains", "logistic"):
            y = Pitched(ops, R, C, 3)
            ld = max(y.t.stride(0), C + 3)
            if kind == "logistic":
                ops._call("bk_gemm_chains_logistic", pa, 16, R, 0, px, 256, y.t.data_ptr(), ld, C, yd.data_ptr(), st)
                want = np.broadcast_to((y_rows - 0.5)[:, None], (R, C))
            else:
                ops._call("bk_gemm_chains", pa, 16, R, 0, px, 256, y.t.data_ptr(), ld, C, 0, 0, st)
                want = np.zeros((R, C))
            got = y.take()
            assert np.array_equal(got, want) and not np.signbit(got[want == 0]).any(), (R, C, kind)
    # a null pointer is refused at any size
    y = Pitched(ops, 4, 8, 3)
    for args in [(0, 16, 4, 16, px, 256, y.t.data_ptr(), 11, 8), (pa, 16, 4, 16, 0, 256, y.t.data_ptr(), 11, 8),
                 (pa, 16, 4, 16, px, 256, 0, 11, 8), (0, 16, 4, 0, px, 256, y.t.data_ptr(), 11, 8)]:
        assert _refused(lambda: ops._call("bk_gemm_chains", *args, 0, 0, st))
    assert bool((y.buf == SENT).all())


# ---- bk_logistic_residual ----------------------------------------------------------------------------------------------
RESIDUAL_CASES = [(1, 1), (5, 256), (7, 3), (8, 1), (9, 2), (255, 256), (256, 256), (257, 256), (1000, 7), (4000, 256),
                  (4001, 65535)]
RESIDUAL_C = (1, 63, 256, 257)
SPECIAL_LOGITS = [0.0] + [s * v for v in (1e-300, 36.7, 37.0, 709.0, 745.2, 800.0) for s in (1.0, -1.0)]
Y_KINDS = ("mixed", "zeros", "ones", "quarter")


def logits_with_specials(g, N, C):
    """~N(0, 2^2) logits with the special values planted: every one of them when N * C >= 13 cells, spread over rows and
    columns (else the first N * C of a shuffled list)."""
    z = 2.0 * g.normal(size=(N, C))
    sp = np.array(SPECIAL_LOGITS)
    g.shuffle(sp)
    reps = max(1, min(8, (N * C) // (4 * len(sp))))
    cells = g.choice(N * C, size=min(N * C, reps * len(sp)), replace=False)
    z.reshape(-1)[cells] = np.resize(sp, len(cells))
    return z


def make_y(g, kind, N):
    return {"mixed": (g.uniform(size=N) < 0.5).astype(np.float64), "zeros": np.zeros(N), "ones": np.ones(N),
            "quarter": np.full(N, 0.25)}[kind]


def call_residual(ops, z, y, segments, with_part=True):
    N, C = z.shape
    Z = Pitched(ops, N, C, 5, 0, z)
    part = torch.full((segments, C), SENT, dtype=F64, device=ops.device) if with_part else None
    ops.logistic_residual(Z.t, dev(y, ops), part, segments)
    return Z.take(), (None if part is None else part.cpu().numpy())


def check_residual(ops, N, segments, C):
    """r within 8 u of the long-double residual (check_epilogue's derivation); exactly y - 1 or y where exp(-|z|) is 0 in
    double; every part[s] within u (rows_per_seg + 8) sum(|y z| + softplus z) of the long-double segment sum -- per cell
    one rounding for y z, exp (3 ulp) and log1p (2 ulp) on log1p(e) <= softplus, one for max(z, 0) + log1p(e), one for
    the subtraction, then at most rows_per_seg roundings of the running sum, each relative to a partial sum that the
    magnitude sum bounds; segments past the data exactly 0.0; part = NULL and another `segments` leave r's bits alone."""
    worst_r = worst_p = 0.0
    for yk in Y_KINDS:
        g = np.random.default_rng([13, N, segments, C, Y_KINDS.index(yk)])
        z, y = logits_with_specials(g, N, C), make_y(g, yk, N)
        r, part = call_residual(ops, z, y, segments)
        worst_r = max(worst_r, ratio_of(np.abs(r - ref.residual(z, y)), np.full(r.shape, 8 * U), ("r", N, segments, C, yk)))
        with np.errstate(under="ignore"):
            dead = np.exp(-np.abs(z)) == 0.0
        yy = np.broadcast_to(y[:, None], z.shape)
        assert np.array_equal(r[dead & (z > 0)], (yy - 1.0)[dead & (z > 0)]), ("saturated +", N, segments, C, yk)
        assert np.array_equal(r[dead & (z < 0)], yy[dead & (z < 0)]), ("saturated -", N, segments, C, yk)
        pref, pmag, rows = ref.segment_sums(z, y, segments)
        used = -(-N // rows)
        assert np.array_equal(part[used:], np.zeros((segments - used, C))) and not np.signbit(part[used:]).any()
        worst_p = max(worst_p, ratio_of(np.abs(part - pref), U * (rows + 8) * pmag, ("part", N, segments, C, yk)))
        r2, _ = call_residual(ops, z, y, segments, with_part=False)
        assert np.array_equal(r2, r), ("part = NULL changes r", N, segments, C, yk)
        for s2 in (1, 256):
            if s2 != segments:
                r3, _ = call_residual(ops, z, y, s2, with_part=(s2 == 1))
                assert np.array_equal(r3, r), ("segments changes r", N, segments, s2, C, yk)
    say(f"residual r (N, segments, C) = {(N, segments, C)}", worst_r)
    say(f"residual part (N, segments, C) = {(N, segments, C)}", worst_p)
    return worst_r, worst_p


def check_residual_nonfinite(ops, N=64, C=70, segments=8):
    """Non-finite logits in a few cells: the call returns, every other cell of r and every segment sum without such a
    cell keep their bits, and the affected ones are what oracle.models.LogisticRegression's formula gives for that cell
    (r = y - 1 / (1 + exp(-z)),  term = y z - logaddexp(0, z)):

        z      r       term, y = 0           term, y > 0
        +inf   y - 1   NaN  (0 * inf)        NaN  (inf - inf)
        -inf   y       NaN  (0 * -inf)       -inf
        NaN    NaN     NaN                   NaN

    A segment sum with a NaN term is NaN; one with -inf terms and no NaN is -inf."""
    g = np.random.default_rng(17)
    z0 = 2.0 * g.normal(size=(N, C))
    y = np.where(g.uniform(size=N) < 0.3, 0.25, (g.uniform(size=N) < 0.5).astype(np.float64))
    y[:6] = [0.0, 1.0, 0.25, 0.0, 1.0, 0.25]
    z = z0.copy()
    cells = [(0, 0, np.inf), (1, 1, np.inf), (2, 2, np.inf), (3, 3, -np.inf), (4, 4, -np.inf), (5, 5, -np.inf),
             (0, 6, np.nan), (1, 7, np.nan), (63, 69, -np.inf), (40, 69, np.nan), (17, 33, np.inf), (9, 4, -np.inf)]
    y[9], y[63] = 1.0, 1.0
    for n, c, v in cells:
        z[n, c] = v
    hit = ~np.isfinite(z)
    r0, part0 = call_residual(ops, z0, y, segments)
    r, part = call_residual(ops, z, y, segments)
    assert np.array_equal(r[~hit], r0[~hit])
    with np.errstate(all="ignore"):
        r_formula = y[:, None] - 1.0 / (1.0 + np.exp(-z))
        term = y[:, None] * z - np.logaddexp(0.0, z)
    assert np.array_equal(r[hit], r_formula[hit], equal_nan=True)
    for n, c, v in cells:  # the table, spelled out
        want_r = np.nan if np.isnan(v) else (y[n] - 1.0 if v > 0 else y[n])
        assert np.array_equal(r[n, c], want_r, equal_nan=True), (n, c, v)
        want_t = -np.inf if (v == -np.inf and y[n] > 0) else np.nan
        assert np.array_equal(term[n, c], want_t, equal_nan=True), (n, c, v)
    rows = ref.rows_per_segment(N, segments)
    for s in range(segments):
        seg_hit = hit[s * rows:(s + 1) * rows].any(axis=0)
        assert np.array_equal(part[s][~seg_hit], part0[s][~seg_hit]), s
        with np.errstate(all="ignore"):
            want = term[s * rows:(s + 1) * rows].sum(axis=0)
        assert not np.isfinite(want[seg_hit]).any()
        assert np.array_equal(part[s][seg_hit], want[seg_hit], equal_nan=True), s


# ---- bk_logistic_finish ------------------------------------------------------------------------------------------------
def check_finish(ops, D, C, segments):
    """grad = t G + (-(inv_s2 theta)), loglik = the left-to-right sum of part, logp = t loglik + (-0.5 inv_s2 sum theta^2)
    (theta^2 summed in row order): every operation is one correctly rounded IEEE operation and the build does not contract,
    so the NumPy restatement in the same order is held BIT FOR BIT.  t = 0: logp is the prior alone and grad is
    -(inv_s2 theta), in VALUE: 0 * G is -0.0 where G < 0 and -0.0 + -0.0 is -0.0 where theta = 0, so a gradient of
    -0.0 against +0.0 is accepted there (array_equal compares values) and nowhere else is there a difference to accept.
    NULL combinations accepted: grad only, logp only, loglik only (G = NULL with grad = NULL); refused with BK_E_ARG:
    logp or loglik without part, grad without G."""
    g = np.random.default_rng([19, D, C, segments])
    inv = 1.0 / 1.7 ** 2
    th, G = g.normal(size=(D, C)), 50.0 * g.normal(size=(D, C))
    th.reshape(-1)[g.choice(D * C, size=max(1, D * C // 9), replace=False)] = 0.0
    part = 100.0 * g.normal(size=(segments, C))
    ll = np.zeros(C)
    for s in range(segments):
        ll = ll + part[s]
    s2 = np.zeros(C)
    for d in range(D):
        s2 = s2 + th[d] * th[d]
    prior = -0.5 * inv * s2
    partd = dev(part, ops)
    for t in (0.0, 0.25, 1.0):
        T, Gd, gr = Pitched(ops, D, C, 3, 0, th), Pitched(ops, D, C, 3, 0, G), Pitched(ops, D, C, 3)
        lp = torch.full((C + 4,), SENT, dtype=F64, device=ops.device)
        lk = torch.full((C + 4,), SENT, dtype=F64, device=ops.device)
        ops.logistic_finish(Gd.t, T.t, partd, inv, t, gr.t, lp[:C], lk[:C])
        grad = gr.take()
        assert np.array_equal(T.take(), th) and np.array_equal(Gd.take(), G)
        assert bool((lp[C:] == SENT).all()) and bool((lk[C:] == SENT).all())
        logp, loglik = lp[:C].cpu().numpy(), lk[:C].cpu().numpy()
        assert np.array_equal(loglik, ll), ("loglik is not the left-to-right sum of part", D, C, segments)
        want_g = t * G + (-(inv * th))
        if t == 0.0:
            assert np.array_equal(logp, prior) and np.array_equal(grad, -(inv * th))
        else:
            assert np.array_equal(grad, want_g) and np.array_equal(np.signbit(grad), np.signbit(want_g))
        assert np.array_equal(logp, t * ll + prior), (D, C, segments, t)
        # the accepted NULL combinations give the same bits as the full call
        g2 = Pitched(ops, D, C, 3)
        ops.logistic_finish(Gd.t, T.t, None, inv, t, g2.t, None, None)
        assert np.array_equal(g2.take(), grad)
        lp2 = torch.full((C,), SENT, dtype=F64, device=ops.device)
        ops.logistic_finish(None, T.t, partd, inv, t, None, lp2, None)
        assert np.array_equal(lp2.cpu().numpy(), logp)
        lk2 = torch.full((C,), SENT, dtype=F64, device=ops.device)
        ops.logistic_finish(None, T.t, partd, inv, t, None, None, lk2)
        assert np.array_equal(lk2.cpu().numpy(), loglik)
        ops.logistic_finish(None, T.t, None, inv, t, None, None, None)  # nothing asked for: accepted, nothing written
        # refused
        g3 = Pitched(ops, D, C, 3)
        lp3 = torch.full((C,), SENT, dtype=F64, device=ops.device)
        assert _refused(lambda: ops.logistic_finish(Gd.t, T.t, None, inv, t, g3.t, lp3, None))
        assert _refused(lambda: ops.logistic_finish(Gd.t, T.t, None, inv, t, None, None, lp3))
        assert _refused(lambda: ops.logistic_finish(None, T.t, partd, inv, t, g3.t, lp3, None))
        assert bool((g3.buf == SENT).all()) and bool((lp3 == SENT).all())


# ---- the target as a whole ---------------------------------------------------------------------------------------------
TARGET_SHAPES = [(1536, 16, 256), (2100, 40, 130), (130, 1, 1), (17, 513, 64), (5000, 24, 2049)]
THETA_SCALES = (1.0, 30.0, 0.0)


def make_data(N, D, seed):
    g = np.random.default_rng(seed)
    X = g.normal(size=(N, D)) / np.sqrt(D)
    tstar = g.normal(size=D)
    y = (g.uniform(size=N) < 1 / (1 + np.exp(-X @ tstar))).astype(np.float64)
    return X, y, g


def target_bounds(rf, e, Theta, t, N, D, segments, S2):
    """Componentwise bounds on the product's errors against the long-double evaluation `e` (u = 2^-53; first order in u
    except where stated; the reference's own error, 2^-11 of these, is inside the slack of the constants).

      z = X Theta, one slab:                |dz| <= ez := (D + 2) u |X||Theta|                         (check_gemm)
      r = y - sigmoid(z):                   |dr| <= 8 u + ez / 4      (check_epilogue; sigmoid is 1/4-Lipschitz, exactly)
      G = X^T r over S2 slabs:              |dG| <= (N + S2 + 1) u |X^T| 1 + |X^T| (8 u + ez / 4)      (|r| <= 1)
      grad = t G + (-(inv theta)):          3 roundings on |t G| <= t |X^T| 1 and |theta| inv:
                                            |dgrad| <= t |dG| + 3 u (t |X^T| 1 + |theta| inv)
                                          = u (N + S2 + 1 + 8 + 3) t |X^T| 1 + t |X|^T ez / 4 + 3 u |theta| inv
      loglik: a segment's sum is within u (rows + 8) of its magnitude sum (check_residual), summing `segments` of them adds
              (segments - 1) u of the total magnitude, and d(term)/dz = y - sigmoid(z) in [-1, 1] carries dz:
                                            |dll| <= u (rows + 8 + segments) llmag + sum_n ez[n]
      prior = (-0.5 inv) * sum theta^2:     D squares, D additions, one product: <= (D + 2) u |prior|
      logp = t ll + prior:                  2 more roundings on t llmag + |prior|:
                                            |dlogp| <= t |dll| + u (D + 4) |prior| + 2 u t llmag
                                                    <= u (rows + segments + D + 8 + 4) (t llmag + |prior|) + t sum_n ez[n]

    The issue's sketch of these two composite bounds has the same shape; the derivation adds the z error carried through
    the residual into G (which the sketch leaves out) and the final operations' roundings (+3 and +4)."""
    rows = ref.rows_per_segment(N, segments)
    absX = np.abs(rf.X)
    ez = (D + 2) * U * e["zmag"]
    col1 = absX.sum(axis=0)[:, None]  # |X^T| 1
    gb = U * (N + S2 + 12) * t * col1 + t * (absX.T @ ez) / 4 + 3 * U * np.abs(Theta) * rf.inv_s2
    llb = U * (rows + 8 + segments) * e["llmag"] + ez.sum(axis=0)
    lpb = U * (rows + segments + D + 12) * (t * e["llmag"] + e["prior"]) + t * ez.sum(axis=0)
    return gb, llb, lpb


def eval_target(model, Theta, t=None):
    """(logp, grad [D, C], loglik, gradient-only grad) of bk.LogisticRegression at the columns of Theta."""
    ops = model._get_ops()
    D, C = Theta.shape
    th = dev(Theta, ops)
    if t is None:
        lp, g = model.log_density_gradient(th.t())
    else:
        lp, g = model.log_density_gradient_tempered(th.t(), t)
    ll = model.log_likelihood(th.t())
    g_only = torch.full((D, C), SENT, dtype=F64, device=ops.device)
    model.bk_eval(th, g_only, None, 1.0 if t is None else t)  # (the leapfrog path: residual in the GEMM's epilogue)
    return lp.cpu().numpy(), g.t().cpu().numpy().copy(), ll.cpu().numpy(), g_only.cpu().numpy()


def check_target(ops, N, D, C, scale):
    """bk.LogisticRegression's four entry points against the long-double evaluation, EVERY chain, within
    target_bounds; the gradient-only evaluation (epilogue path) gives the full evaluation's gradient bit for bit."""
    X, y, g = make_data(N, D, [23, N, D, C])
    Theta = scale * g.normal(size=(D, C))
    rf = ref.LogisticRef(X, y, prior_scale=2.0)
    model = bk.LogisticRegression(X, y, prior_scale=2.0, ops=ops)
    segments = min(model.SEGMENTS, max(1, N))
    S2 = slab_count(ops.gemm_chains_work(D, N, C), D, C)
    ts = (None, 0.3)
    got = [eval_target(model, Theta, t) for t in ts]
    for t, (lp, grad, ll, g_only) in zip(ts, got):
        assert np.array_equal(g_only, grad), ("gradient-only evaluation differs", N, D, C, scale, t)
    out = [[0.0, 0.0, 0.0] for _ in ts]
    for c0 in range(0, C, 512):  # (column chunks: the long-double cells of 5000 x 2049 at once are a gigabyte)
        sl = slice(c0, min(C, c0 + 512))
        e = rf.evaluate(Theta[:, sl], tuple(1.0 if t is None else t for t in ts))
        for i, (t, (lp, grad, ll, g_only)) in enumerate(zip(ts, got)):
            tt = 1.0 if t is None else t
            gb, llb, lpb = target_bounds(rf, e, Theta[:, sl], tt, N, D, segments, S2)
            what = (N, D, C, scale, t, c0)
            out[i][0] = max(out[i][0], ratio_of(np.abs(grad[:, sl] - e["grad"][i]), gb, ("grad",) + what))
            out[i][1] = max(out[i][1], ratio_of(np.abs(ll[sl] - e["loglik"]), llb, ("loglik",) + what))
            out[i][2] = max(out[i][2], ratio_of(np.abs(lp[sl] - e["logp"][i]), lpb, ("logp",) + what))
    for t, worst in zip(ts, out):
        for name, w in zip(("grad", "loglik", "logp"), worst):
            say(f"target {name} (N, D, C) = {(N, D, C)} scale {scale} t {1.0 if t is None else t}", w)
    if scale == 0.0:  # all logits zero: r = y - 1/2 exactly, so G is an exact-input GEMM and z contributes no error
        assert np.all(ll < 0)
    return out


def check_sharing_invariance(ops, N=5000, D=24, C=2049):
    """A chain's logp and gradient are the same bits evaluated among 2,049 chains, among 256 (a shard from the middle,
    through the same model's buffers -- pitched views -- and through a fresh model) or alone."""
    X, y, g = make_data(N, D, [29, N, D, C])
    Theta = g.normal(size=(D, C))
    model = bk.LogisticRegression(X, y, prior_scale=2.0, ops=ops)
    lp, grad, ll, g_only = eval_target(model, Theta)
    for mk in (lambda: model, lambda: bk.LogisticRegression(X, y, prior_scale=2.0, ops=ops)):
        for sl in (slice(256, 512), slice(0, 256), slice(C - 256, C)):
            lp2, grad2, ll2, g2 = eval_target(mk(), Theta[:, sl])
            assert np.array_equal(lp2, lp[sl]) and np.array_equal(grad2, grad[:, sl]) and np.array_equal(ll2, ll[sl])
            assert np.array_equal(g2, g_only[:, sl])
        for c in (0, 63, 64, 127, 128, 300, C - 1):
            lp1, grad1, ll1, g1 = eval_target(mk(), Theta[:, c:c + 1])
            assert lp1[0] == lp[c] and ll1[0] == ll[c] and np.array_equal(grad1[:, 0], grad[:, c]), c
            assert np.array_equal(g1[:, 0], g_only[:, c]), c


# ---- fixtures run by the reference itself --------------------------------------------------------------------------------
FIXTURE_WIDTHS = (256, 130)  # chains per run: 256 reaches the unchecked GEMM kernel in X Theta, 130 the checked one


def run_logistic_fixture(ops, name, chains, **extra):
    """The many-chain sampler of a logistic fixture on `chains` chains (ids 0 .. chains - 1); returns what the stored
    chain ids did: theta0, draws [N, 8, D], logp [N, 8], accepted [N, 8], final stream words [8, words]."""
    from tests.helpers import load_case, logistic_data
    from tests.sampler_parity import build_sampler

    case, z = load_case(name)
    ids = z["chain_ids"]
    assert chains > ids.max()
    X, y = logistic_data(case["model"])
    model = bk.LogisticRegression(X, y, prior_scale=case["model"]["prior_scale"], ops=ops)
    s = build_sampler(case, model, ops, case["seed"], chains=chains, **extra)
    N = z["draws"].shape[0]
    prev = s._theta.cpu().numpy()[ids].copy()
    out = dict(theta0=prev.copy(), draws=[], logp=[], accepted=[])
    for _ in range(N):
        th, lp = s.sample()
        th, lp = th.cpu().numpy()[ids].copy(), lp.cpu().numpy()[ids].copy()
        out["accepted"].append(np.any(th != prev, axis=1))
        out["draws"].append(th)
        out["logp"].append(lp)
        prev = th
    for k in ("draws", "logp", "accepted"):
        out[k] = np.stack(out[k])
    out["rng_state"] = s.rng_state().T[ids].copy()
    return out, z


def check_logistic_fixture(ops, name, **extra):
    """A fixture produced by the reference's own HMCDiag / MALA on oracle.models.LogisticRegression
    (tests/golden/make_golden.py) against bk.LogisticRegression under the many-chain sampler, run with 256 chains and again
    with 130.  In every run, for the stored chain ids: theta (relative, absolute below |theta| = 1e-3) and logp (relative)
    within the fixture's own tol at every draw -- 100 x the deviation of a long-double rerun of the oracle, asserted
    <= 1e-9 by the generator, which also asserted that no decision of these chains flips under rounding; so `accepted` and
    the final stream state are exact.  The two runs agree with each other bit for bit on the stored chains."""
    runs = []
    for C in FIXTURE_WIDTHS:
        got, z = run_logistic_fixture(ops, name, C, **extra)
        tol = float(z["tol"])
        assert 0.0 < tol <= 1e-9
        assert np.array_equal(got["theta0"], z["theta0"]), (name, C)
        assert np.array_equal(got["accepted"], z["accepted"]), (name, C, "an accept decision differs")
        assert np.array_equal(got["rng_state"], z["rng_state"]), (name, C)
        eth = np.abs(got["draws"] - z["draws"]) / np.maximum(np.abs(z["draws"]), 1e-3)
        elp = np.abs(got["logp"] - z["logp"]) / np.abs(z["logp"])
        say(f"fixture {name} {extra} chains {C} (tol {tol:.2e})", max(eth.max(), elp.max()) / tol)
        worst = int(np.argmax(eth.max(axis=(1, 2))))
        assert eth.max() <= tol, (name, C, "theta", float(eth.max()), "tol", tol, "first worst draw", worst)
        assert elp.max() <= tol, (name, C, "logp", float(elp.max()), "tol", tol)
        runs.append(got)
    for k in ("draws", "logp", "rng_state"):
        assert np.array_equal(runs[0][k], runs[1][k]), (name, k, "a chain depends on the width of its run")


def check_logistic_smc_fixture(ops, name="smc_logistic8_m256"):
    """The reference's TemperedLikelihoodSMC + metropolis_kernel on the logistic model, through the product in
    reference-stream mode with bk.LogisticRegression: ancestor indices and the final stream position exact, the moved and
    the resampled particles within the fixture's tol after every temperature (a particle is theta + scale * z or theta, so
    with every decision equal -- the generator's conditions -- the tol it measured is 0: equal bits)."""
    from tests.helpers import load_case, logistic_data, smc_expected_thetas

    case, z = load_case(name)
    tol = float(z["tol"])
    assert 0.0 <= tol <= 1e-9
    X, y = logistic_data(case["model"])
    model = bk.LogisticRegression(X, y, prior_scale=case["model"]["prior_scale"], ops=ops)
    np.random.seed(case["seed"])
    smc = bk.TemperedLikelihoodSMC(model, case["M"], case["N"], z["theta0"], bk.metropolis_kernel(case["scale"]),
                                   seed=np.random, ops=ops)
    want = smc_expected_thetas(z)
    close = lambda a, b: np.all(np.abs(a - b) <= tol * np.maximum(np.abs(b), 1e-3))  # noqa: E731
    for n in range(1, case["N"] + 1):
        seen = {}
        gather = ops.gather_columns

        def spy(index, src, dst, _seen=seen, _gather=gather):
            _seen["moved"] = np.asarray(src.cpu()).T.copy()
            _gather(index, src, dst)

        ops.gather_columns = spy
        try:
            smc.transition(n)
        finally:
            del ops.gather_columns
        assert np.array_equal(np.asarray(smc._idx.cpu()), z["idx"][n - 1]), (name, n)
        assert close(seen["moved"], z["moved"][n - 1]), (name, n)
        assert close(np.asarray(torch.as_tensor(smc.thetas).cpu()), want[n - 1]), (name, n)
    st = np.random.get_state(legacy=False)
    assert st["state"]["pos"] == int(z["final_pos"]) and st["has_gauss"] == int(z["final_has_gauss"])
    assert np.array_equal(st["state"]["key"][:8], z["final_key"])
