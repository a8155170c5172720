"""tests/hist_parity.py without a GPU: the checks pass on the NumPy stand-in that walks bk_hist_accumulate's launch; each of
the stand-in's planted faults -- one broken seam each -- makes the exact check fail at the case named for it; the library's
argument checks and its slab rule (no device needed); and RunningHistogram's host logic on the stand-in."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import bayes_kit_amd as bk
from tests import fake_ops_hist as fh
from tests import hist_parity as hp
from tests.fake_ops_hist import HistFakeOps


@pytest.fixture(scope="module")
def ops():
    return HistFakeOps()


SLAB_CASES = hp.slab_cases(HistFakeOps())
WINDOW_CASES = hp.window_cases(HistFakeOps())
ALL_CASES = hp.BASE_CASES + hp.BIN_CASES + SLAB_CASES + WINDOW_CASES


def _ids(cases):
    return [hp.case_id(c) for c in cases]


# ---- the checks on the fault-free stand-in -------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", hp.BASE_CASES, ids=_ids(hp.BASE_CASES))
def test_exact(ops, c):
    hp.check_exact(ops, c)


@pytest.mark.parametrize("c", hp.BIN_CASES, ids=_ids(hp.BIN_CASES))
def test_exact_bin_counts(ops, c):
    hp.check_exact(ops, c)


@pytest.mark.parametrize("c", SLAB_CASES, ids=_ids(SLAB_CASES))
def test_exact_at_the_slab_seam(ops, c):
    hp.check_exact(ops, c)


@pytest.mark.parametrize("c", WINDOW_CASES, ids=_ids(WINDOW_CASES))
def test_exact_at_the_lds_window_seam(ops, c):
    hp.check_exact(ops, c)


def test_edges_land_in_their_bins(ops):
    hp.check_edges_land_in_their_bins(ops)


@pytest.mark.parametrize("kind,B", [("dyadic", 64), ("nondyadic", 37)])
def test_all_equal_rows(ops, kind, B):
    hp.check_all_equal_rows(ops, kind, B)


def test_accumulation(ops):
    hp.check_accumulation(ops)


def test_deterministic(ops):
    hp.check_deterministic(ops, hp.Case("nondyadic", 5, hp.SEAM_C, 37, 1))


def test_quantile_bound(ops):
    assert hp.check_quantile_bound(ops, bk) <= 1.0


def test_running_histogram_counts(ops):
    hp.check_running_histogram_counts(ops, bk)


def test_the_data_tells_the_two_product_formula_from_the_contract():
    """The edge neighbourhoods are what makes the exact check bite: counted here, asserted at import of hist_parity."""
    for D in (1, 5):
        n = hp.two_product_differs("nondyadic", D, hp.SEAM_C, 37)
        print(f"D={D}: {n} values of the B = 37 data fall into another slot under x * scale - lo * scale")
        assert n >= 1
    lo, _, scale = hp.grid("nondyadic", 1, 37)
    e = hp.edge_neighbourhood(lo[0], scale[0], 37)
    assert len(e) == 324
    assert (fh.slots_ref(e, lo[0], scale[0], 37) != fh.slots_two_product(e, lo[0], scale[0], 37)).sum() >= 1
    u = np.random.default_rng(0).uniform(lo[0], 0.7001, size=200_000)
    assert np.array_equal(fh.slots_ref(u, lo[0], scale[0], 37), fh.slots_two_product(u, lo[0], scale[0], 37))


# ---- each planted fault is noticed ---------------------------------------------------------------------------------------------
FAULT_CASES = {
    "two_product": hp.Case("nondyadic", 1, hp.SEAM_C, 37, 0),
    "x_edges": hp.Case("nondyadic", 5, hp.SEAM_C, 37, 1),
    "below_le": hp.Case("dyadic", 5, hp.SEAM_C, 64, 1),
    "above_gt": hp.Case("dyadic", 5, hp.SEAM_C, 64, 1),
    "nan_below": hp.Case("dyadic", 1, hp.SEAM_C, 64, 0),
    "odd_tail": hp.Case("dyadic", 1, 65, 64, 0),
    "pitch": hp.Case("nondyadic", 5, 65, 37, 1),
    "slab_seam": hp.Case("nondyadic", 5, 2049, 37, 0),
    "flush_zero": hp.Case("nondyadic", 1, hp.SEAM_C, 37, 0),
}


def test_every_fault_has_a_listed_case():
    assert sorted(FAULT_CASES) == sorted(fh.FAULTS)
    assert set(FAULT_CASES.values()) <= set(ALL_CASES)


@pytest.mark.parametrize("fault", sorted(FAULT_CASES))
def test_fault_is_noticed_by_the_exact_check(fault):
    c = FAULT_CASES[fault]
    with pytest.raises(AssertionError, match="counts differ from the NumPy restatement") as e:
        hp.check_exact(HistFakeOps(fault), c)
    print(fault, hp.case_id(c), e.value)


def test_flush_fault_is_noticed_by_the_accumulation_check_too():
    with pytest.raises(AssertionError, match="accumulated counts differ"):
        hp.check_accumulation(HistFakeOps("flush_zero"))


# ---- the library without a device: argument checks and the slab rule -----------------------------------------------------------
def test_c_abi_argument_checks_and_slab_rule():
    from bayes_kit_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    OK, E_ARG = 0, -1
    f = lib.bk_hist_accumulate
    assert f(p, 0, 0, 5, p, p, 8, p, 11, None) == OK            # C == 0
    assert f(p, 4, 4, 0, p, p, 8, p, 11, None) == OK            # D == 0
    for bad in ((None, 4, 4, 5, p, p, 8, p, 11, None), (p, 4, 4, 5, None, p, 8, p, 11, None),
                (p, 4, 4, 5, p, None, 8, p, 11, None), (p, 4, 4, 5, p, p, 8, None, 11, None),
                (p, 4, -1, 5, p, p, 8, p, 11, None), (p, 4, 4, -1, p, p, 8, p, 11, None),
                (p, 4, 4, 5, p, p, 0, p, 11, None), (p, 4, 4, 5, p, p, 65537, p, 65540, None),
                (p, 3, 4, 5, p, p, 8, p, 11, None),             # ld < C
                (p, 4, 4, 5, p, p, 8, p, 10, None)):            # ldc < B + 3
        assert f(*bad) == E_ARG, bad
    L = lib.bk_hist_lds_bins()
    assert L == fh.LDS_BINS and 2 <= L < 65536
    for C in (0, 1, 2047, 2048, 2049, 4099, 65536, 1 << 20, (1 << 31) + 5, 1 << 40):
        for D in (0, 1, 5, 1024, 2048, 5000):
            for B in (0, 1, 37, 512, L - 1, L, L + 1, 65536, 65537):
                s = lib.bk_hist_slab_chains(C, D, B)
                assert s == fh.slab_chains(C, D, B), (C, D, B)
                if s:
                    assert s % fh.UNIT == 0 and s <= 1 << 30     # a 32-bit counter holds a whole slab
                    assert s >= 2 * min(B + 3, L + 3)


# ---- RunningHistogram: host logic ------------------------------------------------------------------------------------------------
def _hand(ops, rows, B=4, lo=0.0, hi=4.0):
    rows = np.asarray(rows, dtype=np.int64)
    h = bk.RunningHistogram(np.full(rows.shape[0], lo), np.full(rows.shape[0], hi), bins=B, ops=ops)
    h._counts.copy_(torch.from_numpy(rows))
    h.n = int(rows.sum())
    return h


def test_quantiles_of_hand_made_counts(ops):
    #            below  b0 b1 b2 b3 above NaN
    h = _hand(ops, [[0, 2, 0, 3, 0, 0, 5]])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        q = h.quantile([0.0, 0.4, 0.41, 0.5, 1.0])[:, 0]          # k = 1, 2, 3, 3, 5 of n = 5: the NaNs are not counted
        assert np.array_equal(q, [0.0 + 0.5 / 2, 0.0 + 1.5 / 2, 2.0 + 0.5 / 3, 2.0 + 0.5 / 3, 2.0 + 2.5 / 3])
        assert h.median()[0] == 2.0 + 0.5 / 3
        lower, upper = h.interval(0.5)                           # p = 0.25, 0.75: k = 2, 4
        assert lower[0] == 0.75 and upper[0] == 2.0 + 1.5 / 3
        assert h.coverage()[0] == 1.0
        nan_only = _hand(ops, [[0, 0, 0, 0, 0, 0, 3]])
        assert np.isnan(nan_only.quantile([0.0, 0.5, 1.0])).all() and np.isnan(nan_only.coverage()[0])
    assert np.array_equal(h.edges(), [[0.0, 1.0, 2.0, 3.0, 4.0]])
    mixed = _hand(ops, [[1, 2, 0, 3, 0, 2, 5]])
    assert mixed.coverage()[0] == 5.0 / 8.0
    with pytest.warns(RuntimeWarning, match="1 of 1 coordinates") as rec:
        q = mixed.quantile([0.0, 0.125, 0.126, 0.75, 0.76, 1.0])[:, 0]   # k = 1 | 1 | 2 .. | 6 | 7, 8
    assert len(rec) == 1
    assert np.array_equal(q, [-np.inf, -np.inf, 0.0 + 0.5 / 2, 2.0 + 2.5 / 3, np.inf, np.inf])
    off = _hand(ops, [[7, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 9, 1], [0, 1, 1, 1, 1, 0, 0]])
    with pytest.warns(RuntimeWarning, match="2 of 3 coordinates") as rec:
        q = off.quantile([0.001, 0.5, 0.999])
    assert len(rec) == 1
    assert (q[:, 0] == -np.inf).all() and (q[:, 1] == np.inf).all() and np.array_equal(q[:, 2], [0.5, 1.5, 3.5])
    assert np.array_equal(off.coverage(), [0.0, 0.0, 1.0])
    with pytest.raises(ValueError, match="probabilities"):
        h.quantile([1.5])
    with pytest.raises(ValueError, match="mass"):
        h.interval(1.0)


def test_constructor_errors_name_the_coordinates(ops):
    with pytest.raises(ValueError, match=r"not finite at coordinates \[1, 2\]"):
        bk.RunningHistogram([0.0, np.nan, 0.0], [1.0, 1.0, np.inf], ops=ops)
    with pytest.raises(ValueError, match=r"hi <= lo at coordinate \[2\]"):
        bk.RunningHistogram([0.0, 0.0, 1.0], [1.0, 1.0, 1.0], ops=ops)
    with pytest.raises(ValueError, match=r"finite positive number at coordinate \[0\]"):
        bk.RunningHistogram([0.0], [5e-324], bins=512, ops=ops)              # bins / (hi - lo) overflows
    with pytest.raises(ValueError, match=r"finite positive number at coordinate \[1\]"):
        bk.RunningHistogram([0.0, -1e308], [1.0, 1e308], bins=2, ops=ops)    # hi - lo overflows: scale = 0
    for bins in (0, 65537):
        with pytest.raises(ValueError, match="bins"):
            bk.RunningHistogram([0.0], [1.0], bins=bins, ops=ops)
    with pytest.raises(ValueError, match="one length"):
        bk.RunningHistogram([0.0, 1.0], [1.0], ops=ops)
    h = bk.RunningHistogram([0.0, 0.0], [1.0, 1.0], bins=8, ops=ops)
    with pytest.raises(ValueError):
        h.update(torch.zeros((3, 7), dtype=torch.float64))                   # neither extent is D... (3, 7) vs D = 2
    with pytest.raises(ValueError, match="2-D"):
        h.update(torch.zeros(4, dtype=torch.float64))


def _pooled_mean_sd(draws):
    """[N, D, C] -> the pooled mean and RunningMoments.pooled_variance's formula, in NumPy."""
    n = draws.shape[0]
    mean_c, var_c = draws.mean(axis=0), draws.var(axis=0, ddof=1)
    var = (n - 1.0) / n * var_c.mean(axis=1) + mean_c.var(axis=1, ddof=1)
    return mean_c.mean(axis=1), np.sqrt(var)


def test_from_moments(ops):
    N, D, C = 12, 4, 200
    g = np.random.default_rng(11)
    draws = g.normal(size=(N, D, C)) * np.array([1.0, 0.5, 2.0, 10.0])[None, :, None] + np.array([0.0, 3.0, -1.0, 50.0])[
        None, :, None]
    rm = bk.RunningMoments(D, C, ops=ops)
    for t in range(N):
        rm.update(torch.from_numpy(draws[t]), layout="dc")
    mean, sd = _pooled_mean_sd(draws)
    np.testing.assert_allclose(rm.pooled_mean(), mean, rtol=1e-12, atol=1e-13)
    for bins, width in ((512, 8.0), (64, 5.0)):
        h = bk.RunningHistogram.from_moments(rm, bins=bins, width=width)
        np.testing.assert_allclose(h._lo_h, mean - width * sd, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(h._hi_h, mean + width * sd, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(1.0 / h._scale_h, 2.0 * width * sd / bins, rtol=1e-12)  # default: 1/32 of an sd
        assert h.bins == bins and h._ops is ops and h.n == 0
    # a coordinate that never moved has no variance: named
    still = draws.copy()
    still[:, 2, :] = 1.5
    rm2 = bk.RunningMoments(D, C, ops=ops)
    for t in range(N):
        rm2.update(torch.from_numpy(still[t]), layout="dc")
    with pytest.raises(ValueError, match=r"variance > 0: not so at coordinate \[2\]"):
        bk.RunningHistogram.from_moments(rm2)
    bad = draws.copy()
    bad[3, 1, 5] = np.inf
    rm3 = bk.RunningMoments(D, C, ops=ops)
    for t in range(N):
        rm3.update(torch.from_numpy(bad[t]), layout="dc")
    with pytest.raises(ValueError, match=r"not so at coordinate \[1\]"):
        bk.RunningHistogram.from_moments(rm3)
    with pytest.raises(ValueError, match="width"):
        bk.RunningHistogram.from_moments(rm, width=0.0)


def test_state_dict_round_trip_continues_to_the_same_integers(ops):
    D, B = 5, 37
    lo, hi, scale = hp.grid("nondyadic", D, B)
    xs = [torch.from_numpy(np.array(hp.data("nondyadic", D, C, B))) for C in hp.ACC_CHAINS]
    a = bk.RunningHistogram(lo, hi, bins=B, ops=ops)
    a.update(xs[0])
    a.update(xs[1])
    sd = a.state_dict()
    assert sorted(sd) == ["bins", "counts", "hi", "lo", "n"] and sd["n"] == 65 + 2049
    b = bk.RunningHistogram(lo, hi, bins=B, ops=ops)
    b.load_state_dict(sd)
    a.update(xs[2])
    b.update(xs[2])
    assert b.n == a.n == sum(hp.ACC_CHAINS) and torch.equal(a.counts(), b.counts())
    want = fh.counts_ref(np.concatenate([x.numpy() for x in xs], axis=1), lo, scale, B)
    assert np.array_equal(b.counts().numpy(), want)
    for other in (bk.RunningHistogram(lo, hi, bins=B + 1, ops=ops), bk.RunningHistogram(lo, hi + 1e-9, bins=B, ops=ops),
                  bk.RunningHistogram(lo[:4], hi[:4], bins=B, ops=ops)):
        with pytest.raises(ValueError, match="another grid"):
            other.load_state_dict(sd)
    b.reset()
    assert b.n == 0 and not b.counts().any() and np.array_equal(b._lo_h, lo)
    b.update(xs[0])
    assert np.array_equal(b.counts().numpy(), fh.counts_ref(xs[0].numpy(), lo, scale, B))
    c = a.counts()
    c.zero_()                                                     # counts() hands out a copy
    assert a.counts().sum() == sum(hp.ACC_CHAINS) * D


def test_layouts_and_square_draws(ops):
    D = 5
    lo, hi, scale = hp.grid("nondyadic", D, 37)
    x = hp.finite_data(D, D, 3)                                   # a square draw
    want = fh.counts_ref(x, lo, scale, 37)
    buf = torch.from_numpy(np.ascontiguousarray(x))               # the engine's [D, C] buffer
    for draw, layout in ((buf, None), (buf.t(), None), (buf, "dc"), (buf.t(), "cd"), (buf.t().contiguous(), "cd")):
        h = bk.RunningHistogram(lo, hi, bins=37, ops=ops)
        h.update(draw, layout=layout)
        assert np.array_equal(h.counts().numpy(), want) and h.n == D
    h = bk.RunningHistogram(lo, hi, bins=37, ops=ops)
    with pytest.raises(ValueError, match="layout"):
        h.update(buf, layout="rows")
    h.update(torch.from_numpy(np.ascontiguousarray(x[:, :3])).to(torch.float32).to(torch.float64).t())   # (C, D), C = 3
    assert h.n == 3
