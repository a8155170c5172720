"""CPU side of the sort's edge work: the two references of tests/sort_parity.py against each other, the shared bodies run on
the stand-in (tests/fake_ops.FakeOps, whose sort and search state the raw contract of csrc/bk_sort.hip) -- which checks the
bodies, their references and the stand-in; the kernels themselves are held to them in tests/test_gpu_sort.py.  Each body
is also shown to notice a wrong kernel: the ``*_notices_*`` cases run it on a stand-in with one defect planted.  And the
pooled ranks are shown to depend on diagnostics._canonical_keys: without it the stand-in, like the device, ranks a
sign-bit NaN first."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from bayes_kit_amd import diagnostics as dg
from tests import sort_parity as sp
from tests.fake_ops import FakeOps, FakeSortLib

CSRC = os.path.join(os.path.dirname(__file__), "..", "bayes-kit_amd", "csrc")
U64 = np.uint64


@pytest.fixture(scope="module")
def ops():
    return FakeOps()


def _image_t(keys):
    return sp.image(keys.contiguous().numpy().view(U64))


# ---- planted defects ----------------------------------------------------------------------------------------------------------
class ReversesTies(FakeOps):
    def sort_by_key(self, keys, vals):
        n = keys.numel()
        order = torch.from_numpy(np.lexsort((-np.arange(n), _image_t(keys))))
        return keys[order], vals[order]


class SortsByValue(FakeOps):
    """torch.sort: -0.0 ties with +0.0 and every NaN goes last."""

    def sort_by_key(self, keys, vals):
        ko, order = torch.sort(keys, stable=True)
        return ko, vals[order]


class CutsPayloadsTo32Bits(FakeOps):
    def sort_by_key(self, keys, vals):
        ko, vo = super().sort_by_key(keys, vals)
        return ko, vo & 0xFFFFFFFF


class StableInsideBlocksOnly(FakeOps):
    """Equal keys keep their order inside a block of 4,096 inputs; the blocks' shares of a run come out last block first."""

    def sort_by_key(self, keys, vals):
        pos = np.arange(keys.numel())
        order = torch.from_numpy(np.lexsort((pos, -(pos // sp.TILE), _image_t(keys))))
        return keys[order], vals[order]


class SkipsTheLowByte(FakeOps):
    def sort_by_key(self, keys, vals):
        order = torch.from_numpy(np.argsort(_image_t(keys) >> U64(8), kind="stable"))
        return keys[order], vals[order]


class ReturnsCanonicalNaNs(FakeOps):
    def sort_by_key(self, keys, vals):
        ko, vo = super().sort_by_key(keys, vals)
        return torch.where(torch.isnan(ko), torch.full_like(ko, float("nan")), ko), vo


class CountsBelowOrEqual(FakeOps):
    def count_below(self, sorted_keys, queries):
        with np.errstate(invalid="ignore"):
            return torch.from_numpy(np.array([int((sorted_keys.numpy() <= v).sum()) for v in queries.numpy()], dtype=np.int64))


class NaNQueryGivesN(FakeOps):
    """np.searchsorted's answer."""

    def count_below(self, sorted_keys, queries):
        out = super().count_below(sorted_keys, queries)
        out[torch.isnan(queries)] = sorted_keys.numel()
        return out


class ZeroBasedRanks(FakeOps):
    def scatter_ranks(self, payload, base, out):
        out[payload] = base + torch.arange(0, payload.numel(), dtype=out.dtype)


class _LibWritesBehindWork(FakeSortLib):
    def bk_sort_by_key(self, keys_in, keys_out, vals_in, vals_out, n, work, work_bytes, stream):
        rc = super().bk_sort_by_key(keys_in, keys_out, vals_in, vals_out, n, work, work_bytes, stream)
        if rc == 0 and n > 0:
            ctypes.c_uint8.from_address(work + work_bytes).value = 0
        return rc


class _LibTakesAShortWork(FakeSortLib):
    def bk_sort_by_key(self, keys_in, keys_out, vals_in, vals_out, n, work, work_bytes, stream):
        return super().bk_sort_by_key(keys_in, keys_out, vals_in, vals_out, n, work, work_bytes + 1, stream)


def _with_lib(lib_cls):
    ops = FakeOps()
    ops.sort_lib = lib_cls(ops)
    return ops


# ---- the references -------------------------------------------------------------------------------------------------------------
def test_image_and_preimage_are_inverse_and_order_the_classes_as_documented():
    rng = np.random.default_rng(0)
    b = np.concatenate([sp.random_bits(rng, 100_000), sp.KEY_CLASSES])
    assert np.array_equal(sp.preimage(sp.image(b)), b) and np.array_equal(sp.image(sp.preimage(b)), b)
    c = sp.KEY_CLASSES[np.argsort(sp.image(sp.KEY_CLASSES))]
    x = c.view(np.float64)
    assert c[0] == 0xFFFFFFFFFFFFFFFF and c[-1] == 0x7FFFFFFFFFFFFFFF
    assert np.isnan(x[:6]).all() and np.signbit(x[:6]).all() and np.isnan(x[-6:]).all() and not np.signbit(x[-6:]).any()
    assert x[6] == -np.inf and x[7] == -sp.DBL_MAX and x[-7] == np.inf and x[-8] == sp.DBL_MAX
    mid = x[6:-6]
    assert np.all(mid[1:] >= mid[:-1]) and list(c[6 + 8:6 + 10]) == [0x8000000000000000, 0x0]
    # what an x86 host and torch's CPU kernels return for 0.0 / 0.0: the sign-bit quiet NaN, which this order puts FIRST
    with np.errstate(invalid="ignore"):
        q = np.zeros(1) / np.zeros(1)
    assert q.view(U64)[0] == 0xFFF8000000000000 and sp.image(q.view(U64))[0] < sp.image(np.array([-np.inf]).view(U64))[0]


def test_the_restated_constants_are_the_ones_in_the_source():
    src = open(os.path.join(CSRC, "bk_sort.hip")).read()
    assert "SORT_THREADS = 256, SORT_ITEMS = 16, SORT_TILE = SORT_THREADS * SORT_ITEMS, SORT_BINS = 256;" in src
    assert "SORT_CHUNK = SORT_TILE / SORT_WAVES;" in src and "constexpr int PER = 8;" in src
    assert re.search(r"c0 \+= SORT_THREADS \* PER", src) and "__launch_bounds__(64) void k_count_below" in src
    assert (sp.TILE, sp.CHUNK, sp.SCAN_ROUND) == (4096, 1024, 2048) and sp.SCAN_TILES == (2047, 2048, 2049, 4097)
    assert sp.work_bytes_restated(1) == 256 * 2 + 1024 + 2056 and sp.work_bytes_restated(4097) == 2 * 32_768 + 256 + 256 + 2048 + 2056
    for n in (1, 31, 32, 33, 4096, 4097, 8197, 70_001, 2 ** 31 - 1, 2 ** 31, 0):
        assert FakeSortLib.bk_sort_by_key_work_bytes(n) == sp.work_bytes_restated(n)


def _outputs_at_2_18():
    n = 1 << 18
    rng = np.random.default_rng(18)
    pool = np.concatenate([sp.random_bits(rng, 5000), sp.KEY_CLASSES])
    kb = pool[rng.integers(0, len(pool), size=n)]
    k, v = sp.keys_tensor(kb, FakeOps()), torch.arange(n, dtype=torch.int64)
    outs = {}
    for cls in (FakeOps, ReversesTies, SortsByValue, StableInsideBlocksOnly, SkipsTheLowByte, ReturnsCanonicalNaNs):
        ko, vo = cls().sort_by_key(k, v)
        outs[cls.__name__] = (sp.bits(ko), vo.numpy().copy())
    gk, gv = (a.copy() for a in outs["FakeOps"])
    gv[[7, 8]] = gv[[8, 7]]
    outs["payloads of two neighbours swapped"] = (gk, gv)
    gk, gv = (a.copy() for a in outs["FakeOps"])
    gv[n // 2] = gv[n // 2 + 1]
    outs["one payload twice"] = (gk, gv)
    gk, gv = (a.copy() for a in outs["FakeOps"])
    gk[[0, n - 1]], gv[[0, n - 1]] = gk[[n - 1, 0]], gv[[n - 1, 0]]
    outs["first and last pair exchanged"] = (gk, gv)
    return kb, outs


def test_the_property_check_and_the_argsort_reference_accept_exactly_the_same_outputs():
    kb, outs = _outputs_at_2_18()
    vals = np.arange(len(kb), dtype=np.int64)
    verdicts = {}
    for name, (gk, gv) in outs.items():
        v = []
        for ref in (lambda: sp.against_argsort(kb, vals, gk, gv, name), lambda: sp.properties(kb, gk, gv, name)):
            try:
                ref()
                v.append(True)
            except AssertionError:
                v.append(False)
        verdicts[name] = v
        assert v[0] == v[1], (name, v)
    assert verdicts.pop("FakeOps") == [True, True] and not any(a or b for a, b in verdicts.values()), verdicts


def test_the_property_check_notices_a_sort_stable_only_inside_blocks():
    n = 2 * sp.TILE + 5
    kb = np.random.default_rng(1).permutation(sp.KEY_CLASSES)[np.arange(n) % 30]
    gk, gv = sp.run_sort(FakeOps(), kb)
    sp.properties(kb, gk, gv, "right")
    gk, gv = sp.run_sort(StableInsideBlocksOnly(), kb)
    with pytest.raises(AssertionError, match="ties out of input order"):
        sp.properties(kb, gk, gv, "blocks")
    gk, gv = sp.run_sort(StableInsideBlocksOnly(), kb[:sp.TILE])  # (one block: the planted defect alone changes nothing)
    sp.properties(kb[:sp.TILE], gk, gv, "one block")


# ---- the shared bodies on the stand-in ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sp.KEY_IMAGE_SIZES)
def test_key_image_body_on_the_stand_in(ops, n):
    sp.check_key_image(ops, n)


@pytest.mark.parametrize("n", sp.SINGLE_BYTE_SIZES)
def test_single_byte_passes_body_on_the_stand_in(ops, n):
    assert sp.check_single_byte_passes(ops, n) == 34
    for name, kb in sp.single_byte_cases(n):  # the inputs are what they claim to be
        differ = [k for k in range(8) if len(np.unique((sp.image(kb) >> U64(8 * k)) & U64(255))) > 1]
        assert differ == ([] if name.startswith("identical") else [int(name.split()[1])]), name
        if "one" in name:
            k = differ[0]
            assert np.bincount(((sp.image(kb) >> U64(8 * k)) & U64(255)).astype(np.int64)).max() == n - 1


@pytest.mark.parametrize("n", sp.SEAM_SIZES)
def test_tile_and_chunk_seams_body_on_the_stand_in(ops, n):
    sp.check_tile_and_chunk_seams(ops, n)


def test_the_seam_sizes_and_payloads_are_the_ones_asked_for():
    assert len(sp.SEAM_SIZES) == 29 and {1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097} <= set(sp.SEAM_SIZES)
    assert {-(-n // sp.TILE) for n in sp.SEAM_SIZES} >= {1, 2, 7, 8, 9, 10, 15, 16, 17, 18}
    kb, vals = sp.seam_input(4097)
    assert len(np.unique(kb)) == 257 and {sp.I64_MIN, -1} <= set(vals.tolist()) and (vals > 2 ** 32).any()
    assert all(len(np.unique((kb >> U64(8 * k)) & U64(255))) > 100 for k in range(8))


def test_skewed_digits_body_on_the_stand_in(ops):
    sp.check_skewed_digits(ops)
    (_, a), (_, b) = sp.skewed_cases()
    low = (sp.image(a) & U64(255)).reshape(5, sp.TILE)
    assert len(np.unique(low[2])) == 1 and all(len(np.unique(low[t])) > 200 for t in (0, 1, 3, 4))
    assert np.array_equal((sp.image(b) & U64(255)).reshape(5, sp.TILE), np.repeat(np.arange(5), sp.TILE).reshape(5, sp.TILE))


def test_scan_round_inputs_are_what_the_device_test_needs():
    """check_scan_rounds itself runs on the device only (the stand-in has no tiles); its inputs at the smallest size."""
    for mode in sp.SCAN_MODES:
        kb = sp.scan_input(sp.SCAN_TILES[0], mode)
        assert len(kb) == 2046 * sp.TILE + 5
        if mode == "pool":
            assert 900_000 < len(np.unique(kb)) <= 1 << 20
        else:
            assert np.array_equal(sp.image(kb) & U64(255), (np.arange(len(kb)) // sp.TILE) % 256)
    assert [-(-t // sp.SCAN_ROUND) for t in sp.SCAN_TILES] == [1, 1, 2, 3] and 4096 * sp.TILE + 5 > sp.HOST_SORT_MAX


def test_work_buffer_and_views_body_on_the_stand_in(ops):
    assert sp.check_work_buffer_and_views(ops) == 4


def test_count_below_body_on_the_stand_in(ops):
    assert sp.check_count_below(ops) == 6 * len(sp.COUNT_M)
    keys = sp.count_below_keys()
    assert [len(k) for k in keys] == [0, 1, 1, 2, 2, 4097]
    runs = np.unique(keys[-1][:-5], return_counts=True)[1]
    assert runs.max() == 1000 and sorted(runs)[-3:] == [500, 999, 1000]


def test_scatter_ranks_body_on_the_stand_in(ops):
    assert sp.check_scatter_ranks(ops) == 20


def test_pooled_ranks_body_on_the_stand_in(ops):
    sp.check_pooled_ranks_against_numpy(ops)


# ---- each body notices a wrong kernel -----------------------------------------------------------------------------------------
def test_key_image_body_notices_a_sort_by_value_and_canonical_nans():
    with pytest.raises(AssertionError, match="key image n=63: key bits"):
        sp.check_key_image(SortsByValue(), 63)
    with pytest.raises(AssertionError, match="key image n=4097: key bits"):
        sp.check_key_image(ReturnsCanonicalNaNs(), 4097)
    with pytest.raises(AssertionError, match="key image n=63: payloads"):
        sp.check_key_image(ReversesTies(), 63)


def test_single_byte_passes_body_notices_reversed_ties_and_a_skipped_pass():
    with pytest.raises(AssertionError, match="single byte n=4097 byte 0 pos: payloads"):
        sp.check_single_byte_passes(ReversesTies(), sp.TILE + 1)
    with pytest.raises(AssertionError, match="single byte n=4097 byte 0 pos: key bits"):
        sp.check_single_byte_passes(SkipsTheLowByte(), sp.TILE + 1)


def test_tile_and_chunk_seams_body_notices_payloads_cut_to_32_bits():
    for n in (1, 65, sp.TILE + 1):
        with pytest.raises(AssertionError, match=f"seams n={n}, random payloads: payloads"):
            sp.check_tile_and_chunk_seams(CutsPayloadsTo32Bits(), n)
    with pytest.raises(AssertionError, match="seams n=32769, random payloads: payloads"):
        sp.check_tile_and_chunk_seams(StableInsideBlocksOnly(), 8 * sp.TILE + 1)
    sp.check_tile_and_chunk_seams(StableInsideBlocksOnly(), sp.TILE)  # (one block: nothing to get wrong)


def test_skewed_digits_body_notices_a_skipped_low_byte_and_reversed_ties():
    with pytest.raises(AssertionError, match="skewed digits, one tile, one low byte: key bits"):
        sp.check_skewed_digits(SkipsTheLowByte())
    with pytest.raises(AssertionError, match="skewed digits, one tile, one low byte: payloads"):
        sp.check_skewed_digits(ReversesTies())


def test_work_buffer_body_notices_a_write_behind_work_and_a_short_buffer_accepted():
    with pytest.raises(AssertionError, match="a write behind the work buffer"):
        sp.check_work_buffer_and_views(_with_lib(_LibWritesBehindWork))
    with pytest.raises(AssertionError, match="work one byte short: not refused"):
        sp.check_work_buffer_and_views(_with_lib(_LibTakesAShortWork))
    with pytest.raises(AssertionError, match="work buffer: second sort on the same work: key bits"):
        sp.check_work_buffer_and_views(ReturnsCanonicalNaNs())


def test_count_below_body_notices_less_or_equal_and_a_nan_query_answered_with_n():
    with pytest.raises(AssertionError, match="count_below n=1, every query"):
        sp.check_count_below(CountsBelowOrEqual())
    with pytest.raises(AssertionError, match="count_below n=1, every query"):
        sp.check_count_below(NaNQueryGivesN())
    for cls in (CountsBelowOrEqual, NaNQueryGivesN):  # ... and at the launch seam alone
        ops = cls()
        ops_right = FakeOps()
        wrong, ops.count_below = ops.count_below, lambda k, q: wrong(k, q) if q.numel() in sp.COUNT_M else ops_right.count_below(k, q)
        with pytest.raises(AssertionError, match="count_below n=1 m="):
            sp.check_count_below(ops)


def test_scatter_ranks_body_notices_zero_based_ranks():
    with pytest.raises(AssertionError, match="scatter_ranks n=1 base=0.0"):
        sp.check_scatter_ranks(ZeroBasedRanks())


def test_pooled_ranks_body_notices_reversed_ties():
    with pytest.raises(AssertionError, match="pooled ranks, _ranks_pooled"):
        sp.check_pooled_ranks_against_numpy(ReversesTies())


def test_pooled_ranks_need_the_canonical_keys(ops, monkeypatch):
    """Hand the sort the users' own bit patterns and a sign-bit NaN ranks first, -0.0 below +0.0: diagnostics._canonical_keys
    is what stands between them and wrong ranks, on the device and -- now that its sort is the raw contract -- on the stand-in."""
    sp.check_pooled_ranks_against_numpy(ops)
    monkeypatch.setattr(dg, "_canonical_keys", lambda flat: flat)
    with pytest.raises(AssertionError, match="pooled ranks, _ranks_pooled"):
        sp.check_pooled_ranks_against_numpy(ops)
