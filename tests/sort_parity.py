"""The radix sort, the splitter search and the rank scatter of csrc/bk_sort.hip at their tile, scan and key-image edges --
shared test bodies (GPU: tests/test_gpu_sort.py on the HIP library; CPU: tests/test_sort_cpu.py on tests/fake_ops.FakeOps,
which exercises these bodies and their references without a device, and shows each of them failing on a planted defect).

Every body calls ``ops.sort_by_key``, ``ops.count_below`` or ``ops.scatter_ranks`` itself (or the C entry point through
``ops.lib``, on the stand-in ``ops.sort_lib``, where the wrapper hides the argument under test).  Everything is bit-exact: keys are compared as ``uint64``
bit patterns, payloads and counts as integers, ranks as doubles that are exact integers.  There is no tolerance here.

The contract that is pinned (bk_sort_by_key): the keys are ordered by the RAW order of their bit patterns,
    image(b) = ~b if the top bit of b is set, else b | 2**63,
stably (equal images keep their input order), and come back with their own bits.  In values that is: sign-bit NaNs first
(the larger the payload the earlier), -inf, -DBL_MAX, ..., the negative subnormals, -0.0, +0.0, the positive subnormals,
..., +DBL_MAX, +inf, positive NaNs last (the larger the payload the later).  ``0.0 / 0.0`` on an x86 host is a sign-bit
NaN: callers that want NumPy's order canonicalise their keys first (bayes_kit_amd.diagnostics._canonical_keys)."""
import numpy as np
import torch

from bayes_kit_amd import diagnostics as dg
from tests.diag_kernel_parity import SlackVec, dev

U64 = np.uint64
TOP = U64(1) << U64(63)
LOW63 = TOP - U64(1)
TILE, THREADS, BINS, CHUNK = 4096, 256, 256, 1024   # SORT_TILE, SORT_THREADS, SORT_BINS, SORT_CHUNK of csrc/bk_sort.hip
SCAN_ROUND = THREADS * 8                            # tiles k_sort_scan takes per round (SORT_THREADS * PER)
HOST_SORT_MAX = 1 << 20                             # above this many keys the host does not sort: properties()
BK_E_ARG = -1
KEY_SENTINEL = U64(0x7FF8DEAD0000BEEF)              # a NaN no input holds
VAL_SENTINEL = -77
I64_MIN = -(2 ** 63)


# =====================================================================================================================
# the reference
# =====================================================================================================================
def image(b):
    """The order-preserving image of a key's bit pattern (uint64 -> uint64)."""
    b = np.asarray(b, dtype=U64)
    return np.where((b >> U64(63)).astype(bool), ~b, b | TOP)


def preimage(u):
    """The inverse of image()."""
    u = np.asarray(u, dtype=U64)
    return np.where((u >> U64(63)).astype(bool), u & LOW63, ~u)


def reference_order(kb):
    return np.argsort(image(kb), kind="stable")


def keys_tensor(kb, ops):
    """A device float64 tensor holding exactly the bit patterns kb (torch copies bytes; NaN payloads survive)."""
    return torch.from_numpy(np.ascontiguousarray(kb, dtype=U64).view(np.float64).copy()).to(ops.device)


def bits(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(U64)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape}, expected {want.shape}"
    if not np.array_equal(got, want):
        i = int(np.flatnonzero(got != want)[0])
        fmt = (lambda v: f"{int(v):#018x}") if got.dtype == U64 else (lambda v: repr(v.item()))
        raise AssertionError(f"{what}: {int((got != want).sum())} of {got.size} differ, first at {i}: "
                             f"got {fmt(got[i])}, expected {fmt(want[i])}")


def against_argsort(kb, vals, got_k, got_v, what):
    """The outputs are those of the stable argsort of the images: keys_in[order] as bits, vals_in[order]."""
    order = reference_order(kb)
    _same(got_k, kb[order], f"{what}: key bits")
    _same(got_v, vals[order], f"{what}: payloads")


def properties(kb, got_k, got_v, what):
    """O(n), from the bit patterns alone, for a sort whose payload was arange(n):
      1. image(keys_out) is non-decreasing;
      2. vals_out is a permutation of arange(n), and keys_in[p] == keys_out bitwise with p = vals_out, the input
         position of each output;
      3. inside every run of equal images the input positions increase.
    Together the three determine the stable sort uniquely: by 2 the output is a rearrangement of the input pairs, by 1
    the images are in order, so the only freedom left is the order inside each run of equal images, and 3 fixes that to
    the input order -- which is what argsort(kind="stable") returns.  (tests/test_sort_cpu.py shows the two references
    accepting and rejecting the same outputs at 2^18 keys.)"""
    n = len(kb)
    assert got_k.shape == (n,) and got_v.shape == (n,), f"{what}: output shapes"
    img = image(got_k)
    down = img[1:] < img[:-1]
    assert not down.any(), f"{what}: image order: {int(down.sum())} descents, first at {int(np.flatnonzero(down)[0]) if down.any() else -1}"
    inside = (got_v >= 0) & (got_v < n)
    assert inside.all(), f"{what}: not a permutation: {int((~inside).sum())} payloads outside [0, n)"
    seen = np.bincount(got_v, minlength=n)
    assert (seen == 1).all(), f"{what}: not a permutation: {int((seen != 1).sum())} positions missing or repeated"
    _same(kb[got_v], got_k, f"{what}: pairs broken, keys_in[vals_out] against keys_out")
    tie = img[1:] == img[:-1]
    back = tie & (got_v[1:] < got_v[:-1])
    assert not back.any(), f"{what}: ties out of input order: {int(back.sum())}, first at {int(np.flatnonzero(back)[0]) if back.any() else -1}"


def run_sort(ops, kb, vals=None):
    """ops.sort_by_key on the bit patterns kb (payload arange unless given) -> (key bits out, payloads out); the inputs
    must come back bitwise unchanged."""
    kb = np.ascontiguousarray(kb, dtype=U64)
    vals = np.arange(len(kb), dtype=np.int64) if vals is None else np.ascontiguousarray(vals, dtype=np.int64)
    k, v = keys_tensor(kb, ops), torch.from_numpy(vals.copy()).to(ops.device)
    ko, vo = ops.sort_by_key(k, v)
    gk, gv = bits(ko), vo.cpu().numpy()
    assert np.array_equal(bits(k), kb) and np.array_equal(v.cpu().numpy(), vals), "the sort changed its inputs"
    return gk, gv


def sorted_right(ops, kb, what):
    """One sort with arange payloads against the reference: the argsort up to 2^20 keys, the three properties above."""
    gk, gv = run_sort(ops, kb)
    if len(kb) <= HOST_SORT_MAX:
        against_argsort(kb, np.arange(len(kb), dtype=np.int64), gk, gv, what)
    else:
        properties(np.ascontiguousarray(kb, dtype=U64), gk, gv, what)
    return gk, gv


def random_bits(rng, n):
    return rng.integers(0, 2 ** 64, size=n, dtype=U64)


# =====================================================================================================================
# 1. the key image on every class of double
# =====================================================================================================================
KEY_IMAGE_SIZES = (63, 4097, 70_001)
NEGATIVE_CLASSES = np.array([
    0xFFFFFFFFFFFFFFFF, 0xFFF8000000000001, 0xFFF8000000000000, 0xFFF7FFFFFFFFFFFF, 0xFFF4000000000000,
    0xFFF0000000000001,                                              # sign-bit NaNs: quiet, signalling, payloads
    0xFFF0000000000000, 0xFFEFFFFFFFFFFFFF,                          # -inf, -DBL_MAX
    0xC004000000000000, 0xBFF0000000000000, 0x81A56E1FC2F8F359, 0x8010000000000000,  # -2.5, -1, -1e-300, -DBL_MIN
    0x800FFFFFFFFFFFFF, 0x8000000000000001,                          # the largest and the smallest negative subnormal
    0x8000000000000000,                                              # -0.0
], dtype=U64)
KEY_CLASSES = np.concatenate([NEGATIVE_CLASSES, NEGATIVE_CLASSES & LOW63])  # ... and the positive mirror: +0.0 .. +inf, NaNs
assert {0x0, 0x7FF0000000000000, 0x7FF0000000000001, 0x7FFFFFFFFFFFFFFF, 0x7FEFFFFFFFFFFFFF} <= set(KEY_CLASSES.tolist())
assert len(KEY_CLASSES) == 30 and np.array_equal(preimage(image(KEY_CLASSES)), KEY_CLASSES)


def key_image_input(n, seed=0):
    rng = np.random.default_rng([n, seed, 1])
    return rng.permutation(np.resize(KEY_CLASSES, n))


def check_key_image(ops, n):
    """Every class of double, repeated and shuffled to n keys: the output bits are the reference's.  The resulting order,
    also asserted from the values: sign-bit NaNs, -inf, -DBL_MAX, ..., -0.0, +0.0, ..., +DBL_MAX, +inf, positive NaNs."""
    kb = key_image_input(n)
    gk, gv = sorted_right(ops, kb, f"key image n={n}")
    # the same order said in values, without the image: [sign-bit NaNs][ascending non-NaN, -0.0 before +0.0][positive NaNs]
    x = gk.view(np.float64)
    neg_nan, pos_nan = np.isnan(x) & np.signbit(x), np.isnan(x) & ~np.signbit(x)
    a, b = int(neg_nan.sum()), n - int(pos_nan.sum())
    assert neg_nan[:a].all() and pos_nan[b:].all() and a > 0 and b < n, f"key image n={n}: NaNs by sign, first and last"
    mid = x[a:b]
    assert np.all(mid[1:] >= mid[:-1]) and mid[0] == -np.inf and mid[-1] == np.inf, f"key image n={n}: values ascend"
    zeros = np.flatnonzero(mid == 0.0)
    nz = int(np.signbit(mid[zeros]).sum())
    assert nz > 0 and np.signbit(mid[zeros[:nz]]).all() and not np.signbit(mid[zeros[nz:]]).any(), "-0.0 before +0.0"
    return gk, gv


# =====================================================================================================================
# 2. passes in which every key has the same digit
# =====================================================================================================================
SINGLE_BYTE_SIZES = (TILE + 1, 3 * TILE + 5)
FIXED_IMAGE = U64(0xA53C5AC3966987E1)  # no byte of it is zero (nor of its complement); the image of a positive double
assert all((int(FIXED_IMAGE) >> (8 * k)) & 255 for k in range(8))


def _with_byte(base, k, digit):
    sh = U64(8 * k)
    return (np.asarray(base, dtype=U64) & ~(U64(255) << sh)) | (np.asarray(digit, dtype=U64) << sh)


def single_byte_cases(n, seed=0):
    """-> [(name, key bits)]: per byte position k the images differ in byte k only (seven passes copy, one scatters: k = 0
    is the FIRST scatter, k = 7 the LAST); all keys identical (eight copies, the image applied in the first and undone
    in the last); and per k one key alone off the common digit -- nearly `same`, the flag must stay 0 -- once with the
    smaller digit in the last cell (the ragged tile), once with the larger digit in the first."""
    rng = np.random.default_rng([n, seed, 2])
    cases = []
    for base in (FIXED_IMAGE, ~FIXED_IMAGE):  # keys of both signs: b | 2^63 and ~b on the way in, both branches back
        tag = "pos" if base == FIXED_IMAGE else "neg"
        for k in range(8):
            cases.append((f"byte {k} {tag}", preimage(_with_byte(np.full(n, base), k, rng.integers(0, 256, size=n).astype(U64)))))
        cases.append((f"identical {tag}", preimage(np.full(n, base))))
    for k in range(8):
        common = (int(FIXED_IMAGE) >> (8 * k)) & 255
        img = np.full(n, FIXED_IMAGE)
        img[n - 1] = _with_byte(FIXED_IMAGE, k, common - 1)
        cases.append((f"byte {k} one smaller, last", preimage(img)))
        img = np.full(n, FIXED_IMAGE)
        img[0] = _with_byte(FIXED_IMAGE, k, common + 1)
        cases.append((f"byte {k} one larger, first", preimage(img)))
    return cases


def check_single_byte_passes(ops, n):
    cases = single_byte_cases(n)
    for name, kb in cases:
        gk, gv = sorted_right(ops, kb, f"single byte n={n} {name}")
        if name.startswith("identical"):
            assert np.array_equal(gv, np.arange(n)), f"single byte n={n} {name}: eight copies are the identity"
    return len(cases)


# =====================================================================================================================
# 3. tile counts around the eight XCDs, the chunk seam, payload bits
# =====================================================================================================================
SEAM_SIZES = tuple([1, 2, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, TILE - 1, TILE, TILE + 1]
                   + [t * TILE + r for t in (7, 8, 9, 15, 16, 17) for r in (-1, 0, 1)])
SPECIAL_PAYLOADS = (I64_MIN, -1, (1 << 32) + 5, (1 << 40) + (1 << 31), 2 ** 63 - 1)


def seam_input(n, seed=0):
    """Keys from a pool of 257 distinct random bit patterns (ties everywhere, every byte varies); payloads random int64
    with INT64_MIN, -1 and values above 2^32 among them (as many of those as n has room for)."""
    rng = np.random.default_rng([n, seed, 3])
    pool = np.unique(random_bits(rng, 300))[:257]
    assert len(pool) == 257
    kb = rng.permutation(pool)[rng.integers(0, 257, size=n)]
    vals = rng.integers(I64_MIN, 2 ** 63 - 1, size=n, dtype=np.int64, endpoint=True)
    spots = rng.permutation(n)[:len(SPECIAL_PAYLOADS)]
    vals[spots] = SPECIAL_PAYLOADS[:len(spots)]
    return kb, vals


def check_tile_and_chunk_seams(ops, n):
    """The only body whose payload is not arange: all 64 bits and the sign of every payload must arrive.  Stability is
    checked through a second sort of the same keys with arange payloads."""
    kb, vals = seam_input(n)
    gk, gv = run_sort(ops, kb, vals)
    against_argsort(kb, vals, gk, gv, f"seams n={n}, random payloads")
    sorted_right(ops, kb, f"seams n={n}, arange payloads")


# =====================================================================================================================
# 4. skewed digits
# =====================================================================================================================
SKEW_N = 5 * TILE


def skewed_cases(seed=0):
    """The upper seven bytes come from 1,024 patterns, so that keys tie there and the low byte decides their order."""
    rng = np.random.default_rng([seed, 4])
    tile = np.arange(SKEW_N) // TILE
    upper = lambda: (random_bits(rng, 1024) & ~U64(255))[rng.integers(0, 1024, size=SKEW_N)]  # noqa: E731
    # (a) a whole tile whose keys share their low byte while the other tiles differ: every pass still scatters, and in
    #     that tile each wavefront's counter of the digit reaches 1,024
    a = upper() | np.where(tile == 2, U64(0x37), rng.integers(0, 256, size=SKEW_N).astype(U64))
    # (b) low byte = tile index: a digit's row of tile counts is 4,096 in one tile and 0 elsewhere
    b = upper() | tile.astype(U64)
    return [("one tile, one low byte", preimage(a)), ("low byte = tile index", preimage(b))]


def check_skewed_digits(ops):
    for name, kb in skewed_cases():
        sorted_right(ops, kb, f"skewed digits, {name}")


# =====================================================================================================================
# 5. the scan's rounds (device only: the stand-in has no tiles)
# =====================================================================================================================
SCAN_TILES = (SCAN_ROUND - 1, SCAN_ROUND, SCAN_ROUND + 1, 2 * SCAN_ROUND + 1)  # 2,047, 2,048, 2,049 and 4,097: 1, 1, 2, 3 rounds
SCAN_LAST = 5  # keys of the last tile
SCAN_MODES = ("pool", "every 256th tile")


def scan_input(tiles, mode, seed=0):
    n = (tiles - 1) * TILE + SCAN_LAST
    rng = np.random.default_rng([tiles, seed, 5, SCAN_MODES.index(mode)])
    if mode == "pool":  # 2^20 distinct-ish bit patterns: ties, every byte varies, every tile holds every digit
        return random_bits(rng, 1 << 20)[rng.integers(0, 1 << 20, size=n)]
    # byte 0 of the image = tile index mod 256: a digit's row of tile counts is non-zero only at every 256th tile, so
    # what one round hands to the next is a handful of full tiles; the upper bytes are random
    img = _with_byte(random_bits(rng, n), 0, ((np.arange(n, dtype=np.int64) >> 12) & 255).astype(U64))
    return preimage(img)


def check_scan_rounds(ops, tiles, mode):
    """k_sort_scan carries a running total from one round of 2,048 tiles to the next: 4,097 tiles (16.8 M keys) is three
    rounds, the smallest size at which a carry that forgets the earlier rounds shows.  arange payloads, the properties."""
    kb = scan_input(tiles, mode)
    assert -(-len(kb) // TILE) == tiles and len(kb) % TILE == SCAN_LAST
    sorted_right(ops, kb, f"scan rounds tiles={tiles} {mode}")


# =====================================================================================================================
# 6. the C entry point: work buffer, output views, refusals
# =====================================================================================================================
def work_bytes_restated(n):
    """sort_plan of csrc/bk_sort.hip: keys and payloads in flight (256-byte multiples), the digit-major tile histogram,
    256 totals + 256 bases + done + same."""
    if n <= 0:
        return 0
    if n > 0x7FFFFFFF:
        return -1
    arr = -(-n * 8 // 256) * 256
    tiles = -(-n // TILE)
    return 2 * arr + tiles * BINS * 4 + (2 * BINS + 2) * 4  # (tiles * 1,024 is a multiple of 256 as it stands)


def _clib(ops):
    """The C entry points: the loaded library, or the stand-in's restatement of the three used here."""
    return ops.sort_lib if hasattr(ops, "sort_lib") else ops.lib


def _stream(ops):
    return ops._s() if hasattr(ops, "_s") else None


class _SortCall:
    """One problem's buffers for direct calls of _clib(ops).bk_sort_by_key: `work` is exactly work_bytes(n) bytes, 16-byte
    aligned, inside a byte buffer filled with 0xA5; keys_out / vals_out are the first n cells of sentinel-filled n + 3."""
    GUARD = 64

    def __init__(self, ops, n):
        self.ops, self.n = ops, n
        self.nb = int(_clib(ops).bk_sort_by_key_work_bytes(n))
        assert self.nb == work_bytes_restated(n), ("bk_sort_by_key_work_bytes", n, self.nb, work_bytes_restated(n))
        self.raw = torch.full((self.nb + 2 * self.GUARD + 16,), 0xA5, dtype=torch.uint8, device=ops.device)
        self.off = self.GUARD + (-(self.raw.data_ptr() + self.GUARD)) % 16
        self.work = self.raw.data_ptr() + self.off
        assert self.work % 16 == 0 and self.off >= self.GUARD and self.off + self.nb + self.GUARD <= self.raw.numel()
        self.ko = keys_tensor(np.full(n + 3, KEY_SENTINEL), ops)
        self.vo = torch.full((n + 3,), VAL_SENTINEL, dtype=torch.int64, device=ops.device)

    def call(self, k, v, n=None, work=None, work_bytes=None, keys_out=None):
        return _clib(self.ops).bk_sort_by_key(k.data_ptr(), self.ko.data_ptr() if keys_out is None else keys_out, v.data_ptr(),
                                              self.vo.data_ptr(), self.n if n is None else n,
                                              self.work if work is None else work,
                                              self.nb if work_bytes is None else work_bytes, _stream(self.ops))

    def guards_intact(self, what):
        raw = self.raw.cpu().numpy()
        assert (raw[:self.off] == 0xA5).all(), f"{what}: a write before the work buffer"
        assert (raw[self.off + self.nb:] == 0xA5).all(), f"{what}: a write behind the work buffer"

    def outputs(self, what):
        gk, gv = bits(self.ko), self.vo.cpu().numpy()
        assert (gk[self.n:] == KEY_SENTINEL).all() and (gv[self.n:] == VAL_SENTINEL).all(), f"{what}: a write behind the outputs"
        return gk[:self.n].copy(), gv[:self.n].copy()

    def outputs_untouched(self, what):
        assert (bits(self.ko) == KEY_SENTINEL).all() and (self.vo.cpu().numpy() == VAL_SENTINEL).all(), \
            f"{what}: a refused call wrote to its outputs"


def check_work_buffer_and_views(ops, n=2 * TILE + 5):
    rng = np.random.default_rng([n, 6])
    # first sort: doubles in [1, 2) -- the top byte of every image is 0xbf, so the last pass is a `same` pass and leaves
    # its flag set in `work`; the second sort, random bit patterns, reuses that `work` as it is
    first = (U64(0x3FF0000000000000) | (random_bits(rng, n) >> U64(12)))
    assert len(np.unique(image(first) >> U64(56))) == 1 and len(np.unique((image(first) >> U64(48)) & U64(255))) > 1
    second = random_bits(rng, n)
    c = _SortCall(ops, n)
    vals = np.arange(n, dtype=np.int64)
    v = torch.from_numpy(vals.copy()).to(ops.device)
    for name, kb in (("first sort (ends on a same pass)", first), ("second sort on the same work", second)):
        k = keys_tensor(kb, ops)
        assert c.call(k, v) == 0, name
        gk, gv = c.outputs(name)
        c.guards_intact(name)
        against_argsort(kb, vals, gk, gv, f"work buffer: {name}")
        assert np.array_equal(bits(k), kb) and np.array_equal(v.cpu().numpy(), vals), f"{name}: the inputs changed"
    # the refusals: BK_E_ARG and nothing written
    r = _SortCall(ops, n)
    k = keys_tensor(second, ops)
    refusals = (("work one byte short", dict(work_bytes=r.nb - 1)),
                ("work off by 8 bytes", dict(work=r.work + 8)),
                ("keys_in == keys_out", dict(keys_out=k.data_ptr())),
                ("n = 2**31", dict(n=2 ** 31, work_bytes=2 ** 40)))
    for name, kw in refusals:
        assert r.call(k, v, **kw) == BK_E_ARG, f"{name}: not refused"
        r.outputs_untouched(name)
        r.guards_intact(name)
        assert np.array_equal(bits(k), second), f"{name}: the inputs changed"
    assert _clib(ops).bk_sort_by_key_work_bytes(2 ** 31) == -1 and _clib(ops).bk_sort_by_key_work_bytes(0) == 0
    return len(refusals)


# =====================================================================================================================
# 7. bk_count_below
# =====================================================================================================================
COUNT_M = (1, 63, 64, 65, 129)
DBL_MAX = np.finfo(np.float64).max


def count_below_keys():
    """-> [ascending float64 arrays, positive NaNs (if any) at the end]: n = 0, 1, 1, 2, 2 and 4,097 with runs of up to
    1,000 duplicates."""
    rng = np.random.default_rng(7)
    runs = [(-np.inf, 3), (-DBL_MAX, 2), (-5.0, 1000), (-5e-324, 1), (-0.0, 2), (0.0, 2), (5e-324, 1), (1.5, 500),
            (np.nextafter(1.5, 2.0), 1), (3.0, 999), (DBL_MAX, 2), (np.inf, 3), (np.nan, 5)]
    fixed = np.concatenate([np.full(c, v) for v, c in runs])
    filler = np.round(rng.normal(size=4097 - len(fixed)), 1) + 0.05  # (short runs between the long ones, none of their values)
    big = np.concatenate([fixed, filler])
    big = big[np.argsort(image(big.view(U64)), kind="stable")]  # every NaN here is positive: ascending, NaNs last
    assert len(big) == 4097 and np.isnan(big[-5:]).all() and not np.isnan(big[:-5]).any() and np.all(big[1:-5] >= big[:-6])
    return [np.zeros(0), np.array([1.5]), np.array([np.nan]), np.array([1.5, 1.5]), np.array([0.0, np.nan]), big]


def count_below_queries(keys):
    """Every distinct key, the next double below and above each, -inf, +inf, -0.0, +0.0, DBL_MAX and NaN."""
    d = np.unique(keys[~np.isnan(keys)])
    with np.errstate(over="ignore"):
        q = np.concatenate([d, np.nextafter(d, -np.inf), np.nextafter(d, np.inf), [-np.inf, np.inf, -0.0, 0.0, DBL_MAX, np.nan]])
    return q


def count_below_reference(keys, q):
    """The kernel's own definition: the number of k with keys[k] < q in IEEE comparison.  A NaN query compares false with
    everything and gives 0 (np.searchsorted gives n); NaN keys are below nothing."""
    with np.errstate(invalid="ignore"):
        return np.array([int((keys < v).sum()) for v in q], dtype=np.int64)


def _count_into(ops, k, q, m):
    """bk_count_below through the C entry point into the first m cells of a sentinel vector."""
    out = SlackVec(ops, m, dtype=torch.int64)
    qt = dev(q, ops)
    assert _clib(ops).bk_count_below(k.data_ptr() if k.numel() else 0, k.numel(), qt.data_ptr(), m, out.t.data_ptr(), _stream(ops)) == 0
    return out.take(f"count_below m={m}")


def check_count_below(ops):
    cases = 0
    for keys in count_below_keys():
        n = len(keys)
        q = count_below_queries(keys)
        want = count_below_reference(keys, q)
        assert want[-1] == 0  # (the NaN query)
        k = dev(keys, ops)
        _same(ops.count_below(k, dev(q, ops)).cpu().numpy(), want, f"count_below n={n}, every query")
        for m in COUNT_M:  # the 64-thread launch seam; the NaN query in the last cell
            qm = np.resize(np.roll(q, -m), m)
            qm[-1] = np.nan
            _same(_count_into(ops, k, qm, m), count_below_reference(keys, qm), f"count_below n={n} m={m}")
            cases += 1
    return cases


# =====================================================================================================================
# 8. bk_scatter_ranks
# =====================================================================================================================
SCATTER_N = (1, 255, 256, 257, 70_001)
SCATTER_BASE = (0.0, 10.0, float(2 ** 31 * 8))  # every base + j + 1 is an integer below 2^53: exact


def check_scatter_ranks(ops):
    for n in SCATTER_N:
        rng = np.random.default_rng([n, 8])
        perm = rng.permutation(n).astype(np.int64)
        p = torch.from_numpy(perm).to(ops.device)
        for base in SCATTER_BASE:
            out = SlackVec(ops, n)
            ops.scatter_ranks(p, base, out.t)
            want = np.empty(n)
            want[perm] = base + np.arange(1, n + 1, dtype=np.float64)
            _same(out.take(f"scatter_ranks n={n}").view(U64), want.view(U64), f"scatter_ranks n={n} base={base}")
        # a permutation of a subset of [0, n + 3): only the named cells are written
        m = max(1, (n + 3) // 2)
        sub = rng.permutation(n + 3)[:m].astype(np.int64)
        buf = torch.full((n + 3,), float("nan"), dtype=torch.float64, device=ops.device)
        ops.scatter_ranks(torch.from_numpy(sub).to(ops.device), 10.0, buf)
        want = np.full(n + 3, np.nan)
        want[sub] = 10.0 + np.arange(1, m + 1, dtype=np.float64)
        got = buf.cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(want)), f"scatter_ranks n={n}: cells outside the payload written"
        _same(got[sub].view(U64), want[sub].view(U64), f"scatter_ranks n={n}, subset")
    return len(SCATTER_N) * (len(SCATTER_BASE) + 1)


# =====================================================================================================================
# 9. pooled ranks against NumPy
# =====================================================================================================================
def pooled_input(n, seed=0):
    """Heavy ties with NaNs of both signs, -0.0 / +0.0 and both infinities scattered in."""
    rng = np.random.default_rng([n, seed, 9])
    v = np.round(rng.normal(size=n), 1)
    special = np.array([np.nan, np.copysign(np.nan, -1.0), 0.0, -0.0, np.inf, -np.inf])
    spots = rng.permutation(n)[:n // 4]
    v[spots] = special[rng.integers(0, 6, size=len(spots))]
    assert (np.isnan(v) & np.signbit(v)).any() and (np.isnan(v) & ~np.signbit(v)).any()
    return v


def numpy_ranks(flat):
    """rhat.py:51-52 with the tie order the docstring of rank_chains promises: order of appearance."""
    return (np.argsort(flat, kind="stable").argsort() + 1).astype(np.float64)


def check_pooled_ranks_against_numpy(ops):
    flat = pooled_input(5000)
    want = numpy_ranks(flat)
    _same(dg._ranks_pooled(dev(flat, ops), ops).cpu().numpy(), want, "pooled ranks, _ranks_pooled")
    got = dg.rank_chains([flat[:1234], flat[1234:]], ops=ops)  # two ragged chains, pooled in order
    _same(np.concatenate(got), want, "pooled ranks, rank_chains of two chains")
    N, C = 200, 37
    x = pooled_input(N * C, seed=1).reshape(N, C)
    x[:, 5] = np.where(np.arange(N) % 3 == 0, np.copysign(np.nan, -1.0), np.nan)  # one column all NaN, both signs
    x[:, 11] = 0.7                                                                  # one column constant
    want = numpy_ranks(x.T.reshape(-1)).reshape(C, N).T
    _same(dg.rank_chains(dev(x, ops), ops=ops).cpu().numpy(), want, "pooled ranks, rank_chains [N, C]")
