"""tests/mala_kernel_parity.py without a GPU: every check at the small shapes on the NumPy stand-in (the device's summation order),
the launch forms each listed shape reaches, stand-ins with one defect planted -- each must be caught --, and the step kernels'
offset guard against the offsets restated with Python integers."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import mala_adapt_parity as ap
from tests import mala_kernel_parity as mk
from tests.fake_ops_mala_adapt import MalaAdaptFakeOps, _residuals, step_slots, step_sum

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LIM = 2 ** 32


@pytest.fixture(scope="module")
def fake():
    return MalaAdaptFakeOps()


def _read(name):
    with open(os.path.join(ROOT, "bayes-kit_amd", "csrc", name)) as f:
        return f.read()


# ---- the bodies on the stand-in ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", mk.KINDS)
def test_planted_thresholds(fake, kind):
    worst = 0.0
    for D in mk.PLANT_D:
        for C in mk.PLANT_C + (mk.PLANT_C_AT_65 if D == 65 else ()):
            worst = max(worst, mk.check_planted(fake, kind, C, D))
    mk.say(f"planted thresholds, {kind}", worst)


@pytest.mark.parametrize("kind", mk.KINDS)
def test_layouts_and_guard_cells(fake, kind):
    for D in mk.LAYOUT_D:
        for C in mk.LAYOUT_C:
            mk.check_layouts(fake, kind, C, D)


@pytest.mark.parametrize("kind", mk.KINDS)
def test_nonfinite_values_and_the_pair_partner(fake, kind):
    for C, D in mk.NONFINITE_SHAPES:
        mk.check_nonfinite(fake, kind, C, D)


def test_small_kernels(fake):
    worst = max(mk.check_logq(fake, C, D) for D in mk.LOGQ_D for C in mk.LOGQ_C)
    mk.say("bk_mala_logq", worst)
    mk.check_logq_no_dims(fake)
    for C, D in mk.PROPOSE_Z_SHAPES:
        mk.check_propose_from_normals(fake, C, D)
    for C, D in mk.PROPOSE_SHAPES:
        mk.check_propose(fake, C, D)


# ---- the forms -------------------------------------------------------------------------------------------------------------------
def test_each_listed_shape_reaches_the_form_named_for_it():
    assert [step_slots(D) for D in mk.PLANT_D] == [2, 2, 2, 2, 2, 2, 2, 4, 4, 4, 8, 8, 8, 16, 16, 16]
    assert [mk.step_form("step", C, 65)[1] for C in mk.PLANT_C_AT_65] == [1, 1, 1, 2, 7, 8, 9, 16, 17]
    assert [mk.step_form("step", C, 65)[1] for C in mk.PLANT_C] == [2, 9]
    assert [step_slots(D) for D in mk.LAYOUT_D] == [2, 2, 4, 16]
    want = {("step", 128): (32768, 32770), ("step", 256): (16384, 16386), ("step", 512): (8192, 8194),
            ("step", 1024): (4096, 4098), ("gauss", 128): (49152, 49154), ("gauss", 256): (24576, 24578),
            ("gauss", 512): (12288, 12290), ("gauss", 1024): (6144, 6146)}
    seen = {}
    for kind, C, D, streams in mk.SEAMS:
        E, blocks, nt = mk.step_form(kind, C, D)
        assert nt == streams and E == {128: 2, 256: 4, 512: 8, 1024: 16}[D] and blocks == -(-C // 16)
        seen.setdefault((kind, D), []).append(C)
        h = C // 4 * 2   # the halves of check_seam: even, resident, and a ragged or whole number of blocks
        assert h % 2 == 0 and not mk.step_form(kind, h, D)[2] and not mk.step_form(kind, C - h, D)[2]
    assert {k: tuple(v) for k, v in seen.items()} == want
    # none of the small shapes streams, whatever the kind
    assert not any(mk.step_form(k, 258, 1024)[2] for k in mk.KINDS)
    # the restated choices are the source's
    step, sep, common = _read("bk_mala.hip"), _read("bk_mala_step.hpp"), _read("bk_common.hpp")
    assert "return elems * 8 > ((i64)192 << 20);" in common
    assert "const bool nt = bk_streams_past_llc(6 * C * D);" in step and "const bool nt = bk_streams_past_llc(4 * C * D);" in sep
    assert "dim3 grid((unsigned)bk_cdiv(C, MS_CHAINS))" in step and "constexpr int MS_CHAINS = 2 * MS_PAIRS;" in step
    for src, m in ((step, "BK_MS_LAUNCH"), (sep, "BKM_LAUNCH")):
        assert f"if (D <= 128) {m}(2);\n  else if (D <= 256) {m}(4);\n  else if (D <= 512) {m}(8);\n  else {m}(16);" in src
        assert "const unsigned per = gridDim.x / 8u;\n    if (bid < per * 8u) bid = (bid % 8u) * per + bid / 8u;" in src
    assert "return D <= 128 ? 2 : D <= 256 ? 4 : D <= 512 ? 8 : 16;" in common


def test_xcd_walk_is_a_permutation_with_both_kinds_of_block():
    for blocks in (1, 2, 7, 8, 9, 16, 17, 2048, 2049):
        m = mk.xcd_map(blocks)
        assert sorted(m) == list(range(blocks))
    assert mk.xcd_map(7) == list(range(7))                       # per = 0: nothing remapped
    assert mk.xcd_map(9) == [0, 1, 2, 3, 4, 5, 6, 7, 8]          # per = 1: remapped onto themselves, block 8 kept
    m = mk.xcd_map(17)                                            # per = 2: workgroup b -> (b % 8) * 2 + b / 8, block 16 kept
    assert m[1] == 2 and m[8] == 1 and m[15] == 15 and m[16] == 16


# ---- planted defects -------------------------------------------------------------------------------------------------------------
def _sequential(x):
    s = np.zeros(x.shape[1])
    for d in range(x.shape[0]):
        s = s + x[d]
    return s


def _groups_reversed(x):
    D, C = x.shape
    E = step_slots(D)
    pad = np.zeros((64 * E, C))
    pad[:D] = x
    s = np.zeros((64, C))
    for e in range(E):
        s = s + pad.reshape(E, 64, C)[e]
    g = s.reshape(8, 8, C)
    g = ((g[:, 0] + g[:, 1]) + (g[:, 2] + g[:, 3])) + ((g[:, 4] + g[:, 5]) + (g[:, 6] + g[:, 7]))
    t = g[7]
    for k in range(6, -1, -1):
        t = t + g[k]
    return t


def _last_slot_dropped(x):
    y = x.copy()
    y[64 * (step_slots(x.shape[0]) - 1):] = 0.0
    return step_sum(y)


class Planted(MalaAdaptFakeOps):
    """The stand-in's step with ONE defect."""

    def __init__(self, defect):
        super().__init__()
        self.defect = defect

    def _step(self, theta, theta_out, grad, theta_prop, grad_prop, lp, lp_prop, log_u, zt_next, eps, sqrt2eps, mask, ret,
              count, pd):
        d = self.defect
        th, g, thp, gp = theta.numpy(), grad.numpy(), theta_prop.numpy(), grad_prop.numpy()
        D, C = th.shape
        tf, tr = _residuals(th, g, thp, gp, eps, pd)
        if d == "forward and reverse swapped":
            tf, tr = tr, tf
        ssum = {"sequential sum": _sequential, "row groups combined in reverse": _groups_reversed,
                "last slot dropped": _last_slot_dropped}.get(d, step_sum)
        k = -0.25 / eps
        l0, l1, lu = lp.numpy().copy(), lp_prop.numpy(), log_u.numpy()
        with np.errstate(invalid="ignore", over="ignore"):
            T = (l1 - l0) + (k * ssum(tr) - k * ssum(tf))
            acc = lu <= T if d == "<= for <" else lu < T
        if d == "a bad chain's partner refused with it":
            bad = ~(np.isfinite(T) & np.isfinite(lu))
            acc = acc & ~bad[np.arange(C) ^ 1]
        new_th = np.where(acc[None, :], thp, th)
        new_g = g.copy() if d == "gradient not selected on accept" else np.where(acc[None, :], gp, g)
        theta_out.numpy()[...] = new_th
        grad.numpy()[...] = new_g
        lp.numpy()[...] = np.where(acc, l1, l0)
        if ret is not None:
            ret.numpy()[...] = l1 if d == "ret = lp' regardless of the decision" else lp.numpy()
        if mask is not None:
            mask.numpy()[...] = acc
        if count is not None:
            if d == "count overwritten instead of added to":
                count.fill_(int(acc.sum()))
            else:
                count += int(acc.sum())
        if zt_next is not None:
            z = zt_next.numpy()[:, :D].T
            if d == "normals read with pitch D instead of ldz":
                z = torch.as_strided(zt_next, (C, D), (D, 1)).numpy().T
            base = th if d == "next proposal formed from the old state" else new_th
            if pd is None:
                theta_prop.numpy()[...] = (base + eps * new_g) + sqrt2eps * z
            else:
                theta_prop.numpy()[...] = (base + eps * (pd[0][:, None] * new_g)) + sqrt2eps * (pd[1][:, None] * z)
        cells = theta_out.untyped_storage().nbytes() // 8
        for name, cell in (("a write into a pad column", theta_out.storage_offset() + C),
                           ("a write into row D", theta_out.storage_offset() + D * theta_out.stride(0))):
            if d == name and cell < cells and (name.endswith("row D") or theta_out.stride(0) > C):
                torch.as_strided(theta_out, (1,), (1,), cell).fill_(0.0)


BODIES = {
    "planted": lambda o: [mk.check_planted(o, "step", 18, 65), mk.check_planted(o, "gauss_precond", 130, 129)],
    "layouts": lambda o: [mk.check_layouts(o, "step", 18, 33), mk.check_layouts(o, "gauss", 18, 33)],
    "nonfinite": lambda o: mk.check_nonfinite(o, "step", 18, 65),
}
DEFECTS = [("sequential sum", "planted"), ("row groups combined in reverse", "planted"), ("last slot dropped", "planted"),
           ("<= for <", "planted"), ("forward and reverse swapped", "planted"),
           ("gradient not selected on accept", "planted"), ("next proposal formed from the old state", "planted"),
           ("normals read with pitch D instead of ldz", "planted"), ("a write into a pad column", "layouts"),
           ("a write into row D", "layouts"), ("count overwritten instead of added to", "layouts"),
           ("ret = lp' regardless of the decision", "planted"), ("a bad chain's partner refused with it", "nonfinite")]


@pytest.mark.parametrize("defect,body", DEFECTS)
def test_planted_defect_is_caught(defect, body):
    with pytest.raises(AssertionError):
        BODIES[body](Planted(defect))


def test_the_defect_harness_passes_without_a_defect():
    for body in BODIES.values():
        body(Planted(None))
    assert len(DEFECTS) == 13 and len({d for d, _ in DEFECTS}) == 13


# ---- F. the guard follows from the offsets ------------------------------------------------------------------------------------------
def _basic(C, D, ld):
    return C > 0 and 0 < D <= 1024 and C % 2 == 0 and ld % 2 == 0 and ld >= C


def _largest_ld(D):
    """The largest even ld = C whose state offsets stay below 2**32."""
    lo, hi = 2, 2 ** 31
    while hi - lo > 2:
        mid = (lo + hi) // 4 * 2
        lo, hi = (mid, hi) if mk.step_offsets(mid, D, mid) < LIM else (lo, mid)
    return lo


def _grid():
    pts = [(4_400_000, 32, 4_400_000), (65_536, 1024, 65_536), (65_536, 1024, 65_536 + 144), (400_000 - 6, 513, 400_000)]
    for D in (1, 32, 63, 64, 128, 129, 256, 257, 512, 513, 1023, 1024):
        for b in (_largest_ld(D), (2 ** 28 - 1) // D // 2 * 2):
            for ld in (b - 2, b, b + 2, b + 4):
                pts += [(ld, D, ld), (ld - 2, D, ld), (ld // 16 * 16, D, ld), (ld // 2 // 2 * 2, D, ld)]
    return pts


def test_supported_shapes_form_no_offset_past_32_bits():
    """bk_mala_step_supported => every offset of the state arrays, with the access width, below 2**32 (restated with Python
    integers); the refusing side through the four entry points on a dummy buffer: BK_E_ALIGN before any HIP call.  Nothing is
    launched at these sizes."""
    from bayes_kit_amd import _lib

    lib = _lib.load()
    fake = MalaAdaptFakeOps()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    E_ALIGN = -2

    def refused(C, D, ld, zt=None, ldz=0):
        r = [lib.bk_mala_step(p, p, p, p, p, ld, p, p, p, zt, ldz, 0.1, 0.4, None, None, None, C, D, None),
             lib.bk_mala_step_precond(p, p, p, p, p, ld, p, p, p, p, zt, ldz, 0.1, 0.4, None, None, None, C, D, None),
             lib.bk_mala_step_gaussian(p, p, p, ld, p, p, p, p, zt, ldz, 0.1, 0.4, None, None, None, C, D, None),
             lib.bk_mala_step_gaussian(p, p, p, ld, None, p, p, p, zt, ldz, 0.1, 0.4, None, None, None, C, D, None),
             lib.bk_mala_step_gaussian_precond(p, p, p, ld, p, p, p, p, p, zt, ldz, 0.1, 0.4, None, None, None, C, D, None)]
        return all(x == E_ALIGN for x in r)

    n_yes = n_no = n_z = 0
    for C, D, ld in _grid():
        ok = bool(lib.bk_mala_step_supported(C, D, ld))
        assert ok == fake.mala_step_supported(C, D, ld), (C, D, ld)
        fits = _basic(C, D, ld) and mk.step_offsets(C, D, ld) < LIM
        assert fits or not ok, (C, D, ld, mk.step_offsets(C, D, ld))            # supported => every offset fits
        assert ok == (fits and D * ld < 2 ** 28), (C, D, ld)                     # ... and nothing else is given up
        if not ok:
            assert refused(C, D, ld), (C, D, ld)
            n_no += 1
            continue
        n_yes += 1
        # the normals: ldz on either side of both of their bounds, refused where an offset would reach 2**32
        E = step_slots(D)
        edge = [(LIM // 8 - D) // (C - 1) // 2 * 2, (LIM - 16 * 64 - 1024 * (E // 2 - 1)) // 8 // (C - 1) // 2 * 2] if C > 2 else []
        for b in edge:
            for ldz in (b - 2, b, b + 2, b + 4):
                if ldz >= D and mk.step_offsets(C, D, ld, ldz) >= LIM:
                    assert refused(C, D, ld, p, ldz), (C, D, ld, ldz)
                    n_z += 1
        for ldz in ((D + 7) // 8 * 8, 64 * E):                                   # the samplers' pitch never adds a restriction
            assert mk.step_offsets(C, D, ld, ldz) < LIM, (C, D, ld, ldz)
    assert n_yes > 50 and n_no > 50 and n_z > 50
    # the two examples: rows past D at a small D, and the normals of many chains
    assert not lib.bk_mala_step_supported(4_400_000, 32, 4_400_000) and 127 * 4_400_000 * 8 > LIM
    # (65,536 chains with ldz = 8,192: the last chain's row starts 65,536 bytes below 2**32 and D <= 1024 normals still fit;
    # one even pitch further they do not)
    assert lib.bk_mala_step_supported(65_536, 1024, 65_536) and mk.step_offsets(65_536, 1024, 65_536, 8192) < LIM
    assert mk.step_offsets(65_536, 1024, 65_536, 8194) >= LIM and refused(65_536, 1024, 65_536, p, 8194)
    assert mk.step_offsets(65_538, 1024, 65_538, 8192) >= LIM and refused(65_538, 1024, 65_538, p, 8192)
    # a ragged last block's dropped stores: num_records + the slot offset wrapped back inside the array
    assert (512 * 400_000 + 399_994) * 8 + 15 * 64 * 400_000 * 8 > LIM and not lib.bk_mala_step_supported(399_994, 513, 400_000)
    # the benchmarked shape (with the sampler's row padding and without) and every shape of the suite stay supported
    for C, D, ld in [(65_536, 1024, 65_536), (65_536, 1024, 65_536 + 144)] + \
            [(C, D, C) for C, D, _, _ in ap.STEP_SHAPES] + \
            [(C, D, C + 6) for D in mk.PLANT_D + mk.LAYOUT_D for C in mk.PLANT_C_AT_65] + \
            [(C, D, C) for _, C, D, _ in mk.SEAMS]:
        assert lib.bk_mala_step_supported(C, D, ld) and fake.mala_step_supported(C, D, ld), (C, D, ld)


def test_logq_without_dimensions_writes_nothing_and_launches_nothing():
    from bayes_kit_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_double * 16)(*([7.0] * 16))
    p = ctypes.addressof(buf)
    assert lib.bk_mala_logq(p, p, p, p, 4, 0.1, p, p, 4, 0, None) == 0
    assert lib.bk_mala_logq_precond(p, p, p, p, 4, p, 0.1, p, p, 4, 0, None) == 0
    assert list(buf) == [7.0] * 16


class _Refusing(MalaAdaptFakeOps):
    """A library whose step kernel does not take the shape asked for (what (4,400,000 x 32) is to the device)."""

    def mala_step_supported(self, C, D, ld):
        return False


def test_sampler_takes_the_step_by_step_path_at_an_unsupported_shape():
    C, D = 16, 40
    s = ap.make(_Refusing(), C, D)
    assert s.path == "step-by-step"
    want = ap.make(MalaAdaptFakeOps(), C, D, two_pass=False)
    assert MalaAdaptFakeOps().mala_step_supported(C, D, C) and ap.make(MalaAdaptFakeOps(), C, D).path != "step-by-step"
    for x, y in zip(ap.run_draws(s, 3), ap.run_draws(want, 3)):
        assert np.array_equal(x, y)
    with pytest.raises(ValueError, match="two_pass=True needs"):
        ap.make(_Refusing(), C, D, two_pass=True)
    assert not MalaAdaptFakeOps().mala_step_supported(4_400_000, 32, 4_400_000)
