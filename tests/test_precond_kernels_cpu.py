"""CPU side of the preconditioned HMC kernels' edge work: the checks of tests/precond_kernel_parity.py on the NumPy stand-in
(tests/fake_ops_adapt.AdaptFakeOps) at the small shapes -- which checks the bodies, the derived bound and the stand-in; the
kernels themselves are held to them in tests/test_gpu_precond_kernels.py --, the restated launch choices against the conditions
in csrc/ and against the forms the listed shapes claim, and the sensitivity of every layer: the bodies run on stand-ins with
one defect planted and must fail at the layer named."""
import os

import numpy as np
import pytest
import torch

from tests import precond_kernel_parity as pk
from tests.fake_ops_adapt import AdaptFakeOps, quarter_sum

CSRC = os.path.join(os.path.dirname(__file__), "..", "bayes-kit_amd", "csrc")


@pytest.fixture(scope="module")
def ops():
    return AdaptFakeOps()


# ---- the bodies on the stand-in -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", pk.FINISH_D)
def test_finish_body_on_the_stand_in(ops, D):
    for C in pk.FINISH_C:
        assert pk.check_finish_small(ops, C, D) < 1.0


@pytest.mark.parametrize("arrays", ["distinct", "inplace", "noout"])
def test_finish_seam_body_on_the_stand_in(ops, arrays):
    assert pk.check_finish_seam(ops, 130, 33, arrays, negate=arrays == "inplace") < 1.0


@pytest.mark.parametrize("D", pk.REFRESH_LANES_D + pk.REFRESH_ROWS_D)
def test_refresh_body_on_the_stand_in(ops, D):
    for C in (pk.REFRESH_LANES_C if D < 32 else pk.REFRESH_ROWS_C):
        assert pk.check_refresh(ops, C, D) < 1.0


@pytest.mark.parametrize("D", pk.REFRESH_PLAIN_D)
def test_refresh_body_on_the_stand_in_past_the_rows_kernel(ops, D):
    for C in pk.REFRESH_PLAIN_C:
        assert pk.check_refresh(ops, C, D) < 1.0


@pytest.mark.parametrize("C,D", pk.REFRESH_PCG)
def test_refresh_body_on_the_stand_in_pcg64(ops, C, D):
    assert pk.check_refresh(ops, C, D, pcg=True) < 1.0


@pytest.mark.parametrize("D", pk.DRAW_D)
def test_draw_body_on_the_stand_in(ops, D):
    for C in pk.DRAW_C[:4]:
        assert pk.check_draw(ops, C, D) < 1.0


def test_draw_body_on_the_stand_in_at_the_workgroup_switch(ops):
    assert pk.check_draw(ops, pk.DRAW_C[-1], 9) < 1.0


def test_the_bound_of_layer_2_on_the_stand_ins_arithmetic():
    """err / (u * ref) of the quarter-wise double sum against long double stays far inside Dq + 8 at every D from 1 to 1,024
    the checks' v and momenta."""
    rng = np.random.default_rng(1)
    worst = 0.0
    for D in list(range(1, 66)) + [127, 128, 129, 253, 256, 257, 1023, 1024]:
        v = pk.wide_v(D, rng)
        r = rng.normal(size=(D, 64)) * np.sqrt(v)[:, None]
        got = 0.5 * quarter_sum(r * ((1.0 / v)[:, None] * r))
        ref = np.longdouble(0.5) * pk.kin_terms(r, v).sum(axis=0)
        worst = max(worst, float(np.max(np.abs(got - ref) / (pk.U * ref))))
        assert pk.layer2(got, pk.kin_terms(r, v), f"D={D}") < 1.0
    print(f"[precond-kernels] largest err / (u ref), D = 1 .. 1024: {worst:.3g} (the bound is Dq + 8 = 9 .. 264)")


def test_host_subset_holds_the_ragged_groups_and_both_sides_of_every_boundary():
    assert np.array_equal(pk.host_subset(130), np.arange(130))
    for C in sorted({c for c, *_ in pk.FINISH_SEAMS} | {pk.REFRESH_LANES_BIG[0], pk.REFRESH_PLAIN_BIG[0], pk.REFRESH_NT[0]}):
        idx = pk.host_subset(C)
        s = set(idx.tolist())
        assert 512 <= len(s) == len(idx) <= 1024 and idx.min() == 0 and idx.max() == C - 1
        assert set(range(16)) <= s and set(range(C - 18, C)) <= s
        for c in s:
            assert c % 128 != 127 or c + 1 >= C or c + 1 in s
            assert c % 128 != 0 or c == 0 or c - 1 in s
        assert sum(1 for c in s if c % 128 == 0 and c > 0) >= 9


# ---- the restated launch choices ---------------------------------------------------------------------------------------------------
def _src(name):
    return open(os.path.join(CSRC, name)).read()


def test_the_restated_conditions_are_the_ones_in_the_sources():
    """Matches the source lines literally: meant to trip on any edit of them, so that whoever moves a threshold looks at the
    restatements in tests/precond_kernel_parity.py and moves the shapes with it."""
    integ, rng, elem, common = _src("bk_integrator.hip"), _src("bk_rng.hip"), _src("bk_elementwise.hpp"), _src("bk_common.hpp")
    assert "const bool vec = plain && C % 2 == 0 && ld % 2 == 0 && C * D >= ((i64)1 << 22) && bk_aligned16(rho_in) &&" in integ
    assert "(!grad || (ldg_c == 1 && ldg_d % 2 == 0 && bk_aligned16(grad)));" in integ
    assert "if (vec && !bk_streams_past_llc(bk_distinct_arrays({rho_in, rho_out, grad}) * C * D))" in integ
    assert "constexpr int FIN_UNROLL = 8;" in integ and "constexpr int BK_RED_T_CP = 8, BK_RED_T_U = 8;" in integ
    assert "return elems * 8 > ((i64)192 << 20);" in common
    assert "if (dp <= 128 && lds <= 65536)" in rng
    assert "const size_t lds = (size_t)(64 * (dp + 1) + 256) * sizeof(double);" in rng
    assert "else if (bk_streams_past_llc(bk_distinct_arrays({work, out, loc_in}) * C * D))" in rng
    assert "if (work && D >= 32 && work_elems >= bk_refresh_work_elems(C, D)) {" in rng
    assert "static inline int rng_block(i64 C) { return C <= 32768 ? 32 : 64; }" in rng
    assert "constexpr int RK_CH = 16;" in rng
    assert "const int tq_block = C * 4 <= 256 * BLOCK ? BK_WAVE : BLOCK;" in elem and "constexpr int BLOCK = 256;" in elem
    assert "constexpr int TQ_ROWS = 8;" in elem


def test_every_listed_shape_reaches_the_form_its_row_claims():
    n_arrays = {"distinct": 3, "inplace": 2, "noout": 2}
    # A: the small shapes are unaligned views: the scalar kernel, whatever the gradient's layout
    for C in pk.FINISH_C:
        for D in pk.FINISH_D:
            assert pk.finish_form(C, D, C + 7, 3, aligned=False, ldg_d=C + 7) == "scalar"
    assert all(C * D < 1 << 22 for C in pk.FINISH_C for D in pk.FINISH_D)
    seen = set()
    for C, D, arrays, form in pk.FINISH_SEAMS:
        assert C % 2 == 0
        assert pk.finish_form(C, D, C + 8, n_arrays[arrays], aligned=True, ldg_d=C + 8) == form, (C, D, arrays)
        assert pk.finish_form(C, D, C + 7, n_arrays[arrays], aligned=False, ldg_d=C + 7) == "scalar"
        seen.add(form)
    assert seen == {"scalar", "tile", "stream"}
    assert 16320 * 257 == 4_194_240 < 1 << 22 <= 16322 * 257 == 4_194_754 and 16322 == 16 * 1020 + 2
    assert 3 * 32634 * 257 * 8 < pk.LLC_BYTES < 3 * 32642 * 257 * 8 and 2 * 32642 * 257 * 8 < pk.LLC_BYTES
    # (the tile form walks a quarter in chunks of 8 * 8 = 64 rows: one chunk exactly, a short last quarter, two chunks)
    assert [(D + 3) // 4 for _, D, _, f in pk.FINISH_SEAMS if f == "tile"][:3] == [65, 64, 64] and 253 - 3 * 64 == 61
    # B
    work = lambda C, D: C * ((D + 7) // 8 * 8)  # noqa: E731
    for D in pk.REFRESH_LANES_D:
        for C in pk.REFRESH_LANES_C:
            assert pk.refresh_form(C, D, work_elems=work(C, D)) == pk.refresh_form(C, D) == "lanes"
            assert pk.refresh_rng_block(C) == 32
    C, D = pk.REFRESH_LANES_BIG
    assert pk.refresh_form(C, D, work_elems=work(C, D)) == "lanes" and pk.refresh_rng_block(C) == 64
    for C, D in pk.REFRESH_PCG:
        assert pk.refresh_form(C, D, philox=False, work_elems=work(C, D)) == "lanes"
    for D in pk.REFRESH_ROWS_D:
        for C in pk.REFRESH_ROWS_C:
            assert pk.refresh_form(C, D, work_elems=work(C, D)) == "rows"
            assert pk.refresh_form(C, D, work_elems=work(C, D) - 1) == "lanes"
    for D in pk.REFRESH_PLAIN_D:
        for C in pk.REFRESH_PLAIN_C:
            assert pk.refresh_form(C, D, work_elems=work(C, D)) == "plain"
            assert pk.refresh_form(C, D, work_elems=work(C, D) - 1) == "lanes"
    assert max(pk.REFRESH_ROWS_D) == 120 and min(pk.REFRESH_PLAIN_D) == 121  # the hand-over, crossed on both sides
    assert [(D + 3) // 4 for D in pk.REFRESH_PLAIN_D] == [31, 32, 33, 65]
    assert pk.refresh_form(*pk.REFRESH_PLAIN_BIG, work_elems=work(*pk.REFRESH_PLAIN_BIG)) == "plain"
    assert pk.refresh_form(*pk.REFRESH_NT, work_elems=work(*pk.REFRESH_NT)) == "nt"
    assert 2 * 48960 * 257 * 8 < pk.LLC_BYTES < 2 * 48962 * 257 * 8
    # C
    assert [pk.draw_block(C) for C in pk.DRAW_C] == [64, 64, 64, 64, 64, 256]


# ---- each layer notices a wrong kernel ---------------------------------------------------------------------------------------------
class Planted(AdaptFakeOps):
    """AdaptFakeOps with ONE defect planted in the three preconditioned entry points:
    sqrt_for_inverse   sqrt(v) read for 1/v in the kinetic energy
    association        (1/v) * (r * r) instead of r * ((1/v) * r)
    sequential         the per-chain sums taken sequentially in d instead of by quarters
    drops_a_row        the last row of the third quarter left out of the sums
    kick_sqrt          the kick taken with sqrt(v) instead of v"""

    def __init__(self, defect):
        super().__init__()
        self.defect = defect

    def _sum(self, x):
        if self.defect == "sequential":
            s = np.zeros(x.shape[1])
            for d in range(x.shape[0]):
                s = s + x[d]
            return s
        if self.defect == "drops_a_row":
            x = x.copy()
            x[3 * ((x.shape[0] + 3) // 4) - 1] = 0.0
        return quarter_sum(x)

    def _kin(self, r, precond):
        _, sd, vinv = self._pd(precond)
        w = (sd if self.defect == "sqrt_for_inverse" else vinv)[:, None]
        return 0.5 * self._sum(w * (r * r) if self.defect == "association" else r * (w * r))

    def _kick(self, precond):
        return precond[1] if self.defect == "kick_sqrt" else precond[0]

    def momentum_refresh_precond(self, kind, state, out, precond, kin_out, work=None):
        super().momentum_refresh_precond(kind, state, out, precond, kin_out, work)
        kin_out.numpy()[...] = self._kin(out.numpy(), precond)

    def leapfrog_finish_precond(self, rho_in, rho_out, grad, precond, half, negate, kin_out):
        r = rho_in.numpy().copy() if grad is None else rho_in.numpy() + half * (self._kick(precond).numpy()[:, None] * grad.numpy())
        if negate:
            r = -r
        if rho_out is not None:
            rho_out.numpy()[...] = r
        if kin_out is not None:
            kin_out.numpy()[...] = self._kin(r, precond)

    def hmc_draw_gaussian(self, theta_in, theta_out, rho_in, zt, lam, metric, eps, steps, part, kin0, kin1, lp_out,
                          accept=None, precond=None):
        D = theta_in.shape[0]
        sd = self._pd(precond)[1]
        r0 = torch.from_numpy(0.0 + sd[:, None] * zt.numpy()[:, :D].T) if zt is not None else rho_in
        r1 = torch.empty_like(theta_in)
        k0 = torch.from_numpy(self._kin(r0.numpy(), precond))
        if kin0 is not None:
            kin0.copy_(k0)
        self.hmc_trajectory_gaussian(theta_in, theta_out, r0, r1, lam, self._kick(precond), eps, steps)
        kin1.numpy()[...] = self._kin(r1.numpy(), precond)
        th = theta_out.numpy()
        lp_out.numpy()[...] = -0.5 * self._sum(th * (th if lam is None else lam.numpy()[:, None] * th))
        if accept is not None:
            lp_cur, log_u, mask, ret, count = accept
            self.mh_accept(0, lp_cur, k0, lp_out, kin1, log_u, mask, ret, count)


BODIES = {"finish": lambda o: pk.check_finish_small(o, 65, 33), "refresh": lambda o: pk.check_refresh(o, 65, 33),
          # (five steps: without a drift theta_out cannot show a wrong kick)
          "draw": lambda o: pk.check_draw(o, 65, 33, all_steps=(5,))}


@pytest.mark.parametrize("body", sorted(BODIES))
def test_the_planted_class_without_a_defect_passes(body):
    assert BODIES[body](Planted(None)) < 1.0


@pytest.mark.parametrize("body", sorted(BODIES))
@pytest.mark.parametrize("defect,layer", [("sqrt_for_inverse", 2), ("association", 3), ("sequential", 3), ("drops_a_row", 2),
                                          ("kick_sqrt", 1)])
def test_each_layer_notices_its_planted_defect(body, defect, layer):
    """The layers are asserted in the order 1, 2, 3: a failure at layer 3 is one that layers 1 and 2 let pass."""
    if (body, defect) == ("refresh", "kick_sqrt"):  # the refresh has no kick: the defect changes nothing there
        assert BODIES[body](Planted(defect)) < 1.0
        return
    with pytest.raises(AssertionError, match=rf"^layer {layer} \("):
        BODIES[body](Planted(defect))
