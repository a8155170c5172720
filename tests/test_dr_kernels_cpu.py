"""tests/dr_kernel_parity.py without a GPU: the checks pass with the NumPy stand-in as the library; the input builders reach
every branch of the stage kernels at every parametrisation tests/test_gpu_dr_kernels.py uses (a condition on the inputs, asserted
on the stand-in's outputs, so that a GPU pass cannot come from inputs that never left the common branch); no retry decision
lies within a last-bit difference of its threshold; and stand-ins with one planted fault each fail the checks."""
import math

import numpy as np
import pytest
import torch

from tests import dr_kernel_parity as dk
from tests.fake_ops import FakeOps


@pytest.fixture()
def ops():
    return FakeOps()


# ---- the parametrisations are the issue's ---------------------------------------------------------------------------------------
def test_the_listed_values():
    assert dk.LANE_SIZES == (1, 63, 64, 65, 255, 256, 257, 700, 1025) and dk.PAD == 37
    assert [dk.n_dev_value(257, w) for w in dk.N_DEV] == [None, 257, 262, 187, 0]
    assert [dk.lanes(257, w) for w in dk.N_DEV] == [257, 257, 257, 187, 0] and dk.lanes(63, "n-70") == 0
    assert dk.PROB_RETRY == (1.0, 0.0, 0.35) and dk.N_COUNTERS == (0, 1, 5, 64) and dk.STAGE_CHAINS == (1, 63, 64, 65, 700)
    assert dk.COMPACT_SIZES == (1, 7, 8, 9, 8191, 8192, 8193, 16384, 16385) and dk.DENSITIES == (0.0, 0.03, 0.5, 1.0)
    assert dk.SCATTER_DIMS == (0, 1, 7, 8, 9, 33) and dk.STEP_PADS == (0, 5, 6)
    assert dk.STEP_SHAPES == ((2, 1), (64, 3), (65, 4), (130, 5), (258, 33))
    assert (dk.F_SENT, dk.B_SENT, dk.I_SENT) == (7.0, 9, -1) and dk.RTOL == 1e-14 and dk.MARGIN == 1e-13


def test_the_accept_and_ghost_cases_cover_the_table():
    cases = dk.accept_cases()
    assert {(c.n, c.kind, c.n_dev) for c in cases if c.index} == {(n, k, w) for n in dk.LANE_SIZES for k in dk.KINDS for w in dk.N_DEV}
    for n in dk.LANE_SIZES:
        for kind in dk.KINDS:  # the three full-size forms of every size carry the three values of prob_retry
            assert {c.pr for c in cases if (c.n, c.kind) == (n, kind) and c.n_dev in ("none", "n", "n+5")} == set(dk.PROB_RETRY)
    assert {(c.kind, c.pr) for c in cases if not c.index} == {(k, p) for k in dk.KINDS for p in dk.PROB_RETRY}
    assert all(dk.accept_inputs(c.n, c.kind, c.pr, c.index)["C"] == (c.n + 37 if c.index else c.n) for c in cases)
    ghosts = dk.ghost_cases()
    assert {(c.n, c.n_dev, c.sub) for c in ghosts} == {(n, w, s) for n in dk.LANE_SIZES for w in dk.N_DEV for s in (True, False)}
    assert {c.pr for c in ghosts} == set(dk.PROB_RETRY)


@pytest.mark.parametrize("kind", dk.KINDS)
def test_the_warmed_table_holds_every_stream_position(kind):
    """Chain c has made c % 4 draws: fresh streams, and Philox buffer positions on both sides of a refill, before the one or
    two draws of a stage."""
    from bayes_kit_amd._engine import numpy_generator_from_words

    k, words, u = dk.stream_table(kind, 100)
    _, fresh = dk._fresh(kind, 100, torch.device("cpu"))
    for c in range(8):
        g = numpy_generator_from_words(k, fresh.numpy().view(np.uint64)[:, c])
        g.uniform(size=c % 4)
        assert (g.uniform(), g.uniform()) == tuple(u[c])
    if kind == "philox":
        assert {int(v) for v in words.view(np.uint64)[10]} == {4, 1, 2, 3}  # (buffer_pos; 4 = empty: the next draw refills)


# ---- the inputs reach every branch ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dk.accept_cases(), ids=dk.case_id)
def test_accept_inputs_reach_every_branch(case):
    r = dk.accept_report(case)
    print(r)
    eff = r["eff"]
    assert eff == dk.lanes(case.n, case.n_dev)
    if eff >= 63:
        need = math.ceil(0.05 * eff)
        assert min(r["accepted"], r["retry"], r["not_live"], r["a_zero"]) >= need, r
        # prob_retry = 0: pr * r is 0 for every finite r and log(u) < 0, so a rejected chain always proposes again
        # (drghmc.py:317 and :370) -- the class is empty by the sampler's rule, not for want of inputs
        assert (r["die"] >= need) if case.pr > 0 else (r["die"] == 0), r
        assert min(r["nan"], r["pinf"], r["ninf"]) == 1, r
    elif eff:
        assert r["accepted"] + r["retry"] + r["die"] == eff == 1
    assert r["margin"] >= dk.MARGIN, r


@pytest.mark.parametrize("case", dk.ghost_cases(), ids=dk.case_id)
def test_ghost_inputs_reach_every_branch(case):
    r = dk.ghost_report(case)
    eff = r["eff"]
    if eff >= 63:
        need = math.ceil(0.05 * eff)
        assert min(r["goes_on"], r["a_zero"], r["not_live"]) >= need, r
        assert r["neg_zero"] >= 1 and r["pos_zero"] >= 1 and min(r["nan"], r["pinf"], r["ninf"]) == 1, r


@pytest.mark.parametrize("kind", dk.KINDS)
@pytest.mark.parametrize("C", dk.STAGE_CHAINS)
def test_retry_test_inputs(C, kind):
    rej, alive = dk.retry_inputs(C, kind)
    if C >= 63:
        for share in ((rej == 0).mean(), np.isneginf(rej).mean(), (alive == 0).mean(), (alive == 1).mean()):
            assert share >= 0.05
    assert dk.retry_margin(C, kind) >= dk.MARGIN
    outcomes = set()
    for pr in dk.PROB_RETRY:  # the test passes and fails for live chains, at every prob_retry that lets it
        kind_id, st = dk.streams(FakeOps(), kind, C + dk.PAD)
        a = torch.from_numpy(alive.copy())
        with np.errstate(invalid="ignore"):
            FakeOps().dr_retry_test(kind_id, st[:, :C], torch.from_numpy(rej.copy()), pr, a)
        outcomes |= {(pr, int(v)) for v in a.numpy()[alive == 1]}
    if C >= 63:
        assert outcomes == {(1.0, 0), (1.0, 1), (0.0, 0), (0.0, 1), (0.35, 0), (0.35, 1)}


def test_compaction_flags_use_every_byte():
    for n in dk.COMPACT_SIZES[4:]:
        f = dk.compaction_flags(n, 0.5, 0)
        assert set(np.unique(f)) == {0, 1, 2, 0x80, 0xFF}
    assert not dk.compaction_flags(8193, 0.0, 0).any() and dk.compaction_flags(8193, 1.0, 0).all()


# ---- the checks on the stand-in -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", dk.KINDS)
@pytest.mark.parametrize("C", dk.STAGE_CHAINS)
def test_stage_scalars(ops, C, kind):
    dk.check_stage_scalars(ops, C, kind)


@pytest.mark.parametrize("case", dk.accept_cases(), ids=dk.case_id)
def test_accept_forms(ops, case):
    dk.check_accept_forms(ops, case)


@pytest.mark.parametrize("case", dk.ghost_cases(), ids=dk.case_id)
def test_ghost_forms(ops, case):
    dk.check_ghost_forms(ops, case)


@pytest.mark.parametrize("n", dk.COMPACT_SIZES)
def test_compaction(ops, n):
    dk.check_compaction(ops, n)


@pytest.mark.parametrize("D", dk.SCATTER_DIMS)
@pytest.mark.parametrize("n", dk.SCATTER_LANES)
def test_scatter(ops, n, D):
    dk.check_scatter(ops, n, D)


@pytest.mark.parametrize("target", ("gaussian", "funnel"))
@pytest.mark.parametrize("C,D", dk.STEP_SHAPES)
def test_single_step(ops, C, D, target):
    dk.check_single_step(ops, C, D, target)


# ---- planted faults: the checks notice ------------------------------------------------------------------------------------------
class NoClamp(FakeOps):
    """bk_lanes without its min: a count above the launch size is taken as it is."""

    @staticmethod
    def _lanes(n, n_dev):
        return n if n_dev is None else int(n_dev[0])


class StoresBeforeSecondDraw(FakeOps):
    """k_dr_accept_test storing the stream before the next stage's uniform is drawn: a rejected chain ends one draw on."""

    _second = False

    def dr_accept_prob_test(self, *args, **kw):
        super().dr_accept_prob_test(*args, **kw)
        self._second = self._in_next

    def _put(self, kind, state, c, gen):
        if not self._second:
            super()._put(kind, state, c, gen)

    def dr_accept_prob_test_next(self, *args, **kw):
        self._in_next = True
        try:
            super().dr_accept_prob_test_next(*args, **kw)
        finally:
            self._in_next = self._second = False

    _in_next = False


def _append_wg(takers, values, size, own_wave):
    """bk_append_wg<4>'s positions for lane j = takers, workgroups in order; own_wave: the prefix counts `w <= wave`."""
    out = np.full(size, dk.I_SENT, dtype=np.int32)
    base = 0
    for wg in range(0, len(takers), 256):
        counts = [int(takers[wg + 64 * w: wg + 64 * w + 64].sum()) for w in range(4)]
        for j in np.flatnonzero(takers[wg: wg + 256]):
            wave = j // 64
            pos = base + sum(counts[: wave + 1 if own_wave else wave]) + int(takers[wg + 64 * wave: wg + j].sum())
            if pos < size:  # (the device would write past the list)
                out[pos] = values[wg + j]
        base += sum(counts)
    return out


class PrefixCountsOwnWave(FakeOps):
    """bk_append_wg with `w <= wave` in its prefix: every wavefront's entries land one wavefront's count further on."""

    def dr_accept_prob_test_next(self, kind, state, chain_index, H, h, live, a, prob_retry, n, cur_H, cur_h, rej, alive,
                                 accepted, next_index, next_count, n_dev=None):
        super().dr_accept_prob_test_next(kind, state, chain_index, H, h, live, a, prob_retry, n, cur_H, cur_h, rej, alive,
                                         accepted, next_index, next_count, n_dev)
        chain = np.arange(n) if chain_index is None else chain_index.numpy()
        takers = np.zeros(n, dtype=bool)
        takers[: self._lanes(n, n_dev)] = alive.numpy()[chain[: self._lanes(n, n_dev)]] == 1
        next_index.numpy()[:] = _append_wg(takers, chain, n, own_wave=True)


def test_the_list_emulation_is_a_list_when_not_faulty():
    rng = np.random.default_rng(0)
    takers = rng.uniform(size=700) < 0.3
    values = rng.permutation(700).astype(np.int32)
    got = _append_wg(takers, values, 700, own_wave=False)
    assert np.array_equal(got[: takers.sum()], values[takers]) and (got[takers.sum():] == -1).all()


def _case(n, kind, n_dev):
    return next(c for c in dk.accept_cases() if (c.n, c.kind, c.n_dev, c.index) == (n, kind, n_dev, True))


def test_a_count_that_is_not_clamped_is_noticed():
    with pytest.raises((AssertionError, IndexError)):
        dk.check_accept_forms(NoClamp(), _case(257, "pcg64", "n+5"))
    with pytest.raises((AssertionError, IndexError)):
        dk.check_ghost_forms(NoClamp(), next(c for c in dk.ghost_cases() if (c.n, c.n_dev) == (65, "n+5")))
    dk.check_accept_forms(NoClamp(), _case(257, "pcg64", "n-70"))  # (the same fault is invisible below the launch size)


@pytest.mark.parametrize("kind", dk.KINDS)
def test_a_stream_stored_before_the_second_draw_is_noticed(kind):
    with pytest.raises(AssertionError, match="next: state"):
        dk.check_accept_forms(StoresBeforeSecondDraw(), _case(65, kind, "none"))


@pytest.mark.parametrize("n", [65, 257])
def test_a_prefix_that_counts_its_own_wavefront_is_noticed(n):
    with pytest.raises(AssertionError, match="the chains that propose again"):
        dk.check_accept_forms(PrefixCountsOwnWave(), _case(n, "pcg64", "none"))
