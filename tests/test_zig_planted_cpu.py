"""tests/golden/zig_planted.json holds what it claims (no GPU): every planted state, walked sequentially, gives numpy's
normals and numpy's final state; every claimed fact -- word classes at window positions, attempt lengths, which attempt
emits dimension D - 1, what stays unconsumed -- holds; no wedge comparison in a consumed range is close enough for a
last-bit difference of exp() to flip it; no tail near a planted stream is long enough to come near the generator's
abort path; and every event class is there for every window size it applies to."""
import numpy as np
import pytest

from tests import zig_planted as zp

WW = (64, 128, 256)
# event class -> window sizes it must be planted for
REQUIRED = {
    # window end
    "end_wedge_last": WW, "end_tail_last": WW,
    "end_wedge_m2_acc_lastpasses": WW, "end_wedge_m2_rej_lastpasses": WW,
    "end_wedge_m2_acc_lastfails": WW, "end_wedge_m2_rej_lastfails": WW,
    "end_tail3_fits": WW, "end_tail3_runs_out": WW, "end_tail5_fits": WW, "end_tail5_runs_out": WW,
    "longest_tail": WW,
    # ordering
    "adj_in_lane": WW, "adj_cross_lane": WW, "three_in_row": WW, "fail_then_tail_word": WW, "fail_then_tail_attempt": WW,
    "fail_in_tail_pairs": WW, "lane_k0_k2": WW, "rej_wedge_then_exception": WW,
    # carry-in
    "carry_bp1": WW, "carry_bp2": WW, "carry_bp3": WW, "carry_bp4": WW, "carry_consumed_fail": WW,
    # last dimension
    "last_fast_at_window_end": WW, "last_wedge_accepted": WW, "last_tail": WW,
    "last_after_one_rejected_wedge": WW, "last_after_two_rejected_wedges": WW,
    "last_then_rejected_wedge": WW, "last_then_tail_start": WW,
    "late_tail_out_of_window": WW, "late_failing_last_word": WW, "late_neighbouring_exceptions": WW,
    "last_wedge_accepted_small_D": (64,), "last_tail_small_D": (64,),  # D in 1..31: bk_normals_chain_major only
    # counter carries
    "ctr_carry_between_lanes": WW, "ctr_two_limbs_max": WW, "ctr_written_back_crosses": WW,
    # next_normal_pair(Philox&) of the one-lane kernels (no window there; planted once)
    "pair_first_fails": (64,), "pair_second_fails": (64,), "pair_both_fail": (64,), "pair_unget_crosses_refill": (64,),
    "pair_tail_first": (64,), "odd_D_ends_on_exception": (64,),
}
PCG_REQUIRED = ("pcg_tail", "pcg_rejected_then_accepted_wedge")

PHILOX = zp.entries("philox")
PCG = zp.entries("pcg64")


def _id(e):
    return f"{e['name']}-{e['ww']}"


@pytest.mark.parametrize("e", PHILOX, ids=[_id(e) + f"-{i}" for i, e in enumerate(PHILOX)])
def test_planted_entry_is_what_it_claims(e):
    attempts, normals, final, end = zp.check_facts(e)
    zp.check_safety(e)
    assert len(normals) == e["D"] and e["ww"] == 4 * e["lpc"] and 1 <= e["buffer_pos"] <= 4
    # the walker against numpy itself, started from the same state: normals and the final bit generator state
    g = zp.numpy_generator(e)
    want = g.normal(size=e["D"])
    assert np.array_equal(want.view(np.uint64), normals.view(np.uint64))
    st = g.bit_generator.state
    assert [int(v) for v in st["state"]["counter"]] == final["counter"]
    assert [int(v) for v in st["buffer"]] == final["buffer"] and st["buffer_pos"] == final["buffer_pos"]
    # the final position the walker counted is the one the state encodes
    blocks = (end - 1) // 4
    assert zp.ctr_add(e["counter"], blocks) == final["counter"] and end - 4 * blocks == final["buffer_pos"]
    # the emitted values are the attempts' values, in order
    assert [a[5] for a in attempts if a[3]] == list(normals)


def test_the_longest_planted_tail_has_at_least_seven_words():
    scan = zp.load_fixture()["scan"]
    for e in PHILOX:
        if e["name"] == "longest_tail":
            L = [f[2] for f in e["facts"] if f[0] == "taillen"][0]
            assert L >= 7 and L == scan["longest_tail"] and L + [f[1] for f in e["facts"] if f[0] == "taillen"][0] <= e["ww"]


def test_every_event_class_is_planted_for_every_window_size():
    have = {}
    for e in PHILOX:
        have.setdefault(e["name"], set()).add(e["ww"])
    missing = [(n, w) for n, wws in REQUIRED.items() for w in wws if w not in have.get(n, set())]
    assert not missing, missing
    assert sorted(e["name"] for e in PCG) == sorted(PCG_REQUIRED)
    assert zp.load_fixture()["not_found"] == []
    # the window-end classes are planted where the launch goes on into a second window; the ordering classes inside one pass
    for e in PHILOX:
        if e["name"].startswith("end_"):
            assert (e["C"], e["D"]) == zp.MULTI[e["lpc"]] and ["passes", 2] in e["facts"], _id(e)
        elif e["name"].startswith("late_"):
            assert ["passes", 1] in e["facts"], _id(e)
    assert {e["buffer_pos"] for e in PHILOX} == {1, 2, 3, 4}


def test_planted_chains_sit_in_first_inner_and_last_segments_between_unplanted_neighbours():
    for lpc in (16, 32, 64):
        per_wave = 64 // lpc
        segs, waves_mixed = set(), 0
        for (l, C, D), es in zp.groups_by_shape().items():
            if l != lpc:
                continue
            words, where = zp.build_table(es, C)
            assert len(where) == len(es) and C % (4 * per_wave) != 0 or (C, D) == zp.MULTI[lpc]
            for col, e in where.items():
                assert [int(v) for v in words[:, col]] == [int(v) for v in zp.state_words(e)]
                segs.add(col % per_wave)
                neighbours = [c for c in range(col - col % per_wave, min(col - col % per_wave + per_wave, C)) if c != col]
                waves_mixed += any(c not in where for c in neighbours)
            unplanted = [c for c in range(C) if c not in where]
            assert unplanted and all(int(words[10, c]) == 4 and int(words[2, c]) == 0 for c in unplanted)
        assert segs == set(range(per_wave)), (lpc, segs)
        assert lpc == 64 or waves_mixed > 10, (lpc, waves_mixed)


def test_the_carry_in_state_with_a_consumed_failing_word_is_reached_by_a_uniform_draw():
    """Generator.uniform() consumes one word whatever it is: from the state one word earlier it lands on the planted one."""
    n = 0
    for e in PHILOX:
        if e["name"] == "carry_consumed_fail":
            before = dict(e, buffer_pos=e["buffer_pos"] - 1)
            assert before["buffer_pos"] >= 1
            g = zp.numpy_generator(before)
            g.uniform()
            st = g.bit_generator.state
            assert st["buffer_pos"] == e["buffer_pos"] and [int(v) for v in st["state"]["counter"]] == e["counter"]
            assert [int(v) for v in st["buffer"]] == zp.block_of(e, 0)
            n += 1
    assert n == 3


def test_the_launch_shapes_select_the_window_sizes_the_fixture_was_built_for():
    """bk_normals_lanes_per_chain launches nothing: the choice rule itself, asked here without a GPU."""
    from bayes_kit_amd import _lib

    lib = _lib.load()
    q = lib.bk_normals_lanes_per_chain
    for e in PHILOX:
        assert q(e["C"], e["D"]) == e["lpc"], _id(e)
    for lpc, (lo, hi) in zp.D_RANGE.items():
        assert q(zp.SMALL_C, lo) == lpc and q(zp.SMALL_C, hi) == lpc, lpc
    assert q(zp.SMALL_C, 1) == 16 and q(zp.SMALL_C, 31) == 16
    assert q(zp.SMALL_C, 57) == 16 and q(zp.SMALL_C, 58) == 32 and q(zp.SMALL_C, 120) == 32 and q(zp.SMALL_C, 121) == 64
    for lpc, (C, D) in zp.MULTI.items():
        assert q(C, D) == lpc
        assert 1.0085 * D + 6.0 > 4 * lpc  # (more than one pass)
    assert q(0, 5) == 0 and q(5, 0) == 0 and q(-1, -1) == 0


@pytest.mark.parametrize("e", PCG, ids=[e["name"] for e in PCG])
def test_planted_pcg64_entry_is_what_it_claims(e):
    bg = np.random.PCG64(e["seed"])
    bg.advance(e["advance"])
    words = [int(v) for v in bg.random_raw(4 * e["D"])]
    att, end = zp.walk_words(words, e["D"])
    starts = {a[0]: a for a in att}
    for f in e["facts"]:
        assert f[0] == "attempt" and list(starts[f[1]][1:4]) == f[2:5], f
    for a in att:
        if a[2] == "W":
            assert zp.wedge_test(words[a[0]], words[a[0] + 1])[1] > zp.MARGIN
    # numpy consumes exactly the words the walk says
    g = zp.numpy_generator(e)
    g.normal(size=e["D"])
    ref = np.random.PCG64(e["seed"])
    ref.advance(e["advance"] + end)
    assert g.bit_generator.state["state"] == ref.state["state"]


# ---- the kernel's window bookkeeping, restated (tests/zig_planted.py: window_model) ---------------------------------------
# event class -> branches its entries must take in the FIRST window (the one the event was planted in)
BRANCHES = {
    "end_wedge_last": {"defer"}, "end_tail_last": {"defer"},
    "end_wedge_m2_acc_lastfails": {"defer", "cover_gt_stop"}, "end_wedge_m2_rej_lastfails": {"defer", "cover_gt_stop"},
    "end_tail3_fits": {"tail", "ordered"}, "end_tail5_fits": {"tail", "ordered"},
    "end_tail3_runs_out": {"tail", "short"}, "end_tail5_runs_out": {"tail", "short"},
    "longest_tail": {"tail", "ordered"},
    "adj_in_lane": {"neighbours", "ordered", "two_in_lane"}, "adj_cross_lane": {"neighbours", "ordered"},
    "three_in_row": {"neighbours", "ordered"}, "fail_then_tail_word": {"neighbours", "tail", "ordered"},
    "fail_then_tail_attempt": {"tail", "ordered"}, "fail_in_tail_pairs": {"tail", "ordered"},
    "lane_k0_k2": {"two_in_lane"}, "late_tail_out_of_window": {"tail", "short"}, "late_failing_last_word": {"defer"},
    "late_neighbouring_exceptions": {"neighbours", "ordered"},
}


@pytest.mark.parametrize("e", PHILOX, ids=[_id(e) + f"-{i}" for i, e in enumerate(PHILOX)])
def test_window_model_equals_the_walker_and_takes_the_planted_branch(e):
    assert zp.model_agrees(e)
    _, _, _, passes = zp.window_model(e)
    assert BRANCHES.get(e["name"], set()) <= passes[0], (passes[0], e["name"])
    assert (len(passes) > 1) == any(f == ["passes", 2] for f in e["facts"]) or not any(f[0] == "passes" for f in e["facts"])


def test_every_branch_of_the_bookkeeping_is_reached_for_every_window_size():
    seen = {ww: set() for ww in WW}
    multi = {ww: False for ww in WW}
    for e in PHILOX:
        passes = zp.window_model(e)[3]
        seen[e["ww"]] |= set().union(*passes)
        multi[e["ww"]] |= len(passes) > 1
    for ww in WW:
        assert seen[ww] >= {"defer", "short", "shortcut", "ordered", "tail", "two_in_lane", "covered_exception", "neighbours",
                            "cover_gt_stop"}, (ww, seen[ww])
        assert multi[ww]


@pytest.mark.parametrize("fault", zp.FAULTS)
def test_a_fault_planted_in_the_bookkeeping_is_noticed(fault):
    """Every fault changes the result of at least one entry of every window size (so the fixture would see the same mistake
    in the kernel); the un-faulted model agrees everywhere (above)."""
    caught = {ww: [e["name"] for e in PHILOX if e["ww"] == ww and not zp.model_agrees(e, fault)] for ww in WW}
    assert all(caught.values()), (fault, {ww: len(v) for ww, v in caught.items()})
