"""The look-ahead generator (prefetch_rng) on the CPU: the per-stream launch order of HMCDiag and MALA across every
operation that has to drop or keep what was generated ahead (tests/lookahead_trace.py, against the recorded log of the
package before the generator got one owner), the same draws as a sampler that generates in line, and the owner alone."""
import json

import numpy as np
import pytest

from tests import lookahead_trace as lt


@pytest.fixture(scope="module")
def golden():
    with open(lt.GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("sampler,op", lt.CASES)
def test_launch_order_per_stream_is_the_recorded_one(sampler, op, golden):
    got, want = lt.run(sampler, op, True)[0], golden[lt.key(sampler, op)]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, got[max(0, i - 6):i + 3], want[max(0, i - 6):i + 3])
    assert len(got) == len(want)
    assert any(e.startswith("s1 ") and "record" not in e and "wait" not in e for e in got)  # (launches on the side stream)


@pytest.mark.parametrize("sampler,op", lt.CASES)
def test_generating_ahead_changes_nothing(sampler, op):
    a, b = lt.run(sampler, op, True)[1], lt.run(sampler, op, False)[1]
    for when, x, y in (("before", a[0], b[0]), ("after", a[2], b[2])):
        for what, u, v in zip(("theta", "logp", "rng_state"), x, y):
            assert np.array_equal(u, v), (when, what)
    assert np.array_equal(a[1], b[1]), "rng_state() right after the operation"


# ---- the owner alone ---------------------------------------------------------------------------------------------------
@pytest.fixture
def alone(monkeypatch):
    """(a LookAhead on the stand-in streams, the recorder, the slots a counting generator was called with)."""
    from bayes_kit_amd._engine import LookAhead

    rec = lt.Recorder()
    rec.install(monkeypatch)
    calls = []
    return LookAhead("cpu"), rec, calls, calls.append


def _waits(rec):
    return [e for e in rec.normalised() if " wait " in e]


def test_a_first_take_generates_in_line(alone):
    la, rec, calls, gen = alone
    assert la.take(gen) == 0 and calls == [0] and not la.ahead
    assert rec.log == []  # (no event, no wait: the generator ran on the current stream)


def test_later_takes_wait_for_the_event_the_last_start_recorded(alone):
    la, rec, calls, gen = alone
    la.take(gen)
    for n in range(1, 5):
        seen = len(rec.log)
        la.start_next(gen)
        main_ready, side_wait, side_done = rec.log[seen:]
        assert (main_ready[0], main_ready[1]) == (rec.main, "record") and side_wait == (la._side, "wait", main_ready[2])
        assert (side_done[0], side_done[1]) == (la._side, "record") and side_done[2] is not main_ready[2]
        assert la.ahead and la.slot == n % 2 and la.consumed == 1 - n % 2 and calls[-1] == n % 2
        seen = len(rec.log)
        assert la.take(gen) == n % 2 and len(calls) == n + 1  # (nothing generated in line)
        assert rec.log[seen:] == [(rec.main, "wait", side_done[2])]


def test_the_table_is_copied_in_front_of_the_generator_on_the_side_stream(alone):
    import torch

    la, rec, calls, _ = alone
    table, copy = torch.arange(4), torch.zeros(4, dtype=torch.int64)

    def gen(slot):
        assert rec.current is la._side and torch.equal(copy, torch.arange(4))
        table.add_(1)

    la.start_next(gen, (copy, table))
    assert torch.equal(copy, torch.arange(4)) and torch.equal(table, torch.arange(4) + 1) and rec.current is rec.main


def test_a_drop_with_a_wait_waits_once_and_one_without_does_not(alone):
    la, rec, calls, gen = alone
    for wait in (True, False):
        la.start_next(gen)
        seen, slot = len(_waits(rec)), la.slot
        la.drop(wait=wait)
        assert len(_waits(rec)) == seen + (1 if wait else 0) and not la.ahead
        n = len(calls)
        assert la.take(gen) == slot and calls[n:] == [slot]  # (generated again in line, into the slot that was ahead)
        assert len(_waits(rec)) == seen + (1 if wait else 0)
    seen = len(_waits(rec))
    la.drop(wait=True)  # (nothing ahead: nothing to wait for)
    assert len(_waits(rec)) == seen


def test_after_a_reset_the_next_take_generates_in_line_on_slot_0(alone):
    la, rec, calls, gen = alone
    la.start_next(gen)
    assert la.slot == 1 and la.ahead
    la.reset()
    seen = len(rec.log)
    assert la.take(gen) == 0 and calls[-1] == 0 and rec.log[seen:] == []


def test_a_join_with_nothing_pending_does_nothing(alone):
    la, rec, calls, gen = alone
    la.join(), la.synchronize()
    assert rec.log == []
    la.start_next(gen)
    la.join()
    assert rec.log[-1][:2] == (rec.main, "wait") and rec.log[-1][2] is rec.log[-2][2]  # (the generator's done event)
    la.drop(wait=False)
    seen = len(rec.log)
    la.join(), la.synchronize()
    assert rec.log[seen:] == []
    la.drain()
    assert rec.log[seen:] == [(la._side, "synchronize")]
