"""The rank launcher of the suite (tests/ranks.py) on the CPU: results in rank order, a failed rank ends the world within the grace, a hung world ends at
its one deadline, nobody is left alive, every rank is reported, and the two rules of GPU worlds (at most 16 processes, nothing after an incident).
The ranks are those of tests/ranks_probe_worker.py: gloo and the clock only."""
import multiprocessing
import time

import pytest

import ranks
import ranks_probe_worker as probe

STARTUP = 5.0      # seconds; twice the 2.5 s measured by test_results_come_back_in_rank_order (printed there): run_ranks() called -> first line of the slowest rank's function


def _failing(*args, **kw):
    t0 = time.monotonic()
    with pytest.raises(AssertionError) as ex:
        ranks.run_ranks(*args, gpu=False, **kw)
    return str(ex.value), time.monotonic() - t0


def test_results_come_back_in_rank_order():
    t0 = time.time()
    res = ranks.run_ranks(probe.returns, 3, timeout=120, gpu=False)          # (a return at all means: every rank stored a result and left with status 0)
    assert [r["rank"] for r in res] == [0, 1, 2]
    print("start-up of a spawned rank: %.1f s" % (max(r["first_line"] for r in res) - t0))
    assert not multiprocessing.active_children()


def test_a_rank_that_raises_ends_the_world_within_the_grace():
    text, dt = _failing(probe.one_raises, 3, 1, 2, timeout=300, grace=2.0)
    assert "RuntimeError: rank 1 raises on purpose" in text and "Traceback" in text
    assert "in the grace after a peer failed" in text.split("rank 2:")[1].split("\n")[0]
    assert all("rank %d: exit status" % r in text for r in range(3))
    assert dt <= 2.0 + ranks.TERMINATE_WAIT + STARTUP, dt
    assert not multiprocessing.active_children()


def test_a_rank_that_leaves_without_a_result_is_named_with_its_status():
    text, dt = _failing(probe.one_exits, 2, 1, 3, timeout=300, grace=2.0)
    assert "rank 1: exit status 3" in text and "stored no result" in text.split("rank 1: exit status 3")[1].split("\n")[0]
    assert not multiprocessing.active_children()


@pytest.fixture(scope="module")
def hung_world():
    """one world whose rank 0 sleeps far past a deadline of 4 s, without the GPU, with the incident variable cleared around it"""
    before = ranks._gpu_incident
    ranks._gpu_incident = None
    try:
        text, dt = _failing(probe.one_sleeps, 2, 0, 600.0, timeout=4.0)
        return dict(text=text, dt=dt, children=multiprocessing.active_children(), incident=ranks._gpu_incident)
    finally:
        ranks._gpu_incident = before


def test_a_hung_rank_is_ended_at_the_one_deadline(hung_world):
    assert "rank 0: exit status -" in hung_world["text"] and "at the deadline (hung)" in hung_world["text"].split("rank 0:")[1].split("\n")[0]
    assert hung_world["dt"] <= 4.0 + ranks.TERMINATE_WAIT + STARTUP, hung_world["dt"]
    assert not hung_world["children"]


def _no_process(monkeypatch):
    def boom():
        raise RuntimeError("the launcher went on to start processes")
    monkeypatch.setattr(ranks, "free_port", boom)                    # (what run_ranks calls before it creates the first process)


def test_sixteen_ranks_on_the_gpu_are_refused_before_anything_starts(monkeypatch):
    _no_process(monkeypatch)
    monkeypatch.setattr(ranks, "_gpu_incident", None)
    with pytest.raises(AssertionError, match="more than 16 processes"):
        ranks.run_ranks(None, 16, timeout=1, gpu=True)


def test_after_an_incident_no_gpu_world_starts(monkeypatch):
    """the latch, set by hand and set by the launcher itself: a world counted as a GPU world (its ranks are host processes) in which rank 1 dies by a
    signal nobody here sent, while rank 0 hears of it in the barrier and leaves on its own"""
    monkeypatch.setattr(ranks, "_gpu_incident", None)
    with pytest.raises(AssertionError) as ex:
        ranks.run_ranks(probe.one_is_signalled, 2, 1, timeout=300, gpu=True, grace=2.0)
    assert "rank 1: exit status -15, stored no result" in str(ex.value) and ranks._gpu_incident == str(ex.value)
    _no_process(monkeypatch)
    with pytest.raises(AssertionError, match="rank 1: exit status -15, stored no result"):
        ranks.run_ranks(None, 2, timeout=1, gpu=True)
    monkeypatch.setattr(ranks, "_gpu_incident", "rank 1: exit status -11")
    with pytest.raises(AssertionError, match="rank 1: exit status -11"):
        ranks.run_ranks(None, 2, timeout=1, gpu=True)


def test_a_hung_world_without_the_gpu_is_no_incident(hung_world):
    assert hung_world["incident"] is None
