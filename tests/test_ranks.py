"""The launcher of the multi-rank tests (tests/_ranks.py) itself, on CPU ranks over gloo: the happy path with h x w groups, a
failing rank, the time limit, and the guard on the number of processes.  No GPU is touched."""
import multiprocessing
import os
import tempfile
import time

import pytest
import torch

import _ranks
from _ranks import hw_groups, launch, ranks


def _no_child_alive():
    return not multiprocessing.active_children()


def _worker_groups(rank, world, rendezvous):
    with ranks(rank, world, rendezvous) as dist:
        ih, iw, hg, wg = hw_groups(rank, 2, 2)
        assert (ih, iw) == (rank // 2, rank % 2)
        over_h, over_w = torch.tensor([float(rank)]), torch.tensor([float(rank)])
        dist.all_reduce(over_h, group=hg)
        dist.all_reduce(over_w, group=wg)
        # hg joins the ranks iw and 2 + iw of a column, wg the ranks 2 ih and 2 ih + 1 of a row
        assert over_h.item() == 2 * iw + 2 and over_w.item() == 4 * ih + 1, (rank, over_h, over_w)


def test_four_ranks_meet_over_the_file_and_reduce_over_their_h_and_w_groups():
    launch(_worker_groups, 4, limit=120)
    assert "MASTER_PORT" not in os.environ and _ranks._LIMIT_ENV not in os.environ
    assert _no_child_alive()


def _worker_boom(rank, world, rendezvous):
    if rank == 1:
        raise ValueError("boom")
    with ranks(rank, world, rendezvous) as dist:          # rank 0 waits for a peer that never comes
        dist.barrier()


def test_a_failing_rank_ends_the_launch_with_its_traceback():
    t0 = time.monotonic()
    with pytest.raises(Exception, match="boom"):
        launch(_worker_boom, 2, limit=120)
    assert time.monotonic() - t0 < 60
    assert _no_child_alive()


def _worker_sleep(rank, world, rendezvous):
    time.sleep(600)


def test_the_limit_ends_sleeping_ranks_and_removes_the_rendezvous(monkeypatch):
    made = []

    class Recorded(tempfile.TemporaryDirectory):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self.name)

    monkeypatch.setattr(tempfile, "TemporaryDirectory", Recorded)
    t0 = time.monotonic()
    with pytest.raises(TimeoutError, match=r"_worker_sleep: 2 ranks did not finish within 5 s"):
        launch(_worker_sleep, 2, limit=5)
    assert 5 <= time.monotonic() - t0 < 60
    assert _no_child_alive()
    assert len(made) == 1 and not os.path.exists(made[0])


def test_more_than_fifteen_ranks_are_refused_before_any_process_starts(monkeypatch):
    import torch.multiprocessing as mp
    monkeypatch.setattr(mp, "spawn", lambda *a, **k: pytest.fail("a process was started"))
    with pytest.raises(ValueError, match="16 ranks"):
        launch(_worker_sleep, 16, limit=5)
    assert _no_child_alive()
