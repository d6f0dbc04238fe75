"""rank functions of tests/test_ranks_host.py: they use gloo and the clock, never the GPU or the library"""
import os, signal, time

import ranks


@ranks.entry
def returns(rank, world):
    return dict(rank=rank, first_line=time.time())


@ranks.entry
def one_raises(rank, world, who, deaf):
    if rank == who:
        raise RuntimeError("rank %d raises on purpose" % rank)
    if rank == deaf:
        time.sleep(600.0)                      # a peer that does not notice: the launcher has to end it when the grace is over
    return dict(rank=rank)                     # the others go on into the barrier of ranks.entry, where gloo tells them that a peer is gone


@ranks.entry
def one_exits(rank, world, who, status):
    if rank == who:
        os._exit(status)
    return dict(rank=rank)


@ranks.entry
def one_is_signalled(rank, world, who):
    if rank == who:
        os.kill(os.getpid(), signal.SIGTERM)   # a rank that dies by a signal the launcher did not send (a host process only: nothing here is near the GPU)
        time.sleep(600.0)
    return dict(rank=rank)


@ranks.entry
def one_sleeps(rank, world, who, seconds):
    if rank == who:
        time.sleep(seconds)
    return dict(rank=rank)
