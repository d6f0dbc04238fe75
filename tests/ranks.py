"""The one place of the suite that spawns ranks (`run_ranks`, parent side) and the one that opens a process group (`entry`, worker side).

A world gets ONE deadline; a rank that failed ends the world after a short grace; whoever is still alive then is ended the way `timeout -k 10` ends
a command (terminate, 10 s, kill, join); every rank's exit status is read; and after a rank of a GPU world died by a signal or hung, this pytest
process starts no further GPU world."""
import functools, os, socket, sys, time, traceback
from multiprocessing.connection import wait

GRACE = 30.0               # seconds the peers of a failed rank may still take to leave on their own: a cap on idle waiting, not a measurement
TERMINATE_WAIT = 10.0      # seconds between terminate() and kill()
MAX_GPU_PROCESSES = 16     # processes that may hold the GPU open at once, the pytest process included
POLL = 0.5                 # seconds between two looks at the results (an `error` result wakes no sentinel until its rank has left)

_gpu_incident = None       # the report of the first GPU world in which a rank died by a signal or hung; set once, ends every later GPU world


def free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _failed(res):
    return isinstance(res, dict) and "error" in res


def _end(ps):
    """terminate(), TERMINATE_WAIT, kill(), join(): nobody of `ps` is alive afterwards"""
    alive = [p for p in ps if p.is_alive()]
    for p in alive:
        p.terminate()
    t_end = time.monotonic() + TERMINATE_WAIT
    for p in alive:                                    # (a join per rank, not connection.wait on those still alive: with none left that list is empty and wait sleeps the time out)
        p.join(max(t_end - time.monotonic(), 0.0))
    for p in alive:
        if p.is_alive():
            p.kill()
    for p in ps:
        p.join()


def _report(ps, res, ended, head):
    lines = [head]
    for r, p in enumerate(ps):
        how = {None: "", "hung": ", ended by the launcher at the deadline (hung)", "grace": ", ended by the launcher in the grace after a peer failed"}[ended.get(r)]
        what = "no result" if r not in res else "an error" if _failed(res[r]) else "a result"
        lines.append("rank %d: exit status %s%s, stored %s" % (r, p.exitcode, how, what))
        if _failed(res.get(r)):
            lines.append(str(res[r]["error"]).rstrip())
    return "\n".join(lines)


def run_ranks(target, world, *args, timeout, gpu=True, grace=GRACE):
    """Start `world` processes of `target` (a function under `@entry`) with `args`, wait for them until ONE deadline `timeout` seconds away, and return
    their results in rank order.  Anything else -- a rank without a result, with an `error` result, with an exit status other than 0, or one that had to be
    ended -- raises an AssertionError whose text reports every rank."""
    global _gpu_incident
    if gpu:
        assert world + 1 <= MAX_GPU_PROCESSES, "%d ranks and the pytest process: more than %d processes with the GPU open" % (world, MAX_GPU_PROCESSES)
        assert _gpu_incident is None, "no further ranks on the GPU after a rank died by a signal or hung; the first incident:\n" + str(_gpu_incident)
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    ended = {}
    with ctx.Manager() as m:
        out = m.dict()
        port = free_port()
        ps = [ctx.Process(target=target, args=(r, world, port) + tuple(args) + (out,)) for r in range(world)]
        try:
            for p in ps:
                p.start()
            deadline = time.monotonic() + timeout
            why, seen = "hung", set()
            while True:
                alive = [r for r, p in enumerate(ps) if p.exitcode is None]
                if not alive:
                    break
                new = [r for r in out.keys() if r not in seen]          # (each result crosses from the manager once, not at every poll)
                seen.update(new)
                if why == "hung" and (any(p.exitcode not in (None, 0) for p in ps) or any(_failed(out[r]) for r in new)):
                    why = "grace"; deadline = min(deadline, time.monotonic() + grace)
                left = deadline - time.monotonic()
                if left <= 0:
                    ended = {r: why for r in alive}
                    break
                wait([ps[r].sentinel for r in alive], timeout=min(left, POLL))
        finally:
            _end([p for p in ps if p.pid is not None])
        res = dict(out)
    ok = all(p.exitcode == 0 for p in ps) and all(r in res and not _failed(res[r]) for r in range(world))
    if ok:
        return [res[r] for r in range(world)]
    report = _report(ps, res, ended, "%d ranks of %s.%s, deadline %g s:" % (world, target.__module__, target.__qualname__, timeout))
    if gpu and _gpu_incident is None and (any(p.exitcode < 0 for r, p in enumerate(ps) if r not in ended) or "hung" in ended.values()):
        _gpu_incident = report
    raise AssertionError(report)


def entry(fn):
    """`fn(rank, world, *args) -> result` becomes the spawn target `(rank, world, port, *args, out)`: it opens the gloo group, stores what `fn` returns
    as `out[rank]`, leaves through a barrier, and stores `dict(error=<traceback>)` instead on any exception."""
    @functools.wraps(fn)
    def spawned(rank, world, port, *rest):
        *args, out = rest
        try:
            here = os.path.dirname(os.path.abspath(__file__))
            for p in (here, os.path.dirname(here)):
                if p not in sys.path:
                    sys.path.insert(0, p)
            import torch.distributed as dist
            os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
            dist.init_process_group("gloo", rank=rank, world_size=world)
            out[rank] = fn(rank, world, *args)
            dist.barrier(); dist.destroy_process_group()
        except Exception:
            out[rank] = dict(error=traceback.format_exc())
    return spawned


def staged_transport(capacity_doubles=1 << 20, cls=None):
    """the host-staged transport of a rank that shares GPU 0 with its peers; the caller attaches it to its engine"""
    import torch
    from rxmd_amd.comm import TorchTransport
    return (cls or TorchTransport)(mode="staged", device=torch.device("cuda", 0), capacity_doubles=capacity_doubles)
