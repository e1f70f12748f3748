"""Run a function in `world` fresh processes that form one torch.distributed group (the tests of
sidecar_amd.dist.DistShard over gloo, and over a one-rank RCCL group)."""
import multiprocessing as mp
import os
import queue
import socket
import time


def free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _entry(target, rank, world, port, args, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        q.put((rank, target(rank, world, *args), None))
    except BaseException as ex:  # reported to the parent instead of a silent hang on q.get
        q.put((rank, None, repr(ex)))
        raise


def run_ranks(target, world, args=(), timeout=240):
    """target(rank, world, *args) in `world` spawned processes, with MASTER_ADDR / MASTER_PORT set for
    init_process_group; returns what each returned (picklable), by rank. A rank that raises, dies or
    does not report within `timeout` seconds fails the caller at once; every rank must exit with 0."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    ps = [ctx.Process(target=_entry, args=(target, r, world, port, args, q)) for r in range(world)]
    for p in ps:
        p.start()
    got = {}
    deadline = time.monotonic() + timeout
    try:
        while len(got) < world:
            try:
                rank, res, err = q.get(timeout=1)
            except queue.Empty:
                dead = [p.exitcode for p in ps if p.exitcode]
                assert not dead, f"a rank exited with {dead} before it reported"
                assert time.monotonic() < deadline, f"ranks {sorted(set(range(world)) - set(got))} did not report"
                continue
            assert err is None, f"rank {rank}: {err}"
            got[rank] = res
    finally:
        for p in ps:  # the others of a failed rank wait in a collective: no patience with them
            p.join(timeout=60 if len(got) == world else 0)
            if p.is_alive():
                p.kill()
                p.join()
    assert [p.exitcode for p in ps] == [0] * world
    return [got[r] for r in range(world)]
