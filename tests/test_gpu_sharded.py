"""BASELINE config 4 through the C entry points: dliom_rtcsm3d_match_sharded with a collective between two and
between EIGHT ranks (all on GPU 0 -- the collective is the caller's, so a one-GPU box can run the N-rank protocol,
including the rank that fails before the exchange), and
dliom_rtcsm3d_match_sharded_rccl on a one-rank RCCL communicator (ncclAllReduce really runs).

At most MAX_RANK_PROCESSES processes open the GPU besides the pytest process (a shared GPU admits only a few processes
at a time): eight ranks run as two threads in each of four processes (calls on different contexts are concurrency-safe,
include/dliom.h).  A rank's MAX all-reduce meets its process's other ranks at a barrier and goes between the processes
as one gloo all-reduce."""
import ctypes as C
import os
import socket
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _scene(dl, ctx):
    from oracle import oracle as orc
    from dliom import synth
    from helpers import DEFAULT_RTCSM, build_oracle_submap, to_device_grid
    og = build_oracle_submap(orc, 0.1, num_scans=6, beams=16, azimuths=256)
    truth = synth.trajectory_pose(0.6)
    pts, _ = synth.scan(truth, 32, 512)
    init = synth.perturb_pose(truth, 0.1, 0.5, seed=13)
    return orc, og, to_device_grid(dl, ctx, og), pts, init, DEFAULT_RTCSM


MAX_RANK_PROCESSES = 4


class _ProcessRanks:
    """The ranks of one process, one thread each: the MAX all-reduce meets at a barrier here, and the barrier's action
    runs the gloo all-reduce between the processes (one gloo rank per process)."""

    def __init__(self, num_local):
        import threading
        self.values = [0] * num_local
        self.barrier = threading.Barrier(num_local, action=self._reduce)
        self.result = None

    def _reduce(self):
        import torch
        import torch.distributed as dist
        t = torch.tensor([max(self.values)], dtype=torch.int64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        self.result = int(t.item())

    def exchange(self, local, value):
        self.values[local] = value
        self.barrier.wait(timeout=300)
        return self.result


class _RankDist:
    """What dliom.sharded uses of torch.distributed, for one rank of a _ProcessRanks."""

    def __init__(self, ranks, local, world):
        import torch.distributed as dist
        self.ReduceOp = dist.ReduceOp
        self.ranks, self.local, self.world = ranks, local, world

    def is_initialized(self):
        return True

    def get_world_size(self):
        return self.world

    def all_reduce(self, t, op):
        assert op == self.ReduceOp.MAX and t.numel() == 1
        t.fill_(self.ranks.exchange(self.local, int(t.item())))


def _rank_groups(world):
    per = -(-world // MAX_RANK_PROCESSES)
    return [list(range(r, min(r + per, world))) for r in range(0, world, per)]


def _process(body, index, groups, world, port, ret):
    """One process: gloo rank `index` among len(groups) processes, the world ranks groups[index] on threads."""
    import threading
    for p in (ROOT, os.path.join(ROOT, "d-liom_amd"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=index, world_size=len(groups))
    import dliom as dl
    from oracle import oracle as orc
    dl.load_library()
    orc.lib()
    ranks = _ProcessRanks(len(groups[index]))

    def run(local, rank):
        try:
            ret[rank] = body(rank, world, _RankDist(ranks, local, world))
        except Exception as e:
            ret[rank] = "%s: %s" % (type(e).__name__, e)
            ranks.barrier.abort()

    threads = [threading.Thread(target=run, args=(i, r)) for i, r in enumerate(groups[index])]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    dist.barrier()
    dist.destroy_process_group()


def _run_world(body, world, timeout):
    import torch.multiprocessing as mp
    mpc = mp.get_context("spawn")
    ret = mpc.Manager().dict()
    port = _free_port()
    groups = _rank_groups(world)
    assert len(groups) <= MAX_RANK_PROCESSES
    procs = [mpc.Process(target=_process, args=(body, i, groups, world, port, ret)) for i in range(len(groups))]
    deadline = time.monotonic() + timeout
    try:
        for p in procs:
            p.start()
        for p in procs:
            p.join(max(0.0, deadline - time.monotonic()))
            assert p.exitcode == 0, "a rank process hung or crashed: %s" % dict(ret)
    finally:
        for p in procs:  # the others wait in the collective for a rank that is gone
            if p.is_alive():
                p.kill()
                p.join()
    return dict(ret)


def _worker(rank, world, dist):
    import dliom as dl
    from dliom import sharded
    ctx = dl.Context(0)
    orc, og, dg, pts, init, opts = _scene(dl, ctx)
    cloud = dl.PointCloud(ctx, pts)
    shard = dl.RtcsmShard(ctx, opts, rank, world)
    score, pose = sharded.sharded_match(shard, init, cloud, dg, dist=dist)  # -> dliom_rtcsm3d_match_sharded
    ref = orc.rtcsm3d_match(opts, init, pts, og)
    ok = bool(np.float32(score) == np.float32(ref["score"]) and np.array_equal(pose, ref["pose"]))
    cloud.close()
    dg.close()
    ctx.close()
    return ok


@pytest.mark.parametrize("world", [2, 8])
def test_ranks_one_collective_through_the_c_entry_point(world):
    """world = 8 is the control flow of the driver's 8-GPU run (eight shards of the rotations, one exchange) with every
    rank on GPU 0: the collective is the caller's, so a one-GPU box can run it."""
    ret = _run_world(_worker, world, 600)
    assert all(ret.get(r) is True for r in range(world)), ret


def _failing_worker(rank, world, dist):
    """The last rank hands in an empty cloud (DLIOM_ERR_EMPTY_CLOUD before any kernel): it must still join the collective,
    and every other rank must come back with DLIOM_ERR_PEER_FAILED instead of hanging in the all-reduce."""
    import dliom as dl
    from dliom import sharded
    ctx = dl.Context(0)
    orc, og, dg, pts, init, opts = _scene(dl, ctx)
    cloud = dl.PointCloud(ctx, pts if rank != world - 1 else pts[:0])  # the LAST rank fails
    shard = dl.RtcsmShard(ctx, opts, rank, world)
    try:
        sharded.sharded_match(shard, init, cloud, dg, dist=dist)
        status = "no error"
    except dl.DliomError as e:
        status = e.status
    cloud.close()
    dg.close()
    ctx.close()
    return status


@pytest.mark.parametrize("world", [2, 8])
def test_a_failing_rank_still_joins_the_collective(world):
    import dliom as dl
    ret = _run_world(_failing_worker, world, 300)
    assert all(ret.get(r) == dl.ERR_PEER_FAILED for r in range(world - 1)) and ret.get(world - 1) == dl.ERR_EMPTY_CLOUD, ret


def _rccl_one_rank_main():
    """Body of the RCCL test; runs in a process of its own (see the test)."""
    for p in (ROOT, os.path.join(ROOT, "d-liom_amd"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import dliom as dl
    dl.load_library()
    rccl = C.CDLL("librccl.so.1")

    class UniqueId(C.Structure):
        _fields_ = [("internal", C.c_char * 128)]

    uid = UniqueId()
    rc = rccl.ncclGetUniqueId(C.byref(uid))
    assert rc == 0, "ncclGetUniqueId -> %d" % rc
    comm = C.c_void_p()
    rccl.ncclCommInitRank.argtypes = [C.POINTER(C.c_void_p), C.c_int, UniqueId, C.c_int]
    ctx = dl.Context(0)
    rc = rccl.ncclCommInitRank(C.byref(comm), 1, uid, 0)
    assert rc == 0, "ncclCommInitRank -> %d" % rc
    orc, og, dg, pts, init, opts = _scene(dl, ctx)
    cloud = dl.PointCloud(ctx, pts)
    score, pose = dl.RtcsmShard(ctx, opts, 0, 1).match_rccl(init, cloud, dg, comm.value)
    ref = orc.rtcsm3d_match(opts, init, pts, og)
    assert np.float32(score) == np.float32(ref["score"]) and np.array_equal(pose, ref["pose"])
    rccl.ncclCommDestroy.argtypes = [C.c_void_p]
    rccl.ncclCommDestroy(comm)
    cloud.close()
    dg.close()
    ctx.close()
    print("rccl-one-rank ok")


def test_rccl_entry_point_on_a_one_rank_communicator():
    """In a fresh process: RCCL's bootstrap (sockets, its own HIP streams and IPC probing) must not depend on
    what the 100+ earlier tests left behind in the pytest process.  RCCL's own log is part of the failure text."""
    import subprocess
    env = dict(os.environ, NCCL_DEBUG="WARN", HSA_ENABLE_IPC_MODE_LEGACY="0", NCCL_SOCKET_IFNAME="lo",
               MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "rccl-one-rank"], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "rccl-one-rank ok" in r.stdout, r.stdout[-3000:] + "\n" + r.stderr[-3000:]


if __name__ == "__main__" and sys.argv[1:] == ["rccl-one-rank"]:
    _rccl_one_rank_main()
