#!/usr/bin/env python3
"""X-ray projections of a submap (dliom_grid_xray_texture: Submap3D::ToResponseProto's texture;
dliom_grid_project_to_image: ProjectToCvMat) on the device against the host path a caller has without them:
dliom_grid_to_proto (the whole pool copied down) plus the reference's single-threaded walk (tests/cpp/xray_model.cc,
process start included).  Grids: a front end's finished submap (0.10 m and its 0.45 m twin) and BASELINE config 5's
0.05 m high-resolution grid.  Prints per grid the leaves, occupied cells (>= 0.501) and pixels, the device ms per call
(preallocated buffer, one pass; median of --reps) and the host path's ms, and checks that both give the same bytes.
One JSON line per grid and projection."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "d-liom_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def front_end_submap(dl, ctx):
    from dliom import synth
    from test_gpu_parity import FRONT_END_OPTS
    fe = dl.LocalTrajectoryBuilder3D(ctx, FRONT_END_OPTS)
    gravity = np.array([1.0, 0, 0, 0])
    for s in range(40):
        truth = synth.trajectory_pose(0.1 * s)
        pts, _ = synth.scan(truth, 16, 1024)
        r = fe.match(synth.perturb_pose(truth, 0.03, 0.2, seed=300 + s), np.zeros(3, np.float32), pts)
        fe.insert(int(s * 1e6), r["pose_estimate"], gravity)
        if fe.num_finished_submaps() > 0:
            sub = fe.take_finished_submap()
            fe.close()
            return sub
    raise RuntimeError("no submap finished")


def occupied_cells(dl, grid):
    """(cells with ValueToProbability >= 0.501, leaves)"""
    table = dl.value_to_probability_table()[:32768]
    _, values = grid.download_blocks()
    return int((table[values & 0x7FFF] >= np.float32(0.501)).sum()), int(len(values))


def device_ms(dl, grid, pose, mode, reps):
    L = dl.load_library()
    p = np.ascontiguousarray(pose, dtype=np.float64)
    pp = p.ctypes.data_as(C.POINTER(C.c_double))
    w, h, res, ox, oy = C.c_int32(), C.c_int32(), C.c_double(), C.c_double(), C.c_double()
    sl = (C.c_double * 7)()
    if mode == "texture":
        call = lambda buf, n: L.dliom_grid_xray_texture(grid.h, pp, buf, n, C.byref(w), C.byref(h), C.byref(res), sl)
    else:
        call = lambda buf, n: L.dliom_grid_project_to_image(grid.h, pp, buf, n, C.byref(w), C.byref(h), C.byref(ox),
                                                            C.byref(oy), C.byref(res))
    assert call(None, 0) == 0
    n = (2 if mode == "texture" else 1) * w.value * h.value
    buf = (C.c_uint8 * max(n, 1))()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        assert call(buf, n) == 0
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), w.value * h.value


def host_ms(model, grid, pose, mode, tmp):
    from test_xray_host import run_model
    t0 = time.perf_counter()
    proto = grid.to_proto()
    t1 = time.perf_counter()
    out = run_model(model, mode, proto, pose, tmp)
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import dliom as dl
    from dliom import synth
    from benchlib.config5 import config5_scene
    from test_gpu_xray import same_image, same_texture
    import pathlib
    tmp = pathlib.Path(tempfile.mkdtemp(prefix="xray_bench_"))
    model = str(tmp / "xray_model")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-o", model,
                           os.path.join(ROOT, "tests", "cpp", "xray_model.cc")])
    ctx = dl.Context(0)
    sub = front_end_submap(dl, ctx)
    _, c5_grids, sc, _ = config5_scene(dl, synth, ctx)
    pose = list(sub["local_pose"])
    grids = [("front_end_0.10", sub["hi"]), ("front_end_0.45", sub["lo"]), ("config5_0.05", c5_grids[0])]
    ok = True
    for name, g in grids:
        occ, leaves = occupied_cells(dl, g)
        for mode in ("texture", "image"):
            dev, pixels = device_ms(dl, g, pose, mode, args.reps)
            proto_ms, walk_ms, want = host_ms(model, g, pose, mode, tmp)
            got = dl.grid_xray_texture(g, pose) if mode == "texture" else dl.grid_project_to_image(g, pose)
            equal = bool(same_texture(got, want) if mode == "texture" else same_image(got, want))
            ok &= equal
            print(json.dumps(dict(grid=name, projection=mode, leaves=leaves, occupied_cells=occ, pixels=pixels,
                                  device_ms=round(dev, 3), host_to_proto_ms=round(proto_ms, 2),
                                  host_walk_ms=round(walk_ms, 2), host_total_ms=round(proto_ms + walk_ms, 2),
                                  equal=equal)), flush=True)
    for g in c5_grids:
        g.close()
    sc["cloud"].close()
    sub["hi"].close()
    sub["lo"].close()
    ctx.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
