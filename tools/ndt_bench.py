"""dliom_ndt_align on pairs of synthetic scans against the CPU model (tests/ndt_common.py) on one thread -- this
repository's statement of NDT, NOT PCL.  Both scene families, 64 x 1024 and 128 x 2048 scans taken at trajectory_pose(0.30)
(target) and (0.35) (source), raw (the ground-truth tool) and filtered by the ApproximateVoxelGrid model at 0.2 m (the front
end's MatchByNDT), the tool's settings.  A line of JSON a case: results checked equal to the model, ms a target build, ms an
alignment and an evaluation, and the build / evaluate / reduce / host split from a second, profiled call.
usage: python tools/ndt_bench.py [--scenes cube ground] [--sizes 64x1024 128x2048] [--repeats 3] [--no-model] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "d-liom_amd"))
import ndt_common as nd  # noqa: E402
import dliom as dl  # noqa: E402
from dliom import synth  # noqa: E402

HEADER = """# python tools/ndt_bench.py
# one MI355X, one run; an alignment is the best of the repeated calls after a first call that reserves the scratch; the stages come
# from a further, profiled call (host_ms: the call's time less the two kernels' -- pseudo-inverse, step length, launches and polling);
# the CPU column is tests/ndt_common.py (numpy, one thread): this repository's statement of NDT, not PCL
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=["cube", "ground"])
    ap.add_argument("--sizes", nargs="+", default=["64x1024", "128x2048"])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ndt_bench.txt"))
    args = ap.parse_args()
    ctx = dl.Context(0)
    lines = []
    for scene in args.scenes:
        for size in args.sizes:
            beams, azimuths = (int(v) for v in size.split("x"))
            with synth.scene(scene, trajectory=False):
                raw_target = synth.scan(synth.trajectory_pose(0.30), beams, azimuths)[0]
                raw_source = synth.scan(synth.trajectory_pose(0.35), beams, azimuths)[0]
            for clouds in ("raw", "filtered_0.2m"):
                if clouds == "raw":
                    target, source, filter_ms = raw_target, raw_source, 0.0
                else:
                    t = time.perf_counter()
                    target, source = nd.approximate_voxel_grid(raw_target, 0.2), nd.approximate_voxel_grid(raw_source, 0.2)
                    filter_ms = (time.perf_counter() - t) * 1e3
                options = dl.ndt_options()
                dl.NdtTarget(ctx, target, options).close()  # the first build loads the kernels' code
                builds = []
                for _ in range(args.repeats):
                    t = time.perf_counter()
                    ndt_target = dl.NdtTarget(ctx, target, options)
                    builds.append((time.perf_counter() - t) * 1e3)
                    if len(builds) < args.repeats:
                        ndt_target.close()
                cloud = dl.PointCloud(ctx, source)
                ndt = dl.Ndt(ndt_target, options)
                got, aligned = ndt.align(cloud, want_aligned=True)  # the first call reserves the scratch
                times = []
                for _ in range(args.repeats):
                    t = time.perf_counter()
                    got = ndt.align(cloud)
                    times.append((time.perf_counter() - t) * 1e3)
                ctx.set_profiling(1)
                staged = ndt.align(cloud)
                ctx.set_profiling(0)
                evaluations = got["evaluations_with_hessian"] + got["evaluations_without_hessian"]
                line = dict(scene=scene, scan=size, clouds=clouds, source_points=len(source), target_points=len(target),
                            target=ndt_target.memory_stats(), target_build_ms=min(builds), target_build_ms_calls=builds,
                            iterations=got["iterations"], reason=got["reason"], evaluations=evaluations, pairs=got["pairs"],
                            score=got["score"], transformation_probability=got["transformation_probability"],
                            device_ms_per_alignment=min(times), device_ms_calls=times,
                            device_ms_per_evaluation=min(times) / max(evaluations, 1),
                            stages_ms={k: staged[k] for k in ("evaluate_ms", "reduce_ms", "host_ms")}, read_backs=got["read_backs"],
                            python_filter_model_ms=filter_ms)
                if not args.no_model:
                    o = nd.options()
                    t = time.perf_counter()
                    cells = nd.build_cells(target, o)
                    model_build_ms = (time.perf_counter() - t) * 1e3
                    t = time.perf_counter()
                    want = nd.align(cells, source, None, None, o)
                    model_ms = (time.perf_counter() - t) * 1e3
                    equal = all(got[k] == want[k] for k in ("converged", "reason", "iterations", "pairs", "evaluations_with_hessian")) and \
                        got["p"].tobytes() == want["p"].tobytes() and got["transform"].tobytes() == want["transform"].tobytes() and \
                        np.float64(got["score"]).tobytes() == np.float64(want["score"]).tobytes() and \
                        aligned.tobytes() == want["aligned"].tobytes()
                    line.update(results_equal_model=bool(equal), model_one_thread_ms_per_alignment=model_ms,
                                model_one_thread_build_ms=model_build_ms)
                print(json.dumps(line), flush=True)
                lines.append(json.dumps(line))
                cloud.close()
                ndt_target.close()
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(HEADER + "".join(line + "\n" for line in lines))


if __name__ == "__main__":
    main()
