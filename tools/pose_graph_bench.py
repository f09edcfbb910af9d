"""dliom_pose_graph_solve against the CPU model (tests/cpp/pose_graph_model.cc, one thread -- this repository's model,
NOT Ceres) on graphs of S submaps with M nodes a submap: milliseconds a Solve and an iteration, the stage split of the
summary (a second, profiled run: the stages are then separated by synchronisations), polled read-backs.
usage: python tools/pose_graph_bench.py [--sizes 3x100,40x100,360x100] [--repeats 3]"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "d-liom_amd"))
import pose_graph_common as pc  # noqa: E402
import dliom as dl  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="3x100,40x100,360x100")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    L = dl.load_library()
    ctx = dl.Context(0)
    d = tempfile.mkdtemp()
    exe = pc.build_model(d)
    for size in args.sizes.split(","):
        s, m = (int(v) for v in size.split("x"))
        g = pc.synthetic(s, m * s, max(1, s // 10), seed=s, max_iterations=10)  # S * M nodes in all
        model = pc.model_solve(exe, g, d)
        n0 = C.c_int64()
        L.dliom_ctx_read_backs(ctx.h, C.byref(n0))
        times = []
        for _ in range(args.repeats):
            p = g.device(dl, ctx)
            t = time.perf_counter()
            summary = p.solve()
            times.append((time.perf_counter() - t) * 1e3)
        n1 = C.c_int64()
        L.dliom_ctx_read_backs(ctx.h, C.byref(n1))
        L.dliom_ctx_set_profiling(ctx.h, 1)
        staged = g.device(dl, ctx).solve()
        L.dliom_ctx_set_profiling(ctx.h, 0)
        iterations = max(summary["num_iterations"] - 1, 1)
        print(json.dumps(dict(
            submaps=s, nodes=len(g.nodes), constraints=len(g.constraints), reduced_dimension=summary["reduced_dimension"],
            iterations=summary["num_iterations"], same_steps_as_model=summary["steps"] == model["steps"],
            device_ms_per_solve=min(times), device_ms_first_solve=times[0], device_ms_per_iteration=min(times) / iterations,
            read_backs_per_solve=(n1.value - n0.value) / args.repeats,
            stages_ms={k: staged[k] for k in ("linearise_ms", "eliminate_ms", "factor_ms", "back_substitute_ms", "host_ms")},
            model_one_thread_ms_per_solve=model["seconds"] * 1e3)))
    ctx.close()


if __name__ == "__main__":
    main()
