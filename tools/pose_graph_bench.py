"""dliom_pose_graph_solve against the CPU model (tests/cpp/pose_graph_model.cc, one thread -- this repository's model,
NOT Ceres) on graphs of S submaps with M nodes a submap: milliseconds a Solve and an iteration, the stage split of the
summary (a second, profiled run: the stages are then separated by synchronisations), polled read-backs.
--terms adds the further terms of dliom_pose_graph_solve_terms to each graph: two fixed frames, one constraining every
fifth node of the first half and one every fifth of the second, and HuberLoss(1e3) on the loop closures, one more of
which is 5 m wrong.
--landmarks adds 8 landmarks to each graph, seen in turn from every 10th node (dliom_pose_graph_solve_landmarks: two
promoted nodes a sighting, so 360x100 with its 7 200 promoted nodes is past the column cap and reported as refused); the
model is then run only up to 1 024 columns (its dense reduced system takes minutes beyond).
usage: python tools/pose_graph_bench.py [--sizes 3x100,40x100,360x100] [--repeats 3] [--terms | --landmarks]"""
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
    ap.add_argument("--terms", action="store_true")
    ap.add_argument("--landmarks", action="store_true")
    args = ap.parse_args()
    L = dl.load_library()
    ctx = dl.Context(0)
    d = tempfile.mkdtemp()
    if args.terms or args.landmarks:
        import pose_graph_terms_common as tc
    if args.landmarks:
        import pose_graph_landmarks_common as lc
    exe = pc.build_model(d)
    for size in args.sizes.split(","):
        s, m = (int(v) for v in size.split("x"))
        if args.landmarks:
            g, truth, _ = tc.synthetic(s, m * s, max(1, s // 10), seed=s, max_iterations=10)  # the plain bench's graph
            g = lc.with_landmarks(g, truth, lc.some_landmarks(8, s), lc._every(len(g.nodes), 10, 8), seed=s)
            try:
                columns = g.device(dl, ctx).step(1e4)[2]
            except dl.DliomError as e:
                print(json.dumps(dict(submaps=s, nodes=len(g.nodes), landmarks=len(g.landmarks), observations=len(g.observations),
                                      refused=e.status, too_large=e.status == dl.ERR_TOO_LARGE)))
                continue
            model = pc.model_solve(exe, g, d) if columns <= 1024 else None
        elif args.terms:
            g, truth, inter = tc.synthetic(s, m * s, max(1, s // 10), seed=s, max_iterations=10)
            g, inter = tc.false_closure(g, inter, truth, 5.0, submap=1, node=len(g.nodes) // 2, seed=s)
            half = len(g.nodes) // 2
            frames = [dict(origin=tc._yaw_pose([1.0, 2.0, 0.0], -0.4), nodes=list(range(0, half, 5))),
                      dict(origin=tc._yaw_pose([0.0, -3.0, 0.5], 2.0), nodes=list(range(half, len(g.nodes), 5)))]
            g = tc.with_fixed_frames(g, truth, frames, seed=s, huber_scale=tc.LOSS_HUBER_SCALE, inter_submap=inter)
            model = pc.model_solve(exe, g, d)
        else:
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
            submaps=s, nodes=len(g.nodes), constraints=len(g.constraints), terms=args.terms,
            landmarks=len(g.landmarks) if args.landmarks else 0, observations=len(g.observations) if args.landmarks else 0,
            reduced_dimension=summary["reduced_dimension"],
            iterations=summary["num_iterations"], same_steps_as_model=None if model is None else summary["steps"] == model["steps"],
            device_ms_per_solve=min(times), device_ms_first_solve=times[0], device_ms_per_iteration=min(times) / iterations,
            read_backs_per_solve=(n1.value - n0.value) / args.repeats,
            stages_ms={k: staged[k] for k in ("linearise_ms", "eliminate_ms", "factor_ms", "back_substitute_ms", "host_ms")},
            model_one_thread_ms_per_solve=None if model is None else model["seconds"] * 1e3)))
    ctx.close()


if __name__ == "__main__":
    main()
