"""dliom_icp_align on pairs of synthetic scans against the CPU model (tests/icp_common.py) whose search is
scipy.spatial.cKDTree on one thread -- this repository's statement of ICP, NOT PCL.  Both scene families, 64 x 1024 and
128 x 2048 scans taken at trajectory_pose(0.30) (target) and (0.35) (source), both presets (30 m: the ground-truth tool;
3 m: MatchByICP).  A line of JSON a case: results checked equal to the model, ms an alignment and an iteration, the four
stages from a second, profiled call, the share of the queries each search path settled, one search under DLIOM_NN_AUTO and
under DLIOM_NN_BRUTE_FORCE.  cKDTree works in double: its eight nearest are re-ranked by the float rule, and the line says
how many queries that re-decided (or sent to the brute-force model because the eight did not settle them).
usage: python tools/icp_bench.py [--scenes cube ground] [--sizes 64x1024 128x2048] [--repeats 3] [--no-model]"""
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
import icp_common as ic  # noqa: E402
import dliom as dl  # noqa: E402
from dliom import synth  # noqa: E402


class KdTreeSearch:
    """ic.nn_search's answer from a kd-tree: exact by the float rule, or handed to ic.nn_search"""

    def __init__(self, targets):
        from scipy.spatial import cKDTree
        self.targets = np.ascontiguousarray(targets, np.float32)
        self.valid = np.flatnonzero(np.isfinite(self.targets).all(axis=1))
        self.tree = cKDTree(self.targets[self.valid].astype(np.float64))
        self.queries = self.redecided = self.brute_forced = 0
        self.seconds = 0.0

    def __call__(self, queries, targets, max_distance=ic.INF):
        t0 = time.perf_counter()
        q = np.ascontiguousarray(queries, np.float32)
        k = min(8, len(self.valid))
        live = np.isfinite(q).all(axis=1)
        dist, near = self.tree.query(np.where(live[:, None], q, 0).astype(np.float64), k=k, workers=1)
        dist, near = dist.reshape(len(q), k), near.reshape(len(q), k)
        cand = self.targets[self.valid[near]]  # (n, k, 3)
        with np.errstate(over="ignore", invalid="ignore"):
            dx, dy, dz = (q[:, None, a] - cand[:, :, a] for a in range(3))
            s = (dx * dx + dy * dy) + dz * dz
        index = self.valid[near]
        order = np.lexsort((index, s), axis=1)[:, 0]  # least d2, then least index
        rows = np.arange(len(q))
        best, j = s[rows, order], index[rows, order]
        # the eight settle a query when the last of them is clearly farther than the winner (else more may tie: brute force)
        unsure = live & (k < len(self.valid)) & ~(dist[:, -1] ** 2 * (1 - 1e-5) > best.astype(np.float64))
        if unsure.any():
            j[unsure], best[unsure] = ic.nn_search(q[unsure], self.targets, ic.INF)
        self.redecided += int((live & (j != self.valid[near[:, 0]])).sum())
        self.brute_forced += int(unsure.sum())
        self.queries += int(live.sum())
        keep = live & (best.astype(np.float64) <= float(max_distance) * float(max_distance))
        self.seconds += time.perf_counter() - t0
        return np.where(keep, j, -1).astype(np.int32), np.where(keep, best, np.inf).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=["cube", "ground"])
    ap.add_argument("--sizes", nargs="+", default=["64x1024", "128x2048"])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-model", action="store_true")
    args = ap.parse_args()
    ctx = dl.Context(0)
    for scene in args.scenes:
        for size in args.sizes:
            beams, azimuths = (int(v) for v in size.split("x"))
            with synth.scene(scene, trajectory=False):
                target = synth.scan(synth.trajectory_pose(0.30), beams, azimuths)[0]
                source = synth.scan(synth.trajectory_pose(0.35), beams, azimuths)[0]
            t = time.perf_counter()
            index = dl.NnIndex(ctx, target)
            build_ms = (time.perf_counter() - t) * 1e3
            cloud = dl.PointCloud(ctx, source)
            searches = {}
            for name, mode in (("auto", dl.NN_AUTO), ("brute_force", dl.NN_BRUTE_FORCE)):
                index.query(cloud, 30.0, search=mode)
                ctx.set_profiling(1)
                searches[name + "_search_ms"] = index.query(cloud, 30.0, search=mode)[2]["search_ms"]
                ctx.set_profiling(0)
            for preset, options in (("ground_truth_30m", dl.ground_truth_icp_options()), ("match_by_icp_3m", dl.match_by_icp_options())):
                icp = dl.Icp(index, options)
                got, aligned = icp.align(cloud, want_aligned=True)  # the first call reserves the scratch
                times = []
                for _ in range(args.repeats):
                    t = time.perf_counter()
                    got = icp.align(cloud)
                    times.append((time.perf_counter() - t) * 1e3)
                ctx.set_profiling(1)
                staged = icp.align(cloud)
                ctx.set_profiling(0)
                line = dict(scene=scene, scan=size, preset=preset, source_points=len(source), target_points=len(target),
                            index_build_ms=build_ms, index=index.memory_stats(), iterations=got["iterations"], reason=got["reason"],
                            correspondences=got["correspondences"], fitness_score=got["fitness_score"],
                            device_ms_per_alignment=min(times), device_ms_calls=times,
                            device_ms_per_iteration=min(times) / max(got["iterations"] + 1, 1),  # (+ the fitness search)
                            stages_ms={k: staged[k] for k in ("search_ms", "reduce_ms", "solve_ms", "transform_ms")},
                            read_backs=got["read_backs"],
                            share_settled_by_grid=got["settled_by_grid"] / max(got["settled_by_grid"] + got["settled_by_brute_force"], 1),
                            share_settled_by_brute_force=got["settled_by_brute_force"] /
                            max(got["settled_by_grid"] + got["settled_by_brute_force"], 1), **searches)
                if not args.no_model:
                    search = KdTreeSearch(target)
                    t = time.perf_counter()
                    want = ic.align(source, target, None, ic.options(max_correspondence_distance=options.max_correspondence_distance),
                                    search=search)
                    model_ms = (time.perf_counter() - t) * 1e3
                    equal = all(got[k] == want[k] for k in ("converged", "reason", "iterations", "correspondences", "fitness_count")) and \
                        got["transform"].tobytes() == want["transform"].tobytes() and \
                        np.float64(got["fitness_score"]).tobytes() == np.float64(want["fitness_score"]).tobytes() and \
                        aligned.tobytes() == want["aligned"].tobytes()
                    line.update(results_equal_model=bool(equal), model_one_thread_ms_per_alignment=model_ms,
                                model_kd_tree_ms=search.seconds * 1e3, kd_tree_queries=search.queries,
                                kd_tree_redecided_by_float_rule=search.redecided, kd_tree_sent_to_brute_force=search.brute_forced)
                print(json.dumps(line), flush=True)
            cloud.close()
            index.close()
    ctx.close()


if __name__ == "__main__":
    main()
