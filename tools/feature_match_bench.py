"""dliom_feature_index_match against the CPU model (tests/cpp/feature_match_model.cc, one thread -- this repository's
model, NOT OpenCV's FLANN and RANSAC) on S stored sets of K key points each (D floats a descriptor), every `--overlap-every`-th
of which shares 120 planted features with the query: results checked equal field by field, milliseconds a call, the split
over the three kernels (a second, profiled call), polled read-backs.
usage: python tools/feature_match_bench.py [--sets 200] [--keypoints 1000] [--descriptor-size 64] [--repeats 3]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "d-liom_amd"))
import feature_match_common as fc  # noqa: E402
import dliom as dl  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=200)
    ap.add_argument("--keypoints", type=int, default=1000)
    ap.add_argument("--descriptor-size", type=int, default=64)
    ap.add_argument("--overlap-every", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    S, K, D = args.sets, args.keypoints, args.descriptor_size
    rng = np.random.RandomState(S + K)
    query = fc.make_set(rng, K, D)
    sets = [fc.overlapping_set(rng, query, min(120, K), K - min(120, K)) if k % args.overlap_every == 0 else fc.make_set(rng, K, D)
            for k in range(S)] + [query]
    options = fc.Options()
    d = tempfile.mkdtemp()
    exe = fc.build_model(d)
    want, ratio_margin, threshold_margin, model_seconds = fc.model_match(exe, d, sets, S, list(range(S)), options)
    ctx = dl.Context(0)
    index = dl.FeatureIndex(ctx, D)
    for k, s in enumerate(sets):
        index.add(k, s.descriptors, s.keypoints, s.ox, s.oy, s.resolution)
    keys = list(range(S))
    o = options.device(dl)
    got, stats = index.match(S, keys, o)  # the first call reserves the scratch
    first = ctx.read_backs()
    times = []
    for _ in range(args.repeats):
        t = time.perf_counter()
        got, stats = index.match(S, keys, o)
        times.append((time.perf_counter() - t) * 1e3)
    read_backs = (ctx.read_backs() - first) / args.repeats
    ctx.set_profiling(1)
    _, staged = index.match(S, keys, o)
    ctx.set_profiling(0)
    equal = all(got[k].tobytes() == want[k].tobytes() for k in fc.SUBMAP_MATCH.names)
    print(json.dumps(dict(
        sets=S, keypoints=K, descriptor_size=D, multiply_adds=S * K * K * D, results_equal_model=equal,
        matched=stats["matched"], ransac_pairs=stats["ransac_pairs"], device_ms_per_call=min(times), device_ms_calls=times,
        kernels_ms={k: staged[k] for k in ("knn_ms", "good_ms", "ransac_ms")}, read_backs_per_call=read_backs,
        model_one_thread_ms_per_call=model_seconds * 1e3, ratio_margin=ratio_margin, threshold_margin=threshold_margin,
        index_memory=index.memory_stats())))
    index.close()
    ctx.close()
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
