"""The fixed schedule of dliom_icp_align_batch (dliom.h "Schedule"), stated in Python for the tests, and the clouds and
comparisons the batch tests share."""
import numpy as np

RESULT_FIELDS = ("converged", "reason", "iterations", "correspondences", "fitness_count", "read_backs", "settled_by_grid",
                 "settled_by_brute_force")
RESULT_DOUBLES = ("mse", "fitness_score")


def chunks(scratch_bytes, max_pairs_in_flight, max_scratch_bytes):
    """scratch_bytes: dliom_icp_batch_scratch_bytes of every pair, in input order -> the chunks as (first, end) runs.  A
    chunk closes when it holds max_pairs_in_flight pairs, or when the next pair's bytes would take its sum above
    max_scratch_bytes; it always holds at least one pair."""
    out, first = [], 0
    while first < len(scratch_bytes):
        end, total = first, 0
        while end < len(scratch_bytes) and end - first < max_pairs_in_flight:
            if end > first and total + scratch_bytes[end] > max_scratch_bytes:
                break
            total += scratch_bytes[end]
            end += 1
        out.append((first, end))
        first = end
    return out


def expected_stats(searches, scratch_bytes, max_pairs_in_flight, max_scratch_bytes):
    """searches: every pair's searches (the single call's read_backs) -> the call's pairs, chunks, steps, read_backs,
    pair_searches and max_in_flight.  Chunks are not refilled: a chunk takes as many steps as its longest pair."""
    runs = chunks(scratch_bytes, max_pairs_in_flight, max_scratch_bytes)
    steps = sum(max(searches[a:b]) for a, b in runs)
    return dict(pairs=len(searches), chunks=len(runs), steps=steps, read_backs=steps, pair_searches=sum(searches),
                max_in_flight=max([b - a for a, b in runs], default=0))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(a, b):
    """Bit for bit, any NaN standing for any other"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a)[~nan], bits(b)[~nan])


def same_result(got, want):
    """Every field of a result that dliom.h promises of a batch, as a list of the names that differ"""
    bad = [k for k in RESULT_FIELDS if got[k] != want[k]]
    bad += [k for k in RESULT_DOUBLES if not same_bits(np.float64([got[k]]), np.float64([want[k]]))]
    if not same_bits(got["transform"], want["transform"]):
        bad.append("transform")
    return bad


def cloud_points(rng, n):
    """A wall, a floor and scattered points, as tests/test_gpu_icp.py makes them"""
    kind = rng.randint(0, 3, n)
    p = rng.uniform(-20.0, 20.0, (n, 3))
    p[kind == 0, 2] = -1.8 + 0.01 * rng.standard_normal((kind == 0).sum())
    p[kind == 1, 0] = 12.0 + 0.01 * rng.standard_normal((kind == 1).sum())
    return p.astype(np.float32)
