"""The fixed schedule of dliom_ndt_align_batch (dliom.h, the NDT batch's "Schedule"), stated in Python for the tests, the
CPU model's evaluation sequence of a pair, and the zoo of pairs the batch tests share."""
import numpy as np

import icp_common as ic
import ndt_common as nd
from icp_batch_common import bits, chunks, same_bits  # noqa: F401  (the chunk rule is the ICP batch's)

RESULT_FIELDS = ("converged", "reason", "iterations", "evaluations_with_hessian", "evaluations_without_hessian", "fitness_count",
                 "pairs")
RESULT_DOUBLES = ("score", "transformation_probability", "fitness_score")

SOURCE_SIZES = (0, 1, 65, 2047, 2048, 2049, 4097)  # both sides of one workgroup and of the tree's 2048-leaf block; none
MOVED_GUESS = nd.transform_of([0.1, -0.05, 0.02, 0.01, 0.02, -0.03])  # tests/test_gpu_ndt.py's
GENERIC_GUESS = nd.transform_of([0.4, -0.3, 0.2, 0.05, -0.08, 0.11])
ZOO_OPTIONS = dict(maximum_iterations=2)  # it > 2 ends an alignment: at most four iterations


def same_result(got, want, read_backs=True):
    """Every field of a result that dliom.h promises of a batch (p and transform by their bits, any NaN standing for any
    other), as a list of the names that differ.  want: a single call's result, or the CPU model's (then without read_backs)."""
    bad = [k for k in RESULT_FIELDS if got[k] != want[k]]
    bad += [k for k in RESULT_DOUBLES if not same_bits(np.float64([got[k]]), np.float64([want[k]]))]
    bad += [k for k in ("p", "transform") if not same_bits(np.float64(got[k]), np.float64(want[k]))]
    if read_backs and got["read_backs"] != want["read_backs"]:
        bad.append("read_backs")
    return bad


# ---- the model's evaluation sequence --------------------------------------------------------------------------------------------
class _RecordingRun(nd.Run):
    kinds = None

    def evaluate(self, p, what, sums):
        _RecordingRun.kinds.append(what)
        super().evaluate(p, what, sums)


def model_alignment(cells, source, target, guess, o):
    """nd.align -> (its result, the kinds of its evaluations in order)"""
    saved, nd.Run = nd.Run, _RecordingRun
    _RecordingRun.kinds = []
    try:
        result = nd.align(cells, source, target, guess, o)
        return result, list(_RecordingRun.kinds)
    finally:
        nd.Run = saved


# ---- the schedule ---------------------------------------------------------------------------------------------------------------
def expected_stats(sequences, finals, sizes, scratch_bytes, max_pairs_in_flight, max_scratch_bytes):
    """sequences: every pair's evaluation kinds in order; finals: whether the pair takes a final round (it has a fitness
    index or the clouds are wanted); sizes: its source points -> the call's statistics.  Round r of a chunk evaluates kind
    sequences[i][r] of every pair that has one, and is the final round of a pair with len(sequences[i]) == r.  A kind
    launches once a round if a pair with points evaluates it.  Chunks are not refilled."""
    runs = chunks(scratch_bytes, max_pairs_in_flight, max_scratch_bytes)
    steps, mixed, launches = 0, 0, [0, 0, 0]
    for a, b in runs:
        rounds = max(len(sequences[i]) + (1 if finals[i] else 0) for i in range(a, b))
        steps += rounds
        for r in range(rounds):
            kinds = {sequences[i][r] for i in range(a, b) if r < len(sequences[i]) and sizes[i] > 0}
            final = any(finals[i] and len(sequences[i]) == r for i in range(a, b))
            for k in kinds:
                launches[k] += 1
            if len(kinds) + (1 if final else 0) > 1:
                mixed += 1
    return dict(pairs=len(sequences), chunks=len(runs), steps=steps, read_backs=steps,
                max_in_flight=max([b - a for a, b in runs], default=0), pair_evaluations=sum(len(s) for s in sequences),
                pair_searches=sum(1 for f in finals if f), evaluation_launches=launches, mixed_steps=mixed)


def rounds_of(sequence, final):
    """A result's read_backs in a batch: the pair's rounds"""
    return len(sequence) + (1 if final else 0)


# ---- the zoo --------------------------------------------------------------------------------------------------------------------
def blob(rng, centre, n, spread=0.15):
    return (np.asarray(centre) + spread * rng.standard_normal((n, 3))).astype(np.float32)


def scene_points():
    """About 280 valid cells in 3.6 k points: blobs on a 10 x 10 x 3 lattice of cell centres (tests/test_gpu_ndt.py's scene)"""
    rng = np.random.RandomState(5)
    centres = np.stack(np.meshgrid(np.arange(-5, 5), np.arange(-5, 5), np.arange(-1, 2)), axis=-1).reshape(-1, 3) + 0.5
    return np.concatenate([blob(rng, c + rng.uniform(-0.2, 0.2, 3), rng.randint(4, 20)) for c in centres])


def zoo_targets():
    """name -> points: a scene, a target without a valid cell (five points), one with exactly one valid cell"""
    rng = np.random.RandomState(6)
    one = (np.array([0.5, 0.5, 0.5]) + rng.uniform(-0.3, 0.3, (16, 3))).astype(np.float32)
    return {"scene": scene_points(), "none": one[:5].copy(), "one": one}


def zoo_pairs():
    """17 pairs as (target name, source (n, 3) float32, guess 4x4 or None, with a fitness index): every source size, the
    three targets, the three guesses.  Pair 3 is a copy of scene points under the identity (it ends by the epsilon)."""
    targets = zoo_targets()
    scene = targets["scene"]
    rng = np.random.RandomState(29)
    pairs = []
    for i in range(17):
        n = SOURCE_SIZES[i % len(SOURCE_SIZES)]
        name = "none" if i == 9 else ("one" if i in (8, 12) else "scene")
        guess = (None, GENERIC_GUESS, MOVED_GUESS)[i % 3]
        picked = scene[rng.randint(0, len(scene), n)]
        if i == 3:
            source, guess = picked.copy(), None
        else:
            moved = nd.pose_terms([0.1, -0.05, 0.02, 0.01, 0.02, -0.03] if guess is None or i % 3 == 1 else [0.0] * 6)
            noisy = picked + (0.03 * rng.standard_normal((n, 3))).astype(np.float32)
            inverse_R = np.array(moved[0]).T
            source = ((noisy.astype(np.float64) - np.array(moved[1])) @ inverse_R.T).astype(np.float32).reshape(-1, 3)
        if name == "one":
            source = (source * np.float32(0.05) + np.float32(0.5)).astype(np.float32)  # into and around the one cell
        pairs.append((name, np.ascontiguousarray(source, np.float32).reshape(-1, 3), guess, i % 4 != 1))
    return targets, pairs


_MODEL = {}


def zoo_model(mode):
    """The CPU model of every zoo pair under `mode`, computed once and left unchanged -> [(result, kinds)]"""
    if mode not in _MODEL:
        targets, pairs = zoo_pairs()
        o = nd.options(step_mode=mode, **ZOO_OPTIONS)
        cells = {name: nd.build_cells(points, o) for name, points in targets.items()}
        _MODEL[mode] = [model_alignment(cells[name], source, targets[name] if fitness else None, guess, o)
                        for name, source, guess, fitness in pairs]
    return _MODEL[mode]
