"""The chunk scan's two-level walk (d-liom_amd/csrc/sequential_sums.hip, method 2): wave 0 walks every binade of the
sequential float sum alone -- whole super-chunks of 4 096 additions, then the 64 chunks of the super-chunk that halts it,
then the 64 elements of the crossing chunk -- and the last rescoring kernel writes the match's read-back itself.

The sizes are the smallest at which the super-chunk level can go wrong: 4 097, 8 193, 12 289 and 20 000 points (one
addition behind a super-chunk edge, behind the former limit of wave 0's own passes, behind three super-chunks, and a
cloud whose last super-chunk is cut).  The grids: one whose cells all hold one of five values with probabilities 0.1,
0.3, 0.5, 0.7 and 0.9 (round-to-even ties everywhere; a mean of 0.5, so the sum reaches 2^k around addition 2^(k+1) and
the binade crossings of different candidates scatter around the super-chunk edges), one all-32767 and one without a
cell near any look-up (every look-up unknown).

Where the crossings fall is computed HERE, on the CPU, from np.cumsum of every checked candidate's float32
probabilities -- which is the sequential sum, and is held against the oracle's loop first.  test_inputs_cover_the_walks_edges
fails if the candidates do not contain a crossing in the first and in the last chunk of a super-chunk, at element 0 and
at element 63 of a chunk, and a pass that resumes in the last element of a chunk."""
import numpy as np
import pytest

from helpers import DEFAULT_RTCSM, build_oracle_submap, to_device_grid

SIZES = (4097, 8193, 12289, 20000)
GRIDS = ("ties", "saturated", "unknown")
SERIAL_PREFIX = 256  # additions replayed one by one in front of the walk
CHUNK, SUPER = 64, 4096
TIE_VALUES = np.array([1, 8192, 16384, 24576, 32767], dtype=np.uint16)
CANDIDATES = {"ties": 24, "saturated": 2, "unknown": 2}
HALF = 32  # the filled cube, in cells: [-32, 32)^3 around the points' [-2.5 m, 2.5 m]^3 and the search window


def _grid(orc, kind):
    og = orc.HybridGrid(0.1)
    if kind == "unknown":
        og.set_values(np.array([[400, 400, 400]]), np.array([32767], dtype=np.uint16))  # far from every look-up
        return og
    ax = np.arange(-HALF, HALF)
    xyz = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1).reshape(-1, 3)
    if kind == "ties":
        vals = np.random.RandomState(11).choice(TIE_VALUES, size=len(xyz))
    else:
        vals = np.full(len(xyz), 32767, dtype=np.uint16)
    og.set_values(xyz, vals)
    return og


def _crossings(cum):
    """Indices of the additions behind the serial prefix whose result is in a higher binade than the sum in front."""
    exps = cum.view(np.uint32) >> 23
    i = np.nonzero(exps[1:] != exps[:-1])[0] + 1
    return i[i >= SERIAL_PREFIX]


@pytest.fixture(scope="module")
def cases(orc):
    """(grid kind, n) -> oracle grid, points, initial pose, candidate indices, the oracle's sums and the crossings of
    every candidate's sequential sum: computed once, on the CPU."""
    table = orc.value_to_probability_table()
    init = orc.pose((0.01, -0.02, 0.03))
    grids = {kind: _grid(orc, kind) for kind in GRIDS}
    out = {}
    for kind in GRIDS:
        for n in SIZES:
            rng = np.random.RandomState(n)
            pts = rng.uniform(-2.5, 2.5, size=(n, 3)).astype(np.float32)
            w = orc.rtcsm3d_window(DEFAULT_RTCSM, 0.1, pts)
            num = (2 * w["linear_window"] + 1) ** 3 * (2 * w["angular_window"] + 1) ** 3
            idx = np.unique(np.concatenate([[0, num - 1], rng.randint(0, num, size=CANDIDATES[kind] - 2)])).astype(np.int64)
            want = orc.rtcsm3d_float_sums(DEFAULT_RTCSM, init, pts, grids[kind], idx)
            _, absolute = orc.rtcsm3d_candidates(DEFAULT_RTCSM, 0.1, pts, init)
            assert len(absolute) == num
            crossings = []
            for k, c in enumerate(idx):
                cells = orc.transform_cell_indices(absolute[c], pts, 0.1)
                cum = np.cumsum(table[grids[kind].values(cells) & 0x7FFF], dtype=np.float32)
                assert cum[-1].tobytes() == want[k].tobytes(), (kind, n, int(c))  # np.cumsum IS the reference's loop
                crossings.append(_crossings(cum))
            out[kind, n] = dict(og=grids[kind], pts=pts, init=init, idx=idx, want=want, crossings=crossings)
    return out


def test_inputs_cover_the_walks_edges(cases):
    """Without a GPU: the candidates the GPU test checks cross binades at every edge of the two-level walk."""
    hits = dict(first_chunk_of_super=0, last_chunk_of_super=0, element_0=0, element_63=0, resumes_in_last_element=0,
                behind_one_super_chunk=0, all=0)
    for (kind, n), case in cases.items():
        for cr in case["crossings"]:
            chunk_in_super, element = (cr // CHUNK) % (SUPER // CHUNK), cr % CHUNK
            hits["all"] += len(cr)
            hits["behind_one_super_chunk"] += int(np.sum(cr >= SUPER))
            hits["first_chunk_of_super"] += int(np.sum((chunk_in_super == 0) & (cr >= SUPER)))
            hits["last_chunk_of_super"] += int(np.sum(chunk_in_super == SUPER // CHUNK - 1))
            hits["element_0"] += int(np.sum(element == 0))
            hits["element_63"] += int(np.sum(element == CHUNK - 1))
            hits["resumes_in_last_element"] += int(np.sum((element == CHUNK - 2) & (cr + 1 < n)))
    print(hits)
    missing = [k for k, v in hits.items() if v == 0]
    assert not missing, "inputs do not cover: %s" % ", ".join(missing)


@pytest.fixture(scope="module")
def dl():
    import dliom
    dliom.load_library()
    assert dliom.device_count() > 0, "no HIP device: the GPU tests must not pass on a fallback"
    return dliom


@pytest.fixture(scope="module")
def ctx(dl):
    c = dl.Context(0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", GRIDS)
@pytest.mark.parametrize("n", SIZES)
def test_two_level_walk_bit_exact(dl, ctx, cases, kind, n):
    """Method 2 (the walk) equals method 0 (one lane replays the loop) and the oracle's loop bit for bit."""
    case = cases[kind, n]
    dg = to_device_grid(dl, ctx, case["og"])
    m = dl.RealTimeCorrelativeScanMatcher3D(ctx, DEFAULT_RTCSM)
    assert m.window(0.1, case["pts"]).num_candidates > case["idx"].max()
    serial = m.sequential_sums(case["init"], case["pts"], dg, case["idx"], 0)
    walk = m.sequential_sums(case["init"], case["pts"], dg, case["idx"], 2)
    dg.close()
    print(kind, n, [len(c) for c in case["crossings"]])
    assert np.array_equal(serial.view(np.uint32), case["want"].view(np.uint32))
    assert np.array_equal(walk.view(np.uint32), case["want"].view(np.uint32))
    assert np.array_equal(walk.view(np.uint32), serial.view(np.uint32))


# The parent commit's num_rescored for the two matches below (the oracle does not compute the bounds): the same count
# means that the bounds kernel's table look-up left every lo[] / hi[] where the per-candidate loop put it.
PARENT_NUM_RESCORED = {(32, 512): 1, (8, 40): 1}


@pytest.mark.gpu
@pytest.mark.parametrize("beams,azimuths,max_range", [(32, 512, None), (8, 40, 15.0)])
def test_match_equals_oracle_and_parent(dl, ctx, orc, beams, azimuths, max_range):
    """One whole match with the chunk scan (16 384 points) and one with the serial replay (a few hundred): winner, score
    bits and pose are the oracle's, num_rescored the parent's, through the read-back the rescoring kernel writes."""
    from dliom import synth
    og = build_oracle_submap(orc, 0.1, num_scans=6, beams=16, azimuths=256)
    truth = synth.trajectory_pose(0.6)
    pts, _ = synth.scan(truth, beams, azimuths)
    if max_range is not None:
        pts = synth.range_filter(pts, max_range)
    init = synth.perturb_pose(truth, 0.1, 0.5, seed=13)
    dg = to_device_grid(dl, ctx, og)
    m = dl.RealTimeCorrelativeScanMatcher3D(ctx, DEFAULT_RTCSM)
    score, pose = m.Match(init, pts, dg)
    st = m.last_stats()
    score2, pose2 = m.Match(init, pts, dg)  # the arrival counter was re-armed
    st2 = m.last_stats()
    box_error = m.box_error()
    dg.close()
    ref = orc.rtcsm3d_match_parallel(DEFAULT_RTCSM, init, pts, og, threads=8)
    print(beams, azimuths, len(pts), st.best_index, st.num_rescored, score)
    assert st.best_index == ref["best_index"] == st2.best_index
    assert np.float32(score).tobytes() == np.float32(ref["score"]).tobytes() == np.float32(score2).tobytes()
    assert np.array_equal(pose, ref["pose"]) and np.array_equal(pose2, pose)
    assert st.num_rescored == PARENT_NUM_RESCORED[beams, azimuths] == st2.num_rescored
    assert box_error == 0
