"""The export stages' voxel table (d-liom_amd/csrc/voxel_hash.h, voxel_table.hip) where hashing is crowded: chains of 64
keys with one home entry, the wrap from the last entry to entry 0, a growth to eight times the size over such a chain,
and whole wavefronts that race for the entries of one chain -- in moving-object removal (outlier.hip, the leaf table) and
in the point-cloud x-ray (points_xray.hip, the leaf table and the column table).

The inputs come from tests/voxel_table_common.py: voxels whose keys collide, found on the host with a mirror of
hash_key.  tests/test_voxel_table_host.py shows on a sequential model of the table that every case is crowded as it
claims.  Every comparison here is exact equality with the CPU model of the stage (a std::map: it shares nothing with
the table): for the remover the whole voxel table (keys, hits, rays) after every mark and at the end, every kept_index and
the kept clouds' bytes; for the x-ray the column table with its sums as bits, the voxel list, the bounding box and the
image bytes.

Each test proves that it was crowded: `probes`, the entries the device's look-ups read, is at least what the layout
forces (voxel_table_common.py, "The probe sums": L (L + 1) / 2 for L keys with one home entry, looked up once each).
Were the mirror of the hash wrong, or the hash changed, the keys would no longer collide and these bounds would fail."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voxel_table_common as vt  # noqa: E402
from voxel_table_common import FILTER, MARK, oc, xc  # noqa: E402

pytestmark = pytest.mark.gpu
KINDS = ["leaves", "columns"]
VS = vt.VOXEL_SIZE


@pytest.fixture(scope="module")
def dl():
    import dliom
    return dliom


@pytest.fixture(scope="module")
def ctx(dl):
    c = dl.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def remover_model(tmp_path_factory):
    return oc.build_model(tmp_path_factory.mktemp("outlier_model"))


@pytest.fixture(scope="module")
def xray_model(tmp_path_factory):
    return xc.build_model(tmp_path_factory.mktemp("points_xray_model"))


# ---- moving-object removal ---------------------------------------------------------------------------------------------
def assert_table_equal(remover, table):
    xyz, hits, rays = remover.voxels()
    assert np.array_equal(xyz, table[0]) and np.array_equal(hits, table[1]) and np.array_equal(rays, table[2])
    return xyz, hits, rays


def run_remover(dl, ctx, model, directory, ops, probes_after):
    """`ops` on the model and on one OutlierRemover, compared after every mark, at every filter and at the end
    -> (stats after every mark, `probes` after the first `probes_after` operations, stats at the end, the device's table
    at the end)."""
    results, table = oc.run_model(model, VS, ops, directory)
    assert all((r if isinstance(r, int) else r[0]) == 0 for r in results), "a case may not contain a refusal"
    after_mark = [oc.run_model(model, VS, ops[:k + 1], directory)[1] for k, o in enumerate(ops) if o[0] == MARK]
    r = dl.OutlierRemover(ctx, VS)
    mark_stats, probes = [], None
    try:
        for done, ((kind, origin, _, _, pts), want) in enumerate(zip(ops, results)):
            if done == probes_after:
                probes = r.stats()["probes"]
            cloud = dl.PointCloud(ctx, pts)
            try:
                if kind == MARK:
                    r.mark_hits(cloud)
                    assert_table_equal(r, after_mark[len(mark_stats)])
                    mark_stats.append(r.stats())
                elif kind == FILTER:
                    kept, index = r.filter(cloud)
                    try:
                        assert np.array_equal(index, want[1])
                        assert kept.download().tobytes() == pts[want[1]].tobytes()
                    finally:
                        kept.close()
                else:
                    r.count_rays(origin, cloud)
            finally:
                cloud.close()
        voxels = assert_table_equal(r, table)
        stats = r.stats()
        assert stats["voxels"] == len(table[1]) and stats["phase"] == 3
    finally:
        r.close()
    return mark_stats, probes, stats, voxels


@pytest.mark.parametrize("name", vt.REMOVER_CASES)
def test_remover_equals_model_on_a_crowded_table(dl, ctx, remover_model, tmp_path, name):
    """a. one chain of 64 among 200 ordinary points; b. 40 keys on the last entry and 10 on entries 0 and 1; c. 64 keys,
    then 3000 points that grow the table from 1024 to 8192 entries in one step, then the 64 voxels again; d. 64 keys hit
    by 128 points each, adjacent and shuffled; e. case a with rays through the crowded voxels to 2x and 3x their distance.

    Pass 2 looks a leaf up for every leaf a ray crosses, so the long rays' `probes` are mostly misses on the way.  Before
    them, a to d send one short ray (one sample, one look-up, nothing counted) to every leaf of the table (c: to the 64
    crowded ones): what those read is the chains' sum and nothing else -- exactly, where every key of the table is looked
    up.  Then rays go from the origin to the centre cells of the crowded leaves (in a and b to every point): each of
    those leaves is looked up again at the ray's end."""
    case, short, ray_clouds, more = vt.remover_case(name)
    ops = vt.remover_ops(case, short, ray_clouds, more)
    mark_stats, short_probes, stats, (xyz, hits, rays) = run_remover(dl, ctx, remover_model, tmp_path, ops,
                                                                    len(case.batches) + len(short))
    bound, _ = vt.remover_probe_bound(case, ray_clouds[0])
    print("remover %s: probes %d after the short rays, %d at the end, bound %d for either, L (L + 1) / 2 = %d; %s" % (
        name, short_probes, stats["probes"], bound, vt.chain_bound(case.length), stats))
    assert [s["table_capacity"] for s in mark_stats] == case.capacities
    assert stats["leaves"] == len(np.unique(vt.leaf_key(np.concatenate(case.batches))))
    assert bound >= vt.chain_bound(case.length) and stats["probes"] >= short_probes + bound
    if len(short) > 0:
        short_bound, exact = vt.remover_probe_bound(case, short)
        assert short_bound == bound and short_probes >= short_bound
        assert short_probes == short_bound or not exact
    crowd = set(tuple(int(v) for v in c) for c in case.crowd)
    device = {tuple(int(v) for v in c): (int(h), int(r)) for c, h, r in zip(xyz, hits, rays)}
    if name == "growth":
        assert mark_stats[1]["growths"] > mark_stats[0]["growths"]
        assert set(c for c, (h, _) in device.items() if h == 2) == crowd and len(device) == 3064
    if name.startswith("contention"):
        assert set(device) == crowd and all(h == 128 for h, _ in device.values())
    if name == "ray_walk":
        assert any(device[c][1] >= 3 * device[c][0] for c in crowd)
        assert any(0 < device[c][1] < 3 * device[c][0] for c in crowd)


# ---- the point-cloud x-ray ----------------------------------------------------------------------------------------------
def compare_xray(dl, ctx, model, directory, case, colors="point", batches=None):
    ops = vt.xray_ops(case, colors)[:batches]
    result, stats, _ = xc.compare(dl, ctx, model, VS, xc.IDENTITY, ops, directory, need_honest=False)
    return result, stats[0]


def assert_crowded_xray(case, stats):
    """The slot counts read back are the distinct keys; `probes` is at least what the two tables' layouts force, which is
    at least the crowded chain's sum and one entry for every other look-up in that table (and one a point in the other)."""
    voxels = np.concatenate(case.batches)
    points = len(voxels)
    bound, exact = vt.xray_probe_bound(case)
    print("x-ray %s (%s): probes %d, bound %d, L (L + 1) / 2 + (points - L) = %d; %s" % (
        case.name, case.kind, stats["probes"], bound, vt.chain_bound(case.length) + points - case.length, stats))
    assert stats["points"] == points and stats["inserts"] == len(case.batches)
    assert stats["leaves"] == len(np.unique(vt.leaf_key(voxels))) and stats["columns"] == len(np.unique(vt.column_key(voxels[:, 1:])))
    assert bound >= vt.chain_bound(case.length) + (points - case.length) + points
    assert stats["probes"] >= bound
    assert stats["probes"] == bound or not exact  # one point a key in both tables: nothing else to read


@pytest.mark.parametrize("kind", KINDS)
def test_xray_one_chain(dl, ctx, xray_model, tmp_path, kind):
    """a. 64 colliding leaves, or 64 colliding columns of 3 to 70 points each with per-point colours (one lane sums up to
    64 points of a column, a wavefront more: neighbouring entries of the chain take both paths), among 200 ordinary
    points, in one batch."""
    case = vt.one_chain(kind)
    result, stats = compare_xray(dl, ctx, xray_model, tmp_path, case)
    assert_crowded_xray(case, stats)
    if kind == "columns":
        assert stats["longest_segment"] == 70 == result.aggregations[0]["counts"].max()


@pytest.mark.parametrize("kind", KINDS)
def test_xray_wrap_around(dl, ctx, xray_model, tmp_path, kind):
    """b. 40 keys whose home is entry 1023 of 1024 and 10 whose home is entry 0 or 1: the chain runs 1023, 0, 1, ... 48."""
    case = vt.wrap_around(kind)
    _, stats = compare_xray(dl, ctx, xray_model, tmp_path, case)
    assert_crowded_xray(case, stats)


@pytest.mark.parametrize("kind", KINDS)
def test_xray_growth_over_a_crowded_chain(dl, ctx, xray_model, tmp_path, kind):
    """c. 64 colliding keys, 3000 points that grow both tables from 1024 to 8192 entries in one step, the 64 voxels again;
    compared after every insert."""
    case = vt.growth(kind)
    _, first = compare_xray(dl, ctx, xray_model, tmp_path, case, batches=1)
    _, second = compare_xray(dl, ctx, xray_model, tmp_path, case, batches=2)
    result, stats = compare_xray(dl, ctx, xray_model, tmp_path, case)
    assert_crowded_xray(case, stats)
    assert second["growths"] > first["growths"] and stats["growths"] == second["growths"]
    assert (first["voxels"], second["voxels"], stats["voxels"]) == (64, 3064, 3064)
    a = result.aggregations[0]
    if kind == "columns":
        twice = set(tuple(int(v) for v in yz) for yz in a["yz"][a["counts"] == 2])
        assert twice == set(tuple(int(v) for v in c) for c in case.crowd) and len(a["yz"]) == 3064


@pytest.mark.parametrize("colors", ["none", "point"])
@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_xray_contention(dl, ctx, xray_model, tmp_path, kind, shuffled, colors):
    """d. 64 colliding keys, each hit by 128 points of one batch of 8192 (32 workgroups, capacity 16384): adjacent, so that a
    wave's 64 lanes claim one key, and shuffled, so that they hold many keys of the one chain."""
    case = vt.contention(kind, shuffled)
    result, stats = compare_xray(dl, ctx, xray_model, tmp_path, case, colors)
    assert_crowded_xray(case, stats)
    a = result.aggregations[0]
    assert int(a["counts"].sum()) == 8192 and np.all(a["counts"] % 128 == 0)
    if kind == "columns":
        assert stats["columns"] == 64 and np.all(a["counts"] == 128) and stats["longest_segment"] == 128
    else:
        assert stats["leaves"] == 64 and stats["voxels"] == 64
