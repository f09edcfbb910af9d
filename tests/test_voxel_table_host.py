"""The export stages' voxel table under crowded hashing, without a GPU: the sequential model of the table
(tests/voxel_table_common.py) shows that every case of tests/test_gpu_voxel_table.py is crowded in the way it claims --
the chain's length, the wrap past the last entry, the collision's survival through the growth the case triggers -- and
the two CPU models (tests/cpp/outlier_model.cc, tests/cpp/points_xray_model.cc) accept every case and meet the
conditions the device tests rely on.  The seeds of the cases were chosen here."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voxel_table_common as vt  # noqa: E402
from voxel_table_common import oc, xc  # noqa: E402

KINDS = ["leaves", "columns"]


@pytest.fixture(scope="module")
def remover_model(tmp_path_factory):
    return oc.build_model(tmp_path_factory.mktemp("outlier_model"))


@pytest.fixture(scope="module")
def xray_model(tmp_path_factory):
    return xc.build_model(tmp_path_factory.mktemp("points_xray_model"))


def run_of(table, entry):
    """The run of occupied entries around `entry` -> (first entry, length)."""
    mask = table.capacity - 1
    first = entry
    while table.keys[(first - 1) & mask] is not None:
        first = (first - 1) & mask
    length = 0
    while table.keys[(first + length) & mask] is not None:
        length += 1
    return first, length


def one_home(table, keys):
    homes = {table.home(k) for k in keys}
    assert len(homes) == 1, homes
    return homes.pop()


# ---- the mirrors and the sequential model ------------------------------------------------------------------------------
def test_mirrors_agree_and_keys_are_the_stated_bit_fields():
    rng = np.random.RandomState(0)
    keys = rng.randint(0, 1 << 62, 1000, dtype=np.int64).astype(np.uint64)
    assert [vt.hash_int(int(k)) for k in keys] == vt.hash_key(keys).tolist()
    assert vt.hash_int(0) == 0 and vt.hash_key([0]).tolist() == [0]  # every step of the finaliser maps 0 to 0
    # the finaliser is a bijection of 64 bits made of xor-shifts and odd multipliers: one flipped input bit changes the hash
    assert len(set(vt.hash_int(1 << b) for b in range(42))) == 42
    assert vt.leaf_key([[-8192, -8192, -8192]]).tolist() == [0]
    assert vt.leaf_key([[8191, -8192, -8192], [-8192, 8191, -8192], [-8192, -8192, 8191]]).tolist() == [2047, 2047 << 14, 2047 << 28]
    assert vt.leaf_key([[7, 8, -1]]).tolist() == [1024 | (1025 << 14) | (1023 << 28)]
    assert vt.column_key([[-8192, -8192], [8191, 8191], [0, 1]]).tolist() == [0, (16383 << 14) | 16383, (8192 << 14) | 8193]


def test_colliding_keys_collide_are_distinct_centred_and_hold_the_corners():
    for bits, bucket in ((10, 1023), (10, 0), (14, vt.LEAVES.corner_bucket(14, 80)), (16, vt.LEAVES.corner_bucket(16, 64))):
        voxels = vt.colliding_leaves(40, bits, bucket)
        assert np.all((vt.hash_key(vt.leaf_key(voxels)) & ((1 << bits) - 1)) == bucket)
        assert len(np.unique(vt.leaf_key(voxels))) == 40 and np.all((voxels & 7) == 4)
        assert np.all((voxels >= -8192) & (voxels <= 8191))
        assert voxels is vt.colliding_leaves(40, bits, bucket) and not voxels.flags.writeable  # searched once, left unchanged
        # the corner leaves of the bucket come first; the buckets of the cases hold both kinds
        assert -8188 in voxels[:8, 0] and 8188 in voxels[:8, 0], (bits, bucket, voxels[:8, 0])
    for bits, bucket in ((10, 1023), (10, 1), (14, vt.COLUMNS.corner_bucket(14, 80)), (16, vt.COLUMNS.corner_bucket(16, 64))):
        columns = vt.colliding_columns(64, bits, bucket)
        assert np.all((vt.hash_key(vt.column_key(columns)) & ((1 << bits) - 1)) == bucket)
        assert len(np.unique(vt.column_key(columns))) == 64
        assert -8192 in columns[:8, 0] or 8191 in columns[:8, 0]


def test_sequential_table_keeps_slots_and_its_probe_sum_ignores_the_order():
    rng = np.random.RandomState(5)
    keys = [int(k) for k in vt.leaf_key(np.concatenate([vt.colliding_leaves(64, 14, 3), vt.colliding_leaves(30, 10, 1023),
                                                        vt.LEAVES.ordinary(300, 6, 14, 3)]))]
    sums, occupied = set(), set()
    for trial in range(6):
        order = keys if trial == 0 else [keys[i] for i in rng.permutation(len(keys))]
        t = vt.Table()
        t.insert_batch(order + order[:10])  # claimed twice: one slot
        assert t.capacity == 1024 and len(t.slot_key) == len(keys) and t.growths == 0
        assert all(t.find(k) == (s, t.find(k)[1]) for s, k in enumerate(t.slot_key)) and t.find(12345)[0] is None
        assert t.probe_sum() == vt.closed_form_probe_sum(t)
        sums.add(t.probe_sum())
        occupied.add(tuple(t.occupied()))
        before = {k: t.find(k)[0] for k in keys}
        t.grow(2000, order=None if trial == 0 else rng.permutation(len(keys)))  # 1024 -> 4096 in one step
        assert t.capacity == 4096 and t.growths == 1 and {k: t.find(k)[0] for k in keys} == before
        assert t.probe_sum() == vt.closed_form_probe_sum(t)
        assert t.probe_sum(keys[:64]) >= vt.chain_bound(64)  # 14 shared bits outlive a table of 12
    assert len(sums) == 1 and len(occupied) == 1
    # L keys with one home and nothing in their way: L (L + 1) / 2
    t = vt.Table()
    t.insert_batch(keys[:64])
    assert t.probe_sum() == vt.chain_bound(64) == 2080


# ---- the cases are crowded as they claim ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_one_chain_is_one_chain_that_other_keys_run_into(kind):
    case = vt.one_chain(kind)
    table, capacities = vt.simulate(case)
    assert capacities == case.capacities and case.length == 64 and len(table.slot_key) == 264
    home = one_home(table, case.crowd_keys)
    first, length = run_of(table, home)
    others = [int(k) for k in vt.key_function(kind)(case.others)]
    near = [k for k in others if ((table.home(k) - home + 4) & (table.capacity - 1)) < 68]
    inside = [k for k in near if ((table.home(k) - home) & (table.capacity - 1)) < 64]
    # a key whose home is one of the 64 entries from the crowd's home on lies in the crowd's run, whatever the order
    assert len(near) >= 50 and len(inside) >= 40 and length >= 64 + len(inside)
    assert table.probe_sum(case.crowd_keys) >= vt.chain_bound(64)
    assert max(table.find(k)[1] for k in case.crowd_keys) >= 64
    assert sum(table.find(k)[1] > 1 for k in near) >= 40  # in batch order; the sum over all keys holds for every order
    assert table.probe_sum() == vt.closed_form_probe_sum(table) >= vt.chain_bound(64) + 200
    if kind == "leaves":
        assert capacities == [1024] and len(case.batches[0]) == 264
    else:
        _, counts = np.unique(vt.column_key(case.batches[0][:, 1:]), return_counts=True)
        crowd_counts = sorted(counts[counts > 1].tolist())
        assert len(crowd_counts) == 64 and crowd_counts[0] == 3 and crowd_counts[-1] == 70
        assert 64 in crowd_counts and 65 in crowd_counts  # one lane sums up to 64 points of a column, a wavefront more
        assert capacities == [8192] and 2 * len(case.batches[0]) > 4096  # 14 shared bits: one home in 8192 entries too
        # a column's points are not adjacent in the batch: only a stable sort keeps them in order
        keys = vt.column_key(case.batches[0][:, 1:])
        assert np.mean(keys[1:] == keys[:-1]) < 0.1


@pytest.mark.parametrize("kind", KINDS)
def test_wrap_around_fills_the_last_entry_and_the_first_ones(kind):
    case = vt.wrap_around(kind)
    alone = vt.Table()
    alone.insert_batch(case.crowd_keys)
    assert alone.capacity == 1024 and one_home(alone, case.crowd_keys) == 1023
    assert alone.occupied() == list(range(39)) + [1023]
    table, capacities = vt.simulate(case)
    assert capacities == [1024] and table.occupied() == list(range(49)) + [1023]
    behind = [int(k) for k in (vt.leaf_key(case.behind) if kind == "leaves" else vt.column_key(case.behind))]
    assert sorted(table.home(k) for k in behind) == [0] * 5 + [1] * 5
    # entries 1023 .. 1023 + 49 from homes 40 x 1023, 5 x 1024, 5 x 1025: 50 + 1225 - 15, whatever the order
    assert table.probe_sum() == vt.closed_form_probe_sum(table) == 1260 >= vt.chain_bound(40) + 10


@pytest.mark.parametrize("kind", KINDS)
def test_growth_keeps_the_collision(kind):
    case = vt.growth(kind)
    table, capacities = vt.simulate(case, batches=1)
    assert capacities == [1024] and one_home(table, case.crowd_keys) is not None and table.probe_sum() == vt.chain_bound(64)
    slots = {k: table.find(k)[0] for k in case.crowd_keys}
    table, capacities = vt.simulate(case)
    assert capacities == case.capacities == [1024, 8192, 8192] and table.growths == 1  # one step to eight times the size
    assert len(table.slot_key) == 3064 and len(case.batches[1]) == 3000
    one_home(table, case.crowd_keys)
    assert {k: table.find(k)[0] for k in case.crowd_keys} == slots
    assert table.probe_sum(case.crowd_keys) >= vt.chain_bound(64)
    key_of = vt.key_function(kind)
    assert len(np.unique(key_of(case.batches[1]))) == 3000 and not set(key_of(case.batches[1]).tolist()) & set(case.crowd_keys)
    assert sorted(key_of(case.batches[2]).tolist()) == sorted(case.crowd_keys)
    assert np.array_equal(np.sort(key_of(case.batches[0])), np.sort(key_of(case.batches[2])))


@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_contention_puts_whole_waves_on_one_chain(kind, shuffled):
    case = vt.contention(kind, shuffled)
    table, capacities = vt.simulate(case)
    assert capacities == [16384] and len(case.batches[0]) == 8192 and len(table.slot_key) == 64
    one_home(table, case.crowd_keys)
    assert table.probe_sum() == vt.chain_bound(64)
    keys = vt.key_function(kind)(case.batches[0])
    assert np.all(np.unique(keys, return_counts=True)[1] == 128)
    per_wave = [len(np.unique(keys[w:w + 64])) for w in range(0, 8192, 64)]
    assert (min(per_wave) >= 30) if shuffled else (max(per_wave) == 1), (min(per_wave), max(per_wave))
    assert vt.lookup_bound(table, keys) == 128 * vt.chain_bound(64)


# ---- the CPU models accept every case and meet the conditions -----------------------------------------------------------
def table_dict(table):
    return {tuple(int(v) for v in c): (int(h), int(r)) for c, h, r in zip(*table)}


@pytest.mark.parametrize("name", vt.REMOVER_CASES)
def test_remover_model_accepts_the_case_and_meets_its_conditions(remover_model, tmp_path, name):
    case, short, ray_clouds, more = vt.remover_case(name)
    ops = vt.remover_ops(case, short, ray_clouds, more)
    results, table = oc.run_model(remover_model, vt.VOXEL_SIZE, ops, tmp_path)
    assert all((r if isinstance(r, int) else r[0]) == 0 for r in results), "a refusal"
    voxels = table_dict(table)
    crowd = [tuple(int(v) for v in c) for c in case.crowd]
    assert all(c in voxels for c in crowd)  # a point c * 0.5 lands in voxel c
    bound, exact = vt.remover_probe_bound(case, ray_clouds[0])
    assert bound >= vt.chain_bound(case.length)
    if len(short) > 0:
        # the short rays look the same leaves up, every crowded one among them; all of the table's except in `growth`
        assert vt.remover_probe_bound(case, short) == (bound, name != "growth")
        assert set(crowd) <= set(tuple(int(v) for v in c) for c in short)
        # a short ray is one sample, in the cell before its end: it reads the end's leaf once and counts nothing
        without = oc.run_model(remover_model, vt.VOXEL_SIZE, vt.remover_ops(case, (), ray_clouds, more), tmp_path)
        assert all(np.array_equal(a, b) for a, b in zip(table, without[1]))
        for v in short[:8]:
            _, origin, _, _, end = vt.short_ray(v)
            (trace,), _ = oc.run_model(remover_model, vt.VOXEL_SIZE, [oc.op(oc.TRACE, end, origin)], tmp_path)
            assert len(trace) == 1 and trace[0][0].tolist() == [[int(v[0]) - 1, int(v[1]), int(v[2])]]
            assert (int(v[0]) - 1) >> 3 == int(v[0]) >> 3
    if name == "growth":
        assert sorted(c for c, (hits, _) in voxels.items() if hits == 2) == sorted(crowd)
        assert len(voxels) == 3064
    if name.startswith("contention"):
        assert sorted(voxels) == sorted(crowd) and all(hits == 128 for hits, _ in voxels.values())
        kept = results[-1][1]
        assert len(kept) == 8192  # 64 rays cannot reach 3 * 128
    if name == "ray_walk":
        assert len(ray_clouds) == 3 and len(ray_clouds[0]) == 64 and len(ray_clouds[1]) >= 10 and len(ray_clouds[2]) >= 5
        rays = [voxels[c][1] for c in crowd]
        assert all(voxels[c][0] == 1 for c in crowd)
        removed, survives = sum(r >= 3 for r in rays), sum(0 < r < 3 for r in rays)
        print("crowded voxels with rays >= 3 * hits: %d, with 0 < rays < 3 * hits: %d" % (removed, survives))
        assert removed >= 1 and survives >= 1
        kept = results[len(case.batches) + len(ray_clouds)][1]  # of the marked cloud
        assert 0 < len(kept) < len(case.batches[0])
        assert all(len(r[1]) == 0 for r in results[-2:])  # the clouds at 2x and 3x hit no marked voxel


@pytest.mark.parametrize("kind", KINDS)
def test_xray_model_accepts_the_cases_and_meets_their_conditions(xray_model, tmp_path, kind):
    for case in (vt.one_chain(kind), vt.wrap_around(kind), vt.growth(kind), vt.contention(kind, True)):
        points = sum(len(b) for b in case.batches)
        result = xc.run_model(xray_model, vt.VOXEL_SIZE, xc.IDENTITY, vt.xray_ops(case), tmp_path)
        assert result.statuses == [0] * len(case.batches), case.name
        a = result.aggregations[0]
        table = vt.simulate(case, "columns")[0]
        assert len(a["yz"]) == len(table.slot_key) and int(a["counts"].sum()) == points
        distinct = len(np.unique(np.concatenate(case.batches), axis=0))
        assert len(a["voxels"]) == distinct == int(a["occupied"].sum())
        bound, exact = vt.xray_probe_bound(case)
        assert bound >= vt.chain_bound(case.length) + (points - case.length) + points
        assert exact == (case.name == "wrap-around")  # one point a leaf and a column: `probes` can only be the bound
        crowd_columns = set(tuple(int(v) for v in c) for c in (case.crowd[:, 1:] if kind == "leaves" else case.crowd))
        counts = {tuple(int(v) for v in yz): int(n) for yz, n in zip(a["yz"], a["counts"])}
        if case.name == "growth" and kind == "columns":
            assert set(c for c, n in counts.items() if n == 2) == crowd_columns and len(counts) == 3064
        if case.name == "contention":
            assert all(counts[c] % 128 == 0 for c in crowd_columns) and sum(counts[c] for c in crowd_columns) == 8192
        if case.name == "one chain" and kind == "columns":
            assert max(counts.values()) == 70
            # the sums of the long columns depend on the order of their points
            reds = {}
            for v, c in zip(case.batches[0], case.colors[0]):
                reds.setdefault((int(v[1]), int(v[2])), []).append(c[0])
            differ = 0
            for column, values in reds.items():
                if len(values) >= 32:
                    forward = backward = vt.f32(0)
                    for r in values:
                        forward = vt.f32(forward + r)
                    for r in values[::-1]:
                        backward = vt.f32(backward + r)
                    differ += forward.tobytes() != backward.tobytes()
            assert differ >= 5, differ
