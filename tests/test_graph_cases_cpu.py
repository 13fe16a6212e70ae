"""The clouds of tests/_graph_cases.py have the structure their names claim
(no GPU): candidate totals, box sizes, shared buckets, alternating slots,
cube levels -- by the NumPy restatement of the device's bucket function -- and
the three CPU forms of the radius predicate agree on them, the reference's own
scikit-learn call included (the inclusive edge at exactly r is the point)."""
import numpy as np
import pytest

import _graph_cases as GC
from oracle import graph_oracle as go


def _set(e):
    return go.canonical_edges(e)


def test_hash_bits_floor_and_steps():
    assert GC.hash_bits(1) == 10 and GC.hash_bits(512) == 10
    assert GC.hash_bits(513) == 11
    assert GC.hash_bits(32768) == 16 and GC.hash_bits(32769) == 17
    assert GC.hash_bits(10 ** 9) == 22


def test_chunk_sweep_candidate_totals():
    case, ms = GC.chunk_sweep()
    grid = GC.RadiusGrid(case.points, case.r)
    n_cells, totals = grid.profile(case.centers)
    assert np.all(n_cells == 27)
    assert np.array_equal(totals, ms)          # candidate total = m exactly
    want = set(range(1, 201)) | {255, 256, 257}
    assert set(totals[0::2].tolist()) == want and \
        set(totals[1::2].tolist()) == want
    for seam in (63, 64, 65, 127, 128, 129, 191, 192, 193):
        assert seam in totals
    assert len(np.unique(case.points, axis=0)) == len(case.points)
    # mid-cell centres: every candidate is a neighbour; corner centres: about
    # a third of the candidates are not
    ref = go.radius_graph_c(case.points, case.centers, case.r)
    deg = np.bincount(ref[:, 1], minlength=len(case.centers))
    assert np.array_equal(deg[0::2], ms[0::2])
    big = ms[1::2] >= 60
    frac = 1.0 - deg[1::2][big] / ms[1::2][big].astype(np.float64)
    assert 0.2 < frac.mean() < 0.45 and frac.min() > 0.1
    # and around every seam both kinds of candidate occur
    assert np.all(deg[1::2][big] < ms[1::2][big])


def test_lattices_box_sizes_and_exact_r():
    sizes = set()
    for case in GC.lattices():
        grid = GC.RadiusGrid(case.points, case.r, case.scale)
        n_cells, totals = grid.profile(case.centers)
        assert n_cells.max() <= 64
        exact = GC.exact_r_pairs(case.points, case.centers, case.r, case.scale)
        if case.name.startswith("lattice8_r1"):
            assert np.all(n_cells == 64), case.name
            # 6 neighbours at exactly r per interior direction
            assert exact == 2 * 3 * 8 * 8 * 7
        if case.name.startswith("lattice12_r5"):
            assert set(n_cells.tolist()) == {27, 36, 48, 64}, case.name
            assert exact > 0 and totals.min() >= 64 and totals.max() > 1024
            sizes |= set(n_cells.tolist())
        if case.name.startswith("lattice12_scaled"):
            assert exact > 0, case.name
        if "tenth" not in case.name:
            assert exact > 0, case.name
    assert sizes == {27, 36, 48, 64}


def test_lattice_forms_share_one_graph():
    """the float32, float64 and shifted forms of an integer lattice are the
    same graph"""
    by = {c.name: c for c in GC.lattices()}
    ref = {n: go.radius_graph_c(c.points, c.centers, c.r, c.scale)
           for n, c in by.items()}
    for stem in ("lattice8_r1", "lattice12_r5", "lattice12_scaled"):
        assert np.array_equal(ref[stem + "_f32"], ref[stem + "_f64"])
    assert np.array_equal(ref["lattice12_r5_f32"], ref["lattice12_r5_negative_f32"])
    assert np.array_equal(ref["lattice8_r1_f64"], ref["lattice8_r1_negative_f64"])


def test_shared_bucket_box_structure():
    case, info = GC.shared_bucket_box()
    assert len(case.points) <= 400 and GC.hash_bits(len(case.points)) == 10
    grid = GC.RadiusGrid(case.points, case.r)
    ref = go.radius_graph_c(case.points, case.centers, case.r)
    for q, rec in enumerate(info):
        n_cells, total, buckets = grid.query(case.centers[q])
        assert n_cells == 27
        cells = GC.box_cells(case.centers[q].astype(np.float64), case.r)
        ia = np.flatnonzero((cells == rec["a"]).all(1))
        ib = np.flatnonzero((cells == rec["b"]).all(1))
        assert len(ia) == 1 and len(ib) == 1 and ia[0] != ib[0]
        assert buckets[ia[0]] == buckets[ib[0]] == rec["bucket"]
        nbrs = set(ref[ref[:, 1] == q, 0].tolist())
        # true neighbours in both cells, each in the cell it is named for
        for idx, cell in ((rec["idx_a"], rec["a"]), (rec["idx_b"], rec["b"])):
            assert set(idx) <= nbrs
            assert np.all(grid.cells[idx] == cell)
            assert np.all(grid.bucket[idx] == rec["bucket"])
        # the far point: same bucket, another cell, not a neighbour, between
        # the first A and the first B in index order
        f = rec["idx_far"]
        assert grid.bucket[f] == rec["bucket"] and f not in nbrs
        assert np.all(grid.cells[f] == rec["far"])
        assert np.abs(rec["far"] - rec["a"]).max() >= 4
        assert rec["idx_a"][0] < f < rec["idx_b"][0]
        # the bucket's slice is walked twice
        assert total >= 2 * 7


def test_sort_scan_edges_sizes():
    cases = {c.name: c for c in GC.sort_scan_edges()}
    assert [len(cases["points%d" % n].points) for n in GC.SORT_POINTS] == \
        list(GC.SORT_POINTS)
    assert [len(cases["centers%d" % q].centers) for q in GC.SCAN_CENTERS] == \
        list(GC.SCAN_CENTERS)
    for c in cases.values():
        assert len(c.points) * len(c.centers) < 3e8
    # sparse, not empty: a few neighbours per centre
    c = cases["points2049"]
    deg = np.bincount(go.radius_graph_c(c.points, c.centers, c.r)[:, 1],
                      minlength=len(c.centers))
    assert 1.0 < deg.mean() < 8.0


def test_fanin_caps_fan_in():
    case, where, caps = GC.fanin_caps()
    ref = go.radius_graph_c(case.points, case.centers, case.r)
    deg = np.bincount(ref[:, 1], minlength=len(case.centers))
    assert set(where) == {63, 64, 65, 128, 129}
    for f, q in where.items():
        assert deg[q] == f
    assert caps == (1, 63, 64, 65)


def test_voxel_bucket_pairs_share_and_alternate():
    points, pairs = GC.voxel_bucket_pairs()
    vi, origin = GC.vox_index(points, GC.VOXEL)
    assert np.all(origin == -0.5)
    mask = (1 << GC.hash_bits(len(points))) - 1
    bucket = GC.cell_hash(vi, mask)
    # the 'random' grids give the same indices (graph_gen.py:121-129)
    off = np.asarray([np.amin(points, axis=0)])
    assert np.array_equal(((points - off) // GC.VOXEL).astype(np.int64), vi)
    jit = GC.VOXEL * np.asarray([GC.JITTER])
    assert np.array_equal(((points - off + jit) // GC.VOXEL).astype(np.int64), vi)
    counts = set()
    for rec in pairs:
        i1, i2 = rec["idx1"], rec["idx2"]
        assert np.all(vi[i1] == rec["v1"]) and np.all(vi[i2] == rec["v2"])
        assert not np.array_equal(rec["v1"], rec["v2"])
        b = bucket[i1[0]]
        assert np.all(bucket[i1 + i2] == b)
        assert np.array_equal(np.flatnonzero(bucket == b), np.sort(i1 + i2))
        merged = sorted([(i, 1) for i in i1] + [(i, 2) for i in i2])
        who = [w for _, w in merged]
        assert who[0] == 1                     # V1 leads the bucket
        lead = 5 if rec["late"] else 0
        assert who[:lead] == [1] * lead
        k = min(len(i1) - lead, len(i2))
        assert who[lead:lead + 2 * k] == [1, 2] * k
        if rec["late"]:
            assert who.index(2) >= 5
        counts.add((len(i1), len(i2), rec["late"]))
    assert {(a, b, False) for a in range(1, 10) for b in range(1, 10)} <= counts
    assert {(a, b, True) for a in range(6, 10) for b in range(1, 10)} <= counts


def test_nn_face_and_tie_clouds():
    p = GC.nn_face_cloud()
    vi, _ = GC.vox_index(p, GC.VOXEL)
    assert vi.tolist() == [[0, 0, 0], [2, 2, 2], [2, 2, 2], [3, 2, 2]]
    _, idx = go.keypoints_center(p, p, GC.VOXEL)
    assert sorted(idx[:, 0].tolist()) == [0, 3, 3]   # (2,2,2) takes point 3
    p = GC.nn_tie_cloud()
    vi, _ = GC.vox_index(p, GC.VOXEL)
    assert vi.tolist() == [[0, 0, 0], [4, 4, 4], [4, 4, 4], [5, 4, 4], [3, 4, 4]]
    c = p[1:3].astype(np.float64).mean(0)
    d = ((p.astype(np.float64) - c) ** 2).sum(1)
    assert d[3] == d[4] and d[3] < d[1] and d[3] < d[2]   # the exact tie


@pytest.mark.parametrize("sign", [1, -1])
def test_nn_corner_cloud(sign):
    p = GC.nn_corner_cloud(sign)
    vi, _ = GC.vox_index(p, GC.VOXEL)
    assert vi[1:4].tolist() == [[4, 4, 4]] * 3
    assert vi[4].tolist() == [4 + sign] * 3          # the corner voxel
    # (dz, dy, dx) order: (+1,+1,+1) is lane 26, (-1,-1,-1) lane 0
    assert (vi[4] - vi[1] + 1) @ np.array([1, 3, 9]) == (26 if sign > 0 else 0)
    _, idx = go.keypoints_center(p, p, GC.VOXEL)
    assert sorted(idx[:, 0].tolist()) == [0, 4, 4]


def test_nn_neighbourhood_totals():
    for total in GC.NN_TOTALS:
        p, v = GC.nn_neighbourhood_cloud(total)
        vi, _ = GC.vox_index(p, GC.VOXEL)
        mask = (1 << GC.hash_bits(len(p))) - 1
        size = np.bincount(GC.cell_hash(vi, mask), minlength=mask + 1)
        nb = np.stack(np.meshgrid(*[np.arange(-1, 2)] * 3, indexing="ij"),
                      -1).reshape(-1, 3)
        b = GC.cell_hash(v + nb, mask)
        assert len(set(b.tolist())) == 27
        assert int(size[b].sum()) == total
        assert np.all(size[b] >= 1)
        assert np.all(np.abs(vi[1:] - v).max(1) <= 1)


def test_nn_from_levels_and_face_bound():
    points, base, names = GC.nn_from_cloud()
    b64 = base.astype(np.float64)
    got = {}
    for i, name in enumerate(names):
        level, best = GC.from_level(points, base, GC.VOXEL, i)
        got[name] = level
        # the stop test is sound: the point found at that level is the
        # brute-force nearest of ALL base points
        d2 = ((b64 - points[i].astype(np.float64)) ** 2).sum(1)
        assert d2[best] == d2.min() and (d2 == d2.min()).sum() == 1, name
    for name, level in GC.FROM_WANT.items():
        assert got[name] == level, (name, got)
    # stopping at r = 1 would be wrong for corner_then_r2
    i = names.index("corner_then_r2")
    vc, origin = GC.vox_index(points, GC.VOXEL)
    vb = np.floor((b64 - origin) / GC.VOXEL).astype(np.int64)
    in1 = np.flatnonzero(np.all(np.abs(vb - vc[i]) <= 1, axis=1))
    assert len(in1) == 1 and in1[0] != GC.from_level(points, base, GC.VOXEL, i)[1]
    _, ref = go.keypoints_center(points, base, GC.VOXEL)
    assert len(ref) == len(points)


def _small_radius_cases():
    out = list(GC.lattices())
    out.append(GC.shared_bucket_box()[0])
    out.append([c for c in GC.sort_scan_edges() if c.name == "points2049"][0])
    return out


@pytest.mark.parametrize("case", _small_radius_cases(), ids=repr)
def test_three_cpu_forms_agree(case):
    """C restatement == NumPy brute force == the reference's scikit-learn call,
    as edge sets -- on clouds full of pairs at exactly r"""
    c = go.radius_graph_c(case.points, case.centers, case.r, case.scale)
    b = go.radius_graph_bruteforce(case.points, case.centers, case.r, case.scale)
    s = go.radius_graph_sklearn(case.points, case.centers, case.r,
                                scale=case.scale)
    assert np.array_equal(_set(c), _set(b))
    assert np.array_equal(_set(c), _set(s))


def test_chunk_sweep_cpu_forms_agree():
    case, _ = GC.chunk_sweep()
    c = go.radius_graph_c(case.points, case.centers, case.r)
    s = go.radius_graph_sklearn(case.points, case.centers, case.r)
    assert np.array_equal(_set(c), _set(s))
