"""The graph builder where its kernels branch, and on capped grids
(csrc/graph.hip, csrc/sort.hip, the launches of csrc/kdtree.hip).

The clouds come from tests/_graph_cases.py (tests/test_graph_cases_cpu.py
proves that each reaches the branch it is named for); every expected value
comes from oracle/graph_oracle.py and everything is compared with == on
integers.  Needs a real MI355X."""
import os
import random

import numpy as np
import pytest

import pointgnn_amd  # noqa: F401
import _graph_cases as GC
from _multilevel import BASE_VOXEL, LEVEL_CONFIGS
from oracle import graph_oracle as go

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from pointgnn_amd import _lib
    lib = _lib.load()            # raises if the HIP extension is missing
    t = torch.zeros(4, device="cuda")
    _lib.check(lib.pgnn_check_device_pointer(_lib.ptr(t)), "runtime binding")
    return torch.device("cuda")


def T(a, dev, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(dev)


# ----------------------------------------------------------------------------
# radius graph
# ----------------------------------------------------------------------------
_SWEEP = GC.chunk_sweep()
_SHARED = GC.shared_bucket_box()
RADIUS_CASES = [_SWEEP[0]] + GC.lattices() + [_SHARED[0]] + GC.sort_scan_edges()
_REF = {}


def _ref(case):
    """the oracle's edge set of a case, computed once and left unchanged"""
    if case.name not in _REF:
        r = go.radius_graph_c(case.points, case.centers, case.r, case.scale)
        r.setflags(write=False)
        _REF[case.name] = r
    return _REF[case.name]


def _has_capacity_form(case):
    return case.name == "chunk_sweep" or case.name.startswith("lattice")


def _check_radius(case, dtype, dev, tag):
    import torch
    from pointgnn_amd import _lib, graph_gen as G
    ref = _ref(case)
    n_c = len(case.centers)
    p, c = T(case.points.astype(dtype), dev), T(case.centers.astype(dtype), dev)
    edges, offsets = G.radius_graph_device(p, c, case.r, case.scale)
    e, off = edges.cpu().numpy(), offsets.cpu().numpy()
    what = "%s %s" % (case.name, tag)
    # no row twice (asked first: a double visit of a shared bucket shows here)
    got = go.canonical_edges(e)
    dup = got[1:][(np.diff(got, axis=0) == 0).all(1)]
    assert len(dup) == 0, "%s: %d duplicate rows, e.g. %s" % (
        what, len(dup), [tuple(r) for r in dup[:3]])
    # the edge set is the oracle's
    if got.shape != ref.shape or not np.array_equal(got, ref):
        gs, rs = set(map(tuple, got)), set(map(tuple, ref))
        missing, extra = sorted(rs - gs), sorted(gs - rs)
        per = sorted(set(q for _, q in missing + extra))
        raise AssertionError(
            "%s: %d edges vs %d; missing %s extra %s; first centres %s" % (
                what, len(got), len(ref), missing[:4], extra[:4], per[:6]))
    # offsets = cumulative degree; column 1 ascends and agrees with them
    deg = np.bincount(ref[:, 1], minlength=n_c)
    assert off.shape == (n_c + 1,)
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(deg)])), what
    assert np.all(np.diff(e[:, 1]) >= 0), what
    assert np.array_equal(e[:, 1], np.repeat(np.arange(n_c), np.diff(off))), what
    # the same array from a second call
    edges2, offsets2 = G.radius_graph_device(p, c, case.r, case.scale)
    assert torch.equal(edges, edges2) and torch.equal(offsets, offsets2), what
    if not _has_capacity_form(case):
        return
    # ... and from the capacity form: ~30 % tail rows behind the device-side
    # counts, copies of real rows (they would be neighbours if a kernel read
    # them)
    n_p = len(case.points)
    tp, tc = max(1, (3 * n_p) // 10), max(1, (3 * n_c) // 10)
    pcap = np.concatenate([case.points, case.points[:tp]]).astype(dtype)
    ccap = np.concatenate([case.centers, case.centers[:tc]]).astype(dtype)
    counts = torch.tensor([n_p, n_c, 0, 0], dtype=torch.int32, device=dev)
    pt = _lib.tag_count(T(pcap, dev), _lib.DeviceCount(counts[0:1], n_p))
    ct = _lib.tag_count(T(ccap, dev), _lib.DeviceCount(counts[1:2], n_c))
    cap = len(e) + 1000
    got = G.radius_graph_dyn_device(pt, ct, case.r, case.scale, cap, counts[2:4])
    assert counts[2:4].tolist() == [len(e), len(e)], what
    assert torch.equal(got[:len(e)], edges), what + ": capacity form differs"


def _dtypes(case):
    if case.points.dtype == np.float32:
        return ((np.float32, "float32 entry"), (np.float64, "_f64 entry"))
    return ((np.float64, "_f64 entry"),)


@pytest.mark.parametrize("case", RADIUS_CASES, ids=repr)
def test_radius_case(dev, case):
    """edge set == oracle, offsets == cumulative degree, grouped and ascending
    by centre, no duplicate row, identical on a second call and in the
    capacity form -- through the float32 and the _f64 entries."""
    for dtype, tag in _dtypes(case):
        _check_radius(case, dtype, dev, tag)


def test_radius_chunk_sweep_per_cluster(dev):
    """the sweep again, reported per cluster size: the degree of EVERY centre
    (candidate totals 1..200, 255..257) equals the oracle's"""
    from pointgnn_amd import graph_gen as G
    case, ms = _SWEEP
    ref = _ref(case)
    deg = np.bincount(ref[:, 1], minlength=len(case.centers))
    _, offsets = G.radius_graph_device(T(case.points, dev),
                                       T(case.centers, dev), case.r)
    got = np.diff(offsets.cpu().numpy())
    bad = np.flatnonzero(got != deg)
    assert bad.size == 0, "first wrong cluster sizes m = %s (degree %s vs %s)" % (
        ms[bad[:8]].tolist(), got[bad[:8]].tolist(), deg[bad[:8]].tolist())


def test_radius_shared_bucket_rows(dev):
    """each aimed centre of shared_bucket_box has its neighbours of BOTH cells
    once, and not the far point of their bucket"""
    from pointgnn_amd import graph_gen as G
    case, info = _SHARED
    edges, offsets = G.radius_graph_device(T(case.points, dev),
                                           T(case.centers, dev), case.r)
    e, off = edges.cpu().numpy(), offsets.cpu().numpy()
    for q, rec in enumerate(info):
        rows = e[off[q]:off[q + 1], 0].tolist()
        for i in rec["idx_a"] + rec["idx_b"]:
            assert rows.count(i) == 1, (q, i, rows)
        assert rec["idx_far"] not in rows


# ----------------------------------------------------------------------------
# fan-in cap
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("cap", GC.CAPS)
def test_fanin_cap_keeps_order(dev, cap):
    """cap_fill_kernel keeps edges in chunks of 64 and emits them 'in original
    order': each centre's capped rows are a SUBSEQUENCE of its uncapped rows,
    min(deg, cap) of them, and a centre with deg <= cap is copied verbatim --
    at fan-in 63 / 64 / 65 / 128 / 129 among all the others of the sweep."""
    from pointgnn_amd import graph_gen as G
    case, where, _ = GC.fanin_caps()
    p, c = T(case.points, dev), T(case.centers, dev)
    full, foff = G.radius_graph_device(p, c, case.r)
    full, foff = full.cpu().numpy(), foff.cpu().numpy()
    assert np.array_equal(go.canonical_edges(full), _ref(case))
    deg = np.diff(foff)
    for f, q in where.items():
        assert deg[q] == f
    pos_of = {(int(a), int(b)): i for i, (a, b) in enumerate(full)}
    for seed in (7, 8):
        e, off = G.radius_graph_device(p, c, case.r, None, cap, seed)
        e, off = e.cpu().numpy(), off.cpu().numpy()
        assert np.array_equal(np.diff(off), np.minimum(deg, cap)), (cap, seed)
        assert np.array_equal(e[:, 1], np.repeat(np.arange(len(deg)),
                                                 np.diff(off)))
        pos = np.array([pos_of.get((int(a), int(b)), -1) for a, b in e])
        assert np.all(pos >= 0), "a capped row is not an uncapped row"
        # strictly ascending positions: a subsequence, centre by centre
        bad = np.flatnonzero(np.diff(pos) <= 0)
        assert bad.size == 0, "cap %d seed %d: order broken at centres %s" % (
            cap, seed, sorted(set(e[bad + 1, 1].tolist()))[:6])
        for q in np.flatnonzero(deg <= cap):
            assert np.array_equal(e[off[q]:off[q + 1]],
                                  full[foff[q]:foff[q + 1]]), (cap, seed, q)


# ----------------------------------------------------------------------------
# keypoints
# ----------------------------------------------------------------------------
_PAIRS = GC.voxel_bucket_pairs()


def _center_equal(dev, points, voxel, base=None):
    from pointgnn_amd import graph_gen as G
    if base is None:
        xyz, idx = G.keypoints_device(T(points, dev), voxel, 'center')
        src = points
    else:
        xyz, idx = G.keypoints_device(T(points, dev), voxel, 'center',
                                      base=T(base, dev))
        src = base
    _, ref = go.keypoints_center(points, src, voxel)
    idx = idx.cpu().numpy()
    assert idx.shape == ref.shape, "K %s vs %s voxels" % (idx.shape, ref.shape)
    # voxel order is the device's hash order: compare as multisets (the form
    # test_center_keypoints uses, exact under ties)
    assert np.array_equal(np.sort(idx[:, 0]), np.sort(ref[:, 0]))
    assert np.array_equal(xyz.cpu().numpy(), src[idx[:, 0]])
    return idx[:, 0]


def test_center_keypoints_voxels_sharing_buckets(dev):
    """voxel_leader_kernel where two voxels share a bucket: the second one's
    leader is found by the walk, the member loop drops the other voxel's
    slots by value, 1..9 members each (4-wide loop and tail)."""
    points, pairs = _PAIRS
    got = _center_equal(dev, points, GC.VOXEL)
    assert len(got) == 1 + 2 * len(pairs)
    # ... and as the search set of a second level (a grid of its own)
    _center_equal(dev, points, GC.VOXEL, base=points[::2].copy())


@pytest.mark.parametrize("name", ["face", "tie", "corner_hi", "corner_lo",
                                  "n63", "n64", "n65", "n129"])
def test_center_keypoints_nn_cases(dev, name):
    """voxel_nn_kernel: the nearest point across a face, an exact tie across
    voxels, the nearest point in the last / first of the 27 voxels, and
    63 / 64 / 65 / 129 candidates in them"""
    if name == "face":
        points = GC.nn_face_cloud()
    elif name == "tie":
        points = GC.nn_tie_cloud()
    elif name.startswith("corner"):
        points = GC.nn_corner_cloud(1 if name == "corner_hi" else -1)
    else:
        points, _ = GC.nn_neighbourhood_cloud(int(name[1:]))
    got = _center_equal(dev, points, GC.VOXEL)
    if name == "face":
        assert sorted(got.tolist()) == [0, 3, 3]
    if name.startswith("corner"):
        assert sorted(got.tolist()) == [0, 4, 4]
    _center_equal(dev, points, GC.VOXEL, base=points[::2].copy())


def test_center_keypoints_from_levels(dev):
    """voxel_nn_from_kernel: centroids decided at r = 1, 2, 3 and by the
    every-point pass in ONE call, and one where stopping at r = 1 would take
    the wrong point"""
    points, base, names = GC.nn_from_cloud()
    _center_equal(dev, points, GC.VOXEL, base=base)
    from pointgnn_amd import graph_gen as G
    _, idx = G.keypoints_device(T(points, dev), GC.VOXEL, 'center',
                                base=T(base, dev))
    want = sorted(GC.from_level(points, base, GC.VOXEL, i)[1]
                  for i in range(len(points)))
    _, ref = go.keypoints_center(points, base, GC.VOXEL)
    assert sorted(ref[:, 0].tolist()) == want      # (restatement == oracle)
    assert sorted(idx.cpu().numpy()[:, 0].tolist()) == want


def _oracle_voxels(points, jitter):
    """voxel index of every point by the arithmetic of graph_gen.py:121-129
    (the lines oracle.keypoints_random runs)"""
    off = np.asarray([np.amin(points, axis=0)])
    if jitter is None:
        ijk = (points - off) // GC.VOXEL
    else:
        ijk = (points - off + GC.VOXEL * np.asarray([jitter])) // GC.VOXEL
    return ijk.astype(np.int32)


def _oracle_k(points, jitter):
    off = np.asarray([np.amin(points, axis=0)])
    np.random.seed(GC.JITTER_SEED)      # the oracle draws the jitter itself
    random.seed(0)
    return len(go.keypoints_random(points, off, GC.VOXEL,
                                   add_rnd3d=jitter is not None)[1])


def _random_clouds():
    out = {"pairs": _PAIRS[0], "face": GC.nn_face_cloud(),
           "tie": GC.nn_tie_cloud(), "corner": GC.nn_corner_cloud(1)}
    for t in GC.NN_TOTALS:
        out["n%d" % t] = GC.nn_neighbourhood_cloud(t)[0]
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("jitter", [None, GC.JITTER], ids=["plain", "jitter"])
def test_random_keypoints_cases(dev, dtype, jitter):
    """'random' keypoints: K is the oracle's voxel count and each pick is a
    member of a distinct oracle voxel -- on the shared-bucket voxels and the
    nearest-neighbour clouds"""
    from pointgnn_amd import graph_gen as G
    for name, pts in _random_clouds().items():
        pts = pts.astype(dtype)
        vox = _oracle_voxels(pts, jitter)
        k_ref = _oracle_k(pts, jitter)
        assert k_ref == len(np.unique(vox, axis=0))
        jit = None if jitter is None else GC.VOXEL * np.asarray(jitter)
        for seed in (1, 2, 3):
            xyz, idx = G.keypoints_device(T(pts, dev), GC.VOXEL, 'random',
                                          jitter=jit, seed=seed)
            idx = idx.cpu().numpy()[:, 0]
            assert len(idx) == k_ref, (name, seed)
            assert idx.min() >= 0 and idx.max() < len(pts)
            assert len(np.unique(vox[idx], axis=0)) == k_ref, (name, seed)
            assert np.array_equal(xyz.cpu().numpy(), pts[idx])


def test_random_keypoints_cover_a_shared_bucket(dev):
    """voxel_random_pick_kernel over 40 seeds: in the pair of 9-member voxels
    that share a bucket every member is picked at least once, and the pick of
    a voxel is never a member of the other one"""
    from pointgnn_amd import graph_gen as G
    points, pairs = _PAIRS
    rec = [r for r in pairs if len(r["idx1"]) == 9 and len(r["idx2"]) == 9
           and not r["late"]][0]
    vox = _oracle_voxels(points, None)
    owner = {}
    for r in pairs:
        owner[tuple(r["v1"])] = set(r["idx1"])
        owner[tuple(r["v2"])] = set(r["idx2"])
    seen = {tuple(rec["v1"]): set(), tuple(rec["v2"]): set()}
    p = T(points, dev)
    for seed in range(40):
        _, idx = G.keypoints_device(p, GC.VOXEL, 'random', seed=seed)
        idx = idx.cpu().numpy()[:, 0]
        assert len(idx) == 1 + 2 * len(pairs)
        for i in idx:
            v = tuple(vox[i])
            if v in owner:
                assert int(i) in owner[v]      # never the other voxel's
            if v in seen:
                seen[v].add(int(i))
    print("picked members over 40 seeds: V1 %d of 9, V2 %d of 9" % (
        len(seen[tuple(rec["v1"])]), len(seen[tuple(rec["v2"])])))
    assert seen[tuple(rec["v1"])] == set(rec["idx1"])
    assert seen[tuple(rec["v2"])] == set(rec["idx2"])


# ----------------------------------------------------------------------------
# capped grids
# ----------------------------------------------------------------------------
def _env_tunable(key):
    for kv in filter(None, os.environ.get("PGNN_TUNE", "").split(",")):
        k, v = kv.split("=")
        if k.strip() == key:
            return int(v)
    return 0


class _capped(object):
    """graph_max_wgs / graph_lds_pad for the duration of a block (the module
    cannot configure the session; it sets and restores the tunables itself)"""

    def __init__(self, max_wgs, lds_pad):
        self.v = (max_wgs, lds_pad)

    def __enter__(self):
        from pointgnn_amd import _lib
        _lib.set_tunable("graph_max_wgs", self.v[0])
        _lib.set_tunable("graph_lds_pad", self.v[1])

    def __exit__(self, *exc):
        from pointgnn_amd import _lib
        _lib.set_tunable("graph_max_wgs", _env_tunable("graph_max_wgs"))
        _lib.set_tunable("graph_lds_pad", _env_tunable("graph_lds_pad"))


N_CLOUD, N_CENTERS = 6000, 4500
SCALE = [1.0, 2.0, 0.5]


def _cloud():
    rng = np.random.default_rng(11)
    xyz = rng.uniform(0.0, 12.0, (N_CLOUD, 3)).astype(np.float32)
    wide = xyz.astype(np.float64) + rng.uniform(0, 1e-6, xyz.shape)
    return xyz, wide


def _surface(dev):
    """every builder entry on one cloud -> {name: numpy array}.  6000 points
    and 4500 centres: 3 sort tiles, 2 scan tiles, more than 16 centres per
    1024-thread block, more than 1024 sorted slots, kd-tree top levels."""
    import torch
    from pointgnn_amd import graph_gen as G
    xyz, wide = _cloud()
    out = {}

    def put(name, *ts):
        for k, t in enumerate(ts):
            out["%s.%d" % (name, k)] = t.cpu().numpy() if isinstance(
                t, torch.Tensor) else np.asarray(t)
    p32, c32 = T(xyz, dev), T(xyz[:N_CENTERS], dev)
    p64, c64 = T(wide, dev), T(wide[:N_CENTERS], dev)
    put("radius_f32", *G.radius_graph_device(p32, c32, 1.0))
    put("radius_f32_scale", *G.radius_graph_device(p32, c32, 1.0, SCALE))
    put("radius_f64", *G.radius_graph_device(p64, c64, 1.0))
    put("radius_f64_scale", *G.radius_graph_device(p64, c64, 1.0, SCALE))
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    dyn = G.radius_graph_dyn_device(p32, c32, 1.0, None, 200000, counts)
    n = counts.tolist()
    assert n[0] == n[1] < 200000
    put("radius_dyn", dyn[:n[0]], counts)
    put("kp_center", *G.keypoints_device(p32, 0.8, 'center'))
    put("kp_random_f32", *G.keypoints_device(p32, 0.8, 'random', seed=5))
    put("kp_random_f32_jit", *G.keypoints_device(
        p32, 0.8, 'random', jitter=[0.1, 0.5, 0.7], seed=5))
    put("kp_random_f64", *G.keypoints_device(p64, 0.8, 'random', seed=5))
    base = T(xyz[::3].copy(), dev)
    put("kp_center_base", *G.keypoints_device(p32, 2.0, 'center', base=base))
    put("kp_random_base", *G.keypoints_device(p32, 2.0, 'random', seed=6,
                                              base=base))
    idx, bounds, status = G.kdtree_replica(p32)
    put("kdtree", idx, bounds, [status])
    for method in ('center', 'random'):
        np.random.seed(3)
        coords, kps, edges = G.gen_multi_level_local_graph_v3(
            p32, BASE_VOXEL, LEVEL_CONFIGS, downsample_method=method)
        put("multi_%s_coords" % method, *coords)
        put("multi_%s_kps" % method, *kps)
        put("multi_%s_edges" % method, *edges)
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def uncapped(dev):
    with _capped(0, 0):
        return _surface(dev)


def test_uncapped_surface_equals_oracle(dev, uncapped):
    """the run the capped ones are compared with is itself the oracle's"""
    from sklearn.neighbors import KDTree
    u = uncapped
    xyz, wide = _cloud()
    for name, pts, scale in (("radius_f32", xyz, None),
                             ("radius_f32_scale", xyz, SCALE),
                             ("radius_f64", wide, None),
                             ("radius_f64_scale", wide, SCALE),
                             ("radius_dyn", xyz, None)):
        ref = go.radius_graph_c(pts, pts[:N_CENTERS], 1.0, scale)
        assert np.array_equal(go.canonical_edges(u[name + ".0"]), ref), name
        if name != "radius_dyn":
            deg = np.bincount(ref[:, 1], minlength=N_CENTERS)
            assert np.array_equal(u[name + ".1"],
                                  np.concatenate([[0], np.cumsum(deg)]))
    assert np.array_equal(u["radius_dyn.0"], u["radius_f32.0"])
    _, ref = go.keypoints_center(xyz, xyz, 0.8)
    assert np.array_equal(np.sort(u["kp_center.1"][:, 0]), np.sort(ref[:, 0]))
    assert np.array_equal(u["kp_center.0"], xyz[u["kp_center.1"][:, 0]])
    base = xyz[::3]
    _, ref = go.keypoints_center(xyz, base, 2.0)
    assert np.array_equal(np.sort(u["kp_center_base.1"][:, 0]),
                          np.sort(ref[:, 0]))
    off = np.asarray([np.amin(xyz, axis=0)])
    for name, pts, src, voxel, jit in (
            ("kp_random_f32", xyz, xyz, 0.8, None),
            ("kp_random_f32_jit", xyz, xyz, 0.8, [0.1, 0.5, 0.7]),
            ("kp_random_f64", wide, wide, 0.8, None),
            ("kp_random_base", xyz, base, 2.0, None)):
        o = np.asarray([np.amin(pts, axis=0)])
        q = (src - o) if jit is None else (src - o + np.asarray([jit]))
        vox = (q // voxel).astype(np.int32)
        idx = u[name + ".1"][:, 0]
        assert len(idx) == len(np.unique(vox, axis=0)) == \
            len(np.unique(vox[idx], axis=0)), name
        assert np.array_equal(u[name + ".0"], src[idx]), name
    _, idx_ref, node_data, node_bounds = KDTree(
        xyz.astype(np.float64), leaf_size=30).get_arrays()
    assert u["kdtree.2"][0] == 0
    assert np.array_equal(u["kdtree.0"], idx_ref)
    assert np.array_equal(u["kdtree.1"][:, :3], node_bounds[0])
    assert np.array_equal(u["kdtree.1"][:, 3:], node_bounds[1])
    for method in ('center', 'random'):
        coords = [u["multi_%s_coords.%d" % (method, k)] for k in range(4)]
        assert np.array_equal(coords[0], xyz)
        for l, cfg in enumerate(LEVEL_CONFIGS):
            lvl = cfg['graph_level']
            ref = go.radius_graph_c(coords[lvl], coords[lvl + 1],
                                    cfg['graph_gen_kwargs']['radius'])
            assert np.array_equal(
                go.canonical_edges(u["multi_%s_edges.%d" % (method, l)]),
                ref), (method, l)
            kp = u["multi_%s_kps.%d" % (method, l)][:, 0]
            assert np.array_equal(coords[l + 1], coords[l][kp]), (method, l)
    _, ref = go.keypoints_center(xyz, xyz, BASE_VOXEL)
    assert np.array_equal(np.sort(u["multi_center_kps.0"][:, 0]),
                          np.sort(ref[:, 0]))


@pytest.mark.parametrize("max_wgs,lds_pad", [(1, 0), (3, 0), (8, 32768)])
def test_capped_grids_are_byte_identical(dev, uncapped, max_wgs, lds_pad):
    """pgnn_set_tunable("graph_max_wgs") caps every builder launch and makes
    every kernel stride over its work (sort tiles, scan tiles, kd-tree levels
    and subtrees, centres, sorted slots; 1024-thread blocks; spw = 64): every
    array the builder returns is byte-identical to the uncapped run --
    include/pointgnn_hip.h, "leaves results bit-identical (tested)"."""
    with _capped(max_wgs, lds_pad):
        got = _surface(dev)
    assert sorted(got) == sorted(uncapped)
    for name in sorted(uncapped):
        a, b = got[name], uncapped[name]
        assert a.dtype == b.dtype and a.shape == b.shape, name
        assert a.tobytes() == b.tobytes(), "%s differs under graph_max_wgs=%d" \
            % (name, max_wgs)


def test_zz_tunables_are_back_at_zero(dev):
    """the last test of the module: with the tunables at 0 a small radius
    graph is the oracle's"""
    from pointgnn_amd import _lib, graph_gen as G
    _lib.set_tunable("graph_max_wgs", _env_tunable("graph_max_wgs"))
    _lib.set_tunable("graph_lds_pad", _env_tunable("graph_lds_pad"))
    case = [c for c in RADIUS_CASES if c.name == "lattice8_r1_f32"][0]
    fresh = go.radius_graph_c(case.points, case.centers, case.r)
    edges, _ = G.radius_graph_device(T(case.points, dev), T(case.centers, dev),
                                     case.r)
    assert np.array_equal(go.canonical_edges(edges.cpu().numpy()), fresh)
