"""The farthest-point sampling restatement of tests/_fps_cases.py is the
reference's own function, every cloud reaches what it is named for, and the
host logic of the feature (argument checks, the num_keypoints forms, the C
entries' validation before any HIP call).  No GPU."""
import ctypes
import os

import numpy as np
import pytest

import pointgnn_amd  # noqa: F401

import _fps_cases as FC

ENTRIES = ("pgnn_farthest_first_workspace_bytes", "pgnn_farthest_first",
           "pgnn_farthest_first_f64")
CASES = FC.all_cases()
BY_NAME = {c.name: c for c in CASES}


# ---- the restatement is the reference's function ----------------------------
@pytest.fixture(scope="module")
def ref_dataset():
    mod = FC.reference_kitti_dataset()
    if mod is None:
        pytest.skip("the reference is not on this machine")
    return object.__new__(mod.KittiDataset)   # farthest_first needs no state


@pytest.mark.parametrize("dtype", FC.DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name", ["n1", "n65", "block+1", "lattice",
                                  "duplicated", "all_equal", "untied",
                                  "winners", "kN+3"])
def test_restatement_equals_the_reference(ref_dataset, name, dtype):
    case = BY_NAME[name]
    pts = case.cast(dtype)
    for seed in (0, 1, 2):
        np.random.seed(seed)
        want = ref_dataset.farthest_first(pts, case.k)
        np.random.seed(seed)
        start = np.random.randint(len(pts))
        idx, _ = FC.fps_reference(pts, case.k, start)
        got = pts[idx].astype(np.float64)
        assert want.dtype == np.float64 and want.shape == (case.k, 3)
        assert np.array_equal(got, want)
        # the draw is the only one: the global stream is where the
        # reference left it
        after = np.random.randint(1 << 30)
        np.random.seed(seed)
        ref_dataset.farthest_first(pts, case.k)
        assert np.random.randint(1 << 30) == after


@pytest.mark.parametrize("dtype", FC.DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("order", ["C", "F"])
def test_row_sum_equals_the_parenthesised_form(ref_dataset, dtype, order):
    pts = np.asarray(FC.blob(3000, 5).astype(dtype), order=order)
    p0 = np.zeros(3)
    p0[:] = pts[17]
    want = ref_dataset.calc_distances(p0, pts)
    assert np.array_equal(FC.dist(p0, pts.astype(np.float64)), want)


# ---- the cases reach what they are named for ----------------------------------
def test_sizes_sit_on_the_seams():
    n = {c.name: c.n for c in CASES}
    assert [n["n%d" % i] for i in (1, 2, 63, 64, 65)] == [1, 2, 63, 64, 65]
    assert [n["block%+d" % i] for i in (-1, 0, 1)] == \
        [FC.BLOCK - 1, FC.BLOCK, FC.BLOCK + 1]
    assert [n["res32%+d" % i] for i in (-1, 0, 1)] == \
        [FC.RES32 - 1, FC.RES32, FC.RES32 + 1]
    assert [n["res64%+d" % i] for i in (-1, 0, 1)] == \
        [FC.RES64 - 1, FC.RES64, FC.RES64 + 1]
    assert FC.RES64 <= FC.RES32 and FC.RES32 % FC.BLOCK == 0 and \
        FC.RES64 % FC.BLOCK == 0 and FC.BLOCK % 64 == 0
    # the benchmark frame's cloud is resident
    from pointgnn_amd.synthetic import CLOUD_PRESETS
    assert CLOUD_PRESETS["car_600k"]["n_points"] <= FC.RES32
    # streaming for both dtypes, a few times the limit, K <= 64
    s = BY_NAME["streaming"]
    assert 3 * FC.RES32 < s.n < 4 * FC.RES32 and s.k <= 64
    assert all(c.k <= FC.K_MAX for c in CASES)
    # more than one stride, and a tail past the last full one
    w = BY_NAME["winners"]
    assert w.n > 3 * FC.BLOCK and w.n % FC.BLOCK != 0


def test_k_and_start_forms():
    for name, k in (("k1", 1), ("kN", 65), ("kN+3", 68)):
        assert BY_NAME[name].k == k and BY_NAME[name].n == 65
    for n in (1, 2, 63, 64, 65):
        assert BY_NAME["n%d" % n].k == n + 3
    c = BY_NAME["start_first"]
    assert (c.start, BY_NAME["start_last"].start,
            BY_NAME["start_middle"].start) == (0, c.n - 1, c.n // 2)


@pytest.mark.parametrize("dtype", FC.DTYPES, ids=["f32", "f64"])
def test_k_beyond_n_repeats_index_zero(dtype):
    for name in ("n1", "n2", "n65", "kN+3"):
        case = BY_NAME[name]
        idx, nd, _ = FC.reference_of(name, dtype)
        assert nd == case.n < case.k
        assert sorted(idx[:nd].tolist()) == list(range(case.n))
        assert (idx[nd:] == 0).all()


@pytest.mark.parametrize("dtype", FC.DTYPES, ids=["f32", "f64"])
def test_tie_cases_have_ties_and_the_untied_one_has_none(dtype):
    _, nd, mult = FC.reference_of("lattice", dtype)
    assert nd == BY_NAME["lattice"].k
    tied = sum(m >= 2 for m in mult)
    assert tied > len(mult) // 2, (tied, len(mult))
    idx, nd, mult = FC.reference_of("duplicated", dtype)
    assert nd == 100 < BY_NAME["duplicated"].k
    assert all(m >= 2 for m in mult[:nd - 1])
    # of two coincident rows the smaller index is the pick
    assert (idx[1:nd] % 2 == 0).all() and (idx[nd:] == 0).all()
    idx, nd, mult = FC.reference_of("all_equal", dtype)
    assert nd == 1 < BY_NAME["all_equal"].k
    assert idx[0] == 77 and (idx[1:] == 0).all()
    _, nd, mult = FC.reference_of("untied", dtype)
    assert nd == BY_NAME["untied"].k and set(mult) == {1}


@pytest.mark.parametrize("dtype", FC.DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name", ["winners", "streaming"])
def test_winners_sit_where_they_were_put(name, dtype):
    case = BY_NAME[name]
    idx, nd, _ = FC.reference_of(name, dtype)
    assert nd == case.k
    for rnd, i in case.expect.items():
        assert idx[rnd] == i, (rnd, i, idx[:8])
    lanes = {i % 64 for i in case.expect.values()}
    waves = {i % FC.BLOCK // 64 for i in case.expect.values()}
    assert 63 in lanes and FC.BLOCK // 64 - 1 in waves
    tail = case.n // FC.BLOCK * FC.BLOCK
    assert any(i >= tail for i in case.expect.values())


def test_segments_are_the_five_kinds():
    pts, off, st = FC.segmented()
    sizes = np.diff(off)
    assert len(sizes) == 5 and off[-1] == len(pts)
    assert sizes[0] == 0 and sizes[1] == 1 and 1 < sizes[2] < 64
    assert FC.BLOCK < sizes[3] <= FC.RES64 and sizes[4] > FC.RES32
    assert ((st >= 0) & ((st < sizes) | (sizes == 0))).all()
    assert FC.SEG_K <= 64


# ---- host logic -------------------------------------------------------------
def test_segment_starts_checks_and_draws():
    from pointgnn_amd import sampling
    sizes = [0, 1, 40, 700]
    assert sampling.segment_starts(sizes, [0, 0, 39, 5]).tolist() == \
        [0, 0, 39, 5]
    assert sampling.segment_starts(sizes, [0, 0, 39, 5]).dtype == np.int32
    for bad in ([0, 1, 0, 0], [0, 0, 40, 0], [0, 0, 0, -1], [0, 0, 0]):
        with pytest.raises(ValueError):
            sampling.segment_starts(sizes, bad)
    with pytest.raises(ValueError):
        sampling.segment_starts(sizes, [0.0, 0.0, 1.0, 2.0])
    # None: one draw per non-empty segment, in segment order
    np.random.seed(3)
    got = sampling.segment_starts(sizes)
    after = np.random.randint(1 << 30)
    np.random.seed(3)
    want = [0] + [np.random.randint(n) for n in sizes[1:]]
    assert got.tolist() == want and np.random.randint(1 << 30) == after


def test_segment_sizes_checks():
    from pointgnn_amd import sampling
    assert sampling.segment_sizes([0, 0, 3, 10], 10).tolist() == [0, 3, 7]
    for off in ([0, 3, 9], [1, 3, 10], [0, 5, 3, 10], [0]):
        with pytest.raises(ValueError):
            sampling.segment_sizes(off, 10)
    for k in (-1, 2.0, True):
        with pytest.raises(ValueError):
            sampling.check_count(k)


def test_num_keypoints_forms():
    from pointgnn_amd import graph_gen
    # car_auto_T1's scales: one pooling level, then two levels that keep it
    assert graph_gen.keypoint_counts(256, [1, 1, 1]) == {0: 256}
    assert graph_gen.keypoint_counts([256], [1, 1, 1]) == {0: 256}
    assert graph_gen.keypoint_counts(64, [1, 2, 2, 4]) == {0: 64, 1: 64, 3: 64}
    assert graph_gen.keypoint_counts((512, 128, 32), [1, 2, 2, 4]) == \
        {0: 512, 1: 128, 3: 32}
    # scale 0 first: level 0 keeps the cloud (graph_gen.py:76-81)
    assert graph_gen.keypoint_counts([100], [0, 1]) == {1: 100}
    for bad in (None, 0, -3, 2.5, True, [256, 64], [], [0], ["a"]):
        with pytest.raises(ValueError):
            graph_gen.keypoint_counts(bad, [1, 1, 1])


def test_multi_level_graph_argument_errors():
    """raised before anything touches the device"""
    from pointgnn_amd import configs, graph_gen
    cfg = configs.get_config("car_auto_T1")
    kw = dict(cfg["runtime_graph_gen_kwargs"])
    xyz = np.zeros((10, 3), np.float32)
    with pytest.raises(ValueError, match="needs num_keypoints"):
        graph_gen.gen_multi_level_local_graph_v3(
            xyz, **dict(kw, downsample_method="farthest"))
    with pytest.raises(ValueError, match="pooling levels"):
        graph_gen.gen_multi_level_local_graph_v3(
            xyz, **dict(kw, downsample_method="farthest",
                        num_keypoints=[64, 32]))
    for method in ("center", "random"):
        with pytest.raises(ValueError, match="num_keypoints belongs"):
            graph_gen.gen_multi_level_local_graph_v3(
                xyz, **dict(kw, downsample_method=method, num_keypoints=64))
    with pytest.raises(ValueError, match="unknown downsample_method"):
        graph_gen.gen_multi_level_local_graph_v3(
            xyz, **dict(kw, downsample_method="farthest_first"))
    hints = graph_gen.CountHints(k=64, edges=[1000, 1000])
    with pytest.raises(NotImplementedError, match="no capacity form"):
        graph_gen.gen_multi_level_local_graph_v3(
            xyz, deferred_counts=hints,
            **dict(kw, downsample_method="farthest", num_keypoints=64))


# ---- the C entries ------------------------------------------------------------
def _lib():
    from pointgnn_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        from pointgnn_amd import build
        build.build(verbose=False)
    return L, L.load()


def test_entries_exist_and_check_their_arguments():
    L, lib = _lib()
    assert set(ENTRIES) <= set(L.exported_symbols())
    ws = lib.pgnn_farthest_first_workspace_bytes
    assert ws(0, 1, 8) == 0 and ws(FC.RES64, 1, 8) == 0
    assert ws(FC.RES64 + 1, 1, 8) >= 8 * (FC.RES64 + 1)
    assert ws(4 * FC.RES32, 5, 64) >= 8 * 4 * FC.RES32
    null = ctypes.c_void_p(0)
    one = (ctypes.c_int32 * 4)()
    p = ctypes.cast(one, ctypes.c_void_p)
    for fn in (lib.pgnn_farthest_first, lib.pgnn_farthest_first_f64):
        # (points, offsets, S, N, start, k, ws, ws_bytes, idx, xyz, nd, stream)
        assert fn(p, null, 2, 4, p, 1, null, 0, p, null, p, null) == \
            L.E_INVALID                      # no offsets, two segments
        assert fn(p, null, 1, -1, p, 1, null, 0, p, null, p, null) == \
            L.E_INVALID
        assert fn(p, null, 1, 4, p, -1, null, 0, p, null, p, null) == \
            L.E_INVALID
        assert fn(p, null, 1, 1 << 31, p, 1, null, 0, p, null, p, null) == \
            L.E_INVALID
        assert fn(null, null, 1, 4, p, 1, null, 0, p, null, p, null) == \
            L.E_INVALID                      # points
        assert fn(p, null, 1, 4, null, 1, null, 0, p, null, p, null) == \
            L.E_INVALID                      # start
        assert fn(p, null, 1, 4, p, 1, null, 0, null, null, p, null) == \
            L.E_INVALID                      # out_idx
        assert fn(p, null, 1, 4, p, 1, null, 0, p, null, null, null) == \
            L.E_INVALID                      # num_distinct
        # a streaming-size cloud without its workspace
        assert fn(p, null, 1, 4 * FC.RES32, p, 1, null, 0, p, null, p,
                  null) == L.E_WORKSPACE
        assert fn(p, p, 0, 0, p, 1, null, 0, p, null, p, null) == 0
