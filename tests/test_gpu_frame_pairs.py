"""Frame pairs: two capacity-form frames merged on the device
(pgnn_merge_frames_dyn, graph_gen.merge_frames_dyn) and run through the model
as ONE pass (InferenceEngine.run_frames_on_streams, frames_per_pass=2).

The bar is the one the capacity form itself is held to: nothing changes.  A
frame's logits and box encodings out of a pair are BIT-identical to the frame
run alone, `frame_shapes` is the same list, and the merged arrays are the
NumPy concatenation with offsets, up to the merged counts.  The per-vertex
kernels of the capacity form must fit two workgroups on a CU without scratch,
or the pair's 2 x tiles run as two rounds and gain nothing."""
import numpy as np
import pytest

import pointgnn_amd  # noqa: F401
from pointgnn_amd import configs, weights
from pointgnn_amd.synthetic import synthetic_cloud

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from pointgnn_amd import _lib
    _lib.load()
    return torch.device("cuda")


def T(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---- the merge alone -------------------------------------------------------------
def _hand_frame(rng, dev, n, k, e_written, e_required, e_caps):
    """A hand-made capacity-form frame of the car graphs' structure (points ->
    keypoints, keypoints -> keypoints): n points, k keypoints in arrays of n
    rows, edge lists of e_caps rows with e_written valid ones.  Everything
    behind a count is an IN-RANGE index of a row of huge values far away: a
    kernel that read a tail would change a result, never fault."""
    import torch
    from pointgnn_amd import _lib, graph_gen as G
    pts = rng.random((n, 3)).astype(np.float32) * 30
    feat = rng.random((n, 1)).astype(np.float32)
    pts[n - 1] = 1e6            # the row the tails point at
    feat[n - 1] = 1e30
    kp_idx = np.full((n, 1), n - 1, np.int32)
    kp_idx[:k, 0] = np.sort(rng.permutation(n - 1)[:k])
    kp_xyz = np.full((n, 3), -1e6, np.float32)
    kp_xyz[:k] = pts[kp_idx[:k, 0]]
    edges = []
    for lvl, (w, cap) in enumerate(zip(e_written, e_caps)):
        n_src = n if lvl == 0 else k
        e = np.empty((cap, 2), np.int32)
        e[:, 0] = n - 1 if lvl == 0 else k - 1
        e[:, 1] = k - 1
        e[:w, 0] = rng.integers(0, n_src - 1, w)
        e[:w, 1] = np.sort(rng.integers(0, k, w))     # grouped by centre
        edges.append(e)
    rec = [k, 0]
    for w, r in zip(e_written, e_required):
        rec += [w, r]
    counts = torch.tensor(rec, dtype=torch.int32, device=dev)
    frame = G.FrameCounts(counts, e_caps)
    cnt_k = _lib.DeviceCount(counts[0:1], k, frame)
    c1 = _lib.tag_count(T(kp_xyz, dev), cnt_k)
    coords = [T(pts, dev), c1, c1]
    kps = [_lib.tag_count(T(kp_idx, dev), cnt_k),
           _lib.tag_count(G._identity_indices(n, dev), cnt_k)]
    e_dev = []
    for lvl, e in enumerate(edges):
        t = _lib.tag_count(T(e, dev), _lib.DeviceCount(
            counts[2 + 2 * lvl:3 + 2 * lvl], e_written[lvl], frame))
        t._pgnn_sorted = 1
        e_dev.append(t)
    host = dict(pts=pts, feat=feat, kp_idx=kp_idx, kp_xyz=kp_xyz, edges=edges,
                k=k, n=n, written=list(e_written), required=list(e_required))
    return (coords, kps, e_dev), T(feat, dev), host


@pytest.mark.parametrize("overflow", [False, True])
def test_merge_frames_equals_numpy_concatenation(dev, overflow):
    """K_A = 37, K_B = 25: B's rows start at an offset that is no multiple of
    16, read from A's record on the device, and one 16-row tile straddles the
    frames.  Merged arrays up to the merged counts and the merged record ==
    NumPy concatenation with offsets.  overflow: B's level-1 list needs more
    rows than its capacity holds -- the merged record shows it."""
    import torch
    from pointgnn_amd import _lib, graph_gen as G
    rng = np.random.default_rng(17)
    ga, fa, a = _hand_frame(rng, dev, 120, 37, (310, 420), (310, 420),
                            (512, 640))
    wb1, rb1 = (448, 700) if overflow else (365, 365)
    gb, fb, b = _hand_frame(rng, dev, 90, 25, (280, wb1), (280, rb1),
                            (400, 448))
    feats, coords, kps, edges = G.merge_frames_dyn(ga, fa, gb, fb)
    torch.cuda.synchronize()
    frame = _lib.count_of(edges[0]).frame
    k = a["k"] + b["k"]
    want = [k, 0]
    for lvl in (0, 1):
        want += [a["written"][lvl] + b["written"][lvl],
                 a["required"][lvl] + b["required"][lvl]]
    assert frame.read() == want
    assert frame.overflowed == ([1] if overflow else [])
    assert frame.k == k and _lib.count_of(coords[1]).frame is frame
    # the frames' own records are untouched
    assert ga[2][0]._pgnn_count.frame.read()[0] == 37
    assert gb[2][0]._pgnn_count.frame.read()[0] == 25
    assert np.array_equal(coords[0].cpu().numpy(),
                          np.concatenate([a["pts"], b["pts"]]))
    assert np.array_equal(feats.cpu().numpy(),
                          np.concatenate([a["feat"], b["feat"]]))
    assert coords[2] is coords[1]
    assert np.array_equal(coords[1][:k].cpu().numpy(), np.concatenate(
        [a["kp_xyz"][:37], b["kp_xyz"][:25]]))
    assert np.array_equal(kps[0][:k].cpu().numpy(), np.concatenate(
        [a["kp_idx"][:37], b["kp_idx"][:25] + a["n"]]))
    assert np.array_equal(kps[1][:k, 0].cpu().numpy(), np.arange(k))
    for lvl in (0, 1):
        wa, wb = a["written"][lvl], b["written"][lvl]
        shift = np.array([a["n"] if lvl == 0 else 37, 37], np.int32)
        ref = np.concatenate([a["edges"][lvl][:wa],
                              b["edges"][lvl][:wb] + shift])
        got = edges[lvl][:wa + wb].cpu().numpy()
        assert np.array_equal(got, ref)
        assert getattr(edges[lvl], "_pgnn_sorted", 0) == 1
        assert np.all(np.diff(got[:, 1]) >= 0)       # still grouped by centre
        assert int(edges[lvl].shape[0]) >= wa + wb
        assert _lib.count_of(edges[lvl]).hint == wa + wb


# ---- pairs against single frames, through the engine ------------------------------
def _frames(dev, sizes):
    out = []
    for seed, n in sizes:
        xyz, inten = synthetic_cloud(seed, n_points=n)
        assert xyz.shape[0] == n
        out.append((T(xyz, dev), T(inten, dev)))
    return out


def _count_pairs(eng):
    calls = []
    inner = eng.run_pair_deferred

    def counted(a, b):
        calls.append(1)
        return inner(a, b)
    eng.run_pair_deferred = counted
    return calls


def _same(a, b):
    import torch
    assert len(a) == len(b)
    for (l0, b0), (l1, b1) in zip(a, b):
        assert l0.shape[0] > 0 and l0.shape == l1.shape
        assert torch.equal(l0, l1) and torch.equal(b0, b1)


@pytest.fixture(scope="module")
def car_engine(dev):
    from pointgnn_amd.engine import InferenceEngine
    cfg = configs.car_auto_config(3)
    params = weights.init_params(cfg, seed=4, bias_scale=0.05)
    return InferenceEngine(cfg, params, device=dev)


def test_pairs_equal_single_frames(dev, car_engine):
    """car_auto_T3, clouds of 1 500 / 2 300 / 1 900 points: one pair plus an
    odd frame.  frames_per_pass=2 == frames_per_pass=1 bit for bit, frame by
    frame, and the same frame_shapes."""
    eng = car_engine
    frames = _frames(dev, [(1, 1500), (2, 2300), (3, 1900)])
    eng.frame_shapes = []
    single = eng.run_frames_on_streams(frames, 3, frames_per_pass=1)
    shapes = list(eng.frame_shapes)
    assert len(shapes) == 3
    calls = _count_pairs(eng)
    try:
        for n_streams in (1, 3):
            eng.frame_shapes = []
            paired = eng.run_frames_on_streams(frames, n_streams)  # default: 2
            assert eng.frame_shapes == shapes
            _same(single, paired)
    finally:
        del eng.run_pair_deferred
    assert len(calls) == 2          # one pair per call; the odd frame alone
    assert eng.deferred_overflows == 0


def test_pair_at_the_weights_stationary_threshold(dev, car_engine):
    """The smallest clouds whose PAIR takes the weights-stationary edge kernel:
    that kernel is chosen from 16 * 2 * 8 * CUs expected edges on (ws_launch.h,
    edge_ws_applies) -- 65 536 on 256 CUs -- and a pair expects twice the
    hinted count.  synthetic_cloud(7, n_points=700) has E1 = 33 841 (600
    points: 31 797), so the pair runs the weights-stationary kernel where each
    frame alone runs the LDS-tile kernel; K = 363 + 386 keeps the 16-row
    per-vertex kernels.  Different kernels, the same bits."""
    import torch
    eng = car_engine
    frames = _frames(dev, [(7, 700), (8, 700)])
    eng.run_frame(*frames[0])          # the hints every frame below gets
    k, e0, e1 = eng.frame_shapes.pop()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    threshold = 16 * 2 * 8 * cus
    assert e1 < threshold <= 2 * e1, (e1, threshold)
    assert 2 * k <= 32 * cus
    eng.frame_shapes = []
    single = eng.run_frames_on_streams(frames, 2, frames_per_pass=1)
    shapes = list(eng.frame_shapes)
    eng.run_frame(*frames[0])          # the same hints again
    eng.frame_shapes = []
    calls = _count_pairs(eng)
    try:
        paired = eng.run_frames_on_streams(frames, 2, frames_per_pass=2)
    finally:
        del eng.run_pair_deferred
    assert len(calls) == 1 and eng.frame_shapes == shapes
    _same(single, paired)


def test_pair_with_an_overflowing_second_frame(dev, car_engine):
    """The second frame's level-1 list does not fit a deliberately small
    capacity: both frames of the pass are rebuilt singly and come back equal
    to their single runs; deferred_overflows counts the frame that
    overflowed."""
    from pointgnn_amd import graph_gen as G
    eng = car_engine
    frames = _frames(dev, [(1, 1500), (2, 2300)])
    eng.frame_shapes = []
    single = eng.run_frames_on_streams(frames, 2, frames_per_pass=1)
    (k_a, e0_a, e1_a), (k_b, e0_b, e1_b) = eng.frame_shapes
    assert e1_a < e1_b
    cap1 = (e1_a + e1_b) // 2          # holds A's list, not B's
    eng._hints = G.CountHints(k_a, [e0_a, e1_a], [2 * e0_b, cap1])
    before = eng.deferred_overflows
    eng.frame_shapes = []
    calls = _count_pairs(eng)
    try:
        paired = eng.run_frames_on_streams(frames, 2, frames_per_pass=2)
    finally:
        del eng.run_pair_deferred
    assert len(calls) == 1
    assert eng.deferred_overflows == before + 1
    assert eng.frame_shapes == [(k_a, e0_a, e1_a), (k_b, e0_b, e1_b)]
    _same(single, paired)
    assert eng._hints.cap(1) >= e1_b


# ---- two workgroups of the per-vertex kernels on a CU ------------------------------
def test_capacity_form_vertex_kernels_fit_two_workgroups_per_cu(dev, car_engine):
    """pgnn_kernel_occupancy for the three capacity-form per-vertex kernels at
    the LDS bytes of their launches in a car_auto_T3 frame: at least two
    workgroups per CU (<= 128 VGPRs at 8 waves a workgroup, <= half a CU's
    LDS) and no scratch."""
    from pointgnn_amd import _lib
    eng = car_engine
    frames = _frames(dev, [(1, 1500)])
    eng.run_frame(*frames[0])
    eng.frame_shapes.pop()
    eng.model.fuse_vertex_stages = False    # vertex_pre_edge on its own
    try:
        eng.run_frame_deferred(*frames[0]).result()
    finally:
        eng.model.fuse_vertex_stages = True
    eng.run_frame_deferred(*frames[0]).result()
    for name in ("vertex_pre_edge_dyn", "vertex_update_pre_edge_dyn",
                 "vertex_mlp2_dyn"):
        occ = _lib.kernel_occupancy(name)
        print(name, occ)
        assert occ["lds_bytes"] > 0
        assert occ["workgroups_per_cu"] >= 2, (name, occ)
        assert occ["scratch_bytes"] == 0, (name, occ)
        assert occ["vgprs"] <= 128, (name, occ)
