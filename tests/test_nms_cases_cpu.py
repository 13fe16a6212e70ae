"""The scenes and helper references of tests/_nms_cases.py, proved on the CPU
against oracle/detect_oracle.py (itself pinned to the reference's output in
tests/test_detect_cpu.py), so that tests/test_gpu_nms_structure.py may use the
cheap forms where the full oracle loop would take too long.  No GPU."""
import numpy as np
import pytest

import _nms_cases as NC
from oracle import detect_oracle as DO

THR_CHAIN = 0.1
THR_CLUSTER = 0.01
CLUSTER_SIZES = [1024, 1025, 1026, 1500, 7, 2]
CLUSTER_QUANTUM = [None, 1.0 / 32, None, None, None, None]


@pytest.fixture(scope="module")
def chains():
    return NC.chain_scene(840, 5, 1, "random")


@pytest.mark.parametrize("mode", ["uncertainty", "merge_only", "score_only"])
def test_sparse_loop_equals_oracle(chains, mode):
    labels, boxes, scores, nb = chains
    want = DO.nms_boxes_3d(labels, boxes, scores, THR_CHAIN, mode)
    got = NC.nms_sparse(labels, boxes, scores, THR_CHAIN, mode, nb)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    assert 0 < len(want[3]) < len(labels)
    if mode == "uncertainty":
        # the integer greedy takes the same decisions
        kept, by = NC.keep_only(labels, scores, nb, return_removed_by=True)
        assert np.array_equal(kept, want[3])
        gone = np.setdiff1d(np.arange(len(labels)), kept)
        assert np.all(by[gone] >= 0) and np.all(by[kept] < 0)


def test_sparse_loop_and_greedy_respect_top_k(chains):
    labels, boxes, scores, nb = chains
    sub = slice(0, 600)     # neighbours outside the slice: drop them
    nb600 = np.where(nb[sub] < 600, nb[sub], -1)
    for top_k in (1, 64, 65, 599, 600, 700):
        want = DO.nms_boxes_3d(labels[sub], boxes[sub], scores[sub], THR_CHAIN,
                               "uncertainty", top_k=top_k)
        got = NC.nms_sparse(labels[sub], boxes[sub], scores[sub], THR_CHAIN,
                            "uncertainty", nb600, top_k=top_k)
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
        assert np.array_equal(
            NC.keep_only(labels[sub], scores[sub], nb600, top_k=top_k),
            want[3])


def test_chain_scene_overlaps_are_far_from_the_threshold(chains):
    """Condition of the GPU tests: neighbours overlap by 0.2308, 0.1308 from
    the threshold; every other pair is apart in the bounds test (exact 0)."""
    labels, boxes, scores, nb = chains
    n = len(labels)
    corners = DO.boxes_3d_to_corners(boxes)
    have = np.nonzero(nb[:, 1] >= 0)[0]
    ov = np.array([DO.overlapped_boxes_3d_fast_poly(
        corners[i], corners[[nb[i, 1]]])[0] for i in have])
    assert np.all(ov == ov[0])          # translations of one exact pair
    assert ov[0] == pytest.approx(NC.CHAIN_OVERLAP, rel=1e-6)
    assert abs(ov[0] - THR_CHAIN) > 0.13 > NC.MARGIN
    lo, hi = corners.min(axis=1), corners.max(axis=1)
    apart = np.zeros((n, n), bool)
    for k in (0, 2):
        apart |= (hi[:, None, k] < lo[None, :, k]) | \
            (lo[:, None, k] > hi[None, :, k])
    linked = np.eye(n, dtype=bool)
    for col in (0, 1):
        src = np.nonzero(nb[:, col] >= 0)[0]
        linked[src, nb[src, col]] = True
    assert np.array_equal(~apart, linked)
    assert np.array_equal(linked, linked.T)
    # both labels occur and some neighbours differ in label (broken chains)
    assert 0.1 < np.mean(labels == 3) < 0.3
    assert np.any(labels[have] != labels[nb[have, 1]])


@pytest.mark.parametrize("order", NC.ORDERS)
def test_chain_orders(order):
    labels, boxes, scores, nb = NC.chain_scene(2, 70, 5, order)
    rank = np.empty(140, np.int64)
    rank[np.argsort(-scores, kind="stable")] = np.arange(140)
    # walk each chain from its left end
    chains = []
    for start in np.nonzero(nb[:, 0] < 0)[0]:
        k, c = int(start), []
        while k >= 0:
            c.append(k)
            k = int(nb[k, 1])
        chains.append(np.array(c))
    assert sorted(len(c) for c in chains) == [70, 70]
    if order == "desc":
        assert all(np.all(np.diff(rank[c]) > 0) for c in chains)
    elif order == "asc":
        assert all(np.all(np.diff(rank[c]) < 0) for c in chains)
    elif order == "interleaved":
        a, b = sorted(chains, key=lambda c: rank[c[0]])
        assert np.array_equal(rank[a], 2 * np.arange(70))
        assert np.array_equal(rank[b], 2 * np.arange(70) + 1)
    want = DO.nms_boxes_3d(labels, boxes, scores, THR_CHAIN, "uncertainty")
    assert np.array_equal(NC.keep_only(labels, scores, nb), want[3])
    if order == "desc":
        assert set(want[3].tolist()) == NC.desc_survivors(labels, nb)


def test_cluster_scene_removed_sets_and_margin():
    """The builder asserts the margin; here the figure itself and the sizes
    of the removed sets the GPU test relies on."""
    labels, boxes, scores = NC.cluster_scene(CLUSTER_SIZES, 2, CLUSTER_QUANTUM)
    least = NC.winner_overlap_min(boxes, scores, len(CLUSTER_SIZES))
    print("smallest winner-to-vote overlap: %.4f" % least)
    assert least > THR_CLUSTER + NC.MARGIN
    assert len(np.unique(scores)) == len(scores) == sum(CLUSTER_SIZES)
    obj = np.round((boxes[:, 0] - 1.0) / 30.0).astype(int)
    assert np.bincount(obj).tolist() == CLUSTER_SIZES
    # the quantised object: few distinct values per component
    q = boxes[obj == 1]
    assert np.array_equal(q * 32, np.round(q * 32))
    assert max(len(np.unique(q[:, c])) for c in range(7)) < 12
    want = DO.nms_boxes_3d(labels, boxes, scores, THR_CLUSTER, "merge_only")
    assert len(want[3]) == 6
    assert sorted(np.bincount(obj[want[3]]).tolist()) == [1] * 6


@pytest.mark.parametrize("entry", NC.OVERLAP_TABLE, ids=lambda e: e[0])
def test_overlap_table_matches_oracle_polygons(entry):
    name, a, b, area = entry
    for box in (a, b):      # stored as float32: what the device receives
        assert box.dtype == np.float32
    corners = DO.boxes_3d_to_corners(np.stack([a, b]))
    pa = DO.ConvexPolygon(corners[0][:4][:, [0, 2]])
    pb = DO.ConvexPolygon(corners[1][:4][:, [0, 2]])
    for got in (pa.intersection(pb).area, pb.intersection(pa).area):
        assert got == pytest.approx(area, rel=1e-6, abs=0.0)
    ov = DO.overlapped_boxes_3d_fast_poly(corners[0], corners[1:])[0]
    assert ov == pytest.approx(NC.overlap_from_area(a, b, area), rel=1e-6,
                               abs=0.0)
    vo = DO.overlapped_boxes_3d_fast_poly(corners[1], corners[:1])[0]
    assert vo == pytest.approx(ov, rel=1e-6, abs=0.0)


def test_overlap_table_holds_what_it_should():
    names = [e[0] for e in NC.OVERLAP_TABLE]
    for need in ("corner_touching", "edge_sharing", "contained_rotated",
                 "identical", "bar_across_yaw0", "bar_across_half_pi",
                 "octagon", "disjoint"):
        assert need in names
    assert sum(n.startswith("shifted") for n in names) >= 3
    table = {e[0]: e for e in NC.OVERLAP_TABLE}
    assert table["contained_rotated"][3] == pytest.approx(0.15, rel=1e-7)
    assert table["octagon"][3] == pytest.approx(
        2 * (np.sqrt(2) - 1) * 4.0, rel=1e-15)
    assert NC.overlap_from_area(*table["identical"][1:]) == 1.0
