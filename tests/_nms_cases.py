"""Scenes and references for the structural NMS tests
(tests/test_nms_cases_cpu.py proves them, tests/test_gpu_nms_structure.py uses
them on the device).

The scenes are built so that the scan's outcome is a matter of ORDER alone:
every overlap a scan can evaluate is either an exact zero (the bounds test) or
farther than `MARGIN` from the threshold, so no rounding decides a pair and the
kept indices can be demanded exactly.  The builders assert that condition.

  chain_scene    chains of axis-aligned boxes in which only neighbours overlap:
                 who survives depends on the order the scan takes them in
  cluster_scene  objects with many jittered votes: removed sets of a chosen
                 size (the in-LDS list holds 1024 entries)
  nms_sparse     the oracle's loop restricted to neighbour lists
  keep_only      the same decisions by integers alone (chain scenes only)
  OVERLAP_TABLE  pairs of boxes with a closed-form BEV intersection area
"""
import numpy as np

from oracle import detect_oracle as DO

MARGIN = 0.05
CHAIN_SIZE = (4.0, 1.5, 1.6)    # l, h, w
CHAIN_STEP = 2.5
# neighbours share 1.5 of 4.0 in x and everything else: 3.6 / (19.2 - 3.6)
CHAIN_OVERLAP = 3.6 / 15.6
CHAINS_PER_ROW = 120
ORDERS = ("random", "desc", "asc", "interleaved")


def _chain_ranks(n_chains, length, order, rng):
    """rank[c, p] of box p of chain c: 0 = best score; all distinct."""
    c = np.arange(n_chains)[:, None]
    p = np.arange(length)[None, :]
    if order == "random":
        return rng.permutation(n_chains * length).reshape(n_chains, length)
    if order == "desc":
        return c * length + p
    if order == "asc":
        return c * length + (length - 1 - p)
    if order == "interleaved":     # A0 > B0 > A1 > B1 ... for chains (A, B)
        return (c // 2) * 2 * length + 2 * p + (c % 2)
    raise ValueError(order)


def chain_scene(n_chains, length, seed, order, thr=0.1):
    """-> (labels int64 [n], boxes float32 [n,7], scores float32 [n],
    neighbours int64 [n,2]) with n = n_chains * length, shuffled.

    neighbours[i] holds the INPUT indices of box i's chain neighbours (-1:
    none).  Neighbours overlap by CHAIN_OVERLAP, every other pair by exactly 0
    (apart in x or z: the bounds test), and every coordinate is a multiple of
    0.5, hence exact in float32.  Labels come from {1, 3} with p = (0.8, 0.2):
    a mismatch breaks a chain.  `order` sets the scores, see ORDERS."""
    assert abs(CHAIN_OVERLAP - thr) > MARGIN and thr > MARGIN, thr
    rng = np.random.default_rng(seed)
    n = n_chains * length
    l, h, w = CHAIN_SIZE
    pitch = CHAIN_STEP * (length - 1) + 14.0
    c = np.repeat(np.arange(n_chains), length)
    p = np.tile(np.arange(length), n_chains)
    boxes = np.zeros((n, 7), np.float64)
    boxes[:, 0] = (c % CHAINS_PER_ROW) * pitch + p * CHAIN_STEP
    boxes[:, 1] = 1.0
    boxes[:, 2] = (c // CHAINS_PER_ROW) * 8.0
    boxes[:, 3:6] = (l, h, w)
    assert np.array_equal(boxes[:, :3] * 2, np.round(boxes[:, :3] * 2))
    labels = rng.choice([1, 3], n, p=[0.8, 0.2]).astype(np.int64)
    ranks = _chain_ranks(n_chains, length, order, rng).reshape(-1)
    assert len(np.unique(ranks)) == n
    top = float(ranks.max() + 2)
    scores = ((top - 1 - ranks) / top).astype(np.float32)
    assert len(np.unique(scores)) == n
    perm = rng.permutation(n)           # input index k holds ordered box perm[k]
    where = np.empty(n, np.int64)
    where[perm] = np.arange(n)
    idx = np.arange(n)
    left = np.where(p > 0, where[np.maximum(idx - 1, 0)], -1)
    right = np.where(p < length - 1, where[np.minimum(idx + 1, n - 1)], -1)
    neighbours = np.stack([left, right], 1)[perm]
    return labels[perm], boxes[perm].astype(np.float32), scores[perm], \
        neighbours


def cluster_scene(sizes, seed, quantum=None, thr=0.01):
    """One object per entry of `sizes`, 30 m apart, with that many votes:
    centre + N(0, 0.03) on all seven components -> (labels, boxes, scores).

    `quantum`: None, one value, or one per object (None: leave it alone); the
    votes of that object are rounded to multiples of it, which ties many values
    of the rank-count median.  Scores are distinct, so each object's winner is
    its best-scored vote; the builder asserts that the winner's overlap with
    every other vote of its object clears `thr` by MARGIN (the objects are
    apart from one another: exact zeros)."""
    rng = np.random.default_rng(seed)
    if quantum is None or np.isscalar(quantum):
        quantum = [quantum] * len(sizes)
    assert len(quantum) == len(sizes)
    boxes, obj = [], []
    for k, (cnt, q) in enumerate(zip(sizes, quantum)):
        ctr = np.array([1.0 + 30.0 * k, 1.25, 20.0, 3.875, 1.5, 1.625, 0.40625])
        v = ctr + rng.normal(0, 0.03, (cnt, 7))
        if q:
            v = np.round(v / q) * q
        boxes.append(v)
        obj += [k] * cnt
    boxes = np.concatenate(boxes).astype(np.float32)
    obj = np.array(obj)
    n = len(boxes)
    labels = np.ones(n, np.int64)
    scores = (0.26 + 0.7 * (rng.permutation(n) + 0.5) / n).astype(np.float32)
    assert len(np.unique(scores)) == n
    perm = rng.permutation(n)
    labels, boxes, scores, obj = labels[perm], boxes[perm], scores[perm], \
        obj[perm]
    assert winner_overlap_min(boxes, scores, len(sizes)) > thr + MARGIN
    corners = DO.boxes_3d_to_corners(boxes)
    lo, hi = corners.min(axis=1)[:, 0], corners.max(axis=1)[:, 0]
    for k in range(len(sizes)):      # objects are apart in x: exact zeros
        assert np.all((hi[obj != k] < lo[obj == k].min()) |
                      (lo[obj != k] > hi[obj == k].max()))
    return labels, boxes, scores


def winner_overlap_min(boxes, scores, n_objects):
    """Smallest overlap of an object's best-scored vote with its other votes
    in a cluster_scene (objects are told apart by their 30 m pitch)."""
    obj = np.round((boxes[:, 0] - 1.0) / 30.0).astype(int)
    corners = DO.boxes_3d_to_corners(boxes)
    best = np.inf
    for k in range(n_objects):
        mine = np.nonzero(obj == k)[0]
        win = mine[np.argmax(scores[mine])]
        rest = mine[mine != win]
        if len(rest):
            best = min(best, DO.overlapped_boxes_3d_fast_poly(
                corners[win], corners[rest]).min())
    return best


def _sorted_view(labels, scores, top_k):
    order = np.argsort(-np.asarray(scores), kind="stable")
    if top_k > 0:
        order = order[:top_k]
    pos = np.full(len(np.asarray(labels)), -1, np.int64)
    pos[order] = np.arange(len(order))
    return order, pos


def row_arithmetic(boxes, scores, corners, i, hit, merge, rescore):
    """What the oracle's loop does to row i once its removed set `hit`
    (ascending sorted positions) is known: median merge and score
    accumulation, in place on the sorted copies (detect_oracle.nms_boxes_3d)."""
    if merge:
        boxes[i] = np.median(np.concatenate([boxes[hit], boxes[[i]]]), axis=0)
    if rescore:
        mean_corners = DO.boxes_3d_to_corners(boxes[[i]])[0]
        ov2 = DO.overlapped_boxes_3d_fast_poly(mean_corners, corners[hit])
        scores[i] += np.sum(scores[hit] * ov2)


def nms_sparse(labels, boxes, scores, thr, mode, neighbours, top_k=-1,
               appr_factor=10.0):
    """detect_oracle.nms_boxes_3d with `later` restricted to each box's
    neighbour list (input indices, -1 = none): the same result wherever every
    pair outside the lists overlaps by 0, at a cost linear in the boxes."""
    labels = np.asarray(labels)
    order, pos = _sorted_view(labels, scores, top_k)
    s_lab = labels[order]
    s_sco = np.array(scores)[order]
    s_box = np.array(boxes)[order]
    merge = mode in ("uncertainty", "merge_only")
    rescore = mode in ("uncertainty", "score_only")
    corners = DO.boxes_3d_to_corners(s_box)
    if mode == "plain":
        corners = np.int32(corners * appr_factor)
    m = len(order)
    nb_pos = np.where(np.asarray(neighbours) >= 0,
                      pos[np.maximum(neighbours, 0)], -1)[order]
    keep = np.ones(m, bool)
    for i in range(m - 1):
        if not keep[i]:
            continue
        later = np.array(sorted(j for j in nb_pos[i] if j > i and keep[j]),
                         np.int64)
        ov = DO.overlapped_boxes_3d_fast_poly(corners[i], corners[later])
        hit = later[(ov > thr) & (s_lab[later] == s_lab[i])]
        row_arithmetic(s_box, s_sco, corners, i, hit, merge, rescore)
        keep[hit] = False
    return s_lab[keep], s_box[keep], s_sco[keep], order[keep]


def keep_only(labels, scores, neighbours, top_k=-1, return_removed_by=False):
    """The scan's decisions on a chain_scene by integers alone: a later, still
    kept neighbour with the same label is a hit (neighbours overlap beyond the
    threshold, nothing else overlaps).  -> kept input indices in score order
    [, removed_by: input index of the box that removed each box, -1 = kept]."""
    labels = np.asarray(labels)
    order, pos = _sorted_view(labels, scores, top_k)
    n = len(labels)
    keep = pos >= 0
    removed_by = np.full(n, -1, np.int64)
    lab = labels.tolist()
    nbs = np.asarray(neighbours).tolist()
    posl = pos.tolist()
    for i in order.tolist():
        if not keep[i]:
            continue
        for j in nbs[i]:
            if j >= 0 and posl[j] > posl[i] and keep[j] and lab[j] == lab[i]:
                keep[j] = False
                removed_by[j] = i
    kept = order[keep[order]]
    return (kept, removed_by) if return_removed_by else kept


def desc_survivors(labels, neighbours):
    """Closed form for order "desc": the scores fall along a chain, so a box is
    removed exactly when its left neighbour survives and has its label -- the
    survivors are the even positions of each label-unbroken run.  -> set of
    kept input indices."""
    labels = np.asarray(labels)
    kept = set()
    for start in np.nonzero(neighbours[:, 0] < 0)[0]:
        k, run_pos = int(start), 0
        while k >= 0:
            if run_pos % 2 == 0:
                kept.add(k)
            nxt = int(neighbours[k, 1])
            run_pos = run_pos + 1 if nxt >= 0 and labels[nxt] == labels[k] \
                else 0
            k = nxt
    return kept


# ---------------------------------------------------------------------------
# closed-form overlaps.  Boxes are float32 (x, y, z, l, h, w, yaw); sizes and
# centres are stored as the float32 values the device receives and the areas
# below are computed from those, so that only cos/sin of the yaw round.
def _box(cx, cz, l, w, yaw, y=0.0, h=1.0):
    return np.array([cx, y, cz, l, h, w, yaw], np.float32)


def _table():
    t = []
    sq = _box(0, 0, 2, 2, 0.0)

    def other(cx, cz, l, w, yaw):       # y range [-0.5, 0.5] against [-1, 0]
        return _box(cx, cz, l, w, yaw, y=0.5, h=1.0)

    for dx, dz in ((0.5, 0.0), (1.0, 1.0), (1.5, -0.25)):
        t.append(("shifted_%g_%g" % (dx, dz), sq, other(dx, dz, 2, 2, 0.0),
                  (2 - abs(dx)) * (2 - abs(dz))))
    t.append(("corner_touching", sq, other(2, 2, 2, 2, 0.0), 0.0))
    t.append(("edge_sharing", sq, other(2, 0, 2, 2, 0.0), 0.0))
    inner = other(0.1, -0.2, 0.5, 0.3, 0.7)
    t.append(("contained_rotated", sq, inner,
              float(inner[3]) * float(inner[5])))          # 0.15 in float32
    t.append(("identical", sq, sq.copy(), 4.0))
    t.append(("bar_across_yaw0", sq, other(0, 0, 6, 1, 0.0), 2.0))
    t.append(("bar_across_half_pi", sq, other(0, 0, 1, 6, np.pi / 2), 2.0))
    t.append(("octagon", sq, other(0, 0, 2, 2, np.pi / 4),
              2 * (np.sqrt(2.0) - 1) * 4.0))
    t.append(("disjoint", sq, other(5, 5, 2, 2, 0.3), 0.0))
    return t


OVERLAP_TABLE = _table()   # (name, box a, box b, BEV intersection area)


def overlap_from_area(a, b, area):
    """overlapped_boxes_3d_fast_poly's value (nms.py:64-88) for two boxes whose
    BEV intersection area is known: float32(shared_y * area) / (union - it),
    with the boxes' own volumes from l * h * w."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    if area == 0.0:
        return 0.0
    shared_y = min(a[1], b[1]) - max(a[1] - a[4], b[1] - b[4])
    inter = shared_y * area
    union = a[3] * a[4] * a[5] + b[3] * b[4] * b[5]
    return float(np.float32(inter)) / (union - inter)


def isolated_grid(n, seed):
    """n boxes on an 8 m grid with random yaw and labels: nothing overlaps, so
    NMS is a sort -> (labels, boxes)."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n)))
    boxes = np.zeros((n, 7), np.float32)
    boxes[:, 0] = (np.arange(n) % side) * 8.0
    boxes[:, 2] = (np.arange(n) // side) * 8.0
    boxes[:, 1] = 1.0
    boxes[:, 3:6] = (3.9, 1.5, 1.6)
    boxes[:, 6] = rng.uniform(-3, 3, n)
    return rng.choice([1, 3], n).astype(np.int64), boxes
