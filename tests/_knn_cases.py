"""The kNN-within-radius contract (include/pointgnn_hip.h,
pgnn_knn_graph_count) restated in NumPy float64, and the clouds that aim at
the branches of knn_select_kernel (csrc/graph.hip).

tests/test_knn_cases_cpu.py proves that every cloud reaches the branch it is
named for; tests/test_gpu_knn_graph.py holds the device to `knn_reference` with
`==` on all of them, in float32 and in float64.

The restatement forms all (centre, point) pairs:
  coordinates widened to float64 and pre-divided by `scale` (load_point),
  d2 = (dx*dx + dy*dy) + dz*dz, one rounding per operation (NumPy evaluates
  every ufunc separately, so nothing is contracted),
  N(q) = {i : d2 <= r*r},
  kept(q) = the first min(k, |N(q)|) of N(q) under lexsort on (idx, d2).
Since the order does not depend on k, the whole sorted neighbourhood is
computed once per cloud (`neighbourhoods`) and every k takes a prefix of it.
"""
import numpy as np

import _graph_cases as gc

K_MAX = 256
K_EDGES = (1, 4, 63, 64, 65, 128, 255, 256)   # lane and key-per-lane seams
CHUNK_TOTALS = (64, 65, 128, 129)             # chunk and double-chunk seams
MANY = 4                                      # "many times k": fan-in >= 4 k


# --------------------------------------------------------------------------
# the restatement
# --------------------------------------------------------------------------
def pair_d2(points, centers, scale=None):
    """float64 squared distances [Q, N] with the contract's parenthesisation"""
    p, c = gc._scaled(points, scale), gc._scaled(centers, scale)
    d = p[None, :, :] - c[:, None, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + \
        d[..., 2] * d[..., 2]


def neighbourhoods(points, centers, r, scale=None):
    """-> list over centres of (idx int64 [fan-in], d2 float64 [fan-in]): the
    radius neighbourhood of every centre in ascending (d2, idx) order"""
    out = []
    r2 = float(r) * float(r)
    n = len(points)
    step = max(1, (1 << 22) // max(n, 1))
    for q0 in range(0, len(centers), step):
        d2 = pair_d2(points, centers[q0:q0 + step], scale)
        for row in d2:
            idx = np.flatnonzero(row <= r2)
            order = np.lexsort((idx, row[idx]))
            out.append((idx[order], row[idx][order]))
    return out


def take_k(hoods, k):
    """-> (edges int32 [E,2] rows (point, centre), offsets int32 [Q+1])"""
    rows = [np.stack([idx[:k], np.full(min(k, len(idx)), q, np.int64)], 1)
            for q, (idx, _) in enumerate(hoods)]
    counts = [len(x) for x in rows]
    edges = np.concatenate(rows) if rows else np.zeros((0, 2), np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)]) if rows else \
        np.zeros(1, np.int64)
    return edges.astype(np.int32).reshape(-1, 2), offsets.astype(np.int32)


def knn_reference(points, centers, r, k, scale=None):
    return take_k(neighbourhoods(points, centers, r, scale), k)


def cut_ties(hoods, k):
    """Per centre with fan-in > k: how many members of N(q) share the d2 of the
    k-th kept one, as (kept among them, dropped among them).  A centre whose
    second number is positive had its k-th place decided by the point index."""
    out = []
    for idx, d2 in hoods:
        if len(idx) <= k:
            out.append((0, 0))
            continue
        tied = d2 == d2[k - 1]
        out.append((int(tied[:k].sum()), int(tied[k:].sum())))
    return out


def walk_positions(points, center, r, scale=None):
    """Position of every candidate in the concatenated candidate list the wave
    walks for `center` (graph.hip: box cells in (z, y, x) lane order, each
    cell's bucket slice in index order), for the visit under the point's OWN
    cell -- the one at which it is accepted.  -> (dict idx -> position,
    candidate total)"""
    grid = gc.RadiusGrid(points, r, scale)
    c = gc._scaled(np.asarray(center).reshape(1, 3), scale)[0]
    cells = gc.box_cells(c, grid.r)
    buckets = gc.cell_hash(cells, grid.mask)
    pos, at = {}, 0
    for cell, b in zip(cells, buckets):
        members = np.flatnonzero(grid.bucket == b)      # index order
        for s, i in enumerate(members):
            if np.array_equal(grid.cells[i], cell):
                pos[int(i)] = at + s
        at += len(members)
    return pos, at


# --------------------------------------------------------------------------
# the cases
# --------------------------------------------------------------------------
class KnnCase(object):
    """One cloud with the k values it is run at.  `same`: the device test
    passes ONE tensor as points and centres."""

    def __init__(self, name, points, centers, r, ks, scale=None, same=False):
        self.name, self.points, self.centers = name, points, centers
        self.r, self.ks, self.scale, self.same = r, tuple(ks), scale, same

    def __repr__(self):
        return self.name

    def cast(self, dtype):
        p = np.ascontiguousarray(self.points, dtype=dtype)
        c = p if self.same else np.ascontiguousarray(self.centers, dtype=dtype)
        return p, c


FAR_CENTRE = (200.0, 200.0, 200.0)


EXTRA_M = 254                     # K_EDGES has 255: its k - 1
EXTRA_CELL = (100, 100, 100)      # chunk_sweep's cells lie in [1, 60)^3


def sweep():
    """chunk_sweep (fan-in exactly m = 1..200, 255, 256, 257 at the mid-cell
    centres, candidate total exactly m), one more cluster of 254 points in a
    cell of its own (appended: chunk_sweep's indices stay) and one centre with
    no neighbour, at every k of K_EDGES: fan-in 0, 1, k - 1, k, k + 1 for each
    of them.
    -> (KnnCase, m of every centre; 0 for the one without neighbours)"""
    case, ms = gc.chunk_sweep()
    rng = np.random.default_rng(254)
    q = rng.choice(1022 ** 2, size=EXTRA_M, replace=False)
    frac = np.stack([q % 1022 + 1, q // 1022 + 1,
                     rng.integers(1, 1023, EXTRA_M)], 1) / 1024.0
    cell = np.array(EXTRA_CELL, np.float64)
    points = np.concatenate([case.points, (cell + frac).astype(np.float32)])
    centers = np.concatenate([case.centers,
                              np.array([cell + 0.5, FAR_CENTRE], np.float32)])
    return (KnnCase("sweep", points, centers, case.r, K_EDGES),
            np.concatenate([ms, [EXTRA_M, 0]]))


DENSE_N = 1200


def dense():
    """1200 distinct points (multiples of 2^-10) in the cube [0.5, 1.5)^3,
    r = 1: the cube spans 8 cells, the centre (1, 1, 1) lies on three cell
    faces (a 64-cell box) and has every point within r -- a fan-in of many
    times k for every k up to 256, over 19 chunks."""
    rng = np.random.default_rng(77)
    q = rng.choice(1024 ** 3, size=DENSE_N, replace=False)
    pts = np.stack([q % 1024, (q // 1024) % 1024, q // (1024 * 1024)],
                   1) / 1024.0 + 0.5
    centers = np.concatenate([[[1.0, 1.0, 1.0]], pts[:12],
                              [[0.75, 1.25, 1.0], [2.25, 1.0, 1.0]]])
    return KnnCase("dense", pts.astype(np.float32),
                   centers.astype(np.float32), 1.0, (1, 4, 64, 256))


def lattice_r2():
    """The 8^3 integer lattice as points AND centres, r = 2.  An interior
    centre has 1, 6, 12, 8, 6 neighbours at d2 = 0, 1, 2, 3, 4 (33 in all, the
    last six at exactly r):
      k = 4   cuts the six at d2 = 1            (index decides)
      k = 10  cuts the twelve at d2 = 2         (index decides)
      k = 30  cuts the six at exactly r         (they win or lose by index)
      k = 33  keeps them all"""
    l8 = gc._lattice(8)
    return [KnnCase("lattice8_r2_" + tag, l8.astype(dt), l8.astype(dt), 2.0,
                    (4, 10, 30, 33), same=True)
            for dt, tag in ((np.float32, "f32"), (np.float64, "f64"))]


LATTICE_K = {"lattice8_r1": (4,), "lattice12_r5": (65,),
             "lattice12_scaled": (16,), "lattice8_tenth": (3,)}


def lattices():
    """_graph_cases.lattices(): centres ON cell faces (64-cell boxes),
    neighbours at exactly r, negative coordinates, the anisotropic scale
    (1, 2, 0.5), the decimal lattice."""
    out = []
    for case in gc.lattices():
        ks = [v for key, v in LATTICE_K.items() if case.name.startswith(key)]
        out.append(KnnCase(case.name, case.points, case.centers, case.r,
                           ks[0], case.scale))
    return out


def duplicates():
    """300 points (multiples of 2^-8), each present three times, shuffled; the
    centres are 60 of them.  Every distance occurs three times: k = 2 cuts the
    triple at d2 = 0, k = 5 the next one."""
    rng = np.random.default_rng(31)
    base = rng.integers(0, 4 * 256, (300, 3)) / 256.0
    pts = np.concatenate([base, base, base])[rng.permutation(900)]
    return KnnCase("duplicates", pts.astype(np.float32),
                   base[:60].astype(np.float32), 1.0, (2, 5))


TIE_NEAR, TIE_FAR = 10, 140
TIE_CENTRE = (10.5, 10.5, 10.5)


def tie_two_chunks():
    """r = 1, one centre in the middle of cell (10, 10, 10).  Six points at
    exactly d2 = 0.5625, one in each face-neighbour cell; the centre's own cell
    holds 10 nearer points and 140 farther ones (still within r), which the
    walk meets between the first three tied points and the last three -- more
    than two chunks apart.  k = 13 keeps the 10 near points and the three tied
    points of smallest index: 0 and 2, which the walk meets LAST, and 1, which
    it meets first."""
    rng = np.random.default_rng(5)
    c = np.array(TIE_CENTRE)
    e = np.eye(3) * 0.75
    # walk order (z, y, x): -z, -y, -x, [own cell], +x, +y, +z
    tied = {"-z": c - e[2], "-y": c - e[1], "-x": c - e[0],
            "+x": c + e[0], "+y": c + e[1], "+z": c + e[2]}
    near, far = [], []
    while len(near) < TIE_NEAR:
        p = c + rng.integers(-64, 65, 3) / 256.0
        if not any(np.array_equal(p, x) for x in near):
            near.append(p)
    while len(far) < TIE_FAR:
        p = np.floor(c) + rng.integers(1, 256, 3) / 256.0
        if ((p - c) ** 2).sum() > 0.6 and \
                not any(np.array_equal(p, x) for x in far):
            far.append(p)
    pts = [tied["+z"], tied["-x"], tied["+y"]] + near + far + \
        [tied["-z"], tied["+x"], tied["-y"]]
    return KnnCase("tie_two_chunks", np.array(pts, np.float32),
                   np.array([c], np.float32), 1.0, (13,))


def shared_bucket():
    """_graph_cases.shared_bucket_box: two cells of the box in one bucket,
    with a stranger between them; k below and above the six aimed
    neighbours."""
    case, info = gc.shared_bucket_box()
    return KnnCase("shared_bucket_box", case.points, case.centers, case.r,
                   (2, 4, 8)), info


BLOB_N, BLOB_K = 1500, 24


def _blob():
    rng = np.random.default_rng(2024)
    pts = rng.uniform(0.0, 6.0, (BLOB_N, 3)).astype(np.float32)
    own = pts[rng.choice(BLOB_N, 200, replace=False)]
    away = rng.uniform(-1.0, 7.0, (50, 3)).astype(np.float32)
    return pts, np.concatenate([own, away])


def blobs():
    """A uniform float32 cloud without exact ties; centres are 200 of its
    points and 50 points that are not (some outside the cloud).  Plain, with
    an anisotropic scale and with a scalar one."""
    pts, ctr = _blob()
    return [KnnCase("blob", pts, ctr, 1.0, (BLOB_K,)),
            KnnCase("blob_aniso", pts, ctr, 1.0, (BLOB_K,), [1.0, 2.0, 0.5]),
            KnnCase("blob_scalar", pts, ctr, 0.5, (BLOB_K,), 2.0)]


def blob_shuffled():
    """-> (KnnCase of the blob in a shuffled point order, perm) with
    shuffled.points[j] == blob.points[perm[j]]"""
    pts, ctr = _blob()
    perm = np.random.default_rng(8).permutation(BLOB_N)
    return KnnCase("blob_shuffled", pts[perm], ctr, 1.0, (BLOB_K,)), perm


def degenerate():
    one = np.array([[1.0, 2.0, 3.0]], np.float32)
    three = np.array([[1.0, 2.0, 3.0], [1.5, 2.0, 3.0], [4.0, 2.0, 3.0]],
                     np.float32)
    pts, _ = _blob()
    return [KnnCase("no_centres", pts[:100], np.zeros((0, 3), np.float32),
                    1.0, (1, 4)),
            KnnCase("one_point", one, three, 1.0, (1, 4))]


def all_cases():
    out = [sweep()[0], dense()] + lattice_r2() + lattices() + \
        [duplicates(), tie_two_chunks(), shared_bucket()[0]] + blobs() + \
        degenerate()
    assert len(set(c.name for c in out)) == len(out)
    return out


_HOODS = {}


def hoods_of(case, dtype):
    """neighbourhoods of `case` run in `dtype`, computed once and shared"""
    key = (case.name, np.dtype(dtype).name)
    if key not in _HOODS:
        p, c = case.cast(dtype)
        _HOODS[key] = neighbourhoods(p, c, case.r, case.scale)
    return _HOODS[key]
