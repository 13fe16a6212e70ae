"""Plain kNN (no radius; include/pointgnn_hip.h, pgnn_knn_nearest): the clouds
that aim at the places where knn_nearest_kernel (csrc/graph.hip) can go wrong,
and a NumPy walk of its search that says which place a cloud reaches.

The contract's restatement is tests/_knn_cases.py: `knn_reference(points,
centers, np.inf, k, scale)` -- `d2 <= inf` keeps every point and the lexsort
on (idx, d2) is the key order -- so every centre has min(k, N) rows and the
offsets are the arithmetic CSR.  Expected rows always come from it.

`shell_walk` restates the SEARCH (not the contract): the grid of edge
`cell_size`, the shells clamped to the cloud's cell bounding box in the
kernel's slab order, 64 cells a lane batch, and the stopping bound b_s with
its shrink.  It only characterises a case; tests/test_nearest_cases_cpu.py
additionally checks that it returns the restatement's rows, i.e. that the
stopping rule is exact on these clouds.
"""
import numpy as np

import _graph_cases as gc
import _knn_cases as KC

K_EDGES = KC.K_EDGES
FAR_CENTRE = KC.FAR_CENTRE
CELL_SIZES = (0.25, 1.0, 7.3, 1000.0)      # 1000: the whole cloud in one cell


class NearestCase(object):
    """One cloud with the k values it is run at and the grid edge it is aimed
    with.  `same`: the device test passes ONE tensor as points and centres.
    `r` is the radius of the restatement: none."""
    r = np.inf

    def __init__(self, name, points, centers, ks, cell=1.0, scale=None,
                 same=False):
        self.name, self.points, self.centers = name, points, centers
        self.ks, self.cell, self.scale, self.same = tuple(ks), cell, scale, same

    def __repr__(self):
        return self.name

    def cast(self, dtype):
        p = np.ascontiguousarray(self.points, dtype=dtype)
        c = p if self.same else np.ascontiguousarray(self.centers, dtype=dtype)
        return p, c


def reference(case, dtype, k):
    """-> edges int32 [Q * min(k, N), 2] of the restatement (hoods shared)"""
    return KC.take_k(KC.hoods_of(case, dtype), k)[0]


# --------------------------------------------------------------------------
# the search, restated
# --------------------------------------------------------------------------
def shell_cells(cc, s, lo, hi):
    """Cells of shell s around cell `cc` inside [lo, hi], in the kernel's slab
    order: z = cz -/+ s, then y = cy -/+ s over the inner z range, then
    x = cx -/+ s over the inner y and z ranges.  -> int array [n, 3]"""
    b0 = np.maximum(lo, cc - s)
    b1 = np.minimum(hi, cc + s)
    yi = (max(b0[1], cc[1] - s + 1), min(b1[1], cc[1] + s - 1))
    zi = (max(b0[2], cc[2] - s + 1), min(b1[2], cc[2] + s - 1))
    xs = np.arange(b0[0], b1[0] + 1)
    ys = np.arange(b0[1], b1[1] + 1)
    yin = np.arange(yi[0], yi[1] + 1)
    zin = np.arange(zi[0], zi[1] + 1)

    def slab(a, b, c, order):
        """cells with the slow axis a, the fast axis b and the plane c"""
        aa, bb = np.meshgrid(a, b, indexing="ij")
        cols = {order[0]: aa.ravel(), order[1]: bb.ravel(),
                order[2]: np.full(aa.size, c)}
        return np.stack([cols["x"], cols["y"], cols["z"]], 1)
    out = []
    for sign in ((-1,) if s == 0 else (-1, 1)):
        z = cc[2] + sign * s
        if lo[2] <= z <= hi[2]:
            out.append(slab(ys, xs, z, "yxz"))
    for sign in (-1, 1):
        y = cc[1] + sign * s
        if lo[1] <= y <= hi[1]:
            out.append(slab(zin, xs, y, "zxy"))
    for sign in (-1, 1):
        x = cc[0] + sign * s
        if lo[0] <= x <= hi[0]:
            out.append(slab(zin, yin, x, "zyx"))
    out = [o for o in out if len(o)]
    return np.concatenate(out) if out else np.zeros((0, 3), np.int64)


def bound(c, cc, s, lo, hi, cell, shrink=True):
    """b_s: the smallest distance from centre c to a face of the scanned box
    cc -/+ s that still has cells of [lo, hi] behind it (inf: none has)"""
    b = np.inf
    for a in range(3):
        if cc[a] - s > lo[a]:
            b = min(b, c[a] - float(cc[a] - s) * cell)
        if cc[a] + s < hi[a]:
            b = min(b, float(cc[a] + s + 1) * cell - c[a])
    if shrink:
        b = b * (1.0 - 1e-9) - 2e-15 * (np.abs(c).max() + (s + 2.0) * cell)
    return b


def shell_walk(points, center, k, cell, scale=None):
    """The kernel's search for one centre.
    -> (point indices in ascending key order,
        info: dict(first, shells=[dict(s, cells, batches, hits, kth, b)],
                   stop='bound' | 'cover'))
    `kth` is the list's last d2 after the shell (None while it is not full),
    `b` the EXACT face distance (no shrink) the stop test is about."""
    grid = gc.RadiusGrid(points, cell, scale)
    c = gc._scaled(np.asarray(center).reshape(1, 3), scale)[0]
    cc = gc.rcell_of(c, cell)
    lo, hi = grid.cells.min(0), grid.cells.max(0)
    m = min(k, len(grid.p))
    first = int(max(0, (lo - cc).max(), (cc - hi).max()))
    cover = int(max((cc - lo).max(), (hi - cc).max()))
    keys, shells, stop = [], [], "cover"
    for s in range(first, cover + 1):
        cells = shell_cells(cc, s, lo, hi)
        hits = 0
        buckets = gc.cell_hash(cells, grid.mask) if len(cells) else []
        for at in np.flatnonzero(grid.size[buckets] > 0) if len(cells) else []:
            # (the lane batch of this cell is at // 64; a bucket's slice is
            # visited once per cell that hashes to it)
            for i in np.flatnonzero(grid.bucket == buckets[at]):
                if np.array_equal(grid.cells[i], cells[at]):
                    d = grid.p[i] - c
                    d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                    keys.append((float(d2), int(i)))
                    hits += 1
        keys = sorted(keys)[:m]
        full = len(keys) == m
        shells.append(dict(s=s, cells=len(cells),
                           batches=(len(cells) + 63) // 64, hits=hits,
                           kth=keys[-1][0] if full and m else None,
                           b=bound(c, cc, s, lo, hi, cell, shrink=False)))
        if full and s < cover:
            b = bound(c, cc, s, lo, hi, cell)
            if b > 0.0 and keys[-1][0] < b * b:
                stop = "bound"
                break
    return [i for _, i in keys], dict(first=first, shells=shells, stop=stop)


# --------------------------------------------------------------------------
# the cases
# --------------------------------------------------------------------------
def small_n():
    """N = 5, 8 and 9 points at k = 8: m = min(k, N) is the row stride"""
    rng = np.random.default_rng(11)
    out = []
    for name, n in (("n_lt_k", 5), ("n_eq_k", 8), ("n_eq_k1", 9)):
        pts = rng.uniform(0.0, 3.0, (n, 3)).astype(np.float32)
        ctr = np.concatenate([pts[:3], rng.uniform(-1.0, 4.0, (4, 3))])
        out.append(NearestCase(name, pts, ctr.astype(np.float32), (8,)))
    return out


def k_seams():
    """the blob of _knn_cases (1500 points) and 40 of its centres, own points
    and strangers, at every k of K_EDGES"""
    pts, ctr = KC._blob()
    return NearestCase("k_seams", pts, ctr[180:220], K_EDGES)


SHELL0_K = 8


def shell0():
    """60 points within 0.2 of the middle of cell (5, 5, 5), the centre in
    that middle (b_0 = 0.5), 200 points elsewhere: the k nearest lie in the
    centre's own cell and the walk stops after shell 0."""
    rng = np.random.default_rng(12)
    mid = np.array([5.5, 5.5, 5.5])
    near = mid + rng.integers(-25, 26, (60, 3)) / 128.0
    rest = rng.uniform(0.0, 11.0, (200, 3))
    rest = rest[np.abs(rest - mid).max(1) > 0.5]
    pts = np.concatenate([rest[:100], near, rest[100:]])
    return NearestCase("shell0", pts.astype(np.float32),
                       np.array([mid], np.float32), (SHELL0_K,))


def shell_tie():
    """The 8^3 integer lattice as points AND centres, cell_size = 1.  A centre
    sits on the low faces of its own cell; after shell 1 the nearest face is at
    distance exactly 1 and the interior centres' six neighbours at d2 = 1 put
    the k-th d2 ON b_1^2 for k = 2 .. 7: the walk must take shell 2.  k = 4
    also cuts those six by index."""
    l8 = gc._lattice(8).astype(np.float32)
    return NearestCase("shell_tie", l8, l8, (4, 7), same=True)


FACE_TIE_K = 3


def face_tie():
    """cell_size = 1, centre (4.75, 4.5, 4.5): b_0 = 0.25, the +x face.  Own
    cell: points at d2 = 0.015625, 0.03125 and, with index 9, one at exactly
    0.0625 = b_0^2.  Index 2 lies ON that face from the other side (x = 5.0, in
    cell 5) at d2 = 0.0625 too: after shell 0 the list is full with its k-th d2
    equal to b_0^2, and the unscanned point wins the tie by its index."""
    c = np.array([4.75, 4.5, 4.5])
    pts = np.tile(np.array([[1.5, 1.5, 1.5]]), (12, 1)) + \
        np.arange(12)[:, None] * np.array([[0.5, 0.25, 0.125]])
    pts[2] = [5.0, 4.5, 4.5]
    pts[5] = c + [0.0, 0.125, 0.0]
    pts[7] = c + [0.0, 0.125, 0.125]
    pts[9] = c + [0.0, -0.25, 0.0]
    return NearestCase("face_tie", pts.astype(np.float32),
                       np.array([c], np.float32), (FACE_TIE_K,))


SHELL_K = 6


def _ring(s, name, seed):
    """cell_size = 1, centre in the middle of cell (12, 12, 12); the six
    nearest points sit on the axes at distance s + 0.1 -- in the six slabs of
    shell s, so in its first and its last lane batch -- everything else is at
    Chebyshev distance >= s + 1.5, on all sides (the shell is not clamped)."""
    rng = np.random.default_rng(seed)
    mid = np.array([12.5, 12.5, 12.5])
    axes = np.concatenate([np.eye(3), -np.eye(3)]) * (s + 0.1) + mid
    rest = rng.uniform(0.0, 25.0, (900, 3))
    rest = rest[np.abs(rest - mid).max(1) > s + 1.5][:400]
    pts = np.concatenate([rest[:150], axes[:3], rest[150:300], axes[3:],
                          rest[300:]])
    ctr = np.concatenate([[mid], rest[:6] + 0.01])
    return NearestCase(name, pts.astype(np.float32), ctr.astype(np.float32),
                       (SHELL_K,))


def shell2():
    return _ring(2, "shell2", 13)


def shell3():
    return _ring(3, "shell3", 14)


def far_centre():
    """a centre far outside the cloud: the walk starts at the first shell that
    reaches the cloud's cells and ends when the box covers them"""
    pts, _ = KC._blob()
    ctr = np.array([FAR_CENTRE, (-40.0, 3.0, 3.0)], np.float32)
    return NearestCase("far_centre", pts[:600], ctr, (4, 24))


DUP_COPIES = 70


def duplicates():
    """70 copies of one point among 300 others, shuffled; centres: that point,
    a point beside it and five others.  k = 5 and k = 65 < 70 cut inside the
    copies: the smallest indices win."""
    rng = np.random.default_rng(15)
    one = np.array([[2.25, 1.5, 3.0]])
    other = rng.integers(0, 5 * 64, (300, 3)) / 64.0
    pts = np.concatenate([np.repeat(one, DUP_COPIES, 0), other])
    pts = pts[rng.permutation(len(pts))]
    ctr = np.concatenate([one, one + 0.03125, other[:5]])
    return NearestCase("nn_duplicates", pts.astype(np.float32),
                       ctr.astype(np.float32), (5, 65))


def shared_bucket():
    """_knn_cases.shared_bucket(): two cells of a centre's first shells in one
    hash bucket, with a stranger between them (cell_size = its r = 1)"""
    case, info = KC.shared_bucket()
    return NearestCase("nn_shared_bucket", case.points, case.centers,
                       (2, 4, 8), cell=case.r), info


def scaled():
    pts, ctr = KC._blob()
    return NearestCase("nn_scaled", pts[:800], ctr[190:215], (16,), cell=0.7,
                       scale=[1.0, 2.0, 0.5])


def same():
    """one array as points and centres: every centre finds itself first"""
    pts = KC._blob()[0][:300]
    return NearestCase("nn_same", pts, pts, (1, 9), cell=1.5, same=True)


def blob_shuffled():
    """-> (case of the blob, case of the blob in shuffled point order, perm)
    with shuffled.points[j] == blob.points[perm[j]]"""
    pts, ctr = KC._blob()
    perm = np.random.default_rng(8).permutation(len(pts))
    return (NearestCase("nn_blob", pts, ctr[175:225], (KC.BLOB_K,)),
            NearestCase("nn_blob_shuffled", pts[perm], ctr[175:225],
                        (KC.BLOB_K,)), perm)


def all_cases():
    out = small_n() + [k_seams(), shell0(), shell_tie(), face_tie(), shell2(),
                       shell3(), far_centre(), duplicates(),
                       shared_bucket()[0], scaled(), same()] + \
        list(blob_shuffled()[:2])
    assert len(set(c.name for c in out)) == len(out)
    return out
