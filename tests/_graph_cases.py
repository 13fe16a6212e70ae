"""Clouds for the structural tests of the graph builder
(tests/test_graph_cases_cpu.py proves them, tests/test_gpu_graph_structure.py
runs them on the device).

Every cloud is deterministic and aims at one branch of csrc/graph.hip,
csrc/sort.hip or the launches of csrc/kdtree.hip that a random cloud reaches
only by luck: a candidate total at a chunk seam, a 64-cell box, two box cells
in one bucket, two voxels in one bucket, a sort or scan tile edge.

To AIM, this module restates the builder's bucket function in NumPy:

  hash_bits    graph.hip:895-899 `hash_bits`      (host helper, 10 .. 22 bits)
  cell_hash    graph.hip:36-42   `cell_hash`      (uint32 products, h ^= h >> 15)
  rcell_of     graph.hip:58-60   `rcell_of`       floor(v * (1 / r))
  box_of       graph.hip:216, :226-236 (radius_query_kernel), the `rr` widening:
               rr = r * (1 + 1e-9) + 1e-300, cells rcell(c - rr) .. rcell(c + rr),
               lane order (z, y, x)
  vox_index    graph.hip:47-49 `cell_of`, :74-77 `vox_cell` mode 0 ('center':
               open3d 0.7, origin = cloud minimum - voxel / 2, :1593)
  from_level   graph.hip:726-784 voxel_nn_from_kernel's cube growth and `face`
               stop test

The restatement only CHARACTERISES a case (which branch it reaches); expected
edges and keypoints always come from oracle/graph_oracle.py.  If the device
hash changes, the GPU tests still hold the kernels to the oracle -- they only
lose their aim, and tests/test_graph_cases_cpu.py says so.
"""
import numpy as np

# --------------------------------------------------------------------------
# the restated bucket function
# --------------------------------------------------------------------------
def hash_bits(n):
    b = 10
    while b < 22 and (1 << b) < 2 * n:
        b += 1
    return b


def cell_hash(cells, mask):
    """cells: int array [..., 3] -> uint32 bucket"""
    c = np.asarray(cells).astype(np.int64)
    m32 = np.uint64(0xFFFFFFFF)
    u = (c & 0xFFFFFFFF).astype(np.uint64)          # two's complement uint32
    h = ((u[..., 0] * np.uint64(73856093)) & m32) ^ \
        ((u[..., 1] * np.uint64(19349663)) & m32) ^ \
        ((u[..., 2] * np.uint64(83492791)) & m32)
    h ^= h >> np.uint64(15)
    return (h & np.uint64(mask)).astype(np.int64)


def _scaled(a, scale):
    a = np.asarray(a).astype(np.float64)            # the widening is exact
    if scale is not None:
        a = a / np.asarray(scale, np.float64)       # graph_gen.py:203-206
    return a


def rcell_of(v, r):
    return np.floor(np.asarray(v, np.float64) * (1.0 / float(r))).astype(np.int64)


def box_of(center, r):
    """-> (lo[3], hi[3]) cell bounds of the box a query at `center` scans"""
    r = float(r)
    rr = r * (1.0 + 1e-9) + 1e-300
    c = np.asarray(center, np.float64)
    return rcell_of(c - rr, r), rcell_of(c + rr, r)


def box_cells(center, r):
    """the box's cells in the kernel's lane order (z, y, x)"""
    lo, hi = box_of(center, r)
    zz, yy, xx = np.meshgrid(np.arange(lo[2], hi[2] + 1),
                             np.arange(lo[1], hi[1] + 1),
                             np.arange(lo[0], hi[0] + 1), indexing="ij")
    return np.stack([xx.ravel(), yy.ravel(), zz.ravel()], axis=1)


class RadiusGrid(object):
    """The cell grid of one radius graph: bucket of every point."""

    def __init__(self, points, r, scale=None):
        self.r = float(r)
        self.p = _scaled(points, scale)
        self.scale = scale
        self.mask = (1 << hash_bits(len(self.p))) - 1
        self.cells = rcell_of(self.p, self.r)
        self.bucket = cell_hash(self.cells, self.mask)
        self.size = np.bincount(self.bucket, minlength=self.mask + 1)

    def query(self, center):
        """-> (n_cells, candidate total, buckets of the box cells)"""
        c = _scaled(np.asarray(center).reshape(1, 3), self.scale)[0]
        b = cell_hash(box_cells(c, self.r), self.mask)
        return len(b), int(self.size[b].sum()), b

    def profile(self, centers):
        """-> (n_cells[Q], candidate totals[Q])"""
        out = [self.query(c)[:2] for c in np.asarray(centers)]
        return (np.array([o[0] for o in out]), np.array([o[1] for o in out]))


def exact_r_pairs(points, centers, r, scale=None):
    """number of (point, centre) pairs whose float64 squared distance is
    exactly r * r (the inclusive edge of the predicate)"""
    p, c = _scaled(points, scale), _scaled(centers, scale)
    n = 0
    for q0 in range(0, len(c), 256):
        d = c[q0:q0 + 256, None, :] - p[None]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        n += int((d2 == float(r) * float(r)).sum())
    return n


def vox_index(points, voxel, anchor=None):
    """open3d-0.7 voxel index ('center' keypoints; vox_cell mode 0):
    floor((p - (min - voxel / 2)) / voxel), float64; `anchor`: the cloud whose
    minimum places the grid (default: `points`)"""
    p = np.asarray(points).astype(np.float64)
    a = p if anchor is None else np.asarray(anchor).astype(np.float64)
    origin = a.min(axis=0) - float(voxel) * 0.5
    return np.floor((p - origin) / float(voxel)).astype(np.int64), origin


class RadiusCase(object):
    def __init__(self, name, points, centers, r, scale=None):
        self.name, self.points, self.centers = name, points, centers
        self.r, self.scale = r, scale

    def __repr__(self):
        return self.name


# --------------------------------------------------------------------------
# chunk_sweep
# --------------------------------------------------------------------------
SWEEP_M = tuple(range(1, 201)) + (255, 256, 257)
# the off-middle centre of every cluster, relative to its cell: a third of the
# cell lies farther than r = 1 from it
SWEEP_OFF = 0.0625


def chunk_sweep():
    """One cloud, r = 1.  Cluster k holds SWEEP_M[k] distinct points inside ONE
    cell, and that cell's 26 neighbours and every bucket they hash to are
    empty: the candidate total of a centre inside the cell is exactly m, in a
    box of 27 cells.  Every cluster has two centres: 2k in the middle of the
    cell (the whole cell is within r: fan-in m) and 2k + 1 near the cell's low
    corner (about a third of the cluster is farther than r: candidates that
    are not neighbours, on either side of every chunk seam).

    -> (RadiusCase, m of every centre [2 * len(SWEEP_M)])"""
    rng = np.random.default_rng(20260)
    n = int(np.sum(SWEEP_M))
    mask = (1 << hash_bits(n)) - 1
    nb = np.stack(np.meshgrid(*[np.arange(-1, 2)] * 3, indexing="ij"),
                  -1).reshape(-1, 3)
    used = set()          # buckets of every placed box
    own = set()           # buckets that hold a cluster
    cells = []
    for m in SWEEP_M:
        while True:
            cell = rng.integers(1, 60, 3)
            b = cell_hash(cell + nb, mask)
            me = int(cell_hash(cell, mask))
            others = set(int(x) for x in b) - {me}
            if len(set(int(x) for x in b)) == 27 and me not in used and \
                    not (others & own) and me not in own:
                break
        used |= set(int(x) for x in b)
        own.add(me)
        cells.append(cell)
    pts, ctr, ms = [], [], []
    for m, cell in zip(SWEEP_M, cells):
        # distinct points strictly inside the cell, multiples of 2^-10
        q = rng.choice(1022 ** 2, size=m, replace=False)
        frac = np.stack([(q % 1022 + 1), (q // 1022 + 1),
                         rng.integers(1, 1023, m)], 1) / 1024.0
        pts.append(cell + frac)
        ctr.append(cell + 0.5)
        ctr.append(cell + SWEEP_OFF)
        ms += [m, m]
    order = rng.permutation(n)      # clusters interleaved in index order
    points = np.concatenate(pts)[order].astype(np.float32)
    return (RadiusCase("chunk_sweep", points,
                       np.array(ctr, np.float32), 1.0), np.array(ms))


# --------------------------------------------------------------------------
# lattices
# --------------------------------------------------------------------------
def _lattice(n):
    g = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1)
    return g.reshape(-1, 3)


def lattices():
    """Integer and decimal lattices: centres ON cell faces (64-cell boxes) and
    neighbours at distance exactly r.  float32 and float64 forms; a float32
    case is also run widened by the device tests."""
    l8, l12 = _lattice(8), _lattice(12)
    out = []
    for dt, tag in ((np.float32, "f32"), (np.float64, "f64")):
        out.append(RadiusCase("lattice8_r1_" + tag, l8.astype(dt),
                              l8.astype(dt), 1.0))
        out.append(RadiusCase("lattice12_r5_" + tag, l12.astype(dt),
                              l12[::37].astype(dt), 5.0))
        out.append(RadiusCase("lattice12_scaled_" + tag, l12.astype(dt),
                              l12[::37].astype(dt), 2.5, [1.0, 2.0, 0.5]))
        out.append(RadiusCase("lattice12_r5_negative_" + tag,
                              (l12 - 10).astype(dt), (l12[::37] - 10).astype(dt),
                              5.0))
        out.append(RadiusCase("lattice8_r1_negative_" + tag,
                              (l8 - 5).astype(dt), (l8 - 5).astype(dt), 1.0))
    # the decimal lattice: 0.1 * i has no exact faces
    f32 = (np.float32(0.1) * l8.astype(np.float32)).astype(np.float32)
    out.append(RadiusCase("lattice8_tenth_f32", f32, f32,
                          float(np.float32(0.1))))
    f64 = 0.1 * l8.astype(np.float64)
    out.append(RadiusCase("lattice8_tenth_f64", f64, f64, 0.1))
    return out


# --------------------------------------------------------------------------
# shared_bucket_box
# --------------------------------------------------------------------------
def shared_bucket_box(n_boxes=4, n_fill=150):
    """A few hundred points (hash_bits at its floor of 10), r = 1.  For each of
    `n_boxes` centres two cells A, B of its 27-cell box hash to ONE bucket;
    both hold true neighbours, and a point of a far cell F of the same bucket
    (not a neighbour) sits between them in index order.  The bucket's slice is
    therefore walked twice, once as A and once as B: every point of it must be
    accepted under exactly one of them.

    -> (RadiusCase, info: list of dict(center, a, b, far, idx_a, idx_b, idx_far))"""
    rng = np.random.default_rng(57)
    per = 3
    n = n_boxes * (2 * per + 1) + n_fill
    assert hash_bits(n) == 10
    mask = 1023
    nb = np.stack(np.meshgrid(*[np.arange(-1, 2)] * 3, indexing="ij"),
                  -1).reshape(-1, 3)
    rows, info, ctr = [], [], []
    taken = set()
    while len(info) < n_boxes:
        cell = rng.integers(-40, 40, 3)
        box = cell + nb
        b = cell_hash(box, mask)
        vals, cnt = np.unique(b, return_counts=True)
        if not (cnt == 2).any() or (cnt > 2).any():
            continue
        bucket = int(vals[np.argmax(cnt == 2)])
        if bucket in taken:
            continue
        ia, ib = np.flatnonzero(b == bucket)
        a, bb = box[ia], box[ib]
        c = cell + 0.5
        # true neighbours of c inside A and inside B (multiples of 2^-8)
        def inside(cc):
            got = []
            while len(got) < per:
                p = cc + rng.integers(1, 255, 3) / 256.0
                if ((p - c) ** 2).sum() < 0.9:
                    got.append(p)
            return got
        if any(np.all(np.abs(x - cell) == 1) for x in (a, bb)):
            continue      # a corner cell has no room within 0.9 r^2
        # a far cell of the same bucket
        while True:
            far = cell + rng.integers(5, 30, 3) * rng.choice([-1, 1], 3)
            if int(cell_hash(far, mask)) == bucket:
                break
        taken.add(bucket)
        pa, pb = inside(a), inside(bb)
        pf = far + rng.integers(1, 255, 3) / 256.0
        base = len(rows)
        # index order: A, far, B, A, B, A, B
        seq = [pa[0], pf, pb[0]]
        for k in range(1, per):
            seq += [pa[k], pb[k]]
        rows += seq
        ia_ = [base, base + 3, base + 5]
        ib_ = [base + 2, base + 4, base + 6]
        info.append(dict(center=c, a=a, b=bb, far=far, bucket=bucket,
                         idx_a=ia_, idx_b=ib_, idx_far=base + 1))
        ctr.append(c)
    fill = rng.uniform(-42, 42, (n_fill, 3))
    points = np.concatenate([np.array(rows), fill]).astype(np.float32)
    # the filler doubles as centres: ordinary boxes beside the aimed ones
    centers = np.concatenate([np.array(ctr), fill[:40]]).astype(np.float32)
    return RadiusCase("shared_bucket_box", points, centers, 1.0), info


# --------------------------------------------------------------------------
# sort_scan_edges
# --------------------------------------------------------------------------
SORT_POINTS = (2047, 2048, 2049, 4097, 32768, 32769)
SCAN_CENTERS = (1, 4095, 4096, 4097, 8193)


def _sparse(rng, n, per_ball=3.0):
    """uniform cloud with about `per_ball` points per unit ball"""
    side = (n * 4.18879 / per_ball) ** (1.0 / 3.0)
    return rng.uniform(0.0, side, (n, 3)).astype(np.float32)


def sort_scan_edges():
    """Uniform sparse clouds, r = 1, at the sort tile (2048 keys), at the step
    from 16 to 17 key bits (2 -> 3 radix passes: the sorted keys end in the
    other ping-pong buffer), at the scan tile (4096 counts) and at the thread
    that writes the grand total out[n].  Large point counts come with few
    centres and large centre counts with few points."""
    out = []
    for n in SORT_POINTS:
        rng = np.random.default_rng(n)
        p = _sparse(rng, n)
        c = p[rng.choice(n, 61, replace=False)] + \
            rng.uniform(-0.3, 0.3, (61, 3)).astype(np.float32)
        out.append(RadiusCase("points%d" % n, p, c.astype(np.float32), 1.0))
    for q in SCAN_CENTERS:
        rng = np.random.default_rng(100000 + q)
        p = _sparse(rng, 700)
        side = float(p.max())
        c = rng.uniform(0.0, side, (q, 3)).astype(np.float32)
        out.append(RadiusCase("centers%d" % q, p, c, 1.0))
    return out


# --------------------------------------------------------------------------
# fanin_caps
# --------------------------------------------------------------------------
FANIN = (63, 64, 65, 128, 129)
CAPS = (1, 63, 64, 65)


def fanin_caps():
    """The chunk_sweep cloud: its mid-cell centres have fan-in exactly m.
    -> (RadiusCase, {fan-in: centre index}, CAPS)"""
    case, ms = chunk_sweep()
    where = {f: 2 * SWEEP_M.index(f) for f in FANIN}
    return case, where, CAPS


# --------------------------------------------------------------------------
# voxel_bucket_pairs
# --------------------------------------------------------------------------
VOXEL = 1.0
# jitter of the 'random' mode runs: below 0.5 voxel on every axis, so a point
# of [i + 0.05, i + 0.45) keeps the index i
# (the first draw of numpy.random after seed(JITTER_SEED): the oracle's
# keypoints_random draws it itself, graph_gen.py:126-128)
JITTER_SEED = 33
JITTER = tuple(np.random.RandomState(JITTER_SEED).random_sample(3))
assert 0.05 < min(JITTER) and max(JITTER) < 0.5


def _in_voxel(rng, v, m):
    """m points with voxel index v under BOTH grids the keypoint modes use
    when the cloud's minimum is the origin: 'center' floor(p + 0.5), 'random'
    floor(p) and floor(p + JITTER)"""
    return v + rng.integers(13, 115, (m, 3)) / 256.0     # [0.05, 0.45)


def voxel_bucket_pairs():
    """Pairs of voxels (V1, V2) that hash to ONE bucket, alone in it.  Their
    points alternate in index order (V1, V2, V1, ...: the stable sort then
    alternates their slots), with a = 1..9 members in V1 and b = 1..9 in V2 --
    across the 4-wide member loop and its scalar tail; V2's leader is found by
    the walk over the earlier slots.  'late' pairs put five members of V1 in
    front of V2's first.  Point 0 is the origin: it anchors both grids.

    -> (points float32 [n,3], pairs: list of dict(v1, v2, idx1, idx2, late))"""
    rng = np.random.default_rng(4242)
    combos = [(a, b, False) for a in range(1, 10) for b in range(1, 10)]
    combos += [(a, b, True) for a in range(6, 10) for b in range(1, 10)]
    n = 1 + sum(a + b for a, b, _ in combos)
    mask = (1 << hash_bits(n)) - 1
    side = 18
    vox = _lattice(side) + 2                       # indices 2 .. 19
    h = cell_hash(vox, mask)
    order = np.argsort(h, kind="stable")
    groups = np.split(order, np.flatnonzero(np.diff(h[order])) + 1)
    groups = [g for g in groups if len(g) >= 2 and h[g[0]] != 0]  # 0: origin's
    pick = rng.permutation(len(groups))
    assert len(groups) >= len(combos)
    rows = [np.zeros(3)]
    pairs = []
    for (a, b, late), gi in zip(combos, pick):
        g = groups[gi]
        v1, v2 = vox[g[0]], vox[g[1]]
        p1, p2 = _in_voxel(rng, v1, a), _in_voxel(rng, v2, b)
        seq = [(1, k) for k in range(5)] if late else []
        i1, i2 = len(seq), 0
        while i1 < a or i2 < b:
            if i1 < a:
                seq.append((1, i1))
                i1 += 1
            if i2 < b:
                seq.append((2, i2))
                i2 += 1
        base = len(rows)
        idx1 = [base + s for s, (w, _) in enumerate(seq) if w == 1]
        idx2 = [base + s for s, (w, _) in enumerate(seq) if w == 2]
        rows += [p1[k] if w == 1 else p2[k] for w, k in seq]
        pairs.append(dict(v1=v1, v2=v2, idx1=idx1, idx2=idx2, late=late))
    points = np.array(rows).astype(np.float32)
    assert len(points) == n
    return points, pairs


# --------------------------------------------------------------------------
# nn_cases
# --------------------------------------------------------------------------
def nn_face_cloud():
    """Voxel (2,2,2) holds two points near opposite corners; the nearest point
    to their centroid lies just across a face, in voxel (3,2,2)."""
    return np.array([[0, 0, 0],
                     [1.5625, 1.5625, 1.5625], [2.4375, 2.4375, 2.4375],
                     [2.5625, 2.0, 2.0]], np.float32)


def nn_tie_cloud():
    """The centroid of voxel (4,4,4) is exactly equidistant from a point of
    voxel (3,4,4) and a point of voxel (5,4,4), both nearer than its own."""
    return np.array([[0, 0, 0],
                     [3.5625, 3.5625, 4.0], [4.4375, 4.4375, 4.0],
                     [4.5625, 4.0, 4.0], [3.4375, 4.0, 4.0]], np.float32)


def nn_corner_cloud(sign):
    """Voxel (4,4,4) holds three points near three of its corners; the nearest
    point to their centroid lies across the (sign, sign, sign) CORNER, in the
    last (sign = +1: lane 26) or first (sign = -1: lane 0) of the 27 voxels
    the kernel concatenates -- the candidate the scan total must still cover.
    Point 4 is that one."""
    v = np.array([4.0, 4.0, 4.0])
    own = v + sign * 0.4375 * np.array([[1, 1, -1], [1, -1, 1], [-1, 1, 1]])
    far = v + sign * 0.5078125 * np.ones(3)
    return np.concatenate([np.zeros((1, 3)), own, far[None]]).astype(np.float32)


NN_TOTALS = (63, 64, 65, 129)


def nn_neighbourhood_cloud(total):
    """`total` points spread over the 27 voxels round a central one, whose 27
    buckets are distinct and hold nothing else: the central voxel's leader
    walks exactly `total` candidates.  -> (points, central voxel index)"""
    rng = np.random.default_rng(900 + total)
    n = total + 1
    mask = (1 << hash_bits(n)) - 1
    nb = np.stack(np.meshgrid(*[np.arange(-1, 2)] * 3, indexing="ij"),
                  -1).reshape(-1, 3)
    while True:
        v = rng.integers(3, 40, 3)
        b = cell_hash(v + nb, mask)
        if len(set(b.tolist())) == 27 and \
                int(cell_hash(np.zeros(3, np.int64), mask)) not in b.tolist():
            break
    # every voxel of the neighbourhood is occupied, the rest go anywhere in it
    which = np.concatenate([np.arange(27), rng.integers(0, 27, total - 27)])
    rng.shuffle(which)
    pts = (v + nb[which]) + rng.integers(-127, 127, (total, 3)) / 256.0
    return np.concatenate([np.zeros((1, 3)), pts]).astype(np.float32), v


FROM_WANT = {"r1": 1, "r2": 2, "r3": 3, "fallback": 4, "corner_then_r2": 2}


def nn_from_cloud():
    """Second-level search (voxel_nn_from_kernel), voxel 1.  `points` has one
    point per voxel, so every centroid is that point.  `base`:
      r1              a base point 0.75 away                      -> r = 1
      r2              nothing in the 27 cells, one 2.0 away       -> r = 2
      r3              nothing in the 125 cells, one 3.0 away      -> r = 3
      fallback        nothing within the 343 cells (the nearest base point is
                      the origin's, far away)                     -> every point
      corner_then_r2  a base point in a CORNER cell of the r = 1 cube, 2.25
                      away (farther than the cube's face at 1.5), and a nearer
                      one 1.75 away in the r = 2 shell: stopping at r = 1
                      would return the wrong point
    -> (points, base, names of the centroids by point index)"""
    names = ["origin", "r1", "r2", "r3", "fallback", "corner_then_r2"]
    points = np.array([[0, 0, 0], [8, 8, 8], [30, 8, 8], [8, 30, 8],
                       [60, 60, 60], [8, 8, 30]], np.float32)
    base = np.array([[0.25, 0, 0],
                     [8.75, 8, 8],
                     [30, 10, 8],
                     [8, 30, 5],
                     [9.25, 9.25, 31.375], [8, 6.25, 30]], np.float32)
    return points, base, names


def from_level(points, base, voxel, i):
    """The cube size at which voxel_nn_from_kernel decides the centroid of the
    (single-point) voxel of points[i]: 1, 2, 3, or 4 for the every-point
    fallback.  -> (level, index of the best base point at that level)"""
    voxel = float(voxel)
    vc, origin = vox_index(points, voxel)
    vb = np.floor((np.asarray(base, np.float64) - origin) / voxel).astype(np.int64)
    c = np.asarray(points[i], np.float64)
    b64 = np.asarray(base, np.float64)
    d = b64 - c
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    for r in (1, 2, 3):
        inside = np.all(np.abs(vb - vc[i]) <= r, axis=1)
        lo = origin + (vc[i] - r) * voxel
        hi = origin + (vc[i] + r + 1) * voxel
        face = min((c - lo).min(), (hi - c).min()) - 1.0e-9 * voxel
        if inside.any():
            best = d2[inside].min()
            if face > 0.0 and best < face * face:
                return r, int(np.flatnonzero(inside & (d2 == best))[0])
    return 4, int(np.argmin(d2))
