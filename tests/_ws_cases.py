"""Shared pieces of tests/test_gpu_ws_geometry.py (and the geometry cases of
tests/test_gpu_train_fullsize.py): the grid geometries the weights-stationary
kernels are swept over, the table that predicts which of them a kernel runs
at, CU-masked streams, input builders, float64 evaluations and the accounting
of the kernels' own stamps.  Nothing here needs a GPU at import time."""
import collections
import contextlib
import ctypes
import os
import random

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LOWEST = np.finfo(np.float32).min
WAVES = 8                 # kWsWaves
STAMP_STRIDE = 8 + 4 * 38  # kWsStampStride, int64 words per wave
MAX_SLICES = 8            # kWsMaxSlices: more slices -> no tile pool, no balance

# ---- geometries ---------------------------------------------------------------
# stream: CUs of the stream's mask (256 = the plain stream); the other fields
# are the library tunables of the same name (ws_pool_pct / ws_chunk as pool /
# chunk).
Geo = collections.namedtuple("Geo", "stream reserve xcds balance pool chunk")
DEFAULT = Geo(256, 0, 8, 1, 0, 2)
STREAMS = (256, 248, 240, 192, 128, 72, 64, 252)
RESERVES = (0, 8, 64, 128)
XCDS = (1, 2, 3, 4, 8, 16, 32, 64)   # 3 does not divide 256: falls back to 8
BALANCES = (0, 1, 2)
POOLS = ((0, 2), (15, 2), (80, 1), (80, 5))


def geo_id(g):
    return "s%d-r%d-x%d-b%d-p%dc%d" % g


def effective(g):
    """(CUs the launchers plan with, row slices they use): `ws_reserve` is
    ignored when it would leave fewer than 64 CUs, a `ws_xcds` that does not
    divide the CUs falls back to 8."""
    cus = g.stream
    if g.reserve > 0 and cus - g.reserve >= 64:
        cus -= g.reserve
    return cus, (g.xcds if cus % g.xcds == 0 else 8)


def sweep():
    """One factor at a time around the default, the geometries the issue names
    (reserve on the 240- and 72-CU streams, slice counts the CUs do not divide
    into, partitions with fewer workgroups per slice than column groups), then
    a seeded sample of 24 of the full product."""
    out = [DEFAULT]

    def add(g):
        if g not in out:
            out.append(g)
    for s in STREAMS:
        add(DEFAULT._replace(stream=s))
    for s in (256, 240, 72):
        for r in RESERVES[1:]:
            add(DEFAULT._replace(stream=s, reserve=r))
    for x in XCDS:
        add(DEFAULT._replace(xcds=x))
    for s, x in ((248, 16), (72, 16), (240, 3), (240, 4)):
        add(DEFAULT._replace(stream=s, xcds=x))     # 248, 72: 16 does not divide
    for b in BALANCES:
        add(DEFAULT._replace(balance=b))
    for p, c in POOLS:
        add(DEFAULT._replace(pool=p, chunk=c))
        add(DEFAULT._replace(pool=p, chunk=c, balance=2))
    # fewer workgroups per slice than column groups: the partition is
    # infeasible and the launchers must say so BEFORE anything is enqueued
    for s, r, x in ((64, 0, 32), (64, 0, 64), (128, 0, 64), (192, 0, 64),
                    (256, 128, 64), (192, 128, 32), (256, 64, 64)):
        add(DEFAULT._replace(stream=s, reserve=r, xcds=x))
    rng = random.Random(20240607)
    full = [Geo(s, r, x, b, p, c) for s in STREAMS for r in RESERVES
            for x in XCDS for b in BALANCES for p, c in POOLS]
    for g in rng.sample(full, 24):
        add(g)
    return out


# ---- which kernel runs where --------------------------------------------------
# (column tiles, largest column group) of every launch that goes through the
# column-group partition; car pooling (pool_ws.h, pool_ws_f16.h) has one group
# of 19 and a grid of `cus` workgroups
SHAPES = {
    ("edge_f32", 300): (19, 7), ("edge_f32", 256): (16, 8),
    ("pool_ped", 512): (32, 8),
    ("edge_bf16x3", 300): (19, 5), ("edge_bf16x3", 256): (16, 5),
    ("edge_f16x2", 300): (19, 7), ("edge_f16x2", 256): (16, 6),
}


def grouping(nt, ntmax):
    groups = -(-nt // ntmax)
    return [nt // groups + (1 if g < nt % groups else 0) for g in range(groups)]


def runs(leg, width, g):
    """Does the weights-stationary kernel of this leg run at geometry `g`?"""
    cus, xcds = effective(g)
    if leg in ("pool_car", "pool_f16x2"):
        return cus >= 8
    nt, ntmax = SHAPES[(leg, width)]
    return cus >= 64 and cus % 8 == 0 and cus // xcds >= -(-nt // ntmax)


# ---- streams and tunables -----------------------------------------------------
@contextlib.contextmanager
def masked_stream(stream_cus):
    """A torch stream restricted to `stream_cus` CUs (the plain current stream
    for the whole device), made and destroyed through the library's own two
    entries the way engine.InferenceEngine does."""
    import torch
    from pointgnn_amd import _lib
    dev = torch.device("cuda", torch.cuda.current_device())
    total = torch.cuda.get_device_properties(dev).multi_processor_count
    if stream_cus >= total:
        yield torch.cuda.current_stream(dev)
        return
    lib = _lib.load()
    h = ctypes.c_void_p()
    _lib.check(lib.pgnn_stream_create_cu_mask(0, total - stream_cus, 1,
                                              ctypes.byref(h)),
               "pgnn_stream_create_cu_mask")
    s = torch.cuda.ExternalStream(h.value, device=dev)
    try:
        yield s
    finally:
        torch.cuda.synchronize()
        for k in [k for k in _lib._SCHED_WS if k[1] == h.value]:
            del _lib._SCHED_WS[k]
        del s
        torch.cuda.empty_cache()
        _lib.check(lib.pgnn_stream_destroy(h), "pgnn_stream_destroy")


TUNABLE_DEFAULTS = {"ws_reserve": 0, "ws_xcds": 8, "ws_balance": 1,
                    "ws_pool_pct": 0, "ws_chunk": 2}


@contextlib.contextmanager
def tunables(g):
    from pointgnn_amd import _lib
    try:
        _lib.set_tunable("ws_reserve", g.reserve)
        _lib.set_tunable("ws_xcds", g.xcds)
        _lib.set_tunable("ws_balance", g.balance)
        _lib.set_tunable("ws_pool_pct", g.pool)
        _lib.set_tunable("ws_chunk", g.chunk)
        yield
    finally:
        for k, v in TUNABLE_DEFAULTS.items():
            _lib.set_tunable(k, v)


# ---- inputs -------------------------------------------------------------------
INPUTS = ("fanins", "shuffled", "ragged", "five_edges", "one_segment",
          "graph_small", "capacity")


def gold(name):
    return dict(np.load(os.path.join(GOLD, name)))


def dst_list(case, k, rng):
    """Destination column of the synthetic edge lists (test_gpu_parity.py)."""
    if case == "five_edges":     # fewer tiles than waves
        return np.array([3, 3, 3, 9, 600], np.int32)
    if case == "one_segment":    # every wave flushes the same row atomically
        return np.full(70001, 5, np.int32)
    deg = rng.choice([1, 2, 3, 5, 9, 16, 17, 40, 64, 65, 130, 300], size=k)
    dst = np.repeat(np.arange(k), deg).astype(np.int32)
    if case == "ragged":
        dst = dst[:len(dst) - len(dst) % 16 - 3]
    return dst


def _pad_capacity(edges):
    """Capacity form: a buffer longer than the list, the tail poisoned."""
    pad = np.full((len(edges) + 1000, 2), -7, np.int32)
    pad[:len(edges)] = edges
    return pad


def edge_input(case, c, seed=11):
    """P, Q, one c x c layer and an edge list for the edge stage."""
    rng = np.random.default_rng(seed)
    if case == "graph_small":
        g = gold("graph_small.npz")
        edges = g["ref_edges1"].astype(np.int32)
        k = int(g["kp_xyz"].shape[0])
        assert len(edges) >= 70000
    else:
        k = 700
        dst = dst_list(case, k, rng)
        src = rng.integers(0, k, dst.shape[0]).astype(np.int32)
        edges = np.stack([src, dst], axis=1)
        if case == "shuffled":
            edges = edges[rng.permutation(len(edges))]
    wq = 16 * ((c + 15) // 16)
    k_cap = k + 50 if case == "capacity" else k
    p = np.zeros((k_cap, wq), np.float32)
    q = np.zeros((k_cap, wq), np.float32)
    p[:, :c] = rng.standard_normal((k_cap, c))
    q[:, :c] = 0.3 * rng.standard_normal((k_cap, c))
    w = (rng.standard_normal((c, c)) / np.sqrt(c)).astype(np.float32)
    b = (0.1 * rng.standard_normal(c)).astype(np.float32)
    d = edges[:, 1]
    return dict(case=case, c=c, wq=wq, k=k, k_cap=k_cap, p=p, q=q, w=w, b=b,
                edges=edges, n_live=len(edges),
                buf=_pad_capacity(edges) if case == "capacity" else edges,
                sorted=int(bool(np.all(d[1:] >= d[:-1]))))


def edge_f64(inp):
    """float64 evaluation of the edge stage on the fp32 inputs."""
    p, q, w, b, c, k = (inp[n] for n in ("p", "q", "w", "b", "c", "k"))
    edges = inp["edges"]
    src, dst = edges[:, 0].astype(np.int64), edges[:, 1].astype(np.int64)
    ok = (dst >= 0) & (dst < k)
    out = np.full((k, c), LOWEST, np.float64)
    w64, b64 = w.astype(np.float64), b.astype(np.float64)
    for lo in range(0, len(edges), 65536):
        s, d, m = src[lo:lo + 65536], dst[lo:lo + 65536], ok[lo:lo + 65536]
        h1 = np.maximum(p[s, :c] - q[np.where(m, d, 0), :c], 0)  # fp32, as the kernel
        rows = np.maximum(h1.astype(np.float64) @ w64 + b64, 0)
        np.maximum.at(out, d[m], rows[m])
    return out


POOL_WIDTHS = {"car": [4, 32, 64, 128, 300], "ped": [4, 32, 64, 128, 256, 512]}


def pool_input(case, chain, seed=12):
    """Points, keypoints, a point MLP and an edge list for PointSetPooling."""
    rng = np.random.default_rng(seed)
    if case == "graph_small":
        g = gold("graph_small.npz")
        edges = g["ref_edges0"].astype(np.int32)
        xyz = g["xyz"].astype(np.float32)
        inten = g["intensity"].astype(np.float32).reshape(len(xyz), -1)
        kp = g["kp_idx"].reshape(-1).astype(np.int32)
        k = len(kp)
        assert len(edges) >= 70000
    else:
        k, n_pts = 700, 6000
        dst = dst_list(case, k, rng)
        src = rng.integers(0, n_pts, dst.shape[0]).astype(np.int32)
        edges = np.stack([src, dst], axis=1)
        if case == "shuffled":
            edges = edges[rng.permutation(len(edges))]
        xyz = rng.standard_normal((n_pts, 3)).astype(np.float32)
        inten = rng.random((n_pts, 1)).astype(np.float32)
        kp = rng.choice(n_pts, k, replace=False).astype(np.int32)
    widths = POOL_WIDTHS[chain]
    layers = []
    for a, b_ in zip(widths[:-1], widths[1:]):
        w = (rng.standard_normal((a, b_)) * np.sqrt(2.0 / a)).astype(np.float32)
        layers.append((w, (0.1 * rng.standard_normal(b_)).astype(np.float32), 0))
    k_cap = k + 50 if case == "capacity" else k
    kp_buf = np.zeros(k_cap, np.int32)
    kp_buf[:k] = kp
    d = edges[:, 1]
    return dict(case=case, chain=chain, k=k, k_cap=k_cap, xyz=xyz, inten=inten,
                kp=kp, kp_buf=kp_buf, layers=layers, edges=edges,
                n_live=len(edges), c=widths[-1],
                wq=16 * ((widths[-1] + 15) // 16),
                buf=_pad_capacity(edges) if case == "capacity" else edges,
                sorted=int(bool(np.all(d[1:] >= d[:-1]))))


def pool_f64(inp):
    """float64 evaluation of the pooling stage on the fp32 inputs."""
    edges, k, xyz, kp = inp["edges"], inp["k"], inp["xyz"], inp["kp"]
    src, dst = edges[:, 0].astype(np.int64), edges[:, 1].astype(np.int64)
    ok = (dst >= 0) & (dst < k)
    d = np.where(ok, dst, 0)
    x = np.concatenate([inp["inten"][src], xyz[src] - xyz[kp[d]]],
                       axis=1).astype(np.float64)        # fp32 inputs
    for w, b_, _ in inp["layers"]:
        x = np.maximum(x @ w.astype(np.float64) + b_.astype(np.float64), 0)
    out = np.full((k, inp["c"]), LOWEST, np.float64)
    np.maximum.at(out, dst[ok], x[ok])
    return out


# ---- the kernels' own stamps --------------------------------------------------
def check_edge_stamps(st, n_wt, cus, xcds, sizes, balanced, account=True):
    """`st`: int64 [waves + 8, STAMP_STRIDE] read back after an edge_ws_kernel
    launch, the 8 rows behind the grid included; account: the launch had no
    tile pool, so the static ranges are all the work.  Every wave
    of a grid of cus / xcds * xcds workgroups wrote its header -- word 4 its
    static range length, word 5 its column tiles + 100 * its row slice -- and
    the lengths add up so that every (row tile, column group) has exactly one
    owner: per slice and group the slice's tile count (static form), per group
    all tiles (balanced form).  A tile computed twice cannot show in any
    output (max is idempotent); it shows here.

    A slice's workgroups are its groups in order, and groups of equal tile
    count carry the same stamp, so the sums are taken per run of equal stamps:
    the running sum of a run of m groups must pass 1x, 2x .. mx the slice's
    tile count AT workgroup boundaries.  Nothing else about how many
    workgroups a group gets is assumed: the test pins the contract, not one
    split."""
    per_slice = cus // xcds
    grid = per_slice * xcds
    assert st.shape[0] == grid * WAVES + 8
    assert (st[:grid * WAVES, 0] != 0).all(), \
        "%d of %d waves wrote no stamp" % ((st[:grid * WAVES, 0] == 0).sum(),
                                           grid * WAVES)
    assert not st[grid * WAVES:].any(), "stamps behind the expected grid"
    st = st[:grid * WAVES]
    blk = np.repeat(np.arange(grid), WAVES)
    length, ntg, slc = st[:, 4], st[:, 5] % 100, st[:, 5] // 100
    assert np.array_equal(slc, blk % xcds), "row slice of a workgroup"
    assert sorted(set(ntg.tolist())) == sorted(set(sizes)), \
        "column grouping %r, stamped %r" % (sizes, sorted(set(ntg.tolist())))
    assert (length >= 0).all()
    mult = collections.Counter(sizes)
    if balanced and account:
        for v, m in mult.items():
            got = int(length[ntg == v].sum())
            assert got == m * n_wt, \
                "groups of %d column tiles cover %d row tiles, not %d x %d" % (
                    v, got, m, n_wt)
    for s in range(xcds):
        tiles = n_wt * (s + 1) // xcds - n_wt * s // xcds
        sel = slc == s               # in (local workgroup, wave) order
        order = ntg[sel][::WAVES]
        assert (np.diff(order) <= 0).all(), "groups of a slice out of order"
        for v, m in mult.items():
            run = length[sel][ntg[sel] == v]
            assert len(run) % WAVES == 0 and len(run) >= m * WAVES, \
                "slice %d: %d waves for %d groups" % (s, len(run), m)
            if balanced or not account:
                continue
            at_wg = np.cumsum(run)[WAVES - 1::WAVES]
            assert at_wg[-1] == m * tiles and all(
                j * tiles in at_wg for j in range(1, m + 1)), \
                "slice %d, groups of %d column tiles: range lengths sum to " \
                "%r at the workgroup boundaries, the slice has %d row tiles" % (
                    s, v, at_wg.tolist(), tiles)


def check_pool_stamps(st, n_wt, cus, account=True):
    """pool_ws_kernel: a grid of `cus` workgroups, one column group of 19, the
    static ranges add up to the tile count."""
    assert st.shape[0] == cus * WAVES + 8
    assert (st[:cus * WAVES, 0] != 0).all(), "waves without a stamp"
    assert not st[cus * WAVES:].any(), "stamps behind the expected grid"
    st = st[:cus * WAVES]
    assert (st[:, 5] == 19).all()
    assert (st[:, 4] >= 0).all()
    assert not account or int(st[:, 4].sum()) == n_wt, \
        "static ranges cover %d row tiles of %d" % (st[:, 4].sum(), n_wt)
