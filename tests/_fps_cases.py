"""The farthest-point sampling contract (include/pointgnn_hip.h,
pgnn_farthest_first; dataset/kitti_dataset.py:630-641) restated in NumPy, and
the clouds that aim at the seams of csrc/fps.hip.

tests/test_fps_cases_cpu.py proves that the restatement is the reference's own
function and that every cloud reaches what it is named for;
tests/test_gpu_farthest.py holds the device to `fps_reference` with `==` on all
of them, in float32 and in float64.

Sizes come from the header's PGNN_FPS_* numbers: the workgroup size (a thread
owns the points tid, tid + BLOCK, ...) and the two resident limits (float32 /
float64), above which a segment streams its coordinates every round.
"""
import collections
import functools
import os
import sys
import types

import numpy as np

import pointgnn_amd  # noqa: F401
from pointgnn_amd import _header

import _refimport

_C = _header.constants()
BLOCK = _C["PGNN_FPS_BLOCK"]
RESIDENT = {np.dtype(np.float32): _C["PGNN_FPS_RESIDENT"],
            np.dtype(np.float64): _C["PGNN_FPS_RESIDENT_F64"]}
RES32, RES64 = _C["PGNN_FPS_RESIDENT"], _C["PGNN_FPS_RESIDENT_F64"]
K_MAX = 256           # every case but none: tests stay quick
K_STREAM = 48         # the streaming-tier cases (<= 64)
DTYPES = (np.float32, np.float64)


# --------------------------------------------------------------------------
# the restatement
# --------------------------------------------------------------------------
def dist(p0, pts):
    """:631 with the contract's parenthesisation; float64 rows in"""
    d = p0[None, :] - pts
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def fps_trace(pts, k, start):
    """-> (idx int32 [k], num_distinct, multiplicity of the maximum in every
    round 1..k-1).  An empty cloud gives -1 and 0."""
    n = len(pts)
    if n == 0:
        return np.full(k, -1, np.int32), 0, []
    p = np.asarray(pts).astype(np.float64)      # widening float32 is exact
    idx = np.zeros(k, np.int32)
    if k == 0:
        return idx, 0, []
    idx[0] = start
    d = dist(p[start], p)
    nd, mult = k, []
    for i in range(1, k):
        j = int(np.argmax(d))
        if d[j] == 0 and nd == k:
            nd = i
        mult.append(int((d == d[j]).sum()))
        idx[i] = j
        d = np.minimum(d, dist(p[j], p))
    return idx, nd, mult


def fps_reference(pts, k, start):
    idx, nd, _ = fps_trace(pts, k, start)
    return idx, nd


def rows_of(pts, idx):
    """the picked rows in the cloud's dtype; zero rows where idx is -1"""
    pts = np.asarray(pts)
    out = np.zeros((len(idx), 3), pts.dtype)
    ok = np.asarray(idx) >= 0
    out[ok] = pts[np.asarray(idx)[ok]]
    return out


# --------------------------------------------------------------------------
# the reference's own function
# --------------------------------------------------------------------------
def reference_kitti_dataset():
    """The reference's dataset/kitti_dataset.py under empty `open3d` / `cv2`
    stubs (its top-level imports, unused by farthest_first), or None where the
    reference is absent."""
    root = _refimport.REF_ROOT
    if not os.path.isfile(os.path.join(root, "dataset", "kitti_dataset.py")):
        return None
    for name in ("open3d", "cv2"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    if root not in sys.path:
        sys.path.insert(0, root)
    try:
        from dataset import kitti_dataset  # noqa: the reference's module
    finally:
        sys.path.remove(root)
    return kitti_dataset


# --------------------------------------------------------------------------
# the clouds
# --------------------------------------------------------------------------
class Case(collections.namedtuple("Case", "name points k start expect")):
    """points: float64 master array; cast(dtype) is what a run sees (the
    float32 run rounds it, the float64 run keeps every bit).  expect: picks
    the case was built to produce, {round: index}, or None."""

    def cast(self, dtype):
        return np.ascontiguousarray(self.points.astype(dtype))

    @property
    def n(self):
        return len(self.points)


def blob(n, seed, spread=10.0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, 3)) * spread


def with_outliers(n, seed, where):
    """A unit blob with far points at the indices `where`, farther and
    farther apart: started at a blob point, the picks of rounds 1, 2, ... are
    exactly `where` in order."""
    pts = blob(n, seed, spread=1.0)
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1],
                     [0, 0, -1]], np.float64)
    for r, i in enumerate(where):
        # round r + 1's winner: the farthest from everything picked so far
        pts[i] = axes[r % 6] * 1000.0 * 0.5 ** r
    return pts


def _size_cases():
    out = []
    for n in (1, 2, 63, 64, 65):
        out.append(Case("n%d" % n, blob(n, n), n + 3, n // 2, None))
    for n in (BLOCK - 1, BLOCK, BLOCK + 1):
        out.append(Case("block%+d" % (n - BLOCK), blob(n, n), 64, n // 3,
                        None))
    for lim, tag in ((RES64, "res64"), (RES32, "res32")):
        for n in (lim - 1, lim, lim + 1):
            out.append(Case("%s%+d" % (tag, n - lim), blob(n, n), 12, n - 1,
                            None))
    return out


def _k_and_start_cases():
    n = 65
    pts = blob(n, 101)
    out = [Case("k1", pts, 1, 7, None), Case("kN", pts, n, 7, None),
           Case("kN+3", pts, n + 3, 7, None)]
    n = BLOCK + 1
    pts = blob(n, 102)
    for tag, s in (("first", 0), ("last", n - 1), ("middle", n // 2)):
        out.append(Case("start_" + tag, pts, 40, s, None))
    return out


def streaming_n():
    return 3 * RES32 + 77


def _winner_cases():
    # resident, four strides: thread t owns t, t + BLOCK, ...; the tail past
    # the last full stride is [3 BLOCK, n)
    n = 3 * BLOCK + 5
    where = [63,              # last lane of the first wave
             BLOCK - 1,       # last lane of the last wave
             BLOCK - 64 + 3,  # inside the last wave
             n - 1,           # the tail
             BLOCK + 63]      # last lane, second stride
    out = [Case("winners", with_outliers(n, 103, where), 8, 100,
                {r + 1: i for r, i in enumerate(where)})]
    n = streaming_n()
    where = [n - 1, 63, BLOCK - 1, n - 70, 2 * BLOCK + 5]
    out.append(Case("streaming", with_outliers(n, 104, where), K_STREAM, 9,
                    {r + 1: i for r, i in enumerate(where)}))
    return out


def lattice():
    g = np.stack(np.meshgrid(np.arange(9), np.arange(9), np.arange(7),
                             indexing="ij"), -1).reshape(-1, 3)
    return Case("lattice", g.astype(np.float64), 128, 200, None)


def duplicated():
    pts = np.repeat(blob(100, 105), 2, axis=0)
    return Case("duplicated", pts, 150, 31, None)


def all_equal():
    pts = np.tile(np.array([[1.5, -2.25, 3.0]]), (130, 1))
    return Case("all_equal", pts, 10, 77, None)


def untied():
    """a cloud without ties (the CPU test asserts it): a permutation of it
    picks the same points"""
    return Case("untied", blob(1500, 106), 64, 11, None)


def non_finite():
    pts = blob(700, 107)
    pts[5, 0] = np.nan
    pts[64, 1] = np.inf
    pts[300, 2] = -np.inf
    pts[699] = np.nan
    return Case("non_finite", pts, 32, 1, None)


@functools.lru_cache(maxsize=None)
def all_cases():
    """every equality case (non_finite is not one)"""
    return tuple(_size_cases() + _k_and_start_cases() + _winner_cases() +
                 [lattice(), duplicated(), all_equal(), untied()])


# segmented: an empty, a one-point, a sub-wave, a resident and a streaming
# segment (streaming for both dtypes)
SEG_SIZES = (0, 1, 40, BLOCK + 188, RES32 + 300)
SEG_STARTS = (0, 0, 17, BLOCK + 187, 5)
SEG_K = 24


@functools.lru_cache(maxsize=None)
def segmented():
    """-> (points float64 [sum, 3], offsets int32 [6], starts int32 [5])"""
    pts = blob(sum(SEG_SIZES), 108)
    off = np.concatenate([[0], np.cumsum(SEG_SIZES)]).astype(np.int32)
    return pts, off, np.array(SEG_STARTS, np.int32)


@functools.lru_cache(maxsize=None)
def reference_of(name, dtype):
    """(idx, num_distinct, multiplicities) of a case in a dtype, computed
    once per session"""
    case = {c.name: c for c in all_cases()}[name]
    idx, nd, mult = fps_trace(case.cast(dtype), case.k, case.start)
    idx.setflags(write=False)
    return idx, nd, tuple(mult)
