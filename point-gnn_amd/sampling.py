"""Farthest-point sampling of the reference (dataset/kitti_dataset.py:630-641,
`KittiDataset.farthest_first` with `calc_distances`) on the device.

The contract is in include/pointgnn_hip.h, "farthest-point sampling"
(`pgnn_farthest_first`, `pgnn_farthest_first_f64`): pick 0 is the start
index, every later pick is np.argmax of the running minimum distance, in the
reference's float64 arithmetic bit for bit; one workgroup per cloud runs all
k rounds.

    idx, xyz, num_distinct = farthest_first_device(points, k, start=7)
    idx, xyz, num_distinct = farthest_first_device(
        points, k, start=[0, 3, 5], offsets=[0, 100, 2100, 2164])

NumPy in -> NumPy out, CUDA tensors in -> CUDA tensors out.  float64 points
stay float64, every other dtype is taken as float32.
"""
import numpy as np

from . import _lib

BLOCK = _lib._C["PGNN_FPS_BLOCK"]
# largest cloud whose coordinates and distances stay on chip for all rounds
RESIDENT = {np.dtype(np.float32): _lib._C["PGNN_FPS_RESIDENT"],
            np.dtype(np.float64): _lib._C["PGNN_FPS_RESIDENT_F64"]}


def _host_ints(a, what):
    """1-D int64 NumPy copy of host ints, a NumPy array or a tensor."""
    import torch
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    if a.dtype.kind not in "iu" or a.dtype == np.bool_:
        raise ValueError("%s must hold integers, got dtype %s"
                         % (what, a.dtype))
    return a.astype(np.int64).reshape(-1)


def check_count(k, what="k"):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise ValueError("%s must be an integer, got %r" % (what, k))
    if k < 0:
        raise ValueError("%s must be >= 0, got %d" % (what, k))
    return int(k)


def segment_starts(sizes, start=None):
    """The start index of every segment (host logic of
    farthest_first_device): `start` checked against the segment sizes, or, for
    None, one np.random.randint(n) per non-empty segment, in segment order (an
    empty segment draws nothing and gets 0) -> int32 [S]."""
    sizes = np.asarray(sizes, np.int64).reshape(-1)
    if start is None:
        return np.array([np.random.randint(n) if n > 0 else 0 for n in sizes],
                        np.int32)
    st = _host_ints(start, "start")
    if st.shape[0] != sizes.shape[0]:
        raise ValueError("start: %d indices for %d segments"
                         % (st.shape[0], sizes.shape[0]))
    bad = (sizes > 0) & ((st < 0) | (st >= sizes))
    if bad.any():
        s = int(np.flatnonzero(bad)[0])
        raise ValueError("start index %d is outside segment %d of %d points"
                         % (st[s], s, sizes[s]))
    return np.where(sizes > 0, st, 0).astype(np.int32)


def segment_sizes(offsets, n_points):
    """offsets [S+1] over a cloud of n_points rows -> sizes int64 [S]."""
    off = _host_ints(offsets, "offsets")
    if off.shape[0] < 2:
        raise ValueError("offsets must have at least two entries")
    sizes = np.diff(off)
    if off[0] != 0 or off[-1] != n_points or (sizes < 0).any():
        raise ValueError("offsets must ascend from 0 to the number of points "
                         "(%d), got %d .. %d" % (n_points, off[0], off[-1]))
    return sizes


def _points_on_device(points):
    """-> ([n,3] contiguous CUDA tensor, float32 or float64; input was NumPy)"""
    import torch
    as_numpy = not isinstance(points, torch.Tensor)
    if as_numpy:
        points = np.asarray(points)
    shape = tuple(points.shape)
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError("points must be [n, 3], got shape %r" % (shape,))
    wide = points.dtype == (np.float64 if as_numpy else torch.float64)
    dev = points.device if not as_numpy and points.is_cuda else \
        torch.device("cuda", torch.cuda.current_device())
    p = torch.as_tensor(points).to(
        device=dev, dtype=torch.float64 if wide else torch.float32)
    return p.contiguous(), as_numpy


def launch(points, offsets, start, k, want_xyz=True):
    """pgnn_farthest_first / _f64 on device tensors, nothing checked and
    nothing read back: points [n,3] float32 / float64 contiguous, offsets int32
    [S+1] or None (one cloud), start int32 [S] -> (idx int32 [S,k], xyz
    [S,k,3] or None, num_distinct int32 [S])."""
    import torch
    lib = _lib.load()
    dev = points.device
    n = int(points.shape[0])
    n_seg = 1 if offsets is None else int(offsets.shape[0]) - 1
    wide = points.dtype == torch.float64
    # -1 / zero rows: what the kernel writes for an empty segment, also for the
    # empty single cloud, which it leaves alone
    idx = torch.full((n_seg, k), -1, dtype=torch.int32, device=dev)
    xyz = torch.zeros((n_seg, k, 3), dtype=points.dtype, device=dev) \
        if want_xyz else None
    num = torch.empty((n_seg,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        ws_bytes = int(lib.pgnn_farthest_first_workspace_bytes(n, n_seg, k))
        ws = torch.empty((max(ws_bytes, 1),), dtype=torch.uint8, device=dev)
        fn = lib.pgnn_farthest_first_f64 if wide else lib.pgnn_farthest_first
        _lib.check(fn(
            _lib.ptr(points), _lib.ptr(offsets), n_seg, n, _lib.ptr(start),
            k, _lib.ptr(ws), ws_bytes, _lib.ptr(idx), _lib.ptr(xyz),
            _lib.ptr(num), _lib.stream_ptr()), "pgnn_farthest_first")
    return idx, xyz, num


def farthest_first_device(points, k, start=None, offsets=None):
    """kitti_dataset.py:633-641 with the start index as an argument.

    points [n,3]; k picks; start: the index of pick 0 (None: one
    np.random.randint(n), the reference's draw).  Returns (idx int32 [k], xyz
    [k,3] the picked rows bit for bit in the points' dtype, num_distinct):
    picks [0, num_distinct) are pairwise non-coincident, later picks are index
    0 (duplicate points, k > n).

    Segmented: offsets int32 [S+1] over the concatenated cloud, start one LOCAL
    index per segment (None: one draw per non-empty segment, in segment
    order); idx [S,k] local, xyz [S,k,3], num_distinct [S].  An empty segment
    gets -1, zero rows and num_distinct 0.

    ValueError for a start index outside its segment.  The offsets and start
    are read on the host to check them (tensors are copied back for that);
    `launch` is the unchecked call."""
    import torch
    k = check_count(k)
    p, as_numpy = _points_on_device(points)
    n = int(p.shape[0])
    single = offsets is None
    if single:
        sizes = np.array([n], np.int64)
    else:
        sizes = segment_sizes(offsets, n)
    st = torch.from_numpy(segment_starts(sizes, start)).to(p.device)
    off = None
    if not single:
        off = torch.from_numpy(np.concatenate(
            [[0], np.cumsum(sizes)]).astype(np.int32)).to(p.device)
    idx, xyz, num = launch(p, off, st, k)
    if single:
        idx, xyz, num = idx[0], xyz[0], num[0]
    if as_numpy:
        return idx.cpu().numpy(), xyz.cpu().numpy(), num.cpu().numpy()
    return idx, xyz, num
