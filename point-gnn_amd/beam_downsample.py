"""LiDAR beam decimation of the reference's scripts/point_cloud_downsample.py
on the device: the inputs of the sparse-LiDAR experiment (every 2nd, 4th or
8th scanning line of a scan kept).

The script clusters the elevation cosine of every point into 64 beams with an
unseeded `KMeans`, so two runs of it write different files.  Here the
clustering is defined (include/pointgnn_hip.h, "beam decimation";
`pgnn_beam_centers`, `pgnn_beam_select`): integer cosines, farthest-first
initial centres, Lloyd passes with exact sums -- the result is a function of
the input bits only.

    rows = downsample(velo, rate=2)                       # one scan
    write_downsampled_dataset(dataset, out_dir, rate=2)   # the script's loop
    python -m pointgnn_amd.beam_downsample POINT_DIR OUTPUT_DIR --rate 2

or, without a second copy of the dataset,
`KittiDataset(..., beam_downsample_rate=2)`: the frame fetch decimates the
scan on the device before anything else reads it.

NumPy in -> NumPy out, CUDA tensor in -> CUDA tensor out.
"""
import argparse
import os
import warnings

import numpy as np

from . import _lib

MAX_BEAMS = 64
STATUS_OK, STATUS_FEW_POINTS, STATUS_FEW_VALUES, STATUS_MAX_ITER = 0, 1, 2, 3


def _check_args(n_beams=64, rate=1, max_iter=300):
    for name, val in (("n_beams", n_beams), ("rate", rate),
                      ("max_iter", max_iter)):
        if isinstance(val, bool) or not isinstance(val, (int, np.integer)):
            raise ValueError("%s must be an integer, got %r" % (name, val))
    if not 2 <= n_beams <= MAX_BEAMS:
        raise ValueError("n_beams must be 2..%d, got %d" % (MAX_BEAMS,
                                                            n_beams))
    if rate < 1:
        raise ValueError("rate must be >= 1, got %d" % rate)
    if max_iter < 1:
        raise ValueError("max_iter must be >= 1, got %d" % max_iter)


def _check_rows(velo):
    shape = tuple(velo.shape)
    if len(shape) != 2 or shape[1] != 4:
        raise ValueError("velo must be [n, 4] rows (x, y, z, reflectance), "
                         "got shape %r" % (shape,))


def _rows_on_device(velo):
    """-> ([n,4] float32 contiguous CUDA tensor, input was NumPy)."""
    import torch
    as_numpy = not isinstance(velo, torch.Tensor)
    if as_numpy:
        velo = np.asarray(velo)
    _check_rows(velo)
    dev = velo.device if not as_numpy and velo.is_cuda else \
        torch.device("cuda", torch.cuda.current_device())
    v = torch.as_tensor(velo).to(device=dev, dtype=torch.float32).contiguous()
    return v, as_numpy


def _workspace(lib, n, dev):
    import torch
    ws_bytes = int(lib.pgnn_beam_workspace_bytes(n))
    return torch.empty((max(ws_bytes, 1),), dtype=torch.uint8,
                       device=dev), ws_bytes


def _centers(lib, v, n_beams, max_iter, ws, ws_bytes, centers, info):
    _lib.check(lib.pgnn_beam_centers(
        _lib.ptr(v), int(v.shape[0]), int(n_beams), int(max_iter),
        _lib.ptr(ws), ws_bytes, _lib.ptr(centers), _lib.ptr(info),
        _lib.stream_ptr()), "pgnn_beam_centers")


def _select(lib, v, centers, n_beams, rate, info, ws, ws_bytes, rows, count):
    _lib.check(lib.pgnn_beam_select(
        _lib.ptr(v), int(v.shape[0]), _lib.ptr(centers), int(n_beams),
        int(rate), _lib.ptr(info), _lib.ptr(ws), ws_bytes, _lib.ptr(rows),
        _lib.ptr(count), _lib.stream_ptr()), "pgnn_beam_select")


def beam_centers(velo, n_beams=64, max_iter=300):
    """The beam centres of one scan (:22-27 with the defined clustering) ->
    (centers float64 [n_beams] ascending, info int32 [4] = n_valid, passes,
    status, 0), both on the device; nothing is read back."""
    import torch
    _check_args(n_beams=n_beams, max_iter=max_iter)
    lib = _lib.load()
    v, _ = _rows_on_device(velo)
    centers = torch.empty((n_beams,), dtype=torch.float64, device=v.device)
    info = torch.empty((4,), dtype=torch.int32, device=v.device)
    with torch.cuda.device(v.device):
        ws, ws_bytes = _workspace(lib, int(v.shape[0]), v.device)
        _centers(lib, v, n_beams, max_iter, ws, ws_bytes, centers, info)
    return centers, info


def beam_select(velo, centers, rate, info=None):
    """:27-35, :50 -> (rows [n,4] float32, count int32 [1]) on the device, in
    capacity form: the first `count` rows are the kept ones, in their original
    order.  info: that of beam_centers (status 1 / 2 keeps nothing)."""
    import torch
    lib = _lib.load()
    v, _ = _rows_on_device(velo)
    c = torch.as_tensor(centers).to(device=v.device, dtype=torch.float64)
    c = c.reshape(-1).contiguous()
    n_beams = int(c.shape[0])
    _check_args(n_beams=n_beams, rate=rate)
    if info is not None:
        info = torch.as_tensor(info).to(device=v.device, dtype=torch.int32)
        info = info.reshape(4).contiguous()
    rows = torch.empty_like(v)
    count = torch.empty((1,), dtype=torch.int32, device=v.device)
    with torch.cuda.device(v.device):
        ws, ws_bytes = _workspace(lib, int(v.shape[0]), v.device)
        _select(lib, v, c, n_beams, rate, info, ws, ws_bytes, rows, count)
    return rows, count


def downsample_rows(v, rate, n_beams=64, max_iter=300):
    """downsample() of an [n,4] float32 CUDA tensor -> CUDA tensor [m,4].
    Both entries are enqueued back to back; the one host read fetches the
    count and the info together."""
    import torch
    lib = _lib.load()
    dev = v.device
    centers = torch.empty((n_beams,), dtype=torch.float64, device=dev)
    meta = torch.empty((5,), dtype=torch.int32, device=dev)  # info | count
    info, count = meta[:4], meta[4:]
    rows = torch.empty_like(v)
    with torch.cuda.device(dev):
        ws, ws_bytes = _workspace(lib, int(v.shape[0]), dev)
        _centers(lib, v, n_beams, max_iter, ws, ws_bytes, centers, info)
        _select(lib, v, centers, n_beams, rate, info, ws, ws_bytes, rows,
                count)
        n_valid, passes, status, _, m = meta.tolist()
    if status == STATUS_FEW_POINTS:
        raise ValueError("beam decimation needs at least n_beams=%d valid "
                         "points, the scan has %d" % (n_beams, n_valid))
    if status == STATUS_FEW_VALUES:
        raise ValueError("beam decimation needs at least n_beams=%d distinct "
                         "elevations among the scan's %d valid points"
                         % (n_beams, n_valid))
    if status == STATUS_MAX_ITER:
        warnings.warn("beam clustering stopped after max_iter=%d passes "
                      "without reaching a fixed point" % passes,
                      RuntimeWarning, stacklevel=2)
    return rows[:m]


def downsample(velo, rate, n_beams=64, max_iter=300):
    """One scan with every rate-th beam kept (:22-50): velo [n,4] float32 rows
    (x, y, z, reflectance) -> [m,4], the kept rows bit for bit in their
    original order.  ValueError when the scan has fewer than n_beams valid
    points or distinct elevations (the script's KMeans raises for n_samples <
    n_clusters); RuntimeWarning when max_iter passes did not converge."""
    _check_args(n_beams=n_beams, rate=rate, max_iter=max_iter)
    v, as_numpy = _rows_on_device(velo)
    out = downsample_rows(v, rate, n_beams, max_iter)
    return out.cpu().numpy() if as_numpy else out


def write_downsampled_dataset(dataset, output_dir, rate, n_beams=64,
                              frame_indices=None):
    """The script's loop (:19-53): <output_dir>/<frame>.bin, float32 [m,4],
    for every frame of `dataset` (or those of frame_indices).  Returns the
    paths written."""
    _check_args(n_beams=n_beams, rate=rate)
    if frame_indices is None:
        frame_indices = range(dataset.num_files)
    os.makedirs(output_dir, exist_ok=True)
    paths = []
    for frame_idx in frame_indices:
        pts = dataset.get_velo_points(frame_idx)
        velo = np.ascontiguousarray(
            np.hstack([pts.xyz, pts.attr]).astype(np.float32, copy=False))
        out = downsample(velo, rate, n_beams=n_beams)
        path = os.path.join(output_dir,
                            dataset.get_filename(frame_idx) + ".bin")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        out.tofile(path)
        paths.append(path)
    return paths


def build_parser():
    ap = argparse.ArgumentParser(
        prog="python -m pointgnn_amd.beam_downsample",
        description="Write a velodyne directory with every RATE-th LiDAR "
                    "beam of every scan kept.")
    ap.add_argument("point_dir", metavar="POINT_DIR",
                    help="directory of <frame>.bin scans")
    ap.add_argument("output_dir", metavar="OUTPUT_DIR")
    ap.add_argument("--rate", type=int, required=True,
                    help="keep beams 0, RATE, 2 RATE, ...")
    ap.add_argument("--beams", type=int, default=64,
                    help="beams of the sensor (2..64, default 64)")
    ap.add_argument("--split", metavar="FILE", default=None,
                    help="frame names, one per line (default: every scan)")
    return ap


def main(argv=None):
    from .kitti_dataset import KittiDataset
    ap = build_parser()
    args = ap.parse_args(argv)
    try:
        _check_args(n_beams=args.beams, rate=args.rate)
    except ValueError as e:
        ap.error(str(e))
    dataset = KittiDataset(args.point_dir, args.point_dir, args.point_dir,
                           index_filename=args.split)
    paths = write_downsampled_dataset(dataset, args.output_dir, args.rate,
                                      n_beams=args.beams)
    print("wrote %d scans to %s" % (len(paths), args.output_dir))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
