"""KITTI frame ingest of the reference (dataset/kitti_dataset.py) with the
per-point work on the GPU: velodyne scan -> camera frame -> camera-image crop.

`KittiDataset` keeps the reference's method names for this slice
(`get_calib`, `get_velo_points`, `get_cam_points_in_image`,
`get_cam_points_in_image_with_rgb`, `get_filename`); file reads and the
calibration algebra stay on the host (a few 4x4 products per frame), the
per-point transform / projection / crop / ordered compaction is
`pgnn_kitti_cam_points_in_image`.  Results are `Points(xyz, attr)` with CUDA
tensors, ready for `graph_gen` and the model.

With a voxel size (`downsample_by_voxel_size` of the configs) the frame is
voxel-averaged between the transform and the crop
(`downsample_by_average_voxel`, kitti_dataset.py:16-48, `pgnn_voxel_average_f32`
/ `pgnn_kitti_cam_points_voxel_in_image`) and comes out float64, as the
reference's does.

Colour: the crop needs only the image SIZE, read from the PNG header, and by
default the file is not decoded (the colour columns of
`get_cam_points_in_image_with_rgb` are then zero unless the caller passes a
decoded BGR array).  `KittiDataset(..., decode_images=True)` decodes the
frame's PNG itself -- zlib on the host, the scanline filters on the device
(`pointgnn_amd.png`, `pgnn_png_unfilter`) -- and fills them: the 'irgb' /
'0rgb' / 'rgb' input features from a KITTI directory.  `get_image` is that
image, a BGR CUDA tensor.
"""
import os
import struct
from collections import namedtuple

import numpy as np

from . import _lib

Points = namedtuple('Points', ['xyz', 'attr'])   # kitti_dataset.py:14


def parse_calib(path_or_lines):
    """kitti_dataset.py:483-522 `get_calib`: the dictionary of calibration
    matrices with the reference's dtypes (P2 / R0_rect / Tr_velo_to_cam are
    float32 as parsed; every derived matrix is float64)."""
    if isinstance(path_or_lines, str):
        with open(path_or_lines, 'r') as f:
            lines = f.readlines()
    else:
        lines = list(path_or_lines)
    calib = {}
    for line in lines:
        fields = line.split(' ')
        name = fields[0].rstrip(':')
        if not name.strip():
            continue
        calib[name] = np.array(fields[1:], dtype=np.float32)
    p2 = calib['P2'].reshape(3, 4)
    r0 = calib['R0_rect'].reshape(3, 3)
    tr = calib['Tr_velo_to_cam'].reshape(3, 4)
    calib['P2'], calib['R0_rect'], calib['Tr_velo_to_cam'] = p2, r0, tr
    bottom = np.array([[0.0, 0.0, 0.0, 1.0]])
    calib['velo_to_rect'] = np.concatenate([tr.astype(np.float64), bottom])
    calib['cam_to_image'] = np.concatenate(
        [p2[:, 0:3].astype(np.float64), np.zeros((3, 1))], axis=1)
    # rectified -> camera-2 frame: rotation R0 and the baseline shift
    # inv(P2[:, :3]) @ P2[:, 3], both evaluated in float32 like the reference
    shift = np.matmul(np.linalg.inv(p2[:, 0:3]), p2[:, [3]])
    rect_to_cam = np.concatenate([r0, shift], axis=1).astype(np.float64)
    calib['rect_to_cam'] = np.concatenate([rect_to_cam, bottom])
    calib['velo_to_cam'] = np.matmul(calib['rect_to_cam'],
                                     calib['velo_to_rect'])
    calib['cam_to_velo'] = np.linalg.inv(calib['velo_to_cam'])
    calib['velo_to_image'] = np.matmul(calib['cam_to_image'],
                                       calib['velo_to_cam'])
    return calib


def png_size(path):
    """(height, width) from a PNG's IHDR chunk (no decoder needed)."""
    with open(path, 'rb') as f:
        head = f.read(24)
    if len(head) < 24 or head[:8] != b'\x89PNG\r\n\x1a\n' or \
            head[12:16] != b'IHDR':
        raise ValueError("%s is not a PNG file" % path)
    width, height = struct.unpack('>II', head[16:24])
    return int(height), int(width)


def _stage_upload(arr, dev):
    """Host float32 array -> device tensor through pinned memory (an
    asynchronous copy-engine transfer instead of the runtime's pageable
    staging path).  The block comes from torch's caching host allocator, which
    hands it out again only after the copy has run."""
    import torch
    host = torch.empty(int(arr.size), dtype=torch.float32, pin_memory=True)
    host.numpy()[:] = arr.reshape(-1)
    return host.to(dev, non_blocking=True)


class PendingPoints(object):
    """cam_points_in_image(..., deferred=True): the crop is enqueued, the
    number of points inside the image is on its way to pinned memory, nothing
    has been waited for.  `event` orders a consumer stream behind the crop;
    result() waits for the count (not for the device) and returns Points --
    call it with the consuming stream current and after
    `stream.wait_event(pending.event)`."""

    def __init__(self, xyz, attr, count_host, event, pad_rgb):
        self.xyz, self.attr, self.count_host = xyz, attr, count_host
        self.event, self.pad_rgb = event, pad_rgb

    def result(self):
        import torch
        self.event.synchronize()
        m = int(self.count_host[0])
        xyz, attr = self.xyz[:m], self.attr[:m]
        if self.pad_rgb:
            zeros = torch.zeros((m, 3), dtype=attr.dtype, device=attr.device)
            attr = torch.cat([attr, zeros], dim=1)
        return Points(xyz=xyz, attr=attr)


def _cuda_device(t):
    import torch
    if isinstance(t, torch.Tensor) and t.is_cuda:
        return t.device
    return torch.device("cuda", torch.cuda.current_device())


def downsample_by_average_voxel(points, voxel_size):
    """kitti_dataset.py:16-48: the mean of the points (and attributes) of every
    occupied voxel, rows in ascending voxel key.  `points`: Points of float32
    NumPy arrays or CUDA tensors, `attr` [n,a] (a <= 4) or None -> Points of
    float64 CUDA tensors (float32 sums divided by int64 counts are float64 in
    the reference).  The points of a voxel are added in ascending index (the
    reference's unstable argsort leaves that order to NumPy's sort)."""
    import torch
    lib = _lib.load()
    dev = _cuda_device(points.xyz)
    xyz = torch.as_tensor(points.xyz).to(device=dev, dtype=torch.float32)
    xyz = xyz.reshape(-1, 3).contiguous()
    n = int(xyz.shape[0])
    attr, attr_dim = None, 0
    if points.attr is not None:
        attr = torch.as_tensor(points.attr).to(device=dev,
                                               dtype=torch.float32)
        attr = attr.reshape(n, -1).contiguous()
        attr_dim = int(attr.shape[1])
    out_xyz = torch.empty((n, 3), dtype=torch.float64, device=dev)
    out_attr = torch.empty((n, attr_dim), dtype=torch.float64, device=dev) \
        if attr is not None else None
    count = torch.zeros((1,), dtype=torch.int32, device=dev)
    ws_bytes = int(lib.pgnn_voxel_average_workspace_bytes(n, attr_dim))
    ws = torch.empty((max(ws_bytes, 1),), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.pgnn_voxel_average_f32(
            _lib.ptr(xyz), _lib.ptr(attr) if attr is not None else None,
            attr_dim, n, None, float(voxel_size), _lib.ptr(ws), ws_bytes,
            _lib.ptr(out_xyz),
            _lib.ptr(out_attr) if out_attr is not None else None, None, n,
            _lib.ptr(count), _lib.stream_ptr()), "pgnn_voxel_average_f32")
        m = int(count.item())
    return Points(xyz=out_xyz[:m],
                  attr=out_attr[:m] if out_attr is not None else None)


def cam_points_in_image(velo_data, calib, image_shape, image=None,
                        with_rgb=False, deferred=False,
                        downsample_voxel_size=None):
    """velo_data [n,4] float32 (x,y,z,reflectance; NumPy or CUDA tensor) ->
    Points(xyz [m,3], attr [m,1] or [m,4]) as CUDA tensors:
    kitti_dataset.py:666-689 (`get_cam_points_in_image`) / :691-716 (`..._with_
    rgb`) after the file reads.  image_shape = (height, width); image = decoded
    BGR uint8 [H,W,3] (cv2.imread layout) when with_rgb.
    downsample_voxel_size: the cloud is voxel-averaged between the transform
    and the crop (:612-628) and the result is float64, rows in voxel order."""
    import torch
    lib = _lib.load()
    dev = velo_data.device if isinstance(velo_data, torch.Tensor) and \
        velo_data.is_cuda else torch.device("cuda",
                                            torch.cuda.current_device())
    if isinstance(velo_data, np.ndarray) and velo_data.dtype == np.float32 \
            and velo_data.flags.c_contiguous and velo_data.size:
        v = _stage_upload(velo_data, dev)
    else:
        v = torch.as_tensor(velo_data).to(device=dev, dtype=torch.float32)
    v = v.reshape(-1, 4).contiguous()
    n = int(v.shape[0])
    height, width = int(image_shape[0]), int(image_shape[1])
    # kitti_dataset.py:1002-1005: the float32 casts of the transposed blocks
    rt = np.ascontiguousarray(calib['velo_to_cam'][:3, :4].astype(np.float32))
    p = np.ascontiguousarray(calib['cam_to_image'][:3, :3].astype(np.float64))
    attr_dim = 4 if with_rgb else 1
    img_t = None
    if with_rgb:
        if image is None:
            raise ValueError("with_rgb needs the decoded BGR image")
        img_t = torch.as_tensor(image).to(device=dev, dtype=torch.uint8)
        img_t = img_t.contiguous()
        if img_t.dim() != 3 or img_t.shape[2] != 3:
            raise ValueError("image must be [H, W, 3] uint8 (BGR)")
    voxel = downsample_voxel_size is not None
    out_dtype = torch.float64 if voxel else torch.float32
    out_xyz = torch.empty((n, 3), dtype=out_dtype, device=dev)
    out_attr = torch.empty((n, attr_dim), dtype=out_dtype, device=dev)
    count = torch.zeros((1,), dtype=torch.int32, device=dev)
    ws_bytes = int(
        lib.pgnn_kitti_cam_points_voxel_in_image_workspace_bytes(n) if voxel
        else lib.pgnn_kitti_ingest_workspace_bytes(n))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    img_args = (_lib.ptr(img_t) if img_t is not None else None,
                int(img_t.shape[0]) if img_t is not None else 0,
                int(img_t.shape[1]) if img_t is not None else 0)
    with torch.cuda.device(dev):
        if voxel:
            _lib.check(lib.pgnn_kitti_cam_points_voxel_in_image(
                _lib.ptr(v), n, rt.ctypes.data, p.ctypes.data, float(width),
                float(height), *img_args, float(downsample_voxel_size),
                _lib.ptr(ws), ws_bytes, _lib.ptr(out_xyz), _lib.ptr(out_attr),
                attr_dim, n, _lib.ptr(count), _lib.stream_ptr()),
                "pgnn_kitti_cam_points_voxel_in_image")
        else:
            _lib.check(lib.pgnn_kitti_cam_points_in_image(
                _lib.ptr(v), n, rt.ctypes.data, p.ctypes.data, float(width),
                float(height), *img_args,
                _lib.ptr(ws), ws_bytes, _lib.ptr(out_xyz), _lib.ptr(out_attr),
                attr_dim, n, _lib.ptr(count), _lib.stream_ptr()),
                "pgnn_kitti_cam_points_in_image")
        if deferred:
            count_host = torch.empty(1, dtype=torch.int32, pin_memory=True)
            count_host.copy_(count, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            return PendingPoints(out_xyz, out_attr, count_host, ev, False)
        m = int(count.item())
    return Points(xyz=out_xyz[:m], attr=out_attr[:m])


class KittiDataset(object):
    """The inference-side slice of kitti_dataset.py:187-216: an index of
    frames under `image_dir` / `point_dir` / `calib_dir` (KITTI object layout:
    <name>.png, <name>.bin, <name>.txt)."""

    def __init__(self, image_dir, point_dir, calib_dir, label_dir=None,
                 index_filename=None, is_training=False, is_raw=False,
                 difficulty=-100, num_classes=8, beam_downsample_rate=None,
                 beam_count=64, decode_images=False):
        """decode_images (extension): get_cam_points_in_image_with_rgb called
        without `image=` decodes the frame's PNG (get_image) and fills the
        colour columns; False leaves them zero, as before.
        beam_downsample_rate (extension): every method that reads a scan
        keeps every rate-th of its `beam_count` LiDAR beams first
        (beam_downsample.downsample, scripts/point_cloud_downsample.py) --
        the WHOLE scan, before xyz_range, the transform, voxel averaging and
        the crop, as a dataset read back from the script's output directory
        behaves."""
        if beam_downsample_rate is not None:
            from .beam_downsample import _check_args
            _check_args(n_beams=beam_count, rate=beam_downsample_rate)
        self._beam_rate = beam_downsample_rate
        self._beam_count = beam_count
        self._decode_images = bool(decode_images)
        if is_raw:
            raise NotImplementedError(
                "the raw-sequence layout is outside the ingest slice")
        if is_training and not label_dir:
            raise ValueError("is_training needs label_dir")
        self._image_dir = image_dir
        self._point_dir = point_dir
        self._calib_dir = calib_dir
        self._label_dir = label_dir
        if index_filename:
            with open(index_filename, 'r') as f:
                self._file_list = [l.rstrip('\n') for l in f if l.strip()]
        else:
            self._file_list = sorted(
                f[:-4] for f in os.listdir(point_dir) if f.endswith('.bin'))
        self.num_classes = num_classes
        self.difficulty = difficulty

    @property
    def num_files(self):
        return len(self._file_list)

    def get_filename(self, frame_idx):
        return self._file_list[frame_idx]

    def get_calib(self, frame_idx):
        return parse_calib(os.path.join(
            self._calib_dir, self._file_list[frame_idx]) + '.txt')

    def _read_scan(self, frame_idx, on_device=False):
        """The file's [n,4] float32 rows (kitti_dataset.py:589-592).  With a
        beam_downsample_rate: the decimated scan -- a CUDA tensor when
        on_device (the rows stay where the crop wants them), else host rows.
        The decimation's one host read happens here, on the calling thread."""
        data = np.fromfile(os.path.join(
            self._point_dir, self._file_list[frame_idx]) + '.bin',
            dtype=np.float32).reshape(-1, 4)
        if self._beam_rate is None:
            return data
        import torch
        from .beam_downsample import downsample_rows
        dev = _cuda_device(None)
        v = _stage_upload(data, dev) if data.size else \
            torch.empty(0, dtype=torch.float32, device=dev)
        rows = downsample_rows(v.reshape(-1, 4), self._beam_rate,
                               n_beams=self._beam_count)
        return rows if on_device else rows.cpu().numpy()

    def get_velo_points(self, frame_idx, xyz_range=None):
        """kitti_dataset.py:587-609 -> host Points (the crop runs later)."""
        data = self._read_scan(frame_idx)
        if xyz_range is not None:
            m = np.ones(len(data), bool)
            for axis, (lo, hi) in enumerate(xyz_range):
                m &= (data[:, axis] > lo) & (data[:, axis] < hi)
            data = data[m]
        return Points(xyz=data[:, :3], attr=data[:, [3]])

    def _image_shape(self, frame_idx):
        return png_size(os.path.join(
            self._image_dir, self._file_list[frame_idx]) + '.png')

    def get_image(self, frame_idx):
        """kitti_dataset.py:691-701 (`cv2.imread`): the frame's image, uint8
        [H, W, 3] in BGR order, as a CUDA tensor; decoded on the current
        stream (png.read_png), nothing read back."""
        from . import png
        return png.read_png(os.path.join(
            self._image_dir, self._file_list[frame_idx]) + '.png', order='bgr')

    def get_cam_points(self, frame_idx, downsample_voxel_size=None,
                       calib=None, xyz_range=None):
        """kitti_dataset.py:612-628: the whole scan in camera coordinates (no
        crop), voxel-averaged when a size is given.  The float32 transform is
        the reference's expression on the host (:998-1006); Points of CUDA
        tensors, float32 without a voxel size and float64 with one."""
        import torch
        if calib is None:
            calib = self.get_calib(frame_idx)
        pts = self.get_velo_points(frame_idx, xyz_range=xyz_range)
        m = np.transpose(calib['velo_to_cam'])
        cam_xyz = np.matmul(pts.xyz, m[:3, :3].astype(np.float32))
        cam_xyz += m[[3], :3].astype(np.float32)
        dev = _cuda_device(None)
        cam = Points(xyz=torch.from_numpy(cam_xyz).to(dev),
                     attr=torch.from_numpy(np.ascontiguousarray(pts.attr)
                                           ).to(dev))
        if downsample_voxel_size is not None:
            cam = downsample_by_average_voxel(cam, downsample_voxel_size)
        return cam

    def calc_distances(self, p0, points):
        """kitti_dataset.py:630-631 on the host: squared distance of every
        row of `points` to `p0` (the arithmetic the sampling kernel restates:
        (dx*dx + dy*dy) + dz*dz in the promoted dtype)."""
        diff = np.asarray(p0) - np.asarray(points)
        return (diff * diff).sum(axis=1)

    def farthest_first(self, pts, K, start=None, return_indices=False):
        """kitti_dataset.py:633-641 on the device (sampling.py): K rows of
        `pts` [n,3], each the farthest from those picked before it -> float64
        [K,3] like the reference.  `start` (extension): the index of the first
        pick; None draws exactly one np.random.randint(len(pts)), the
        reference's draw, so the result after np.random.seed(s) is the
        reference's.  `return_indices` (extension): -> (rows, idx int32 [K]).
        float32 clouds stay float32 on the device (the kernel widens them as
        NumPy's promotion does), every other dtype goes through float64."""
        from . import sampling
        K = sampling.check_count(K, "K")
        pts = np.asarray(pts)
        if pts.dtype != np.float32:
            pts = pts.astype(np.float64)
        if start is None:
            start = np.random.randint(len(pts))
        idx, xyz, _ = sampling.farthest_first_device(pts, K, start=start)
        rows = xyz.astype(np.float64)
        return (rows, idx) if return_indices else rows

    def get_cam_points_in_image(self, frame_idx, downsample_voxel_size=None,
                                calib=None, xyz_range=None):
        if calib is None:
            calib = self.get_calib(frame_idx)
        if self._beam_rate is not None and xyz_range is None:
            velo = self._read_scan(frame_idx, on_device=True)
        else:
            pts = self.get_velo_points(frame_idx, xyz_range=xyz_range)
            velo = np.concatenate([pts.xyz, pts.attr], axis=1)
        return cam_points_in_image(
            velo, calib, self._image_shape(frame_idx),
            downsample_voxel_size=downsample_voxel_size)

    def get_cam_points_in_image_with_rgb(self, frame_idx,
                                         downsample_voxel_size=None,
                                         calib=None, xyz_range=None,
                                         image=None, deferred=False):
        """With `image` (decoded BGR array) the attributes are
        [reflectance, r, g, b]; without one the frame's PNG is decoded when
        the dataset was built with decode_images=True, else the colour
        channels are zero -- enough for the 'i' / 'i000' / '0' input features
        of the shipped configs (run.py:226-241).
        deferred (extension): enqueue only and return a PendingPoints; the
        decode too runs on the caller's current stream."""
        if calib is None:
            calib = self.get_calib(frame_idx)
        if image is None and self._decode_images:
            image = self.get_image(frame_idx)
        if xyz_range is None:
            # the file's [n,4] rows as they are (no split + re-join)
            velo = self._read_scan(frame_idx, on_device=True)
        else:
            pts = self.get_velo_points(frame_idx, xyz_range=xyz_range)
            velo = np.concatenate([pts.xyz, pts.attr], axis=1)
        shape = image.shape[:2] if image is not None \
            else self._image_shape(frame_idx)
        if image is None:
            import torch
            p = cam_points_in_image(
                velo, calib, shape, deferred=deferred,
                downsample_voxel_size=downsample_voxel_size)
            if deferred:
                p.pad_rgb = True
                return p
            zeros = torch.zeros((p.attr.shape[0], 3), dtype=p.attr.dtype,
                                device=p.attr.device)
            return Points(xyz=p.xyz, attr=torch.cat([p.attr, zeros], dim=1))
        return cam_points_in_image(
            velo, calib, shape, image=image, with_rgb=True, deferred=deferred,
            downsample_voxel_size=downsample_voxel_size)

    # ---- labels and training targets (kitti_dataset.py:703-751, 1132-1284)
    def get_label(self, frame_idx, no_orientation=False):
        """kitti_dataset.py:703-751: list of label dictionaries of a frame."""
        return read_label_file(os.path.join(
            self._label_dir, self._file_list[frame_idx]) + '.txt',
            self.difficulty)

    def sel_xyz_in_box3d(self, label, xyz, expend_factor=(1.0, 1.0, 1.0)):
        return sel_xyz_in_box3d(label, xyz, expend_factor)

    def box3d_to_cam_points(self, label, expend_factor=(1.0, 1.0, 1.0)):
        return box3d_to_cam_points(label, expend_factor)

    def box3d_to_normals(self, label, expend_factor=(1.0, 1.0, 1.0)):
        return box3d_to_normals(label, expend_factor)

    def assign_classaware_label_to_points(self, labels, xyz, expend_factor):
        """kitti_dataset.py:1132-1182 (label_method 'yaw', 8 classes)."""
        assert self.num_classes == 8
        return assign_label_to_points(labels, xyz, expend_factor, {
            'Background': 0, 'Car': 1, 'Pedestrian': 3, 'Cyclist': 5,
            'DontCare': 7})

    def assign_classaware_car_label_to_points(self, labels, xyz,
                                              expend_factor):
        """kitti_dataset.py:1184-1232 (label_method 'Car', 4 classes)."""
        assert self.num_classes == 4
        return assign_label_to_points(labels, xyz, expend_factor, {
            'Background': 0, 'Car': 1, 'DontCare': 3})

    def assign_classaware_ped_and_cyc_label_to_points(self, labels, xyz,
                                                      expend_factor):
        """kitti_dataset.py:1234-1284 ('Pedestrian_and_Cyclist', 6)."""
        assert self.num_classes == 6
        return assign_label_to_points(labels, xyz, expend_factor, {
            'Background': 0, 'Pedestrian': 1, 'Cyclist': 3, 'DontCare': 5})


_LABEL_FIELDS = (('truncation', float), ('occlusion', int), ('alpha', float),
                 ('xmin', float), ('ymin', float), ('xmax', float),
                 ('ymax', float), ('height', float), ('width', float),
                 ('length', float), ('x3d', float), ('y3d', float),
                 ('z3d', float), ('yaw', float))


def read_label_file(path, difficulty=-100):
    """kitti_dataset.py:703-751: KITTI label txt -> list of dicts, filtered by
    `difficulty` (0/1/2 = easy/moderate/hard limits; < 0 keeps everything)."""
    min_height = (40, 25, 25)
    max_occlusion = (0, 1, 2)
    max_truncation = (0.15, 0.3, 0.5)
    labels = []
    with open(path, 'r') as f:
        for line in f:
            fields = line.strip().split(' ')
            if fields == ['']:
                continue
            label = {'name': fields[0]}
            for (key, conv), text in zip(_LABEL_FIELDS, fields[1:15]):
                label[key] = conv(text)
            if len(fields) > 15:
                label['score'] = float(fields[15])
            if difficulty > -1:
                if label['truncation'] > max_truncation[difficulty] or \
                        label['occlusion'] > max_occlusion[difficulty] or \
                        label['ymax'] - label['ymin'] < min_height[difficulty]:
                    continue
            labels.append(label)
    return labels


def box3d_to_cam_points(label, expend_factor=(1.0, 1.0, 1.0)):
    """kitti_dataset.py:85-116: the 8 corners [8,3] float64 of a label box in
    camera coordinates (y down: the box bottom is at y3d), optionally
    expanded: height by expend_factor[0] (half above, half below), width and
    length by [1] and [2].  Returns Points(xyz, None)."""
    yaw = label['yaw']
    c, s = np.cos(yaw), np.sin(yaw)
    h = label['height']
    dh = h * (expend_factor[0] - 1)
    hw = label['width'] * expend_factor[1] / 2
    hl = label['length'] * expend_factor[2] / 2
    top, bottom = dh / 2, -h - dh / 2
    local = np.array([[hl, top, hw], [hl, top, -hw], [-hl, top, -hw],
                      [-hl, top, hw], [hl, bottom, hw], [hl, bottom, -hw],
                      [-hl, bottom, -hw], [-hl, bottom, hw]])
    rot = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    xyz = local.dot(rot.T) + np.array([label['x3d'], label['y3d'],
                                       label['z3d']])
    return Points(xyz=xyz, attr=None)


def box3d_to_normals(label, expend_factor=(1.0, 1.0, 1.0)):
    """kitti_dataset.py:118-141: edge directions of the box (rows wx, wy, wz)
    and the [lower, upper] bounds of a point's projections on them."""
    p = box3d_to_cam_points(label, expend_factor).xyz
    normals, lower, upper = [], [], []
    for far in (4, 1, 3):              # corner 0 against corners 4, 1, 3
        w = p[[0], :] - p[[far], :]
        normals.append(w)
        lower.append(np.matmul(w, p[far, :]))
        upper.append(np.matmul(w, p[0, :]))
    return (np.concatenate(normals, axis=0), np.concatenate(lower),
            np.concatenate(upper))


def _label_records(labels, expend_factor, label_map):
    """Host half of assign_*_label_to_points: one 24-double record per label
    (layout in include/pointgnn_hip.h)."""
    default = label_map['DontCare']
    rec = np.zeros((len(labels), 24), np.float64)
    for i, label in enumerate(labels):
        name = label['name']
        obj_cls = label_map.get(name, default)
        if 1 <= obj_cls <= default - 1:
            yaw = label['yaw']
            while yaw < -0.25 * np.pi:
                yaw += np.pi
            while yaw > 0.75 * np.pi:
                yaw -= np.pi
            action = 1.0
            cls = obj_cls if yaw < 0.25 * np.pi else obj_cls + 1
            box = (label['x3d'], label['y3d'], label['z3d'], label['length'],
                   label['height'], label['width'], yaw)
        elif name != 'DontCare':
            action, cls, box = 2.0, obj_cls, (0.0,) * 7
        else:
            continue                      # record stays action 0 (skipped)
        normals, lower, upper = box3d_to_normals(label, expend_factor)
        rec[i, 0:9] = normals.reshape(-1)
        rec[i, 9:12] = lower
        rec[i, 12:15] = upper
        rec[i, 15] = action
        rec[i, 16] = cls
        rec[i, 17:24] = box
    return rec


def _assign(xyz, rec, want_boxes=True):
    import torch
    lib = _lib.load()
    as_numpy = not isinstance(xyz, torch.Tensor)
    dev = xyz.device if not as_numpy and xyz.is_cuda else \
        torch.device("cuda", 0)
    p = torch.as_tensor(xyz)
    # float64 vertices stay float64 (train.py:100-118 passes the float64
    # vertex_coord_list of the augmented cloud; np.matmul then runs in float64
    # on the exact coordinates); everything else is the float32 cloud
    wide = p.dtype == torch.float64
    p = p.to(device=dev, dtype=torch.float64 if wide else torch.float32
             ).contiguous()
    n = int(p.shape[0])
    r = torch.from_numpy(np.ascontiguousarray(rec)).to(dev)
    cls = torch.empty((n,), dtype=torch.int32, device=dev)
    boxes = torch.empty((n, 7), dtype=torch.float64, device=dev) \
        if want_boxes else None
    valid = torch.empty((n,), dtype=torch.float32, device=dev)
    owner = torch.empty((n,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        entry = lib.pgnn_assign_box_labels_f64 if wide else \
            lib.pgnn_assign_box_labels
        _lib.check(entry(
            _lib.ptr(p), n, _lib.ptr(r), int(r.shape[0]), _lib.ptr(cls),
            _lib.ptr(boxes) if boxes is not None else None, _lib.ptr(valid),
            _lib.ptr(owner), _lib.stream_ptr()), "pgnn_assign_box_labels")
    return as_numpy, cls, boxes, valid, owner


def sel_xyz_in_box3d(label, xyz, expend_factor=(1.0, 1.0, 1.0)):
    """kitti_dataset.py:143-162: bool mask of the points strictly inside the
    (expanded) box.  NumPy in -> NumPy out, CUDA tensor in -> CUDA tensor."""
    rec = np.zeros((1, 24), np.float64)
    normals, lower, upper = box3d_to_normals(label, expend_factor)
    rec[0, 0:9], rec[0, 9:12], rec[0, 12:15] = normals.reshape(-1), lower, upper
    rec[0, 15] = 2.0
    as_numpy, _, _, _, owner = _assign(xyz, rec, want_boxes=False)
    mask = owner >= 0
    return mask.cpu().numpy() if as_numpy else mask


def sel_xyz_in_box2d(label, xyz, expend_factor=(1.0, 1.0, 1.0)):
    """kitti_dataset.py:164-182: the strict predicate on the box's y and z
    normals only (the column of space above and below the box).  Same kernel
    as sel_xyz_in_box3d: the height normal's row is zero between infinite
    bounds, so its test passes for every finite point."""
    rec = np.zeros((1, 24), np.float64)
    normals, lower, upper = box3d_to_normals(label, expend_factor)
    rec[0, 3:9], rec[0, 10:12], rec[0, 13:15] = \
        normals[1:].reshape(-1), lower[1:], upper[1:]
    rec[0, 9], rec[0, 12] = -np.inf, np.inf
    rec[0, 15] = 2.0
    as_numpy, _, _, _, owner = _assign(xyz, rec, want_boxes=False)
    mask = owner >= 0
    return mask.cpu().numpy() if as_numpy else mask


def assign_label_to_points(labels, xyz, expend_factor, label_map):
    """The shared body of kitti_dataset.py:1132-1284 -> (cls_labels [K,1],
    boxes_3d [K,1,7] float64, valid_boxes [K,1,1] float32, label_map).
    Class values: an object of class c gets c (|yaw| "horizontal") or c+1
    (vertical, yaw wrapped into (-pi/4, 3pi/4]); names outside the map get the
    DontCare value with valid 0; 'DontCare' boxes are ignored."""
    xyz_n = xyz.shape[0]
    assert xyz_n > 0, "No point No prediction"
    assert xyz.shape[1] == 3
    rec = _label_records(labels, expend_factor, label_map)
    as_numpy, cls, boxes, valid, _ = _assign(xyz, rec)
    cls = cls.reshape(-1, 1)
    boxes = boxes.reshape(-1, 1, 7)
    valid = valid.reshape(-1, 1, 1)
    if as_numpy:
        return (cls.cpu().numpy().astype(np.int64), boxes.cpu().numpy(),
                valid.cpu().numpy(), label_map)
    return cls, boxes, valid, label_map
