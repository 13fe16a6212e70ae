"""Ground-truth object pasting of the reference (models/crop_aug.py) with the
per-point work on the GPU: the same names, keywords and defaults
(`save_cropped_boxes`, `load_cropped_boxes`, `parser_without_collision`,
`CropAugSampler.crop_aug`; the `vis_*` helpers are not part of this), the same
file format, the same consumption of NumPy's global random stream.

`parser_without_collision` is a sequential search: for every sampled object up
to `max_trails` random yaws, each needing a ground-height reduction, a point
count and a box-overlap test over the CURRENT cloud.  Written with the
primitives of preprocess.py that would be one host read per trial (up to
`samples * max_trails` per frame); here the whole search is ONE launch,
`pgnn_crop_aug_place`, and ONE host read (include/pointgnn_hip.h has the
contract):

  * the yaws are drawn up front -- `samples * max_trails` values in one sized
    call, which yields what that many scalar calls would -- and the kernel
    consumes them from one flat cursor, one per trial actually run;
  * the host reads the kernel's record (per sample: accepted, the index of the
    accepting draw, the ground height; the draws consumed; the final size),
    restores the saved RNG state and draws exactly the consumed number again,
    so NumPy's stream ends where the reference's does;
  * the new labels are built in NumPy from the accepting draw and the ground
    height with the reference's expressions, so their values are its values;
  * the kernel leaves the working cloud as [object S-1, ..., object 0, base]
    with alive flags; one order-preserving compaction gives the reference's
    order (each accepted object prepended).  The attributes take the same
    layout and the same compaction.

The cloud is float64 on the device from here on, as in preprocess.py; the
attributes stay float32 (a database's attribute values are float32 values
written as decimals, nothing is lost).  The caller's tensors are not written;
the caller's label list is appended to in place, as the reference does.

Deviations: a `method_name` other than 'normal' / 'uniform' and `attr=None`
raise ValueError up front (the reference fails inside its loop); a frame
without labels is an empty corner list (the reference's np.max over axis 1 of
an empty array raises).  cos / sin of a NEW label's yaw are the device's in the
kernel's box tests, so a decision that hangs on the last bit of a box face or
of an integer corner coordinate can differ from NumPy's.
"""
import json
from copy import deepcopy

import numpy as np

from . import _lib
from .kitti_dataset import Points
from .preprocess import (_attr_of, _box7, _compact, _f64_points, _in_box,
                         _yaw_matrix)

_OVERLAP_MODES = {'box': 0, 'point': 1, 'box_and_point': 2}


def save_cropped_boxes(dataset, filename, expand_factor=[1.1, 1.1, 1.1],
                       minimum_points=10, backlist=[]):
    """crop_aug.py:17-42: the points inside every (expanded) object box of the
    dataset with more than `minimum_points` of them, as the reference's JSON
    pair (cropped_labels, cropped_cam_points).  An offline step: one host read
    per label."""
    cropped_labels = {}
    cropped_cam_points = {}
    for frame_idx in range(dataset.num_files):
        labels = dataset.get_label(frame_idx)
        cam_points = dataset.get_cam_points_in_image_with_rgb(frame_idx)
        xyz = _f64_points(cam_points)      # float32 values, exactly
        attr = _attr_of(cam_points, xyz)
        for label in labels:
            if label['name'] == "DontCare" or label['name'] in backlist:
                continue
            mask, count = _in_box(xyz, label, expand_factor, want_mask=True)
            n_in = int(count.item())
            if n_in > minimum_points:
                obj_xyz, obj_attr = _compact(xyz, attr, n_in, keep=mask)
                cropped_labels.setdefault(label['name'], []).append(label)
                cropped_cam_points.setdefault(label['name'], []).append(
                    [obj_xyz.cpu().numpy().tolist(),
                     obj_attr.cpu().numpy().tolist()])
    with open(filename, 'w') as outfile:
        json.dump((cropped_labels, cropped_cam_points), outfile)


class CroppedPoints(dict):
    """cropped_cam_points of load_cropped_boxes: name -> list of host
    Points, like the reference's, plus every object's points resident on the
    device: `xyz` float64 [P,3], `attr` float32 [P,a], and `offsets[(name,
    index)] = (first row, end row)`.  `device_points(name, index)` is a Points
    of views into the two blocks."""

    xyz = None
    attr = None
    offsets = None

    def upload(self, device=None):
        import torch
        dev = device if device is not None else torch.device(
            "cuda", torch.cuda.current_device())
        xs, ats, self.offsets, row = [], [], {}, 0
        for key in self:
            for i, pts in enumerate(self[key]):
                x = np.asarray(pts.xyz, np.float64).reshape(-1, 3)
                xs.append(x)
                ats.append(np.asarray(pts.attr, np.float32).reshape(len(x), -1))
                self.offsets[(key, i)] = (row, row + len(x))
                row += len(x)
        width = ats[0].shape[1] if ats else 0
        self.xyz = torch.from_numpy(
            np.concatenate(xs) if xs else np.zeros((0, 3))).to(dev)
        self.attr = torch.from_numpy(
            np.concatenate(ats) if ats else np.zeros((0, width), np.float32)
        ).to(dev)
        return self

    def device_points(self, name, index):
        a, b = self.offsets[(name, int(index))]
        return Points(xyz=self.xyz[a:b], attr=self.attr[a:b])


def load_cropped_boxes(filename):
    """crop_aug.py:44-52 -> (cropped_labels, cropped_cam_points); the second
    is a CroppedPoints whose objects are also resident on the device."""
    with open(filename, 'r') as infile:
        cropped_labels, cam_points = json.load(infile)
    cropped_cam_points = CroppedPoints()
    for key in cam_points:
        print("Load %d %s" % (len(cam_points[key]), key))
        cropped_cam_points[key] = [
            Points(xyz=np.array(xyz), attr=np.array(attr))
            for xyz, attr in cam_points[key]]
    return cropped_labels, cropped_cam_points.upload()


def _device_rows(x, dtype, dev):
    import torch
    if not isinstance(x, torch.Tensor):
        x = torch.as_tensor(np.asarray(x))
    x = x.to(device=dev, dtype=dtype)
    return x.reshape(-1, 1) if x.dim() == 1 else x


def _draw_yaws(method_name, yaw_std, size):
    if method_name == 'normal':
        return np.random.normal(scale=yaw_std, size=size)
    return np.random.uniform(low=-yaw_std, high=yaw_std, size=size)


def place(xyz, sample_xyz, sample_offsets, sample_boxes, label_corners, table,
          max_trails, mode, auto_box_height, must_have_ground,
          max_overlap_rate, appr_factor, max_overlap_num_allowed,
          expand_factor):
    """pgnn_crop_aug_place -> (work_xyz [M+N,3], alive int32 [M+N], record
    float64 [3S+2] on the device).  xyz [N,3] / sample_xyz [M,3] are float64
    device tensors; sample_offsets [S+1], sample_boxes [S,7], label_corners
    [L,8,3] int32 and the draw table [S*max_trails,3] are host arrays (two
    uploads).  The kernel's candidate scratch (M+N rows) is allocated here."""
    import torch
    lib = _lib.load()
    dev = xyz.device
    n, m = int(xyz.shape[0]), int(sample_xyz.shape[0])
    s, n_lab = len(sample_boxes), len(label_corners)
    f64 = np.concatenate([
        np.asarray(sample_boxes, np.float64).reshape(-1),
        np.asarray(table, np.float64).reshape(-1), np.zeros(1)])
    i32 = np.concatenate([
        np.asarray(sample_offsets, np.int32).reshape(-1),
        np.asarray(label_corners, np.int32).reshape(-1),
        np.zeros(1, np.int32)])
    d_f64 = torch.from_numpy(f64).to(dev)
    d_i32 = torch.from_numpy(i32).to(dev)
    expand = np.ascontiguousarray(expand_factor, np.float64)
    work = torch.empty((m + n, 3), dtype=torch.float64, device=dev)
    alive = torch.empty((m + n,), dtype=torch.int32, device=dev)
    cand_xyz = torch.empty((m + n, 3), dtype=torch.float64, device=dev)
    cand_idx = torch.empty((m + n,), dtype=torch.int32, device=dev)
    record = torch.empty((3 * s + 2,), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.pgnn_crop_aug_place(
            _lib.ptr(xyz), n, _lib.ptr(sample_xyz), d_i32.data_ptr(), s, m,
            d_f64.data_ptr(), d_i32.data_ptr() + 4 * (s + 1), n_lab,
            d_f64.data_ptr() + 8 * 7 * s, int(max_trails), int(mode),
            int(bool(auto_box_height)), int(bool(must_have_ground)),
            float(max_overlap_rate), float(appr_factor),
            float(max_overlap_num_allowed), expand.ctypes.data,
            _lib.ptr(work), _lib.ptr(alive), _lib.ptr(cand_xyz),
            _lib.ptr(cand_idx), _lib.ptr(record),
            _lib.stream_ptr()), "pgnn_crop_aug_place")
    return work, alive, record


def parser_without_collision(cam_rgb_points, labels,
                             sample_cam_points, sample_labels,
                             overlap_mode='box',
                             auto_box_height=False,
                             max_overlap_rate=0.01,
                             appr_factor=100,
                             max_overlap_num_allowed=1, max_trails=1,
                             method_name='normal',
                             yaw_std=0.3, expand_factor=(1.1, 1.1, 1.1),
                             must_have_ground=False):
    """crop_aug.py:75-186: paste each sampled object at a random yaw about the
    origin where it collides with nothing -- see the module text.  Returns
    (Points of device tensors, labels); `labels` is the caller's list, the
    accepted objects' labels appended."""
    import torch
    from . import nms
    if method_name not in ('normal', 'uniform'):
        raise ValueError(method_name)
    if cam_rgb_points.attr is None:
        raise ValueError("crop_aug needs point attributes (attr=None)")
    xyz = _f64_points(cam_rgb_points)
    attr = _attr_of(cam_rgb_points, xyz)
    n_samples, trails = len(sample_labels), max(int(max_trails), 0)
    if n_samples == 0 or trails == 0:
        return Points(xyz=xyz, attr=attr), labels
    state = np.random.get_state()
    draws = _draw_yaws(method_name, yaw_std, n_samples * trails)
    if overlap_mode not in _OVERLAP_MODES:
        # crop_aug.py:130-165: below_overlap stays False, every trial is spent
        return Points(xyz=xyz, attr=attr), labels
    mode = _OVERLAP_MODES[overlap_mode]
    corners = np.zeros((0, 8, 3), np.int32)
    if mode != _OVERLAP_MODES['point'] and len(labels) > 0:
        corners = np.int32(appr_factor * nms.boxes_3d_to_corners(
            np.array([_box7(l) for l in labels])))
    dev = xyz.device
    s_xyz = [_device_rows(p.xyz, torch.float64, dev).reshape(-1, 3)
             for p in sample_cam_points]
    s_attr = [_device_rows(p.attr, torch.float32, dev)
              for p in sample_cam_points]
    for a in s_attr:
        if int(a.shape[1]) != int(attr.shape[1]):
            raise ValueError("a sample has %d attribute columns, the cloud %d"
                             % (a.shape[1], attr.shape[1]))
    offsets = np.concatenate([[0], np.cumsum([int(x.shape[0])
                                              for x in s_xyz])])
    table = np.stack([draws, np.cos(draws), np.sin(draws)], axis=1)
    work, alive, record = place(
        xyz, torch.cat(s_xyz, dim=0).contiguous(), offsets,
        [_box7(l) for l in sample_labels], corners, table, trails, mode,
        auto_box_height, must_have_ground, max_overlap_rate, appr_factor,
        max_overlap_num_allowed, expand_factor)
    record = record.cpu().numpy()                      # the one host read
    consumed, n_out = int(record[-2]), int(record[-1])
    if consumed < 0:
        raise _lib.PointGnnHipError("pgnn_crop_aug_place: bad offset table")
    # NumPy's stream as the reference leaves it: one draw per trial run
    np.random.set_state(state)
    _draw_yaws(method_name, yaw_std, consumed)
    for i, label in enumerate(sample_labels):
        accepted, draw_index, ground = record[3 * i:3 * i + 3]
        if accepted == 0:
            continue
        # crop_aug.py:103-127 for the accepting draw
        delta_yaw = draws[int(draw_index)]
        new_label = deepcopy(label)
        centre = np.array([[new_label['x3d'], new_label['y3d'],
                            new_label['z3d']]])
        centre = centre.dot(np.transpose(_yaw_matrix(delta_yaw)))
        new_label['x3d'], new_label['y3d'], new_label['z3d'] = centre[0]
        new_label['yaw'] = new_label['yaw'] + delta_yaw
        if auto_box_height:
            y3d_adjust = 0 if np.isnan(ground) else ground - new_label['y3d']
            new_label['y3d'] += y3d_adjust
        labels.append(new_label)
    work_attr = torch.cat(s_attr[::-1] + [attr], dim=0).contiguous()
    out_xyz, out_attr = _compact(work, work_attr, n_out, keep=alive)
    return Points(xyz=out_xyz, attr=out_attr), labels


class CropAugSampler():
    """crop_aug.py:188-209: sample objects from a cropped-box file and paste
    them into a frame."""

    def __init__(self, crop_filename):
        self._cropped_labels, self._cropped_cam_points = load_cropped_boxes(
            crop_filename)

    def crop_aug(self, cam_rgb_points, labels,
                 sample_rate={"Car": 1, "Pedestrian": 1, "Cyclist": 1},
                 parser_kwargs={}):
        sample_labels = []
        sample_cam_points = []
        for key in sample_rate:
            sample_indices = np.random.choice(
                len(self._cropped_labels[key]), size=sample_rate[key],
                replace=False)
            sample_labels.extend(deepcopy(
                [self._cropped_labels[key][idx] for idx in sample_indices]))
            # views of the resident blocks: nothing below writes them
            sample_cam_points.extend(
                self._cropped_cam_points.device_points(key, idx)
                for idx in sample_indices)
        return parser_without_collision(cam_rgb_points, labels,
                                        sample_cam_points, sample_labels,
                                        **parser_kwargs)
