"""Training augmentations of the reference (models/preprocess.py) with the
per-point work on the GPU: every entry of its `aug_method_map` except
`random_jitter`, which is deliberately left raising NotImplementedError.

Same registry (`get_data_aug(aug_configs)`, `aug_method_map`), same call shape
`fn(cam_rgb_points, labels, **method_kwargs) -> (cam_rgb_points, labels)`, the
same keyword names and defaults (the reference's spellings and its unused
kwargs included) and the same consumption of NumPy's global random stream (the
same calls, sizes and order, on the host; per-point draws such as
random_drop's are host draws that get uploaded), so a seeded run makes the
same random choices.

Points live in a float64 CUDA tensor from the first augmentation on, like the
reference's array after its first `xyz.dot(R.T)` (preprocess.py:55);
`finish(points)` is train.py:124's cast back to float32.  The caller's tensors
are never written.  Deviation: where a pipeline STARTS with a method that keeps
the reference's float32 array in float32 (random_transition, random_scale_all,
random_drop, the voxel and box methods, ...), the reference goes on in float32
until a rotation widens it; here the arithmetic is float64 from the first step.
Label dictionaries are edited on the host exactly where the reference edits
them, and the returned label lists have its order and content.

When points are removed or reordered the attributes (float32 [n,a] or None)
follow row for row: pgnn_points_compact_f64 keeps the original order
(`xyz[mask]`), pgnn_points_in_boxes_f64 is the union-of-boxes mask of
remove_background / dilute_background.  Rotations about a pivot are three
pgnn_points_affine_f64 calls (shift, rotate, shift), i.e. the reference's three
roundings.  The two voxel-based methods (random_voxel_downsample,
dilute_background) reuse the float64 random-voxel keypoint entry
(graph_gen.keypoints_device): the voxelisation is the reference's
(`(xyz - min + jitter) // voxel` with NumPy's jitter draw); WHICH member of a
voxel survives is the reference's `random.choice` per voxel, here one seed
drawn from Python's `random` -- NumPy's stream ends where the reference's does,
Python's does not, and the survivors come in the device's voxel order.

Host reads: one per call whose output size the device decides (one per trial
in the box methods, the count that decides the trial); none where the host
knows the size (random_drop; the deletion of random_box_global_rotation).
dilute_background reads twice: the size of its front block, then the number of
occupied voxels.

`random_box_shift` tests a candidate position against the already placed boxes
with the reference's raster overlap (`nms.overlapped_boxes_3d`, nms.py:29-62:
cv2.fillPoly on the integer corner grid): `pgnn_overlapped_boxes_3d_raster`
produces cv2's pixel counts in closed form.  cv2 itself is absent from the
image; the fill rule is restated from OpenCV 4.2's drawing.cpp
(oracle/raster_oracle.py) and the fixtures come from the reference's own
preprocess.py / nms.py running on that restatement.
"""
import random
from copy import deepcopy

import numpy as np

from . import _lib
from . import kitti_dataset
from .kitti_dataset import Points


def _f64_points(cam_rgb_points):
    import torch
    xyz = cam_rgb_points.xyz
    if not isinstance(xyz, torch.Tensor):
        xyz = torch.as_tensor(np.asarray(xyz))
    if not xyz.is_cuda:
        xyz = xyz.cuda()
    if xyz.dtype != torch.float64:
        xyz = xyz.to(torch.float64)     # a copy: inputs stay untouched
    return xyz.contiguous()


def finish(cam_rgb_points):
    """train.py:124: the float32 cloud the graph builder receives."""
    import torch
    return Points(xyz=cam_rgb_points.xyz.to(torch.float32),
                  attr=cam_rgb_points.attr)


def _affine(xyz, rot=None, shift=None, select=None):
    import torch
    lib = _lib.load()
    r = np.ascontiguousarray(rot, np.float64) if rot is not None else None
    s = np.ascontiguousarray(shift, np.float64) if shift is not None else None
    with torch.cuda.device(xyz.device):
        _lib.check(lib.pgnn_points_affine_f64(
            _lib.ptr(xyz), int(xyz.shape[0]),
            r.ctypes.data if r is not None else None,
            s.ctypes.data if s is not None else None,
            _lib.ptr(select) if select is not None else None,
            _lib.stream_ptr()), "pgnn_points_affine_f64")


def _box_record(label, expend_factor):
    rec = np.zeros(24, np.float64)
    normals, lower, upper = kitti_dataset.box3d_to_normals(label, expend_factor)
    rec[0:9], rec[9:12], rec[12:15] = normals.reshape(-1), lower, upper
    rec[15] = 2.0
    return rec


def _in_box(xyz, label, expend_factor, exclude=None, want_mask=False):
    """(mask int32 [n] or None, count) of the points strictly inside the box
    (kitti_dataset.sel_xyz_in_box3d on the float64 cloud)."""
    import torch
    lib = _lib.load()
    rec = _box_record(label, expend_factor)
    n = int(xyz.shape[0])
    mask = torch.empty((n,), dtype=torch.int32, device=xyz.device) \
        if want_mask else None
    count = torch.zeros((1,), dtype=torch.int32, device=xyz.device)
    with torch.cuda.device(xyz.device):
        _lib.check(lib.pgnn_points_in_box_f64(
            _lib.ptr(xyz), n, rec.ctypes.data,
            _lib.ptr(exclude) if exclude is not None else None,
            _lib.ptr(mask) if mask is not None else None, _lib.ptr(count),
            _lib.stream_ptr()), "pgnn_points_in_box_f64")
    return mask, count


def _yaw_matrix(delta_yaw):
    c, s = np.cos(delta_yaw), np.sin(delta_yaw)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def random_rotation_all(cam_rgb_points, labels, method_name='normal',
                        yaw_std=0.3, expend_factor=(1.0, 1.1, 1.1)):
    """preprocess.py:44-66: one yaw rotation of the whole scene."""
    xyz = _f64_points(cam_rgb_points)
    if method_name == 'normal':
        delta_yaw = np.random.normal(scale=yaw_std)
    elif method_name == 'uniform':
        delta_yaw = np.random.uniform(low=-yaw_std, high=yaw_std)
    else:
        raise ValueError(method_name)
    rot = _yaw_matrix(delta_yaw)
    _affine(xyz, rot=rot)
    for label in labels:
        if label['name'] != 'DontCare':
            centre = np.array([[label['x3d'], label['y3d'], label['z3d']]])
            centre = centre.dot(np.transpose(rot))
            label['x3d'], label['y3d'], label['z3d'] = centre[0]
            label['yaw'] = label['yaw'] + delta_yaw
    return Points(xyz=xyz, attr=cam_rgb_points.attr), labels


def random_flip_all(cam_rgb_points, labels, flip_prob=0.5):
    """preprocess.py:68-77: mirror x with probability flip_prob."""
    xyz = _f64_points(cam_rgb_points)
    p = np.random.uniform()
    if p < flip_prob:
        _affine(xyz, rot=np.diag([-1.0, 1.0, 1.0]))
        for label in labels:
            if label['name'] != 'DontCare':
                label['x3d'] = -label['x3d']
                label['yaw'] = np.pi - label['yaw']
    return Points(xyz=xyz, attr=cam_rgb_points.attr), labels


_AUGMENT_LIST = ['Car', 'Pedestrian', 'Cyclist', 'Van', 'Truck', 'Misc',
                 'Tram', 'Person_sitting']


def _box7(label):
    return [label['x3d'], label['y3d'], label['z3d'], label['length'],
            label['height'], label['width'], label['yaw']]


def random_box_shift(cam_rgb_points, labels, max_overlap_num_allowed=0.1,
                     max_overlap_rate=None, max_trails=100, appr_factor=100,
                     method_name='normal', xyz_std=(1, 0, 1),
                     expend_factor=(1.0, 1.1, 1.1),
                     augment_list=_AUGMENT_LIST, shuffle=False):
    """preprocess.py:239-326: move each object (its box and the points inside
    it) by a random offset, retrying up to max_trails times until the new
    position swallows fewer than max_overlap_num_allowed foreign points and
    overlaps no already placed box by max_overlap_rate or more."""
    from . import nms
    xyz = _f64_points(cam_rgb_points)
    movable = [l for l in labels if l['name'] != 'DontCare']
    if shuffle:
        random.shuffle(movable)
    placed = []
    for label in movable:
        if label['name'] not in augment_list:
            placed.append(label)
            continue
        own, _ = _in_box(xyz, label, expend_factor, want_mask=True)
        accepted = None
        for _ in range(max_trails):
            if method_name == 'normal':
                delta = np.random.normal(scale=xyz_std)
            elif method_name == 'uniform':
                delta = np.random.uniform(low=-np.asarray(xyz_std),
                                          high=np.asarray(xyz_std))
            else:
                raise ValueError(method_name)
            moved = deepcopy(label)
            moved['x3d'] = moved['x3d'] + delta[0]
            moved['y3d'] = moved['y3d'] + delta[1]
            moved['z3d'] = moved['z3d'] + delta[2]
            _, extra = _in_box(xyz, moved, expend_factor, exclude=own)
            ok = int(extra.item()) < max_overlap_num_allowed
            if max_overlap_rate is not None and placed:
                # preprocess.py:281-301: integer corner grids (truncation of
                # appr_factor * corners), cv2 raster overlap against every
                # label placed so far -- shifted or not
                new_corners = np.int32(appr_factor * nms.boxes_3d_to_corners(
                    np.array([_box7(moved)])))
                placed_corners = np.int32(
                    appr_factor * nms.boxes_3d_to_corners(
                        np.array([_box7(l) for l in placed])))
                overlap = nms.overlapped_boxes_3d(new_corners[0],
                                                  placed_corners)
                ok = ok and bool(np.all(overlap < max_overlap_rate))
            if ok:
                _affine(xyz, shift=delta, select=own)
                accepted = moved
                break
        placed.append(accepted if accepted is not None else label)
    assert len(placed) == len(movable)
    placed.extend([l for l in labels if l['name'] == 'DontCare'])
    assert len(placed) == len(labels)
    return Points(xyz=xyz, attr=cam_rgb_points.attr), placed


def _in_boxes(xyz, labels, expend_factor, exclude=None):
    """(mask int32 [n], count int32 [1]) of the points strictly inside any of
    the labels' boxes (and, with `exclude`, not marked there): the
    `mask += sel_xyz_in_box3d(...)` loops of preprocess.py:359-360, :420-421."""
    import torch
    lib = _lib.load()
    n = int(xyz.shape[0])
    rec = np.zeros((max(len(labels), 1), 24), np.float64)
    for i, label in enumerate(labels):
        rec[i] = _box_record(label, expend_factor)
    rec_dev = torch.from_numpy(rec).to(xyz.device)
    mask = torch.empty((n,), dtype=torch.int32, device=xyz.device)
    count = torch.zeros((1,), dtype=torch.int32, device=xyz.device)
    with torch.cuda.device(xyz.device):
        _lib.check(lib.pgnn_points_in_boxes_f64(
            _lib.ptr(xyz), n, _lib.ptr(rec_dev), len(labels),
            _lib.ptr(exclude) if exclude is not None else None,
            _lib.ptr(mask), _lib.ptr(count), _lib.stream_ptr()),
            "pgnn_points_in_boxes_f64")
    return mask, count


def _attr_of(cam_rgb_points, xyz):
    """The float32 [n,a] device attributes that follow the cloud row for row
    (None stays None)."""
    import torch
    attr = cam_rgb_points.attr
    if attr is None:
        return None
    if not isinstance(attr, torch.Tensor):
        attr = torch.as_tensor(np.asarray(attr))
    attr = attr.to(device=xyz.device, dtype=torch.float32)
    if attr.dim() == 1:
        attr = attr.reshape(-1, 1)
    if int(attr.shape[0]) != int(xyz.shape[0]):
        raise ValueError("attr has %d rows, xyz %d" % (attr.shape[0],
                                                        xyz.shape[0]))
    return attr.contiguous()


def _compact(xyz, attr, n_out, keep=None, drop=None):
    """(xyz[m], attr[m]) for m = keep && !drop, in the original order
    (pgnn_points_compact_f64).  `n_out`, the number of kept rows, is known to
    the host at every call site -- nothing is read back."""
    import torch
    lib = _lib.load()
    n, dev = int(xyz.shape[0]), xyz.device
    a = int(attr.shape[1]) if attr is not None else 0
    if a > 4:
        raise NotImplementedError("more than 4 attribute columns")
    out_xyz = torch.empty((n_out, 3), dtype=torch.float64, device=dev)
    out_attr = torch.empty((n_out, a), dtype=torch.float32, device=dev) \
        if attr is not None else None
    ws_bytes = lib.pgnn_points_compact_workspace_bytes(n)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    count = torch.empty((1,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.pgnn_points_compact_f64(
            _lib.ptr(xyz), _lib.ptr(attr), a, n, _lib.ptr(keep),
            _lib.ptr(drop), _lib.ptr(ws), ws_bytes, _lib.ptr(out_xyz),
            _lib.ptr(out_attr), n_out, _lib.ptr(count), _lib.stream_ptr()),
            "pgnn_points_compact_f64")
    return out_xyz, out_attr


def _random_voxel(xyz, attr, voxel_size):
    """dataset/kitti_dataset.py:50-82 downsample_by_random_voxel(...,
    add_rnd3d=True) on the float64 cloud: one member per occupied voxel of
    `(xyz - min + voxel * np.random.random((1, 3))) // voxel`.  The jitter is
    NumPy's draw, like the reference's; the member choice (the reference's
    `random.choice` per voxel) is seeded from Python's `random`, so NumPy's
    stream is left where the reference leaves it.  One host read (the number
    of occupied voxels)."""
    from . import graph_gen
    if int(xyz.shape[0]) == 0:
        # np.amax of an empty array (kitti_dataset.py:52)
        raise ValueError("zero-size array to reduction operation maximum "
                         "which has no identity")
    jitter = voxel_size * np.random.random((1, 3))
    seed = random.getrandbits(63)
    kp_xyz, kp_idx = graph_gen.keypoints_device(
        xyz, float(voxel_size), 'random', jitter, seed)
    kp_attr = attr[kp_idx.reshape(-1).long()] if attr is not None else None
    return kp_xyz, kp_attr


def random_transition(cam_rgb_points, labels, xyz_std=(0.1, 0.1, 0.1)):
    """preprocess.py:430-440: one offset for the whole scene -- added to the
    centre of EVERY label, DontCare included (the reference does not
    filter)."""
    xyz = _f64_points(cam_rgb_points)
    x_delta = np.random.normal(scale=xyz_std[0])
    y_delta = np.random.normal(scale=xyz_std[1])
    z_delta = np.random.normal(scale=xyz_std[2])
    _affine(xyz, shift=[x_delta, y_delta, z_delta])
    for label in labels:
        label['x3d'] += x_delta
        label['y3d'] += y_delta
        label['z3d'] += z_delta
    return Points(xyz=xyz, attr=cam_rgb_points.attr), labels


def random_scale_all(cam_rgb_points, labels, method_name='normal',
                     scale_std=0.05):
    """preprocess.py:79-96: one scale factor for the points and for the
    centres and sizes of the objects."""
    xyz = _f64_points(cam_rgb_points)
    if method_name == 'normal':
        scale = np.random.normal(scale=scale_std) + 1.0
    elif method_name == 'uniform':
        scale = np.random.uniform(low=-scale_std, high=scale_std) + 1
    else:
        raise ValueError(method_name)
    _affine(xyz, rot=np.diag([scale, scale, scale]))   # x*s + y*0 + z*0
    for label in labels:
        if label['name'] != 'DontCare':
            for key in ('x3d', 'y3d', 'z3d', 'length', 'width', 'height'):
                label[key] *= scale
    return Points(xyz=xyz, attr=cam_rgb_points.attr), labels


def random_drop(cam_rgb_points, labels, drop_prob=0.5, tier_prob=None):
    """preprocess.py:19-27: drop every point with probability drop_prob (a
    list: one of its tiers, chosen with tier_prob); an attempt to drop all
    points keeps all.  The per-point uniforms are NumPy's host draw, uploaded
    as the keep mask, so the host knows the output size: no read back."""
    import torch
    if isinstance(drop_prob, list):
        drop_prob = np.random.choice(drop_prob, p=tier_prob)
    xyz = _f64_points(cam_rgb_points)
    attr = _attr_of(cam_rgb_points, xyz)
    mask = np.random.uniform(size=int(xyz.shape[0])) > drop_prob
    kept = int(np.sum(mask))
    if kept == 0 or kept == len(mask):
        return Points(xyz=xyz, attr=attr), labels
    keep = torch.from_numpy(mask.astype(np.int32)).to(xyz.device)
    xyz, attr = _compact(xyz, attr, kept, keep=keep)
    return Points(xyz=xyz, attr=attr), labels


def random_global_drop(cam_rgb_points, labels, drop_std=0.25):
    """preprocess.py:29-32."""
    drop_prob = np.abs(np.random.normal(scale=drop_std))
    return random_drop(cam_rgb_points, labels, drop_prob=drop_prob)


def random_voxel_downsample(cam_rgb_points, labels, voxel_std=0.2,
                            min_voxel=0.02, max_voxel=0.8):
    """preprocess.py:34-42: random-voxel downsample at a random voxel size;
    below min_voxel the cloud passes through with no further draw."""
    voxel_size = np.abs(np.random.normal(scale=voxel_std))
    voxel_size = np.minimum(voxel_size, max_voxel)
    xyz = _f64_points(cam_rgb_points)
    if voxel_size < min_voxel:
        return Points(xyz=xyz, attr=cam_rgb_points.attr), labels
    xyz, attr = _random_voxel(xyz, _attr_of(cam_rgb_points, xyz), voxel_size)
    return Points(xyz=xyz, attr=attr), labels


def _draw_yaw(method_name, yaw_std):
    if method_name == 'normal':
        return np.random.normal(scale=yaw_std)
    if method_name == 'uniform':
        return np.random.uniform(low=-yaw_std, high=yaw_std)
    raise ValueError(method_name)


def random_box_rotation(cam_rgb_points, labels, max_overlap_num_allowed=0.1,
                        max_trails=100, appr_factor=100, method_name='normal',
                        yaw_std=0.3, expend_factor=(1.0, 1.1, 1.1),
                        augment_list=_AUGMENT_LIST):
    """preprocess.py:98-164: turn each object (its box and the points inside
    it) about its own centre by a random yaw, retrying up to max_trails times
    until the turned box swallows fewer than max_overlap_num_allowed foreign
    points.  One host read per trial (the count that decides it)."""
    xyz = _f64_points(cam_rgb_points)
    new_labels = []
    for label in [l for l in labels if l['name'] != 'DontCare']:
        if label['name'] not in augment_list:
            new_labels.append(label)
            continue
        own, _ = _in_box(xyz, label, expend_factor, want_mask=True)
        accepted = None
        for _ in range(max_trails):
            delta_yaw = _draw_yaw(method_name, yaw_std)
            turned = deepcopy(label)
            turned['yaw'] = turned['yaw'] + delta_yaw
            _, extra = _in_box(xyz, turned, expend_factor, exclude=own)
            if int(extra.item()) < max_overlap_num_allowed:
                # (p - c).dot(R.T) + c, rounded after each of the three steps
                # like the reference's three NumPy statements (:143-148)
                centre = np.array([label['x3d'], label['y3d'], label['z3d']])
                _affine(xyz, shift=-centre, select=own)
                _affine(xyz, rot=_yaw_matrix(delta_yaw), select=own)
                _affine(xyz, shift=centre, select=own)
                accepted = turned
                break
        new_labels.append(accepted if accepted is not None else label)
    new_labels.extend([l for l in labels if l['name'] == 'DontCare'])
    assert len(new_labels) == len(labels)
    return Points(xyz=xyz, attr=cam_rgb_points.attr), new_labels


def random_box_global_rotation(cam_rgb_points, labels,
                               max_overlap_num_allowed=0.1, max_trails=100,
                               appr_factor=100, method_name='normal',
                               yaw_std=0.3, expend_factor=(1.1, 1.1, 1.1),
                               augment_list=_AUGMENT_LIST):
    """preprocess.py:167-236: turn each object about the ORIGIN (the label's
    centre and the points of its box) by a random yaw.  An accepted move
    deletes the foreign points its new box swallows (`new_mask & ~mask`) from
    the cloud and the attributes, so later objects see the shorter cloud.  One
    host read per trial; the deletion needs none (the count that decided the
    trial is the number of rows that go)."""
    xyz = _f64_points(cam_rgb_points)
    attr = _attr_of(cam_rgb_points, xyz)
    new_labels = []
    for label in [l for l in labels if l['name'] != 'DontCare']:
        if label['name'] not in augment_list:
            new_labels.append(label)
            continue
        own, _ = _in_box(xyz, label, expend_factor, want_mask=True)
        accepted = None
        for _ in range(max_trails):
            delta_yaw = _draw_yaw(method_name, yaw_std)
            turned = deepcopy(label)
            turned['yaw'] = turned['yaw'] + delta_yaw
            rot = _yaw_matrix(delta_yaw)
            turned['x3d'], turned['y3d'], turned['z3d'] = np.array(
                [turned['x3d'], turned['y3d'], turned['z3d']]).dot(
                    np.transpose(rot))
            more, extra = _in_boxes(xyz, [turned], expend_factor, exclude=own)
            n_more = int(extra.item())
            if n_more < max_overlap_num_allowed:
                _affine(xyz, rot=rot, select=own)
                if n_more > 0:
                    xyz, attr = _compact(xyz, attr, int(xyz.shape[0]) - n_more,
                                         drop=more)
                accepted = turned
                break
        new_labels.append(accepted if accepted is not None else label)
    new_labels.extend([l for l in labels if l['name'] == 'DontCare'])
    assert len(new_labels) == len(labels)
    return Points(xyz=xyz, attr=attr), new_labels


_KEEP_LIST = ['Car', 'Pedestrian', 'Cyclist', 'Van', 'Truck', 'Misc',
              'Person_sitting']


def _kept_labels(labels, keep_list):
    """preprocess.py:346-355 / :400-409: the labels named in keep_list; if
    there is none, every label that is not DontCare."""
    kept = [l for l in labels if l['name'] in keep_list]
    if len(kept) < 1:
        kept = [l for l in labels if l['name'] != 'DontCare']
    return kept


def _front_mask(xyz, selected, expend_factor):
    """(mask, number of front points): the union of the selected boxes; an
    empty union keeps point 0 (preprocess.py:363-365, :424-426).  The one host
    read of remove_background; the first of dilute_background's two."""
    mask, count = _in_boxes(xyz, selected, expend_factor)
    n_front = int(count.item())
    if n_front == 0:
        mask[0] = 1     # IndexError on an empty cloud, like the reference
        n_front = 1
    return mask, n_front


def remove_background(cam_rgb_points, labels, expend_factor=(4.0, 4.0, 4.0),
                      keep_list=_KEEP_LIST, num_object=-1,
                      mask_random_rotation_std=0,
                      mask_random_jitter_stds=(0., 0., 0., 0., 0., 0.)):
    """preprocess.py:380-428: keep only the points inside the (expanded)
    boxes of the kept labels -- of num_object of them, sampled with
    replacement, when num_object > 0.  Returns the filtered label list."""
    xyz = _f64_points(cam_rgb_points)
    attr = _attr_of(cam_rgb_points, xyz)
    kept = _kept_labels(labels, keep_list)
    if num_object > 0:
        sample_idx = np.random.choice(len(kept), num_object)
        selected = [kept[i] for i in sample_idx]
    else:
        selected = kept
    mask, n_front = _front_mask(xyz, selected, expend_factor)
    xyz, attr = _compact(xyz, attr, n_front, keep=mask)
    return Points(xyz=xyz, attr=attr), kept


def dilute_background(cam_rgb_points, labels, dilute_voxel_base=0.4,
                      expend_factor=(4.0, 4.0, 4.0), keep_list=_KEEP_LIST):
    """preprocess.py:328-378: the points inside the (expanded) boxes of the
    kept labels in their original order, followed by a random-voxel
    downsample of all the others.  An empty background raises ValueError like
    the reference's np.amax of an empty array.  Two host reads: the size of
    the front block, then the number of occupied background voxels (the voxel
    entry takes its input size from the host)."""
    import torch
    xyz = _f64_points(cam_rgb_points)
    attr = _attr_of(cam_rgb_points, xyz)
    kept = _kept_labels(labels, keep_list)
    mask, n_front = _front_mask(xyz, kept, expend_factor)
    n_back = int(xyz.shape[0]) - n_front
    if n_back == 0:
        raise ValueError("zero-size array to reduction operation maximum "
                         "which has no identity")
    front_xyz, front_attr = _compact(xyz, attr, n_front, keep=mask)
    back_xyz, back_attr = _compact(xyz, attr, n_back, drop=mask)
    back_xyz, back_attr = _random_voxel(back_xyz, back_attr, dilute_voxel_base)
    return Points(
        xyz=torch.cat([front_xyz, back_xyz], dim=0),
        attr=torch.cat([front_attr, back_attr], dim=0)
        if attr is not None else None), kept


def empty(cam_rgb_points, labels):
    return cam_rgb_points, labels


def _not_implemented(name):
    def fn(*args, **kwargs):
        raise NotImplementedError(
            "%s has no device path and is deliberately left out: every other "
            "entry of the reference's aug_method_map is implemented" % name)
    return fn


# preprocess.py:446-460
aug_method_map = {
    'random_jitter': _not_implemented('random_jitter'),
    'random_box_rotation': random_box_rotation,
    'random_box_shift': random_box_shift,
    'random_transition': random_transition,
    'remove_background': remove_background,
    'random_rotation_all': random_rotation_all,
    'random_flip_all': random_flip_all,
    'random_drop': random_drop,
    'random_global_drop': random_global_drop,
    'random_voxel_downsample': random_voxel_downsample,
    'random_scale_all': random_scale_all,
    'random_box_global_rotation': random_box_global_rotation,
    'dilute_background': dilute_background,
}


def get_data_aug(aug_configs=[]):
    """preprocess.py:461-471."""
    if len(aug_configs) == 0:
        return empty

    def multiple_aug(cam_rgb_points, labels):
        for aug_config in aug_configs:
            method = aug_method_map[aug_config['method_name']]
            cam_rgb_points, labels = method(cam_rgb_points, labels,
                                            **aug_config['method_kwargs'])
        return cam_rgb_points, labels
    return multiple_aug
