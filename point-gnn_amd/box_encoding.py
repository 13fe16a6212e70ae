"""Box codec of the reference (models/box_encoding.py) on the GPU.

Same registry (`get_box_encoding_fn` / `get_box_decoding_fn` /
`get_encoding_len`, box_encoding.py:469-508) and the same call signature
`fn(cls_labels [R,1], points_xyz [R,3], boxes [R,B,7], label_map)`.  Both keys
a reference config can select are implemented:

  'classaware_all_class_box_encoding'            box_encoding.py:231-299, the
      method of every shipped config: offset / median size, log size ratio,
      yaw relative to the anchor in units of pi/4;
  'classaware_all_class_box_canonical_encoding'  box_encoding.py:301-395: the
      same, with the (x, z) offset rotated into the anchor's own frame by the
      relative yaw `a` and divided by (l, w) for a horizontal anchor, (w, l)
      for a vertical one (the reference's swap, :331-337).

The other four keys (`direct_encoding`, `center_box_encoding`,
`voxelnet_box_encoding`, `classaware_voxelnet_box_encoding`) raise
NotImplementedError: they take three arguments (box_encoding.py:5-208) while
every caller of the reference passes four (train.py:123-124, eval.py:106-107,
run.py:276-277), so no reference config can run with them either.

NumPy in -> NumPy out, CUDA tensors in -> CUDA tensors out, inputs are never
written; the arithmetic runs in libpointgnn_hip.so
(`pgnn_box_{decode,encode}[_canonical]_f32`), float32 like the reference's
NumPy code on its float32 network outputs: cos/sin/exp/log in double on the
float32 argument and rounded once, everything else float32 in the reference's
operation order.  float64 boxes (the training targets) select the float64
encoders (`pgnn_box_encode[_canonical]_f64[_xyz64]`), rounded to float32 once.
"""
import math

import numpy as np

from . import _lib

# box_encoding.py:210-220 -- (l, h, w) medians of the KITTI classes
median_object_size_map = {
    'Cyclist': (1.76, 1.75, 0.6),
    'Van': (4.98, 2.13, 1.88),
    'Tram': (14.66, 3.61, 2.6),
    'Car': (3.88, 1.5, 1.63),
    'Misc': (2.52, 1.65, 1.51),
    'Pedestrian': (0.88, 1.77, 0.65),
    'Truck': (10.81, 3.34, 2.63),
    'Person_sitting': (0.75, 1.26, 0.59),
}


def class_table(label_map, dtype=np.float32):
    """[n,5] rows {l, h, w, yaw_offset, active} indexed by label value
    (box_encoding.py:239-262,268-291: label -> horizontal anchor, label+1 ->
    the same size turned by pi/2).  Later label_map entries overwrite earlier
    ones like the reference's loop does."""
    rows = {}
    for name, label in label_map.items():
        if name in ("Background", "DontCare"):
            continue
        l, h, w = median_object_size_map[name]
        rows[int(label)] = (l, h, w, 0.0)
        rows[int(label) + 1] = (l, h, w, 0.5 * math.pi)
    n = (max(rows) + 1) if rows else 0
    table = np.zeros((n, 5), dtype)
    for label, (l, h, w, yaw) in rows.items():
        table[label] = (l, h, w, yaw, 1.0)
    return table


_TABLES = {}


def _device_table(label_map, dtype, dev):
    """class_table(label_map) on `dev`, uploaded once per (map, dtype, device):
    the frame loop decodes every frame with the same table."""
    import torch
    key = (tuple(sorted(label_map.items())), np.dtype(dtype).str, str(dev))
    t = _TABLES.get(key)
    if t is None:
        t = _TABLES[key] = torch.from_numpy(class_table(label_map, dtype)).to(dev)
        torch.cuda.current_stream(dev).synchronize()   # used on any stream
    return t


PLAIN = 'classaware_all_class_box_encoding'
CANONICAL = 'classaware_all_class_box_canonical_encoding'

# (method, direction) -> C entries for (float32 boxes, float64 boxes with
# float32 vertices, float64 boxes with float64 vertices); decoding is float32
# only (network outputs)
_ENTRIES = {
    (PLAIN, 'encode'): ("pgnn_box_encode_f32", "pgnn_box_encode_f64",
                        "pgnn_box_encode_f64_xyz64"),
    (PLAIN, 'decode'): ("pgnn_box_decode_f32", None, None),
    (CANONICAL, 'encode'): ("pgnn_box_encode_canonical_f32",
                            "pgnn_box_encode_canonical_f64",
                            "pgnn_box_encode_canonical_f64_xyz64"),
    (CANONICAL, 'decode'): ("pgnn_box_decode_canonical_f32", None, None),
}


def _run(method, direction, cls_labels, points_xyz, boxes, label_map):
    import torch
    lib = _lib.load()
    entry32, entry64, entry64_xyz64 = _ENTRIES[method, direction]
    as_numpy = not isinstance(boxes, torch.Tensor)
    dev = boxes.device if not as_numpy else torch.device("cuda", 0)
    if dev.type != "cuda":
        raise _lib.PointGnnHipError(
            "box codec runs on the GPU only (no CPU fallback)")

    def to(x, dtype):
        return torch.as_tensor(np.asarray(x) if not isinstance(
            x, torch.Tensor) else x).to(device=dev, dtype=dtype).contiguous()

    def is_f64(x):
        return (x.dtype == torch.float64) if isinstance(x, torch.Tensor) \
            else np.asarray(x).dtype == np.float64

    # float64 ground-truth boxes (kitti_dataset.py:1199 np.zeros default) are
    # encoded in float64 and rounded once, like train.py:120-130
    wide = entry64 is not None and is_f64(boxes)
    if wide:
        b = to(boxes, torch.float64)
        rows, per_row = int(b.shape[0]), int(b.shape[1])
        lab = to(cls_labels, torch.int32).reshape(-1)
        # float64 vertices (the training path, train.py:120-122) are used
        # as they are; float32 ones are widened inside the kernel
        xyz64 = is_f64(points_xyz)
        xyz = to(points_xyz, torch.float64 if xyz64 else torch.float32)
        table = _device_table(label_map, np.float64, dev)
        out = torch.empty(tuple(b.shape), dtype=torch.float32, device=dev)
        entry = entry64_xyz64 if xyz64 else entry64
        with torch.cuda.device(dev):
            _lib.check(getattr(lib, entry)(
                _lib.ptr(lab), _lib.ptr(xyz), _lib.ptr(b), _lib.ptr(table),
                int(table.shape[0]), rows, per_row, _lib.ptr(out),
                _lib.stream_ptr()), entry)
        return out.cpu().numpy() if as_numpy else out
    b = to(boxes, torch.float32)
    if b.dim() != 3 or b.shape[2] != 7:
        raise ValueError("boxes must be [R, B, 7]")
    rows, per_row = int(b.shape[0]), int(b.shape[1])
    lab = to(cls_labels, torch.int32).reshape(-1)
    xyz = to(points_xyz, torch.float32)
    if lab.numel() != rows or tuple(xyz.shape) != (rows, 3):
        raise ValueError("cls_labels [R,1] / points_xyz [R,3] do not match boxes")
    table = _device_table(label_map, np.float32, dev)
    out = torch.empty_like(b)
    with torch.cuda.device(dev):
        _lib.check(getattr(lib, entry32)(
            _lib.ptr(lab), _lib.ptr(xyz), _lib.ptr(b), _lib.ptr(table),
            int(table.shape[0]), rows, per_row, _lib.ptr(out),
            _lib.stream_ptr()), entry32)
    return out.cpu().numpy() if as_numpy else out


def classaware_all_class_box_encoding(cls_labels, points_xyz, boxes_3d,
                                      label_map):
    """box_encoding.py:231-263."""
    return _run(PLAIN, 'encode', cls_labels, points_xyz, boxes_3d, label_map)


def classaware_all_class_box_decoding(cls_labels, points_xyz, encoded_boxes,
                                      label_map):
    """box_encoding.py:265-299."""
    return _run(PLAIN, 'decode', cls_labels, points_xyz, encoded_boxes,
                label_map)


def classaware_all_class_box_canonical_encoding(cls_labels, points_xyz,
                                                boxes_3d, label_map):
    """box_encoding.py:301-343: the offset box centre - vertex rotated into the
    anchor's frame (by the yaw for a horizontal anchor, yaw - pi/2 for a
    vertical one) and divided by (l, w) resp. (w, l)."""
    return _run(CANONICAL, 'encode', cls_labels, points_xyz, boxes_3d,
                label_map)


def classaware_all_class_box_canonical_decoding(cls_labels, points_xyz,
                                                encoded_boxes, label_map):
    """box_encoding.py:345-395."""
    return _run(CANONICAL, 'decode', cls_labels, points_xyz, encoded_boxes,
                label_map)


_METHODS = ('direct_encoding', 'center_box_encoding', 'voxelnet_box_encoding',
            'classaware_voxelnet_box_encoding', PLAIN, CANONICAL)
_ENCODERS = {PLAIN: classaware_all_class_box_encoding,
             CANONICAL: classaware_all_class_box_canonical_encoding}
_DECODERS = {PLAIN: classaware_all_class_box_decoding,
             CANONICAL: classaware_all_class_box_canonical_decoding}


def _lookup(name, fns):
    if name not in _METHODS:
        raise KeyError(name)
    if name not in fns:
        raise NotImplementedError(
            "%s: the reference's callers pass (cls_labels, xyz, boxes, "
            "label_map) to every codec (train.py:123-124, eval.py:106-107, "
            "run.py:276-277) and this one takes three arguments "
            "(box_encoding.py:5-208), so no config can select it there "
            "either; only %r and %r have HIP implementations"
            % (name, PLAIN, CANONICAL))
    return fns[name]


def get_box_encoding_fn(encoding_method_name):
    return _lookup(encoding_method_name, _ENCODERS)


def get_box_decoding_fn(encoding_method_name):
    return _lookup(encoding_method_name, _DECODERS)


def get_encoding_len(encoding_method_name):
    if encoding_method_name not in _METHODS:
        raise KeyError(encoding_method_name)
    return 7
