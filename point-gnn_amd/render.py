"""Headless visualisation: what the reference's `run.py -l 1|2` shows in an
open3d window and a cv2 image (:152-175, :328-359, :410-421, :434-535), drawn
into uint8 RGB images on the device and written as PNG or PPM files.

The rasteriser (csrc/render.hip, include/pointgnn_hip.h "rendering") has
defined, integer-exact semantics: points with a depth test, line segments with
a fixed midpoint rule and the later segment on top, segments over points over
the background.  Text (`cv2.putText`) is a pass over a finished image,
`draw_text`, with the library's own 5 x 7 bitmap font; `render_frame(...,
text=True)` writes the reference's 'P | 0.873' beside every detection.  Not
drawn: the interactive 3D window.

    view = bev_view()                                 # 800 x 800, forward is up
    img = render(view, points=xyz, point_colors=colorize(inten, 0, 1),
                 segments=box_segments(boxes), segment_colors=(255, 0, 0))
    write_png('frame.png', img)           # encoder='device': deflate on the GPU
    draw_text(img, ['C | 0.912'], [(40, 120)], colors=(0, 255, 0))
    render_results(dataset, result_dir, render_dir, views=('bev', 'camera'))
    python -m pointgnn_amd.render DATASET_DIR RESULT_DIR RENDER_DIR --view bev
        [--text]

Every box in the colour of its outcome in the KITTI matching (kitti_eval.match,
DESIGN.md section 9.13; tags and colours: OUTCOME_TAGS, OUTCOME_COLORS):

    errors = kitti_eval.match(gt, det, '3d', 'Car', 'moderate', score_threshold=t)
    render_frame(dataset, f, det[f], gt[f], outcomes=errors.frame(f), text=True)
    render_results(dataset, result_dir, render_dir, errors={'cls': 'Car'})
    python -m pointgnn_amd.render ... --errors [--at-threshold f1|<float>]
        [--show-below]

NumPy arrays or CUDA tensors go in, a uint8 [H, W, 3] CUDA tensor comes out.
"""
import math
import os
import struct
import zlib
from collections import namedtuple

import numpy as np

from . import _header, _lib

MAX_DIM = _header.constants()["PGNN_RENDER_MAX_DIM"]

# run.py:176-178 (there divided by 255 for open3d)
CLASS_COLORS = np.array([(211, 211, 211), (255, 0, 0), (255, 20, 147),
                         (65, 244, 101), (169, 244, 65), (65, 79, 244),
                         (65, 181, 244), (229, 244, 66)], dtype=np.uint8)
# run.py:180-189
GT_COLORS = {
    'Pedestrian': (0, 255, 255),
    'Person_sitting': (218, 112, 214),
    'Car': (154, 205, 50),
    'Truck': (255, 215, 0),
    'Van': (255, 20, 147),
    'Tram': (250, 128, 114),
    'Misc': (128, 0, 128),
    'Cyclist': (255, 165, 0),
}
DETECTION_COLOR = (255, 0, 0)    # boxes_3d_to_line_set's default colour
RECT_COLOR = (0, 255, 0)         # run.py:411-413
# cv2.putText's colours of run.py:417 / :421, BGR there: [is a Pedestrian]
DETECTION_TEXT_COLORS = ((0, 255, 0), (0, 255, 255))

# the twelve edges of a box, kitti_dataset.py:807-810
BOX_EDGES = np.array([[0, 1], [0, 4], [0, 3], [1, 2], [1, 5], [2, 3],
                      [2, 6], [3, 7], [4, 5], [4, 7], [5, 6], [6, 7]])


def _tables():
    i = np.arange(256, dtype=np.int64)
    gray = np.stack([i, i, i], axis=1).astype(np.uint8)

    def tri(centre):   # 1.5 - |4 x - c| of the classic blue-to-red ramp, in 1/255
        return np.clip(382 - np.abs(4 * i - centre), 0, 255)
    ramp = np.stack([tri(765), tri(510), tri(255)], axis=1).astype(np.uint8)
    return gray, ramp


GRAY_TABLE, RAMP_TABLE = _tables()

View = namedtuple('View', ['m', 'd', 'near', 'width', 'height'])


def _view(m, d, near, width, height):
    m = np.ascontiguousarray(np.asarray(m, dtype=np.float64).reshape(3, 4))
    d = np.ascontiguousarray(np.asarray(d, dtype=np.float64).reshape(4))
    return View(m, d, float(near), int(width), int(height))


def camera_view(calib, image_size):
    """The camera image: M = calib['cam_to_image'], depth = z, near 0.1;
    image_size = (width, height)."""
    return _view(calib['cam_to_image'], (0.0, 0.0, 1.0, 0.0), 0.1,
                 image_size[0], image_size[1])


def bev_view(x_range=(-40, 40), z_range=(0, 80), scale=10.0):
    """Bird's eye view of the camera frame, forward (z) up, `scale` pixels
    per metre.  Camera y points down: the smallest depth is the highest
    point."""
    xmin, xmax = float(x_range[0]), float(x_range[1])
    zmin, zmax = float(z_range[0]), float(z_range[1])
    s = float(scale)
    m = [[s, 0.0, 0.0, -s * xmin], [0.0, 0.0, -s, s * zmax],
         [0.0, 0.0, 0.0, 1.0]]
    return _view(m, (0.0, 1.0, 0.0, 0.0), 0.5,
                 math.ceil((xmax - xmin) * s), math.ceil((zmax - zmin) * s))


def pixel_view(width, height):
    """(x, y, anything) is pixel (floor(x), floor(y)): for 2D overlays such
    as rect_segments."""
    m = [[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0]]
    return _view(m, (0.0, 0.0, 0.0, 0.0), 0.5, width, height)


# ---- device plumbing ---------------------------------------------------------
def _device(*things):
    import torch
    for t in things:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            return t.device
    return torch.device("cuda", torch.cuda.current_device())


def _coords(a, dev, tail, what):
    """-> contiguous float32 or float64 CUDA tensor [n, *tail]."""
    import torch
    if _lib.count_of(a) is not None:
        raise ValueError("%s is in capacity form: slice it to its count first"
                         % what)
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(
        np.ascontiguousarray(a))
    if t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float64)
    t = t.to(dev).contiguous()
    if tuple(t.shape[1:]) != tuple(tail):
        raise ValueError("%s must be [n, %s], got shape %r" % (
            what, ", ".join(str(x) for x in tail), tuple(t.shape)))
    return t


def _colors(c, n, dev, what):
    """None / one colour / [n, 3] -> (uint8 CUDA tensor [k, 3], k); k is 1 or
    n (0 when there is nothing to colour)."""
    import torch
    if c is None:
        c = (255, 255, 255)
    t = c if isinstance(c, torch.Tensor) else torch.from_numpy(
        np.ascontiguousarray(np.asarray(c)))
    if t.dtype != torch.uint8:
        if not isinstance(c, torch.Tensor):
            a = np.asarray(c)
            if a.size and (a.min() < 0 or a.max() > 255):
                raise ValueError("%s must be 0..255" % what)
        t = t.to(torch.uint8)
    t = t.to(dev).reshape(-1, 3).contiguous()
    k = int(t.shape[0])
    if k != 1 and k != n:
        raise ValueError("%s must be one colour or [%d, 3], got %d rows" % (
            what, n, k))
    return t, k


def _check_canvas(view):
    if not (1 <= view.width <= MAX_DIM and 1 <= view.height <= MAX_DIM):
        raise ValueError("canvas %d x %d: width and height must be 1..%d" % (
            view.width, view.height, MAX_DIM))


def _host_ptr(a):
    return a.ctypes.data_as(_lib.c_vp)


def colorize(values, lo, hi, table=None):
    """values [n] (float32 / float64) -> uint8 [n, 3] CUDA tensor:
    table[clamp(floor((v - lo) / (hi - lo) * 255), 0, 255)], NaN -> table[0];
    table uint8 [256, 3], default GRAY_TABLE."""
    import torch
    lib = _lib.load()
    dev = _device(values)
    v = values if isinstance(values, torch.Tensor) else torch.from_numpy(
        np.ascontiguousarray(values))
    if v.dtype not in (torch.float32, torch.float64):
        v = v.to(torch.float64)
    v = v.to(dev).reshape(-1).contiguous()
    tab = GRAY_TABLE if table is None else table
    tab = tab if isinstance(tab, torch.Tensor) else torch.from_numpy(
        np.ascontiguousarray(tab))
    if tab.dtype != torch.uint8 or tuple(tab.shape) != (256, 3):
        raise ValueError("table must be uint8 [256, 3]")
    tab = tab.to(dev).contiguous()
    n = int(v.shape[0])
    out = torch.empty((n, 3), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.pgnn_render_colorize(
            _lib.ptr(v), int(v.dtype == torch.float64), n, float(lo),
            float(hi), _lib.ptr(tab), _lib.ptr(out), _lib.stream_ptr()),
            "pgnn_render_colorize")
    return out


def class_colors(labels):
    """run.py:176-178, :332-333: class index [n] -> uint8 [n, 3] (a CUDA
    tensor for a CUDA tensor, else NumPy)."""
    import torch
    if isinstance(labels, torch.Tensor):
        tab = torch.from_numpy(CLASS_COLORS).to(labels.device)
        return tab[labels.long()]
    return CLASS_COLORS[np.asarray(labels, dtype=np.int64)]


def render(view, points=None, point_colors=None, point_size=1, segments=None,
           segment_colors=None, thickness=1, background=None):
    """One image of `view`: points [n, 3] with point_colors ([n, 3] uint8 or
    one colour, default white), segments [S, 2, 3] with segment_colors and
    thickness (1..3, or uint8 [S]), over background (uint8 [H, W, 3] or one
    colour, default black).  Order within an argument is stacking order:
    concatenate several sets.  Returns a uint8 [H, W, 3] CUDA tensor; nothing
    is read back."""
    import torch
    lib = _lib.load()
    _check_canvas(view)
    if isinstance(point_size, bool) or int(point_size) != point_size or \
            not 1 <= point_size <= 3:
        raise ValueError("point_size must be 1, 2 or 3, got %r" % (point_size,))
    dev = _device(points, segments, background)
    w, h = view.width, view.height
    view_m = np.ascontiguousarray(view.m, dtype=np.float64)
    view_d = np.ascontiguousarray(view.d, dtype=np.float64)
    if view_m.size != 12 or view_d.size != 4:
        raise ValueError("a view has a [3, 4] matrix and a [4] depth row")
    n = s = 0
    if points is not None:
        pts = _coords(points, dev, (3,), "points")
        n = int(pts.shape[0])
    if segments is not None:
        seg = _coords(segments, dev, (2, 3), "segments")
        s = int(seg.shape[0])
    pcol, n_pcol = _colors(point_colors, n, dev, "point_colors")
    scol, n_scol = _colors(segment_colors, s, dev, "segment_colors")
    thick_t, thick = None, 1
    if isinstance(thickness, (int, np.integer)) and \
            not isinstance(thickness, bool):
        thick = int(thickness)
        if not 1 <= thick <= 3:
            raise ValueError("thickness must be 1, 2 or 3, got %d" % thick)
    else:
        if not isinstance(thickness, torch.Tensor):
            a = np.asarray(thickness)
            if a.size and (a.min() < 1 or a.max() > 3):
                raise ValueError("thickness values must be 1, 2 or 3")
            thickness = torch.from_numpy(np.ascontiguousarray(
                a.astype(np.uint8)))
        thick_t = thickness.to(device=dev, dtype=torch.uint8).reshape(
            -1).contiguous()
        if int(thick_t.shape[0]) != s:
            raise ValueError("thickness must be one value or [%d]" % s)
    bg_t, bg_rgb = None, 0
    if background is not None:
        b = background if isinstance(background, torch.Tensor) else \
            torch.from_numpy(np.ascontiguousarray(np.asarray(background)))
        if b.numel() == 3 and b.dim() == 1:
            r, g, bl = (int(x) for x in b.tolist())
            if min(r, g, bl) < 0 or max(r, g, bl) > 255:
                raise ValueError("background must be 0..255")
            bg_rgb = r << 16 | g << 8 | bl
        else:
            if b.dtype != torch.uint8 or tuple(b.shape) != (h, w, 3):
                raise ValueError("background must be one colour or uint8 "
                                 "[%d, %d, 3], got %s %r" % (
                                     h, w, b.dtype, tuple(b.shape)))
            bg_t = b.to(dev).contiguous()
    image = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        ws_bytes = int(lib.pgnn_render_workspace_bytes(w, h))
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
        stream = _lib.stream_ptr()
        _lib.check(lib.pgnn_render_clear(w, h, _lib.ptr(ws), ws_bytes, stream),
                   "pgnn_render_clear")
        if n:
            _lib.check(lib.pgnn_render_points(
                _lib.ptr(pts), int(pts.dtype == torch.float64), n,
                _host_ptr(view_m), _host_ptr(view_d), float(view.near), w, h,
                int(point_size), _lib.ptr(ws), ws_bytes, stream),
                "pgnn_render_points")
        if s:
            _lib.check(lib.pgnn_render_segments(
                _lib.ptr(seg), int(seg.dtype == torch.float64), s,
                _host_ptr(view_m), float(view.near), w, h, _lib.ptr(thick_t),
                thick,
                _lib.ptr(ws), ws_bytes, stream), "pgnn_render_segments")
        _lib.check(lib.pgnn_render_resolve(
            w, h, _lib.ptr(ws), ws_bytes, _lib.ptr(pcol) if n else None,
            n_pcol if n else 0, _lib.ptr(scol) if s else None,
            n_scol if s else 0, _lib.ptr(bg_t), bg_rgb, _lib.ptr(image),
            stream), "pgnn_render_resolve")
    return image


# ---- text ----------------------------------------------------------------------------
FONT_FIRST, FONT_GLYPHS, FONT_ROWS, FONT_COLS = 0x20, 95, 7, 5
MAX_SCALE = 4
_I32_MIN, _I32_MAX = -2 ** 31, 2 ** 31 - 1


def font_table():
    """The library's font (pgnn_render_font): uint8 [95, 7], one row mask per
    byte for the codes 0x20..0x7E; bit 4 is the leftmost of the 5 columns,
    row 0 the top.  Read from the library: there is no copy here."""
    out = np.zeros((FONT_GLYPHS, FONT_ROWS), dtype=np.uint8)
    _lib.check(_lib.load().pgnn_render_font(_host_ptr(out)),
               "pgnn_render_font")
    return out


def _check_scale(scale):
    if isinstance(scale, bool) or int(scale) != scale or \
            not 1 <= scale <= MAX_SCALE:
        raise ValueError("scale must be 1..%d, got %r" % (MAX_SCALE, scale))
    return int(scale)


def text_size(string, scale=1):
    """(width, height) in pixels of `string` drawn at `scale`:
    ((6 len - 1) scale, 7 scale); (0, 0) for an empty string."""
    scale = _check_scale(scale)
    n = len(string)
    return ((6 * n - 1) * scale, 7 * scale) if n else (0, 0)


def _text_bytes(s):
    if isinstance(s, (bytes, bytearray)):
        return bytes(s)
    if isinstance(s, str):
        return s.encode('latin-1', errors='replace')
    raise ValueError("strings are str or bytes, got %r" % (s,))


def draw_text(image, strings, anchors, colors=(255, 255, 255), scale=1,
              plate=None, anchor='bl'):
    """Draws `strings` into `image` (a CUDA uint8 [H, W, 3] tensor, modified
    IN PLACE and returned) with the built-in 5 x 7 font, as cv2.putText draws
    into its image (include/pointgnn_hip.h, "text").  strings: a list of str
    (encoded latin-1, what it cannot encode becomes '?') or bytes; anchors
    [n, 2] integer (x, y): with anchor='bl' the bottom left of the text, cv2's
    `org` (the top left is (x, y - 7 scale)), with 'tl' its top left.  scale:
    1..4, one value or one per string; colors: one colour or [n, 3]; plate:
    None, one colour or [n, 3] -- a filled rectangle one `scale` wider than
    the text on every side, under its glyphs.  Later strings cover earlier
    ones.  Nothing is read back."""
    import torch
    lib = _lib.load()
    if not (isinstance(image, torch.Tensor) and image.is_cuda and
            image.dtype == torch.uint8 and image.dim() == 3 and
            image.shape[2] == 3 and image.is_contiguous()):
        raise ValueError("image must be a contiguous CUDA uint8 [H, W, 3] "
                         "tensor, got %r" % (
                             (image.dtype, tuple(image.shape))
                             if isinstance(image, torch.Tensor)
                             else type(image),))
    h, w = int(image.shape[0]), int(image.shape[1])
    if not (1 <= w <= MAX_DIM and 1 <= h <= MAX_DIM):
        raise ValueError("canvas %d x %d: width and height must be 1..%d" % (
            w, h, MAX_DIM))
    if anchor not in ('bl', 'tl'):
        raise ValueError("anchor must be 'bl' or 'tl', got %r" % (anchor,))
    if isinstance(strings, (str, bytes, bytearray)):
        raise ValueError("strings must be a list of str or bytes")
    data = [_text_bytes(s) for s in strings]
    n = len(data)
    dev = image.device
    if isinstance(anchors, torch.Tensor):
        anc = anchors.to(device=dev, dtype=torch.int64)
    else:
        a = np.asarray(anchors)
        if a.size and a.dtype.kind not in 'iu':
            raise ValueError("anchors must be integers, got %s" % a.dtype)
        if a.size and (a.min() < _I32_MIN or a.max() > _I32_MAX):
            raise ValueError("anchors must fit int32, got %d .. %d" % (
                a.min(), a.max()))
        anc = torch.from_numpy(np.ascontiguousarray(
            a.astype(np.int64))).to(dev)
    if anc.numel() != 2 * n:
        raise ValueError("anchors must be [%d, 2], got shape %r" % (
            n, tuple(anc.shape)))
    anc = anc.reshape(n, 2)
    scale_t, scale_1 = None, 1
    if isinstance(scale, (int, np.integer)):
        scale_1 = _check_scale(scale)
    else:
        if not isinstance(scale, torch.Tensor):
            a = np.asarray(scale)
            if a.size and (a.min() < 1 or a.max() > MAX_SCALE):
                raise ValueError("scale values must be 1..%d, got %d .. %d" % (
                    MAX_SCALE, a.min(), a.max()))
            scale = torch.from_numpy(np.ascontiguousarray(a.astype(np.uint8)))
        scale_t = scale.to(device=dev, dtype=torch.uint8).reshape(
            -1).contiguous()
        if int(scale_t.shape[0]) != n:
            raise ValueError("scale must be one value or [%d], got %d" % (
                n, int(scale_t.shape[0])))
    col, n_col = _colors(colors, n, dev, "colors")
    plate_t, n_plate = None, 0
    if plate is not None:
        plate_t, n_plate = _colors(plate, n, dev, "plate")
    lengths = np.array([len(d) for d in data], dtype=np.int64)
    total = int(lengths.sum())
    if total > _I32_MAX:
        raise ValueError("%d characters: the total must be below 2^31" % total)
    if n == 0 or total == 0:
        return image
    if anchor == 'bl':
        anc = anc.clone()
        anc[:, 1] -= FONT_ROWS * (scale_t.to(torch.int64)
                                  if scale_t is not None else scale_1)
    # a top edge below int32 is far off the canvas either way
    anc = anc.clamp(_I32_MIN, _I32_MAX).to(torch.int32).contiguous()
    offsets = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(lengths, out=offsets[1:])
    chars = torch.from_numpy(np.frombuffer(b"".join(data), dtype=np.uint8)
                             .copy()).to(dev)
    offsets = torch.from_numpy(offsets).to(dev)
    with torch.cuda.device(dev):
        ws_bytes = int(lib.pgnn_render_text_workspace_bytes(w, h))
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
        _lib.check(lib.pgnn_render_text(
            _lib.ptr(image), w, h, _lib.ptr(chars), _lib.ptr(offsets), n,
            _lib.ptr(anc), _lib.ptr(scale_t), scale_1, _lib.ptr(col),
            n_col, _lib.ptr(plate_t), n_plate, _lib.ptr(ws),
            ws_bytes, _lib.stream_ptr()), "pgnn_render_text")
    return image


# ---- segments of boxes, rectangles and graphs ----------------------------------
def box_corners(boxes_3d):
    """[m, 7] (x, y, z, l, h, w, yaw) -> [m, 8, 3] float64, the corners of
    boxes_3d_to_line_set (kitti_dataset.py:795-804; those of
    kitti_dataset.box3d_to_cam_points)."""
    boxes = np.asarray(boxes_3d, dtype=np.float64).reshape(-1, 7)
    out = np.empty((len(boxes), 8, 3), dtype=np.float64)
    for i, (x, y, z, l, h, w, yaw) in enumerate(boxes):
        c, s = np.cos(yaw), np.sin(yaw)
        hl, hw = l / 2, w / 2
        local = np.array([[hl, 0.0, hw], [hl, 0.0, -hw], [-hl, 0.0, -hw],
                          [-hl, 0.0, hw], [hl, -h, hw], [hl, -h, -hw],
                          [-hl, -h, -hw], [-hl, -h, hw]])
        rot = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
        out[i] = local.dot(rot.T) + np.array([x, y, z])
    return out


def box_segments(boxes_3d):
    """boxes_3d_to_line_set (kitti_dataset.py:785-822) as segments: [m, 7]
    (x, y, z, l, h, w, yaw) -> [12 m, 2, 3] float64, the twelve edges of each
    box in the order of :807-810.  On the host."""
    corners = box_corners(boxes_3d)
    return np.ascontiguousarray(corners[:, BOX_EDGES, :].reshape(-1, 2, 3))


_ROW_KEYS = ('name', 'truncation', 'occlusion', 'alpha', 'xmin', 'ymin',
             'xmax', 'ymax', 'height', 'width', 'length', 'x3d', 'y3d', 'z3d',
             'yaw', 'score')


def as_labels(rows):
    """Label dictionaries as they are; the 16-field tuples of
    kitti_output.detections_to_kitti_labels (run.detect_frame's rows) as
    dictionaries with read_label_file's keys."""
    return [r if isinstance(r, dict) else dict(zip(_ROW_KEYS, r))
            for r in (rows or [])]


def label_boxes(labels):
    """Label dictionaries -> [m, 7] (x3d, y3d, z3d, length, height, width,
    yaw), run.py:441-444."""
    labels = as_labels(labels)
    return np.array([[l['x3d'], l['y3d'], l['z3d'], l['length'], l['height'],
                      l['width'], l['yaw']] for l in labels],
                    dtype=np.float64).reshape(-1, 7)


def label_segments(labels):
    """box_segments of label dictionaries (kitti_dataset.read_label_file)."""
    return box_segments(label_boxes(labels))


def rect_segments(rows):
    """The 2D boxes of label dictionaries (run.py:411-413, vis_draw_2d_box:
    corners int(xmin), int(ymin), int(xmax), int(ymax)) -> [4 m, 2, 3] float64
    in pixel coordinates, for pixel_view(): top, right, bottom, left."""
    rows = as_labels(rows)
    out = np.zeros((len(rows), 4, 2, 3), dtype=np.float64)
    for i, r in enumerate(rows):
        x0, y0, x1, y1 = (float(int(r[k])) for k in
                          ('xmin', 'ymin', 'xmax', 'ymax'))
        out[i, :, :, :2] = [[(x0, y0), (x1, y0)], [(x1, y0), (x1, y1)],
                            [(x1, y1), (x0, y1)], [(x0, y1), (x0, y0)]]
    return out.reshape(-1, 2, 3)


def _kept_edges(edges, dst_mask, n_dst):
    """The rows of `edges` whose destination is set in dst_mask (bool [n_dst]
    or indices), in their order (run.py:341-343)."""
    import torch
    e = edges
    if dst_mask is None:
        return e
    m = torch.as_tensor(dst_mask).to(e.device)
    if m.dtype != torch.bool:
        flags = torch.zeros(n_dst, dtype=torch.bool, device=e.device)
        flags[m.long()] = True
        m = flags
    return e[m[e[:, 1].long()]].contiguous()


def graph_segments(coords, edges, level, dst_mask=None):
    """The edges of one graph level as segments, on the device: [E, 2, 3]
    float32 from coords[level][edges[level][:, 0]] to
    coords[level + 1][edges[level][:, 1]] (vis_graph); dst_mask (bool
    [n_dst], or destination indices) keeps only the edges into those vertices
    (run.py:341-350).  `edges` is the list of a graph (or one [E, 2] array for
    `level`).  Host-sized inputs only: capacity-form tensors raise."""
    import torch
    lib = _lib.load()
    e = edges[level] if isinstance(edges, (list, tuple)) else edges
    src, dst = coords[level], coords[level + 1]
    for t, what in ((e, "edges"), (src, "coords[level]"),
                    (dst, "coords[level + 1]")):
        if _lib.count_of(t) is not None:
            raise ValueError("%s is in capacity form: graph_segments takes "
                             "host-sized graphs only" % what)
    dev = _device(e, src, dst)
    as_t = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(
        np.ascontiguousarray(a))
    e = as_t(e).to(device=dev, dtype=torch.int32).reshape(-1, 2).contiguous()
    src = as_t(src).to(device=dev, dtype=torch.float32).contiguous()
    dst = as_t(dst).to(device=dev, dtype=torch.float32).contiguous()
    e = _kept_edges(e, dst_mask, int(dst.shape[0]))
    n_e = int(e.shape[0])
    out = torch.empty((n_e, 2, 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.pgnn_render_graph_segments(
            _lib.ptr(src), int(src.shape[0]), _lib.ptr(dst),
            int(dst.shape[0]), _lib.ptr(e), n_e, _lib.ptr(out),
            _lib.stream_ptr()), "pgnn_render_graph_segments")
    return out


# ---- a frame -------------------------------------------------------------------------
def frame_layers(points, det_labels=None, gt_labels=None, stages=None,
                 color_by='intensity', show_graph=False, det_colors=None,
                 gt_colors=None):
    """What render_frame draws, before any view: dict(points, point_colors,
    segments, segment_colors) of CUDA tensors (segments float64).  Stacking
    order of the segments: graph edges, ground truth, detections.  det_colors
    / gt_colors: one RGB per label instead of DETECTION_COLOR / GT_COLORS
    (every label given is then drawn, whatever its name)."""
    import torch
    det_labels, gt_labels = as_labels(det_labels), as_labels(gt_labels)
    xyz = points.xyz
    dev = _device(xyz)
    as_dev = lambda a: a if isinstance(a, torch.Tensor) else \
        torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    xyz = as_dev(xyz)
    if color_by == 'intensity':
        colors = colorize(as_dev(points.attr)[:, 0].contiguous(), 0.0, 1.0,
                          GRAY_TABLE)
    elif color_by == 'height':
        # camera y points down: 2 m below the camera is blue, 2 m above red
        colors = colorize(xyz[:, 1].contiguous(), 2.0, -2.0, RAMP_TABLE)
    elif color_by == 'class':
        if stages is None:
            raise ValueError("color_by='class' needs `stages` (the second "
                             "result of run.detect_frame)")
        colors = colorize(as_dev(points.attr)[:, 0].contiguous(), 0.0, 1.0,
                          GRAY_TABLE)
    else:
        raise ValueError("color_by must be 'intensity', 'height' or 'class', "
                         "got %r" % (color_by,))
    pts = [xyz.to(torch.float64)]
    pcols = [colors]
    vert_colors = None
    if stages is not None and (color_by == 'class' or show_graph):
        verts = stages['coords'][-1]
        labels = torch.argmax(stages['probs'], dim=1)
        vert_colors = class_colors(labels)                  # run.py:330-333
    if color_by == 'class':
        # the vertices come first: at equal depth the smaller index wins
        pts.insert(0, verts.to(torch.float64))
        pcols.insert(0, vert_colors)
    segs, scols = [], []
    if show_graph:
        if stages is None:
            raise ValueError("show_graph needs `stages`")
        level = len(stages['edges']) - 1
        e = stages['edges'][level]
        if _lib.count_of(e) is not None:
            raise ValueError("show_graph takes host-sized graphs only")
        nc = int(stages['probs'].shape[1])
        kept = (stages['candidate_indices'].long()[
            stages['nms_indices'].long()] // nc)             # run.py:339
        e = _kept_edges(e.to(torch.int32), kept,
                        int(stages['coords'][level + 1].shape[0]))
        segs.append(graph_segments(stages['coords'], e, level).to(
            torch.float64))
        scols.append(vert_colors[e[:, 1].long()])            # run.py:347-348
    u8 = lambda rows: torch.from_numpy(np.asarray(rows, dtype=np.uint8).reshape(
        -1, 3)).to(dev)
    if gt_labels and gt_colors is not None:
        segs.append(torch.from_numpy(label_segments(gt_labels)).to(dev))
        scols.append(u8(gt_colors).repeat_interleave(12, dim=0))
    elif gt_labels:
        gt = [l for l in gt_labels if l['name'] in GT_COLORS]  # run.py:438-444
        if gt:
            segs.append(torch.from_numpy(label_segments(gt)).to(dev))
            scols.append(u8([GT_COLORS[l['name']] for l in gt]
                            ).repeat_interleave(12, dim=0))
    if det_labels and det_colors is not None:
        segs.append(torch.from_numpy(label_segments(det_labels)).to(dev))
        scols.append(u8(det_colors).repeat_interleave(12, dim=0))
    elif det_labels:
        segs.append(torch.from_numpy(label_segments(det_labels)).to(dev))
        scols.append(u8([DETECTION_COLOR]).repeat(12 * len(det_labels), 1))
    return {
        'points': torch.cat(pts), 'point_colors': torch.cat(pcols),
        'segments': torch.cat(segs) if segs else None,
        'segment_colors': torch.cat(scols) if segs else None}


def frame_view(dataset, frame_idx, view, calib=None):
    """'bev' / 'camera' (the frame's calibration and image size) / a View."""
    if isinstance(view, View):
        return view
    if view == 'bev':
        return bev_view()
    if view == 'camera':
        if calib is None:
            calib = dataset.get_calib(frame_idx)
        h, w = dataset._image_shape(frame_idx)
        return camera_view(calib, (w, h))
    raise ValueError("view must be 'bev', 'camera' or a View, got %r" % (view,))


def detection_string(label):
    """run.py:414-421: 'P | 0.873' for a Pedestrian, 'C | 0.912' for every
    other class."""
    return '%s | %.3f' % ('P' if label['name'] == 'Pedestrian' else 'C',
                          label['score'])


def center_pixel(view, label):
    """The pixel of a label's box centre (x3d, y3d, z3d) under `view`, by the
    header's float64 formula (floor(hu / hw), floor(hv / hw)); None when the
    centre is not visible or its pixel is off the canvas."""
    x, y, z = float(label['x3d']), float(label['y3d']), float(label['z3d'])
    rows = np.asarray(view.m, dtype=np.float64).reshape(3, 4).tolist() + \
        [np.asarray(view.d, dtype=np.float64).reshape(4).tolist()]
    # Python floats are IEEE float64: the header's sums, in its order
    hu, hv, hw, dep = (((r[0] * x + r[1] * y) + r[2] * z) + r[3]
                       for r in rows)
    if not all(math.isfinite(t) for t in (hu, hv, hw, dep)):
        return None
    if not hw >= view.near or hw == 0.0:   # x / 0 is on no canvas
        return None
    u, w = hu / hw, hv / hw
    if not (0.0 <= u < view.width and 0.0 <= w < view.height):
        return None                        # floor keeps both comparisons
    return int(math.floor(u)), int(math.floor(w))


def frame_text(det_labels, gt_labels, view, camera):
    """What render_frame(text=True) writes: (strings, anchors [n, 2], colors
    [n, 3]) for draw_text(anchor='bl').  Ground truth names first (the labels
    whose wireframe is drawn, in its colour), detections after them (so they
    win overlaps): detection_string in DETECTION_TEXT_COLORS.  camera: the
    anchors are the reference's, org = (int(xmin), int(ymin)), a Pedestrian
    detection's int(xmin / 10) higher (run.py:414-421, vis_draw_2d_box);
    otherwise center_pixel(view, label), and a label without one gets no
    string."""
    det_labels, gt_labels = as_labels(det_labels), as_labels(gt_labels)
    strings, anchors, colors = [], [], []

    def add(string, label, color, lift):
        if camera:
            org = (int(label['xmin']), int(label['ymin']) - lift)
        else:
            org = center_pixel(view, label)
            if org is None:
                return
        strings.append(string)
        anchors.append(org)
        colors.append(color)
    for l in gt_labels:
        if l['name'] in GT_COLORS:
            add(l['name'], l, GT_COLORS[l['name']], 0)
    for l in det_labels:
        ped = l['name'] == 'Pedestrian'
        add(detection_string(l), l, DETECTION_TEXT_COLORS[ped],
            int(l['xmin'] / 10) if ped and camera else 0)
    return (strings, np.array(anchors, dtype=np.int64).reshape(-1, 2),
            np.array(colors, dtype=np.uint8).reshape(-1, 3))


# ---- outcomes of the KITTI matching on the boxes -------------
# A box's tag by its outcome code (kitti_eval.DET_OUTCOMES / GT_OUTCOMES); a
# box tagged None (code OTHER: another class's) is not drawn.  A detection
# under the threshold and the ground truth it would have found share 'LOW'; the
# ignored kinds share 'IGN'.
OUTCOME_TAGS = {
    'det': {'OTHER': None, 'BELOW': 'LOW', 'TP': 'TP',
            'MATCHED_IGNORED': 'IGN', 'IGNORED_SMALL': 'IGN',
            'DONTCARE': 'IGN', 'FP_DUPLICATE': 'DUP', 'FP_CONFUSION': 'CONF',
            'FP_LOCALISATION': 'LOC', 'FP_BACKGROUND': 'BG'},
    'gt': {'OTHER': None, 'IGNORED': 'IGN', 'IGNORED_MATCHED': 'IGN',
           'TP': 'TP', 'MATCHED_SMALL': 'IGN', 'FN_LOW_SCORE': 'LOW',
           'FN_LOCALISATION': 'LOC', 'FN_MISSED': 'MISS'}}
# one RGB per tag, the same for a detection and a ground truth
OUTCOME_COLORS = {'TP': (0, 220, 0), 'DUP': (255, 165, 0),
                  'LOC': (255, 255, 0), 'CONF': (255, 0, 255),
                  'BG': (255, 0, 0), 'LOW': (0, 200, 255),
                  'MISS': (255, 105, 180), 'IGN': (128, 128, 128)}


def outcome_tags(side, codes):
    """'det' / 'gt' and outcome codes -> the tags, None for a box that is not
    drawn."""
    from . import kitti_eval
    names = kitti_eval.DET_OUTCOMES if side == 'det' else \
        kitti_eval.GT_OUTCOMES
    return [OUTCOME_TAGS[side][names[int(c)]] for c in codes]


def frame_outcomes(det_labels, gt_labels, outcomes, show_below=False,
                   with_text=True):
    """What render_frame(outcomes=...) draws of a frame: dict(det, gt: the
    labels drawn, in their order; det_colors, gt_colors: uint8 [n, 3];
    det_strings, gt_strings).  outcomes: KittiMatchResult.frame(f), for these
    labels.  Not drawn: boxes of code OTHER and, without show_below,
    detections under the threshold.  A string is the tag, then two decimals:
    a detection's overlap with its partner, its score where it has none (BG,
    LOW, an unmatched IGN); a ground truth's overlap with its partner where
    that detection's partner is this ground truth (TP, the matched IGN, most
    LOC), else the partner's score (LOW, the other LOC); MISS and an unmatched
    IGN stand alone."""
    det_labels, gt_labels = as_labels(det_labels), as_labels(gt_labels)
    det_outcome, det_partner, det_overlap, gt_outcome, gt_partner = outcomes
    if len(det_outcome) != len(det_labels) or len(gt_outcome) != len(gt_labels):
        raise ValueError("outcomes are for %d detections and %d labels, the "
                         "frame has %d and %d" % (
                             len(det_outcome), len(gt_outcome),
                             len(det_labels), len(gt_labels)))
    out = {'det': [], 'gt': [], 'det_strings': [], 'gt_strings': []}
    colors = {'det': [], 'gt': []}
    for j, tag in enumerate(outcome_tags('det', det_outcome)):
        if tag is None or (tag == 'LOW' and not show_below):
            continue
        value = float(det_overlap[j]) if det_partner[j] >= 0 else \
            float(det_labels[j]['score'])
        out['det'].append(det_labels[j])
        colors['det'].append(OUTCOME_COLORS[tag])
        out['det_strings'].append('%s %.2f' % (tag, value))
    for i, tag in enumerate(outcome_tags('gt', gt_outcome)):
        if tag is None:
            continue
        p = int(gt_partner[i])
        if p < 0:
            string = tag
        elif det_partner[p] == i:
            string = '%s %.2f' % (tag, float(det_overlap[p]))
        else:
            string = '%s %.2f' % (tag, float(det_labels[p]['score']))
        out['gt'].append(gt_labels[i])
        colors['gt'].append(OUTCOME_COLORS[tag])
        out['gt_strings'].append(string)
    for side in ('det', 'gt'):
        out[side + '_colors'] = np.array(colors[side],
                                         dtype=np.uint8).reshape(-1, 3)
    return out


def outcome_text(drawn, view, camera):
    """(strings, anchors, colors) of frame_outcomes' result for draw_text
    (anchor='bl'): ground truths first, each string in its box's colour at
    frame_text's anchor (no lift)."""
    strings, anchors, colors = [], [], []
    for side in ('gt', 'det'):
        for label, string, color in zip(drawn[side], drawn[side + '_strings'],
                                        drawn[side + '_colors']):
            org = (int(label['xmin']), int(label['ymin'])) if camera else \
                center_pixel(view, label)
            if org is None:
                continue
            strings.append(string)
            anchors.append(org)
            colors.append(color)
    return (strings, np.array(anchors, dtype=np.int64).reshape(-1, 2),
            np.array(colors, dtype=np.uint8).reshape(-1, 3))


def _render_frame_outcomes(dataset, frame_idx, det_labels, gt_labels, view,
                           stages, color_by, show_graph, background, text,
                           text_plate, outcomes, show_below):
    calib = stages['calib'] if stages is not None else None
    v = frame_view(dataset, frame_idx, view, calib)
    points = stages['points'] if stages is not None else \
        dataset.get_cam_points_in_image_with_rgb(frame_idx, calib=calib)
    drawn = frame_outcomes(det_labels, gt_labels, outcomes, show_below)
    layers = frame_layers(points, drawn['det'], drawn['gt'], stages, color_by,
                          show_graph, det_colors=drawn['det_colors'],
                          gt_colors=drawn['gt_colors'])
    image = render(v, points=layers['points'],
                   point_colors=layers['point_colors'],
                   segments=layers['segments'],
                   segment_colors=layers['segment_colors'],
                   background=background)
    if view == 'camera' and drawn['det']:
        image = render(pixel_view(v.width, v.height),
                       segments=rect_segments(drawn['det']),
                       segment_colors=np.repeat(drawn['det_colors'], 4, axis=0),
                       thickness=2, background=image)
    if text:
        strings, anchors, colors = outcome_text(drawn, v, view == 'camera')
        if strings:
            draw_text(image, strings, anchors, colors=colors, scale=1,
                      plate=text_plate, anchor='bl')
    return image


def render_frame(dataset, frame_idx, det_labels=None, gt_labels=None,
                 view='bev', stages=None, color_by='intensity',
                 show_graph=False, background=None, text=False,
                 text_plate=None, outcomes=None, show_below=False):
    """One frame of `dataset`: the cloud cropped to the camera image (coloured
    by 'intensity', 'height', or by 'class' on the last level's vertices),
    ground truth wireframes in GT_COLORS (labels filtered like run.py:438-444),
    detections in red; in the camera view also every detection's 2D rectangle
    in (0, 255, 0) at thickness 2 (run.py:411-413).  stages: the second result
    of run.detect_frame; it supplies the points and allows color_by='class'
    and show_graph (the last level's edges into the vertices of the kept
    boxes, run.py:339-350).  text: also the strings of frame_text, drawn last
    with draw_text (scale 1, anchor='bl'; text_plate: a plate colour under
    them); without it no text pass runs.  outcomes: the frame's five arrays
    of a kitti_eval.match (KittiMatchResult.frame): every box then takes its
    outcome's colour (OUTCOME_TAGS, OUTCOME_COLORS) -- wireframes, rectangles
    and strings -- boxes of another class are not drawn, detections under the
    threshold only with show_below, and with `text` the strings are
    frame_outcomes' ('LOC 0.41').  -> uint8 [H, W, 3] CUDA tensor."""
    if outcomes is not None:
        return _render_frame_outcomes(
            dataset, frame_idx, det_labels, gt_labels, view, stages, color_by,
            show_graph, background, text, text_plate, outcomes, show_below)
    calib = stages['calib'] if stages is not None else None
    v = frame_view(dataset, frame_idx, view, calib)
    points = stages['points'] if stages is not None else \
        dataset.get_cam_points_in_image_with_rgb(frame_idx, calib=calib)
    layers = frame_layers(points, det_labels, gt_labels, stages, color_by,
                          show_graph)
    image = render(v, points=layers['points'],
                   point_colors=layers['point_colors'],
                   segments=layers['segments'],
                   segment_colors=layers['segment_colors'],
                   background=background)
    det_labels = as_labels(det_labels)
    if view == 'camera' and det_labels:
        image = render(pixel_view(v.width, v.height),
                       segments=rect_segments(det_labels),
                       segment_colors=RECT_COLOR, thickness=2,
                       background=image)
    if text:
        strings, anchors, colors = frame_text(det_labels, gt_labels, v,
                                              view == 'camera')
        if strings:
            draw_text(image, strings, anchors, colors=colors, scale=1,
                      plate=text_plate, anchor='bl')
    return image


# ---- files ------------------------------------------------------------------------------
def _host_image(image):
    import torch
    if isinstance(image, torch.Tensor):
        image = image.cpu().numpy()
    image = np.ascontiguousarray(image)
    if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
        raise ValueError("image must be uint8 [H, W, 3]")
    return image


PNG_ENCODERS = ('zlib', 'device')


def _check_encoder(encoder):
    if encoder not in PNG_ENCODERS:
        raise ValueError("encoder must be 'zlib' or 'device', got %r"
                         % (encoder,))


def png_bytes(image, compress_level=6, encoder='zlib'):
    """8-bit RGB PNG, filter type 0 on every row, one IDAT chunk.  encoder
    'zlib': the image goes to the host and through zlib.compress at
    compress_level.  'device': png.encode_png -- compressed on the device
    (fixed Huffman codes, larger files), only the compressed bytes come back;
    compress_level is not used."""
    _check_encoder(encoder)
    if encoder == 'device':
        from . import png
        return png.encode_png(image)
    image = _host_image(image)
    h, w = image.shape[:2]
    raw = np.zeros((h, 1 + 3 * w), dtype=np.uint8)
    raw[:, 1:] = image.reshape(h, 3 * w)

    def chunk(kind, data):
        body = kind + data
        return struct.pack(">I", len(data)) + body + struct.pack(
            ">I", zlib.crc32(body) & 0xffffffff)
    return b"".join([
        b"\x89PNG\r\n\x1a\n",
        chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)),
        chunk(b"IDAT", zlib.compress(raw.tobytes(), compress_level)),
        chunk(b"IEND", b"")])


def write_png(path, image, compress_level=6, encoder='zlib'):
    data = png_bytes(image, compress_level, encoder)
    with open(path, "wb") as f:
        f.write(data)


def write_ppm(path, image):
    """Binary PPM (P6)."""
    image = _host_image(image)
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (image.shape[1], image.shape[0]))
        f.write(image.tobytes())


def image_background(dataset):
    """A `background_reader` for render_results: the frame's camera image,
    decoded on the device (png.read_png) as uint8 RGB [H, W, 3] -- the camera
    view then draws on the photograph, as run.py -l does."""
    from . import png

    def reader(frame_idx):
        return png.read_png(os.path.join(
            dataset._image_dir, dataset.get_filename(frame_idx) + '.png'),
            order='rgb')
    return reader


def render_results(dataset, result_dir, render_dir, views=('bev',),
                   frame_indices=None, fmt='png', with_gt=True,
                   background_reader=None, time_dict=None, text=False,
                   text_plate=None, png_encoder='zlib', errors=None,
                   show_below=False):
    """Draws every frame of a result directory (<result_dir>/<name>.txt as
    run.run_dataset writes them under <output_dir>/data, or any other KITTI
    result directory) into <render_dir>/<view>/<name>.<fmt>, fmt 'png' or
    'ppm'.  with_gt: also the labels, when the dataset has a label directory.
    background_reader(frame_idx) -> uint8 RGB [H, W, 3] for the camera view
    (image_background(dataset): the frame's own PNG, decoded on the device).
    text / text_plate: render_frame's.  png_encoder: png_bytes' `encoder`;
    with 'device' the image stays on the device and only its compressed bytes
    are read (time_dict's 'encode png' then holds that encode, 'render' ends
    at a synchronise).  Sequential: one host read per image (two short ones
    with 'device').  errors: a dict of kitti_eval.match's keyword arguments
    (metric, cls, difficulty, score_threshold, min_overlap, loc_floor; {} for
    its defaults but score_threshold, which defaults to 'f1': the
    combination's best_f1_threshold, from one evaluation of the frame set).
    The frame set is then matched once and every frame is drawn with its
    outcomes (render_frame's `outcomes`, `show_below`); needs the labels.
    Returns the paths written."""
    from . import kitti_eval
    import time
    import torch
    if fmt not in ('png', 'ppm'):
        raise ValueError("fmt must be 'png' or 'ppm', got %r" % (fmt,))
    _check_encoder(png_encoder)
    on_device = fmt == 'png' and png_encoder == 'device'
    views = (views,) if isinstance(views, str) else tuple(views)
    for view in views:
        if view not in ('bev', 'camera'):
            raise ValueError("views are 'bev' and 'camera', got %r" % (view,))
    if frame_indices is None:
        frame_indices = range(dataset.num_files)
    td = time_dict if time_dict is not None else {}
    paths = []
    matched = None
    if errors is not None:
        frame_indices = list(frame_indices)
        matched = _match_frames(dataset, result_dir, frame_indices, errors)
    for k, frame_idx in enumerate(frame_indices):
        name = dataset.get_filename(frame_idx)
        det = kitti_eval.read_result_file(
            os.path.join(result_dir, name + '.txt'))
        gt = None
        if (with_gt or matched is not None) and dataset._label_dir:
            gt = dataset.get_label(frame_idx)
        more = {} if matched is None else {'outcomes': matched.frame(k),
                                           'show_below': show_below}
        calib = dataset.get_calib(frame_idx)
        points = dataset.get_cam_points_in_image_with_rgb(frame_idx,
                                                          calib=calib)
        stages = {'calib': calib, 'points': points}
        for view in views:
            t0 = time.time()
            background = None
            if view == 'camera' and background_reader is not None:
                background = background_reader(frame_idx)
            image = render_frame(dataset, frame_idx, det, gt, view=view,
                                 stages=stages, background=background,
                                 text=text, text_plate=text_plate, **more)
            if on_device:
                torch.cuda.synchronize(image.device)   # 'render' ends here
                host = image
            else:
                host = image.cpu().numpy()
            t1 = time.time()
            path = os.path.join(render_dir, view, name + '.' + fmt)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            if fmt == 'png':
                data = png_bytes(host, encoder=png_encoder)
                t2 = time.time()
                with open(path, "wb") as f:
                    f.write(data)
                td['encode png'] = td.get('encode png', 0.0) + t2 - t1
            else:
                write_ppm(path, host)
            td['render'] = td.get('render', 0.0) + t1 - t0
            td['write'] = td.get('write', 0.0) + time.time() - t1
            paths.append(path)
    return paths


def _match_frames(dataset, result_dir, frame_indices, errors):
    """kitti_eval.match of the frames render_results draws, in their order."""
    from . import kitti_eval
    if not dataset._label_dir:
        raise ValueError("errors needs the labels: the dataset has no label "
                         "directory")
    kwargs = dict(errors)
    gt = [dataset.get_label(i) for i in frame_indices]
    det = [kitti_eval.read_result_file(os.path.join(
        result_dir, dataset.get_filename(i) + '.txt')) for i in frame_indices]
    combo = [kwargs.setdefault(key, value) for key, value in
             (('metric', '3d'), ('cls', 'Car'), ('difficulty', 'moderate'))]
    threshold = kwargs.pop('score_threshold', 'f1')
    if isinstance(threshold, str):
        evaluated = kitti_eval.evaluate(
            gt, det, min_overlap=kwargs.get('min_overlap'),
            device=kwargs.get('device'))
        threshold = kitti_eval.resolve_threshold(threshold, evaluated, *combo)
    return kitti_eval.match(gt, det, score_threshold=threshold, **kwargs)


def build_parser():
    import argparse
    from . import kitti_eval
    ap = argparse.ArgumentParser(
        prog="python -m pointgnn_amd.render",
        description="Draw every frame of a KITTI result directory: the "
                    "cloud, the labels and the detections, one image per "
                    "frame and view.")
    ap.add_argument('dataset_dir', metavar='DATASET_DIR',
                    help="KITTI object directory holding image_2/, velodyne/, "
                         "calib/ and, for ground truth, label_2/")
    ap.add_argument('result_dir', metavar='RESULT_DIR',
                    help="directory of <frame>.txt detections")
    ap.add_argument('render_dir', metavar='RENDER_DIR')
    ap.add_argument('--view', action='append', choices=('bev', 'camera'),
                    help="repeatable; default bev")
    ap.add_argument('--label-dir', metavar='DIR', default=None,
                    help="labels (default: DATASET_DIR/label_2 if present)")
    ap.add_argument('--split', metavar='FILE', default=None,
                    help="frame names, one per line (default: every scan)")
    ap.add_argument('--ppm', action='store_true',
                    help="write binary PPM files instead of PNG")
    ap.add_argument('--png-encoder', choices=PNG_ENCODERS, default='zlib',
                    help="zlib: compress on the host (level 6); device: "
                         "compress on the GPU, only the compressed bytes are "
                         "read back (faster, larger files)")
    ap.add_argument('--image-background', action='store_true',
                    help="camera view: draw on the frame's decoded image "
                         "instead of black")
    ap.add_argument('--text', action='store_true',
                    help="write every detection's class letter and score "
                         "('P | 0.873') and every drawn label's name")
    kitti_eval.add_error_arguments(
        ap, "colour every box by its outcome in the KITTI matching of one "
            "combination at one score threshold (with --text: tag and "
            "overlap, 'LOC 0.41'); needs the labels")
    ap.add_argument('--show-below', action='store_true',
                    help="with --errors: also draw the detections under the "
                         "threshold")
    return ap


def main(argv=None):
    from .kitti_dataset import KittiDataset
    args = build_parser().parse_args(argv)
    root = args.dataset_dir
    label_dir = args.label_dir
    if label_dir is None and os.path.isdir(os.path.join(root, 'label_2')):
        label_dir = os.path.join(root, 'label_2')
    dataset = KittiDataset(os.path.join(root, 'image_2'),
                           os.path.join(root, 'velodyne'),
                           os.path.join(root, 'calib'), label_dir,
                           index_filename=args.split)
    paths = render_results(dataset, args.result_dir, args.render_dir,
                           views=tuple(args.view or ('bev',)),
                           fmt='ppm' if args.ppm else 'png',
                           background_reader=image_background(dataset)
                           if args.image_background else None,
                           text=args.text, png_encoder=args.png_encoder,
                           errors=dict(metric=args.error_metric,
                                       cls=args.error_class,
                                       difficulty=args.error_difficulty,
                                       score_threshold=args.at_threshold)
                           if args.errors else None,
                           show_below=args.show_below)
    print("wrote %d images to %s" % (len(paths), args.render_dir))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
