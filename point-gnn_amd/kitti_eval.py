"""KITTI object-detection average precision on the device (csrc/kitti_eval.hip).

The reference's README hands its result files to an external evaluation
program; this module scores them here: the 2D box, the bird's-eye box and the
3D box, per class (Car, Pedestrian, Cyclist) and difficulty (easy, moderate,
hard), with 11- and 40-point interpolation.  The protocol is DESIGN.md §9.5.

    result = evaluate(gt_labels, det_labels)      # lists over frames of labels
    result = evaluate_dirs(label_dir, result_dir)  # KITTI txt on both sides
    result.ap('3d', 'Car', 1)                      # AP_R40, moderate, in [0, 1]
    print(result.format())

    python -m pointgnn_amd.kitti_eval LABEL_DIR RESULT_DIR [--split FILE] [--json]
        [--aos] [--alpha-from-box] [--min-overlap official|loose|<9 numbers>]
        [--plot DIR]

    write_pr_data(result, directory)     # <class>_detection.txt, ... 41 lines
    image = plot_pr(result, '3d', 'Car')  # the three curves, drawn on the device
    write_pr_plots(result, directory)

A label is the dict of `kitti_dataset.read_label_file`; a detection carries
`score` as well.

Two additions go through `pgnn_kitti_eval_ex`, and only when asked for:

    result = evaluate(gt, det, aos=True)            # orientation similarity
    result.aos('Car', 'moderate')                   # AOS_R40, beside the 2D AP
    result = evaluate(gt, det, aos=True, det_alpha='box')   # alpha from the box
    result = evaluate(gt, det, min_overlap='loose')  # BEV / 3D at .5 / .25 / .25

Which boxes cost the AP, and why (pgnn_kitti_match): the
matching of one combination at one score threshold, box by box.

    t = best_f1_threshold(result, '3d', 'Car', 'moderate')
    errors = match(gt, det, '3d', 'Car', 'moderate', score_threshold=t)
    errors.fp, errors.totals['DET_FP_LOCALISATION'], errors.frame(0)
    print(errors.format())

    python -m pointgnn_amd.kitti_eval LABEL_DIR RESULT_DIR --errors
        [--error-metric 3d] [--error-class Car] [--error-difficulty moderate]
        [--at-threshold f1|<float>]
"""
import ctypes
import json
import os

import numpy as np
import torch

from . import _header, _lib
from . import kitti_dataset

CLASSES = ('Car', 'Pedestrian', 'Cyclist')
METRICS = ('2d', 'bev', '3d')
DIFFICULTIES = ('easy', 'moderate', 'hard')
# the official tool's names of the three metrics in its report lines
REPORT_NAMES = ('detection', 'detection_ground', 'detection_3d')
_C = _header.constants()
ROW, N_SAMPLE_PTS, N_COMBOS = (_C["PGNN_KITTI_ROW"], _C["PGNN_KITTI_SAMPLE_PTS"],
                               _C["PGNN_KITTI_COMBOS"])
MAX_DET, MAX_GT = _C["PGNN_KITTI_MAX_DET"], _C["PGNN_KITTI_MAX_GT"]
# MIN_OVERLAP[metric][class] (METRICS, CLASSES); the official table is what
# pgnn_kitti_eval has compiled in
OFFICIAL_MIN_OVERLAP = ((0.7, 0.5, 0.5),) * 3
LOOSE_MIN_OVERLAP = ((0.7, 0.5, 0.5), (0.5, 0.25, 0.25), (0.5, 0.25, 0.25))
# a detection file written without an observation angle carries this alpha;
# the official rule: one such detection and AOS is not computed
NO_ALPHA = -10.0

# name codes of the C ABI; names compare case-insensitively
_NAME_CODES = {'car': 0, 'pedestrian': 1, 'cyclist': 2, 'van': 3,
               'person_sitting': 4, 'dontcare': 5}
_OTHER = 6
_ROW_KEYS = ('xmin', 'ymin', 'xmax', 'ymax', 'height', 'width', 'length',
             'x3d', 'y3d', 'z3d', 'yaw')


def name_code(name):
    return _NAME_CODES.get(str(name).lower(), _OTHER)


def pack_labels(frames):
    """Lists over frames of label dicts -> (offsets int32 [F+1], rows float64
    [N, 14], name codes int32 [N]) in the layout of pgnn_kitti_eval."""
    offsets = np.zeros(len(frames) + 1, np.int32)
    n = 0
    for f, labels in enumerate(frames):
        n += len(labels)
        offsets[f + 1] = n
    rows = np.zeros((n, ROW), np.float64)
    names = np.zeros(n, np.int32)
    k = 0
    for labels in frames:
        for lab in labels:
            rows[k, :11] = [lab[key] for key in _ROW_KEYS]
            rows[k, 11] = lab.get('truncation', 0.0)
            rows[k, 12] = lab.get('occlusion', 0)
            rows[k, 13] = lab.get('score', 0.0)
            names[k] = name_code(lab['name'])
            k += 1
    return offsets, rows, names


def pack_alpha(frames):
    """Lists over frames of label dicts -> float64 [N], the `alpha` fields in
    the order of `pack_labels`' rows."""
    return np.array([lab['alpha'] for labels in frames for lab in labels],
                    np.float64)


def alpha_from_box(rows):
    """The observation angle of packed rows from their 3D box: yaw -
    atan2(x3d, z3d), float64, not wrapped (only its cosine is used)."""
    rows = np.asarray(rows, np.float64).reshape(-1, ROW)
    return rows[:, 10] - np.arctan2(rows[:, 7], rows[:, 9])


def min_overlap_table(value):
    """None / 'official' / 'loose' / a 3x3 array-like (or 9 numbers) ->
    float64 [3, 3], [metric][class].  The range of the entries is the C
    entry's check."""
    if value is None:
        return np.array(OFFICIAL_MIN_OVERLAP, np.float64)
    if isinstance(value, str):
        named = {'official': OFFICIAL_MIN_OVERLAP, 'loose': LOOSE_MIN_OVERLAP}
        if value.lower() in named:
            return np.array(named[value.lower()], np.float64)
        try:
            value = [float(x) for x in value.split(',')]
        except ValueError:
            raise ValueError("min_overlap: 'official', 'loose' or 9 "
                             "comma-separated numbers, not %r" % (value,))
    table = np.array(value, np.float64)
    if table.size != 9:
        raise ValueError("min_overlap needs 3 x 3 numbers [metric][class], "
                         "got %d" % table.size)
    return np.ascontiguousarray(table.reshape(3, 3))


def _pair_count(gt_off, det_off):
    return int(np.sum(np.diff(gt_off).astype(np.int64) *
                      np.diff(det_off).astype(np.int64)))


def _host_ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def _device(device):
    return torch.device(device if device is not None else 'cuda')


# sections of the one output buffer, each a multiple of 8 bytes but the last
_OUT_LAYOUT = (('precision', np.float64, (3, 3, 3, N_SAMPLE_PTS)),
               ('recall', np.float64, (3, 3, 3, N_SAMPLE_PTS)),
               ('counters', np.int64, (3, 3, 3, N_SAMPLE_PTS, 3)),
               ('thresholds', np.float64, (3, 3, 3, N_SAMPLE_PTS)),
               ('n_gt', np.int64, (3, 3, 3)),
               ('ap_r11', np.float64, (3, 3, 3)),
               ('ap_r40', np.float64, (3, 3, 3)),
               ('n_thresholds', np.int32, (3, 3, 3)))


def _out_sections():
    off, sections = 0, {}
    for key, dtype, shape in _OUT_LAYOUT:
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        sections[key] = (off, nbytes, dtype, shape)
        off += nbytes
    return sections, off


def output_bytes():
    return _out_sections()[1]


# the output buffer of run_packed_ex: the sections above (int32 n_thresholds
# last) with the orientation outputs of the 2D metric, [class][difficulty]
_AOS_LAYOUT = (('similarity', np.float64, (3, 3, N_SAMPLE_PTS)),
               ('orientation', np.float64, (3, 3, N_SAMPLE_PTS)),
               ('aos_r11', np.float64, (3, 3)),
               ('aos_r40', np.float64, (3, 3)))
_EX_LAYOUT = _OUT_LAYOUT[:-1] + _AOS_LAYOUT + _OUT_LAYOUT[-1:]


def _sections_of(layout):
    off, sections = 0, {}
    for key, dtype, shape in layout:
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        sections[key] = (off, nbytes, dtype, shape)
        off += nbytes
    return sections, off


def output_bytes_ex():
    return _sections_of(_EX_LAYOUT)[1]


def run_packed(gt, det, out=None, device=None):
    """pgnn_kitti_eval on packed labels (`pack_labels` triples).  `out`: a
    uint8 device tensor of output_bytes() bytes to write into (a new one
    otherwise).  Returns it; nothing has been read back."""
    lib = _lib.load()
    gt_off, gt_rows, gt_names = gt
    det_off, det_rows, det_names = det
    if len(gt_off) != len(det_off):
        raise ValueError("ground truth and detections cover %d and %d frames"
                         % (len(gt_off) - 1, len(det_off) - 1))
    dev = _device(device)
    sections, total = _out_sections()
    if out is None:
        out = torch.empty(total, dtype=torch.uint8, device=dev)
    n_frames = len(gt_off) - 1
    n_pairs = _pair_count(gt_off, det_off)
    ws_bytes = int(lib.pgnn_kitti_eval_workspace_bytes(
        n_frames, len(gt_rows), len(det_rows), n_pairs))
    ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=dev)
    d_gt = torch.from_numpy(gt_rows).to(dev)
    d_gt_names = torch.from_numpy(gt_names).to(dev)
    d_det = torch.from_numpy(det_rows).to(dev)
    d_det_names = torch.from_numpy(det_names).to(dev)

    def at(key):
        return ctypes.c_void_p(out.data_ptr() + sections[key][0])

    def dptr(t):
        return _lib.ptr(t if t.numel() else None)

    gt_off = np.ascontiguousarray(gt_off, np.int32)
    det_off = np.ascontiguousarray(det_off, np.int32)
    with torch.cuda.device(dev):
        _lib.check(lib.pgnn_kitti_eval(
            _host_ptr(gt_off), _host_ptr(det_off), n_frames, dptr(d_gt),
            dptr(d_gt_names), dptr(d_det), dptr(d_det_names), _lib.ptr(ws),
            ws.numel(), at('precision'), at('recall'), at('counters'),
            at('thresholds'), at('n_thresholds'), at('n_gt'), at('ap_r11'),
            at('ap_r40'), _lib.stream_ptr()), "pgnn_kitti_eval")
        # the host offsets and the device inputs must outlive the launches
        torch.cuda.current_stream().synchronize()
    return out


def run_packed_ex(gt, det, gt_alpha=None, det_alpha=None, min_overlap=None,
                  out=None, device=None):
    """pgnn_kitti_eval_ex on packed labels.  gt_alpha / det_alpha: float64
    host arrays, one per row (`pack_alpha`, `alpha_from_box`), both or
    neither; without them no orientation work is launched and the four
    orientation sections of `out` are not written.  min_overlap: see
    `min_overlap_table`.  `out`: a uint8 device tensor of output_bytes_ex()
    bytes (a new one otherwise).  Returns it; nothing has been read back."""
    lib = _lib.load()
    gt_off, gt_rows, gt_names = gt
    det_off, det_rows, det_names = det
    if len(gt_off) != len(det_off):
        raise ValueError("ground truth and detections cover %d and %d frames"
                         % (len(gt_off) - 1, len(det_off) - 1))
    if (gt_alpha is None) != (det_alpha is None):
        raise ValueError("gt_alpha and det_alpha: both or neither")
    with_aos = gt_alpha is not None
    table = min_overlap_table(min_overlap)
    dev = _device(device)
    sections, total = _sections_of(_EX_LAYOUT)
    if out is None:
        out = torch.empty(total, dtype=torch.uint8, device=dev)
    n_frames = len(gt_off) - 1
    n_pairs = _pair_count(gt_off, det_off)
    ws_bytes = int(lib.pgnn_kitti_eval_ex_workspace_bytes(
        n_frames, len(gt_rows), len(det_rows), n_pairs, int(with_aos)))
    ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=dev)
    d_gt = torch.from_numpy(gt_rows).to(dev)
    d_gt_names = torch.from_numpy(gt_names).to(dev)
    d_det = torch.from_numpy(det_rows).to(dev)
    d_det_names = torch.from_numpy(det_names).to(dev)
    d_gt_alpha = d_det_alpha = None
    if with_aos:
        d_gt_alpha = _alpha_tensor(gt_alpha, len(gt_rows), 'gt_alpha', dev)
        d_det_alpha = _alpha_tensor(det_alpha, len(det_rows), 'det_alpha', dev)

    def at(key):
        return ctypes.c_void_p(out.data_ptr() + sections[key][0])

    def dptr(t):
        return _lib.ptr(t if t.numel() else None)

    gt_off = np.ascontiguousarray(gt_off, np.int32)
    det_off = np.ascontiguousarray(det_off, np.int32)
    with torch.cuda.device(dev):
        _lib.check(lib.pgnn_kitti_eval_ex(
            _host_ptr(gt_off), _host_ptr(det_off), n_frames, dptr(d_gt),
            dptr(d_gt_names), dptr(d_det), dptr(d_det_names), _lib.ptr(ws),
            ws.numel(), at('precision'), at('recall'), at('counters'),
            at('thresholds'), at('n_thresholds'), at('n_gt'), at('ap_r11'),
            at('ap_r40'), _lib.ptr(d_gt_alpha), _lib.ptr(d_det_alpha),
            _host_ptr(table), at('similarity'), at('orientation'),
            at('aos_r11'), at('aos_r40'), _lib.stream_ptr()),
            "pgnn_kitti_eval_ex")
        # the host offsets and the device inputs must outlive the launches
        torch.cuda.current_stream().synchronize()
    return out


def _alpha_tensor(alpha, n, what, dev):
    """One float64 per row on the device; a set without rows still hands the
    entry a pointer (NULL there means "no orientation")."""
    alpha = np.ascontiguousarray(alpha, np.float64).reshape(-1)
    if len(alpha) != n:
        raise ValueError("%s has %d entries for %d rows" % (what, len(alpha), n))
    if n == 0:
        return torch.zeros(1, dtype=torch.float64, device=dev)
    return torch.from_numpy(alpha).to(dev)


def pair_orientation(gt_labels, det_labels, gt_alpha=None, det_alpha=None,
                     device=None):
    """pgnn_kitti_pair_orientation -> (sim float64 [n_pairs], pair_off int64
    [F+1]) in the layout of one plane of `pair_overlaps`: (1 + cos(alpha_gt -
    alpha_det)) / 2 where the pair's 2D overlap is > 0, else 0.  The alphas
    default to the labels' `alpha` fields."""
    lib = _lib.load()
    gt_off, gt_rows, _ = pack_labels(gt_labels)
    det_off, det_rows, _ = pack_labels(det_labels)
    if len(gt_off) != len(det_off):
        raise ValueError("frame counts differ")
    if gt_alpha is None:
        gt_alpha = pack_alpha(gt_labels)
    if det_alpha is None:
        det_alpha = pack_alpha(det_labels)
    dev = _device(device)
    n_frames = len(gt_off) - 1
    per_frame = np.diff(gt_off).astype(np.int64) * np.diff(det_off)
    pair_off = np.concatenate([[0], np.cumsum(per_frame)]).astype(np.int64)
    n_pairs = int(pair_off[-1])
    ws_bytes = int(lib.pgnn_kitti_eval_workspace_bytes(
        n_frames, len(gt_rows), len(det_rows), n_pairs))
    ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=dev)
    sim = torch.zeros(n_pairs, dtype=torch.float64, device=dev)
    d_gt = torch.from_numpy(gt_rows).to(dev)
    d_det = torch.from_numpy(det_rows).to(dev)
    d_gt_alpha = _alpha_tensor(gt_alpha, len(gt_rows), 'gt_alpha', dev)
    d_det_alpha = _alpha_tensor(det_alpha, len(det_rows), 'det_alpha', dev)
    with torch.cuda.device(dev):
        _lib.check(lib.pgnn_kitti_pair_orientation(
            _host_ptr(gt_off), _host_ptr(det_off), n_frames,
            _lib.ptr(d_gt if len(gt_rows) else None),
            _lib.ptr(d_det if len(det_rows) else None), _lib.ptr(d_gt_alpha),
            _lib.ptr(d_det_alpha), _lib.ptr(ws), ws.numel(),
            _lib.ptr(sim if n_pairs else None), _lib.stream_ptr()),
            "pgnn_kitti_pair_orientation")
        torch.cuda.current_stream().synchronize()
    return sim.cpu().numpy(), pair_off


def pair_overlaps(gt_labels, det_labels, device=None):
    """pgnn_kitti_pair_overlaps -> (overlaps float64 [4, n_pairs], pair_off
    int64 [F+1]): planes 2D, BEV, 3D, DontCare detection criterion; the block
    of frame f starts at pair_off[f], row-major [ground truth][detection]."""
    lib = _lib.load()
    gt_off, gt_rows, gt_names = pack_labels(gt_labels)
    det_off, det_rows, _ = pack_labels(det_labels)
    if len(gt_off) != len(det_off):
        raise ValueError("frame counts differ")
    dev = _device(device)
    n_frames = len(gt_off) - 1
    per_frame = np.diff(gt_off).astype(np.int64) * np.diff(det_off)
    pair_off = np.concatenate([[0], np.cumsum(per_frame)]).astype(np.int64)
    n_pairs = int(pair_off[-1])
    ws_bytes = int(lib.pgnn_kitti_eval_workspace_bytes(
        n_frames, len(gt_rows), len(det_rows), n_pairs))
    ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=dev)
    ov = torch.zeros((4, n_pairs), dtype=torch.float64, device=dev)
    d_gt = torch.from_numpy(gt_rows).to(dev)
    d_gt_names = torch.from_numpy(gt_names).to(dev)
    d_det = torch.from_numpy(det_rows).to(dev)
    with torch.cuda.device(dev):
        _lib.check(lib.pgnn_kitti_pair_overlaps(
            _host_ptr(gt_off), _host_ptr(det_off), n_frames,
            _lib.ptr(d_gt if len(gt_rows) else None),
            _lib.ptr(d_gt_names if len(gt_rows) else None),
            _lib.ptr(d_det if len(det_rows) else None), _lib.ptr(ws),
            ws.numel(), _lib.ptr(ov if n_pairs else None),
            _lib.stream_ptr()), "pgnn_kitti_pair_overlaps")
        torch.cuda.current_stream().synchronize()
    return ov.cpu().numpy(), pair_off


def _index(value, names, what):
    if isinstance(value, str):
        low = [n.lower() for n in names]
        if value.lower() not in low:
            raise ValueError("unknown %s %r (one of %s)" % (what, value, names))
        return low.index(value.lower())
    value = int(value)
    if not 0 <= value < len(names):
        raise ValueError("%s index %d out of range" % (what, value))
    return value


class KittiEvalResult(object):
    """The arrays of pgnn_kitti_eval on the host, indexed [metric][class]
    [difficulty] (METRICS, CLASSES, DIFFICULTIES): precision, recall,
    thresholds [.., 41]; counters [.., 41, 3] (tp, fp, fn); n_thresholds, n_gt,
    ap_r11, ap_r40 [..].  `min_overlap` [metric][class] is the table the run
    used.  With `has_aos`, the orientation of the 2D metric, [class]
    [difficulty]: similarity, orientation [.., 41]; aos_r11, aos_r40 [..];
    without, those arrays are NaN."""

    def __init__(self, arrays, classes=CLASSES, has_aos=False,
                 min_overlap=None):
        for key, _, _ in _OUT_LAYOUT:
            setattr(self, key, arrays[key])
        self.has_aos = bool(has_aos)
        for key, _, shape in _AOS_LAYOUT:
            setattr(self, key, arrays[key] if self.has_aos
                    else np.full(shape, np.nan))
        self.min_overlap = min_overlap_table(min_overlap)
        self.classes = tuple(CLASSES[_index(c, CLASSES, 'class')]
                             for c in classes)

    @classmethod
    def from_buffer(cls, out, classes=CLASSES, ex=False, has_aos=False,
                    min_overlap=None):
        """One read of the device output buffer: run_packed's, or with `ex`
        run_packed_ex's (`has_aos`: it ran with alphas)."""
        host = out.cpu().numpy().tobytes()
        sections, _ = _sections_of(_EX_LAYOUT if ex else _OUT_LAYOUT)
        arrays = {}
        for key, (off, nbytes, dtype, shape) in sections.items():
            arrays[key] = np.frombuffer(
                host, dtype=dtype, count=nbytes // np.dtype(dtype).itemsize,
                offset=off).reshape(shape).copy()
        return cls(arrays, classes, has_aos, min_overlap)

    def aos(self, cls, difficulty, points=40):
        """One average orientation similarity in [0, 1] (NaN without
        `has_aos`); arguments as `ap`'s."""
        c = _index(cls, CLASSES, 'class')
        d = _index(difficulty, DIFFICULTIES, 'difficulty')
        if points not in (11, 40):
            raise ValueError("points must be 11 or 40")
        table = self.aos_r40 if points == 40 else self.aos_r11
        return float(table[c, d])

    def ap(self, metric, cls, difficulty, points=40):
        """One average precision in [0, 1].  metric: '2d' / 'bev' / '3d' (or
        the report names, or 0-2); cls: a class name or 0-2; difficulty:
        'easy' / 'moderate' / 'hard' or 0-2; points: 40 or 11."""
        if isinstance(metric, str) and metric.lower() in REPORT_NAMES:
            m = REPORT_NAMES.index(metric.lower())
        else:
            m = _index(metric, METRICS, 'metric')
        c = _index(cls, CLASSES, 'class')
        d = _index(difficulty, DIFFICULTIES, 'difficulty')
        if points not in (11, 40):
            raise ValueError("points must be 11 or 40")
        table = self.ap_r40 if points == 40 else self.ap_r11
        return float(table[m, c, d])

    def format(self, points=40, alongside=True):
        """The official tool's report lines, `<class>_<metric> AP: easy
        moderate hard` in percent, for the `points`-point interpolation; with
        `alongside` the other interpolation follows under `<...>_R11` (or
        `_R40`) names.  With `has_aos`, `<class>_orientation AOS: ...`
        follows each class's `detection` line."""
        lines = []
        sets = [(points, '')]
        if alongside:
            other = 11 if points == 40 else 40
            sets.append((other, '_R%d' % other))
        for pts, suffix in sets:
            for cls in self.classes:
                for m, rep in enumerate(REPORT_NAMES):
                    lines.append('%s_%s%s AP: %s' % (
                        cls.lower(), rep, suffix, ' '.join(
                            '%.6f' % (100.0 * self.ap(m, cls, d, pts))
                            for d in range(3))))
                    if m == 0 and self.has_aos:
                        lines.append('%s_orientation%s AOS: %s' % (
                            cls.lower(), suffix, ' '.join(
                                '%.6f' % (100.0 * self.aos(cls, d, pts))
                                for d in range(3))))
        return '\n'.join(lines)

    def to_json(self):
        out = {}
        for cls in self.classes:
            for m, rep in enumerate(REPORT_NAMES):
                for pts in (40, 11):
                    out['%s_%s_R%d' % (cls.lower(), rep, pts)] = [
                        100.0 * self.ap(m, cls, d, pts) for d in range(3)]
            if self.has_aos:
                for pts in (40, 11):
                    out['%s_orientation_R%d' % (cls.lower(), pts)] = [
                        100.0 * self.aos(cls, d, pts) for d in range(3)]
        return out


def detection_alpha(det_labels, det_rows, source):
    """The detections' alphas for AOS, or None where the official rule says
    AOS is not computed.  source 'file': the labels' `alpha`, None if any is
    -10; 'box': `alpha_from_box` of the packed rows."""
    if source == 'box':
        return alpha_from_box(det_rows)
    if source != 'file':
        raise ValueError("det_alpha must be 'file' or 'box', not %r"
                         % (source,))
    alpha = pack_alpha(det_labels)
    return None if np.any(alpha == NO_ALPHA) else alpha


def evaluate(gt_labels, det_labels, classes=CLASSES, device=None, aos=False,
             det_alpha='file', min_overlap=None):
    """gt_labels / det_labels: lists, over the same frames, of label lists.
    `classes` picks (and orders) the classes of the report; all three are
    always computed.  aos: also the orientation similarity of the 2D metric,
    ground-truth alpha from the labels, detection alpha by `det_alpha` ('file'
    or 'box', see `detection_alpha`).  min_overlap: None / 'official' /
    'loose' / 3x3 [metric][class].  Returns a KittiEvalResult."""
    if len(gt_labels) != len(det_labels):
        raise ValueError("ground truth and detections cover %d and %d frames"
                         % (len(gt_labels), len(det_labels)))
    gt, det = pack_labels(gt_labels), pack_labels(det_labels)
    if not aos and min_overlap is None:
        return KittiEvalResult.from_buffer(run_packed(gt, det, device=device),
                                           classes)
    alpha_det = detection_alpha(det_labels, det[1], det_alpha) if aos else None
    has_aos = alpha_det is not None
    out = run_packed_ex(gt, det, pack_alpha(gt_labels) if has_aos else None,
                        alpha_det, min_overlap, device=device)
    return KittiEvalResult.from_buffer(out, classes, True, has_aos,
                                       min_overlap)


def read_result_file(path):
    """Detections of one frame; a missing or empty file has none."""
    if not os.path.exists(path):
        return []
    return kitti_dataset.read_label_file(path)


def read_dirs(label_dir, result_dir, frame_names=None):
    """-> (frame_names, gt_labels, det_labels); frame_names defaults to the
    label files present."""
    if frame_names is None:
        frame_names = sorted(f[:-4] for f in os.listdir(label_dir)
                             if f.endswith('.txt'))
    gt = [kitti_dataset.read_label_file(os.path.join(label_dir, n + '.txt'))
          for n in frame_names]
    det = [read_result_file(os.path.join(result_dir, n + '.txt'))
           for n in frame_names]
    return list(frame_names), gt, det


def evaluate_dirs(label_dir, result_dir, frame_names=None, classes=CLASSES,
                  device=None, aos=False, det_alpha='file', min_overlap=None):
    _, gt, det = read_dirs(label_dir, result_dir, frame_names)
    return evaluate(gt, det, classes, device, aos, det_alpha, min_overlap)


def evaluate_dataset(dataset, result_dir, classes=CLASSES, device=None,
                     aos=False, det_alpha='file', min_overlap=None):
    """Scores `result_dir` (one <frame>.txt per frame, as run.run_dataset
    writes them) against the labels of a KittiDataset, over its frame list."""
    gt, det = [], []
    for i in range(dataset.num_files):
        gt.append(dataset.get_label(i))
        det.append(read_result_file(os.path.join(
            result_dir, dataset.get_filename(i) + '.txt')))
    return evaluate(gt, det, classes, device, aos, det_alpha, min_overlap)


# ---- per-box outcomes at one threshold ----------------------
def _codes(prefix):
    """The header's outcome codes of one side, names in code order."""
    n = _C[prefix + 'CODES']
    by_code = {v: k[len(prefix):] for k, v in _C.items()
               if k.startswith(prefix) and k != prefix + 'CODES'}
    return tuple(by_code[k] for k in range(n))


DET_OUTCOMES = _codes('PGNN_KITTI_DET_')     # DET_OUTCOMES[code] = 'TP', ...
GT_OUTCOMES = _codes('PGNN_KITTI_GT_')
DET_FP_KINDS = ('FP_DUPLICATE', 'FP_CONFUSION', 'FP_LOCALISATION',
                'FP_BACKGROUND')
GT_FN_KINDS = ('FN_LOW_SCORE', 'FN_LOCALISATION', 'FN_MISSED')


def run_match_packed(gt, det, metric, cls, difficulty, score_threshold,
                     min_overlap=None, loc_floor=0.1, device=None):
    """pgnn_kitti_match on packed labels (`pack_labels` triples) and indices
    0..2 -> dict of CUDA tensors: gt_outcome, gt_partner [n_gt] int32,
    det_outcome, det_partner [n_det] int32, det_overlap [n_det] float64,
    totals [18] int64.  Nothing has been read back."""
    lib = _lib.load()
    gt_off, gt_rows, gt_names = gt
    det_off, det_rows, det_names = det
    if len(gt_off) != len(det_off):
        raise ValueError("ground truth and detections cover %d and %d frames"
                         % (len(gt_off) - 1, len(det_off) - 1))
    table = min_overlap_table(min_overlap)
    dev = _device(device)
    n_frames, n_gt, n_det = len(gt_off) - 1, len(gt_rows), len(det_rows)
    ws_bytes = int(lib.pgnn_kitti_match_workspace_bytes(
        n_frames, n_gt, n_det, _pair_count(gt_off, det_off)))
    ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=dev)
    d_gt = torch.from_numpy(gt_rows).to(dev)
    d_gt_names = torch.from_numpy(gt_names).to(dev)
    d_det = torch.from_numpy(det_rows).to(dev)
    d_det_names = torch.from_numpy(det_names).to(dev)
    out = {'gt_outcome': torch.empty(n_gt, dtype=torch.int32, device=dev),
           'gt_partner': torch.empty(n_gt, dtype=torch.int32, device=dev),
           'det_outcome': torch.empty(n_det, dtype=torch.int32, device=dev),
           'det_partner': torch.empty(n_det, dtype=torch.int32, device=dev),
           'det_overlap': torch.empty(n_det, dtype=torch.float64, device=dev),
           'totals': torch.empty(_C['PGNN_KITTI_MATCH_TOTALS'],
                                 dtype=torch.int64, device=dev)}

    def dptr(t):
        return _lib.ptr(t if t.numel() else None)

    gt_off = np.ascontiguousarray(gt_off, np.int32)
    det_off = np.ascontiguousarray(det_off, np.int32)
    with torch.cuda.device(dev):
        _lib.check(lib.pgnn_kitti_match(
            _host_ptr(gt_off), _host_ptr(det_off), n_frames, dptr(d_gt),
            dptr(d_gt_names), dptr(d_det), dptr(d_det_names),
            _host_ptr(table), int(metric), int(cls), int(difficulty),
            float(score_threshold), float(loc_floor), _lib.ptr(ws),
            ws.numel(), dptr(out['gt_outcome']), dptr(out['gt_partner']),
            dptr(out['det_outcome']), dptr(out['det_partner']),
            dptr(out['det_overlap']), _lib.ptr(out['totals']),
            _lib.stream_ptr()), "pgnn_kitti_match")
        # the host offsets and the device inputs must outlive the launches
        torch.cuda.current_stream().synchronize()
    return out


class KittiMatchResult(object):
    """The outcome of every box of a frame set under one (metric, class,
    difficulty) at one score threshold, on the host.  Packed over the frames,
    frame f owning gt_offsets[f] .. gt_offsets[f + 1] (det_offsets likewise):
    det_outcome, det_partner (int32), det_overlap (float64), gt_outcome,
    gt_partner (int32); codes index DET_OUTCOMES / GT_OUTCOMES, partners are
    indices within the frame or -1.  `totals`: boxes per code, keyed 'DET_TP',
    'GT_FN_MISSED', ...  `tp`, `fp`, `fn`: what the protocol counts at this
    threshold (fp: the four FP kinds, fn: the three FN kinds)."""

    def __init__(self, arrays, gt_offsets, det_offsets, metric, cls,
                 difficulty, score_threshold, loc_floor, min_overlap=None,
                 frame_names=None):
        for key in ('det_outcome', 'det_partner', 'det_overlap', 'gt_outcome',
                    'gt_partner'):
            setattr(self, key, arrays[key])
        self.gt_offsets = np.asarray(gt_offsets, np.int32)
        self.det_offsets = np.asarray(det_offsets, np.int32)
        self.metric, self.cls, self.difficulty = metric, cls, difficulty
        self.score_threshold = float(score_threshold)
        self.loc_floor = float(loc_floor)
        self.min_overlap = min_overlap_table(min_overlap)
        self.frame_names = None if frame_names is None else list(frame_names)
        counts = [int(x) for x in arrays['totals']]
        self.totals = dict(
            [('DET_' + n, counts[k]) for k, n in enumerate(DET_OUTCOMES)] +
            [('GT_' + n, counts[len(DET_OUTCOMES) + k])
             for k, n in enumerate(GT_OUTCOMES)])
        self.tp = self.totals['GT_TP']
        self.fp = sum(self.totals['DET_' + k] for k in DET_FP_KINDS)
        self.fn = sum(self.totals['GT_' + k] for k in GT_FN_KINDS)

    @property
    def n_frames(self):
        return len(self.gt_offsets) - 1

    def frame(self, f):
        """(det_outcome, det_partner, det_overlap, gt_outcome, gt_partner) of
        frame f: what render_frame's `outcomes` takes."""
        if not 0 <= f < self.n_frames:
            raise IndexError("frame %d of %d" % (f, self.n_frames))
        d = slice(self.det_offsets[f], self.det_offsets[f + 1])
        g = slice(self.gt_offsets[f], self.gt_offsets[f + 1])
        return (self.det_outcome[d], self.det_partner[d], self.det_overlap[d],
                self.gt_outcome[g], self.gt_partner[g])

    def format(self):
        """A small table: the combination and threshold, tp / fp / fn, then
        the false positives and the false negatives by kind, then the other
        codes that occur."""
        lines = ['%s %s %s at score >= %.6f: tp %d fp %d fn %d' % (
            CLASSES[self.cls].lower(), REPORT_NAMES[self.metric],
            DIFFICULTIES[self.difficulty], self.score_threshold, self.tp,
            self.fp, self.fn)]

        def share(key, of):
            n = self.totals[key]
            lines.append('  %-20s %7d %6.1f%%' % (
                key.split('_', 1)[1].lower(), n, 100.0 * n / of if of else 0.0))
        lines.append('false positives')
        for kind in DET_FP_KINDS:
            share('DET_' + kind, self.fp)
        lines.append('false negatives')
        for kind in GT_FN_KINDS:
            share('GT_' + kind, self.fn)
        rest = [k for k in self.totals if self.totals[k] and
                k.split('_', 1)[1] not in DET_FP_KINDS + GT_FN_KINDS]
        lines.append('other boxes')
        for key in rest:
            lines.append('  %-20s %7d' % (key.lower(), self.totals[key]))
        return '\n'.join(lines)

    def to_json(self):
        return {'metric': METRICS[self.metric], 'class': CLASSES[self.cls],
                'difficulty': DIFFICULTIES[self.difficulty],
                'score_threshold': self.score_threshold,
                'loc_floor': self.loc_floor,
                'min_overlap': float(self.min_overlap[self.metric, self.cls]),
                'tp': self.tp, 'fp': self.fp, 'fn': self.fn,
                'totals': dict(self.totals)}


def _combination(metric, cls, difficulty):
    if isinstance(metric, str) and metric.lower() in REPORT_NAMES:
        m = REPORT_NAMES.index(metric.lower())
    else:
        m = _index(metric, METRICS, 'metric')
    return (m, _index(cls, CLASSES, 'class'),
            _index(difficulty, DIFFICULTIES, 'difficulty'))


def match(gt_labels, det_labels, metric='3d', cls='Car', difficulty='moderate',
          score_threshold=0.0, min_overlap=None, loc_floor=0.1, device=None,
          frame_names=None):
    """The official matching of one (metric, class, difficulty) at one score
    threshold over a frame set, box by box (pgnn_kitti_match; the outcome
    codes and the error kinds are DESIGN.md §9.13).  gt_labels / det_labels as
    `evaluate`'s; metric / cls / difficulty: names or 0..2; min_overlap as
    `evaluate`'s; loc_floor: the overlap from which a miss counts as a
    localisation error.  One read of each output.  Returns a
    KittiMatchResult."""
    if len(gt_labels) != len(det_labels):
        raise ValueError("ground truth and detections cover %d and %d frames"
                         % (len(gt_labels), len(det_labels)))
    m, c, d = _combination(metric, cls, difficulty)
    gt, det = pack_labels(gt_labels), pack_labels(det_labels)
    out = run_match_packed(gt, det, m, c, d, score_threshold, min_overlap,
                           loc_floor, device)
    arrays = {key: t.cpu().numpy() for key, t in out.items()}
    return KittiMatchResult(arrays, gt[0], det[0], m, c, d, score_threshold,
                            loc_floor, min_overlap, frame_names)


def match_dirs(label_dir, result_dir, frame_names=None, **kwargs):
    """`match` of two directories of KITTI txt files, read as `evaluate_dirs`
    reads them; the result carries the frame names."""
    names, gt, det = read_dirs(label_dir, result_dir, frame_names)
    return match(gt, det, frame_names=names, **kwargs)


def best_f1_threshold(result, metric, cls, difficulty):
    """The stored threshold of a KittiEvalResult's combination at which
    2 tp / (2 tp + fp + fn) of its counters is largest; of equal values the
    higher threshold.  The comparison is on integers (cross products), so no
    rounding decides.  ValueError when the combination has no threshold.  On
    the host."""
    m, c, d = _combination(metric, cls, difficulty)
    n = int(result.n_thresholds[m, c, d])
    if n == 0:
        raise ValueError("%s %s %s has no threshold: no ground truth was "
                         "matched" % (METRICS[m], CLASSES[c], DIFFICULTIES[d]))
    best, best_num, best_den = None, 0, 1
    for t in range(n):
        tp, fp, fn = (int(x) for x in result.counters[m, c, d, t])
        num, den = 2 * tp, 2 * tp + fp + fn
        thr = float(result.thresholds[m, c, d, t])
        # num / den against best_num / best_den; 0 / 0 counts as 0
        left, right = num * max(best_den, 1), best_num * max(den, 1)
        if best is None or left > right or (left == right and thr > best):
            best, best_num, best_den = thr, num, den
    return best


# ---- precision / recall curves: data files and plots -------------------------
ORIENTATION = 'orientation'     # the fourth file and plot, with has_aos
CURVE_COLORS = ((0, 160, 0), (0, 0, 255), (255, 0, 0))   # easy, moderate, hard
PLOT_MIN_SIZE = (160, 120)


def _curve_key(metric):
    """-> 0..2 (METRICS / REPORT_NAMES) or ORIENTATION."""
    if isinstance(metric, str) and metric.lower() in (ORIENTATION, 'aos'):
        return ORIENTATION
    if isinstance(metric, str) and metric.lower() in REPORT_NAMES:
        return REPORT_NAMES.index(metric.lower())
    return _index(metric, METRICS, 'metric')


def _curves(result, key, c):
    """([3, 41] curve values, [3] R40 averages, file stem) of one class."""
    if key == ORIENTATION:
        if not result.has_aos:
            raise ValueError("the result carries no orientation similarity")
        return result.orientation[c], result.aos_r40[c], ORIENTATION
    return result.precision[key, c], result.ap_r40[key, c], REPORT_NAMES[key]


def _curve_keys(result):
    return (0, 1, 2) + ((ORIENTATION,) if result.has_aos else ())


def write_pr_data(result, directory):
    """One file per class of the report and metric, named as the official
    tool names them: <class>_detection.txt, _detection_ground.txt,
    _detection_3d.txt and, when the result carries AOS, _orientation.txt.  41
    lines "%f %f %f %f": the recall i / 40, then the easy, moderate and hard
    value the result holds at that sample point (precision; orientation
    similarity in the fourth file).  Returns the paths."""
    os.makedirs(directory, exist_ok=True)
    paths = []
    for cls in result.classes:
        c = CLASSES.index(cls)
        for key in _curve_keys(result):
            values, _, stem = _curves(result, key, c)
            path = os.path.join(directory, '%s_%s.txt' % (cls.lower(), stem))
            with open(path, 'w') as f:
                for i in range(N_SAMPLE_PTS):
                    f.write('%f %f %f %f\n' % (
                        i / (N_SAMPLE_PTS - 1.0), values[0, i], values[1, i],
                        values[2, i]))
            paths.append(path)
    return paths


def plot_area(width=640, height=480):
    """(x0, y0, x1, y1): the pixels of the axis box of a plot_pr image.  A
    recall r in [0, 1] is drawn in column x(r) = x0 + floor(r * (x1 - x0)), a
    precision p in row y(p) = y1 - floor(p * (y1 - y0))."""
    width, height = int(width), int(height)
    if width < PLOT_MIN_SIZE[0] or height < PLOT_MIN_SIZE[1] or \
            width > 4096 or height > 4096:
        raise ValueError("a plot is %d x %d .. 4096 x 4096, got %d x %d" % (
            PLOT_MIN_SIZE + (width, height)))
    return 40, 28, width - 16, height - 30


def plot_x(area, r):
    return area[0] + int(np.floor(r * (area[2] - area[0])))


def plot_y(area, p):
    return area[3] - int(np.floor(p * (area[3] - area[1])))


def plot_pr(result, metric, cls, width=640, height=480):
    """The curves of one class and metric ('2d' / 'bev' / '3d', a report name,
    or 'orientation') as a CUDA uint8 [height, width, 3] image: white ground,
    the axis box of plot_area with ticks and labels 0.0 .. 1.0 every 0.2, the
    easy, moderate and hard curve in CURVE_COLORS as polylines through the 41
    sample points (drawn in that order: hard is on top), a title naming class
    and metric and, in the lower left of the box, the three R40 averages in
    percent in their curve's colour.  A NaN value breaks the curve there."""
    from . import render as R
    key = _curve_key(metric)
    c = _index(cls, CLASSES, 'class')
    values, averages, stem = _curves(result, key, c)
    area = plot_area(width, height)
    x0, y0, x1, y1 = area
    black = (0, 0, 0)
    segs, cols = [], []

    def line(xa, ya, xb, yb, color):
        segs.append(((xa, ya, 0.0), (xb, yb, 0.0)))
        cols.append(color)
    for xa, ya, xb, yb in ((x0, y0, x1, y0), (x1, y0, x1, y1),
                           (x1, y1, x0, y1), (x0, y1, x0, y0)):
        line(xa, ya, xb, yb, black)
    ticks = [k / 5.0 for k in range(6)]
    strings, anchors, colors = [], [], []

    def write(string, x, y, color=black, scale=1):
        strings.append((string, scale))
        anchors.append((x, y))
        colors.append(color)
    for t in ticks:
        label = '%.1f' % t
        tw, th = R.text_size(label)
        x, y = plot_x(area, t), plot_y(area, t)
        line(x, y1, x, y1 + 4, black)
        line(x0 - 4, y, x0, y, black)
        write(label, x - tw // 2, y1 + 7)
        write(label, x0 - 7 - tw, y - th // 2)
    for d in range(3):
        xs = [plot_x(area, i / (N_SAMPLE_PTS - 1.0))
              for i in range(N_SAMPLE_PTS)]
        for i in range(N_SAMPLE_PTS - 1):
            a, b = float(values[d, i]), float(values[d, i + 1])
            if not (np.isfinite(a) and np.isfinite(b)):
                continue
            a, b = min(max(a, 0.0), 1.0), min(max(b, 0.0), 1.0)
            line(xs[i], plot_y(area, a), xs[i + 1], plot_y(area, b),
                 CURVE_COLORS[d])
    image = R.render(R.pixel_view(width, height),
                     segments=np.array(segs, dtype=np.float64),
                     segment_colors=np.array(cols, dtype=np.uint8),
                     background=(255, 255, 255))
    write('%s %s' % (CLASSES[c], stem), x0, 6, scale=2)
    write('Precision' if key != ORIENTATION else 'Orientation', 2, y0 - 9)
    tw, _ = R.text_size('Recall')
    write('Recall', (x0 + x1 - tw) // 2, y1 + 18)
    for d in range(3):
        write('%-8s %6.2f' % (DIFFICULTIES[d], 100.0 * averages[d]),
              x0 + 8, y1 - 36 + 10 * d, CURVE_COLORS[d])
    return R.draw_text(image, [s for s, _ in strings], anchors,
                       colors=np.array(colors, dtype=np.uint8),
                       scale=np.array([k for _, k in strings], dtype=np.uint8),
                       anchor='tl')


def write_pr_plots(result, directory, fmt='png', png_encoder='zlib'):
    """plot_pr of every class of the report and metric that has ground truth,
    as <directory>/<class>_<report name>.<fmt>, fmt 'png' or 'ppm'.
    png_encoder: 'zlib' (host) or 'device', render.write_png's `encoder`.
    Returns the paths."""
    from . import render as R
    if fmt not in ('png', 'ppm'):
        raise ValueError("fmt must be 'png' or 'ppm', got %r" % (fmt,))
    R._check_encoder(png_encoder)
    os.makedirs(directory, exist_ok=True)
    paths = []
    for cls in result.classes:
        c = CLASSES.index(cls)
        for key in _curve_keys(result):
            m = 0 if key == ORIENTATION else key
            if not int(np.sum(result.n_gt[m, c])):
                continue
            stem = ORIENTATION if key == ORIENTATION else REPORT_NAMES[key]
            path = os.path.join(directory, '%s_%s.%s' % (
                cls.lower(), stem, fmt))
            image = plot_pr(result, key, c)
            if fmt == 'png':
                R.write_png(path, image, encoder=png_encoder)
            else:
                R.write_ppm(path, image)
            paths.append(path)
    return paths


def parse_args(argv=None):
    import argparse
    ap = argparse.ArgumentParser(
        description="KITTI object AP (2D, BEV, 3D) of a result directory")
    ap.add_argument('label_dir')
    ap.add_argument('result_dir')
    ap.add_argument('--split', metavar='FILE',
                    help="frame names, one per line (default: every label "
                         "file)")
    ap.add_argument('--json', action='store_true',
                    help="print one JSON line after the report")
    ap.add_argument('--aos', action='store_true',
                    help="also the average orientation similarity (2D)")
    ap.add_argument('--alpha-from-box', action='store_true',
                    help="with --aos: the detections' alpha is yaw - "
                         "atan2(x3d, z3d) of their 3D box, not the alpha field")
    ap.add_argument('--min-overlap', metavar='TABLE', type=min_overlap_table,
                    default=None,
                    help="official (default), loose (BEV and 3D at 0.5 / 0.25 "
                         "/ 0.25) or 9 comma-separated numbers [metric][class]")
    ap.add_argument('--plot', metavar='DIR', default=None,
                    help="write the precision/recall data files "
                         "(<class>_detection.txt, ...) and one plot per class "
                         "and metric into DIR")
    ap.add_argument('--png-encoder', choices=('zlib', 'device'),
                    default='zlib',
                    help="with --plot: compress the plots on the host (zlib) "
                         "or on the GPU (device: faster, larger files)")
    add_error_arguments(ap, "also print, for one combination at one score "
                            "threshold, the false positives and false "
                            "negatives by kind")
    return ap.parse_args(argv)


def threshold_argument(value):
    """'f1' or a float: the --at-threshold of the command lines."""
    if str(value).lower() == 'f1':
        return 'f1'
    try:
        return float(value)
    except ValueError:
        raise ValueError("a threshold is 'f1' or a number, not %r" % (value,))


def add_error_arguments(ap, errors_help):
    ap.add_argument('--errors', action='store_true', help=errors_help)
    ap.add_argument('--error-metric', choices=METRICS, default='3d')
    ap.add_argument('--error-class', choices=CLASSES, default='Car')
    ap.add_argument('--error-difficulty', choices=DIFFICULTIES,
                    default='moderate')
    ap.add_argument('--at-threshold', metavar='f1|SCORE',
                    type=threshold_argument, default='f1',
                    help="with --errors: a score, or f1 (default): the "
                         "stored threshold of the combination with the best "
                         "F1")


def resolve_threshold(score_threshold, result, metric, cls, difficulty):
    """'f1' -> best_f1_threshold of `result` (a KittiEvalResult; 0.0 where the
    combination has no threshold: every detection is kept); a number ->
    itself."""
    if isinstance(score_threshold, str):
        if score_threshold.lower() != 'f1':
            raise ValueError("score_threshold is a number or 'f1', not %r"
                             % (score_threshold,))
        try:
            return best_f1_threshold(result, metric, cls, difficulty)
        except ValueError:
            return 0.0
    return float(score_threshold)


def main(argv=None):
    args = parse_args(argv)
    names = None
    if args.split:
        with open(args.split) as f:
            names = [l.strip() for l in f if l.strip()]
    result = evaluate_dirs(args.label_dir, args.result_dir, names,
                           aos=args.aos,
                           det_alpha='box' if args.alpha_from_box else 'file',
                           min_overlap=args.min_overlap)
    print(result.format())
    if args.plot:
        write_pr_data(result, args.plot)
        write_pr_plots(result, args.plot, png_encoder=args.png_encoder)
    errors = None
    if args.errors:
        combo = (args.error_metric, args.error_class, args.error_difficulty)
        errors = match_dirs(
            args.label_dir, args.result_dir, names, metric=combo[0],
            cls=combo[1], difficulty=combo[2], min_overlap=args.min_overlap,
            score_threshold=resolve_threshold(args.at_threshold, result,
                                              *combo))
        print(errors.format())
    if args.json:
        js = result.to_json()
        if errors is not None:
            js['errors'] = errors.to_json()
        print(json.dumps(js))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
