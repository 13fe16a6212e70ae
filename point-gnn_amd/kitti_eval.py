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

A label is the dict of `kitti_dataset.read_label_file`; a detection carries
`score` as well.
"""
import ctypes
import json
import os

import numpy as np
import torch

from . import _lib
from . import kitti_dataset

CLASSES = ('Car', 'Pedestrian', 'Cyclist')
METRICS = ('2d', 'bev', '3d')
DIFFICULTIES = ('easy', 'moderate', 'hard')
# the official tool's names of the three metrics in its report lines
REPORT_NAMES = ('detection', 'detection_ground', 'detection_3d')
ROW = 14            # PGNN_KITTI_ROW
N_SAMPLE_PTS = 41   # PGNN_KITTI_SAMPLE_PTS
N_COMBOS = 27       # PGNN_KITTI_COMBOS
MAX_DET = 1024      # PGNN_KITTI_MAX_DET
MAX_GT = 1024       # PGNN_KITTI_MAX_GT

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
    ap_r11, ap_r40 [..]."""

    def __init__(self, arrays, classes=CLASSES):
        for key, _, _ in _OUT_LAYOUT:
            setattr(self, key, arrays[key])
        self.classes = tuple(CLASSES[_index(c, CLASSES, 'class')]
                             for c in classes)

    @classmethod
    def from_buffer(cls, out, classes=CLASSES):
        """One read of the device output buffer."""
        host = out.cpu().numpy().tobytes()
        sections, _ = _out_sections()
        arrays = {}
        for key, (off, nbytes, dtype, shape) in sections.items():
            arrays[key] = np.frombuffer(
                host, dtype=dtype, count=nbytes // np.dtype(dtype).itemsize,
                offset=off).reshape(shape).copy()
        return cls(arrays, classes)

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
        `_R40`) names."""
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
        return '\n'.join(lines)

    def to_json(self):
        out = {}
        for cls in self.classes:
            for m, rep in enumerate(REPORT_NAMES):
                for pts in (40, 11):
                    out['%s_%s_R%d' % (cls.lower(), rep, pts)] = [
                        100.0 * self.ap(m, cls, d, pts) for d in range(3)]
        return out


def evaluate(gt_labels, det_labels, classes=CLASSES, device=None):
    """gt_labels / det_labels: lists, over the same frames, of label lists.
    `classes` picks (and orders) the classes of the report; all three are
    always computed.  Returns a KittiEvalResult."""
    if len(gt_labels) != len(det_labels):
        raise ValueError("ground truth and detections cover %d and %d frames"
                         % (len(gt_labels), len(det_labels)))
    out = run_packed(pack_labels(gt_labels), pack_labels(det_labels),
                     device=device)
    return KittiEvalResult.from_buffer(out, classes)


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
                  device=None):
    _, gt, det = read_dirs(label_dir, result_dir, frame_names)
    return evaluate(gt, det, classes, device)


def evaluate_dataset(dataset, result_dir, classes=CLASSES, device=None):
    """Scores `result_dir` (one <frame>.txt per frame, as run.run_dataset
    writes them) against the labels of a KittiDataset, over its frame list."""
    gt, det = [], []
    for i in range(dataset.num_files):
        gt.append(dataset.get_label(i))
        det.append(read_result_file(os.path.join(
            result_dir, dataset.get_filename(i) + '.txt')))
    return evaluate(gt, det, classes, device)


def main(argv=None):
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
    args = ap.parse_args(argv)
    names = None
    if args.split:
        with open(args.split) as f:
            names = [l.strip() for l in f if l.strip()]
    result = evaluate_dirs(args.label_dir, args.result_dir, names)
    print(result.format())
    if args.json:
        print(json.dumps(result.to_json()))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
