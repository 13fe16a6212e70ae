"""Host restatement of the KITTI object AP protocol, a seeded
generator of frames and the hand-built cases, shared by test_kitti_eval_cpu.py
and test_gpu_kitti_eval.py.

The restatement follows the protocol text in plain Python, one step per
heading; it knows nothing of the kernels.  Its polygon intersection is
oracle.detect_oracle.ConvexPolygon (vertex collection and angular sort), not
the Sutherland-Hodgman clip of csrc/box_overlap.h.
"""
import math

import numpy as np

from oracle.detect_oracle import ConvexPolygon

CLASSES = ('Car', 'Pedestrian', 'Cyclist')
MIN_HEIGHT = (40, 25, 25)
MAX_OCCLUSION = (0, 1, 2)
MAX_TRUNCATION = (0.15, 0.3, 0.5)
MIN_OVERLAP = (0.7, 0.5, 0.5)
N_SAMPLE_PTS = 41
NEIGHBOUR = {'car': 'van', 'pedestrian': 'person_sitting', 'cyclist': None}
ALL_NAMES = ('Car', 'Van', 'Truck', 'Pedestrian', 'Person_sitting', 'Cyclist',
             'Tram', 'Misc', 'DontCare')


def label(name, box2d, hwl=(1.5, 1.6, 3.9), xyz=(0.0, 1.6, 20.0), yaw=0.0,
          truncation=0.0, occlusion=0, score=None):
    """A label dict as kitti_dataset.read_label_file returns it."""
    lab = {'name': name, 'truncation': float(truncation),
           'occlusion': int(occlusion), 'alpha': 0.0,
           'xmin': float(box2d[0]), 'ymin': float(box2d[1]),
           'xmax': float(box2d[2]), 'ymax': float(box2d[3]),
           'height': float(hwl[0]), 'width': float(hwl[1]),
           'length': float(hwl[2]), 'x3d': float(xyz[0]),
           'y3d': float(xyz[1]), 'z3d': float(xyz[2]), 'yaw': float(yaw)}
    if score is not None:
        lab['score'] = float(score)
    return lab


def detection_of(gt, score, name=None):
    det = dict(gt)
    det['score'] = float(score)
    if name is not None:
        det['name'] = name
    return det


# ---------------------------------------------------------------- overlaps
def overlap_2d(a, b, criterion):
    w = min(a['xmax'], b['xmax']) - max(a['xmin'], b['xmin'])
    h = min(a['ymax'], b['ymax']) - max(a['ymin'], b['ymin'])
    if w <= 0 or h <= 0:
        return 0.0
    inter = w * h
    area_a = (a['xmax'] - a['xmin']) * (a['ymax'] - a['ymin'])
    area_b = (b['xmax'] - b['xmin']) * (b['ymax'] - b['ymin'])
    if criterion == 'union':
        return inter / (area_a + area_b - inter)
    return inter / area_a


def bev_corners(b):
    c, s = math.cos(b['yaw']), math.sin(b['yaw'])
    hl, hw = b['length'] / 2, b['width'] / 2
    return [(c * dx + s * dz + b['x3d'], -s * dx + c * dz + b['z3d'])
            for dx, dz in ((hl, hw), (hl, -hw), (-hl, -hw), (-hl, hw))]


def inter_bev(a, b):
    # rectangles whose centres are further apart than their half diagonals
    # reach share nothing: the area is exactly 0 (saves the polygon code on
    # the many far pairs of a frame)
    ra = 0.5 * math.hypot(a['length'], a['width'])
    rb = 0.5 * math.hypot(b['length'], b['width'])
    if math.hypot(a['x3d'] - b['x3d'], a['z3d'] - b['z3d']) > \
            1.001 * (ra + rb) + 1e-6:
        return 0.0
    return float(ConvexPolygon(bev_corners(a)).intersection(
        ConvexPolygon(bev_corners(b))).area)


def frame_overlaps(gts, dets):
    """[4, ng, nd]: 2D, BEV, 3D union overlaps of (gt i, det j); plane 3 the
    2D detection-criterion overlap for DontCare ground truths (else 0)."""
    ov = np.zeros((4, len(gts), len(dets)))
    for i, b in enumerate(gts):
        for j, a in enumerate(dets):
            ov[0, i, j] = overlap_2d(a, b, 'union')
            inter = inter_bev(a, b)
            ov[1, i, j] = inter / (a['length'] * a['width'] +
                                   b['length'] * b['width'] - inter)
            ymax = min(a['y3d'], b['y3d'])
            ymin = max(a['y3d'] - a['height'], b['y3d'] - b['height'])
            vol = inter * max(0, ymax - ymin)
            ov[2, i, j] = vol / (a['height'] * a['length'] * a['width'] +
                                 b['height'] * b['length'] * b['width'] - vol)
            if b['name'].lower() == 'dontcare':
                ov[3, i, j] = overlap_2d(a, b, 'detection')
    return ov


# ---------------------------------------------------------------- cleaning
def clean(gts, dets, c, d):
    cls = CLASSES[c].lower()
    ignored_gt, ignored_det, dc, n_gt = [], [], [], 0
    for i, g in enumerate(gts):
        name = g['name'].lower()
        height = abs(g['ymax'] - g['ymin'])
        valid = 1 if name == cls else (0 if name == NEIGHBOUR[cls] else -1)
        ignore = g['occlusion'] > MAX_OCCLUSION[d] or \
            g['truncation'] > MAX_TRUNCATION[d] or height <= MIN_HEIGHT[d]
        if valid == 1 and not ignore:
            ignored_gt.append(0)
            n_gt += 1
        elif valid == 0 or (ignore and valid == 1):
            ignored_gt.append(1)
        else:
            ignored_gt.append(-1)
        if name == 'dontcare':
            dc.append(i)
    for a in dets:
        height = abs(a['ymax'] - a['ymin'])
        if height < MIN_HEIGHT[d]:
            ignored_det.append(1)
        elif a['name'].lower() == cls:
            ignored_det.append(0)
        else:
            ignored_det.append(-1)
    return ignored_gt, ignored_det, dc, n_gt


# ---------------------------------------------------------------- matching
def match(ignored_gt, ignored_det, dc, ov, ov_dc, scores, min_overlap, thresh,
          compute_fp, is_2d):
    """-> tp, fp, fn, recorded scores."""
    nd = len(ignored_det)
    assigned = [False] * nd
    below = [compute_fp and scores[j] < thresh for j in range(nd)]
    tp = fp = fn = 0
    recorded = []
    for i in range(len(ignored_gt)):
        if ignored_gt[i] == -1:
            continue
        det_idx, valid_detection = -1, None
        max_overlap, assigned_ignored = 0.0, False
        for j in range(nd):
            if ignored_det[j] == -1 or assigned[j] or below[j]:
                continue
            o = ov[i, j]
            if not compute_fp and o > min_overlap and \
                    (valid_detection is None or scores[j] > valid_detection):
                det_idx, valid_detection = j, scores[j]
            elif compute_fp and o > min_overlap and \
                    (o > max_overlap or assigned_ignored) and \
                    ignored_det[j] == 0:
                max_overlap, det_idx = o, j
                valid_detection, assigned_ignored = 1, False
            elif compute_fp and o > min_overlap and \
                    valid_detection is None and ignored_det[j] == 1:
                det_idx, valid_detection, assigned_ignored = j, 1, True
        if valid_detection is None and ignored_gt[i] == 0:
            fn += 1
        elif valid_detection is not None and \
                (ignored_gt[i] == 1 or ignored_det[det_idx] == 1):
            assigned[det_idx] = True
        elif valid_detection is not None:
            tp += 1
            recorded.append(scores[det_idx])
            assigned[det_idx] = True
    if compute_fp:
        for j in range(nd):
            if not (assigned[j] or ignored_det[j] in (-1, 1) or below[j]):
                fp += 1
        nstuff = 0
        if is_2d:
            for i in dc:
                for j in range(nd):
                    if assigned[j] or ignored_det[j] in (-1, 1) or below[j]:
                        continue
                    if ov_dc[i, j] > min_overlap:
                        assigned[j] = True
                        nstuff += 1
        fp -= nstuff
    return tp, fp, fn, recorded


def thresholds_of(v, n_gt):
    v = sorted(v, reverse=True)
    out = []
    current_recall = 0.0
    for i in range(len(v)):
        l = (i + 1) / n_gt
        r = (i + 2) / n_gt if i < len(v) - 1 else l
        if (r - current_recall) < (current_recall - l) and i < len(v) - 1:
            continue
        out.append(v[i])
        current_recall += 1.0 / 40.0
    return out


def evaluate_host(gt_frames, det_frames, overlaps=None):
    """The whole protocol -> dict of the arrays pgnn_kitti_eval returns,
    indexed [metric][class][difficulty]."""
    if overlaps is None:
        overlaps = [frame_overlaps(g, d) for g, d in zip(gt_frames, det_frames)]
    res = {'precision': np.zeros((3, 3, 3, N_SAMPLE_PTS)),
           'recall': np.zeros((3, 3, 3, N_SAMPLE_PTS)),
           'counters': np.zeros((3, 3, 3, N_SAMPLE_PTS, 3), np.int64),
           'thresholds': np.zeros((3, 3, 3, N_SAMPLE_PTS)),
           'n_thresholds': np.zeros((3, 3, 3), np.int32),
           'n_gt': np.zeros((3, 3, 3), np.int64),
           'ap_r11': np.zeros((3, 3, 3)), 'ap_r40': np.zeros((3, 3, 3))}
    scores = [[a['score'] for a in dets] for dets in det_frames]
    for c in range(3):
        for d in range(3):
            cleaned = [clean(g, a, c, d) for g, a in zip(gt_frames, det_frames)]
            n_gt = sum(x[3] for x in cleaned)
            for m in range(3):
                v = []
                for f, (ig, idet, dc, _) in enumerate(cleaned):
                    v += match(ig, idet, dc, overlaps[f][m], overlaps[f][3],
                               scores[f], MIN_OVERLAP[c], 0, False, m == 0)[3]
                thr = thresholds_of(v, n_gt)
                assert len(thr) <= N_SAMPLE_PTS
                res['n_gt'][m, c, d] = n_gt
                res['n_thresholds'][m, c, d] = len(thr)
                precision = [0.0] * N_SAMPLE_PTS
                for t, thresh in enumerate(thr):
                    tp = fp = fn = 0
                    for f, (ig, idet, dc, _) in enumerate(cleaned):
                        a, b, e, _ = match(ig, idet, dc, overlaps[f][m],
                                           overlaps[f][3], scores[f],
                                           MIN_OVERLAP[c], thresh, True, m == 0)
                        tp, fp, fn = tp + a, fp + b, fn + e
                    res['thresholds'][m, c, d, t] = thresh
                    res['counters'][m, c, d, t] = (tp, fp, fn)
                    # a quotient without a denominator is 0 (§9.5)
                    precision[t] = tp / (tp + fp) if tp + fp else 0.0
                    res['recall'][m, c, d, t] = tp / (tp + fn) if tp + fn else 0.0
                for t in range(N_SAMPLE_PTS):
                    precision[t] = max(precision[t:])
                res['precision'][m, c, d] = precision
                s11 = 0.0
                for t in range(0, N_SAMPLE_PTS, 4):
                    s11 += precision[t]
                s40 = 0.0
                for t in range(1, N_SAMPLE_PTS):
                    s40 += precision[t]
                res['ap_r11'][m, c, d] = s11 / 11
                res['ap_r40'][m, c, d] = s40 / 40
    return res


# --------------------------------------------------------------- generator
_SIZES = {'Car': (1.5, 1.6, 3.9), 'Van': (2.0, 1.9, 5.0),
          'Truck': (3.2, 2.6, 10.0), 'Pedestrian': (1.7, 0.6, 0.8),
          'Person_sitting': (1.3, 0.6, 0.8), 'Cyclist': (1.7, 0.6, 1.8),
          'Tram': (3.5, 2.5, 15.0), 'Misc': (2.0, 1.5, 3.0)}
# 2D heights spread around the 25 and 40 px limits, truncations around theirs
_HEIGHTS = (18.0, 24.5, 25.0, 25.5, 33.0, 39.5, 40.0, 40.5, 55.0, 70.0, 90.0,
            140.0)
_TRUNCATIONS = (0.0, 0.0, 0.0, 0.0, 0.1, 0.14, 0.16, 0.29, 0.31, 0.49, 0.51, 0.8)
# all nine names, the three evaluated classes more often than the rest
_NAME_WEIGHTS = (0.24, 0.06, 0.04, 0.2, 0.06, 0.2, 0.04, 0.04, 0.12)


def _random_gt(rng, name):
    x0 = float(rng.integers(0, 1100))
    y0 = float(rng.integers(100, 200))
    if name == 'DontCare':
        w, h = float(rng.integers(40, 200)), float(rng.integers(20, 80))
        return label(name, (x0, y0, x0 + w, y0 + h), (-1, -1, -1),
                     (-1000, -1000, -1000), -10, -1, -1)
    h2d = float(rng.choice(_HEIGHTS))
    w2d = h2d * float(rng.uniform(0.4, 2.0))
    size = np.array(_SIZES[name]) * rng.uniform(0.85, 1.15, 3)
    xyz = (rng.uniform(-25, 25), rng.uniform(1.2, 2.0), rng.uniform(5, 70))
    return label(name, (x0, y0, x0 + w2d, y0 + h2d), size, xyz,
                 rng.uniform(-math.pi, math.pi),
                 float(rng.choice(_TRUNCATIONS)),
                 int(rng.choice(4, p=(0.45, 0.25, 0.2, 0.1))))


def _jitter(rng, gt, name, amount):
    """A detection near `gt`: 2D corners moved by a few per cent of the box,
    the 3D box by `amount` of its size."""
    w, h = gt['xmax'] - gt['xmin'], gt['ymax'] - gt['ymin']
    j2 = rng.normal(0, 0.04 * amount, 4) * (w, h, w, h)
    j3 = rng.normal(0, 0.06 * amount, 3)
    size = np.array([gt['height'], gt['width'], gt['length']])
    return label(name, (gt['xmin'] + j2[0], gt['ymin'] + j2[1],
                        gt['xmax'] + j2[2], gt['ymax'] + j2[3]),
                 size * rng.uniform(0.95, 1.05, 3),
                 (gt['x3d'] + j3[0] * size[2], gt['y3d'] + j3[1] * 0.3,
                  gt['z3d'] + j3[2] * size[2]),
                 gt['yaw'] + rng.normal(0, 0.1 * amount), -1, -1,
                 score=float(rng.integers(1, 21)) / 20.0)   # exact ties


def _stray(rng, dcs):
    """A free-standing false positive, half of them inside a DontCare region
    (when the frame has one)."""
    fp = _random_gt(rng, str(rng.choice(CLASSES)))
    if dcs and rng.random() < 0.5:
        r = dcs[int(rng.integers(len(dcs)))]
        w, h = r['xmax'] - r['xmin'], r['ymax'] - r['ymin']
        fp.update(xmin=r['xmin'] + 0.1 * w, xmax=r['xmin'] + 0.6 * w,
                  ymin=r['ymin'] - 0.1 * h, ymax=r['ymax'] + 0.2 * h)
    fp.update(truncation=-1.0, occlusion=-1,
              score=float(rng.integers(1, 21)) / 20.0)
    return fp


def random_frame(rng, n_gt, n_free):
    gts = [_random_gt(rng, str(rng.choice(ALL_NAMES, p=_NAME_WEIGHTS)))
           for _ in range(n_gt)]
    dets = []
    for g in gts:
        if g['name'] == 'DontCare':
            continue
        # detections carry one of the three classes: mostly the right one, a
        # Van / Person_sitting is reported as its neighbour class
        guess = {'Van': 'Car', 'Person_sitting': 'Pedestrian'}.get(g['name'])
        name = g['name'] if g['name'] in CLASSES else \
            (guess or str(rng.choice(CLASSES)))
        if rng.random() < 0.1:
            name = str(rng.choice(CLASSES))
        if rng.random() < 0.85:
            dets.append(_jitter(rng, g, name, rng.choice((0.3, 1.0, 2.5))))
            if rng.random() < 0.35:            # a duplicate of the same box
                dup = dict(dets[-1])
                dup['score'] = float(rng.integers(1, 21)) / 20.0
                dets.append(dup)
            if rng.random() < 0.25:            # a second, looser vote
                dets.append(_jitter(rng, g, name, 2.0))
    dcs = [g for g in gts if g['name'] == 'DontCare']
    for _ in range(n_free):
        dets.append(_stray(rng, dcs))
    order = rng.permutation(len(dets))
    return gts, [dets[k] for k in order]


def assert_rotated_gate(overlaps):
    """No BEV or 3D overlap within 1e-9 of a MIN_OVERLAP: the two clip
    algorithms differ in the last bits and a flip there would be an artefact
    of the test.  A condition on the committed seeds, not a tolerance."""
    for ov in overlaps:
        for bound in set(MIN_OVERLAP):
            assert not np.any(np.abs(ov[1:3] - bound) < 1e-9), \
                "seed puts a rotated overlap on a MIN_OVERLAP: pick another"


_CACHE = {}


def generated(seed, n_frames, n_gt=(10, 18), n_free=(2, 6)):
    """(gt_frames, det_frames, overlaps, host result), computed once per
    argument set and shared; callers must not modify it."""
    key = (seed, n_frames, n_gt, n_free)
    if key not in _CACHE:
        rng = np.random.default_rng(seed)
        frames = [random_frame(rng, int(rng.integers(n_gt[0], n_gt[1] + 1)),
                               int(rng.integers(n_free[0], n_free[1] + 1)))
                  for _ in range(n_frames)]
        gt = [f[0] for f in frames]
        det = [f[1] for f in frames]
        ov = [frame_overlaps(g, d) for g, d in zip(gt, det)]
        assert_rotated_gate(ov)
        _CACHE[key] = (gt, det, ov, evaluate_host(gt, det, ov))
    return _CACHE[key]


def with_host(key, build):
    """build() -> (gt_frames, det_frames); adds overlaps and the host result,
    once per key."""
    if key not in _CACHE:
        gt, det = build()
        ov = [frame_overlaps(g, d) for g, d in zip(gt, det)]
        assert_rotated_gate(ov)
        _CACHE[key] = (gt, det, ov, evaluate_host(gt, det, ov))
    return _CACHE[key]


# -------------------------------------------------------------- hand cases
def easy_car(k=0, name='Car', h2d=60.0):
    """Car k of a row of well separated, unoccluded, untruncated cars: 2D
    boxes 100 px apart, 3D boxes 10 m apart."""
    return label(name, (20.0 + 100 * k, 100.0, 80.0 + 100 * k, 100.0 + h2d),
                 xyz=(-40.0 + 10 * k, 1.6, 20.0))


def case_one_car():
    g = easy_car()
    return [[g]], [[detection_of(g, 0.9)]]


def case_forty_cars():
    gt, det = [], []
    for f in range(4):
        cars = [easy_car(k) for k in range(10)]
        gt.append(cars)
        det.append([detection_of(c, 0.01 * (1 + f * 10 + k))
                    for k, c in enumerate(cars)])
    return gt, det


def case_van():
    car, van = easy_car(0), easy_car(1, 'Van')
    return [[car, van]], [[detection_of(car, 0.9),
                           detection_of(van, 0.95, 'Car')]]


def case_dontcare():
    car = easy_car(0)
    region = label('DontCare', (500.0, 100.0, 700.0, 200.0), (-1, -1, -1),
                   (-1000, -1000, -1000), -10, -1, -1)
    stray = label('Car', (520.0, 120.0, 600.0, 180.0), xyz=(10.0, 1.6, 40.0),
                  score=0.95)
    return [[car, region]], [[detection_of(car, 0.9), stray]]


def case_low_detection():
    big = easy_car(0)
    low_gt = label('Car', (300.0, 100.0, 400.0, 130.0), xyz=(0.0, 1.6, 30.0))
    low_det = detection_of(low_gt, 0.9)
    low_det.update(ymin=103.0, ymax=127.0)            # 24 px
    return [[big, low_gt]], [[detection_of(big, 0.5), low_det]]


def case_exact_ties():
    """2D IoU of exactly 0.5 with a Pedestrian (no match: the comparison is
    `>`), a detection and a ground truth of height exactly 25."""
    size = _SIZES['Pedestrian']
    ped = label('Pedestrian', (100.0, 100.0, 120.0, 140.0), size,
                (0.0, 1.7, 15.0))
    half = detection_of(ped, 0.8)
    half.update(xmax=110.0)        # inter 10 x 40, union 20 x 40: exactly 0.5
    ped30 = label('Pedestrian', (300.0, 100.0, 320.0, 130.0), size,
                  (5.0, 1.7, 15.0))
    det25 = detection_of(ped30, 0.7)
    det25.update(ymin=102.5, ymax=127.5)   # 25 px: inter 500, union 600
    ped25 = label('Pedestrian', (500.0, 100.0, 520.0, 125.0), size,
                  (10.0, 1.7, 15.0))
    return [[ped, ped30, ped25]], [[half, det25, detection_of(ped25, 0.65)]]


def case_sized(seed, n_gt, n_det):
    """One generated frame with exactly n_gt ground truths and n_det
    detections."""
    def build():
        rng = np.random.default_rng(seed)
        gts, dets = random_frame(rng, n_gt, 0)
        dcs = [g for g in gts if g['name'] == 'DontCare']
        while len(dets) < n_det:
            dets.append(_stray(rng, dcs))
        return [gts], [dets[:n_det]]
    return build


def case_bits_63_64():
    """Two Cars whose detections are number 63 and 64 of the frame: the last
    bit of the first mask word and the first of the second."""
    a, b = easy_car(0), easy_car(1)
    dets = [label('Car', (10.0 * k, 250.0, 10.0 * k + 8, 300.0),
                  xyz=(-70.0 + 2.2 * k, 1.6, 60.0), score=0.85)
            for k in range(63)]
    dets += [detection_of(a, 0.9), detection_of(b, 0.8), dict(dets[0])]
    return [[a, b]], [dets]


def case_cars(seed, per_frame, p_det=0.9):
    """Frames of easy Cars (per_frame[f] of them), most with a jittered
    detection (probability p_det), some with a stray one; scores tie."""
    def build():
        rng = np.random.default_rng(seed)
        gt, det = [], []
        for n in per_frame:
            slots = rng.permutation(10)[:n]
            cars = [easy_car(int(k)) for k in slots]
            dets = [_jitter(rng, c, 'Car', 0.3) for c in cars
                    if rng.random() < p_det]
            if rng.random() < 0.5:
                dets.append(_stray(rng, []))
            gt.append(cars)
            det.append(dets)
        return gt, det
    return build


def case_long_lists(seed, n_frames=9, per_frame=1000, cars=8):
    """Frames of `per_frame` ground truths, all `Misc` far away but `cars`
    easy Cars at random places of the list: the recorded scores lie
    scattered over n_frames * per_frame slots (several tiles of the
    device's sort), the lists are near the per-frame cap."""
    def build():
        rng = np.random.default_rng(seed)
        filler = label('Misc', (1200.0, 300.0, 1230.0, 360.0),
                       xyz=(500.0, 1.6, 500.0))
        gt, det = [], []
        for _ in range(n_frames):
            gts = [filler] * per_frame
            found = []
            for k, at in zip(rng.permutation(10)[:cars],
                             rng.permutation(per_frame)[:cars]):
                gts[int(at)] = easy_car(int(k))
                found.append(gts[int(at)])
            dets = [_jitter(rng, c, 'Car', 0.3) for c in found
                    if rng.random() < 0.9]
            dets.append(_stray(rng, []))
            gt.append(gts)
            det.append([dets[k] for k in rng.permutation(len(dets))])
        return gt, det
    return build


def case_equal_scores():
    gt, det, _, _ = generated(11, 6)
    return gt, [[dict(a, score=0.5) for a in dets] for dets in det]


HAND_CASES = {'one_car': case_one_car, 'forty_cars': case_forty_cars,
              'van': case_van, 'dontcare': case_dontcare,
              'low_detection': case_low_detection,
              'exact_ties': case_exact_ties}
