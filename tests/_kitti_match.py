"""Host restatement of the per-box outcomes of DESIGN.md §9.13 and the cases
that reach each of its rules, shared by test_kitti_match_cases_cpu.py and
test_gpu_kitti_match.py.

`match_frame` is the serial loop of tests/_kitti_eval.py::match (compute_fp),
extended to remember who was assigned to whom, followed by the classification
rules written as the section states them.  Plain Python over one frame's
overlap table; it knows nothing of the kernel.  The codes are the header's.
"""
import numpy as np

import _kitti_eval as K
from _kitti_eval import MIN_OVERLAP, clean
from pointgnn_amd import _header

_C = _header.constants()
DET = {k[len('PGNN_KITTI_DET_'):]: v for k, v in _C.items()
       if k.startswith('PGNN_KITTI_DET_') and not k.endswith('_CODES')}
GT = {k[len('PGNN_KITTI_GT_'):]: v for k, v in _C.items()
      if k.startswith('PGNN_KITTI_GT_') and not k.endswith('_CODES')}
N_DET_CODES, N_GT_CODES = _C['PGNN_KITTI_DET_CODES'], _C['PGNN_KITTI_GT_CODES']
FP_KINDS = ('FP_DUPLICATE', 'FP_CONFUSION', 'FP_LOCALISATION', 'FP_BACKGROUND')
FN_KINDS = ('FN_LOW_SCORE', 'FN_LOCALISATION', 'FN_MISSED')
OFFICIAL = (MIN_OVERLAP,) * 3              # [metric][class]
LOOSE = ((0.7, 0.5, 0.5), (0.5, 0.25, 0.25), (0.5, 0.25, 0.25))
CAR, PED, CYC = 0, 1, 2
EASY, MODERATE, HARD = 0, 1, 2
M2D, BEV, M3D = 0, 1, 2


def match_frame(gts, dets, ov, metric, c, d, thresh, min_overlap,
                loc_floor=0.1):
    """-> (det_outcome, det_partner, det_overlap, gt_outcome, gt_partner) of
    one frame; ov: its [4, ng, nd] overlap table."""
    ignored_gt, ignored_det, dc, _ = clean(gts, dets, c, d)
    ng, nd = len(gts), len(dets)
    scores = [a['score'] for a in dets]
    o, ov_dc = ov[metric], ov[3]
    below = [scores[j] < thresh for j in range(nd)]
    det_gt = [-1] * nd              # the ground truth a detection was given to
    gt_det = [-1] * ng
    absorbed = [-1] * nd            # the DontCare row that took it
    # ---- §9.5 "Matching", compute_fp, remembering the assignments
    for i in range(ng):
        if ignored_gt[i] == -1:
            continue
        det_idx, valid_detection = -1, None
        max_overlap, assigned_ignored = 0.0, False
        for j in range(nd):
            if ignored_det[j] == -1 or det_gt[j] >= 0 or below[j]:
                continue
            if o[i, j] > min_overlap and \
                    (o[i, j] > max_overlap or assigned_ignored) and \
                    ignored_det[j] == 0:
                max_overlap, det_idx = o[i, j], j
                valid_detection, assigned_ignored = 1, False
            elif o[i, j] > min_overlap and valid_detection is None and \
                    ignored_det[j] == 1:
                det_idx, valid_detection, assigned_ignored = j, 1, True
        if valid_detection is not None:
            det_gt[det_idx], gt_det[i] = i, det_idx
    if metric == 0:
        for i in dc:
            for j in range(nd):
                if det_gt[j] >= 0 or absorbed[j] >= 0 or \
                        ignored_det[j] in (-1, 1) or below[j]:
                    continue
                if ov_dc[i, j] > min_overlap:
                    absorbed[j] = i
    # ---- detections, the rules in their order
    det_outcome, det_partner, det_overlap = [], [], []
    for j in range(nd):
        partner, with_ = -1, 0.0
        if ignored_det[j] == -1:
            code = 'OTHER'
        elif below[j]:
            code = 'BELOW'
        elif det_gt[j] >= 0:
            partner = det_gt[j]
            with_ = o[partner, j]
            code = 'TP' if ignored_gt[partner] == 0 and ignored_det[j] == 0 \
                else 'MATCHED_IGNORED'
        elif ignored_det[j] == 1:
            code = 'IGNORED_SMALL'
        elif absorbed[j] >= 0:
            code, partner = 'DONTCARE', absorbed[j]
            with_ = ov_dc[partner, j]
        else:
            b, b_i, x, x_i = 0.0, -1, 0.0, -1
            for i in range(ng):
                if ignored_gt[i] >= 0:
                    if o[i, j] > b:
                        b, b_i = o[i, j], i
                elif i not in dc and o[i, j] > x:
                    x, x_i = o[i, j], i
            if b > min_overlap:
                code, partner, with_ = 'FP_DUPLICATE', b_i, b
            elif x >= loc_floor and x > b:
                code, partner, with_ = 'FP_CONFUSION', x_i, x
            elif b >= loc_floor:
                code, partner, with_ = 'FP_LOCALISATION', b_i, b
            else:
                code = 'FP_BACKGROUND'
        det_outcome.append(DET[code])
        det_partner.append(partner)
        det_overlap.append(with_)
    # ---- ground truths
    gt_outcome, gt_partner = [], []
    for i in range(ng):
        partner = gt_det[i]
        if ignored_gt[i] == -1:
            code = 'OTHER'
        elif ignored_gt[i] == 1:
            code = 'IGNORED_MATCHED' if partner >= 0 else 'IGNORED'
        elif partner >= 0:
            code = 'TP' if ignored_det[partner] == 0 else 'MATCHED_SMALL'
        else:
            low = [j for j in range(nd) if ignored_det[j] != -1 and below[j]
                   and o[i, j] > min_overlap]
            loc = [j for j in range(nd) if ignored_det[j] == 0 and
                   not below[j] and loc_floor <= o[i, j] <= min_overlap]
            if low:
                code, who = 'FN_LOW_SCORE', low
            elif loc:
                code, who = 'FN_LOCALISATION', loc
            else:
                code, who = 'FN_MISSED', []
            if who:
                top = max(o[i, j] for j in who)
                partner = min(j for j in who if o[i, j] == top)
        gt_outcome.append(GT[code])
        gt_partner.append(partner)
    return (np.array(det_outcome, np.int32), np.array(det_partner, np.int32),
            np.array(det_overlap, np.float64), np.array(gt_outcome, np.int32),
            np.array(gt_partner, np.int32))


def match_set(gt_frames, det_frames, overlaps, metric, c, d, thresh,
              min_overlap=None, loc_floor=0.1):
    """The frames of a set, packed as pgnn_kitti_match packs them -> dict of
    det_outcome, det_partner, det_overlap, gt_outcome, gt_partner, totals."""
    table = OFFICIAL if min_overlap is None else min_overlap
    parts = [match_frame(g, a, ov, metric, c, d, thresh, table[metric][c],
                         loc_floor)
             for g, a, ov in zip(gt_frames, det_frames, overlaps)]
    keys = ('det_outcome', 'det_partner', 'det_overlap', 'gt_outcome',
            'gt_partner')
    dtypes = (np.int32, np.int32, np.float64, np.int32, np.int32)
    out = {}
    for k, (key, dtype) in enumerate(zip(keys, dtypes)):
        out[key] = np.concatenate([p[k] for p in parts] +
                                  [np.zeros(0, dtype)]).astype(dtype)
    out['totals'] = np.concatenate([
        np.bincount(out['det_outcome'], minlength=N_DET_CODES),
        np.bincount(out['gt_outcome'], minlength=N_GT_CODES)]).astype(np.int64)
    return out


def counts(result):
    """(tp, fp, fn) as the protocol counts them, from `totals`."""
    t = result['totals']
    return (int(t[N_DET_CODES + GT['TP']]),
            int(sum(t[DET[k]] for k in FP_KINDS)),
            int(sum(t[N_DET_CODES + GT[k]] for k in FN_KINDS)))


# -------------------------------------------------------------------- cases
# Every case: (gt_frames, det_frames), 1 to 3 frames.  Detections to be kept
# score >= 0.5, the threshold the tests use unless they say otherwise.
THRESHOLD = 0.5


def shifted(gt, metres, score):
    """A detection of gt's size `metres` further along x: 3D and BEV overlap
    (3.9 - s) / (3.9 + s) with a Car of yaw 0; the 2D box stays."""
    det = K.detection_of(gt, score)
    det['x3d'] = gt['x3d'] + metres
    return det


def case_duplicate():
    car = K.easy_car(0)
    return [[car]], [[shifted(car, 0.2, 0.9), K.detection_of(car, 0.8)]]


def case_localisation():
    car = K.easy_car(0)                      # 1.8 / 6.0 = 0.3
    return [[car]], [[shifted(car, 2.1, 0.9)]]


def case_confusion():
    cyc = K.easy_car(0, 'Cyclist')
    van = K.easy_car(1, 'Van')
    return [[cyc, van]], [[K.detection_of(cyc, 0.9, 'Car'),
                           K.detection_of(van, 0.8, 'Car')]]


def case_background():
    car = K.easy_car(0)
    stray = K.label('Car', (820.0, 120.0, 900.0, 180.0), xyz=(30.0, 1.6, 50.0),
                    score=0.9)
    return [[car]], [[K.detection_of(car, 0.8), stray]]


def case_low_score():
    car = K.easy_car(0)
    return [[car], [car]], [[K.detection_of(car, 0.25)],
                            [K.detection_of(car, THRESHOLD)]]


def case_fn_localisation():
    a, b = K.easy_car(0), K.easy_car(1)
    return [[a, b]], [[shifted(b, 2.1, 0.7), shifted(b, 2.6, 0.9)]]


def case_missed():
    a, b = K.easy_car(0), K.easy_car(1)
    return [[a, b]], [[K.detection_of(a, 0.9)]]


def _low(gt, score, name=None):
    """gt's detection with a 2D box of 24 px: idj == 1 at every difficulty."""
    det = K.detection_of(gt, score, name)
    det.update(ymin=gt['ymin'] + 3.0, ymax=gt['ymin'] + 27.0)
    return det


def _car30(k):
    """An easy_car whose 2D box is 30 px high: ig == 0 at moderate and hard,
    1 at easy; its 24 px detection overlaps it by 0.8 in 2D."""
    car = K.easy_car(k)
    car['ymax'] = car['ymin'] + 30.0
    return car


def case_small_det():
    car = _car30(0)
    lone = K.label('Car', (820.0, 120.0, 900.0, 144.0), xyz=(30.0, 1.6, 50.0),
                   score=0.9)                # 24 px, on nothing
    # a second car, found at the threshold: the set has a stored threshold
    other = K.easy_car(3)
    return [[car, other]], [[_low(car, 0.9), lone,
                             K.detection_of(other, THRESHOLD)]]


def case_small_then_valid():
    car = _car30(0)
    other = K.easy_car(3)        # as in case_small_det
    return [[car, other]], [[_low(car, 0.95), K.detection_of(car, 0.6),
                             K.detection_of(other, THRESHOLD)]]


def case_valid_tie():
    """Two different boxes with the same bits of 2D overlap on a Pedestrian
    (600 / 800 from either end); their 3D boxes are the ground truth's, so
    BEV and 3D tie at 1.0."""
    ped = K.label('Pedestrian', (100.0, 100.0, 120.0, 140.0),
                  K._SIZES['Pedestrian'], (0.0, 1.7, 15.0))
    left, right = K.detection_of(ped, 0.6), K.detection_of(ped, 0.9)
    left.update(xmax=115.0)
    right.update(xmin=105.0)
    return [[ped]], [[left, right]]


def case_dontcare_2d():
    return K.case_dontcare()


def case_harder_gt():
    seen = K.easy_car(0)
    seen['occlusion'] = 1
    unseen = K.easy_car(1)
    unseen['occlusion'] = 1
    return [[seen, unseen]], [[K.detection_of(seen, 0.9)]]


def case_empty_sides():
    car = K.easy_car(0)
    return [[car], [], []], [[], [K.detection_of(car, 0.9)], []]


def case_word_seams():
    gt, det = [], []
    for n in (63, 64, 65):
        car = K.easy_car(0)
        filler = [K.label('Car', (10.0 * k, 250.0, 10.0 * k + 8, 300.0),
                          xyz=(-70.0 + 2.2 * k, 1.6, 60.0), score=0.85)
                  for k in range(n - 1)]
        gt.append([car])
        det.append(filler + [K.detection_of(car, 0.9)])
    return gt, det


GT_SEAMS = (62, 63, 64, 127, 128, 129)


def case_gt_seams():
    """130 ground truths, far-away Misc but six easy Cars either side of the
    indices 64 and 128: missed, found, found, found, 0.3 off, under the
    threshold.  The detections come in another order."""
    filler = K.label('Misc', (1200.0, 300.0, 1230.0, 360.0),
                     xyz=(500.0, 1.6, 500.0))
    gts = [filler] * 130
    cars = [K.easy_car(k) for k in range(6)]
    for at, car in zip(GT_SEAMS, cars):
        gts[at] = car
    dets = [K.detection_of(cars[3], 0.9), K.detection_of(cars[2], 0.8),
            shifted(cars[4], 2.1, 0.7), K.detection_of(cars[1], 0.6),
            K.detection_of(cars[5], 0.25)]
    return [gts], [dets]


LOC_FLOOR_EDGE = 0.25       # the loc_floor the next case is built for


def case_loc_floor_edge():
    """2D overlaps that are exact in binary, with Pedestrians (min_overlap
    0.5) and loc_floor = LOC_FLOOR_EDGE: 400 / 800 = min_overlap, 200 / 800 =
    loc_floor, 100 / 800 under it."""
    size = K._SIZES['Pedestrian']
    peds = [K.label('Pedestrian', (100.0 + 200 * k, 100.0, 120.0 + 200 * k,
                                   140.0), size, (5.0 * k, 1.7, 15.0))
            for k in range(3)]
    dets = []
    for ped, width in zip(peds, (10.0, 5.0, 2.5)):
        det = K.detection_of(ped, 0.9)
        det['xmax'] = ped['xmin'] + width
        dets.append(det)
    return [peds], [dets]


def case_generated():
    gt, det, _, _ = K.generated(11, 6)
    return gt, det


CASES = {'duplicate': case_duplicate, 'localisation': case_localisation,
         'confusion': case_confusion, 'background': case_background,
         'low_score': case_low_score, 'fn_localisation': case_fn_localisation,
         'missed': case_missed, 'small_det': case_small_det,
         'small_then_valid': case_small_then_valid,
         'valid_tie': case_valid_tie, 'dontcare_2d': case_dontcare_2d,
         'harder_gt': case_harder_gt, 'empty_sides': case_empty_sides,
         'word_seams': case_word_seams, 'gt_seams': case_gt_seams,
         'loc_floor_edge': case_loc_floor_edge,
         'generated': case_generated}
SMALL_CASES = sorted(set(CASES) - {'generated'})


def case(name):
    """(gt_frames, det_frames, host overlaps, host evaluation), built once."""
    if name == 'generated':
        return K.generated(11, 6)
    return K.with_host('match_' + name, CASES[name])
