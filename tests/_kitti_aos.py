"""Host restatement of the additions to the KITTI protocol (DESIGN.md §9.5,
"Orientation" and "Overlap table"), shared by test_kitti_aos_cpu.py and
test_gpu_kitti_aos.py.  Everything else -- overlaps, cleaning, thresholds,
the generator, the hand cases -- is tests/_kitti_eval.py, unchanged.
"""
import math

import numpy as np

import _kitti_eval as K

OFFICIAL = ((0.7, 0.5, 0.5),) * 3
LOOSE = ((0.7, 0.5, 0.5), (0.5, 0.25, 0.25), (0.5, 0.25, 0.25))
HALF = ((0.5, 0.5, 0.5),) * 3
BOUNDS = (0.25, 0.5, 0.7)
EPS = 2.0 ** -53
# the deltas of the pair-plane test beside the random ones
SPECIAL_DELTAS = (0.0, math.pi / 2, -math.pi / 2, math.pi, -math.pi,
                  2 * math.pi, -2 * math.pi, 3 * math.pi, -3 * math.pi, 1e-300)


def match_pairs(ignored_gt, ignored_det, dc, ov, ov_dc, scores, min_overlap,
                thresh, compute_fp, is_2d):
    """K.match, restated, -> tp, fp, fn, recorded scores, and the (i,
    det_idx) of every true positive in the order they are found."""
    nd = len(ignored_det)
    assigned = [False] * nd
    below = [compute_fp and scores[j] < thresh for j in range(nd)]
    tp = fp = fn = 0
    recorded, pairs = [], []
    for i in range(len(ignored_gt)):
        if ignored_gt[i] == -1:
            continue
        det_idx, valid_detection = -1, None
        max_overlap, assigned_ignored = 0.0, False
        for j in range(nd):
            if ignored_det[j] == -1 or assigned[j] or below[j]:
                continue
            o = ov[i, j]
            if not o > min_overlap:
                continue
            if not compute_fp:
                if valid_detection is None or scores[j] > valid_detection:
                    det_idx, valid_detection = j, scores[j]
            elif (o > max_overlap or assigned_ignored) and ignored_det[j] == 0:
                max_overlap, det_idx = o, j
                valid_detection, assigned_ignored = 1, False
            elif valid_detection is None and ignored_det[j] == 1:
                det_idx, valid_detection, assigned_ignored = j, 1, True
        if valid_detection is None:
            if ignored_gt[i] == 0:
                fn += 1
            continue
        assigned[det_idx] = True
        if not (ignored_gt[i] == 1 or ignored_det[det_idx] == 1):
            tp += 1
            recorded.append(scores[det_idx])
            pairs.append((i, det_idx))
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
    return tp, fp, fn, recorded, pairs


def _checked_match(*args):
    got = match_pairs(*args)
    assert got[:4] == K.match(*args), "match_pairs left K.match"
    return got


def term(alpha_gt, alpha_det):
    return (1.0 + math.cos(alpha_gt - alpha_det)) / 2.0


def alphas_of(frames):
    return [[lab['alpha'] for lab in labels] for labels in frames]


def with_alphas(frames, alphas):
    """Copies of the labels with their `alpha` replaced."""
    return [[dict(lab, alpha=float(a)) for lab, a in zip(labels, al)]
            for labels, al in zip(frames, alphas)]


def random_alphas(frames, seed):
    rng = np.random.default_rng(seed)
    return [[float(a) for a in rng.uniform(-math.pi, math.pi, len(labels))]
            for labels in frames]


def assert_gate(overlaps, table):
    """No BEV or 3D overlap within 1e-9 of a bound of `table` (see
    K.assert_rotated_gate: a condition on the input, not a tolerance)."""
    for ov in overlaps:
        for bound in set(np.asarray(table, np.float64).reshape(-1)):
            assert not np.any(np.abs(ov[1:3] - bound) < 1e-9), \
                "a rotated overlap lies on the bound %r: pick another seed" \
                % bound


def evaluate_host_ex(gt_frames, det_frames, overlaps=None, table=None,
                     gt_alpha=None, det_alpha=None, metrics=(0, 1, 2),
                     classes=(0, 1, 2), check_match=True):
    """K.evaluate_host with MIN_OVERLAP[metric][class] from `table` (None:
    the official one) and, given the alphas (lists over frames of lists), the
    orientation of the 2D metric: similarity, orientation [3, 3, 41]; aos_r11,
    aos_r40 [3, 3], indexed [class][difficulty].  `metrics` / `classes`
    restrict the work (the rest stays 0)."""
    if overlaps is None:
        overlaps = [K.frame_overlaps(g, d)
                    for g, d in zip(gt_frames, det_frames)]
    table = np.asarray(OFFICIAL if table is None else table, np.float64)
    assert table.shape == (3, 3)
    aos = gt_alpha is not None
    match = _checked_match if check_match else match_pairs
    n_pts = K.N_SAMPLE_PTS
    res = {'precision': np.zeros((3, 3, 3, n_pts)),
           'recall': np.zeros((3, 3, 3, n_pts)),
           'counters': np.zeros((3, 3, 3, n_pts, 3), np.int64),
           'thresholds': np.zeros((3, 3, 3, n_pts)),
           'n_thresholds': np.zeros((3, 3, 3), np.int32),
           'n_gt': np.zeros((3, 3, 3), np.int64),
           'ap_r11': np.zeros((3, 3, 3)), 'ap_r40': np.zeros((3, 3, 3))}
    if aos:
        res.update(similarity=np.zeros((3, 3, n_pts)),
                   orientation=np.zeros((3, 3, n_pts)),
                   aos_r11=np.zeros((3, 3)), aos_r40=np.zeros((3, 3)))
    scores = [[a['score'] for a in dets] for dets in det_frames]

    def curve(values):
        values = list(values)
        for t in range(n_pts):
            values[t] = max(values[t:])
        s11 = 0.0
        for t in range(0, n_pts, 4):
            s11 += values[t]
        s40 = 0.0
        for t in range(1, n_pts):
            s40 += values[t]
        return values, s11 / 11, s40 / 40

    for c in classes:
        for d in range(3):
            cleaned = [K.clean(g, a, c, d)
                       for g, a in zip(gt_frames, det_frames)]
            n_gt = sum(x[3] for x in cleaned)
            for m in metrics:
                bound = float(table[m, c])
                v = []
                for f, (ig, idet, dc, _) in enumerate(cleaned):
                    v += match(ig, idet, dc, overlaps[f][m], overlaps[f][3],
                               scores[f], bound, 0, False, m == 0)[3]
                thr = K.thresholds_of(v, n_gt)
                assert len(thr) <= n_pts
                res['n_gt'][m, c, d] = n_gt
                res['n_thresholds'][m, c, d] = len(thr)
                precision = [0.0] * n_pts
                orientation = [0.0] * n_pts
                for t, thresh in enumerate(thr):
                    tp = fp = fn = 0
                    terms = []
                    for f, (ig, idet, dc, _) in enumerate(cleaned):
                        a, b, e, _, pairs = match(
                            ig, idet, dc, overlaps[f][m], overlaps[f][3],
                            scores[f], bound, thresh, True, m == 0)
                        tp, fp, fn = tp + a, fp + b, fn + e
                        if aos and m == 0:
                            terms += [term(gt_alpha[f][i], det_alpha[f][j])
                                      for i, j in pairs]
                    res['thresholds'][m, c, d, t] = thresh
                    res['counters'][m, c, d, t] = (tp, fp, fn)
                    precision[t] = tp / (tp + fp) if tp + fp else 0.0
                    res['recall'][m, c, d, t] = tp / (tp + fn) if tp + fn else 0.0
                    if aos and m == 0:
                        sim = math.fsum(terms)
                        res['similarity'][c, d, t] = sim
                        orientation[t] = sim / (tp + fp) if tp + fp else 0.0
                res['precision'][m, c, d], s11, s40 = curve(precision)
                res['ap_r11'][m, c, d], res['ap_r40'][m, c, d] = s11, s40
                if aos and m == 0:
                    res['orientation'][c, d], s11, s40 = curve(orientation)
                    res['aos_r11'][c, d], res['aos_r40'][c, d] = s11, s40
    return res


def similarity_bounds(host, term_tol):
    """[3, 3, 41] bounds on |device similarity - host similarity| and on the
    |orientation difference|, and the one on the AOS differences.  N = tp
    terms, each within term_tol of the host's, added in float64 in some order
    (N - 1 roundings of partial sums of non-negative terms, none above the
    total S) where the host has the exact sum, fsum:
        similarity   N * term_tol + (N - 1) * 2^-53 * S
        orientation  that / (tp + fp) + 2^-52  (the division on either side)
        AOS          the largest orientation bound + 41 * 2^-53  (the running
                     maximum moves no value by more than the largest bound;
                     then at most 41 terms in [0, 1] are added)"""
    tp = host['counters'][0, :, :, :, 0].astype(np.float64)
    fp = host['counters'][0, :, :, :, 1].astype(np.float64)
    sim = tp * term_tol + np.maximum(tp - 1, 0) * EPS * host['similarity']
    ori = sim / np.maximum(tp + fp, 1) + 2 * EPS
    return sim, ori, ori.max(axis=-1) + 41 * EPS


def case_special_deltas():
    """One Car and a detection per SPECIAL_DELTAS entry on its 2D box
    (overlap 1 > 0): alpha_gt = 0 and alpha_det = -delta, so alpha_gt -
    alpha_det is the delta itself."""
    car = K.easy_car()
    dets = [dict(K.detection_of(car, 0.5), alpha=-delta)
            for delta in SPECIAL_DELTAS]
    return [[dict(car, alpha=0.0)]], [dets]
