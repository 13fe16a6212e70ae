"""Per-box outcomes of the KITTI matching without a GPU: the
restatement of tests/_kitti_match.py on the cases that reach each rule, the
restatement against the protocol statement of tests/_kitti_eval.py at every
stored threshold, best_f1_threshold on hand-made counters and the argument
checks of pgnn_kitti_match (which run before any HIP call)."""
import ctypes

import numpy as np
import pytest

import _kitti_match as M
from _kitti_match import (BEV, CAR, CYC, DET, EASY, GT, HARD, M2D, M3D,
                          MODERATE, PED)


def _run(name, metric=M3D, c=CAR, d=MODERATE, thresh=M.THRESHOLD, **kw):
    gt, det, ov, _ = M.case(name)
    return M.match_set(gt, det, ov, metric, c, d, thresh, **kw)


def _names(table, codes):
    back = {v: k for k, v in table.items()}
    return [back[int(c)] for c in codes]


def test_codes_are_dense_and_distinct():
    assert sorted(DET.values()) == list(range(M.N_DET_CODES)) and len(DET) == 10
    assert sorted(GT.values()) == list(range(M.N_GT_CODES)) and len(GT) == 8
    assert M._C['PGNN_KITTI_MATCH_TOTALS'] == 18
    # the rules are tested in the order of the codes
    assert [DET[k] for k in ('OTHER', 'BELOW', 'TP', 'MATCHED_IGNORED',
                             'IGNORED_SMALL', 'DONTCARE')] == list(range(6))


def test_duplicate():
    r = _run('duplicate')
    # detection 1 is the ground truth's own box (overlap 1.0) and takes it;
    # detection 0, 0.2 m off, overlaps by 3.7 / 4.1 > 0.7 and is left over
    assert _names(DET, r['det_outcome']) == ['FP_DUPLICATE', 'TP']
    assert list(r['det_partner']) == [0, 0] and list(r['gt_partner']) == [1]
    assert abs(r['det_overlap'][0] - 3.7 / 4.1) < 1e-12
    assert r['det_overlap'][1] > r['det_overlap'][0]
    assert _names(GT, r['gt_outcome']) == ['TP']
    assert M.counts(r) == (1, 1, 0)


def test_localisation_both_sides():
    r = _run('localisation')
    assert _names(DET, r['det_outcome']) == ['FP_LOCALISATION']
    assert _names(GT, r['gt_outcome']) == ['FN_LOCALISATION']
    assert list(r['det_partner']) == [0] and list(r['gt_partner']) == [0]
    assert abs(r['det_overlap'][0] - 0.3) < 1e-12
    # a floor above the overlap: background and missed, no partners
    r = _run('localisation', loc_floor=0.4)
    assert _names(DET, r['det_outcome']) == ['FP_BACKGROUND']
    assert _names(GT, r['gt_outcome']) == ['FN_MISSED']
    assert list(r['det_partner']) == [-1] and list(r['gt_partner']) == [-1]
    assert r['det_overlap'][0] == 0.0


def test_confusion_and_the_neighbour_class():
    r = _run('confusion')
    # a Car on a Cyclist is a confusion; a Car on a Van is matched and ignored
    assert _names(DET, r['det_outcome']) == ['FP_CONFUSION', 'MATCHED_IGNORED']
    assert _names(GT, r['gt_outcome']) == ['OTHER', 'IGNORED_MATCHED']
    assert list(r['det_partner']) == [0, 1]
    # the restatement's polygon clip of a box with itself: 1 to a few ulps
    assert np.abs(r['det_overlap'] - 1.0).max() < 1e-12
    assert M.counts(r) == (0, 1, 0)
    # evaluating Cyclist, both detections are another class's
    r = _run('confusion', c=CYC)
    assert _names(DET, r['det_outcome']) == ['OTHER', 'OTHER']
    assert _names(GT, r['gt_outcome']) == ['FN_MISSED', 'OTHER']


def test_background():
    r = _run('background')
    assert _names(DET, r['det_outcome']) == ['TP', 'FP_BACKGROUND']
    assert r['det_partner'][1] == -1 and r['det_overlap'][1] == 0.0


def test_low_score_and_the_comparison_is_less_than():
    r = _run('low_score')
    assert _names(DET, r['det_outcome']) == ['BELOW', 'TP']
    assert _names(GT, r['gt_outcome']) == ['FN_LOW_SCORE', 'TP']
    assert list(r['gt_partner']) == [0, 0]
    assert list(r['det_partner']) == [-1, 0]


def test_fn_localisation_names_the_nearest_and_missed_has_no_partner():
    r = _run('fn_localisation')
    assert _names(GT, r['gt_outcome']) == ['FN_MISSED', 'FN_LOCALISATION']
    assert list(r['gt_partner']) == [-1, 0]      # 0.3 beats 0.2
    assert _names(DET, r['det_outcome']) == ['FP_LOCALISATION'] * 2
    assert list(r['det_partner']) == [1, 1]
    r = _run('missed')
    assert _names(GT, r['gt_outcome']) == ['TP', 'FN_MISSED']


def test_small_detections():
    r = _run('small_det')
    assert _names(DET, r['det_outcome']) == ['MATCHED_IGNORED',
                                             'IGNORED_SMALL', 'TP']
    assert _names(GT, r['gt_outcome']) == ['MATCHED_SMALL', 'TP']
    assert M.counts(r) == (1, 0, 0)   # the protocol counts neither
    r = _run('small_then_valid')
    assert _names(DET, r['det_outcome']) == ['IGNORED_SMALL', 'TP', 'TP']
    assert list(r['gt_partner']) == [1, 2]
    # at easy the 30 px ground truth is itself ignored
    r = _run('small_then_valid', d=EASY)
    assert _names(GT, r['gt_outcome']) == ['IGNORED_MATCHED', 'TP']


def test_valid_tie_goes_to_the_lower_index():
    gt, det, ov, _ = M.case('valid_tie')
    assert ov[0][0, 0, 0] == ov[0][0, 0, 1] == 0.75
    for metric in (M2D, BEV, M3D):
        r = _run('valid_tie', metric=metric, c=PED)
        assert _names(DET, r['det_outcome']) == ['TP', 'FP_DUPLICATE']
        assert list(r['gt_partner']) == [0]


def test_dontcare_only_under_the_2d_metric():
    r = _run('dontcare_2d', metric=M2D)
    assert _names(DET, r['det_outcome']) == ['TP', 'DONTCARE']
    assert r['det_partner'][1] == 1 and r['det_overlap'][1] == 1.0
    assert M.counts(r) == (1, 0, 0)
    for metric in (BEV, M3D):
        r = _run('dontcare_2d', metric=metric)
        assert _names(DET, r['det_outcome']) == ['TP', 'FP_BACKGROUND']
        assert M.counts(r) == (1, 1, 0)


def test_harder_ground_truth():
    r = _run('harder_gt', d=EASY)
    assert _names(GT, r['gt_outcome']) == ['IGNORED_MATCHED', 'IGNORED']
    assert _names(DET, r['det_outcome']) == ['MATCHED_IGNORED']
    r = _run('harder_gt', d=MODERATE)
    assert _names(GT, r['gt_outcome']) == ['TP', 'FN_MISSED']


def test_empty_sides():
    r = _run('empty_sides')
    assert _names(GT, r['gt_outcome']) == ['FN_MISSED']
    assert _names(DET, r['det_outcome']) == ['FP_BACKGROUND']
    assert r['totals'].sum() == 2


def test_word_seams():
    r = _run('word_seams')
    last = np.cumsum([63, 64, 65]) - 1
    assert _names(DET, r['det_outcome'][last]) == ['TP'] * 3
    assert list(r['gt_partner']) == [62, 63, 64]
    assert M.counts(r) == (3, 62 + 63 + 64, 0)


def test_gt_seams():
    r = _run('gt_seams')
    at = list(M.GT_SEAMS)
    assert _names(GT, r['gt_outcome'][at]) == [
        'FN_MISSED', 'TP', 'TP', 'TP', 'FN_LOCALISATION', 'FN_LOW_SCORE']
    assert list(r['gt_partner'][at]) == [-1, 3, 1, 0, 2, 4]
    assert list(r['det_partner']) == [127, 64, 128, 63, -1]
    assert r['totals'][M.N_DET_CODES + GT['OTHER']] == 124


def test_loc_floor_edge():
    gt, det, ov, _ = M.case('loc_floor_edge')
    assert [ov[0][0, k, k] for k in range(3)] == [0.5, 0.25, 0.125]
    r = _run('loc_floor_edge', metric=M2D, c=PED,
             loc_floor=M.LOC_FLOOR_EDGE)
    # 0.5 is not > min_overlap and is <= it; 0.25 is >= loc_floor
    assert _names(DET, r['det_outcome']) == ['FP_LOCALISATION',
                                             'FP_LOCALISATION',
                                             'FP_BACKGROUND']
    assert _names(GT, r['gt_outcome']) == ['FN_LOCALISATION',
                                           'FN_LOCALISATION', 'FN_MISSED']
    assert list(r['det_overlap']) == [0.5, 0.25, 0.0]


def test_generated_reaches_most_codes():
    seen_det, seen_gt = set(), set()
    for metric, c, d in ((M2D, CAR, MODERATE), (M3D, PED, HARD),
                         (BEV, CYC, EASY)):
        r = _run('generated', metric=metric, c=c, d=d)
        seen_det |= set(_names(DET, r['det_outcome']))
        seen_gt |= set(_names(GT, r['gt_outcome']))
    assert len(seen_det) >= 8 and len(seen_gt) >= 6, (seen_det, seen_gt)


# ------------------------------------------- against the protocol statement
@pytest.mark.parametrize("name", ['generated', 'dontcare_2d', 'small_det',
                                  'small_then_valid', 'valid_tie',
                                  'word_seams', 'gt_seams', 'harder_gt'])
def test_counts_equal_the_protocols_counters_at_every_threshold(name):
    gt, det, ov, host = M.case(name)
    combos = [(m, c, d) for m in range(3) for c in range(3) for d in range(3)]
    if name == 'generated':
        combos = [(M2D, CAR, EASY), (M2D, PED, MODERATE), (BEV, CAR, HARD),
                  (BEV, CYC, MODERATE), (M3D, CAR, MODERATE), (M3D, PED, HARD)]
    checked = 0
    for m, c, d in combos:
        for t in range(host['n_thresholds'][m, c, d]):
            r = M.match_set(gt, det, ov, m, c, d,
                            host['thresholds'][m, c, d, t])
            assert M.counts(r) == tuple(host['counters'][m, c, d, t]), \
                (name, m, c, d, t)
            # both sides count the same true positives
            assert r['totals'][DET['TP']] == r['totals'][M.N_DET_CODES +
                                                         GT['TP']]
            checked += 1
    assert checked > 0


# --------------------------------------------------------- best_f1_threshold
def _eval_result(thresholds, counters, at=(2, 0, 1)):
    from pointgnn_amd import kitti_eval as E
    arrays = {key: np.zeros(shape, dtype) for key, dtype, shape in
              E._OUT_LAYOUT}
    n = len(thresholds)
    arrays['n_thresholds'][at] = n
    arrays['thresholds'][at][:n] = thresholds
    arrays['counters'][at][:n] = counters
    return E.KittiEvalResult(arrays)


def test_best_f1_threshold():
    from pointgnn_amd import kitti_eval as E
    # F1 = 2 tp / (2 tp + fp + fn): 2/7, 4/6, 6/9, 6/14: 0.8 and 0.7 tie at
    # 2/3 and the higher threshold wins
    r = _eval_result([0.9, 0.8, 0.7, 0.6],
                     [(1, 0, 5), (2, 0, 2), (3, 2, 1), (3, 8, 0)])
    assert E.best_f1_threshold(r, '3d', 'Car', 'moderate') == 0.8
    assert E.best_f1_threshold(r, 2, 0, 1) == 0.8
    assert E.best_f1_threshold(r, 'detection_3d', 'car', 'Moderate') == 0.8
    # a single maximum at the end
    r = _eval_result([0.9, 0.5], [(1, 0, 3), (4, 1, 0)])
    assert E.best_f1_threshold(r, '3d', 'Car', 1) == 0.5
    # counters past n_thresholds are not read
    r.counters[2, 0, 1, 2] = (100, 0, 0)
    assert E.best_f1_threshold(r, '3d', 'Car', 1) == 0.5
    # equal thresholds, all-zero counters
    r = _eval_result([0.4, 0.4], [(0, 0, 0), (0, 0, 0)])
    assert E.best_f1_threshold(r, '3d', 'Car', 1) == 0.4
    # another combination of the same result has no threshold
    with pytest.raises(ValueError):
        E.best_f1_threshold(r, '2d', 'Car', 1)
    with pytest.raises(ValueError):
        E.best_f1_threshold(r, '4d', 'Car', 1)
    assert E.resolve_threshold('f1', r, '2d', 'Car', 1) == 0.0
    assert E.resolve_threshold(0.25, r, '2d', 'Car', 1) == 0.25


def test_result_object_on_the_restatements_arrays():
    from pointgnn_amd import kitti_eval as E
    assert E.DET_OUTCOMES[DET['FP_CONFUSION']] == 'FP_CONFUSION'
    assert E.GT_OUTCOMES[GT['FN_MISSED']] == 'FN_MISSED'
    gt, det, ov, _ = M.case('generated')
    arrays = M.match_set(gt, det, ov, M3D, CAR, MODERATE, 0.5)
    gt_off, det_off = E.pack_labels(gt)[0], E.pack_labels(det)[0]
    res = E.KittiMatchResult(arrays, gt_off, det_off, M3D, CAR, MODERATE, 0.5,
                             0.1)
    assert (res.tp, res.fp, res.fn) == M.counts(arrays)
    assert sum(res.totals.values()) == det_off[-1] + gt_off[-1]
    for f in range(len(gt)):
        got = res.frame(f)
        want = M.match_frame(gt[f], det[f], ov[f], M3D, CAR, 1, 0.5, 0.7)
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
    with pytest.raises(IndexError):
        res.frame(len(gt))
    text = res.format()
    assert text.startswith('car detection_3d moderate at score >= 0.500000: '
                           'tp %d fp %d fn %d' % (res.tp, res.fp, res.fn))
    assert 'fp_localisation' in text and 'fn_missed' in text
    js = res.to_json()
    assert js['totals']['DET_TP'] == res.tp and js['min_overlap'] == 0.7


# ----------------------------------------------------------- argument checks
def test_match_rejects_bad_arguments_without_gpu():
    from pointgnn_amd import _lib as L
    lib = L.load()
    assert 'pgnn_kitti_match' in L.exported_symbols()
    fake = ctypes.c_void_p(256)        # never dereferenced: checks come first
    ok = np.asarray([0, 1], np.int32)
    p_ok = ctypes.c_void_p(ok.ctypes.data)

    def call(gt_off=p_ok, det_off=p_ok, n=1, boxes=(fake,) * 4, table=None,
             combo=(2, 0, 1), thresh=0.5, floor=0.1, ws=fake, ws_bytes=1 << 30,
             outs=(fake,) * 6):
        return lib.pgnn_kitti_match(gt_off, det_off, n, *boxes, table, *combo,
                                    thresh, floor, ws, ws_bytes, *outs, None)

    assert call(None, None) == -1
    assert b"kitti_match: null offsets" in lib.pgnn_last_error()
    assert call(n=-1) == -1
    bad = np.asarray([0, 3, 2], np.int32)
    p_bad = ctypes.c_void_p(bad.ctypes.data)
    assert call(p_bad, p_bad, 2) == -1
    assert b"ascending" in lib.pgnn_last_error()
    # the caps, by argument only
    big = np.asarray([0, 1025], np.int32)
    p_big = ctypes.c_void_p(big.ctypes.data)
    assert call(det_off=p_big) == L.E_UNSUPPORTED
    assert b"1025 detections" in lib.pgnn_last_error()
    assert call(gt_off=p_big) == L.E_UNSUPPORTED
    assert call(n=(1 << 24) + 1) == L.E_UNSUPPORTED
    assert call(boxes=(None,) * 4) == -1
    assert b"null box" in lib.pgnn_last_error()
    assert call(outs=(None,) * 6) == -1
    assert b"output" in lib.pgnn_last_error()
    assert call(ws=None) == -1
    for combo in ((3, 0, 0), (0, 3, 0), (0, 0, 3), (-1, 0, 0), (0, 0, -1)):
        assert call(combo=combo) == -1
        assert b"0, 1 or 2" in lib.pgnn_last_error()
    for value in (float('nan'), float('inf'), -float('inf')):
        assert call(thresh=value) == -1
        assert b"score_threshold" in lib.pgnn_last_error()
    for value in (float('nan'), float('inf'), -0.01, 1.01):
        assert call(floor=value) == -1
        assert b"loc_floor" in lib.pgnn_last_error()
    table = np.asarray([0.7, 0.5, 0.5, 0.7, 1.5, 0.5, 0.7, 0.5, 0.5])
    assert call(table=ctypes.c_void_p(table.ctypes.data)) == -1
    assert b"min_overlap[1][1]" in lib.pgnn_last_error()
    # every check passed: the workspace is what stops these
    assert call(ws_bytes=16) == L.E_WORKSPACE
    assert b"kitti_match: workspace too small" in lib.pgnn_last_error()
    assert call(floor=0.0, thresh=-1.0, ws_bytes=16) == L.E_WORKSPACE
    assert call(floor=1.0, combo=(0, 2, 2), ws_bytes=16) == L.E_WORKSPACE


def test_match_workspace_query():
    from pointgnn_amd import _lib as L
    lib = L.load()
    q = lib.pgnn_kitti_match_workspace_bytes
    assert q(0, 0, 0, 0) > 0
    assert q(-1, 0, 0, 0) == 0 and q(1, 2, 2, 5) == 0
    small, large = q(10, 100, 150, 1500), q(10, 100, 150, 3000)
    # four pair planes of float64
    assert abs(large - small - 4 * 8 * 1500) < 1024    # 256-byte alignment
    # no sort keys: smaller than the evaluation's workspace for many boxes
    assert q(3769, 40000, 66000, 700000) < \
        lib.pgnn_kitti_eval_workspace_bytes(3769, 40000, 66000, 700000)
