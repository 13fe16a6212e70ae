"""KITTI object AP without a GPU: the host restatement of DESIGN.md §9.5
against answers derived by hand, the txt round trip of `evaluate_dirs`, and
the argument checks of the new C entries (which run before any HIP call)."""
import ctypes
import os

import numpy as np
import pytest

import _kitti_eval as K

CAR, PED = 0, 1
EASY, MODERATE, HARD = 0, 1, 2


def _host(name):
    return K.with_host(name, K.HAND_CASES[name])[3]


def test_one_car_one_perfect_detection():
    # n_gt = 1, one recorded score v = [0.9].  i = 0 is the last index, so it
    # is appended: one threshold.  At it tp = 1, fp = fn = 0: precision[0] =
    # 1, every later entry 0, and the running maximum changes nothing.
    # AP_R11 = (p[0] + p[4] + ... + p[40]) / 11 = 1/11;
    # AP_R40 = (p[1] + ... + p[40]) / 40 = 0.
    r = _host('one_car')
    for m in range(3):
        for d in range(3):
            assert r['n_gt'][m, CAR, d] == 1
            assert r['n_thresholds'][m, CAR, d] == 1
            assert r['thresholds'][m, CAR, d, 0] == 0.9
            assert tuple(r['counters'][m, CAR, d, 0]) == (1, 0, 0)
            assert r['precision'][m, CAR, d, 0] == 1.0
            assert not r['precision'][m, CAR, d, 1:].any()
            assert r['ap_r11'][m, CAR, d] == 1.0 / 11
            assert r['ap_r40'][m, CAR, d] == 0.0
    # no Pedestrian or Cyclist anywhere: no thresholds, AP 0
    assert not r['n_thresholds'][:, 1:].any() and not r['ap_r40'][:, 1:].any()


def test_forty_cars_distinct_scores():
    # n_gt = 40 and 40 recorded scores.  With current_recall = i/40 (up to
    # rounding) before step i, l = (i+1)/40 and r = (i+2)/40, so r -
    # current_recall ~ 2/40 is never below current_recall - l ~ -1/40: every
    # score is a threshold, 40 of them.  At the k-th threshold the k + 1 best
    # detections are kept, all true positives: precision 1 at t = 0..39 and 0
    # at t = 40.  AP_R40 = 39/40; AP_R11 reads t = 0, 4, .., 36 (ten ones)
    # and t = 40 (zero): 10/11.
    r = _host('forty_cars')
    for m in range(3):
        assert r['n_gt'][m, CAR, EASY] == 40
        assert r['n_thresholds'][m, CAR, EASY] == 40
        assert np.array_equal(r['precision'][m, CAR, EASY],
                              [1.0] * 40 + [0.0])
        assert np.array_equal(r['counters'][m, CAR, EASY, :40, 0],
                              np.arange(1, 41))
        assert np.array_equal(r['counters'][m, CAR, EASY, :40, 2],
                              np.arange(39, -1, -1))
        assert r['ap_r40'][m, CAR, EASY] == 39.0 / 40
        assert r['ap_r11'][m, CAR, EASY] == 10.0 / 11


def test_van_under_a_car_detection_is_neither_tp_nor_fp():
    # The Van is a neighbouring class of Car: ignored_gt = 1.  n_gt = 1 (the
    # Car), v = [0.9], one threshold 0.9.  There the Car's detection is a tp;
    # the Car detection on the Van (score 0.95, kept) is matched to the Van
    # and only marked assigned: fp = 0.  Were the Van not there, fp = 1.
    r = _host('van')
    for m in range(3):
        assert r['n_gt'][m, CAR, EASY] == 1
        assert tuple(r['counters'][m, CAR, EASY, 0]) == (1, 0, 0)
        assert r['precision'][m, CAR, EASY, 0] == 1.0


def test_false_positive_in_dontcare_region():
    # One Car with its detection (0.9) and a stray Car detection (0.95) whose
    # 2D box lies wholly inside the DontCare region: inter / area_det = 1 >
    # 0.7.  2D: fp = 1 - nstuff = 0.  BEV and 3D have no DontCare step, and
    # the stray box is 20 m from the Car: fp = 1, precision 1/2.
    r = _host('dontcare')
    assert tuple(r['counters'][0, CAR, EASY, 0]) == (1, 0, 0)
    assert tuple(r['counters'][1, CAR, EASY, 0]) == (1, 1, 0)
    assert tuple(r['counters'][2, CAR, EASY, 0]) == (1, 1, 0)
    assert r['precision'][0, CAR, EASY, 0] == 1.0
    assert r['precision'][1, CAR, EASY, 0] == 0.5


def test_low_detection_on_a_ground_truth():
    # Moderate: both Cars count (heights 60 and 30 > 25), n_gt = 2.  The
    # detection on the second Car is 24 px high: ignored_det = 1.  2D IoU of
    # (100 x 24) inside (100 x 30) = 2400 / 3000 = 0.8 > 0.7.  Pass 1 matches
    # it but records nothing (ignored_det of the match is 1): v = [0.5], one
    # threshold.  At 0.5: first Car tp; second Car takes the low detection by
    # rule (c) and is only marked assigned: no tp, no fn; the low detection is
    # no fp (ignored).  (tp, fp, fn) = (1, 0, 0).
    r = _host('low_detection')
    for m in range(3):
        assert r['n_gt'][m, CAR, MODERATE] == 2
        assert r['n_thresholds'][m, CAR, MODERATE] == 1
        assert tuple(r['counters'][m, CAR, MODERATE, 0]) == (1, 0, 0)
        # easy: the 30 px Car is ignored (30 <= 40): n_gt = 1, same counts
        assert r['n_gt'][m, CAR, EASY] == 1
        assert tuple(r['counters'][m, CAR, EASY, 0]) == (1, 0, 0)


def test_exact_ties():
    # Pedestrians, moderate (MIN_HEIGHT 25, MIN_OVERLAP 0.5).
    #  A (40 px) with a detection of 2D IoU 400/800 = 0.5 exactly, score 0.8;
    #  B (30 px) with a detection 25 px high, IoU 500/600, score 0.7: the
    #    detection is NOT ignored (25 < 25 is false);
    #  C (25 px) with a perfect detection, 0.65: C IS ignored (25 <= 25).
    # n_gt = 2.  2D: A finds nothing (0.5 > 0.5 is false), B records 0.7, C's
    # match is only assigned: one threshold 0.7, where tp = 1 (B), fn = 1 (A),
    # fp = 1 (A's detection; C's is below the threshold).
    # BEV / 3D: A's detection has A's 3D box: v = [0.8, 0.7], two thresholds;
    # at 0.8 (1, 0, 1), at 0.7 (2, 0, 0).
    r = _host('exact_ties')
    assert r['n_gt'][0, PED, MODERATE] == 2
    assert r['n_thresholds'][0, PED, MODERATE] == 1
    assert r['thresholds'][0, PED, MODERATE, 0] == 0.7
    assert tuple(r['counters'][0, PED, MODERATE, 0]) == (1, 1, 1)
    for m in (1, 2):
        assert r['n_thresholds'][m, PED, MODERATE] == 2
        assert tuple(r['counters'][m, PED, MODERATE, 0]) == (1, 0, 1)
        assert tuple(r['counters'][m, PED, MODERATE, 1]) == (2, 0, 0)


def test_generator_seeds_pass_the_rotated_overlap_gate():
    """The committed seeds of the GPU file: the gate is asserted inside."""
    gt, det, ov, _ = K.generated(11, 6)
    assert len(gt) == 6 and sum(len(d) for d in det) > 40
    names = {g['name'] for f in gt for g in f}
    assert {'Car', 'Pedestrian', 'Cyclist', 'DontCare'} <= names
    scores = [a['score'] for f in det for a in f]
    assert len(set(scores)) < len(scores)              # exact ties


def test_txt_round_trip(tmp_path):
    """write_kitti_txt -> the parsing of evaluate_dirs gives the labels
    back, and a missing or empty result file has no detections."""
    from pointgnn_amd import kitti_eval, kitti_output
    gt, det, _, _ = K.generated(11, 6)
    keys = ('name', 'truncation', 'occlusion', 'alpha', 'xmin', 'ymin',
            'xmax', 'ymax', 'height', 'width', 'length', 'x3d', 'y3d', 'z3d',
            'yaw')
    names = ['%06d' % f for f in range(len(gt) + 2)]
    for f in range(len(gt)):
        kitti_output.write_kitti_txt(
            str(tmp_path / 'label' / (names[f] + '.txt')),
            [tuple(g[k] for k in keys) for g in gt[f]])
        kitti_output.write_kitti_txt(
            str(tmp_path / 'result' / (names[f] + '.txt')),
            [tuple(a[k] for k in keys + ('score',)) for a in det[f]])
    # two more frames: one with an empty result file, one with none
    for f in (len(gt), len(gt) + 1):
        kitti_output.write_kitti_txt(
            str(tmp_path / 'label' / (names[f] + '.txt')), [])
    kitti_output.write_kitti_txt(
        str(tmp_path / 'result' / (names[len(gt)] + '.txt')), [])
    got_names, got_gt, got_det = kitti_eval.read_dirs(
        str(tmp_path / 'label'), str(tmp_path / 'result'))
    assert got_names == names
    assert got_gt[:len(gt)] == gt and got_det[:len(gt)] == det
    assert got_gt[len(gt):] == [[], []] and got_det[len(gt):] == [[], []]
    # the packed form keeps every number
    off, rows, codes = kitti_eval.pack_labels(det)
    assert off[-1] == sum(len(d) for d in det) and rows.shape[1] == 14
    first = det[0][0]
    assert rows[0, 13] == first['score'] and rows[0, 10] == first['yaw']
    assert kitti_eval.name_code('PERSON_SITTING') == 4
    assert kitti_eval.name_code('Tram') == 6


def _lib():
    from pointgnn_amd import _lib as L
    return L, L.load()


def _offsets(values):
    a = np.asarray(values, np.int32)
    return a, ctypes.c_void_p(a.ctypes.data)


def test_entries_reject_bad_arguments_without_gpu():
    L, lib = _lib()
    eight = [None] * 8
    fake = ctypes.c_void_p(256)        # never dereferenced: checks come first
    ok, p_ok = _offsets([0, 1])
    # null pointers
    assert lib.pgnn_kitti_eval(None, None, 1, None, None, None, None, None,
                               0, *eight, None) == -1
    assert b"kitti_eval" in lib.pgnn_last_error()
    assert lib.pgnn_kitti_eval(p_ok, p_ok, 1, None, None, None, None, fake,
                               1 << 20, *([fake] * 8), None) == -1
    assert b"null" in lib.pgnn_last_error()
    assert lib.pgnn_kitti_eval(p_ok, p_ok, 1, fake, fake, fake, fake, fake,
                               1 << 20, *eight, None) == -1
    # negative count
    assert lib.pgnn_kitti_eval(p_ok, p_ok, -1, fake, fake, fake, fake, fake,
                               1 << 20, *([fake] * 8), None) == -1
    assert b"n_frames" in lib.pgnn_last_error()
    # offsets not ascending / not starting at 0
    bad, p_bad = _offsets([0, 3, 2])
    assert lib.pgnn_kitti_eval(p_bad, p_bad, 2, fake, fake, fake, fake, fake,
                               1 << 20, *([fake] * 8), None) == -1
    assert b"ascending" in lib.pgnn_last_error()
    one, p_one = _offsets([1, 2])
    assert lib.pgnn_kitti_eval(p_one, p_ok, 1, fake, fake, fake, fake, fake,
                               1 << 20, *([fake] * 8), None) == -1
    # workspace too small
    assert lib.pgnn_kitti_eval(p_ok, p_ok, 1, fake, fake, fake, fake, fake,
                               16, *([fake] * 8), None) == L.E_WORKSPACE
    # above the caps: unsupported, with the frame in the message
    big, p_big = _offsets([0, 1025])
    assert lib.pgnn_kitti_eval(p_ok, p_big, 1, fake, fake, fake, fake, fake,
                               1 << 30, *([fake] * 8), None) == L.E_UNSUPPORTED
    assert b"1025 detections" in lib.pgnn_last_error()
    # the pair entry checks the same way
    assert lib.pgnn_kitti_pair_overlaps(None, None, 1, None, None, None, None,
                                        0, None, None) == -1
    assert lib.pgnn_kitti_pair_overlaps(p_bad, p_bad, 2, fake, fake, fake,
                                        fake, 1 << 20, fake, None) == -1
    assert lib.pgnn_kitti_pair_overlaps(p_ok, p_big, 1, fake, fake, fake,
                                        fake, 1 << 30, fake,
                                        None) == L.E_UNSUPPORTED
    with pytest.raises(L.PointGnnHipError):
        L.check(L.E_UNSUPPORTED, "pgnn_kitti_eval")


def test_workspace_query():
    _, lib = _lib()
    q = lib.pgnn_kitti_eval_workspace_bytes
    base = q(10, 100, 150, 1500)
    assert base > 0
    assert q(1000, 100, 150, 1500) > base          # frames: offset tables
    assert q(10, 5000, 150, 1500) > base           # ground truths: score slots
    assert q(10, 100, 50000, 1500) > base          # detections: flags
    assert q(10, 100, 150, 15000) > base           # pairs: overlap planes
    assert q(10, 100, 150, 15000) - base >= 4 * 8 * (15000 - 1500) - 1024
    assert q(0, 0, 0, 0) > 0
    for bad in ((-1, 0, 0, 0), (1, -1, 0, 0), (1, 0, -1, 0), (1, 0, 0, -1),
                (1, 2, 3, 7)):                     # more pairs than n_gt*n_det
        assert q(*bad) == 0
