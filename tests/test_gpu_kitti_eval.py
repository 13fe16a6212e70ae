"""KITTI object AP on the device (pointgnn_amd.kitti_eval, csrc/kitti_eval.hip)
against the host restatement of DESIGN.md §9.5 in tests/_kitti_eval.py.

What is compared how:
  n_gt, n_thresholds, thresholds, the int64 tp / fp / fn counters   ==
  precision, recall (one float64 division of the same integers)     ==
  AP_R11, AP_R40    1e-12 (at most 40 float64 terms in [0, 1]: summation
                    orders differ by at most 40 * 2^-53)
  pair overlaps     the 2D planes ==; BEV and 3D 5e-12 absolute (see OVERLAP_TOL)
"""
import os

import numpy as np
import pytest

import pointgnn_amd  # noqa: F401
import _kitti_eval as K

pytestmark = pytest.mark.gpu

EXACT = ('n_gt', 'n_thresholds', 'thresholds', 'counters', 'precision',
         'recall')
AP_TOL = 1e-12
# BEV / 3D overlaps.  Both polygon codes end in a shoelace sum over absolute
# camera coordinates: up to 8 products of |x| <= 25 by |z| <= 78 (the
# generator's range, KITTI's), each rounded to 2^-53 relative, so either
# side's area carries up to 8 * 1950 * 2^-53 / 2 = 0.9e-12 m^2 of rounding.
# The overlap divides by a union as small as one pedestrian's footprint, 0.35
# m^2: 2.5e-12 per side, 5e-12 between the two.  1e-12 is below what float64
# gives at these coordinates.  The restatement alone, against an exact rational
# clip of the same corners, is off by 2.4e-12 (seed 11) and 2.5e-12 (seed 13),
# both on a pedestrian 50-70 m out.  Largest device - restatement difference
# measured on the committed seeds (MI355X): 1.68e-12 (seed 11), 2.98e-12
# (seed 13).
OVERLAP_TOL = 5e-12


def _device_result(gt, det):
    from pointgnn_amd import kitti_eval
    return kitti_eval.evaluate(gt, det)


def _assert_matches_host(dev, host, what):
    for key in EXACT:
        got, want = getattr(dev, key), host[key]
        assert got.shape == want.shape and got.dtype == want.dtype, (what, key)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, "%s: %s differs at %s: device %r, host %r" % (
            what, key, bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
    for key in ('ap_r11', 'ap_r40'):
        diff = np.abs(getattr(dev, key) - host[key]).max()
        print("%s: max |%s difference| = %.3g" % (what, key, diff))
        assert diff <= AP_TOL, (what, key, diff)


def _check(key, build):
    gt, det, _, host = K.with_host(key, build)
    dev = _device_result(gt, det)
    _assert_matches_host(dev, host, key)
    return dev, host


@pytest.mark.parametrize("name", sorted(K.HAND_CASES))
def test_hand_cases(name):
    dev, _ = _check(name, K.HAND_CASES[name])
    if name == 'one_car':
        assert dev.ap('2d', 'Car', 'easy', points=11) == 1.0 / 11
        assert dev.ap('3d', 'Car', 0) == 0.0
    if name == 'forty_cars':
        assert dev.ap('bev', 'Car', 'easy') == 39.0 / 40
        assert dev.ap('bev', 'Car', 'easy', points=11) == 10.0 / 11


def _empty_cases():
    car = K.easy_car()
    return {
        'gt_only': ([[car]], [[]]),
        'det_only': ([[]], [[K.detection_of(car, 0.9)]]),
        'neither': ([[]], [[]]),
        # Cars only: Pedestrian and Cyclist are absent from the whole set
        'mixed': ([[car], [], [], [K.easy_car(1)]],
                  [[], [K.detection_of(car, 0.7)], [],
                   [K.detection_of(K.easy_car(1), 0.6)]]),
    }


@pytest.mark.parametrize("name", ['gt_only', 'det_only', 'neither', 'mixed'])
def test_empty_frames_and_absent_classes(name):
    dev, host = _check('empty_' + name, lambda: _empty_cases()[name])
    # a class without ground truth: no thresholds, AP 0
    assert not dev.n_thresholds[:, 1:].any()
    assert not dev.ap_r40[:, 1:].any() and not dev.ap_r11[:, 1:].any()
    if name == 'gt_only':
        assert dev.n_gt[0, 0, 0] == 1 and dev.n_thresholds[0, 0, 0] == 0
    if name == 'mixed':
        assert dev.n_gt[0, 0, 0] == 2 and dev.n_thresholds[0, 0, 0] == 1


@pytest.mark.parametrize("seed", [11, 13])
def test_generated_frames_all_combinations(seed):
    from pointgnn_amd import kitti_eval
    gt, det, ov, host = K.generated(seed, 6)
    dev = _device_result(gt, det)
    _assert_matches_host(dev, host, "seed %d" % seed)
    # every combination has work to do somewhere in the two sets
    assert host['n_thresholds'][:, :, 2].min() > 0
    # the pair kernel alone
    got, pair_off = kitti_eval.pair_overlaps(gt, det)
    worst = 0.0
    for f in range(len(gt)):
        block = got[:, pair_off[f]:pair_off[f + 1]].reshape(ov[f].shape)
        # the 2D overlaps are the same float64 expressions on both sides
        assert np.array_equal(block[[0, 3]], ov[f][[0, 3]])
        worst = max(worst, np.abs(block - ov[f]).max())
    print("seed %d: max |overlap difference| = %.3g" % (seed, worst))
    assert worst <= OVERLAP_TOL


def test_mask_word_boundaries():
    """65 detections; 130 detections with 70 ground truths; matches at bits 63
    and 64 of the assigned mask."""
    _check('sized_65', K.case_sized(21, 30, 65))
    _check('sized_130', K.case_sized(22, 70, 130))
    dev, host = _check('bits_63_64', K.case_bits_63_64)
    # both Cars are found at the lower threshold, and the 64 strays count
    assert tuple(host['counters'][0, 0, 0, 1]) == (2, 64, 0)
    assert tuple(dev.counters[0, 0, 0, 1]) == (2, 64, 0)


def test_fewer_and_more_scores_than_sample_points():
    """n_gt = 7 (fewer than 41 recorded scores) and 300 Cars over 300 frames
    (more; 75 frame groups and all 41 thresholds in the second pass)."""
    dev, _ = _check('cars_7', K.case_cars(5, (4, 3)))
    assert dev.n_gt[0, 0, 0] == 7 and 0 < dev.n_thresholds[0, 0, 0] <= 7
    dev, _ = _check('cars_300', K.case_cars(6, (1,) * 300, 1.0))
    assert dev.n_gt[0, 0, 0] == 300 and dev.n_thresholds[0, 0, 0] == 41
    dev, _ = _check('cars_300_missed', K.case_cars(7, (1,) * 300, 0.9))
    assert 30 < dev.n_thresholds[0, 0, 0] < 41


def test_scores_scattered_over_several_sort_tiles():
    """9 frames of 1 000 ground truths: 9 000 score slots per combination
    (16 384 sorted keys: four LDS tiles and the global-memory steps), 72 of
    them filled."""
    dev, host = _check('long_lists', K.case_long_lists(8))
    assert dev.n_gt[0, 0, 0] == 72
    assert 30 < dev.n_thresholds[0, 0, 0] <= 41
    n = dev.n_thresholds[2, 0, 0]
    assert np.all(np.diff(dev.thresholds[2, 0, 0, :n]) <= 0)


def test_all_scores_equal():
    dev, host = _check('equal_scores', K.case_equal_scores)
    for idx in np.argwhere(dev.n_thresholds > 0):
        m, c, d = idx
        n = dev.n_thresholds[m, c, d]
        # the same value repeated; no detection is ever below it, so every
        # threshold sees the same counts
        assert np.all(dev.thresholds[m, c, d, :n] == 0.5)
        assert np.all(dev.counters[m, c, d, :n] == dev.counters[m, c, d, 0])


def test_above_the_cap_raises_and_writes_nothing():
    import torch
    from pointgnn_amd import _lib, kitti_eval
    car = K.easy_car()
    det = [[K.detection_of(car, 0.5) for _ in range(kitti_eval.MAX_DET + 1)]]
    out = torch.full((kitti_eval.output_bytes(),), 0xAB, dtype=torch.uint8,
                     device='cuda')
    with pytest.raises(_lib.PointGnnHipError, match="1025 detections"):
        kitti_eval.run_packed(kitti_eval.pack_labels([[car]]),
                              kitti_eval.pack_labels(det), out=out)
    torch.cuda.synchronize()
    assert bool((out == 0xAB).all())
    # at the cap it runs: 1 024 detections on one Car, one true positive
    res = kitti_eval.evaluate([[car]], [det[0][:kitti_eval.MAX_DET]])
    assert tuple(res.counters[0, 0, 0, 0]) == (1, 1023, 0)
    assert tuple(res.counters[2, 0, 0, 0]) == (1, 1023, 0)


def test_runs_are_bit_identical_also_on_another_stream():
    import torch
    from pointgnn_amd import kitti_eval
    gt, det, _, _ = K.generated(13, 6)
    packed = kitti_eval.pack_labels(gt), kitti_eval.pack_labels(det)
    first = kitti_eval.run_packed(*packed).cpu()
    second = kitti_eval.run_packed(*packed).cpu()
    assert torch.equal(first, second)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        third = kitti_eval.run_packed(*packed)
        stream.synchronize()
    assert torch.equal(first, third.cpu())


def test_evaluate_dirs_and_report(tmp_path, capsys):
    """Files written by kitti_output.write_kitti_txt from the detect oracle's
    synthetic detections -> evaluate_dirs == evaluate on the parsed labels;
    the report and the command line print the numbers of .ap()."""
    from oracle import detect_oracle as DO, ingest_oracle as IO
    from pointgnn_amd import kitti_dataset, kitti_eval, kitti_output
    calib = kitti_dataset.parse_calib(IO.CALIB_LINES)
    label_dir, result_dir = str(tmp_path / 'label_2'), str(tmp_path / 'data')
    methods = ('Car', 'Pedestrian_and_Cyclist', 'Car')
    for f, method in enumerate(methods):
        labels, boxes, scores = DO.synthetic_detections(
            f, n_objects=6, votes=(2, 6), noise_boxes=6, half_width=8.0,
            depth=(8.0, 40.0))
        rows = DO.kitti_labels(labels, boxes.astype(np.float64), scores,
                               calib['cam_to_image'], method, None,
                               use_box_score=False)
        kitti_output.write_kitti_txt(
            os.path.join(result_dir, '%06d.txt' % f), rows)
        # every third detection, without its score, stands in as ground truth
        kitti_output.write_kitti_txt(
            os.path.join(label_dir, '%06d.txt' % f),
            [r[:1] + (0.0, 0) + r[3:15] for r in rows[::3]])
    # a labelled frame without a result file
    kitti_output.write_kitti_txt(os.path.join(label_dir, '000003.txt'),
                                 [('Car', 0.0, 0, 0, 100.0, 100.0, 200.0,
                                   180.0, 1.5, 1.6, 3.9, 0.0, 1.6, 20.0, 0.1)])
    names, gt, det = kitti_eval.read_dirs(label_dir, result_dir)
    assert names == ['000000', '000001', '000002', '000003'] and det[3] == []
    assert sum(len(d) for d in det) > 20
    from_dirs = kitti_eval.evaluate_dirs(label_dir, result_dir)
    direct = kitti_eval.evaluate(gt, det)
    for key in EXACT + ('ap_r11', 'ap_r40'):
        assert np.array_equal(getattr(from_dirs, key), getattr(direct, key))
    assert direct.n_thresholds[:, 0].min() > 0       # Cars were scored
    # the nine report lines, R40 first, with the numbers of .ap()
    lines = from_dirs.format().split('\n')
    assert len(lines) == 18
    k = 0
    for cls in ('car', 'pedestrian', 'cyclist'):
        for m, rep in enumerate(('detection', 'detection_ground',
                                 'detection_3d')):
            want = '%s_%s AP: %s' % (cls, rep, ' '.join(
                '%.6f' % (100 * from_dirs.ap(m, cls, d)) for d in range(3)))
            assert lines[k] == want
            assert lines[9 + k].startswith('%s_%s_R11 AP: ' % (cls, rep))
            assert lines[9 + k].split()[2] == '%.6f' % (
                100 * from_dirs.ap(m, cls, 'easy', points=11))
            k += 1
    assert from_dirs.format(alongside=False) == '\n'.join(lines[:9])
    # a split file restricts the frame set; --json adds one line
    split = tmp_path / 'val.txt'
    split.write_text('000000\n000002\n')
    assert kitti_eval.main([label_dir, result_dir, '--split', str(split),
                            '--json']) == 0
    printed = capsys.readouterr().out.strip().split('\n')
    subset = kitti_eval.evaluate_dirs(label_dir, result_dir,
                                      ['000000', '000002'])
    assert printed[:18] == subset.format().split('\n')
    import json
    assert json.loads(printed[18])['car_detection_3d_R40'] == [
        100 * subset.ap('3d', 'Car', d) for d in range(3)]
