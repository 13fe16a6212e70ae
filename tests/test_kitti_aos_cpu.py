"""Orientation similarity (AOS) and overlap tables of the KITTI evaluation
without a GPU: the host restatement of DESIGN.md §9.5's additions against
tests/_kitti_eval.py and answers derived by hand, the alpha written by
kitti_output, the packing and parsing helpers of pointgnn_amd.kitti_eval and
the argument checks of the new C entries (which run before any HIP call)."""
import ctypes
import math
import os

import numpy as np
import pytest

import _kitti_eval as K
import _kitti_aos as A

CAR, PED = 0, 1
EASY = 0
KEYS = ('precision', 'recall', 'counters', 'thresholds', 'n_thresholds',
        'n_gt', 'ap_r11', 'ap_r40')


def _same(got, want, what):
    for key in KEYS:
        assert got[key].dtype == want[key].dtype, (what, key)
        assert np.array_equal(got[key], want[key]), (what, key)


@pytest.mark.parametrize("name", sorted(K.HAND_CASES))
def test_official_table_without_alphas_is_the_restatement_hand(name):
    gt, det, ov, host = K.with_host(name, K.HAND_CASES[name])
    _same(A.evaluate_host_ex(gt, det, ov), host, name)
    _same(A.evaluate_host_ex(gt, det, ov, A.OFFICIAL), host, name)


@pytest.mark.parametrize("seed", [11, 13])
def test_official_table_without_alphas_is_the_restatement_generated(seed):
    gt, det, ov, host = K.generated(seed, 6)
    A.assert_gate(ov, A.LOOSE)          # bounds 0.25, 0.5, 0.7
    got = A.evaluate_host_ex(gt, det, ov)
    _same(got, host, seed)
    # orientation decides nothing: the same arrays with alphas
    with_aos = A.evaluate_host_ex(gt, det, ov, None, A.random_alphas(gt, 1),
                                  A.random_alphas(det, 2))
    _same(with_aos, host, seed)
    assert with_aos['similarity'][:, 2].max() > 1.0
    # the loose table moves BEV / 3D counters and leaves the 2D metric alone
    loose = A.evaluate_host_ex(gt, det, ov, A.LOOSE)
    for key in KEYS:
        assert np.array_equal(loose[key][0], host[key][0]), key
    assert not np.array_equal(loose['counters'][1:], host['counters'][1:])


def test_one_car_delta_zero_and_a_quarter_turn():
    # One Car, one perfect detection (K.case_one_car): one threshold, tp = 1,
    # fp = 0.  delta = 0: the term is (1 + cos 0) / 2 = 1.0 exactly, so
    # similarity[0] = 1, orientation = [1, 0, 0, ...] = precision and AOS = AP
    # (1/11 and 0).
    gt, det = K.case_one_car()
    r = A.evaluate_host_ex(gt, det, None, None, [[0.3]], [[0.3]])
    for d in range(3):
        assert r['similarity'][CAR, d, 0] == 1.0
        assert np.array_equal(r['orientation'][CAR, d],
                              r['precision'][0, CAR, d])
        assert r['aos_r11'][CAR, d] == r['ap_r11'][0, CAR, d] == 1.0 / 11
        assert r['aos_r40'][CAR, d] == r['ap_r40'][0, CAR, d] == 0.0
    assert not r['similarity'][1:].any() and not r['orientation'][1:].any()
    # delta = pi/2: cos is 6.1e-17, not 0, and 1 + that rounds to 1: 0.5
    r = A.evaluate_host_ex(gt, det, None, None, [[math.pi / 2]], [[0.0]])
    assert abs(r['similarity'][CAR, EASY, 0] - 0.5) <= 2.0 ** -52
    assert abs(r['aos_r11'][CAR, EASY] - 0.5 / 11) <= 2.0 ** -52
    # delta = pi: the box faces the other way, similarity 0
    r = A.evaluate_host_ex(gt, det, None, None, [[math.pi]], [[0.0]])
    assert r['similarity'][CAR, EASY, 0] == 0.0
    assert r['aos_r11'][CAR, EASY] == 0.0


def test_false_positives_add_nothing():
    # The Car's detection (0.9, delta 0) and a stray Car detection (0.95) on
    # no ground truth: one threshold 0.9 with tp = 1, fp = 1.  The stray's
    # alpha (2.0) enters nowhere: similarity 1, orientation 1 / (1 + 1) =
    # 0.5 = precision.  A stray Pedestrian detection: that class has no
    # ground truth, no thresholds, and its orientation is 0 throughout.
    car = K.easy_car(0)
    stray = K.label('Car', (520.0, 120.0, 600.0, 180.0), xyz=(10.0, 1.6, 40.0),
                    score=0.95)
    ped = K.label('Pedestrian', (820.0, 120.0, 850.0, 190.0),
                  K._SIZES['Pedestrian'], (15.0, 1.6, 30.0), score=0.9)
    gt, det = [[car]], [[K.detection_of(car, 0.9), stray, ped]]
    r = A.evaluate_host_ex(gt, det, None, None, [[0.1]], [[0.1, 2.0, 1.0]])
    assert tuple(r['counters'][0, CAR, EASY, 0]) == (1, 1, 0)
    assert r['similarity'][CAR, EASY, 0] == 1.0
    assert r['orientation'][CAR, EASY, 0] == 0.5
    assert r['aos_r11'][CAR, EASY] == 0.5 / 11
    assert r['n_thresholds'][0, PED, EASY] == 0
    assert not r['orientation'][PED].any() and not r['aos_r11'][PED].any()


def test_all_half_table_on_the_exact_tie():
    # K.case_exact_ties under a table of 0.5 everywhere: Pedestrians already
    # use 0.5, so that class is what it was; the tie at exactly 0.5 still
    # fails `>`.
    gt, det, ov, host = K.with_host('exact_ties', K.case_exact_ties)
    r = A.evaluate_host_ex(gt, det, ov, A.HALF)
    for key in KEYS:
        assert np.array_equal(r[key][:, PED], host[key][:, PED]), key
    assert tuple(r['counters'][0, PED, 1, 0]) == (1, 1, 1)


# ------------------------------------------------------------ written alpha
def _synthetic_rows(write_alpha, boxes=None):
    from oracle import detect_oracle as DO, ingest_oracle as IO
    from pointgnn_amd import kitti_dataset, kitti_output
    calib = kitti_dataset.parse_calib(IO.CALIB_LINES)
    labels, synth, scores = DO.synthetic_detections(
        0, n_objects=6, votes=(2, 6), noise_boxes=6, half_width=8.0,
        depth=(8.0, 40.0))
    if boxes is None:
        boxes = synth
    n = len(boxes)
    return boxes, kitti_output.detections_to_kitti_labels(
        np.asarray(labels[:n]), np.asarray(boxes), np.asarray(scores[:n]),
        calib, 'Car', use_box_score=False, host_only=True,
        write_alpha=write_alpha)


def test_write_alpha_is_the_formula_and_touches_nothing_else():
    boxes, plain = _synthetic_rows(False)
    _, rows = _synthetic_rows(True)
    assert len(rows) == len(plain) > 5
    for row, ref in zip(rows, plain):
        assert len(row) == 16 and ref[3] == 0
        assert row[:3] == ref[:3] and row[4:] == ref[4:]
        x3d, z3d, yaw = row[11], row[13], row[14]
        a = float(np.float64(yaw) - np.arctan2(np.float64(x3d),
                                               np.float64(z3d)))
        while a > math.pi:
            a -= 2 * math.pi
        while a < -math.pi:
            a += 2 * math.pi
        assert type(row[3]) is float and row[3] == a
        assert -math.pi <= row[3] <= math.pi


def test_write_alpha_wraps_and_survives_the_txt(tmp_path):
    from pointgnn_amd import kitti_dataset, kitti_output
    # (x, y, z, l, h, w, yaw) in front of the camera: atan2(-2, 20) = -0.0997,
    # so yaw 3.1 gives 3.1997 > pi -> minus a turn; yaw -3.1 with x = +2
    # gives -3.1997 < -pi -> plus a turn
    boxes = np.array([[-2.0, 1.6, 20.0, 3.9, 1.5, 1.6, 3.1],
                      [2.0, 1.6, 20.0, 3.9, 1.5, 1.6, -3.1],
                      [1.0, 1.6, 15.0, 3.9, 1.5, 1.6, 0.4]], np.float32)
    _, rows = _synthetic_rows(True, boxes)
    assert len(rows) == 3
    raw = [float(np.float64(b[6]) - np.arctan2(np.float64(b[0]),
                                               np.float64(b[2])))
           for b in boxes]
    assert raw[0] > math.pi and raw[1] < -math.pi
    assert rows[0][3] == raw[0] - 2 * math.pi
    assert rows[1][3] == raw[1] + 2 * math.pi
    assert rows[2][3] == raw[2]
    path = str(tmp_path / 'data' / '000000.txt')
    kitti_output.write_kitti_txt(path, rows)
    back = kitti_dataset.read_label_file(path)
    assert [lab['alpha'] for lab in back] == [row[3] for row in rows]
    # what `det_alpha='box'` computes from the same file differs from the
    # written alpha by whole turns only -- up to the text of the file: the
    # float32 box fields are written by their shortest repr, which read back
    # as float64 is within half a float32 ulp (6e-8 relative, of 3.1 and 20)
    # of the float64 the alpha was computed from
    from pointgnn_amd import kitti_eval
    _, packed, _ = kitti_eval.pack_labels([back])
    from_box = kitti_eval.alpha_from_box(packed)
    turns = (from_box - kitti_eval.pack_alpha([back])) / (2 * math.pi)
    assert np.allclose(turns, np.round(turns), rtol=0, atol=1e-7)
    assert list(np.round(turns)) == [1.0, -1.0, 0.0]


# ------------------------------------------------------------------ helpers
def test_pack_alpha_alpha_from_box_and_the_minus_ten_rule():
    from pointgnn_amd import kitti_eval
    gt, det, _, _ = K.generated(11, 6)
    det = A.with_alphas(det, A.random_alphas(det, 3))
    alpha = kitti_eval.pack_alpha(det)
    off, rows, _ = kitti_eval.pack_labels(det)
    assert alpha.dtype == np.float64 and alpha.shape == (off[-1],)
    assert alpha[off[1]] == det[1][0]['alpha']
    assert kitti_eval.pack_alpha([[], []]).shape == (0,)
    box = kitti_eval.alpha_from_box(rows)
    first = det[0][0]
    assert box[0] == first['yaw'] - math.atan2(first['x3d'], first['z3d'])
    assert box.shape == alpha.shape
    # the source of the detections' alpha
    assert np.array_equal(kitti_eval.detection_alpha(det, rows, 'file'), alpha)
    assert np.array_equal(kitti_eval.detection_alpha(det, rows, 'box'), box)
    with pytest.raises(ValueError):
        kitti_eval.detection_alpha(det, rows, 'label')
    # one detection written without an alpha: AOS is not computed
    det[2][1]['alpha'] = -10.0
    assert kitti_eval.detection_alpha(det, rows, 'file') is None
    assert kitti_eval.detection_alpha(det, rows, 'box') is not None


def test_min_overlap_tables():
    from pointgnn_amd import kitti_eval as E
    assert E.OFFICIAL_MIN_OVERLAP == A.OFFICIAL
    assert E.LOOSE_MIN_OVERLAP == A.LOOSE
    official = np.array(A.OFFICIAL)
    for value in (None, 'official', 'OFFICIAL', A.OFFICIAL,
                  '0.7,0.5,0.5,0.7,0.5,0.5,0.7,0.5,0.5'):
        got = E.min_overlap_table(value)
        assert got.dtype == np.float64 and got.flags['C_CONTIGUOUS']
        assert np.array_equal(got, official)
    assert np.array_equal(E.min_overlap_table('loose'), np.array(A.LOOSE))
    assert np.array_equal(E.min_overlap_table(list(range(9))),
                          np.arange(9.0).reshape(3, 3))
    for bad in ('strict', '0.5,0.5', [[0.5] * 3] * 2, 0.5):
        with pytest.raises(ValueError):
            E.min_overlap_table(bad)


def test_command_line_arguments():
    from pointgnn_amd import kitti_eval as E
    args = E.parse_args(['labels', 'results'])
    assert (args.aos, args.alpha_from_box, args.min_overlap, args.json) == \
        (False, False, None, False)
    args = E.parse_args(['labels', 'results', '--aos', '--alpha-from-box',
                         '--min-overlap', 'loose', '--json'])
    assert args.aos and args.alpha_from_box and args.json
    assert np.array_equal(args.min_overlap, np.array(A.LOOSE))
    args = E.parse_args(['l', 'r', '--min-overlap',
                         '0.7,0.5,0.5,0.5,0.3,0.3,0.5,0.25,0.25'])
    assert args.min_overlap[1, 1] == 0.3 and args.min_overlap[2, 2] == 0.25
    with pytest.raises(SystemExit):
        E.parse_args(['l', 'r', '--min-overlap', 'tight'])


def _hand_arrays():
    from pointgnn_amd import kitti_eval as E
    rng = np.random.default_rng(5)
    arrays = {}
    for key, dtype, shape in E._OUT_LAYOUT:
        arrays[key] = (rng.random(shape) * 40).astype(dtype)
    arrays['ap_r11'] = rng.random((3, 3, 3))
    arrays['ap_r40'] = rng.random((3, 3, 3))
    return arrays


def test_report_without_aos_is_todays_text():
    from pointgnn_amd import kitti_eval as E
    arrays = _hand_arrays()
    res = E.KittiEvalResult(arrays, ('Cyclist', 'Car'))
    assert res.has_aos is False
    assert np.isnan(res.aos_r40).all() and np.isnan(res.similarity).all()
    assert res.orientation.shape == (3, 3, 41) and res.aos_r11.shape == (3, 3)
    assert np.isnan(res.aos('Car', 'easy'))
    assert np.array_equal(res.min_overlap, np.array(A.OFFICIAL))
    # the text of the report as it was before orientation existed
    want, as_json = [], {}
    for table, suffix in ((arrays['ap_r40'], ''), (arrays['ap_r11'], '_R11')):
        for cls, c in (('cyclist', 2), ('car', 0)):
            for m, rep in enumerate(('detection', 'detection_ground',
                                     'detection_3d')):
                want.append('%s_%s%s AP: %s' % (cls, rep, suffix, ' '.join(
                    '%.6f' % (100.0 * float(table[m, c, d]))
                    for d in range(3))))
    assert res.format() == '\n'.join(want)
    assert sorted(res.to_json()) == sorted(
        '%s_%s_R%d' % (cls, rep, pts) for cls in ('cyclist', 'car')
        for rep in ('detection', 'detection_ground', 'detection_3d')
        for pts in (11, 40))
    assert res.to_json()['car_detection_3d_R40'] == [
        100.0 * float(arrays['ap_r40'][2, 0, d]) for d in range(3)]


def test_report_with_aos():
    from pointgnn_amd import kitti_eval as E
    arrays = _hand_arrays()
    rng = np.random.default_rng(6)
    for key, dtype, shape in E._AOS_LAYOUT:
        arrays[key] = rng.random(shape)
    res = E.KittiEvalResult(arrays, has_aos=True, min_overlap='loose')
    assert np.array_equal(res.min_overlap, np.array(A.LOOSE))
    assert res.aos('Pedestrian', 'hard') == arrays['aos_r40'][1, 2]
    assert res.aos(2, 0, points=11) == arrays['aos_r11'][2, 0]
    lines = res.format().split('\n')
    assert len(lines) == 24
    # the official tool's order: detection, orientation, ground, 3d
    assert [l.split(' ')[0] for l in lines[:4]] == [
        'car_detection', 'car_orientation', 'car_detection_ground',
        'car_detection_3d']
    assert lines[1] == 'car_orientation AOS: ' + ' '.join(
        '%.6f' % (100.0 * arrays['aos_r40'][0, d]) for d in range(3))
    assert lines[12 + 5] == 'pedestrian_orientation_R11 AOS: ' + ' '.join(
        '%.6f' % (100.0 * arrays['aos_r11'][1, d]) for d in range(3))
    without = E.KittiEvalResult(arrays).format().split('\n')
    assert [l for l in lines if ' AOS: ' not in l] == without
    js = res.to_json()
    assert js['cyclist_orientation_R40'] == [
        100.0 * arrays['aos_r40'][2, d] for d in range(3)]
    assert 'car_orientation_R11' in js and len(js) == 24


# --------------------------------------------------------- argument checks
def _lib():
    from pointgnn_amd import _lib as L
    return L, L.load()


def _offsets(values):
    a = np.asarray(values, np.int32)
    return a, ctypes.c_void_p(a.ctypes.data)


def _table(values):
    a = np.asarray(values, np.float64)
    return a, ctypes.c_void_p(a.ctypes.data)


def test_new_entries_are_declared_and_exported():
    import re
    L, lib = _lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "pointgnn_hip.h")).read()
    for name in ('pgnn_kitti_eval_ex_workspace_bytes', 'pgnn_kitti_eval_ex',
                 'pgnn_kitti_pair_orientation'):
        assert re.search(r"\b%s\(" % name, header)
        assert name in L.exported_symbols() and hasattr(lib, name)
    assert 'define PGNN_KITTI_ROW 14' in header


def test_eval_ex_rejects_bad_arguments_without_gpu():
    L, lib = _lib()
    fake = ctypes.c_void_p(256)        # never dereferenced: checks come first
    ok, p_ok = _offsets([0, 1])
    boxes = [fake] * 4                 # gt rows, gt names, det rows, det names
    outs = [fake] * 8
    aos_outs = [fake] * 4

    def call(gt_off=p_ok, det_off=p_ok, n=1, boxes=boxes, ws=fake,
             ws_bytes=1 << 30, outs=outs, alphas=(None, None), table=None,
             aos_outs=aos_outs):
        return lib.pgnn_kitti_eval_ex(gt_off, det_off, n, *boxes, ws, ws_bytes,
                                      *outs, *alphas, table, *aos_outs, None)

    # offsets, as the existing entry checks them
    assert call(None, None) == -1
    assert b"kitti_eval_ex: null offsets" in lib.pgnn_last_error()
    assert call(n=-1) == -1
    assert b"n_frames" in lib.pgnn_last_error()
    bad, p_bad = _offsets([0, 3, 2])
    assert call(p_bad, p_bad, 2) == -1
    assert b"ascending" in lib.pgnn_last_error()
    one, p_one = _offsets([1, 2])
    assert call(p_one) == -1
    assert b"start at 0" in lib.pgnn_last_error()
    big, p_big = _offsets([0, 1025])
    assert call(det_off=p_big) == L.E_UNSUPPORTED
    assert b"1025 detections" in lib.pgnn_last_error()
    # null boxes / outputs
    assert call(boxes=[None] * 4) == -1
    assert b"null box" in lib.pgnn_last_error()
    assert call(outs=[None] * 8) == -1
    assert b"output" in lib.pgnn_last_error()
    # exactly one alpha
    assert call(alphas=(fake, None)) == -1
    assert b"both" in lib.pgnn_last_error()
    assert call(alphas=(None, fake)) == -1
    assert b"both" in lib.pgnn_last_error()
    # both alphas but no place for the orientation
    assert call(alphas=(fake, fake), aos_outs=[None] * 4) == -1
    assert b"orientation output" in lib.pgnn_last_error()
    assert call(alphas=(fake, fake), aos_outs=[fake, fake, fake, None]) == -1
    # table entries out of range, not finite
    for entry in (1.5, -0.1, float('nan'), float('inf')):
        values = [0.7, 0.5, 0.5] * 3
        values[4] = entry
        keep, p_table = _table(values)
        assert call(table=p_table) == -1
        assert b"min_overlap[1][1]" in lib.pgnn_last_error()
    # every check passed: the workspace is what stops these two (a table at
    # the ends of the range; no alphas and no orientation outputs)
    keep, p_table = _table([0.0, 1.0, 0.5] * 3)
    assert call(table=p_table, ws_bytes=16) == L.E_WORKSPACE
    assert call(aos_outs=[None] * 4, ws_bytes=16) == L.E_WORKSPACE
    assert call(alphas=(fake, fake), ws_bytes=16) == L.E_WORKSPACE
    assert b"workspace too small" in lib.pgnn_last_error()


def test_pair_orientation_rejects_bad_arguments_without_gpu():
    L, lib = _lib()
    fake = ctypes.c_void_p(256)
    ok, p_ok = _offsets([0, 1])
    f = lib.pgnn_kitti_pair_orientation
    assert f(None, None, 1, None, None, None, None, None, 0, None, None) == -1
    assert b"kitti_pair_orientation" in lib.pgnn_last_error()
    # a missing alpha, a missing output
    assert f(p_ok, p_ok, 1, fake, fake, None, fake, fake, 1 << 20, fake,
             None) == -1
    assert b"null pointer" in lib.pgnn_last_error()
    assert f(p_ok, p_ok, 1, fake, fake, fake, None, fake, 1 << 20, fake,
             None) == -1
    assert f(p_ok, p_ok, 1, fake, fake, fake, fake, fake, 1 << 20, None,
             None) == -1
    bad, p_bad = _offsets([0, 3, 2])
    assert f(p_bad, p_bad, 2, fake, fake, fake, fake, fake, 1 << 20, fake,
             None) == -1
    assert b"ascending" in lib.pgnn_last_error()
    big, p_big = _offsets([0, 1025])
    assert f(p_ok, p_big, 1, fake, fake, fake, fake, fake, 1 << 30, fake,
             None) == L.E_UNSUPPORTED
    assert f(p_ok, p_ok, 1, fake, fake, fake, fake, fake, 16, fake,
             None) == L.E_WORKSPACE


def test_ex_workspace_query():
    _, lib = _lib()
    q, old = lib.pgnn_kitti_eval_ex_workspace_bytes, \
        lib.pgnn_kitti_eval_workspace_bytes
    for sizes in ((10, 100, 150, 1500), (0, 0, 0, 0), (3769, 40000, 66000,
                                                       700000)):
        assert q(*sizes, 0) == old(*sizes) > 0
    # the fifth pair plane and [9][waves][41] doubles, waves = 4 per group of
    # four frames, at most 1 024
    plane = 8 * 1500
    assert 0 <= q(10, 100, 150, 1500, 1) - q(10, 100, 150, 1500, 0) - plane \
        - 9 * 12 * 41 * 8 < 1024
    grown = q(5000, 100, 150, 1500, 1) - q(5000, 100, 150, 1500, 0)
    assert 0 <= grown - plane - 9 * 1024 * 41 * 8 < 1024
    assert q(10 ** 6, 100, 150, 1500, 1) - q(10 ** 6, 100, 150, 1500, 0) == grown
    for bad in ((-1, 0, 0, 0), (1, -1, 0, 0), (1, 2, 3, 7)):
        assert q(*bad, 1) == 0
