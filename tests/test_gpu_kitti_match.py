"""Per-box outcomes of the KITTI matching on the device (pgnn_kitti_match,
pointgnn_amd.kitti_eval.match) against the host restatement
in tests/_kitti_match.py.

The restatement is fed the device's own pair overlaps (kitti_eval.
pair_overlaps), so only decisions are compared, and everything is compared
with ==: the outcome codes, the partners, the overlaps (copies of table
entries) and the totals."""
import json
import os

import numpy as np
import pytest

import pointgnn_amd  # noqa: F401
import _kitti_eval as K
import _kitti_match as M
import _render as RR

pytestmark = pytest.mark.gpu

KEYS = ('det_outcome', 'det_partner', 'det_overlap', 'gt_outcome',
        'gt_partner')
ALL_COMBOS = [(m, c, d) for m in range(3) for c in range(3) for d in range(3)]
_OVERLAPS = {}


def device_overlaps(name):
    """The frames' [4, ng, nd] tables as the device computes them, once."""
    if name not in _OVERLAPS:
        from pointgnn_amd import kitti_eval
        gt, det = M.case(name)[:2]
        flat, pair_off = kitti_eval.pair_overlaps(gt, det)
        _OVERLAPS[name] = [
            flat[:, pair_off[f]:pair_off[f + 1]].reshape(4, len(g), len(a))
            for f, (g, a) in enumerate(zip(gt, det))]
    return _OVERLAPS[name]


def assert_same(res, want, what):
    for key in KEYS:
        got = getattr(res, key)
        assert got.dtype == want[key].dtype and got.shape == want[key].shape, \
            (what, key)
        bad = np.argwhere(got != want[key])
        assert len(bad) == 0, "%s: %s differs at %s: device %r, host %r" % (
            what, key, bad[0], got[tuple(bad[0])], want[key][tuple(bad[0])])
    totals = [res.totals['DET_' + n] for n in sorted(M.DET, key=M.DET.get)] + \
        [res.totals['GT_' + n] for n in sorted(M.GT, key=M.GT.get)]
    assert totals == list(want['totals']), what
    assert (res.tp, res.fp, res.fn) == M.counts(want), what


@pytest.mark.parametrize("name", M.SMALL_CASES)
def test_small_cases_all_combinations(name):
    from pointgnn_amd import kitti_eval
    gt, det = M.case(name)[:2]
    ov = device_overlaps(name)
    floor = M.LOC_FLOOR_EDGE if name == 'loc_floor_edge' else 0.1
    seen = set()
    for m, c, d in ALL_COMBOS:
        res = kitti_eval.match(gt, det, m, c, d, score_threshold=M.THRESHOLD,
                               loc_floor=floor)
        want = M.match_set(gt, det, ov, m, c, d, M.THRESHOLD, loc_floor=floor)
        assert_same(res, want, (name, m, c, d))
        seen |= {k for k, n in res.totals.items() if n}
    # the case reaches the code it is named for, on the device
    reaches = {'duplicate': 'DET_FP_DUPLICATE',
               'localisation': 'DET_FP_LOCALISATION',
               'confusion': 'DET_FP_CONFUSION',
               'background': 'DET_FP_BACKGROUND', 'low_score': 'GT_FN_LOW_SCORE',
               'fn_localisation': 'GT_FN_LOCALISATION',
               'missed': 'GT_FN_MISSED', 'small_det': 'GT_MATCHED_SMALL',
               'small_then_valid': 'DET_IGNORED_SMALL',
               'valid_tie': 'DET_FP_DUPLICATE', 'dontcare_2d': 'DET_DONTCARE',
               'harder_gt': 'GT_IGNORED_MATCHED', 'empty_sides': 'GT_FN_MISSED',
               'word_seams': 'DET_TP', 'gt_seams': 'GT_FN_LOW_SCORE',
               'loc_floor_edge': 'GT_FN_LOCALISATION'}
    assert reaches[name] in seen, (name, sorted(seen))


def test_named_boxes_on_the_device():
    from pointgnn_amd import kitti_eval as E
    gt, det = M.case('valid_tie')[:2]
    res = E.match(gt, det, '2d', 'Pedestrian', 'moderate', score_threshold=0.5)
    assert list(res.det_outcome) == [M.DET['TP'], M.DET['FP_DUPLICATE']]
    assert list(res.det_overlap) == [0.75, 0.75] and list(res.gt_partner) == [0]
    gt, det = M.case('small_then_valid')[:2]
    res = E.match(gt, det, '3d', 'Car', 'moderate', score_threshold=0.5)
    assert list(res.gt_partner) == [1, 2]
    gt, det = M.case('low_score')[:2]
    res = E.match(gt, det, '3d', 'Car', 'moderate', score_threshold=0.5)
    assert list(res.det_outcome) == [M.DET['BELOW'], M.DET['TP']]
    assert list(res.gt_outcome) == [M.GT['FN_LOW_SCORE'], M.GT['TP']]
    gt, det = M.case('word_seams')[:2]
    res = E.match(gt, det, '3d', 'Car', 'moderate', score_threshold=0.5)
    assert list(res.gt_partner) == [62, 63, 64]
    d_out, d_par, d_ov, g_out, g_par = res.frame(2)
    assert len(d_out) == 65 and d_out[64] == M.DET['TP'] and d_par[64] == 0
    gt, det = M.case('gt_seams')[:2]
    res = E.match(gt, det, '3d', 'Car', 'moderate', score_threshold=0.5)
    assert list(res.gt_partner[list(M.GT_SEAMS)]) == [-1, 3, 1, 0, 2, 4]
    assert list(res.det_partner) == [127, 64, 128, 63, -1]
    gt, det = M.case('loc_floor_edge')[:2]
    res = E.match(gt, det, '2d', 'Pedestrian', 'moderate', score_threshold=0.5,
                  loc_floor=M.LOC_FLOOR_EDGE)
    assert list(res.det_overlap) == [0.5, 0.25, 0.0]
    assert list(res.gt_outcome) == [M.GT['FN_LOCALISATION']] * 2 + \
        [M.GT['FN_MISSED']]


@pytest.mark.parametrize("combo", [(0, 0, 1), (1, 2, 0), (2, 1, 2)])
def test_generated(combo):
    from pointgnn_amd import kitti_eval
    gt, det = M.case('generated')[:2]
    ov = device_overlaps('generated')
    for thresh, floor in ((0.5, 0.1), (0.0, 0.0), (0.85, 1.0)):
        res = kitti_eval.match(gt, det, *combo, score_threshold=thresh,
                               loc_floor=floor)
        assert_same(res, M.match_set(gt, det, ov, *combo, thresh,
                                     loc_floor=floor), (combo, thresh))


def test_loose_table():
    from pointgnn_amd import kitti_eval
    gt, det = M.case('generated')[:2]
    ov = device_overlaps('generated')
    moved = 0
    for combo in ((1, 0, 1), (2, 1, 2), (2, 2, 0), (0, 0, 1)):
        res = kitti_eval.match(gt, det, *combo, score_threshold=0.5,
                               min_overlap='loose')
        assert_same(res, M.match_set(gt, det, ov, *combo, 0.5,
                                     min_overlap=M.LOOSE), combo)
        official = kitti_eval.match(gt, det, *combo, score_threshold=0.5)
        differs = not np.array_equal(res.det_outcome, official.det_outcome)
        if combo[0] == 0:       # the loose table leaves the 2D metric alone
            assert not differs
        moved += differs
    assert moved > 0
    assert res.min_overlap[1, 1] == 0.25


def test_counts_are_the_evaluations_counters_at_every_threshold():
    from pointgnn_amd import kitti_eval
    gt, det = M.case('generated')[:2]
    ev = kitti_eval.evaluate(gt, det)
    checked = 0
    for m, c, d in ALL_COMBOS:
        for t in range(ev.n_thresholds[m, c, d]):
            res = kitti_eval.match(gt, det, m, c, d,
                                   score_threshold=ev.thresholds[m, c, d, t])
            assert (res.tp, res.fp, res.fn) == \
                tuple(ev.counters[m, c, d, t]), (m, c, d, t)
            assert res.totals['DET_TP'] == res.tp
            checked += 1
    assert checked == ev.n_thresholds.sum() and checked > 27
    # the threshold of the best F1 is one of the stored ones
    best = kitti_eval.best_f1_threshold(ev, '3d', 'Car', 'moderate')
    assert best in ev.thresholds[2, 0, 1, :ev.n_thresholds[2, 0, 1]]


def test_caps_are_refused_before_anything_is_launched():
    from pointgnn_amd import _lib as L, kitti_eval
    car = K.easy_car(0)
    many = [K.detection_of(car, 0.9)] * (kitti_eval.MAX_DET + 1)
    with pytest.raises(L.PointGnnHipError) as err:
        kitti_eval.match([[car]], [many])
    assert "1025 detections" in str(err.value)
    with pytest.raises(L.PointGnnHipError):
        kitti_eval.match([[car] * (kitti_eval.MAX_GT + 1)],
                         [[K.detection_of(car, 0.9)]])
    with pytest.raises(ValueError):
        kitti_eval.match([[car]], [[], []])
    with pytest.raises(ValueError):
        kitti_eval.match([[car]], [[]], metric='4d')


def test_two_streams_give_equal_bytes():
    import torch
    from pointgnn_amd import kitti_eval
    gt, det = M.case('generated')[:2]
    packed = kitti_eval.pack_labels(gt), kitti_eval.pack_labels(det)
    outs = []
    for _ in range(2):
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            out = kitti_eval.run_match_packed(*packed, 2, 0, 1, 0.5)
        stream.synchronize()
        outs.append({k: t.cpu().numpy().tobytes() for k, t in out.items()})
    torch.cuda.synchronize()
    assert outs[0] == outs[1]
    again = kitti_eval.run_match_packed(*packed, 2, 0, 1, 0.5)
    assert {k: t.cpu().numpy().tobytes() for k, t in again.items()} == outs[0]


# ------------------------------------------------------------------ renderer
def _frame_rows():
    """Labels and detections of one frame in front of the camera whose
    matching (3D, Car, hard, threshold 0.5) has a true positive, a
    localisation error, a background box, an ignored one, one under the
    threshold and boxes of other classes."""
    gt, _ = RR.frame_labels(0)
    for g in gt:
        g['ymax'] = g['ymin'] + 45.0           # above every height limit
    car, ped, dontcare, van = gt
    hit = dict(car, score=0.9)
    near = dict(car, score=0.8, x3d=car['x3d'] + 1.0, z3d=car['z3d'] + 1.0)
    far = dict(car, score=0.7, x3d=-car['x3d'], z3d=car['z3d'] + 12.0,
               xmin=80.0, xmax=120.0)
    on_van = dict(van, name='Car', score=0.6)
    low = dict(car, score=0.1, z3d=car['z3d'] + 20.0)
    walker = dict(ped, score=0.95)
    return gt, [near, hit, far, on_van, low, walker]


@pytest.fixture(scope="module")
def kitti(tmp_path_factory):
    from pointgnn_amd import kitti_dataset as KD, synthetic as S
    root = str(tmp_path_factory.mktemp("match_kitti"))
    S.write_kitti_frames(root, [0], preset="small", behind_points=2000)
    label_dir, result_dir = (os.path.join(root, d) for d in
                             ("label_2", "results"))
    os.makedirs(label_dir)
    os.makedirs(result_dir)
    gt, det = _frame_rows()
    RR.write_label_file(os.path.join(label_dir, "000000.txt"), gt)
    RR.write_label_file(os.path.join(result_dir, "000000.txt"), det)
    ds = KD.KittiDataset(*(os.path.join(root, d) for d in
                           ("image_2", "velodyne", "calib")),
                         label_dir=label_dir)
    return root, ds, label_dir, result_dir, gt, det


def _composition(ds, view_name, gt, gt_colors, det, det_colors, rect_colors):
    """tests/test_gpu_render.py's frame_reference with the colours given."""
    from pointgnn_amd import render as R
    pts = ds.get_cam_points_in_image_with_rgb(0)
    xyz = pts.xyz.cpu().numpy().astype(np.float64)
    col = RR.colorize(pts.attr[:, 0].cpu().numpy(), 0.0, 1.0, R.GRAY_TABLE)
    segs = [R.label_segments(gt), R.label_segments(det)]
    cols = [np.repeat(np.asarray(gt_colors, np.uint8).reshape(-1, 3), 12, 0),
            np.repeat(np.asarray(det_colors, np.uint8).reshape(-1, 3), 12, 0)]
    if view_name == 'bev':
        v = RR.bev_view((-40, 40), (0, 80), 10.0)
    else:
        h, w = ds._image_shape(0)
        v = RR.view(ds.get_calib(0)['cam_to_image'], (0, 0, 1, 0), 0.1, w, h)
    img = RR.render(v, points=xyz, point_colors=col,
                    segments=np.concatenate(segs),
                    segment_colors=np.concatenate(cols))
    if view_name == 'camera' and det:
        img = RR.render(RR.view([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1]],
                                (0, 0, 0, 0), 0.5, v.width, v.height),
                        segments=R.rect_segments(det),
                        segment_colors=np.repeat(np.asarray(
                            rect_colors, np.uint8).reshape(-1, 3), 4, 0),
                        thickness=2, background=img)
    return img


@pytest.mark.parametrize("view_name", ["bev", "camera"])
def test_render_frame_with_outcomes(kitti, view_name):
    from pointgnn_amd import kitti_eval, render as R
    root, ds, label_dir, result_dir, gt, det = kitti
    res = kitti_eval.match([gt], [det], '3d', 'Car', 'hard',
                           score_threshold=0.5)
    det_tags = R.outcome_tags('det', res.det_outcome)
    gt_tags = R.outcome_tags('gt', res.gt_outcome)
    assert det_tags[1] == 'TP' and det_tags[3] == 'IGN' and \
        det_tags[4] == 'LOW' and det_tags[5] is None, det_tags
    assert det_tags[0] == 'LOC' and det_tags[2] == 'BG', det_tags
    assert gt_tags == ['TP', None, None, 'IGN'], gt_tags
    for show_below in (False, True):
        keep = [j for j, t in enumerate(det_tags)
                if t is not None and (t != 'LOW' or show_below)]
        dcols = [R.OUTCOME_COLORS[det_tags[j]] for j in keep]
        want = _composition(
            ds, view_name, [gt[0], gt[3]],
            [R.OUTCOME_COLORS['TP'], R.OUTCOME_COLORS['IGN']],
            [det[j] for j in keep], dcols, dcols)
        got = R.render_frame(ds, 0, det, gt, view=view_name,
                             outcomes=res.frame(0), show_below=show_below)
        assert np.array_equal(got.cpu().numpy(), want), (view_name, show_below)
        flat = want.reshape(-1, 3)
        for tag in ('TP', 'BG', 'IGN'):
            assert np.any(np.all(flat == np.array(R.OUTCOME_COLORS[tag],
                                                  np.uint8), axis=1)), tag
    # without outcomes: the picture of before, in the old colours
    shown = [g for g in gt if g['name'] in R.GT_COLORS]
    want = _composition(ds, view_name, shown,
                        [R.GT_COLORS[g['name']] for g in shown], det,
                        [(255, 0, 0)] * len(det), [(0, 255, 0)] * len(det))
    for kw in ({}, {'outcomes': None}):
        got = R.render_frame(ds, 0, det, gt, view=view_name, **kw)
        assert np.array_equal(got.cpu().numpy(), want), view_name
    # the strings
    drawn = R.frame_outcomes(det, gt, res.frame(0), show_below=True)
    assert drawn['det_strings'][1] == 'TP 1.00'
    assert drawn['det_strings'][2] == 'BG 0.70'
    assert drawn['det_strings'][4] == 'LOW 0.10'
    assert drawn['det_strings'][0] == 'LOC 0.42'
    assert drawn['gt_strings'] == ['TP 1.00', 'IGN 1.00']
    plain = R.render_frame(ds, 0, det, gt, view=view_name,
                           outcomes=res.frame(0)).cpu().numpy()
    texted = R.render_frame(ds, 0, det, gt, view=view_name,
                            outcomes=res.frame(0), text=True).cpu().numpy()
    changed = np.any(plain != texted, axis=2)
    assert changed.any()
    # text only adds pixels of the outcome colours
    allowed = {tuple(R.OUTCOME_COLORS[t]) for t in ('TP', 'BG', 'IGN', 'LOC')}
    assert {tuple(p) for p in texted[changed]} <= allowed
    with pytest.raises(ValueError):
        R.render_frame(ds, 0, det[:2], gt, view=view_name,
                       outcomes=res.frame(0))


def test_render_results_with_errors(kitti, tmp_path):
    from pointgnn_amd import kitti_eval, render as R
    root, ds, label_dir, result_dir, gt, det = kitti
    plain = R.render_results(ds, result_dir, str(tmp_path / "a"), fmt='ppm')
    again = R.render_results(ds, result_dir, str(tmp_path / "b"), fmt='ppm',
                             errors=None)
    assert open(plain[0], 'rb').read() == open(again[0], 'rb').read()
    errs = R.render_results(ds, result_dir, str(tmp_path / "c"), fmt='ppm',
                            errors={'difficulty': 'hard',
                                    'score_threshold': 0.5})
    res = kitti_eval.match([gt], [det], '3d', 'Car', 'hard',
                           score_threshold=0.5)
    want = R.render_frame(ds, 0, det, gt, outcomes=res.frame(0)).cpu().numpy()
    assert np.array_equal(RR.decode_ppm(open(errs[0], 'rb').read()), want)
    # 'f1' (the default): the threshold of the one true positive, 0.9
    f1 = R.render_results(ds, result_dir, str(tmp_path / "d"), fmt='ppm',
                          errors={'difficulty': 'hard'}, show_below=True)
    res = kitti_eval.match([gt], [det], '3d', 'Car', 'hard',
                           score_threshold=0.9)
    want = R.render_frame(ds, 0, det, gt, outcomes=res.frame(0),
                          show_below=True).cpu().numpy()
    assert np.array_equal(RR.decode_ppm(open(f1[0], 'rb').read()), want)
    assert R.main([root, result_dir, str(tmp_path / "e"), '--ppm', '--errors',
                   '--error-difficulty', 'hard', '--at-threshold', '0.5']) == 0
    assert open(os.path.join(str(tmp_path / "e"), 'bev', '000000.ppm'),
                'rb').read() == open(errs[0], 'rb').read()


# -------------------------------------------------------------- command line
def test_command_line_with_errors(tmp_path, capsys):
    from pointgnn_amd import kitti_eval
    gt, det = M.case('generated')[:2]
    label_dir, result_dir = str(tmp_path / "label"), str(tmp_path / "result")
    os.makedirs(label_dir)
    os.makedirs(result_dir)
    for f in range(3):
        RR.write_label_file(os.path.join(label_dir, "%06d.txt" % f), gt[f])
        RR.write_label_file(os.path.join(result_dir, "%06d.txt" % f), det[f])
    assert kitti_eval.main([label_dir, result_dir, '--json']) == 0
    before = capsys.readouterr().out
    assert kitti_eval.main([label_dir, result_dir, '--json', '--errors',
                            '--error-metric', '2d', '--at-threshold',
                            '0.5']) == 0
    after = capsys.readouterr().out
    report, js = before.rstrip('\n').rsplit('\n', 1)
    assert 'errors' not in before
    assert after.startswith(report + '\n')
    res = kitti_eval.match_dirs(label_dir, result_dir, metric='2d',
                                score_threshold=0.5)
    assert res.frame_names == ['000000', '000001', '000002']
    direct = kitti_eval.match(gt[:3], det[:3], '2d', 'Car', 'moderate',
                              score_threshold=0.5)
    assert res.totals == direct.totals and res.tp + res.fp + res.fn > 0
    table, js_after = after[len(report) + 1:].rstrip('\n').rsplit('\n', 1)
    assert table == res.format()
    js, js_after = json.loads(js), json.loads(js_after)
    assert js_after.pop('errors') == res.to_json()
    assert js_after == js
    # 'f1' is the default: the threshold comes from the evaluation
    assert kitti_eval.main([label_dir, result_dir, '--errors']) == 0
    out = capsys.readouterr().out
    ev = kitti_eval.evaluate_dirs(label_dir, result_dir)
    best = kitti_eval.best_f1_threshold(ev, '3d', 'Car', 'moderate')
    assert 'car detection_3d moderate at score >= %.6f' % best in out
