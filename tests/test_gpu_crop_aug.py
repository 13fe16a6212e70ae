"""crop_aug object pasting (pointgnn_amd.crop_aug, the kernel
pgnn_crop_aug_place) against fixtures written by the reference's own
models/crop_aug.py with NumPy's RNG seeded
(tests/golden/make_golden_crop_aug.py imports CASES, DB, scene() and
run_case() from this file, so the test and the fixture cannot drift apart).

Bars, those of test_gpu_aug_registry.py: the same random decisions (NumPy's
global RNG ends in the same state), identical label names, label values to
1e-13, the same number of points, points within 1 float32 ulp of the
reference's after finish(), attribute rows bit-identical and in the same
order, the caller's tensors untouched, the caller's label list appended in
place.  The generator asserts that no point of any box test lies within 1e-9 of
a box face, no integer corner coordinate within 1e-9 of a truncation boundary
and no overlap within 1e-9 of the threshold, so a last-bit difference of a
float64 value cannot change a decision: a count mismatch is a defect.  It also
asserts that the branches the cases are named for are taken."""
import copy
import json
import os

import numpy as np
import pytest

from oracle import labels_oracle as LO

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLD, "crop_aug.npz")
DB_FILE = os.path.join(GOLD, "crop_aug_db.json")
LABEL_KEYS = ('x3d', 'y3d', 'z3d', 'yaw', 'length', 'height', 'width')
K_POINTS, N_BOXES = 5000, 18

# the object database: save_cropped_boxes over these scenes
DB = dict(seeds=(100, 101, 102, 103), k=5000, expand_factor=[1.1, 1.1, 1.1],
          minimum_points=3, backlist=['Van', 'Truck', 'Person_sitting'])

_GROUND = dict(overlap_mode='box_and_point', auto_box_height=True,
               max_overlap_rate=1e-6, appr_factor=100,
               max_overlap_num_allowed=50, expand_factor=(1.1, 1.1, 1.1))
# name: seed, scene variant, points, sample_rate, parser_kwargs; `truncate`:
# parser_without_collision directly, on Car samples cut to that many points
CASES = {
    # one trial each: some objects land on a label or on one another
    "box_one_trial": dict(
        seed=30, variant=None, k=K_POINTS,
        sample_rate={"Car": 8, "Pedestrian": 3, "Cyclist": 3},
        parser_kwargs=dict(overlap_mode='box', max_trails=1,
                           method_name='normal', yaw_std=0.3)),
    # a yaw that hardly moves the object: one that collides fails all trials
    "box_trials": dict(
        seed=31, variant=None, k=K_POINTS,
        sample_rate={"Car": 10, "Pedestrian": 3, "Cyclist": 3},
        parser_kwargs=dict(overlap_mode='box', max_trails=3,
                           method_name='normal', yaw_std=0.05,
                           max_overlap_rate=0.01, appr_factor=100)),
    # objects may overlap: a later one swallows points an earlier one brought
    "point": dict(
        seed=81, variant=None, k=K_POINTS,
        sample_rate={"Car": 12, "Cyclist": 2},
        parser_kwargs=dict(overlap_mode='point', max_trails=2,
                           max_overlap_num_allowed=60, method_name='normal',
                           yaw_std=0.1, expand_factor=(1.2, 1.1, 1.1))),
    # the reference's own example (crop_aug.py:216-229), fewer trials
    "ground_required": dict(
        seed=33, variant=None, k=K_POINTS,
        sample_rate={"Car": 6, "Pedestrian": 3, "Cyclist": 3},
        parser_kwargs=dict(_GROUND, max_trails=3, method_name='normal',
                           yaw_std=0.3, must_have_ground=True)),
    # far turns leave the scene: no ground there, y3d_adjust = 0
    "ground_optional_uniform": dict(
        seed=34, variant=None, k=K_POINTS,
        sample_rate={"Car": 6, "Pedestrian": 2, "Cyclist": 2},
        parser_kwargs=dict(_GROUND, max_trails=2, method_name='uniform',
                           yaw_std=0.7, must_have_ground=False)),
    # every label DontCare: the box test still sees them
    "dontcare_scene": dict(
        seed=35, variant="dontcare", k=K_POINTS,
        sample_rate={"Car": 8, "Pedestrian": 2, "Cyclist": 2},
        parser_kwargs=dict(overlap_mode='box', max_trails=2,
                           method_name='normal', yaw_std=0.2)),
    "tiny_cloud": dict(
        seed=36, variant=None, k=37,
        sample_rate={"Car": 3, "Pedestrian": 1, "Cyclist": 1},
        parser_kwargs=dict(_GROUND, max_trails=2, method_name='normal',
                           yaw_std=0.3, must_have_ground=False)),
    "one_point_sample": dict(
        seed=37, variant=None, k=K_POINTS, truncate=(1, 2, None, 1),
        parser_kwargs=dict(overlap_mode='box', max_trails=3,
                           method_name='uniform', yaw_std=0.4)),
}


def scene(seed, variant=None, k=K_POINTS):
    """test_gpu_aug_registry.py's scene."""
    xyz = LO.synthetic_vertices(seed, k=k)
    labels = LO.synthetic_labels(seed, xyz, n_boxes=N_BOXES)
    attr = np.random.default_rng(seed).uniform(0, 1, (len(xyz), 1)
                                               ).astype(np.float32)
    for label in labels:
        if variant == "dontcare":
            label['name'] = 'DontCare'
    return xyz, attr, labels


class SceneDataset(object):
    """The three members save_cropped_boxes uses, over DB's scenes; `wrap`
    turns (xyz, attr) into the Points of the module under test."""

    def __init__(self, wrap):
        self.num_files = len(DB["seeds"])
        self._wrap = wrap

    def get_label(self, frame_idx):
        return scene(DB["seeds"][frame_idx], None, DB["k"])[2]

    def get_cam_points_in_image_with_rgb(self, frame_idx):
        xyz, attr, _ = scene(DB["seeds"][frame_idx], None, DB["k"])
        return self._wrap(xyz, attr)


def run_case(mod, sampler, case, points, labels):
    """One case through `mod` (the reference's models.crop_aug or
    pointgnn_amd.crop_aug) -> (Points, labels).  The caller has seeded
    NumPy."""
    if "truncate" not in case:
        return sampler.crop_aug(
            points, labels, sample_rate=copy.deepcopy(case["sample_rate"]),
            parser_kwargs=copy.deepcopy(case["parser_kwargs"]))
    cut = case["truncate"]
    idx = np.random.choice(len(sampler._cropped_labels["Car"]), size=len(cut),
                           replace=False)
    s_labels = copy.deepcopy([sampler._cropped_labels["Car"][i] for i in idx])
    s_points = []
    for i, n in zip(idx, cut):
        p = sampler._cropped_cam_points["Car"][i]
        s_points.append(mod.Points(xyz=np.array(p.xyz[:n]),
                                   attr=np.array(p.attr[:n])))
    return mod.parser_without_collision(points, labels, s_points, s_labels,
                                        **copy.deepcopy(case["parser_kwargs"]))


_FIX = {}
_SAMPLER = []


def _fixture():
    if not _FIX:
        with np.load(FIXTURE) as f:
            _FIX.update({k: f[k] for k in f.files})
    return _FIX


def _sampler():
    from pointgnn_amd import crop_aug as CA
    if not _SAMPLER:
        _SAMPLER.append(CA.CropAugSampler(DB_FILE))
    return _SAMPLER[0]


def _label_array(labs):
    return np.array([[l[k] for k in LABEL_KEYS] for l in labs],
                    np.float64).reshape(len(labs), len(LABEL_KEYS))


def _ulp(got, ref):
    return np.abs(got.astype(np.float64) - ref) / np.spacing(
        np.maximum(np.abs(got), np.abs(ref)))


def _device_points(xyz, attr):
    import torch
    from pointgnn_amd.kitti_dataset import Points
    return Points(xyz=torch.from_numpy(xyz).cuda(),
                  attr=torch.from_numpy(attr).cuda())


@pytest.mark.parametrize("name", list(CASES))
def test_cases_match_reference_fixture(name, monkeypatch):
    import torch
    from pointgnn_amd import crop_aug as CA, preprocess as PP
    fix = _fixture()
    case = CASES[name]
    pre = name + "_"
    xyz, attr, labels = scene(case["seed"], case["variant"],
                              int(fix[pre + "k_points"]))
    pts = _device_points(xyz, attr)
    given_xyz, given_attr = pts.xyz, pts.attr
    sampler = _sampler()
    db_xyz, db_attr = sampler._cropped_cam_points.xyz.clone(), \
        sampler._cropped_cam_points.attr.clone()
    seen = {}
    real_place = CA.place

    def recording_place(xyz, sample_xyz, offsets, boxes, *args):
        out = real_place(xyz, sample_xyz, offsets, boxes, *args)
        seen["record"] = out[2].cpu().numpy()
        seen["boxes"], seen["max_trails"] = np.array(boxes), args[2]
        return out
    monkeypatch.setattr(CA, "place", recording_place)
    labs_in = copy.deepcopy(labels)
    np.random.seed(case["seed"])
    out, labs = run_case(CA, sampler, case, pts, labs_in)
    assert labs is labs_in                           # appended in place
    assert out.xyz.dtype == torch.float64 and out.attr.dtype == torch.float32
    out = PP.finish(out)
    assert np.random.uniform() == float(fix[pre + "rng_after"])   # same draws
    # per sample: accepted, trials used, y3d_adjust
    rec, boxes = seen["record"], seen["boxes"]
    n_s = len(boxes)
    accepted = rec[0:3 * n_s:3] != 0
    trials, start = [], 0
    for i in range(n_s):
        used = int(rec[3 * i + 1]) - start + 1 if accepted[i] \
            else seen["max_trails"]
        trials.append(used)
        start += used
    assert start == int(rec[-2])
    ground = rec[2:3 * n_s:3]
    adjust = np.where(np.isnan(ground), 0.0, ground - boxes[:, 1])
    print(name, "accepted", accepted.astype(int), "trials", trials)
    assert np.array_equal(accepted, fix[pre + "accepted"] != 0)
    assert np.array_equal(trials, fix[pre + "trials"])
    np.testing.assert_allclose(adjust[accepted],
                               fix[pre + "y3d_adjust"][accepted],
                               rtol=1e-13, atol=1e-13)
    assert [l['name'] for l in labs] == [str(s) for s in fix[pre + "names"]]
    assert len(labs) == len(labels) + int(accepted.sum())
    np.testing.assert_allclose(_label_array(labs), fix[pre + "labels"],
                               rtol=1e-13, atol=1e-13)
    got, ref = out.xyz.cpu().numpy(), fix[pre + "xyz"]
    got_attr = out.attr.cpu().numpy()
    print(name, "points", len(xyz), "->", got.shape[0], "reference",
          ref.shape[0])
    assert got.shape == ref.shape
    assert got.shape[0] == int(rec[-1])
    assert got_attr.shape == fix[pre + "attr"].shape
    assert np.array_equal(got_attr, fix[pre + "attr"])
    ulp = _ulp(got, ref)
    print(name, "identical %.5f, max %.2f ulp" % (np.mean(ulp == 0),
                                                  ulp.max()))
    assert ulp.max() <= 1.0
    # inputs untouched: the caller's tensors and the resident database
    assert np.array_equal(given_xyz.cpu().numpy(), xyz)
    assert np.array_equal(given_attr.cpu().numpy(), attr)
    assert given_xyz.dtype == torch.float32
    assert torch.equal(sampler._cropped_cam_points.xyz, db_xyz)
    assert torch.equal(sampler._cropped_cam_points.attr, db_attr)


def test_load_cropped_boxes_keeps_the_objects_on_the_device():
    import torch
    from pointgnn_amd import crop_aug as CA
    fix = _fixture()
    with open(DB_FILE) as f:
        file_labels, file_points = json.load(f)
    labels, points = CA.load_cropped_boxes(DB_FILE)
    assert labels == file_labels
    assert list(points) == list(file_points) == list(labels)
    counts = {k: len(v) for k, v in points.items()}
    assert counts == dict(zip([str(s) for s in fix["db_names"]],
                              [int(c) for c in fix["db_counts"]]))
    assert points.xyz.dtype == torch.float64 and points.xyz.is_cuda
    assert points.attr.dtype == torch.float32 and points.attr.is_cuda
    d_xyz, d_attr = points.xyz.cpu().numpy(), points.attr.cpu().numpy()
    rows = 0
    for key in file_points:
        for i, (xyz, attr) in enumerate(file_points[key]):
            a, b = points.offsets[(key, i)]
            assert a == rows and b - a == len(xyz) > DB["minimum_points"]
            rows = b
            assert np.array_equal(d_xyz[a:b], np.array(xyz))
            assert np.array_equal(d_attr[a:b],
                                  np.array(attr).astype(np.float32))
            assert np.array_equal(d_attr[a:b].astype(np.float64),
                                  np.array(attr))          # float32 values
            assert np.array_equal(points[key][i].xyz, np.array(xyz))
            view = points.device_points(key, i)
            assert view.xyz.data_ptr() == points.xyz[a:b].data_ptr()
    assert rows == d_xyz.shape[0] == d_attr.shape[0]


def test_save_cropped_boxes_writes_the_reference_file(tmp_path):
    from pointgnn_amd import crop_aug as CA
    path = str(tmp_path / "db.json")
    CA.save_cropped_boxes(
        SceneDataset(_device_points), path,
        expand_factor=DB["expand_factor"],
        minimum_points=DB["minimum_points"], backlist=DB["backlist"])
    with open(path) as f:
        got = json.load(f)
    with open(DB_FILE) as f:
        want = json.load(f)
    assert isinstance(got, list) and len(got) == 2      # the reference's pair
    assert got[0] == want[0]                            # labels
    assert list(got[1]) == list(want[1])
    for key in want[1]:
        assert len(got[1][key]) == len(want[1][key])
        for (g_xyz, g_attr), (w_xyz, w_attr) in zip(got[1][key],
                                                    want[1][key]):
            assert g_xyz == w_xyz and g_attr == w_attr
    labels, points = CA.load_cropped_boxes(path)
    assert {k: len(v) for k, v in points.items()} == \
        {k: len(v) for k, v in want[1].items()}


@pytest.mark.parametrize("n", [1, 37, 5000])
def test_sel_xyz_in_box2d_against_numpy(n):
    import torch
    from pointgnn_amd import kitti_dataset as KD
    xyz = LO.synthetic_vertices(50 + n, k=n)
    labels = LO.synthetic_labels(51, LO.synthetic_vertices(50 + n, k=max(n, 9)),
                                 n_boxes=9)
    expend = (1.3, 1.1, 1.2)
    hits = 0
    for label in labels:
        w, lower, upper = LO.box_normals(label, expend)
        proj = np.matmul(xyz, w[1:].T)
        want = np.all((proj > lower[1:]) & (proj < upper[1:]), axis=1)
        got = KD.sel_xyz_in_box2d(label, torch.from_numpy(xyz).cuda(), expend)
        assert got.dtype == torch.bool and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), want)
        assert np.array_equal(KD.sel_xyz_in_box2d(label, xyz, expend), want)
        # the column holds the box
        assert not np.any(LO.sel_xyz_in_box3d(label, xyz, expend) & ~want)
        hits += int(want.sum())
    assert n < 37 or hits > 0


def _place_alone(n_samples, n_labels, mode):
    import torch
    from pointgnn_amd import crop_aug as CA
    xyz = torch.from_numpy(LO.synthetic_vertices(60, k=700).astype(np.float64)
                           ).cuda()
    s_xyz = torch.zeros((n_samples, 3), dtype=torch.float64, device="cuda")
    work, alive, record = CA.place(
        xyz, s_xyz, np.arange(n_samples + 1),
        np.tile([0.0, 1.0, 20.0, 4.0, 1.5, 1.6, 0.0], (n_samples, 1)),
        np.zeros((n_labels, 8, 3), np.int32), np.zeros((n_samples * 2, 3)),
        2, mode, False, False, 0.01, 100, 1, (1.1, 1.1, 1.1))
    return xyz, work, alive, record


def test_kernel_alone_without_samples_and_beyond_its_limit():
    import torch
    from pointgnn_amd import _lib
    xyz, work, alive, record = _place_alone(0, 5, 0)
    assert torch.equal(work, xyz)                 # the cloud, unchanged
    assert bool((alive == 1).all())
    assert record.cpu().tolist() == [0.0, 700.0]  # no draw spent, 700 rows
    # labels + samples beyond the boxes kept in LDS: refused, not truncated
    _place_alone(6, 250, 0)
    with pytest.raises(_lib.PointGnnHipError, match="256"):
        _place_alone(7, 250, 0)
    _place_alone(7, 250, 1)                       # 'point' keeps no boxes


def test_parser_argument_errors_and_database_errors():
    from pointgnn_amd import crop_aug as CA
    from pointgnn_amd.kitti_dataset import Points
    xyz, attr, labels = scene(40, None, 300)
    pts = _device_points(xyz, attr)
    sampler = _sampler()
    with pytest.raises(ValueError):
        CA.parser_without_collision(pts, labels, [], [], method_name='other')
    with pytest.raises(ValueError):
        CA.parser_without_collision(Points(xyz=pts.xyz, attr=None), labels,
                                    [], [])
    with pytest.raises(KeyError):
        sampler.crop_aug(pts, labels, sample_rate={"Tram": 1})
    with pytest.raises(ValueError):             # np.random.choice's
        sampler.crop_aug(pts, labels, sample_rate={"Car": 10 ** 6})
    # no labels: an empty corner list, every object is accepted
    np.random.seed(40)
    empty = []
    out, labs = sampler.crop_aug(
        pts, empty, sample_rate={"Car": 1},
        parser_kwargs=dict(overlap_mode='box', max_trails=1))
    assert labs is empty and len(labs) == 1
    assert out.xyz.shape[0] > len(xyz)


def test_training_sample_with_crop_aug(tmp_path):
    """train.fetch_data with 'crop_aug' in the train_config on KITTI files
    (the tree of test_gpu_aug_registry.py's end-to-end test): a 7-tuple,
    pasted labels reach the targets, one Trainer step is finite."""
    import torch
    from test_ingest_cpu import _write_png_header_only
    from test_gpu_e2e import _velodyne_scan
    from oracle import ingest_oracle as IO
    from pointgnn_amd import configs, kitti_dataset as KD, train, weights
    cfg = configs.get_config("car_auto_T1")
    for d in ("image_2", "velodyne", "calib", "label_2"):
        (tmp_path / d).mkdir()
    velo = _velodyne_scan(5)
    velo.tofile(str(tmp_path / "velodyne" / "000001.bin"))
    (tmp_path / "calib" / "000001.txt").write_text("".join(IO.CALIB_LINES))
    _write_png_header_only(str(tmp_path / "image_2" / "000001.png"), 375, 1242)
    cam, _, _ = IO.cam_points_in_image(velo, IO.get_calib(IO.CALIB_LINES),
                                       (375, 1242))
    LO.write_label_file(str(tmp_path / "label_2" / "000001.txt"),
                        LO.synthetic_labels(5, cam, n_boxes=12))
    ds = KD.KittiDataset(str(tmp_path / "image_2"), str(tmp_path / "velodyne"),
                         str(tmp_path / "calib"), str(tmp_path / "label_2"),
                         is_training=True, num_classes=cfg["num_classes"])
    # a database of this dataset's own objects (4 attribute columns)
    db = str(tmp_path / "db.json")
    from pointgnn_amd import crop_aug as CA
    CA.save_cropped_boxes(ds, db, minimum_points=3,
                          backlist=['Van', 'Truck', 'Pedestrian', 'Cyclist',
                                    'Person_sitting'])
    n_db = len(CA.load_cropped_boxes(db)[0]["Car"])
    assert n_db >= 1
    tcfg = {'data_aug_configs': [],
            'crop_aug': {'crop_filename': db, 'sample_rate': {"Car": n_db},
                         'parser_kwargs': dict(
                             overlap_mode='point', max_trails=20,
                             max_overlap_num_allowed=10 ** 6,
                             method_name='uniform', yaw_std=0.3)}}
    n_labels = len(ds.get_label(0))
    n_in = int(ds.get_cam_points_in_image_with_rgb(
        0, cfg['downsample_by_voxel_size']).xyz.shape[0])
    np.random.seed(5)
    sample = train.fetch_data(ds, 0, cfg, tcfg)
    assert len(sample) == 7
    input_v, coords, kps, edges, cls, enc, valid = sample
    assert input_v.shape[0] == coords[0].shape[0]
    assert input_v.dtype == torch.float32
    # the same pasting again for the label list fetch_data worked with
    np.random.seed(5)
    sampler = train.get_crop_sampler(tcfg)
    assert sampler is train.get_crop_sampler(tcfg)          # built once
    pts, labels = sampler.crop_aug(
        ds.get_cam_points_in_image_with_rgb(
            0, cfg['downsample_by_voxel_size']), ds.get_label(0),
        sample_rate=tcfg['crop_aug']['sample_rate'],
        parser_kwargs=tcfg['crop_aug']['parser_kwargs'])
    assert len(labels) == n_labels + n_db                   # all pasted
    assert int(pts.xyz.shape[0]) == int(coords[0].shape[0]) != n_in
    level = cfg['model_kwargs']['layer_configs'][-1]['graph_level']
    last = coords[level + 1]
    last64 = pts.xyz[kps[0].reshape(-1).long()]
    assert torch.equal(last64.to(torch.float32), last)
    o_cls, o_boxes, o_valid, _ = LO.assign_labels(
        labels, last64.cpu().numpy(), (1.0, 1.0, 1.0), "Car")
    assert np.array_equal(cls.cpu().numpy(), o_cls)
    assert np.array_equal(valid.cpu().numpy(), o_valid)
    # vertices that only a PASTED label claims
    before, _, _, _ = LO.assign_labels(
        labels[:n_labels], last64.cpu().numpy(), (1.0, 1.0, 1.0), "Car")
    pasted, _, _, _ = LO.assign_labels(
        labels[n_labels:], last64.cpu().numpy(), (1.0, 1.0, 1.0), "Car")
    assert int(((pasted > 0) & (before == 0) & (o_cls > 0)).sum()) > 0
    assert bool(torch.isfinite(enc).all())
    tr = train.Trainer(cfg, params=weights.init_params(cfg, seed=1),
                       device=last.device)
    out = tr.train_step(sample, num_valid=float(o_valid.sum()))
    assert np.isfinite([out['cls_loss'], out['loc_loss'], out['reg_loss']]).all()
    assert out['num_endpoint'] == len(o_cls)
