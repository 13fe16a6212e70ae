#!/usr/bin/env python
"""Generate tests/golden/crop_aug_db.json and tests/golden/crop_aug.npz by
running the reference's own models/crop_aug.py (imported from its checkout at
run time) with NumPy's global RNG seeded: `save_cropped_boxes` over the
database scenes, then every case of tests/test_gpu_crop_aug.py (CASES, DB,
scene(), SceneDataset and run_case() are imported from there, so the test and
the fixture cannot drift apart).  open3d / cv2 / shapely are stubbed as in
make_golden_aug_registry.py, tqdm passes its argument through.

Per case: the final cloud as float32, its attributes, the label names and
values, `rng_after = np.random.uniform()`, and per sample whether it was
accepted, the trials it used and the y3d_adjust of the accepting trial.

Conditions on the inputs, asserted here, so that a last-bit difference of a
float64 value cannot change a decision: in every sel_xyz_in_box3d /
sel_xyz_in_box2d call no point lies within 1e-9 of a box face in the projected
coordinate; no `appr_factor * corner` coordinate lies within 1e-9 of an
integer; no overlap lies within 1e-9 of max_overlap_rate.  And the branches
the cases are there for are really taken (check_branches).

    python tests/golden/make_golden_crop_aug.py
    python tests/golden/make_golden_crop_aug.py --search NAME   # try seeds
"""
import copy
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
REF = "/root/reference"
MAX_BYTES = 1 << 20          # no committed file above 1 MiB

from oracle import detect_oracle as DO  # noqa: E402
from oracle import raster_oracle as RO  # noqa: E402
import test_gpu_crop_aug as T  # noqa: E402

MARGIN = 1e-9
DB_PATH = os.path.join(HERE, "crop_aug_db.json")
_SAMPLE_ID = ('length', 'height', 'width', 'alpha', 'truncation', 'ymax')


def load_reference():
    sys.modules.setdefault("open3d", types.ModuleType("open3d"))
    sys.modules["cv2"] = RO.cv2_stub()
    shp = types.ModuleType("shapely")
    geo = types.ModuleType("shapely.geometry")
    geo.Polygon = DO.ConvexPolygon
    shp.geometry = geo
    sys.modules["shapely"], sys.modules["shapely.geometry"] = shp, geo
    tq = types.ModuleType("tqdm")
    tq.tqdm = lambda it, *a, **k: it
    sys.modules.setdefault("tqdm", tq)
    sys.path.insert(0, REF)
    try:
        from models import crop_aug
        from dataset import kitti_dataset
    finally:
        sys.path.remove(REF)
    return crop_aug, kitti_dataset


def write_database(ca, kd, path):
    ca.save_cropped_boxes(
        T.SceneDataset(lambda xyz, attr: kd.Points(xyz=xyz, attr=attr)), path,
        expand_factor=T.DB["expand_factor"],
        minimum_points=T.DB["minimum_points"], backlist=T.DB["backlist"])


class Tracker(object):
    """Wraps the functions parser_without_collision calls and follows its
    state from outside: which sample a trial belongs to, whether the trial
    before was accepted (the cloud is a new array then), how many rows at the
    front of the cloud were pasted (an accepted object is prepended, removal
    keeps the order) and whether an accepted box removed some of them."""

    def __init__(self, ca, kd, kwargs):
        self.ca, self.kd = ca, kd
        self.auto = bool(kwargs.get('auto_box_height', False))
        self.must = bool(kwargs.get('must_have_ground', False))
        self.appr = kwargs.get('appr_factor', 100)
        self.rate = kwargs.get('max_overlap_rate', 0.01)
        self.max_trails = kwargs.get('max_trails', 1)
        self.real = {n: getattr(ca, n) for n in (
            'sel_xyz_in_box3d', 'sel_xyz_in_box2d', 'boxes_3d_to_corners',
            'overlapped_boxes_3d_fast_poly', 'parser_without_collision')}
        self.closest = np.inf
        self.samples, self.sizes = None, None
        self.trial = None          # the running trial
        self.n_pasted = 0
        self.pasted_removed = 0
        self.spent_no_ground = 0
        self.accepted_without_ground = 0     # ... and y3d_adjust = 0

    def __enter__(self):
        for n in self.real:
            setattr(self.ca, n, getattr(self, n))
        return self

    def __exit__(self, *exc):
        for n, fn in self.real.items():
            setattr(self.ca, n, fn)

    def _faces(self, label, xyz, expend, rows):
        normals, lower, upper = self.kd.box3d_to_normals(label, expend)
        proj = np.matmul(np.asarray(xyz, np.float64),
                         np.transpose(normals[rows]))
        if proj.size:
            gap = min(np.abs(proj - lower[rows]).min(),
                      np.abs(proj - upper[rows]).min())
            self.closest = min(self.closest, gap)
            assert gap > MARGIN, "a point within 1e-9 of a box face"

    def _settle(self, xyz):
        """The trial before: accepted when it reached the 3-D test and the
        cloud is another array now."""
        t, self.trial = self.trial, None
        if t is None or t.get("mask") is None or xyz is t["xyz"]:
            return
        i = t["sample"]
        self.accepted[i] = True
        self.adjust[i] = t["adjust"]
        if t.get("ground") is False:
            self.accepted_without_ground += 1
            assert t["adjust"] == 0.0
        gone = int(t["mask"][:self.n_pasted].sum())
        self.pasted_removed += gone
        self.n_pasted = self.n_pasted - gone + self.sizes[i]
        assert len(xyz) == len(t["xyz"]) - int(t["mask"].sum()) + self.sizes[i]

    def _begin(self, label, xyz):
        self._settle(xyz)
        hits = [i for i, s in enumerate(self.samples)
                if all(s[k] == label[k] for k in _SAMPLE_ID)]
        assert len(hits) == 1
        i = hits[0]
        assert not self.accepted[i]
        self.trials[i] += 1
        self.trial = {"sample": i, "xyz": xyz, "adjust": 0.0, "mask": None}

    def sel_xyz_in_box2d(self, label, xyz, expend_factor=(1.0, 1.0, 1.0)):
        assert self.auto
        self._begin(label, xyz)
        self._faces(label, xyz, expend_factor, slice(1, 3))
        mask = self.real['sel_xyz_in_box2d'](label, xyz, expend_factor)
        if np.sum(mask) > 0:
            # crop_aug.py:118-119
            self.trial["adjust"] = np.amax(xyz[mask][:, 1]) - label['y3d']
            self.trial["ground"] = True
        else:
            self.trial["ground"] = False
            if self.must:
                self.spent_no_ground += 1
        return mask

    def sel_xyz_in_box3d(self, label, xyz, expend_factor=(1.0, 1.0, 1.0)):
        if not self.auto:
            self._begin(label, xyz)
        assert xyz is self.trial["xyz"]
        self._faces(label, xyz, expend_factor, slice(0, 3))
        mask = self.real['sel_xyz_in_box3d'](label, xyz, expend_factor)
        self.trial["mask"] = mask
        return mask

    def boxes_3d_to_corners(self, boxes_3d):
        corners = self.real['boxes_3d_to_corners'](boxes_3d)
        if corners.size:
            grid = self.appr * corners
            assert np.abs(grid - np.round(grid)).min() > MARGIN, \
                "an integer corner coordinate within 1e-9 of a boundary"
        return corners

    def overlapped_boxes_3d_fast_poly(self, single_box, box_list):
        ov = self.real['overlapped_boxes_3d_fast_poly'](single_box, box_list)
        assert not np.any(np.abs(ov - self.rate) <= MARGIN), \
            "an overlap within 1e-9 of max_overlap_rate"
        return ov

    def parser_without_collision(self, cam_rgb_points, labels,
                                 sample_cam_points, sample_labels, **kwargs):
        self.samples = copy.deepcopy(sample_labels)
        self.sizes = [len(p.xyz) for p in sample_cam_points]
        n = len(sample_labels)
        self.accepted, self.trials = [False] * n, [0] * n
        self.adjust = [0.0] * n
        out, labs = self.real['parser_without_collision'](
            cam_rgb_points, labels, sample_cam_points, sample_labels,
            **kwargs)
        self._settle(out.xyz)
        assert sum(self.accepted) == len(labs) - self.n_labels_in
        return out, labs


def check_branches(name, case, trk, counts):
    """The branches the cases are there for."""
    acc = np.array(trk.accepted)
    trials = np.array(trk.trials)
    kw = case["parser_kwargs"]
    failed_all = ~acc & (trials == kw["max_trails"])
    if name == "box_one_trial":
        assert kw["max_trails"] == 1 and 0 < acc.sum() < len(acc)
    if name == "box_trials":
        assert kw["max_trails"] > 1 and acc.any() and failed_all.any()
        assert np.any(acc & (trials > 1))        # accepted after a rejection
    if name == "point":
        assert trk.pasted_removed > 0 and 0 < acc.sum() < len(acc)
    if name == "ground_required":
        assert trk.spent_no_ground > 0
        assert np.any(acc & (np.array(trk.adjust) != 0))
        assert failed_all.any() or np.any(trials > 1)
    if name == "ground_optional_uniform":
        assert kw["method_name"] == "uniform"
        assert trk.accepted_without_ground > 0
    if name == "dontcare_scene":
        assert 0 < acc.sum() < len(acc)
    if name == "tiny_cloud":
        assert counts[0] == 37 and acc.any()
    if name == "one_point_sample":
        assert 1 in trk.sizes and acc[trk.sizes.index(1)]
        assert kw["method_name"] == "uniform"


def run_reference_case(ca, kd, sampler, name, case, seed, k):
    xyz, attr, labels = T.scene(seed, case["variant"], k)
    if case["variant"] == "dontcare":
        assert labels and all(l['name'] == 'DontCare' for l in labels)
    pts = kd.Points(xyz=xyz.copy(), attr=attr.copy())
    labs = copy.deepcopy(labels)
    np.random.seed(seed)
    with Tracker(ca, kd, case["parser_kwargs"]) as trk:
        trk.n_labels_in = len(labs)
        out, labs = T.run_case(ca, sampler, case, pts, labs)
    pre = name + "_"
    res = {
        pre + "k_points": np.array(k),
        pre + "xyz": np.asarray(out.xyz).astype(np.float32),
        pre + "attr": np.asarray(out.attr, np.float32).reshape(
            len(out.xyz), -1),
        pre + "names": np.array([l['name'] for l in labs], dtype=str),
        pre + "labels": np.array(
            [[l[key] for key in T.LABEL_KEYS] for l in labs],
            np.float64).reshape(len(labs), len(T.LABEL_KEYS)),
        pre + "rng_after": np.array(np.random.uniform()),
        pre + "accepted": np.array(trk.accepted, np.int32),
        pre + "trials": np.array(trk.trials, np.int32),
        pre + "y3d_adjust": np.array(trk.adjust, np.float64),
    }
    assert np.asarray(out.xyz).dtype == np.float64 or not any(trk.accepted)
    counts = (len(xyz), len(out.xyz))
    check_branches(name, case, trk, counts)
    print("%-24s seed %d  points %d -> %d  labels %d -> %d  accepted %s  "
          "trials %s  pasted rows removed %d  closest face %.3g" % (
              name, seed, counts[0], counts[1], len(labels), len(labs),
              "".join(map(str, res[pre + "accepted"])), list(trk.trials),
              trk.pasted_removed, trk.closest))
    return res


def search(ca, kd, sampler, name):
    case = T.CASES[name]
    for seed in range(case["seed"], case["seed"] + 400):
        try:
            run_reference_case(ca, kd, sampler, name, case, seed, case["k"])
        except AssertionError as exc:
            print("seed %d: %s" % (seed, exc or "branch not taken"))
            continue
        print("seed %d meets the conditions of %s" % (seed, name))
        return 0
    return 1


def main(argv):
    ca, kd = load_reference()
    write_database(ca, kd, DB_PATH)
    size = os.path.getsize(DB_PATH)
    print("database: %d bytes" % size)
    assert size <= MAX_BYTES
    sampler = ca.CropAugSampler(DB_PATH)
    if len(argv) > 2 and argv[1] == "--search":
        return search(ca, kd, sampler, argv[2])
    out = {"db_names": np.array(list(sampler._cropped_labels), dtype=str),
           "db_counts": np.array([len(v) for v in
                                  sampler._cropped_labels.values()])}
    for name, case in T.CASES.items():
        out.update(run_reference_case(ca, kd, sampler, name, case,
                                      case["seed"], case["k"]))
    path = os.path.join(HERE, "crop_aug.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("fixture: %d bytes" % size)
    assert size <= MAX_BYTES
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
