#!/usr/bin/env python
"""Generate tests/golden/aug_registry.npz by running the reference's own
augmentation functions (models/preprocess.py, imported from its checkout at
run time) with NumPy's global RNG seeded, on the seeded synthetic scenes and
the pipelines of tests/test_gpu_aug_registry.py (CASES and scene() are
imported from there, so the test and the fixture cannot drift apart).
open3d / cv2 / shapely are stubbed as in make_golden_aug.py.

Per case: the final cloud as float32, its attributes, the label names and
values, and `rng_after = np.random.uniform()`.  For the two voxel-based
methods also the voxel size, the jitter the reference drew and the number of
occupied voxels.

Conditions on the inputs, asserted here: in every sel_xyz_in_box3d call no
point lies within 1e-9 of a box face in the projected coordinate, and in every
random-voxel downsample no coordinate lies within 1e-9 voxels of a voxel
boundary -- so a last-bit difference in float64 coordinates cannot change a
mask or a voxel, and the branches the cases are there for are really taken.

    python tests/golden/make_golden_aug_registry.py
"""
import copy
import os
import random
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
import test_gpu_aug_registry as T  # noqa: E402

MARGIN = 1e-9


def load_reference():
    sys.modules.setdefault("open3d", types.ModuleType("open3d"))
    sys.modules["cv2"] = RO.cv2_stub()
    shp = types.ModuleType("shapely")
    geo = types.ModuleType("shapely.geometry")
    geo.Polygon = DO.ConvexPolygon
    shp.geometry = geo
    sys.modules["shapely"], sys.modules["shapely.geometry"] = shp, geo
    sys.path.insert(0, REF)
    try:
        from models import preprocess
        from dataset import kitti_dataset
    finally:
        sys.path.remove(REF)
    return preprocess, kitti_dataset


def generate(k):
    preprocess, kitti_dataset = load_reference()
    Points = kitti_dataset.Points
    seen = {"box_calls": 0, "closest": np.inf, "voxel": []}
    # (generate() may run again with a smaller k: wrap the originals)
    real_sel = getattr(preprocess, "_real_sel", preprocess.sel_xyz_in_box3d)
    real_voxel = getattr(preprocess, "_real_voxel",
                         preprocess.downsample_by_random_voxel)
    preprocess._real_sel, preprocess._real_voxel = real_sel, real_voxel

    def checked_sel(label, xyz, expend_factor=(1.0, 1.0, 1.0)):
        normals, lower, upper = kitti_dataset.box3d_to_normals(label,
                                                               expend_factor)
        proj = np.matmul(np.asarray(xyz, np.float64), np.transpose(normals))
        if proj.size:
            gap = min(np.abs(proj - lower).min(), np.abs(proj - upper).min())
            seen["closest"] = min(seen["closest"], gap)
            assert gap > MARGIN, "a point within 1e-9 of a box face"
        seen["box_calls"] += 1
        return real_sel(label, xyz, expend_factor)

    def recording_voxel(points, voxel_size, add_rnd3d=False):
        assert add_rnd3d
        state = np.random.get_state()
        jitter = voxel_size * np.random.random((1, 3))
        np.random.set_state(state)
        out = real_voxel(points, voxel_size, add_rnd3d=add_rnd3d)
        offset = np.amin(points.xyz, axis=0, keepdims=True)
        cell = (points.xyz - offset + jitter) / voxel_size
        edge = np.abs(cell - np.round(cell))
        # (the minimum itself sits on a boundary when the jitter is 0: it is
        # not, the draw is from (0, 1) times the voxel)
        assert edge.min() > MARGIN, "a point within 1e-9 voxels of a boundary"
        idx = (points.xyz - offset + jitter) // voxel_size
        assert len(np.unique(idx, axis=0)) == len(out.xyz)
        seen["voxel"].append((float(voxel_size), jitter, len(out.xyz),
                              len(points.xyz)))
        return out

    preprocess.sel_xyz_in_box3d = checked_sel
    preprocess.downsample_by_random_voxel = recording_voxel
    assert set(preprocess.aug_method_map) == T.REGISTRY_KEYS
    out = {"k_points": np.array(k)}
    for name, (seed, variant, steps) in T.CASES.items():
        xyz, attr, labels = T.scene(seed, variant, k)
        pts = Points(xyz=xyz.copy(), attr=attr.copy())
        labs = copy.deepcopy(labels)
        np.random.seed(seed)
        random.seed(seed)
        seen["voxel"] = []
        counts = [len(xyz)]
        for method, kwargs in steps:
            pts, labs = preprocess.aug_method_map[method](
                pts, labs, **copy.deepcopy(kwargs))
            counts.append(len(pts.xyz))
        assert np.asarray(pts.xyz).dtype == np.float64
        pre = name + "_"
        out[pre + "xyz"] = np.asarray(pts.xyz).astype(np.float32)
        out[pre + "attr"] = np.asarray(pts.attr, np.float32).reshape(
            len(pts.xyz), -1)
        out[pre + "names"] = np.array([l['name'] for l in labs], dtype=str)
        out[pre + "labels"] = np.array(
            [[l[key] for key in T.LABEL_KEYS] for l in labs],
            np.float64).reshape(len(labs), len(T.LABEL_KEYS))
        out[pre + "rng_after"] = np.array(np.random.uniform())
        if name in T.VOXEL_CASES:
            assert len(seen["voxel"]) == 1 and steps[-1][0] in (
                "random_voxel_downsample", "dilute_background")
            voxel, jitter, n_vox, n_in = seen["voxel"][0]
            out[pre + "voxel_size"] = np.array(voxel)
            out[pre + "jitter"] = jitter
            out[pre + "voxel_count"] = np.array(n_vox)
            assert 1 < n_vox < n_in
        else:
            assert not seen["voxel"]
        print("%-26s points %s  labels %d -> %d" % (
            name, " -> ".join(map(str, counts)), len(labels), len(labs)))
        # the branches the cases are there for
        n0, n1 = counts[-2], counts[-1]
        if name in ("drop_all", "voxel_below"):
            assert n1 == n0 == k
        if name in ("drop_scalar", "drop_tier", "global_drop", "voxel_above",
                    "remove_all_objects", "remove_three_objects",
                    "remove_keep_list_fallback", "dilute"):
            assert 1 < n1 < n0
        if name == "remove_only_dontcare":
            assert n1 == 1 and len(labs) == 0
        if name == "remove_keep_list_fallback":
            assert labs and all(l['name'] == 'Tram' for l in labs)
        if name == "box_rotation_fail":
            # ROT turned every object's yaw; a failed label keeps that one
            rot_only = copy.deepcopy(labels)
            np.random.seed(seed)
            _, rot_only = preprocess.random_rotation_all(
                Points(xyz=xyz.copy(), attr=attr), rot_only, **steps[0][1])
            objs = [l for l in rot_only if l['name'] != 'DontCare']
            same = sum(a['yaw'] == b['yaw'] for a, b in zip(objs, labs))
            print("    labels that failed all trials: %d of %d" % (same,
                                                                    len(objs)))
            assert 0 < same < len(objs)
        if name == "box_global_rotation":
            assert n1 < n0                       # foreign points were deleted
        if name == "long":
            assert counts[4] < counts[3] and counts[5] < counts[4]
            assert counts[7] < counts[6]
    print("sel_xyz_in_box3d calls %d, closest point to a face %.3g" % (
        seen["box_calls"], seen["closest"]))
    return out


def main():
    k = T.K_POINTS
    while True:
        out = generate(k)
        path = os.path.join(HERE, "aug_registry.npz")
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
        print("k = %d: %d bytes" % (k, size))
        if size <= MAX_BYTES:
            break
        k = k * 3 // 4                 # the file would be too large: shrink k
    return 0


if __name__ == "__main__":
    sys.exit(main())
