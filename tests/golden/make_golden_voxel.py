#!/usr/bin/env python
"""Generate tests/golden/voxel_average.npz with the reference's own
`downsample_by_average_voxel`, `velo_points_to_cam`, `cam_points_to_image` and
`rgb_to_cam_points` (dataset/kitti_dataset.py), imported under empty `open3d`
/ `cv2` stubs exactly as make_golden_ingest.py does.

Inputs are seeded (oracle.ingest_oracle) and stored as digests.  Per voxel
size: `lens`, the float64 rows of voxels with more than two points in full,
a sha256 over the rows of voxels with one or two points (their sums do not
depend on the order NumPy's unstable argsort leaves the points in); for 0.4
the rows that survive the front mask / image crop / colour lookup; and one
small cloud whose int32 voxel key wraps.

    python tests/golden/make_golden_voxel.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from oracle import ingest_oracle as IO  # noqa: E402
from make_golden_ingest import reference_dataset_module  # noqa: E402
import _voxel as V  # noqa: E402


def reference_calib(kd, ds):
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "000000.txt"), "w") as f:
            f.writelines(IO.CALIB_LINES)
        ds._calib_dir = tmp
        ds._file_list = ["000000"]
        return ds.get_calib(0)


def main():
    kd = reference_dataset_module()
    ds = object.__new__(kd.KittiDataset)
    calib = reference_calib(kd, ds)
    velo = IO.synthetic_velo_scan(0, n=60000)
    image = IO.synthetic_image(0)
    height, width = image.shape[:2]
    cam = ds.velo_points_to_cam(
        kd.Points(xyz=velo[:, :3], attr=velo[:, [3]]), calib)
    out = {"velo_sha256": V.sha256(velo), "image_sha256": V.sha256(image),
           "cam_sha256": V.sha256(cam.xyz)}
    for voxel in V.VOXELS:
        ref = kd.downsample_by_average_voxel(cam, voxel)
        assert ref.xyz.dtype == np.float64 and ref.attr.dtype == np.float64
        # lens: the reference does not return them; the voxel partition is
        # order-free, so the defined form's are the reference's (row count
        # checked here, every row checked by the tests)
        _, _, lens, _ = V.defined_voxel_average(cam.xyz, cam.attr, voxel)
        assert len(lens) == len(ref.xyz)
        wide = lens > 2
        t = V.tag(voxel)
        out["lens_" + t] = lens.astype(np.int32)
        out["wide_" + t] = np.concatenate(
            [ref.xyz[wide], ref.attr[wide]], axis=1)
        out["narrow_sha256_" + t] = V.sha256(ref.xyz[~wide], ref.attr[~wide])
        print("voxel", voxel, "rows", len(lens), "lens > 2: %.3f%%"
              % (100 * wide.mean()))
        if voxel == 0.4:
            front = ref.xyz[:, 2] > 0.1
            front_pts = kd.Points(ref.xyz[front, :], ref.attr[front, :])
            img = ds.cam_points_to_image(front_pts, calib)
            inside = np.logical_and.reduce(
                [img.xyz[:, 0] > 0, img.xyz[:, 0] < width,
                 img.xyz[:, 1] > 0, img.xyz[:, 1] < height])
            in_img = kd.Points(xyz=front_pts.xyz[inside, :],
                               attr=front_pts.attr[inside, :])
            with_rgb = ds.rgb_to_cam_points(in_img, image, calib)
            assert with_rgb.attr.dtype == np.float64
            out["in_image_kept"] = np.arange(
                len(lens), dtype=np.int32)[front][inside]
            out["in_image_xyz"] = in_img.xyz
            out["in_image_attr_rgb"] = with_rgb.attr
            print("in image", len(in_img.xyz))
    wx, wa = V.wrap_cloud()
    ref = kd.downsample_by_average_voxel(kd.Points(xyz=wx, attr=wa), 0.01)
    out["wrap_xyz_in"], out["wrap_attr_in"] = wx, wa
    out["wrap_xyz"], out["wrap_attr"] = ref.xyz, ref.attr
    print("wrap cloud", len(wx), "->", len(ref.xyz))
    path = os.path.join(HERE, "voxel_average.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
