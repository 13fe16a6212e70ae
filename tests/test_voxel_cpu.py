"""Voxel-average down-sampling, no GPU: the NumPy evaluation of the DEFINED
form (tests/_voxel.py: stable argsort, sequential float32 sums in ascending
original index) against the reference's own `downsample_by_average_voxel` --
live where the reference tree is present, and through
tests/golden/voxel_average.npz (tests/golden/make_golden_voxel.py) always.

Rule: identical `lens` and row count; rows of voxels with one or two points
bit-identical (a + b = b + a); rows with k > 2 points within
2 * gamma_{k-1} * sum|x_i| / k per column (tests/_voxel.py order_bound): the
reference's argsort is not stable, so its summation order there is NumPy's
sort implementation's.  Every row is checked one way or the other, and the
share that is not bit-compared is capped."""
import os

import numpy as np
import pytest

import pointgnn_amd  # noqa: F401
import _voxel as V
from _refimport import REF_ROOT as REF


@pytest.fixture(scope="module")
def fix():
    return V.load_fixture()


@pytest.fixture(scope="module")
def cloud(fix):
    velo, image, cam = V.inputs(fix)
    return cam, velo[:, [3]]


def test_fixture_is_small():
    assert os.path.getsize(os.path.join(V.GOLD, "voxel_average.npz")) < 1 << 20


@pytest.mark.parametrize("voxel", V.VOXELS)
def test_defined_form_against_fixture(fix, cloud, voxel):
    xyz, attr, lens, mag = V.defined_voxel_average(cloud[0], cloud[1], voxel)
    t = V.tag(voxel)
    V.check_against_reference(voxel, xyz, attr, lens, mag, fix["lens_" + t],
                              fix["wide_" + t], fix["narrow_sha256_" + t],
                              "fixture")


def test_wrap_cloud_against_fixture(fix):
    """dim_x * dim_y * dim_z > 2^31: the int32 key wraps; a uint32 evaluation
    read as int32 gives the reference's rows (no voxel of the cloud has more
    than two points, so every row is bit-compared)."""
    wx, wa = V.wrap_cloud()
    assert np.array_equal(wx, fix["wrap_xyz_in"])
    assert np.array_equal(wa, fix["wrap_attr_in"])
    off = wx.min(0)
    dim = ((wx - off) // np.float32(0.01)).astype(np.int64).max(0) + 1
    assert int(dim[0]) * int(dim[1]) * int(dim[2]) > 2 ** 31
    xyz, attr, lens, _ = V.defined_voxel_average(wx, wa, 0.01)
    assert lens.max() == 2 and (lens == 2).sum() > 10
    assert xyz.dtype == np.float64
    assert np.array_equal(xyz, fix["wrap_xyz"])
    assert np.array_equal(attr, fix["wrap_attr"])


def _reference():
    if not os.path.isdir(os.path.join(REF, "dataset")):
        pytest.skip("the reference tree is not on this machine")
    import sys
    sys.path.insert(0, V.GOLD)
    try:
        from make_golden_ingest import reference_dataset_module
    finally:
        sys.path.remove(V.GOLD)
    return reference_dataset_module()


@pytest.mark.parametrize("voxel", V.VOXELS + (2.0,))
def test_defined_form_against_live_reference(cloud, voxel):
    kd = _reference()
    ref = kd.downsample_by_average_voxel(
        kd.Points(xyz=cloud[0], attr=cloud[1]), voxel)
    xyz, attr, lens, mag = V.defined_voxel_average(cloud[0], cloud[1], voxel)
    wide = lens > 2
    assert len(ref.xyz) == len(lens)
    V.check_against_reference(
        voxel, xyz, attr, lens, mag, lens,
        np.concatenate([ref.xyz[wide], ref.attr[wide]], axis=1),
        V.sha256(ref.xyz[~wide], ref.attr[~wide]), "live")


def test_live_reference_without_attr_and_wrap():
    kd = _reference()
    wx, wa = V.wrap_cloud()
    ref = kd.downsample_by_average_voxel(kd.Points(xyz=wx, attr=None), 0.01)
    xyz, attr, _, _ = V.defined_voxel_average(wx, None, 0.01)
    assert attr is None and ref.attr is None
    assert np.array_equal(xyz, ref.xyz)
