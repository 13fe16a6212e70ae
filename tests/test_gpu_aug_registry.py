"""The nine augmentations of the reference's registry beyond the shipped
configs' three (pointgnn_amd.preprocess: random_transition, random_scale_all,
random_drop, random_global_drop, random_voxel_downsample, random_box_rotation,
random_box_global_rotation, remove_background, dilute_background) against
fixtures written by the reference's own models/preprocess.py with NumPy's RNG
seeded (tests/golden/make_golden_aug_registry.py imports CASES and scene() from
this file), and the two device entries under them (pgnn_points_compact_f64,
pgnn_points_in_boxes_f64) against NumPy.

Every pipeline starts with random_rotation_all, so the reference's cloud is
float64 like ours from the first step on.  (A pipeline that STARTS with one of
the nine keeps the reference's float32 array in float32; we compute in float64
there -- the deviation test_gpu_aug.py states for random_box_shift.)

Bars for the deterministic methods: the same random decisions (NumPy's global
RNG ends in the same state), identical label lists (values to 1e-13), the same
number of points, points within 1 float32 ulp of the reference's after
finish(), attribute rows bit-identical and in the same order, the caller's
tensors untouched.  The generator asserts that no point of any box test lies
within 1e-9 of a box face, so a last-bit difference of the float64 coordinates
cannot change a mask: a count mismatch is a defect.

The voxel-based methods choose the surviving member of a voxel with Python's
`random` (the reference: random.choice per voxel; here one seed), so their
voxelisation is compared: the fixture's occupied-voxel count, every output row
bit-equal to an input row and carrying its attributes, exactly one output per
voxel of the reference's NumPy key expression under the jitter the reference
drew."""
import copy
import os
import random

import numpy as np
import pytest

from oracle import labels_oracle as LO

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLD, "aug_registry.npz")
LABEL_KEYS = ('x3d', 'y3d', 'z3d', 'yaw', 'length', 'height', 'width')
K_POINTS, N_BOXES = 5000, 18

ROT = ("random_rotation_all", dict(method_name='normal',
                                   yaw_std=0.39269908169872414,
                                   expend_factor=(1.0, 1.0, 1.0)))
_GLOBAL_ROT = ("random_box_global_rotation", dict(
    max_overlap_num_allowed=100, max_trails=10, method_name='normal',
    yaw_std=0.25, expend_factor=(1.2, 1.2, 1.2)))
# name: (seed, scene variant, [(method, kwargs), ...]); the LAST step of the
# VOXEL cases is the voxel-based one
CASES = {
    "transition": (0, None, [ROT, ("random_transition",
                                   dict(xyz_std=(0.2, 0.05, 0.3)))]),
    "scale_normal": (1, None, [ROT, ("random_scale_all", dict(
        method_name='normal', scale_std=0.1))]),
    "scale_uniform": (2, None, [ROT, ("random_scale_all", dict(
        method_name='uniform', scale_std=0.08))]),
    "drop_scalar": (3, None, [ROT, ("random_drop", dict(drop_prob=0.3))]),
    "drop_tier": (4, None, [ROT, ("random_drop", dict(
        drop_prob=[0.1, 0.5, 0.8], tier_prob=[0.2, 0.5, 0.3]))]),
    # nothing survives the draw: the keep-everything branch
    "drop_all": (5, None, [ROT, ("random_drop", dict(drop_prob=1.0))]),
    "global_drop": (6, None, [ROT, ("random_global_drop",
                                    dict(drop_std=0.4))]),
    "voxel_above": (7, None, [ROT, ("random_voxel_downsample", dict(
        voxel_std=0.5, min_voxel=0.01, max_voxel=0.6))]),
    "voxel_below": (8, None, [ROT, ("random_voxel_downsample", dict(
        voxel_std=0.2, min_voxel=5.0, max_voxel=0.8))]),
    # one foreign point already rejects a trial: some labels fail all three
    "box_rotation_fail": (9, None, [ROT, ("random_box_rotation", dict(
        max_overlap_num_allowed=1, max_trails=3, method_name='normal',
        yaw_std=0.8, expend_factor=(1.0, 1.1, 1.1)))]),
    "box_rotation_ok": (10, None, [ROT, ("random_box_rotation", dict(
        max_overlap_num_allowed=100, max_trails=20, method_name='uniform',
        yaw_std=0.5, expend_factor=(1.1, 1.1, 1.1)))]),
    # accepted moves swallow foreign points, which are deleted
    "box_global_rotation": (11, None, [ROT, _GLOBAL_ROT]),
    "remove_all_objects": (12, None, [ROT, ("remove_background", dict(
        expend_factor=(2.0, 2.0, 2.0), num_object=-1))]),
    "remove_three_objects": (13, None, [ROT, ("remove_background", dict(
        expend_factor=(3.0, 3.0, 3.0), num_object=3))]),
    # no label survives either filter: the union is empty, point 0 stays
    "remove_only_dontcare": (14, "dontcare", [ROT, ("remove_background", dict(
        expend_factor=(2.0, 2.0, 2.0)))]),
    # no label is in keep_list: fall back to everything but DontCare
    "remove_keep_list_fallback": (15, "tram", [ROT, ("remove_background", dict(
        expend_factor=(1.5, 1.5, 1.5)))]),
    "dilute": (16, None, [ROT, ("dilute_background", dict(
        dilute_voxel_base=0.6, expend_factor=(2.0, 2.0, 2.0)))]),
    # six of the nine in a row, with a deletion followed by a drop
    "long": (17, None, [
        ROT, ("random_transition", dict(xyz_std=(0.3, 0.02, 0.3))),
        ("random_scale_all", dict(method_name='uniform', scale_std=0.05)),
        _GLOBAL_ROT, ("random_global_drop", dict(drop_std=0.3)),
        ("random_box_rotation", dict(
            max_overlap_num_allowed=50, max_trails=5, method_name='normal',
            yaw_std=0.4, expend_factor=(1.1, 1.1, 1.1))),
        ("remove_background", dict(expend_factor=(3.0, 3.0, 3.0),
                                   num_object=-1))]),
}
VOXEL_CASES = ("voxel_above", "dilute")
REGISTRY_KEYS = {
    'random_jitter', 'random_box_rotation', 'random_box_shift',
    'random_transition', 'remove_background', 'random_rotation_all',
    'random_flip_all', 'random_drop', 'random_global_drop',
    'random_voxel_downsample', 'random_scale_all',
    'random_box_global_rotation', 'dilute_background'}


def scene(seed, variant=None, k=K_POINTS):
    """tests/golden/make_golden_aug.py's scene; `variant` renames labels:
    'dontcare' every label to DontCare, 'tram' every object to Tram (which the
    default keep_list does not hold)."""
    xyz = LO.synthetic_vertices(seed, k=k)
    labels = LO.synthetic_labels(seed, xyz, n_boxes=N_BOXES)
    attr = np.random.default_rng(seed).uniform(0, 1, (len(xyz), 1)
                                               ).astype(np.float32)
    for label in labels:
        if variant == "dontcare":
            label['name'] = 'DontCare'
        elif variant == "tram" and label['name'] != 'DontCare':
            label['name'] = 'Tram'
    return xyz, attr, labels


_FIX = {}


def _fixture():
    if not _FIX:
        with np.load(FIXTURE) as f:
            _FIX.update({k: f[k] for k in f.files})
    return _FIX


def _configs(steps):
    return [{"method_name": m, "method_kwargs": kw} for m, kw in steps]


def _label_array(labs):
    return np.array([[l[k] for k in LABEL_KEYS] for l in labs],
                    np.float64).reshape(len(labs), len(LABEL_KEYS))


def _check_labels(labs, fix, pre):
    assert [l['name'] for l in labs] == [str(s) for s in fix[pre + "names"]]
    np.testing.assert_allclose(_label_array(labs), fix[pre + "labels"],
                               rtol=1e-13, atol=1e-13)


def _ulp(got, ref):
    return np.abs(got.astype(np.float64) - ref) / np.spacing(
        np.maximum(np.abs(got), np.abs(ref)))


def _device_scene(seed, variant, k):
    import torch
    from pointgnn_amd.kitti_dataset import Points
    xyz, attr, labels = scene(seed, variant, k)
    pts = Points(xyz=torch.from_numpy(xyz).cuda(),
                 attr=torch.from_numpy(attr).cuda())
    return xyz, attr, labels, pts


@pytest.mark.parametrize("name", [c for c in CASES if c not in VOXEL_CASES])
def test_deterministic_methods_match_reference_fixture(name):
    import torch
    from pointgnn_amd import preprocess as PP
    fix = _fixture()
    seed, variant, steps = CASES[name]
    xyz, attr, labels, pts = _device_scene(seed, variant, int(fix["k_points"]))
    given_xyz, given_attr = pts.xyz, pts.attr
    np.random.seed(seed)
    random.seed(seed)
    out, labs = PP.get_data_aug(_configs(steps))(pts, copy.deepcopy(labels))
    assert out.xyz.dtype == torch.float64          # like the reference's array
    out = PP.finish(out)
    assert out.xyz.dtype == torch.float32
    pre = name + "_"
    assert np.random.uniform() == float(fix[pre + "rng_after"])   # same draws
    _check_labels(labs, fix, pre)
    got, ref = out.xyz.cpu().numpy(), fix[pre + "xyz"]
    got_attr = out.attr.cpu().numpy()
    print(name, "points", got.shape[0], "of", len(xyz), "reference",
          ref.shape[0])
    assert got.shape == ref.shape
    assert out.attr.dtype == torch.float32
    assert got_attr.shape == fix[pre + "attr"].shape
    assert np.array_equal(got_attr, fix[pre + "attr"])
    ulp = _ulp(got, ref)
    print(name, "identical %.5f, max %.2f ulp" % (np.mean(ulp == 0),
                                                  ulp.max()))
    assert ulp.max() <= 1.0
    # the caller's tensors are untouched
    assert np.array_equal(given_xyz.cpu().numpy(), xyz)
    assert np.array_equal(given_attr.cpu().numpy(), attr)
    assert given_xyz.dtype == torch.float32


def _row_index(rows):
    """bytes of a float64 row -> its index (rows are distinct)."""
    table = {r.tobytes(): i for i, r in enumerate(rows)}
    assert len(table) == len(rows)
    return table


def _check_one_per_voxel(inp_xyz, inp_attr, out_xyz, out_attr, voxel, jitter,
                         n_voxels):
    """`out` = one member of every occupied voxel of `inp` under the
    reference's key expression (dataset/kitti_dataset.py:52-63)."""
    table = _row_index(inp_xyz)
    src = np.array([table.get(r.tobytes(), -1) for r in out_xyz])
    assert np.all(src >= 0)                      # rows of the input, bit-equal
    assert np.array_equal(out_attr, inp_attr[src])
    offset = np.asarray([np.amin(inp_xyz, axis=0)])
    idx = (inp_xyz - offset + jitter) // voxel
    occupied = np.unique(idx, axis=0)
    assert len(occupied) == n_voxels == len(out_xyz)
    assert len(np.unique(idx[src], axis=0)) == n_voxels


@pytest.mark.parametrize("name", VOXEL_CASES)
def test_voxel_methods_match_reference_voxelisation(name):
    import torch
    from pointgnn_amd import preprocess as PP
    fix = _fixture()
    seed, variant, steps = CASES[name]
    xyz, attr, labels, pts = _device_scene(seed, variant, int(fix["k_points"]))
    np.random.seed(seed)
    random.seed(seed)
    mid, labs = PP.get_data_aug(_configs(steps[:-1]))(pts,
                                                      copy.deepcopy(labels))
    inp_xyz, inp_attr = mid.xyz.cpu().numpy(), mid.attr.cpu().numpy()
    out, labs = PP.get_data_aug(_configs(steps[-1:]))(mid, labs)
    assert out.xyz.dtype == torch.float64 and out.attr.dtype == torch.float32
    pre = name + "_"
    assert np.random.uniform() == float(fix[pre + "rng_after"])
    _check_labels(labs, fix, pre)
    assert np.array_equal(mid.xyz.cpu().numpy(), inp_xyz)    # input untouched
    got_xyz, got_attr = out.xyz.cpu().numpy(), out.attr.cpu().numpy()
    n_voxels = int(fix[pre + "voxel_count"])
    voxel, jitter = float(fix[pre + "voxel_size"]), fix[pre + "jitter"]
    assert got_xyz.shape == fix[pre + "xyz"].shape
    assert got_attr.shape == fix[pre + "attr"].shape
    n_front = len(got_xyz) - n_voxels
    print(name, "points", len(inp_xyz), "->", len(got_xyz), "front", n_front,
          "voxels", n_voxels)
    if name == "dilute":
        assert 0 < n_front < len(inp_xyz)
        table = _row_index(inp_xyz)
        front = np.array([table.get(r.tobytes(), -1)
                          for r in got_xyz[:n_front]])
        assert np.all(front >= 0) and np.all(np.diff(front) > 0)   # in order
        assert np.array_equal(got_attr[:n_front], fix[pre + "attr"][:n_front])
        assert np.array_equal(got_attr[:n_front], inp_attr[front])
        f32 = PP.finish(out).xyz.cpu().numpy()[:n_front]
        assert _ulp(f32, fix[pre + "xyz"][:n_front]).max() <= 1.0
        back = np.ones(len(inp_xyz), bool)
        back[front] = False
        inp_xyz, inp_attr = inp_xyz[back], inp_attr[back]
    else:
        assert n_front == 0
    _check_one_per_voxel(inp_xyz, inp_attr, got_xyz[n_front:],
                         got_attr[n_front:], voxel, jitter, n_voxels)


def test_dilute_background_with_empty_background_raises():
    """Every point inside the one (huge) box: the reference's np.amax of the
    empty background raises ValueError (kitti_dataset.py:52)."""
    from pointgnn_amd import preprocess as PP
    xyz, attr, labels, pts = _device_scene(20, None, 300)
    box = dict(labels[0], name='Car', x3d=0.0, y3d=500.0, z3d=20.0,
               length=1000.0, height=1000.0, width=1000.0, yaw=0.3)
    np.random.seed(20)
    with pytest.raises(ValueError):
        PP.aug_method_map['dilute_background'](pts, [box])
    after = np.random.uniform()
    np.random.seed(20)
    assert after == np.random.uniform()    # raised before the jitter draw


def test_registry_keys_and_the_entry_left_out():
    from pointgnn_amd import preprocess as PP
    assert set(PP.aug_method_map) == REGISTRY_KEYS      # the reference's 13
    with pytest.raises(NotImplementedError):
        PP.aug_method_map['random_jitter'](None, None)
    for key in REGISTRY_KEYS - {'random_jitter'}:
        # a body, not the raising stand-in
        assert PP.aug_method_map[key].__name__ == key


def test_attributes_may_be_absent():
    """attr=None passes through the methods that remove points."""
    import torch
    from pointgnn_amd import preprocess as PP
    from pointgnn_amd.kitti_dataset import Points
    xyz, _, labels = scene(21, None, 700)
    pts = Points(xyz=torch.from_numpy(xyz).cuda(), attr=None)
    np.random.seed(21)
    out, _ = PP.random_drop(pts, labels, drop_prob=0.5)
    np.random.seed(21)
    keep = np.random.uniform(size=len(xyz)) > 0.5
    assert out.attr is None
    assert np.array_equal(out.xyz.cpu().numpy(), xyz[keep].astype(np.float64))
    out, kept = PP.remove_background(pts, labels)
    assert out.attr is None and 0 < out.xyz.shape[0] < len(xyz)


# ---- the device entries ------------------------------------------------------

def _compact(xyz, attr, keep, drop, capacity, sentinel_rows=0):
    """pgnn_points_compact_f64 through the binding -> (out_xyz, out_attr,
    count); the output buffers hold `capacity + sentinel_rows` rows of -7."""
    import torch
    from pointgnn_amd import _lib
    lib = _lib.load()
    n = len(xyz)
    a = attr.shape[1] if attr is not None else 0
    dev = torch.device("cuda")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev) \
        if x is not None else None                         # noqa: E731
    d_xyz, d_attr, d_keep, d_drop = t(xyz), t(attr), t(keep), t(drop)
    rows = capacity + sentinel_rows
    out_xyz = torch.full((rows, 3), -7.0, dtype=torch.float64, device=dev)
    out_attr = torch.full((rows, a), -7.0, dtype=torch.float32, device=dev) \
        if attr is not None else None
    ws_bytes = lib.pgnn_points_compact_workspace_bytes(n)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    count = torch.full((1,), -1, dtype=torch.int32, device=dev)
    _lib.check(lib.pgnn_points_compact_f64(
        _lib.ptr(d_xyz), _lib.ptr(d_attr), a, n, _lib.ptr(d_keep),
        _lib.ptr(d_drop), _lib.ptr(ws), ws_bytes, _lib.ptr(out_xyz),
        _lib.ptr(out_attr), capacity, _lib.ptr(count), _lib.stream_ptr()),
        "pgnn_points_compact_f64")
    return (out_xyz.cpu().numpy(),
            out_attr.cpu().numpy() if out_attr is not None else None,
            int(count.item()))


def _masks(n, rng):
    i = np.arange(n)
    first, last = np.zeros(n, bool), np.zeros(n, bool)
    first[0], last[-1] = True, True
    return {
        "all": np.ones(n, bool), "none": np.zeros(n, bool), "first": first,
        "last": last, "alternating": i % 2 == 0,
        "random": rng.uniform(size=n) < 0.5,
        # whole 256-point blocks (and whole waves of the others) empty
        "empty_blocks": ((i // 256) % 2 == 1) & ((i // 64) % 4 != 2)
        if n > 256 else (i // 64) % 2 == 1,
    }


@pytest.mark.parametrize("attr_width", [None, 1, 4])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025, 5000])
def test_points_compact_equals_boolean_indexing(n, attr_width):
    rng = np.random.default_rng(n)
    xyz = rng.normal(size=(n, 3))
    attr = rng.uniform(size=(n, attr_width)).astype(np.float32) \
        if attr_width else None
    for tag, keep in _masks(n, rng).items():
        kept = int(keep.sum())
        got_xyz, got_attr, count = _compact(xyz, attr, keep.astype(np.int32),
                                            None, kept)
        assert count == kept, tag
        assert np.array_equal(got_xyz, xyz[keep]), tag
        if attr is not None:
            assert np.array_equal(got_attr, attr[keep]), tag
    # the second mask: keep && !drop in one pass, and !drop alone
    keep, drop = rng.uniform(size=n) < 0.6, rng.uniform(size=n) < 0.3
    for k_mask, m in ((keep, keep & ~drop), (None, ~drop)):
        got_xyz, got_attr, count = _compact(
            xyz, attr, k_mask.astype(np.int32) if k_mask is not None else None,
            drop.astype(np.int32), int(m.sum()))
        assert count == int(m.sum())
        assert np.array_equal(got_xyz, xyz[m])
        if attr is not None:
            assert np.array_equal(got_attr, attr[m])


def test_points_compact_reports_the_count_beyond_capacity():
    n, capacity = 1025, 100
    rng = np.random.default_rng(3)
    xyz = rng.normal(size=(n, 3))
    attr = rng.uniform(size=(n, 4)).astype(np.float32)
    keep = np.arange(n) % 2 == 0
    got_xyz, got_attr, count = _compact(xyz, attr, keep.astype(np.int32), None,
                                        capacity, sentinel_rows=10)
    assert count == int(keep.sum()) == 513
    assert np.array_equal(got_xyz[:capacity], xyz[keep][:capacity])
    assert np.array_equal(got_attr[:capacity], attr[keep][:capacity])
    assert np.all(got_xyz[capacity:] == -7.0)       # nothing past the capacity
    assert np.all(got_attr[capacity:] == -7.0)
    # an empty cloud: the count is zeroed, nothing else happens
    e_xyz, _, count = _compact(np.zeros((0, 3)), None,
                               np.zeros(0, np.int32), None, 0, sentinel_rows=2)
    assert count == 0 and np.all(e_xyz == -7.0)


@pytest.mark.parametrize("n_boxes", [0, 1, 18, 70])
def test_points_in_boxes_is_the_union_of_single_boxes(n_boxes):
    import torch
    from pointgnn_amd import _lib, preprocess as PP
    lib = _lib.load()
    expend = (1.5, 1.3, 1.2)
    xyz = LO.synthetic_vertices(40 + n_boxes, k=5000).astype(np.float64)
    xyz += np.random.default_rng(n_boxes).normal(0, 1e-3, xyz.shape)
    labels = LO.synthetic_labels(41 + n_boxes, xyz, n_boxes=n_boxes)
    d_xyz = torch.from_numpy(xyz).cuda()
    single = np.zeros(len(xyz), bool)
    oracle = np.zeros(len(xyz), bool)
    for label in labels:
        m, _ = PP._in_box(d_xyz, label, expend, want_mask=True)
        single |= m.cpu().numpy() != 0
        oracle |= LO.sel_xyz_in_box3d(label, xyz, expend)
    mask, count = PP._in_boxes(d_xyz, labels, expend)
    mask = mask.cpu().numpy()
    print(n_boxes, "boxes:", int(mask.sum()), "points inside")
    assert set(np.unique(mask)) <= {0, 1}
    assert np.array_equal(mask != 0, single)
    assert np.array_equal(mask != 0, oracle)
    assert int(count.item()) == int(single.sum())
    assert n_boxes == 0 or 0 < single.sum() < len(xyz)
    # `exclude` takes points out of the mask and of the count
    excl = (np.arange(len(xyz)) % 3 == 0).astype(np.int32)
    mask, count = PP._in_boxes(d_xyz, labels, expend,
                               exclude=torch.from_numpy(excl).cuda())
    assert np.array_equal(mask.cpu().numpy() != 0, single & (excl == 0))
    assert int(count.item()) == int((single & (excl == 0)).sum())
    # the count alone (inside = NULL), and an empty cloud
    rec = np.zeros((max(n_boxes, 1), 24))
    for i, label in enumerate(labels):
        rec[i] = PP._box_record(label, expend)
    d_rec = torch.from_numpy(rec).cuda()
    cnt = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    _lib.check(lib.pgnn_points_in_boxes_f64(
        _lib.ptr(d_xyz), len(xyz), _lib.ptr(d_rec), n_boxes, None, None,
        _lib.ptr(cnt), _lib.stream_ptr()), "pgnn_points_in_boxes_f64")
    assert int(cnt.item()) == int(single.sum())
    _lib.check(lib.pgnn_points_in_boxes_f64(
        None, 0, _lib.ptr(d_rec), n_boxes, None, None, _lib.ptr(cnt),
        _lib.stream_ptr()), "pgnn_points_in_boxes_f64")
    assert int(cnt.item()) == 0


# ---- end to end --------------------------------------------------------------

def test_training_sample_with_registry_augmentations(tmp_path):
    """train.fetch_data on KITTI files with rotation, scale, box global
    rotation (which deletes points) and global drop in data_aug_configs:
    features and cloud agree row for row, the targets are the oracle's on the
    returned vertices, one Trainer step is finite."""
    import torch
    from test_ingest_cpu import _write_png_header_only
    from test_gpu_e2e import _velodyne_scan
    from oracle import ingest_oracle as IO
    from pointgnn_amd import (configs, kitti_dataset as KD, preprocess as PP,
                              train, weights)
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
    tcfg = {'data_aug_configs': _configs([
        ("random_rotation_all", dict(method_name='normal', yaw_std=0.39,
                                     expend_factor=(1.0, 1.0, 1.0))),
        ("random_scale_all", dict(method_name='normal', scale_std=0.05)),
        ("random_box_global_rotation", dict(
            max_overlap_num_allowed=100, max_trails=100, method_name='normal',
            yaw_std=0.1, expend_factor=(1.1, 1.1, 1.1))),
        ("random_global_drop", dict(drop_std=0.25))])}
    n_in = int(ds.get_cam_points_in_image_with_rgb(
        0, cfg['downsample_by_voxel_size']).xyz.shape[0])
    np.random.seed(5)
    sample = train.fetch_data(ds, 0, cfg, tcfg)
    input_v, coords, kps, edges, cls, enc, valid = sample
    assert input_v.shape[0] == coords[0].shape[0] < n_in      # points went
    assert input_v.dtype == torch.float32
    # the same augmentation again for the label list fetch_data worked with
    np.random.seed(5)
    pts, labels = PP.get_data_aug(tcfg['data_aug_configs'])(
        ds.get_cam_points_in_image_with_rgb(
            0, cfg['downsample_by_voxel_size']), ds.get_label(0))
    assert torch.equal(PP.finish(pts).xyz, coords[0])
    assert torch.equal(pts.attr[:, :1], input_v)
    level = cfg['model_kwargs']['layer_configs'][-1]['graph_level']
    last = coords[level + 1]
    # label assignment saw the float64 vertices (train.py:100-118): rows of
    # the float64 cloud, which the returned float32 vertices are casts of
    last64 = pts.xyz[kps[0].reshape(-1).long()]
    assert torch.equal(last64.to(torch.float32), last)
    o_cls, o_boxes, o_valid, _ = LO.assign_labels(
        labels, last64.cpu().numpy(), (1.0, 1.0, 1.0), "Car")
    assert np.array_equal(cls.cpu().numpy(), o_cls)
    assert np.array_equal(valid.cpu().numpy(), o_valid)
    assert int((o_cls > 0).sum()) > 0
    assert enc.shape == (len(o_cls), 1, 7)
    assert bool(torch.isfinite(enc).all())
    tr = train.Trainer(cfg, params=weights.init_params(cfg, seed=1),
                       device=last.device)
    out = tr.train_step(sample, num_valid=float(o_valid.sum()))
    assert np.isfinite([out['cls_loss'], out['loc_loss'], out['reg_loss']]).all()
    assert out['num_endpoint'] == len(o_cls)
