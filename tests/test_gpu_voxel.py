"""Voxel-average down-sampling on the device (csrc/voxel_avg.hip):
`pgnn_voxel_average_f32` and `pgnn_kitti_cam_points_voxel_in_image` through
ctypes and through `pointgnn_amd.kitti_dataset`, against
tests/golden/voxel_average.npz (written by the reference's own functions,
tests/golden/make_golden_voxel.py) and against the NumPy evaluation of the
DEFINED summation order in tests/_voxel.py (ascending original index): the
device result equals the latter bit for bit on every row, which is the test of
the order; against the reference the three-way rule of test_voxel_cpu.py
holds.  Reads tests/golden and oracle/ only."""
import copy
import os

import numpy as np
import pytest

import pointgnn_amd  # noqa: F401
from pointgnn_amd import configs
from oracle import ingest_oracle as IO
import _voxel as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fix():
    return V.load_fixture()


@pytest.fixture(scope="module")
def cloud(fix):
    velo, image, cam = V.inputs(fix)
    return velo, image, cam, np.ascontiguousarray(velo[:, [3]])


def _voxel_call(xyz, attr, voxel, capacity=None, n_dev=None, rows=None,
                ws_bytes=None, attr_dim=None, want_lens=True):
    """pgnn_voxel_average_f32 through ctypes -> (rc, xyz, attr, lens, count);
    the outputs keep their whole capacity (filled with a sentinel first).
    rows: the leading dimension handed to the entry (default len(xyz))."""
    import torch
    from pointgnn_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    x = torch.from_numpy(np.ascontiguousarray(xyz, np.float32)).to(dev)
    a = None if attr is None else torch.from_numpy(
        np.ascontiguousarray(attr, np.float32)).to(dev)
    n = int(x.shape[0]) if rows is None else int(rows)
    ad = (0 if a is None else int(a.shape[1])) if attr_dim is None \
        else int(attr_dim)
    cap = n if capacity is None else int(capacity)
    need = int(lib.pgnn_voxel_average_workspace_bytes(max(n, 0), min(ad, 4)))
    wb = need if ws_bytes is None else int(ws_bytes)
    ws = torch.empty((max(need, 1),), dtype=torch.uint8, device=dev)
    o_xyz = torch.full((max(cap, 1), 3), -7.0, dtype=torch.float64, device=dev)
    o_attr = torch.full((max(cap, 1), max(ad, 1)), -7.0, dtype=torch.float64,
                        device=dev)
    o_lens = torch.full((max(cap, 1),), -7, dtype=torch.int32, device=dev)
    count = torch.full((1,), -7, dtype=torch.int32, device=dev)
    nd = None if n_dev is None else torch.tensor([n_dev], dtype=torch.int32,
                                                 device=dev)
    rc = lib.pgnn_voxel_average_f32(
        _lib.ptr(x), _lib.ptr(a), ad, n, _lib.ptr(nd), float(voxel),
        _lib.ptr(ws), wb, _lib.ptr(o_xyz), _lib.ptr(o_attr),
        _lib.ptr(o_lens) if want_lens else None, cap, _lib.ptr(count),
        _lib.stream_ptr())
    torch.cuda.synchronize()
    return (rc, o_xyz.cpu().numpy(), o_attr.cpu().numpy()[:, :max(ad, 1)],
            o_lens.cpu().numpy(), int(count.item()))


def _assert_defined(got, xyz, attr, voxel):
    rc, gx, ga, gl, m = got
    assert rc == 0
    wx, wa, wl, mag = V.defined_voxel_average(xyz, attr, voxel)
    assert m == len(wl)
    assert np.array_equal(gl[:m], wl)
    assert gx.dtype == np.float64 and np.array_equal(gx[:m], wx)
    if attr is not None:
        assert np.array_equal(ga[:m], wa)
    return wx, wa, wl, mag


@pytest.mark.parametrize("voxel", V.VOXELS)
def test_entry_equals_defined_form_and_reference_fixture(fix, cloud, voxel):
    _, _, cam, refl = cloud
    got = _voxel_call(cam, refl, voxel)
    wx, wa, wl, mag = _assert_defined(got, cam, refl, voxel)
    m = got[4]
    # nothing written behind the last row
    assert (got[1][m:] == -7.0).all() and (got[3][m:] == -7).all()
    t = V.tag(voxel)
    V.check_against_reference(voxel, got[1][:m], got[2][:m], wl, mag,
                              fix["lens_" + t], fix["wide_" + t],
                              fix["narrow_sha256_" + t], "device")


def test_wrap_cloud_is_the_reference_bit_for_bit(fix):
    wx, wa = fix["wrap_xyz_in"], fix["wrap_attr_in"]
    rc, gx, ga, gl, m = _voxel_call(wx, wa, 0.01)
    assert rc == 0 and m == len(fix["wrap_xyz"])
    assert np.array_equal(gx[:m], fix["wrap_xyz"])
    assert np.array_equal(ga[:m], fix["wrap_attr"])
    _assert_defined((rc, gx, ga, gl, m), wx, wa, 0.01)


def test_device_count_shuffle_and_determinism(cloud):
    _, _, cam, refl = cloud
    voxel, n = 0.4, len(cam)
    base = _voxel_call(cam, refl, voxel)
    m = base[4]
    # two consecutive calls: the same bits
    again = _voxel_call(cam, refl, voxel)
    for a, b in zip(base[1:4], again[1:4]):
        assert np.array_equal(a, b)
    # the count in device memory, buffers larger than the cloud (rows behind
    # the count hold values that would change every mean if they were read)
    pad = 1000
    big_xyz = np.concatenate([cam, np.full((pad, 3), 1e6, np.float32)])
    big_attr = np.concatenate([refl, np.full((pad, 1), 1e6, np.float32)])
    dyn = _voxel_call(big_xyz, big_attr, voxel, n_dev=n)
    assert dyn[0] == 0 and dyn[4] == m
    for a, b in zip(base[1:4], dyn[1:4]):
        assert np.array_equal(a[:m], b[:m])
    # shuffled input: rows still come out by key, the same voxels; sums of one
    # or two points are order-free, the rest moves within the order bound
    perm = np.random.RandomState(5).permutation(n)
    shuf = _voxel_call(cam[perm], refl[perm], voxel)
    assert shuf[0] == 0 and shuf[4] == m
    assert np.array_equal(shuf[3][:m], base[3][:m])
    lens = base[3][:m]
    narrow = lens <= 2
    assert np.array_equal(shuf[1][:m][narrow], base[1][:m][narrow])
    assert np.array_equal(shuf[2][:m][narrow], base[2][:m][narrow])
    _, _, wl, mag = V.defined_voxel_average(cam, refl, voxel)
    bound = V.order_bound(wl, mag)
    d = np.abs(np.concatenate([shuf[1][:m], shuf[2][:m]], 1) -
               np.concatenate([base[1][:m], base[2][:m]], 1))
    assert (d <= bound).all()
    # and the shuffled call is itself the defined form of the shuffled cloud
    _assert_defined(shuf, cam[perm], refl[perm], voxel)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 20000])
def test_one_voxel_holds_every_point(n):
    rng = np.random.RandomState(n)
    xyz = (rng.uniform(0.0, 1.0, (n, 3)) + [5.0, -3.0, 20.0]).astype(np.float32)
    attr = rng.uniform(0.0, 1.0, (n, 1)).astype(np.float32)
    got = _voxel_call(xyz, attr, 10.0)
    _assert_defined(got, xyz, attr, 10.0)
    assert got[4] == 1 and got[3][0] == n


def test_long_voxels_between_short_ones():
    """Voxels of hundreds to thousands of points that start in the middle of
    a wave's 64 rows, with single points before, between and after them."""
    rng = np.random.RandomState(11)
    parts = [rng.uniform(0.0, 50.0, (3000, 3))]
    for k, c in ((700, 3.3), (64, 17.1), (129, 31.7), (5000, 44.9)):
        parts.append(c + rng.uniform(0.0, 0.05, (k, 3)))
    xyz = np.concatenate(parts).astype(np.float32)
    xyz = xyz[rng.permutation(len(xyz))]
    attr = rng.uniform(0.0, 1.0, (len(xyz), 1)).astype(np.float32)
    got = _voxel_call(xyz, attr, 0.1)
    _, _, wl, _ = _assert_defined(got, xyz, attr, 0.1)
    assert wl.max() >= 600 and (wl == 1).sum() > 1000


def test_attribute_shapes(cloud):
    _, _, cam, refl = cloud
    cam, refl = cam[:5000], refl[:5000]
    # no attributes
    got = _voxel_call(cam, None, 0.8)
    wx, _, wl, _ = V.defined_voxel_average(cam, None, 0.8)
    assert got[0] == 0 and got[4] == len(wl)
    assert np.array_equal(got[1][:len(wl)], wx)
    assert np.array_equal(got[3][:len(wl)], wl)
    # four columns, and no `lens` output
    rng = np.random.RandomState(2)
    attr4 = np.concatenate(
        [refl, rng.uniform(0, 1, (len(cam), 3)).astype(np.float32)], axis=1)
    for ad in (2, 4):
        got = _voxel_call(cam, attr4[:, :ad], 0.8, want_lens=False)
        wx, wa, wl, _ = V.defined_voxel_average(cam, attr4[:, :ad], 0.8)
        assert got[0] == 0 and got[4] == len(wl)
        assert np.array_equal(got[1][:len(wl)], wx)
        assert np.array_equal(got[2][:len(wl)], wa)
        assert (got[3] == -7).all()


def test_capacity_too_small_still_counts(cloud):
    _, _, cam, refl = cloud
    full = _voxel_call(cam, refl, 0.8)
    m = full[4]
    cap = 1000
    got = _voxel_call(cam, refl, 0.8, capacity=cap)
    assert got[0] == 0 and got[4] == m and m > cap
    assert np.array_equal(got[1], full[1][:cap])
    assert np.array_equal(got[2], full[2][:cap])
    assert np.array_equal(got[3], full[3][:cap])


def test_error_returns(cloud):
    from pointgnn_amd import _lib
    lib = _lib.load()
    _, _, cam, refl = cloud
    cam, refl = cam[:1000], refl[:1000]
    for bad in (0.0, -0.4, float("nan"), float("inf"), 1e-60):
        rc = _voxel_call(cam, refl, bad)[0]
        assert rc == _lib.E_INVALID, bad
        assert b"voxel_size" in lib.pgnn_last_error()
    wide = np.zeros((1000, 5), np.float32)
    assert _voxel_call(cam, wide, 0.4, attr_dim=5)[0] == _lib.E_INVALID
    assert b"attr_dim" in lib.pgnn_last_error()
    assert _voxel_call(cam, refl, 0.4, rows=0)[0] == _lib.E_INVALID
    assert b"n_points" in lib.pgnn_last_error()
    need = int(lib.pgnn_voxel_average_workspace_bytes(1000, 1))
    assert need > 0
    assert _voxel_call(cam, refl, 0.4, ws_bytes=need - 256)[0] == \
        _lib.E_WORKSPACE
    assert b"workspace" in lib.pgnn_last_error()
    # the Python surface raises on them
    from pointgnn_amd import kitti_dataset as KD
    with pytest.raises(_lib.PointGnnHipError, match="voxel_size"):
        KD.downsample_by_average_voxel(KD.Points(cam, refl), 0.0)


def test_python_downsample_by_average_voxel(cloud):
    import torch
    from pointgnn_amd import kitti_dataset as KD
    _, _, cam, refl = cloud
    wx, wa, wl, _ = V.defined_voxel_average(cam, refl, 0.4)
    for pts in (KD.Points(cam, refl),
                KD.Points(torch.from_numpy(cam).cuda(),
                          torch.from_numpy(refl).cuda())):
        got = KD.downsample_by_average_voxel(pts, 0.4)
        assert got.xyz.is_cuda and got.xyz.dtype == torch.float64
        assert got.attr.dtype == torch.float64
        assert np.array_equal(got.xyz.cpu().numpy(), wx)
        assert np.array_equal(got.attr.cpu().numpy(), wa)
    got = KD.downsample_by_average_voxel(KD.Points(cam, None), 0.4)
    assert got.attr is None and np.array_equal(got.xyz.cpu().numpy(), wx)


def test_chain_against_reference_fixture(fix, cloud, monkeypatch):
    """get_cam_points_in_image_with_rgb with a voxel size of 0.4: the rows
    that survive the crop are the reference's (same count, same voxels); rows
    of voxels with one or two points bit-identical in all seven columns, the
    others within the order bound; every colour is the image's pixel under
    the row's own projection.  Eager and deferred give the same tensors."""
    import torch
    from pointgnn_amd import kitti_dataset as KD
    velo, image, cam, refl = cloud
    calib = KD.parse_calib(IO.CALIB_LINES)
    pts = KD.cam_points_in_image(velo, calib, image.shape[:2], image=image,
                                 with_rgb=True, downsample_voxel_size=0.4)
    assert pts.xyz.dtype == torch.float64 and pts.attr.dtype == torch.float64
    xyz, attr = pts.xyz.cpu().numpy(), pts.attr.cpu().numpy()
    kept = fix["in_image_kept"]
    print("chain: %d rows in the image, the reference keeps %d"
          % (len(xyz), len(kept)))
    assert xyz.shape == fix["in_image_xyz"].shape and attr.shape[1] == 4
    _, _, wl, mag = V.defined_voxel_average(cam, refl, 0.4)
    lens, mag = wl[kept], mag[kept]
    narrow = lens <= 2
    assert np.array_equal(xyz[narrow], fix["in_image_xyz"][narrow])
    assert np.array_equal(attr[narrow], fix["in_image_attr_rgb"][narrow])
    bound = V.order_bound(lens, mag)
    got4 = np.concatenate([xyz, attr[:, :1]], axis=1)
    want4 = np.concatenate([fix["in_image_xyz"],
                            fix["in_image_attr_rgb"][:, :1]], axis=1)
    assert (np.abs(got4 - want4) <= bound).all()
    img = IO.cam_to_image(xyz, IO.get_calib(IO.CALIB_LINES))
    rgb = image[np.int32(img[:, 1]), np.int32(img[:, 0]), ::-1].astype(
        np.float32) / 255
    assert np.array_equal(attr[:, 1:], rgb.astype(np.float64))
    # deferred: the same tensors; the call itself reads nothing back and
    # waits for nothing (the one count read per frame is result()'s)
    def host_read(*args, **kwargs):
        raise AssertionError("host read / wait in the deferred fetch")
    with monkeypatch.context() as mp:
        for owner, name in ((torch.Tensor, "item"), (torch.Tensor, "cpu"),
                            (torch.Tensor, "tolist"),
                            (torch.cuda, "synchronize"),
                            (torch.cuda.Stream, "synchronize"),
                            (torch.cuda.Event, "synchronize")):
            mp.setattr(owner, name, host_read)
        pend = KD.cam_points_in_image(
            velo, calib, image.shape[:2], image=image, with_rgb=True,
            deferred=True, downsample_voxel_size=0.4)
    assert isinstance(pend, KD.PendingPoints)
    torch.cuda.current_stream().wait_event(pend.event)
    got = pend.result()
    assert torch.equal(got.xyz, pts.xyz) and torch.equal(got.attr, pts.attr)
    # reflectance only
    p1 = KD.cam_points_in_image(velo, calib, image.shape[:2],
                                downsample_voxel_size=0.4)
    assert torch.equal(p1.xyz, pts.xyz)
    assert torch.equal(p1.attr, pts.attr[:, :1])


def test_without_a_voxel_size_nothing_changes(cloud):
    import torch
    from pointgnn_amd import kitti_dataset as KD
    velo, image, _, _ = cloud
    gold = np.load(os.path.join(V.GOLD, "ingest_kitti.npz"))
    calib = KD.parse_calib(IO.CALIB_LINES)
    a = KD.cam_points_in_image(velo, calib, image.shape[:2], image=image,
                               with_rgb=True)
    b = KD.cam_points_in_image(velo, calib, image.shape[:2], image=image,
                               with_rgb=True, downsample_voxel_size=None)
    assert a.xyz.dtype == torch.float32 and b.attr.dtype == torch.float32
    assert torch.equal(a.xyz, b.xyz) and torch.equal(a.attr, b.attr)
    assert np.array_equal(b.attr.cpu().numpy(), gold["attr_rgb"])


def _kitti_tree(tmp_path, n_frames, preset="small"):
    from pointgnn_amd import synthetic as S
    root = str(tmp_path / "kitti")
    S.write_kitti_frames(root, list(range(n_frames)), preset=preset,
                         behind_points=4000)
    return [os.path.join(root, d) for d in ("image_2", "velodyne", "calib")]


def _voxel_config(name="car_auto_T1", method="random"):
    cfg = copy.deepcopy(configs.get_config(name))
    cfg['downsample_by_voxel_size'] = 0.4
    cfg['runtime_graph_gen_kwargs']['downsample_method'] = method
    cfg['runtime_graph_gen_kwargs']['add_rnd3d'] = False
    return cfg


def _read_rows(out_dir, ds):
    rows = {}
    for i in range(ds.num_files):
        with open(os.path.join(out_dir, "data",
                               ds.get_filename(i) + ".txt"), "rb") as f:
            rows[i] = f.read()
    return rows


def test_dataset_methods_and_detect_frame(tmp_path):
    import torch
    from pointgnn_amd import kitti_dataset as KD, run as RUN, weights
    dirs = _kitti_tree(tmp_path, 1)
    ds = KD.KittiDataset(*dirs)
    plain = ds.get_cam_points_in_image_with_rgb(0)
    down = ds.get_cam_points_in_image_with_rgb(0, 0.4)
    assert plain.xyz.dtype == torch.float32 and down.xyz.dtype == torch.float64
    assert down.attr.shape == (down.xyz.shape[0], 4)
    assert down.attr.dtype == torch.float64
    assert bool((down.attr[:, 1:] == 0).all())
    assert 0 < down.xyz.shape[0] < plain.xyz.shape[0]
    d1 = ds.get_cam_points_in_image(0, 0.4)
    assert torch.equal(d1.xyz, down.xyz)
    assert torch.equal(d1.attr, down.attr[:, :1])
    # get_cam_points: the whole scan, no crop
    whole = ds.get_cam_points(0)
    assert whole.xyz.dtype == torch.float32
    assert whole.xyz.shape[0] == ds.get_velo_points(0).xyz.shape[0]
    wd = ds.get_cam_points(0, 0.4)
    want = V.defined_voxel_average(whole.xyz.cpu().numpy(),
                                   whole.attr.cpu().numpy(), 0.4)
    assert np.array_equal(wd.xyz.cpu().numpy(), want[0])
    assert np.array_equal(wd.attr.cpu().numpy(), want[1])
    # run.py's frame: the graph of the down-sampled frame is smaller
    cfg0 = _voxel_config()
    cfg0['downsample_by_voxel_size'] = None
    cfg = _voxel_config()
    params = weights.init_params(cfg, seed=3, bias_scale=0.05)
    model = RUN.build_model(cfg, params=params)
    np.random.seed(1)
    _, st0 = RUN.detect_frame(ds, 0, model, cfg0)
    np.random.seed(1)
    rows, st = RUN.detect_frame(ds, 0, model, cfg)
    assert st['points'].xyz.dtype == torch.float64
    assert torch.equal(st['points'].xyz, down.xyz)
    assert st['coords'][0].shape[0] == down.xyz.shape[0]
    assert st['coords'][0].shape[0] < st0['coords'][0].shape[0]
    assert st['coords'][1].shape[0] <= st0['coords'][1].shape[0]
    assert st['logits'].dtype == torch.float32
    assert bool(torch.isfinite(st['logits']).all())
    # 'center' keypoints on a cloud that is not float32-representable: the
    # existing error, out of this feature's scope
    with pytest.raises(NotImplementedError,
                       match="not float32-representable"):
        RUN.detect_frame(ds, 0, model, _voxel_config(method="center"))


def test_frame_loops_with_a_voxel_size(tmp_path):
    """run_dataset, sequential and pipelined (FramePipeline), with
    downsample_by_voxel_size = 0.4 and 'random' keypoints.  'random' draws
    from NumPy's global RNG, so the two loops' KITTI txt are compared byte for
    byte with the RNG seeded the same before each: on a one-frame run, and on
    a three-frame run with one frame in flight when no frame fell back to the
    sequential path (a fallback draws its keypoints a second time; without
    one both loops draw once per frame, in frame order)."""
    import torch
    from pointgnn_amd import kitti_dataset as KD, run as RUN, weights
    cfg = _voxel_config()
    dirs = _kitti_tree(tmp_path, 3)
    ds = KD.KittiDataset(*dirs)
    params = weights.init_params(cfg, seed=3, bias_scale=0.05)
    outs = {}
    for name, frames, kw in (
            ("seq1", [0], dict(pipelined=False)),
            ("pipe1", [0], dict(pipelined=True, in_flight=1, prefetch=2)),
            ("seq3", None, dict(pipelined=False)),
            ("pipe3", None, dict(pipelined=True, in_flight=1, prefetch=2)),
            ("pipe3x3", None, dict(pipelined=True, in_flight=3, prefetch=2))):
        out = str(tmp_path / name)
        np.random.seed(9)
        td = RUN.run_dataset(ds, cfg, None, out, params=params,
                             frame_indices=frames, **kw)
        torch.cuda.synchronize()
        assert td['frames'] == (1 if frames else 3)
        outs[name] = (out, td)
    for name in ("seq1", "pipe1"):
        with open(os.path.join(outs[name][0], "data",
                               ds.get_filename(0) + ".txt"), "rb") as f:
            outs[name] += (f.read(),)
    assert outs["pipe1"][2] == outs["seq1"][2]
    want = _read_rows(outs["seq3"][0], ds)
    assert sum(len(w) > 1 for w in want.values()) >= 1, "no detections"
    fallbacks = outs["pipe3"][1].get('sequential fallbacks', 0)
    print("three frames, one in flight: %d sequential fallbacks" % fallbacks)
    if fallbacks == 0:
        assert _read_rows(outs["pipe3"][0], ds) == want
    assert len(_read_rows(outs["pipe3x3"][0], ds)) == 3


def test_train_fetch_with_a_voxel_size(tmp_path):
    import torch
    from oracle import labels_oracle as LO
    from pointgnn_amd import kitti_dataset as KD, train
    cfg = copy.deepcopy(configs.get_config("car_auto_T1"))
    cfg['downsample_by_voxel_size'] = 0.4
    assert cfg['graph_gen_kwargs']['downsample_method'] == 'random'
    dirs = _kitti_tree(tmp_path, 1)
    label_dir = tmp_path / "kitti" / "label_2"
    label_dir.mkdir()
    ds0 = KD.KittiDataset(*dirs)
    chain = ds0.get_cam_points_in_image_with_rgb(0, 0.4)
    LO.write_label_file(
        str(label_dir / "000000.txt"),
        LO.synthetic_labels(30, chain.xyz.cpu().numpy().astype(np.float32),
                            n_boxes=10))
    ds = KD.KittiDataset(*dirs, str(label_dir), is_training=True,
                         num_classes=cfg["num_classes"])
    np.random.seed(3)
    sample = train.fetch_data(ds, 0, cfg, {'data_aug_configs': []})
    input_v, coords = sample[0], sample[1]
    assert coords[0].shape[0] == chain.xyz.shape[0]
    assert input_v.shape[0] == chain.xyz.shape[0]
    assert input_v.dtype == torch.float32 and coords[0].dtype == torch.float32
    assert torch.equal(coords[0], chain.xyz.to(torch.float32))
    k = int(coords[-1].shape[0])
    assert sample[4].shape == (k, 1) and sample[5].shape == (k, 1, 7)
