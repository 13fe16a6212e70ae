"""PNG decode on the device (pointgnn_amd.png, pgnn_png_unfilter): every case
of tests/_png_cases.py and the libpng-written golden file bit for bit, and the
places the decoded image goes -- the colour columns of the KITTI ingest, the
frame loop's loader thread, the camera view's background."""
import os

import numpy as np
import pytest

import pointgnn_amd  # noqa: F401
from oracle import ingest_oracle as IO
import _png_cases as PC

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = PC.cases()
CASE_ORDERS = [(c, o) for c in CASES for o in c.orders]


@pytest.mark.parametrize("case,order", CASE_ORDERS,
                         ids=["%s-%s" % (c.name, o) for c, o in CASE_ORDERS])
def test_read_png_cases(case, order):
    import torch
    from pointgnn_amd import png as P
    got = P.read_png(PC.case_bytes(case), order=order)
    assert got.is_cuda and got.dtype == torch.uint8
    want = PC.expected(case, order)
    assert tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy(), want)


def test_read_png_golden_file():
    from pointgnn_amd import png as P
    want = np.load(os.path.join(GOLD, "png_adaptive.npy"))
    path = os.path.join(GOLD, "png_adaptive.png")
    assert np.array_equal(P.read_png(path, order='rgb').cpu().numpy(), want)
    assert np.array_equal(P.read_png(path).cpu().numpy(), want[:, :, ::-1])
    with open(path, "rb") as f:
        assert np.array_equal(P.read_png(f.read(), 'rgb').cpu().numpy(), want)
    with pytest.raises(ValueError):
        P.read_png(path, order='gbr')


def test_read_png_on_a_side_stream():
    import torch
    from pointgnn_amd import png as P
    by_name = {c.name: c for c in CASES}
    for name in ("h600_w100", "palette_beyond"):
        case = by_name[name]
        data = PC.case_bytes(case)
        first = P.read_png(data)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            second = P.read_png(data)
        side.synchronize()
        assert torch.equal(first, second)
        assert np.array_equal(second.cpu().numpy(), PC.expected(case, 'bgr'))


def test_unfilter_checks_its_arguments():
    import torch
    from pointgnn_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    w, h = 5, 3
    raw = torch.zeros(h * (1 + 3 * w), dtype=torch.uint8, device=dev)
    img = torch.full((h, w, 3), 7, dtype=torch.uint8, device=dev)
    pal = torch.zeros((4, 3), dtype=torch.uint8, device=dev)
    ws_bytes = int(lib.pgnn_png_unfilter_workspace_bytes(w, h))
    assert ws_bytes > 0
    assert lib.pgnn_png_unfilter_workspace_bytes(0, 5) == 0
    assert lib.pgnn_png_unfilter_workspace_bytes(5, -1) == 0
    assert lib.pgnn_png_unfilter_workspace_bytes(1 << 61, 16) == 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)

    def call(width=w, height=h, color_type=2, palette=None, entries=0,
             raw_t=raw, ws_t=ws, nbytes=ws_bytes, img_t=img):
        return lib.pgnn_png_unfilter(
            _lib.ptr(raw_t), width, height, color_type, _lib.ptr(palette),
            entries, 1, _lib.ptr(ws_t), nbytes, _lib.ptr(img_t),
            _lib.stream_ptr())

    bad = [dict(width=0), dict(height=0), dict(width=-3), dict(color_type=1),
           dict(color_type=5), dict(color_type=7), dict(raw_t=None),
           dict(img_t=None), dict(ws_t=None), dict(color_type=3),
           dict(color_type=3, palette=pal, entries=0),
           dict(color_type=3, palette=pal, entries=257),
           dict(width=1 << 61, height=16)]
    for kw in bad:
        assert call(**kw) == _lib.E_INVALID, kw
        assert b"pgnn_png_unfilter" in lib.pgnn_last_error(), kw
    assert call(nbytes=ws_bytes - 1) == _lib.E_WORKSPACE
    assert b"pgnn_png_unfilter" in lib.pgnn_last_error()
    torch.cuda.synchronize()
    assert bool((img == 7).all()), "a rejected call wrote the image"
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((img == 0).all())


# ---- the dataset -------------------------------------------------------------
def _write_rgb_png(path, bgr, seed):
    """`bgr` (cv2's layout) stored as the RGB file cv2.imread would read it
    from, filters mixed."""
    ft = np.random.default_rng(seed).integers(0, 5, bgr.shape[0])
    with open(path, "wb") as f:
        f.write(PC.png_bytes(bgr[:, :, ::-1], 2, ft))


@pytest.fixture(scope="module")
def kitti_dir(tmp_path_factory):
    root = tmp_path_factory.mktemp("kitti_png")
    for d in ("image_2", "velodyne", "calib"):
        (root / d).mkdir()
    IO.synthetic_velo_scan(0, n=60000).tofile(
        str(root / "velodyne" / "000000.bin"))
    (root / "calib" / "000000.txt").write_text("".join(IO.CALIB_LINES))
    _write_rgb_png(str(root / "image_2" / "000000.png"),
                   IO.synthetic_image(0), 0)
    return root


def _dataset(root, **kw):
    from pointgnn_amd import kitti_dataset as KD
    return KD.KittiDataset(str(root / "image_2"), str(root / "velodyne"),
                           str(root / "calib"), **kw)


def test_dataset_decodes_its_images(kitti_dir):
    import torch
    fix = np.load(os.path.join(GOLD, "ingest_kitti.npz"))
    image = IO.synthetic_image(0)
    ds = _dataset(kitti_dir, decode_images=True)
    got = ds.get_image(0)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), image)
    pts = ds.get_cam_points_in_image_with_rgb(0)
    assert np.array_equal(pts.attr.cpu().numpy(), fix["attr_rgb"])
    assert float(pts.attr[:, 1:].abs().sum()) > 0
    # deferred: the decode and the crop on the caller's stream
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        pending = ds.get_cam_points_in_image_with_rgb(0, deferred=True)
    torch.cuda.current_stream().wait_event(pending.event)
    later = pending.result()
    assert torch.equal(later.xyz, pts.xyz) and torch.equal(later.attr, pts.attr)
    # voxel-averaged: the same rows as with the image passed in
    down = ds.get_cam_points_in_image_with_rgb(0, 0.4)
    want = _dataset(kitti_dir).get_cam_points_in_image_with_rgb(
        0, 0.4, image=image)
    assert down.attr.shape[1] == 4 and torch.equal(down.attr, want.attr)
    assert torch.equal(down.xyz, want.xyz)
    # an image passed in still wins over the file
    other = np.ascontiguousarray(image[:, :, ::-1])
    a = ds.get_cam_points_in_image_with_rgb(0, image=other)
    assert np.array_equal(a.attr.cpu().numpy()[:, 1:],
                          fix["attr_rgb"][:, :0:-1])
    # the default constructor: zero colour columns, as before
    plain = _dataset(kitti_dir).get_cam_points_in_image_with_rgb(0)
    assert plain.attr.shape == pts.attr.shape
    assert torch.equal(plain.attr[:, :1], pts.attr[:, :1])
    assert float(plain.attr[:, 1:].abs().sum()) == 0.0
    assert torch.equal(plain.xyz, pts.xyz)


def test_frame_loop_decodes_on_the_loader_thread(tmp_path):
    """An 'i' config reads no colour: run_dataset writes the same files with
    and without decode_images=True, the decode running in FramePipeline's
    loader thread on its stream."""
    from test_gpu_e2e import _velodyne_scan
    from pointgnn_amd import configs, run as RUN, weights
    cfg = configs.get_config("car_auto_T1")
    assert cfg["input_features"] == "i"
    for d in ("image_2", "velodyne", "calib"):
        (tmp_path / d).mkdir()
    rng = np.random.default_rng(8)
    for i, seed in enumerate((21, 5)):
        name = "%06d" % i
        _velodyne_scan(seed).tofile(str(tmp_path / "velodyne" / (name + ".bin")))
        (tmp_path / "calib" / (name + ".txt")).write_text(
            "".join(IO.CALIB_LINES))
        _write_rgb_png(str(tmp_path / "image_2" / (name + ".png")),
                       rng.integers(0, 256, (375, 1242, 3)).astype(np.uint8), i)
    params = weights.init_params(cfg, seed=3, bias_scale=0.05)
    files = {}
    for decode in (False, True):
        ds = _dataset(tmp_path, decode_images=decode)
        out = str(tmp_path / ("out%d" % decode))
        td = RUN.run_dataset(ds, cfg, None, out, params=params)
        assert td['frames'] == 2
        files[decode] = [open(os.path.join(out, "data", "%06d.txt" % i),
                              "rb").read() for i in range(2)]
    assert files[True] == files[False]
    assert sum(len(f) > 1 for f in files[True]) >= 1, "no detections at all"
    # and the colour is there for a config that would read it
    pts = _dataset(tmp_path, decode_images=True
                   ).get_cam_points_in_image_with_rgb(0)
    assert float(pts.attr[:, 1:].abs().sum()) > 0


# ---- the camera view's background ---------------------------------------------
def _read_ppm(path):
    with open(path, "rb") as f:
        data = f.read()
    magic, size, maxval, body = data.split(b"\n", 3)
    w, h = (int(t) for t in size.split())
    assert magic == b"P6" and maxval == b"255"
    return np.frombuffer(body, dtype=np.uint8).reshape(h, w, 3)


def test_camera_view_over_the_decoded_image(kitti_dir, tmp_path):
    from pointgnn_amd import render as R
    ds = _dataset(kitti_dir)
    result_dir = tmp_path / "results"
    result_dir.mkdir()
    (result_dir / "000000.txt").write_text(
        "Car -1 -1 0 500.0 150.0 640.0 230.0 1.5 1.6 4.0 1.0 1.6 15.0 0.3 "
        "0.9 \n")
    from pointgnn_amd import kitti_eval
    det = kitti_eval.read_result_file(str(result_dir / "000000.txt"))
    assert len(det) == 1
    rgb = np.ascontiguousarray(IO.synthetic_image(0)[:, :, ::-1])
    reader = R.image_background(ds)
    assert np.array_equal(reader(0).cpu().numpy(), rgb)
    out = str(tmp_path / "render")
    paths = R.render_results(ds, str(result_dir), out, views=('camera',),
                             fmt='ppm', background_reader=reader)
    assert paths == [os.path.join(out, "camera", "000000.ppm")]
    got = _read_ppm(paths[0])
    want = R.render_frame(ds, 0, det, None, view='camera', background=rgb)
    assert np.array_equal(got, want.cpu().numpy())
    black = R.render_frame(ds, 0, det, None, view='camera').cpu().numpy()
    assert not np.array_equal(got, black)
    assert np.mean(np.all(got == rgb, axis=2)) > 0.5   # mostly photograph
    # the command line
    cli = str(tmp_path / "cli")
    assert R.main([str(kitti_dir), str(result_dir), cli, "--view", "camera",
                   "--ppm", "--image-background"]) == 0
    assert np.array_equal(_read_ppm(os.path.join(cli, "camera", "000000.ppm")),
                          got)
    assert R.main([str(kitti_dir), str(result_dir), cli + "0", "--view",
                   "camera", "--ppm"]) == 0
    assert np.array_equal(
        _read_ppm(os.path.join(cli + "0", "camera", "000000.ppm")), black)
