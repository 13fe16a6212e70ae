"""The rasteriser on the device (csrc/render.hip through pointgnn_amd.render
and through the C ABI) against the NumPy restatement of tests/_render.py, whose
cases tests/test_render_cpu.py proves on the CPU.  Every image is compared with
== on every byte; there is no tolerance anywhere."""
import ctypes
import os

import numpy as np
import pytest

import pointgnn_amd  # noqa: F401
from pointgnn_amd import render as R
import _render as RR

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5                  # guard bytes around the image and the workspace
GUARD = 4096


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from pointgnn_amd import _lib
    _lib.load()
    return torch.device("cuda")


def device_image(case, as_tensors=False, dev=None):
    import torch
    args = RR.render_args(case)
    if as_tensors:
        for k in ('points', 'point_colors', 'segments', 'segment_colors',
                  'background'):
            if isinstance(args.get(k), np.ndarray):
                args[k] = torch.from_numpy(np.ascontiguousarray(
                    args[k])).to(dev)
    img = R.render(case['view'], **args)
    assert img.is_cuda and img.dtype == torch.uint8
    return img.cpu().numpy()


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = np.argwhere(np.any(got != want, axis=2))
    assert len(bad) == 0, "%s: %d pixels differ, first (y, x) = %s: %s != %s" % (
        what, len(bad), bad[0].tolist(), got[tuple(bad[0])].tolist(),
        want[tuple(bad[0])].tolist())


# ---- 1. every case on every canvas ---------------------------------------------------
@pytest.mark.parametrize("name", RR.CASE_NAMES)
@pytest.mark.parametrize("canvas", RR.CANVASES, ids=lambda c: "%dx%d" % c)
def test_case(dev, canvas, name):
    case, want = RR.reference(canvas[0], canvas[1], name)
    same(device_image(case), want, name)


@pytest.mark.parametrize("name", ["layers", "bev", "camera",
                                  "segments_thick_each", "points_n257_float32"])
def test_cuda_tensors_go_in_as_numpy_does(dev, name):
    case, want = RR.reference(67, 45, name)
    same(device_image(case, as_tensors=True, dev=dev), want, name)


def test_render_refuses_bad_arguments(dev):
    v = RR.flat_view(8, 8)
    pts = np.zeros((2, 3))
    for kw in (dict(point_size=0), dict(point_size=4), dict(thickness=0),
               dict(thickness=4), dict(point_colors=np.zeros((3, 3), np.uint8)),
               dict(background=np.zeros((8, 9, 3), np.uint8)),
               dict(segments=np.zeros((2, 3, 3))),
               dict(segments=np.zeros((2, 2, 3)),
                    thickness=np.array([1, 4], np.uint8))):
        with pytest.raises(ValueError):
            R.render(v, points=pts, **kw)
    for w, h in ((0, 8), (8, 0), (4097, 8), (8, 4097)):
        with pytest.raises(ValueError):
            R.render(RR.view(v.m, v.d, v.near, w, h), points=pts)


def test_largest_canvas(dev):
    """4096 x 4096: the pixel index times 3 and times 8 stays in range; a
    point in the last pixel, a segment along the last row and column."""
    W = H = 4096
    v = RR.flat_view(W, H)
    pts = np.array([[W - 0.5, H - 0.5, 1.0], [0.5, 0.5, 1.0]])
    seg = np.array([[(0.5, H - 0.5, 1), (W - 2.5, H - 0.5, 1)],
                    [(W - 0.5, 0.5, 1), (W - 0.5, H - 2.5, 1)]])
    got = R.render(v, points=pts, point_colors=(1, 2, 3), segments=seg,
                   segment_colors=(4, 5, 6)).cpu().numpy()
    want = np.zeros((H, W, 3), np.uint8)
    want[H - 1, W - 1] = want[0, 0] = (1, 2, 3)
    want[H - 1, :W - 2] = want[:H - 2, W - 1] = (4, 5, 6)
    assert np.array_equal(got, want)


# ---- 2. colours --------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_colorize(dev, dtype):
    rng = np.random.default_rng(5)
    for vals, lo, hi in ((RR.COLORIZE_VALUES, 0.0, 1.0),
                         (rng.uniform(-3, 3, 257), -2.0, 2.5),
                         (rng.uniform(-3, 3, 65), 2.0, -2.0),
                         (np.zeros(0), 0.0, 1.0)):
        vals = vals.astype(dtype)
        for table in (R.GRAY_TABLE, R.RAMP_TABLE):
            got = R.colorize(vals, lo, hi, table)
            assert got.is_cuda
            assert np.array_equal(got.cpu().numpy(),
                                  RR.colorize(vals, lo, hi, table).reshape(
                                      -1, 3))
    import torch
    lab = torch.tensor([0, 7, 3, 1], device=dev)
    assert np.array_equal(R.class_colors(lab).cpu().numpy(),
                          R.CLASS_COLORS[[0, 7, 3, 1]])


# ---- 3. graph segments -------------------------------------------------------------------
def _graph(n_edges, seed=0):
    rng = np.random.default_rng(seed)
    coords = [rng.normal(size=(40, 3)).astype(np.float32),
              rng.normal(size=(17, 3)).astype(np.float32),
              rng.normal(size=(17, 3)).astype(np.float32)]
    edges = [np.stack([rng.integers(0, 40, n_edges),
                       rng.integers(0, 17, n_edges)], 1).astype(np.int32),
             np.stack([rng.integers(0, 17, n_edges),
                       rng.integers(0, 17, n_edges)], 1).astype(np.int32)]
    return coords, edges


@pytest.mark.parametrize("n_edges", [0, 1, 65])
def test_graph_segments(dev, n_edges):
    import torch
    coords, edges = _graph(n_edges, seed=n_edges)
    mask = np.random.default_rng(9).random(17) < 0.5
    if n_edges:
        mask[edges[0][0, 1]] = mask[edges[1][0, 1]] = True
    keep = np.nonzero(mask)[0]
    for level in (0, 1):
        for m in (None, mask, keep):
            want = RR.graph_segments(coords, edges, level, m)
            got = R.graph_segments(coords, edges, level, m)
            assert got.is_cuda and got.dtype == torch.float32
            assert tuple(got.shape) == want.shape
            assert np.array_equal(got.cpu().numpy().view(np.uint32),
                                  want.view(np.uint32))
            t_coords = [torch.from_numpy(c).to(dev) for c in coords]
            t_edges = [torch.from_numpy(e).to(dev) for e in edges]
            got = R.graph_segments(t_coords, t_edges, level,
                                   None if m is None else
                                   torch.from_numpy(m).to(dev))
            assert np.array_equal(got.cpu().numpy().view(np.uint32),
                                  want.view(np.uint32))


def test_graph_segments_refuses_capacity_form(dev):
    import torch
    from pointgnn_amd import _lib
    coords, edges = _graph(65)
    t_coords = [torch.from_numpy(c).to(dev) for c in coords]
    t_edges = [torch.from_numpy(e).to(dev) for e in edges]
    cnt = _lib.DeviceCount(torch.tensor([10], dtype=torch.int32, device=dev),
                           10)
    _lib.tag_count(t_edges[1], cnt)
    with pytest.raises(ValueError, match="capacity"):
        R.graph_segments(t_coords, t_edges, 1)
    R.graph_segments(t_coords, t_edges, 0)
    _lib.tag_count(t_coords[1], cnt)
    with pytest.raises(ValueError, match="capacity"):
        R.graph_segments(t_coords, t_edges, 0)


def test_graph_segments_index_out_of_range_is_dropped(dev):
    coords, _ = _graph(1)
    e = np.array([[0, 1], [40, 1], [3, -1], [5, 17], [2, 2]], np.int32)
    got = R.graph_segments(coords, e, 0).cpu().numpy()
    assert np.array_equal(got[[0, 4]], RR.graph_segments(coords, e[[0, 4]], 0))
    assert np.all(np.isnan(got[1, 0])) and np.all(np.isnan(got[2, 1]))
    assert np.all(np.isnan(got[3, 1]))
    assert np.array_equal(got[1, 1], coords[1][1])


# ---- 4. the C ABI with guards ------------------------------------------------------------
class Guarded(object):
    """[guard | n bytes | guard] of sentinel bytes on the device."""

    def __init__(self, dev, n):
        import torch
        self.n = n
        self.buf = torch.full((2 * GUARD + n,), SENTINEL, dtype=torch.uint8,
                              device=dev)
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + GUARD)

    def body(self):
        b = self.buf.cpu().numpy()
        assert np.all(b[:GUARD] == SENTINEL), "wrote in front"
        assert np.all(b[GUARD + self.n:] == SENTINEL), "wrote behind"
        return b[GUARD:GUARD + self.n]

    def untouched(self):
        return bool(np.all(self.body() == SENTINEL))


def _host(a):
    return np.ascontiguousarray(a).ctypes.data_as(ctypes.c_void_p)


@pytest.mark.parametrize("name", ["layers", "camera", "bev",
                                  "segments_far_end", "segments_thick_each",
                                  "points_size3"])
@pytest.mark.parametrize("canvas", RR.CANVASES, ids=lambda c: "%dx%d" % c)
def test_entries_write_only_the_image_and_the_workspace(dev, canvas, name):
    import torch
    from pointgnn_amd import _lib
    lib = _lib.load()
    W, H = canvas
    case, want = RR.reference(W, H, name)
    v = case['view']
    T = lambda a, dt: torch.from_numpy(np.array(a, dtype=dt)).to(dev)
    ws_bytes = int(lib.pgnn_render_workspace_bytes(W, H))
    assert ws_bytes >= 8 * W * H and ws_bytes % 256 == 0
    ws, img = Guarded(dev, ws_bytes), Guarded(dev, 3 * W * H)
    stream = _lib.stream_ptr()
    m, d = _host(v.m), _host(v.d)
    assert lib.pgnn_render_clear(W, H, ws.ptr, ws_bytes, stream) == 0
    n = s = 0
    pcol = scol = None
    if case.get('points') is not None:
        pts = T(case['points'], case['points'].dtype)
        n = len(pts)
        pcol = T(RR._layer_colors(case.get('point_colors'), n), np.uint8)
        assert lib.pgnn_render_points(
            _lib.ptr(pts), int(pts.dtype == torch.float64), n, m, d, v.near,
            W, H, case.get('point_size', 1), ws.ptr, ws_bytes, stream) == 0
    if case.get('segments') is not None:
        seg = T(case['segments'], case['segments'].dtype)
        s = len(seg)
        scol = T(RR._layer_colors(case.get('segment_colors'), s), np.uint8)
        th = case.get('thickness', 1)
        th_t = T(th, np.uint8) if isinstance(th, np.ndarray) else None
        assert lib.pgnn_render_segments(
            _lib.ptr(seg), int(seg.dtype == torch.float64), s, m, v.near, W,
            H, _lib.ptr(th_t), 1 if th_t is not None else th, ws.ptr,
            ws_bytes, stream) == 0
    bg = case.get('background')
    bg_t, bg_rgb = None, 0
    if bg is not None and np.asarray(bg).ndim == 3:
        bg_t = T(bg, np.uint8)
    elif bg is not None:
        bg_rgb = bg[0] << 16 | bg[1] << 8 | bg[2]
    assert lib.pgnn_render_resolve(
        W, H, ws.ptr, ws_bytes, _lib.ptr(pcol), n, _lib.ptr(scol), s,
        _lib.ptr(bg_t), bg_rgb, img.ptr, stream) == 0
    torch.cuda.synchronize()
    same(img.body().reshape(H, W, 3), want, name)
    ws.body()                                           # the guards


def test_refusals_enqueue_nothing(dev):
    """PGNN_E_INVALID for a canvas of 0 or 4097, point_size or thickness of 0
    or 4, and null pointers with n > 0; PGNN_E_WORKSPACE for a short
    workspace: the image and the workspace keep their sentinel bytes."""
    import torch
    from pointgnn_amd import _lib
    lib = _lib.load()
    W, H = 64, 48
    v = RR.flat_view(W, H)
    m, d = _host(v.m), _host(v.d)
    ws_bytes = int(lib.pgnn_render_workspace_bytes(W, H))
    ws, img = Guarded(dev, ws_bytes), Guarded(dev, 3 * W * H)
    pts = torch.ones((5, 3), dtype=torch.float64, device=dev)
    seg = torch.ones((5, 2, 3), dtype=torch.float64, device=dev)
    col = torch.ones((5, 3), dtype=torch.uint8, device=dev)
    stream = _lib.stream_ptr()
    P, S, C = _lib.ptr(pts), _lib.ptr(seg), _lib.ptr(col)
    INV, WSP = _lib.E_INVALID, _lib.E_WORKSPACE

    def points(xyz=P, n=5, mm=m, dd=d, near=0.5, w=W, h=H, p=1, wsp=ws.ptr,
               nb=ws_bytes):
        return lib.pgnn_render_points(xyz, 1, n, mm, dd, near, w, h, p, wsp,
                                      nb, stream)

    def segments(sg=S, n=5, mm=m, w=W, h=H, th=None, t=1, wsp=ws.ptr,
                 nb=ws_bytes):
        return lib.pgnn_render_segments(sg, 1, n, mm, 0.5, w, h, th, t, wsp,
                                        nb, stream)

    def resolve(w=W, h=H, wsp=ws.ptr, nb=ws_bytes, pc=C, npc=5, sc=C, nsc=5,
                out=img.ptr):
        return lib.pgnn_render_resolve(w, h, wsp, nb, pc, npc, sc, nsc, None,
                                       0, out, stream)

    for w, h in ((0, H), (W, 0), (4097, H), (W, 4097)):
        assert lib.pgnn_render_workspace_bytes(w, h) == 0
        assert lib.pgnn_render_clear(w, h, ws.ptr, ws_bytes, stream) == INV
        assert points(w=w, h=h) == INV
        assert segments(w=w, h=h) == INV
        assert resolve(w=w, h=h) == INV
    for bad in (0, 4):
        assert points(p=bad) == INV
        assert segments(t=bad) == INV
    assert points(xyz=None) == INV
    assert points(mm=None) == INV and points(dd=None) == INV
    assert points(wsp=None) == INV
    assert points(near=float('inf')) == INV
    assert points(n=-1) == INV and points(n=1 << 30) == INV
    assert segments(sg=None) == INV and segments(mm=None) == INV
    assert segments(wsp=None) == INV and segments(n=-1) == INV
    assert resolve(wsp=None) == INV and resolve(out=None) == INV
    assert resolve(pc=None) == INV and resolve(sc=None) == INV
    assert lib.pgnn_render_clear(W, H, None, ws_bytes, stream) == INV
    assert lib.pgnn_render_clear(W, H, ws.ptr, ws_bytes - 1, stream) == WSP
    assert points(nb=ws_bytes - 1) == WSP
    assert segments(nb=ws_bytes - 1) == WSP
    assert resolve(nb=ws_bytes - 1) == WSP
    assert lib.pgnn_render_colorize(None, 1, 5, 0.0, 1.0, C, C, stream) == INV
    assert lib.pgnn_render_colorize(P, 1, 5, 0.0, 1.0, None, C, stream) == INV
    assert lib.pgnn_render_graph_segments(P, 5, P, 5, None, 2, S,
                                          stream) == INV
    assert lib.pgnn_render_graph_segments(P, 5, P, 5, C, 2, None,
                                          stream) == INV
    torch.cuda.synchronize()
    assert ws.untouched() and img.untouched()
    # zero counts with null pointers are fine and draw nothing
    assert lib.pgnn_render_clear(W, H, ws.ptr, ws_bytes, stream) == 0
    assert points(xyz=None, n=0) == 0 and segments(sg=None, n=0) == 0
    assert resolve(pc=None, npc=0, sc=None, nsc=0) == 0
    torch.cuda.synchronize()
    assert np.all(img.body() == 0) and np.all(ws.body() == 0)


# ---- 5. frames and result directories ---------------------------------------------------------
@pytest.fixture(scope="module")
def kitti(tmp_path_factory, dev):
    """Two synthetic frames with label files and result files made here."""
    from pointgnn_amd import kitti_dataset as KD, synthetic as S
    root = str(tmp_path_factory.mktemp("render_kitti"))
    S.write_kitti_frames(root, [0, 1], preset="small", behind_points=2000)
    label_dir, result_dir = (os.path.join(root, d) for d in
                             ("label_2", "results"))
    os.makedirs(label_dir)
    os.makedirs(result_dir)
    rows = {}
    for seed in (0, 1):
        gt, det = RR.frame_labels(seed)
        RR.write_label_file(os.path.join(label_dir, "%06d.txt" % seed), gt)
        if seed == 0:     # frame 1 has no result file: no detections
            RR.write_label_file(os.path.join(result_dir, "%06d.txt" % seed),
                                det)
        rows[seed] = (gt, det if seed == 0 else [])
    ds = KD.KittiDataset(*(os.path.join(root, d) for d in
                           ("image_2", "velodyne", "calib")),
                         label_dir=label_dir)
    return root, ds, result_dir, rows


_frame_refs = {}


def frame_reference(ds, frame_idx, view_name, rows, color_by='intensity',
                    background=None):
    """render_frame restated: the layers assembled here, drawn by the
    restatement; computed once per (frame, view, colouring)."""
    key = (frame_idx, view_name, color_by, background is not None)
    if key in _frame_refs:
        return _frame_refs[key]
    gt, det = rows[frame_idx]
    pts = ds.get_cam_points_in_image_with_rgb(frame_idx)
    xyz = pts.xyz.cpu().numpy().astype(np.float64)
    if color_by == 'intensity':
        col = RR.colorize(pts.attr[:, 0].cpu().numpy(), 0.0, 1.0, R.GRAY_TABLE)
    else:
        col = RR.colorize(xyz[:, 1], 2.0, -2.0, R.RAMP_TABLE)
    gt = [l for l in gt if l['name'] in R.GT_COLORS]
    segs = [R.label_segments(gt), R.label_segments(det)]
    cols = [np.repeat(np.array([R.GT_COLORS[l['name']] for l in gt],
                               np.uint8).reshape(-1, 3), 12, axis=0),
            np.tile(np.array([(255, 0, 0)], np.uint8), (12 * len(det), 1))]
    if view_name == 'bev':
        v = RR.bev_view((-40, 40), (0, 80), 10.0)
    else:
        h, w = ds._image_shape(frame_idx)
        calib = ds.get_calib(frame_idx)
        v = RR.view(calib['cam_to_image'], (0, 0, 1, 0), 0.1, w, h)
    img = RR.render(v, points=xyz, point_colors=col,
                    segments=np.concatenate(segs),
                    segment_colors=np.concatenate(cols), background=background)
    if view_name == 'camera' and det:
        img = RR.render(RR.view([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1]],
                                (0, 0, 0, 0), 0.5, v.width, v.height),
                        segments=R.rect_segments(det),
                        segment_colors=(0, 255, 0), thickness=2,
                        background=img)
    img.setflags(write=False)
    _frame_refs[key] = img
    return img


@pytest.mark.parametrize("view_name", ["bev", "camera"])
def test_render_frame(kitti, view_name):
    root, ds, result_dir, rows = kitti
    for frame_idx in (0, 1):
        gt, det = rows[frame_idx]
        want = frame_reference(ds, frame_idx, view_name, rows)
        got = R.render_frame(ds, frame_idx, det, gt, view=view_name)
        same(got.cpu().numpy(), want, "%s frame %d" % (view_name, frame_idx))
        assert np.any(want != 0)
    # the boxes are in the picture: ground truth and detection colours
    want = frame_reference(ds, 0, view_name, rows)
    flat = want.reshape(-1, 3)
    for colour in (R.GT_COLORS['Car'], (255, 0, 0)):
        assert np.any(np.all(flat == np.array(colour, np.uint8), axis=1))


def test_render_frame_by_height_over_a_background(kitti):
    root, ds, result_dir, rows = kitti
    h, w = ds._image_shape(0)
    bg = np.random.default_rng(3).integers(0, 256, (h, w, 3)).astype(np.uint8)
    want = frame_reference(ds, 0, 'camera', rows, 'height', bg)
    got = R.render_frame(ds, 0, rows[0][1], rows[0][0], view='camera',
                         color_by='height', background=bg)
    same(got.cpu().numpy(), want, "camera by height")
    with pytest.raises(ValueError):
        R.render_frame(ds, 0, view='side')
    with pytest.raises(ValueError):
        R.render_frame(ds, 0, color_by='class')          # needs stages


@pytest.mark.parametrize("fmt", ["png", "ppm"])
def test_render_results(kitti, tmp_path, fmt):
    root, ds, result_dir, rows = kitti
    out = str(tmp_path / "render")
    paths = R.render_results(ds, result_dir, out, views=('bev', 'camera'),
                             fmt=fmt)
    assert len(paths) == 4
    for frame_idx in (0, 1):
        for view_name in ('bev', 'camera'):
            path = os.path.join(out, view_name,
                                "%06d.%s" % (frame_idx, fmt))
            assert path in paths and os.path.exists(path)
            data = open(path, "rb").read()
            img = RR.decode_png(data) if fmt == 'png' else RR.decode_ppm(data)
            same(img, frame_reference(ds, frame_idx, view_name, rows),
                 os.path.basename(path))
    # one frame, without ground truth
    paths = R.render_results(ds, result_dir, str(tmp_path / "r2"),
                             frame_indices=[1], fmt=fmt, with_gt=False)
    assert [os.path.relpath(p, str(tmp_path / "r2")) for p in paths] == [
        os.path.join("bev", "000001." + fmt)]
    with pytest.raises(ValueError):
        R.render_results(ds, result_dir, out, fmt='jpg')


def test_command_line(kitti, tmp_path):
    root, ds, result_dir, rows = kitti
    out = str(tmp_path / "cli")
    split = str(tmp_path / "split.txt")
    with open(split, "w") as f:
        f.write("000000\n")
    assert R.main([root, result_dir, out, "--view", "bev", "--view", "camera",
                   "--split", split]) == 0
    for view_name in ('bev', 'camera'):
        names = os.listdir(os.path.join(out, view_name))
        assert names == ["000000.png"]
        data = open(os.path.join(out, view_name, names[0]), "rb").read()
        same(RR.decode_png(data), frame_reference(ds, 0, view_name, rows),
             view_name)
    assert R.main([root, result_dir, str(tmp_path / "cli2"), "--ppm"]) == 0
    assert sorted(os.listdir(str(tmp_path / "cli2" / "bev"))) == [
        "000000.ppm", "000001.ppm"]


# ---- 6. the frame loop ----------------------------------------------------------------------
def test_run_dataset_render_dir_and_the_graph_of_a_frame(tmp_path, dev):
    """run_dataset(render_dir=...) writes one image per frame and view and
    leaves the txt files byte-identical to a run without it; render_frame
    with the stages of detect_frame (class colours, the last level's edges
    into the kept vertices) equals the restatement."""
    import torch
    from pointgnn_amd import configs, kitti_dataset as KD, run as RUN
    from pointgnn_amd import synthetic as S, weights
    root = str(tmp_path / "kitti")
    S.write_kitti_frames(root, [0, 1], preset="tiny", behind_points=500)
    ds = KD.KittiDataset(*(os.path.join(root, d) for d in
                           ("image_2", "velodyne", "calib")))
    cfg = configs.get_config("car_auto_T1")
    params = weights.init_params(cfg, seed=3, bias_scale=0.05)
    plain, drawn = str(tmp_path / "plain"), str(tmp_path / "drawn")
    RUN.run_dataset(ds, cfg, None, plain, params=params, pipelined=False)
    td = RUN.run_dataset(ds, cfg, None, drawn, params=params, pipelined=False,
                         render_dir=str(tmp_path / "img"),
                         render_views=('bev', 'camera'))
    assert td['render'] > 0
    from pointgnn_amd import kitti_eval
    for i in (0, 1):
        name = ds.get_filename(i) + ".txt"
        a = open(os.path.join(plain, "data", name), "rb").read()
        assert a == open(os.path.join(drawn, "data", name), "rb").read()
        det = kitti_eval.read_result_file(os.path.join(drawn, "data", name))
        for view_name in ('bev', 'camera'):
            path = os.path.join(str(tmp_path / "img"), view_name,
                                ds.get_filename(i) + ".png")
            img = RR.decode_png(open(path, "rb").read())
            got = R.render_frame(ds, i, det, None, view=view_name)
            assert np.array_equal(img, got.cpu().numpy())
    # the graph of frame 0
    model = RUN.build_model(cfg, params=params)
    rows, st = RUN.detect_frame(ds, 0, model, cfg)
    got = R.render_frame(ds, 0, rows, None, view='bev', stages=st,
                         color_by='class', show_graph=True).cpu().numpy()
    xyz = st['points'].xyz.cpu().numpy().astype(np.float64)
    verts = st['coords'][-1].cpu().numpy().astype(np.float64)
    labels = np.argmax(st['probs'].cpu().numpy(), axis=1)
    vcol = R.CLASS_COLORS[labels]
    pcol = RR.colorize(st['points'].attr[:, 0].cpu().numpy(), 0.0, 1.0,
                       R.GRAY_TABLE)
    nc = st['probs'].shape[1]
    kept = (st['candidate_indices'].cpu().numpy()[
        st['nms_indices'].cpu().numpy()] // nc)
    coords = [c.cpu().numpy() for c in st['coords']]
    edges = [e.cpu().numpy() for e in st['edges']]
    level = len(edges) - 1
    e = edges[level][np.isin(edges[level][:, 1], kept)]      # run.py:341-343
    gseg = RR.graph_segments(coords, e, level).astype(np.float64)
    bseg = R.label_segments(rows)
    print("frame 0: %d points, %d vertices, %d of %d edges kept, %d rows" % (
        len(xyz), len(verts), len(e), len(edges[level]), len(rows)))
    want = RR.render(
        RR.bev_view((-40, 40), (0, 80), 10.0),
        points=np.concatenate([verts, xyz]),
        point_colors=np.concatenate([vcol, pcol]),
        segments=np.concatenate([gseg, bseg]),
        segment_colors=np.concatenate([
            vcol[e[:, 1]], np.tile(np.array([(255, 0, 0)], np.uint8),
                                   (len(bseg), 1))]))
    same(got, want, "graph of frame 0")
    assert len(rows) > 0 and len(e) > 0
