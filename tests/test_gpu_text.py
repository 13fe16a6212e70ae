"""Text on the device (csrc/render.hip: pgnn_render_text through
pointgnn_amd.render.draw_text and through the C ABI) against the NumPy
restatement of tests/_text_cases.py, whose cases tests/test_text_cases_cpu.py
proves on the CPU; the scores and names render_frame(text=True) writes, and the
precision/recall plots of kitti_eval.  Every image is compared with == on every
byte; there is no tolerance anywhere."""
import ctypes
import os

import numpy as np
import pytest

import pointgnn_amd  # noqa: F401
from pointgnn_amd import render as R
import _text_cases as TC

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


@pytest.fixture(scope="module")
def table():
    return R.font_table()


_refs = {}


def reference(name, table):
    if name not in _refs:
        img = TC.reference(TC.CASES[name], table)
        img.setflags(write=False)
        _refs[name] = img
    return _refs[name]


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = np.argwhere(np.any(got != want, axis=2))
    assert len(bad) == 0, "%s: %d pixels differ, first (y, x) = %s: %s != %s" % (
        what, len(bad), bad[0].tolist(), got[tuple(bad[0])].tolist(),
        want[tuple(bad[0])].tolist())


class Guarded(object):
    """[guard | n bytes | guard] of sentinel bytes on the device."""

    def __init__(self, dev, n):
        import torch
        self.n = n
        self.buf = torch.full((2 * GUARD + n,), SENTINEL, dtype=torch.uint8,
                              device=dev)
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + GUARD)

    def middle(self):
        return self.buf[GUARD:GUARD + self.n]

    def body(self):
        b = self.buf.cpu().numpy()
        assert np.all(b[:GUARD] == SENTINEL), "wrote in front"
        assert np.all(b[GUARD + self.n:] == SENTINEL), "wrote behind"
        return b[GUARD:GUARD + self.n]

    def untouched(self):
        return bool(np.all(self.body() == SENTINEL))


def guarded_image(dev, background):
    """The image as the middle slice of a larger sentinel buffer."""
    import torch
    h, w = background.shape[:2]
    g = Guarded(dev, 3 * w * h)
    image = g.middle().view(h, w, 3)
    image.copy_(torch.from_numpy(background).to(dev))
    return g, image


def draw_case(dev, case, image):
    import torch
    scales = case['scales']
    if not isinstance(scales, int):      # also the illegal values: no check
        scales = torch.tensor(scales, dtype=torch.uint8, device=dev)
    return R.draw_text(image, case['strings'],
                       np.array(case['anchors'], dtype=np.int64).reshape(-1, 2),
                       colors=np.array(case['colors'], dtype=np.uint8),
                       scale=scales,
                       plate=None if case['plates'] is None else
                       np.array(case['plates'], dtype=np.uint8), anchor='tl')


# ---- 1. every case -------------------------------------------------------------------
@pytest.mark.parametrize("name", TC.CASE_NAMES)
def test_case(dev, table, name):
    case = TC.CASES[name]
    g, image = guarded_image(dev, TC.background(case))
    out = draw_case(dev, case, image)
    assert out is image                                   # in place
    same(g.body().reshape(case['height'], case['width'], 3),
         reference(name, table), name)


def _abi_arguments(dev, case):
    import torch
    T = lambda a, dt: torch.from_numpy(np.array(a, dtype=dt)).to(dev)
    n = len(case['strings'])
    data = b''.join(case['strings'])
    offsets = np.zeros(n + 1, np.int32)
    offsets[1:] = np.cumsum([len(s) for s in case['strings']])
    chars = T(np.frombuffer(data + b'\0', dtype=np.uint8), np.uint8)
    scales = case['scales']
    return dict(
        chars=chars, offsets=T(offsets, np.int32),
        anchors=T(np.array(case['anchors'], np.int64).reshape(-1, 2), np.int32),
        scales=None if isinstance(scales, int) else T(scales, np.uint8),
        scale=scales if isinstance(scales, int) else 77,    # then ignored
        colors=T(np.array(case['colors']).reshape(-1, 3), np.uint8),
        plates=None if case['plates'] is None else T(case['plates'], np.uint8),
        n=n)


@pytest.mark.parametrize("name", [
    "alphabet_scales_2_3", "scale_illegal", "clip_corner_plate",
    "clip_corner_far_plate", "far_anchors", "long_5000",
    "long_5000_scale_4_plate", "canvas_1x1", "canvas_4096x1", "canvas_1x4096",
    "overlap_3_plates", "overlap_300", "bytes_outside", "empty_between",
    "plates_each"])
def test_entry_writes_only_the_image_and_the_workspace(dev, table, name):
    import torch
    from pointgnn_amd import _lib
    lib = _lib.load()
    case = TC.CASES[name]
    W, H = case['width'], case['height']
    a = _abi_arguments(dev, case)
    ws_bytes = int(lib.pgnn_render_text_workspace_bytes(W, H))
    assert ws_bytes >= 4 * W * H and ws_bytes % 256 == 0
    ws = Guarded(dev, ws_bytes)
    g, image = guarded_image(dev, TC.background(case))
    P = _lib.ptr
    assert lib.pgnn_render_text(
        g.ptr, W, H, P(a['chars']), P(a['offsets']), a['n'], P(a['anchors']),
        P(a['scales']), a['scale'], P(a['colors']), len(case['colors']),
        P(a['plates']), 0 if case['plates'] is None else len(case['plates']),
        ws.ptr, ws_bytes, _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    same(g.body().reshape(H, W, 3), reference(name, table), name)
    keys = ws.body()[:4 * W * H].view(np.uint32).reshape(H, W)    # the guards
    # the key plane: (string + 1) << 1 | is_glyph, 0 where nobody drew
    changed = np.any(reference(name, table) != TC.background(case), axis=2)
    assert np.all(keys[changed] != 0)
    assert int(keys.max()) >> 1 <= a['n']


def test_malformed_offsets_drop_their_strings(dev, table):
    """Descending or negative offsets, or an end beyond offsets[n]: those
    strings are dropped on the device, the others drawn."""
    import torch
    from pointgnn_amd import _lib
    lib = _lib.load()
    W, H = 60, 12
    strings = [b'ab', b'cd', b'ef', b'gh', b'ij']
    anchors = [(1, 2), (13, 2), (25, 2), (37, 2), (49, 2)]
    bg = np.random.default_rng(2).integers(0, 256, (H, W, 3)).astype(np.uint8)
    T = lambda a, dt: torch.from_numpy(np.array(a, dtype=dt)).to(dev)
    chars = T(np.frombuffer(b''.join(strings), np.uint8), np.uint8)
    col = T([(9, 8, 7)], np.uint8)
    ws_bytes = int(lib.pgnn_render_text_workspace_bytes(W, H))
    for bad in ([0, 2, 1, 6, 8, 10], [0, 2, -4, 6, 8, 10],
                [0, 2, 4, 6, 12, 10]):
        # which strings a table keeps, restated: 0 <= begin < end <= last
        kept = [j for j in range(5) if 0 <= bad[j] < bad[j + 1] <= bad[-1]]
        ws = Guarded(dev, ws_bytes)
        g, image = guarded_image(dev, bg)
        off_t, anc_t = T(bad, np.int32), T(anchors, np.int32)
        assert lib.pgnn_render_text(
            g.ptr, W, H, _lib.ptr(chars), _lib.ptr(off_t), 5, _lib.ptr(anc_t),
            None, 1, _lib.ptr(col), 1, None, 0, ws.ptr, ws_bytes,
            _lib.stream_ptr()) == 0
        torch.cuda.synchronize()
        data = b''.join(strings)
        want = TC.draw_text_reference(
            bg, [data[bad[j]:bad[j + 1]] for j in kept],
            [anchors[j] for j in kept], 1, [(9, 8, 7)], None, table)
        same(g.body().reshape(H, W, 3), want, str(bad))
        assert 0 < len(kept) < 5
        ws.body()


def test_refusals_enqueue_nothing(dev):
    """PGNN_E_INVALID and PGNN_E_WORKSPACE leave a sentinel image and
    workspace as they were."""
    import torch
    from pointgnn_amd import _lib
    lib = _lib.load()
    W, H = 64, 48
    ws_bytes = int(lib.pgnn_render_text_workspace_bytes(W, H))
    ws, img = Guarded(dev, ws_bytes), Guarded(dev, 3 * W * H)
    a = _abi_arguments(dev, TC.CASES['plates_each'])
    P = _lib.ptr
    stream = _lib.stream_ptr()
    INV, WSP = _lib.E_INVALID, _lib.E_WORKSPACE

    def text(image=img.ptr, w=W, h=H, chars=P(a['chars']),
             offsets=P(a['offsets']), n=3, anchors=P(a['anchors']),
             scales=None, scale=1, colors=P(a['colors']), n_colors=3,
             plates=P(a['plates']), n_plates=3, wsp=ws.ptr, nb=ws_bytes):
        return lib.pgnn_render_text(image, w, h, chars, offsets, n, anchors,
                                    scales, scale, colors, n_colors, plates,
                                    n_plates, wsp, nb, stream)
    for w, h in ((0, H), (W, 0), (4097, H), (W, 4097)):
        assert text(w=w, h=h) == INV
    for s in (0, 5):
        assert text(scale=s) == INV
    assert text(n=-1) == INV and text(n=1 << 30) == INV
    assert text(n_colors=2) == INV and text(n_colors=0) == INV
    assert text(n_plates=2) == INV
    assert text(colors=None) == INV and text(plates=None) == INV
    assert text(image=None) == INV and text(offsets=None) == INV
    assert text(anchors=None) == INV and text(wsp=None) == INV
    assert text(nb=ws_bytes - 1) == WSP
    assert text(n=0, n_colors=1, n_plates=0) == 0          # nothing to draw
    torch.cuda.synchronize()
    assert ws.untouched() and img.untouched()
    assert text() == 0                                      # and the good call
    torch.cuda.synchronize()
    assert not img.untouched()


def test_draw_text_refuses_bad_arguments(dev):
    import torch
    img = torch.zeros((8, 16, 3), dtype=torch.uint8, device=dev)
    ok = dict(strings=['a', 'b'], anchors=[(1, 8), (7, 8)])
    R.draw_text(img, **ok)
    for bad in (dict(scale=0), dict(scale=5), dict(scale=[1, 5]),
                dict(scale=[1, 1, 1]), dict(colors=np.zeros((3, 3), np.uint8)),
                dict(plate=np.zeros((3, 3), np.uint8)), dict(anchor='br'),
                dict(anchors=[(1, 8)]), dict(anchors=[(1, 8), (2 ** 31, 8)]),
                dict(anchors=[(1.5, 8), (2, 8)]), dict(strings='ab'),
                dict(strings=['a', 7]), dict(colors=(256, 0, 0))):
        with pytest.raises(ValueError):
            R.draw_text(img, **dict(ok, **bad))
    for image in (img.cpu(), img.to(torch.float32), img[:, :, :2], img[:, ::2],
                  np.zeros((8, 16, 3), np.uint8)):
        with pytest.raises(ValueError):
            R.draw_text(image, **ok)


def test_anchor_bl_is_tl_shifted_by_the_cell_height(dev, table):
    import torch
    bg = np.random.default_rng(1).integers(0, 256, (40, 90, 3)).astype(np.uint8)
    strings = ['C | 0.912', 'Pg', 'x']
    anchors = np.array([(3, 12), (30, 38), (70, 2)])
    scales = [1, 3, 2]
    want = TC.draw_text_reference(
        bg, [s.encode() for s in strings],
        [(x, y - 7 * s) for (x, y), s in zip(anchors.tolist(), scales)],
        scales, [(1, 2, 3)], [(4, 5, 6)], table)
    for scale in (scales, torch.tensor(scales, dtype=torch.uint8, device=dev)):
        bl = R.draw_text(torch.from_numpy(bg).to(dev), strings, anchors,
                         colors=(1, 2, 3), scale=scale, plate=(4, 5, 6))
        tl = R.draw_text(torch.from_numpy(bg).to(dev), strings,
                         anchors - 7 * np.array(scales)[:, None] * [0, 1],
                         colors=(1, 2, 3), scale=scale, plate=(4, 5, 6),
                         anchor='tl')
        same(bl.cpu().numpy(), want, 'bl')
        same(tl.cpu().numpy(), want, 'tl')
    # str is encoded latin-1; what it cannot encode is '?'
    a = R.draw_text(torch.from_numpy(bg).to(dev), ['é€'], [(2, 9)])
    b = R.draw_text(torch.from_numpy(bg).to(dev), [b'\xe9?'], [(2, 9)])
    c = R.draw_text(torch.from_numpy(bg).to(dev), ['??'], [(2, 9)])
    assert torch.equal(a, b) and torch.equal(a, c)


# ---- 2. frames and result directories --------------------------------------------------
def _write_label_file(path, rows):
    keys = ('truncation', 'occlusion', 'alpha', 'xmin', 'ymin', 'xmax', 'ymax',
            'height', 'width', 'length', 'x3d', 'y3d', 'z3d', 'yaw')
    with open(path, 'w') as f:
        for r in rows:
            fields = [r['name']] + [repr(float(r[k])) if k != 'occlusion'
                                    else str(r[k]) for k in keys]
            if 'score' in r:
                fields.append(repr(float(r['score'])))
            f.write(' '.join(fields) + '\n')


@pytest.fixture(scope="module")
def kitti(tmp_path_factory, dev):
    """One synthetic frame with a label file and a result file made here."""
    from pointgnn_amd import kitti_dataset as KD, synthetic as S
    root = str(tmp_path_factory.mktemp("text_kitti"))
    S.write_kitti_frames(root, [0], preset="small", behind_points=500)
    label_dir, result_dir = (os.path.join(root, d) for d in
                             ("label_2", "results"))
    os.makedirs(label_dir)
    os.makedirs(result_dir)
    gt, det = TC.frame_labels()
    _write_label_file(os.path.join(label_dir, "000000.txt"), gt)
    _write_label_file(os.path.join(result_dir, "000000.txt"), det)
    ds = KD.KittiDataset(*(os.path.join(root, d) for d in
                           ("image_2", "velodyne", "calib")),
                         label_dir=label_dir)
    return root, ds, result_dir, gt, det


_frames = {}


def frame_reference(ds, gt, det, view_name, table):
    """render_frame(text=False), then the restatement fed the strings of the
    frame; once per view."""
    if view_name in _frames:
        return _frames[view_name]
    plain = R.render_frame(ds, 0, det, gt, view=view_name).cpu().numpy()
    view = R.frame_view(ds, 0, view_name)
    strings, anchors, colors = TC.frame_text_reference(
        gt, det, view, view_name == 'camera', R.GT_COLORS)
    want = TC.draw_text_reference(
        plain, [s.encode() for s in strings],
        [(x, y - 7) for x, y in anchors], 1, colors, None, table)
    want.setflags(write=False)
    _frames[view_name] = (plain, want, strings)
    return _frames[view_name]


@pytest.mark.parametrize("view_name", ["camera", "bev"])
def test_render_frame_with_text(kitti, table, view_name):
    root, ds, result_dir, gt, det = kitti
    plain, want, strings = frame_reference(ds, gt, det, view_name, table)
    if view_name == 'camera':
        assert strings == ['Car', 'Pedestrian', 'C | 0.912', 'P | 0.873',
                           'C | 0.310']
    else:    # the third detection's centre is outside the canvas
        assert strings == ['Car', 'Pedestrian', 'C | 0.912', 'P | 0.873']
    got = R.render_frame(ds, 0, det, gt, view=view_name, text=True)
    same(got.cpu().numpy(), want, view_name)
    assert not np.array_equal(want, plain)
    # text=False is what it was
    again = R.render_frame(ds, 0, det, gt, view=view_name, text=False)
    same(again.cpu().numpy(), plain, view_name + " plain")
    # the detections alone; a plate under them
    got = R.render_frame(ds, 0, det, None, view=view_name, text=True,
                         text_plate=(0, 0, 0))
    base = R.render_frame(ds, 0, det, None, view=view_name).cpu().numpy()
    view = R.frame_view(ds, 0, view_name)
    s, a, c = TC.frame_text_reference([], det, view, view_name == 'camera',
                                      R.GT_COLORS)
    want2 = TC.draw_text_reference(base, [x.encode() for x in s],
                                   [(x, y - 7) for x, y in a], 1, c,
                                   [(0, 0, 0)], table)
    same(got.cpu().numpy(), want2, view_name + " plates")


@pytest.mark.parametrize("fmt", ["png", "ppm"])
def test_render_results_with_text(kitti, table, tmp_path, fmt):
    from pointgnn_amd import png
    root, ds, result_dir, gt, det = kitti
    plain_dir, text_dir = str(tmp_path / "plain"), str(tmp_path / "text")
    a = R.render_results(ds, result_dir, plain_dir, views=('bev', 'camera'),
                         fmt=fmt)
    b = R.render_results(ds, result_dir, text_dir, views=('bev', 'camera'),
                         fmt=fmt, text=True)
    assert [os.path.relpath(p, plain_dir) for p in a] == \
        [os.path.relpath(p, text_dir) for p in b] == \
        [os.path.join(v, "000000." + fmt) for v in ('bev', 'camera')]
    for pa, pb, view_name in zip(a, b, ('bev', 'camera')):
        da, db = open(pa, "rb").read(), open(pb, "rb").read()
        assert da != db
        plain, want, _ = frame_reference(ds, gt, det, view_name, table)
        if fmt == 'png':
            got = png.read_png(pb, order='rgb').cpu().numpy()
            same(png.read_png(pa, order='rgb').cpu().numpy(), plain, pa)
        else:
            head = b"P6\n%d %d\n255\n" % (want.shape[1], want.shape[0])
            assert db.startswith(head)
            got = np.frombuffer(db[len(head):], np.uint8).reshape(want.shape)
        same(got, want, pb)


def test_command_line_text(kitti, table, tmp_path):
    root, ds, result_dir, gt, det = kitti
    out = str(tmp_path / "cli")
    assert R.main([root, result_dir, out, "--view", "camera", "--ppm",
                   "--text"]) == 0
    data = open(os.path.join(out, "camera", "000000.ppm"), "rb").read()
    plain, want, _ = frame_reference(ds, gt, det, 'camera', table)
    head = b"P6\n%d %d\n255\n" % (want.shape[1], want.shape[0])
    same(np.frombuffer(data[len(head):], np.uint8).reshape(want.shape), want,
         "--text")


# ---- 3. precision / recall plots --------------------------------------------------------
def hand_result(precision=0.5, has_aos=False):
    from pointgnn_amd import kitti_eval as K
    arrays = {}
    for key, dtype, shape in K._OUT_LAYOUT + K._AOS_LAYOUT:
        arrays[key] = np.zeros(shape, dtype)
    arrays['precision'][:] = precision
    arrays['orientation'][:] = 0.25
    arrays['ap_r40'][:] = precision
    arrays['aos_r40'][:] = 0.25
    arrays['n_gt'][:] = 7
    arrays['n_gt'][:, 2] = 0               # no Cyclist among the ground truth
    return K.KittiEvalResult(arrays, has_aos=has_aos)


def test_plot_pr(dev):
    import torch
    from pointgnn_amd import kitti_eval as K
    result = hand_result(0.5)
    img = K.plot_pr(result, '3d', 'Car')
    assert img.is_cuda and img.dtype == torch.uint8
    assert tuple(img.shape) == (480, 640, 3)
    host = img.cpu().numpy()
    area = K.plot_area(640, 480)
    x0, y0, x1, y1 = area
    hard = np.array(K.CURVE_COLORS[2], np.uint8)
    white = np.array((255, 255, 255), np.uint8)
    row = host[K.plot_y(area, 0.5), K.plot_x(area, 0.0):K.plot_x(area, 1.0) + 1]
    assert len(row) == x1 - x0 + 1 and np.all(row == hard)
    assert not np.any(np.all(host[K.plot_y(area, 0.75)] == hard, axis=1))
    assert np.all(host[K.plot_y(area, 0.75), x0 + 1:x1] == white)
    # the axis box, the title, the tick labels, the averages
    assert np.all(host[y0, x0:x1 + 1] == 0)
    assert np.all(host[y0:K.plot_y(area, 0.5), x0] == 0)
    assert np.any(host[:y0 - 10, x0:] != white)              # the title
    assert np.any(host[y1 + 5:y1 + 16, x0 - 10:x1 + 10] != white)
    assert np.any(host[y0 - 4:y1 + 4, :x0 - 5] != white)
    legend = host[y1 - 40:y1 - 5, x0 + 8:x0 + 100].reshape(-1, 3)
    for colour in K.CURVE_COLORS:
        assert np.any(np.all(legend == np.array(colour, np.uint8), axis=1))
    assert np.all(host[0] == white) and np.all(host[:, -1] == white)
    # deterministic
    assert torch.equal(img, K.plot_pr(result, '3d', 'Car'))
    assert torch.equal(img, K.plot_pr(result, 'detection_3d', 0))
    # the other metrics and sizes; curves that differ
    other = K.plot_pr(result, 'bev', 'Pedestrian', 320, 200)
    assert tuple(other.shape) == (200, 320, 3)
    result.precision[2, 0, 0] = np.linspace(1.0, 0.0, 41)     # easy, falling
    falling = K.plot_pr(result, '3d', 'Car').cpu().numpy()
    easy = np.array(K.CURVE_COLORS[0], np.uint8)
    assert tuple(falling[K.plot_y(area, 1.0), x0]) == tuple(easy)
    assert tuple(falling[K.plot_y(area, 0.75), K.plot_x(area, 0.25)]) == \
        tuple(easy)
    assert tuple(falling[K.plot_y(area, 0.5), K.plot_x(area, 0.5)]) == \
        tuple(hard)                                           # hard is on top
    with pytest.raises(ValueError):
        K.plot_pr(result, 'orientation', 'Car')               # no AOS
    with pytest.raises(ValueError):
        K.plot_pr(result, '3d', 'Car', 50, 50)
    aos = K.plot_pr(hand_result(0.5, True), 'orientation', 'Car').cpu().numpy()
    assert np.all(aos[K.plot_y(area, 0.25), x0:x1 + 1] == hard)


def test_write_pr_plots(dev, tmp_path):
    from pointgnn_amd import kitti_eval as K, png
    result = hand_result(0.5, has_aos=True)
    paths = K.write_pr_plots(result, str(tmp_path / "p"))
    names = ['%s_%s.png' % (c, s) for c in ('car', 'pedestrian')
             for s in ('detection', 'detection_ground', 'detection_3d',
                       'orientation')]
    assert [os.path.basename(p) for p in paths] == names   # none for Cyclist
    got = png.read_png(paths[2], order='rgb')
    assert np.array_equal(got.cpu().numpy(),
                          K.plot_pr(result, '3d', 'Car').cpu().numpy())
    ppm = K.write_pr_plots(hand_result(0.5), str(tmp_path / "q"), fmt='ppm')
    assert len(ppm) == 6 and all(p.endswith('.ppm') for p in ppm)
    with pytest.raises(ValueError):
        K.write_pr_plots(result, str(tmp_path / "r"), fmt='jpg')


def test_command_line_plot(kitti, tmp_path, capsys):
    from pointgnn_amd import kitti_eval as K
    root, ds, result_dir, gt, det = kitti
    label_dir = os.path.join(root, "label_2")
    assert K.main([label_dir, result_dir]) == 0
    plain = capsys.readouterr().out
    out = str(tmp_path / "plot")
    assert K.main([label_dir, result_dir, "--plot", out]) == 0
    assert capsys.readouterr().out == plain                 # output unchanged
    stems = ('detection', 'detection_ground', 'detection_3d')
    want = ['%s_%s.txt' % (c, s) for c in ('car', 'pedestrian', 'cyclist')
            for s in stems]
    # ground truth: a Car and a Pedestrian
    want += ['%s_%s.png' % (c, s) for c in ('car', 'pedestrian')
             for s in stems]
    assert sorted(os.listdir(out)) == sorted(want)
    assert not os.path.exists(str(tmp_path / "none"))
