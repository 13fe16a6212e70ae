"""The render cases of tests/_render.py proved on the CPU, and the host side of
pointgnn_amd.render: every case reaches the branch it names (its image changes
under the wrong semantics it is there to catch), lights a pixel unless it is
meant to light none; the view constructors, box segments, colour tables and
the PNG / PPM writers against values written out here."""
import io
import struct
import zlib

import numpy as np
import pytest

import pointgnn_amd  # noqa: F401
from pointgnn_amd import kitti_dataset
from pointgnn_amd import render as R
import _render as RR

BIG = [c for c in RR.CANVASES if c != (1, 1)]


def lit(img, case):
    bg = case.get('background')
    base = np.zeros_like(img)
    if bg is not None:
        base[:] = np.asarray(bg, dtype=np.uint8)
    return int(np.any(img != base, axis=2).sum())


# ---- the cases ----------------------------------------------------------------------
@pytest.mark.parametrize("canvas", RR.CANVASES, ids=lambda c: "%dx%d" % c)
def test_every_case_lights_what_it_should(canvas):
    W, H = canvas
    for name in RR.CASE_NAMES:
        case, img = RR.reference(W, H, name)
        assert img.shape == (H, W, 3) and img.dtype == np.uint8
        assert (case['view'].width, case['view'].height) == (W, H), name
        n = lit(img, case)
        if case['lights']:
            assert n > 0, "%s lights nothing on %dx%d" % (name, W, H)
        else:
            assert n == 0, "%s lights %d pixels" % (name, n)


@pytest.mark.parametrize("canvas", BIG, ids=lambda c: "%dx%d" % c)
def test_cases_differ_under_the_semantics_they_guard(canvas):
    W, H = canvas
    seen = set()
    for name in RR.CASE_NAMES:
        case, img = RR.reference(W, H, name)
        for switch in case['differs']:
            wrong = RR.render(case['view'], **dict(RR.render_args(case),
                                                   **{switch: True}))
            assert not np.array_equal(wrong, img), (name, switch)
            seen.add(switch)
    assert seen == {'trunc', 'half_down', 'seg_min_wins', 'no_clip',
                    'depth64'}


def test_tie_case_has_equal_float32_and_unequal_float64_depths():
    case, img = RR.reference(64, 48, 'points_tie32')
    _, _, _, dep = RR.project(case['view'], case['points'])
    assert dep[0] != dep[1] and dep[0] > dep[1]
    assert np.float32(dep[0]) == np.float32(dep[1])
    # index 0 wins: the smallest index among equal float32 depths
    assert tuple(img[0, 0]) == (255, 0, 0)


def test_depth_case_nearer_point_has_the_larger_index():
    case, img = RR.reference(64, 48, 'points_depth')
    assert tuple(img[0, 0]) == (0, 255, 0)


def test_negative_case_is_between_minus_one_and_zero():
    case, _ = RR.reference(64, 48, 'points_negative')
    hu, hv, hw, _ = RR.project(case['view'], case['points'])
    assert -1.0 < hu[0] / hw[0] < 0.0 and -1.0 < hv[1] / hw[1] < 0.0
    assert np.floor(hu[0] / hw[0]) == -1.0 and np.trunc(hu[0] / hw[0]) == 0.0


def test_half_cases_put_the_midpoint_up_in_both_directions():
    v = RR.flat_view(64, 48)
    for name in ('segments_half_ab', 'segments_half_ba'):
        case, _ = RR.reference(64, 48, name)
        a, b = case['segments'][0]
        pix = RR.segment_pixels(v, a, b)
        ys = sorted(set(pix[:, 1].tolist()))
        xs = sorted(pix[:, 0].tolist())
        mid = pix[pix[:, 0] == xs[1]][0]
        assert len(pix) == 3 and mid[1] == ys[1]          # the upper row
        down = RR.segment_pixels(v, a, b, half_down=True)
        assert down[down[:, 0] == xs[1]][0][1] == ys[0]


def test_clipped_cases_have_exactly_one_end_behind_near():
    for name in ('segments_clipped', 'segments_clipped_a'):
        case, _ = RR.reference(64, 48, name)
        _, _, hw, _ = RR.project(case['view'], case['segments'][0])
        assert int((hw < case['view'].near).sum()) == 1, name
    case, _ = RR.reference(64, 48, 'segments_behind')
    for seg in case['segments']:
        _, _, hw, _ = RR.project(case['view'], seg)
        assert np.all(hw < case['view'].near)
    case, _ = RR.reference(64, 48, 'segments_at_near')
    _, _, hw, _ = RR.project(case['view'], case['segments'][0])
    assert hw[0] == case['view'].near
    case, _ = RR.reference(64, 48, 'points_near')
    _, _, hw, _ = RR.project(case['view'], case['points'])
    near = case['view'].near
    assert hw[0] < near and hw[1] == near and hw[2] > near
    assert np.nextafter(hw[0], 1.0) == near == np.nextafter(hw[2], 0.0)


def test_far_and_limit_cases_reach_their_coordinates():
    v = RR.flat_view(64, 48)
    case, _ = RR.reference(64, 48, 'segments_far_end')
    ends = np.floor(case['segments'][:, :, :2])
    assert np.abs(ends).max() == 2.0 ** 29
    for a, b in case['segments']:
        pix = RR.segment_pixels(v, a, b)
        assert pix is not None and 0 < len(pix) <= 64 + 4   # canvas-bounded
    case, _ = RR.reference(64, 48, 'segments_limit')
    assert np.floor(case['segments'][:, :, :2]).max() == 2.0 ** 30 - 1
    case, _ = RR.reference(64, 48, 'segments_beyond_limit')
    for a, b in case['segments']:
        assert RR.segment_pixels(v, a, b) is None
        assert np.abs(np.floor(np.array([a, b])[:, :2])).max() >= 2.0 ** 30


def test_canvas_cut_equals_the_whole_line():
    """Visiting only the k near the canvas draws what every k of 0..N draws."""
    for W, H in BIG:
        for name in RR.CASE_NAMES:
            case, _ = RR.reference(W, H, name)
            seg = case.get('segments')
            if seg is None or name in ('segments_far_end', 'segments_limit'):
                continue
            v = case['view']
            for a, b in np.asarray(seg, dtype=np.float64):
                cut = RR.segment_pixels(v, a, b)
                if cut is None:
                    continue
                whole = RR.segment_pixels(v, a, b, full=True)
                if len(whole) > 100000:
                    continue
                on = lambda p: set(map(tuple, p[
                    (p[:, 0] >= -1) & (p[:, 0] <= W) & (p[:, 1] >= -1) &
                    (p[:, 1] <= H)].tolist()))
                assert on(cut) == on(whole), name


def test_octants_cover_all_eight():
    case, _ = RR.reference(64, 48, 'segments_octants')
    d = np.floor(case['segments'][:, 1, :2]) - np.floor(
        case['segments'][:, 0, :2])
    kinds = {(np.sign(x), np.sign(y), abs(x) >= abs(y)) for x, y in d}
    for sx in (1, -1):
        for sy in (1, -1):
            assert (sx, sy, True) in kinds and (sx, sy, False) in kinds
    assert (1, 0, True) in kinds and (0, 1, False) in kinds


def test_bev_case_ranges_are_not_integers_before_the_ceil():
    for W, H in RR.CANVASES:
        case, _ = RR.reference(W, H, 'bev')
        v = case['view']
        s = v.m[0, 0]
        w_exact = (W / 20.0 - 0.01 - (-W / 20.0 + 0.03)) * s
        assert w_exact != np.floor(w_exact) and np.ceil(w_exact) == W
        assert (v.width, v.height) == (W, H)


# ---- views ------------------------------------------------------------------------------
def test_bev_view_against_hand_values():
    v = R.bev_view()
    assert (v.width, v.height, v.near) == (800, 800, 0.5)
    assert v.m.dtype == np.float64 and v.m.flags['C_CONTIGUOUS']
    assert v.m.tolist() == [[10.0, 0.0, 0.0, 400.0], [0.0, 0.0, -10.0, 800.0],
                            [0.0, 0.0, 0.0, 1.0]]
    assert v.d.tolist() == [0.0, 1.0, 0.0, 0.0]
    v = R.bev_view((-3.37, 3.3), (0.0, 4.45), 10.0)
    assert (v.width, v.height) == (67, 45)
    assert v.m.tolist() == [[10.0, 0.0, 0.0, -10.0 * -3.37],
                            [0.0, 0.0, -10.0, 10.0 * 4.45],
                            [0.0, 0.0, 0.0, 1.0]]
    w = RR.bev_view((-3.37, 3.3), (0.0, 4.45), 10.0)
    assert np.array_equal(v.m, w.m) and np.array_equal(v.d, w.d)
    # forward is up: z = zmax is row 0, x = xmin is column 0
    img = RR.render(v, points=np.array([[-3.37 + 1e-9, 0.0, 4.45 - 1e-9]]))
    assert tuple(img[0, 0]) == (255, 255, 255)


def test_camera_view_against_hand_values():
    lines = ["P0: 1 0 0 0 0 1 0 0 0 0 1 0\n",
             "P2: 700.5 0 600.25 44.0 0 701.5 180.5 0.25 0 0 1 0.002\n",
             "R0_rect: 1 0 0 0 1 0 0 0 1\n",
             "Tr_velo_to_cam: 0 -1 0 0 0 0 -1 0 1 0 0 0\n"]
    calib = kitti_dataset.parse_calib(lines)
    v = R.camera_view(calib, (1242, 375))
    assert (v.width, v.height, v.near) == (1242, 375, 0.1)
    assert v.m.tolist() == [[700.5, 0.0, 600.25, 0.0],
                            [0.0, 701.5, 180.5, 0.0], [0.0, 0.0, 1.0, 0.0]]
    assert v.d.tolist() == [0.0, 0.0, 1.0, 0.0]
    v = R.pixel_view(5, 4)
    img = RR.render(v, points=np.array([[4.9, 3.2, 123.0]]))
    assert tuple(img[3, 4]) == (255, 255, 255) and lit(img, {}) == 1


# ---- boxes ------------------------------------------------------------------------------
def test_box_segments_against_corners_and_the_edge_table():
    rng = np.random.default_rng(0)
    boxes = np.stack([rng.uniform(-10, 10, 5), rng.uniform(1, 2, 5),
                      rng.uniform(5, 40, 5), rng.uniform(3, 5, 5),
                      rng.uniform(1.4, 2, 5), rng.uniform(1.5, 2, 5),
                      rng.uniform(-4, 4, 5)], axis=1)
    # kitti_dataset.py:807-810
    edges = [[0, 1], [0, 4], [0, 3], [1, 2], [1, 5], [2, 3],
             [2, 6], [3, 7], [4, 5], [4, 7], [5, 6], [6, 7]]
    assert R.BOX_EDGES.tolist() == edges
    seg = R.box_segments(boxes)
    assert seg.shape == (60, 2, 3) and seg.dtype == np.float64
    labels = [{'x3d': b[0], 'y3d': b[1], 'z3d': b[2], 'length': b[3],
               'height': b[4], 'width': b[5], 'yaw': b[6]} for b in boxes]
    for i, label in enumerate(labels):
        corners = kitti_dataset.box3d_to_cam_points(label).xyz
        assert np.array_equal(R.box_corners(boxes[i:i + 1])[0], corners)
        for j, (p, q) in enumerate(edges):
            assert np.array_equal(seg[12 * i + j, 0], corners[p])
            assert np.array_equal(seg[12 * i + j, 1], corners[q])
    assert np.array_equal(R.label_segments(labels), seg)
    assert R.box_segments(np.zeros((0, 7))).shape == (0, 2, 3)
    assert R.label_segments([]).shape == (0, 2, 3)


def test_rect_segments():
    rows = [{'xmin': 3.9, 'ymin': 2.2, 'xmax': 10.99, 'ymax': 7.0}]
    seg = R.rect_segments(rows)
    assert seg.shape == (4, 2, 3)
    assert seg[:, :, :2].tolist() == [
        [[3.0, 2.0], [10.0, 2.0]], [[10.0, 2.0], [10.0, 7.0]],
        [[10.0, 7.0], [3.0, 7.0]], [[3.0, 7.0], [3.0, 2.0]]]
    img = RR.render(R.pixel_view(16, 12), segments=seg, thickness=1)
    assert lit(img, {}) == 2 * 8 + 2 * 4 and tuple(img[2, 3]) == (255,) * 3
    assert R.rect_segments([]).shape == (0, 2, 3)


# ---- colours ----------------------------------------------------------------------------
def test_colour_tables_against_the_reference_values():
    # run.py:176-178
    assert R.CLASS_COLORS.tolist() == [
        [211, 211, 211], [255, 0, 0], [255, 20, 147], [65, 244, 101],
        [169, 244, 65], [65, 79, 244], [65, 181, 244], [229, 244, 66]]
    assert R.CLASS_COLORS.dtype == np.uint8
    # run.py:180-189
    assert R.GT_COLORS == {
        'Pedestrian': (0, 255, 255), 'Person_sitting': (218, 112, 214),
        'Car': (154, 205, 50), 'Truck': (255, 215, 0), 'Van': (255, 20, 147),
        'Tram': (250, 128, 114), 'Misc': (128, 0, 128),
        'Cyclist': (255, 165, 0)}
    assert R.class_colors(np.array([0, 7, 3])).tolist() == [
        [211, 211, 211], [229, 244, 66], [65, 244, 101]]


def test_tables():
    assert R.GRAY_TABLE.shape == R.RAMP_TABLE.shape == (256, 3)
    assert R.GRAY_TABLE.dtype == R.RAMP_TABLE.dtype == np.uint8
    assert R.GRAY_TABLE[:, 0].tolist() == list(range(256))
    assert np.all(R.GRAY_TABLE == R.GRAY_TABLE[:, :1])
    # the ramp: blue at the bottom through green to red at the top
    for i in (0, 1, 63, 64, 127, 128, 191, 192, 255):
        want = [min(255, max(0, 382 - abs(4 * i - c))) for c in
                (765, 510, 255)]
        assert R.RAMP_TABLE[i].tolist() == want
    assert R.RAMP_TABLE[0].tolist() == [0, 0, 127]
    assert R.RAMP_TABLE[128].tolist() == [129, 255, 125]
    assert R.RAMP_TABLE[255].tolist() == [127, 0, 0]


def test_colorize_restatement_on_its_cases():
    i = RR.colorize(RR.COLORIZE_VALUES, 0.0, 1.0,
                    np.arange(256)[:, None].repeat(3, 1))[:, 0]
    # below lo, at lo, at hi, above hi, NaN, +-inf, the middle, a table
    # boundary and the value just below it
    assert i[:7].tolist() == [0, 0, 255, 255, 0, 255, 0]
    assert i[7] == 127 and i[8] == 51 and i[9] == 50
    assert RR.COLORIZE_VALUES[8] * 255.0 == 51.0


# ---- files -------------------------------------------------------------------------------
def _image(h=5, w=7, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3)).astype(
        np.uint8)


def test_write_png_round_trip_with_the_stdlib(tmp_path):
    for h, w in ((5, 7), (1, 1), (48, 64)):
        img = _image(h, w)
        path = str(tmp_path / ("a%d.png" % h))
        R.write_png(path, img)
        data = open(path, "rb").read()
        # decoded here: signature, IHDR, one IDAT, IEND, every CRC
        assert data[:8] == b"\x89PNG\r\n\x1a\n"
        n, = struct.unpack(">I", data[8:12])
        assert n == 13 and data[12:16] == b"IHDR"
        assert struct.unpack(">IIBBBBB", data[16:29]) == (w, h, 8, 2, 0, 0, 0)
        assert struct.unpack(">I", data[29:33])[0] == \
            zlib.crc32(data[12:29]) & 0xffffffff
        assert data.count(b"IDAT") == 1 and data[-12:-8] == b"\0\0\0\0"
        assert data[-8:-4] == b"IEND"
        assert np.array_equal(RR.decode_png(data), img)
        assert kitti_dataset.png_size(path) == (h, w)
        assert R.png_bytes(img) == data


def test_write_png_round_trip_with_pil(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    img = _image(9, 11, seed=3)
    data = R.png_bytes(img)
    back = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    assert np.array_equal(back, img)


def test_write_ppm_round_trip(tmp_path):
    img = _image(6, 3, seed=1)
    path = str(tmp_path / "a.ppm")
    R.write_ppm(path, img)
    data = open(path, "rb").read()
    assert data.startswith(b"P6\n3 6\n255\n")
    assert len(data) == len(b"P6\n3 6\n255\n") + 6 * 3 * 3
    assert np.array_equal(RR.decode_ppm(data), img)


def test_writers_refuse_what_is_not_an_image(tmp_path):
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 3), np.float32),
                np.zeros((4, 4, 4), np.uint8)):
        with pytest.raises(ValueError):
            R.write_png(str(tmp_path / "x.png"), bad)
        with pytest.raises(ValueError):
            R.write_ppm(str(tmp_path / "x.ppm"), bad)


# ---- the entries refuse before they touch the device ----------------------------------------
def test_entries_validate_without_a_gpu():
    from pointgnn_amd import _lib
    lib = _lib.load()
    m = np.zeros(12)
    mp = m.ctypes.data_as(_lib.c_vp)
    assert lib.pgnn_render_workspace_bytes(64, 48) == 64 * 48 * 8
    assert lib.pgnn_render_workspace_bytes(67, 45) == 24320   # 256-aligned
    for w, h in ((0, 4), (4, 0), (4097, 4), (4, 4097), (-1, 4)):
        assert lib.pgnn_render_workspace_bytes(w, h) == 0
        assert lib.pgnn_render_clear(w, h, None, 0, None) == _lib.E_INVALID
        assert lib.pgnn_render_points(None, 0, 0, mp, mp, 0.5, w, h, 1, None,
                                      0, None) == _lib.E_INVALID
        assert b"1..4096" in lib.pgnn_last_error()
        assert lib.pgnn_render_segments(None, 0, 0, mp, 0.5, w, h, None, 1,
                                        None, 0, None) == _lib.E_INVALID
        assert lib.pgnn_render_resolve(w, h, None, 0, None, 0, None, 0, None,
                                       0, None, None) == _lib.E_INVALID
    for p in (0, 4, -1):
        assert lib.pgnn_render_points(None, 0, 0, mp, mp, 0.5, 4, 4, p, None,
                                      0, None) == _lib.E_INVALID
        assert b"point_size" in lib.pgnn_last_error()
        assert lib.pgnn_render_segments(None, 0, 0, mp, 0.5, 4, 4, None, p,
                                        None, 0, None) == _lib.E_INVALID
        assert b"thickness" in lib.pgnn_last_error()
    # null pointers with n > 0 (the workspace stands in as a non-null value)
    ws = np.zeros(16, np.uint64)
    wp = ws.ctypes.data_as(_lib.c_vp)
    assert lib.pgnn_render_points(None, 0, 5, mp, mp, 0.5, 4, 4, 1, wp, 128,
                                  None) == _lib.E_INVALID
    assert b"null" in lib.pgnn_last_error()
    assert lib.pgnn_render_segments(None, 0, 5, mp, 0.5, 4, 4, None, 1, wp,
                                    128, None) == _lib.E_INVALID
    assert lib.pgnn_render_points(wp, 0, 5, None, mp, 0.5, 4, 4, 1, wp, 128,
                                  None) == _lib.E_INVALID
    assert lib.pgnn_render_points(wp, 0, 5, mp, mp, 0.5, 4, 4, 1, wp, 127,
                                  None) == _lib.E_WORKSPACE
    assert lib.pgnn_render_points(wp, 0, 5, mp, mp, float('nan'), 4, 4, 1, wp,
                                  128, None) == _lib.E_INVALID
    assert lib.pgnn_render_colorize(None, 0, 5, 0.0, 1.0, wp, wp,
                                    None) == _lib.E_INVALID
    assert lib.pgnn_render_graph_segments(wp, 1, wp, 1, None, 3, wp,
                                          None) == _lib.E_INVALID
