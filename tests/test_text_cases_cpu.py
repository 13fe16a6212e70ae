"""The text cases of tests/_text_cases.py proved on the CPU -- every case
reaches the branch it is named for -- and the host side of text drawing: the
font table read from the built library, text_size, the argument checks of
pgnn_render_text (which answer before any HIP call) and the precision/recall
data files of kitti_eval."""
import ctypes
import os

import numpy as np
import pytest

import pointgnn_amd  # noqa: F401
import _text_cases as TC


@pytest.fixture(scope="module")
def lib():
    from pointgnn_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        from pointgnn_amd import build
        build.build(verbose=False)
    return L.load()


@pytest.fixture(scope="module")
def table(lib):
    out = np.full((95, 7), 0xFF, dtype=np.uint8)
    assert lib.pgnn_render_font(out.ctypes.data_as(ctypes.c_void_p)) == 0
    return out


def _glyph(rows):
    """'.#' pictures -> row masks, bit 4 the leftmost column."""
    return [sum(1 << (4 - c) for c, ch in enumerate(row) if ch == '#')
            for row in rows]


# ---- the font -------------------------------------------------------------------
def test_font_table(lib, table):
    from pointgnn_amd import render as R
    assert table.shape == (95, 7) and table.dtype == np.uint8
    assert np.array_equal(R.font_table(), table)
    assert int(table.max()) < 32
    assert not table[0].any()                                   # space
    assert all(table[g].any() for g in range(1, 95))
    assert len({bytes(table[g]) for g in range(95)}) == 95
    assert lib.pgnn_render_font(None) == -1
    # bit and row order
    pictures = {
        '1': ['..#..', '.##..', '..#..', '..#..', '..#..', '..#..', '.###.'],
        '0': ['.###.', '#...#', '#..##', '#.#.#', '##..#', '#...#', '.###.'],
        'A': ['.###.', '#...#', '#...#', '#...#', '#####', '#...#', '#...#'],
        '|': ['..#..'] * 7,
        '.': ['.....'] * 5 + ['.##..'] * 2,
    }
    for ch, rows in pictures.items():
        assert table[ord(ch) - 0x20].tolist() == _glyph(rows), ch
    assert _glyph(['#....', '....#']) == [16, 1]


def test_text_size():
    from pointgnn_amd import render as R
    assert R.text_size('') == (0, 0) and R.text_size(b'', 3) == (0, 0)
    assert R.text_size('a') == (5, 7)
    assert R.text_size('C | 0.912') == (53, 7)
    assert R.text_size('ab', 2) == (22, 14)
    assert R.text_size(b'P | 0.873', 4) == (212, 28)
    for bad in (0, 5, 1.5, True):
        with pytest.raises(ValueError):
            R.text_size('a', bad)


# ---- the cases ------------------------------------------------------------------
def _owned(case, table):
    return TC.rectangles(case['strings'], case['anchors'], case['scales'],
                         case['plates'], table)


def _on(case, rect):
    _, _, _, x0, y0, x1, y1 = rect
    return x0 < case['width'] and x1 > 0 and y0 < case['height'] and y1 > 0


def _inside(case, rect):
    _, _, _, x0, y0, x1, y1 = rect
    return x0 >= 0 and y0 >= 0 and x1 <= case['width'] and \
        y1 <= case['height']


def test_case_list_is_complete():
    assert len(TC.CASE_NAMES) == len(TC.CASES) >= 50
    for prefix in ('alphabet', 'scale_', 'clip_', 'off_', 'far_', 'long_',
                   'canvas_', 'overlap_', 'bytes_', 'empty_', 'no_strings',
                   'colors_', 'plates_'):
        assert any(n.startswith(prefix) for n in TC.CASE_NAMES), prefix
    for name, case in TC.CASES.items():
        n = len(case['strings'])
        assert len(case['anchors']) == n
        assert len(case['colors']) in (1, n)
        assert case['plates'] is None or len(case['plates']) in (1, n)
        for x, y in case['anchors']:
            assert TC.I32_MIN <= x <= TC.I32_MAX and \
                TC.I32_MIN <= y <= TC.I32_MAX
        bg = TC.background(case)
        assert len(np.unique(bg)) > 1 or bg.size <= 3        # non-uniform


def test_every_case_changes_what_it_should(table):
    for name, case in TC.CASES.items():
        bg, img = TC.background(case), TC.reference(case, table)
        changed = int(np.any(img != bg, axis=2).sum())
        if case.get('nothing'):
            assert changed == 0, name
        else:
            assert changed > 0, name
            # and leaves the rest (a canvas of a pixel or a line may be full)
            if case['width'] > 1 and case['height'] > 1 and \
                    'long_5000_scale_4' not in name:
                assert changed < case['width'] * case['height'], name


def test_alphabet_cases_hold_every_code(table):
    for name in ('alphabet', 'alphabet_scales_2_3'):
        case = TC.CASES[name]
        assert sorted(b''.join(case['strings'])) == list(range(0x20, 0x7F))
        rects = [r for r in _owned(case, table) if r[1] == 'glyph']
        assert all(_inside(case, r) for r in rects), name
    assert TC.CASES['alphabet']['width'] == 6 * 95
    assert TC.CASES['alphabet']['height'] == 9
    assert TC.CASES['alphabet_scales_2_3']['scales'] == [2, 3]


def test_scale_cases(table):
    assert [TC.CASES['scale_%d' % s]['scales'] for s in (1, 2, 3, 4)] == \
        [1, 2, 3, 4]
    assert TC.CASES['scale_each']['scales'] == [1, 2, 3, 4]
    case = TC.CASES['scale_illegal']
    assert [case['scales'][j] for j in case['dropped']] == [0, 5]
    drawn = {r[0] for r in _owned(case, table)}
    assert drawn == {0, 2, 4}
    # the dropped strings would have been on the canvas
    legal = dict(case, scales=[2, 1, 1, 1, 3])
    assert {r[0] for r in _owned(legal, table) if _on(case, r)} == \
        {0, 1, 2, 3, 4}


def test_clipped_cases_are_lit_inside_and_outside(table):
    names = [n for n in TC.CASE_NAMES if TC.CASES[n].get('clipped')]
    assert len(names) == 12
    for name in names:
        case = TC.CASES[name]
        glyphs = [r for r in _owned(case, table) if r[1] == 'glyph']
        assert any(_inside(case, r) for r in glyphs), name
        assert any(not _on(case, r) for r in glyphs), name
        if case['plates'] is not None:
            plate = [r for r in _owned(case, table) if r[1] == 'plate'][0]
            assert _on(case, plate) and not _inside(case, plate), name
    # a corner case leaves the canvas on two sides
    for name, sides in (('clip_corner', (0, 1)), ('clip_corner_far', (2, 3))):
        case = TC.CASES[name]
        glyphs = [r for r in _owned(case, table) if r[1] == 'glyph']
        assert any(r[3] < 0 for r in glyphs) == (0 in sides)
        assert any(r[4] < 0 for r in glyphs) == (1 in sides)
        assert any(r[5] > case['width'] for r in glyphs) == (2 in sides)
        assert any(r[6] > case['height'] for r in glyphs) == (3 in sides)


def test_off_cases_are_wholly_off(table):
    names = [n for n in TC.CASE_NAMES if n.startswith('off_') and
             TC.CASES[n].get('nothing')]
    assert len(names) == 8
    for name in names:
        case = TC.CASES[name]
        assert not any(_on(case, r) for r in _owned(case, table)), name
    for name in TC.CASE_NAMES:
        case = TC.CASES[name]
        if case.get('plate_only'):
            rects = _owned(case, table)
            assert not any(_on(case, r) for r in rects if r[1] == 'glyph')
            assert any(_on(case, r) for r in rects if r[1] == 'plate'), name


def test_far_case_reaches_the_ends_of_int32(table):
    case = TC.CASES['far_anchors']
    flat = [v for a in case['anchors'] for v in a]
    for value in (2 ** 30, -2 ** 30, TC.I32_MIN, TC.I32_MAX):
        assert value in flat
    on = {r[0] for r in _owned(case, table) if _on(case, r)}
    assert on == {len(case['strings']) - 1}


def test_long_case_shows_exactly_forty_characters(table):
    case = TC.CASES['long_5000']
    assert len(case['strings'][0]) == 5000
    glyphs = [r for r in _owned(case, table) if r[1] == 'glyph']
    seen = sorted({r[2] for r in glyphs if _on(case, r)})
    assert seen == list(range(2000, 2040))
    # no glyph of the string is empty: the neighbours are off, not blank
    assert {r[2] for r in glyphs} == set(range(5000))
    case = TC.CASES['long_5000_scale_4_plate']
    seen = {r[2] for r in _owned(case, table) if r[1] == 'glyph' and
            _on(case, r)}
    assert 0 < len(seen) <= 96 // 24 + 2 and min(seen) >= 3000


def test_canvas_cases():
    sizes = {(TC.CASES[n]['width'], TC.CASES[n]['height'])
             for n in TC.CASE_NAMES if n.startswith('canvas_')}
    assert sizes == {(1, 1), (4096, 1), (1, 4096)}


def test_overlap_cases_have_contested_pixels(table):
    names = [n for n in TC.CASE_NAMES if TC.CASES[n].get('contested')]
    assert len(names) == 9
    for name in names:
        case = TC.CASES[name]
        owners = {}
        for r in _owned(case, table):
            for y in range(max(r[4], 0), min(r[6], case['height'])):
                for x in range(max(r[3], 0), min(r[5], case['width'])):
                    owners.setdefault((x, y), set()).add((r[0], r[1]))
        contested = [k for k, v in owners.items()
                     if len({j for j, _ in v}) > 1]
        assert contested, name
        if case['plates'] is not None and not case.get('last_wins'):
            # a later plate over an earlier glyph, a later glyph over an
            # earlier plate
            assert any(any(k == 'glyph' and j < max(jj for jj, _ in v)
                           for j, k in v) for v in owners.values()), name
            assert any(any(k == 'plate' and j < max(
                jj for jj, kk in v if kk == 'glyph') for j, k in v)
                for v in owners.values()
                if any(kk == 'glyph' for _, kk in v)), name
        if 'reversed_name' in case:
            other = TC.CASES[case['reversed_name']]
            assert other['strings'] == case['strings'][::-1]
            a, b = TC.reference(case, table), TC.reference(other, table)
            # the same ground under both, so only the order differs
            a = TC.draw_text_reference(np.zeros_like(a), case['strings'],
                                       case['anchors'], case['scales'],
                                       case['colors'], case['plates'], table)
            b = TC.draw_text_reference(np.zeros_like(b), other['strings'],
                                       other['anchors'], other['scales'],
                                       other['colors'], other['plates'], table)
            assert not np.array_equal(a, b), name
    case = TC.CASES['overlap_300']
    img = TC.reference(case, table)
    want = TC.draw_text_reference(
        TC.background(case), case['strings'][-1:], case['anchors'][-1:], 1,
        case['colors'][-1:], case['plates'][-1:], table)
    assert np.array_equal(img, want)


def test_byte_cases(table):
    case = TC.CASES['bytes_outside']
    assert list(case['strings'][0][:4]) == [0x00, 0x1F, 0x7F, 0xFF]
    other = dict(case, strings=[case['same_as']])
    assert np.array_equal(TC.reference(case, table),
                          TC.reference(other, table))
    assert TC.CASES['empty_alone']['strings'] == [b'']
    assert TC.CASES['empty_between']['strings'][1] == b''
    assert {r[0] for r in _owned(TC.CASES['empty_between'], table)} == {0, 2}
    assert TC.CASES['no_strings']['strings'] == []


def test_colour_cases(table):
    for one, each in (('colors_one', 'colors_each'),
                      ('plates_one', 'plates_each')):
        a, b = TC.CASES[one], TC.CASES[each]
        assert len(a['colors']) == 1 and len(b['colors']) == 3
        assert a['strings'] == b['strings']
    assert len(TC.CASES['plates_one']['plates']) == 1
    assert len(TC.CASES['plates_each']['plates']) == 3
    img = TC.reference(TC.CASES['plates_each'], table).reshape(-1, 3)
    for colour in TC.CASES['plates_each']['plates'] + \
            TC.CASES['plates_each']['colors']:
        assert np.any(np.all(img == np.array(colour, np.uint8), axis=1))


# ---- the entry refuses before it touches the device ----------------------------
def test_render_text_validates_without_a_gpu(lib):
    from pointgnn_amd import _lib
    INV = _lib.E_INVALID
    buf = np.zeros(64, np.uint64)
    p = buf.ctypes.data_as(ctypes.c_void_p)       # stands in as non-null

    def text(image=p, w=4, h=4, chars=p, offsets=p, n=2, anchors=p,
             scales=None, scale=1, colors=p, n_colors=1, plates=None,
             n_plates=0, ws=p, ws_bytes=256):
        return lib.pgnn_render_text(image, w, h, chars, offsets, n, anchors,
                                    scales, scale, colors, n_colors, plates,
                                    n_plates, ws, ws_bytes, None)
    assert lib.pgnn_render_text_workspace_bytes(64, 48) == 64 * 48 * 4
    assert lib.pgnn_render_text_workspace_bytes(67, 45) == 12288  # 256-aligned
    for w, h in ((0, 4), (4, 0), (4097, 4), (4, 4097), (-1, 4)):
        assert lib.pgnn_render_text_workspace_bytes(w, h) == 0
        assert text(w=w, h=h) == INV
        assert b"1..4096" in lib.pgnn_last_error()
    for s in (0, 5, -1):
        assert text(scale=s) == INV
        assert b"scale" in lib.pgnn_last_error()
    assert text(n=-1) == INV and text(n=1 << 30) == INV
    for k in (0, 3, -1):
        assert text(n_colors=k) == INV
        assert b"n_colors" in lib.pgnn_last_error()
    for k in (3, -1):
        assert text(plates=p, n_plates=k) == INV
        assert b"n_plate_colors" in lib.pgnn_last_error()
    assert text(colors=None) == INV
    assert b"null" in lib.pgnn_last_error()
    assert text(plates=None, n_plates=1) == INV
    assert text(image=None) == INV and text(offsets=None) == INV
    assert text(anchors=None) == INV and text(ws=None) == INV
    assert text(ws_bytes=63) == _lib.E_WORKSPACE
    # no strings: nothing to do, and nothing is touched
    assert text(image=None, chars=None, offsets=None, n=0, anchors=None,
                ws=None, ws_bytes=0) == 0
    assert text(image=None, n=0, colors=None, n_colors=0, ws=None) == 0
    assert not buf.any()


# ---- precision / recall data files ---------------------------------------------
def hand_result(has_aos=True, seed=0):
    from pointgnn_amd import kitti_eval as K
    rng = np.random.default_rng(seed)
    arrays = {}
    for key, dtype, shape in K._OUT_LAYOUT + K._AOS_LAYOUT:
        if np.dtype(dtype).kind == 'f':
            arrays[key] = rng.random(shape)
        else:
            arrays[key] = rng.integers(1, 50, shape).astype(dtype)
    return K.KittiEvalResult(arrays, has_aos=has_aos)


@pytest.mark.parametrize("has_aos", [False, True])
def test_write_pr_data_parses_back(tmp_path, has_aos):
    from pointgnn_amd import kitti_eval as K
    result = hand_result(has_aos)
    out = str(tmp_path / "plot")
    paths = K.write_pr_data(result, out)
    stems = ['detection', 'detection_ground', 'detection_3d'] + \
        (['orientation'] if has_aos else [])
    want = ['%s_%s.txt' % (c, s) for c in ('car', 'pedestrian', 'cyclist')
            for s in stems]
    assert [os.path.basename(p) for p in paths] == want
    assert sorted(os.listdir(out)) == sorted(want)
    for c, cls in enumerate(('car', 'pedestrian', 'cyclist')):
        for m, stem in enumerate(stems):
            lines = open(os.path.join(out, '%s_%s.txt' % (cls, stem))
                         ).read().split('\n')
            assert len(lines) == 42 and lines[-1] == ''
            rows = np.array([[float(v) for v in l.split(' ')]
                             for l in lines[:41]])
            assert rows.shape == (41, 4)
            held = result.precision[m, c] if m < 3 else result.orientation[c]
            assert np.array_equal(rows[:, 0], np.round(np.arange(41) / 40.0,
                                                       6))
            assert np.array_equal(rows[:, 1:], np.round(held.T, 6))
            assert lines[0] == '%f %f %f %f' % (0.0, held[0, 0], held[1, 0],
                                                held[2, 0])
    # the classes of the report pick the files
    few = K.KittiEvalResult({k: getattr(result, k) for k, _, _ in
                             K._OUT_LAYOUT + K._AOS_LAYOUT},
                            classes=('Cyclist',), has_aos=False)
    assert [os.path.basename(p) for p in
            K.write_pr_data(few, str(tmp_path / "few"))] == [
        'cyclist_detection.txt', 'cyclist_detection_ground.txt',
        'cyclist_detection_3d.txt']


def test_plot_area_and_its_maps():
    from pointgnn_amd import kitti_eval as K
    area = K.plot_area()
    assert area == K.plot_area(640, 480) == (40, 28, 624, 450)
    x0, y0, x1, y1 = area
    assert K.plot_x(area, 0.0) == x0 and K.plot_x(area, 1.0) == x1
    assert K.plot_y(area, 0.0) == y1 and K.plot_y(area, 1.0) == y0
    assert K.plot_x(area, 0.5) == x0 + (x1 - x0) // 2
    assert K.plot_y(area, 0.75) == y1 - int(np.floor(0.75 * (y1 - y0)))
    for w, h in ((100, 480), (640, 50), (5000, 480)):
        with pytest.raises(ValueError):
            K.plot_area(w, h)
