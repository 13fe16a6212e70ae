"""Text drawing (include/pointgnn_hip.h, "text") restated in NumPy, and the
cases the device is held to.  The restatement paints string by string, glyph
by glyph, in painter's order with plain slicing and clipping; it takes the font
table as an argument, so it shares nothing with the kernel but the table.
tests/test_text_cases_cpu.py proves that every case reaches the branch it is
named for; tests/test_gpu_text.py compares the device with == on every byte.

A case: dict(width, height, strings (bytes), anchors (top left, Python ints),
scales (an int for all, or a list, one per string), colors [1 or n, 3], plates
(None or [1 or n, 3])).  Every case is drawn over `background(case)`, a
non-uniform random image, so a pixel nobody owns is compared too."""
import zlib

import numpy as np

FIRST, GLYPHS, ROWS, COLS, ADVANCE = 0x20, 95, 7, 5, 6
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def _scale_of(scales, j):
    return int(scales) if np.ndim(scales) == 0 else int(scales[j])


def _row_of(table, j):
    table = np.asarray(table).reshape(-1, 3)
    return table[0 if len(table) == 1 else j]


def rectangles(strings, anchors, scales, plates, table):
    """What the strings own, unclipped, in painter's order: a list of
    (string, kind, character, x0, y0, x1, y1) with kind 'plate' or 'glyph';
    a glyph rectangle is one lit glyph pixel, scale x scale."""
    out = []
    for j, data in enumerate(strings):
        s = _scale_of(scales, j)
        n = len(data)
        if not 1 <= s <= 4 or n == 0:
            continue
        x, y = int(anchors[j][0]), int(anchors[j][1])
        if plates is not None:
            out.append((j, 'plate', -1, x - s, y - s, x + (6 * n - 1) * s + s,
                        y + 7 * s + s))
        for i, byte in enumerate(data):
            code = byte if FIRST <= byte < FIRST + GLYPHS else ord('?')
            glyph = table[code - FIRST]
            for r in range(ROWS):
                for c in range(COLS):
                    if (int(glyph[r]) >> (COLS - 1 - c)) & 1:
                        x0, y0 = x + (ADVANCE * i + c) * s, y + r * s
                        out.append((j, 'glyph', i, x0, y0, x0 + s, y0 + s))
    return out


def draw_text_reference(image, strings, anchors, scales, colors, plates,
                        table):
    """-> a copy of `image` [H, W, 3] with the strings painted over it."""
    out = np.array(image, dtype=np.uint8, copy=True)
    h, w = out.shape[:2]
    for j, kind, _, x0, y0, x1, y1 in rectangles(strings, anchors, scales,
                                                 plates, table):
        x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, w), min(y1, h)
        if x0 < x1 and y0 < y1:
            out[y0:y1, x0:x1] = _row_of(plates if kind == 'plate' else colors,
                                        j)
    return out


def background(case):
    seed = zlib.crc32(case['name'].encode())
    return np.random.default_rng(seed).integers(
        0, 256, (case['height'], case['width'], 3)).astype(np.uint8)


def reference(case, table):
    return draw_text_reference(background(case), case['strings'],
                               case['anchors'], case['scales'],
                               case['colors'], case['plates'], table)


# ---- the cases ----------------------------------------------------------------
CASES = {}
WHITE = [(255, 255, 255)]
PLATE = [(10, 20, 30)]


def _colors(n, seed):
    """n distinct colours, none of them a likely background byte triple."""
    rng = np.random.default_rng(seed)
    return [tuple(int(v) for v in rng.integers(0, 256, 3)) for _ in range(n)]


def case(name, width, height, strings, anchors, scales=1, colors=WHITE,
         plates=None, **tags):
    strings = [s.encode('latin-1') if isinstance(s, str) else bytes(s)
               for s in strings]
    assert len(anchors) == len(strings) and name not in CASES
    CASES[name] = dict(tags, name=name, width=width, height=height,
                       strings=strings, anchors=[tuple(a) for a in anchors],
                       scales=scales, colors=list(colors),
                       plates=None if plates is None else list(plates))


ALPHABET = bytes(range(FIRST, FIRST + GLYPHS))

# alphabet: every glyph once
case('alphabet', 6 * 95, 9, [ALPHABET], [(0, 1)])
case('alphabet_scales_2_3', 850, 40, [ALPHABET[:48], ALPHABET[48:]],
     [(1, 1), (2, 17)], scales=[2, 3], colors=[(255, 0, 0), (0, 255, 255)])

# scales
for _s in (1, 2, 3, 4):
    case('scale_%d' % _s, 80, 32, ['P|5'], [(3, 2)], scales=_s,
         plates=PLATE if _s == 3 else None)
case('scale_each', 80, 72, ['P|5'] * 4, [(1, 1), (1, 10), (1, 26), (1, 44)],
     scales=[1, 2, 3, 4], colors=_colors(4, 1))
case('scale_illegal', 80, 72, ['a0', 'b1', 'c2', 'd3', 'e4'],
     [(1, 1), (1, 10), (1, 26), (1, 40), (1, 50)], scales=[2, 0, 1, 5, 3],
     colors=_colors(5, 2), plates=_colors(5, 3), dropped=(1, 3))

# clipping: a 3-character string of scale 2 is 34 x 14
_W, _H = 40, 24
for _plates in (None, PLATE):
    _suffix = '' if _plates is None else '_plate'
    for _name, _anchor in (('left', (-15, 5)), ('right', (_W - 15, 5)),
                           ('top', (3, -6)), ('bottom', (3, _H - 7)),
                           ('corner', (-9, -5)),
                           ('corner_far', (_W - 9, _H - 5))):
        case('clip_' + _name + _suffix, _W, _H, ['Qg#'], [_anchor], scales=2,
             colors=[(200, 100, 0)], plates=_plates, clipped=True)
    for _name, _anchor in (('left', (-36, 5)), ('right', (_W + 2, 5)),
                           ('top', (3, -16)), ('bottom', (3, _H + 2))):
        case('off_' + _name + _suffix, _W, _H, ['Qg#'], [_anchor], scales=2,
             plates=_plates, nothing=True)
# the glyphs are off the canvas, a strip of the plate is on it
case('off_right_plate_on', _W, _H, ['Qg#'], [(_W + 1, 5)], scales=2,
     plates=PLATE, plate_only=True)
case('off_top_plate_on', _W, _H, ['Qg#'], [(3, -15)], scales=2, plates=PLATE,
     plate_only=True)
case('far_anchors', _W, _H, ['far'] * 10 + ['ok'],
     [(2 ** 30, 3), (-2 ** 30, 3), (3, 2 ** 30), (3, -2 ** 30),
      (I32_MIN, I32_MIN), (I32_MAX, I32_MAX), (I32_MIN, 3), (3, I32_MAX),
      (I32_MAX, 3), (3, I32_MIN), (4, 4)], scales=[4] * 10 + [1],
     plates=PLATE, only_last=True)
_rng = np.random.default_rng(7)
LONG = bytes(_rng.integers(0x21, 0x7F, 5000).astype(np.uint8))
case('long_5000', 240, 9, [LONG], [(-6 * 2000, 1)], visible=(2000, 2039))
case('long_5000_scale_4_plate', 96, 30, [LONG], [(-24 * 3000 - 7, 1)],
     scales=4, plates=PLATE)
case('canvas_1x1', 1, 1, ['#'], [(-2, -2)])
case('canvas_1x1_plate', 1, 1, ['#'], [(1, 1)], plates=PLATE, plate_only=True)
case('canvas_4096x1', 4096, 1, [ALPHABET * 8, 'Wide'], [(-10, -3), (4000, -8)],
     scales=[1, 4], colors=_colors(2, 4))
case('canvas_1x4096', 1, 4096, ['#'] * 60 + ['Tall'],
     [(-2, 64 * k) for k in range(60)] + [(-8, 4080)],
     scales=[1] * 60 + [4], colors=_colors(61, 5))

# overlap: the later string wins, by a glyph or by a plate
_three = (['MMMM', '####', 'WW8W'], [(4, 4), (6, 5), (5, 7)])
for _n in (2, 3):
    for _plates in (None, _colors(3, 6)[:_n]):
        _name = 'overlap_%d%s' % (_n, '' if _plates is None else '_plates')
        case(_name, 48, 24, _three[0][:_n], _three[1][:_n], scales=2,
             colors=_colors(3, 8)[:_n], plates=_plates, contested=True,
             reversed_name=_name + '_reversed')
        case(_name + '_reversed', 48, 24, _three[0][:_n][::-1],
             _three[1][:_n][::-1], scales=2, colors=_colors(3, 8)[:_n][::-1],
             plates=None if _plates is None else _plates[::-1],
             contested=True)
case('overlap_300', 16, 16, [bytes([0x21 + k % 94]) for k in range(300)],
     [(3, 3)] * 300, scales=1, colors=_colors(300, 9), plates=_colors(300, 10),
     contested=True, last_wins=True)

# bytes
case('bytes_outside', 40, 10, [bytes([0x00, 0x1F, 0x7F, 0xFF, 0x41])],
     [(2, 1)], same_as=b'????A')
case('empty_alone', 20, 12, [b''], [(2, 2)], plates=PLATE, nothing=True)
case('empty_between', 40, 12, ['ab', '', 'cd'], [(1, 2), (8, 2), (20, 2)],
     colors=_colors(3, 11), plates=_colors(3, 12))
case('no_strings', 20, 12, [], [], nothing=True)

# colours
for _name, _c, _p in (('colors_one', [(1, 2, 3)], None),
                      ('colors_each', _colors(3, 13), None),
                      ('plates_one', [(1, 2, 3)], [(250, 251, 252)]),
                      ('plates_each', _colors(3, 14), _colors(3, 15))):
    case(_name, 60, 30, ['x1', 'y2', 'z3'], [(2, 2), (20, 11), (40, 20)],
         colors=_c, plates=_p)

CASE_NAMES = sorted(CASES)


# ---- a frame: what render_frame(text=True) writes (the issue's section 2) -----
DET_COLORS = {True: (0, 255, 255), False: (0, 255, 0)}   # Pedestrian or not


def frame_labels():
    """Two ground-truth labels and three detections (one a Pedestrian; the
    last one's centre is outside the bird's eye canvas)."""
    def row(name, x, z, xmin, ymin, score=None):
        d = {'name': name, 'truncation': 0.0, 'occlusion': 0, 'alpha': 0.0,
             'xmin': xmin, 'ymin': ymin, 'xmax': xmin + 40.5,
             'ymax': ymin + 25.25, 'height': 1.5, 'width': 1.6, 'length': 3.9,
             'x3d': x, 'y3d': 1.7, 'z3d': z, 'yaw': 0.3}
        if score is not None:
            d['score'] = score
        return d
    gt = [row('Car', -3.2, 14.6, 30.7, 44.2), row('Pedestrian', 4.4, 9.3,
                                                  93.1, 50.9)]
    det = [row('Car', -3.0, 14.9, 33.4, 41.8, 0.912),
           row('Pedestrian', 4.5, 9.1, 95.6, 52.3, 0.8726),
           row('Cyclist', 55.0, 20.0, 60.2, 30.1, 0.31)]
    return gt, det


def frame_text_reference(gt, det, view, camera, gt_colors):
    """-> (strings, bottom-left anchors, colors): names of the ground truth
    first, 'P | 0.873' / 'C | 0.912' of the detections after them."""
    out = []
    rows = [(l, l['name'], gt_colors[l['name']], 0) for l in gt
            if l['name'] in gt_colors]
    for l in det:
        ped = l['name'] == 'Pedestrian'
        rows.append((l, '%s | %.3f' % ('P' if ped else 'C', l['score']),
                     DET_COLORS[ped], int(l['xmin'] / 10) if ped else 0))
    for l, string, color, lift in rows:
        if camera:
            out.append((string, (int(l['xmin']), int(l['ymin']) - lift),
                        color))
            continue
        m = np.asarray(view.m, np.float64).reshape(3, 4)
        x, y, z = float(l['x3d']), float(l['y3d']), float(l['z3d'])
        hu, hv, hw = (((r[0] * x + r[1] * y) + r[2] * z) + r[3] for r in m)
        if not hw >= view.near:
            continue
        u, v = np.floor(hu / hw), np.floor(hv / hw)
        if 0 <= u < view.width and 0 <= v < view.height:
            out.append((string, (int(u), int(v)), color))
    return ([o[0] for o in out], [o[1] for o in out], [o[2] for o in out])
