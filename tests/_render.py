"""NumPy restatement of the rasteriser's semantics (include/pointgnn_hip.h,
"rendering") and the cases the render tests run.

Every operation is an IEEE float64 + - * / in the order the header writes it,
a floor, or integer arithmetic: images are compared with == on every byte.
No matmul on the per-point path: the rows are written out.

The keyword switches of the restatement (trunc, half_down, seg_min_wins,
no_clip, depth64) are WRONG semantics on purpose.  tests/test_render_cpu.py
uses them to prove that a case reaches the branch it names: the image of the
case changes when the switch is on.
"""
from collections import OrderedDict, namedtuple

import numpy as np

View = namedtuple('View', ['m', 'd', 'near', 'width', 'height'])

CANVASES = ((64, 48), (67, 45), (1, 1))
COORD_LIMIT = float(2 ** 30)


def view(m, d, near, width, height):
    return View(np.asarray(m, dtype=np.float64).reshape(3, 4),
                np.asarray(d, dtype=np.float64).reshape(4), float(near),
                int(width), int(height))


def flat_view(w, h):
    """pixel = (floor(x), floor(y)), depth = z, hw = 1."""
    return view([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1]], (0, 0, 1, 0), 0.5,
                w, h)


def pinhole_view(w, h, f=8.0, near=0.1):
    """hw = z: u = floor((f x + cx z) / z)."""
    cx, cy = w / 2.0, h / 2.0
    return view([[f, 0, cx, 0], [0, f, cy, 0], [0, 0, 1, 0]], (0, 0, 1, 0),
                near, w, h)


# ---- the restatement ---------------------------------------------------------
def _row(r, x, y, z):
    return ((r[0] * x + r[1] * y) + r[2] * z) + r[3]


def project(v, xyz):
    """[n, 3] float32 / float64 -> float64 (hu, hv, hw, depth)."""
    xyz = np.asarray(xyz)
    x, y, z = (xyz[:, i].astype(np.float64) for i in range(3))
    with np.errstate(all='ignore'):
        return (_row(v.m[0], x, y, z), _row(v.m[1], x, y, z),
                _row(v.m[2], x, y, z), _row(v.d, x, y, z))


def _pixel(h, w, trunc):
    with np.errstate(all='ignore'):
        q = h / w
        return np.trunc(q) if trunc else np.floor(q)


def point_winners(v, xyz, point_size=1, trunc=False, depth64=False):
    """-> int64 [H, W]: index of the winning point per pixel, -1 for none."""
    W, H = v.width, v.height
    win = np.full((H, W), -1, dtype=np.int64)
    if xyz is None or len(xyz) == 0:
        return win
    hu, hv, hw, dep = project(v, xyz)
    ok = np.isfinite(hu) & np.isfinite(hv) & np.isfinite(hw) & np.isfinite(dep)
    with np.errstate(all='ignore'):
        ok &= hw >= v.near
        u, w = _pixel(hu, hw, trunc), _pixel(hv, hw, trunc)
        ok &= (u >= 0.0) & (u < float(W)) & (w >= 0.0) & (w < float(H))
        d = dep if depth64 else dep.astype(np.float32)
    idx = np.nonzero(ok)[0]
    best = np.full((H, W), np.inf, dtype=np.float64)
    for i in idx:                                   # ascending index
        px, py = int(u[i]), int(w[i])
        for yy in range(py, min(py + point_size, H)):
            for xx in range(px, min(px + point_size, W)):
                # strictly smaller: among equal depths the smallest index
                # stays (-0 == +0 here as on the device)
                if win[yy, xx] < 0 or d[i] < best[yy, xx]:
                    win[yy, xx] = i
                    best[yy, xx] = d[i]
    return win


def _floordiv(num, den, half_down):
    if half_down:   # ceil(x - 1/2) where floor(x + 1/2) is asked for
        return -((-(num - 2 * (den // 2))) // den)
    return num // den


def segment_pixels(v, a, b, trunc=False, half_down=False, no_clip=False,
                   full=False):
    """One segment (ends a, b: 3 values each) -> int64 [k, 2] centre pixels
    (x, y) before stamping, or None when it is dropped.  full: every k of
    0..N instead of those near the canvas (small N only)."""
    ends = np.array([a, b])
    hu, hv, hw, _ = project(v, ends)
    if not (np.all(np.isfinite(hu)) and np.all(np.isfinite(hv)) and
            np.all(np.isfinite(hw))):
        return None
    behind = hw < v.near
    if behind[0] and behind[1]:
        return None
    if (behind[0] or behind[1]) and not no_clip:
        i = 0 if behind[0] else 1
        j = 1 - i
        with np.errstate(all='ignore'):
            t = (v.near - hw[i]) / (hw[j] - hw[i])
            hu[i] = hu[i] + t * (hu[j] - hu[i])
            hv[i] = hv[i] + t * (hv[j] - hv[i])
        hw[i] = v.near
    px, py = _pixel(hu, hw, trunc), _pixel(hv, hw, trunc)
    with np.errstate(all='ignore'):
        if not (np.all(np.abs(px) < COORD_LIMIT) and
                np.all(np.abs(py) < COORD_LIMIT)):
            return None
    x0, y0, x1, y1 = int(px[0]), int(py[0]), int(px[1]), int(py[1])
    dx, dy = x1 - x0, y1 - y0
    n = max(abs(dx), abs(dy))
    if n == 0:
        return np.array([[x0, y0]], dtype=np.int64)
    swap = not abs(dx) >= abs(dy)
    a0, b0, da, db = (y0, x0, dy, dx) if swap else (x0, y0, dx, dy)
    lim = v.height if swap else v.width
    s = 1 if da > 0 else -1
    lo, hi = -2, lim + 1     # two beside the canvas: a stamp reaches one
    if full:
        k0, k1 = 0, n
    elif s > 0:
        k0, k1 = max(0, lo - a0), min(n, hi - a0)
    else:
        k0, k1 = max(0, a0 - hi), min(n, a0 - lo)
    if k0 > k1:
        return np.zeros((0, 2), dtype=np.int64)
    k = np.arange(k0, k1 + 1, dtype=np.int64)
    major = a0 + k * s
    minor = b0 + _floordiv(2 * k * db + n, 2 * n, half_down)
    return np.stack([minor, major] if swap else [major, minor], axis=1)


def segment_winners(v, segments, thickness=1, seg_min_wins=False, **kw):
    """-> int64 [H, W]: index of the winning segment per pixel, -1 for none."""
    W, H = v.width, v.height
    win = np.full((H, W), -1, dtype=np.int64)
    if segments is None or len(segments) == 0:
        return win
    thick = np.broadcast_to(np.asarray(thickness), (len(segments),))
    order = range(len(segments))
    for i in (reversed(order) if seg_min_wins else order):   # the last stays
        t = int(thick[i])
        if not 1 <= t <= 3:
            continue
        pix = segment_pixels(v, segments[i][0], segments[i][1], **kw)
        if pix is None:
            continue
        for oy in range(-((t - 1) // 2), t // 2 + 1):
            for ox in range(-((t - 1) // 2), t // 2 + 1):
                x, y = pix[:, 0] + ox, pix[:, 1] + oy
                on = (x >= 0) & (x < W) & (y >= 0) & (y < H)
                win[y[on], x[on]] = i
    return win


def _layer_colors(c, n):
    if c is None:
        c = (255, 255, 255)
    c = np.asarray(c, dtype=np.uint8).reshape(-1, 3)
    return np.broadcast_to(c, (n, 3)) if len(c) == 1 else c


def render(v, points=None, point_colors=None, point_size=1, segments=None,
           segment_colors=None, thickness=1, background=None, trunc=False,
           half_down=False, seg_min_wins=False, no_clip=False, depth64=False):
    """The image pointgnn_amd.render.render must equal, uint8 [H, W, 3]."""
    W, H = v.width, v.height
    img = np.zeros((H, W, 3), dtype=np.uint8)
    if background is not None:
        img[:] = np.asarray(background, dtype=np.uint8)
    pw = point_winners(v, points, point_size, trunc=trunc, depth64=depth64)
    if points is not None and len(points):
        pc = _layer_colors(point_colors, len(points))
        img[pw >= 0] = pc[pw[pw >= 0]]
    sw = segment_winners(v, segments, thickness, seg_min_wins=seg_min_wins,
                         trunc=trunc, half_down=half_down, no_clip=no_clip)
    if segments is not None and len(segments):
        sc = _layer_colors(segment_colors, len(segments))
        img[sw >= 0] = sc[sw[sw >= 0]]
    return img


def colorize(values, lo, hi, table):
    v = np.asarray(values).astype(np.float64)
    with np.errstate(all='ignore'):
        f = np.floor((v - lo) / (hi - lo) * 255.0)
    i = np.where(f >= 255.0, 255, np.where(f >= 0.0, f, 0.0))   # NaN -> 0
    return np.asarray(table)[i.astype(np.int64)]


def graph_segments(coords, edges, level, dst_mask=None):
    e = np.asarray(edges[level] if isinstance(edges, (list, tuple))
                   else edges).reshape(-1, 2)
    if dst_mask is not None:
        m = np.asarray(dst_mask)
        if m.dtype != np.bool_:
            flags = np.zeros(len(coords[level + 1]), dtype=bool)
            flags[m] = True
            m = flags
        e = e[m[e[:, 1]]]
    return np.stack([np.asarray(coords[level], np.float32)[e[:, 0]],
                     np.asarray(coords[level + 1], np.float32)[e[:, 1]]],
                    axis=1).reshape(-1, 2, 3)


# ---- files -----------------------------------------------------------------------
def decode_png(data):
    """8-bit RGB, filter type 0 PNG bytes -> uint8 [H, W, 3], with the stdlib
    only; checks the signature, every CRC and the chunk order."""
    import struct
    import zlib
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, = struct.unpack(">I", data[pos:pos + 4])
        kind, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        crc, = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(kind + body) & 0xffffffff
        chunks.append((kind, body))
        pos += 12 + n
    assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    w, h, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB",
                                                         chunks[0][1])
    assert (depth, ctype, comp, filt, lace) == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(chunks[1][1]), dtype=np.uint8)
    raw = raw.reshape(h, 1 + 3 * w)
    assert np.all(raw[:, 0] == 0)
    return raw[:, 1:].reshape(h, w, 3).copy()


def decode_ppm(data):
    head, w_h, maxval, body = data.split(b"\n", 3)
    assert head == b"P6" and maxval == b"255"
    w, h = (int(t) for t in w_h.split())
    return np.frombuffer(body, dtype=np.uint8).reshape(h, w, 3).copy()


# ---- cases ---------------------------------------------------------------------------
# A case is the keyword arguments of render() plus
#   lights   whether it must light at least one pixel
#   differs  the wrong-semantics switches under which its image must change
#            (proved on canvases of more than one pixel)
def _case(v, lights=True, differs=(), **kw):
    d = dict(view=v, lights=lights, differs=tuple(differs))
    d.update(kw)
    return d


def _rgb(rng, n):
    return rng.integers(1, 256, size=(n, 3)).astype(np.uint8)


def render_args(case):
    return {k: val for k, val in case.items()
            if k not in ('view', 'lights', 'differs')}


POINT_COUNTS = (0, 1, 63, 64, 65, 257)
SEGMENT_COUNTS = (0, 1, 63, 64, 65)


def point_cases(W, H):
    c = OrderedDict()
    fv = flat_view(W, H)
    for n in POINT_COUNTS:
        rng = np.random.default_rng(100 + n)
        xyz = np.stack([rng.uniform(-3, W + 3, n), rng.uniform(-3, H + 3, n),
                        rng.choice([1.0, 2.0, 2.0 + 2.0 ** -40, 5.5], n)],
                       axis=1)
        if n:
            xyz[0, :2] = 0.5
        for dt in (np.float64, np.float32):
            c['points_n%d_%s' % (n, np.dtype(dt).name)] = _case(
                fv, lights=n > 0, points=xyz.astype(dt),
                point_colors=_rgb(rng, n), point_size=1 + n % 3)
    # on each border and one pixel outside each
    xs = [0.0, -1.0, W - 1.0, float(W), W / 2.0, W / 2.0, W / 2.0, W / 2.0]
    ys = [H / 2.0, H / 2.0, H / 2.0, H / 2.0, 0.0, -1.0, H - 1.0, float(H)]
    xyz = np.stack([np.array(xs) + 0.25, np.array(ys) + 0.25, np.ones(8)], 1)
    c['points_border'] = _case(fv, points=xyz, point_colors=_rgb(
        np.random.default_rng(1), 8))
    # hw just below, at and above near (hw = z)
    pv = pinhole_view(W, H)
    z = np.array([np.nextafter(pv.near, 0.0), pv.near,
                  np.nextafter(pv.near, 1.0)])
    xyz = np.stack([np.zeros(3), np.zeros(3), z], axis=1)
    xyz[:, 0] = (np.arange(3) - 1) * z / 8.0 * min(1.0, (W - 1) / 2.0)
    c['points_near'] = _case(pv, points=xyz, point_colors=[(255, 0, 0), (
        0, 255, 0), (0, 0, 255)])
    bad = np.array([[np.nan, 0.5, 1], [0.5, np.inf, 1], [0.5, 0.5, -np.inf],
                    [np.inf, np.nan, 1], [0.5, 0.5, 3.0]])
    c['points_nonfinite'] = _case(fv, points=bad, point_colors=_rgb(
        np.random.default_rng(2), 5))
    # one pixel, different depths: the nearer one has the larger index
    c['points_depth'] = _case(
        fv, points=np.array([[0.5, 0.5, 4.0], [0.7, 0.2, 3.0]]),
        point_colors=[(255, 0, 0), (0, 255, 0)])
    # equal float32 depth, unequal float64 depth: index 0 wins although it is
    # the farther one in float64
    c['points_tie32'] = _case(
        fv, points=np.array([[0.5, 0.5, 1.0 + 2.0 ** -40], [0.5, 0.5, 1.0]]),
        point_colors=[(255, 0, 0), (0, 255, 0)], differs=('depth64',))
    for p in (1, 2, 3):
        xyz = np.array([[W - 0.5, H / 2.0, 1], [W / 2.0, H - 0.5, 1],
                        [W - 0.5, H - 0.5, 1], [0.5, 0.5, 2]])
        c['points_size%d' % p] = _case(fv, points=xyz, point_size=p,
                                       point_colors=_rgb(
                                           np.random.default_rng(p), 4))
    # hu / hw in (-1, 0): floor is -1 (off the canvas), truncation 0
    c['points_negative'] = _case(
        fv, points=np.array([[-0.5, 0.5, 1.0], [0.5, -0.25, 1.0],
                             [W - 0.5, H - 0.5, 1.0]]),
        point_colors=[(255, 0, 0), (0, 255, 0), (0, 0, 255)],
        differs=('trunc',))
    return c


def _seg(pairs):
    """[((x0, y0), (x1, y1)), ...] pixel centres -> [S, 2, 3] for flat_view."""
    out = np.zeros((len(pairs), 2, 3))
    for i, (a, b) in enumerate(pairs):
        out[i, 0, :2] = (a[0] + 0.5, a[1] + 0.5)
        out[i, 1, :2] = (b[0] + 0.5, b[1] + 0.5)
    out[:, :, 2] = 1.0
    return out


def segment_cases(W, H):
    c = OrderedDict()
    fv = flat_view(W, H)
    cx, cy = W // 2, H // 2
    for n in SEGMENT_COUNTS:
        rng = np.random.default_rng(200 + n)
        seg = np.ones((n, 2, 3))
        seg[:, :, 0] = rng.uniform(-5, W + 5, (n, 2))
        seg[:, :, 1] = rng.uniform(-5, H + 5, (n, 2))
        if n:
            seg[-1, :, :2] = [[0.5, 0.5], [W - 0.5, H - 0.5]]
        thick = rng.integers(1, 4, n).astype(np.uint8) if n % 2 else 1 + n % 3
        for dt in (np.float64, np.float32):
            c['segments_n%d_%s' % (n, np.dtype(dt).name)] = _case(
                fv, lights=n > 0, segments=seg.astype(dt),
                segment_colors=_rgb(rng, n), thickness=thick)
    # horizontal, vertical, +-45 degrees, shallow and steep: all eight octants
    dirs = [(9, 0), (-9, 0), (0, 9), (0, -9), (7, 7), (7, -7), (-7, 7),
            (-7, -7)]
    dirs += [(sx * 10, sy * 3) for sx in (1, -1) for sy in (1, -1)]
    dirs += [(sx * 3, sy * 10) for sx in (1, -1) for sy in (1, -1)]
    c['segments_octants'] = _case(
        fv, segments=_seg([((cx, cy), (cx + dx, cy + dy)) for dx, dy in dirs]),
        segment_colors=_rgb(np.random.default_rng(3), len(dirs)))
    # the midpoint falls on a half: both directions put it one up
    a, b = (cx, cy), (cx + 2, cy + 1)
    c['segments_half_ab'] = _case(fv, segments=_seg([(a, b)]),
                                  differs=('half_down',))
    c['segments_half_ba'] = _case(fv, segments=_seg([(b, a)]),
                                  differs=('half_down',))
    a, b = (cx, cy), (cx - 1, cy + 6)
    c['segments_half_steep'] = _case(fv, segments=_seg([(a, b), (b, a)]),
                                     differs=('half_down',))
    c['segments_zero_length'] = _case(fv, segments=_seg([((cx, cy), (cx, cy))]),
                                      thickness=3)
    c['segments_off_canvas'] = _case(fv, lights=False, segments=_seg([
        ((-9, -4), (-2, H + 5)), ((W + 1, 0), (W + 30, H)),
        ((-5, -2), (W + 5, -3)), ((-3, H + 1), (W + 9, H + 1)),
        ((W + 2, -9), (W + 40, 3))]))
    c['segments_cross_borders'] = _case(fv, segments=_seg([
        ((-7, cy), (3, cy + 2)), ((W - 3, cy), (W + 8, cy - 3)),
        ((cx, -6), (cx + 2, 2)), ((cx, H - 2), (cx - 3, H + 9)),
        ((-4, -3), (W + 4, H + 2))]),
        segment_colors=_rgb(np.random.default_rng(4), 5))
    far = 2 ** 29
    c['segments_far_end'] = _case(fv, segments=_seg([
        ((cx, cy), (far, cy + 10 * far // 37)), ((-far, -far // 3), (cx, 0)),
        ((0, cy), (cx // 2, far)), ((cx, -far), (0, H - 1)),
        ((far, far), (0, 0)), ((-far, cy), (far, cy))]),
        segment_colors=_rgb(np.random.default_rng(5), 6), thickness=2)
    c['segments_limit'] = _case(fv, segments=_seg([
        ((0, 0), (2 ** 30 - 1, 0))]))                  # the last end allowed
    c['segments_beyond_limit'] = _case(fv, lights=False, segments=_seg([
        ((0, 0), (2 ** 30, 0)), ((0, -2 ** 30), (0, 0)),
        ((0, 0), (0, 2.0 ** 40)), ((-2.0 ** 62, 0), (0, 0))]))
    # the near plane (hw = z)
    pv = pinhole_view(W, H)
    e = lambda x, y, z: (x * z / 8.0, y * z / 8.0, z)   # -> pixel offset (x, y)
    qx, qy = min(cx, 20), min(cy, 14)
    c['segments_clipped'] = _case(pv, segments=np.array([
        [e(-qx / 2.0, 0, 1.0), (0.3, -0.2, -2.0)]]), differs=('no_clip',))
    c['segments_clipped_a'] = _case(pv, segments=np.array([
        [(-0.3, 0.1, 0.05), e(qx / 2.0, -qy / 2.0, 2.0)]]),
        differs=('no_clip',))
    c['segments_behind'] = _case(pv, lights=False, segments=np.array([
        [(0.0, 0.0, 0.05), (0.01, 0.0, -1.0)],
        [(0.0, 0.0, np.nextafter(pv.near, 0.0)), (0.0, 0.01, 0.0)]]))
    c['segments_at_near'] = _case(pv, segments=np.array([
        [(0.0, 0.0, pv.near), e(qx / 2.0, qy / 2.0, 1.0)]]))
    nan = np.nan
    c['segments_nonfinite'] = _case(fv, segments=np.array([
        [(nan, 0.5, 1), (3.5, 0.5, 1)], [(0.5, 0.5, 1), (0.5, np.inf, 1)],
        [(0.5, 0.5, -np.inf), (0.5, 3.5, 1)],
        [(0.5, 0.5, 1), (min(W, 6) - 0.5, 0.5, 1)]]),
        segment_colors=_rgb(np.random.default_rng(6), 4))
    border = [((0, 0), (W - 1, 0)), ((W - 1, 0), (W - 1, H - 1)),
              ((W - 1, H - 1), (0, H - 1)), ((0, H - 1), (0, 0)),
              ((-1, -1), (W, -1)), ((W, -1), (W, H)), ((W, H), (-1, H)),
              ((-1, H), (-1, -1))]
    for t in (1, 2, 3):
        c['segments_thick%d' % t] = _case(
            fv, segments=_seg(border), thickness=t,
            segment_colors=_rgb(np.random.default_rng(10 + t), 8))
    c['segments_thick_each'] = _case(
        fv, segments=_seg(border),
        thickness=np.array([1, 2, 3, 1, 3, 2, 3, 2], dtype=np.uint8),
        segment_colors=_rgb(np.random.default_rng(14), 8))
    x = [((cx - 6, cy - 4), (cx + 6, cy + 4)), ((cx - 6, cy + 4),
                                                (cx + 6, cy - 4))]
    col = [(255, 0, 0), (0, 255, 0)]
    c['segments_crossing_01'] = _case(fv, segments=_seg(x), segment_colors=col,
                                      differs=('seg_min_wins',))
    c['segments_crossing_10'] = _case(fv, segments=_seg(x[::-1]),
                                      segment_colors=col[::-1],
                                      differs=('seg_min_wins',))
    return c


def layer_cases(W, H):
    """A segment over a point over a background image; both real views."""
    c = OrderedDict()
    fv = flat_view(W, H)
    rng = np.random.default_rng(7)
    bg = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    cx, cy = W // 2, H // 2
    c['layers'] = _case(
        fv, points=np.array([[cx + 0.5, cy + 0.5, 1.0], [0.5, 0.5, 1.0],
                             [W - 0.5, H - 0.5, 2.0]]),
        point_colors=[(255, 0, 0), (0, 255, 0), (0, 0, 255)], point_size=3,
        segments=_seg([((cx - 3, cy), (cx + 3, cy))]),
        segment_colors=(255, 255, 0), background=bg)
    c['layers_one_colour'] = _case(
        fv, points=np.array([[0.5, 0.5, 1.0]]), point_colors=(9, 8, 7),
        background=(40, 50, 60))
    # a bird's eye view whose W, H are not integers before the ceil
    s = 10.0
    bv = bev_view((-W / 20.0 + 0.03, W / 20.0 - 0.01),
                  (1.0, 1.0 + H / 10.0 - 0.05), s)
    n = 300
    xyz = np.stack([rng.uniform(bv_x0(bv) - 0.5, bv_x0(bv) + W / s + 0.5, n),
                    rng.uniform(-2.0, 2.0, n),
                    rng.uniform(0.5, 1.5 + H / s, n)], axis=1)
    seg = np.stack([xyz[:40], xyz[40:80] + rng.uniform(-1, 1, (40, 3))], axis=1)
    c['bev'] = _case(bv, points=xyz.astype(np.float32),
                     point_colors=_rgb(rng, n), point_size=2,
                     segments=seg, segment_colors=_rgb(rng, 40))
    pv = pinhole_view(W, H, f=30.0)
    xyz = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n),
                    rng.uniform(-1.0, 6.0, n)], axis=1)
    seg = np.stack([xyz[:60], xyz[60:120]], axis=1)
    c['camera'] = _case(pv, points=xyz, point_colors=_rgb(rng, n),
                        segments=seg.astype(np.float32),
                        segment_colors=_rgb(rng, 60), thickness=2,
                        background=bg)
    return c


def bev_view(x_range, z_range, scale):
    """The hand-written arrays of render.bev_view."""
    import math
    xmin, xmax = float(x_range[0]), float(x_range[1])
    zmin, zmax = float(z_range[0]), float(z_range[1])
    s = float(scale)
    return view([[s, 0, 0, -s * xmin], [0, 0, -s, s * zmax], [0, 0, 0, 1]],
                (0, 1, 0, 0), 0.5, math.ceil((xmax - xmin) * s),
                math.ceil((zmax - zmin) * s))


def bv_x0(bv):
    return -bv.m[0, 3] / bv.m[0, 0]


def all_cases(W, H):
    c = OrderedDict()
    c.update(point_cases(W, H))
    c.update(segment_cases(W, H))
    c.update(layer_cases(W, H))
    return c


CASE_NAMES = tuple(all_cases(64, 48))

_reference = {}


def reference(W, H, name):
    """(case, the restatement's image), computed once per session and never
    changed."""
    key = (W, H, name)
    if key not in _reference:
        case = all_cases(W, H)[name]
        img = render(case['view'], **render_args(case))
        img.setflags(write=False)
        _reference[key] = (case, img)
    return _reference[key]


COLORIZE_VALUES = np.array([-3.0, 0.0, 1.0, 7.5, np.nan, np.inf, -np.inf,
                            0.5, 51.0 / 255.0, np.nextafter(51.0 / 255.0, 0),
                            0.2, 0.999999, 2.0 / 3.0])


def frame_labels(seed):
    """Label rows and result rows of one synthetic frame, made here: boxes in
    front of the camera, one of a class without a ground-truth colour."""
    rng = np.random.default_rng(1000 + seed)

    def row(name, score=None):
        x, z = rng.uniform(-8, 8), rng.uniform(8, 40)
        xmin, ymin = rng.uniform(5, 60), rng.uniform(5, 40)
        d = {'name': name, 'truncation': 0.0, 'occlusion': 0, 'alpha': 0.0,
             'xmin': xmin, 'ymin': ymin, 'xmax': xmin + rng.uniform(10, 50),
             'ymax': ymin + rng.uniform(10, 30),
             'height': rng.uniform(1.4, 1.8), 'width': rng.uniform(1.5, 1.9),
             'length': rng.uniform(3.2, 4.5), 'x3d': x, 'y3d': 1.7, 'z3d': z,
             'yaw': rng.uniform(-3.1, 3.1)}
        if score is not None:
            d['score'] = score
        return d
    gt = [row('Car'), row('Pedestrian'), row('DontCare'), row('Van')]
    det = [row('Car', 0.9), row('Car', 0.4), row('Pedestrian', 0.7)]
    return gt, det


LABEL_KEYS = ('truncation', 'occlusion', 'alpha', 'xmin', 'ymin', 'xmax',
              'ymax', 'height', 'width', 'length', 'x3d', 'y3d', 'z3d', 'yaw')


def write_label_file(path, rows):
    with open(path, 'w') as f:
        for r in rows:
            fields = [r['name']] + [repr(float(r[k])) if k != 'occlusion'
                                    else str(r[k]) for k in LABEL_KEYS]
            if 'score' in r:
                fields.append(repr(float(r['score'])))
            f.write(' '.join(fields) + '\n')
