"""PNG test cases (helpers only, no tests): a writer that forces a filter type
per row, a row-serial NumPy restatement of the unfilter, and the case list
shared by tests/test_png_cases_cpu.py and tests/test_gpu_png.py.

The expected image of every case is the array that was encoded."""
import struct
import zlib
from collections import namedtuple

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


# ---- writer -----------------------------------------------------------------
def chunk(kind, data):
    body = kind + data
    return struct.pack(">I", len(data)) + body + struct.pack(
        ">I", zlib.crc32(body) & 0xffffffff)


def _paeth(a, b, c):
    """The Paeth predictor on int arrays (PNG specification 9.4)."""
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(pixels, ftypes):
    """pixels uint8 [H, W, C], ftypes [H] in 0..4 -> the filtered scanlines
    uint8 [H, 1 + W * C].  Filtering reads only the original bytes."""
    h, w, ch = pixels.shape
    cur = pixels.reshape(h, w * ch).astype(np.int64)
    a = np.zeros_like(cur)
    a[:, ch:] = cur[:, :-ch] if w > 1 else 0
    b = np.zeros_like(cur)
    b[1:] = cur[:-1]
    c = np.zeros_like(cur)
    c[:, ch:] = b[:, :-ch] if w > 1 else 0
    ft = np.asarray(ftypes, dtype=np.int64).reshape(h, 1)
    pred = np.select([ft == 0, ft == 1, ft == 2, ft == 3, ft == 4],
                     [np.zeros_like(cur), a, b, (a + b) >> 1, _paeth(a, b, c)])
    raw = np.empty((h, 1 + w * ch), dtype=np.uint8)
    raw[:, 0] = ft[:, 0]
    raw[:, 1:] = ((cur - pred) & 255).astype(np.uint8)
    return raw


def png_bytes(pixels, color_type, ftypes, palette=None, split=None, level=6,
              extra_chunks=()):
    """An 8-bit PNG of `pixels` ([H, W] or [H, W, C]) whose row r is filtered
    with ftypes[r].  split: the zlib stream is cut into IDAT chunks after
    these byte offsets (an int or a list).  extra_chunks: (kind, data) pairs
    placed between IHDR and the rest."""
    pixels = np.asarray(pixels, dtype=np.uint8)
    if pixels.ndim == 2:
        pixels = pixels[:, :, None]
    h, w, ch = pixels.shape
    assert ch == CHANNELS[color_type]
    stream = zlib.compress(filter_rows(pixels, ftypes).tobytes(), level)
    cuts = [0] + sorted([split] if isinstance(split, int) else
                        list(split or [])) + [len(stream)]
    parts = [SIGNATURE,
             chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, color_type,
                                        0, 0, 0))]
    parts += [chunk(k, d) for k, d in extra_chunks]
    if palette is not None:
        parts.append(chunk(b"PLTE", np.asarray(palette, np.uint8).tobytes()))
    parts += [chunk(b"IDAT", stream[lo:hi]) for lo, hi in zip(cuts, cuts[1:])]
    parts.append(chunk(b"IEND", b""))
    return b"".join(parts)


# ---- restatement of the unfilter --------------------------------------------
def unfilter_ref(raw, width, height, channels):
    """The inflated stream (uint8 [H * (1 + W * C)]) -> uint8 [H, W * C]: PNG
    specification 9.2, one row after the other, one byte after the other."""
    stride = 1 + width * channels
    rows = np.asarray(raw, dtype=np.uint8).reshape(height, stride)
    n = width * channels
    prev = [0] * n
    out = np.empty((height, n), dtype=np.uint8)
    for r in range(height):
        ft = int(rows[r, 0])
        f = rows[r, 1:].tolist()
        cur = [0] * n
        if ft == 0:
            cur = f
        elif ft == 1:
            for i in range(n):
                a = cur[i - channels] if i >= channels else 0
                cur[i] = (f[i] + a) & 255
        elif ft == 2:
            cur = [(f[i] + prev[i]) & 255 for i in range(n)]
        elif ft == 3:
            for i in range(n):
                a = cur[i - channels] if i >= channels else 0
                cur[i] = (f[i] + ((a + prev[i]) >> 1)) & 255
        elif ft == 4:
            for i in range(n):
                a = cur[i - channels] if i >= channels else 0
                b = prev[i]
                c = prev[i - channels] if i >= channels else 0
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                cur[i] = (f[i] + pred) & 255
        else:
            raise ValueError("filter type %d" % ft)
        out[r] = cur
        prev = cur
    return out


def to_image(pixels, color_type, palette=None, order='rgb'):
    """What a decode of `pixels` gives: uint8 [H, W, 3]; grey replicated,
    alpha dropped, palette looked up (an index past its end: 0, 0, 0)."""
    pixels = np.asarray(pixels, dtype=np.uint8)
    if pixels.ndim == 2:
        pixels = pixels[:, :, None]
    if color_type in (0, 4):
        img = np.repeat(pixels[:, :, :1], 3, axis=2)
    elif color_type in (2, 6):
        img = pixels[:, :, :3]
    else:
        table = np.zeros((256, 3), dtype=np.uint8)
        pal = np.asarray(palette, dtype=np.uint8).reshape(-1, 3)
        table[:len(pal)] = pal
        img = table[pixels[:, :, 0]]
    if order == 'bgr':
        img = img[:, :, ::-1]
    return np.ascontiguousarray(img)


# ---- the cases ----------------------------------------------------------------
Case = namedtuple("Case", ["name", "pixels", "color_type", "ftypes", "palette",
                           "split", "orders"])

PALETTE5 = np.array([(255, 0, 0), (0, 255, 0), (0, 0, 255), (17, 34, 51),
                     (250, 128, 3)], dtype=np.uint8)
# heights at the edges of the rows in flight (a wave, the workgroup's 512
# rows, two and four bands of them)
HEIGHTS = (1, 2, 63, 64, 65, 128, 129, 257, 511, 512, 513, 1025, 2049)
WIDTHS = (1, 2, 63, 64, 65, 200)

_cases = None


def _seed(name):
    return zlib.crc32(name.encode())


def _make(name, h, w, color_type=2, ftypes='mix', lo=0, hi=256, palette=None,
          split=None, orders=('bgr',)):
    rng = np.random.default_rng(_seed(name))
    ch = CHANNELS[color_type]
    pixels = rng.integers(lo, hi, (h, w, ch)).astype(np.uint8)
    if ftypes == 'mix':
        ft = rng.integers(0, 5, h)
    else:
        ft = np.full(h, int(ftypes))
    return Case(name, pixels, color_type, ft.astype(np.uint8), palette, split,
                tuple(orders))


def cases():
    """The list of cases, built once."""
    global _cases
    if _cases is not None:
        return _cases
    out = []
    for h in HEIGHTS:
        out.append(_make("h%d_w5" % h, h, 5))
    for w in WIDTHS:
        out.append(_make("h70_w%d" % w, 70, w))
    # every wave of the workgroup, two bands, a ring that wraps
    out.append(_make("h600_w100", 600, 100))
    for ft in range(5):
        out.append(_make("all_type%d" % ft, 70, 33, ftypes=ft))
    out.append(_make("mix_h70_w33", 70, 33))
    # data that breaks wrong arithmetic
    out.append(_make("ties_paeth", 70, 33, ftypes=4, lo=0, hi=4))
    out.append(_make("ties_mix", 70, 33, lo=0, hi=4))
    for ft in (1, 2, 3, 4):
        out.append(_make("wrap_type%d" % ft, 40, 21, ftypes=ft, lo=250, hi=256))
    out.append(_make("wrap_mix", 70, 33, lo=250, hi=256))
    out.append(_make("average_carry", 70, 33, ftypes=3, lo=200, hi=256))
    # colour types, both output orders
    both = ('bgr', 'rgb')
    out.append(_make("grey", 70, 33, color_type=0, orders=both))
    out.append(_make("grey_alpha", 70, 33, color_type=4, orders=both))
    out.append(_make("rgb", 70, 33, color_type=2, orders=both, split=7))
    out.append(_make("rgba", 70, 33, color_type=6, orders=both))
    out.append(_make("palette", 70, 33, color_type=3, lo=0, hi=5,
                     palette=PALETTE5, orders=both))
    out.append(_make("palette_beyond", 70, 33, color_type=3, lo=0, hi=9,
                     palette=PALETTE5, orders=both))
    out.append(_make("grey_alpha_tall", 600, 7, color_type=4))
    out.append(_make("rgba_tall", 600, 7, color_type=6))
    # the workload's own shape
    out.append(_make("kitti_375x1242", 375, 1242, split=[100000, 100001]))
    assert len(set(c.name for c in out)) == len(out)
    for c in out:
        c.pixels.setflags(write=False)
    _cases = out
    return out


def case_bytes(case):
    return png_bytes(case.pixels, case.color_type, case.ftypes,
                     palette=case.palette, split=case.split)


def expected(case, order):
    return to_image(case.pixels, case.color_type, case.palette, order)
