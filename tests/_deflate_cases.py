"""'pgnn deflate v1' (include/pointgnn_hip.h, "PNG encode")
restated in plain Python, and the images the encoder is tested on.

The restatement follows the header's text line by line and shares no code
with csrc/png_encode.hip: the code tables are RFC 1951's, written out; the
parse walks one position at a time.  The device must give the same bytes
(tests/test_gpu_png_encode.py, `==`); tests/test_deflate_cases_cpu.py checks
the restatement itself against zlib and that every case reaches the branch it
is named for.
"""
import functools
from collections import namedtuple

import numpy as np

MOD = 65521
MAX_MATCH = 258
DEFAULT_CHUNK = 32768

# RFC 1951 3.2.5: length codes 257..285 and distance codes 0..29
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43,
            51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4,
             4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257,
             385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9,
              9, 10, 10, 11, 11, 12, 12, 13, 13)

# a token: `pos` in S; a literal has dist 0 and length 1
Token = namedtuple("Token", ["pos", "length", "dist"])


def scanlines(image):
    """uint8 [H, W, 3] -> S, uint8 [H * (3 W + 1)]: a filter byte 0 in front
    of every row."""
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] == 3
    h, w = image.shape[:2]
    raw = np.zeros((h, 1 + 3 * w), dtype=np.uint8)
    raw[:, 1:] = image.reshape(h, 3 * w)
    return raw.reshape(-1)


def slot_bytes(length):
    """The most bytes a chunk of `length` stream bytes can take: 3 header
    bits, 9 bits per byte, 7 bits of end-of-block, the 3 header bits of the
    stored block, padding, its 4 bytes."""
    return (9 * length + 13 + 7) // 8 + 4


def capacity(height, width, chunk):
    """The header's out_capacity formula."""
    n = height * (3 * width + 1)
    full, rest = divmod(n, chunk)
    return 6 + full * slot_bytes(chunk) + (slot_bytes(rest) if rest else 0)


def distances(row_stride):
    return (1, 3, row_stride) if row_stride <= 32768 else (1, 3)


def match_length(s, a, e, i, d):
    """L_d(i) of chunk [a, e); 0 where candidate d is not valid at i."""
    if i - d < a:
        return 0
    n = 0
    while n < min(MAX_MATCH, e - i) and s[i + n] == s[i + n - d]:
        n += 1
    return n


def chunk_tokens(s, a, e, row_stride):
    out, i = [], a
    cands = distances(row_stride)
    while i < e:
        best, best_d = 0, 0
        for d in cands:
            n = match_length(s, a, e, i, d)
            if n > best:            # ties go to the earlier candidate
                best, best_d = n, d
        if best >= 3:
            out.append(Token(i, best, best_d))
            i += best
        else:
            out.append(Token(i, 1, 0))
            i += 1
    return out


class _Bits(object):
    """Deflate's bit order: the first bit written is bit 0 of the first byte."""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value, nbits):
        """`nbits` of value, least significant bit first (extra bits, headers)."""
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def put_code(self, code, nbits):
        """A Huffman code: most significant bit first."""
        self.put(int(format(code, "0%db" % nbits)[::-1], 2), nbits)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)


def _put_symbol(bits, sym):
    """Fixed literal / length code of RFC 1951 3.2.6."""
    if sym < 144:
        bits.put_code(0x30 + sym, 8)
    elif sym < 256:
        bits.put_code(0x190 + sym - 144, 9)
    elif sym < 280:
        bits.put_code(sym - 256, 7)
    else:
        bits.put_code(0xC0 + sym - 280, 8)


def length_code(length):
    k = max(j for j in range(29) if LEN_BASE[j] <= length)
    return k, length - LEN_BASE[k]


def dist_code(dist):
    k = max(j for j in range(30) if DIST_BASE[j] <= dist)
    return k, dist - DIST_BASE[k]


def adler_pair(data):
    a, b = 1, 0
    for v in bytes(data):
        a = (a + v) % MOD
        b = (b + a) % MOD
    return a, b


def adler_combine(first, second, len2):
    """The header's combine: (A, B) of a concatenation from the pairs of its
    two parts, each started at (1, 0)."""
    (a1, b1), (a2, b2) = first, second
    return ((a1 + a2 - 1) % MOD, (b1 + b2 + len2 * (a1 - 1)) % MOD)


def deflate(image, chunk=DEFAULT_CHUNK):
    """-> (the zlib stream, [the tokens of chunk 0, of chunk 1, ...])."""
    assert chunk % 256 == 0 and 256 <= chunk <= 32768
    s = scanlines(image)
    n, row_stride = len(s), 1 + 3 * np.asarray(image).shape[1]
    sl = s.tolist()
    bits, tokens = _Bits(), []
    bits.put(0x78, 8)
    bits.put(0x01, 8)
    pair = (1, 0)
    starts = list(range(0, n, chunk))
    for a in starts:
        e = min(n, a + chunk)
        last = a == starts[-1]
        toks = chunk_tokens(sl, a, e, row_stride)
        tokens.append(toks)
        bits.put(1 if last else 0, 1)        # BFINAL
        bits.put(1, 2)                       # BTYPE = 01
        for t in toks:
            if t.dist == 0:
                _put_symbol(bits, sl[t.pos])
                continue
            k, extra = length_code(t.length)
            _put_symbol(bits, 257 + k)
            bits.put(extra, LEN_EXTRA[k])
            k, extra = dist_code(t.dist)
            bits.put_code(k, 5)
            bits.put(extra, DIST_EXTRA[k])
        _put_symbol(bits, 256)
        if not last:
            bits.put(0, 3)                   # stored, not final
            bits.align()
            bits.put(0x0000, 16)
            bits.put(0xFFFF, 16)
        else:
            bits.align()
        pair = adler_combine(pair, adler_pair(s[a:e].tobytes()), e - a)
    adler = pair[1] << 16 | pair[0]
    return bytes(bits.out) + adler.to_bytes(4, "big"), tokens


@functools.lru_cache(maxsize=None)
def _reference(name):
    case = {c.name: c for c in cases()}[name]
    return deflate(case.image, case.chunk)


def reference(case):
    """deflate(case.image, case.chunk), computed once per process."""
    return _reference(case.name)


# ---- the cases -------------------------------------------------------------------
# check(tokens, s, chunk, row_stride) raises AssertionError unless the case
# reaches the branch it is named for
Case = namedtuple("Case", ["name", "image", "chunk", "check"])


def _flat(tokens):
    return [t for toks in tokens for t in toks]


def _bounds(tokens, s, chunk):
    return [(a, min(len(s), a + chunk)) for a in range(0, len(s), chunk)]


def _row_image(stream_tail, width):
    """A one-row image whose scanline stream is 0 followed by stream_tail."""
    tail = np.asarray(stream_tail, dtype=np.uint8)
    assert len(tail) == 3 * width
    return tail.reshape(1, width, 3)


def _mixed(h, w, seed):
    """Runs of a few colours, some grey, some noise: every kind of token."""
    rng = np.random.RandomState(seed)
    palette = np.array([(0, 0, 0), (90, 90, 90), (200, 30, 150), (7, 143, 144),
                        (255, 255, 0)], dtype=np.uint8)
    flat = np.zeros((h * w, 3), dtype=np.uint8)
    i = 0
    while i < h * w:
        run = int(rng.randint(1, 40))
        if rng.rand() < 0.2:
            flat[i:i + run] = rng.randint(0, 256, (len(flat[i:i + run]), 3))
        else:
            flat[i:i + run] = palette[rng.randint(len(palette))]
        i += run
    img = flat.reshape(h, w, 3)
    if h > 1:
        img[h // 2] = img[h // 2 - 1]       # one row equal to the row above
    return img


def _check_chunks(count, seams=()):
    def check(tokens, s, chunk, row_stride):
        assert len(tokens) == count
        for seam, at_row_start in seams:
            assert seam % chunk == 0 and 0 < seam < len(s)
            assert (seam % row_stride == 0) == at_row_start
    return check


def _runs_image():
    """One row of constant runs: a literal and then a match of every length
    3..258; the lengths the 32768 seam falls into come a second time; then a
    run far beyond the cap."""
    tail, value = [], 1
    for k in list(range(3, 259)) + list(range(245, 259)):
        tail += [value] * (k + 1)
        value = value % 250 + 1             # 1..250, the neighbour differs
    tail += [value] * 800
    tail += [251, 252, 253][:(-len(tail)) % 3]
    return _row_image(tail, len(tail) // 3)


def _check_runs(tokens, s, chunk, row_stride):
    assert row_stride > 32768               # only d = 1 and d = 3 here
    lengths = {t.length for t in _flat(tokens) if t.dist == 1}
    assert lengths >= set(range(3, 259))
    assert {length_code(n)[0] for n in lengths} == set(range(29))
    assert length_code(257) == (27, 30) and length_code(258) == (28, 0)
    # the cap: a 258 whose run goes on
    assert any(t.length == 258 and s[t.pos + 258] == s[t.pos]
               for t in _flat(tokens) if t.pos + 258 < len(s))


def _chunk_end_image():
    """C = 256, one row of 514 stream bytes: a run that ends with chunk 0 and
    one that chunk 1's end cuts."""
    tail = [(37 * i + 11) % 199 + 1 for i in range(513)]    # no matches
    for p in range(235, 256):
        tail[p - 1] = 222                   # stream 235..255
    for p in range(500, 514):
        tail[p - 1] = 233                   # stream 500..513
    return _row_image(tail, 171)


def _check_chunk_end(tokens, s, chunk, row_stride):
    assert chunk == 256 and len(tokens) == 3
    exact = [t for t in tokens[0] if t.dist and t.pos + t.length == 256]
    assert exact and s[256] != s[255]
    cut = [t for t in tokens[1] if t.dist and t.pos + t.length == 512]
    assert cut and s[512] == s[511]
    assert all(t.dist == 0 for t in tokens[2])


def _check_last_chunk_of_one(tokens, s, chunk, row_stride):
    assert len(s) % chunk == 1
    assert tokens[-1] == [Token(len(s) - 1, 1, 0)]


def _check_literals(tokens, s, chunk, row_stride):
    toks = _flat(tokens)
    assert all(t.dist == 0 for t in toks)
    assert {143, 144} <= {int(s[t.pos]) for t in toks}


def _check_valid_source(d):
    def check(tokens, s, chunk, row_stride):
        a = chunk                           # chunk 1
        by_pos = {t.pos: t for t in tokens[1]}
        for i in range(a, a + d):
            assert s[i] == s[i - d]         # would match if it might look back
            if d == 3:
                assert by_pos[i].dist == 0
        if d == 1:
            assert by_pos[a].dist == 0 and by_pos[a + 1].dist == 1
        else:
            assert by_pos[a + 3].dist == 3
    return check


def _check_tie(first, second_is_row):
    def check(tokens, s, chunk, row_stride):
        second = row_stride if second_is_row else 3
        sl, found = s.tolist(), 0
        for (a, e), toks in zip(_bounds(tokens, s, chunk), tokens):
            for t in toks:
                n1 = match_length(sl, a, e, t.pos, first)
                n2 = match_length(sl, a, e, t.pos, second)
                if n1 == n2 and n1 >= 3 and t.length == n1:
                    assert t.dist == first
                    found += 1
        assert found
    return check


def _check_row_distance(used, code=None, valid_positions=None):
    def check(tokens, s, chunk, row_stride):
        uses = [t for t in _flat(tokens) if t.dist == row_stride]
        assert bool(uses) == used
        assert bool(np.any(s[row_stride:] == s[:-row_stride]))
        if code is not None:
            assert dist_code(row_stride)[0] == code
        if valid_positions is not None:
            count = sum(max(0, e - (a + row_stride))
                        for a, e in _bounds(tokens, s, chunk))
            kept = row_stride in distances(row_stride)
            assert (count if kept else 0) == valid_positions
    return check


def _rows(h, w, seed):
    rng = np.random.RandomState(seed)
    row = rng.randint(0, 256, (1, w, 3)).astype(np.uint8)
    return np.repeat(row, h, axis=0)


def _check_worst_case(tokens, s, chunk, row_stride):
    toks = _flat(tokens)
    assert all(t.dist == 0 for t in toks)
    lits = np.array([s[t.pos] for t in toks])
    # every byte but the filter bytes costs 9 bits
    assert np.all((lits >= 144) | (np.arange(len(s)) % row_stride == 0))


_GLYPHS = ((0x0E, 0x11, 0x11, 0x1F, 0x11, 0x11, 0x11),
           (0x1E, 0x11, 0x1E, 0x11, 0x11, 0x11, 0x1E),
           (0x0E, 0x11, 0x10, 0x10, 0x10, 0x11, 0x0E))


def _rendered_image():
    img = np.zeros((64, 96, 3), dtype=np.uint8)
    img[10, 5:80] = (255, 0, 0)
    img[5:60, 40] = (154, 205, 50)
    for k in range(40):
        img[20 + k // 2, 10 + k] = (211, 211, 211)
    for g, rows in enumerate(_GLYPHS):
        for r, mask in enumerate(rows):
            for c in range(5):
                if mask >> (4 - c) & 1:
                    img[30 + r, 50 + 6 * g + c] = (0, 255, 0)
    return img


def _check_rendered(tokens, s, chunk, row_stride):
    assert {t.dist for t in _flat(tokens)} >= {0, 1, 3, row_stride}


def cases():
    rng = np.random.RandomState(20240521)
    grey = np.full((1, 300, 3), 77, dtype=np.uint8)
    colour = np.zeros((1, 200, 3), dtype=np.uint8)
    colour[:] = (1, 2, 3)
    two_rows = np.zeros((2, 300, 3), dtype=np.uint8)
    two_rows[:] = (1, 2, 3)
    literals = _row_image([142, 143, 144, 145, 255, 0], 2)
    noise = rng.randint(144, 256, (40, 40, 3)).astype(np.uint8)
    return [
        Case("tiny_1x1", np.array([[[9, 8, 7]]], dtype=np.uint8), 256,
             _check_chunks(1)),
        Case("row_is_one_chunk_1x85", _mixed(1, 85, 1), 256, _check_chunks(1)),
        Case("seam_at_row_start_2x85", _mixed(2, 85, 2), 256,
             _check_chunks(2, [(256, True)])),
        Case("seam_in_mid_row_3x86", _mixed(3, 86, 3), 256,
             _check_chunks(4, [(256, False), (512, False), (768, False)])),
        Case("every_run_length", _runs_image(), 32768, _check_runs),
        Case("run_to_chunk_end_and_cut", _chunk_end_image(), 256,
             _check_chunk_end),
        Case("last_chunk_of_one_byte", _mixed(27, 6, 4), 256,
             _check_last_chunk_of_one),
        Case("literals_143_144", literals, 256, _check_literals),
        Case("valid_source_d1", grey[:, :200], 256, _check_valid_source(1)),
        Case("valid_source_d3", colour, 256, _check_valid_source(3)),
        Case("tie_d1_d3_grey_run", grey, 1024, _check_tie(1, False)),
        Case("tie_d3_row_two_equal_rows", two_rows, 2048, _check_tie(3, True)),
        Case("row_never_valid_7x300", _rows(7, 300, 5), 256,
             _check_row_distance(False, valid_positions=0)),
        Case("row_valid_7x300", _rows(7, 300, 5), 4096,
             _check_row_distance(True)),
        Case("row_code_23_3x1242", _rows(3, 1242, 6), 32768,
             _check_row_distance(True, code=23)),
        Case("row_code_29_2x10922", _rows(2, 10922, 7), 32768,
             _check_row_distance(False, code=29, valid_positions=1)),
        Case("row_dropped_2x10923", _rows(2, 10923, 8), 32768,
             _check_row_distance(False, valid_positions=0)),
        Case("noise_worst_case_slot", noise, 1024, _check_worst_case),
        Case("rendered_lines_and_glyphs", _rendered_image(), 4096,
             _check_rendered),
        # 301 chunks: more than the 256 CUs, so workgroups take several chunks
        Case("more_chunks_than_workgroups_64x400", _mixed(64, 400, 9), 256,
             _check_chunks(301)),
    ]
