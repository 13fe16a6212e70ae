"""The PNG cases themselves, and the host half of the decoder
(pointgnn_amd.png.parse / inflate), without a GPU: the forced-filter writer and
the row-serial restatement agree with each other and with PIL, the parser
rejects what it must, and the golden file holds the filters it is there for."""
import io
import os
import struct
import zlib

import numpy as np
import pytest

import pointgnn_amd  # noqa: F401
from pointgnn_amd import png as P
import _png_cases as PC

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = PC.cases()


def _ids(cases):
    return [c.name for c in cases]


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_restatement_round_trips(case):
    data = PC.case_bytes(case)
    info = P.parse(data)
    h, w = case.pixels.shape[:2]
    assert (info.width, info.height, info.color_type, info.channels) == (
        w, h, case.color_type, PC.CHANNELS[case.color_type])
    raw = P.inflate(info)
    assert np.array_equal(raw[::1 + w * info.channels], case.ftypes)
    got = PC.unfilter_ref(raw, w, h, info.channels)
    assert np.array_equal(got.reshape(case.pixels.shape), case.pixels)
    if case.color_type == 3:
        assert np.array_equal(info.palette, case.palette)
    else:
        assert info.palette is None


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_pil_decodes_the_cases(case):
    Image = pytest.importorskip("PIL.Image")
    im = Image.open(io.BytesIO(PC.case_bytes(case)))
    assert im.mode == {0: "L", 2: "RGB", 3: "P", 4: "LA", 6: "RGBA"}[
        case.color_type]
    got = np.asarray(im)          # mode P: the indices
    assert np.array_equal(got.reshape(case.pixels.shape), case.pixels)


def test_expected_images():
    """to_image: grey replicated, alpha dropped, palette looked up, an index
    past the palette black, 'bgr' the reverse of 'rgb'."""
    by_name = {c.name: c for c in CASES}
    c = by_name["palette_beyond"]
    img = PC.expected(c, 'rgb')
    idx = c.pixels[:, :, 0]
    assert idx.max() >= len(PC.PALETTE5)
    assert np.all(img[idx >= 5] == 0) and np.array_equal(
        img[idx < 5], PC.PALETTE5[idx[idx < 5]])
    c = by_name["grey_alpha"]
    assert np.array_equal(PC.expected(c, 'bgr'),
                          np.repeat(c.pixels[:, :, :1], 3, axis=2))
    c = by_name["rgba"]
    assert np.array_equal(PC.expected(c, 'bgr'), c.pixels[:, :, 2::-1])


def _small():
    rng = np.random.default_rng(1)
    return rng.integers(0, 256, (6, 5, 3)).astype(np.uint8)


def _ihdr(w, h, depth=8, color_type=2, compression=0, filt=0, interlace=0):
    return PC.chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, color_type,
                                         compression, filt, interlace))


def _file(ihdr, stream, plte=None):
    return b"".join([PC.SIGNATURE, ihdr] +
                    ([PC.chunk(b"PLTE", plte)] if plte else []) +
                    [PC.chunk(b"IDAT", stream), PC.chunk(b"IEND", b"")])


def _stream(pixels, ftypes=None):
    h = pixels.shape[0]
    ft = np.zeros(h, np.uint8) if ftypes is None else ftypes
    return PC.filter_rows(pixels, ft).tobytes()


def _decode_host(data):
    return P.inflate(P.parse(data))


def test_parse_rejects():
    px = _small()
    good = _file(_ihdr(5, 6), zlib.compress(_stream(px)))
    assert len(_decode_host(good)) == 6 * 16
    # a bad signature
    with pytest.raises(ValueError, match="signature"):
        P.parse(b"\x89PNX" + good[4:])
    # a corrupted IDAT CRC
    at = good.index(b"IDAT")
    length, = struct.unpack(">I", good[at - 4:at])
    crc_at = at + 4 + length
    bad = good[:crc_at] + bytes([good[crc_at] ^ 1]) + good[crc_at + 1:]
    with pytest.raises(ValueError, match="IDAT.*CRC"):
        P.parse(bad)
    # a flipped data byte fails the same check
    bad = good[:at + 6] + bytes([good[at + 6] ^ 0x10]) + good[at + 7:]
    with pytest.raises(ValueError, match="CRC"):
        P.parse(bad)
    # 16-bit, interlaced, other methods, zero sizes
    with pytest.raises(ValueError, match="bit depth"):
        P.parse(_file(_ihdr(5, 6, depth=16), zlib.compress(b"\0" * 6 * 31)))
    with pytest.raises(ValueError, match="interlace"):
        P.parse(_file(_ihdr(5, 6, interlace=1), zlib.compress(_stream(px))))
    with pytest.raises(ValueError, match="compression"):
        P.parse(_file(_ihdr(5, 6, compression=1), zlib.compress(_stream(px))))
    with pytest.raises(ValueError, match="filter method"):
        P.parse(_file(_ihdr(5, 6, filt=1), zlib.compress(_stream(px))))
    with pytest.raises(ValueError, match="dimensions"):
        P.parse(_file(_ihdr(0, 6), zlib.compress(b"")))
    with pytest.raises(ValueError, match="dimensions"):
        P.parse(_file(_ihdr(5, 0), zlib.compress(b"")))
    with pytest.raises(ValueError, match="colour type"):
        P.parse(_file(_ihdr(5, 6, color_type=5), zlib.compress(_stream(px))))
    # colour type 3 without PLTE
    idx = px[:, :, :1] % 4
    with pytest.raises(ValueError, match="PLTE"):
        P.parse(_file(_ihdr(5, 6, color_type=3), zlib.compress(_stream(idx))))
    ok = P.parse(_file(_ihdr(5, 6, color_type=3), zlib.compress(_stream(idx)),
                       plte=bytes(range(12))))
    assert ok.palette.shape == (4, 3) and ok.channels == 1
    # IHDR must come first; a file cut short
    with pytest.raises(ValueError, match="IHDR"):
        P.parse(PC.SIGNATURE + PC.chunk(b"gAMA", b"\0\0\0\1") + good[8:])
    for cut in (len(good) - 1, len(good) - 12, at + 10, 20, 8):
        with pytest.raises(ValueError):
            P.parse(good[:cut])


def test_inflate_rejects():
    px = _small()
    stream = _stream(px)
    # a truncated stream: compressed bytes missing, and rows missing
    comp = zlib.compress(stream)
    with pytest.raises(ValueError, match="stream"):
        _decode_host(_file(_ihdr(5, 6), comp[:len(comp) - 5]))
    with pytest.raises(ValueError, match="truncated"):
        _decode_host(_file(_ihdr(5, 6), zlib.compress(stream[:-1])))
    with pytest.raises(ValueError, match="truncated"):
        _decode_host(_file(_ihdr(5, 7), comp))
    # an over-long stream
    with pytest.raises(ValueError, match="longer"):
        _decode_host(_file(_ihdr(5, 6), zlib.compress(stream + b"\0")))
    with pytest.raises(ValueError, match="longer"):
        _decode_host(_file(_ihdr(5, 5), comp))
    # not a zlib stream at all
    with pytest.raises(ValueError, match="stream"):
        _decode_host(_file(_ihdr(5, 6), b"\x01\x02\x03\x04\x05\x06"))
    # filter byte 5
    ft = np.array([0, 1, 2, 5, 3, 4], np.uint8)
    bad = bytearray(_stream(px))
    bad[3 * 16] = 5
    with pytest.raises(ValueError, match="filter type: 5"):
        _decode_host(_file(_ihdr(5, 6), zlib.compress(bytes(bad))))
    ft[3] = 4
    assert len(_decode_host(_file(_ihdr(5, 6),
                                  zlib.compress(_stream(px, ft))))) == 96


def test_multi_idat_and_ancillary_chunks():
    rng = np.random.default_rng(2)
    px = rng.integers(0, 256, (40, 31, 3)).astype(np.uint8)
    ft = rng.integers(0, 5, 40)
    one = P.parse(PC.png_bytes(px, 2, ft))
    for split in (7, [1, 2], [7, 7, 100], len(one.idat) - 1):
        many = P.parse(PC.png_bytes(px, 2, ft, split=split))
        assert many.idat == one.idat
        assert np.array_equal(P.inflate(many), P.inflate(one))
    # ancillary chunks are skipped, CRC unread
    extra = [(b"gAMA", struct.pack(">I", 45455)), (b"tRNS", b"\0\1\0\2\0\3"),
             (b"tEXt", b"Comment\0made for a test")]
    with_extra = PC.png_bytes(px, 2, ft, extra_chunks=extra)
    assert P.parse(with_extra).idat == one.idat
    at = with_extra.index(b"tEXt") + 4 + len(extra[2][1])
    broken = with_extra[:at] + b"\0\0\0\0" + with_extra[at + 4:]
    assert P.parse(broken).idat == one.idat
    # an unknown critical chunk is not skipped
    with pytest.raises(ValueError, match="critical"):
        P.parse(PC.png_bytes(px, 2, ft, extra_chunks=[(b"ABCD", b"")]))


def test_golden_file_holds_adaptive_filters():
    with open(os.path.join(GOLD, "png_adaptive.png"), "rb") as f:
        info = P.parse(f.read())
    want = np.load(os.path.join(GOLD, "png_adaptive.npy"))
    assert want.dtype == np.uint8 and want.shape == (info.height, info.width, 3)
    assert info.color_type == 2
    raw = P.inflate(info)
    types = set(raw[::1 + 3 * info.width].tolist())
    assert len(types) >= 3 and 4 in types and 2 in types, types
    got = PC.unfilter_ref(raw, info.width, info.height, 3)
    assert np.array_equal(got.reshape(want.shape), want)
