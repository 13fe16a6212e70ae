"""PNG files -> device images: what `cv2.imread` does for the reference
(kitti_dataset.py:691-701), split where the work changes character.

    info = parse(data)            # chunks, CRCs, IHDR / PLTE / IDAT   (host)
    raw = inflate(info)           # zlib, C speed, releases the GIL    (host)
    img = unfilter(raw, info)     # scanline filters + channel layout  (device)
    img = read_png(path)          # the three in sequence

Inflate is sequential bit twiddling and stays in zlib.  Undoing the scanline
filters is serial per byte within a row and from row to row (Paeth), hopeless
in Python and a skewed wavefront on the device (csrc/png.hip,
include/pointgnn_hip.h "PNG scanline unfilter"); it leaves the uint8
[H, W, 3] image -- BGR as `cv2.imread` returns it, or RGB -- where the crop
(`kitti_dataset.cam_points_in_image`) and the renderer want it.

Supported: bit depth 8, no interlace, colour types 0 (grey), 2 (RGB), 3
(palette), 4 (grey + alpha), 6 (RGBA).  Alpha is dropped, not composited, and
tRNS is ignored, as `cv2.imread`'s default flag does.  Anything else raises
ValueError naming the property.

And device images -> PNG files, cut the other way round: deflate is where the
time goes (render.png_bytes: one host thread in zlib), so that half runs on
the device and only the compressed bytes come back.

    data = deflate_device(image)  # the zlib stream 'pgnn deflate v1'   (device)
    data = encode_png(image)      # signature, IHDR, IDAT + CRC, IEND   (host)

8-bit RGB, filter type 0 on every row, fixed Huffman codes: larger files than
zlib's, written many times faster (csrc/png_encode.hip, include/pointgnn_hip.h
"PNG encode"; the stream is defined to the bit there).
"""
import struct
import zlib
from collections import namedtuple

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}    # colour type -> bytes per pixel
_CRITICAL = (b"IHDR", b"PLTE", b"IDAT", b"IEND")

PngInfo = namedtuple("PngInfo", ["width", "height", "color_type", "channels",
                                 "palette", "idat"])


def parse(data):
    """The bytes of a PNG file -> PngInfo(width, height, color_type, channels,
    palette (uint8 [entries, 3] RGB or None), idat (the IDAT chunks'
    contents, concatenated in order)).  Ancillary chunks are skipped (their
    CRC is not looked at); every critical chunk's CRC is checked."""
    data = bytes(data)
    if data[:8] != SIGNATURE:
        raise ValueError("PNG signature: not a PNG file")
    pos, first = 8, True
    ihdr, palette, idat, ended = None, None, [], False
    while pos < len(data):
        if len(data) - pos < 12:
            raise ValueError("PNG chunk: truncated file (chunk header)")
        length, = struct.unpack(">I", data[pos:pos + 4])
        kind = data[pos + 4:pos + 8]
        end = pos + 8 + length
        if end + 4 > len(data):
            raise ValueError("PNG chunk %r: truncated file" % (kind,))
        if first and kind != b"IHDR":
            raise ValueError("PNG chunk order: IHDR must come first, got %r"
                             % (kind,))
        first = False
        body = data[pos + 8:end]
        if kind in _CRITICAL:
            crc, = struct.unpack(">I", data[end:end + 4])
            if zlib.crc32(data[pos + 4:end]) & 0xffffffff != crc:
                raise ValueError("PNG chunk %s: CRC mismatch"
                                 % kind.decode("ascii"))
        elif not (kind[0:1].isalpha() and kind[0:1].islower()):
            raise ValueError("PNG chunk %r: unknown critical chunk" % (kind,))
        if kind == b"IHDR":
            if ihdr is not None or length != 13:
                raise ValueError("PNG chunk IHDR: malformed")
            ihdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"PLTE":
            if length == 0 or length % 3 or length > 768:
                raise ValueError("PNG chunk PLTE: length %d" % length)
            palette = np.frombuffer(body, dtype=np.uint8).reshape(-1, 3).copy()
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            ended = True
            break
        pos = end + 4
    if ihdr is None:
        raise ValueError("PNG chunk IHDR: missing")
    if not ended:
        raise ValueError("PNG chunk IEND: missing (truncated file)")
    width, height, depth, color_type, compression, filt, interlace = ihdr
    if width == 0 or height == 0:
        raise ValueError("PNG dimensions: %d x %d" % (width, height))
    if color_type not in CHANNELS:
        raise ValueError("PNG colour type: %d" % color_type)
    if depth != 8:
        raise ValueError("PNG bit depth: %d (only 8 is supported)" % depth)
    if compression != 0:
        raise ValueError("PNG compression method: %d" % compression)
    if filt != 0:
        raise ValueError("PNG filter method: %d" % filt)
    if interlace != 0:
        raise ValueError("PNG interlace method: %d (interlaced files are not "
                         "supported)" % interlace)
    if color_type == 3 and palette is None:
        raise ValueError("PNG palette: colour type 3 without a PLTE chunk")
    if not idat:
        raise ValueError("PNG chunk IDAT: missing")
    return PngInfo(int(width), int(height), int(color_type),
                   CHANNELS[color_type],
                   palette if color_type == 3 else None, b"".join(idat))


def inflate(info):
    """info.idat -> uint8 [height * (1 + width * channels)]: the filtered
    scanlines, a filter byte in front of each.  ValueError unless the stream
    inflates to exactly that length and every filter byte is 0..4."""
    stride = 1 + info.width * info.channels
    want = info.height * stride
    d = zlib.decompressobj()
    try:
        raw = d.decompress(info.idat, want + 1)
    except zlib.error as e:
        raise ValueError("PNG stream: %s" % e)
    if len(raw) > want:
        raise ValueError("PNG stream: longer than %d rows of %d bytes"
                         % (info.height, stride))
    if len(raw) < want or not d.eof:
        raise ValueError("PNG stream: truncated (%d of %d bytes)"
                         % (len(raw), want))
    raw = np.frombuffer(raw, dtype=np.uint8)
    worst = int(raw[::stride].max())
    if worst > 4:
        raise ValueError("PNG filter type: %d" % worst)
    return raw


def _stage_upload_u8(arr, dev):
    """kitti_dataset._stage_upload for bytes: through pinned memory, an
    asynchronous copy on the current stream."""
    import torch
    host = torch.empty(int(arr.size), dtype=torch.uint8, pin_memory=True)
    host.numpy()[:] = arr.reshape(-1)
    return host.to(dev, non_blocking=True)


def unfilter(raw, info, order='bgr', device=None):
    """The inflated stream (inflate()) -> uint8 [H, W, 3] CUDA tensor in
    'bgr' (cv2.imread's layout) or 'rgb' order: pgnn_png_unfilter on the
    current stream; nothing is read back."""
    import torch
    from . import _lib
    if order not in ('bgr', 'rgb'):
        raise ValueError("order must be 'bgr' or 'rgb', got %r" % (order,))
    lib = _lib.load()
    dev = torch.device(device) if device is not None else \
        torch.device("cuda", torch.cuda.current_device())
    w, h = int(info.width), int(info.height)
    raw = np.ascontiguousarray(raw, dtype=np.uint8).reshape(-1)
    if raw.size != h * (1 + w * info.channels):
        raise ValueError("raw has %d bytes, %d rows of %d expected"
                         % (raw.size, h, 1 + w * info.channels))
    with torch.cuda.device(dev):
        raw_t = _stage_upload_u8(raw, dev)
        pal_t, entries = None, 0
        if info.color_type == 3:
            pal = np.ascontiguousarray(info.palette, dtype=np.uint8)
            entries = int(pal.shape[0])
            pal_t = _stage_upload_u8(pal, dev)
        image = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
        ws_bytes = int(lib.pgnn_png_unfilter_workspace_bytes(w, h))
        ws = torch.empty((max(ws_bytes, 1),), dtype=torch.uint8, device=dev)
        _lib.check(lib.pgnn_png_unfilter(
            _lib.ptr(raw_t), w, h, int(info.color_type), _lib.ptr(pal_t),
            entries, int(order == 'bgr'), _lib.ptr(ws), ws_bytes,
            _lib.ptr(image), _lib.stream_ptr()), "pgnn_png_unfilter")
    return image


# ---- encode: device image -> zlib stream -> file ---------------------------------
DEFAULT_CHUNK_BYTES = 32768


def _check_chunk(chunk_bytes):
    if isinstance(chunk_bytes, bool) or int(chunk_bytes) != chunk_bytes or \
            chunk_bytes % 256 or not 256 <= chunk_bytes <= 32768:
        raise ValueError("chunk_bytes must be a multiple of 256 in "
                         "256..32768, got %r" % (chunk_bytes,))
    return int(chunk_bytes)


def deflate_capacity(height, width, chunk_bytes=DEFAULT_CHUNK_BYTES):
    """out_capacity of pgnn_png_encode (the header's formula): the most
    bytes the stream of a height x width image can take."""
    c = _check_chunk(chunk_bytes)
    slot = lambda length: (9 * length + 20) // 8 + 4
    full, rest = divmod(int(height) * (3 * int(width) + 1), c)
    return 6 + full * slot(c) + (slot(rest) if rest else 0)


def _device_image(image):
    """-> a CUDA uint8 [H, W, 3] tensor whose rows are dense (the rows
    themselves may be strided); anything else is uploaded or copied."""
    import torch
    if not isinstance(image, torch.Tensor):
        image = torch.from_numpy(np.ascontiguousarray(image))
    if image.dtype != torch.uint8 or image.dim() != 3 or image.shape[2] != 3:
        raise ValueError("image must be uint8 [H, W, 3], got %s %r" % (
            image.dtype, tuple(image.shape)))
    h, w = int(image.shape[0]), int(image.shape[1])
    if h < 1 or w < 1:
        raise ValueError("image must be at least 1 x 1, got %d x %d" % (w, h))
    if not image.is_cuda:
        image = image.to(torch.device("cuda", torch.cuda.current_device()))
    if not (image.stride(2) == 1 and image.stride(1) == 3 and
            (h == 1 or image.stride(0) >= 3 * w)):
        image = image.contiguous()
    return image


def _deflate_enqueue(image, chunk_bytes):
    """pgnn_png_encode on the current stream -> (out uint8 [capacity], the
    stream's length as an int64 [1] tensor); nothing is read back."""
    import torch
    from . import _lib
    lib = _lib.load()
    c = _check_chunk(chunk_bytes)
    image = _device_image(image)
    h, w = int(image.shape[0]), int(image.shape[1])
    row_stride = int(image.stride(0)) if h > 1 else 3 * w
    dev = image.device
    with torch.cuda.device(dev):
        capacity = deflate_capacity(h, w, c)
        out = torch.empty((capacity,), dtype=torch.uint8, device=dev)
        n_out = torch.empty((1,), dtype=torch.int64, device=dev)
        ws_bytes = int(lib.pgnn_png_encode_workspace_bytes(h, w, c))
        ws = torch.empty((max(ws_bytes, 1),), dtype=torch.uint8, device=dev)
        _lib.check(lib.pgnn_png_encode(
            _lib.ptr(image), h, w, row_stride, c, _lib.ptr(ws), ws_bytes,
            _lib.ptr(out), capacity, _lib.ptr(n_out), _lib.stream_ptr()),
            "pgnn_png_encode")
    return out, n_out


def deflate_device(image, chunk_bytes=DEFAULT_CHUNK_BYTES):
    """uint8 [H, W, 3] RGB (a CUDA tensor; anything else is uploaded) -> the
    zlib stream of its PNG scanlines, filter type 0 on every row, compressed
    on the device ('pgnn deflate v1', include/pointgnn_hip.h "PNG encode").
    The device is read twice: the length, then that many bytes; the image is
    never copied to the host."""
    out, n_out = _deflate_enqueue(image, chunk_bytes)
    n = int(n_out.item())
    return out[:n].cpu().numpy().tobytes()


def _chunk(kind, data):
    body = kind + data
    return struct.pack(">I", len(data)) + body + struct.pack(
        ">I", zlib.crc32(body) & 0xffffffff)


def encode_png(image, chunk_bytes=DEFAULT_CHUNK_BYTES):
    """The PNG file of a uint8 [H, W, 3] RGB image, compressed on the device
    (deflate_device): signature, IHDR (8-bit RGB), one IDAT, IEND -- the
    layout render.png_bytes writes; the IDAT CRC is zlib.crc32 on the host."""
    image = _device_image(image)
    h, w = int(image.shape[0]), int(image.shape[1])
    return b"".join([
        SIGNATURE,
        _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)),
        _chunk(b"IDAT", deflate_device(image, chunk_bytes)),
        _chunk(b"IEND", b"")])


def read_png(path_or_bytes, order='bgr', device=None):
    """A PNG file (path, or its bytes) -> uint8 [H, W, 3] CUDA tensor."""
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        data = bytes(path_or_bytes)
    else:
        with open(path_or_bytes, 'rb') as f:
            data = f.read()
    info = parse(data)
    return unfilter(inflate(info), info, order=order, device=device)
