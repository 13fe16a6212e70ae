"""PNG encode on the device (pointgnn_amd.png.deflate_device / encode_png,
pgnn_png_encode): every case of tests/_deflate_cases.py byte for byte against
the Python restatement of 'pgnn deflate v1', the round trip through zlib and
through the project's own decoder, and the places the encoder is offered --
render.png_bytes / write_png, render_results, kitti_eval.write_pr_plots."""
import ctypes
import os
import struct
import zlib

import numpy as np
import pytest

import pointgnn_amd  # noqa: F401
import _deflate_cases as DC
import _render as RR

pytestmark = pytest.mark.gpu
CASES = DC.cases()
IDS = [c.name for c in CASES]


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _by_name(name):
    return {c.name: c for c in CASES}[name]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_equals_the_restatement(case, dev):
    import torch
    from pointgnn_amd import png as P
    want, _ = DC.reference(case)
    got = P.deflate_device(torch.from_numpy(case.image).to(dev), case.chunk)
    assert len(got) == len(want)
    assert got == want
    assert zlib.decompress(got) == DC.scanlines(case.image).tobytes()
    h, w = case.image.shape[:2]
    assert P.deflate_capacity(h, w, case.chunk) == DC.capacity(h, w, case.chunk)


@pytest.mark.parametrize("name", ["seam_in_mid_row_3x86", "every_run_length",
                                  "rendered_lines_and_glyphs",
                                  "row_code_23_3x1242"])
def test_round_trip_through_the_decoder(name, dev):
    import torch
    from pointgnn_amd import png as P
    case = _by_name(name)
    image = torch.from_numpy(case.image).to(dev)
    data = P.encode_png(image, case.chunk)
    info = P.parse(data)
    h, w = case.image.shape[:2]
    assert (info.width, info.height, info.color_type, info.channels) == (
        w, h, 2, 3)
    assert info.idat == DC.reference(case)[0]
    back = P.read_png(data, order='rgb')
    assert torch.equal(back, image)
    assert np.array_equal(RR.decode_png(data), case.image)


def test_default_chunk_and_host_input(dev):
    from pointgnn_amd import png as P
    case = _by_name("row_code_23_3x1242")       # its chunk is the default
    assert case.chunk == P.DEFAULT_CHUNK_BYTES == DC.DEFAULT_CHUNK
    assert P.deflate_device(case.image) == DC.reference(case)[0]


def test_strided_inputs_give_the_same_bytes(dev):
    import torch
    from pointgnn_amd import png as P
    case = _by_name("seam_in_mid_row_3x86")
    want = DC.reference(case)[0]
    img = torch.from_numpy(case.image).to(dev)
    h, w = img.shape[:2]
    # rows of a wider image: dense pixels, strided rows
    wide = torch.full((h, w + 5, 3), 201, dtype=torch.uint8, device=dev)
    wide[:, 2:2 + w] = img
    view = wide[:, 2:2 + w]
    assert not view.is_contiguous() and view.stride(0) == 3 * (w + 5)
    assert P.deflate_device(view, case.chunk) == want
    # every second row, every second pixel, a channel flip: copied first
    tall = torch.zeros((2 * h, 2 * w, 3), dtype=torch.uint8, device=dev)
    tall[::2, ::2] = img
    assert P.deflate_device(tall[::2, ::2], case.chunk) == want
    bgr = img.flip(2).contiguous()
    assert P.deflate_device(bgr.flip(2), case.chunk) == want
    assert P.deflate_device(img.permute(1, 0, 2).contiguous().permute(1, 0, 2),
                            case.chunk) == want


def test_on_a_side_stream_and_repeated(dev):
    import torch
    from pointgnn_amd import png as P
    case = _by_name("rendered_lines_and_glyphs")
    want = DC.reference(case)[0]
    img = torch.from_numpy(case.image).to(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = [P.deflate_device(img, case.chunk) for _ in range(3)]
    assert got == [want] * 3


def _png_by_hand(image, level=6):
    h, w = image.shape[:2]
    raw = np.zeros((h, 1 + 3 * w), dtype=np.uint8)
    raw[:, 1:] = image.reshape(h, 3 * w)

    def chunk(kind, data):
        body = kind + data
        return struct.pack(">I", len(data)) + body + struct.pack(
            ">I", zlib.crc32(body) & 0xffffffff)
    return b"".join([
        b"\x89PNG\r\n\x1a\n",
        chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)),
        chunk(b"IDAT", zlib.compress(raw.tobytes(), level)),
        chunk(b"IEND", b"")])


def test_png_bytes_and_write_png(dev, tmp_path):
    import torch
    from pointgnn_amd import png as P, render as R
    case = _by_name("rendered_lines_and_glyphs")
    img = torch.from_numpy(case.image).to(dev)
    # the default is today's file, byte for byte
    assert R.png_bytes(img) == _png_by_hand(case.image)
    assert R.png_bytes(case.image, encoder='zlib') == _png_by_hand(case.image)
    assert R.png_bytes(img, 1) == _png_by_hand(case.image, 1)
    want = P.encode_png(img)
    assert R.png_bytes(img, encoder='device') == want
    path = str(tmp_path / "a.png")
    R.write_png(path, img, encoder='device')
    with open(path, "rb") as f:
        assert f.read() == want
    R.write_png(path, img)
    with open(path, "rb") as f:
        assert f.read() == _png_by_hand(case.image)
    with pytest.raises(ValueError):
        R.png_bytes(img, encoder='gpu')


@pytest.fixture(scope="module")
def kitti(tmp_path_factory, dev):
    """Two synthetic frames with label files and result files made here."""
    from pointgnn_amd import kitti_dataset as KD, synthetic as S
    root = str(tmp_path_factory.mktemp("png_encode_kitti"))
    S.write_kitti_frames(root, [0, 1], preset="small", behind_points=2000)
    label_dir, result_dir = (os.path.join(root, d) for d in
                             ("label_2", "results"))
    os.makedirs(label_dir)
    os.makedirs(result_dir)
    for seed in (0, 1):
        gt, det = RR.frame_labels(seed)
        RR.write_label_file(os.path.join(label_dir, "%06d.txt" % seed), gt)
        if seed == 0:
            RR.write_label_file(os.path.join(result_dir, "%06d.txt" % seed),
                                det)
    ds = KD.KittiDataset(*(os.path.join(root, d) for d in
                           ("image_2", "velodyne", "calib")),
                         label_dir=label_dir)
    return ds, result_dir


def test_render_results_with_the_device_encoder(kitti, tmp_path):
    from pointgnn_amd import png as P, render as R
    ds, result_dir = kitti
    dirs = {k: str(tmp_path / k) for k in ("plain", "zlib", "device")}
    views = ('bev', 'camera')
    plain = R.render_results(ds, result_dir, dirs["plain"], views=views)
    host = R.render_results(ds, result_dir, dirs["zlib"], views=views,
                            png_encoder='zlib')
    td = {}
    device = R.render_results(ds, result_dir, dirs["device"], views=views,
                              png_encoder='device', time_dict=td)
    assert len(plain) == len(host) == len(device) == 4
    assert td['encode png'] > 0 and td['render'] > 0
    for a, b, c in zip(plain, host, device):
        assert os.path.relpath(a, dirs["plain"]) == \
            os.path.relpath(c, dirs["device"])
        da, db, dc = (open(p, "rb").read() for p in (a, b, c))
        assert da == db                     # the default did not move
        assert dc != da
        pixels = RR.decode_png(da)
        assert np.any(pixels != 0)
        assert np.array_equal(RR.decode_png(dc), pixels)
        assert np.array_equal(P.read_png(dc, order='rgb').cpu().numpy(),
                              pixels)
    with pytest.raises(ValueError):
        R.render_results(ds, result_dir, dirs["plain"], png_encoder='gpu')
    # a PPM run takes the argument and writes what it wrote before
    ppm = R.render_results(ds, result_dir, str(tmp_path / "ppm"), fmt='ppm',
                           frame_indices=[0], png_encoder='device')
    assert np.array_equal(RR.decode_ppm(open(ppm[0], "rb").read()),
                          RR.decode_png(open(plain[0], "rb").read()))


def test_run_dataset_passes_the_encoder_on(tmp_path, dev):
    from pointgnn_amd import configs, kitti_dataset as KD, png as P
    from pointgnn_amd import run as RUN, synthetic as S, weights
    root = str(tmp_path / "kitti")
    S.write_kitti_frames(root, [0], preset="tiny", behind_points=500)
    ds = KD.KittiDataset(*(os.path.join(root, d) for d in
                           ("image_2", "velodyne", "calib")))
    cfg = configs.get_config("car_auto_T1")
    params = weights.init_params(cfg, seed=3, bias_scale=0.05)
    files = {}
    for enc in ('zlib', 'device'):
        RUN.run_dataset(ds, cfg, None, str(tmp_path / ("out_" + enc)),
                        params=params, pipelined=False,
                        render_dir=str(tmp_path / ("img_" + enc)),
                        png_encoder=enc)
        with open(os.path.join(str(tmp_path / ("img_" + enc)), "bev",
                               ds.get_filename(0) + ".png"), "rb") as f:
            files[enc] = f.read()
    pixels = RR.decode_png(files['zlib'])
    assert np.array_equal(RR.decode_png(files['device']), pixels)
    # the device file is the device encoder's, the other one zlib's at level 6
    assert files['device'] == P.encode_png(pixels)
    assert P.parse(files['device']).idat[:2] == b"\x78\x01"
    assert P.parse(files['zlib']).idat[:2] == b"\x78\x9c"


def test_command_line_option():
    from pointgnn_amd import kitti_eval as K, render as R
    ap = R.build_parser()
    assert ap.parse_args(["d", "r", "o"]).png_encoder == 'zlib'
    assert ap.parse_args(["d", "r", "o", "--png-encoder", "device"]
                         ).png_encoder == 'device'
    with pytest.raises(SystemExit):
        ap.parse_args(["d", "r", "o", "--png-encoder", "gpu"])
    assert K.parse_args(["l", "r"]).png_encoder == 'zlib'
    assert K.parse_args(["l", "r", "--plot", "p", "--png-encoder", "device"]
                        ).png_encoder == 'device'


def _hand_result(precision=0.5):
    from pointgnn_amd import kitti_eval as K
    arrays = {}
    for key, dtype, shape in K._OUT_LAYOUT + K._AOS_LAYOUT:
        arrays[key] = np.zeros(shape, dtype)
    arrays['precision'][:] = precision
    arrays['ap_r40'][:] = precision
    arrays['n_gt'][:] = 7
    arrays['n_gt'][:, 2] = 0               # no Cyclist among the ground truth
    return K.KittiEvalResult(arrays, has_aos=False)


def test_write_pr_plots_with_the_device_encoder(dev, tmp_path):
    from pointgnn_amd import kitti_eval as K
    result = _hand_result()
    a = K.write_pr_plots(result, str(tmp_path / "a"))
    b = K.write_pr_plots(result, str(tmp_path / "b"), png_encoder='device')
    assert a and len(a) == len(b)
    for pa, pb in zip(a, b):
        da, db = open(pa, "rb").read(), open(pb, "rb").read()
        assert da != db
        assert np.array_equal(RR.decode_png(da), RR.decode_png(db))
    with pytest.raises(ValueError):
        K.write_pr_plots(result, str(tmp_path / "c"), png_encoder='gpu')


def test_argument_errors(dev):
    import torch
    from pointgnn_amd import _lib, png as P
    img = torch.zeros((4, 5, 3), dtype=torch.uint8, device=dev)
    for bad in (0, 128, 300, 32768 + 256, 65536, -256, 256.5):
        with pytest.raises(ValueError):
            P.deflate_device(img, bad)
        with pytest.raises(ValueError):
            P.encode_png(img, bad)
    with pytest.raises(ValueError):
        P.deflate_device(img.to(torch.int32))
    with pytest.raises(ValueError):
        P.deflate_device(img.float())
    with pytest.raises(ValueError):
        P.deflate_device(torch.zeros((4, 5, 4), dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        P.deflate_device(torch.zeros((4, 5), dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        P.deflate_device(torch.zeros((0, 5, 3), dtype=torch.uint8, device=dev))

    # the C entry itself
    lib = _lib.load()
    h, w, c = 4, 5, 256
    cap = P.deflate_capacity(h, w, c)
    ws_bytes = int(lib.pgnn_png_encode_workspace_bytes(h, w, c))
    assert ws_bytes > 0
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    out = torch.full((cap + 8,), 0xA5, dtype=torch.uint8, device=dev)
    n_out = torch.full((1,), -1, dtype=torch.int64, device=dev)

    def call(height=h, width=w, stride=3 * w, chunk=c, ws_size=ws_bytes,
             capacity=cap, image=img):
        return lib.pgnn_png_encode(
            _lib.ptr(image), height, width, stride, chunk, _lib.ptr(ws),
            ws_size, _lib.ptr(out), capacity, _lib.ptr(n_out),
            _lib.stream_ptr())
    assert call(capacity=cap - 1) == _lib.E_INVALID
    assert b"out_capacity" in lib.pgnn_last_error()
    assert call(height=0) == _lib.E_INVALID
    assert call(width=0) == _lib.E_INVALID
    assert call(chunk=0) == _lib.E_INVALID
    assert call(chunk=384) == _lib.E_INVALID
    assert call(chunk=65536) == _lib.E_INVALID
    assert call(stride=3 * w - 1) == _lib.E_INVALID
    assert call(image=None) == _lib.E_INVALID
    assert call(ws_size=ws_bytes - 1) == _lib.E_WORKSPACE
    for args in ((0, w, c), (h, 0, c), (h, w, 100), (h, w, 32768 + 256)):
        assert lib.pgnn_png_encode_workspace_bytes(*args) == 0
    torch.cuda.synchronize()
    # nothing was enqueued by the refused calls
    assert int(n_out.item()) == -1 and bool((out == 0xA5).all())
    # the exact capacity is enough, and nothing past the stream is written
    assert call() == 0
    n = int(n_out.item())
    want, _ = DC.deflate(np.zeros((h, w, 3), np.uint8), c)
    assert n == len(want) <= cap
    assert out[:n].cpu().numpy().tobytes() == want
    assert bool((out[n:] == 0xA5).all())


def test_the_binding_sees_the_entries():
    from pointgnn_amd import _header, _lib
    fns = _header.functions()
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    assert fns["pgnn_png_encode_workspace_bytes"] == (
        ctypes.c_size_t, [i64, i64, i32])
    assert fns["pgnn_png_encode"] == (
        i32, [vp, i64, i64, i64, i32, vp, ctypes.c_size_t, vp, i64, vp, vp])
    lib = _lib.load()
    assert lib.pgnn_png_encode.argtypes == fns["pgnn_png_encode"][1]
    assert "pgnn_png_encode" in _lib.exported_symbols()
