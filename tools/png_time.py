#!/usr/bin/env python
"""Time the PNG decode (pointgnn_amd.png, csrc/png.hip) on a 375 x 1242 RGB
file, the size of a KITTI camera image.

    python tools/png_time.py [--calls 20] [--frames 8]

(a) host: parse + inflate of the file, wall time on one thread; beside it,
    where PIL is importable, PIL's whole decode of the same file;
(b) upload of the inflated stream through pinned memory, between device events;
(c) device: pgnn_png_unfilter alone, between device events;
(d) run.run_dataset in frames/s over a synthetic KITTI directory of --frames
    --preset frames (KITTI calibration, real PNG files of that size), with and
    without KittiDataset(decode_images=True), in the same process.
The file is a smooth picture plus noise written by PIL when there is one
(adaptive filters, a realistic compression ratio), else by png_bytes (filter 0,
noise).  Device figures: median of five rounds, each the median of --calls
calls, after a warm-up.  Prints one JSON line."""
import argparse
import io
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS = 5
H, W = 375, 1242


def picture(seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([128 + 90 * np.sin(x / 40.0 + seed) * np.cos(y / 25.0),
                     128 + 90 * np.cos(x / 55.0) * np.sin(y / 30.0 + seed),
                     (x + 2 * y) / 8.0], axis=2)
    return ((base + rng.normal(0, 6, base.shape)).astype(np.int64) & 255
            ).astype(np.uint8)


def encode(rgb):
    """-> (file bytes, the encoder's name)"""
    try:
        from PIL import Image
    except ImportError:
        from pointgnn_amd import render as R
        return R.png_bytes(rgb), "png_bytes"
    buf = io.BytesIO()
    Image.fromarray(rgb, "RGB").save(buf, format="PNG")
    return buf.getvalue(), "PIL"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--preset", default="small",
                    help="synthetic scene of the frame loop in (d)")
    args = ap.parse_args()
    import numpy as np
    import torch
    import pointgnn_amd  # noqa: F401
    from pointgnn_amd import configs, kitti_dataset as KD, png as P
    from pointgnn_amd import run as RUN, synthetic as S, weights
    assert torch.cuda.is_available(), "png_time.py needs the GPU"
    dev = torch.device("cuda", 0)

    def host_ms(fn):
        fn()
        ms = []
        for _ in range(ROUNDS * 4):
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ms)), min(ms), max(ms)

    def device_ms(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        rounds = []
        for _ in range(ROUNDS):
            ms = []
            for _ in range(args.calls):
                a, b = torch.cuda.Event(True), torch.cuda.Event(True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            rounds.append(float(np.median(ms)))
        return float(np.median(rounds)), min(rounds), max(rounds)

    rgb = picture(0)
    data, encoder = encode(rgb)
    info = P.parse(data)
    raw = P.inflate(info)
    out = {"image": [H, W], "file_bytes": len(data), "encoder": encoder,
           "filter_types": sorted(set(raw[::1 + 3 * W].tolist())),
           "calls": args.calls, "rounds": ROUNDS}
    assert np.array_equal(P.read_png(data, order='rgb').cpu().numpy(), rgb)
    # (a)
    out["a_host_parse_inflate_ms"] = host_ms(lambda: P.inflate(P.parse(data)))
    try:
        from PIL import Image
        out["a_pil_decode_ms"] = host_ms(
            lambda: np.asarray(Image.open(io.BytesIO(data))))
    except ImportError:
        out["a_pil_decode_ms"] = None
    # (b)
    out["b_upload_ms"] = device_ms(lambda: P._stage_upload_u8(raw, dev))
    # (c) the entry alone: everything it needs is on the device already
    from pointgnn_amd import _lib
    lib = _lib.load()
    raw_t = torch.from_numpy(raw.copy()).to(dev)
    image = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    ws_bytes = int(lib.pgnn_png_unfilter_workspace_bytes(W, H))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)

    def unfilter_only():
        _lib.check(lib.pgnn_png_unfilter(
            _lib.ptr(raw_t), W, H, 2, None, 0, 1, _lib.ptr(ws), ws_bytes,
            _lib.ptr(image), _lib.stream_ptr()), "pgnn_png_unfilter")
    out["c_device_unfilter_ms"] = device_ms(unfilter_only)
    assert np.array_equal(image.cpu().numpy(), rgb[:, :, ::-1])
    out["c_read_png_whole_ms"] = host_ms(
        lambda: (P.read_png(data), torch.cuda.synchronize()))
    # (d)
    cfg = configs.get_config("car_auto_T1")
    params = weights.init_params(cfg, seed=3, bias_scale=0.05)
    from oracle import ingest_oracle as IO
    cam_to_velo = IO.get_calib(IO.CALIB_LINES)["cam_to_velo"]
    with tempfile.TemporaryDirectory() as tmp:
        # the scene under a KITTI calibration with a 375 x 1242 image
        dirs = [os.path.join(tmp, "kitti", d)
                for d in ("image_2", "velodyne", "calib")]
        for d in dirs:
            os.makedirs(d)
        n_points = []
        for i in range(args.frames):
            xyz, inten = S.synthetic_cloud(seed=i, preset=args.preset)
            homo = np.hstack([xyz.astype(np.float64), np.ones((len(xyz), 1))])
            front = np.hstack([(homo @ cam_to_velo.T)[:, :3], inten])
            back = IO.synthetic_velo_scan(i, n=15000)
            scan = np.vstack([front, back[back[:, 0] < -1.0]]
                             ).astype(np.float32)
            n_points.append(len(scan))
            scan.tofile(os.path.join(dirs[1], "%06d.bin" % i))
            with open(os.path.join(dirs[2], "%06d.txt" % i), "w") as f:
                f.write("".join(IO.CALIB_LINES))
            with open(os.path.join(dirs[0], "%06d.png" % i), "wb") as f:
                f.write(encode(picture(i))[0])
        out["d_scan_points"] = int(np.median(n_points))
        for decode in (False, True):
            ds = KD.KittiDataset(*dirs, decode_images=decode)
            rates = []
            for rep in range(ROUNDS + 1):       # the first pass warms up
                td = RUN.run_dataset(ds, cfg, None,
                                     os.path.join(tmp, "out%d_%d" % (decode,
                                                                     rep)),
                                     params=params)
                torch.cuda.synchronize()
                if rep:
                    rates.append(td['frames'] / td['wall'])
            out["d_frames_per_s_%s" % ("decode" if decode else "plain")] = [
                float(np.median(rates)), min(rates), max(rates)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
