#!/usr/bin/env python
"""Time the PNG encode on the device (pointgnn_amd.png.encode_png,
csrc/png_encode.hip) against host zlib, with the method of tools/png_time.py.

    python tools/png_encode_time.py [--calls 20] [--frames 8] [--images-only]

Two images: (bev) the 800 x 800 bird's eye view of the `car_600k` seed-0 frame
with 32 seeded boxes, black with long runs; (camera) the 1242 x 375 camera view
of the same frame drawn over a picture (a smooth image plus noise, standing in
for a photograph: mostly literals).  For each:
(a) host: render.png_bytes at zlib level 6 and level 1, the image on the device
    when the call starts (so the copy is inside), wall time on one thread; and
    zlib.compress alone on the scanlines;
(b) device: pgnn_png_encode alone (its three launches), between device events;
(c) png.encode_png whole: entry, the two reads, CRC and file assembly, wall
    time around a call that ends with the bytes on the host;
    and the sizes of the three files.
(d) render_results in frames/s over a synthetic KITTI directory of --frames
    car_600k frames (their image_2 files hold the picture): the 'bev' view and
    the 'camera' view with image_background, each as png/zlib, png/device and
    ppm, the three alternating in every round.
Device figures: median of five rounds, each the median of --calls calls, after
a warm-up.  Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

ROUNDS = 5


def picture(seed, h, w):
    import numpy as np
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 90 * np.sin(x / 40.0 + seed) * np.cos(y / 25.0),
                     128 + 90 * np.cos(x / 55.0) * np.sin(y / 30.0 + seed),
                     (x + 2 * y) / 8.0], axis=2)
    return ((base + rng.normal(0, 6, base.shape)).astype(np.int64) & 255
            ).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--images-only", action="store_true",
                    help="(a)-(c) only: kernel A/B runs under PGNN_LIB")
    args = ap.parse_args()
    import numpy as np
    import torch
    import pointgnn_amd  # noqa: F401
    from pointgnn_amd import _lib, kitti_dataset as KD, kitti_eval as KE
    from pointgnn_amd import png as P
    from pointgnn_amd import render as R, synthetic as S
    from render_time import seeded_boxes
    assert torch.cuda.is_available(), "png_encode_time.py needs the GPU"
    dev = torch.device("cuda", 0)
    lib = _lib.load()

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

    out = {"calls": args.calls, "rounds": ROUNDS, "lib": _lib.LIB_PATH}
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, "kitti")
        dirs = S.write_kitti_frames(root, range(args.frames),
                                    preset="car_600k")
        result_dir = os.path.join(tmp, "results")
        os.makedirs(result_dir)
        for i in range(args.frames):
            with open(os.path.join(result_dir, "%06d.txt" % i), "w") as f:
                for b in seeded_boxes(32, seed=i):
                    x, y, z, l, h, w, yaw = (float(t) for t in b)
                    f.write("Car -1 -1 0 100.0 100.0 200.0 180.0 %r %r %r %r "
                            "%r %r %r 0.9 \n" % (h, w, l, x, y, z, yaw))
        ds = KD.KittiDataset(*dirs)
        for i in range(args.frames):     # real files for image_background
            h, w = ds._image_shape(i)
            R.write_png(os.path.join(dirs[0], "%06d.png" % i),
                        picture(i, h, w))
        det = KE.read_result_file(os.path.join(result_dir, "000000.txt"))
        reader = R.image_background(ds)
        images = {
            "bev": R.render_frame(ds, 0, det, view='bev'),
            "camera": R.render_frame(ds, 0, det, view='camera',
                                     background=reader(0))}
        for name, image in images.items():
            h, w = int(image.shape[0]), int(image.shape[1])
            host = image.cpu().numpy()
            raw = np.zeros((h, 1 + 3 * w), dtype=np.uint8)
            raw[:, 1:] = host.reshape(h, 3 * w)
            raw = raw.tobytes()
            rec = {"size": [w, h], "raw_bytes": len(raw),
                   "pixels_lit": int((host != 0).any(axis=2).sum())}
            # (a)
            for level in (6, 1):
                rec["a_png_bytes_zlib%d_ms" % level] = host_ms(
                    lambda: R.png_bytes(image, level))
                rec["a_zlib%d_alone_ms" % level] = host_ms(
                    lambda: zlib.compress(raw, level))
                rec["file_bytes_zlib%d" % level] = len(R.png_bytes(image,
                                                                   level))
            # (b)
            c = P.DEFAULT_CHUNK_BYTES
            cap = P.deflate_capacity(h, w, c)
            ws_bytes = int(lib.pgnn_png_encode_workspace_bytes(h, w, c))
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            buf = torch.empty(cap, dtype=torch.uint8, device=dev)
            n_out = torch.empty(1, dtype=torch.int64, device=dev)

            def entry():
                _lib.check(lib.pgnn_png_encode(
                    _lib.ptr(image), h, w, 3 * w, c, _lib.ptr(ws), ws_bytes,
                    _lib.ptr(buf), cap, _lib.ptr(n_out), _lib.stream_ptr()),
                    "pgnn_png_encode")
            rec["b_device_entry_ms"] = device_ms(entry)
            # (c)
            rec["c_encode_png_whole_ms"] = host_ms(lambda: P.encode_png(image))
            data = P.encode_png(image)
            rec["file_bytes_device"] = len(data)
            rec["size_ratio_device_over_zlib6"] = len(data) / float(
                rec["file_bytes_zlib6"])
            assert torch.equal(P.read_png(data, order='rgb'), image)
            out[name] = rec
        # (d)
        kinds = (("png_zlib", "png", "zlib"), ("png_device", "png", "device"),
                 ("ppm", "ppm", "zlib"))
        for view, bg in (() if args.images_only else
                         (("bev", None), ("camera", reader))):
            rates = {k[0]: [] for k in kinds}
            enc = {k[0]: [] for k in kinds}
            for rep in range(ROUNDS + 1):        # the first pass warms up
                for key, fmt, encoder in kinds:
                    td = {}
                    t0 = time.time()
                    R.render_results(ds, result_dir, os.path.join(
                        tmp, "img_%s_%s_%d" % (view, key, rep)), views=(view,),
                        fmt=fmt, background_reader=bg, time_dict=td,
                        png_encoder=encoder)
                    wall = time.time() - t0
                    if rep:
                        rates[key].append(args.frames / wall)
                        enc[key].append(td.get('encode png', 0.0) / wall)
            for key, _, _ in kinds:
                out["d_%s_%s_frames_per_s" % (view, key)] = [
                    float(np.median(rates[key])), min(rates[key]),
                    max(rates[key])]
                if key != "ppm":
                    out["d_%s_%s_encode_share_of_wall" % (view, key)] = float(
                        np.median(enc[key]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
