#!/usr/bin/env python
"""Time text drawing (csrc/render.hip pgnn_render_text, pointgnn_amd.render
draw_text) on a 1242 x 375 image, with the method of tools/render_time.py.

    python tools/text_time.py [--frames 8] [--calls 20]

(a) the ~20 strings of a typical frame ('C | 0.912' and class names);
(b) 1 000 strings of 12 characters, seeded positions;
    each as draw_text (it uploads the characters, offsets and anchors) and as
    the C entry alone on arrays already on the device (its three launches);
(c) render_results in frames/s over a synthetic KITTI directory of --frames
    car_600k frames, png and ppm, without and with text=True, the two
    alternating in every round.
A call is timed between device events; every figure is the median of five
rounds, each the median of --calls calls, after a warm-up, in one process.
Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS = 5
W, H = 1242, 375


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    import numpy as np
    import torch
    import pointgnn_amd  # noqa: F401
    from pointgnn_amd import _lib, kitti_dataset as KD
    from pointgnn_amd import render as R, synthetic as S
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from render_time import seeded_boxes
    assert torch.cuda.is_available(), "text_time.py needs the GPU"
    dev = torch.device("cuda", 0)
    lib = _lib.load()

    def timed(fn):
        """-> (median of the rounds' medians, smallest, largest round), ms"""
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

    rng = np.random.default_rng(0)
    image = torch.from_numpy(rng.integers(0, 256, (H, W, 3)).astype(
        np.uint8)).to(dev)
    frame = ['C | %.3f' % s for s in rng.uniform(0.3, 1.0, 12)] + \
        ['P | %.3f' % s for s in rng.uniform(0.3, 1.0, 3)] + \
        ['Car', 'Car', 'Van', 'Pedestrian', 'Cyclist']
    many = [''.join(chr(c) for c in rng.integers(0x21, 0x7F, 12))
            for _ in range(1000)]
    out = {"canvas": [W, H], "calls": args.calls, "rounds": ROUNDS}
    for key, strings in (("a_frame", frame), ("b_1000x12", many)):
        n = len(strings)
        anchors = np.stack([rng.integers(0, W - 60, n),
                            rng.integers(8, H, n)], axis=1)
        colors = rng.integers(0, 256, (n, 3)).astype(np.uint8)
        out[key + "_strings"] = n
        out[key + "_draw_text_ms"] = timed(lambda: R.draw_text(
            image, strings, anchors, colors=colors))
        # the entry alone
        data = [s.encode() for s in strings]
        offsets = np.zeros(n + 1, np.int32)
        offsets[1:] = np.cumsum([len(d) for d in data])
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        chars = T(np.frombuffer(b''.join(data), np.uint8).copy())
        off_t, col_t = T(offsets), T(colors)
        anc_t = T((anchors - [0, 7]).astype(np.int32))
        ws_bytes = int(lib.pgnn_render_text_workspace_bytes(W, H))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)

        def entry():
            _lib.check(lib.pgnn_render_text(
                _lib.ptr(image), W, H, _lib.ptr(chars), _lib.ptr(off_t), n,
                _lib.ptr(anc_t), None, 1, _lib.ptr(col_t), n, None, 0,
                _lib.ptr(ws), ws_bytes, _lib.stream_ptr()), "pgnn_render_text")
        out[key + "_entry_ms"] = timed(entry)
    # (c)
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
        for fmt in ("png", "ppm"):
            rates = {False: [], True: []}
            for rep in range(ROUNDS + 1):       # the first pass warms up
                for text in (False, True):
                    t0 = time.time()
                    R.render_results(ds, result_dir, os.path.join(
                        tmp, "img_%s_%d_%d" % (fmt, rep, text)), fmt=fmt,
                        text=text)
                    wall = time.time() - t0
                    if rep:
                        rates[text].append(args.frames / wall)
            for text in (False, True):
                out["c_%s%s_frames_per_s" % (fmt, "_text" if text else "")] = [
                    float(np.median(rates[text])), min(rates[text]),
                    max(rates[text])]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
