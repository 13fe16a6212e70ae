#!/usr/bin/env python
"""Time the rasteriser (csrc/render.hip, pointgnn_amd.render) on the
`car_600k` seed-0 frame in the 800 x 800 bird's eye view.

    python tools/render_time.py [--frames 8] [--calls 20]

(a) render() of the cloud and 32 seeded car-sized boxes (384 segments);
(b) the same with the level-1 graph (keypoint to keypoint edges of the
    car_auto_T3 runtime graph) as segments, the gather of graph_segments
    timed apart;
(c) render_results in frames/s over a synthetic KITTI directory of --frames
    car_600k frames, for png and ppm, with the host time spent in zlib.
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


def seeded_boxes(n, seed=0):
    import numpy as np
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-30, 30, n), np.full(n, 1.7),
                     rng.uniform(5, 70, n), rng.uniform(3.2, 4.8, n),
                     rng.uniform(1.4, 1.9, n), rng.uniform(1.5, 1.9, n),
                     rng.uniform(-3.14, 3.14, n)], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--config", default="car_auto_T3")
    args = ap.parse_args()
    import numpy as np
    import torch
    import pointgnn_amd  # noqa: F401
    from pointgnn_amd import configs, graph_gen, kitti_dataset as KD
    from pointgnn_amd import render as R, synthetic as S
    assert torch.cuda.is_available(), "render_time.py needs the GPU"
    dev = torch.device("cuda", 0)

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

    cfg = configs.get_config(args.config)
    xyz, inten = S.synthetic_cloud(seed=0, preset="car_600k")
    pts = torch.from_numpy(xyz).to(dev)
    view = R.bev_view()
    colors = R.colorize(torch.from_numpy(inten[:, 0].copy()).to(dev), 0.0, 1.0)
    boxes = torch.from_numpy(R.box_segments(seeded_boxes(32))).to(dev)
    red = torch.tensor([[255, 0, 0]], dtype=torch.uint8, device=dev)
    out = {"points": int(len(xyz)), "box_segments": int(boxes.shape[0]),
           "canvas": [view.width, view.height], "calls": args.calls,
           "rounds": ROUNDS}
    # (a)
    out["a_cloud_boxes_ms"] = timed(lambda: R.render(
        view, points=pts, point_colors=colors, segments=boxes,
        segment_colors=red))
    # (b)
    fn = graph_gen.get_graph_generate_fn(cfg['graph_gen_method'])
    coords, kps, edges = fn(pts, **cfg['runtime_graph_gen_kwargs'])
    level = len(edges) - 1
    gseg = R.graph_segments(coords, edges, level)
    out["graph_segments"] = int(gseg.shape[0])
    out["b_graph_segments_gather_ms"] = timed(
        lambda: R.graph_segments(coords, edges, level))
    seg = torch.cat([gseg.to(torch.float64), boxes])
    scol = torch.cat([
        torch.tensor([[0, 120, 255]], dtype=torch.uint8,
                     device=dev).repeat(int(gseg.shape[0]), 1),
        red.repeat(int(boxes.shape[0]), 1)])
    out["b_cloud_graph_boxes_ms"] = timed(lambda: R.render(
        view, points=pts, point_colors=colors, segments=seg,
        segment_colors=scol))
    seg32 = seg.to(torch.float32)
    out["b_cloud_graph_boxes_f32_ms"] = timed(lambda: R.render(
        view, points=pts, point_colors=colors, segments=seg32,
        segment_colors=scol))
    img = R.render(view, points=pts, point_colors=colors, segments=seg,
                   segment_colors=scol)
    out["b_pixels_lit"] = int((img != 0).any(dim=2).sum().item())
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
            rates, enc = [], []
            for rep in range(ROUNDS + 1):       # the first pass warms up
                td = {}
                t0 = time.time()
                R.render_results(ds, result_dir,
                                 os.path.join(tmp, "img_%s_%d" % (fmt, rep)),
                                 fmt=fmt, time_dict=td)
                wall = time.time() - t0
                if rep:
                    rates.append(args.frames / wall)
                    enc.append(td.get('encode png', 0.0) / wall)
            out["c_%s_frames_per_s" % fmt] = [float(np.median(rates)),
                                               min(rates), max(rates)]
            if fmt == "png":
                out["c_png_zlib_share_of_wall"] = float(np.median(enc))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
