#!/usr/bin/env python
"""Time the beam decimation (csrc/beam.hip, pointgnn_amd.beam_downsample) on
generated HDL-64-like scans of ~120 k rows (tests/_beam.py hdl64_scan).

    python tools/beam_downsample_time.py --mode device
    python tools/beam_downsample_time.py --mode sklearn
    python tools/beam_downsample_time.py --mode loop
    rocprofv3 --kernel-trace --stats -d DIR -o run -- \\
        python tools/beam_downsample_time.py --mode calls

device   downsample_rows between events, median of --calls after a warm-up,
         and the same for the two entries apart
sklearn  KMeans(n_clusters=64) on the same scan's cosines on the host
loop     run_dataset frames/s with beam_downsample_rate=--rate against the
         same loop over the directory write_downsampled_dataset wrote
calls    --calls calls of downsample_rows and nothing else (every kernel of a
         rocprofv3 trace of this mode belongs to the decimation)
Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def write_tree(root, scans):
    """KITTI-object tree of the scans; the calibration is fitted to the
    returns in front of the camera (90 degrees of azimuth)."""
    import numpy as np
    from pointgnn_amd import synthetic as S
    dirs = [os.path.join(root, d) for d in ("image_2", "velodyne", "calib")]
    for d in dirs:
        os.makedirs(d)
    for i, velo in enumerate(scans):
        name = "%06d" % i
        velo.tofile(os.path.join(dirs[1], name + ".bin"))
        front = velo[(velo[:, 0] > 3) & (np.abs(velo[:, 1]) < 0.8 * velo[:, 0])]
        cam = np.stack([-front[:, 1] - 0.004, -front[:, 2] - 0.076,
                        front[:, 0] - 0.272], 1)
        lines, (height, width) = S.synthetic_calib(cam)
        with open(os.path.join(dirs[2], name + ".txt"), "w") as f:
            f.writelines(lines)
        S.write_png_header(os.path.join(dirs[0], name + ".png"), height, width)
    return dirs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("device", "sklearn", "loop", "calls"),
                    default="device")
    ap.add_argument("--rate", type=int, default=2)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--n-az", type=int, default=2400)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--config", default="car_auto_T3")
    args = ap.parse_args()
    import numpy as np
    import _beam as B
    velo = B.hdl64_scan(100, args.n_az, 0.4, 0.02)[0]
    out = {"mode": args.mode, "rate": args.rate, "rows": int(len(velo))}
    if args.mode == "sklearn":
        from sklearn.cluster import KMeans
        cos, valid = B.cos_valid(velo)
        times = []
        for _ in range(3):
            t0 = time.time()
            km = KMeans(n_clusters=64).fit(cos[valid][:, None])
            times.append(time.time() - t0)
        out["sklearn_kmeans_s"] = times
        out["sklearn_n_iter"] = int(km.n_iter_)
        print(json.dumps(out))
        return
    import torch
    import pointgnn_amd  # noqa: F401
    from pointgnn_amd import beam_downsample as BD
    dev = torch.device("cuda", 0)
    v = torch.from_numpy(velo).to(dev)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.calls):
            a, b = torch.cuda.Event(True), torch.cuda.Event(True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return float(np.median(ms)), float(min(ms))

    if args.mode == "calls":
        for _ in range(args.calls):
            rows = BD.downsample_rows(v, args.rate)
        out["rows_out"] = int(rows.shape[0])
    elif args.mode == "device":
        rows = BD.downsample_rows(v, args.rate)
        c, info = BD.beam_centers(v)
        out["rows_out"] = int(rows.shape[0])
        out["info"] = info.tolist()
        out["downsample_ms_median_min"] = timed(
            lambda: BD.downsample_rows(v, args.rate))
        out["beam_centers_ms_median_min"] = timed(lambda: BD.beam_centers(v))
        out["beam_select_ms_median_min"] = timed(
            lambda: BD.beam_select(v, c, args.rate, info=info))
    else:
        from pointgnn_amd import configs, kitti_dataset as KD, run as RUN, \
            weights
        cfg = configs.get_config(args.config)
        params = weights.init_params(cfg, seed=3, bias_scale=0.05)
        scans = [B.hdl64_scan(200 + i, args.n_az, 0.4, 0.02)[0]
                 for i in range(args.frames)]
        with tempfile.TemporaryDirectory() as tmp:
            dirs = write_tree(os.path.join(tmp, "kitti"), scans)
            pre_dir = os.path.join(tmp, "velodyne_pre")
            t0 = time.time()
            BD.write_downsampled_dataset(KD.KittiDataset(*dirs), pre_dir,
                                         args.rate)
            out["write_s_per_scan"] = (time.time() - t0) / args.frames
            sets = {"fetch": KD.KittiDataset(*dirs,
                                             beam_downsample_rate=args.rate),
                    "prewritten": KD.KittiDataset(dirs[0], pre_dir, dirs[2])}
            rates = {k: [] for k in sets}
            fetch = {k: [] for k in sets}
            # the two loops take turns; the first pass of each warms up
            for rep in range(args.repeats + 1):
                for name, ds in sets.items():
                    np.random.seed(rep)
                    td = RUN.run_dataset(ds, cfg, None, os.path.join(
                        tmp, "out_%s_%d" % (name, rep)), params=params)
                    torch.cuda.synchronize()
                    if rep:
                        rates[name].append(td['frames'] / td['wall'])
                        fetch[name].append(
                            1e3 * td['fetch input'] / td['frames'])
            for name, ds in sets.items():
                out[name + "_frames_per_s"] = rates[name]
                out[name + "_frames_per_s_median"] = float(
                    np.median(rates[name]))
                out[name + "_loader_fetch_ms_per_frame"] = float(
                    np.median(fetch[name]))
                # the fetch alone on an idle device (sequential loop)
                td = RUN.run_dataset(ds, cfg, None, os.path.join(
                    tmp, "out_%s_seq" % name), params=params, pipelined=False)
                out[name + "_sequential_fetch_ms_per_frame"] = \
                    1e3 * td['fetch input'] / td['frames']
                out[name + "_sequential_frames_per_s"] = \
                    td['frames'] / td['wall']
    print(json.dumps(out))


if __name__ == "__main__":
    main()
