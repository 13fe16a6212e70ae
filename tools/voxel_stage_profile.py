#!/usr/bin/env python
"""Time the voxel-average down-sampling stage (csrc/voxel_avg.hip) where it
runs: the frame fetch and the pipelined frame loop of pointgnn_amd.run on
synthetic KITTI-sized scans (~120 k points per .bin).

    python tools/voxel_stage_profile.py --mode loop  --voxel 0.4
    python tools/voxel_stage_profile.py --mode fetch --voxel 0.4
    rocprofv3 --kernel-trace --stats -d DIR -o run -- \\
        python tools/voxel_stage_profile.py --mode fetch --voxel 0.4

--mode loop: run_dataset (FramePipeline) over --frames frames, timed after a
warm-up pass; --mode fetch: get_cam_points_in_image_with_rgb alone, --frames
calls after a warm-up (under rocprofv3 every kernel of that trace belongs to
the fetch, so launches per frame can be counted).  --voxel none runs the same
loop without the key.  Keypoints are 'random' (the 'center' replica takes the
float32 cloud only).  Prints one JSON line."""
import argparse
import copy
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("loop", "fetch"), default="loop")
    ap.add_argument("--voxel", default="none")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--config", default="car_auto_T3")
    args = ap.parse_args()
    import numpy as np
    import torch
    import pointgnn_amd  # noqa: F401
    from pointgnn_amd import configs, kitti_dataset as KD, run as RUN, \
        synthetic as S, weights
    voxel = None if args.voxel == "none" else float(args.voxel)
    cfg = copy.deepcopy(configs.get_config(args.config))
    cfg['downsample_by_voxel_size'] = voxel
    cfg['runtime_graph_gen_kwargs']['downsample_method'] = 'random'
    cfg['runtime_graph_gen_kwargs']['add_rnd3d'] = False
    out = {"mode": args.mode, "voxel": voxel, "frames": args.frames,
           "config": args.config}
    with tempfile.TemporaryDirectory() as tmp:
        dirs = S.write_kitti_frames(os.path.join(tmp, "kitti"),
                                    list(range(args.frames)))
        ds = KD.KittiDataset(*dirs)
        out["scan_points"] = int(ds.get_velo_points(0).xyz.shape[0])
        if args.mode == "fetch":
            p = ds.get_cam_points_in_image_with_rgb(0, voxel)   # warm-up
            out["points_out"] = int(p.xyz.shape[0])
            torch.cuda.synchronize()
            t0 = time.time()
            for i in range(args.frames):
                ds.get_cam_points_in_image_with_rgb(i, voxel)
            torch.cuda.synchronize()
            out["fetch_ms_per_frame"] = 1e3 * (time.time() - t0) / args.frames
        else:
            params = weights.init_params(cfg, seed=3, bias_scale=0.05)
            rates = []
            for rep in range(args.repeats + 1):     # the first pass warms up
                np.random.seed(rep)
                td = RUN.run_dataset(ds, cfg, None,
                                     os.path.join(tmp, "out%d" % rep),
                                     params=params)
                torch.cuda.synchronize()
                if rep:
                    rates.append(td['frames'] / td['wall'])
                out["sequential_fallbacks"] = td.get('sequential fallbacks', 0)
            out["frames_per_s"] = rates
            out["frames_per_s_median"] = float(np.median(rates))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
