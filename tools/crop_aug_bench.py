#!/usr/bin/env python
"""Time of crop_aug on a headline-size frame: the reference's own example
(models/crop_aug.py:216-229: Car 2 / Pedestrian 10 / Cyclist 10, 100 trials,
'box_and_point', auto_box_height, must_have_ground) on a 20 k-point frame of
pointgnn_amd.synthetic.  The object database is cut from other synthetic frames
with save_cropped_boxes.  Prints the median over `--calls` calls (after
warm-up) of the whole `CropAugSampler.crop_aug` call (host clock; the call ends
in its one host read) and of the placement kernel alone (HIP events round
pgnn_crop_aug_place), with the draws the kernel consumed.

    python tools/crop_aug_bench.py [--calls 30] [--labels 12]
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import pointgnn_amd  # noqa: E402,F401
from pointgnn_amd import crop_aug as CA  # noqa: E402
from pointgnn_amd.kitti_dataset import Points  # noqa: E402
from pointgnn_amd.synthetic import synthetic_cloud  # noqa: E402

SIZES = {'Car': (3.9, 1.5, 1.6), 'Pedestrian': (0.9, 1.8, 0.7),
         'Cyclist': (1.8, 1.7, 0.6)}
EXAMPLE = {'max_overlap_num_allowed': 50, 'max_trails': 100,
           'method_name': 'normal', 'yaw_std': np.pi / 16,
           'expand_factor': (1.1, 1.1, 1.1), 'auto_box_height': True,
           'overlap_mode': 'box_and_point', 'max_overlap_rate': 1e-6,
           'appr_factor': 100, 'must_have_ground': True}
RATE = {"Car": 2, "Pedestrian": 10, "Cyclist": 10}


def labels_on(xyz, rng, n, names=('Car', 'Pedestrian', 'Cyclist')):
    """n boxes standing on the ground (y = 1.73, camera y is down) at random
    points of the cloud nearer than 30 m."""
    near = xyz[xyz[:, 2] < 30.0]
    out = []
    for i in range(n):
        name = names[i % len(names)]
        l, h, w = np.array(SIZES[name]) * rng.uniform(0.9, 1.15, 3)
        c = near[int(rng.integers(len(near)))]
        out.append({'name': name, 'length': float(l), 'height': float(h),
                    'width': float(w), 'x3d': float(c[0]), 'y3d': 1.73,
                    'z3d': float(c[2]),
                    'yaw': float(rng.uniform(-np.pi, np.pi))})
    return out


class Frames(object):
    def __init__(self, seeds, n_labels):
        self.num_files = len(seeds)
        self._seeds, self._n = seeds, n_labels

    def _cloud(self, i):
        return synthetic_cloud(seed=self._seeds[i], preset="car")

    def get_label(self, i):
        return labels_on(self._cloud(i)[0],
                         np.random.default_rng(self._seeds[i]), self._n)

    def get_cam_points_in_image_with_rgb(self, i):
        xyz, inten = self._cloud(i)
        return Points(xyz=torch.from_numpy(xyz).cuda(),
                      attr=torch.from_numpy(inten).cuda())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--labels", type=int, default=12)
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        db = os.path.join(tmp, "db.json")
        CA.save_cropped_boxes(Frames(list(range(100, 112)), 30), db,
                              minimum_points=10)
        sampler = CA.CropAugSampler(db)
    frame = Frames([7], args.labels)
    pts = frame.get_cam_points_in_image_with_rgb(0)
    labels = frame.get_label(0)
    kernel_ms, seen = [], {}
    real_place = CA.place

    def timed_place(*a):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        out = real_place(*a)
        e1.record()
        seen["events"], seen["record"] = (e0, e1), out[2]
        return out
    CA.place = timed_place
    call_ms, draws, accepted, sizes = [], [], [], []
    np.random.seed(0)
    for i in range(args.warmup + args.calls):
        labs = [dict(l) for l in labels]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out, labs = sampler.crop_aug(pts, labs, sample_rate=RATE,
                                     parser_kwargs=EXAMPLE)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if i < args.warmup:
            continue
        call_ms.append((t1 - t0) * 1e3)
        kernel_ms.append(seen["events"][0].elapsed_time(seen["events"][1]))
        rec = seen["record"].cpu().numpy()
        draws.append(int(rec[-2]))
        accepted.append(len(labs) - len(labels))
        sizes.append(int(out.xyz.shape[0]))
    print("frame %d points, %d labels, %d samples, database %s" % (
        pts.xyz.shape[0], len(labels), sum(RATE.values()),
        {k: len(v) for k, v in sampler._cropped_labels.items()}))
    print("calls %d: draws consumed median %d (min %d, max %d of %d), "
          "accepted median %d, points out median %d" % (
              len(call_ms), np.median(draws), min(draws), max(draws),
              sum(RATE.values()) * EXAMPLE['max_trails'],
              np.median(accepted), np.median(sizes)))
    print("crop_aug call: median %.3f ms (min %.3f, max %.3f)" % (
        np.median(call_ms), min(call_ms), max(call_ms)))
    print("pgnn_crop_aug_place: median %.3f ms (min %.3f, max %.3f); "
          "%.1f us per draw" % (
              np.median(kernel_ms), min(kernel_ms), max(kernel_ms),
              1e3 * sum(kernel_ms) / max(sum(draws), 1)))


if __name__ == "__main__":
    main()
