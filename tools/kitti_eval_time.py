"""Times pointgnn_amd.kitti_eval.evaluate on a synthetic input of the KITTI val
split's size (3 769 frames, about 10 ground truths and 15 detections each,
fixed seed), and the tests' host restatement on 200 of those frames.  A
measurement for DESIGN.md §9.5, not a test: there is no bar to meet.

    python tools/kitti_eval_time.py [--frames 3769] [--host-frames 200]
        [--aos] [--min-overlap official|loose|<9 numbers>]

--aos (orientation similarity, random alphas) and --min-overlap time the same
input through pgnn_kitti_eval_ex; without them the existing entry runs.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=3769)
    ap.add_argument("--host-frames", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--aos", action="store_true")
    ap.add_argument("--min-overlap", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import pointgnn_amd  # noqa: F401
    from pointgnn_amd import kitti_eval
    import _kitti_eval as K

    rng = np.random.default_rng(0)
    frames = [K.random_frame(rng, int(rng.integers(7, 14)),
                             int(rng.integers(3, 9)))
              for _ in range(args.frames)]
    gt = [f[0] for f in frames]
    det = [f[1] for f in frames]
    n_gt = sum(len(g) for g in gt)
    n_det = sum(len(d) for d in det)

    t0 = time.perf_counter()
    packed = kitti_eval.pack_labels(gt), kitti_eval.pack_labels(det)
    pack_s = time.perf_counter() - t0
    ex = args.aos or args.min_overlap is not None
    if ex:
        arng = np.random.default_rng(1)
        alphas = (arng.uniform(-np.pi, np.pi, n_gt),
                  arng.uniform(-np.pi, np.pi, n_det)) if args.aos \
            else (None, None)

        def run():
            return kitti_eval.run_packed_ex(*packed, *alphas,
                                            min_overlap=args.min_overlap)
    else:
        def run():
            return kitti_eval.run_packed(*packed)
    run()                                               # warm-up
    whole, device = [], []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(True), torch.cuda.Event(True)
        t0 = time.perf_counter()
        start.record()
        out = run()
        stop.record()
        result = kitti_eval.KittiEvalResult.from_buffer(
            out, ex=True, has_aos=args.aos) if ex \
            else kitti_eval.KittiEvalResult.from_buffer(out)
        whole.append(time.perf_counter() - t0)
        device.append(start.elapsed_time(stop) * 1e-3)

    n = min(args.host_frames, args.frames)
    t0 = time.perf_counter()
    host = K.evaluate_host(gt[:n], det[:n])
    host_s = time.perf_counter() - t0
    sub = kitti_eval.evaluate(gt[:n], det[:n])
    same = all(np.array_equal(getattr(sub, k), host[k])
               for k in ('counters', 'thresholds', 'n_gt'))

    print(json.dumps({
        "frames": args.frames, "ground_truths": n_gt, "detections": n_det,
        "entry": "pgnn_kitti_eval_ex" if ex else "pgnn_kitti_eval",
        "aos": args.aos, "min_overlap": args.min_overlap or "official",
        "pack_labels_s": round(pack_s, 4),
        # upload + nine launches + one read, host clock / events around the
        # upload and the launches
        "evaluate_packed_s_median": round(float(np.median(whole)), 5),
        "upload_and_kernels_s_median": round(float(np.median(device)), 5),
        "evaluate_packed_s_calls": [round(x, 5) for x in whole],
        "car_3d_moderate_ap_r40": result.ap('3d', 'Car', 1),
        "host_restatement_frames": n,
        "host_restatement_s": round(host_s, 2),
        "host_restatement_agrees": bool(same),
    }))


if __name__ == "__main__":
    main()
