"""Times pgnn_kitti_match on generated frame sets of 8 frames
and of the KITTI val split's size (3 769 frames; tests/_kitti_eval.py's
generator, about 10 ground truths and 15 detections a frame, fixed seed) and
writes profiles/kitti_match.md.  Three numbers per set, 3D / Car / moderate at
threshold 0.5:

    entry         pgnn_kitti_match alone: inputs, workspace and outputs are on
                  the device already; device events around `calls` calls in a
                  row, divided by `calls`
    match         kitti_eval.match: pack_labels, the uploads, the entry, the
                  reads of the six outputs; a host clock
    restatement   tests/_kitti_match.py::match_set on the same frames, fed the
                  device's overlap table (its time does not hold the overlaps;
                  the entry's does)

A measurement, not a test: there is no bar to meet.  The restatement must
return the device's arrays, or the tool fails.

    python tools/kitti_match_time.py [--frames 8 3769] [--repeats 7]
        [--calls 20] [--out profiles/kitti_match.md]
"""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

COMBO = (2, 0, 1)           # 3D, Car, moderate
THRESHOLD, LOC_FLOOR = 0.5, 0.1


def measure(n_frames, repeats, calls):
    import numpy as np
    import torch
    from pointgnn_amd import _lib, kitti_eval
    import _kitti_eval as K
    import _kitti_match as M

    rng = np.random.default_rng(0)
    frames = [K.random_frame(rng, int(rng.integers(7, 14)),
                             int(rng.integers(3, 9))) for _ in range(n_frames)]
    gt, det = [f[0] for f in frames], [f[1] for f in frames]
    (gt_off, gt_rows, gt_names), (det_off, det_rows, det_names) = \
        kitti_eval.pack_labels(gt), kitti_eval.pack_labels(det)
    n_gt, n_det = len(gt_rows), len(det_rows)
    n_pairs = kitti_eval._pair_count(gt_off, det_off)

    # ---- the entry alone
    lib = _lib.load()
    dev = torch.device('cuda')
    d_in = [torch.from_numpy(a).to(dev) for a in (gt_rows, gt_names, det_rows,
                                                  det_names)]
    ws = torch.empty(int(lib.pgnn_kitti_match_workspace_bytes(
        n_frames, n_gt, n_det, n_pairs)), dtype=torch.uint8, device=dev)
    outs = [torch.empty(n_gt, dtype=torch.int32, device=dev),
            torch.empty(n_gt, dtype=torch.int32, device=dev),
            torch.empty(n_det, dtype=torch.int32, device=dev),
            torch.empty(n_det, dtype=torch.int32, device=dev),
            torch.empty(n_det, dtype=torch.float64, device=dev),
            torch.empty(18, dtype=torch.int64, device=dev)]

    def entry():
        _lib.check(lib.pgnn_kitti_match(
            ctypes.c_void_p(gt_off.ctypes.data),
            ctypes.c_void_p(det_off.ctypes.data), n_frames,
            *[_lib.ptr(t) for t in d_in], None, *COMBO, THRESHOLD, LOC_FLOOR,
            _lib.ptr(ws), ws.numel(), *[_lib.ptr(t) for t in outs],
            _lib.stream_ptr()), "pgnn_kitti_match")
    entry()
    torch.cuda.synchronize()
    entry_s = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(True), torch.cuda.Event(True)
        start.record()
        for _ in range(calls):
            entry()
        stop.record()
        torch.cuda.synchronize()
        entry_s.append(start.elapsed_time(stop) * 1e-3 / calls)

    # ---- match, from label dictionaries to host arrays
    kitti_eval.match(gt, det, *COMBO, score_threshold=THRESHOLD)
    match_s = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = kitti_eval.match(gt, det, *COMBO, score_threshold=THRESHOLD)
        match_s.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    kitti_eval.pack_labels(gt), kitti_eval.pack_labels(det)
    pack_s = time.perf_counter() - t0

    # ---- the restatement on the device's overlaps
    flat, pair_off = kitti_eval.pair_overlaps(gt, det)
    ov = [flat[:, pair_off[f]:pair_off[f + 1]].reshape(4, len(g), len(a))
          for f, (g, a) in enumerate(zip(gt, det))]
    t0 = time.perf_counter()
    want = M.match_set(gt, det, ov, *COMBO, THRESHOLD, loc_floor=LOC_FLOOR)
    host_s = time.perf_counter() - t0
    for key in ('det_outcome', 'det_partner', 'det_overlap', 'gt_outcome',
                'gt_partner'):
        assert np.array_equal(getattr(res, key), want[key]), key
    assert (res.tp, res.fp, res.fn) == M.counts(want)
    med = lambda xs: float(np.median(xs))
    return {'frames': n_frames, 'n_gt': n_gt, 'n_det': n_det,
            'n_pairs': n_pairs, 'entry_s': med(entry_s),
            'entry_spread': (min(entry_s), max(entry_s)),
            'match_s': med(match_s), 'match_spread': (min(match_s),
                                                      max(match_s)),
            'pack_s': pack_s, 'host_s': host_s,
            'counts': (res.tp, res.fp, res.fn)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs='+', default=[8, 3769])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles",
                                                  "kitti_match.md"))
    args = ap.parse_args()
    import torch
    import pointgnn_amd  # noqa: F401
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    rows = [measure(n, args.repeats, args.calls) for n in args.frames]
    ms = lambda s: '%.3f' % (1e3 * s)
    lines = [
        "# pgnn_kitti_match: per-box outcomes at one threshold",
        "",
        "Written by `tools/kitti_match_time.py` on %s.  Generated frames "
        "(tests/_kitti_eval.py, seed 0), 3D / Car / moderate, threshold %.1f, "
        "loc_floor %.1f.  Medians of %d repeats (min .. max); the entry is "
        "timed with device events over %d calls in a row, the rest with a "
        "host clock.  Times in ms." % (
            torch.cuda.get_device_name(0), THRESHOLD, LOC_FLOOR, args.repeats,
            args.calls),
        "",
        "| frames | ground truths | detections | pairs | entry alone | "
        "`match` (pack, upload, entry, reads) | of which pack_labels | "
        "restatement (matching only) | restatement / `match` | "
        "restatement / entry |",
        "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(
            "| %d | %d | %d | %d | %s (%s .. %s) | %s (%s .. %s) | %s | %s | "
            "%.1f x | %.0f x |" % (
                r['frames'], r['n_gt'], r['n_det'], r['n_pairs'],
                ms(r['entry_s']), ms(r['entry_spread'][0]),
                ms(r['entry_spread'][1]), ms(r['match_s']),
                ms(r['match_spread'][0]), ms(r['match_spread'][1]),
                ms(r['pack_s']), ms(r['host_s']), r['host_s'] / r['match_s'],
                r['host_s'] / r['entry_s']))
    lines += [
        "",
        "The restatement is fed the device's overlap table, so its time is "
        "the matching and the classification alone; it returned the device's "
        "five arrays and (tp, fp, fn) = %s on the larger set." % (
            rows[-1]['counts'],),
        "The entry is four launches, two offset uploads and one memset "
        "whatever the number of frames; on the small set its time is that "
        "fixed cost."]
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
