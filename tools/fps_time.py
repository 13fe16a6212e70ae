#!/usr/bin/env python
"""Time farthest-point sampling on the device (pgnn_farthest_first,
sampling.launch) beside the same loop written with torch ops on the same device
and the NumPy loop of dataset/kitti_dataset.py:630-641 on the host.

    python tools/fps_time.py [--calls 5] [--markdown profiles/fps_time.md]

Clouds: the synthetic `car_600k` frames (float32, camera frame).
  one       seed 0 alone (resident tier: coordinates and distances on chip)
  eight     seeds 0..7 as eight segments of one call (one workgroup each)
  large     seeds 0..6 concatenated into ONE cloud (streaming tier)
  one f64   seed 0 widened: above the float64 resident limit, so streaming
  small     the `tiny` preset (1 500 points, three strides of the workgroup):
            what a round costs when there is next to nothing to compute
K: the 'center' method's level-1 keypoint count on seed 0 under car_auto_T3's
runtime kwargs, 256 and 1024.
A call is timed between device events, after a warm-up; every kernel figure is
(median of five rounds, smallest round, largest round), each round the median
of --calls calls; us/round divides by the k - 1 rounds of a call.  The torch
loop and the NumPy loop are timed once per K (three calls / one call): they are
there for scale.  Every timed result is first checked against the NumPy loop
with `==`.  Prints one JSON line."""
import argparse
import datetime
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS = 5


def numpy_loop(pts, k, start):
    """:630-641 with the start index given -> idx [k]"""
    import numpy as np
    p = pts.astype(np.float64)

    def dist(p0):
        d = p0[None, :] - p
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    idx = np.zeros(k, np.int32)
    idx[0] = start
    d = dist(p[start])
    for i in range(1, k):
        j = int(np.argmax(d))
        idx[i] = j
        d = np.minimum(d, dist(p[j]))
    return idx


def torch_loop(torch, p64, k, start):
    """the same loop with torch ops, nothing read back -> idx [k] on the
    device.  (torch.argmax does not promise the first maximum: on clouds with
    ties this baseline may pick another index; the timed clouds have none.)"""
    idx = torch.zeros(k, dtype=torch.int64, device=p64.device)
    cur = torch.full((1,), start, dtype=torch.int64, device=p64.device)
    idx[0:1] = cur
    d = None
    for i in range(1, k):
        diff = p64.index_select(0, cur) - p64
        sq = diff * diff
        new = (sq[:, 0] + sq[:, 1]) + sq[:, 2]
        d = new if d is None else torch.minimum(d, new)
        cur = torch.argmax(d).reshape(1)
        idx[i:i + 1] = cur
    return idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--markdown", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import pointgnn_amd  # noqa: F401
    from pointgnn_amd import _lib, configs, graph_gen, sampling
    from pointgnn_amd.synthetic import synthetic_cloud
    assert torch.cuda.is_available(), "fps_time.py needs the GPU"
    dev = torch.device("cuda", 0)
    _lib.load()

    def timed(fn, calls=args.calls, rounds=ROUNDS, warm=3):
        """-> (median of the rounds' medians, smallest, largest round), ms"""
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(rounds):
            ms = []
            for _ in range(calls):
                a, b = torch.cuda.Event(True), torch.cuda.Event(True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            out.append(float(np.median(ms)))
        return [float(np.median(out)), min(out), max(out)]

    clouds = [synthetic_cloud(seed=s, preset="car_600k")[0] for s in range(8)]
    cfg = configs.get_config("car_auto_T3")
    rk = cfg["runtime_graph_gen_kwargs"]
    coords, _ = graph_gen.multi_layer_downsampling_select(
        torch.from_numpy(clouds[0]).to(dev), rk["base_voxel_size"],
        [rk["level_configs"][0]["graph_scale"]])
    k_center = int(coords[1].shape[0])
    ks = (k_center, 256, 1024)
    start = 0

    def device_cloud(parts, dtype):
        sizes = [len(c) for c in parts]
        p = torch.from_numpy(np.concatenate(parts).astype(dtype)).to(dev)
        off = torch.from_numpy(np.concatenate(
            [[0], np.cumsum(sizes)]).astype(np.int32)).to(dev)
        st = torch.full((len(parts),), start, dtype=torch.int32, device=dev)
        return p.contiguous(), off, st

    layouts = (
        ("one", [clouds[0]], np.float32, False),
        ("eight segments", clouds, np.float32, True),
        ("large (seeds 0..6 as one cloud)", [np.concatenate(clouds[:7])],
         np.float32, False),
        ("one, float64", [clouds[0]], np.float64, False),
        ("small (`tiny` preset)",
         [synthetic_cloud(seed=0, preset="tiny")[0]], np.float32, False),
    )
    rows = []
    host = {}
    for k in ks:
        t0 = time.perf_counter()
        want = numpy_loop(clouds[0], k, start)
        host[k] = (want, (time.perf_counter() - t0) * 1e3)
    for name, parts, dtype, segmented in layouts:
        p, off, st = device_cloud(parts, dtype)
        limit = sampling.RESIDENT[np.dtype(dtype)]
        tier = "resident" if max(len(c) for c in parts) <= limit else \
            "streaming"
        for k in ks:
            if (tier == "streaming" and k > 1024) or k > len(parts[0]):
                continue
            run = lambda: sampling.launch(p, off if segmented else None, st, k)
            idx = run()[0].cpu().numpy()
            # results first: the first cloud of every layout but `large` is
            # seed 0, whose picks the host loop gave
            if len(parts[0]) == len(clouds[0]):
                assert np.array_equal(idx[0], host[k][0]), (name, k)
            else:
                assert np.array_equal(
                    idx[0], numpy_loop(parts[0].astype(dtype), k, start))
            ms = timed(run)
            rows.append({"cloud": name, "dtype": np.dtype(dtype).name,
                         "tier": tier,
                         "points": [len(c) for c in parts], "k": k,
                         "kernel_ms": ms,
                         "us_per_round": ms[0] * 1e3 / max(k - 1, 1)})
    p64 = torch.from_numpy(clouds[0].astype(np.float64)).to(dev)
    base = []
    for k in ks:
        got = torch_loop(torch, p64, k, start).cpu().numpy()
        same = bool(np.array_equal(got, host[k][0]))
        ms = timed(lambda: torch_loop(torch, p64, k, start), calls=3,
                   rounds=1, warm=1)
        base.append({"k": k, "torch_ms": ms[0], "torch_equal": same,
                     "torch_us_per_round": ms[0] * 1e3 / max(k - 1, 1),
                     "numpy_ms": host[k][1],
                     "numpy_us_per_round": host[k][1] * 1e3 / max(k - 1, 1)})
    out = {"date": datetime.date.today().isoformat(), "calls": args.calls,
           "rounds": ROUNDS, "k_center": k_center, "rows": rows,
           "baselines": base,
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out))
    if args.markdown:
        span = lambda t: "%.3f (%.3f - %.3f)" % tuple(t)
        lines = [
            "# Farthest-point sampling: tools/fps_time.py",
            "",
            "%s, %s; --calls %d, %d rounds; `car_600k` frames; K of the "
            "'center' method on seed 0: %d." % (
                out["date"], out["device"], args.calls, ROUNDS, k_center),
            "",
            "| cloud | dtype | tier | points | k | kernel ms per call | "
            "us per round |",
            "|---|---|---|---|---|---|---|"]
        for r in rows:
            pts = r["points"]
            lines.append("| %s | %s | %s | %s | %d | %s | %.2f |" % (
                r["cloud"], r["dtype"], r["tier"],
                pts[0] if len(pts) == 1 else "%d x ~%d" % (
                    len(pts), int(np.mean(pts))),
                r["k"], span(r["kernel_ms"]), r["us_per_round"]))
        lines += [
            "",
            "Seed 0 alone, the same loop elsewhere (float64 arithmetic; the "
            "torch loop enqueues about eight kernels a round and reads "
            "nothing back):",
            "",
            "| k | torch ops on the device, ms | us per round | equal picks | "
            "NumPy on the host, ms | us per round |",
            "|---|---|---|---|---|---|"]
        for b in base:
            lines.append("| %d | %.1f | %.1f | %s | %.0f | %.0f |" % (
                b["k"], b["torch_ms"], b["torch_us_per_round"],
                "yes" if b["torch_equal"] else "no", b["numpy_ms"],
                b["numpy_us_per_round"]))
        os.makedirs(os.path.dirname(os.path.abspath(args.markdown)),
                    exist_ok=True)
        with open(args.markdown, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
