#!/usr/bin/env python
"""Time the plain kNN graph (pgnn_knn_nearest, graph_gen.knn_nearest_device:
the k nearest points, no radius) on the level-0 and level-1 point and centre
sets of the `car_600k` seed-0 frame under car_auto_T3.

    python tools/knn_nearest_time.py [--calls 10] \
        [--markdown profiles/knn_nearest.md]

Per level and k = 16, 64, 256:
  nearest_ms   knn_nearest_device at every cell_size of CELLS (no host read)
               and at the default (None: one host read of the bounding box;
               the cell it chose is reported)
  cdist_ms     (a) torch.cdist + topk(k, largest=False) on the device, centres
               in chunks of CDIST_CHUNK rows -- unordered ties, float32: a
               time to compare with, not the same rows
  covering_ms  (b) knn_graph_device (pgnn_knn_graph_count + _fill) at a radius
               that covers the cloud: the same rows, one cell
  consumer_us  the kernel that consumes the list, launched alone on it: the
               pooling kernel (level 0) or the fused edge kernel (level 1,
               bench.roofline_edge_kernel); E = centres * k
and the expected worst case, far-field centres: FAR_N level-1 centres moved
FAR_OFFSET metres off the cloud, at k = 16 over the cell sizes of FAR_CELLS
(few calls: a call can take seconds).
A call is timed between device events; every figure is (median of the rounds,
smallest round, largest round), each round the median of --calls calls, after
a warm-up, in one process.  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS = 5
KS = (16, 64, 256)
CELLS = (0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0)
CDIST_CHUNK = 1024
FAR_N, FAR_OFFSET, FAR_CELLS = 64, 200.0, (0.5, 1.0, 4.0, 16.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--markdown", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import pointgnn_amd  # noqa: F401
    from pointgnn_amd import _lib, configs, gnn, graph_gen, weights
    from pointgnn_amd.engine import InferenceEngine
    from pointgnn_amd.synthetic import synthetic_cloud
    import bench
    assert torch.cuda.is_available(), "knn_nearest_time.py needs the GPU"
    dev = torch.device("cuda", 0)
    lib = _lib.load()

    def timed(fn, calls=None, rounds=ROUNDS, warm=3):
        """-> (median of the rounds' medians, smallest, largest round), ms"""
        calls = calls or args.calls
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

    def pool_kernel_us(eng, x, f, kps, e0):
        """the pooling kernel alone on the level-0 list `e0` (the launch of
        bench.roofline_pool_kernel; as tools/knn_time.py)"""
        lc = eng.config['model_kwargs']['layer_configs'][0]
        widths = list(lc['kwargs']['point_MLP_depth_list'])
        chain = eng.model._store._cache.get(
            ('mlp', lc['scope'] + '/extract_vertex_features', tuple(widths),
             False))
        if chain is None:
            return None
        kp = kps[0].reshape(-1).to(torch.int32).contiguous()
        n_feat, k, n_e = int(f.shape[1]), int(kp.shape[0]), int(e0.shape[0])
        agg = torch.empty((k, gnn.padded_width(chain.n_out)), device=dev)
        ws_bytes = ctypes.c_size_t(0)
        _lib.check(lib.pgnn_point_set_pooling_workspace_bytes(
            chain.array, chain.n, n_feat, n_e, 0, ctypes.byref(ws_bytes)),
            "pooling workspace query")
        work = torch.empty(max(ws_bytes.value // 4, 1), device=dev)

        def run():
            _lib.check(lib.pgnn_point_set_pooling_fwd_ws(
                _lib.ptr(f), n_feat, _lib.ptr(x), _lib.ptr(kp), _lib.ptr(e0),
                n_e, k, chain.array, chain.n, 1, _lib.ptr(agg), agg.stride(0),
                _lib.ptr(_lib.sched_ws()), None, None,
                _lib.ptr(work) if ws_bytes.value else None, ws_bytes.value,
                _lib.stream_ptr()), "pooling kernel")
        return bench.time_kernel(run, args.reps, torch) * 1e6

    def cdist_topk(p, c, k):
        for q0 in range(0, int(c.shape[0]), CDIST_CHUNK):
            torch.cdist(c[q0:q0 + CDIST_CHUNK], p).topk(
                min(k, int(p.shape[0])), dim=1, largest=False)

    cfg = configs.get_config("car_auto_T3")
    eng = InferenceEngine(cfg, weights.init_params(cfg, seed=0,
                                                   bias_scale=0.05),
                          device=dev)
    xyz, inten = synthetic_cloud(seed=0, preset="car_600k")
    x, f = torch.from_numpy(xyz).to(dev), torch.from_numpy(inten).to(dev)
    eng.run_frame(x, f)
    coords, kps, edges = eng.last_graph
    n_k = int(coords[1].shape[0])
    rows, far_rows = [], []
    for level in (0, 1):
        kw = cfg['runtime_graph_gen_kwargs']['level_configs'][level][
            'graph_gen_kwargs']
        p, c = coords[level].contiguous(), coords[level + 1].contiguous()
        scale = kw.get('scale')
        both = torch.cat([p, c])
        cover = 2.0 * float((both.max(0).values - both.min(0).values).norm()) \
            + 1.0

        def consumer_us(e):
            e = e.contiguous()
            if level == 0:
                return pool_kernel_us(eng, x, f, kps, e)
            r = bench.roofline_edge_kernel(torch, eng, e, n_k, reps=args.reps,
                                           frame=(x, f))
            return r["avg_launch_us"] if r else None

        for k in KS:
            e_near = graph_gen.knn_nearest_device(p, c, k, scale, 1.0)
            e_cov, _ = graph_gen.knn_graph_device(p, c, cover, k, scale)
            assert torch.equal(e_near, e_cov), "the two kernels disagree"
            rows.append({
                "graph": "car_600k level %d" % level, "k": k,
                "points": int(p.shape[0]), "centres": int(c.shape[0]),
                "E": int(e_near.shape[0]),
                "E_radius": int(edges[level].shape[0]),
                "nearest_ms": {
                    "%g" % cell: timed(lambda: graph_gen.knn_nearest_device(
                        p, c, k, scale, cell)) for cell in CELLS},
                "default_cell": graph_gen._nearest_default_cell(p, scale, k),
                "default_ms": timed(lambda: graph_gen.knn_nearest_device(
                    p, c, k, scale)),
                "cdist_ms": timed(lambda: cdist_topk(p, c, k)),
                "covering_ms": timed(lambda: graph_gen.knn_graph_device(
                    p, c, cover, k, scale)),
                "consumer": "pooling" if level == 0 else "edge",
                "consumer_radius_us": consumer_us(edges[level]),
                "consumer_nearest_us": consumer_us(e_near)})
        if level == 1:
            far = (c[:FAR_N] + FAR_OFFSET).contiguous()
            for cell in FAR_CELLS:
                far_rows.append({
                    "cell": cell, "k": 16, "points": int(p.shape[0]),
                    "centres": FAR_N, "offset_m": FAR_OFFSET,
                    "ms": timed(lambda: graph_gen.knn_nearest_device(
                        p, far, 16, scale, cell), calls=3, rounds=3, warm=1)})
    out = {"calls": args.calls, "rounds": ROUNDS, "reps": args.reps,
           "rows": rows, "far_field": far_rows}
    print(json.dumps(out))
    if args.markdown:
        span = lambda t: "%.3f (%.3f - %.3f)" % tuple(t)
        us = lambda v: "n/a" if v is None else "%.0f" % v
        lines = [
            "| graph | k | points | centres | E = centres x k | E radius | " +
            " | ".join("cell %g ms" % c for c in CELLS) +
            " | default cell | default ms | cdist + topk ms | "
            "kNN within covering radius ms | consumer | radius list us | "
            "nearest list us |",
            "|" + "---|" * (13 + len(CELLS))]
        for r in rows:
            lines.append("| %s | %d | %d | %d | %d | %d | %s | %.3g | %s | %s "
                         "| %s | %s | %s | %s |" % (
                             r["graph"], r["k"], r["points"], r["centres"],
                             r["E"], r["E_radius"],
                             " | ".join(span(r["nearest_ms"]["%g" % c])
                                        for c in CELLS),
                             r["default_cell"], span(r["default_ms"]),
                             span(r["cdist_ms"]), span(r["covering_ms"]),
                             r["consumer"], us(r["consumer_radius_us"]),
                             us(r["consumer_nearest_us"])))
        lines += ["", "Far-field centres (%d level-1 centres moved %g m off "
                  "the cloud, k = 16; 3 rounds of 3 calls):" % (FAR_N,
                                                                FAR_OFFSET),
                  "", "| cell | points | centres | ms |", "|---|---|---|---|"]
        for r in far_rows:
            lines.append("| %g | %d | %d | %s |" % (
                r["cell"], r["points"], r["centres"], span(r["ms"])))
        os.makedirs(os.path.dirname(os.path.abspath(args.markdown)),
                    exist_ok=True)
        with open(args.markdown, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
