#!/usr/bin/env python
"""Time the kNN-within-radius graph (pgnn_knn_graph_*, graph_gen.
knn_graph_device) against the existing way of bounding a neighbourhood to k
rows, the radius graph with the random fan-in cap
(graph_gen.radius_graph_device(..., num_neighbors=k)): count + fill + cap.

    python tools/knn_time.py [--calls 10] [--markdown profiles/knn_time.md]

Graphs: level 1 (keypoints to keypoints) of the `car` and `car_600k` seed-0
frames under car_auto_T3, level 0 (points to keypoints) of the `ped_dense`
frame under ped_cyl_auto_T3; k = 16, 64, 256.  Per graph and k:
  knn_ms     knn_graph_device: count, one host read of E, fill
  capped_ms  radius_graph_device(num_neighbors=k): count, read, fill, cap
             count, read, cap fill -- the baseline
  E_radius / E_knn / E_capped   rows uncapped and rows kept
  consumer_us  the kernel that consumes the list, launched alone on each of
             the two lists: the fused edge kernel (level 1,
             bench.roofline_edge_kernel) or the pooling kernel (level 0)
A call is timed between device events; every figure is (median of five
rounds, smallest round, largest round), each round the median of --calls
calls, after a warm-up, in one process.  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS = 5
KS = (16, 64, 256)
GRAPHS = (("car", "car_auto_T3", 1), ("car_600k", "car_auto_T3", 1),
          ("ped_dense", "ped_cyl_auto_T3", 0))


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
    assert torch.cuda.is_available(), "knn_time.py needs the GPU"
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
        return [float(np.median(rounds)), min(rounds), max(rounds)]

    def pool_kernel_us(eng, x, f, kps, e0):
        """the pooling kernel alone on the level-0 list `e0` (the launch of
        bench.roofline_pool_kernel)"""
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

    rows = []
    engines = {}
    for preset, name, level in GRAPHS:
        cfg = configs.get_config(name)
        if name not in engines:
            engines[name] = InferenceEngine(
                cfg, weights.init_params(cfg, seed=0, bias_scale=0.05),
                device=dev)
        eng = engines[name]
        xyz, inten = synthetic_cloud(seed=0, preset=preset)
        x, f = torch.from_numpy(xyz).to(dev), torch.from_numpy(inten).to(dev)
        eng.run_frame(x, f)
        coords, kps, edges = eng.last_graph
        kw = cfg['runtime_graph_gen_kwargs']['level_configs'][level][
            'graph_gen_kwargs']
        p, c = coords[level].contiguous(), coords[level + 1].contiguous()
        radius, scale = kw['radius'], kw.get('scale')
        n_k = int(coords[1].shape[0])
        e_radius = int(edges[level].shape[0])

        def consumer_us(e):
            e = e.contiguous()
            if level == 0:
                return pool_kernel_us(eng, x, f, kps, e)
            r = bench.roofline_edge_kernel(torch, eng, e, n_k, reps=args.reps,
                                           frame=(x, f))
            return r["avg_launch_us"] if r else None

        base_us = consumer_us(edges[level])
        for k in KS:
            e_knn, _ = graph_gen.knn_graph_device(p, c, radius, k, scale)
            e_cap, _ = graph_gen.radius_graph_device(p, c, radius, scale,
                                                     num_neighbors=k, seed=1)
            rows.append({
                "graph": "%s level %d" % (preset, level), "k": k,
                "points": int(p.shape[0]), "centres": int(c.shape[0]),
                "E_radius": e_radius, "E_knn": int(e_knn.shape[0]),
                "E_capped": int(e_cap.shape[0]),
                "knn_ms": timed(lambda: graph_gen.knn_graph_device(
                    p, c, radius, k, scale)),
                "capped_ms": timed(lambda: graph_gen.radius_graph_device(
                    p, c, radius, scale, num_neighbors=k, seed=1)),
                "consumer": "pooling" if level == 0 else "edge",
                "consumer_radius_us": base_us,
                "consumer_knn_us": consumer_us(e_knn),
                "consumer_capped_us": consumer_us(e_cap)})
    out = {"calls": args.calls, "rounds": ROUNDS, "reps": args.reps,
           "rows": rows}
    print(json.dumps(out))
    if args.markdown:
        span = lambda t: "%.3f (%.3f - %.3f)" % tuple(t)
        lines = [
            "| graph | k | points | centres | E radius | E kNN | E capped | "
            "kNN ms | capped (baseline) ms | kNN / baseline | consumer | "
            "radius list us | kNN list us | capped list us |",
            "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
        us = lambda v: "n/a" if v is None else "%.0f" % v
        for r in rows:
            lines.append("| %s | %d | %d | %d | %d | %d | %d | %s | %s | %.2f "
                         "| %s | %s | %s | %s |" % (
                             r["graph"], r["k"], r["points"], r["centres"],
                             r["E_radius"], r["E_knn"], r["E_capped"],
                             span(r["knn_ms"]), span(r["capped_ms"]),
                             r["knn_ms"][0] / r["capped_ms"][0],
                             r["consumer"], us(r["consumer_radius_us"]),
                             us(r["consumer_knn_us"]),
                             us(r["consumer_capped_us"])))
        os.makedirs(os.path.dirname(os.path.abspath(args.markdown)),
                    exist_ok=True)
        with open(args.markdown, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
