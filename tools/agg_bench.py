#!/usr/bin/env python
"""Max, sum and mean aggregation of the two fused stages on one bench frame's
real inputs (level-0 pooling, first GNN iteration's level-1 edge stage): time
of a stage by device events around each call, the variants ALTERNATING after a
common warm-up so that clocks and cache state drift over all of them alike.
A sum / mean call is everything the entry enqueues (the zero fill, and for
the mean the in-degree and finishing passes), a max call likewise (its
lowest() fill).  The general path (gather, row MLP, scatter-add) runs beside
the weights-stationary sum, so the fused kernel's gain is on record.

    python tools/agg_bench.py [--preset car_600k] [--config car_auto_T3]
                              [--rounds 12] [--json profiles/agg_bench.json]
"""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import pointgnn_amd  # noqa: E402,F401
from pointgnn_amd import _lib, configs, gnn, weights  # noqa: E402
from pointgnn_amd.engine import InferenceEngine  # noqa: E402
from pointgnn_amd.synthetic import synthetic_cloud  # noqa: E402


def opt(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


preset, config = opt("--preset", "car_600k"), opt("--config", "car_auto_T3")
rounds = int(opt("--rounds", "12"))
dev = torch.device("cuda", 0)
cfg = configs.get_config(config)
params = weights.init_params(cfg, seed=0, bias_scale=0.05)
eng = InferenceEngine(cfg, params, device=dev)
xyz, inten = synthetic_cloud(seed=0, preset=preset)
x, f = torch.from_numpy(xyz).to(dev), torch.from_numpy(inten).to(dev)
gnn.EDGE_INPUT_TAP = []
eng.run_frame(x, f)
p, q = [t.clone() for t in gnn.EDGE_INPUT_TAP[0]]
gnn.EDGE_INPUT_TAP = None
coords, kps, edges = eng.last_graph
lib = _lib.load()
store = eng.model._store
key = [k for k in store._cache if k[0] == 'edge'][0]
c, p_chain, wx_dev, rest = store._cache[key]
pkey = [k for k in store._cache if k[0] == 'mlp' and
        k[1].endswith('layer1/extract_vertex_features')][0]
point_chain = store._cache[pkey]
wq = int(wx_dev.shape[1])
e0, e1 = edges[0].contiguous(), edges[1].contiguous()
kp = kps[0].reshape(-1).to(torch.int32).contiguous()
n_k = int(coords[1].shape[0])
feat = f.contiguous()
pts = coords[0].to(torch.float32).contiguous()
sched, st = _lib.ptr(_lib.sched_ws()), _lib.stream_ptr()


def stage(name):
    """-> (args up to sched_ws, query head, n_edges, output)"""
    if name == "edge":
        out = torch.empty((n_k, gnn.padded_width(rest.n_out)), device=dev)
        return ("pgnn_edge_mlp_scatter_agg",
                (_lib.ptr(p), _lib.ptr(q), wq, int(rest.k_in), _lib.ptr(e1),
                 int(e1.shape[0]), n_k, rest.array, rest.n, 1, _lib.ptr(out),
                 out.stride(0), sched),
                (rest.array, rest.n, int(rest.k_in)), int(e1.shape[0]), out)
    out = torch.empty((n_k, gnn.padded_width(point_chain.n_out)), device=dev)
    return ("pgnn_point_set_pooling_agg",
            (_lib.ptr(feat), int(feat.shape[1]), _lib.ptr(pts), _lib.ptr(kp),
             _lib.ptr(e0), int(e0.shape[0]), n_k, point_chain.array,
             point_chain.n, 1, _lib.ptr(out), out.stride(0), sched),
            (point_chain.array, point_chain.n, int(feat.shape[1])),
            int(e0.shape[0]), out)


def variant(name, code, debug):
    entry, args, qhead, n_e, out = stage(name)
    _lib.set_tunable("mlp_debug", debug)
    nbytes = ctypes.c_size_t(0)
    _lib.check(getattr(lib, entry + "_workspace_bytes")(
        *qhead, n_e, 0, n_k, code, 0, st, ctypes.byref(nbytes)), entry)
    _lib.set_tunable("mlp_debug", 0)
    work = torch.empty(nbytes.value // 4 + 1, device=dev)

    def call():
        _lib.set_tunable("mlp_debug", debug)
        _lib.check(getattr(lib, entry + "_fwd")(
            *args, code, _lib.ptr(work), nbytes.value, st), entry)
        _lib.set_tunable("mlp_debug", 0)
    return call, out, work


result = {"preset": preset, "config": config, "K": n_k,
          "E0": int(e0.shape[0]), "E1": int(e1.shape[0]), "rounds": rounds}
for name in ("edge", "pool"):
    runs = {"max": variant(name, _lib.AGG_MAX, 0),
            "sum": variant(name, _lib.AGG_SUM, 0),
            "mean": variant(name, _lib.AGG_MEAN, 0),
            "sum_general": variant(name, _lib.AGG_SUM, 2048 | 8192)}
    for call, _, _ in runs.values():     # warm-up
        call()
        call()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(rounds):
        for k, (call, _, _) in runs.items():   # alternating
            a, b = torch.cuda.Event(enable_timing=True), \
                torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) * 1e3)
    med = {k: float(np.median(v)) for k, v in times.items()}
    spread = {k: [float(np.min(v)), float(np.max(v))] for k, v in times.items()}
    diff = float((runs["sum"][1] - runs["sum_general"][1]).abs().max())
    result[name] = {"median_us": med, "min_max_us": spread,
                    "sum_over_max": med["sum"] / med["max"],
                    "mean_over_max": med["mean"] / med["max"],
                    "general_over_ws_sum": med["sum_general"] / med["sum"],
                    "max_abs_ws_minus_general": diff}
    print("%s stage (%s/%s)" % (name, config, preset))
    for k in runs:
        print("  %-12s %9.1f us  (min %.1f, max %.1f)" % (
            k, med[k], spread[k][0], spread[k][1]))
    print("  sum / max %.3f   mean / max %.3f   general / ws sum %.2f   "
          "max |ws - general| %.3g" % (
              result[name]["sum_over_max"], result[name]["mean_over_max"],
              result[name]["general_over_ws_sum"], diff))
path = opt("--json", "")
if path:
    with open(path, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
print(json.dumps(result, sort_keys=True))
