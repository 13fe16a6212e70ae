"""Computes, from a checkout of the reference (the Point-GNN repository), what
the CPU tests used to read from that checkout at test time, so that the suite
needs nothing outside this repository:

    python tests/golden/make_golden_reference.py PATH_TO_REFERENCE_CHECKOUT

writes
  * ref_digests.json
      "configs": per configs/ file, SHA-256 of its parsed form
        (config_digest below) -- test_host_cpu: the generated configs equal
        them;
      "checkpoints": SHA-256 of every file of the TF-written
        checkpoints/car_auto_T{0,1}_train/ -- test_host_cpu: the bundle
        writer reproduces them bit for bit from weights_car_auto_T{0,1}.npz;
      "car_auto_T3_train_variables": name -> shape that tf_bundle reads from
        the index-only checkpoint;
  * live_reference.npz: graph_gen.gen_disjointed_rnn_local_graph_v3 and
    gen_multi_level_local_graph_v3 of the reference on the seeded `tiny`
    cloud -- test_oracle_cpu: the oracle equals them;
  * tfgraph_live.npz: the shipped car_auto_T{0,1} MetaGraphDefs evaluated by
    oracle/tf_graph_ref.py on graph_tiny.npz with the fixture weights
    (variable shapes, logits, box encodings, the UnsortedSegmentMax layers'
    count and shape) -- test_tfgraph_cpu.
"""
import glob
import hashlib
import json
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import pointgnn_amd  # noqa: E402,F401
import _refimport  # noqa: E402
from pointgnn_amd import configs, tf_bundle  # noqa: E402
from pointgnn_amd.synthetic import synthetic_cloud  # noqa: E402
from oracle import graph_oracle as go  # noqa: E402

DIGESTED = ("car_auto_T0_train", "car_auto_T1_train")


def config_digest(cfg):
    """SHA-256 of a parsed config in canonical JSON (sorted keys)."""
    return hashlib.sha256(json.dumps(cfg, sort_keys=True).encode()).hexdigest()


def file_digest(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def graph_live(ref, name):
    """What test_tfgraph_cpu.test_reference_graph_live reads from the graph."""
    from oracle import tf_graph_ref as tg
    import test_tfgraph_cpu as T
    meta, = glob.glob(os.path.join(ref, "checkpoints", T.CHECKPOINTS[name],
                                   "model-*.meta"))
    g = tg.ReferenceGraph(meta)
    cfg = configs.get_config(name)
    w, _ = T.fixture_weights(name, cfg)
    out = {}
    for v, s in g.variable_shapes().items():
        out["%s/shape/%s" % (name, v)] = np.asarray(s, np.int64)
    g.set_weights(w)
    kw = T.graph_inputs("graph_tiny.npz")
    lg, bx, _ = g.predict(**kw)
    out[name + "/logits"], out[name + "/box_encodings"] = lg, bx
    seg = T.segment_max_nodes(g)
    vals = g.g.run(seg, g.feed(0, is_training=False, **kw))
    out[name + "/n_segment_max"] = np.asarray(len(seg))
    out[name + "/segment_max0_shape"] = np.asarray(vals[0].shape, np.int64)
    out[name + "/has_logits_node"] = np.asarray(
        g.towers[0]["logits"] in g.g.nodes)
    return out


def main(ref):
    digests = {"configs": {}, "checkpoints": {}}
    for name in sorted(os.listdir(os.path.join(ref, "configs"))):
        path = os.path.join(ref, "configs", name)
        load = configs.load_train_config if name.endswith("_train_config") \
            and name[:-len("_train_config")] in configs._TRAIN_TABLE \
            else configs.load_config
        digests["configs"][name] = config_digest(load(path))
    for ck in DIGESTED:
        src = os.path.join(ref, "checkpoints", ck)
        digests["checkpoints"][ck] = {
            f: file_digest(os.path.join(src, f))
            for f in sorted(os.listdir(src))
            if f == "checkpoint" or f.endswith((".index",
                                                ".data-00000-of-00001"))}
    names = tf_bundle.list_variables(os.path.join(
        ref, "checkpoints", "car_auto_T3_train", "model-1400000"))
    digests["car_auto_T3_train_variables"] = {
        n: list(s) for n, _, s, _, _ in names}
    with open(os.path.join(HERE, "ref_digests.json"), "w") as f:
        json.dump(digests, f, indent=1, sort_keys=True)
        f.write("\n")

    _refimport.REF_ROOT = ref
    gg = _refimport.reference_graph_gen()
    assert gg is not None, "no models/graph_gen.py under %s" % ref
    xyz, _ = synthetic_cloud(seed=3, preset="tiny")
    kp, _ = go.keypoints_center(xyz, xyz, 0.4)
    out = {"xyz": xyz, "kp": kp, "radius_edges": go.canonical_edges(
        gg.gen_disjointed_rnn_local_graph_v3(xyz, kp, 1.0, -1))}
    np.random.seed(5)
    random.seed(5)
    _, rk, re = gg.gen_multi_level_local_graph_v3(
        xyz, **configs.car_auto_config(3)["graph_gen_kwargs"])
    for i, a in enumerate(rk):
        out["multi_kp%d" % i] = np.asarray(a)
    for i, a in enumerate(re):
        out["multi_edges%d" % i] = np.asarray(a)
    np.savez_compressed(os.path.join(HERE, "live_reference.npz"), **out)

    live = {}
    for name in ("car_auto_T0", "car_auto_T1"):
        live.update(graph_live(ref, name))
    np.savez_compressed(os.path.join(HERE, "tfgraph_live.npz"), **live)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
