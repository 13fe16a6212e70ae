"""k nearest neighbours within the radius on the device (pgnn_knn_graph_*,
graph_gen.knn_graph_device and the 'disjointed_knn_local_graph_v3' registry
key) against the NumPy restatement of tests/_knn_cases.py.  Every graph
comparison is `==`; no case is excluded.  Needs a real MI355X."""
import functools

import numpy as np
import pytest

import pointgnn_amd  # noqa: F401
from pointgnn_amd import configs, weights
from pointgnn_amd.synthetic import CLOUD_PRESETS, synthetic_cloud
from oracle import gnn_oracle as gn

import _knn_cases as KC
from test_gpu_parity import FP_TOL      # the package-vs-oracle logit tolerance
from test_gpu_graph_structure import _capped    # sets / restores the tunables

pytestmark = pytest.mark.gpu

CASES = KC.all_cases()
BY_NAME = {c.name: c for c in CASES}
RUNS = [(c, k) for c in CASES for k in c.ks]
DTYPES = [np.float32, np.float64]
KNN_KEY = "disjointed_knn_local_graph_v3"


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from pointgnn_amd import _lib
    _lib.load()
    return torch.device("cuda")


def T(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _device_inputs(case, dtype, dev):
    p, c = case.cast(dtype)
    tp = T(p, dev)
    return tp, (tp if case.same else T(c, dev))


def _rows_per_centre(edges, n_centres):
    rows = [set() for _ in range(n_centres)]
    for p, q in np.asarray(edges).tolist():
        rows[q].add(p)
    return rows


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("case,k", RUNS,
                         ids=["%s-k%d" % (c.name, k) for c, k in RUNS])
def test_knn_graph_equals_restatement(dev, case, k, dtype):
    import torch
    from pointgnn_amd import graph_gen
    tp, tc = _device_inputs(case, dtype, dev)
    edges, offsets = graph_gen.knn_graph_device(tp, tc, case.r, k, case.scale)
    ref_e, ref_o = KC.take_k(KC.hoods_of(case, dtype), k)
    assert edges.dtype == torch.int32 and offsets.dtype == torch.int32
    assert getattr(edges, "_pgnn_sorted", 0) == 1
    got_e, got_o = edges.cpu().numpy(), offsets.cpu().numpy()
    assert got_o.shape == ref_o.shape and np.array_equal(got_o, ref_o)
    assert got_e.shape == ref_e.shape and np.array_equal(got_e, ref_e)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_knn_rows_are_a_prefix_sized_subset_of_the_device_radius_graph(dev,
                                                                       case):
    """Against the device's OWN radius graph of the same inputs: the count is
    min(k, fan-in) and every row is one of the radius graph's."""
    from pointgnn_amd import graph_gen
    dtype = np.asarray(case.points).dtype
    tp, tc = _device_inputs(case, dtype, dev)
    r_edges, r_off = graph_gen.radius_graph_device(tp, tc, case.r, case.scale)
    fan = np.diff(r_off.cpu().numpy())
    full = _rows_per_centre(r_edges.cpu().numpy(), len(fan))
    for k in case.ks:
        edges, offsets = graph_gen.knn_graph_device(tp, tc, case.r, k,
                                                    case.scale)
        off = offsets.cpu().numpy()
        assert np.array_equal(np.diff(off), np.minimum(k, fan))
        e = edges.cpu().numpy()
        assert np.array_equal(e[:, 1], np.repeat(np.arange(len(fan)),
                                                 np.diff(off)))
        got = _rows_per_centre(e, len(fan))
        assert all(g <= f and len(g) == min(k, len(f))
                   for g, f in zip(got, full))


@pytest.mark.parametrize("name", ["lattice8_r2_f32", "lattice8_r2_f64",
                                  "duplicates", "tie_two_chunks",
                                  "shared_bucket_box", "blob", "blob_aniso",
                                  "blob_scalar", "one_point"])
def test_k_at_least_the_largest_fanin_gives_the_radius_graph(dev, name):
    from pointgnn_amd import graph_gen
    case = BY_NAME[name]
    dtype = np.asarray(case.points).dtype
    tp, tc = _device_inputs(case, dtype, dev)
    r_edges, r_off = graph_gen.radius_graph_device(tp, tc, case.r, case.scale)
    fan = np.diff(r_off.cpu().numpy())
    assert 0 < fan.max() <= KC.K_MAX
    for k in sorted({int(fan.max()), KC.K_MAX}):
        edges, offsets = graph_gen.knn_graph_device(tp, tc, case.r, k,
                                                    case.scale)
        assert np.array_equal(offsets.cpu().numpy(), r_off.cpu().numpy())
        assert _rows_per_centre(edges.cpu().numpy(), len(fan)) == \
            _rows_per_centre(r_edges.cpu().numpy(), len(fan))


@pytest.mark.parametrize("max_wgs,lds_pad", [(1, 0), (3, 0), (8, 32768)])
@pytest.mark.parametrize("name,k", [("dense", 256), ("sweep", 65),
                                    ("lattice8_r2_f64", 30)])
def test_capped_grids_give_the_same_graph(dev, name, k, max_wgs, lds_pad):
    """graph_max_wgs caps the launches: 16 waves a workgroup, every wave
    strides over many centres and reuses its LDS list; at k = 256 the lists
    take 48 KiB, with graph_lds_pad 80 KiB (more dynamic LDS than a kernel
    gets without asking).  Same rows as the restatement."""
    from pointgnn_amd import graph_gen
    case = BY_NAME[name]
    dtype = np.asarray(case.points).dtype
    tp, tc = _device_inputs(case, dtype, dev)
    ref_e, ref_o = KC.take_k(KC.hoods_of(case, dtype), k)
    with _capped(max_wgs, lds_pad):
        edges, offsets = graph_gen.knn_graph_device(tp, tc, case.r, k,
                                                    case.scale)
        got_e, got_o = edges.cpu().numpy(), offsets.cpu().numpy()
    assert np.array_equal(got_o, ref_o)
    assert np.array_equal(got_e, ref_e)


def test_point_order_does_not_change_the_neighbour_sets(dev):
    from pointgnn_amd import graph_gen
    base = BY_NAME["blob"]
    shuf, perm = KC.blob_shuffled()
    k, = base.ks
    out = []
    for case in (base, shuf):
        tp, tc = _device_inputs(case, np.float32, dev)
        e, off = graph_gen.knn_graph_device(tp, tc, case.r, k)
        out.append((e.cpu().numpy(), off.cpu().numpy()))
    (ea, oa), (eb, ob) = out
    assert np.array_equal(oa, ob)
    # no exact ties in this cloud (test_knn_cases_cpu): even the order agrees
    assert np.array_equal(ea[:, 0], perm[eb[:, 0]])
    assert np.array_equal(ea[:, 1], eb[:, 1])


def test_generator_takes_numpy_and_tensors(dev):
    import torch
    from pointgnn_amd import graph_gen
    case = BY_NAME["blob_aniso"]
    k, = case.ks
    ref_e, _ = KC.take_k(KC.hoods_of(case, np.float32), k)
    fn = graph_gen.get_graph_generate_fn(KNN_KEY)
    got = fn(case.points, case.centers, case.r, k, scale=case.scale)
    assert isinstance(got, np.ndarray) and np.array_equal(got, ref_e)
    got = fn(T(case.points, dev), T(case.centers, dev), radius=case.r,
             num_neighbors=k, scale=case.scale)
    assert isinstance(got, torch.Tensor) and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), ref_e)
    from pointgnn_amd import _lib
    with pytest.raises(ValueError):
        fn(T(case.points, dev), T(case.centers, dev), case.r, 0)
    with pytest.raises(_lib.PointGnnHipError):
        fn(T(case.points, dev), T(case.centers, dev), case.r, KC.K_MAX + 1)


# ---- through the layers above ---------------------------------------------------
KNN_LEVEL_K = 32


def _level_configs(cfg_levels):
    """the config's own levels with level 1 switched to the kNN generator"""
    lv0, lv1 = [dict(l) for l in cfg_levels]
    lv1["graph_gen_method"] = KNN_KEY
    lv1["graph_gen_kwargs"] = {
        "radius": lv1["graph_gen_kwargs"]["radius"],
        "num_neighbors": KNN_LEVEL_K}
    return [lv0, lv1]


@functools.lru_cache(maxsize=None)
def _cloud():
    """about 2 k points of the `tiny` scene"""
    preset = dict(CLOUD_PRESETS["tiny"], n_points=2000)
    return synthetic_cloud(seed=4, **preset)


def _knn_config():
    cfg = configs.get_config("car_auto_T1")
    for key in ("graph_gen_kwargs", "runtime_graph_gen_kwargs"):
        cfg[key] = dict(cfg[key], level_configs=_level_configs(
            cfg[key]["level_configs"]))
    return cfg


def test_multi_level_graph_with_a_knn_level(dev):
    import torch
    from pointgnn_amd import graph_gen
    xyz, _ = _cloud()
    rk = _knn_config()["runtime_graph_gen_kwargs"]
    coords, kps, edges = graph_gen.gen_multi_level_local_graph_v3(xyz, **rk)
    coords, kps, edges = list(coords), list(kps), list(edges)
    assert all(isinstance(a, np.ndarray) for a in coords + kps + edges)
    lv = rk["level_configs"]
    ref1, _ = KC.knn_reference(coords[1], coords[2],
                               lv[1]["graph_gen_kwargs"]["radius"],
                               KNN_LEVEL_K, lv[1]["graph_gen_kwargs"].get(
                                   "scale"))
    assert len(ref1) > 0 and np.array_equal(edges[1], ref1)
    deg = np.bincount(edges[1][:, 1], minlength=len(coords[2]))
    assert deg.max() == KNN_LEVEL_K and deg.min() < KNN_LEVEL_K
    # level 0 is still the radius graph: more rows than k per centre somewhere
    assert np.bincount(edges[0][:, 1]).max() > KNN_LEVEL_K
    t_coords, t_kps, t_edges = graph_gen.gen_multi_level_local_graph_v3(
        T(xyz, dev), **rk)
    t_coords, t_kps, t_edges = list(t_coords), list(t_kps), list(t_edges)
    assert all(isinstance(a, torch.Tensor) and a.is_cuda
               for a in t_coords + t_kps + t_edges)
    for a, b in zip(coords + kps + edges, t_coords + t_kps + t_edges):
        assert np.array_equal(a, b.cpu().numpy())
    # the capacity form keeps refusing a generator it has no form for
    hints = graph_gen.CountHints(k=2000, edges=[100000, 100000])
    with pytest.raises(NotImplementedError, match="no capacity form"):
        graph_gen.gen_multi_level_local_graph_v3(T(xyz, dev),
                                                 deferred_counts=hints, **rk)


def test_logits_on_a_knn_graph_match_the_oracle(dev):
    """car_auto_T1 with a kNN level 1: the package's logits and boxes against
    oracle/gnn_oracle.py on the SAME edge lists, within the tolerance of
    tests/test_gpu_parity.py::test_predict_end_to_end_device_graph."""
    from pointgnn_amd import graph_gen, models
    cfg = _knn_config()
    xyz, inten = _cloud()
    params = weights.init_params(cfg, seed=2, bias_scale=0.05)
    fn = graph_gen.get_graph_generate_fn(cfg["graph_gen_method"])
    coords, kps, edges = fn(T(xyz, dev), **cfg["runtime_graph_gen_kwargs"])
    model = models.get_model(cfg["model_name"])(
        num_classes=cfg["num_classes"], box_encoding_len=7, mode="test",
        **cfg["model_kwargs"]).load_state_dict(params)
    logits, boxes = model.predict(T(inten, dev), coords, kps, edges, False)
    c_np = [c.cpu().numpy() for c in coords]
    k_np = [k.cpu().numpy() for k in kps]
    e_np = [e.cpu().numpy() for e in edges]
    lv1 = cfg["runtime_graph_gen_kwargs"]["level_configs"][1]
    ref1, _ = KC.knn_reference(c_np[1], c_np[2],
                               lv1["graph_gen_kwargs"]["radius"], KNN_LEVEL_K)
    assert np.array_equal(e_np[1], ref1)
    lg, bx = gn.predict(params, cfg, inten, c_np, k_np, e_np, dtype=np.float64)
    print("kNN level: N", len(xyz), "K", len(c_np[1]), "E",
          [len(e) for e in e_np],
          "max|dlogit| %.3g" % np.abs(logits.cpu().numpy() - lg).max())
    assert np.abs(lg).max() > 1e-3
    np.testing.assert_allclose(logits.cpu().numpy(), lg, atol=FP_TOL, rtol=1e-4)
    np.testing.assert_allclose(boxes.cpu().numpy(), bx, atol=FP_TOL, rtol=1e-4)


def test_one_trainer_step_on_a_knn_graph(dev):
    from pointgnn_amd import graph_gen, train
    cfg = _knn_config()
    xyz, inten = _cloud()
    rk = cfg["runtime_graph_gen_kwargs"]
    coords, kps, edges = graph_gen.gen_multi_level_local_graph_v3(xyz, **rk)
    k = len(coords[-1])
    rng = np.random.default_rng(6)
    labels = rng.integers(0, cfg["num_classes"], (k, 1)).astype(np.int32)
    labels[rng.random((k, 1)) < 0.5] = 0
    boxes = (rng.standard_normal((k, 1, 7)) * 1.5).astype(np.float32)
    valid = (labels > 0).astype(np.float32).reshape(k, 1, 1)
    params = weights.init_params(cfg, seed=5, bias_scale=0.1)
    tr = train.Trainer(cfg, params=params, device=dev)
    before = tr.state_dict()
    out = tr.train_step((inten, coords, kps, edges, labels, boxes, valid))
    losses = {n: float(v) for n, v in out.items()
              if np.ndim(v) == 0 and "loss" in n}
    assert {"cls_loss", "loc_loss"} <= set(losses)
    assert all(np.isfinite(v) for v in losses.values()), losses
    assert losses["cls_loss"] > 0 and losses["loc_loss"] > 0
    after = tr.state_dict()
    changed = [n for n in before if not np.array_equal(before[n], after[n])]
    assert all(np.isfinite(v).all() for v in after.values())
    # every layer saw a gradient through the kNN level's edges
    assert {n.split("/")[0] for n in changed} >= {"layer1", "layer2", "output"}


# ---- the C ABI: capacity smaller than E ------------------------------------------
@pytest.mark.parametrize("wide", [False, True], ids=["f32", "f64"])
def test_fill_with_a_short_capacity_stops_at_the_buffer(dev, wide):
    """Rows at or beyond `capacity` are not written, the rows before it are
    the ones a full-size fill writes, and the call succeeds -- as
    pgnn_radius_graph_fill.  The buffer has a guard region behind it."""
    import torch
    from pointgnn_amd import _lib
    lib = _lib.load()
    case, k = BY_NAME["dense"], 64
    dtype = np.float64 if wide else np.float32
    tp, tc = _device_inputs(case, dtype, dev)
    ref_e, ref_o = KC.take_k(KC.hoods_of(case, dtype), k)
    n_p, n_c, n_e = len(case.points), len(case.centers), len(ref_e)
    count = lib.pgnn_knn_graph_count_f64 if wide else lib.pgnn_knn_graph_count
    fill = lib.pgnn_knn_graph_fill_f64 if wide else lib.pgnn_knn_graph_fill
    ws_bytes = lib.pgnn_knn_graph_workspace_bytes(n_p, n_c, k)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    offsets = torch.empty(n_c + 1, dtype=torch.int32, device=dev)
    st, null = _lib.stream_ptr(), _lib.ptr(None)
    _lib.check(count(_lib.ptr(tp), n_p, _lib.ptr(tc), n_c, case.r, null, k,
                     _lib.ptr(ws), ws_bytes, _lib.ptr(offsets), st))
    assert np.array_equal(offsets.cpu().numpy(), ref_o)
    GUARD = -7
    for cap in (n_e, n_e - 1, 3 * k + 17, 1, 0):     # inside a centre's rows
        buf = torch.full((n_e + 4096, 2), GUARD, dtype=torch.int32, device=dev)
        _lib.check(fill(_lib.ptr(tp), n_p, _lib.ptr(tc), n_c, case.r, null, k,
                        _lib.ptr(ws), ws_bytes, _lib.ptr(offsets),
                        _lib.ptr(buf), cap, st))
        got = buf.cpu().numpy()
        assert np.array_equal(got[:cap], ref_e[:cap]), cap
        assert (got[cap:] == GUARD).all(), cap
