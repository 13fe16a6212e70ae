"""Farthest-point sampling on the device (pgnn_farthest_first,
sampling.farthest_first_device, KittiDataset.farthest_first and the
'farthest' keypoints of graph_gen) against the NumPy restatement of
tests/_fps_cases.py.  Every sampling comparison is `==`, the copied rows are
compared as bits.  Needs a real MI355X."""
import numpy as np
import pytest

import pointgnn_amd  # noqa: F401
from pointgnn_amd import configs, weights
from oracle import gnn_oracle as gn

import _fps_cases as FC
from test_gpu_parity import FP_TOL      # the package-vs-oracle logit tolerance
from test_gpu_knn_graph import _cloud, _knn_config   # car_auto_T1, ~2 k points

pytestmark = pytest.mark.gpu

CASES = FC.all_cases()
BY_NAME = {c.name: c for c in CASES}
DTYPES = list(FC.DTYPES)
NUM_KEYPOINTS = 300


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


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _assert_picks(pts, got, want_idx, want_nd):
    idx, xyz, nd = got
    assert idx.dtype == np.int32 and xyz.dtype == pts.dtype
    assert np.array_equal(idx, want_idx)
    assert int(nd) == want_nd
    assert np.array_equal(bits(xyz), bits(FC.rows_of(pts, want_idx)))


# ---- every case, both dtypes, tensors and NumPy ---------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_device_equals_restatement(dev, case, dtype):
    import torch
    from pointgnn_amd import sampling
    pts = case.cast(dtype)
    want_idx, want_nd, _ = FC.reference_of(case.name, dtype)
    out = sampling.farthest_first_device(T(pts, dev), case.k, start=case.start)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in out)
    _assert_picks(pts, [t.cpu().numpy() for t in out], want_idx, want_nd)
    out = sampling.farthest_first_device(pts, case.k, start=case.start)
    assert all(isinstance(a, np.ndarray) for a in out)
    _assert_picks(pts, out, want_idx, want_nd)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_segmented_equals_per_segment_calls(dev, dtype):
    from pointgnn_amd import sampling
    pts64, off, st = FC.segmented()
    pts = np.ascontiguousarray(pts64.astype(dtype))
    k, n_seg = FC.SEG_K, len(st)
    idx, xyz, nd = [t.cpu().numpy() for t in sampling.farthest_first_device(
        T(pts, dev), k, start=T(st, dev), offsets=T(off, dev))]
    assert idx.shape == (n_seg, k) and xyz.shape == (n_seg, k, 3) and \
        nd.shape == (n_seg,)
    for s in range(n_seg):
        seg = pts[off[s]:off[s + 1]]
        want_idx, want_nd = FC.fps_reference(seg, k, int(st[s]))
        _assert_picks(seg, (idx[s], xyz[s], nd[s]), want_idx, want_nd)
        if len(seg):
            one = sampling.farthest_first_device(seg, k, start=int(st[s]))
            _assert_picks(seg, one, idx[s], int(nd[s]))
    # the empty segment: -1, zero rows (as bits), 0
    assert (idx[0] == -1).all() and not bits(xyz[0]).any() and nd[0] == 0
    # NumPy in, NumPy out, the same numbers
    again = sampling.farthest_first_device(pts, k, start=st, offsets=off)
    for a, b in zip(again, (idx, xyz, nd)):
        assert isinstance(a, np.ndarray) and a.dtype == b.dtype and \
            a.tobytes() == b.tobytes()


def test_start_outside_its_segment_is_refused(dev):
    from pointgnn_amd import sampling
    pts = BY_NAME["n65"].cast(np.float32)
    for s in (-1, 65):
        with pytest.raises(ValueError, match="outside segment"):
            sampling.farthest_first_device(T(pts, dev), 4, start=s)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_c_abi_without_rows_and_the_empty_forms(dev, dtype):
    import torch
    from pointgnn_amd import sampling
    case = BY_NAME["block+1"]
    pts = case.cast(dtype)
    want_idx, want_nd, _ = FC.reference_of(case.name, dtype)
    st = torch.tensor([case.start], dtype=torch.int32, device=dev)
    idx, xyz, nd = sampling.launch(T(pts, dev), None, st, case.k,
                                   want_xyz=False)      # out_xyz == NULL
    assert xyz is None
    assert np.array_equal(idx.cpu().numpy()[0], want_idx)
    assert int(nd.item()) == want_nd
    # k == 0 and n == 0: nothing but num_distinct
    idx, xyz, nd = sampling.farthest_first_device(T(pts, dev), 0, start=3)
    assert tuple(idx.shape) == (0,) and tuple(xyz.shape) == (0, 3)
    assert int(nd.item()) == 0
    idx, xyz, nd = sampling.farthest_first_device(
        np.zeros((0, 3), dtype), 5, start=0)
    assert (idx == -1).all() and not xyz.any() and int(nd) == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_a_permuted_cloud_picks_the_same_points(dev, dtype):
    from pointgnn_amd import sampling
    case = BY_NAME["untied"]      # no ties: tests/test_fps_cases_cpu.py
    pts = case.cast(dtype)
    want_idx, _, _ = FC.reference_of(case.name, dtype)
    perm = np.random.default_rng(9).permutation(case.n)
    where = np.empty(case.n, np.int64)
    where[perm] = np.arange(case.n)           # old index -> new index
    shuffled = np.ascontiguousarray(pts[perm])
    idx, xyz, nd = sampling.farthest_first_device(
        shuffled, case.k, start=int(where[case.start]))
    assert np.array_equal(perm[idx], want_idx)
    assert np.array_equal(bits(xyz), bits(pts[want_idx])) and nd == case.k


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_dataset_method_equals_restatement_under_a_seed(dev, dtype):
    from pointgnn_amd.kitti_dataset import KittiDataset
    ds = object.__new__(KittiDataset)         # the method needs no state
    case = BY_NAME["start_middle"]
    pts = case.cast(dtype)
    np.random.seed(12)
    got = ds.farthest_first(pts, case.k)
    after = np.random.randint(1 << 30)
    np.random.seed(12)
    start = np.random.randint(len(pts))
    assert np.random.randint(1 << 30) == after      # exactly one draw
    want_idx, _ = FC.fps_reference(pts, case.k, start)
    assert got.dtype == np.float64 and got.shape == (case.k, 3)
    assert np.array_equal(got, pts[want_idx].astype(np.float64))
    rows, idx = ds.farthest_first(pts, case.k, start=start,
                                  return_indices=True)
    assert np.array_equal(rows, got) and np.array_equal(idx, want_idx)
    d = ds.calc_distances(got[0], pts)
    assert np.array_equal(d, FC.dist(got[0], pts.astype(np.float64)))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_non_finite_rows_terminate_in_range(dev, dtype):
    from pointgnn_amd import sampling
    case = FC.non_finite()
    pts = case.cast(dtype)
    idx, xyz, nd = sampling.farthest_first_device(pts, case.k,
                                                  start=case.start)
    assert ((idx >= 0) & (idx < case.n)).all() and 1 <= nd <= case.k


# ---- 'farthest' keypoints in the multi-level graph -------------------------------
def _farthest_kwargs(knn):
    cfg = _knn_config() if knn else configs.get_config("car_auto_T1")
    for key in ("graph_gen_kwargs", "runtime_graph_gen_kwargs"):
        cfg[key] = dict(cfg[key], downsample_method="farthest",
                        num_keypoints=NUM_KEYPOINTS)
    return cfg


@pytest.mark.parametrize("knn", [False, True], ids=["radius", "knn"])
def test_multi_level_graph_with_farthest_keypoints(dev, knn):
    import torch
    from pointgnn_amd import graph_gen
    xyz, _ = _cloud()
    rk = _farthest_kwargs(knn)["runtime_graph_gen_kwargs"]
    np.random.seed(21)
    coords, kps, edges = graph_gen.gen_multi_level_local_graph_v3(xyz, **rk)
    coords, kps, edges = list(coords), list(kps), list(edges)
    assert all(isinstance(a, np.ndarray) for a in coords + kps + edges)
    np.random.seed(21)
    start = np.random.randint(len(xyz))
    want_idx, want_nd = FC.fps_reference(xyz, NUM_KEYPOINTS, start)
    assert want_nd == NUM_KEYPOINTS
    assert kps[0].shape == (NUM_KEYPOINTS, 1) and \
        np.array_equal(kps[0][:, 0], want_idx)
    assert np.array_equal(bits(coords[1]), bits(xyz[want_idx]))
    # the same-scale level keeps the vertices
    assert np.array_equal(kps[1][:, 0], np.arange(NUM_KEYPOINTS))
    assert np.array_equal(bits(coords[2]), bits(coords[1]))
    assert len(edges[0]) > 0 and len(edges[1]) > 0
    assert edges[0][:, 0].max() < len(xyz) and \
        edges[0][:, 1].max() < NUM_KEYPOINTS
    np.random.seed(21)
    t_out = graph_gen.gen_multi_level_local_graph_v3(T(xyz, dev), **rk)
    t_all = [t for lst in t_out for t in lst]
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in t_all)
    for a, b in zip(coords + kps + edges, t_all):
        assert np.array_equal(a, b.cpu().numpy())
    hints = graph_gen.CountHints(k=NUM_KEYPOINTS, edges=[100000, 100000])
    with pytest.raises(NotImplementedError, match="no capacity form"):
        graph_gen.gen_multi_level_local_graph_v3(T(xyz, dev),
                                                 deferred_counts=hints, **rk)


def test_more_keypoints_than_points_keeps_the_distinct_ones(dev):
    from pointgnn_amd import graph_gen
    pts = BY_NAME["duplicated"].cast(np.float32)
    rk = dict(_farthest_kwargs(False)["runtime_graph_gen_kwargs"],
              num_keypoints=[10000])
    np.random.seed(4)
    coords, kps, _ = graph_gen.gen_multi_level_local_graph_v3(pts, **rk)
    np.random.seed(4)
    start = np.random.randint(len(pts))
    want_idx, want_nd = FC.fps_reference(pts, len(pts), start)
    assert want_nd == 100 and len(coords[1]) == 100
    assert np.array_equal(kps[0][:, 0], want_idx[:100])


def test_logits_on_farthest_keypoints_match_the_oracle(dev):
    """car_auto_T1 on 'farthest' keypoints: the package's logits and boxes
    against oracle/gnn_oracle.py on the SAME lists, within the tolerance of
    tests/test_gpu_parity.py."""
    from pointgnn_amd import graph_gen, models
    cfg = _farthest_kwargs(True)
    xyz, inten = _cloud()
    params = weights.init_params(cfg, seed=2, bias_scale=0.05)
    fn = graph_gen.get_graph_generate_fn(cfg["graph_gen_method"])
    np.random.seed(22)
    coords, kps, edges = fn(T(xyz, dev), **cfg["runtime_graph_gen_kwargs"])
    model = models.get_model(cfg["model_name"])(
        num_classes=cfg["num_classes"], box_encoding_len=7, mode="test",
        **cfg["model_kwargs"]).load_state_dict(params)
    logits, boxes = model.predict(T(inten, dev), coords, kps, edges, False)
    c_np = [c.cpu().numpy() for c in coords]
    k_np = [k.cpu().numpy() for k in kps]
    e_np = [e.cpu().numpy() for e in edges]
    assert len(c_np[1]) == NUM_KEYPOINTS
    lg, bx = gn.predict(params, cfg, inten, c_np, k_np, e_np, dtype=np.float64)
    print("farthest keypoints: N", len(xyz), "K", len(c_np[1]), "E",
          [len(e) for e in e_np],
          "max|dlogit| %.3g" % np.abs(logits.cpu().numpy() - lg).max())
    assert np.abs(lg).max() > 1e-3
    np.testing.assert_allclose(logits.cpu().numpy(), lg, atol=FP_TOL, rtol=1e-4)
    np.testing.assert_allclose(boxes.cpu().numpy(), bx, atol=FP_TOL, rtol=1e-4)


def test_one_trainer_step_on_farthest_keypoints(dev):
    from pointgnn_amd import graph_gen, train
    cfg = _farthest_kwargs(True)
    xyz, inten = _cloud()
    np.random.seed(23)
    coords, kps, edges = graph_gen.gen_multi_level_local_graph_v3(
        xyz, **cfg["runtime_graph_gen_kwargs"])
    k = len(coords[-1])
    assert k == NUM_KEYPOINTS
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
    assert {n.split("/")[0] for n in changed} >= {"layer1", "layer2", "output"}
