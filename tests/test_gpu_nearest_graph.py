"""k nearest neighbours without a radius on the device (pgnn_knn_nearest,
graph_gen.knn_nearest_device, the 'disjointed_nearest_local_graph_v3' registry
key and its capacity form) against the NumPy restatement
tests/_knn_cases.knn_reference(..., r=inf) on the clouds of
tests/_nearest_cases.py.  Every graph comparison is `==`; no case is excluded.
Needs a real MI355X."""
import functools
import os

import numpy as np
import pytest

import pointgnn_amd  # noqa: F401
from pointgnn_amd import configs, weights
from pointgnn_amd.synthetic import CLOUD_PRESETS, synthetic_cloud
from oracle import gnn_oracle as gn

import _knn_cases as KC
import _nearest_cases as NC
from test_gpu_parity import FP_TOL      # the package-vs-oracle logit tolerance

pytestmark = pytest.mark.gpu

CASES = NC.all_cases()
BY_NAME = {c.name: c for c in CASES}
RUNS = [(c, k) for c in CASES for k in c.ks]
DTYPES = [np.float32, np.float64]
NEAREST_KEY = "disjointed_nearest_local_graph_v3"


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


# ---- device == restatement ------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("case,k", RUNS,
                         ids=["%s-k%d" % (c.name, k) for c, k in RUNS])
def test_nearest_graph_equals_restatement(dev, case, k, dtype):
    import torch
    from pointgnn_amd import graph_gen
    tp, tc = _device_inputs(case, dtype, dev)
    edges = graph_gen.knn_nearest_device(tp, tc, k, case.scale, case.cell)
    ref = NC.reference(case, dtype, k)
    assert edges.dtype == torch.int32
    assert getattr(edges, "_pgnn_sorted", 0) == 1
    got = edges.cpu().numpy()
    assert got.shape == ref.shape == (len(tc) * min(k, len(tp)), 2)
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("name", ["k_seams", "shell_tie", "far_centre"])
def test_rows_do_not_depend_on_cell_size(dev, name):
    """0.25, 1.0, 7.3 and 1000 (the whole cloud in one cell), and the default
    (one host read of the bounding box): identical rows"""
    from pointgnn_amd import graph_gen
    case = BY_NAME[name]
    tp, tc = _device_inputs(case, np.float32, dev)
    for k in (case.ks[0], case.ks[-1]):
        ref = NC.reference(case, np.float32, k)
        for cell in NC.CELL_SIZES + (None,):
            got = graph_gen.knn_nearest_device(tp, tc, k, case.scale, cell)
            assert np.array_equal(got.cpu().numpy(), ref), (k, cell)


KNN_CLOUDS = [c for c in KC.all_cases() if len(c.centers) and len(c.points)]


@pytest.mark.parametrize("case", KNN_CLOUDS, ids=repr)
def test_knn_within_a_covering_radius_is_the_same_graph(dev, case):
    """The two kernels against each other on the clouds of _knn_cases: with a
    radius of at least the cloud's diameter plus the farthest centre's offset,
    knn_graph_device keeps the k nearest of ALL points."""
    from pointgnn_amd import graph_gen
    dtype = np.asarray(case.points).dtype
    tp, tc = _device_inputs(case, dtype, dev)
    import _graph_cases as GC
    p, c = GC._scaled(case.points, case.scale), GC._scaled(
        case.points if case.same else case.centers, case.scale)
    lo, hi = np.minimum(p.min(0), c.min(0)), np.maximum(p.max(0), c.max(0))
    radius = 2.0 * float(np.linalg.norm(hi - lo)) + 1.0
    for k in (case.ks[0], case.ks[-1]):
        within, off = graph_gen.knn_graph_device(tp, tc, radius, k, case.scale)
        plain = graph_gen.knn_nearest_device(tp, tc, k, case.scale,
                                             float(case.r))
        m = min(k, len(tp))
        assert np.array_equal(off.cpu().numpy(), np.arange(len(tc) + 1) * m)
        assert np.array_equal(within.cpu().numpy(), plain.cpu().numpy())


# ---- the C ABI: capacity form, short buffer, empty inputs -----------------------
GUARD = -7


def _call(dev, wide, tp, n_p_dev, tc, n_c_dev, k, cell, edge_cap, rows,
          scale=None):
    """one pgnn_knn_nearest call into a GUARD-filled [rows, 2] buffer
    -> (buffer, record) as NumPy"""
    import ctypes
    import torch
    from pointgnn_amd import _lib
    lib = _lib.load()
    fn = lib.pgnn_knn_nearest_f64 if wide else lib.pgnn_knn_nearest
    n_p, n_c = int(tp.shape[0]), int(tc.shape[0])
    ws_bytes = lib.pgnn_knn_nearest_workspace_bytes(n_p, n_c, k)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    buf = torch.full((rows, 2), GUARD, dtype=torch.int32, device=dev)
    rec = torch.full((2,), GUARD, dtype=torch.int32, device=dev)
    s = None if scale is None else np.ascontiguousarray(scale, np.float64)
    sp = ctypes.c_void_p(0 if s is None else s.ctypes.data)
    _lib.check(fn(_lib.ptr(tp), n_p, _lib.ptr(n_p_dev), _lib.ptr(tc), n_c,
                  _lib.ptr(n_c_dev), sp, k, float(cell), _lib.ptr(ws),
                  ws_bytes, _lib.ptr(buf), edge_cap, _lib.ptr(rec),
                  _lib.stream_ptr()), "pgnn_knn_nearest")
    return buf.cpu().numpy(), rec.cpu().numpy()


@pytest.mark.parametrize("wide", [False, True], ids=["f32", "f64"])
def test_capacity_form_reads_no_row_behind_the_counts(dev, wide):
    """points_cap / centers_cap larger than the device counts; the tail rows
    of the POINTS hold copies of the centres' own coordinates, so they would be
    the nearest neighbours (d2 = 0) if a kernel read them; the tail of the
    centres would add rows.  Rows == the host-sized result, record {Q m, Q m}."""
    import torch
    case, k = BY_NAME["nn_blob"], 24
    dtype = np.float64 if wide else np.float32
    p, c = case.cast(dtype)
    n_p, n_c = len(p), len(c)
    tail_p = np.concatenate([c, c[:13]])            # the centres themselves
    tail_c = p[:29] + dtype(0.125)
    tp, tc = T(np.concatenate([p, tail_p]), dev), T(np.concatenate([c, tail_c]),
                                                    dev)
    cnt = torch.tensor([n_p, n_c], dtype=torch.int32, device=dev)
    ref = NC.reference(case, dtype, k)
    rows = int(tc.shape[0]) * k + 64
    got, rec = _call(dev, wide, tp, cnt[0:1], tc, cnt[1:2], k, case.cell,
                     rows, rows)
    assert rec.tolist() == [n_c * k, n_c * k] == [len(ref)] * 2
    assert np.array_equal(got[:len(ref)], ref)
    assert (got[len(ref):] == GUARD).all()
    # counts larger than the capacities are clamped to them
    big = torch.tensor([n_p + 10 ** 6, n_c + 10 ** 6], dtype=torch.int32,
                       device=dev)
    got2, rec2 = _call(dev, wide, T(p, dev), big[0:1], T(c, dev), big[1:2], k,
                       case.cell, rows, rows)
    assert rec2.tolist() == [n_c * k] * 2
    assert np.array_equal(got2[:len(ref)], ref)
    # fewer valid points than k: m is evaluated on the device
    few = torch.tensor([5, 7], dtype=torch.int32, device=dev)
    got3, rec3 = _call(dev, wide, T(p, dev), few[0:1], T(c, dev), few[1:2], k,
                       case.cell, rows, rows)
    ref3, _ = KC.knn_reference(p[:5], c[:7], np.inf, k)
    assert rec3.tolist() == [35, 35] and len(ref3) == 35
    assert np.array_equal(got3[:35], ref3) and (got3[35:] == GUARD).all()


@pytest.mark.parametrize("wide", [False, True], ids=["f32", "f64"])
def test_short_buffer_stops_at_the_capacity(dev, wide):
    """edge_capacity = Q m - 3: the record is {Q m - 3, Q m} and the three rows
    past the end are untouched (the buffer is one row longer than that)"""
    case, k = BY_NAME["k_seams"], 65
    dtype = np.float64 if wide else np.float32
    tp, tc = _device_inputs(case, dtype, dev)
    ref = NC.reference(case, dtype, k)
    n_e = len(ref)
    assert n_e == len(case.centers) * k
    got, rec = _call(dev, wide, tp, None, tc, None, k, case.cell, n_e - 3,
                     n_e + 1)
    assert rec.tolist() == [n_e - 3, n_e]
    assert np.array_equal(got[:n_e - 3], ref[:n_e - 3])
    assert (got[n_e - 3:] == GUARD).all()


def test_zero_valid_points_or_centres_write_nothing(dev):
    import torch
    case, k = BY_NAME["shell0"], 8
    tp, tc = _device_inputs(case, np.float32, dev)
    zero = torch.zeros(1, dtype=torch.int32, device=dev)
    for n_p_dev, n_c_dev in ((zero, None), (None, zero), (zero, zero)):
        got, rec = _call(dev, False, tp, n_p_dev, tc, n_c_dev, k, 1.0, 64, 64)
        assert rec.tolist() == [0, 0] and (got == GUARD).all()
    empty = torch.zeros((0, 3), dtype=torch.float32, device=dev)
    for a, b in ((empty, tc), (tp, empty), (empty, empty)):
        got, rec = _call(dev, False, a, None, b, None, k, 1.0, 64, 64)
        assert rec.tolist() == [0, 0] and (got == GUARD).all()
    from pointgnn_amd import graph_gen
    assert tuple(graph_gen.knn_nearest_device(empty, tc, k).shape) == (0, 2)
    assert tuple(graph_gen.knn_nearest_device(tp, empty, k, None,
                                              1.0).shape) == (0, 2)


def test_generator_takes_numpy_and_tensors(dev):
    import torch
    from pointgnn_amd import _lib, graph_gen
    case = BY_NAME["nn_scaled"]
    k, = case.ks
    ref = NC.reference(case, np.float32, k)
    fn = graph_gen.get_graph_generate_fn(NEAREST_KEY)
    got = fn(case.points, case.centers, k, scale=case.scale)
    assert isinstance(got, np.ndarray) and np.array_equal(got, ref)
    got = fn(T(case.points, dev), T(case.centers, dev), num_neighbors=k,
             scale=case.scale, cell_size=case.cell)
    assert isinstance(got, torch.Tensor) and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), ref)
    with pytest.raises(ValueError):
        fn(T(case.points, dev), T(case.centers, dev), 0)
    with pytest.raises(ValueError):
        fn(T(case.points, dev), T(case.centers, dev), k, cell_size=0.0)
    with pytest.raises(_lib.PointGnnHipError):
        fn(T(case.points, dev), T(case.centers, dev), KC.K_MAX + 1)


# ---- through the layers above ---------------------------------------------------
LEVEL_K = 16
LEVEL_KW = {"num_neighbors": LEVEL_K, "cell_size": 1.0}


def _level_configs(cfg_levels, which):
    levels = [dict(l) for l in cfg_levels]
    for l in which:
        levels[l]["graph_gen_method"] = NEAREST_KEY
        levels[l]["graph_gen_kwargs"] = dict(LEVEL_KW)
    return levels


def _nearest_config(which):
    cfg = configs.get_config("car_auto_T1")
    for key in ("graph_gen_kwargs", "runtime_graph_gen_kwargs"):
        cfg[key] = dict(cfg[key], level_configs=_level_configs(
            cfg[key]["level_configs"], which))
    return cfg


@functools.lru_cache(maxsize=None)
def _cloud():
    """about 2 k points of the `tiny` scene"""
    preset = dict(CLOUD_PRESETS["tiny"], n_points=2000)
    return synthetic_cloud(seed=4, **preset)


@pytest.mark.parametrize("which", [(1,), (0, 1)], ids=["level1", "both"])
def test_multi_level_graph_with_nearest_levels(dev, which):
    import torch
    from pointgnn_amd import _lib, graph_gen
    xyz, _ = _cloud()
    rk = _nearest_config(which)["runtime_graph_gen_kwargs"]
    coords, kps, edges = graph_gen.gen_multi_level_local_graph_v3(xyz, **rk)
    coords, kps, edges = list(coords), list(kps), list(edges)
    assert all(isinstance(a, np.ndarray) for a in coords + kps + edges)
    for l in which:
        ref, _ = KC.knn_reference(coords[l], coords[l + 1], np.inf, LEVEL_K)
        assert len(ref) == LEVEL_K * len(coords[l + 1]) > 0
        assert np.array_equal(edges[l], ref)
    if 0 not in which:      # level 0 is still the radius graph
        assert np.bincount(edges[0][:, 1]).min() < LEVEL_K < \
            np.bincount(edges[0][:, 1]).max()
    t_coords, t_kps, t_edges = graph_gen.gen_multi_level_local_graph_v3(
        T(xyz, dev), **rk)
    tensors = list(t_coords) + list(t_kps) + list(t_edges)
    assert all(isinstance(a, torch.Tensor) and a.is_cuda for a in tensors)
    for a, b in zip(coords + kps + edges, tensors):
        assert np.array_equal(a, b.cpu().numpy())
    # the capacity form: the same arrays after cutting at the record, from
    # cold hints too (a nearest level's buffer cannot overflow)
    for hints in (graph_gen.CountHints(),
                  graph_gen.CountHints(k=len(coords[1]),
                                       edges=[len(e) for e in edges]).update(
                      len(coords[1]), [len(e) for e in edges])):
        for overlap in (False, True):
            d_coords, d_kps, d_edges = graph_gen.gen_multi_level_local_graph_v3(
                T(xyz, dev), deferred_counts=hints, overlap_build=overlap, **rk)
            frame = _lib.count_of(d_edges[0]).frame
            assert all(_lib.count_of(e).frame is frame for e in d_edges)
            cold = hints.cap(0) < len(edges[0])
            assert frame.overflowed == ([0] if cold and 0 not in which else [])
            assert frame.k == len(coords[1])
            assert frame.edges == [len(e) for e in edges]
            for l in which:
                assert int(d_edges[l].shape[0]) >= len(edges[l])
                assert getattr(d_edges[l], "_pgnn_sorted", 0) == 1
                n = int(_lib.count_of(d_edges[l]).dev.item())
                assert np.array_equal(d_edges[l][:n].cpu().numpy(), edges[l])
            if not frame.overflowed:
                for l in range(len(edges)):
                    n = int(_lib.count_of(d_edges[l]).dev.item())
                    assert np.array_equal(d_edges[l][:n].cpu().numpy(),
                                          edges[l])
    one = graph_gen.gen_multi_level_local_graph_v3_one_read(
        T(xyz, dev), graph_gen.CountHints(), **rk)
    for a, b in zip(coords + kps + edges,
                    list(one[0]) + list(one[1]) + list(one[2])):
        assert np.array_equal(a, b.cpu().numpy())


def test_logits_on_a_nearest_graph_match_the_oracle(dev):
    """car_auto_T1 with both levels on the new key: the package's logits and
    boxes against oracle/gnn_oracle.py on the SAME edge lists, within the
    tolerance of tests/test_gpu_parity.py::test_predict_end_to_end_device_graph
    -- host-sized and through the capacity form (run_frame_deferred)."""
    import torch
    from pointgnn_amd import engine, graph_gen, models
    cfg = _nearest_config((0, 1))
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
    for l in (0, 1):
        ref, _ = KC.knn_reference(c_np[l], c_np[l + 1], np.inf, LEVEL_K)
        assert np.array_equal(e_np[l], ref)
    lg, bx = gn.predict(params, cfg, inten, c_np, k_np, e_np, dtype=np.float64)
    print("nearest levels: N", len(xyz), "K", len(c_np[1]), "E",
          [len(e) for e in e_np],
          "max|dlogit| %.3g" % np.abs(logits.cpu().numpy() - lg).max())
    assert np.abs(lg).max() > 1e-3
    np.testing.assert_allclose(logits.cpu().numpy(), lg, atol=FP_TOL, rtol=1e-4)
    np.testing.assert_allclose(boxes.cpu().numpy(), bx, atol=FP_TOL, rtol=1e-4)
    eng = engine.InferenceEngine(cfg, params, device=dev)
    lg1, bx1 = eng.run_frame(T(xyz, dev), T(inten, dev))
    d = eng.run_frame_deferred(T(xyz, dev), T(inten, dev))
    assert d.counts._host is None          # nothing was read while enqueuing
    lg2, bx2 = d.result()
    assert eng.deferred_overflows == 0 and not d.counts.overflowed
    assert eng.frame_shapes[-1] == (len(c_np[1]), len(e_np[0]), len(e_np[1]))
    # the same edges through the same kernels as the host-sized frame
    assert torch.equal(lg1, lg2) and torch.equal(bx1, bx2)
    np.testing.assert_allclose(lg2.cpu().numpy(), lg, atol=FP_TOL, rtol=1e-4)
    np.testing.assert_allclose(bx2.cpu().numpy(), bx, atol=FP_TOL, rtol=1e-4)


def test_pipelined_frame_loop_on_nearest_levels(tmp_path, dev):
    """run.run_dataset over a small generated dataset: the pipelined loop
    (capacity-form graphs) writes the sequential loop's files byte for byte,
    and -- a nearest level cannot outgrow its buffer -- no frame falls back,
    although the frames grow."""
    import torch
    from pointgnn_amd import kitti_dataset as KD, run as RUN, synthetic as S
    cfg = _nearest_config((0, 1))
    presets = ["tiny", "small", "tiny", "small"]
    root = str(tmp_path / "kitti")
    for i, preset in enumerate(presets):
        S.write_kitti_frames(root, [i], preset=preset, behind_points=4000)
    ds = KD.KittiDataset(*[os.path.join(root, d)
                           for d in ("image_2", "velodyne", "calib")])
    params = weights.init_params(cfg, seed=3, bias_scale=0.05)
    seq_dir = str(tmp_path / "seq")
    td0 = RUN.run_dataset(ds, cfg, None, seq_dir, params=params,
                          pipelined=False)
    assert td0['frames'] == len(presets)
    out = str(tmp_path / "pipe")
    td = RUN.run_dataset(ds, cfg, None, out, params=params, in_flight=2,
                         prefetch=2)
    torch.cuda.synchronize()
    assert td['frames'] == len(presets) and td['sequential fallbacks'] == 0
    sizes = []
    for i in range(ds.num_files):
        name = os.path.join("data", ds.get_filename(i) + ".txt")
        with open(os.path.join(seq_dir, name), "rb") as f:
            want = f.read()
        with open(os.path.join(out, name), "rb") as f:
            assert f.read() == want, i
        sizes.append(len(want))
    assert sum(s > 1 for s in sizes) >= 2, "no detections at all"


def test_one_trainer_step_one_read_equals_host_sized(tmp_path, dev):
    """train.fetch_data on a KITTI frame with a nearest-graph training config:
    the one-read path (capacity form, graph_hints) gives the host-sized path's
    tensors, and one Trainer step on each gives the same loss bit for bit."""
    import torch
    from test_gpu_e2e import _velodyne_scan
    from test_ingest_cpu import _write_png_header_only
    from oracle import ingest_oracle as IO
    from oracle import labels_oracle as LO
    from pointgnn_amd import graph_gen, kitti_dataset as KD, train
    cfg = _nearest_config((0, 1))
    for d in ("image_2", "velodyne", "calib", "label_2"):
        (tmp_path / d).mkdir()
    name = "000000"
    velo = _velodyne_scan(30)
    velo.tofile(str(tmp_path / "velodyne" / (name + ".bin")))
    (tmp_path / "calib" / (name + ".txt")).write_text("".join(IO.CALIB_LINES))
    _write_png_header_only(str(tmp_path / "image_2" / (name + ".png")), 375,
                           1242)
    cam, _, _ = IO.cam_points_in_image(velo, IO.get_calib(IO.CALIB_LINES),
                                       (375, 1242))
    LO.write_label_file(str(tmp_path / "label_2" / (name + ".txt")),
                        LO.synthetic_labels(30, cam, n_boxes=10))
    ds = KD.KittiDataset(str(tmp_path / "image_2"), str(tmp_path / "velodyne"),
                         str(tmp_path / "calib"), str(tmp_path / "label_2"),
                         is_training=True, num_classes=cfg["num_classes"])
    tcfg = {'batch_size': 1, 'initial_lr': 0.05, 'decay_step': 4,
            'decay_factor': 0.5, 'optimizer': 'sgd', 'unify_copies': True,
            'data_aug_configs': []}
    np.random.seed(3)
    host = train.fetch_data(ds, 0, cfg, tcfg)
    hints = graph_gen.CountHints()
    np.random.seed(3)
    one = train.fetch_data(ds, 0, cfg, tcfg, graph_hints=hints)
    assert hints.k == int(host[1][1].shape[0]) > 0
    assert hints.edges == [LEVEL_K * hints.k] * 2
    for a, b in zip(host, one):
        for x, y in zip(a if isinstance(a, (list, tuple)) else [a],
                        b if isinstance(b, (list, tuple)) else [b]):
            assert x.dtype == y.dtype and torch.equal(x, y)
    params = weights.init_params(cfg, seed=5, bias_scale=0.1)
    losses = []
    for sample in (host, one):
        tr = train.Trainer(cfg, tcfg, params=params, device=dev)
        out = tr.train_step(sample)
        losses.append({n: float(v) for n, v in out.items()
                       if np.ndim(v) == 0 and "loss" in n})
    assert {"cls_loss", "loc_loss"} <= set(losses[0])
    assert all(np.isfinite(v) for v in losses[0].values()), losses[0]
    # the losses that see the graph: bit for bit (same edges, same kernels)
    for name in ("cls_loss", "loc_loss"):
        assert losses[0][name] == losses[1][name], (name, losses)
    assert losses[0]["cls_loss"] > 0 and losses[0]["loc_loss"] > 0
    # reg_loss is a norm of the weights alone and never sees the graph; its
    # kernel adds at most 128 float64 partial sums (one per workgroup, of
    # positive terms) with an atomic in arrival order, so each run is within
    # 127 roundings of 2^-53 of the exact sum and two runs on the SAME weights
    # within twice that of each other: 256 * 2^-53 = 2.8e-14 relative
    assert abs(losses[0]["reg_loss"] - losses[1]["reg_loss"]) <= \
        256 * 2.0 ** -53 * losses[0]["reg_loss"]
    assert set(losses[0]) == set(losses[1])
