"""Host-side logic that needs no GPU: configs, variable specs, checkpoint
reader, synthetic input, C-ABI library load/symbols, weight packing layout."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import pointgnn_amd  # noqa: F401
from pointgnn_amd import configs, tf_bundle, weights
from pointgnn_amd.synthetic import synthetic_cloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
# what the reference checkout holds, computed by
# tests/golden/make_golden_reference.py
REF_DIGESTS = os.path.join(GOLD, "ref_digests.json")


def _ref_digests():
    with open(REF_DIGESTS) as f:
        return json.load(f)


def _sha256(path):
    import hashlib
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def test_param_counts_match_reference_checkpoints():
    # SURVEY.md §8c totals (include the int32 global-step scalar)
    expect = {"car_auto_T0": 344933, "car_auto_T1": 726492,
              "car_auto_T2": 1108051, "car_auto_T3": 1489610,
              "ped_cyl_auto_T3": 1357274, "car_fixed_T3": 1431233}
    for name, total in expect.items():
        assert weights.count_params(configs.get_config(name)) + 1 == total


def test_variable_names_match_golden_weights():
    for t in (0, 1):
        w = np.load(os.path.join(GOLD, "weights_car_auto_T%d.npz" % t))
        spec = dict(weights.variable_specs(configs.car_auto_config(t)))
        assert set(spec) == set(w.files)
        for k, shape in spec.items():
            assert w[k].shape == tuple(shape)


def test_generated_configs_equal_reference_json():
    from golden.make_golden_reference import config_digest
    ref = _ref_digests()["configs"]
    pairs = [("car_auto_T0", "car_auto_T0_train_config"),
             ("car_auto_T1", "car_auto_T1_train_config"),
             ("car_auto_T2", "car_auto_T2_train_config"),
             ("car_auto_T3", "car_auto_T3_train_config"),
             ("car_auto_T3", "car_auto_T3_trainval_config"),
             ("car_fixed_T3", "car_fixed_T3_train_config"),
             ("ped_cyl_auto_T3", "ped_cyl_auto_T3_trainval_config")]
    for name, fname in pairs:
        assert ref[fname] == config_digest(configs.get_config(name)), fname


def test_generated_train_and_eval_configs_equal_reference_json(tmp_path):
    from golden.make_golden_reference import config_digest
    ref = _ref_digests()["configs"]
    for name in configs._TRAIN_TABLE:
        assert ref[name + "_train_config"] == config_digest(
            configs.get_train_config(name)), name
        assert ref[name + "_eval_config"] == config_digest(
            configs.get_eval_config(name)), name
    # save/load round trip in the reference's JSON form
    path = str(tmp_path / "train_config")
    configs.save_train_config(path, configs.get_train_config("car_auto_T3_train"))
    assert configs.load_train_config(path) == \
        configs.get_train_config("car_auto_T3_train")


def _reference_checkpoint(tmp_path, t):
    """checkpoints/car_auto_T<t>_train re-encoded from the golden weights and
    proven byte-identical to the TF-written files by their SHA-256."""
    gold = np.load(os.path.join(GOLD, "weights_car_auto_T%d.npz" % t))
    d = str(tmp_path / ("t%d" % t))
    prefix = tf_bundle.save_checkpoint(d, {k: gold[k] for k in gold.files},
                                       global_step=1400000)
    want = _ref_digests()["checkpoints"]["car_auto_T%d_train" % t]
    assert sorted(want) == sorted(os.listdir(d))
    for f in want:
        assert _sha256(os.path.join(d, f)) == want[f], f
    return d, prefix


def test_tf_bundle_reader_on_reference_checkpoints(tmp_path):
    for t in (0, 1):
        src, prefix = _reference_checkpoint(tmp_path, t)
        ck = tf_bundle.load_checkpoint(src)
        assert int(ck["Variable"]) == 1400000
        gold = np.load(os.path.join(GOLD, "weights_car_auto_T%d.npz" % t))
        for k in gold.files:
            assert np.array_equal(ck[k], gold[k])
        # index-only checkpoints still list names/shapes
        os.remove(prefix + ".data-00000-of-00001")
        spec = dict(weights.variable_specs(configs.car_auto_config(t)))
        got = {n: s for n, _, s, _, _ in tf_bundle.list_variables(prefix)
               if n != "Variable"}
        assert got == {k: tuple(v) for k, v in spec.items()}
    # what the reader listed from the reference's index-only T3 checkpoint
    names = _ref_digests()["car_auto_T3_train_variables"]
    spec = dict(weights.variable_specs(configs.car_auto_config(3)))
    got = {n: tuple(s) for n, s in names.items() if n != "Variable"}
    assert got == {k: tuple(v) for k, v in spec.items()}


def test_crc32c_known_answers():
    # RFC 3720 B.4 check value and TF's masking identity
    assert tf_bundle.crc32c(b"123456789") == 0xE3069283
    assert tf_bundle.crc32c(b"") == 0
    assert tf_bundle.crc32c(b"6789", tf_bundle.crc32c(b"12345")) == 0xE3069283


def test_checkpoint_writer_round_trip(tmp_path):
    gold = np.load(os.path.join(GOLD, "weights_car_auto_T0.npz"))
    params = {k: gold[k] for k in gold.files}
    prefix = tf_bundle.save_checkpoint(str(tmp_path), params, global_step=77)
    assert os.path.basename(prefix) == "model-77"
    back = tf_bundle.load_checkpoint(str(tmp_path))   # via the `checkpoint` file
    assert int(back.pop("Variable")) == 77
    assert set(back) == set(params)
    for k in params:
        assert back[k].dtype == params[k].dtype
        assert np.array_equal(back[k], params[k])
    names = [n for n, _, _, _, _ in tf_bundle.list_variables(prefix)]
    assert names == sorted(names)                      # SSTable key order


def test_checkpoint_writer_is_byte_identical_to_tensorflow(tmp_path):
    """Re-encoding the variables of the reference's TF-written checkpoints
    reproduces both files and the `checkpoint` file bit for bit (table
    layout, prefix compression, masked crc32c of every tensor and block):
    SHA-256 of the reference's files in ref_digests.json."""
    for t in (0, 1):
        _reference_checkpoint(tmp_path, t)


def test_synthetic_cloud_is_deterministic_and_shaped():
    a, ia = synthetic_cloud(seed=4, preset="tiny")
    b, ib = synthetic_cloud(seed=4, preset="tiny")
    assert np.array_equal(a, b) and np.array_equal(ia, ib)
    assert a.dtype == np.float32 and a.shape == (1500, 3)
    assert ia.shape == (1500, 1) and ia.min() >= 0 and ia.max() < 1
    c, _ = synthetic_cloud(seed=5, preset="tiny")
    assert not np.array_equal(a, c)
    assert a[:, 2].min() > 0          # camera frame: z forward
    rng = np.sqrt((a ** 2).sum(1))
    assert rng.min() > 1.9 and rng.max() < 71


def test_init_params_shapes_and_seed():
    cfg = configs.car_auto_config(1)
    p = weights.init_params(cfg, seed=1)
    q = weights.init_params(cfg, seed=1)
    for (name, shape) in weights.variable_specs(cfg):
        assert p[name].shape == tuple(shape) and p[name].dtype == np.float32
        assert np.array_equal(p[name], q[name])
    w = p["layer2/extract_vertex_features/fully_connected/weights"]
    assert w.shape == (303, 300)
    assert np.abs(w).max() <= np.sqrt(6.0 / 603) + 1e-6


# ---- C-ABI library ---------------------------------------------------------
def _lib():
    from pointgnn_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        from pointgnn_amd import build
        build.build(verbose=False)
    return L, L.load()


def test_library_exports_every_declared_symbol():
    L, lib = _lib()
    header = open(os.path.join(ROOT, "include", "pointgnn_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(pgnn_[a-z0-9_]+)\s*\(", header))
    assert declared, "no declarations parsed"
    for name in declared:
        assert hasattr(lib, name), "missing export: " + name
    # the Python binding covers the header (plus the tuning hook)
    assert declared <= set(L.exported_symbols())
    # ... through the header reader, which must find the same names as this
    # cruder parse and whose types are what the loaded functions carry
    from pointgnn_amd import _header
    assert declared == set(_header.functions())
    for name, (res, args) in _header.functions().items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert lib.pgnn_version() >= 100


def test_error_reporting_without_gpu():
    L, lib = _lib()
    # argument validation happens before any HIP call
    rc = lib.pgnn_scatter_max_f32(None, 4, None, 5, 8, 3, None, 4, 0, None)
    assert rc == -1
    assert b"stride" in lib.pgnn_last_error()
    assert lib.pgnn_pack_fc(None, None, 4, 4, None) == -1
    assert lib.pgnn_packed_fc_floats(303, 300) == 19 * 19 * 256 + 19 * 16
    with pytest.raises(L.PointGnnHipError):
        L.check(-1, "demo")
    # the widened entries validate before touching HIP as well
    assert lib.pgnn_nms_boxes_3d(None, None, None, None, -1, 0.5, 1, 10.0, -1,
                                 None, 0, None, None, None, None, None,
                                 None) == -1
    assert lib.pgnn_nms_boxes_3d(None, None, None, None, 5, 0.5, 9, 10.0, -1,
                                 None, 0, None, None, None, None, None,
                                 None) == -1          # mode out of range
    assert b"nms_boxes_3d" in lib.pgnn_last_error()
    assert lib.pgnn_nms_workspace_bytes(-1) == 0
    assert 0 < lib.pgnn_nms_workspace_bytes(100) < \
        lib.pgnn_nms_workspace_bytes(10000)
    assert lib.pgnn_box_decode_f32(None, None, None, None, 0, 5, 0, None,
                                   None) == -1        # boxes_per_row = 0
    assert lib.pgnn_kitti_cam_points_in_image(
        None, 10, None, None, 1242.0, 375.0, None, 0, 0, None, 0, None, None,
        1, 10, None, None) == -1                       # no count pointer
    assert lib.pgnn_kitti_ingest_workspace_bytes(120000) > 0
    # collectives: arguments are checked before RCCL is entered
    import ctypes
    h = ctypes.c_void_p()
    assert lib.pgnn_comm_unique_id(None) == -1
    assert lib.pgnn_comm_init_rank(None, 1, 0, ctypes.byref(h)) == -1
    assert lib.pgnn_comm_init_rank(b"\0" * 128, 2, 2, ctypes.byref(h)) == -1
    assert lib.pgnn_allreduce_sum_f32(None, None, 4, None) == -1
    assert lib.pgnn_allreduce_step(None, None, 0, None, 0, None) == -1
    assert lib.pgnn_comm_destroy(None) == 0
    assert b"rccl" in lib.pgnn_comm_library().lower()
    assert lib.pgnn_assign_box_labels(None, -1, None, 0, None, None, None,
                                      None, None) == -1
    assert lib.pgnn_vertex_pre_edge_fwd(None, 0, 0, None, None, 0, None, None,
                                        5, None, None, 0, None, 0, None) == -1
    assert lib.pgnn_points_in_box_f64(None, 5, None, None, None, None,
                                      None) == -1
    assert lib.pgnn_metrics_state_bytes(4, 200) == 4 * (3 + 2 * 201) * 8
    assert lib.pgnn_metrics_state_bytes(0, 200) == 0
    assert lib.pgnn_metrics_update(None, 4, None, 10, 4, 5000, None,
                                   None) == -1        # too many thresholds
    assert lib.pgnn_metrics_update(None, 2, None, 10, 4, 200, None,
                                   None) == -1        # stride < classes
    assert lib.pgnn_metrics_compute(None, 4, 200, None, None) == -1


def test_capacity_form_host_logic():
    """The host side of the capacity form (graph_gen deferred_counts): size
    hints and capacities, the FrameCounts record, the pgnn_dyn_count struct
    and the *_dyn entries' argument checks -- no GPU involved."""
    import ctypes
    from pointgnn_amd import graph_gen as G
    L, lib = _lib()
    # struct pgnn_dyn_count {const int32_t *dev; int64_t hint;}
    assert ctypes.sizeof(L.DynCount) == 16
    assert L.DynCount.dev.offset == 0 and L.DynCount.hint.offset == 8
    h = G.CountHints()
    assert h.cap(0) == G.CountHints.MIN_EDGE_CAP and h.edge_hint(1) == 0
    h.update(3000, [350000, 600000])
    assert h.k == 3000 and h.edges == [350000, 600000]
    assert h.cap(0) >= 2 * 350000 and h.cap(1) >= 2 * 600000
    caps = list(h.edge_caps)
    h.update(2500, [10, 20])                  # hints follow, capacities stay
    assert h.k == 2500 and h.edges == [10, 20] and h.edge_caps == caps
    h.update(2500, [900000, 20])              # ... and only ever grow
    assert h.cap(0) >= 1800000 and h.cap(1) == caps[1]
    c = G.FrameCounts(None, [100, 50])
    c._host = [7, 0, 100, 130, 40, 40]        # level 0 needed 130 rows, had 100
    assert (c.k, c.kd_status, c.edges, c.overflowed) == (7, 0, [130, 40], [0])
    c._host = [7, 0, 90, 90, 40, 40]
    assert c.overflowed == [] and c.raw_edges is None
    # levels with a fan-in cap (training kwargs): the uncapped list has its
    # own capacity and its own record behind the levels' (written, required)
    assert h.raw_cap(1) == 2 * h.cap(1)       # nothing seen yet
    h.update(2500, [900000, 20], raw_edges=[900000, 5000])
    assert h.raw_cap(0) >= 1800000 and h.raw_cap(1) == G.CountHints.MIN_EDGE_CAP
    c._host = [7, 0, 90, 90, 0, 40, 0, 0, 300, 500]   # level 1: uncapped list cut
    assert c.raw_edges == [0, 500] and c.edges == [90, 40]
    assert c.overflowed == [1]                # flagged as {0, required}
    assert lib.pgnn_radius_graph_dyn_cap(None, 0, 10, 10, None, 0, None, 8, 1,
                                         None, None, 0, None, None) == -1
    assert lib.pgnn_radius_graph_dyn_cap(None, 0, 10, 10, None, 0, None, 0, 1,
                                         None, None, 0, None, None) == -1
    # the f16x2 pooling entry: null layers / image are argument errors
    assert lib.pgnn_point_set_pooling_f16x2_fwd(
        None, 1, None, None, None, 0, 0, None, 4, None, None, 1, None, 304,
        None, None, None, None, None) == -1
    # the capacity-form entries validate before any HIP call
    assert lib.pgnn_radius_graph_dyn_workspace_bytes(-1, 5) == 0
    assert lib.pgnn_radius_graph_dyn_workspace_bytes(20000, 20000) > \
        lib.pgnn_radius_graph_workspace_bytes(20000, 20000)
    assert lib.pgnn_radius_graph_dyn(None, 10, None, None, 10, None, 1.0, None,
                                     None, 0, None, 100, None, None) == -1
    # ... and so do its two stages (grid: points only; query: centres too)
    assert lib.pgnn_radius_graph_dyn_grid(None, 10, None, 10, 1.0, None, None,
                                          0, None) == -1
    assert lib.pgnn_radius_graph_dyn_grid(None, 0, None, 0, -1.0, None, None,
                                          0, None) == -1
    assert lib.pgnn_radius_graph_dyn_query(None, 0, None, 10, None, 1.0, None,
                                           None, 0, None, 100, None,
                                           None) == -1
    assert lib.pgnn_mlp_fwd_dyn(None, 0, 4, None, 0, 0, 16, None, 1, None, 0,
                                None, 0, None, None) == -1   # null count
    assert b"count" in lib.pgnn_last_error()
    assert lib.pgnn_vertex_pre_edge_fwd_dyn(None, 0, 0, None, None, 0, None,
                                            None, 5, None, None, 0, None, 0,
                                            None, None) == -1
    # builder tunables of the frame pipeline exist and are range-checked
    for key, ok, bad in (("graph_max_wgs", 8, -1), ("graph_lds_pad", 32768,
                                                    1 << 20),
                         ("ws_reserve", 8, 3)):
        assert lib.pgnn_set_tunable(key.encode(), ok) == 0
        assert lib.pgnn_set_tunable(key.encode(), bad) != 0
        assert lib.pgnn_set_tunable(key.encode(), 0) == 0


def _emulate_mfma_layer(x, packed, k_in, n_out):
    """NumPy model of mlp_engine.h: A fragment = x[row][16q + 4g + s], B
    fragment = packed[q][t][lane][s]; v_mfma_f32_16x16x4 sums the four k-slots
    g = lane>>4; D[row][col] lives in lane = col + 16*(row//4), reg row%4."""
    kq, nt = (k_in + 15) // 16, (n_out + 15) // 16
    rows = x.shape[0]
    assert rows % 16 == 0
    xp = np.zeros((rows, 16 * kq), np.float32)
    xp[:, :k_in] = x
    w = packed[:kq * nt * 256].reshape(kq, nt, 64, 4)
    bias = packed[kq * nt * 256:]
    out = np.zeros((rows, 16 * nt), np.float32)
    lanes = np.arange(64)
    for m in range(rows // 16):
        for t in range(nt):
            acc = np.zeros((16, 16), np.float32)
            for q in range(kq):
                for s in range(4):
                    a = np.zeros((16, 4), np.float32)   # A[i][kslot]
                    b = np.zeros((4, 16), np.float32)   # B[kslot][j]
                    a[lanes & 15, lanes >> 4] = xp[16 * m + (lanes & 15),
                                                   16 * q + 4 * (lanes >> 4) + s]
                    b[lanes >> 4, lanes & 15] = w[q, t, lanes, s]
                    acc += a @ b
            out[16 * m:16 * m + 16, 16 * t:16 * t + 16] = acc
    return out + bias[None, :]


@pytest.mark.parametrize("k_in,n_out", [(4, 32), (303, 300), (64, 3), (20, 17)])
def test_pack_fc_layout_reproduces_matmul(k_in, n_out):
    L, lib = _lib()
    rng = np.random.default_rng(k_in * 1000 + n_out)
    w = rng.standard_normal((k_in, n_out)).astype(np.float32)
    b = rng.standard_normal(n_out).astype(np.float32)
    n = lib.pgnn_packed_fc_floats(k_in, n_out)
    packed = np.full(n, np.nan, np.float32)
    assert lib.pgnn_pack_fc(w.ctypes.data, b.ctypes.data, k_in, n_out,
                            packed.ctypes.data) == 0
    assert np.isfinite(packed).all()
    x = rng.standard_normal((16, k_in)).astype(np.float32)
    got = _emulate_mfma_layer(x, packed, k_in, n_out)
    ref = x.astype(np.float64) @ w.astype(np.float64) + b
    np.testing.assert_allclose(got[:, :n_out], ref, atol=1e-4, rtol=1e-4)
    assert np.all(got[:, n_out:] == 0)       # zero padding stays zero


def test_product_path_has_no_oracle_import():
    """The shipped package must never reach into oracle/ (or any CPU
    fallback)."""
    pkg = os.path.join(ROOT, "point-gnn_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in src and "from oracle" not in src, f


def test_input_features_switch_matches_run_py():
    """run.py:226-241 / train.py:91-104: the `input_features` config key."""
    import torch
    from pointgnn_amd.kitti_dataset import Points
    from pointgnn_amd.run import _input_features
    attr = torch.arange(20, dtype=torch.float32).reshape(5, 4) + 1
    pts = Points(xyz=torch.zeros(5, 3), attr=attr)
    a = attr.numpy()
    want = {
        'irgb': a,
        '0rgb': np.hstack([np.zeros((5, 1)), a[:, 1:]]),
        '0000': np.zeros_like(a),
        'i000': np.hstack([a[:, [0]], np.zeros((5, 3))]),
        'i': a[:, [0]],
        '0': np.zeros((5, 1)),
    }
    for kind, ref in want.items():
        got = _input_features({'input_features': kind}, pts).numpy()
        assert got.shape == ref.shape and np.array_equal(got, ref), kind
    assert np.array_equal(attr.numpy(), a)        # the cloud is not modified
    with pytest.raises(ValueError):
        _input_features({'input_features': 'rgb'}, pts)


def test_learning_rate_schedule_matches_tf_exponential_decay():
    """train.py:375-378: tf.train.exponential_decay(staircase=True)."""
    from pointgnn_amd.train import learning_rate
    tc = configs.get_train_config("car_auto_T3_train")
    assert learning_rate(tc, 0) == 0.125
    assert learning_rate(tc, 399999) == 0.125
    assert learning_rate(tc, 400000) == pytest.approx(0.0125)
    assert learning_rate(tc, 1399999) == pytest.approx(0.125 * 0.1 ** 3)
    ped = configs.get_train_config("ped_cyl_auto_T3_trainval")
    assert learning_rate(ped, 800000) == pytest.approx(0.32 * 0.25 ** 2)


def test_checkpoint_state_file_lists_and_prunes(tmp_path):
    """tf.train.Saver bookkeeping (train.py:496,516,634-636): the `checkpoint`
    state file lists the checkpoints kept so far, oldest first; beyond
    max_to_keep (TF default 5) the oldest are deleted; the prefix comes from
    train_config['checkpoint_path']."""
    import numpy as np
    from pointgnn_amd import tf_bundle
    d = str(tmp_path)
    var = {"layer1/w": np.arange(6, dtype=np.float32).reshape(2, 3)}
    for step in range(1, 8):
        tf_bundle.save_checkpoint(d, var, global_step=step, name="mymodel",
                                  max_to_keep=3)
    lines = open(os.path.join(d, "checkpoint")).read().splitlines()
    assert lines == ['model_checkpoint_path: "mymodel-7"',
                     'all_model_checkpoint_paths: "mymodel-5"',
                     'all_model_checkpoint_paths: "mymodel-6"',
                     'all_model_checkpoint_paths: "mymodel-7"']
    files = sorted(f for f in os.listdir(d) if f.endswith(".index"))
    assert files == ["mymodel-5.index", "mymodel-6.index", "mymodel-7.index"]
    ck = tf_bundle.load_checkpoint(d)
    assert int(ck["Variable"]) == 7 and np.array_equal(ck["layer1/w"], var["layer1/w"])
    # saving the same step again does not duplicate its entry
    tf_bundle.save_checkpoint(d, var, global_step=7, name="mymodel", max_to_keep=3)
    assert open(os.path.join(d, "checkpoint")).read().count("mymodel-7") == 2


def test_sched_ws_size_matches_header():
    """The Python loader allocates the scheduling counters the header
    promises (PGNN_SCHED_WS_INTS), and the kernels' own layout fits in them."""
    from pointgnn_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pointgnn_hip.h")).read()
    m = re.search(r"#define\s+PGNN_SCHED_WS_INTS\s+(\d+)", hdr)
    assert m and int(m.group(1)) == _lib.SCHED_WS_INTS
    src = open(os.path.join(ROOT, "point-gnn_amd", "csrc",
                            "ws_partition.h")).read()
    slices = int(re.search(r"kWsMaxSlices\s*=\s*(\d+)", src).group(1))
    groups = int(re.search(r"kWsMaxGroups\s*=\s*(\d+)", src).group(1))
    assert 2 + slices * groups <= _lib.SCHED_WS_INTS


def test_variable_scope_is_thread_local():
    """gnn.parameters / gnn.variable_scope mirror tf.variable_scope: the stack
    belongs to the calling thread, so two threads driving operators do not see
    (or corrupt) each other's scope."""
    import threading
    from pointgnn_amd import gnn
    seen = {}
    gate_a, gate_b = threading.Event(), threading.Event()

    def worker():
        seen["store_in_thread"] = gnn._state.store
        with gnn.variable_scope("other"):
            gate_a.set()
            gate_b.wait(5)
            seen["scope_in_thread"] = gnn._scope("x")

    store = gnn.ParamStore({})
    with gnn.parameters(store), gnn.variable_scope("layer1"):
        t = threading.Thread(target=worker)
        t.start()
        assert gate_a.wait(5)
        assert gnn._scope("w") == "layer1/w"       # untouched by the thread
        gate_b.set()
        t.join()
    assert seen["store_in_thread"] is None
    assert seen["scope_in_thread"] == "other/x"
    assert gnn._state.scope == [] and gnn._state.store is None


def test_bf16x3_weight_image_is_an_exact_split():
    """pgnn_pack_fc_bf16x3 (host side of csrc/edge_ws_split.h): the three bf16
    parts of every weight sum to the fp32 weight EXACTLY, sit where the
    kernel's A-operand layout expects them ([kb][t][part][lane][8]), pad with
    zeros, and the bias follows in fp32."""
    import numpy as np
    from pointgnn_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(0)
    k_in, n_out = 300, 300
    w = (rng.standard_normal((k_in, n_out)) *
         np.exp(rng.uniform(-20, 5, (k_in, n_out)))).astype(np.float32)
    b = rng.standard_normal(n_out).astype(np.float32)
    nbytes = lib.pgnn_packed_fc_bf16x3_bytes(k_in, n_out)
    kb, nt = 10, 19
    assert nbytes == kb * nt * 3 * 1024 + nt * 16 * 4
    host = np.empty(nbytes, np.uint8)
    _lib.check(lib.pgnn_pack_fc_bf16x3(w.ctypes.data, b.ctypes.data, k_in,
                                       n_out, host.ctypes.data))
    img = host[:kb * nt * 3 * 1024].view(np.uint16).reshape(kb, nt, 3, 64, 8)
    parts = (img.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    total = parts.sum(axis=2)                       # [kb, nt, lane, j]
    lane = np.arange(64)
    kk = (32 * np.arange(kb)[:, None, None, None] +
          8 * (lane >> 4)[None, None, :, None] + np.arange(8)[None, None, None])
    nn = (16 * np.arange(nt)[None, :, None, None] +
          (lane & 15)[None, None, :, None]) + 0 * kk
    kk = kk + 0 * nn
    inside = (kk < k_in) & (nn < n_out)
    want = np.where(inside, w.astype(np.float64)[np.minimum(kk, k_in - 1),
                                                 np.minimum(nn, n_out - 1)], 0.0)
    assert np.array_equal(total, want)              # exact, not approximate
    # each part is what remains after the ones before it, rounded to 8 bits
    assert np.all(np.abs(parts[:, :, 1]) <= np.abs(parts[:, :, 0]) * 2.0 ** -8 + 1e-300)
    bias = host[kb * nt * 3 * 1024:].view(np.float32)
    assert np.array_equal(bias[:n_out], b) and np.all(bias[n_out:] == 0)


def test_f16x2_weight_images_natural_and_accumulator_order():
    """pgnn_pack_fc_f16x2 / _acc (host side of csrc/edge_ws_split.h and
    pool_ws_f16.h): w0 = fp16(w), w1' = fp16((w - w0) 2^11) at
    [kb][t][part][lane][8]; the two entries differ only in WHICH row of W slot
    (g, j) of a block holds -- 8 g + j, or the order in which a lane of the
    previous layer's fp32 accumulators holds a row's features (4 g + j for
    j < 4, 16 + 4 g + j - 4 otherwise); w0 + w1' / 2^11 is within 2^-22 of w."""
    import numpy as np
    from pointgnn_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(1)
    for k_in, n_out in ((64, 128), (128, 300), (300, 300)):
        w = rng.standard_normal((k_in, n_out)).astype(np.float32)
        b = rng.standard_normal(n_out).astype(np.float32)
        kb, nt = (k_in + 31) // 32, (n_out + 15) // 16
        nbytes = lib.pgnn_packed_fc_f16x2_bytes(k_in, n_out)
        assert nbytes == kb * nt * 2 * 1024 + nt * 16 * 4
        lane, j = np.arange(64)[:, None], np.arange(8)[None, :]
        g = lane >> 4
        slot = {"pgnn_pack_fc_f16x2": 8 * g + j,
                "pgnn_pack_fc_f16x2_acc":
                    np.where(j < 4, 4 * g + j, 16 + 4 * g + (j - 4))}
        for name, within in slot.items():
            assert sorted(set(within.reshape(-1).tolist())) == list(range(32))
            host = np.empty(nbytes, np.uint8)
            _lib.check(getattr(lib, name)(w.ctypes.data, b.ctypes.data, k_in,
                                          n_out, host.ctypes.data))
            img = host[:kb * nt * 2 * 1024].view(np.float16).reshape(
                kb, nt, 2, 64, 8).astype(np.float64)
            kk = 32 * np.arange(kb)[:, None, None, None] + within[None, None]
            nn = 16 * np.arange(nt)[None, :, None, None] + \
                (lane & 15)[None, None] + 0 * kk
            kk = kk + 0 * nn
            inside = (kk < k_in) & (nn < n_out)
            want = np.where(inside, w[np.minimum(kk, k_in - 1),
                                      np.minimum(nn, n_out - 1)], 0.0)
            w0 = want.astype(np.float16).astype(np.float64)
            assert np.array_equal(img[:, :, 0], w0)
            assert np.array_equal(
                img[:, :, 1],
                ((want - w0) * 2048.0).astype(np.float16).astype(np.float64))
            err = np.abs(img[:, :, 0] + img[:, :, 1] / 2048.0 - want)
            assert np.all(err <= np.abs(want) * 2.0 ** -22 + 2.0 ** -36)
            bias = host[kb * nt * 2 * 1024:].view(np.float32)
            assert np.array_equal(bias[:n_out], b) and np.all(bias[n_out:] == 0)
    w = np.full((32, 16), 70000.0, np.float32)
    host = np.empty(lib.pgnn_packed_fc_f16x2_bytes(32, 16), np.uint8)
    assert lib.pgnn_pack_fc_f16x2_acc(w.ctypes.data, None, 32, 16,
                                      host.ctypes.data) == _lib.E_UNSUPPORTED


def test_batch_norm_layers_are_folded_and_training_refuses_them():
    """ParamStore.fc folds slim.batch_norm's inference map into a layer that
    has BatchNorm statistics instead of biases (gnn.py:17-23, 60-103); the
    folded layer equals the unfolded expression in float64.  A Trainer given
    such a config refuses it instead of training without the normalizer."""
    import copy
    from pointgnn_amd import gnn, train
    from oracle import gnn_oracle as gn
    rng = np.random.default_rng(0)
    w = rng.standard_normal((7, 5)).astype(np.float32)
    mean = rng.standard_normal(5).astype(np.float32)
    var = rng.uniform(0.3, 3.0, 5).astype(np.float32)
    beta = rng.standard_normal(5).astype(np.float32)
    x = rng.standard_normal((11, 7))
    for with_beta in (True, False):
        params = {"s/fully_connected/weights": w,
                  "s/fully_connected/BatchNorm/moving_mean": mean,
                  "s/fully_connected/BatchNorm/moving_variance": var}
        if with_beta:
            params["s/fully_connected/BatchNorm/beta"] = beta
        wf, bf = gnn.ParamStore(params).fc("s/fully_connected")
        assert wf.dtype == np.float32 and bf.dtype == np.float32
        (w64, b64), = gn._layers(params, "s", np.float64)
        ref = gn.fully_connected(x, w64, b64, relu=False)
        np.testing.assert_allclose(x @ wf.astype(np.float64) + bf, ref,
                                   rtol=0, atol=5e-6)
    # scale=True (not one of the registry's kinds, but what a checkpoint of
    # slim.batch_norm(scale=True) would hold): gamma multiplies the scale
    gamma = rng.uniform(0.5, 1.5, 5).astype(np.float32)
    params["s/fully_connected/BatchNorm/beta"] = beta
    params["s/fully_connected/BatchNorm/gamma"] = gamma
    wf, bf = gnn.ParamStore(params).fc("s/fully_connected")
    (w64, b64), = gn._layers(params, "s", np.float64)
    np.testing.assert_allclose(x @ wf.astype(np.float64) + bf,
                               gn.fully_connected(x, w64, b64, relu=False),
                               rtol=0, atol=5e-6)
    with pytest.raises(KeyError, match="neither biases nor BatchNorm"):
        gnn.ParamStore({"s/fully_connected/weights": w}).fc("s/fully_connected")
    gnn._check_kinds("ReLU", "fused_BN_center")
    with pytest.raises(NotImplementedError, match="normalization 'IN'"):
        gnn._check_kinds("ReLU", "IN")
    with pytest.raises(NotImplementedError, match="activation 'ELU'"):
        gnn._check_kinds("ELU", "NONE")
    cfg = copy.deepcopy(configs.get_config("car_auto_T3"))
    cfg["model_kwargs"]["layer_configs"][1]["kwargs"][
        "edge_MLP_normalization_type"] = "BN"
    import torch
    if not torch.cuda.is_available():
        # the check sits behind the Trainer's no-CPU-fallback guard: call it on
        # the config the way __init__ does
        with pytest.raises(NotImplementedError, match="no training path"):
            train.check_trainable_kinds(cfg)
    train.check_trainable_kinds(configs.get_config("car_auto_T3"))


# ---- the weights-stationary partition (csrc/ws_partition.h), host only --------
_WS_WRAPPERS = r"""
#include "ws_partition.h"
using namespace pgnn;
extern "C" {
int t_sizeof() { return (int)sizeof(WsGeometry); }
int t_slices(int cus, int ws_xcds) { return ws_slice_count(cus, ws_xcds); }
int t_feasible(int nt, int ntmax, int cus, int slices) {
  return ws_feasible(nt, ntmax, cus, slices) ? 1 : 0;
}
int t_partition(WsGeometry *g, int nt, int ntmax, int cus, int slices) {
  return ws_partition(*g, nt, ntmax, cus, slices);
}
void t_balance(WsGeometry *g, int cus, const double *cost, int pool) {
  ws_balance(*g, cus, cost, pool != 0);
}
}
"""


def _ws_partition_lib(tmp_path):
    """csrc/ws_partition.h alone, through the host C++ compiler (g++, else the
    clang++ hipcc drives): the header must not need HIP."""
    import shutil
    import subprocess
    cands = [shutil.which("g++")]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    cands += [os.path.join(rocm, "lib", "llvm", "bin", "clang++"),
              os.path.join(rocm, "llvm", "bin", "clang++")]
    cxx = next((c for c in cands if c and os.path.exists(c)), None)
    assert cxx, "no host C++ compiler (g++ or ROCm's clang++) found"
    src = tmp_path / "ws_partition_test.cpp"
    src.write_text(_WS_WRAPPERS)
    so = tmp_path / "libws_partition_test.so"
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-shared",
                           "-fPIC", "-I", os.path.join(ROOT, "point-gnn_amd",
                                                       "csrc"),
                           "-o", str(so), str(src)])
    return ctypes.CDLL(str(so))


class _WsGeometry(ctypes.Structure):
    _fields_ = [("groups", ctypes.c_int), ("xcds", ctypes.c_int),
                ("tile0", ctypes.c_int * 5), ("wg0", ctypes.c_int * 5),
                ("balanced", ctypes.c_int), ("n_wg", ctypes.c_int * 4),
                ("swg0", (ctypes.c_short * 5) * 8),
                ("sbase", (ctypes.c_short * 4) * 8)]


def _ws_partition_py(nt, ntmax, cus, slices):
    """The partition restated: column tiles as evenly as possible in
    ceil(nt / ntmax) groups, a slice's workgroups in proportion to the tiles,
    largest remainder, the first maximum wins.  None: cannot be served."""
    groups = -(-nt // ntmax)
    per_slice = cus // slices
    if groups > 4 or per_slice < groups:
        return None
    base, extra = divmod(nt, groups)
    size = [base + (1 if g < extra else 0) for g in range(groups)]
    if base < ntmax - 1 or max(size) > ntmax:
        return None
    cnt = [max(1, per_slice * s // nt) for s in size]
    frac = [per_slice * s % nt for s in size]
    if sum(cnt) > per_slice:
        return None
    while sum(cnt) < per_slice:
        best = frac.index(max(frac))
        cnt[best] += 1
        frac[best] = -1
    tile0 = [sum(size[:g]) for g in range(groups + 1)]
    wg0 = [sum(cnt[:g]) for g in range(groups + 1)]
    return tile0, wg0


def test_ws_partition_header_on_every_geometry(tmp_path):
    """csrc/ws_partition.h is the one statement of the column-group partition
    (the `*_applies` predicates and every launcher go through it): on the six
    (column tiles, largest group) shapes in use x CU counts 8..512 x ws_xcds
    1..64 its feasibility answer IS the partition's, the partition equals a
    restatement in Python, and the balanced form keeps its invariants under
    the five cost models of the callers."""
    lib = _ws_partition_lib(tmp_path)
    assert lib.t_sizeof() == ctypes.sizeof(_WsGeometry)
    lib.t_balance.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                              ctypes.c_int]
    shapes = [(19, 7), (16, 8), (32, 8), (19, 5), (16, 5), (16, 6)]
    # relative cost of a row tile of `size` column tiles, per caller:
    # fp32 at KQ = 19 / 16, bf16x3 at KB = 10 / 8, f16x2 at KB = 10 (gnn.hip's
    # launchers; f16x2 at KB = 8 is 0.8 of a model already here up to scale)
    models = [lambda s: 128.0 * 19 * s + 1900.0,
              lambda s: 128.0 * 16 * s + 1900.0,
              lambda s: 960.0 * s + 2400.0,
              lambda s: 960.0 * 8 / 10 * s + 2400.0,
              lambda s: 480.0 * s + 1600.0]
    n_cases = n_feasible = n_balanced = 0
    for nt, ntmax in shapes:
        for cus in range(8, 513, 8):
            for ws_xcds in range(1, 65):
                n_cases += 1
                slices = lib.t_slices(cus, ws_xcds)
                assert slices == (ws_xcds if cus % ws_xcds == 0 else 8)
                g = _WsGeometry()
                why = lib.t_partition(ctypes.byref(g), nt, ntmax, cus, slices)
                feasible = lib.t_feasible(nt, ntmax, cus, slices)
                assert feasible == (1 if why == 0 else 0)
                want = _ws_partition_py(nt, ntmax, cus, slices)
                assert (want is not None) == (why == 0), (nt, ntmax, cus, slices)
                if want is None:
                    continue
                n_feasible += 1
                tile0, wg0 = want
                assert g.groups == len(tile0) - 1 and g.xcds == slices
                assert list(g.tile0)[:g.groups + 1] == tile0
                assert list(g.wg0)[:g.groups + 1] == wg0
                assert wg0[-1] == cus // slices and tile0[-1] == nt
                for model in models:
                    cost = (ctypes.c_double * 4)(*[
                        model(tile0[i + 1] - tile0[i])
                        for i in range(g.groups)])
                    lib.t_balance(ctypes.byref(g), cus, cost, 1)
                    assert g.balanced == 0          # never with a tile pool
                    lib.t_balance(ctypes.byref(g), cus, cost, 0)
                    if not g.balanced:
                        assert slices > 8 or g.groups < 2, (nt, cus, slices)
                        continue
                    n_balanced += 1
                    per_slice = cus // slices
                    run = [0] * g.groups
                    for s in range(slices):
                        c = [g.swg0[s][i + 1] - g.swg0[s][i]
                             for i in range(g.groups)]
                        assert g.swg0[s][0] == 0 and min(c) >= 1
                        assert sum(c) == per_slice
                        assert [g.sbase[s][i] for i in range(g.groups)] == run
                        run = [a + b for a, b in zip(run, c)]
                    assert run == list(g.n_wg)[:g.groups]
                    assert sum(run) == per_slice * slices
    assert n_cases == 24576 and n_feasible == 23601
    assert n_balanced > 0
    # the splits the design documents for the whole chip, 256 CUs in 8 slices:
    # fp32, 7/6/6 tiles: 12/10/10 workgroups in every slice (static)
    g = _WsGeometry()
    assert lib.t_partition(ctypes.byref(g), 19, 7, 256, 8) == 0
    assert list(g.tile0)[:4] == [0, 7, 13, 19]
    assert list(g.wg0)[:4] == [0, 12, 22, 32]
    # bf16x3, 5/5/5/4 tiles: 9/8/8/7 workgroups per XCD as the static split,
    # balanced to 66/66/66/58 over the chip (shares 66.21 x 3 and 57.38: the
    # 256th workgroup goes to the largest remainder)
    assert lib.t_partition(ctypes.byref(g), 19, 5, 256, 8) == 0
    assert list(g.tile0)[:5] == [0, 5, 10, 15, 19]
    assert list(g.wg0)[:5] == [0, 9, 17, 25, 32]
    cost = (ctypes.c_double * 4)(*[models[2](s) for s in (5, 5, 5, 4)])
    lib.t_balance(ctypes.byref(g), 256, cost, 0)
    assert g.balanced == 1 and list(g.n_wg) == [66, 66, 66, 58]


# ---- the native trainer's workspace layout (csrc/trainer_layout.h), host only ---
_LAYOUT_WRAPPERS = r"""
#include <string.h>
#include "trainer_layout.h"
using namespace pgnn;
extern "C" {
int t_sizeof_shape() { return (int)sizeof(TrainerShape); }
// Both layouts of a two-level batch (N, K, E0, E1) over `base` (null: sizing).
// Returns the number of spans (all of them in out[] when <= cap), -1 when
// layout_forward refuses.  info: spans and high-water mark of the forward, the
// final high-water mark, then the offsets of scratch, logits, pred, dhs[0], dq
// of the last stage and the weight-gradient partial slice.
int t_layout(const TrainerShape *sh, const int64_t *nkee, size_t scratch,
             size_t wgrad, char *base, BumpSpan *out, int cap, size_t *info) {
  pgnn_train_batch b;
  memset(&b, 0, sizeof b);
  b.n_levels = 2;
  b.n_feat = 1;
  b.n_vertices[0] = nkee[0];
  b.n_vertices[1] = b.n_vertices[2] = nkee[1];
  b.n_edges[0] = nkee[2];
  b.n_edges[1] = nkee[3];
  std::vector<BumpSpan> log;
  Bump ws(base, (size_t)1 << 40, &log);
  Saved sv;
  Grads gr;
  memset(&sv, 0, sizeof sv);
  memset(&gr, 0, sizeof gr);
  if (!layout_forward(*sh, b, scratch, ws, sv)) return -1;
  info[0] = log.size();
  info[1] = ws.high;
  layout_backward(*sh, b, wgrad, ws, sv, gr);
  info[2] = ws.high;
  const char *zero = base ? base : (const char *)256;  // (sizing: offset + 256)
  const void *named[6] = {sv.scratch, sv.heads.logits, sv.heads.pred, gr.dhs[0],
                          gr.stage[sh->n_stages - 1].dq, gr.wgrad_part};
  for (int i = 0; i < 6; ++i) info[3 + i] = (size_t)((const char *)named[i] - zero);
  for (size_t i = 0; i < log.size() && (int)i < cap; ++i) out[i] = log[i];
  return (int)log.size();
}
}
"""


class _FcShape(ctypes.Structure):
    _fields_ = [("k_in", ctypes.c_int), ("n_out", ctypes.c_int)]


class _StageShape(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int), ("level", ctypes.c_int),
                ("n_a", ctypes.c_int), ("n_b", ctypes.c_int),
                ("n_c", ctypes.c_int), ("a", _FcShape * 8), ("b", _FcShape * 8),
                ("c", _FcShape * 8), ("want_wt", ctypes.c_bool)]


class _TrainerShape(ctypes.Structure):
    _fields_ = [("n_stages", ctypes.c_int), ("stages", _StageShape * 8),
                ("n_groups", ctypes.c_int), ("group_w", (ctypes.c_int * 3) * 4),
                ("cls_w", ctypes.c_int), ("loc_w", (ctypes.c_int * 3) * 16),
                ("num_classes", ctypes.c_int), ("box_len", ctypes.c_int)]


class _BumpSpan(ctypes.Structure):
    _fields_ = [("off", ctypes.c_size_t), ("bytes", ctypes.c_size_t),
                ("released", ctypes.c_int)]


@pytest.fixture(scope="module")
def trainer_layout_lib(tmp_path_factory):
    """csrc/trainer_layout.h alone through the host C++ compiler, as
    _ws_partition_lib builds its header: it must not need HIP."""
    import shutil
    import subprocess
    tmp = tmp_path_factory.mktemp("trainer_layout")
    cands = [shutil.which("g++")]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    cands += [os.path.join(rocm, "lib", "llvm", "bin", "clang++"),
              os.path.join(rocm, "llvm", "bin", "clang++")]
    cxx = next((c for c in cands if c and os.path.exists(c)), None)
    assert cxx, "no host C++ compiler (g++ or ROCm's clang++) found"
    src = tmp / "trainer_layout_test.cpp"
    src.write_text(_LAYOUT_WRAPPERS)
    so = tmp / "libtrainer_layout_test.so"
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "point-gnn_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"),
                           "-o", str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    assert lib.t_sizeof_shape() == ctypes.sizeof(_TrainerShape)
    lib.t_layout.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                             ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
                             ctypes.c_int, ctypes.c_void_p]
    return lib


def _trainer_shape(point_mlp, out_mlp, width, offset_mlp, T, num_classes,
                   fused, sparse):
    """The shape of a shipped model as pgnn_trainer_create derives it: n_feat =
    1, box_len = 7, heads C -> 64 -> nc and C -> 64 -> 64 -> 7, fused into
    groups of at most 320 columns the way plan_head_groups does."""
    def chain(dst, k_in, widths):
        for i, n_out in enumerate(widths):
            dst[i].k_in, dst[i].n_out = k_in, n_out
            k_in = n_out
        return len(widths)
    sh = _TrainerShape()
    sh.n_stages = 1 + T
    s = sh.stages[0]
    s.kind, s.level = 0, 0
    s.n_a = chain(s.a, 1 + 3, point_mlp)
    s.n_b = chain(s.b, point_mlp[-1], out_mlp)
    s.want_wt = sparse
    for i in range(T):
        s = sh.stages[1 + i]
        s.kind, s.level = 1, 1
        s.n_a = chain(s.a, width + 3, [width, width])
        s.n_b = chain(s.b, width, [width, width])
        s.n_c = chain(s.c, width, offset_mlp)
        s.want_wt = sparse
    sh.num_classes, sh.box_len = num_classes, 7
    hw = 64
    if fused:
        lids, first = num_classes, True
        while first or lids:
            take = min(lids, 320 // hw - (1 if first else 0))
            base = 16 if first else 0
            g = sh.group_w[sh.n_groups]
            g[0] = hw * (take + (1 if first else 0))
            g[1] = base + hw * take
            g[2] = base + 8 * take
            sh.n_groups += 1
            lids -= take
            first = False
    else:
        sh.cls_w = hw
        for j in range(num_classes):
            sh.loc_w[j][0], sh.loc_w[j][1], sh.loc_w[j][2] = hw, hw, 7
    return sh


_LAYOUT_MODELS = {
    "car_auto_T3": ([32, 64, 128, 300], [300, 300], 300, [64, 3], 3, 4),
    "car_auto_T1": ([32, 64, 128, 300], [300, 300], 300, [64, 3], 1, 4),
    "car_fixed_T3": ([32, 64, 128, 300], [300, 300], 300, [], 3, 4),
    "ped_cyl_auto_T3": ([32, 64, 128, 256, 512], [256, 256], 256, [64, 3], 3, 6),
}
_LAYOUT_BATCHES = [(0, 0, 0, 0), (5, 1, 5, 0), (40, 7, 33, 12),
                   (1000, 300, 4000, 9000), (20000, 3352, 347456, 674852)]


@pytest.mark.parametrize("sparse", [True, False], ids=["sparse", "dense"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "separate"])
@pytest.mark.parametrize("model", sorted(_LAYOUT_MODELS))
def test_trainer_layout_buffers_are_aligned_disjoint_and_repeatable(
        trainer_layout_lib, model, fused, sparse):
    """csrc/trainer_layout.h is the one statement of where the native training
    step keeps its buffers (the sizing query, the forward and the backward all
    call it).  For the shipped models, fused and separate heads, the sparse
    and the dense last per-edge layer, from an empty batch to a full-size car
    frame: every buffer starts on a 256-byte boundary and ends below the
    high-water mark; buffers that are live together do not overlap (only a
    backward stage's E-row temporaries are ever released, with their stage);
    the backward's buffers lie behind everything the forward keeps; and a
    second layout, over a base address instead of the sizing run's null,
    gives the same offsets."""
    lib = trainer_layout_lib
    sh = _trainer_shape(*_LAYOUT_MODELS[model], fused, sparse)
    assert sh.n_groups == (0 if not fused else 1 if sh.num_classes == 4 else 2)
    scratch, wgrad = 1 << 20, 64 << 20
    # E-row temporaries: ge / ga per layer below the last (not for a two-layer
    # GNN stage's sparse adjoint, which writes dP / dQ), gz and ties when dense
    n_temp = sum((0 if s.kind == 1 and sparse and s.n_a == 2 else s.n_a - 1) +
                 (0 if sparse else 2)
                 for s in list(sh.stages)[:sh.n_stages])
    for sizes in _LAYOUT_BATCHES:
        nkee = (ctypes.c_int64 * 4)(*sizes)
        runs = []
        for base in (None, 1 << 32):
            spans = (_BumpSpan * 512)()
            info = (ctypes.c_size_t * 9)()
            n = lib.t_layout(ctypes.byref(sh), nkee, scratch, wgrad, base, spans,
                             512, info)
            assert 0 < n <= 512
            runs.append(([(s.off, s.bytes, s.released) for s in spans[:n]],
                         list(info)))
        assert runs[0] == runs[1], sizes
        spans, (n_fwd, fwd_high, high, *named) = runs[0]
        assert 0 < n_fwd < len(spans) and fwd_high <= high
        for i, (off, nbytes, released) in enumerate(spans):
            assert off % 256 == 0 and off + nbytes <= high, (sizes, i)
            if i >= n_fwd:
                assert off >= fwd_high, (sizes, i)
            if released >= 0:      # given back once span `released` is made
                assert n_fwd <= i < released <= len(spans), (sizes, i)
            for j in range(i + 1, len(spans)):
                if released < 0 or j < released:      # i is live when j is made
                    o2, b2, _ = spans[j]
                    assert off + nbytes <= o2 or o2 + b2 <= off, (sizes, i, j)
        assert sum(1 for s in spans if s[2] >= 0) == n_temp, sizes
        # the records point at the spans: the first and the last buffer of
        # either direction and two in between
        N, K, E0, E1 = sizes
        at = {off: nbytes for off, nbytes, _ in spans if nbytes}
        assert named[0] == 0 and spans[0] == (0, scratch, -1)
        assert spans[-1] == (named[5], wgrad, -1)
        assert spans[n_fwd - 1][0] == named[2]
        assert spans[n_fwd][0] == named[3] >= fwd_high
        if K:
            assert at[named[1]] == K * 16 * 4               # logits [K, pad(nc)]
            assert at[named[2]] == K * sh.num_classes * 7 * 4
            width = _LAYOUT_MODELS[model][2]
            wq = (width + 15) // 16 * 16
            assert at[named[3]] == K * wq * 4               # dhs[0] [K, hw]
            assert at[named[4] - K * wq * 4] == 2 * K * wq * 4   # dP | dQ
