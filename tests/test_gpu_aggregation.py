"""Sum and mean aggregation in GraphNetAutoCenter and PointSetPooling
(gnn.graph_scatter_sum_fn / graph_scatter_mean_fn as `aggregation_fn`; the
pgnn_*_agg_* entries; csrc/ws_sum.h).

A. Integer-valued inputs: every fp32 partial sum is an integer below 2^24, so
   the result does not depend on the order of the additions and a dropped or
   doubled row changes it -- the sum must EQUAL the int64 reference.
B. The same at grid geometries of the weights-stationary kernels (a sum is not
   idempotent: a tile covered twice, invisible under max, is wrong here).
C. Real-valued inputs: the fused sum against the float64 sum of the device's
   own per-edge rows, within the recursive-summation bound deg 2^-24 A.
D. Whole models against a float64 evaluation, 1e-3 relative to the layer's
   magnitude (the project's parity tolerance), launch fusion on / off, the
   capacity form, edge_arith.
E. The surface: unknown aggregators, unknown codes, max through the new
   entries."""
import ctypes

import numpy as np
import pytest

import pointgnn_amd  # noqa: F401
from pointgnn_amd import configs, weights
import _ws_cases as wc
import _aggregation as ag

pytestmark = pytest.mark.gpu
WS, GENERAL = 4096 | 16384, 2048 | 8192      # mlp_debug: forced kernels
AGG = {"max": 0, "sum": 1, "mean": 2}


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


class forced(object):
    """`mlp_debug` set for the block, 0 afterwards."""

    def __init__(self, bits):
        self.bits = bits

    def __enter__(self):
        from pointgnn_amd import _lib
        _lib.set_tunable("mlp_debug", self.bits)

    def __exit__(self, *exc):
        from pointgnn_amd import _lib
        _lib.set_tunable("mlp_debug", 0)


# ---- the stages through the C ABI ---------------------------------------------
class Stage(object):
    """One stage ("edge" at width c, or car "pool") on one input: device
    buffers made once, launched with any aggregation on the current stream."""

    def __init__(self, dev, kind, inp):
        import torch
        from pointgnn_amd import _lib, gnn
        self.dev, self.kind, self.inp = dev, kind, inp
        self.lib = _lib.load()
        store = gnn.ParamStore({}, device=dev)
        if kind == "edge":
            self.p, self.q = T(inp["p"], dev), T(inp["q"], dev)
            self.chain = gnn.Chain(store, [(inp["w"], inp["b"], 0)])
        else:
            self.feat, self.xyz = T(inp["inten"], dev), T(inp["xyz"], dev)
            self.kp = T(inp["kp_buf"], dev)
            self.chain = gnn.Chain(store, inp["layers"])
        self.edges = T(inp["buf"], dev)
        self.ne = self.nk = None
        if inp["case"] == "capacity":
            i32 = lambda v: torch.tensor([v], dtype=torch.int32, device=dev)
            self.ne = _lib.DeviceCount(i32(inp["n_live"]), inp["n_live"])
            self.nk = _lib.DeviceCount(i32(inp["k"]), inp["k"])

    def head(self, out):
        from pointgnn_amd import _lib
        ptr, inp = _lib.ptr, self.inp
        n, k, ld = len(inp["buf"]), inp["k_cap"], inp["wq"]
        tail = (inp["sorted"], ptr(out), ld, ptr(_lib.sched_ws(self.dev)))
        if self.kind == "edge":
            return (ptr(self.p), ptr(self.q), ld, inp["c"], ptr(self.edges), n,
                    k, self.chain.array, 1) + tail
        return (ptr(self.feat), 1, ptr(self.xyz), ptr(self.kp), ptr(self.edges),
                n, k, self.chain.array, self.chain.n) + tail

    def names(self):
        return "pgnn_edge_mlp_scatter_agg" if self.kind == "edge" else \
            "pgnn_point_set_pooling_agg"

    def query(self, aggregation):
        """(code, bytes) of the workspace query for this call."""
        from pointgnn_amd import _lib
        inp = self.inp
        nbytes = ctypes.c_size_t(0)
        rc = getattr(self.lib, self.names() + "_workspace_bytes")(
            self.chain.array, self.chain.n,
            inp["c"] if self.kind == "edge" else 1, len(inp["buf"]),
            inp["n_live"] if self.ne else 0, inp["k_cap"], AGG[aggregation],
            1 if self.ne else 0, _lib.stream_ptr(), ctypes.byref(nbytes))
        return rc, nbytes.value

    def run(self, aggregation, poison=7.0):
        """-> (code, out [k, padded width] as NumPy, or None when declined).
        `out` starts poisoned: the entry fills it itself."""
        import torch
        from pointgnn_amd import _lib
        inp = self.inp
        out = torch.full((inp["k_cap"], inp["wq"]), poison, dtype=torch.float32,
                         device=self.dev)
        rc, nbytes = self.query(aggregation)
        if rc == _lib.E_UNSUPPORTED:
            assert self.ne is not None, "a host-sized call must be total"
        else:
            _lib.check(rc, "workspace query")
        work = torch.full(((nbytes + 3) // 4 + 1,), 3e38, dtype=torch.float32,
                          device=self.dev)
        tail = (AGG[aggregation], _lib.ptr(work), nbytes, _lib.stream_ptr())
        if self.ne:
            rc2 = getattr(self.lib, self.names() + "_fwd_dyn")(
                *self.head(out), self.ne.arg(), self.nk.arg(), *tail)
        else:
            rc2 = getattr(self.lib, self.names() + "_fwd")(*self.head(out), *tail)
        if rc2 == _lib.E_UNSUPPORTED or rc == _lib.E_UNSUPPORTED:
            assert rc2 == rc == _lib.E_UNSUPPORTED, \
                "query and entry disagree: %d, %d" % (rc, rc2)
            torch.cuda.synchronize()
            assert bool((out == poison).all()), "a declining entry wrote `out`"
            return rc2, None
        _lib.check(rc2, self.names())
        res = out.cpu().numpy()[:inp["k"]]
        assert int(_lib.sched_ws(self.dev).abs().sum().item()) == 0, \
            "tile-pool counters not handed back zeroed"
        return 0, res


_STAGES, _REFS = {}, {}


def exact_stage(dev, kind, c, case):
    """(Stage, sum int64, in-degree) on the integer-valued input, made once."""
    key = (kind, c, case)
    if key not in _STAGES:
        if kind == "edge":
            inp = ag.exact_edge_input(case, c)
            rows, dst = ag.edge_rows_i64(inp)
        else:
            inp = ag.exact_pool_input(case)
            rows, dst = ag.pool_rows_i64(inp)
        _REFS[key] = ag.exact_reference(rows, dst, inp["k"])
        _STAGES[key] = Stage(dev, kind, inp)
    return (_STAGES[key],) + _REFS[key]


LEGS = [("edge", 300), ("edge", 256), ("pool", 300)]


# ---- A: exact ------------------------------------------------------------------
@pytest.mark.parametrize("path", ["ws", "general"])
@pytest.mark.parametrize("case", wc.INPUTS)
@pytest.mark.parametrize("kind,c", LEGS, ids=["edge300", "edge256", "pool"])
def test_exact_sums_through_the_abi(dev, kind, c, case, path):
    """Sum == the int64 reference, mean within one rounding of sum / degree,
    empty segments and pad columns exactly 0 -- on the weights-stationary
    kernel and on the composed general path; the capacity-form entry declines
    (PGNN_E_UNSUPPORTED, nothing written) where only the general path is
    left."""
    from pointgnn_amd import _lib
    st, s, deg = exact_stage(dev, kind, c, case)
    with forced(WS if path == "ws" else GENERAL):
        for aggregation in ("sum", "mean"):
            rc, got = st.run(aggregation)
            what = "%s %d %s %s %s" % (kind, c, case, path, aggregation)
            if case == "capacity" and path == "general":
                assert rc == _lib.E_UNSUPPORTED, what
                continue
            assert rc == 0, what
            ag.check_exact(got, s, deg, aggregation, c, what)


def _layer_params(kind, inp, rng):
    """A ParamStore's variables for one layer class that reproduces the exact
    stage: (params, kwargs of apply_regular, integer vertex inputs)."""
    c = inp["c"]
    if kind == "pool":
        params = {}
        for n, (w, b, _) in zip(weights.mlp_names(
                "L/extract_vertex_features", 4), inp["layers"]):
            params[n + "/weights"], params[n + "/biases"] = w, b
        n = weights.mlp_names("L/combined_features", 1)[0]
        params[n + "/weights"] = np.zeros((c, 16), np.float32)
        params[n + "/biases"] = np.zeros(16, np.float32)
        kw = dict(point_MLP_depth_list=[32, 64, 128, 300],
                  point_MLP_normalization_type='NONE',
                  output_MLP_depth_list=[16],
                  output_MLP_normalization_type='NONE')
        return params, kw, None
    # edge: W1 = [I; Wx], b1 = 0, no offset => P = h + x Wx, Q = x Wx and the
    # hidden row is ReLU(h[s] + (x[s] - x[d]) Wx): h in [-2, 2], x in [-1, 1],
    # one +-1 per column of Wx => hidden <= 4, rows <= 4 * 4 + 3
    k = inp["k_cap"]
    h = rng.integers(-2, 3, (k, c)).astype(np.float32)
    x = rng.integers(-1, 2, (k, 3)).astype(np.float32)
    wx = ag.sparse_signs(rng, 3, c, 1)
    n1, n2 = weights.mlp_names("L/extract_vertex_features", 2)
    nu = weights.mlp_names("L/combined_features", 1)[0]
    params = {n1 + "/weights": np.concatenate([np.eye(c, dtype=np.float32), wx]),
              n1 + "/biases": np.zeros(c, np.float32),
              n2 + "/weights": inp["w"], n2 + "/biases": inp["b"],
              nu + "/weights": np.zeros((c, c), np.float32),
              nu + "/biases": np.zeros(c, np.float32)}
    kw = dict(edge_MLP_depth_list=[c, c], edge_MLP_normalization_type='NONE',
              update_MLP_depth_list=[c], update_MLP_normalization_type='NONE',
              auto_offset=False)
    xw = x @ wx
    inp["p"], inp["q"] = np.zeros_like(inp["p"]), np.zeros_like(inp["q"])
    inp["p"][:, :c], inp["q"][:, :c] = h + xw, xw
    return params, kw, (h, x)


@pytest.mark.parametrize("path", ["ws", "general"])
@pytest.mark.parametrize("case", ["fanins", "shuffled", "capacity"])
@pytest.mark.parametrize("kind", ["edge", "pool"])
def test_exact_sums_through_the_layer_classes(dev, kind, case, path):
    """The same through PointSetPooling / GraphNetAutoCenter.apply_regular
    (fuse_vertex_stages on and off, a DeviceCount-tagged capacity form); the
    aggregated stage is read through gnn.AGGREGATE_TAP.  Capacity form without
    the weights-stationary kernel: the documented NotImplementedError."""
    import torch
    from pointgnn_amd import _lib, gnn
    rng = np.random.default_rng(5)
    inp = ag.exact_edge_input(case, 300) if kind == "edge" else \
        ag.exact_pool_input(case)
    params, kw, vert = _layer_params(kind, inp, rng)
    rows, dst = (ag.edge_rows_i64 if kind == "edge" else ag.pool_rows_i64)(inp)
    s, deg = ag.exact_reference(rows, dst, inp["k"])
    store = gnn.ParamStore(params, dev)
    edges = T(inp["buf"], dev)
    ne = nk = None
    if case == "capacity":
        i32 = lambda v: torch.tensor([v], dtype=torch.int32, device=dev)
        ne = _lib.DeviceCount(i32(inp["n_live"]), inp["n_live"])
        nk = _lib.DeviceCount(i32(inp["k"]), inp["k"])
        _lib.tag_count(edges, ne)
    for aggregation, fn in (("sum", gnn.graph_scatter_sum_fn),
                            ("mean", gnn.graph_scatter_mean_fn)):
        for fuse in (False, True):
            if kind == "edge":
                op = gnn.GraphNetAutoCenter(aggregation_fn=fn)
                args = (_lib.tag_count(T(vert[0], dev), nk), T(vert[1], dev),
                        None, edges)
            else:
                op = gnn.PointSetPooling(aggregation_fn=fn)
                args = (T(inp["inten"], dev), T(inp["xyz"], dev),
                        _lib.tag_count(T(inp["kp_buf"].reshape(-1, 1), dev), nk),
                        edges)
            gnn.AGGREGATE_TAP = tap = []
            try:
                with forced(WS if path == "ws" else GENERAL), \
                        gnn.parameters(store), gnn.variable_scope("L"):
                    if case == "capacity" and path == "general":
                        with pytest.raises(NotImplementedError,
                                           match="capacity form"):
                            with gnn.fuse_vertex_stages(fuse):
                                op.apply_regular(*args, **kw)
                        continue
                    with gnn.fuse_vertex_stages(fuse):
                        op.apply_regular(*args, **kw)
            finally:
                gnn.AGGREGATE_TAP = None
            assert len(tap) == 1
            got = tap[0].cpu().numpy()[:inp["k"]]
            ag.check_exact(got, s, deg, aggregation, inp["c"],
                           "%s %s %s %s fuse=%s" % (kind, case, path,
                                                    aggregation, fuse))


# ---- B: grid geometries ----------------------------------------------------------
GEOS = [wc.Geo(256, 0, 8, 1, 0, 2), wc.Geo(72, 0, 8, 1, 0, 2),
        wc.Geo(256, 0, 1, 1, 0, 2), wc.Geo(256, 0, 8, 0, 80, 1),
        wc.Geo(256, 0, 8, 2, 15, 2), wc.Geo(240, 8, 4, 2, 80, 5)]
POOL_GEOS = [wc.DEFAULT, wc.DEFAULT._replace(pool=80, chunk=1)]
_STAMPS = {}


def _stamp_buffer(dev, waves):
    import torch
    if "buf" not in _STAMPS:
        _STAMPS["buf"] = torch.zeros((256 * wc.WAVES + 8) * wc.STAMP_STRIDE,
                                     dtype=torch.int64, device=dev)
    buf = _STAMPS["buf"][:(waves + 8) * wc.STAMP_STRIDE]
    buf.zero_()
    return buf


def _at_geometry(dev, kind, c, case, g):
    """Exact sums at geometry `g` with the weights-stationary kernel forced.
    Where _ws_cases.runs() says the kernel runs, its stamps show that it did
    and that every (row tile, column group) had one owner; where it says the
    kernel does not, the capacity-form query declines and the host-sized entry
    is still exact (the general path)."""
    import torch
    from pointgnn_amd import _lib
    assert torch.cuda.get_device_properties(dev).multi_processor_count == 256, \
        "the geometry list is written for the MI355X's 256 CUs"
    st, s, deg = exact_stage(dev, kind, c, case)
    leg = "edge_f32" if kind == "edge" else "pool_car"
    expect = wc.runs(leg, c, g)
    cus, xcds = wc.effective(g)
    what = "%s %d %s at %s" % (kind, c, case, wc.geo_id(g))
    with wc.masked_stream(g.stream) as stream, torch.cuda.stream(stream), \
            wc.tunables(g), forced(WS):
        grid = cus if kind == "pool" else cus // xcds * xcds
        stamps = _stamp_buffer(dev, grid * wc.WAVES) if expect else None
        st.lib.pgnn_set_debug_buffer(_lib.ptr(stamps))
        try:
            rc, got = st.run("sum")
        finally:
            st.lib.pgnn_set_debug_buffer(None)
        assert rc == 0, what
        # what the capacity form would answer at this geometry
        nbytes = ctypes.c_size_t(0)
        rc_dyn = getattr(st.lib, st.names() + "_workspace_bytes")(
            st.chain.array, st.chain.n, c if kind == "edge" else 1,
            len(st.inp["buf"]), 0, st.inp["k_cap"], AGG["sum"], 1,
            _lib.stream_ptr(), ctypes.byref(nbytes))
        assert rc_dyn == (0 if expect else _lib.E_UNSUPPORTED), what
        torch.cuda.synchronize()
    ag.check_exact(got, s, deg, "sum", c, what)
    if stamps is not None:
        stn = stamps.cpu().numpy().reshape(-1, wc.STAMP_STRIDE)
        n_wt = (st.inp["n_live"] + 15) // 16
        pooled = g.pool > 0 and xcds <= wc.MAX_SLICES
        if kind == "pool":
            wc.check_pool_stamps(stn, n_wt, cus, account=g.pool == 0)
        else:
            wc.check_edge_stamps(
                stn, n_wt, cus, xcds, wc.grouping(*wc.SHAPES[(leg, c)]),
                balanced=g.balance == 2 and not pooled and
                xcds <= wc.MAX_SLICES, account=not pooled)


@pytest.mark.parametrize("case", ["fanins", "one_segment"])
@pytest.mark.parametrize("geo", GEOS, ids=[wc.geo_id(g) for g in GEOS])
def test_exact_edge_sums_at_geometry(dev, geo, case):
    _at_geometry(dev, "edge", 300, case, geo)


@pytest.mark.parametrize("case", ["fanins", "one_segment"])
@pytest.mark.parametrize("geo", POOL_GEOS, ids=[wc.geo_id(g) for g in POOL_GEOS])
def test_exact_pool_sums_at_geometry(dev, geo, case):
    _at_geometry(dev, "pool", 300, case, geo)


# ---- C: real-valued inputs, summation error only ----------------------------------
def _device_rows(dev, st, path):
    """The per-edge rows the stage adds, from the entries that write them: the
    training-forward kernels (weights-stationary; same accumulators, bias and
    ReLU) or the primitives the general path is composed of."""
    import torch
    from pointgnn_amd import _lib
    lib, inp, ptr = st.lib, st.inp, _lib.ptr
    n, k, ld = len(inp["buf"]), inp["k_cap"], inp["wq"]
    out = torch.empty((k, ld), dtype=torch.float32, device=dev)
    rows = torch.empty((n, ld), dtype=torch.float32, device=dev)
    sp = _lib.stream_ptr()
    if st.kind == "edge" and path == "ws":
        _lib.check(lib.pgnn_edge_mlp_scatter_max_rows_fwd(
            ptr(st.p), ptr(st.q), ld, inp["c"], ptr(st.edges), n, k,
            st.chain.array, inp["sorted"], ptr(out), ld, ptr(rows), ld, None,
            sp), "pgnn_edge_mlp_scatter_max_rows_fwd")
    elif st.kind == "edge":
        h1 = torch.empty((n, ld), dtype=torch.float32, device=dev)
        _lib.check(lib.pgnn_edge_hidden_fwd(ptr(st.p), ptr(st.q), ld,
                                            ptr(st.edges), n, ptr(h1), sp),
                   "pgnn_edge_hidden_fwd")
        _lib.check(lib.pgnn_mlp_fwd(ptr(h1), ld, inp["c"], None, 0, 0, n,
                                    st.chain.array, 1, None, 0, ptr(rows), ld,
                                    sp), "pgnn_mlp_fwd")
    elif path == "ws":
        acts = [torch.empty((n, w), dtype=torch.float32, device=dev)
                for w in (32, 64, 128)] + [rows]
        arr = (ctypes.c_void_p * 4)(*[a.data_ptr() for a in acts])
        _lib.check(lib.pgnn_point_set_pooling_rows_fwd(
            ptr(st.feat), 1, ptr(st.xyz), ptr(st.kp), ptr(st.edges), n, k,
            st.chain.array, st.chain.n, inp["sorted"], ptr(out), ld, arr, ld,
            sp), "pgnn_point_set_pooling_rows_fwd")
    else:
        f = torch.empty((n, 16), dtype=torch.float32, device=dev)
        _lib.check(lib.pgnn_pool_features_fwd(
            ptr(st.feat), 1, ptr(st.xyz), ptr(st.kp), ptr(st.edges), n, ptr(f),
            sp), "pgnn_pool_features_fwd")
        _lib.check(lib.pgnn_mlp_fwd(ptr(f), 16, 4, None, 0, 0, n,
                                    st.chain.array, st.chain.n, None, 0,
                                    ptr(rows), ld, sp), "pgnn_mlp_fwd")
    return rows.cpu().numpy()


@pytest.mark.parametrize("path", ["ws", "general"])
@pytest.mark.parametrize("kind", ["edge", "pool"])
def test_real_sums_within_the_summation_bound(dev, kind, path):
    """graph_small, Gaussian weights: |fused - float64 sum of the device's own
    rows| <= deg 2^-24 A per element (mean: / deg + 2^-22 |S / deg|) -- the
    rows are bit-identical by construction, only the order of the additions
    differs."""
    inp = wc.edge_input("graph_small", 300) if kind == "edge" else \
        wc.pool_input("graph_small", "car")
    st = Stage(dev, kind, inp)
    dst = inp["edges"][:, 1].astype(np.int64)
    with forced(WS if path == "ws" else GENERAL):
        rows = _device_rows(dev, st, path)
        for aggregation in ("sum", "mean"):
            rc, got = st.run(aggregation)
            assert rc == 0
            worst = ag.sum_bound_check(got, rows, dst, inp["k"], inp["c"],
                                       aggregation, "%s %s %s" % (
                                           kind, path, aggregation))
            print("%s %s %s: worst error / bound = %.3f" % (
                kind, path, aggregation, worst))


# ---- D: models -------------------------------------------------------------------
def _graph(fixture):
    g = wc.gold(fixture)
    k = g["kp_xyz"].shape[0]
    return (g["intensity"], [g["xyz"], g["kp_xyz"], g["kp_xyz"]],
            [g["kp_idx"], np.arange(k, dtype=np.int32).reshape(-1, 1)],
            [g["ref_edges0"], g["ref_edges1"]])


def _model(cfg, params, dev, aggregation):
    """The registry edit INTEGRATION.md documents: the model's two graph
    operators rebuilt with another aggregator."""
    from pointgnn_amd import gnn, models
    fn = {"sum": gnn.graph_scatter_sum_fn,
          "mean": gnn.graph_scatter_mean_fn}[aggregation]
    m = models.get_model(cfg["model_name"])(
        num_classes=cfg["num_classes"], box_encoding_len=7, mode="test",
        **cfg["model_kwargs"])
    m._default_layers_type['scatter_max_point_set_pooling'] = \
        gnn.PointSetPooling(aggregation_fn=fn)
    m._default_layers_type['scatter_max_graph_auto_center_net'] = \
        gnn.GraphNetAutoCenter(aggregation_fn=fn)
    m.load_state_dict(params, dev)
    m.keep_features = True
    return m


def _config(aggregation):
    from pointgnn_amd import box_encoding  # noqa: F401
    cfg = configs.get_config("car_auto_T3")
    return ag.with_iterations(cfg, 1) if aggregation == "sum" else cfg


def _close(got, ref, what, report):
    got = np.asarray(got, np.float64)
    err = float(np.abs(got - ref).max())
    scale = max(1.0, float(np.abs(ref).max()))
    report.append("%s: max|got - ref| = %.3g, max|ref| = %.3g" % (what, err,
                                                                  scale))
    assert err <= 1e-3 * scale, report[-1]


@pytest.mark.parametrize("fixture", ["graph_tiny.npz", "graph_small.npz"])
@pytest.mark.parametrize("aggregation", ["sum", "mean"])
def test_model_against_float64(dev, aggregation, fixture):
    """car_auto_T3 (one iteration for the sum: sums grow with the fan-in at
    every iteration) with both operators aggregating by sum / mean == the
    float64 NumPy evaluation, per layer and for logits and boxes, within 1e-3
    of the layer's magnitude."""
    cfg = _config(aggregation)
    params = weights.init_params(cfg, seed=7, bias_scale=0.05)
    feats, coords, kps, edges = _graph(fixture)
    m = _model(cfg, params, dev, aggregation)
    logits, boxes = m.predict(feats, coords, kps, edges, is_training=False)
    r_logits, r_boxes, r_feats = ag.model_f64(params, cfg, feats, coords, kps,
                                              edges, aggregation)
    report = []
    try:
        assert len(m.feature_list) == len(r_feats)
        for i, (f, r) in enumerate(zip(m.feature_list, r_feats)):
            _close(f.cpu().numpy()[:, :r.shape[1]], r, "layer %d" % (i + 1),
                   report)
        _close(logits, r_logits, "logits", report)
        _close(boxes, r_boxes[:, :, :boxes.shape[2]], "boxes", report)
    finally:
        print("%s %s\n  " % (aggregation, fixture) + "\n  ".join(report))


def test_vertex_stage_fusion_does_not_change_a_bit(dev):
    """fuse_vertex_stages is a launch-fusion choice, not an arithmetic one: the
    mean model on graph_tiny gives torch.equal tensors with it on and off.
    (graph_tiny's lists are below the weights-stationary threshold and grouped
    by destination: the general path adds them in row order without atomics,
    so two runs have the same bits to compare.)"""
    import torch
    cfg = _config("mean")
    params = weights.init_params(cfg, seed=7, bias_scale=0.05)
    feats, coords, kps, edges = _graph("graph_tiny.npz")
    m = _model(cfg, params, dev, "mean")
    outs = []
    for fuse in (True, False):
        m.fuse_vertex_stages = fuse
        lg, bx = m.predict(T(feats, dev), [T(c, dev) for c in coords],
                           [T(k, dev) for k in kps],
                           [T(e, dev) for e in edges], is_training=False)
        outs.append((lg.clone(), bx.clone(),
                     [f.clone() for f in m.feature_list]))
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1])
    assert len(outs[0][2]) == len(outs[1][2]) == 4
    for a, b in zip(outs[0][2], outs[1][2]):
        assert torch.equal(a, b)


def test_edge_arith_takes_the_fp32_kernel_for_a_sum(dev):
    """edge_arith 'bf16x3' on the sum model: the split-precision kernels are
    max-only, the fp32 kernel runs -- the pooling stage's aggregate is within
    bound C of the float64 sum of the device's rows under both settings, and
    every tensor downstream agrees within the model tolerance (boundary
    atomics may reorder between two runs)."""
    import torch
    from pointgnn_amd import _lib, gnn
    cfg = _config("sum")
    params = weights.init_params(cfg, seed=7, bias_scale=0.05)
    feats, coords, kps, edges = _graph("graph_small.npz")
    m = _model(cfg, params, dev, "sum")
    got = {}
    for arith in ("f32", "bf16x3"):
        m.edge_arith = arith
        gnn.AGGREGATE_TAP = tap = []
        try:
            _lib.set_tunable("b16_force", 1)
            lg, bx = m.predict(feats, coords, kps, edges, is_training=False)
        finally:
            gnn.AGGREGATE_TAP = None
            _lib.set_tunable("b16_force", 0)
        got[arith] = (lg, bx, [f.cpu().numpy() for f in m.feature_list],
                      [t.cpu().numpy() for t in tap])
    # the pooling stage sees identical inputs in both runs: bound C
    g = wc.gold("graph_small.npz")
    layers = [(w, b, 0) for w, b in
              gnn.ParamStore(params, dev).mlp("layer1/extract_vertex_features",
                                              4)]
    inp = dict(case="graph_small", k=len(kps[0]), k_cap=len(kps[0]),
               xyz=g["xyz"].astype(np.float32),
               inten=g["intensity"].astype(np.float32),
               kp_buf=kps[0].reshape(-1).astype(np.int32), layers=layers,
               edges=edges[0], buf=edges[0].astype(np.int32), n_live=len(edges[0]),
               c=300, wq=304, sorted=1)
    st = Stage(dev, "pool", inp)
    with forced(WS):
        rows = _device_rows(dev, st, "ws")
    dst = edges[0][:, 1].astype(np.int64)
    for arith in ("f32", "bf16x3"):
        ag.sum_bound_check(got[arith][3][0], rows, dst, inp["k"], 300, "sum",
                           "pooling aggregate under %s" % arith)
    report = []
    for i, (a, b) in enumerate(zip(got["f32"][2], got["bf16x3"][2])):
        _close(b, a.astype(np.float64), "layer %d, bf16x3 vs f32" % (i + 1),
               report)
    _close(got["bf16x3"][0], np.asarray(got["f32"][0], np.float64), "logits",
           report)
    _close(got["bf16x3"][1], np.asarray(got["f32"][1], np.float64), "boxes",
           report)
    print("\n  ".join(report))


def test_model_in_capacity_form(dev):
    """Graph build + mean model in capacity form (deferred counts) agree with
    the host-sized frame within the model tolerance; the tiny frame has fewer
    edges than the weights-stationary threshold, so the kernel is forced --
    and without forcing the call raises the documented NotImplementedError."""
    import torch
    from pointgnn_amd import gnn
    from pointgnn_amd.engine import InferenceEngine
    from pointgnn_amd.synthetic import synthetic_cloud
    cfg = _config("mean")
    params = weights.init_params(cfg, seed=4, bias_scale=0.05)
    eng = InferenceEngine(cfg, params, device=dev)
    fn = gnn.graph_scatter_mean_fn
    eng.model._default_layers_type['scatter_max_point_set_pooling'] = \
        gnn.PointSetPooling(aggregation_fn=fn)
    eng.model._default_layers_type['scatter_max_graph_auto_center_net'] = \
        gnn.GraphNetAutoCenter(aggregation_fn=fn)
    xyz, inten = synthetic_cloud(seed=1, preset="tiny")
    x, f = T(xyz, dev), T(inten, dev)
    with forced(WS):
        lg, bx = eng.run_frame(x, f)
        lg, bx = lg.clone(), bx.clone()
        d = eng.run_frame_deferred(x, f)
        assert d.counts is not None and d.counts._host is None
        lg2, bx2 = d.result()
    assert lg2.shape == lg.shape and bx2.shape == bx.shape
    report = []
    _close(lg2.cpu().numpy(), lg.cpu().numpy().astype(np.float64), "logits",
           report)
    _close(bx2.cpu().numpy(), bx.cpu().numpy().astype(np.float64), "boxes",
           report)
    print("\n  ".join(report))
    with pytest.raises(NotImplementedError, match="capacity form"):
        eng.run_frame_deferred(x, f)
    torch.cuda.synchronize()


# ---- E: surface ------------------------------------------------------------------
def test_unknown_aggregators_are_refused():
    from pointgnn_amd import gnn
    for cls in (gnn.GraphNetAutoCenter, gnn.PointSetPooling):
        with pytest.raises(NotImplementedError):
            cls(aggregation_fn=lambda *a: None)
        for fn in (gnn.graph_scatter_max_fn, gnn.graph_scatter_sum_fn,
                   gnn.graph_scatter_mean_fn):
            cls(aggregation_fn=fn)
    assert "graph_scatter_sum_fn" in gnn.__all__
    assert "graph_scatter_mean_fn" in gnn.__all__


@pytest.mark.parametrize("kind,c", LEGS, ids=["edge300", "edge256", "pool"])
def test_abi_codes_and_max_delegation(dev, kind, c):
    """aggregation = 3 is PGNN_E_INVALID; PGNN_AGG_MAX through the new entry
    is torch.equal to the old entry on `fanins`."""
    import torch
    from pointgnn_amd import _lib
    st, _, _ = exact_stage(dev, kind, c, "fanins")
    inp = st.inp
    out = torch.zeros((inp["k_cap"], inp["wq"]), dtype=torch.float32,
                      device=dev)
    new = getattr(st.lib, st.names() + "_fwd")
    old = st.lib.pgnn_edge_mlp_scatter_max_fwd if kind == "edge" else \
        st.lib.pgnn_point_set_pooling_fwd
    assert new(*st.head(out), 3, None, 0, _lib.stream_ptr()) == _lib.E_INVALID
    nbytes = ctypes.c_size_t(5)
    assert getattr(st.lib, st.names() + "_workspace_bytes")(
        st.chain.array, st.chain.n, c if kind == "edge" else 1,
        len(inp["buf"]), 0, inp["k_cap"], 3, 0, _lib.stream_ptr(),
        ctypes.byref(nbytes)) == _lib.E_INVALID
    for bits in (WS, GENERAL):
        with forced(bits):
            a = torch.zeros_like(out)
            b = torch.ones_like(out)
            _lib.check(new(*st.head(a), 0, None, 0, _lib.stream_ptr()), "new")
            _lib.check(old(*st.head(b), _lib.stream_ptr()), "old")
            assert torch.equal(a, b)
