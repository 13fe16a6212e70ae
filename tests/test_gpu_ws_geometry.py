"""The weights-stationary kernels at every grid geometry they can run at.

csrc/edge_ws.h, edge_ws_split.h, pool_ws.h, pool_ws_f16.h and pool_split.h are
persistent kernels: which wave computes which 16-row tile for which column
group is integer arithmetic on the host (launch_edge_ws, ws_partition,
ws_balance, launch_pool_ws, launch_pool_split in csrc/gnn.hip) and on the
device (ws_group, ws_share, ws_who_balanced, ws_pool_size, ws_pool_claim, the
`span * wi / nw` ranges).  Its inputs are the stream's CU count, `ws_reserve`,
`ws_xcds`, `ws_balance`, `ws_pool_pct`, `ws_chunk` and the edge count.  The
other test files run these kernels on the whole chip with 8 row slices only;
the frame pipeline (CU-masked streams, `ws_reserve`) runs them elsewhere.  A
skipped tile only shows when no other edge of its segment dominates it, and a
tile computed twice shows in no output at all.

Geometries (tests/_ws_cases.py, sweep()): CU-masked streams of 248 .. 64 CUs
and one of 252 (not a multiple of 8: the edge kernels decline, the pooling
kernel, whose grid is the CU count itself, runs), `ws_reserve` on the plain,
the 240-CU (29 workgroups per slice) and the 72-CU stream (ignored there),
1 .. 64 row slices including counts the CUs do not divide into, the three
balance modes, four tile-pool settings -- one factor at a time, the partitions
with fewer workgroups per slice than column groups, and a seeded sample of 24
of the full product.  The test id spells the geometry.

Legs: the fp32 edge stage (C = 300, 256), car pooling, ped pooling (two
launches through a workspace), the bf16x3 / f16x2 edge stages (C = 300, 256)
and f16x2 pooling, each forced below its size threshold (`mlp_debug` 4096 /
16384, `b16_force`), on seven inputs: fan-ins 1..300, the same shuffled, a
ragged count, five edges (most slices and groups get nothing), 70001 edges to
one vertex (every wave and pool chunk flushes one row atomically), the
reference's own lists of graph_small.npz, and a capacity-form call (count on
the device, tail rows poisoned).  The training forward forms are in
tests/test_gpu_train_fullsize.py.

Bars (none new): at the default geometry every output is held to a float64
evaluation -- fp32: atol 2e-4, rtol 1e-4; split forms: no further from float64
than 1.25x (layer) / 1.5x (pooling) the fp32 kernel's distance + 1e-7 scale,
and within 2e-6 scale of the fp32 kernel.  At every other geometry the output
is np.array_equal to that one (fp32: to the LDS-tile kernel's, `mlp_debug`
2048 / 8192): the partition changes who computes a tile, never the MFMA update
sequence of an element, and max is exact.  The stream's tile-pool counters sum
to 0 and the f16x2 status word is 0 after every launch.

That the kernel under test ran, not a fallback: the split entries return 0 or
PGNN_E_UNSUPPORTED (without touching the error message), predicted by
_ws_cases.runs(); the fp32 kernels write the stamp buffer of
pgnn_set_debug_buffer, and from the stamps' static range lengths
(_ws_cases.check_edge_stamps / check_pool_stamps) every (row tile, column
group) is shown to have exactly one owner.  The split kernels write no stamps
(their instruction stream is frozen): for them the output equality and the
return code stand alone.

Not covered: pgnn_point_set_pooling_workspace_bytes sizes the split form's
workspace with the DEVICE's CU count while the launch plans with the stream's;
that only moves a threshold between two bit-identical kernels, and this file
always passes a full workspace."""
import numpy as np
import pytest

import pointgnn_amd  # noqa: F401
import _ws_cases as wc

pytestmark = pytest.mark.gpu
FP_TOL = 2e-4

LEGS = [("edge_f32", 300), ("edge_f32", 256), ("pool_car", 300),
        ("pool_ped", 512), ("edge_bf16x3", 300), ("edge_bf16x3", 256),
        ("edge_f16x2", 300), ("edge_f16x2", 256), ("pool_f16x2", 300)]
WS, TILE = 4096 | 16384, 2048 | 8192     # mlp_debug: forced / LDS-tile kernels
SENTINEL = b"unknown tunable"


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from pointgnn_amd import _lib
    _lib.load()
    d = torch.device("cuda")
    assert torch.cuda.get_device_properties(d).multi_processor_count == 256, \
        "the geometry list is written for the MI355X's 256 CUs"
    return d


class Case(object):
    """One leg on one input: device buffers made once, launched many times."""

    def __init__(self, dev, leg, width, name):
        import torch
        from pointgnn_amd import _lib, gnn
        self.dev, self.leg, self.width, self.name = dev, leg, width, name
        self.lib = lib = _lib.load()
        self.fp32 = leg in ("edge_f32", "pool_car", "pool_ped")
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        store = gnn.ParamStore({}, device=dev)
        if leg.startswith("edge"):
            inp = wc.edge_input(name, width)
            self.p, self.q = T(inp["p"]), T(inp["q"])
            if leg == "edge_f32":
                self.chain = gnn.Chain(store, [(inp["w"], inp["b"], 0)])
            else:
                arith = leg[len("edge_"):]
                host = np.empty(getattr(lib, "pgnn_packed_fc_%s_bytes" % arith)(
                    width, width), np.uint8)
                _lib.check(getattr(lib, "pgnn_pack_fc_%s" % arith)(
                    inp["w"].ctypes.data, inp["b"].ctypes.data, width, width,
                    host.ctypes.data))
                self.image = T(host)
        else:
            inp = wc.pool_input(name, "ped" if leg == "pool_ped" else "car")
            self.feat, self.xyz = T(inp["inten"]), T(inp["xyz"])
            self.kp = T(inp["kp_buf"])
            self.chain = gnn.Chain(store, inp["layers"])
            if leg == "pool_ped":
                self.work = torch.empty(len(inp["buf"]) * 256,
                                        dtype=torch.float32, device=dev)
            if leg == "pool_f16x2":
                def image(i, k_in, n_out):
                    w, b = inp["layers"][i][:2]
                    host = np.empty(lib.pgnn_packed_fc_f16x2_bytes(k_in, n_out),
                                    np.uint8)
                    _lib.check(lib.pgnn_pack_fc_f16x2_acc(
                        w.ctypes.data, b.ctypes.data, k_in, n_out,
                        host.ctypes.data))
                    return T(host)
                self.image, self.hidden = image(3, 128, 300), image(2, 64, 128)
        self.inp = inp
        self.edges = T(inp["buf"])
        self.out = torch.empty((inp["k_cap"], inp["wq"]), dtype=torch.float32,
                               device=dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.ne = self.nk = None
        if name == "capacity":
            i32 = lambda v: torch.tensor([v], dtype=torch.int32, device=dev)
            self.ne = _lib.DeviceCount(i32(inp["n_live"]), inp["n_live"])
            self.nk = _lib.DeviceCount(i32(inp["k"]), inp["k"])
        self.n_wt = (inp["n_live"] + 15) // 16
        torch.cuda.synchronize()

    def launch(self):
        """The leg's entry on the current stream; returns its code."""
        from pointgnn_amd import _lib
        lib, inp, ptr = self.lib, self.inp, _lib.ptr
        n, k, ld, flag = len(inp["buf"]), inp["k_cap"], inp["wq"], inp["sorted"]
        ne = self.ne.arg() if self.ne else None
        nk = self.nk.arg() if self.nk else None
        sched, st = ptr(_lib.sched_ws(self.dev)), _lib.stream_ptr()
        if self.leg == "edge_f32":
            head = (ptr(self.p), ptr(self.q), ld, self.width, ptr(self.edges), n,
                    k, self.chain.array, 1, flag, ptr(self.out), ld, sched)
            if ne:
                return lib.pgnn_edge_mlp_scatter_max_fwd_dyn(*head, ne, nk, st)
            return lib.pgnn_edge_mlp_scatter_max_fwd(*head, st)
        if self.leg.startswith("edge"):
            head = (ptr(self.p), ptr(self.q), ld, self.width, ptr(self.edges), n,
                    k, ptr(self.image), self.width, 0, flag, ptr(self.out), ld)
            if self.leg == "edge_bf16x3":
                return lib.pgnn_edge_mlp_scatter_max_bf16x3_fwd(*head, ne, nk, st)
            return lib.pgnn_edge_mlp_scatter_max_f16x2_fwd(
                *head, ptr(self.status), ne, nk, st)
        head = (ptr(self.feat), 1, ptr(self.xyz), ptr(self.kp), ptr(self.edges),
                n, k, self.chain.array, self.chain.n)
        tail = (flag, ptr(self.out), ld, sched)
        if self.leg == "pool_car":
            if ne:
                return lib.pgnn_point_set_pooling_fwd_dyn(*head, *tail, ne, nk, st)
            return lib.pgnn_point_set_pooling_fwd(*head, *tail, st)
        if self.leg == "pool_ped":
            # a hidden row the first launch skipped would win every maximum
            self.work.fill_(3e38)
            return lib.pgnn_point_set_pooling_fwd_ws(
                *head, *tail, ne, nk, ptr(self.work), self.work.numel() * 4, st)
        return lib.pgnn_point_set_pooling_f16x2_fwd(
            *head, ptr(self.image), ptr(self.hidden), *tail, ptr(self.status),
            ne, nk, st)

    def run(self, stamps=None):
        """Launch on the current stream -> (code, out [k, c], stamps read back
        [waves, stride] or None).  The error message is set to a sentinel
        first; the scheduling counters and the status word are checked."""
        from pointgnn_amd import _lib
        lib = self.lib
        assert lib.pgnn_set_tunable(b"no such tunable", 0) == _lib.E_INVALID
        assert lib.pgnn_last_error() == SENTINEL
        self.status.zero_()
        if stamps is not None:
            stamps.zero_()
            lib.pgnn_set_debug_buffer(_lib.ptr(stamps))
        try:
            rc = self.launch()
        finally:
            lib.pgnn_set_debug_buffer(None)
        if self.fp32 or rc != _lib.E_UNSUPPORTED:
            _lib.check(rc, "%s %d on %s" % (self.leg, self.width, self.name))
        else:
            if lib.pgnn_last_error() != SENTINEL:
                raise AssertionError("a declining split-precision entry set an "
                                     "error message: %r" % lib.pgnn_last_error())
        out = self.out.cpu().numpy()[:self.inp["k"], :self.inp["c"]]
        assert int(_lib.sched_ws(self.dev).abs().sum().item()) == 0, \
            "tile-pool counters not handed back zeroed"
        assert int(self.status.item()) == 0, "f16x2 range flag raised"
        st = None
        if stamps is not None:
            st = stamps.cpu().numpy().reshape(-1, wc.STAMP_STRIDE)
        return rc, out, st


_CASES, _BASE, _STAMPS, _REF = {}, {}, {}, {}


def case_of(dev, leg, width, name):
    key = (leg, width, name)
    if key not in _CASES:
        _CASES[key] = Case(dev, leg, width, name)
    return _CASES[key]


def stamp_buffer(dev):
    """Large enough for the stamps of any kernel that reads the debug buffer
    on 256 CUs (the LDS-tile kernels use 256 words per workgroup)."""
    import torch
    if "buf" not in _STAMPS:
        _STAMPS["buf"] = torch.zeros(256 * 8 * 256, dtype=torch.int64,
                                     device=dev)
    return _STAMPS["buf"]


def baseline(dev, leg, width, name):
    """The output every geometry must reproduce: on the plain stream with the
    default tunables, the LDS-tile kernel's (fp32 legs) or the kernel's own
    (split-precision legs)."""
    from pointgnn_amd import _lib
    key = (leg, width, name)
    if key not in _BASE:
        c = case_of(dev, leg, width, name)
        try:
            _lib.set_tunable("mlp_debug", TILE if c.fp32 else WS)
            _lib.set_tunable("b16_force", 1)
            rc, out, _ = c.run()
        finally:
            _lib.set_tunable("mlp_debug", 0)
            _lib.set_tunable("b16_force", 0)
        assert rc == 0
        _BASE[key] = out.copy()
    return _BASE[key]


def run_ws(dev, c, g):
    """Case `c` with the weights-stationary kernel forced, at geometry `g` (the
    tunables and the stream are the caller's); checks the proof that it ran or
    declined as predicted and the stamp accounting; returns the output (None
    from a split-precision entry that declined)."""
    from pointgnn_amd import _lib
    expect = wc.runs(c.leg, c.width, g)
    cus, xcds = wc.effective(g)
    what = "%s %d on %s at %s" % (c.leg, c.width, c.name, wc.geo_id(g))
    stamps = None
    if c.fp32 and expect:
        grid = cus if c.leg == "pool_car" else cus // xcds * xcds
        stamps = stamp_buffer(dev)[:(grid * wc.WAVES + 8) * wc.STAMP_STRIDE]
    try:
        _lib.set_tunable("mlp_debug", WS)
        _lib.set_tunable("b16_force", 1)
        rc, out, st = c.run(stamps)
    finally:
        _lib.set_tunable("mlp_debug", 0)
        _lib.set_tunable("b16_force", 0)
    if not c.fp32:
        assert rc == (0 if expect else _lib.E_UNSUPPORTED), \
            "%s: code %d, the table says it %s" % (
                what, rc, "runs" if expect else "declines")
        if rc:
            return None     # declined: nothing was written
    if st is not None:
        pooled = g.pool > 0 and xcds <= wc.MAX_SLICES
        try:
            if c.leg == "pool_car":
                wc.check_pool_stamps(st, c.n_wt, cus, account=g.pool == 0)
            else:
                wc.check_edge_stamps(
                    st, c.n_wt, cus, xcds,
                    wc.grouping(*wc.SHAPES[(c.leg, c.width)]),
                    balanced=g.balance == 2 and not pooled and
                    xcds <= wc.MAX_SLICES,
                    account=not pooled)
        except AssertionError as err:
            raise AssertionError("%s: %s" % (what, err))
    return out


@pytest.mark.parametrize("leg,width", LEGS,
                         ids=["%s-%d" % lw for lw in LEGS])
def test_default_geometry_against_float64(dev, leg, width):
    """Whole chip, 8 slices: the forced weights-stationary kernel against a
    float64 evaluation on every input (and, fp32, bit for bit against the
    LDS-tile kernel); the distances are printed."""
    import torch
    torch.cuda.synchronize()
    for name in wc.INPUTS:
        c = case_of(dev, leg, width, name)
        base = baseline(dev, leg, width, name)
        with wc.tunables(wc.DEFAULT):
            out = run_ws(dev, c, wc.DEFAULT)
        assert np.array_equal(out, base, equal_nan=True), (leg, width, name)
        rkey = (leg.startswith("edge"), leg == "pool_ped", width, name)
        if rkey not in _REF:    # (the arithmetics of a stage share their inputs)
            with np.errstate(all="ignore"):
                _REF[rkey] = wc.edge_f64(c.inp) if leg.startswith("edge") \
                    else wc.pool_f64(c.inp)
        ref = _REF[rkey]
        fed = ref[:, 0] != wc.LOWEST
        assert np.array_equal(out == wc.LOWEST, ref == wc.LOWEST), name
        scale = np.abs(ref[fed]).max()
        err = np.abs(out[fed] - ref[fed]).max()
        if c.fp32:
            print("%s %d %-11s E %6d: |out|max %.3g, max error vs float64 "
                  "%.3g" % (leg, width, name, c.inp["n_live"], scale, err))
            np.testing.assert_allclose(out[fed], ref[fed], atol=FP_TOL,
                                       rtol=1e-4)
            continue
        f32 = baseline(dev, "edge_f32" if leg.startswith("edge") else
                       "pool_car", width, name)
        e32 = np.abs(f32[fed] - ref[fed]).max()
        d = np.abs(out[fed] - f32[fed]).max()
        print("%s %d %-11s E %6d: |out|max %.3g, max error vs float64: fp32 "
              "%.3g, this %.3g; vs fp32 %.3g" % (
                  leg, width, name, c.inp["n_live"], scale, e32, err, d))
        factor = 1.25 if leg.startswith("edge") else 1.5
        assert err <= factor * e32 + 1e-7 * scale, name
        assert d <= 2e-6 * scale, name


SWEEP = wc.sweep()


@pytest.mark.parametrize("geo", SWEEP[1:], ids=[wc.geo_id(g) for g in SWEEP[1:]])
def test_every_leg_at_geometry(dev, geo):
    """Every leg on every input at one geometry: the bits of the default
    geometry, the kernel that was asked for, every tile with one owner."""
    import torch
    for leg, width in LEGS:
        for name in wc.INPUTS:
            baseline(dev, leg, width, name)      # (on the plain stream)
    torch.cuda.synchronize()
    failures = []
    with wc.masked_stream(geo.stream) as stream, wc.tunables(geo), \
            torch.cuda.stream(stream):
        for leg, width in LEGS:
            for name in wc.INPUTS:
                c = case_of(dev, leg, width, name)
                try:
                    out = run_ws(dev, c, geo)
                except (AssertionError, RuntimeError) as err:
                    failures.append("%s %d %s: %s" % (leg, width, name, err))
                    continue
                base = _BASE[(leg, width, name)]
                if out is None:
                    continue
                if not np.array_equal(out, base, equal_nan=True):
                    bad = np.argwhere(out != base)
                    failures.append(
                        "%s %d %s: %d elements differ from the default "
                        "geometry's, first at %r" % (leg, width, name, len(bad),
                                                     bad[0].tolist()))
        stream.synchronize()
    if failures:
        pytest.fail("%s (CUs, slices = %r):\n%s" % (
            wc.geo_id(geo), wc.effective(geo), "\n".join(failures)),
            pytrace=False)
