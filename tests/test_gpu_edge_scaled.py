"""The SCALED form of the weights-stationary edge kernel (csrc/edge_ws.h,
pk_sub_clamp; pgnn_edge_mlp_scatter_max_scaled_fwd): on P' = 2^-k P, Q' = 2^-k Q
the gather's packed subtraction carries the `clamp` modifier and is the ReLU,
and the kernel multiplies a closed segment's maximum by 2^k.

Every comparison is np.array_equal with the PLAIN entry
(pgnn_edge_mlp_scatter_max_fwd / _dyn) on P = P' 2^k, Q = Q' 2^k, both forced
onto the weights-stationary kernel at these small sizes (`mlp_debug` 4096, as
tests/test_gpu_ws_geometry.py does): a power-of-two scale is exact, commutes
with every rounding of the chain, with ReLU and with max, so there is no
tolerance to choose.  The inputs are drawn in [-0.5, 0.5] (what the guard
admits), the weights as in _ws_cases.edge_input; nothing here is near the
subnormal range where the argument ends.

The first test is the hardware probe the rest stands on: what
`v_pk_add_f32 ... neg_lo:[0,1] neg_hi:[0,1] clamp` makes of differences below,
inside, at the ends of and above [0, 1]."""
import ctypes

import numpy as np
import pytest

import pointgnn_amd  # noqa: F401
import _ws_cases as wc

pytestmark = pytest.mark.gpu
WS = 4096                 # mlp_debug: the weights-stationary edge kernel, forced
K_VERT = 40
EXPS = (0, 1, 5, 12)
COUNTS = (5, 16, 17, 700)


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from pointgnn_amd import _lib
    _lib.load()
    return torch.device("cuda")


def test_probe_clamped_packed_subtraction(dev):
    """Differences -2, -0, +0, 2^-140, 2^-30, 0.5, 1 - 2^-24, 1, 1 + 2^-23, 2:
    0 for the negatives, the difference itself in [0, 1], 1 above -- in the
    low and in the high half of the packed pair."""
    import torch
    from pointgnn_amd import _lib
    lib = _lib.load()
    f = np.float32
    two = lambda e: f(2.0) ** f(e)
    pairs = [(f(-1), f(1), f(0)),                               # -2
             (f(-0.0), f(0.0), f(0)),                           # -0
             (f(0.25), f(0.25), f(0)),                          # +0
             (f(3) * two(-140), two(-139), two(-140)),          # subnormal
             (two(-29), two(-30), two(-30)),
             (f(0.25), f(-0.25), f(0.5)),
             (f(0.5), -(f(0.5) - two(-24)), f(1) - two(-24)),
             (f(0.5), f(-0.5), f(1)),                           # exactly 1
             (f(0.5) + two(-23), f(-0.5), f(1)),                # 1 + 2^-23
             (f(1), f(-1), f(1))]                               # 2
    n = len(pairs)
    # pair i of the wave: (difference i, difference n - 1 - i)
    a = np.array([[pairs[i][0], pairs[n - 1 - i][0]] for i in range(n)], f)
    b = np.array([[pairs[i][1], pairs[n - 1 - i][1]] for i in range(n)], f)
    want = np.array([[pairs[i][2], pairs[n - 1 - i][2]] for i in range(n)], f)
    assert want[3, 0] == two(-140) and want[3, 0] > 0      # (a subnormal)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    out = torch.full((n, 2), -7.0, dtype=torch.float32, device=dev)
    _lib.check(lib.pgnn_debug_pk_sub_clamp(_lib.ptr(ta), _lib.ptr(tb),
                                           _lib.ptr(out), n,
                                           _lib.stream_ptr()),
               "pgnn_debug_pk_sub_clamp")
    got = out.cpu().numpy()
    for i in range(n):
        print("a - b = %-14.9g -> lo %-14.9g hi %-14.9g (want %.9g)" % (
            np.float64(a[i, 0]) - np.float64(b[i, 0]), got[i, 0],
            got[n - 1 - i, 1], want[i, 0]))
    assert np.array_equal(got, want)


# ---- inputs -------------------------------------------------------------------
def fan_ins(rng, total):
    """Fan-ins between 1 and 60 for K_VERT vertices that add up to `total`;
    the first ones put segment ends inside tiles, at tile edges (1 + 15 = 16,
    + 16 = 32) and leave long runs that cross the waves' ranges."""
    deg = np.concatenate([[1, 15, 16, 17, 60, 1, 2, 60],
                          rng.integers(1, 61, K_VERT - 8)])
    while deg.sum() > total:
        deg[8 + np.argmax(deg[8:])] -= 1
    while deg.sum() < total:
        deg[8 + np.argmin(deg[8:])] += 1
    assert deg.min() >= 1 and deg.max() <= 60 and deg.sum() == total
    return deg


def edge_lists(rng):
    """name -> (edges [E, 2], live rows, vertices that exist)"""
    deg = fan_ins(rng, 700)
    dst = np.repeat(np.arange(K_VERT), deg).astype(np.int32)
    src = rng.integers(0, K_VERT, len(dst)).astype(np.int32)
    full = np.stack([src, dst], axis=1)
    out = {"e%d" % e: (full[:e].copy(), e, K_VERT) for e in COUNTS}
    out["unsorted"] = (full[rng.permutation(700)], 700, K_VERT)
    gaps = full.copy()          # every odd vertex loses its edges to the next
    gaps[:, 1] = np.minimum(gaps[:, 1] // 2 * 2, K_VERT - 2)
    out["empty_segments"] = (gaps[np.argsort(gaps[:, 1], kind="stable")], 700,
                             K_VERT)
    # capacity form: 500 live rows of a 700 + 300 row buffer, the tail garbage
    # (ids far outside, a few plausible ones)
    tail = rng.integers(-5, 3 * K_VERT, (300, 2)).astype(np.int32)
    tail[::7] = [[2 ** 30, -2 ** 30]]
    out["capacity"] = (np.concatenate([full[:500], full[500:], tail]), 500,
                       K_VERT - 6)
    return out


class Stage(object):
    """One layer width: the weights, P', Q' and the device buffers."""

    def __init__(self, dev, c, seed=5):
        import torch
        from pointgnn_amd import _lib, gnn
        self.dev, self.c = dev, c
        self.lib = _lib.load()
        rng = np.random.default_rng(seed + c)
        self.wq = 16 * ((c + 15) // 16)
        self.w = (rng.standard_normal((c, c)) / np.sqrt(c)).astype(np.float32)
        self.b = (0.1 * rng.standard_normal(c)).astype(np.float32)
        self.chain = gnn.Chain(gnn.ParamStore({}, device=dev),
                               [(self.w, self.b, 0)])
        self.ps = np.zeros((K_VERT, self.wq), np.float32)
        self.qs = np.zeros((K_VERT, self.wq), np.float32)
        self.ps[:, :c] = rng.uniform(-0.5, 0.5, (K_VERT, c))
        self.qs[:, :c] = rng.uniform(-0.5, 0.5, (K_VERT, c))
        self.lists = edge_lists(rng)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)

    def T(self, a):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def run(self, name, k_exp, scaled, ps=None, qs=None):
        """-> (out [vertices, c], status) of the scaled entry on (P', Q') or
        of the plain entry on (P' 2^k, Q' 2^k); the kernel forced."""
        import torch
        from pointgnn_amd import _lib
        lib, ptr = self.lib, _lib.ptr
        edges, n_live, nv = self.lists[name]
        ps = self.ps if ps is None else ps
        qs = self.qs if qs is None else qs
        mul = np.float32(1.0 if scaled else 2.0 ** k_exp)
        p, q, e = self.T(ps * mul), self.T(qs * mul), self.T(edges)
        d = edges[:n_live, 1]
        flag = int(bool(np.all(d[1:] >= d[:-1])))
        out = torch.full((K_VERT, self.wq), 777.0, dtype=torch.float32,
                         device=self.dev)
        ne = nk = None
        if name == "capacity":
            i32 = lambda v: torch.tensor([v], dtype=torch.int32,
                                         device=self.dev)
            ne = _lib.DeviceCount(i32(n_live), n_live)
            nk = _lib.DeviceCount(i32(nv), nv)
        head = (ptr(p), ptr(q), self.wq, self.c, ptr(e), len(edges), K_VERT,
                self.chain.array, 1, flag, ptr(out), self.wq,
                ptr(_lib.sched_ws(self.dev)))
        st = _lib.stream_ptr()
        self.status.zero_()
        try:
            _lib.set_tunable("mlp_debug", WS)
            if scaled:
                applies = ctypes.c_int32(-1)
                _lib.check(lib.pgnn_edge_ws_applies(
                    self.chain.array, 1, self.c, len(edges), st,
                    ctypes.byref(applies)), "pgnn_edge_ws_applies")
                assert applies.value == 1
                rc = lib.pgnn_edge_mlp_scatter_max_scaled_fwd(
                    *head, k_exp, ptr(self.status),
                    ne.arg() if ne else None, nk.arg() if nk else None, st)
            elif ne:
                rc = lib.pgnn_edge_mlp_scatter_max_fwd_dyn(
                    *head, ne.arg(), nk.arg(), st)
            else:
                rc = lib.pgnn_edge_mlp_scatter_max_fwd(*head, st)
        finally:
            _lib.set_tunable("mlp_debug", 0)
        _lib.check(rc, "edge stage (%s)" % ("scaled" if scaled else "plain"))
        return out.cpu().numpy()[:nv, :self.c], int(self.status.item())


_STAGES, _PLAIN = {}, {}


def stage_of(dev, c):
    if c not in _STAGES:
        _STAGES[c] = Stage(dev, c)
    return _STAGES[c]


def plain(dev, c, name, k_exp):
    """The plain entry's output, computed once per (width, list, exponent)."""
    key = (c, name, k_exp)
    if key not in _PLAIN:
        _PLAIN[key] = stage_of(dev, c).run(name, k_exp, scaled=False)[0]
    return _PLAIN[key]


@pytest.mark.parametrize("c", [300, 256])
def test_same_bits_as_the_plain_entry(dev, c):
    """E in {5, 16, 17, 700} sorted by dst with fan-ins 1..60, an unsorted
    list, one with empty segments, a capacity-form call with a garbage tail;
    k in {0, 1, 5, 12}: every written row equal, status 0."""
    s = stage_of(dev, c)
    for name in s.lists:
        edges, n_live, nv = s.lists[name]
        fed = np.zeros(nv, bool)
        d = edges[:n_live, 1]
        fed[d[(d >= 0) & (d < nv)]] = True
        for k_exp in EXPS:
            want = plain(dev, c, name, k_exp)
            got, status = s.run(name, k_exp, scaled=True)
            assert status == 0, (name, k_exp)
            assert np.array_equal(got, want), (name, k_exp, int(
                (got != want).sum()))
            # rows without an edge stay lowest(), the others were written
            assert np.all(got[~fed] == wc.LOWEST), (name, k_exp)
            assert np.all(got[fed] != wc.LOWEST) and np.all(got[fed] != 777.0)
        if name == "empty_segments":
            assert (~fed).sum() >= K_VERT // 2 - 1
        if name == "unsorted":
            assert not np.all(d[1:] >= d[:-1])


@pytest.mark.parametrize("c", [300, 256])
def test_at_the_bound(dev, c):
    """Rows with P' = 0.5, Q' = -0.5 (difference exactly 1.0), rows with
    P' = Q', rows with P' < Q': the plain kernel's bits, status 0."""
    s = stage_of(dev, c)
    ps, qs = s.ps.copy(), s.qs.copy()
    ps[0:10, :c], qs[0:10, :c] = 0.5, -0.5
    ps[10:20] = ps[10]          # (one vector: any pair of these rows gives 0)
    qs[10:20] = ps[10]
    ps[20:30, :c] = -np.abs(ps[20:30, :c])
    qs[20:30, :c] = np.abs(qs[20:30, :c]) + np.float32(2.0 ** -20)
    edges = s.lists["e700"][0]
    # the three kinds meet on both sides of the subtraction
    assert len({(a // 10, b // 10) for a, b in edges if a < 30 and b < 30}) == 9
    for k_exp in (0, 5):
        want, _ = s.run("e700", k_exp, False, ps, qs)
        got, status = s.run("e700", k_exp, True, ps, qs)
        assert status == 0
        assert np.array_equal(got, want), (k_exp, int((got != want).sum()))


@pytest.mark.parametrize("c", [300, 256])
def test_guard(dev, c):
    """One P' of 0.5 + 2^-24 in a row below the count raises bit 0; the same
    value in a row at or above *num_vertices does not; a NaN does."""
    s = stage_of(dev, c)
    over = np.float32(0.5) + np.float32(2.0 ** -24)
    assert over > np.float32(0.5)
    nv = s.lists["capacity"][2]
    for what, row, col, value, want in (
            ("P over, live row", nv - 1, c - 1, over, 1),
            ("Q over, live row", 0, 0, -over, 1),
            ("over, row at the count", nv, 3, over, 0),
            ("over, last row of the capacity", K_VERT - 1, c - 1, over, 0),
            ("NaN", 7, 130, np.float32(np.nan), 1)):
        ps, qs = s.ps.copy(), s.qs.copy()
        (qs if what.startswith("Q") else ps)[row, col] = value
        _, status = s.run("capacity", 1, True, ps, qs)
        assert status == want, what
    ps = s.ps.copy()
    ps[K_VERT - 1, 0] = over             # host-sized call: every row counts
    assert s.run("e700", 1, True, ps)[1] == 1
    assert s.run("e700", 1, True)[1] == 0


@pytest.mark.parametrize("cus", [64, 128, 256])
def test_geometries(dev, cus):
    """CU-masked streams of 64 and 128 CUs and the whole chip, the 700-edge
    list: the bits of the plain entry on the plain stream."""
    import torch
    total = torch.cuda.get_device_properties(dev).multi_processor_count
    assert total == 256, "the geometries are written for the MI355X's 256 CUs"
    geo = wc.DEFAULT._replace(stream=cus)
    for c in (300, 256):
        want = plain(dev, c, "e700", 5)
        torch.cuda.synchronize()
        with wc.masked_stream(cus) as stream, wc.tunables(geo), \
                torch.cuda.stream(stream):
            got, status = stage_of(dev, c).run("e700", 5, scaled=True)
            stream.synchronize()
        assert status == 0
        assert np.array_equal(got, want), (c, cus)


# ---- the engine -----------------------------------------------------------------
def small_frames(dev, n=4):
    import torch
    from pointgnn_amd.synthetic import synthetic_cloud
    frames = []
    for s in range(n):
        xyz, inten = synthetic_cloud(seed=s, preset="small")
        frames.append((torch.from_numpy(xyz).to(dev),
                       torch.from_numpy(inten).to(dev)))
    return frames


def same_bytes(want, got):
    assert len(want) == len(got)
    for (l0, b0), (l1, b1) in zip(want, got):
        assert l0.shape == l1.shape and b0.shape == b1.shape
        assert l0.cpu().numpy().tobytes() == l1.cpu().numpy().tobytes()
        assert b0.contiguous().cpu().numpy().tobytes() == \
            b1.contiguous().cpu().numpy().tobytes()


def test_engine_same_bytes_scaled_and_plain(dev):
    """Four small synthetic frames through run_frames_on_streams, one and two
    frames per pass, `edge_scaled` on against off: logits and box encodings
    byte for byte; every graph layer calibrated, no rerun."""
    from pointgnn_amd import _lib, configs, weights
    from pointgnn_amd.engine import InferenceEngine
    cfg = configs.car_auto_config(2)
    params = weights.init_params(cfg, seed=4, bias_scale=0.05)
    frames = small_frames(dev)
    try:
        _lib.set_tunable("mlp_debug", WS)
        off = InferenceEngine(cfg, params, device=dev)
        off.model.edge_scaled = False
        on = InferenceEngine(cfg, params, device=dev)
        assert on.model.edge_scaled
        for per_pass in (1, 2):
            want = off.run_frames_on_streams(frames, 2,
                                             frames_per_pass=per_pass)
            got = on.run_frames_on_streams(frames, 2,
                                           frames_per_pass=per_pass)
            same_bytes(want, got)
    finally:
        _lib.set_tunable("mlp_debug", 0)
    exps = on.model.edge_scale_exps()
    print("calibrated exponents:", exps)
    assert len(exps) == 2 and all(0 <= k <= 24 for k in exps.values())
    assert on.model.edge.flags is not None      # scaled kernels ran
    assert on.edge_scale_reruns == 0
    assert off.model.edge_scale_exps() == {} and \
        off.model.edge.flags is None


def test_engine_reruns_a_batch_whose_guard_tripped(dev):
    """With every layer's k forced 6 too small the guard trips: the batch is
    rerun with the plain kernel -- the results are the off path's --, the
    rerun is counted and the tripped layers' k went up by 2."""
    from pointgnn_amd import _lib, configs, weights
    from pointgnn_amd.engine import InferenceEngine
    cfg = configs.car_auto_config(1)
    params = weights.init_params(cfg, seed=4, bias_scale=0.05)
    # activations of ~1000 in front of the graph layer: its k is well above 6
    name = "layer1/combined_features/fully_connected_1/biases"
    params[name] = params[name] + np.float32(1000.0)
    frames = small_frames(dev)
    try:
        _lib.set_tunable("mlp_debug", WS)
        off = InferenceEngine(cfg, params, device=dev)
        off.model.edge_scaled = False
        want = off.run_frames_on_streams(frames, 2)
        eng = InferenceEngine(cfg, params, device=dev)
        same_bytes(want, eng.run_frames_on_streams(frames, 2))
        exps = eng.model.edge_scale_exps()
        assert eng.edge_scale_reruns == 0 and len(exps) == 1
        assert all(k >= 6 for k in exps.values()), exps
        for scope, k in exps.items():
            eng.model.edge.exps[scope] = k - 6
        shapes = len(eng.frame_shapes)
        got = eng.run_frames_on_streams(frames, 2)
        same_bytes(want, got)
        assert eng.edge_scale_reruns == 1 and eng.model.edge_scaled
        assert len(eng.frame_shapes) == shapes + len(frames)
        assert eng.model.edge_scale_exps() == {s: k - 4
                                               for s, k in exps.items()}
    finally:
        _lib.set_tunable("mlp_debug", 0)
