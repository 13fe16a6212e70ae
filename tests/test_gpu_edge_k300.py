"""The scaled edge kernel without the MFMA step of K = 300's padding
(csrc/edge_ws.h, K300; PGNN_EDGE_K300_ORDER): columns 288..303 of P', Q' and
rows 288..303 of the weight image come in the order of pgnn_k300_source, in
which the padding is the last K group's whole fourth step.

Every comparison is np.array_equal with the EXISTING scaled entry on the
operands in natural order, both forced onto the weights-stationary kernel at
these small sizes (`mlp_debug` 4096): the real products keep their place in
every fmaf chain and a dropped product is fma(0, 0, acc), so there is no
tolerance to choose.  The inputs are drawn in [-0.5, 0.5] (what the guard
admits)."""
import ctypes

import numpy as np
import pytest

import pointgnn_amd  # noqa: F401
import _ws_cases as wc

pytestmark = pytest.mark.gpu
WS = 4096                 # mlp_debug: the weights-stationary edge kernel, forced
K_VERT = 40
COUNTS = (5, 16, 17, 700)
LAST = slice(288, 300)    # the real features of the last K group
PAD_K300 = [291, 295, 299, 303]
# twelve odd primes: no value of the last group is a power of two times another
PRIMES = np.array([3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41], np.float32)


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from pointgnn_amd import _lib
    _lib.load()
    return torch.device("cuda")


def fan_ins(rng, total):
    """Fan-ins between 1 and 60 for K_VERT vertices that add up to `total`:
    segment ends inside tiles, at tile edges, runs that cross waves' ranges."""
    deg = np.concatenate([[1, 15, 16, 17, 60, 1, 2, 60],
                          rng.integers(1, 61, K_VERT - 8)])
    while deg.sum() > total:
        deg[8 + np.argmax(deg[8:])] -= 1
    while deg.sum() < total:
        deg[8 + np.argmin(deg[8:])] += 1
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
    # capacity form: 500 live rows of a 1000-row buffer, the tail garbage
    tail = rng.integers(-5, 3 * K_VERT, (300, 2)).astype(np.int32)
    tail[::7] = [[2 ** 30, -2 ** 30]]
    out["capacity"] = (np.concatenate([full[:500], full[500:], tail]), 500,
                       K_VERT - 6)
    return out


class Stage(object):
    """One layer width: the weights, their two images, P', Q' in natural order
    and the edge lists."""

    def __init__(self, dev, c, seed=9):
        import torch
        from pointgnn_amd import _lib, gnn
        self.dev, self.c = dev, c
        self.lib = _lib.load()
        rng = np.random.default_rng(seed + c)
        self.wq = 16 * ((c + 15) // 16)
        self.w = (rng.standard_normal((c, c)) / np.sqrt(c)).astype(np.float32)
        self.b = (0.1 * rng.standard_normal(c)).astype(np.float32)
        store = gnn.ParamStore({}, device=dev)
        self.chain = gnn.Chain(store, [(self.w, self.b, 0)])
        self.chain_k = gnn.Chain(store, [(self.w, self.b, 0)], k300=True) \
            if c == 300 else self.chain
        self.src = gnn.edge_k300_order(self.wq)
        self.ps = np.zeros((K_VERT, self.wq), np.float32)
        self.qs = np.zeros((K_VERT, self.wq), np.float32)
        self.ps[:, :c] = rng.uniform(-0.5, 0.5, (K_VERT, c))
        self.qs[:, :c] = rng.uniform(-0.5, 0.5, (K_VERT, c))
        self.lists = edge_lists(rng)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)

    def T(self, a):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def run(self, name, k_exp, k300, ps=None, qs=None, check=True):
        """-> (out [vertices, c], status, rc) of the scaled entry: on (P', Q')
        and the natural image, or (k300) on their permuted columns, the
        permuted image and the flag."""
        import torch
        from pointgnn_amd import _lib
        lib, ptr = self.lib, _lib.ptr
        edges, n_live, nv = self.lists[name]
        ps = self.ps if ps is None else ps
        qs = self.qs if qs is None else qs
        assert not ps[:, self.c:].any() and not qs[:, self.c:].any()
        if k300:
            ps, qs = ps[:, self.src], qs[:, self.src]
            if self.c == 300:     # the padding: element 3 of every lane group
                assert not ps[:, PAD_K300].any() and not qs[:, PAD_K300].any()
        p, q, e = self.T(ps), self.T(qs), self.T(edges)
        d = edges[:n_live, 1]
        flag = int(bool(np.all(d[1:] >= d[:-1])))
        if k300:
            flag |= _lib.EDGE_K300_ORDER
        out = torch.full((K_VERT, self.wq), 777.0, dtype=torch.float32,
                         device=self.dev)
        ne = nk = None
        if name == "capacity":
            i32 = lambda v: torch.tensor([v], dtype=torch.int32,
                                         device=self.dev)
            ne = _lib.DeviceCount(i32(n_live), n_live)
            nk = _lib.DeviceCount(i32(nv), nv)
        chain = self.chain_k if k300 else self.chain
        st = _lib.stream_ptr()
        self.status.zero_()
        try:
            _lib.set_tunable("mlp_debug", WS)
            applies = ctypes.c_int32(-1)
            _lib.check(lib.pgnn_edge_ws_applies(
                chain.array, 1, self.c, len(edges), st,
                ctypes.byref(applies)), "pgnn_edge_ws_applies")
            assert applies.value == 1
            rc = lib.pgnn_edge_mlp_scatter_max_scaled_fwd(
                ptr(p), ptr(q), self.wq, self.c, ptr(e), len(edges), K_VERT,
                chain.array, 1, flag, ptr(out), self.wq,
                ptr(_lib.sched_ws(self.dev)), k_exp, ptr(self.status),
                ne.arg() if ne else None, nk.arg() if nk else None, st)
        finally:
            _lib.set_tunable("mlp_debug", 0)
        if check:
            _lib.check(rc, "scaled edge stage (k300 = %r)" % k300)
        got = out.cpu().numpy()
        return got[:nv, :self.c], int(self.status.item()), rc, got


_STAGES = {}


def stage_of(dev, c):
    if c not in _STAGES:
        _STAGES[c] = Stage(dev, c)
    return _STAGES[c]


def same(s, name, k_exp, ps=None, qs=None):
    want, st0 = s.run(name, k_exp, False, ps, qs)[:2]
    got, st1 = s.run(name, k_exp, True, ps, qs)[:2]
    assert st0 == 0 and st1 == 0, (name, k_exp)
    assert np.array_equal(got, want), (name, k_exp, int((got != want).sum()))
    return got


def test_same_bits_as_the_scaled_entry(dev):
    """E in {5, 16, 17, 700} sorted by dst, an unsorted list, one with empty
    segments, a capacity-form call with a garbage tail; k in {0, 5}."""
    s = stage_of(dev, 300)
    for name in s.lists:
        edges, n_live, nv = s.lists[name]
        fed = np.zeros(nv, bool)
        d = edges[:n_live, 1]
        fed[d[(d >= 0) & (d < nv)]] = True
        for k_exp in (0, 5):
            got = same(s, name, k_exp)
            assert np.all(got[~fed] == wc.LOWEST), (name, k_exp)
            assert np.all(got[fed] != wc.LOWEST) and np.all(got[fed] != 777.0)
        if name == "empty_segments":
            assert (~fed).sum() >= K_VERT // 2 - 1
        if name == "unsorted":
            assert not np.all(d[1:] >= d[:-1])


def last_group_values(s):
    """P', Q' whose features 288..299 are odd primes times odd row factors
    (over a power of two, inside [-0.5, 0.5]): distinct, and none a power of
    two times another, so no two features can change places unnoticed."""
    ps, qs = s.ps.copy(), s.qs.copy()
    rows = (2 * np.arange(K_VERT, dtype=np.float32) + 1)[:, None]
    ps[:, LAST] = PRIMES[None, :] * rows * np.float32(2.0 ** -13)
    qs[:, LAST] = PRIMES[None, ::-1] * rows[::-1] * np.float32(2.0 ** -14)
    assert np.abs(ps).max() <= 0.5 and np.abs(qs).max() <= 0.5
    assert len(np.unique(ps[3, LAST])) == 12
    return ps, qs


def test_last_group_alone(dev):
    """P', Q' non-zero ONLY in features 288..299: a wrong permutation or a
    wrongly skipped step changes the result -- which does depend on the
    features of every one of the group's three real steps."""
    s = stage_of(dev, 300)
    ps, qs = last_group_values(s)
    ps[:, :288], qs[:, :288] = 0, 0
    got = same(s, "e700", 0, ps, qs)
    for step in range(3):     # features 288 + 4g + step in the natural layout
        p2 = ps.copy()
        p2[:, [288 + step, 292 + step, 296 + step]] = 0
        less = s.run("e700", 0, True, p2, qs)[0]
        assert not np.array_equal(less, got), step
    same(s, "unsorted", 3, ps, qs)


def test_last_group_among_random_features(dev):
    s = stage_of(dev, 300)
    ps, qs = last_group_values(s)
    for name, k_exp in (("e700", 0), ("e17", 2), ("capacity", 5)):
        same(s, name, k_exp, ps, qs)


def test_zero_and_negative_differences_in_the_last_group(dev):
    """Rows whose last group is equal in P' and Q' (differences exactly 0),
    rows with P' < Q' there (the clamp's zeros), rows at difference 1."""
    s = stage_of(dev, 300)
    ps, qs = last_group_values(s)
    qs[10:20, LAST] = ps[10, LAST]
    ps[10:20, LAST] = ps[10, LAST]
    ps[20:30, LAST] = -np.abs(ps[20:30, LAST])
    qs[20:30, LAST] = np.abs(qs[20:30, LAST]) + np.float32(2.0 ** -20)
    ps[30:40, LAST], qs[30:40, LAST] = 0.5, -0.5
    edges = s.lists["e700"][0]
    assert len({(a // 10, b // 10) for a, b in edges}) == 16
    for k_exp in (0, 5):
        same(s, "e700", k_exp, ps, qs)


def test_guard(dev):
    """|v| > 0.5 and a NaN, in the permuted columns too, raise bit 0; a value
    over the bound at or above *num_vertices does not."""
    s = stage_of(dev, 300)
    over = np.float32(0.5) + np.float32(2.0 ** -24)
    nv = s.lists["capacity"][2]
    for what, row, col, value, want in (
            ("P over, live row, last group", nv - 1, 299, over, 1),
            ("Q over, live row", 0, 0, -over, 1),
            ("Q over, last group", 5, 288, over, 1),
            ("over, row at the count", nv, 290, over, 0),
            ("NaN in the last group", 7, 294, np.float32(np.nan), 1)):
        ps, qs = s.ps.copy(), s.qs.copy()
        (qs if what.startswith("Q") else ps)[row, col] = value
        assert s.run("capacity", 1, True, ps, qs)[1] == want, what
    ps = s.ps.copy()
    ps[K_VERT - 1, 297] = over             # host-sized call: every row counts
    assert s.run("e700", 1, True, ps)[1] == 1
    assert s.run("e700", 1, True)[1] == 0


def test_c256_declines(dev):
    """C = 256 has no padding: with the flag the entry declines and writes
    nothing; without it the result is what it was."""
    from pointgnn_amd import _lib
    s = stage_of(dev, 256)
    want = s.run("e700", 5, False)[0]
    _, status, rc, raw = s.run("e700", 5, True, check=False)
    assert rc == _lib.E_UNSUPPORTED and status == 0
    assert np.all(raw == 777.0)
    assert np.array_equal(s.run("e700", 5, False)[0], want)
    # ... and a 300-wide layer asked for with another width
    s3 = stage_of(dev, 300)
    ps, qs = s3.ps.copy(), s3.qs.copy()
    ps[:, 299], qs[:, 299] = 0, 0
    s3.c = 299
    try:
        _, _, rc, raw = s3.run("e700", 5, True, ps, qs, check=False)
    finally:
        s3.c = 300
    assert rc == _lib.E_UNSUPPORTED and np.all(raw == 777.0)


def test_producer_writes_permuted_columns_and_zero_padding(dev):
    """pgnn_vertex_pre_edge_fwd from the column-permuted images of w1, b1, wx:
    P', Q' are the natural ones with their columns permuted, bit for bit, and
    the padding columns (natural 300..303, permuted 291, 295, 299, 303) are
    zero."""
    import torch
    from pointgnn_amd import _lib, gnn
    lib = _lib.load()
    rng = np.random.default_rng(77)
    c, k = 300, 37
    w1 = (rng.standard_normal((c + 3, 300)) / 16).astype(np.float32)
    b1 = (0.1 * rng.standard_normal(300)).astype(np.float32)
    h = torch.from_numpy(rng.standard_normal((k, 304)).astype(np.float32))
    h[:, 300:] = 0
    h = h.to(dev)
    x = torch.from_numpy(rng.standard_normal((k, 3)).astype(np.float32)).to(dev)
    store = gnn.ParamStore({}, device=dev)
    s = np.float32(2.0 ** -3)
    out = {}
    for name, (w, b) in (("natural", (w1, b1)),
                         ("k300", (gnn.edge_k300_columns(w1),
                                   gnn.edge_k300_columns(b1)))):
        chain = gnn.Chain(store, [(w * s, b * s, w.shape[1])])
        wx = np.zeros((3, 304), np.float32)
        wx[:, :w.shape[1]] = w[c:c + 3] * s
        wx_dev = torch.from_numpy(wx).to(dev)
        p = torch.full((k, 304), 9.0, device=dev)
        q = torch.full((k, 304), 9.0, device=dev)
        _lib.check(lib.pgnn_vertex_pre_edge_fwd(
            _lib.ptr(h), 304, c, _lib.ptr(x), None, 0, chain.array,
            _lib.ptr(wx_dev), k, _lib.ptr(p), _lib.ptr(q), 304, None, 0,
            _lib.stream_ptr()), "pgnn_vertex_pre_edge_fwd")
        out[name] = (p.cpu().numpy(), q.cpu().numpy())
    src = gnn.edge_k300_order()
    for nat, per in zip(out["natural"], out["k300"]):
        assert not nat[:, 300:].any() and nat[:, :300].all()
        assert not per[:, PAD_K300].any()
        assert per.tobytes() == nat[:, src].tobytes()


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


def k300_images(eng):
    """Cache keys of the scaled images built in the K = 300 order."""
    return [k for k in eng.model._store._cache
            if k[0] == 'edge_scaled' and k[-1] is True]


def test_engine_same_bytes_k300_scaled_and_plain(dev):
    """Four small frames through run_frames_on_streams, one and two frames per
    pass: the K = 300 order against the scaled stage without it and against
    the plain stage, logits and box encodings byte for byte."""
    from pointgnn_amd import _lib, configs, weights
    from pointgnn_amd.engine import InferenceEngine
    cfg = configs.car_auto_config(2)
    params = weights.init_params(cfg, seed=4, bias_scale=0.05)
    frames = small_frames(dev)
    try:
        _lib.set_tunable("mlp_debug", WS)
        plain = InferenceEngine(cfg, params, device=dev)
        plain.model.edge_scaled = False
        scaled = InferenceEngine(cfg, params, device=dev)
        scaled.model.edge_k300 = False
        new = InferenceEngine(cfg, params, device=dev)
        new.model.edge_k300 = True
        for per_pass in (1, 2):
            want = plain.run_frames_on_streams(frames, 2,
                                               frames_per_pass=per_pass)
            same_bytes(want, scaled.run_frames_on_streams(
                frames, 2, frames_per_pass=per_pass))
            same_bytes(want, new.run_frames_on_streams(
                frames, 2, frames_per_pass=per_pass))
    finally:
        _lib.set_tunable("mlp_debug", 0)
    assert len(k300_images(new)) == 2 and not k300_images(scaled) and \
        not k300_images(plain)
    assert len(new.model.edge_scale_exps()) == 2
    assert new.edge_scale_reruns == 0 and scaled.edge_scale_reruns == 0


def test_engine_reruns_a_batch_whose_guard_tripped(dev):
    """Every layer's k forced 6 too small: the guard of the K = 300 kernel
    trips, the batch is rerun with the plain kernel on natural operands and
    matches the plain path."""
    from pointgnn_amd import _lib, configs, weights
    from pointgnn_amd.engine import InferenceEngine
    cfg = configs.car_auto_config(1)
    params = weights.init_params(cfg, seed=4, bias_scale=0.05)
    name = "layer1/combined_features/fully_connected_1/biases"
    params[name] = params[name] + np.float32(1000.0)
    frames = small_frames(dev)
    try:
        _lib.set_tunable("mlp_debug", WS)
        off = InferenceEngine(cfg, params, device=dev)
        off.model.edge_scaled = False
        want = off.run_frames_on_streams(frames, 2)
        eng = InferenceEngine(cfg, params, device=dev)
        eng.model.edge_k300 = True
        same_bytes(want, eng.run_frames_on_streams(frames, 2))
        exps = eng.model.edge_scale_exps()
        assert eng.edge_scale_reruns == 0 and len(exps) == 1
        assert len(k300_images(eng)) == 1
        for scope, k in exps.items():
            eng.model.edge.exps[scope] = k - 6
        same_bytes(want, eng.run_frames_on_streams(frames, 2))
        assert eng.edge_scale_reruns == 1 and eng.model.edge_k300
        assert eng.model.edge_scale_exps() == {s: k - 4
                                               for s, k in exps.items()}
    finally:
        _lib.set_tunable("mlp_debug", 0)
