"""The training primitives of csrc/train.hip one by one against the plain
references of tests/_train_primitives.py.

Exact cases: integer-valued inputs whose sums of magnitudes stay below 2^24
(asserted by the reference helpers, and for every case without a GPU by
tests/test_train_primitives_cpu.py), so fp32 adds, MFMAs and float atomics are
exact and the device must EQUAL the int64 reference -- a dropped, doubled or
misplaced row, a wrong mask or a wrong tile changes the result.

pgnn_pool_narrow_bwd_f32 on real values (test_pool_narrow_bwd_real_values, E =
20 011 Gaussian rows) is held to the running error bound of
_train_primitives.pool_chain_bounds (u = 2^-24, no other constant); the test
prints the worst error / bound per output."""
import numpy as np
import pytest

import pointgnn_amd  # noqa: F401
import _train_primitives as tp

pytestmark = pytest.mark.gpu

WS_POISON = 3e38
GUARD = 256             # floats between the outputs of one call
WGRAD_WG_TARGET = 512   # csrc/train.hip g_wgrad_wg_target


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


# ---- A / B: pgnn_pool_narrow_bwd_f32 ---------------------------------------------
def _transposed_image(dev, w):
    """pgnn_pack_fc_device(..., transpose = 1): the image of W^T, no bias."""
    import torch
    from pointgnn_amd import _lib
    lib = _lib.load()
    k_in, n_out = w.shape
    out = torch.empty(lib.pgnn_packed_fc_floats(n_out, k_in),
                      dtype=torch.float32, device=dev)
    wd = T(w, dev)
    _lib.check(lib.pgnn_pack_fc_device(_lib.ptr(wd), None, k_in, n_out, 1,
                                       _lib.ptr(out), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return out


_IMAGES = {}


def _exact_images(dev):
    if "exact" not in _IMAGES:
        w1, w2 = tp.pool_chain_weights()
        _IMAGES["exact"] = (w1, w2, _transposed_image(dev, w1),
                            _transposed_image(dev, w2))
    return _IMAGES["exact"]


_OUT_SHAPES = (("dW0", None), ("db0", (32,)), ("dW1", (32, 64)), ("db1", (64,)),
               ("dW2", (64, 128)), ("db2", (128,)))


class _PoolNarrowCall(object):
    """One case's device inputs; run() makes one call into a fresh output
    buffer -- the six outputs in one allocation with GUARD floats of 7.0
    behind each -- and returns (rc, {name: array}, guards intact)."""

    def __init__(self, dev, c, w1t, w2t):
        self.dev, self.c, self.w1t, self.w2t = dev, c, w1t, w2t
        self.inputs = [T(c[k], dev) for k in ("feat", "act0", "act1", "dz2")]

    def run(self, accumulate, prefill, ws_bytes=None, rows=None):
        import torch
        from pointgnn_amd import _lib
        lib = _lib.load()
        c, dev = self.c, self.dev
        rows = c['rows'] if rows is None else rows
        shapes = [(n, s or (c['k_in0'], 32)) for n, s in _OUT_SHAPES]
        host = np.full(sum(int(np.prod(s)) + GUARD for _, s in shapes), 7.0,
                       np.float32)
        at, where = 0, {}
        for n, s in shapes:
            size = int(np.prod(s))
            host[at:at + size] = prefill[n].reshape(-1)
            where[n] = (at, size, s)
            at += size + GUARD
        buf = T(host, dev)
        need = int(lib.pgnn_pool_narrow_bwd_workspace_bytes(rows))
        ws = torch.full((need // 4 + 1,), WS_POISON, dtype=torch.float32,
                        device=dev)
        p = lambda n: buf.data_ptr() + 4 * where[n][0]
        rc = lib.pgnn_pool_narrow_bwd_f32(
            *[_lib.ptr(t) for t in self.inputs], rows, _lib.ptr(self.w2t),
            _lib.ptr(self.w1t), c['k_in0'], p("dW0"), p("db0"), p("dW1"),
            p("db1"), p("dW2"), p("db2"), accumulate, _lib.ptr(ws),
            need if ws_bytes is None else ws_bytes, _lib.stream_ptr())
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        res, guards = {}, True
        for n, (a, size, s) in where.items():
            res[n] = got[a:a + size].reshape(s)
            guards = guards and bool(np.all(got[a + size:a + size + GUARD] == 7.0))
        return rc, res, guards


def _prefill(k_in0, accumulate, seed=1):
    """accumulate = 0: NaN poison; 1: integers in [-5, 5]."""
    rng = np.random.default_rng(seed)
    out = {}
    for n, s in _OUT_SHAPES:
        s = s or (k_in0, 32)
        out[n] = rng.integers(-5, 6, s).astype(np.float32) if accumulate \
            else np.full(s, np.nan, np.float32)
    return out


def _assert_exact(res, ref, prefill, accumulate, what):
    for n, want in ref.items():
        if accumulate:
            want = want + prefill[n].astype(np.int64)
        bad = np.argwhere(res[n] != want)
        assert bad.size == 0, "%s %s: %d entries differ, first at %r: %r != %r" % (
            what, n, len(bad), tuple(bad[0]), res[n][tuple(bad[0])],
            want[tuple(bad[0])])


@pytest.mark.parametrize("rows", tp.POOL_ROWS)
def test_pool_narrow_bwd_exact(dev, rows):
    """The fused three-layer backward of the car pooling chain == the int64
    chain, for k_in0 1 / 4 / 15 (feat's pad columns hold 3.0 and must not
    reach dW0), accumulate 0 into NaN-poisoned outputs and 1 into integers,
    the workspace poisoned with 3e38 before every call; two calls give equal
    bits; nothing is written behind an output.  Row counts: below, at and
    above one 32-row tile; 32 s and 32 s - 5 for slice counts s around the
    16-slice groups and the 4 x 16 unrolling of weight_grad_reduce_kernel<16>
    (a short last tile); 16 379 = 512 slices with a short last one; 20 011 =
    two tiles per slice (the prefetch carries a tile)."""
    w1, w2, w1t, w2t = _exact_images(dev)
    for k_in0 in tp.POOL_K_IN0:
        c = tp.pool_chain_case(rows, k_in0)
        ref, _ = tp.pool_chain_exact(c, w1, w2)
        call = _PoolNarrowCall(dev, c, w1t, w2t)
        for accumulate in (0, 1):
            pre = _prefill(k_in0, accumulate)
            what = "rows %d k_in0 %d accumulate %d" % (rows, k_in0, accumulate)
            rc, res, guards = call.run(accumulate, pre)
            assert rc == 0, what
            assert guards, what + ": written behind an output"
            _assert_exact(res, ref, pre, accumulate, what)
            rc, again, _ = call.run(accumulate, pre)
            assert rc == 0
            for n in res:
                assert np.array_equal(res[n].view(np.uint32),
                                      again[n].view(np.uint32)), what + " " + n


@pytest.mark.parametrize("target", tp.POOL_TUNABLE_TARGETS)
def test_pool_narrow_bwd_exact_at_other_slice_targets(dev, target):
    """`wgrad_wg_target` decides the kernel's slice partition AND its
    workspace size: 1 (one workgroup walks all 626 tiles), 3 and 768 (626
    one-tile slices) at E = 20 011, the workspace queried after the tunable is
    set."""
    from pointgnn_amd import _lib
    lib = _lib.load()
    w1, w2, w1t, w2t = _exact_images(dev)
    rows = tp.POOL_TUNABLE_ROWS
    default_bytes = int(lib.pgnn_pool_narrow_bwd_workspace_bytes(rows))
    _lib.set_tunable("wgrad_wg_target", target)
    try:
        slices = tp.pool_narrow_split(rows, target)[1]
        need = int(lib.pgnn_pool_narrow_bwd_workspace_bytes(rows))
        assert need >= slices * (64 * 128 + 128 + 32 * 64 + 64 + 16 * 32 + 32) * 4
        assert need != default_bytes
        for k_in0 in (4, 15):
            c = tp.pool_chain_case(rows, k_in0)
            ref, _ = tp.pool_chain_exact(c, w1, w2)
            call = _PoolNarrowCall(dev, c, w1t, w2t)
            for accumulate in (0, 1):
                pre = _prefill(k_in0, accumulate)
                what = "target %d k_in0 %d accumulate %d" % (target, k_in0,
                                                             accumulate)
                rc, res, guards = call.run(accumulate, pre)
                assert rc == 0 and guards, what
                _assert_exact(res, ref, pre, accumulate, what)
    finally:
        _lib.set_tunable("wgrad_wg_target", WGRAD_WG_TARGET)
    assert int(lib.pgnn_pool_narrow_bwd_workspace_bytes(rows)) == default_bytes


def test_pool_narrow_bwd_workspace_and_empty_input(dev):
    """One byte less than the query answers is PGNN_E_WORKSPACE and leaves the
    outputs untouched; n_rows = 0 zeroes the outputs with accumulate = 0 and
    leaves them with accumulate = 1."""
    from pointgnn_amd import _lib
    lib = _lib.load()
    w1, w2, w1t, w2t = _exact_images(dev)
    c = tp.pool_chain_case(1000, 4)
    call = _PoolNarrowCall(dev, c, w1t, w2t)
    pre = _prefill(4, 1)
    need = int(lib.pgnn_pool_narrow_bwd_workspace_bytes(1000))
    for accumulate in (0, 1):
        rc, res, guards = call.run(accumulate, pre, ws_bytes=need - 1)
        assert rc == _lib.E_WORKSPACE
        assert guards and all(np.array_equal(res[n], pre[n]) for n in pre)
    rc, res, guards = call.run(0, pre, rows=0)
    assert rc == 0 and guards
    assert all(np.all(res[n] == 0) for n in pre)
    rc, res, guards = call.run(1, pre, rows=0)
    assert rc == 0 and guards
    assert all(np.array_equal(res[n], pre[n]) for n in pre)


def test_pool_narrow_bwd_real_values(dev):
    """E = 20 011 Gaussian rows (act = ReLU of Gaussians, Gaussian weights)
    against the float64 chain within pool_chain_bounds -- the masks are
    inputs, so no decision can flip.  The worst error / bound per output is
    printed.

    (No figures are recorded here yet: the ratios have not been measured on
    an MI355X.)"""
    w = tp.pool_chain_real_case(20011, 4)
    c, w1, w2 = w
    ref, _ = tp.pool_chain_f64(c, w1, w2)
    bound = tp.pool_chain_bounds(c, w1, w2)
    call = _PoolNarrowCall(dev, c, _transposed_image(dev, w1),
                           _transposed_image(dev, w2))
    pre = _prefill(4, 0)
    rc, res, guards = call.run(0, pre)
    assert rc == 0 and guards
    ratios = {n: float((np.abs(res[n].astype(np.float64) - ref[n]) /
                        bound[n]).max()) for n in ref}
    print("pool_narrow_bwd real values, worst error / bound: %s" % (
        {n: "%.3g" % r for n, r in ratios.items()},))
    for n, r in ratios.items():
        assert r <= 1.0, "%s: error %.3g x its bound" % (n, r)


# ---- C: pgnn_scatter_max_bwd_f32 --------------------------------------------------
def _run_scatter_max_bwd(dev, data, seg, nseg, out, gout, relu, layout):
    """layout 'aligned' (vec4 kernels) | 'ld21' (row stride 21) | 'offset1'
    (data one float into its buffer); cols % 4 != 0 is the scalar path by
    itself.  grad_data is written into a NaN-poisoned buffer."""
    import torch
    from pointgnn_amd import _lib
    lib = _lib.load()
    rows, cols = data.shape
    ld = cols + 1 if layout == "ld21" else cols
    off = 1 if layout == "offset1" else 0
    hd = np.full(off + rows * ld, np.nan, np.float32)
    hd[off:].reshape(rows, ld)[:, :cols] = data
    d = T(hd, dev)
    s, o, g = T(seg, dev), T(out, dev), T(gout, dev)
    ties = torch.full((nseg * cols,), -7, dtype=torch.int32, device=dev)
    gd = torch.full((rows, cols), float("nan"), dtype=torch.float32, device=dev)
    _lib.check(lib.pgnn_scatter_max_bwd_f32(
        d.data_ptr() + 4 * off, ld, _lib.ptr(s), rows, cols, nseg, _lib.ptr(o),
        cols, _lib.ptr(g), cols, _lib.ptr(ties), _lib.ptr(gd), cols, relu,
        _lib.stream_ptr()), "pgnn_scatter_max_bwd_f32")
    torch.cuda.synchronize()
    return gd.cpu().numpy()


def _check_scatter_max_bwd(dev, rows, cols, nseg, order, layout):
    data, seg, gout = tp.segmax_case(rows, cols, nseg, order)
    out = tp.segment_max_exact(data, seg, nseg)
    assert (order == "sorted") == bool(np.all(np.diff(seg) >= 0))
    assert not np.any(seg == 2) and (seg == -1).any() and (seg == nseg).any()
    for relu in (0, 1):
        ref, cnt = tp.segmax_bwd_ref(data, seg, nseg, out, gout, relu)
        assert cnt.max() >= 3, "the case was meant to be full of ties"
        got = _run_scatter_max_bwd(dev, data, seg, nseg, out, gout, relu, layout)
        # gout / count: exact for every count whose odd part divides 315 (all
        # up to 10), correctly rounded otherwise -- equality either way
        want = ref.astype(np.float32)
        exact = (want.astype(np.float64) == ref)
        assert exact[(cnt <= 10)[np.where((seg >= 0) & (seg < nseg), seg, 0)]].all()
        bad = np.argwhere(got != want)
        assert bad.size == 0, "relu_mask %d: %d entries differ, first %r: %r != %r" % (
            relu, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
        outside = (seg < 0) | (seg >= nseg)
        assert np.all(got[outside] == 0)
        s = np.where(outside, 0, seg)
        tied_zero = ~outside[:, None] & (out[s] == 0) & (data == 0)
        assert tied_zero[seg == 5].sum() >= 2 * cols
        if relu:
            assert np.all(got[out[s] <= 0] == 0)
        else:
            assert np.all(got[tied_zero] != 0)


@pytest.mark.parametrize("order", ["sorted", "permuted"])
@pytest.mark.parametrize("cols,layout", [(20, "aligned"), (19, "aligned"),
                                         (20, "ld21"), (20, "offset1")])
def test_scatter_max_bwd_both_paths_any_order(dev, cols, layout, order):
    """TF's tie-sharing rule, exactly: the vec4 kernels (20 aligned columns)
    and the scalar ones (19 columns; row stride 21; data one float off 16-byte
    alignment), relu_mask 0 and 1, ids sorted and permuted, an empty segment
    and ids -1 / num_segments (exact zeros in a poisoned grad_data); with
    relu_mask a segment whose maximum is 0 gives nothing to anyone."""
    _check_scatter_max_bwd(dev, 500, cols, 13, order, layout)


@pytest.mark.parametrize("cols,layout", [(32, "aligned"), (32, "offset1"),
                                         (128, "aligned")])
def test_scatter_max_bwd_grid_stride_wraps(dev, cols, layout):
    """70 000 rows: the scalar kernels' grid-stride loop wraps past the
    8192-block cap at 32 columns (8750 blocks of work), the vec4 kernels' at
    128 columns (the 32-column aligned case is their one-pass form); 9000
    segments, most of them with a handful of rows."""
    _check_scatter_max_bwd(dev, 70000, cols, 9000, "permuted", layout)


# ---- D: pgnn_edge_hidden_fwd / _bwd -----------------------------------------------
@pytest.mark.parametrize("ld_pq,n_edges", [(4, 5000), (304, 3000), (304, 28000)])
def test_edge_hidden_fwd_is_one_subtraction_and_one_select(dev, ld_pq, n_edges):
    """H1 == max(P[src] - Q[dst], 0) in float32, bit for bit, edges in random
    order (28 000 x 304: the grid-stride loop wraps)."""
    import torch
    from pointgnn_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(ld_pq + n_edges)
    nv = 211
    p = rng.standard_normal((nv, ld_pq)).astype(np.float32)
    q = rng.standard_normal((nv, ld_pq)).astype(np.float32)
    q[::3] = p[::3]                                  # exact zeros too
    edges = rng.integers(0, nv, (n_edges, 2)).astype(np.int32)
    pd, qd, ed = T(p, dev), T(q, dev), T(edges, dev)
    h1 = torch.full((n_edges, ld_pq), float("nan"), dtype=torch.float32,
                    device=dev)
    _lib.check(lib.pgnn_edge_hidden_fwd(_lib.ptr(pd), _lib.ptr(qd), ld_pq,
                                        _lib.ptr(ed), n_edges, _lib.ptr(h1),
                                        _lib.stream_ptr()))
    want = np.maximum(p[edges[:, 0]] - q[edges[:, 1]], np.float32(0))
    assert np.array_equal(h1.cpu().numpy(), want)


def _run_edge_hidden_bwd(dev, dh1, edges, nv, ld, contiguous):
    import torch
    from pointgnn_amd import _lib
    lib = _lib.load()
    n = nv * ld
    nan = float("nan")
    if contiguous:
        buf = torch.full((2 * n + 8,), nan, dtype=torch.float32, device=dev)
        dp, dq = buf[:n], buf[n:2 * n]
    else:
        dp = torch.full((n + 8,), nan, dtype=torch.float32, device=dev)
        dq = torch.full((n + 8,), nan, dtype=torch.float32, device=dev)
    gd, ed = T(dh1, dev), T(edges, dev)
    _lib.check(lib.pgnn_edge_hidden_bwd(
        _lib.ptr(gd) if len(edges) else None, ld,
        _lib.ptr(ed) if len(edges) else None, len(edges), nv, _lib.ptr(dp),
        _lib.ptr(dq), _lib.stream_ptr()))
    torch.cuda.synchronize()
    if contiguous:
        assert torch.isnan(buf[2 * n:]).all(), "written behind dQ"
    else:
        assert torch.isnan(dp[n:]).all() and torch.isnan(dq[n:]).all()
    return (dp[:n].cpu().numpy().reshape(nv, ld),
            dq[:n].cpu().numpy().reshape(nv, ld))


@pytest.mark.parametrize("contiguous", [True, False])
@pytest.mark.parametrize("n_edges,nv,ld,hot", tp.EDGE_BWD_CASES)
def test_edge_hidden_bwd_equals_the_integer_scatter_adds(dev, n_edges, nv, ld,
                                                         hot, contiguous):
    """dP[src] += dH1, dQ[dst] -= dH1 == the int64 scatter-adds (integer dH1,
    about half zeros), into NaN-poisoned outputs: rows of vertices without
    edges are exactly 0.  dQ directly behind dP (one fill) and apart (two):
    the two branches of zero_pair.  One vertex as the destination of all 20 000
    edges; n_edges = 0 still zeroes."""
    dh1, edges = tp.edge_hidden_bwd_case(n_edges, nv, ld, hot)
    ref_p, ref_q = tp.edge_hidden_bwd_exact(dh1, edges, nv)
    dp, dq = _run_edge_hidden_bwd(dev, dh1, edges, nv, ld, contiguous)
    assert np.array_equal(dp, ref_p) and np.array_equal(dq, ref_q)
    assert np.all(dp[nv // 2:] == 0) and np.all(dq[nv // 2:] == 0)
    if hot:
        assert np.count_nonzero(ref_q[1]) and not np.any(ref_q[2:])
    dp, dq = _run_edge_hidden_bwd(dev, dh1[:0], edges[:0], nv, ld, contiguous)
    assert np.all(dp == 0) and np.all(dq == 0)


# ---- E: the small kernels ---------------------------------------------------------
@pytest.mark.parametrize("count", [1, 255, 257, 8192 * 256 + 5])
def test_relu_mask_mul_is_tf_relu_grad(dev, count):
    """dY <- where(Y > 0, dY, 0) with 0.0, -0.0, negatives, NaN and +inf in Y
    (NaN > 0 is false: nothing passes); 8192 * 256 + 5 elements wrap the grid."""
    import torch
    from pointgnn_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(count)
    special = np.array([0.0, -0.0, -1.5, np.nan, np.inf, 2.0, -np.inf, 0.25],
                       np.float32)
    y = special[rng.integers(0, len(special), count)]
    y[0] = special[(count // 2) % len(special)]
    dy = (rng.standard_normal(count) + 3.0).astype(np.float32)
    buf = T(np.concatenate([dy, np.full(8, 7.0, np.float32)]), dev)
    yd = T(y, dev)
    _lib.check(lib.pgnn_relu_mask_mul(_lib.ptr(buf), _lib.ptr(yd), count,
                                      _lib.stream_ptr()))
    got = buf.cpu().numpy()
    with np.errstate(invalid="ignore"):
        want = np.where(y > 0, dy, np.float32(0))
    assert np.array_equal(got[:count], want)
    assert np.all(got[count:] == 7.0)
    if count > 100:
        assert (want == 0).any() and (want != 0).any()


def _pool_feature_inputs(n_pts, n_kp, n_edges, width, seed):
    rng = np.random.default_rng(seed)
    feats = rng.standard_normal((n_pts, width)).astype(np.float32)
    xyz = rng.standard_normal((n_pts, 3)).astype(np.float32)
    kp = rng.permutation(n_pts)[:n_kp].astype(np.int32)
    edges = np.stack([rng.integers(0, n_pts, n_edges),
                      rng.integers(0, n_kp, n_edges)], 1).astype(np.int32)
    return feats, xyz, kp, edges


@pytest.mark.parametrize("n_feat", [0, 1, 13])
def test_pool_features_fwd_rows(dev, n_feat):
    """[f(src) | xyz(src) - xyz(kp(dst)) | 0 ...] as [E, 16] == NumPy float32,
    bit for bit, the pad columns exactly 0 in a poisoned F; n_feat = 14 does
    not fit 16 columns: PGNN_E_INVALID."""
    import torch
    from pointgnn_amd import _lib
    lib = _lib.load()
    n_e = 4001
    feats, xyz, kp, edges = _pool_feature_inputs(300, 40, n_e, max(n_feat, 1),
                                                 n_feat)
    fd, xd, kd, ed = T(feats, dev), T(xyz, dev), T(kp, dev), T(edges, dev)
    F = torch.full((n_e, 16), float("nan"), dtype=torch.float32, device=dev)
    call = lambda nf: lib.pgnn_pool_features_fwd(
        _lib.ptr(fd) if nf else None, nf, _lib.ptr(xd), _lib.ptr(kd),
        _lib.ptr(ed), n_e, _lib.ptr(F), _lib.stream_ptr())
    _lib.check(call(n_feat))
    got = F.cpu().numpy()
    assert np.array_equal(got, tp.pool_features_ref(feats, n_feat, xyz, kp,
                                                    edges, 16))
    assert np.all(got[:, n_feat + 3:] == 0)
    assert call(14) == _lib.E_INVALID


@pytest.mark.parametrize("ld_f", [304, 320])
def test_pool_features_wide_fwd_rows(dev, ld_f):
    """The same rows for 300 features with row stride 304, into [E, 304] and
    [E, 320]; ld_f < n_feat + 3 is PGNN_E_INVALID."""
    import torch
    from pointgnn_amd import _lib
    lib = _lib.load()
    n_e, n_feat = 2003, 300
    feats, xyz, kp, edges = _pool_feature_inputs(150, 30, n_e, 304, ld_f)
    feats[:, n_feat:] = 9.0          # behind the features: never gathered
    fd, xd, kd, ed = T(feats, dev), T(xyz, dev), T(kp, dev), T(edges, dev)
    F = torch.full((n_e, ld_f), float("nan"), dtype=torch.float32, device=dev)
    call = lambda ld: lib.pgnn_pool_features_wide_fwd(
        _lib.ptr(fd), 304, n_feat, _lib.ptr(xd), _lib.ptr(kd), _lib.ptr(ed),
        n_e, _lib.ptr(F), ld, _lib.stream_ptr())
    _lib.check(call(ld_f))
    got = F.cpu().numpy()
    assert np.array_equal(got, tp.pool_features_ref(feats, n_feat, xyz, kp,
                                                    edges, ld_f))
    assert np.all(got[:, n_feat + 3:] == 0)
    assert call(n_feat + 2) == _lib.E_INVALID


@pytest.mark.parametrize("n", tp.L1_SIZES)
def test_l1_norm_is_the_exact_integer_sum(dev, n):
    """sum |w| over the entries whose mask is non-zero (0 / 1 / 2.0) == the
    int64 sum (the accumulator is a double); `out` is re-zeroed by the call,
    and n = 0 gives 0."""
    import torch
    from pointgnn_amd import _lib
    lib = _lib.load()
    w, mask, ref = tp.l1_case(n)
    wd, md = T(w, dev), T(mask, dev)
    out = torch.full((2,), 12345.0, dtype=torch.float64, device=dev)
    _lib.check(lib.pgnn_l1_norm(_lib.ptr(wd), _lib.ptr(md), n, _lib.ptr(out),
                                _lib.stream_ptr()))
    got = out.cpu().numpy()
    assert got[0] == float(ref) and got[1] == 12345.0
    _lib.check(lib.pgnn_l1_norm(_lib.ptr(wd), _lib.ptr(md), 0, _lib.ptr(out),
                                _lib.stream_ptr()))
    assert out.cpu().numpy()[0] == 0.0
