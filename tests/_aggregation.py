"""Shared pieces of tests/test_gpu_aggregation.py: integer-valued inputs on
which every fp32 partial sum is exact, their int64 references, and a float64
evaluation of a model whose two graph operators aggregate with a sum or a
mean.  Nothing here needs a GPU at import time."""
import copy

import numpy as np

import _ws_cases as wc
from oracle import gnn_oracle as go

EXACT = float(2 ** 24)      # integers below it are exact in fp32


# ---- exact inputs: the edge stage --------------------------------------------
def sparse_signs(rng, k_in, n_out, per_col):
    """[k_in, n_out] with exactly `per_col` entries of +-1 in every column."""
    w = np.zeros((k_in, n_out), np.float32)
    for j in range(n_out):
        rows = rng.choice(k_in, per_col, replace=False)
        w[rows, j] = rng.choice([-1.0, 1.0], per_col)
    return w


def _matmul_i64(x, w):
    """x @ w for small integers: through float64 (BLAS; NumPy's int64 product
    is a plain loop), exact while every dot product stays below 2^53."""
    y = x.astype(np.float64) @ w.astype(np.float64)
    assert np.abs(y).max(initial=0) < 2.0 ** 53
    return np.rint(y).astype(np.int64)


def exact_edge_input(case, c, seed=21):
    """_ws_cases.edge_input with P, Q integers in [-4, 4], four +-1 per column
    of W and a bias of integers in [-3, 3]: a row act(h W + b) is an integer of
    magnitude <= 4 * 8 + 3 = 35."""
    inp = wc.edge_input(case, c)
    rng = np.random.default_rng(seed)
    for name in ("p", "q"):
        a = np.zeros_like(inp[name])
        a[:, :c] = rng.integers(-4, 5, (a.shape[0], c))
        inp[name] = a
    inp["w"] = sparse_signs(rng, c, c, 4)
    inp["b"] = rng.integers(-3, 4, c).astype(np.float32)
    return inp


def edge_rows_i64(inp):
    """The per-edge rows of the live edges and their destinations, int64."""
    p, q, c = inp["p"].astype(np.int64), inp["q"].astype(np.int64), inp["c"]
    e = inp["edges"].astype(np.int64)
    src, dst = e[:, 0], e[:, 1]
    ok = (dst >= 0) & (dst < inp["k"])
    h1 = np.maximum(p[src, :c] - q[np.where(ok, dst, 0), :c], 0)
    rows = np.maximum(_matmul_i64(h1, inp["w"]) + inp["b"].astype(np.int64), 0)
    return rows[ok], dst[ok]


# ---- exact inputs: pooling ---------------------------------------------------
def exact_pool_input(case, seed=22):
    """_ws_cases.pool_input (car) with integer coordinates in [-3, 3],
    intensity in {0, 1}, at most two +-1 per column of every layer and biases
    in {0, 1}."""
    inp = wc.pool_input(case, "car")
    rng = np.random.default_rng(seed)
    n_pts = inp["xyz"].shape[0]
    inp["xyz"] = rng.integers(-3, 4, (n_pts, 3)).astype(np.float32)
    inp["inten"] = rng.integers(0, 2, (n_pts, 1)).astype(np.float32)
    widths = wc.POOL_WIDTHS["car"]
    inp["layers"] = [
        (sparse_signs(rng, a, b, min(2, a)),
         rng.integers(0, 2, b).astype(np.float32), 0)
        for a, b in zip(widths[:-1], widths[1:])]
    return inp


def pool_rows_i64(inp):
    e = inp["edges"].astype(np.int64)
    src, dst = e[:, 0], e[:, 1]
    ok = (dst >= 0) & (dst < inp["k"])
    xyz = inp["xyz"].astype(np.int64)
    kp = inp["kp"].astype(np.int64)
    x = np.concatenate([inp["inten"].astype(np.int64)[src],
                        xyz[src] - xyz[kp[np.where(ok, dst, 0)]]], axis=1)
    for w, b, _ in inp["layers"]:
        x = np.maximum(_matmul_i64(x, w) + b.astype(np.int64), 0)
    return x[ok], dst[ok]


def exact_reference(rows, dst, k):
    """(sum int64 [k, c], in-degree int64 [k]); asserts that every partial sum
    -- in ANY order: the sum of the magnitudes bounds them all -- stays below
    2^24, so that fp32 adds them exactly."""
    s = np.zeros((k, rows.shape[1]), np.int64)
    np.add.at(s, dst, rows)
    # (the rows left a ReLU: no negative terms, the sums ARE the magnitudes')
    assert rows.min(initial=0) >= 0
    assert s.max(initial=0) < EXACT, \
        "a partial sum could leave fp32's exact range"
    return s, np.bincount(dst, minlength=k).astype(np.int64)


def check_exact(got, s, deg, aggregation, c, what):
    """got [k, padded]: sum == the int64 reference; mean within one rounding
    (2^-22: the division may be a reciprocal and a multiply) of sum / max(deg,
    1); empty segments and pad columns exactly 0."""
    assert np.all(got[:, c:] == 0), "%s: pad columns not zero" % what
    assert np.all(got[deg == 0] == 0), "%s: an empty segment is not zero" % what
    if aggregation == "sum":
        bad = np.argwhere(got[:, :c] != s)
        assert bad.size == 0, "%s: %d elements differ, first at %r: %r != %r" % (
            what, len(bad), tuple(bad[0]), got[tuple(bad[0])], s[tuple(bad[0])])
    else:
        want = s / np.maximum(deg, 1)[:, None]
        err = np.abs(got[:, :c].astype(np.float64) - want)
        assert np.all(err <= 2.0 ** -22 * np.abs(want)), \
            "%s: mean off by %g (relative)" % (
                what, (err / np.maximum(np.abs(want), 1e-300)).max())


# ---- real inputs: the summation bound -----------------------------------------
def sum_bound_check(got, rows, dst, k, c, aggregation, what):
    """`rows` are the device's own per-edge rows (bit for bit what the kernel
    adds), so only the order of the additions separates `got` from their
    float64 sum S: |got - S| <= deg * 2^-24 * A with A the sum of magnitudes
    (recursive summation in any order).  Mean: that / deg + 2^-22 |S / deg|.
    Returns the largest error / bound ratio."""
    r = rows[:, :c].astype(np.float64)
    ok = (dst >= 0) & (dst < k)
    S = np.zeros((k, c))
    A = np.zeros((k, c))
    np.add.at(S, dst[ok], r[ok])
    np.add.at(A, dst[ok], np.abs(r[ok]))
    deg = np.bincount(dst[ok], minlength=k).astype(np.float64)
    bound = deg[:, None] * 2.0 ** -24 * A
    want = S
    if aggregation == "mean":
        d = np.maximum(deg, 1)[:, None]
        want = S / d
        bound = bound / d + 2.0 ** -22 * np.abs(want)
    err = np.abs(got[:, :c].astype(np.float64) - want)
    assert np.all(err <= bound), "%s: %d elements beyond the bound, worst %g x" % (
        what, int((err > bound).sum()),
        (err / np.maximum(bound, 1e-300))[err > bound].max())
    assert np.all(got[:, c:] == 0) and np.all(got[deg == 0] == 0), what
    return float((err / np.maximum(bound, 1e-300)).max())


# ---- float64 evaluation of a sum- / mean-aggregating model ----------------------
def segment_reduce(rows, dst, k, aggregation):
    """tf.math.unsorted_segment_sum / _mean."""
    out = np.zeros((k, rows.shape[1]), rows.dtype)
    np.add.at(out, dst, rows)
    if aggregation == "mean":
        out = out / np.maximum(np.bincount(dst, minlength=k), 1)[:, None]
    return out


def _mlp(params, scope, x, is_logits):
    return go.multi_layer_neural_network(x, go._layers(params, scope, x.dtype),
                                         is_logits)


def model_f64(params, config, feats, coords, kps, edges, aggregation):
    """MultiLayerFastLocalGraphModelV2.predict (models.py:79-163) with the
    aggregator of gnn.py:211-220 / 285-296 swapped, in float64.  Returns
    (logits, boxes, [features after every layer])."""
    f8 = np.float64
    feats = feats.astype(f8)
    out = []
    layer_configs = config['model_kwargs']['layer_configs']
    for lc in layer_configs[:-1]:
        lvl, scope = lc['graph_level'], lc['scope']
        e = edges[lvl].astype(np.int64)
        src, dst = e[:, 0], e[:, 1]
        x = coords[lvl].astype(f8)
        if lc['type'] == 'scatter_max_point_set_pooling':
            kp = kps[lvl].reshape(-1).astype(np.int64)
            rows = _mlp(params, scope + '/extract_vertex_features',
                        np.concatenate([feats[src], x[src] - x[kp[dst]]], 1),
                        False)
            agg = segment_reduce(rows, dst, len(kp), aggregation)
            feats = _mlp(params, scope + '/combined_features', agg, False)
        else:
            assert lc['type'] == 'scatter_max_graph_auto_center_net'
            xo = x
            if lc['kwargs']['auto_offset']:
                xo = x + _mlp(params, scope, feats, True)
            rows = _mlp(params, scope + '/extract_vertex_features',
                        np.concatenate([feats[src], x[src] - xo[dst]], 1), False)
            agg = segment_reduce(rows, dst, feats.shape[0], aggregation)
            feats = _mlp(params, scope + '/combined_features', agg, True) + feats
        out.append(feats)
    logits, boxes = go.class_aware_predictor(
        params, layer_configs[-1]['scope'], feats, config['num_classes'], f8)
    return logits, boxes, out


def with_iterations(config, t):
    """`config` with only the first `t` GraphNetAutoCenter layers."""
    cfg = copy.deepcopy(config)
    lcs = cfg['model_kwargs']['layer_configs']
    gnn_layers = [lc for lc in lcs
                  if lc['type'] == 'scatter_max_graph_auto_center_net']
    drop = {id(lc) for lc in gnn_layers[t:]}
    cfg['model_kwargs']['layer_configs'] = [lc for lc in lcs
                                            if id(lc) not in drop]
    return cfg
