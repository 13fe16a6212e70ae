"""References of tests/test_gpu_train_primitives.py: the training primitives of
csrc/train.hip restated in NumPy int64 / float64, and the inputs on which the
device's float32 arithmetic is exact.  Nothing here needs a GPU;
tests/test_train_primitives_cpu.py checks these references themselves.

The instrument is the one of tests/_aggregation.py: integer-valued inputs whose
sums of magnitudes -- which bound every partial sum in any order -- stay below
2^24, so that fp32 adds, MFMAs and float atomics are exact and the device must
EQUAL the int64 result."""
import numpy as np

from _aggregation import EXACT, sparse_signs

U = 2.0 ** -24          # unit roundoff of float32


def _mm(a, b):
    """a @ b for integer-valued arrays through float64 (exact below 2^53)."""
    y = a.astype(np.float64) @ b.astype(np.float64)
    assert np.abs(y).max(initial=0) < 2.0 ** 53
    return y


# ---- A / B: the pooling chain feat -> 32 -> 64 -> 128 ---------------------------
# row counts at the default wgrad_wg_target (512 slices of 32-row tiles)
POOL_ROWS = ([1, 31, 32, 33, 63, 65] +
             [32 * s - d for s in (15, 16, 17, 48, 49, 64, 65) for d in (0, 5)] +
             [16379,        # 512 slices, the last one short
              20011])       # rps = 64: two tiles per slice (the prefetch carries one)
POOL_K_IN0 = (1, 4, 15)
POOL_TUNABLE_ROWS = 20011
POOL_TUNABLE_TARGETS = (1, 3, 768)
FEAT_PAD = 3.0          # columns k_in0..15 of feat: allocated, must not reach dW0


def signed_weights(rng, k_in, n_out):
    """One +-1 per column (_aggregation.sparse_signs) plus one in every row
    that was left empty: every input feeds some output."""
    w = sparse_signs(rng, k_in, n_out, 1)
    for i in np.flatnonzero(~w.any(axis=1)):
        w[i, rng.integers(n_out)] = rng.choice([-1.0, 1.0])
    return w


def pool_chain_weights(seed=5):
    rng = np.random.default_rng(seed)
    return signed_weights(rng, 32, 64), signed_weights(rng, 64, 128)


def pool_chain_case(rows, k_in0, seed=0):
    """Integer inputs of pgnn_pool_narrow_bwd_f32: feat in [-2, 2] (pad columns
    FEAT_PAD), act0 / act1 from {0, 0, 1, 2, 3} (their zeros are the ReLU
    masks), dz2 in [-2, 2]."""
    rng = np.random.default_rng([seed, rows, k_in0])
    feat = np.full((rows, 16), FEAT_PAD, np.float32)
    feat[:, :k_in0] = rng.integers(-2, 3, (rows, k_in0))
    acts = np.array([0, 0, 1, 2, 3], np.float32)
    return dict(rows=rows, k_in0=k_in0, feat=feat,
                act0=acts[rng.integers(0, 5, (rows, 32))],
                act1=acts[rng.integers(0, 5, (rows, 64))],
                dz2=rng.integers(-2, 3, (rows, 128)).astype(np.float32))


def pool_chain_real_case(rows, k_in0, seed=0):
    """Gaussian inputs and weights; act = ReLU of Gaussians (half zeros)."""
    rng = np.random.default_rng([seed, rows, k_in0, 1])
    g = lambda *s: rng.standard_normal(s).astype(np.float32)
    feat = np.full((rows, 16), FEAT_PAD, np.float32)
    feat[:, :k_in0] = g(rows, k_in0)
    w1 = g(32, 64) / np.float32(np.sqrt(32))
    w2 = g(64, 128) / np.float32(np.sqrt(64))
    return dict(rows=rows, k_in0=k_in0, feat=feat,
                act0=np.maximum(g(rows, 32), 0), act1=np.maximum(g(rows, 64), 0),
                dz2=g(rows, 128)), w1, w2


def pool_chain_f64(c, w1, w2):
    """The chain of csrc/train.hip's pool_narrow_bwd_kernel in float64:
         dW2 = A1^T Z2            D1 = (Z2 W2^T) * [A1 > 0]
         dW1 = A0^T D1            D0 = (D1 W1^T) * [A0 > 0]
         dW0 = F^T D0             db_l = column sums of Z2 / D1 / D0
    Returns ({name: array}, (D1, D0))."""
    f8 = np.float64
    F = c['feat'][:, :c['k_in0']].astype(f8)
    A0, A1, Z2 = c['act0'].astype(f8), c['act1'].astype(f8), c['dz2'].astype(f8)
    D1 = (Z2 @ w2.astype(f8).T) * (A1 > 0)
    D0 = (D1 @ w1.astype(f8).T) * (A0 > 0)
    out = dict(dW2=A1.T @ Z2, db2=Z2.sum(0), dW1=A0.T @ D1, db1=D1.sum(0),
               dW0=F.T @ D0, db0=D0.sum(0))
    return out, (D1, D0)


def pool_chain_exact(c, w1, w2):
    """pool_chain_f64 as int64, after asserting the precondition of exactness:
    |X|^T |D| and sum |D| of every layer (they bound every partial sum of every
    output, whatever the slices and the order) and the two dX products stay
    below 2^24.  Returns ({name: int64 array}, largest magnitude sum)."""
    ref, (D1, D0) = pool_chain_f64(c, w1, w2)
    F = np.abs(c['feat'][:, :c['k_in0']])
    A0, A1, Z2 = np.abs(c['act0']), np.abs(c['act1']), np.abs(c['dz2'])
    worst = 0.0
    for X, D in ((A1, Z2), (A0, np.abs(D1)), (F, np.abs(D0))):
        worst = max(worst, _mm(X.T, D).max(initial=0), D.sum(0).max(initial=0))
    worst = max(worst, _mm(Z2, np.abs(w2).T).max(initial=0),
                _mm(np.abs(D1), np.abs(w1).T).max(initial=0))
    assert worst < EXACT, "a partial sum could leave fp32's exact range"
    return {k: np.rint(v).astype(np.int64) for k, v in ref.items()}, worst


def pool_chain_bounds(c, w1, w2):
    """Running error bounds of the float32 chain against pool_chain_f64, in
    float64 from the magnitudes, u = 2^-24 and no other constant (E rows are
    summed per output; the dX products are dot products of 128 and 64 terms):
      |d dW2| <= E u |A1|^T |Z2|
      e1 = 128 u (|Z2| |W2|^T) [A1 > 0]          (error of the device's D1)
      |d dW1| <= E u |A0|^T |D1| + |A0|^T e1
      e0 = (64 u |D1| |W1|^T + e1 |W1|^T) [A0 > 0]
      |d dW0| <= E u |F|^T |D0| + |F|^T e0
    and the db likewise with the all-ones column in place of X."""
    f8 = np.float64
    _, (D1, D0) = pool_chain_f64(c, w1, w2)
    E = float(c['rows'])
    F = np.abs(c['feat'][:, :c['k_in0']].astype(f8))
    A0, A1 = np.abs(c['act0'].astype(f8)), np.abs(c['act1'].astype(f8))
    Z2 = np.abs(c['dz2'].astype(f8))
    aw1, aw2 = np.abs(w1.astype(f8)), np.abs(w2.astype(f8))
    e1 = 128 * U * (Z2 @ aw2.T) * (A1 > 0)
    e0 = (64 * U * (np.abs(D1) @ aw1.T) + e1 @ aw1.T) * (A0 > 0)
    D1, D0 = np.abs(D1), np.abs(D0)
    return dict(dW2=E * U * (A1.T @ Z2), db2=E * U * Z2.sum(0),
                dW1=E * U * (A0.T @ D1) + A0.T @ e1,
                db1=E * U * D1.sum(0) + e1.sum(0),
                dW0=E * U * (F.T @ D0) + F.T @ e0,
                db0=E * U * D0.sum(0) + e0.sum(0))


def pool_narrow_split(rows, target=512):
    """pn_split of csrc/train.hip: (rows per slice, slices)."""
    max_s = (rows + 31) // 32
    s = max(1, min(target, max_s))
    rps = (rows + s - 1) // s
    rps = (rps + 31) // 32 * 32
    return rps, max(1, (rows + rps - 1) // rps)


# ---- C: the gradient of unsorted_segment_max --------------------------------------
GOUT_UNIT = 2520        # divisible by every tie count up to 10


def segment_max_exact(data, seg, nseg):
    """[nseg, cols] maxima over the rows with 0 <= seg < nseg; an empty
    segment is 0 (what pgnn_scatter_max_f32 leaves there)."""
    ok = (seg >= 0) & (seg < nseg)
    out = np.full((nseg, data.shape[1]), -np.inf, data.dtype)
    np.maximum.at(out, seg[ok], data[ok])
    out[np.isinf(out)] = 0
    return out


def segmax_bwd_ref(data, seg, nseg, out, gout, relu_mask):
    """TF's _UnsortedSegmentMinOrMaxGrad in float64: the rows equal to their
    segment's maximum share its gradient equally; relu_mask: rows whose value
    is not > 0 get nothing (and do not count).  Rows with an id outside
    [0, nseg) get zeros.  Returns (grad_data float64, tie counts)."""
    ok = (seg >= 0) & (seg < nseg)
    s = np.where(ok, seg, 0).astype(np.int64)
    d = data.astype(np.float64)
    sel = ok[:, None] & (d == out.astype(np.float64)[s])
    if relu_mask:
        sel &= d > 0
    cnt = np.zeros(out.shape, np.int64)
    np.add.at(cnt, s, sel)
    g = np.where(sel, gout.astype(np.float64)[s] / np.maximum(cnt[s], 1), 0.0)
    return g, cnt


def segmax_case(rows, cols, nseg, order, seed=0):
    """data integers in [-2, 2] (ties are plentiful), ids with an empty
    segment (2) and the ids -1 and nseg among them; the rows of segment 5 are
    held at <= 0 (ReLU outputs that are all zero: its maxima are tied zeros).
    gout: non-zero integer multiples of GOUT_UNIT below 2^24."""
    rng = np.random.default_rng([seed, rows, cols])
    data = rng.integers(-2, 3, (rows, cols)).astype(np.float32)
    seg = np.sort(rng.integers(-1, nseg + 1, rows)).astype(np.int32)
    seg[seg == 2] = 3
    data[seg == 5] = np.minimum(data[seg == 5], 0)
    if order == "permuted":
        p = rng.permutation(rows)
        data, seg = data[p], seg[p]
    m = int(EXACT) // GOUT_UNIT - 1
    gout = (GOUT_UNIT * rng.integers(1, m + 1, (nseg, cols)) *
            rng.choice([-1, 1], (nseg, cols))).astype(np.float32)
    assert np.abs(gout).max() < EXACT
    return data, seg, gout


# ---- D: the edge hidden layer ----------------------------------------------------
def edge_hidden_bwd_exact(dh1, edges, n_vertices):
    """dP[src] += dH1, dQ[dst] -= dH1 in int64; asserts the 2^24 precondition
    on the sums of magnitudes."""
    g = np.rint(dh1).astype(np.int64)
    assert np.array_equal(g, dh1)
    dp = np.zeros((n_vertices, dh1.shape[1]), np.int64)
    dq = np.zeros_like(dp)
    mp, mq = np.zeros_like(dp), np.zeros_like(dp)
    np.add.at(dp, edges[:, 0], g)
    np.add.at(dq, edges[:, 1], -g)
    np.add.at(mp, edges[:, 0], np.abs(g))
    np.add.at(mq, edges[:, 1], np.abs(g))
    assert max(mp.max(initial=0), mq.max(initial=0)) < EXACT
    return dp, dq


def edge_hidden_bwd_case(n_edges, n_vertices, ld, hot, seed=0):
    """Integer dH1 in [-3, 3] with about half zeros; permuted edges over the
    lower half of the vertices (the upper half has no edges); `hot`: vertex 1
    is the destination of every edge."""
    rng = np.random.default_rng([seed, n_edges, ld])
    dh1 = (rng.integers(-3, 4, (n_edges, ld)) *
           rng.integers(0, 2, (n_edges, ld))).astype(np.float32)
    used = max(1, n_vertices // 2)
    edges = rng.integers(0, used, (n_edges, 2)).astype(np.int32)
    if hot:
        edges[:, 1] = 1
    return dh1, edges


# (n_edges, n_vertices, ld, hot): ld 3 / 16 / 304; 20 000 edges into one vertex;
# 7 000 x 304 elements wrap the 8192-block grid
EDGE_BWD_CASES = [(1000, 64, 3, False), (20000, 50, 16, True),
                  (7000, 300, 304, False)]


# ---- E: the small kernels --------------------------------------------------------
def pool_features_ref(feats, n_feat, xyz, kp, edges, ld_f):
    """[f(src)[:n_feat] | xyz(src) - xyz(kp(dst)) | 0 ...] in float32."""
    src, dst = edges[:, 0], edges[:, 1]
    out = np.zeros((len(edges), ld_f), np.float32)
    if n_feat:
        out[:, :n_feat] = feats[src, :n_feat]
    out[:, n_feat:n_feat + 3] = xyz[src] - xyz[kp[dst]]
    return out


L1_SIZES = (1, 1023, 4097, 1500001)


def l1_case(n, seed=0):
    """Integer weights in [-1000, 1000], a mask of 0 / 1 / 2.0 (any non-zero
    value counts); returns (w, mask, exact int64 sum)."""
    rng = np.random.default_rng([seed, n])
    w = rng.integers(-1000, 1001, n).astype(np.float32)
    mask = np.array([0.0, 1.0, 2.0], np.float32)[rng.integers(0, 3, n)]
    ref = int(np.abs(w.astype(np.int64))[mask != 0].sum())
    assert ref < 2 ** 53
    return w, mask, ref
