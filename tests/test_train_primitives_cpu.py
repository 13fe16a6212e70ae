"""The references of tests/_train_primitives.py checked without a GPU: the
pooling-chain adjoint against torch float64 autograd, the tie-sharing rule
against the training oracle's segment max, and the 2^24 precondition of every
integer case tests/test_gpu_train_primitives.py runs."""
import numpy as np
import pytest
import torch

import _train_primitives as tp
from oracle import train_oracle as to


@pytest.mark.parametrize("rows,k_in0", [(1, 1), (257, 4), (1000, 15)])
def test_pool_chain_reference_is_the_autograd_of_the_forward(rows, k_in0):
    """pool_chain_f64 == d/d(W_l, b_l) of sum G * (ReLU(ReLU(F W0 + b0) W1 + b1)
    W2 + b2) by torch float64 autograd, to 1e-12 of each gradient's largest
    entry (observed 1e-13 and below)."""
    rng = np.random.default_rng(rows)
    f8 = torch.float64
    t = lambda a, g=False: torch.tensor(a, dtype=f8, requires_grad=g)
    F = rng.standard_normal((rows, k_in0))
    ws = [t(rng.standard_normal(s) / np.sqrt(s[0]), True)
          for s in ((k_in0, 32), (32, 64), (64, 128))]
    bs = [t(0.3 * rng.standard_normal(n), True) for n in (32, 64, 128)]
    G = rng.standard_normal((rows, 128))
    a0 = torch.relu(t(F) @ ws[0] + bs[0])
    a1 = torch.relu(a0 @ ws[1] + bs[1])
    ((a1 @ ws[2] + bs[2]) * t(G)).sum().backward()
    feat = np.full((rows, 16), tp.FEAT_PAD)
    feat[:, :k_in0] = F
    c = dict(rows=rows, k_in0=k_in0, feat=feat, act0=a0.detach().numpy(),
             act1=a1.detach().numpy(), dz2=G)
    ref, _ = tp.pool_chain_f64(c, ws[1].detach().numpy(), ws[2].detach().numpy())
    for l in (0, 1, 2):
        for name, want in (("dW%d" % l, ws[l].grad.numpy()),
                           ("db%d" % l, bs[l].grad.numpy())):
            err = np.abs(ref[name] - want).max()
            assert err <= 1e-12 * max(1.0, np.abs(want).max()), (name, err)


def test_pool_chain_bounds_hold_for_a_float32_evaluation():
    """The running error bounds cover a plain float32 NumPy evaluation of the
    chain (another order of the same sums), with room: the bound is not
    vacuous and not mis-assembled."""
    c, w1, w2 = tp.pool_chain_real_case(3001, 4)
    ref, _ = tp.pool_chain_f64(c, w1, w2)
    bound = tp.pool_chain_bounds(c, w1, w2)
    F, A0, A1, Z2 = c['feat'][:, :4], c['act0'], c['act1'], c['dz2']
    D1 = (Z2 @ w2.T) * (A1 > 0)
    D0 = (D1 @ w1.T) * (A0 > 0)
    got = dict(dW2=A1.T @ Z2, db2=Z2.sum(0), dW1=A0.T @ D1, db1=D1.sum(0),
               dW0=F.T @ D0, db0=D0.sum(0))
    for name in ref:
        assert got[name].dtype == np.float32
        ratio = (np.abs(got[name] - ref[name]) / bound[name]).max()
        assert ratio <= 1.0, (name, ratio)
        assert np.all(bound[name] < 1e-2 * np.abs(ref[name]).max()), name


def test_tie_sharing_reference_is_the_oracle_segment_max_gradient():
    """segmax_bwd_ref (relu_mask 0) == autograd of oracle.train_oracle's
    _segment_max on integer data full of ties, ids in any order; relu_mask 1
    == that times [data > 0] wherever the maximum is positive, and nothing for
    a maximum <= 0."""
    for order in ("sorted", "permuted"):
        data, seg, gout = tp.segmax_case(500, 20, 13, order)
        keep = (seg >= 0) & (seg < 13)      # the oracle takes valid ids only
        out = tp.segment_max_exact(data, seg, 13)
        got0, cnt = tp.segmax_bwd_ref(data, seg, 13, out, gout, 0)
        assert cnt.max() >= 3, "the case was meant to be full of ties"
        assert np.all(cnt[2] == 0) and np.all(got0[~keep] == 0)
        td = torch.tensor(data[keep], dtype=torch.float64, requires_grad=True)
        o = to._segment_max(td, torch.tensor(seg[keep], dtype=torch.int64), 13)
        o = torch.where(torch.isinf(o), torch.zeros_like(o), o)
        assert np.array_equal(o.detach().numpy(), out)
        (o * torch.tensor(gout, dtype=torch.float64)).sum().backward()
        assert np.array_equal(got0[keep], td.grad.numpy())
        got1, _ = tp.segmax_bwd_ref(data, seg, 13, out, gout, 1)
        s = np.where(keep, seg, 0)
        assert np.array_equal(got1, got0 * (data > 0))
        assert np.all(got1[out[s] <= 0] == 0)
        tied_zero = keep[:, None] & (out[s] == 0) & (data == 0)
        assert tied_zero[seg == 5].sum() >= 2 * data.shape[1], \
            "segment 5 was meant to hold tied zero maxima"
        assert np.all(got0[tied_zero] != 0) and np.all(got1[tied_zero] == 0)


def test_every_integer_case_is_inside_the_exact_range():
    """The 2^24 precondition of every integer-valued case of the GPU tests
    (the helpers assert it; the largest pooling-chain magnitude sum is
    printed)."""
    w1, w2 = tp.pool_chain_weights()
    assert np.all(np.abs(w1).sum(0) >= 1) and np.all(np.abs(w1).sum(1) >= 1)
    assert np.all(np.abs(w2).sum(0) >= 1) and np.all(np.abs(w2).sum(1) >= 1)
    worst = 0.0
    for rows in tp.POOL_ROWS:
        for k_in0 in tp.POOL_K_IN0:
            c = tp.pool_chain_case(rows, k_in0)
            assert np.all(c['feat'][:, k_in0:] == tp.FEAT_PAD)
            ref, w = tp.pool_chain_exact(c, w1, w2)
            # accumulate = 1 starts from integers of magnitude <= 5
            assert w + 5 < tp.EXACT
            worst = max(worst, w)
    print("largest pooling-chain magnitude sum %.3g of 2^24 = %.3g" % (
        worst, tp.EXACT))
    for n_e, n_v, ld, hot in tp.EDGE_BWD_CASES:
        dh1, edges = tp.edge_hidden_bwd_case(n_e, n_v, ld, hot)
        dp, dq = tp.edge_hidden_bwd_exact(dh1, edges, n_v)
        assert np.all(dp[n_v // 2:] == 0) and np.all(dq[n_v // 2:] == 0)
        assert 0.3 < (dh1 == 0).mean() < 0.7
    for n in tp.L1_SIZES:
        tp.l1_case(n)
    for order in ("sorted", "permuted"):
        for rows, cols, nseg in ((500, 19, 13), (500, 20, 13), (70000, 32, 9000),
                                 (70000, 128, 9000)):
            data, seg, gout = tp.segmax_case(rows, cols, nseg, order)
            assert np.abs(gout).max() < tp.EXACT
            assert np.all(np.rint(gout / tp.GOUT_UNIT) * tp.GOUT_UNIT == gout)


def test_pool_narrow_split_reaches_the_intended_partitions():
    """The row counts named for their slice partition do give it (pn_split
    restated): 16 379 rows = 512 slices with a short last one, 20 011 rows =
    64-row slices, and the tunable targets 1 / 3 / 768 give 1, 3 and 626
    slices."""
    assert tp.pool_narrow_split(16379) == (32, 512) and 16379 % 32 != 0
    assert tp.pool_narrow_split(20011)[0] == 64
    got = [tp.pool_narrow_split(tp.POOL_TUNABLE_ROWS, t)[1]
           for t in tp.POOL_TUNABLE_TARGETS]
    assert got == [1, 3, 626], got
