"""Variables of the three prediction heads and the float64 restatement the GPU
tests of tests/test_gpu_train_heads.py compare with (no GPU needed)."""
import numpy as np
import pytest
import torch

import pointgnn_amd  # noqa: F401
from pointgnn_amd import configs, weights
from oracle import gnn_oracle as go
import _train_heads as th


def _separated(nc=4, base="car_auto_T1"):
    return th.head_config(configs.get_config(base), th.SEPARATED, nc)


@pytest.mark.parametrize("nc,s", [(4, 75), (6, 50)])
def test_separated_head_variables(nc, s):
    """models.py:70-74 + gnn.py:196: the class head keeps the full input
    width, the first layer of every box head takes C / num_classes columns;
    names and order are the shared-input head's."""
    cfg = _separated(nc)
    shared = th.head_config(cfg, 'classaware_predictor')
    spec, spec_shared = weights.variable_specs(cfg), \
        weights.variable_specs(shared)
    assert [n for n, _ in spec] == [n for n, _ in spec_shared]
    first = {"output/predictor/loc/cls_%d/fully_connected/weights" % j
             for j in range(nc)}
    for (n, shape), (_, shape_shared) in zip(spec, spec_shared):
        if n in first:
            assert shape == (s, 64) and shape_shared == (300, 64)
        else:
            assert shape == shape_shared, n
    d = dict(spec)
    assert d["output/predictor/cls/fully_connected/weights"] == (300, 64)
    assert d["output/predictor/cls/fully_connected_1/weights"] == (64, nc)
    assert d["output/predictor/loc/cls_%d/fully_connected_2/weights"
             % (nc - 1)] == (64, 7)
    # the head is the last thing in the list: cls, then loc/cls_0 .. nc-1
    tail = [n for n, _ in spec if n.startswith("output/")]
    assert tail == [n for n, _ in spec][-len(tail):]
    assert tail[:4] == ["output/predictor/cls/fully_connected/weights",
                        "output/predictor/cls/fully_connected/biases",
                        "output/predictor/cls/fully_connected_1/weights",
                        "output/predictor/cls/fully_connected_1/biases"]
    assert tail[4] == "output/predictor/loc/cls_0/fully_connected/weights"
    assert weights.count_params(shared) - weights.count_params(cfg) == \
        nc * (300 - s) * 64
    p = weights.init_params(cfg, seed=1)
    assert set(p) == set(d) and all(p[n].shape == d[n] for n in d)


def test_separated_head_needs_a_divisible_width():
    cfg = _separated(8)
    for fn in (weights.variable_specs, weights.count_params,
               weights.init_params):
        with pytest.raises(ValueError) as e:
            fn(cfg)
        assert "300" in str(e.value) and "8" in str(e.value)


def test_shipped_specs_are_unchanged():
    """The two existing heads: the totals of the reference checkpoints
    (tests/test_host_cpu.py; they include the int32
    global step) and the stored weights' names and shapes."""
    expect = {"car_auto_T0": 344933, "car_auto_T1": 726492,
              "car_auto_T2": 1108051, "car_auto_T3": 1489610,
              "ped_cyl_auto_T3": 1357274, "car_fixed_T3": 1431233}
    for name, total in expect.items():
        cfg = configs.get_config(name)
        assert weights.count_params(cfg) + 1 == total
        # `_128`: 64 -> 128 in the nc + 1 heads, nothing else
        c = {"ped_cyl_auto_T3": 256}.get(name, 300)   # feature width
        nc = cfg["num_classes"]
        wide = th.head_config(cfg, 'classaware_predictor_128')

        def head(hw):
            return (c * hw + hw + hw * nc + nc) + nc * (
                c * hw + hw + hw * hw + hw + hw * 7 + 7)
        assert weights.count_params(wide) - weights.count_params(cfg) == \
            head(128) - head(64)
    import os
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    for t in (0, 1):
        w = np.load(os.path.join(gold, "weights_car_auto_T%d.npz" % t))
        spec = weights.variable_specs(configs.car_auto_config(t))
        assert len(spec) == len(w.files)
        for k, shape in spec:
            assert w[k].shape == tuple(shape)


def test_separated_restatement_is_the_shared_head_on_each_slice():
    """The float64 separated head = the shared-input oracle head
    (oracle/gnn_oracle.class_aware_predictor) run on one column slice per
    class, plus the class MLP on all columns."""
    rng = np.random.default_rng(3)
    k, c, nc = 37, 300, 4
    s = c // nc
    cfg = _separated(nc)
    params = {n: rng.standard_normal(shape) / np.sqrt(shape[0])
              for n, shape in weights.variable_specs(cfg)
              if n.startswith("output/")}
    feats = rng.standard_normal((k, c))
    tp = {n: torch.as_tensor(v) for n, v in params.items()}
    logits, boxes = th.separated_head(tp, "output", torch.as_tensor(feats), nc)
    assert logits.shape == (k, nc) and boxes.shape == (k, nc, 7)
    want_logits = go.multi_layer_neural_network(
        feats, go._layers(params, "output/predictor/cls", np.float64),
        is_logits=True)
    np.testing.assert_allclose(logits.numpy(), want_logits, rtol=0, atol=1e-12)
    # a class head of the slice's width so that the shared-input oracle head
    # runs on the slice (its logits are not looked at)
    sliced = dict(params)
    sliced["output/predictor/cls/fully_connected/weights"] = np.zeros((s, 64))
    for j in range(nc):
        _, b = go.class_aware_predictor(sliced, "output",
                                        feats[:, j * s:(j + 1) * s], nc,
                                        dtype=np.float64)
        np.testing.assert_allclose(boxes[:, j].numpy(), b[:, j], rtol=0,
                                   atol=1e-12)
        if j:   # and it is NOT the head on the first slice
            assert np.abs(boxes[:, j].numpy() - b[:, 0]).max() > 1e-3


def test_restated_forward_equals_the_oracle_for_shared_heads():
    """body_features + a shared-input head on top reproduce
    train_oracle.forward exactly, decisions included: the stage code the
    separated restatement stands on is the oracle's own."""
    from oracle import train_oracle as to
    from test_gpu_train import _tiny_batch
    cfg = configs.car_auto_config(1)
    batch = _tiny_batch(seed=3)
    params = {n: torch.as_tensor(v, dtype=torch.float64) for n, v in
              weights.init_params(cfg, seed=5, bias_scale=0.1).items()}
    d0, d1 = to.Decisions(), to.Decisions()
    logits, boxes = to.forward(params, cfg, *batch[:4], decisions=d0)
    feats = th.body_features(params, cfg, *batch[:4], decisions=d1)
    assert to._mlp.__module__ == to.__name__       # (put back)
    assert feats.shape == (logits.shape[0], 300)
    lg = to._mlp(feats, params, "output/predictor/cls", 2, True, d1)
    bx = [to._mlp(feats, params, "output/predictor/loc/cls_%d" % j, 3, True,
                  d1) for j in range(4)]
    assert torch.equal(lg, logits)
    assert all(torch.equal(b, boxes[:, j]) for j, b in enumerate(bx))
    assert len(d0.taken) == len(d1.taken)
    assert all(np.array_equal(a, b) for a, b in zip(d0.taken, d1.taken))


def test_regularizer_scales_by_the_reference_keywords():
    from pointgnn_amd.models import regularizer_scales
    assert regularizer_scales(None, None) == (0.0, 0.0)
    assert regularizer_scales('l1', {'scale': 5e-7}) == (5e-7, 0.0)
    assert regularizer_scales('l2', {'scale': 1e-2}) == (0.0, 1e-2)
    assert regularizer_scales('l1_l2', {}) == (1.0, 1.0)
    assert regularizer_scales('l1_l2', {'scale_l2': 0.5}) == (1.0, 0.5)
    for kind, kw in (('l1', {'scale': 1.0, 'scale_l2': 1.0}),
                     ('l2', {'scales': 1.0}), ('l1_l2', {'scale': 1.0})):
        with pytest.raises(ValueError):
            regularizer_scales(kind, kw)
