"""Float64 restatement of the training step for every prediction head and
weight regularizer of the model registry (reference models/models.py:11-15,
48-75), shared by tests/test_train_heads_cpu.py and
tests/test_gpu_train_heads.py.

oracle/train_oracle.py hard-wires the shared-input head and the l1 term; its
stage code, `loss_terms` and `Decisions` protocol are used as they are, and
only the head (gnn.py:178-213, ClassAwareSeparatedPredictor: box head j reads
the j-th of num_classes equal column slices, tf.split) and the regularizer
(tf.contrib.layers: l1 = scale * sum|w|, l2 = scale * sum(w^2) / 2, l1_l2 their
sum, FC weights only) are restated here.  Decisions are consumed in the
oracle's order: ..., class head, then box heads 0..nc-1."""
import copy

import numpy as np
import torch

from oracle import train_oracle as to

SEPARATED = 'classaware_separated_predictor'


def head_config(base, head, num_classes=None, regularizer=None):
    """`base` (a shipped config) with another predictor type, class count and
    regularizer = (type, kwargs)."""
    cfg = copy.deepcopy(base)
    cfg['model_kwargs']['layer_configs'][-1]['type'] = head
    if num_classes is not None:
        cfg['num_classes'] = num_classes
    if regularizer is not None:
        cfg['model_kwargs']['regularizer_type'] = regularizer[0]
        cfg['model_kwargs']['regularizer_kwargs'] = dict(regularizer[1])
    return cfg


class _Features(Exception):
    def __init__(self, feats):
        self.feats = feats


def body_features(params, config, input_v, coords, kps, edges,
                  dtype=torch.float64, decisions=None):
    """The features entering the head: train_oracle.forward's own stage code,
    left at the point where it turns to the class head."""
    cls_scope = config['model_kwargs']['layer_configs'][-1]['scope'] + \
        '/predictor/cls'
    plain = to._mlp

    def until_head(x, p, scope, *a, **kw):
        if scope == cls_scope:
            raise _Features(x)
        return plain(x, p, scope, *a, **kw)
    to._mlp = until_head
    try:
        to.forward(params, config, input_v, coords, kps, edges, dtype,
                   decisions)
    except _Features as f:
        return f.feats
    finally:
        to._mlp = plain
    raise AssertionError("train_oracle.forward never reached the head")


def separated_head(params, scope, feats, num_classes, dec=None):
    """gnn.py:178-213: logits from all columns, box j from columns
    [j*s, (j+1)*s), s = C / num_classes."""
    c = feats.shape[1]
    assert c % num_classes == 0
    s = c // num_classes
    ps = scope + '/predictor'
    logits = to._mlp(feats, params, ps + '/cls', 2, True, dec)
    boxes = [to._mlp(feats[:, j * s:(j + 1) * s], params,
                     ps + '/loc/cls_%d' % j, 3, True, dec)[:, None, :]
             for j in range(num_classes)]
    return logits, torch.cat(boxes, dim=1)


def forward(params, config, input_v, coords, kps, edges, dtype=torch.float64,
            decisions=None):
    """train_oracle.forward for any of the three heads (the two shared-input
    ones differ in their widths only, which the parameters carry)."""
    head = config['model_kwargs']['layer_configs'][-1]
    if head['type'] != SEPARATED:
        return to.forward(params, config, input_v, coords, kps, edges, dtype,
                          decisions)
    feats = body_features(params, config, input_v, coords, kps, edges, dtype,
                          decisions)
    return separated_head(params, head['scope'], feats, config['num_classes'],
                          decisions)


def regularizer_scales(config):
    """(l1, l2) by tf.contrib.layers' keyword names."""
    mk = config['model_kwargs']
    kind, kw = mk.get('regularizer_type'), mk.get('regularizer_kwargs') or {}
    if kind is None:
        return 0.0, 0.0
    if kind == 'l1':
        return float(kw['scale']), 0.0
    if kind == 'l2':
        return 0.0, float(kw['scale'])
    assert kind == 'l1_l2', kind
    return float(kw.get('scale_l1', 1.0)), float(kw.get('scale_l2', 1.0))


def reg_loss(np_params, config):
    """l1 * sum|w| + l2 * sum(w^2) / 2 over the weights, NumPy float64."""
    l1, l2 = regularizer_scales(config)
    ws = [np.asarray(v, np.float64) for n, v in np_params.items()
          if n.endswith('/weights')]
    return l1 * sum(np.abs(w).sum() for w in ws) + \
        0.5 * l2 * sum((w * w).sum() for w in ws)


def step_gradients(np_params, config, batch, decisions=None):
    """train_oracle.step_gradients for ONE batch and any head: (loss dict,
    {name: gradient of cls + loc})."""
    params = {k: torch.tensor(np.asarray(v), dtype=torch.float64,
                              requires_grad=True)
              for k, v in np_params.items()}
    input_v, coords, kps, edges, labels, boxes, valid = batch
    logits, pred = forward(params, config, input_v, coords, kps, edges,
                           torch.float64, decisions)
    s_ce, s_loc, n, nv = to.loss_terms(config, logits, pred, labels, boxes,
                                       valid)
    cls = config['loss']['cls_loss_weight'] * s_ce / n
    loc = config['loss']['loc_loss_weight'] * s_loc / nv if nv > 0 else \
        torch.zeros((), dtype=torch.float64)
    names = list(params)
    grads = torch.autograd.grad(cls + loc, [params[k] for k in names],
                                allow_unused=True)
    return ({'cls_loss': float(cls.detach()), 'loc_loss': float(loc.detach()),
             'reg_loss': float(reg_loss(np_params, config)),
             'num_endpoint': n, 'num_valid_endpoint': nv},
            {k: (np.zeros(params[k].shape) if g is None
                 else g.detach().numpy()) for k, g in zip(names, grads)})
