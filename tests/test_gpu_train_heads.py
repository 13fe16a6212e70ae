"""Training with every predictor and weight regularizer the model registry
accepts (reference models/models.py:11-15, 48-75): the separated head's column
split, the 128-wide heads' three and four fused groups, the l2 and l1_l2 terms
-- against the float64 restatement of tests/_train_heads.py.

Shapes: tests/test_gpu_train.py's tiny batch on the one-GNN-layer car body
(C = 300).  s = C / nc is 75 for four classes (slices start at columns 75 /
150 / 225: neither 16- nor 4-aligned) and 50 for six (two fused groups: class
head + 4 box heads, then 2); the 128-wide heads form three groups for four
classes and four for six."""
import functools
import warnings

import numpy as np
import pytest

import pointgnn_amd  # noqa: F401
from pointgnn_amd import configs, weights
from oracle import train_oracle as to
from _train_decisions import device_decisions
import _train_heads as th
from test_gpu_train import _grad_errors, _tiny_batch

pytestmark = pytest.mark.gpu

WIDE = 'classaware_predictor_128'
ROWS = [(th.SEPARATED, 4), (th.SEPARATED, 6), (WIDE, 4), (WIDE, 6)]
MODES = (("native", (True, True)), ("python", (False, True)),
         ("dense", (False, False)))


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from pointgnn_amd import _lib
    _lib.load()
    return torch.device("cuda")


@functools.lru_cache(maxsize=None)
def _case(head, nc):
    """(config, parameters, batch) of one row; shared, never written to."""
    cfg = th.head_config(configs.car_auto_config(1), head, nc)
    params = weights.init_params(cfg, seed=5, bias_scale=0.1)
    return cfg, params, _tiny_batch(seed=3, num_classes=nc)


@functools.lru_cache(maxsize=None)
def _free_reference(head, nc):
    """float64 loss, gradients and outputs with the float64 forward's own
    decisions."""
    import torch
    cfg, params, batch = _case(head, nc)
    loss, grads = th.step_gradients(params, cfg, batch)
    with torch.no_grad():
        logits, boxes = th.forward(
            {k: torch.as_tensor(v, dtype=torch.float64)
             for k, v in params.items()}, cfg, *batch[:4])
    return loss, grads, logits.numpy(), boxes.numpy()


def _trainer(head, nc, dev, native=True, sparse=True, **kw):
    from pointgnn_amd import train
    cfg, params, _ = _case(head, nc)
    tr = train.Trainer(cfg, params=params, device=dev, **kw)
    tr.native, tr.sparse_adjoint = native, sparse
    return tr


@pytest.mark.parametrize("head,nc", ROWS)
def test_head_gradients_match_mask_matched_float64(dev, head, nc):
    """tests/test_gpu_train.py::test_full_gradient_matches_mask_matched_oracle
    for the other heads, with its bounds (the kernels and the summation
    lengths are the same ones): the device's own ReLU masks and arg-max
    winners replayed in float64, then every gradient entry of every variable
    within 1e-5 of max|ref| and the losses within 1e-5 -- all three ways of
    running the step."""
    cfg, params, batch = _case(head, nc)
    tr = _trainer(head, nc, dev, native=False)
    tr.forward(*batch[:4])
    masks = device_decisions(tr, cfg)
    dec = to.Decisions(masks)
    loss, g_ref = th.step_gradients(params, cfg, batch, decisions=dec)
    assert dec.pos == len(masks)
    names = [n for n, _ in weights.variable_specs(cfg)]
    s = 300 // nc if head == th.SEPARATED else 300
    hw = 64 if head == th.SEPARATED else 128
    worst = {}
    for mode, (native, sparse) in MODES:
        t2 = _trainer(head, nc, dev, native, sparse)
        out = t2.train_step(batch, apply=False)
        print(mode, "cls %.9g (ref %.9g)  loc %.9g (ref %.9g)" % (
            out['cls_loss'], loss['cls_loss'], out['loc_loss'],
            loss['loc_loss']))
        got = t2.grad_dict()
        assert list(got) == names and set(got) == set(g_ref)
        errs = {n: _grad_errors(got[n], g_ref[n])[0] for n in names}
        worst[mode] = max(errs.values())
        print(mode, "worst entry error %.3g (%s)" % (
            worst[mode], max(errs, key=errs.get)))
        assert abs(out['cls_loss'] - loss['cls_loss']) < \
            1e-5 * max(1, loss['cls_loss'])
        assert abs(out['loc_loss'] - loss['loc_loss']) < \
            1e-5 * max(1, loss['loc_loss'])
        for j in range(nc):
            assert got["output/predictor/loc/cls_%d/fully_connected/weights"
                       % j].shape == (s, hw)
        for n in names:
            assert errs[n] < 1e-5, "%s %s: max-entry rel err %.3g" % (
                mode, n, errs[n])
    print(head, nc, "%d decisions differ; mask-matched worst entry error %s"
          % (sum(dec.flips()), {k: "%.2g" % v for k, v in worst.items()}))


@pytest.mark.parametrize("head,nc", [(th.SEPARATED, 4), (WIDE, 4)])
def test_head_gradients_match_float64(dev, head, nc):
    """tests/test_gpu_train.py::test_full_gradient_matches_oracle's bars with
    the float64 forward left to its own decisions: Frobenius error below 2e-3
    and no entry off by more than 1.2e-2 of max|ref|, per variable."""
    _, _, batch = _case(head, nc)
    loss, g_ref, _, _ = _free_reference(head, nc)
    tr = _trainer(head, nc, dev)
    out = tr.train_step(batch, apply=False)
    got = tr.grad_dict()
    errs = {n: _grad_errors(got[n], ref) for n, ref in g_ref.items()}
    print(head, nc, "worst max-entry %.3g, Frobenius %.3g" % (
        max(e[0] for e in errs.values()), max(e[1] for e in errs.values())))
    assert abs(out['cls_loss'] - loss['cls_loss']) < 1e-4 * max(1, loss['cls_loss'])
    assert abs(out['loc_loss'] - loss['loc_loss']) < 1e-4 * max(1, loss['loc_loss'])
    for n, (e_max, e_fro) in errs.items():
        assert e_fro < 2e-3, "%s: Frobenius rel err %.3g" % (n, e_fro)
        assert e_max < 1.2e-2, "%s: max-entry rel err %.3g" % (n, e_max)


@pytest.mark.parametrize("head,nc", ROWS)
def test_native_step_runs_these_heads(dev, head, nc):
    """The native step takes these models itself: no fall back to the
    Python-driven step (and no warning about one)."""
    _, _, batch = _case(head, nc)
    tr = _trainer(head, nc, dev)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        out = tr.train_step(batch)
    assert tr.native and tr._native_step.handle is not None
    assert np.isfinite(out['cls_loss']) and np.isfinite(out['loc_loss'])


def test_separated_head_needs_a_divisible_width(dev):
    from pointgnn_amd import train
    cfg = th.head_config(configs.car_auto_config(1), th.SEPARATED, 8)
    for fn in (lambda: weights.variable_specs(cfg),
               lambda: train.Trainer(cfg, device=dev)):
        with pytest.raises(ValueError) as e:
            fn()
        assert "300" in str(e.value) and "8" in str(e.value)


@pytest.mark.parametrize("head,nc", ROWS)
def test_training_and_inference_agree(dev, head, nc, tmp_path):
    """Trainer.forward and the inference model on the trainer's weights give
    the float64 restatement's outputs within the project's parity bound
    (1e-3); the separated shapes travel through a checkpoint."""
    import torch
    from pointgnn_amd import models, tf_bundle, train
    cfg, params, batch = _case(head, nc)
    _, _, lg_ref, bx_ref = _free_reference(head, nc)
    tr = _trainer(head, nc, dev)
    logits, boxes = tr.forward(*batch[:4])
    lg_t, bx_t = logits.cpu().numpy(), boxes.cpu().numpy()
    model = models.get_model(cfg["model_name"])(
        num_classes=nc, box_encoding_len=7, mode="test",
        **cfg["model_kwargs"]).load_state_dict(tr.state_dict(), dev)
    lg_m, bx_m = model.predict(*batch[:4], is_training=False)
    for what, got, ref in (("trainer logits", lg_t, lg_ref),
                           ("trainer boxes", bx_t, bx_ref),
                           ("model logits", lg_m, lg_ref),
                           ("model boxes", bx_m, bx_ref)):
        assert got.shape == ref.shape, what
        err = float(np.abs(got - ref).max())
        print(head, nc, what, "max error %.3g" % err)
        assert err < 1e-3, "%s: %.3g" % (what, err)
    if head != th.SEPARATED:
        return
    tr.save_checkpoint(str(tmp_path))
    ck = tf_bundle.load_checkpoint(str(tmp_path))
    for n, shape in weights.variable_specs(cfg):
        assert ck[n].shape == tuple(shape) and np.array_equal(ck[n], params[n])
    assert ck["output/predictor/loc/cls_%d/fully_connected/weights"
              % (nc - 1)].shape == (300 // nc, 64)
    b = train.Trainer(cfg, seed=99, device=dev)
    assert not torch.equal(b.flat, tr.flat)
    b.load_checkpoint(str(tmp_path))
    assert torch.equal(b.flat, tr.flat)


# ---- regularizers ----------------------------------------------------------
REGS = [('l2', {'scale': 1e-2}), ('l1_l2', {'scale_l1': 1e-3, 'scale_l2': 1e-2})]
_TCFG = {'initial_lr': 0.01, 'decay_step': 1000, 'decay_factor': 0.5,
         'optimizer_kwargs': {}, 'unify_copies': True}


def _reg_case(reg):
    cfg = th.head_config(configs.car_auto_config(1), 'classaware_predictor',
                         regularizer=reg)
    return cfg, weights.init_params(cfg, seed=6, bias_scale=0.05), \
        _tiny_batch(seed=4)


@pytest.mark.parametrize("reg", REGS, ids=[r[0] for r in REGS])
@pytest.mark.parametrize("opt", ["sgd", "momentum", "rmsprop", "adam"])
def test_regularized_optimizer_step(dev, opt, reg):
    """One step from fresh slots by TF 1.x's update rules (as replayed in
    test_other_optimizers_follow_tf_update_rules, with its bounds) fed
    g + l1 sign(w) + l2 w on the weights and g on the biases; the step's
    reg_loss against NumPy float64."""
    from pointgnn_amd import train
    cfg, params, batch = _reg_case(reg)
    l1, l2 = th.regularizer_scales(cfg)
    tcfg = dict(_TCFG, optimizer=opt)
    tr = train.Trainer(cfg, train_config=tcfg, params=params, device=dev)
    assert (tr.l1_scale, tr.l2_scale) == (l1, l2)
    f = np.float32
    kw = {'sgd': {}, 'momentum': {'momentum': 0.9},
          'rmsprop': {'momentum': 0.9, 'decay': 0.9, 'epsilon': 1.0},
          'adam': {'beta1': 0.9, 'beta2': 0.999, 'epsilon': 1e-8}}[opt]
    before = tr.state_dict()
    out = tr.train_step(batch)
    g, after = tr.grad_dict(), tr.state_dict()
    want_reg = th.reg_loss(before, cfg)
    print(opt, reg[0], "reg_loss %.9g (float64 %.9g)" % (out['reg_loss'],
                                                         want_reg))
    assert abs(out['reg_loss'] - want_reg) < 1e-5 * max(1, want_reg)
    lr = f(train.learning_rate(tcfg, 0))
    for n in before:
        gi = g[n]
        if n.endswith('/weights'):
            gi = gi + f(l1) * np.sign(before[n]) + f(l2) * before[n]
        gi = gi.astype(f)
        s0 = np.full_like(gi, 1.0 if opt == 'rmsprop' else 0.0)
        s1 = np.zeros_like(gi)
        if opt == 'sgd':
            want = before[n] - lr * gi
        elif opt == 'momentum':
            s0 = f(kw['momentum']) * s0 + gi
            want = before[n] - lr * s0
        elif opt == 'rmsprop':
            s0 = f(kw['decay']) * s0 + f(1 - kw['decay']) * gi * gi
            s1 = f(kw['momentum']) * s1 + lr * gi / np.sqrt(s0 + f(kw['epsilon']))
            want = before[n] - s1
        else:
            lr_t = f(lr * np.sqrt(1 - kw['beta2']) / (1 - kw['beta1']))
            s0 = f(kw['beta1']) * s0 + f(1 - kw['beta1']) * gi
            s1 = f(kw['beta2']) * s1 + f(1 - kw['beta2']) * gi * gi
            want = before[n] - lr_t * s0 / (np.sqrt(s1) + f(kw['epsilon']))
        np.testing.assert_allclose(after[n], want, atol=2e-7, rtol=2e-5,
                                   err_msg="%s %s %s" % (opt, reg[0], n))


@pytest.mark.parametrize("reg", REGS, ids=[r[0] for r in REGS])
def test_model_loss_reports_the_regularizer(dev, reg):
    """models.loss's reg_loss = l1 sum|w| + l2 sum(w^2) / 2 over the weights
    (it used to be 0.0 for 'l2' / 'l1_l2'), equal to the training step's."""
    from pointgnn_amd import models, train
    cfg, params, _ = _reg_case(reg)
    model = models.get_model(cfg["model_name"])(
        num_classes=4, box_encoding_len=7, mode="train",
        **cfg["model_kwargs"]).load_state_dict(params, dev)
    rng = np.random.default_rng(5)
    k = 50
    from test_gpu_train import T
    d = model.loss(T(rng.standard_normal((k, 4)).astype(np.float32), dev),
                   T(rng.integers(0, 4, (k, 1)).astype(np.int32), dev),
                   T(rng.standard_normal((k, 4, 7)).astype(np.float32), dev),
                   T(rng.standard_normal((k, 1, 7)).astype(np.float32), dev),
                   T(np.ones((k, 1, 1), np.float32), dev),
                   cls_loss_type='softmax', loc_loss_type='huber_loss',
                   loc_loss_weight=10.0, cls_loss_weight=0.1)
    want = th.reg_loss(params, cfg)
    print(reg[0], "models.loss reg_loss %.9g (float64 %.9g)" % (d['reg_loss'],
                                                                want))
    assert want > 1.0       # (visible next to the data terms)
    assert abs(d['reg_loss'] - want) < 1e-5 * max(1, want)
    tr = train.Trainer(cfg, params=params, device=dev)
    assert abs(tr.reg_loss() - want) < 1e-5 * max(1, want)


@pytest.mark.parametrize("reg", REGS, ids=[r[0] for r in REGS])
def test_pseudo_batch_doubles_both_regularizer_terms(dev, reg):
    """As test_pseudo_batch_accumulates_like_the_reference: the step that
    applies two summed batches carries the regularizer's gradient twice --
    the l2 term like the l1 term."""
    from pointgnn_amd import train
    cfg, params, _ = _reg_case(reg)
    l1, l2 = th.regularizer_scales(cfg)
    A, B, C = (_tiny_batch(seed=s) for s in (4, 5, 6))
    tcfg = dict(_TCFG, optimizer='sgd', is_pseudo_batch=True,
                pseudo_batch_factor=2)
    tr = train.Trainer(cfg, train_config=tcfg, params=params, device=dev)

    def regg(w, n):
        return n.endswith('/weights') * (l1 * np.sign(w) + l2 * w)
    w0 = tr.state_dict()
    _, applied = tr.pseudo_batch_step(A)
    assert applied
    g, w1 = tr.grad_dict(), tr.state_dict()
    for n in w0:
        np.testing.assert_allclose(w1[n], w0[n] - 0.01 * (g[n] + regg(w0[n], n)),
                                   atol=1e-7, rtol=1e-5)
    _, applied = tr.pseudo_batch_step(B)
    assert not applied
    _, applied = tr.pseudo_batch_step(C)
    assert applied and tr.global_step == 2
    g_sum, w2 = tr.grad_dict(), tr.state_dict()
    for n in w1:
        np.testing.assert_allclose(
            w2[n], w1[n] - 0.01 * (g_sum[n] + 2 * regg(w1[n], n)), atol=1e-7,
            rtol=1e-5)


def test_regularizer_arguments(dev):
    from pointgnn_amd import train
    base = configs.car_auto_config(1)
    for reg in (('l2', {'scale': 1e-2, 'scale_l2': 1.0}),
                ('l1_l2', {'scale': 1e-2}), ('l1', {'scales': 1e-2})):
        with pytest.raises(ValueError):
            train.Trainer(th.head_config(base, 'classaware_predictor',
                                         regularizer=reg), device=dev)
    tr = train.Trainer(th.head_config(base, 'classaware_predictor',
                                      regularizer=('l1_l2', {})), device=dev)
    assert (tr.l1_scale, tr.l2_scale) == (1.0, 1.0)
    tr = train.Trainer(base, device=dev)
    assert (tr.l1_scale, tr.l2_scale) == (5e-7, 0.0)


@pytest.mark.parametrize("opt", ["sgd", "momentum", "rmsprop", "adam"])
def test_l1_step_is_the_same_through_the_old_and_the_new_entry(dev, opt):
    """'l1' with its shipped scale: pgnn_sgd_step / pgnn_optimizer_step and
    their two-scale siblings with l2 = 0 write the same bits."""
    import ctypes
    import torch
    from pointgnn_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(9)
    n = 100003
    w = rng.standard_normal(n).astype(np.float32)
    w[::97] = 0.0
    g = (1e-3 * rng.standard_normal(n)).astype(np.float32)
    mask = (rng.random(n) < 0.9).astype(np.float32)
    st = _lib.stream_ptr()
    cf = ctypes.c_float
    kind = {'sgd': 0, 'momentum': 1, 'rmsprop': 2, 'adam': 3}[opt]
    h = {'sgd': (), 'momentum': (0.9, 0.0, 0.0), 'rmsprop': (0.9, 0.9, 1.0),
         'adam': (0.9, 0.999, 1e-8)}[opt]
    res = []
    for new in (False, True):
        wd, gd, md = (torch.from_numpy(a.copy()).to(dev) for a in (w, g, mask))
        s0 = torch.full_like(wd, 1.0 if opt == 'rmsprop' else 0.0)
        s1 = torch.zeros_like(wd)
        scales = [cf(0.125), cf(1.0), cf(5e-7)] + ([cf(0.0)] if new else [])
        for _ in range(2):
            if kind == 0:
                fn = lib.pgnn_sgd_step_l1l2 if new else lib.pgnn_sgd_step
                _lib.check(fn(_lib.ptr(wd), _lib.ptr(gd), _lib.ptr(md), n,
                              *scales, st), "sgd")
            else:
                fn = lib.pgnn_optimizer_step_l1l2 if new else \
                    lib.pgnn_optimizer_step
                _lib.check(fn(kind, _lib.ptr(wd), _lib.ptr(gd), _lib.ptr(md),
                              _lib.ptr(s0), _lib.ptr(s1), n, *scales,
                              *[cf(v) for v in h], st), "optimizer")
        res.append((wd.cpu(), s0.cpu(), s1.cpu()))
    assert not torch.equal(res[0][0], torch.from_numpy(w))
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_weight_norms_entry(dev):
    """pgnn_weight_norms = {sum |w|, sum w^2} over the weights, float64."""
    import torch
    from pointgnn_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(2)
    for n in (1, 1023, 4097, 300001):
        w = rng.standard_normal(n).astype(np.float32)
        mask = (rng.random(n) < 0.7).astype(np.float32)
        wd, md = torch.from_numpy(w).to(dev), torch.from_numpy(mask).to(dev)
        out = torch.full((3,), 7.0, dtype=torch.float64, device=dev)
        _lib.check(lib.pgnn_weight_norms(_lib.ptr(wd), _lib.ptr(md), n,
                                         _lib.ptr(out), _lib.stream_ptr()),
                   "pgnn_weight_norms")
        got = out.cpu().numpy()
        w64 = w.astype(np.float64) * mask
        # (n float64 additions in some order: n * 2^-53 relative at the worst)
        tol = n * 2.0 ** -53
        assert abs(got[0] - np.abs(w64).sum()) <= tol * np.abs(w64).sum() + 1e-300
        assert abs(got[1] - (w64 * w64).sum()) <= tol * (w64 * w64).sum() + 1e-300
        assert got[2] == 7.0
