"""The training step at the size `bench.py --train` times, against the
mask-matched float64 oracle (oracle/train_oracle.py).

tests/test_gpu_train.py holds the whole gradient to the oracle on one
352-keypoint fixture; at that size the native step (csrc/trainer.hip) never
takes the fused forwards that also write the per-edge rows
(pgnn_point_set_pooling_rows_fwd, pgnn_edge_mlp_scatter_max_rows_fwd: they
decline small inputs) nor the backward that recomputes H1 = ReLU(P[src] -
Q[dst]) from P and Q (library tunable train_h1 = 0).  Here the batches are
built the way bench.train_measure.make_frame builds them (training graph
kwargs: random keypoints, jitter, level-1 fan-in cap 256), seeded:
  car_auto_T3      two `car` frames merged by train.batch_data, the bench's
                   labels (20 % positives, classes 1-2, random boxes);
  ped_cyl_auto_T3  one `ped_dense` frame (the 512-wide pooling chain, 6
                   classes: positives spread over classes 1-5 so that every
                   box head has a gradient).
The measured figures are in profiles/train_grad_fullsize.md.
"""
import resource
import time

import numpy as np
import pytest

import pointgnn_amd  # noqa: F401
from pointgnn_amd import configs, weights
from oracle import train_oracle as to
from _train_decisions import device_decisions

pytestmark = pytest.mark.gpu

BAR = 1e-5          # max-entry error / max|g64|, every variable (the bar of
#                     test_full_gradient_matches_mask_matched_oracle)
E_F32_BAR = 2e-6    # the float32 oracle's own error: 5x under BAR

CASES = {
    # name: (preset, frames, label classes drawn from [1, hi))
    "car_auto_T3": ("car", 2, 3),
    "ped_cyl_auto_T3": ("ped_dense", 1, 6),
}


def _batch(cfg, preset, n_frames, hi, dev, seed=0):
    """bench.train_measure.make_frame + train.batch_data, seeded; returned as
    NumPy arrays (what the oracle reads; the trainer takes them too)."""
    import torch
    from pointgnn_amd import graph_gen, train
    from pointgnn_amd.synthetic import synthetic_cloud
    gen = torch.Generator(device='cpu').manual_seed(1234 + seed)
    np.random.seed(99 + seed)
    hints = graph_gen.CountHints()
    frames = []
    for i in range(n_frames):
        xyz, inten = synthetic_cloud(seed=i, preset=preset)
        x = torch.from_numpy(xyz).to(dev)
        coords, kps, edges = graph_gen.gen_multi_level_local_graph_v3_one_read(
            x, hints, **cfg['graph_gen_kwargs'])
        k = int(coords[1].shape[0])
        lab = (torch.rand(k, generator=gen) < 0.2).to(torch.int32) * \
            torch.randint(1, hi, (k,), generator=gen, dtype=torch.int32)
        lab = lab.reshape(k, 1).to(dev)
        boxes = torch.randn((k, 1, 7), generator=gen).to(dev)
        valid = (lab > 0).to(torch.float32).reshape(k, 1, 1)
        frames.append((torch.from_numpy(inten).to(dev), coords, kps, edges,
                       lab, boxes, valid))
    b = train.batch_data(frames) if n_frames > 1 else frames[0]
    npy = lambda t: t.cpu().numpy()
    return (npy(b[0]), [npy(c) for c in b[1]], [npy(k) for k in b[2]],
            [npy(e) for e in b[3]], npy(b[4]), npy(b[5]), npy(b[6]))


def _fused_forwards_accept(dev, batch, width):
    """rc of pgnn_point_set_pooling_rows_fwd and
    pgnn_edge_mlp_scatter_max_rows_fwd, one call each at the batch's own sizes
    (pooling: the car chain 4-32-64-128-300, the one that kernel has; edge
    stage: one width x width layer) -- 0 when the sizes are above the
    thresholds under which they decline."""
    import ctypes
    import torch
    from pointgnn_amd import _lib, gnn
    from pointgnn_amd.gnn import padded_width
    lib = _lib.load()
    rng = np.random.default_rng(0)
    inten, coords, kps, edges = batch[:4]
    k = int(coords[1].shape[0])
    store = gnn.ParamStore({}, device=dev)
    dims = [4, 32, 64, 128, 300]
    chain = gnn.Chain(store, [
        ((rng.standard_normal((a, b)) / np.sqrt(a)).astype(np.float32),
         (0.1 * rng.standard_normal(b)).astype(np.float32), 0)
        for a, b in zip(dims[:-1], dims[1:])])
    e0 = torch.from_numpy(np.ascontiguousarray(edges[0], np.int32)).to(dev)
    xyz = torch.from_numpy(np.ascontiguousarray(coords[0])).to(dev)
    it = torch.from_numpy(np.ascontiguousarray(inten)).to(dev)
    kd = torch.from_numpy(np.ascontiguousarray(kps[0], np.int32).reshape(-1)).to(dev)
    n0 = e0.shape[0]
    out = torch.empty((k, 304), dtype=torch.float32, device=dev)
    acts = [torch.empty((n0, w), dtype=torch.float32, device=dev)
            for w in (32, 64, 128, 304)]
    ptrs = (ctypes.c_void_p * 4)(*[a.data_ptr() for a in acts])
    rc_pool = lib.pgnn_point_set_pooling_rows_fwd(
        _lib.ptr(it), 1, _lib.ptr(xyz), _lib.ptr(kd), _lib.ptr(e0), n0, k,
        chain.array, 4, int(gnn._edges_sorted_flag(e0)), _lib.ptr(out), 304,
        ptrs, 304, _lib.stream_ptr())
    torch.cuda.synchronize()
    del acts, out
    wq = padded_width(width)
    p = torch.from_numpy(rng.standard_normal((k, wq)).astype(np.float32)).to(dev)
    q = torch.from_numpy(0.3 * rng.standard_normal((k, wq)).astype(np.float32)).to(dev)
    w = (rng.standard_normal((width, width)) / np.sqrt(width)).astype(np.float32)
    bb = (0.1 * rng.standard_normal(width)).astype(np.float32)
    ch1 = gnn.Chain(store, [(w, bb, 0)])
    e1 = torch.from_numpy(np.ascontiguousarray(edges[1], np.int32)).to(dev)
    n1 = e1.shape[0]
    out = torch.empty((k, wq), dtype=torch.float32, device=dev)
    rows = torch.empty((n1, wq), dtype=torch.float32, device=dev)
    rc_edge = lib.pgnn_edge_mlp_scatter_max_rows_fwd(
        _lib.ptr(p), _lib.ptr(q), wq, width, _lib.ptr(e1), n1, k, ch1.array,
        int(gnn._edges_sorted_flag(e1)), _lib.ptr(out), wq, _lib.ptr(rows), wq,
        None, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc_pool, rc_edge


def _worst(got, ref):
    """max over variables of max|got - ref| / max|ref|."""
    w = 0.0
    for n, r in ref.items():
        w = max(w, float(np.abs(got[n] - r).max() / (np.abs(r).max() + 1e-12)))
    return w


# (batch, params, float64 gradients, oracle losses) per config: the oracle run
# is the expensive part and the geometry cases below hold to the same one
_ORACLE = {}


@pytest.mark.parametrize("name", list(CASES))
def test_full_size_gradient_matches_mask_matched_oracle(name):
    """The gradient of every variable at the benchmarked batch size, with the
    device forward's own ReLU masks and arg-max winners replayed in the
    float64 oracle: native step with train_h1 = 1 (the backward reads the H1
    rows the fused forward wrote) and train_h1 = 0 (it recomputes them from P
    and Q), the Python-driven sparse adjoint and the dense adjoint.  Every
    entry within 1e-5 of its variable's max|g64|; losses identical between the
    four and within 1e-5 of the oracle's.  The bar means something only well
    above the oracle's own float32 noise: the same oracle in float32 with the
    same decisions (e_f32) must stay under 2e-6."""
    import torch
    from pointgnn_amd import _lib, train
    dev = torch.device("cuda")
    _lib.load()
    cfg = configs.get_config(name)
    preset, n_frames, hi = CASES[name]
    batch = _batch(cfg, preset, n_frames, hi, dev)
    k = int(batch[1][1].shape[0])
    e0, e1 = int(batch[3][0].shape[0]), int(batch[3][1].shape[0])
    print("\n[fullsize] %s: preset %s x%d  N %d  K %d  E0 %d  E1 %d  "
          "positives %d" % (name, preset, n_frames, batch[1][0].shape[0], k,
                            e0, e1, int((batch[4] > 0).sum())), flush=True)
    width = cfg['model_kwargs']['layer_configs'][1]['kwargs'][
        'edge_MLP_depth_list'][-1]
    rc_pool, rc_edge = _fused_forwards_accept(dev, batch, width)
    assert rc_pool == 0 and rc_edge == 0, (
        "the INPUT is too small, not the device at fault: the fused "
        "rows-writing forwards decline E0 %d / E1 %d (rc %d / %d)" % (
            e0, e1, rc_pool, rc_edge))
    params = weights.init_params(cfg, seed=5, bias_scale=0.1)
    tr = train.Trainer(cfg, params=params, device=dev)
    tr.native = False
    tr.forward(*batch[:4])
    masks = device_decisions(tr, cfg)
    del tr
    torch.cuda.empty_cache()
    dec = to.Decisions(masks)
    t0 = time.perf_counter()
    loss, g64, _ = to.step_gradients(params, cfg, [batch], decisions=[dec])
    t_oracle = time.perf_counter() - t0
    assert dec.pos == len(masks), (
        "the INPUT, not the device: %d of %d decision sites used" % (
            dec.pos, len(masks)))
    flips = dec.flips()
    dec32 = to.Decisions(masks)
    _, g32, _ = to.step_gradients(params, cfg, [batch], dtype=torch.float32,
                                  decisions=[dec32])
    assert dec32.pos == len(masks)
    e_f32 = _worst(g32, g64)
    del g32
    rss_gb = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2.0 ** 20
    print("[fullsize] %s: %d of %d decisions differ from the float64 "
          "forward's own (per site: %s); float64 oracle %.1f s, peak RSS "
          "%.1f GB; e_f32 %.3g" % (name, sum(flips), sum(m.size for m in masks),
                                   [f for f in flips if f], t_oracle, rss_gb,
                                   e_f32), flush=True)
    assert e_f32 <= E_F32_BAR, (
        "the oracle's own float32 error %.3g leaves no margin under the "
        "bar" % e_f32)
    worst, losses, errors = {}, {}, {}
    for mode, native, sparse, h1 in (("native_h1", True, True, 1),
                                     ("native_pq", True, True, 0),
                                     ("python", False, True, 1),
                                     ("dense", False, False, 1)):
        _lib.set_tunable("train_h1", h1)
        try:
            t2 = train.Trainer(cfg, params=params, device=dev)
            t2.native, t2.sparse_adjoint = native, sparse
            out = t2.train_step(batch, apply=False)
            got = t2.grad_dict()
        finally:
            _lib.set_tunable("train_h1", 1)
        assert (getattr(t2._native_step, 'handle', None) is not None) == native
        del t2
        losses[mode] = (out['cls_loss'], out['loc_loss'])
        errors[mode] = {n: float(np.abs(got[n] - r).max() /
                                 (np.abs(r).max() + 1e-12))
                        for n, r in g64.items()}
        worst[mode] = max(errors[mode].values())
        wn = max(errors[mode], key=errors[mode].get)
        at = np.unravel_index(np.argmax(np.abs(got[wn] - g64[wn])),
                              g64[wn].shape)
        print("[fullsize] %s %s: worst entry error %.3g (%s %s of %s); "
              "losses %r" % (name, mode, worst[mode], wn, tuple(map(int, at)),
                             g64[wn].shape, losses[mode]), flush=True)
    print("[fullsize] %s: oracle losses cls %r loc %r" % (
        name, loss['cls_loss'], loss['loc_loss']), flush=True)
    for mode, errs in errors.items():
        for i, key in enumerate(('cls_loss', 'loc_loss')):
            assert abs(losses[mode][i] - loss[key]) <= 1e-5 * abs(loss[key]), (
                mode, key, losses[mode][i], loss[key])
        for n, e in errs.items():
            assert e <= BAR, "%s %s: max-entry rel err %.3g" % (mode, n, e)
    assert len(set(losses.values())) == 1, losses
    _ORACLE[name] = (batch, params, g64, loss)


def _oracle(name, dev):
    """The cached oracle of the test above, or -- this test run alone -- the
    same computation: the Python forward's decisions replayed in float64."""
    import torch
    from pointgnn_amd import train
    if name not in _ORACLE:
        cfg = configs.get_config(name)
        preset, n_frames, hi = CASES[name]
        batch = _batch(cfg, preset, n_frames, hi, dev)
        params = weights.init_params(cfg, seed=5, bias_scale=0.1)
        tr = train.Trainer(cfg, params=params, device=dev)
        tr.native = False
        tr.forward(*batch[:4])
        masks = device_decisions(tr, cfg)
        del tr
        torch.cuda.empty_cache()
        dec = to.Decisions(masks)
        loss, g64, _ = to.step_gradients(params, cfg, [batch], decisions=[dec])
        assert dec.pos == len(masks)
        _ORACLE[name] = (batch, params, g64, loss)
    return _ORACLE[name]


def _native_step(cfg, params, batch, dev):
    """One native car step on the current stream -> (the workspace as the
    forward left it, gradients, losses).  The workspace holds everything the
    forward saves for the backward -- the per-edge rows (`rows_out`), the
    gathered hidden rows (`h1_out`), the pooling activations -- and is zeroed
    first, so that two forwards can be compared byte for byte."""
    from pointgnn_amd import train
    t2 = train.Trainer(cfg, params=params, device=dev)
    t2.native, t2.sparse_adjoint = True, True
    t2.forward(*batch[:4])            # sizes the workspace
    assert t2._native_step.handle is not None
    t2._native_step.workspace.zero_()
    t2.forward(*batch[:4])
    saved = t2._native_step.workspace.clone()
    out = t2.train_step(batch, apply=False)
    got = t2.grad_dict()
    del t2
    return saved, got, (out['cls_loss'], out['loc_loss'])


def test_native_step_at_other_ws_geometries():
    """The training forward forms of the weights-stationary kernels
    (edge_ws_kernel<.., EMIT> with rows_out / h1_out, pool_ws_kernel<true>) at
    two more grid geometries: `ws_reserve` = 64 (192 workgroups) and 4 row
    slices on a 240-CU stream.  The bar of the test above, unchanged -- every
    variable within 1e-5 of max|g64| of the mask-matched float64 oracle --,
    and what the forward saves is bit-equal to the default geometry's: rows,
    hidden rows and activations are per-row quantities with no cross-wave
    sums."""
    import torch
    from pointgnn_amd import _lib
    import _ws_cases as wc
    dev = torch.device("cuda")
    _lib.load()
    name = "car_auto_T3"
    cfg = configs.get_config(name)
    batch, params, g64, loss = _oracle(name, dev)
    base, _, base_losses = _native_step(cfg, params, batch, dev)
    again, _, _ = _native_step(cfg, params, batch, dev)
    assert again.numel() == base.numel() and torch.equal(again, base), \
        "the forward's workspace is not reproducible at ONE geometry"
    del again
    for geo in (wc.DEFAULT._replace(reserve=64),
                wc.DEFAULT._replace(stream=240, xcds=4)):
        with wc.masked_stream(geo.stream) as stream, wc.tunables(geo), \
                torch.cuda.stream(stream):
            assert _fused_forwards_accept(dev, batch, 300) == (0, 0), \
                "the fused rows-writing forwards decline at %s" % wc.geo_id(geo)
            saved, got, losses = _native_step(cfg, params, batch, dev)
            stream.synchronize()
            same = saved.numel() == base.numel() and torch.equal(saved, base)
            del saved
        errs = {n: float(np.abs(got[n] - r).max() / (np.abs(r).max() + 1e-12))
                for n, r in g64.items()}
        wn = max(errs, key=errs.get)
        print("[fullsize] %s native step at %s: worst entry error %.3g (%s); "
              "losses %r; saved activations %s" % (
                  name, wc.geo_id(geo), errs[wn], wn, losses,
                  "bit-equal" if same else "DIFFER"), flush=True)
        assert same, "saved activations differ at %s" % wc.geo_id(geo)
        for i, key in enumerate(('cls_loss', 'loc_loss')):
            assert abs(losses[i] - loss[key]) <= 1e-5 * abs(loss[key]), (
                wc.geo_id(geo), key, losses[i], loss[key])
        assert losses == base_losses, (wc.geo_id(geo), losses, base_losses)
        for n, e in errs.items():
            assert e <= BAR, "%s %s: max-entry rel err %.3g" % (
                wc.geo_id(geo), n, e)
