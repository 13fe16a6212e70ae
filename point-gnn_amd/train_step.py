"""The two engines of a training step and the rule that picks one.

  NativeStep    csrc/trainer.hip: forward and backward are one C call each.
  ComposedStep  the same primitives driven from Python, one C call per layer
                (the readable composition; tests hold the two to the same
                gradients).

Both work on the trainer's flat parameter and gradient buffers and offer
    forward(input_v, coords, kps, edges) -> (logits[:, :nc], pred, state)
    backward(state, dlogits, dpred, sync_sums) -> synced
    repack()
`state`: what the engine's backward needs of its forward.
"""
import collections
import ctypes
import warnings
import weakref

import numpy as np
import torch

from . import _lib, gnn
from .gnn import padded_width
from .weights import mlp_names


class StepEngine(object):
    """The ONE stale bit of an engine's weight images.  An engine implements
    _repack() (refresh every image from the flat buffer), _forward(...) and
    backward(...)."""
    _stale = True

    def mark_stale(self):        # the flat buffer changed
        self._stale = True

    def repack(self):
        self._repack()
        self._stale = False

    def forward(self, input_v, coords, kps, edges):
        if self._stale:
            self.repack()
        return self._forward(input_v, coords, kps, edges)


class StepSelector(object):
    """Which engine runs a step.  The subclass has `native`, `sparse_adjoint`
    (plain attributes: callers flip them between steps), `_native_step` (None
    until a native forward is asked for), `_composed_step`, `_saved`, and
    _create_native_step() -> engine, or None for a model it does not take."""

    def _engine(self):
        """The engine of the next forward: the native one when `native and
        sparse_adjoint` and the model has one, else the composed one."""
        if self.native and self.sparse_adjoint:
            if self._native_step is None:
                self._native_step = self._create_native_step()
            if self._native_step is not None:
                return self._native_step
            self.native = False
        return self._composed_step

    def forward(self, input_v, coords, kps, edges):
        """Returns (logits [K,nc], pred_box [K,nc,L]) and keeps what backward
        needs in self._saved."""
        eng = self._engine()
        logits, pred, state = eng.forward(input_v, coords, kps, edges)
        self._saved = (eng, state)
        return logits, pred

    def backward(self, dlogits, dpred, sync_sums=None):
        """Gradients of the last forward into self.grad.  sync_sums (the loss
        sums of a multi-rank step): with a Communicator and the native step the
        all-reduce of (self.grad, sync_sums) is enqueued by the same C call;
        returns True when that happened (the caller reduces otherwise)."""
        eng, state = self._saved
        synced = eng.backward(state, dlogits, dpred, sync_sums)
        self._saved = None
        return synced

    def repack(self):
        """Refresh the device images derived from the flat buffer (MFMA
        fragment images, plain W^T of the sparse-adjoint layers) -- after
        every optimizer step: ONE launch, for the engine in use.  The other
        engine refreshes at its next forward, a new native one as it binds."""
        for eng in (self._native_step, self._composed_step):
            if eng is not None:
                eng.mark_stale()
        eng = self._native_step if self.native and self.sparse_adjoint \
            else self._composed_step
        if eng is not None:
            eng.repack()


def _stage_layers(lc):
    """(is pooling, a, b, c): the layer names of a pooling / GNN stage's
    config -- a: the per-edge layers, b: the per-vertex layers behind the
    scatter-max, c: the auto-offset layers of a GNN stage (None without)."""
    kw, scope = lc['kwargs'], lc['scope']
    pool = lc['type'] == 'scatter_max_point_set_pooling'
    if not pool and lc['type'] != 'scatter_max_graph_auto_center_net':
        raise NotImplementedError(lc['type'])
    a = mlp_names(scope + '/extract_vertex_features', len(
        kw['point_MLP_depth_list' if pool else 'edge_MLP_depth_list']))
    b = mlp_names(scope + '/combined_features', len(
        kw['output_MLP_depth_list' if pool else 'update_MLP_depth_list']))
    c = None
    if not pool and kw['auto_offset']:
        c = mlp_names(scope, len(kw['auto_offset_MLP_depth_list']))
    return pool, a, b, c


class _TrainerStep(StepEngine):
    """What both engines take from their trainer."""

    def __init__(self, trainer):
        # (a proxy: no cycle keeps the buffers of a dropped trainer alive)
        self.tr = weakref.proxy(trainer)
        self.lib, self.device = trainer.lib, trainer.device
        self.config, self.fc = trainer.config, trainer.fc
        self.nc, self.box_len = trainer.nc, trainer.box_len
        self._head_slice = trainer._head_slice

    def _st(self):
        return _lib.stream_ptr()

    def _batch_tensors(self, input_v, coords, kps, edges):
        """float32 / int32 contiguous device tensors of a batch's graph; edge
        lists tagged with whether they are grouped by ascending dst (a foreign
        list is checked once, and takes the all-atomic scatter-max if not)."""
        dev = self.device
        f32 = lambda t: torch.as_tensor(t).to(
            device=dev, dtype=torch.float32).contiguous()
        i32 = lambda t: torch.as_tensor(t).to(
            device=dev, dtype=torch.int32).contiguous()
        flags = [int(gnn._edges_sorted_flag(torch.as_tensor(e)))
                 for e in edges]
        return (f32(input_v), [f32(c) for c in coords],
                [i32(torch.as_tensor(k).reshape(-1)) for k in kps],
                [gnn.mark_sorted(i32(e), f) for e, f in zip(edges, flags)])


# ---- native step (csrc/trainer.hip) ----------------------------------------------
class NativeStep(_TrainerStep):
    workspace = None

    @classmethod
    def create(cls, trainer):
        """pgnn_trainer_create + bind for the trainer's model; None (and a
        RuntimeWarning) for layer shapes outside what csrc/trainer.hip
        orchestrates: the composition of the same primitives takes those."""
        lib = trainer.lib

        def fc_ref(dst, name):
            off_w, (k, n) = trainer.offsets[name + '/weights']
            off_b, _ = trainer.offsets[name + '/biases']
            dst.w_off, dst.b_off = off_w, off_b
            dst.k_in, dst.n_out = int(k), int(n)

        m = _lib.TrainModel()
        lcs = trainer.config['model_kwargs']['layer_configs']
        m.n_stages = len(lcs) - 1
        m.num_classes, m.box_len = trainer.nc, trainer.box_len
        m.n_params = int(trainer.flat.numel())
        for si, lc in enumerate(lcs[:-1]):
            st = m.stages[si]
            st.graph_level = int(lc['graph_level'])
            pool, a, b, c = _stage_layers(lc)
            st.kind = 0 if pool else 1
            st.n_a, st.n_b, st.n_c = len(a), len(b), len(c or [])
            for arr, names in ((st.a, a), (st.b, b), (st.c, c or [])):
                for i, n in enumerate(names):
                    fc_ref(arr[i], n)
        pc = lcs[-1]
        m.loc_split = int(trainer._head_slice is not None)
        ps = pc['scope'] + '/predictor'
        for i, n in enumerate(mlp_names(ps + '/cls', 2)):
            fc_ref(m.cls[i], n)
        for j in range(trainer.nc):
            for i, n in enumerate(mlp_names(ps + '/loc/cls_%d' % j, 3)):
                fc_ref(m.loc[j][i], n)
        h = ctypes.c_void_p()
        rc = lib.pgnn_trainer_create(ctypes.byref(m), ctypes.byref(h))
        if rc == _lib.E_UNSUPPORTED:
            warnings.warn("native training step unavailable for this model "
                          "(%s); using the Python-driven step" % (
                              (lib.pgnn_last_error() or b'?').decode(),),
                          RuntimeWarning)
            return None
        _lib.check(rc, "pgnn_trainer_create")
        self = cls(trainer)
        self.handle = h
        self.images = torch.empty(int(lib.pgnn_trainer_images_bytes(h)),
                                  dtype=torch.uint8, device=self.device)
        _lib.check(lib.pgnn_trainer_bind(
            h, _lib.ptr(trainer.flat), _lib.ptr(trainer.grad),
            _lib.ptr(self.images), self.images.numel(), self._st()),
            "pgnn_trainer_bind")
        self._stale = False      # (bind packs the images)
        return self

    def destroy(self):
        h, self.handle = self.handle, None
        if h is not None:
            self.lib.pgnn_trainer_destroy(h)

    def _repack(self):
        _lib.check(self.lib.pgnn_trainer_repack(self.handle, self._st()),
                   "pgnn_trainer_repack")

    def batch(self, input_v, coords, kps, edges):
        """pgnn_train_batch for these tensors, and the converted tensors its
        pointers address (kept alive by the caller)."""
        keep = self._batch_tensors(input_v, coords, kps, edges)
        input_v, coords, kps, edges = keep
        b = _lib.TrainBatch()
        b.input_v, b.n_feat = input_v.data_ptr(), int(input_v.shape[1])
        b.n_levels = len(edges)
        for l, c in enumerate(coords):
            b.n_vertices[l], b.coords[l] = int(c.shape[0]), c.data_ptr()
        for l, e in enumerate(edges):
            b.keypoints[l] = kps[l].data_ptr()
            b.edges[l], b.n_edges[l] = e.data_ptr(), int(e.shape[0])
            b.edges_sorted[l] = e._pgnn_sorted
        return b, keep

    def _forward(self, input_v, coords, kps, edges):
        lib, h = self.lib, self.handle
        batch, keep = self.batch(input_v, coords, kps, edges)
        need = int(lib.pgnn_trainer_workspace_bytes(h, ctypes.byref(batch)))
        if need == 0:
            raise _lib.PointGnnHipError("pgnn_trainer_workspace_bytes: %s" % (
                (lib.pgnn_last_error() or b'?').decode()))
        if self.workspace is None or self.workspace.numel() < need:
            self.workspace = torch.empty(
                (int(need * 1.25) + 255) // 256 * 256, dtype=torch.uint8,
                device=self.device)
        lg, ld, pb = ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_void_p()
        _lib.check(lib.pgnn_trainer_forward(
            h, ctypes.byref(batch), _lib.ptr(self.workspace),
            self.workspace.numel(), ctypes.byref(lg), ctypes.byref(ld),
            ctypes.byref(pb), self._st()), "pgnn_trainer_forward")
        k = int(batch.n_vertices[batch.n_levels])
        # views INTO the workspace (valid until the next forward)
        base = self.workspace.data_ptr()
        flat = self.workspace.view(torch.float32)
        o_lg = (lg.value - base) // 4
        o_pb = (pb.value - base) // 4
        logits = flat[o_lg:o_lg + k * ld.value].view(k, ld.value)
        pred = flat[o_pb:o_pb + k * self.nc * self.box_len].view(
            k, self.nc, self.box_len)
        return logits[:, :self.nc], pred, (batch, keep)

    def backward(self, state, dlogits, dpred, sync_sums=None):
        batch, keep = state
        dl = dlogits.contiguous()
        dp = dpred.contiguous()
        # (read now, never kept: the owner may drop its communicator)
        comm = self.tr.comm
        sync = sync_sums is not None and comm is not None
        _lib.check(self.lib.pgnn_trainer_backward_sync(
            self.handle, ctypes.byref(batch), _lib.ptr(self.workspace),
            self.workspace.numel(), _lib.ptr(dl), _lib.ptr(dp),
            comm.handle if sync else None,
            _lib.ptr(sync_sums) if sync else None,
            sync_sums.numel() if sync else 0, self._st()),
            "pgnn_trainer_backward_sync")
        return sync


# ---- the composition of the primitives ---------------------------------------------
# What ComposedStep.forward saves of a stage for its backward (and the tests
# read the device's ReLU masks and arg-max picks from).
PoolStage = collections.namedtuple(
    'PoolStage', 'names acts dst agg onames oacts upper')
GnnStage = collections.namedtuple(
    'GnnStage', 'enames hx xo e eacts dst agg unames uacts off_names '
    'off_acts c')
Heads = collections.namedtuple('Heads', 'cls_names cacts loc')


class ComposedStep(_TrainerStep):
    _ws = _ws2 = _pack_jobs = None     # two scratch buffers, the job table

    def _build_pack_jobs(self):
        """Device table of pgnn_pack_fc_many: the fragment images (forward,
        transposed) of every layer, the W^T rows of the Wx block of each first
        edge layer (dx' = dQ Wx^T), plain W^T of the sparse-adjoint layers."""
        lib = self.lib
        stages = [_stage_layers(lc) for lc in
                  self.config['model_kwargs']['layer_configs'][:-1]]
        # the layers whose output feeds a scatter-max (the last per-edge layer
        # of every stage): their adjoint runs sparse (pgnn_segmax_fc_bwd_f32)
        # and needs a plain W^T image -- and a materialised input activation
        sparse = set(a[-1] for _, a, _, _ in stages if len(a) >= 2)
        jobs = []
        self._pack_blocks = 0

        def add(w_ptr, b_ptr, dst, k_in, n_out, kind):
            if kind == 2:
                elems = n_out * padded_width(k_in)
            elif kind == 1:
                elems = lib.pgnn_packed_fc_floats(n_out, k_in)
            else:
                elems = lib.pgnn_packed_fc_floats(k_in, n_out)
            j = _lib.PackJob()
            j.w, j.b, j.dst = w_ptr, b_ptr or None, dst.data_ptr()
            j.k_in, j.n_out, j.kind = int(k_in), int(n_out), int(kind)
            j.first_block = self._pack_blocks
            self._pack_blocks += (int(elems) + 255) // 256
            jobs.append(j)
        for fc in self.fc.values():
            fc.packed = torch.empty(
                lib.pgnn_packed_fc_floats(fc.k_in, fc.n_out),
                dtype=torch.float32, device=self.device)
            fc.packed_t = torch.empty(
                lib.pgnn_packed_fc_floats(fc.n_out, fc.k_in),
                dtype=torch.float32, device=self.device)
            add(fc.w.data_ptr(), fc.b.data_ptr(), fc.packed, fc.k_in,
                fc.n_out, 0)
            add(fc.w.data_ptr(), 0, fc.packed_t, fc.k_in, fc.n_out, 1)
            if fc.name in sparse:
                fc.wt = torch.empty((fc.n_out, padded_width(fc.k_in)),
                                    dtype=torch.float32, device=self.device)
                add(fc.w.data_ptr(), 0, fc.wt, fc.k_in, fc.n_out, 2)
        # Wx = rows c..c+2 of every first edge layer, transposed image
        self.wx_packed_t = {}
        for pool, a, _, _ in stages:
            if pool:
                continue
            name = a[0]
            w1 = self.fc[name]
            c = w1.k_in - 3
            pk = torch.empty(lib.pgnn_packed_fc_floats(w1.n_out, 3),
                             dtype=torch.float32, device=self.device)
            add(w1.w.data_ptr() + 4 * c * w1.n_out, 0, pk, 3, w1.n_out, 1)
            self.wx_packed_t[name] = pk
        arr = (_lib.PackJob * len(jobs))(*jobs)
        raw = np.frombuffer(bytes(arr), dtype=np.uint8).copy()
        self._pack_jobs = torch.from_numpy(raw).to(self.device)
        self._pack_n = len(jobs)

    def _repack(self):
        if self._pack_jobs is None:
            self._build_pack_jobs()
        _lib.check(self.lib.pgnn_pack_fc_many(
            _lib.ptr(self._pack_jobs), self._pack_n, self._pack_blocks,
            self._st()), "pgnn_pack_fc_many")

    def _mlp1(self, packed, k_in, n_out, relu, x, nx, x2=None, nx2=0,
              residual=None):
        rows = int(x.shape[0])
        y = torch.empty((rows, padded_width(n_out)), dtype=torch.float32,
                        device=self.device)
        arr = (_lib.FcLayer * 1)()
        arr[0].packed = packed.data_ptr()
        arr[0].k_in, arr[0].n_out = int(k_in), int(n_out)
        arr[0].relu_from = 0 if relu else int(n_out)
        _lib.check(self.lib.pgnn_mlp_fwd(
            _lib.ptr(x), x.stride(0), int(nx), _lib.ptr(x2),
            x2.stride(0) if x2 is not None else 0, int(nx2), rows, arr, 1,
            _lib.ptr(residual),
            residual.stride(0) if residual is not None else 0, _lib.ptr(y),
            y.stride(0), self._st()), "pgnn_mlp_fwd")
        return y

    def fc_fwd(self, name, x, relu, x2=None, nx2=0, residual=None):
        fc = self.fc[name]
        return self._mlp1(fc.packed, fc.k_in, fc.n_out, relu, x,
                          fc.k_in - nx2, x2, nx2, residual)

    def _weight_grad(self, x, ld_x, k_in, dz, n_out, gw_ptr, gb_ptr):
        rows = int(dz.shape[0])
        need = self.lib.pgnn_weight_grad_workspace_bytes(k_in, n_out, rows)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(int(need), dtype=torch.uint8,
                                   device=self.device)
        _lib.check(self.lib.pgnn_weight_grad_f32(
            _lib.ptr(x), ld_x, k_in, _lib.ptr(dz), dz.stride(0), n_out, rows,
            gw_ptr, gb_ptr, 1, _lib.ptr(self._ws), self._ws.numel(),
            self._st()), "pgnn_weight_grad_f32")

    def fc_bwd(self, name, x, y, dy, relu, need_dx=True):
        """dy is consumed (masked in place when relu).  x: the saved input
        [rows, >= k_in] (already concatenated for two-input layers)."""
        fc = self.fc[name]
        if relu:
            _lib.check(self.lib.pgnn_relu_mask_mul(
                _lib.ptr(dy), _lib.ptr(y), dy.numel(), self._st()),
                "pgnn_relu_mask_mul")
        self._weight_grad(x, x.stride(0), fc.k_in, dy, fc.n_out,
                          _lib.ptr(fc.gw), _lib.ptr(fc.gb))
        if not need_dx:
            return None
        return self._mlp1(fc.packed_t, fc.n_out, fc.k_in, False, dy, fc.n_out)

    def _chain_bwd(self, names, acts, d, relu_last):
        """fc_bwd through a chain of layers (acts[i] -> acts[i + 1]) that all
        end in a ReLU -- the last one only with relu_last."""
        for i in range(len(names) - 1, -1, -1):
            d = self.fc_bwd(names[i], acts[i], acts[i + 1], d,
                            relu_last or i + 1 < len(names))
        return d

    def _scatter_max(self, data, dst, k):
        out = torch.empty((k, data.shape[1]), dtype=torch.float32,
                          device=self.device)
        _lib.check(self.lib.pgnn_scatter_max_f32(
            _lib.ptr(data), data.stride(0), _lib.ptr(dst), int(data.shape[0]),
            int(data.shape[1]), k, _lib.ptr(out), out.stride(0),
            int(getattr(dst, "_pgnn_sorted", 0)), self._st()),
            "pgnn_scatter_max_f32")
        return out

    def _scatter_max_bwd(self, data, dst, out, gout):
        """Dense adjoint of out = scatter_max(data) for `data` that left a
        ReLU: relu_mask = 1 whatever the order of the ids (rows tied at a
        maximum of exactly 0 get nothing, TF's ReluGrad; both callers hand
        the result to fc_bwd(..., relu=False) as dZ)."""
        k, cols = int(out.shape[0]), int(data.shape[1])
        ties = torch.empty(k * cols, dtype=torch.int32, device=self.device)
        gdata = torch.empty_like(data)
        _lib.check(self.lib.pgnn_scatter_max_bwd_f32(
            _lib.ptr(data), data.stride(0), _lib.ptr(dst), int(data.shape[0]),
            cols, k, _lib.ptr(out), out.stride(0), _lib.ptr(gout),
            gout.stride(0), _lib.ptr(ties), _lib.ptr(gdata), gdata.stride(0),
            1, self._st()), "pgnn_scatter_max_bwd_f32")
        return gdata

    def _segmax_fc_bwd(self, name, y, dst, out, gout, x, need_dx=True,
                       mask_x=True):
        """Adjoint of out = scatter_max(y), y = ReLU(x W + b) for layer `name`
        (pgnn_segmax_fc_bwd_f32): accumulates dW / db, returns dX (masked by
        x > 0) or None."""
        fc = self.fc[name]
        rows, k = int(y.shape[0]), int(out.shape[0])
        need = self.lib.pgnn_segmax_fc_bwd_workspace_bytes(rows, fc.n_out, k,
                                                           fc.k_in)
        if self._ws2 is None or self._ws2.numel() < need:
            self._ws2 = torch.empty(int(need), dtype=torch.uint8,
                                    device=self.device)
        dx = None
        if need_dx:
            dx = torch.empty((rows, int(x.shape[1])), dtype=torch.float32,
                             device=self.device)
        _lib.check(self.lib.pgnn_segmax_fc_bwd_f32(
            _lib.ptr(y), y.stride(0), _lib.ptr(dst), rows, fc.n_out, k,
            _lib.ptr(out), out.stride(0), _lib.ptr(gout), gout.stride(0),
            _lib.ptr(x), x.stride(0), fc.k_in, _lib.ptr(fc.wt),
            fc.wt.stride(0), _lib.ptr(dx),
            dx.stride(0) if dx is not None else 0,
            int(x.shape[1]) if dx is not None else 0, 1 if mask_x else 0,
            _lib.ptr(fc.gw), _lib.ptr(fc.gb), _lib.ptr(self._ws2),
            self._ws2.numel(), self._st()), "pgnn_segmax_fc_bwd_f32")
        return dx

    def _max_bwd(self, sparse, names, acts, s, gout, **kw):
        """Adjoint of a stage's scatter-max -> (g, index of the first layer
        left to differentiate densely).  Sparse: together with the last
        per-edge layer (g is the gradient w.r.t. that layer's input, already
        ReLU-masked); dense: g is the gradient w.r.t. its output rows."""
        if sparse and self.fc[names[-1]].wt is not None:
            return self._segmax_fc_bwd(names[-1], acts[-1], s.dst, s.agg,
                                       gout, acts[-2], **kw), len(names) - 2
        return (self._scatter_max_bwd(acts[-1], s.dst, s.agg, gout),
                len(names) - 1)

    # ---- forward with saved activations ------------------------------------------
    def _forward(self, input_v, coords, kps, edges):
        lib, st = self.lib, self._st()
        dev = self.device
        input_v, coords, kps, edges = self._batch_tensors(input_v, coords, kps,
                                                          edges)
        saved = []
        h = None
        for lc in self.config['model_kwargs']['layer_configs'][:-1]:
            lvl = lc['graph_level']
            pool, names, onames, off_names = _stage_layers(lc)
            if pool:
                e = edges[lvl]
                k = int(kps[lvl].shape[0])
                upper = None
                if h is None:
                    feat = torch.empty((int(e.shape[0]), 16),
                                       dtype=torch.float32, device=dev)
                    _lib.check(lib.pgnn_pool_features_fwd(
                        _lib.ptr(input_v), int(input_v.shape[1]),
                        _lib.ptr(coords[lvl]), _lib.ptr(kps[lvl]), _lib.ptr(e),
                        int(e.shape[0]), _lib.ptr(feat), st),
                        "pgnn_pool_features_fwd")
                else:
                    # a pooling level above the first (models.py:119-149 is
                    # generic; no shipped config has one): the edge rows
                    # [h[src], x[src] - x[kp[dst]]] of the previous level's
                    # features are materialised, as gnn.PointSetPooling's
                    # wide-feature path does
                    n_feat = self.fc[names[0]].k_in - 3
                    feat = torch.empty((int(e.shape[0]),
                                        padded_width(n_feat + 3)),
                                       dtype=torch.float32, device=dev)
                    _lib.check(lib.pgnn_pool_features_wide_fwd(
                        _lib.ptr(h), h.stride(0), n_feat,
                        _lib.ptr(coords[lvl]), _lib.ptr(kps[lvl]), _lib.ptr(e),
                        int(e.shape[0]), _lib.ptr(feat), feat.stride(0), st),
                        "pgnn_pool_features_wide_fwd")
                    upper = (e, n_feat, int(h.shape[0]), int(h.shape[1]))
                acts = [feat]
                for n in names:
                    acts.append(self.fc_fwd(n, acts[-1], True))
                dst = gnn.mark_sorted(e[:, 1].contiguous(), e._pgnn_sorted)
                agg = self._scatter_max(acts[-1], dst, k)
                oacts = [agg]
                for n in onames:
                    oacts.append(self.fc_fwd(n, oacts[-1], True))
                h = oacts[-1]
                saved.append(PoolStage(names, acts, dst, agg, onames, oacts,
                                       upper))
            else:
                enames, unames = names, onames
                e = edges[lvl]
                x = coords[lvl]
                k = int(h.shape[0])
                w1 = self.fc[enames[0]]
                c = w1.k_in - 3
                wq = padded_width(w1.n_out)
                off_acts, delta = None, None
                if off_names is not None:
                    off_acts = [h]
                    for i, n in enumerate(off_names):
                        off_acts.append(self.fc_fwd(
                            n, off_acts[-1], i + 1 < len(off_names)))
                    delta = off_acts[-1]
                wx = torch.zeros((3, wq), dtype=torch.float32, device=dev)
                wx[:, :w1.n_out] = w1.w[c:c + 3]
                xo = torch.empty_like(x)
                q = torch.empty((k, wq), dtype=torch.float32, device=dev)
                _lib.check(lib.pgnn_offset_apply(
                    _lib.ptr(x), _lib.ptr(delta),
                    delta.stride(0) if delta is not None else 0, k,
                    _lib.ptr(wx), _lib.ptr(xo), _lib.ptr(q), wq, st),
                    "pgnn_offset_apply")
                hx = torch.zeros((k, padded_width(c + 3)),
                                 dtype=torch.float32, device=dev)
                hx[:, :c] = h[:, :c]
                hx[:, c:c + 3] = x
                p = self.fc_fwd(enames[0], hx, False)
                h1 = torch.empty((int(e.shape[0]), wq), dtype=torch.float32,
                                 device=dev)
                _lib.check(lib.pgnn_edge_hidden_fwd(
                    _lib.ptr(p), _lib.ptr(q), wq, _lib.ptr(e),
                    int(e.shape[0]), _lib.ptr(h1), st), "pgnn_edge_hidden_fwd")
                eacts = [h1]
                for n in enames[1:]:
                    eacts.append(self.fc_fwd(n, eacts[-1], True))
                dst = gnn.mark_sorted(e[:, 1].contiguous(), e._pgnn_sorted)
                agg = self._scatter_max(eacts[-1], dst, k)
                uacts = [agg]
                for i, n in enumerate(unames):
                    last = i + 1 == len(unames)
                    uacts.append(self.fc_fwd(n, uacts[-1], not last,
                                             residual=h if last else None))
                saved.append(GnnStage(enames, hx, xo, e, eacts, dst, agg,
                                      unames, uacts, off_names, off_acts, c))
                h = uacts[-1]
        pc = self.config['model_kwargs']['layer_configs'][-1]
        ps = pc['scope'] + '/predictor'
        cls_names = mlp_names(ps + '/cls', 2)
        cacts = [h, self.fc_fwd(cls_names[0], h, True)]
        cacts.append(self.fc_fwd(cls_names[1], cacts[-1], False))
        logits = cacts[-1]
        loc = []
        k = int(h.shape[0])
        pred = torch.empty((k, self.nc, self.box_len), dtype=torch.float32,
                           device=dev)
        for j in range(self.nc):
            names = mlp_names(ps + '/loc/cls_%d' % j, 3)
            a = [h]
            if self._head_slice is not None:
                # tf.split (gnn.py:196): this head's columns as rows of their own
                s = self._head_slice
                a = [torch.zeros((k, padded_width(s)), dtype=torch.float32,
                                 device=dev)]
                a[0][:, :s] = h[:, j * s:(j + 1) * s]
            for i, n in enumerate(names):
                a.append(self.fc_fwd(n, a[-1], i < 2))
            pred[:, j, :] = a[-1][:, :self.box_len]
            loc.append((names, a))
        saved.append(Heads(cls_names, cacts, loc))
        return logits[:, :self.nc], pred, saved

    # ---- backward -----------------------------------------------------------------
    def backward(self, state, dlogits, dpred, sync_sums=None):
        """Gradients of forward's `state`; no collective (returns False)."""
        lib, st, dev = self.lib, self._st(), self.device
        sparse = self.tr.sparse_adjoint
        saved = list(state)
        cls_names, cacts, loc = saved.pop()
        k, hw = int(cacts[0].shape[0]), int(cacts[0].shape[1])
        dh = torch.zeros((k, hw), dtype=torch.float32, device=dev)

        def add_dh(dx, width, col0=0):
            dh[:, col0:col0 + width] += dx[:, :width]

        # heads
        dy = torch.zeros((k, padded_width(self.nc)), dtype=torch.float32,
                         device=dev)
        dy[:, :self.nc] = dlogits
        cwidth = self.fc[cls_names[0]].k_in
        add_dh(self._chain_bwd(cls_names, cacts, dy, False), cwidth)
        for j, (names, a) in enumerate(loc):
            dy = torch.zeros((k, padded_width(self.box_len)),
                             dtype=torch.float32, device=dev)
            dy[:, :self.box_len] = dpred[:, j, :]
            d = self._chain_bwd(names, a, dy, False)
            if self._head_slice is not None:
                # a split head's input gradient goes to its own columns
                add_dh(d, self._head_slice, j * self._head_slice)
            else:
                add_dh(d, cwidth)
        # layers in reverse
        while saved:
            s = saved.pop()
            if isinstance(s, GnnStage):
                enames, eacts, unames, uacts = (s.enames, s.eacts, s.unames,
                                                s.uacts)
                dh_in = dh.clone()  # residual branch (gnn.py:372)
                d = self._chain_bwd(unames, uacts, dh.clone(), False)
                g, dense_from = self._max_bwd(sparse, enames, eacts, s, d)
                for i in range(dense_from, 0, -1):
                    # g is already masked by the ReLU of layer i (relu_mask)
                    g = self.fc_bwd(enames[i], eacts[i - 1], eacts[i], g,
                                    relu=False)
                    _lib.check(lib.pgnn_relu_mask_mul(
                        _lib.ptr(g), _lib.ptr(eacts[i - 1]), g.numel(), st),
                        "pgnn_relu_mask_mul")
                kk = int(s.hx.shape[0])
                wq = int(g.shape[1])
                dp = torch.empty((kk, wq), dtype=torch.float32, device=dev)
                dq = torch.empty((kk, wq), dtype=torch.float32, device=dev)
                _lib.check(lib.pgnn_edge_hidden_bwd(
                    _lib.ptr(g), wq, _lib.ptr(s.e), int(s.e.shape[0]), kk,
                    _lib.ptr(dp), _lib.ptr(dq), st), "pgnn_edge_hidden_bwd")
                w1 = self.fc[enames[0]]
                # P = [h, x] W1 + b1
                dhx = self.fc_bwd(enames[0], s.hx, None, dp, False)
                dh_in[:, :s.c] += dhx[:, :s.c]
                # Q = x' Wx, Wx = rows c..c+2 of W1 (pre-activation is P - Q; the
                # minus sign is already in dq)
                gwx_ptr = ctypes.c_void_p(
                    w1.gw.data_ptr() + 4 * s.c * w1.n_out)
                self._weight_grad(s.xo, 3, 3, dq, w1.n_out, gwx_ptr, None)
                if s.off_names is not None:
                    # dx' = dQ Wx^T (image refreshed by repack())
                    d = self._mlp1(self.wx_packed_t[enames[0]], w1.n_out, 3,
                                   False, dq, w1.n_out)
                    d = self._chain_bwd(s.off_names, s.off_acts, d, False)
                    dh_in[:, :s.c] += d[:, :s.c]
                dh = dh_in
            else:
                names, acts, onames, oacts = (s.names, s.acts, s.onames,
                                              s.oacts)
                d = self._chain_bwd(onames, oacts, dh, True)
                # (the gradient w.r.t. the stage's input rows is wanted only
                # above the first level; acts[0] is a gathered input, not a
                # ReLU output: no mask there)
                first = len(names) == 1
                g, dense_from = self._max_bwd(
                    sparse, names, acts, s, d, mask_x=not first,
                    need_dx=not first or s.upper is not None)
                for i in range(dense_from, -1, -1):
                    g = self.fc_bwd(names[i], acts[i], acts[i + 1], g,
                                    relu=False,
                                    need_dx=i > 0 or s.upper is not None)
                    if i > 0:
                        _lib.check(lib.pgnn_relu_mask_mul(
                            _lib.ptr(g), _lib.ptr(acts[i]), g.numel(), st),
                            "pgnn_relu_mask_mul")
                if s.upper is not None:
                    # adjoint of the gather h[src]: dh_prev[src] += g[:, :n]
                    # (the coordinate columns behind them have no parameters
                    # upstream)
                    e, n_feat, k_prev, w_prev = s.upper
                    src = e[:, 0].contiguous()
                    dh = torch.zeros((k_prev, w_prev), dtype=torch.float32,
                                     device=dev)
                    _lib.check(lib.pgnn_scatter_sum_f32(
                        _lib.ptr(g), g.stride(0), _lib.ptr(src),
                        int(src.shape[0]), n_feat, k_prev, _lib.ptr(dh),
                        dh.stride(0), 0, None, st), "pgnn_scatter_sum_f32")
        return False
