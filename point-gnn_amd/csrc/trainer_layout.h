// Workspace layout of the native training step (trainer.hip), without HIP: the
// host compiler compiles this header alone (tests/test_host_cpu.py does).
// layout_forward and layout_backward are the only code that allocates.  The
// sizing query runs them on a null base, the forward and the backward on the
// workspace: the backward finds the forward's buffers again because both are the
// same function of shape and batch sizes (pointers in the handle: not re-entrant).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "pointgnn_hip.h"

namespace pgnn {

inline int pad16(int n) { return (n + 15) / 16 * 16; }

// ---- the allocator ----------------------------------------------------------------
struct BumpSpan {  // (for the host test) released: how many spans existed
  size_t off, bytes;  // when this one was given back, -1: never
  int released;
};
struct Bump {
  char *base;  // null: sizing run, the pointers are never used
  size_t off, cap, high;
  std::vector<BumpSpan> *log;
  Bump(void *p, size_t n, std::vector<BumpSpan> *l = nullptr)
      : base((char *)p), off(0), cap(n), high(0), log(l) {}
  void *raw(size_t bytes) {
    const size_t at = (off + 255) / 256 * 256;
    off = at + bytes;
    if (off > high) high = off;
    if (log) log->push_back({at, bytes, -1});
    if (!base) return (void *)(uintptr_t)(at + 256);
    if (off > cap) return nullptr;
    return base + at;
  }
  float *f(int64_t rows, int64_t ld) { return (float *)raw((size_t)rows * ld * 4); }
  int32_t *i32(int64_t n) { return (int32_t *)raw((size_t)n * 4); }
  // release() gives back everything allocated since mark()
  size_t mark_off = 0, mark_n = 0;
  void mark() {
    mark_off = off;
    mark_n = log ? log->size() : 0;
  }
  void release() {
    for (size_t i = mark_n; log && i < log->size(); ++i)
      (*log)[i].released = (int)log->size();
    off = mark_off;
  }
};

// ---- what the forward keeps for the backward --------------------------------------
struct PoolSaved {
  float *feat;                 // [E, 16]
  float *act[PGNN_TRAIN_MAX_FC];   // outputs of the point MLP layers
  int32_t *dst;
  float *agg;                  // [K, pad(n_out of last a)]
  float *oact[PGNN_TRAIN_MAX_FC];  // outputs of the output MLP layers
};
struct GnnSaved {
  const float *h_in;           // [K, ld_h]
  float *off_act[PGNN_TRAIN_MAX_FC];  // outputs of the offset MLP layers
  float *xx, *xo, *q, *hx, *p;  // xx = [x; x'] [2K, 3], xo = x' its 2nd half
  float *eact[PGNN_TRAIN_MAX_FC];  // eact[0] = H1, eact[i] = output of a[i]
  int32_t *dst;
  float *agg;
  float *uact[PGNN_TRAIN_MAX_FC];  // outputs of the update MLP layers
};
struct HeadsSaved {
  float *y1[4], *y2[4], *y3[4];  // fused groups: outputs of the three layers
  float *c1, *logits;          // [K, 64], [K, pad(nc)]
  float *l1[PGNN_TRAIN_MAX_CLASSES], *l2[PGNN_TRAIN_MAX_CLASSES],
      *l3[PGNN_TRAIN_MAX_CLASSES];
  float *pred;                 // [K, nc, L]
};
struct Saved {
  PoolSaved pool[PGNN_TRAIN_MAX_STAGES];
  GnnSaved gnn[PGNN_TRAIN_MAX_STAGES];
  HeadsSaved heads;
  const float *h_final;
  int ld_h_final;
  int64_t k_final;
  float *scratch;              // weight-grad / segmax workspace
  size_t scratch_bytes;
};

// ---- the backward's buffers ---------------------------------------------------------
// K-row buffers are the dY of deferred weight gradients: they stay to the end of
// the backward.  A stage's E-row temporaries (ge, gz, ties) go with the stage.
struct StageGrads {
  float *du[PGNN_TRAIN_MAX_FC];  // grad w.r.t. the input of b[i] (pooling: "dob")
  float *dp, *dq, *dhx, *dxo;    // gnn: dP | dQ back to back (one fill), [K, 16]
  float *doff[PGNN_TRAIN_MAX_FC];  // gnn: grad w.r.t. the input of c[i]
  float *ge[PGNN_TRAIN_MAX_FC];  // grad w.r.t. the output of a[i] (pooling: "ga")
  float *gz;                     // dense form: grad w.r.t. the last a layer
  int32_t *ties;                 // dense form: tie counts [K, wa]
};
struct Grads {
  // gradient w.r.t. the output of stage i: dhs[i + 1] (dhs[n] = w.r.t. the
  // input of the heads), one buffer per boundary
  float *dhs[PGNN_TRAIN_MAX_STAGES + 1];
  float *dxh;
  float *dy3[4], *dy2[4], *dy1[4];  // fused head groups (one set per group)
  float *dy, *d1, *d2;              // separate heads
  StageGrads stage[PGNN_TRAIN_MAX_STAGES];
  void *wgrad_part;  // partial sums of the deferred weight gradients
};

// ---- the shape of a trainer, filled once from the model -------------------------------
struct FcShape {
  int k_in, n_out;
};
struct StageShape {
  int kind, level;  // 0: PointSetPooling, 1: GraphNetAutoCenter
  int n_a, n_b, n_c;
  FcShape a[PGNN_TRAIN_MAX_FC], b[PGNN_TRAIN_MAX_FC], c[PGNN_TRAIN_MAX_FC];
  bool want_wt;  // the last a layer takes the sparse adjoint
};
struct TrainerShape {
  int n_stages;
  StageShape stages[PGNN_TRAIN_MAX_STAGES];
  int n_groups;        // fused head groups; 0: the heads run one by one
  int group_w[4][3];   // n_out of a group's three fused layers
  int cls_w;           // separate heads: n_out of the class head's first layer
  int loc_w[PGNN_TRAIN_MAX_CLASSES][3];  // and of every box head's layers
  int num_classes, box_len;
};

// Forward: scratch, every stage's saved activations, the heads'.  The `dst`
// column of a level's edge list is shared by the stages of that level and
// allocated by the first of them.  false: more head groups than HeadsSaved holds.
inline bool layout_forward(const TrainerShape &t, const pgnn_train_batch &b,
                           size_t scratch_bytes, Bump &ws, Saved &sv) {
  sv.scratch_bytes = scratch_bytes;
  sv.scratch = (float *)ws.raw(scratch_bytes);
  const float *h = nullptr;
  int ld_h = 0;
  int32_t *dst_of[PGNN_TRAIN_MAX_LEVELS] = {nullptr};
  auto level_dst = [&](int lvl, int64_t E) {
    if (!dst_of[lvl]) dst_of[lvl] = ws.i32(E > 0 ? E : 1);
    return dst_of[lvl];
  };
  for (int si = 0; si < t.n_stages; ++si) {
    const StageShape &s = t.stages[si];
    const int64_t E = b.n_edges[s.level], K = b.n_vertices[s.level + 1];
    const int wa = pad16(s.a[s.n_a - 1].n_out);
    if (s.kind == 0) {
      PoolSaved &p = sv.pool[si];
      p.feat = ws.f(E, 16);
      for (int i = 0; i < s.n_a; ++i) p.act[i] = ws.f(E, pad16(s.a[i].n_out));
      p.agg = ws.f(K, wa);
      p.dst = level_dst(s.level, E);
      for (int i = 0; i < s.n_b; ++i) p.oact[i] = ws.f(K, pad16(s.b[i].n_out));
      h = p.oact[s.n_b - 1];
    } else {
      GnnSaved &g = sv.gnn[si];
      const int cc = s.a[0].k_in - 3, wq = pad16(s.a[0].n_out);
      g.h_in = h;
      for (int i = 0; i < s.n_c; ++i) g.off_act[i] = ws.f(K, pad16(s.c[i].n_out));
      g.xx = ws.f(2 * K, 3);
      g.xo = g.xx ? g.xx + 3 * K : nullptr;
      g.q = ws.f(K, wq);
      g.hx = ws.f(K, pad16(cc + 3));
      g.p = ws.f(K, wq);
      g.eact[0] = ws.f(E, wq);
      for (int i = 1; i < s.n_a; ++i) g.eact[i] = ws.f(E, pad16(s.a[i].n_out));
      g.dst = level_dst(s.level, E);
      g.agg = ws.f(K, wa);
      for (int i = 0; i < s.n_b; ++i) g.uact[i] = ws.f(K, pad16(s.b[i].n_out));
      h = g.uact[s.n_b - 1];
    }
    ld_h = pad16(s.b[s.n_b - 1].n_out);
  }
  const int64_t K = b.n_vertices[b.n_levels];
  const int nc = t.num_classes, L = t.box_len;
  HeadsSaved &hs = sv.heads;
  sv.h_final = h;
  sv.ld_h_final = ld_h;
  sv.k_final = K;
  if (t.n_groups > 4) return false;
  for (int gi = 0; gi < t.n_groups; ++gi) {
    hs.y1[gi] = ws.f(K, pad16(t.group_w[gi][0]));
    hs.y2[gi] = ws.f(K, pad16(t.group_w[gi][1]));
    hs.y3[gi] = ws.f(K, pad16(t.group_w[gi][2]));
  }
  if (t.n_groups == 0) hs.c1 = ws.f(K, pad16(t.cls_w));
  hs.logits = ws.f(K, pad16(nc));
  for (int j = 0; j < nc && t.n_groups == 0; ++j) {
    hs.l1[j] = ws.f(K, pad16(t.loc_w[j][0]));
    hs.l2[j] = ws.f(K, pad16(t.loc_w[j][1]));
    hs.l3[j] = ws.f(K, pad16(L));
  }
  hs.pred = ws.f(K, (int64_t)nc * L);
  return true;
}

// Backward, behind the forward's buffers: the boundary gradients, the heads'
// buffers, the stages in reverse (K-row buffers, then the E-row temporaries
// that the stage's end releases), the deferred weight gradients' partial sums.
inline void layout_backward(const TrainerShape &t, const pgnn_train_batch &b,
                            size_t wgrad_bound, Bump &ws, const Saved &sv,
                            Grads &gr) {
  const int64_t K = sv.k_final;
  const int hw = sv.ld_h_final;
  for (int i = 0; i <= t.n_stages; ++i) gr.dhs[i] = ws.f(K, hw);
  gr.dxh = ws.f(K, hw);
  if (t.n_groups > 0) {
    int w[3] = {16, 16, 16};  // (one width per layer for all groups)
    for (int gi = 0; gi < t.n_groups; ++gi)
      for (int i = 0; i < 3; ++i)
        if (pad16(t.group_w[gi][i]) > w[i]) w[i] = pad16(t.group_w[gi][i]);
    for (int gi = 0; gi < t.n_groups; ++gi) {
      gr.dy3[gi] = ws.f(K, w[2]);
      gr.dy2[gi] = ws.f(K, w[1]);
      gr.dy1[gi] = ws.f(K, w[0]);
    }
  } else {
    const int nc = t.num_classes, L = t.box_len;
    int wh = pad16(t.cls_w);  // widest hidden layer of the heads
    for (int j = 0; j < nc; ++j)
      for (int i = 0; i < 3; ++i)
        if (pad16(t.loc_w[j][i]) > wh) wh = pad16(t.loc_w[j][i]);
    gr.dy = ws.f(K, pad16(nc > L ? nc : L));
    gr.d1 = ws.f(K, wh);
    gr.d2 = ws.f(K, wh);
  }
  for (int si = t.n_stages - 1; si >= 0; --si) {
    const StageShape &s = t.stages[si];
    const int64_t E = b.n_edges[s.level], Ks = b.n_vertices[s.level + 1];
    const int wa = pad16(s.a[s.n_a - 1].n_out);
    StageGrads &g = gr.stage[si];
    for (int i = 0; i < s.n_b; ++i) g.du[i] = ws.f(Ks, pad16(s.b[i].k_in));
    if (s.kind == 1) {
      const int cc = s.a[0].k_in - 3, wq = pad16(s.a[0].n_out);
      g.dp = ws.f(2 * Ks, wq);
      g.dq = g.dp ? g.dp + Ks * wq : nullptr;
      g.dhx = ws.f(Ks, pad16(cc + 3));
      g.dxo = ws.f(Ks, 16);
      for (int i = 0; i < s.n_c; ++i) g.doff[i] = ws.f(Ks, pad16(s.c[i].k_in));
    }
    ws.mark();
    // (a two-layer GNN stage's sparse adjoint writes dP / dQ directly)
    if (!(s.kind == 1 && s.want_wt && s.n_a == 2))
      for (int i = 0; i + 1 < s.n_a; ++i)
        g.ge[i] = ws.f(E, pad16(s.a[i + 1].k_in));
    if (!s.want_wt) {
      g.gz = ws.f(E, wa);
      g.ties = ws.i32(Ks * wa > 0 ? Ks * wa : 1);
    }
    ws.release();
  }
  gr.wgrad_part = ws.raw(wgrad_bound);
}

}  // namespace pgnn
