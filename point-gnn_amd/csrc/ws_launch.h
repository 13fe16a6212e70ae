// Host side of the weights-stationary launches (edge_ws.h, edge_ws_split.h,
// pool_ws.h, pool_split.h): the `*_applies` predicates, the launchers and the
// two split-precision edge entries' body.  A fragment of gnn.hip's translation
// unit, included there once behind Plan, the *Args structs, Dyn and launch_lds.
//
// Every launcher knows its whole geometry (ws_partition.h) before it enqueues
// anything, and every predicate asks the same function: a geometry the
// partition cannot serve takes the LDS-tile kernel or is declined, and no
// half-launched stage is left behind.
#pragma once
#include "ws_partition.h"

namespace {
using namespace pgnn;

// CUs a weights-stationary launch uses of the `cus` it could have: `ws_reserve`
// stay free for the kernels of other streams, while at least 64 remain
inline int ws_cus(int cus) {
  return (g_ws_reserve > 0 && cus - g_ws_reserve >= 64) ? cus - g_ws_reserve : cus;
}
inline int ws_cus(hipStream_t stream) { return ws_cus(stream_cu_count(stream)); }

inline int ws_slices(int cus) { return ws_slice_count(cus, g_ws_xcds); }
inline bool ws_feasible(int nt, int ntmax, int cus) {
  return pgnn::ws_feasible(nt, ntmax, cus, ws_slices(cus));
}

// The launchers' guard on ws_partition's answer (unreachable behind the
// `*_applies` predicates, which have asked ws_feasible).
inline int ws_partition_rc(int why) {
  PGNN_REQUIRE(why != kWsTooFewCus, PGNN_E_UNSUPPORTED,
               "edge_ws: too few CUs for the column groups");
  PGNN_REQUIRE(why == kWsOk, PGNN_E_UNSUPPORTED,
               "edge_ws: column tiles do not group");
  return 0;
}

// Weights-stationary edge kernel (edge_ws.h): one workgroup per CU, the column
// tiles in groups that fit the LDS, the 16-row tiles in one slice per XCD.
// plan_edge_ws fills the kernel's arguments, geometry included, and enqueues
// nothing; run_edge_ws launches them.  ROWS: `ea.P` holds one ready input row
// per edge (pool_split.h).  POL (WsMax / WsSum, ws_sum.h): the aggregation; the
// partition, the tile pool and the balance do not depend on it, and the sum
// kernels exist without EMIT and ROWS only.
template <int KQ, int NTMAX>
int plan_edge_ws(EdgeWsArgs &a, const LayerDev &L, const EdgeArgs &ea,
                 int64_t n_edges, const SegArgs &sa, int cus, int32_t *sched,
                 float *rows_out, int64_t ld_rows, float *h1_out,
                 const int32_t *n_dev) {
  a = {};
  const int rc = ws_partition_rc(ws_partition(a, L.nt, NTMAX, cus, ws_slices(cus)));
  if (rc) return rc;
  a.n_dev = n_dev;
  a.rows_out = rows_out;
  a.ld_rows = ld_rows;
  a.h1_out = h1_out;
  a.P = ea.P;
  a.Q = ea.Q;
  a.ldv4 = (int)(ea.ldpq >> 2);
  a.edges = ea.edges;
  a.n_edges = n_edges;
  a.wp = L.wp;
  a.nt = L.nt;
  a.relu_from = L.relu_from;
  a.out = sa.out;
  a.ldo = sa.ldo;
  a.num_segments = sa.num_segments;
  a.sorted = sa.sorted;
  a.prio = g_ws_prio;
  a.ts = (long long *)g_mlp_ts;
  a.sched = (g_ws_pool_pct > 0 && a.xcds <= kWsMaxSlices) ? sched : nullptr;
  a.pool_pct = g_ws_pool_pct;
  a.chunk = g_ws_chunk;
  if (g_ws_balance >= 2) {
    // relative cost of a row tile: 4 KQ MFMAs of 32 cycles per column tile +
    // ~1.9k cycles of gather VALU / running max per tile (tools/ws_timeline.py)
    // (measured on the fp32 kernel: 977 vs 971 us, no gain -- its 12/10/10
    // imbalance is smaller than the noise between its XCDs; the split-bf16
    // kernel, 9/8/8/7 for 5/5/5/4 tiles, gains 1.7 %.  ws_balance = 2 turns it
    // on here too.)
    double cost[kWsMaxGroups];
    for (int g = 0; g < a.groups; ++g)
      cost[g] = 128.0 * KQ * (a.tile0[g + 1] - a.tile0[g]) + 1900.0;
    ws_balance(a, cus, cost, a.sched != nullptr);
  }
  return 0;
}

template <int KQ, int NTMAX, bool ROWS, class POL = WsMax, bool SCALED = false,
          bool K300 = false>
int run_edge_ws(const EdgeWsArgs &a, int cus, hipStream_t stream) {
  static_assert(!POL::kSum || !ROWS, "the sum kernels read no ready rows");
  static_assert(!SCALED || (!POL::kSum && !ROWS), "scaled: the plain max kernel only");
  PGNN_HIP((hipError_t)arm_sched(a.sched, stream));
  const size_t lds = (size_t)KQ * NTMAX * 1024 + 16 * NTMAX * sizeof(float);
  auto kern = edge_ws_kernel<KQ, NTMAX, false, ROWS, POL, SCALED, K300>;
  if constexpr (!ROWS && !POL::kSum && !SCALED) {  // training forward: the rows are written as well
    if (a.rows_out) kern = edge_ws_kernel<KQ, NTMAX, true>;
  }
  return launch_lds(kern, dim3((unsigned)(cus / a.xcds * a.xcds)),
                    dim3(64 * kWsWaves), lds, stream, a);
}

template <int KQ, int NTMAX, class POL = WsMax>
int launch_edge_ws(const LayerDev &L, const EdgeArgs &ea, int64_t n_edges,
                   const SegArgs &sa, int cus, int32_t *sched,
                   hipStream_t stream, float *rows_out = nullptr,
                   int64_t ld_rows = 0, float *h1_out = nullptr,
                   const int32_t *n_dev = nullptr) {
  EdgeWsArgs a;
  const int rc = plan_edge_ws<KQ, NTMAX>(a, L, ea, n_edges, sa, cus, sched,
                                         rows_out, ld_rows, h1_out, n_dev);
  return rc ? rc : run_edge_ws<KQ, NTMAX, false, POL>(a, cus, stream);
}

// The SCALED form of the same launch (edge_ws.h, pk_sub_clamp): ea.P, ea.Q hold
// 2^-scale_exp x the operands; status / nv_dev: the guard's flag and the
// capacity form's vertex count (both nullable).  K300: the operands' and the
// image's last K group in the order of pgnn_k300_source (edge_ws.h).
template <int KQ, int NTMAX, bool K300 = false>
int launch_edge_ws_scaled(const LayerDev &L, const EdgeArgs &ea, int64_t n_edges,
                          const SegArgs &sa, int cus, int32_t *sched,
                          hipStream_t stream, const int32_t *n_dev,
                          const int32_t *nv_dev, int scale_exp, int32_t *status) {
  EdgeWsArgs a;
  const int rc = plan_edge_ws<KQ, NTMAX>(a, L, ea, n_edges, sa, cus, sched,
                                         nullptr, 0, nullptr, n_dev);
  if (rc) return rc;
  a.nv_dev = nv_dev;
  a.unscale = (float)((int64_t)1 << scale_exp);
  a.status = status;
  return run_edge_ws<KQ, NTMAX, false, WsMax, true, K300>(a, cus, stream);
}

// the shapes edge_ws.h is instantiated for: one square layer of 19 (C = 300)
// or 16 (C = 256) column tiles, a CU count that splits into 8 slices.  (The
// sum kernels share the max kernels' geometry, LDS image and threshold: the
// answer is the same for every policy.)
template <class POL = WsMax>
bool edge_ws_applies(const Plan &p, int64_t n_edges, int cus) {
  if (g_mlp_debug & 2048) return false;
  const LayerDev &L = p.chain.l[0];
  if (p.chain.n != 1 || L.kq != L.nt || (L.nt != 19 && L.nt != 16)) return false;
  if (cus < 64 || cus % 8 != 0) return false;
  if (!ws_feasible(L.nt, L.nt == 19 ? 7 : 8, cus)) return false;
  // one column group of the layer's fragments + bias must fit a workgroup's
  // LDS (133 KiB / 128 KiB on gfx950's 160 KiB); a device with less takes the
  // LDS-tile kernel
  if ((size_t)L.kq * (L.nt == 19 ? 7 : 8) * 1024 + 16 * 8 * sizeof(float) >
      device_max_lds())
    return false;
  if (g_mlp_debug & 4096) return true;
  // below ~2 tiles per wave the fixed cost (133 KiB of weights per workgroup
  // into LDS) is not amortised
  return n_edges >= (int64_t)16 * 2 * kWsWaves * cus;
}

// ... and the K = 300 order of the scaled kernel's last K group (edge_ws.h,
// PGNN_EDGE_K300_ORDER): exactly 300 features in 19 K groups.  C = 256 has no
// padding and no such order.
inline bool edge_k300_applies(const Plan &p, const pgnn_fc_layer *layers,
                              int width) {
  return p.chain.n == 1 && p.chain.l[0].kq == 19 && p.chain.l[0].nt == 19 &&
         layers[0].k_in == 300 && width == 300;
}

// Weights-stationary pooling kernel (pool_ws.h): car's 4-32-64-128-300 chain.
template <class POL = WsMax>
bool pool_ws_applies(const Plan &p, int64_t n_edges, int cus) {
  if (g_mlp_debug & (8192 | 1024)) return false;
  const ChainDev &c = p.chain;
  if (c.n != 4 || c.l[0].kq != 1 || c.l[0].nt != 2 || c.l[1].nt != 4 ||
      c.l[2].nt != 8 || c.l[3].kq != 8 || c.l[3].nt != 19)
    return false;
  if (cus < 8) return false;
  if ((size_t)8 * 19 * 1024 + 16 * 19 * sizeof(float) > device_max_lds())
    return false;
  if (g_mlp_debug & 16384) return true;
  return n_edges >= (int64_t)16 * 2 * kWsWaves * cus;
}

// What pool_ws_kernel, pool_hidden_kernel and pool_ws_f16x2_kernel are all
// told: the inputs, the three hidden layers and the last layer (the f16x2
// kernel gets its fp16 image for `wp` instead).  The output, the tile pool
// and the taps stay zero for the caller to set.
PoolWsArgs pool_ws_args(const Plan &p, const PoolArgs &pa, int64_t n_edges,
                        const int32_t *n_dev, int num_segments) {
  PoolWsArgs a = {};
  a.feat = pa.feat;
  a.nfeat = pa.nfeat;
  a.xyz = pa.xyz;
  a.kp = pa.kp;
  a.edges = pa.edges;
  a.n_edges = n_edges;
  a.n_dev = n_dev;
  a.l0 = p.chain.l[0];
  a.l1 = p.chain.l[1];
  a.l2 = p.chain.l[2];
  a.wp = p.chain.l[3].wp;
  a.kq = p.chain.l[3].kq;
  a.nt = p.chain.l[3].nt;
  a.relu_from = p.chain.l[3].relu_from;
  a.num_segments = num_segments;
  return a;
}

// ... and what the two one-launch kernels add: where the maxima go, and the
// tile pool (armed here: call this last before the launch)
int pool_ws_out(PoolWsArgs &a, const SegArgs &sa, int32_t *sched,
                hipStream_t stream) {
  a.out = sa.out;
  a.ldo = sa.ldo;
  a.sorted = sa.sorted;
  a.sched = g_ws_pool_pct > 0 ? sched : nullptr;
  a.pool_pct = g_ws_pool_pct;
  a.chunk = 1;
  PGNN_HIP((hipError_t)arm_sched(a.sched, stream));
  return 0;
}

template <class POL = WsMax>
int launch_pool_ws(const Plan &p, const PoolArgs &pa, int64_t n_edges,
                   const SegArgs &sa, int cus, int32_t *sched,
                   hipStream_t stream, float *const *acts = nullptr,
                   int64_t ld4 = 0, const int32_t *n_dev = nullptr) {
  PoolWsArgs a = pool_ws_args(p, pa, n_edges, n_dev, sa.num_segments);
  if (acts) {  // training forward: the layers' activations are written too
    a.a1_out = acts[0];
    a.a2_out = acts[1];
    a.a3_out = acts[2];
    a.a4_out = acts[3];
    a.ld4 = ld4;
  }
  a.prio = g_ws_prio;
  a.ts = (long long *)g_mlp_ts;
  const int rc = pool_ws_out(a, sa, sched, stream);
  if (rc) return rc;
  const size_t lds = (size_t)8 * 19 * 1024 + 16 * 19 * sizeof(float);
  auto kern = pool_ws_kernel<false, POL>;
  if constexpr (!POL::kSum) {
    if (acts) kern = pool_ws_kernel<true>;
  }
  return launch_lds(kern, dim3((unsigned)cus), dim3(64 * kWsWaves), lds, stream,
                    a);
}

// Split pooling stage (pool_split.h): ped_cyl's 4-32-64-128-256-512 chain, the
// hidden rows [n_edges, 256] through a caller-provided workspace.  (car's
// 4-32-64-128-300 chain on the same form -- 64 -> 128 in LDS, rows [n_edges,
// 128], 128 -> 300 as edge_ws_kernel<8, 7, ROWS> -- measured 310 us against
// pool_ws.h's 296: its last layer is only 8 K groups deep, so a row tile
// carries half the MFMA work over the same per-tile cost; not kept.)
constexpr int kPoolSplitHidden = 256;
bool pool_split_applies(const Plan &p, int64_t n_edges, int cus) {
  if (g_mlp_debug & (8192 | 1024)) return false;
  const ChainDev &c = p.chain;
  if (c.n != 5 || c.l[0].kq != 1 || c.l[0].nt != 2 || c.l[1].nt != 4 ||
      c.l[2].nt != 8 || c.l[3].kq != 8 || c.l[3].nt != 16 || c.l[4].kq != 16 ||
      c.l[4].nt != 32)
    return false;
  if (cus < 64 || cus % 8 != 0) return false;
  if (!ws_feasible(c.l[4].nt, 8, cus)) return false;
  if ((size_t)16 * 8 * 1024 + 16 * 16 * sizeof(float) > device_max_lds())
    return false;
  if (g_mlp_debug & 16384) return true;
  return n_edges >= (int64_t)16 * 2 * kWsWaves * cus;
}

int launch_pool_split(const Plan &p, const PoolArgs &pa, int64_t n_edges,
                      const SegArgs &sa, int cus, int32_t *sched,
                      hipStream_t stream, const int32_t *n_dev, float *hidden) {
  // the second launch's arguments first: its geometry is known, or the stage
  // declined, before the first launch is enqueued
  const EdgeArgs ea = {hidden, nullptr, kPoolSplitHidden, pa.edges};
  EdgeWsArgs e;
  int rc = plan_edge_ws<16, 8>(e, p.chain.l[4], ea, n_edges, sa, cus, sched,
                               nullptr, 0, nullptr, n_dev);
  if (rc) return rc;
  PoolWsArgs a = pool_ws_args(p, pa, n_edges, n_dev, sa.num_segments);
  a.prio = g_ws_prio;
  a.a4_out = hidden;
  a.ld4 = kPoolSplitHidden;
  a.slices = 8;
  const size_t lds = (size_t)8 * 16 * 1024 + 16 * 16 * sizeof(float);
  rc = launch_lds(pool_hidden_kernel, dim3((unsigned)cus),
                  dim3(64 * kPoolHWaves), lds, stream, a);
  return rc ? rc : run_edge_ws<16, 8, true>(e, cus, stream);
}

// Host side of an arithmetic of edge_ws_split.h: its name in messages, the
// largest column group per K depth (KB = 10: 19 tiles in 5/5/5/4 resp. 7/6/6;
// KB = 8: 16 in 4 x 4 resp. 6/5/5), the relative cost of a row tile per group
// -- mfma cycles of a column tile (60 resp. 30 MFMAs of 16 cycles at KB = 10) +
// the part of the gather / split / segmented max that does not hide behind
// them (bf16x3: round 4's 2.4k cycles, when nothing did; the interleaved body
// leaves about a third) --, and whether the waves raise their priority
// outside the MFMA loop (g_ws_prio)
template <class Arith>
struct SplitHost;
template <>
struct SplitHost<Bf16x3> {
  static constexpr const char *kName = "edge_bf16x3";
  static constexpr int kNtMax10 = 5, kNtMax8 = 5;
  static constexpr double kTileCost = 960.0, kRowCost = 2400.0;
  static int prio() { return g_ws_prio; }
};
template <>
struct SplitHost<F16x2> {
  static constexpr const char *kName = "edge_f16x2";
  static constexpr int kNtMax10 = 7, kNtMax8 = 6;
  static constexpr double kTileCost = 480.0, kRowCost = 1600.0;
  static int prio() { return 0; }
};

template <class Arith>
std::string split_msg(const char *what) {
  return std::string(SplitHost<Arith>::kName) + ": " + what;
}

template <class Arith, int KB, int NTMAX>
int launch_edge_ws_split(EdgeWsArgs &a, int nt, int cus, int32_t *status,
                         hipStream_t stream) {
  using H = SplitHost<Arith>;
  const int rc = ws_partition_rc(ws_partition(a, nt, NTMAX, cus, ws_slices(cus)));
  if (rc) return rc;
  if (g_ws_balance) {
    double cost[kWsMaxGroups];
    for (int g = 0; g < a.groups; ++g)
      cost[g] = H::kTileCost * KB / 10 * (a.tile0[g + 1] - a.tile0[g]) + H::kRowCost;
    ws_balance(a, cus, cost, a.sched != nullptr);
  }
  const size_t lds =
      (size_t)KB * NTMAX * Arith::kParts * 1024 + 16 * NTMAX * sizeof(float);
  PGNN_REQUIRE(lds <= device_max_lds(), PGNN_E_UNSUPPORTED,
               split_msg<Arith>("column group does not fit the LDS").c_str());
  return launch_lds(edge_ws_split_kernel<Arith, KB, NTMAX>,
                    dim3((unsigned)(cus / a.xcds * a.xcds)), dim3(64 * kWsWaves),
                    lds, stream, a, status);
}

// the two split-precision edge entries; status: F16x2's range flag (null for
// Bf16x3, whose kernel has no guard)
template <class Arith>
int edge_split_fwd_impl(const float *P, const float *Q, int64_t ld_pq,
                        int32_t width, const int32_t *edges, int64_t edges_cap,
                        int32_t vertices_cap, const void *image, int32_t n_out,
                        int32_t relu_from, int32_t edges_sorted, float *out,
                        int64_t ld_out, int32_t *status,
                        const pgnn_dyn_count *n_edges,
                        const pgnn_dyn_count *num_vertices, hipStream_t stream) {
  using H = SplitHost<Arith>;
  PGNN_REQUIRE(edges_cap >= 0 && vertices_cap >= 0 && width > 0 && n_out > 0 &&
                   image,
               PGNN_E_INVALID, split_msg<Arith>("bad argument").c_str());
  const Dyn de = dyn_of(n_edges), dk = dyn_of(num_vertices);
  const int kq = (width + 15) / 16, nt = (n_out + 15) / 16;
  const int kb = (width + 31) / 32;
  PGNN_REQUIRE(ld_pq == 16 * kq && ld_out >= 16 * nt, PGNN_E_INVALID,
               split_msg<Arith>("ld_pq / ld_out do not match the padded widths")
                   .c_str());
  const int cus = ws_cus(stream);
  // the shapes the kernel is instantiated for, and enough rows to amortise
  // 150 KiB of weights per workgroup: otherwise the caller runs the fp32 entry
  if (!((kb == 10 && nt == 19) || (kb == 8 && nt == 16)) || cus < 64 ||
      cus % 8 != 0 ||
      !ws_feasible(nt, kb == 10 ? H::kNtMax10 : H::kNtMax8, cus) ||
      (!g_b16_force &&
       expected(de, edges_cap) < (int64_t)16 * 2 * kWsWaves * cus) ||
      // (the kernel addresses P / Q rows with 32-bit byte offsets)
      (int64_t)vertices_cap * ld_pq * 4 >= ((int64_t)1 << 32))
    return PGNN_E_UNSUPPORTED;  // (no message: an expected answer)
  if (vertices_cap == 0) return 0;
  PGNN_REQUIRE(out != nullptr, PGNN_E_INVALID,
               split_msg<Arith>("null output").c_str());
  if (!(edges_sorted & 2)) {
    const int rc = fill_lowest_rows(out, ld_out, vertices_cap, dk, stream);
    if (rc) return rc;
  }
  if (edges_cap == 0) return 0;
  PGNN_REQUIRE(P && Q && edges, PGNN_E_INVALID,
               split_msg<Arith>("null input").c_str());
  PGNN_REQUIRE(((uintptr_t)P % 16 == 0) && ((uintptr_t)Q % 16 == 0) &&
                   ((uintptr_t)image % 16 == 0),
               PGNN_E_INVALID,
               split_msg<Arith>("P / Q / image must be 16-byte aligned").c_str());
  EdgeWsArgs a = {};
  a.P = P;
  a.Q = Q;
  a.ldv4 = (int)(ld_pq >> 2);
  a.edges = edges;
  a.n_edges = edges_cap;
  a.n_dev = de.dev;
  a.wp = reinterpret_cast<const float *>(image);
  a.nt = nt;
  a.relu_from = relu_from;
  a.out = out;
  a.ldo = ld_out;
  a.num_segments = vertices_cap;
  a.sorted = edges_sorted & 1;
  a.prio = H::prio();
  if (Arith::kRangeGuard) a.nv_dev = dk.dev;
  if (kb == 10)
    return launch_edge_ws_split<Arith, 10, H::kNtMax10>(a, nt, cus, status, stream);
  return launch_edge_ws_split<Arith, 8, H::kNtMax8>(a, nt, cus, status, stream);
}

}  // namespace
