// Geometry of a weights-stationary launch (edge_ws.h, edge_ws_split.h,
// pool_split.h): which column tiles form a group and which workgroups of a row
// slice serve it.  Integer arithmetic on the host only -- no HIP header, so a
// host compiler builds this file alone (tests/test_host_cpu.py enumerates it).
//
// This is the ONE statement of the partition: the `*_applies` predicates ask
// ws_feasible, the launchers call ws_partition, and ws_feasible is
// ws_partition into a scratch geometry.  "Applies" and "launches" are one
// decision because they are one function.
#pragma once
#include <stdint.h>

namespace pgnn {

constexpr int kWsMaxGroups = 4;
constexpr int kWsMaxSlices = 8;

// The geometry fields by themselves; EdgeWsArgs (edge_ws.h) carries the same
// fields under the same names, and the functions below take either.
struct WsGeometry {
  int groups;                   // column groups
  int xcds;                     // row slices (workgroup b -> slice b % xcds)
  int tile0[kWsMaxGroups + 1];  // group g owns column tiles [tile0[g], tile0[g+1])
  int wg0[kWsMaxGroups + 1];    // ... and local workgroups [wg0[g], wg0[g+1]) of a slice
  int balanced;                 // 1: the chip-wide tables below hold (ws_balance)
  int n_wg[kWsMaxGroups];
  short swg0[kWsMaxSlices][kWsMaxGroups + 1];
  short sbase[kWsMaxSlices][kWsMaxGroups];
};

// Row slices of a launch on `cus` CUs: `ws_xcds` when it divides them, else
// one per XCD.
inline int ws_slice_count(int cus, int ws_xcds) {
  return (ws_xcds >= 1 && cus % ws_xcds == 0) ? ws_xcds : 8;
}

enum { kWsOk = 0, kWsTooFewCus = 1, kWsNoGrouping = 2 };

// `nt` column tiles in groups of at most `ntmax`, as evenly as possible
// (C = 300: 7/6/6, C = 256: 8/8), and the cus / slices workgroups of a slice
// in proportion to the groups' tiles (largest remainder, the first maximum
// wins).  Returns kWsOk with groups / xcds / tile0 / wg0 filled, or why the
// geometry cannot be served (a.balanced is left alone; no error message).
template <class Geo>
int ws_partition(Geo &a, int nt, int ntmax, int cus, int slices) {
  a.xcds = slices;
  a.groups = (nt + ntmax - 1) / ntmax;
  const int per_slice = cus / slices;
  if (a.groups > kWsMaxGroups || per_slice < a.groups) return kWsTooFewCus;
  const int base = nt / a.groups, extra = nt % a.groups;
  int cnt[kWsMaxGroups], frac[kWsMaxGroups], used = 0;
  a.tile0[0] = 0;
  for (int g = 0; g < a.groups; ++g) {
    const int size = base + (g < extra ? 1 : 0);
    a.tile0[g + 1] = a.tile0[g] + size;
    cnt[g] = per_slice * size / nt;
    if (cnt[g] < 1) cnt[g] = 1;
    frac[g] = per_slice * size % nt;
    used += cnt[g];
  }
  if (base < ntmax - 1 || base + (extra ? 1 : 0) > ntmax || used > per_slice)
    return kWsNoGrouping;
  while (used < per_slice) {
    int best = 0;
    for (int g = 1; g < a.groups; ++g)
      if (frac[g] > frac[best]) best = g;
    ++cnt[best];
    frac[best] = -1;
    ++used;
  }
  a.wg0[0] = 0;
  for (int g = 0; g < a.groups; ++g) a.wg0[g + 1] = a.wg0[g] + cnt[g];
  return kWsOk;
}

// Can `nt` column tiles in groups of at most `ntmax` be served on `cus` CUs in
// `slices` row slices?  A geometry that cannot (e.g. 64 CUs in 32 slices for
// three column groups) takes the LDS-tile kernel or is declined like any other
// unsupported shape.
inline bool ws_feasible(int nt, int ntmax, int cus, int slices) {
  WsGeometry scratch;
  return ws_partition(scratch, nt, ntmax, cus, slices) == kWsOk;
}

// Balanced workgroup counts over the whole chip for the column groups of a
// partitioned geometry (see EdgeWsArgs::balanced).  cost[g] = relative time of
// one row tile in group g (its MFMA issue + the per-tile fixed part).  `pool`:
// the launch hands tiles out dynamically, which the balanced form excludes.
template <class Geo>
void ws_balance(Geo &a, int cus, const double *cost, bool pool) {
  const int per_slice = cus / a.xcds, total = per_slice * a.xcds;
  a.balanced = 0;
  if (a.xcds > kWsMaxSlices || a.groups < 2 || pool) return;
  double sum = 0;
  for (int g = 0; g < a.groups; ++g) sum += cost[g];
  // largest-remainder share of `total` workgroups
  int n[kWsMaxGroups], used = 0;
  double frac[kWsMaxGroups];
  for (int g = 0; g < a.groups; ++g) {
    const double x = total * cost[g] / sum;
    n[g] = (int)x;
    if (n[g] < a.xcds) n[g] = a.xcds;  // at least one per slice
    frac[g] = x - n[g];
    used += n[g];
  }
  while (used < total) {
    int best = 0;
    for (int g = 1; g < a.groups; ++g)
      if (frac[g] > frac[best]) best = g;
    ++n[best];
    frac[best] -= 1.0;
    ++used;
  }
  if (used != total) return;  // (cannot happen for the shipped shapes)
  // per slice: cumulative rounding, then repair each slice's sum to per_slice
  int prev[kWsMaxGroups] = {0, 0, 0, 0};
  for (int s = 0; s < a.xcds; ++s) {
    int c[kWsMaxGroups], tot = 0;
    for (int g = 0; g < a.groups; ++g) {
      const int cum = (int)((int64_t)n[g] * (s + 1) / a.xcds);
      c[g] = cum - prev[g];
      tot += c[g];
    }
    // (the last slice closes every group exactly; earlier slices borrow from /
    // lend to the group that is furthest ahead / behind its share)
    for (int guard = 0; tot != per_slice && guard < 64; ++guard) {
      int pick = -1;
      double worst = 0;
      for (int g = 0; g < a.groups; ++g) {
        const double ideal = (double)n[g] * (s + 1) / a.xcds;
        const double ahead = prev[g] + c[g] - ideal;
        if (tot > per_slice ? (c[g] > 1 && (pick < 0 || ahead > worst))
                            : (prev[g] + c[g] < n[g] &&
                               (pick < 0 || -ahead > worst))) {
          pick = g;
          worst = tot > per_slice ? ahead : -ahead;
        }
      }
      if (pick < 0) return;
      c[pick] += tot > per_slice ? -1 : 1;
      tot += tot > per_slice ? -1 : 1;
    }
    if (tot != per_slice) return;
    a.swg0[s][0] = 0;
    for (int g = 0; g < a.groups; ++g) {
      a.sbase[s][g] = (short)prev[g];
      a.swg0[s][g + 1] = (short)(a.swg0[s][g] + c[g]);
      prev[g] += c[g];
    }
  }
  for (int g = 0; g < a.groups; ++g) {
    if (prev[g] != n[g]) return;
    a.n_wg[g] = n[g];
  }
  a.balanced = 1;
}

}  // namespace pgnn
