// Launch plans of the v4 GEMM family, decided before any HIP call: host
// arithmetic on the arguments, the plan options and a CU count that is a
// parameter. gemm4_plan serves the dense bf16 launches (gemm4.hip) and the two
// fp8 entries (gemm4_fp8.hip), wgrad_plan the grouped weight gradients
// (gemm4_wgrad.hip); the launch functions, the workspace queries and the
// device-free queries (maeclip_gemm_plan, maeclip_gemm_fp8_plan,
// maeclip_wgrad_grouped_plan) all read the same plan. Internal: included by the
// GEMM files only.
#pragma once
#include "gemm_common.h"
#include <algorithm>

// Workspace of the in-launch split (SkPlan, gemm4_body.h): [SK_CNT_BYTES]
// arrival counters, then one SK_SLOT fp32 partial per unit, at most 2 per CU.
constexpr int SK_CNT_STRIDE = 16;                 // counter words apart (64 B)
constexpr int64_t SK_CNT_BYTES = 256 * SK_CNT_STRIDE * 4;
constexpr int64_t SK_SLOT = 256 * 256 * 4;        // one fp32 256x256 tile
constexpr int SPLIT_MAX = 2;   // the fix-up sums two partials
constexpr int WG_MAX = 48;     // problems per grouped weight-gradient launch
constexpr int SKR_CHUNKS = 16; // workgroups per remainder tile of the grouped stream-K reduce

namespace maeclip {

enum { G4_BF16 = 0, G4_FP8_ROWS = 1, G4_FP8_BLOCKS = 2 };   // Gemm4Plan::family

// this device's CU count (gemm4.hip; cached; 256 if the query fails): the one
// place of the GEMM family that asks HIP for it
int gemm4_device_ncu();

// dynamic LDS of a block with BM-row tiles (TileM<BM>::LDS_ALL, gemm4_body.h):
// two operand stages, the fp8-blocks scale images (192 rows), 8 x 4 KiB of
// epilogue scratch
constexpr int gemm4_lds_bytes(int bm) { return 2 * (2 * (bm / 2 * 128) + 2 * 16384) + (bm == 192 ? 2048 : 0) + 8 * 4096; }

struct Gemm4Plan {
  int family;               // G4_BF16, G4_FP8_ROWS, G4_FP8_BLOCKS
  int bm;                   // tile height: 256 / 192 / 128
  int S, L0, NT;            // in-launch split (S = 0: none), slice 0's K-tiles, K-tiles of the whole K
  int nsl;                  // fp32 256x256 slots in the workspace (split only)
  bool persistent;          // one block per CU loops over the tiles; else one block per (tile, slice, batch)
  int gx, gy, gz;           // grid
  int lds_bytes;
  int64_t tiles;
  int64_t workspace_bytes;  // counters + partial tiles of the split (0: none)
};

// Tile height, split and grid of one v4 launch.
//
// A plain launch (one batch, no caller split-K) takes its tile height and
// split plan from a cost model in units of one 256-row K-tile (~2.9k cycles, 64
// KiB of operand DMA per CU): a 192-row K-tile costs 0.89 of it (measured,
// encoder fc2 fwd, one round each); a tile's epilogue ~EPI_C; a split costs
// slice 0's K-tiles (its lead hides the others' publish) + F1 per other slice
// the last block reads back. MAECLIP_GEMM_BM=256 / 192 / 128 forces a tile
// height; MAECLIP_GEMM_SK=1 enables the cost model's split (default off, see
// below); MAECLIP_GEMM_SPLIT=S forces a split of S wherever it fits (A/B,
// tests). 192- and 128-row tiles need a K-contiguous A and no column sums.
// Plain launches are persistent: one block per CU (128 KiB LDS), the whole
// grid when a split is taken (the block positions the plan was made for).
//
// fp8-blocks A: always 192-row tiles (the scale images fit beside their
// operand stages there), no split. Caller split-K / batched launches: 256-row
// tiles, one block per (tile, slice, batch).
//
// ncu: the device's CU count. Diagnostic option GEMM_GRID caps it for these
// launches (contention scans, tools/gemm_grid_scan.py; unset in production); it
// does not cap the grouped weight gradients.
inline Gemm4Plan gemm4_plan(const maeclip_gemm_args& a, int family, int ncu, bool workspace_offered) {
  const int cap = option(MAECLIP_OPT_GEMM_GRID, 0);
  if (cap > 0 && cap < ncu) ncu = cap;
  const int KT = family == G4_BF16 ? 64 : 128;   // elements per K-tile (128 bytes per row)
  const int64_t gn = (a.N + 255) / 256, NT = a.K / KT;
  const bool plain = a.splitk <= 1 && a.batch == 1;
  Gemm4Plan p = {};
  p.family = family;
  p.NT = (int)NT;
  p.bm = 256;
  if (family == G4_FP8_BLOCKS) {
    p.bm = 192;
  } else if (plain) {
    const int force_bm = option(MAECLIP_OPT_GEMM_BM, 0);
    // default off: in the micro-batched step every split cost whole-step
    // throughput although it wins alone (profiles/r05/gemm_split_minK_step_ab_r5i.txt)
    const int sk_mode = option(MAECLIP_OPT_GEMM_SK, 0);   // 0 off, 1 cost model
    const int force_split = option(MAECLIP_OPT_GEMM_SPLIT, 0);
    // the cost model's split only at K >= GEMM_SPLIT_MINK (step A/B)
    const int64_t split_min_k = option(MAECLIP_OPT_GEMM_SPLIT_MINK, 0);
    const bool kc_plain = a.a_layout == LAY_KC && !a.colsum_partial;
    const bool allow192 = force_bm != 256 && force_bm != 128 && kc_plain;
    // 128-row tiles: bf16 only (KT 64); chosen by the cost model only when
    // MAECLIP_GEMM_BM128=1 (A/B) or forced by MAECLIP_GEMM_BM=128
    const bool allow128 =
        KT == 64 && kc_plain && (force_bm == 128 || (force_bm == 0 && option(MAECLIP_OPT_GEMM_BM128, 0) == 1));
    const bool allow256 = (force_bm != 192 || !allow192) && (force_bm != 128 || !allow128);
    const bool allow_sk = (sk_mode != 0 || force_split > 0) && workspace_offered && ncu <= 256;
    constexpr double EPI_C = 2.5, F1 = 2.0;
    // slice 0's lead per other slice (aligned split): about one publish of a
    // 256 x 256 fp32 partial; MAECLIP_GEMM_SPLIT_D overrides
    const int lead = option(MAECLIP_OPT_GEMM_SPLIT_D, 4);
    struct Pick {
      int bm, S, L0;
    };
    Pick best = {256, 0, 0};
    double best_cost = 1e30;
    // the best data-parallel choice: the result whenever no split plan is taken
    // (also when a forced split S does not fit the shape)
    Pick best_dp = {256, 0, 0};
    double best_dp_cost = 1e30;
    auto l0 = [&](int S) {
      // slice 0 longer by `lead` per other slice, every other slice >= 1 K-tile
      const int64_t L0 = (NT + (int64_t)(S - 1) * lead + S - 1) / S;
      return (int)std::max<int64_t>(std::min<int64_t>(L0, NT - (S - 1)), (NT + S - 1) / S);
    };
    for (int bm : {256, 192, 128}) {
      if ((bm == 256 && !allow256) || (bm == 192 && !allow192) || (bm == 128 && !allow128)) continue;
      const double c = bm == 192 ? 0.89 : bm == 128 ? 0.72 : 1.0;
      const int64_t T = (a.M + bm - 1) / bm * gn, R = T % ncu;
      const double dp = (double)((T + ncu - 1) / ncu) * (NT * c + EPI_C);
      if (dp < best_dp_cost - 1e-9) {
        best_dp_cost = dp;
        best_dp = {bm, 0, 0};
      }
      if (dp < best_cost - 1e-9 && force_split == 0) {
        best_cost = dp;
        best = {bm, 0, 0};
      }
      // split: 192-row tiles only (the 256-row body has no registers left for
      // the fix-up: its split instantiation spilled inside the K loop)
      if (!allow_sk || bm != 192 || (force_split == 0 && (R == 0 || a.K < split_min_k))) continue;
      for (int S = 2; S <= SPLIT_MAX; ++S) {
        if ((force_split > 0 && S != force_split) || T * S > 2 * ncu || T > 256 || NT < 2 * S) continue;
        const int64_t rounds = (T * S + ncu - 1) / ncu;
        // the publish of slices >= 1 runs while slice 0 computes its lead
        const double cost = (double)rounds * l0(S) * c + EPI_C + F1 * (S - 1);
        if (force_split > 0 || cost < best_cost - 1e-9) {
          best_cost = force_split > 0 ? -1.0 : cost;
          best = {bm, S, l0(S)};
        }
      }
    }
    const Pick& r = best.S > 0 ? best : best_dp;
    p.bm = r.bm;
    p.S = r.S;
    p.L0 = r.L0;
  }
  p.tiles = (a.M + p.bm - 1) / p.bm * gn;
  p.lds_bytes = gemm4_lds_bytes(p.bm);
  p.persistent = plain;
  p.gx = (int)(plain && (p.S > 0 || p.tiles >= ncu) ? ncu : p.tiles);
  p.gy = plain ? 1 : std::max(a.splitk, 1);
  p.gz = (int)a.batch;
  if (p.S > 0) {
    p.nsl = 2 * ncu;
    p.workspace_bytes = SK_CNT_BYTES + (int64_t)p.nsl * SK_SLOT;
  }
  return p;
}

// out[8] of the device-free queries maeclip_gemm_plan / maeclip_gemm_fp8_plan
inline void gemm4_plan_out(const Gemm4Plan& p, int32_t out[8]) {
  const int32_t v[8] = {p.bm, p.S, p.L0, p.gx, p.gy, p.gz, p.lds_bytes, p.persistent ? 1 : 0};
  std::copy(v, v + 8, out);
}

// ------------------------------------------------- grouped weight gradients
// Slices per tile for one launch of T tiles: the S minimising the number of
// waves of units per tile-K, ceil(T*S/ncu)/S, where S > 1 must beat S = 1 by
// 15% to pay for the fp32 slab write + reduce, and S <= 4 (the slab traffic
// grows with S while the wave quantisation it fixes does not); every slice
// keeps >= 16 K-tiles. The encoder's 48 dW (1296 tiles: 5.06 waves) take S = 1, the
// decoder's 32 (384 tiles: 1.5 waves) S = 2.
inline int wg_splits(int T, int64_t M, int ncu) {
  const double c1 = (double)((T + ncu - 1) / ncu);
  int best = 1;
  double best_cost = c1;
  for (int S = 2; S <= 4; ++S) {
    if (M / 64 / S < 16) break;
    const double cost = (double)((T * S + ncu - 1) / ncu) / S;
    if (cost < 0.85 * c1 && cost < best_cost - 1e-9) {
      best = S;
      best_cost = cost;
    }
  }
  return best;
}

// Stream-K remainder: K-tiles per block when the T tiles leave a partial last
// wave on the grid (0 = none). Each block then runs floor(T / ncu) whole tiles
// plus skw K-tiles of the remainder, so every block does the same work; a
// block's range cuts at most two tiles (two 256 KB fp32 slots). Below 8
// K-tiles per block the slot write + reduce outweighs the balance.
inline int wg_skw(int T, int64_t M, int ncu) {
  const bool enabled = option(MAECLIP_OPT_WG_SK, 1) != 0;   // 0: uniform split-K slices instead (A/B)
  const int G = ncu, R = T % G;
  if (R == 0 || !enabled) return 0;
  const int64_t skw = ((int64_t)R * (M / 64) + G - 1) / G;
  return skw >= 8 ? (int)skw : 0;
}

inline int wg_tiles(const maeclip_wgrad_problem& q) { return (int)(((q.N + 255) / 256) * ((q.K + 255) / 256)); }

enum { WG_REDUCE_NONE = 0, WG_REDUCE_SLABS = 1, WG_REDUCE_STREAMK = 2 };   // WgradPlan::reduce

struct WgradPlan {
  int T;                     // 256x256 output tiles of all problems
  int S;                     // uniform split-K slices per tile (1: none)
  int skw, Tdp, NT;          // stream-K remainder (skw > 0, else all 0): K-tiles per block, whole tiles, K-tiles per tile
  int grid;                  // blocks of the main launch
  int reduce, rgx, rgy;      // second launch (WG_REDUCE_*) and its grid
  int tile_begin[WG_MAX];    // prefix sum of tiles
  int64_t slab_off[WG_MAX];  // floats into the workspace, S > 1 only
  int64_t workspace_bytes;
};

// One grouped launch of n <= WG_MAX problems sharing the token count M (the
// GEMM K) on ncu CUs: a stream-K remainder if the tiles leave a partial last
// wave with enough K per block, else uniform slices if they pay, else whole
// tiles only.
inline WgradPlan wgrad_plan(const maeclip_wgrad_problem* pr, int n, int64_t M, int ncu) {
  WgradPlan p = {};
  int64_t nk = 0, maxnk = 0;
  for (int i = 0; i < n; ++i) {
    p.tile_begin[i] = p.T;
    p.T += wg_tiles(pr[i]);
    nk += pr[i].N * pr[i].K;
    maxnk = std::max(maxnk, pr[i].N * pr[i].K);
  }
  p.S = 1;
  p.skw = wg_skw(p.T, M, ncu);
  if (p.skw > 0) {
    p.NT = (int)(M / 64);
    p.Tdp = p.T - p.T % ncu;
    p.grid = ncu;
    p.reduce = WG_REDUCE_STREAMK;
    p.rgx = p.T - p.Tdp;
    p.rgy = SKR_CHUNKS;
    p.workspace_bytes = (int64_t)2 * ncu * 65536 * 4;   // two fp32 256x256 slots per block
    return p;
  }
  p.S = wg_splits(p.T, M, ncu);
  p.grid = std::min(p.T * p.S, ncu);
  if (p.S > 1) {
    int64_t so = 0;
    for (int i = 0; i < n; ++i) {
      p.slab_off[i] = so;
      so += (int64_t)p.S * pr[i].N * pr[i].K;
    }
    p.reduce = WG_REDUCE_SLABS;
    p.rgx = (int)std::min<int64_t>((maxnk / 4 + 255) / 256, 1024);
    p.rgy = n;
    p.workspace_bytes = (int64_t)p.S * nk * 4;
  }
  return p;
}

}  // namespace maeclip
