// Plan layer of the convolution GEMMs: which kernel serves a forward / data-gradient or weight-gradient problem, in how
// many parts, on which grid and with how much scratch.  Pure host code: no HIP types, no device code, compiles with the
// host compiler alone.  conv_dispatch.hip launches what a plan says; the query entry points (dadet_conv_forward_plan,
// dadet_conv_wgrad_plan, the *_variant / *_workspace_bytes / *_group_plan queries) are views of the same plan.
//
// Every planning switch is read HERE and nowhere else, through sw() below.  Read time: `process` = once, at the first plan
// that consults it; `call` = at every plan (tests and A/B runs flip these at run time).
//   switch                      default  read     meaning
//   DADET_BIG_GEMM              1        process  start-up value of the large-tile mode (dadet_set_big_gemm changes it)
//   DADET_BIG_SPLITS            plan     call     forces the K parts of a large tile (1 .. 8); switches the tail cut off
//   DADET_BIG_TILE_N            256      call     large-tile mode 2 only: 128 picks the 256 x 128 tile
//   DADET_BIG_TAIL              1        call     0: no tail cut
//   DADET_WS_1X1                1        call     0: no weight-stationary 1x1 kernel
//   DADET_WS_K256_BN            128      call     64: K = 256 keeps 64-column panels
//   DADET_EPILOGUE_V4           1        call     0: the 4-byte epilogue (which the weight-stationary / large tiles lack)
//   DADET_FWD_MIN_TILES128      256      process  128 x 128 tiles from this many tiles on
//   DADET_SHORTK_MAX            256      process  64 x 64 tiles for whole-K-tile reductions up to this length
//   DADET_FWD_VARIANT           plan     call     forces the tile variant (0 .. 2) of the split kernels
//   DADET_STREAMK               1        call     0: no stream-K tail
//   DADET_STREAMK_SMALL         mode     call     the below-one-pass stream-K case: on in mode 3, off in mode 4
//   DADET_SPLITK                1        process  0: no split-K
//   DADET_WGRAD_MIN_ROWS        128      call     fewest rows per part of the 128 x 128 weight gradient (>= 32)
//   DADET_WGRAD_SPLITS          plan     call     forces the parts of the 128 x 128 weight gradient
//   DADET_WGRAD_BIG             1        process  0: no 256 x 256 weight gradient
//   DADET_WGRAD_BIG_MIN_TILES   8        process  fewest tiles for a 256 x 256 weight gradient of its own
//   DADET_WGRAD_BIG_SPLITS      plan     call     forces the parts of the 256 x 256 weight gradient
//   DADET_WGRAD_GROUP_128       1        process  0: no grouped launch of the 128 x 128 weight gradient
//   DADET_WGRAD_GROUP_ROWS      plan     call     forces the common rows per part of a grouped launch
//   DADET_ABLATE                0        process  profiling only: stage mask of the split kernel; no stream-K tail with it
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include "../../include/dadet.h"

namespace dadet {
namespace plan {

constexpr int kCUs = 256;             // MI355X (common.h: kNumCU)
constexpr int kBK = 32;               // K-tile of every GEMM kernel
constexpr int kWsRows = 256;          // rows per workgroup pass of the weight-stationary kernel: 8 waves x 32
constexpr int kGroupMax = 4;          // problems per grouped weight-gradient launch
// arrival counters per stream: the stream-K tail's, + the symmetric two-part meeting of conv_big.hip: four words per tile
constexpr int kSkCounters = 4096 + 4 * 2048;

inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// the one place a planning switch is read
inline const char* sw(const char* name) { return getenv(name); }
inline bool sw_off(const char* name) { const char* e = sw(name); return e && e[0] == '0'; }
inline int sw_int(const char* name, int dflt) { const char* e = sw(name); return e ? atoi(e) : dflt; }

inline int big_gemm_default() {
  const int v = sw_int("DADET_BIG_GEMM", 1);
  return v >= 0 && v <= 2 ? v : 1;
}
inline int ablate() {
  static const int v = sw_int("DADET_ABLATE", 0);
  return v;
}

// ---- the GEMM view of a descriptor ----------------------------------------------------------------------------------
struct Gemm {
  int M, K, os;                       // rows N*Ho*Wo, reduction KH*KW*Cin, output scatter stride
  uint64_t x_bytes, w_bytes, y_bytes;
};
inline Gemm gemm_of(const dadet_conv_desc* d) {
  Gemm g;
  g.M = (int)((int64_t)d->N * d->Ho * d->Wo);
  g.K = (int)((int64_t)d->KH * d->KW * d->Cin);
  g.os = d->out_spatial_stride > 0 ? d->out_spatial_stride : 1;
  g.x_bytes = (uint64_t)d->N * d->H * d->W * d->Cin * 4;
  g.w_bytes = (uint64_t)d->Cout * g.K * 4;
  g.y_bytes = (uint64_t)d->N * d->OutH * d->OutW * d->Cout * 4;
  return g;
}

// ---- forward / data gradient ----------------------------------------------------------------------------------------
enum FwdFamily {
  kFwdExact = 0,      // conv_fwd_kernel<TM,TN>: exact fp32 (mode 0)
  kFwdSplit = 1,      // conv_fwd_split_kernel<TM,TN,MODE>
  kFwdSplitSk = 2,    // conv_fwd_split_sk_kernel<MODE>: 128 x 128 tiles with a stream-K tail
  kFwdSplitK = 3,     // conv_fwd_split_kernel over K ranges + splitk_reduce_kernel
  kFwdWs = 4,         // conv1x1_ws_kernel<K,BN,MODE>
  kFwdBig256 = 5,     // conv_big_kernel<256>
  kFwdBig128 = 6,     // conv_big128_kernel
  kFwdFamilies = 7
};

// stream-K tail of the 128 x 128 split kernel: tiles [0, dp_tiles) one per workgroup, the K-tile iterations of the last
// sk_tiles tiles in `units` contiguous ranges of `iters`; a tile meets at most max_parts partial tiles
struct SkPlan { int dp_tiles, sk_tiles, units, iters, max_parts; };

struct FwdPlan {
  int family;
  int variant;          // the label of dadet_conv_forward_variant: 0 .. 2 tile variant, 3 weight-stationary, 4 / 5 large tiles
  int tm, tn;           // exact / split kernels: 32-row blocks per wavefront (tile = 64 tm x 64 tn)
  int tiles_m, tiles_n;
  int ksplit, splits;   // split-K: K elements per range (0: whole), number of ranges (grid.y)
  SkPlan sk;
  int big_splits, big_body;
  int ws_k, ws_bn, ws_erows;            // weight-stationary: template parameters
  int ws_parts, ws_panels[3], ws_grid[3];   // ... its 1 - 3 launches over column-panel ranges
  int epi_v4;           // the 16-byte epilogue is usable (ConvArgs::epi_v4)
  int grid;             // workgroups of the (first) GEMM launch
  size_t workspace_bytes;   // per-stream scratch the launch needs
  bool counters;        // ... and the stream's arrival counters
  const char* name;     // as the profiler spells it
};

// tile variant chosen for a forward / dgrad GEMM of M rows and Cout columns
//   0: 128x128 (TM=2,TN=2)   1: 128x64 (TM=2,TN=1)   2: 64x64 (TM=1,TN=1)
inline int fwd_variant(int M, int Cout) {
  const int64_t t128 = (int64_t)cdiv(M, 128) * cdiv(Cout, 128);
  // 128x128 tiles from one workgroup per CU on: tools/fwd_sweep.py, res4 3x3 256->256 0.115 ms against 0.128 ms with
  // 128x64 tiles, res4 1x1 1024->256 0.061 against 0.064 (with two GEMM streams the step did not notice; with one: +0.3%)
  static const int min_tiles = sw_int("DADET_FWD_MIN_TILES128", kCUs);
  if (Cout > 64 && t128 >= min_tiles) return 0;
  if (Cout > 32) {
    const int64_t t64 = (int64_t)cdiv(M, 128) * cdiv(Cout, 64);
    if (t64 >= kCUs || M <= 64 * 64) return 1;
    return 2;
  }
  return 1;
}

// Tile variant of the split forward / data-gradient GEMM.  Short reductions are HBM bound, and a workgroup's load /
// compute / store phases overlap only across the workgroups that share a CU: 64x64 tiles (30 KB of LDS, 5 workgroups per
// CU instead of 2) run the K <= 256 layers 3 - 38% faster (tools/gemm_table.py: res2 1x1 64->256 0.211 -> 0.153 ms, res3
// 1x1 128->512 0.156 -> 0.130).  Only whole K-tiles (the K = 76 RPN data gradient got 44% slower) and only where the
// 128x128 tile would be chosen.  DADET_FWD_VARIANT forces a variant (tools/fwd_sweep.py).
inline int split_fwd_variant(int M, int Cout, int K) {
  int variant = fwd_variant(M, Cout);
  static const int kmax = sw_int("DADET_SHORTK_MAX", 256);
  if (variant == 0 && K <= kmax && K % kBK == 0) variant = 2;
  if (const char* e = sw("DADET_FWD_VARIANT")) {
    const int v = atoi(e);
    if (v >= 0 && v <= 2) variant = v;
  }
  return variant;
}

// Weight-stationary 1x1 kernel for K = 64 / 128 / 256 (conv_ws.hip).
inline bool ws_eligible(const dadet_conv_desc* d, const Gemm& g, bool epi_v4) {
  if (sw_off("DADET_WS_1X1")) return false;
  if (d->KH != 1 || d->KW != 1 || d->pad != 0 || g.os != 1) return false;
  if (g.K != 64 && g.K != 128 && g.K != 256) return false;
  if (!epi_v4) return false;                                // 16-byte epilogue: Cout % 4 == 0, aligned tensors
  if (g.x_bytes >= 0x80000000ull || g.w_bytes >= 0x80000000ull) return false;   // beyond the kernel's invalid-row offset
  if (d->Cout < 128 || d->Cout % 32) return false;          // narrow layers stay on the 128 x 64 tiles
  if (g.M < 64 * kWsRows) return false;                     // too few slabs to fill the chip's 256 workgroups
  return true;
}

// panel width per K: the three (mode 4: two) planes of BN x (K + 8) 16-bit terms plus the epilogue slices (40 KB) must
// fit 160 KB: 128 columns for K = 64 / 128, 64 for K = 256
inline void ws_plan(const dadet_conv_desc* d, const Gemm& g, int gemm_mode, FwdPlan* p) {
  p->ws_k = g.K;
  p->ws_bn = g.K == 256 ? 64 : 128;
  p->ws_erows = 32;
  if (gemm_mode == 4 && g.K == 256) {
    // K = 256: 128-column panels where the layer has at least 256 columns (res4 conv3 and its mirror, 1024 columns:
    // a workgroup then stores 512 contiguous bytes per row instead of 256, and the activations are read by 8 panels
    // instead of 16) — the weight planes take 132 KB, the epilogue slices are halved to fit.  DADET_WS_K256_BN=64: off
    const bool wide = sw_int("DADET_WS_K256_BN", 128) != 64;
    if (wide && d->Cout >= 256) { p->ws_bn = 128; p->ws_erows = 16; }
  }
  const int panels_all = cdiv(d->Cout, p->ws_bn);
  p->tiles_m = cdiv(g.M, kWsRows);
  p->tiles_n = panels_all;
  // one workgroup per CU: `panels` x G with G a multiple of 8 (the kernel's XCD mapping) and at most one slab group per slab
  const int need = cdiv(p->tiles_m, 8) * 8;
  auto groups = [&](const int panels) {
    int G = (kCUs / panels) / 8 * 8;
    if (G < 8) G = 8;
    return G > need ? need : G;
  };
  // A panel count that does not divide the chip (18 panels of the deformable blocks' data gradient, 2304 columns: 18 x 8 =
  // 144 workgroups walk 8 slabs each) is cut into 2 or 3 launches over column ranges when that shortens the walk: launches
  // x slabs per workgroup is the launch's length in slab times (9 panels x 24 groups: 2 x 3 instead of 8).
  int parts = 1, best = cdiv(p->tiles_m, groups(panels_all));
  for (int q = 2; q <= 3 && q <= panels_all; ++q) {
    const int cost = q * cdiv(p->tiles_m, groups(cdiv(panels_all, q)));
    if (cost * 8 < best * 7) { best = cost; parts = q; }      // (at least an eighth shorter: every launch loads its panels anew)
  }
  const int per = cdiv(panels_all, parts);
  p->ws_parts = 0;
  for (int p0 = 0; p0 < panels_all; p0 += per) {
    const int panels = panels_all - p0 < per ? panels_all - p0 : per;
    p->ws_panels[p->ws_parts] = panels;
    p->ws_grid[p->ws_parts++] = panels * groups(panels);
  }
  p->grid = p->ws_grid[0];
}

// which large-tile kernel (conv_big.hip) serves this problem: 0 none, 1 the 256 x 256 tile, 2 the 256 x 128 tile.
// big_mode 0: never, 1: where the plan below expects a gain, 2: wherever the kernel is applicable (tests)
inline int big_variant(const dadet_conv_desc* d, const Gemm& g, bool epi_v4, int big_mode) {
  if (big_mode == 0) return 0;
  if (g.os != 1 || !epi_v4 || d->Cin % 32 != 0 || g.K % 32 != 0 || d->Cout % 4 != 0) return 0;
  if (g.x_bytes >= 0x7FFFFF00ull || g.w_bytes >= 0x7FFFFF00ull || g.y_bytes >= 0x7FFFFF00ull) return 0;
  if (g.M >= (1 << 24)) return 0;
  if (big_mode == 2) return sw_int("DADET_BIG_TILE_N", 256) == 128 ? 2 : 1;   // tests: wherever applicable
  // plan (tools/native/gemm_lab.hip, profiles/r05_gemm_lab.txt): +29 .. +35% against the 128 x 128 kernel where the grid fills
  // the chip with at most two K parts per tile; 64 tiles of 256 x 256 in four parts — res4 3x3 — only equal it (the last
  // part reads 768 KB), so layers of up to 256 output channels take the 256 x 128 tile
  if (g.K < 512 || g.M < 4096 || d->Cout < 128) return 0;
  const int tm = cdiv(g.M, 256);
  // 129 .. 256 output channels over at least 96 row tiles (the pyramid's 256-channel 3x3 / lateral layers on P2 / P3,
  // M = 262144 / 65536): one column of 256 x 256 tiles fills the chip without any K split, on the kernel whose loop holds
  // the matrix pipe 84% of the time instead of 61% (round 6)
  if (d->Cout > 128 && d->Cout <= 256 && tm >= 96) return 1;
  if (d->Cout <= 256) return tm * cdiv(d->Cout, 128) >= 96 ? 2 : 0;
  return tm * cdiv(d->Cout, 256) >= 96 ? 1 : 0;
}

// Number of K ranges a large tile's reduction is cut into.  Reductions of K >= 8192 (the RPN 3x3 conv) are ALWAYS cut in
// two: the hand-over (the last part reads one parked tile, ~4 us) is small against 288 K-tiles per tile, and the result of
// that layer then does not depend on how many rows the launch happens to have — the overlapped training schedule runs the
// RPN head on the labelled images only, the plain one on all of them, and tests/test_full_size_gpu.py asks both for the
// same sampled ROIs.  Shorter reductions are cut in two only when the grid leaves half of the CUs without a tile.  (The
// bound was K >= 4096 until the box head of the recipes that pool BOTH images showed what that costs: res5 3x3 on 512 ROIs
// is 196 tiles — two parts are 392 workgroups, two rounds on 256 CUs, where one part per tile is one round: `da` 17.77 ->
// 17.53, `triplet` 21.81 -> 21.60 ms per step.  The box head sees the same rows in every schedule.)
// forced: the value of DADET_BIG_SPLITS (tests and A/B runs force the part count), or null
inline int big_split_plan(const int tiles, const int nk, const char* forced) {
  if (forced) {
    const int v = atoi(forced);
    if (v >= 1 && v <= 8 && nk / v >= 1) return v;
  }
  if (nk >= 256) return 2;
  return (tiles <= kCUs / 2 && nk >= 16) ? 2 : 1;
}

// Tail cut: a grid of a few tiles more than a multiple of the CU count (the res5 head on 512 ROIs: 98 x 8 = 784 tiles of
// 256 x 256, 3.06 rounds) runs its last, nearly empty round for a whole tile's time — a fifth of `M=25088 N=2048 K=512`'s
// 265 us.  The tiles of that round (at most a quarter of the chip) are cut into two parts instead (the symmetric meeting):
// twice the workgroups, half the round.  -> number of whole-tile workgroups (0: no tail cut).  DADET_BIG_TAIL=0: never.
inline int big_tail_plan(const int tiles, const int nk) {
  if (sw_off("DADET_BIG_TAIL")) return 0;
  const int tail = tiles % kCUs;
  if (tiles <= kCUs || tiles > 2048 || tail == 0 || tail > kCUs / 4 || nk < 4) return 0;
  return tiles - tail;
}

// the large-tile launch: tile grid, K parts, tail cut, workgroups, scratch
inline void big_plan(const dadet_conv_desc* d, const Gemm& g, int variant, FwdPlan* p) {
  const int bn = variant == 2 ? 128 : 256;
  p->tiles_m = cdiv(g.M, 256);
  p->tiles_n = cdiv(d->Cout, bn);
  const int tiles = p->tiles_m * p->tiles_n, nk = g.K / 32;
  const char* forced = sw("DADET_BIG_SPLITS");
  p->big_splits = tiles <= 2048 ? big_split_plan(tiles, nk, forced) : 1;      // (the counters' bound)
  p->big_body = p->big_splits == 1 && !forced ? big_tail_plan(tiles, nk) : 0; // (a forced uniform cut: no tail cut)
  if (p->big_body) p->big_splits = 2;
  const int cut = tiles - p->big_body;                  // tiles whose reduction is cut into big_splits parts
  p->grid = p->big_body + cut * p->big_splits;
  // the parts of a tile meet in [tile][part][256 x bn] floats of scratch under the stream's counters
  p->workspace_bytes = p->big_splits > 1 ? (size_t)cut * p->big_splits * 256 * bn * sizeof(float) : 0;
  p->counters = p->workspace_bytes != 0;
}

// Stream-K tail plan for the 128x128 split kernel (conv_fwd_split_sk_kernel).  Returns false when the plain grid is at
// least as good: the last pass of the tile grid over the 2 x 256 workgroup slots is (nearly) full, or K is so short that
// parking / summing partial tiles would cost more than the idle slots.
inline bool streamk_plan(int M, int Cout, int K, int variant, int gemm_mode, SkPlan* p) {
  if (sw_off("DADET_STREAMK") || variant != 0 || ablate()) return false;
  const int slots = 2 * kCUs;
  const int tiles = cdiv(M, 128) * cdiv(Cout, 128);
  const int nk = cdiv(K, kBK);
  const int tail = tiles % slots;
  // a grid below one pass is not stream-K'd: cutting 256 tiles into 512 halves measured 7 - 22% SLOWER (the partial-tile
  // round trip costs more than the second workgroup per CU gains; tools/streamk_bench.py)
  if (tiles > kCUs && tiles < slots && nk >= 32) {
    // between one workgroup per CU and two (e.g. the 392 tiles of the res5 GEMMs over 256 ROIs): all workgroups are
    // resident at once, but 136 CUs run two of them and 120 run one — the launch lasts as long as the pairs.  All tiles
    // become stream-K tiles: 512 equal ranges, every CU gets two.  DADET_STREAMK_SMALL=0 switches this case off.
    // Mode 4 (three MFMAs per K=16): a tile's K loop is short enough that parking / summing the partial tiles and the
    // operand panels the ranges no longer share cost more than the uneven CUs — `img_only` 15.27 -> 14.81 ms, R-101-FPN-DCN
    // 49.1 -> 46.6 ms with this case off (three alternating runs each on one box); it stays on for the six-MFMA mode 3,
    // where it was measured (+18% on the res5 GEMMs).  DADET_STREAMK_SMALL = 0 / 1 forces it.
    const char* small = sw("DADET_STREAMK_SMALL");
    if (small ? small[0] == '0' : gemm_mode == 4) return false;
    p->dp_tiles = 0;
    p->sk_tiles = tiles;
    p->iters = cdiv(tiles * nk, slots);
    p->units = cdiv(tiles * nk, p->iters);
    p->max_parts = cdiv(nk, p->iters) + 1;
    return true;
  }
  if (tail == 0 || nk < 16 || tiles < slots || tail > kSkCounters) return false;
  if (tail > slots * 7 / 8) return false;                 // the last pass is full enough
  if (tiles > 6 * slots && tail > slots / 2) return false;  // many passes: the idle share is small
  p->dp_tiles = tiles - tail;
  p->sk_tiles = tail;
  // ranges of at least 8 K-tiles: a short tail (e.g. 32 tiles of 64 K-tiles behind three full passes) is spread over
  // fewer workgroups rather than cut into slivers
  p->iters = cdiv(tail * nk, slots);
  if (p->iters < 8) p->iters = 8;
  p->units = cdiv(tail * nk, p->iters);
  p->max_parts = cdiv(nk, p->iters) + 1;
  return true;
}

// ---- split-K for GEMMs whose tile grid cannot fill the chip (the M = 512 linear layers of the box / instance heads:
// 4 x 16 workgroups walking K = 2048 alone took 40 - 70 us each, one after the other in the loss turn-around).
// The K range is cut over blockIdx.y, partial sums go to the per-stream scratch, and one pass sums them in split order and
// applies the epilogue.  -> number of K elements per split (multiple of the K-tile), or 0 when the launch should not be split
inline int splitk_plan(int M, int Cout, int K, int os, int variant) {
  static const bool enabled = !sw_off("DADET_SPLITK");
  if (!enabled || os != 1 || Cout % 4 != 0 || K < 256) return 0;
  const int bm = variant == 2 ? 64 : 128, bn = variant == 0 ? 128 : 64;
  const int tiles = cdiv(M, bm) * cdiv(Cout, bn);
  if (tiles > kCUs / 2) return 0;
  int want = cdiv(2 * kCUs, tiles);
  if (want > K / 128) want = K / 128;     // at least four K-tiles per workgroup
  if (want < 2) return 0;
  const int ksplit = cdiv(cdiv(K, want), kBK) * kBK;
  return cdiv(K, ksplit) >= 2 ? ksplit : 0;
}

inline const char* fwd_name(int family, int variant, int gemm_mode, int ws_k, int ws_bn) {
  static const char* const exact[3] = {"conv_fwd_kernel<2,2>", "conv_fwd_kernel<2,1>", "conv_fwd_kernel<1,1>"};
  static const char* const split[3][3] = {
      {"conv_fwd_split_kernel<2,2,2>", "conv_fwd_split_kernel<2,1,2>", "conv_fwd_split_kernel<1,1,2>"},
      {"conv_fwd_split_kernel<2,2,3>", "conv_fwd_split_kernel<2,1,3>", "conv_fwd_split_kernel<1,1,3>"},
      {"conv_fwd_split_kernel<2,2,4>", "conv_fwd_split_kernel<2,1,4>", "conv_fwd_split_kernel<1,1,4>"}};
  static const char* const ws[2][4] = {
      {"conv1x1_ws_kernel<64,128,3>", "conv1x1_ws_kernel<128,128,3>", "conv1x1_ws_kernel<256,64,3>", "conv1x1_ws_kernel<256,128,3>"},
      {"conv1x1_ws_kernel<64,128,4>", "conv1x1_ws_kernel<128,128,4>", "conv1x1_ws_kernel<256,64,4>", "conv1x1_ws_kernel<256,128,4>"}};
  switch (family) {
    case kFwdExact: return exact[variant];
    case kFwdWs: return ws[gemm_mode == 4][ws_k == 64 ? 0 : ws_k == 128 ? 1 : ws_bn == 64 ? 2 : 3];
    case kFwdBig256: return "conv_big_kernel<256>";
    case kFwdBig128: return "conv_big128_kernel";
    default: return split[gemm_mode - 2][variant];      // (a stream-K / split-K launch is reported under its tile variant)
  }
}

// which kernel serves the problem, as dadet_conv_forward_variant labels it: 3 weight-stationary 1x1 (K <= 256), 4 / 5 the
// 256 x 256 / 256 x 128 tile (long K), 0 .. 2 the tile variant of the split (exact: mode 0) kernels
inline int fwd_label(const dadet_conv_desc* d, const Gemm& g, bool epi_v4, int gemm_mode, int big_mode) {
  if (gemm_mode >= 3 && ws_eligible(d, g, epi_v4)) return 3;
  if (const int bv = gemm_mode == 4 ? big_variant(d, g, epi_v4, big_mode) : 0) return 3 + bv;
  return gemm_mode != 0 ? split_fwd_variant(g.M, d->Cout, g.K) : fwd_variant(g.M, d->Cout);
}

// The forward / data-gradient plan under a given answer to "is the 16-byte epilogue usable" (plan_forward below asks the
// switch and the alignment; the label query dadet_conv_forward_variant assumes it, as it always has).
// aligned16: y and the epilogue operands (scale, bias, addend, mask_ref) are 16-byte aligned.
// An empty batch (N == 0) launches nothing: its plan is the label alone, every number zero.
inline FwdPlan plan_forward_epi(const dadet_conv_desc* d, bool epi_v4, bool aligned16, int gemm_mode, int big_mode) {
  FwdPlan p = {};
  const Gemm g = gemm_of(d);
  p.epi_v4 = epi_v4;
  p.splits = 1;
  p.variant = fwd_label(d, g, epi_v4, gemm_mode, big_mode);
  p.family = p.variant == 3 ? kFwdWs : p.variant == 4 ? kFwdBig256 : p.variant == 5 ? kFwdBig128
                                                                  : (gemm_mode != 0 ? kFwdSplit : kFwdExact);
  if (g.M == 0) {                            // nothing to plan
  } else if (p.variant == 3) {
    ws_plan(d, g, gemm_mode, &p);
  } else if (p.variant > 3) {
    big_plan(d, g, p.variant - 3, &p);
  } else {
    p.tm = p.variant == 2 ? 1 : 2;
    p.tn = p.variant == 0 ? 2 : 1;
    p.tiles_m = cdiv(g.M, 64 * p.tm);
    p.tiles_n = cdiv(d->Cout, 64 * p.tn);
    p.grid = p.tiles_m * p.tiles_n;
    if (gemm_mode != 0) {
      if (streamk_plan(g.M, d->Cout, g.K, p.variant, gemm_mode, &p.sk)) {
        // partial tiles in the per-stream scratch (reused in stream order), arrival counters in their own buffer
        p.family = kFwdSplitSk;
        p.workspace_bytes = sizeof(float) * (size_t)p.sk.sk_tiles * p.sk.max_parts * 128 * 128;
        p.counters = true;
        p.grid = p.sk.dp_tiles + p.sk.units;
      } else if (const int ksplit = aligned16 ? splitk_plan(g.M, d->Cout, g.K, g.os, p.variant) : 0) {
        p.family = kFwdSplitK;
        p.ksplit = ksplit;
        p.splits = cdiv(g.K, ksplit);
        p.workspace_bytes = sizeof(float) * (size_t)g.M * d->Cout * p.splits;
        p.grid *= p.splits;
      }
    }
  }
  p.name = fwd_name(p.family, p.variant <= 2 ? p.variant : 0, gemm_mode, p.ws_k, p.ws_bn);
  return p;
}

inline FwdPlan plan_forward(const dadet_conv_desc* d, bool aligned16, int gemm_mode, int big_mode) {
  const int os = d->out_spatial_stride > 0 ? d->out_spatial_stride : 1;
  // DADET_EPILOGUE_V4=0: the 4-byte epilogue (A/B runs, bit-identity test)
  const bool epi_v4 = !sw_off("DADET_EPILOGUE_V4") && os == 1 && d->Cout % 4 == 0 && aligned16;
  return plan_forward_epi(d, epi_v4, aligned16, gemm_mode, big_mode);
}

// ---- weight gradient ------------------------------------------------------------------------------------------------
enum WgradFamily {
  kWgradExact = 0,          // conv_wgrad_kernel: exact fp32 (mode 0), 128 x 128 tiles
  kWgradSplit = 1,          // conv_wgrad_split_kernel<MODE, false>
  kWgradSplitSmallMap = 2,  // conv_wgrad_split_kernel<MODE, true>: maps narrower than one K-step of rows (Wo < 32)
  kWgradBig = 3,            // conv_wgrad_big_kernel: 256 x 256 tiles (mode 4)
  kWgradFamilies = 4
};

struct WgradPlan {
  int family;
  int tiles_co, tiles_kc, splits, rows_per_split;   // rows_per_split is a multiple of 32
  int grid;
  size_t workspace_bytes;   // [splits][...] partial sums the caller provides (0: dw is written directly)
  const char* name;
};

inline bool wgrad_big_enabled(int gemm_mode, int big_mode) {
  static const bool enabled = !sw_off("DADET_WGRAD_BIG");   // A/B runs
  return enabled && big_mode != 0 && gemm_mode == 4;
}

// Split plan of the 128 x 128 weight gradient: the (co tile, kc tile) grid is small (4 ... 576 tiles), so the reduction
// over the M = N*Ho*Wo rows is cut into `splits` ranges to fill the 2 x 256 workgroup slots of the chip.  The number of
// workgroups matters in steps of 512: one more than a multiple of 512 costs a whole extra pass of mostly idle CUs
// (tools/wgrad_sweep.py: res5 3x3, 144 tiles: 3 splits = 432 workgroups 0.80 ms, 4 splits = 576 workgroups 0.99 ms,
// 7 splits = 1008 workgroups 0.73 ms).  The plan minimises a small cost model fitted to that sweep, in microseconds:
// passes x (fixed + K-steps x step time) + the reduction pass over the partial results.
inline void wgrad_plan(const dadet_conv_desc* d, WgradPlan* p) {
  const Gemm g = gemm_of(d);
  const int M = g.M, K = g.K;
  p->tiles_co = cdiv(d->Cout, 128);
  p->tiles_kc = cdiv(K, 128);
  const int tiles = p->tiles_co * p->tiles_kc;
  int min_rows = 128;                           // at least 4 K-steps per split
  { const int v = sw_int("DADET_WGRAD_MIN_ROWS", 0); if (v >= 32) min_rows = v; }
  const int max_splits = cdiv(M, min_rows);
  const int slots = 2 * kCUs;                   // two workgroups per CU
  const double kStep2 = 3.0, kStep1 = 2.0;      // one 32-row K-step with two / one workgroup(s) on the CU
  const double kFixed = 9.0;                    // prologue + epilogue of a workgroup
  const double dw_bytes = 4.0 * d->Cout * (double)K;
  int best = 1;
  double best_cost = 1e30;
  for (int s = 1; s <= max_splits && (s == 1 || (long)tiles * s <= 8 * slots); ++s) {
    int rows = cdiv(cdiv(M, s), 32) * 32;
    if (cdiv(M, rows) != s) continue;           // same plan as a smaller s
    const double steps = rows / 32.0;
    const long wgs = (long)tiles * s;
    const long full = wgs / slots, rem = wgs % slots;
    double cost = full * (kFixed + steps * kStep2);
    if (rem > 0) {
      const double step = rem <= slots / 2 ? kStep1 : kStep1 + (kStep2 - kStep1) * (rem - slots / 2) / (slots / 2);
      cost += kFixed + steps * step;
    }
    if (s > 1) cost += 5.0 + (s + 1) * dw_bytes / 3.0e6;   // reduction pass: launch + (s reads + 1 write) at 3 TB/s
    if (cost < best_cost) { best_cost = cost; best = s; }
  }
  { const int v = sw_int("DADET_WGRAD_SPLITS", 0); if (v > 0) best = v < max_splits ? v : max_splits; }
  const int rows = cdiv(cdiv(M, best), 32) * 32;
  p->rows_per_split = rows;
  p->splits = cdiv(M, rows);
  // partial sums rounded up to whole 128 x 128 tiles
  p->workspace_bytes = p->splits > 1 ? sizeof(float) * (size_t)p->splits * p->tiles_co * p->tiles_kc * 128 * 128 : 0;
  p->grid = tiles * p->splits;
}

// Weight gradient on 256 x 256 tiles (conv_big.hip).  The grid is small (Cout x K in tiles of 256 x 256: 4 .. 72 tiles), so
// the reduction over the M rows is cut into `splits` ranges of whole K-tiles that fill the 256 CUs once.  Returns false
// when the 128 x 128 kernel should run.
inline bool wgrad_big_plan(const dadet_conv_desc* d, int gemm_mode, int big_mode, WgradPlan* p) {
  if (!wgrad_big_enabled(gemm_mode, big_mode)) return false;
  const Gemm g = gemm_of(d);
  const int M = g.M, K = g.K;
  if (d->Cin % 4 != 0 || K % 4 != 0 || M >= (1 << 24)) return false;
  if (g.x_bytes >= 0x7FFFFF00ull || (uint64_t)M * ((d->Cout + 3) / 4 * 4) * 4 >= 0x7FFFFF00ull) return false;
  if (big_mode != 2 && (d->Cout < 256 || K < 256 || M < 2048)) return false;
  p->tiles_co = cdiv(d->Cout, 256);
  p->tiles_kc = cdiv(K, 256);
  const int tiles = p->tiles_co * p->tiles_kc;
  // Every workgroup leaves a 256 KB tile of partial sums: 64 MB per launch once the chip is full, whatever the layer.  A
  // weight of four tiles (res4's 1x1 layers: 1 MB) would be cut into 64 parts — 64 MB written and read again for 41 us of
  // GEMM, where the 128 x 128 kernel's 16 tiles need a quarter of that traffic for 47 us: below eight tiles it keeps the
  // layer (profiles/r05_step_timeline_img_only.txt: the step-end reduction passes read what these launches park)
  static const int min_tiles = sw_int("DADET_WGRAD_BIG_MIN_TILES", 8);
  if (big_mode != 2 && tiles < min_tiles) return false;
  int s = kCUs / tiles;
  const int forced = sw_int("DADET_WGRAD_BIG_SPLITS", 0);
  if (forced > 0) s = forced;
  if (s < 1) s = 1;
  // a part is ONE fp32 accumulator chain over its rows: beyond ~4096 rows the chain's own rounding shows against the
  // exact-fp32 kernel, whose plan always cuts (tests/test_ops_gpu.py::test_split_bf16_accuracy_at_production_k: the RPN
  // conv's dense gradient, 8192 rows x 144 tiles in one part, RMS 1.27e-6 against 1.01e-6) — at least ceil(M / 4096) parts
  // (the step has no such launch: its 144-tile weight is the RPN conv, whose gradient runs on the <= 256 sampled rows)
  if (!sw("DADET_WGRAD_BIG_SPLITS") && s < cdiv(M, 4096)) s = cdiv(M, 4096);
  const int max_s = cdiv(M, 128);                 // at least four K-tiles per part
  if (s > max_s) s = max_s;
  const int rows = cdiv(cdiv(M, s), 32) * 32;
  p->rows_per_split = rows;
  p->splits = cdiv(M, rows);
  // dense [splits][Cout][K] partial sums
  p->workspace_bytes = p->splits > 1 ? sizeof(float) * (size_t)p->splits * d->Cout * K : 0;
  p->grid = tiles * p->splits;
  return true;
}

// gy_ld: floats between rows of gy (Cout, or Cout rounded up to a multiple of four: the 256 x 256 kernel wants dense rows)
inline WgradPlan plan_wgrad(const dadet_conv_desc* d, int gy_ld, int gemm_mode, int big_mode) {
  WgradPlan p = {};
  const bool empty = d->N == 0;               // an empty batch launches nothing: the label alone, every number zero
  if (!empty && gy_ld == d->Cout && wgrad_big_plan(d, gemm_mode, big_mode, &p)) {
    p.family = kWgradBig;
    p.name = "conv_wgrad_big_kernel";
    return p;
  }
  if (!empty) wgrad_plan(d, &p);
  static const char* const split[3] = {"conv_wgrad_split_kernel<2>", "conv_wgrad_split_kernel<3>", "conv_wgrad_split_kernel<4>"};
  p.family = gemm_mode == 0 ? kWgradExact : (d->Wo < 32 ? kWgradSplitSmallMap : kWgradSplit);
  p.name = gemm_mode == 0 ? "conv_wgrad_kernel" : split[gemm_mode - 2];
  return p;
}

// ---- several weight gradients in one launch (conv_big.hip: conv_wgrad_big_group_kernel; conv_split.hip: its 128 x 128 form)
struct WgradGroupPlan {
  int kind;             // 256 / 128: the tile of the grouped kernel; 0: no grouped launch
  int rows;             // rows per part, the same for every problem
  int small_map;        // 128 x 128 form: the SMALL_MAP kernel (every problem's Wo < 32)
  int tiles_co[kGroupMax], tiles_kc[kGroupMax], splits[kGroupMax];
  size_t workspace_bytes[kGroupMax];
};

// can this weight gradient be a member of a grouped 256 x 256 launch (the tile kernel's own conditions; no lower bound on the tiles)
inline bool wgrad_group_member(const dadet_conv_desc* d, int gemm_mode, int big_mode) {
  if (!wgrad_big_enabled(gemm_mode, big_mode)) return false;
  const Gemm g = gemm_of(d);
  if (d->Cin % 4 != 0 || g.K % 4 != 0 || d->Cout % 4 != 0 || g.M >= (1 << 24) || g.M < 256) return false;
  if (g.x_bytes >= 0x7FFFFF00ull || (uint64_t)g.M * d->Cout * 4 >= 0x7FFFFF00ull) return false;
  return big_mode == 2 || (d->Cout >= 256 && g.K >= 256 && g.M >= 2048);
}

// which kernel serves the whole group: 256 (every problem qualifies for the 256 x 256 tile), 128 (contraction mode 4, every
// problem on the 128 x 128 kernel's ordinary path and on the same side of its small-map switch), 0 (no grouped launch).
// The descriptors are valid (the caller checked them).
inline int wgrad_group_kind(const dadet_conv_desc* descs, const int n, int gemm_mode, int big_mode) {
  if (n < 1 || n > kGroupMax || gemm_mode != 4) return 0;
  bool big = true, small = true;
  for (int i = 0; i < n; ++i) {
    const dadet_conv_desc& d = descs[i];
    if (d.N == 0) return 0;
    const Gemm g = gemm_of(&d);
    if (g.K % 4 != 0 || d.Cout % 4 != 0 || g.M < 128) return 0;
    if (g.x_bytes >= 0x7FFFFF00ull || (uint64_t)g.M * d.Cout * 4 >= 0x7FFFFF00ull) return 0;
    big = big && wgrad_group_member(&d, gemm_mode, big_mode);
    small = small && (d.Wo < 32) == (descs[0].Wo < 32);
  }
  static const bool small_on = !sw_off("DADET_WGRAD_GROUP_128");
  return big ? 256 : (small && small_on ? 128 : 0);
}

// Rows per part R (a multiple of 32, the same for every problem of the group — every workgroup then runs the same number
// of K-tiles on one tile, whatever its problem): the smallest R whose parts fit the chip's workgroup slots (256 for the
// 256 x 256 tile, 2 x 256 for the 128 x 128 kernel), at least 128 rows (four K-tiles), at most 4096 (+ an eighth where that
// saves a round of workgroups).  splits[i] = ceil(M_i / R).  DADET_WGRAD_GROUP_ROWS forces R (tests).
inline WgradGroupPlan plan_wgrad_group(const dadet_conv_desc* d, const int n, int gemm_mode, int big_mode) {
  WgradGroupPlan p = {};
  p.kind = wgrad_group_kind(d, n, gemm_mode, big_mode);
  if (!p.kind) return p;
  const int tile = p.kind;
  const int slots = tile == 256 ? kCUs : 2 * kCUs;
  int M[kGroupMax], max_m = 0;
  for (int i = 0; i < n; ++i) {
    const Gemm g = gemm_of(&d[i]);
    p.tiles_co[i] = cdiv(d[i].Cout, tile);
    p.tiles_kc[i] = cdiv(g.K, tile);
    M[i] = g.M;
    max_m = g.M > max_m ? g.M : max_m;
  }
  int R = 128;
  if (const char* e = sw("DADET_WGRAD_GROUP_ROWS")) {
    const int v = atoi(e);
    R = v >= 32 ? v / 32 * 32 : R;
  } else {
    const int top = cdiv(max_m, 32) * 32;
    for (; R < top; R += 32) {
      int wgs = 0;
      for (int i = 0; i < n; ++i) wgs += p.tiles_co[i] * p.tiles_kc[i] * cdiv(M[i], R);
      if (wgs <= slots) break;
    }
    // one part is ONE fp32 accumulator chain over its rows: never more than 4096 of them (wgrad_big_plan's bound, for the
    // same reason) — a group whose tiles alone nearly fill the slots (the res5 head on 512 ROIs: ~100 tiles x 25088 rows)
    // then takes a second / third round of workgroups, cut into equal parts rather than 4096 + a remainder
    // (an eighth of slack: the res5 head on 256 ROIs — 68 tiles, 12544 rows — fits the slots in three parts of 4192 rows;
    // cutting it into four of 3136 is 272 workgroups, a second round for 16 of them: the family went 1.8 -> 2.2 ms per step)
    const int cap = cdiv(cdiv(max_m, cdiv(max_m, 4096)), 32) * 32;
    if (R > 4096 + 512) R = cap;
  }
  p.rows = R;
  for (int i = 0; i < n; ++i) {
    p.splits[i] = cdiv(M[i], R);
    // both grouped kernels park dense [splits][Cout][K] partial sums
    p.workspace_bytes[i] = p.splits[i] > 1 ? sizeof(float) * (size_t)p.splits[i] * d[i].Cout * d[i].KH * d[i].KW * d[i].Cin : 0;
  }
  p.small_map = d[0].Wo < 32;
  return p;
}

// ---- the flat view the query entry points hand out (include/dadet.h: dadet_conv_plan_info) ---------------------------
inline void fill_info(const FwdPlan& p, dadet_conv_plan_info* o) {
  *o = dadet_conv_plan_info();
  o->family = p.family; o->variant = p.variant;
  o->tiles_m = p.tiles_m; o->tiles_n = p.tiles_n; o->ksplit = p.ksplit; o->splits = p.splits;
  o->sk_dp_tiles = p.sk.dp_tiles; o->sk_tiles = p.sk.sk_tiles; o->sk_units = p.sk.units; o->sk_iters = p.sk.iters;
  o->sk_max_parts = p.sk.max_parts;
  o->big_splits = p.big_splits; o->big_body = p.big_body;
  o->launches = p.family == kFwdWs ? p.ws_parts : (p.family == kFwdSplitK ? 2 : p.grid ? 1 : 0);
  o->grid = p.grid; o->needs_counters = p.counters ? 1 : 0;
  o->workspace_bytes = p.workspace_bytes;
  size_t i = 0;
  for (; p.name[i] && i + 1 < sizeof(o->name); ++i) o->name[i] = p.name[i];
}
inline void fill_info(const WgradPlan& p, dadet_conv_plan_info* o) {
  *o = dadet_conv_plan_info();
  o->family = p.family; o->variant = p.family == kWgradBig ? 1 : 0;
  o->tiles_m = p.tiles_co; o->tiles_n = p.tiles_kc; o->splits = p.splits; o->rows_per_split = p.rows_per_split;
  o->launches = p.grid ? 1 : 0;
  o->grid = p.grid;
  o->workspace_bytes = p.workspace_bytes;
  size_t i = 0;
  for (; p.name[i] && i + 1 < sizeof(o->name); ++i) o->name[i] = p.name[i];
}

}  // namespace plan
}  // namespace dadet
