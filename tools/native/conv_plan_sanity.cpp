// Stand-alone run of the convolution plan layer (da_detect_amd/csrc/conv_plan.h is pure host code) over the descriptor grid
// and the settings of tests/golden/make_conv_plans.py, for a host sanitizer:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/native/conv_plan_sanity.cpp -o /tmp/conv_plan_sanity && /tmp/conv_plan_sanity
// Prints the number of plans and a checksum of their integer fields.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include "../../da_detect_amd/csrc/conv_plan.h"

using namespace dadet;

static unsigned long long sum = 0;
static long plans = 0;
static void mix(long long v) { sum = sum * 1099511628211ull + (unsigned long long)v; }

static dadet_conv_desc desc(int N, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad, int Ho, int Wo) {
  dadet_conv_desc d = {N, H, W, Cin, Cout, kh, kw, stride, pad, Ho, Wo, Ho, Wo, 1, 0};
  return d;
}

static void one(const dadet_conv_desc& d, int mode, int big) {
  const plan::FwdPlan f = plan::plan_forward(&d, true, mode, big);
  const plan::FwdPlan l = plan::plan_forward_epi(&d, d.Cout % 4 == 0, true, mode, big);
  mix(f.family); mix(f.variant); mix(l.variant); mix(f.tiles_m); mix(f.tiles_n); mix(f.ksplit); mix(f.splits); mix(f.grid);
  mix(f.sk.dp_tiles); mix(f.sk.sk_tiles); mix(f.sk.units); mix(f.sk.iters); mix(f.sk.max_parts);
  mix(f.big_splits); mix(f.big_body); mix((long long)f.workspace_bytes); mix(f.name[0]);
  for (int i = 0; i < f.ws_parts; ++i) { mix(f.ws_panels[i]); mix(f.ws_grid[i]); }
  for (int gy_ld : {d.Cout, (d.Cout + 3) / 4 * 4}) {
    const plan::WgradPlan w = plan::plan_wgrad(&d, gy_ld, mode, big);
    mix(w.family); mix(w.tiles_co); mix(w.tiles_kc); mix(w.splits); mix(w.rows_per_split); mix(w.grid);
    mix((long long)w.workspace_bytes); mix(w.name[0]);
  }
  plans += 3;
}

static void group(const int (*g)[7], int mode, int big) {
  dadet_conv_desc d[3];
  for (int i = 0; i < 3; ++i) d[i] = desc(g[i][0], g[i][1], g[i][2], g[i][3], g[i][4], g[i][5], g[i][5], g[i][6], g[i][5] / 2, g[i][1], g[i][2]);
  const plan::WgradGroupPlan p = plan::plan_wgrad_group(d, 3, mode, big);
  mix(p.kind); mix(p.rows);
  for (int i = 0; i < 3 && p.kind; ++i) { mix(p.splits[i]); mix((long long)p.workspace_bytes[i]); }
  ++plans;
}

int main() {
  static const int maps[][3] = {{2, 256, 512}, {2, 128, 256}, {2, 64, 128}, {2, 32, 64}, {3, 64, 128}, {256, 7, 7}, {512, 7, 7},
                                {256, 14, 14}, {512, 14, 14}, {1, 8, 8}, {1, 128, 257}, {2, 200, 330}};
  static const int cins[] = {64, 128, 256, 512, 1024, 2048};
  static const int couts[] = {18, 32, 64, 128, 132, 256, 260, 512, 1024, 2048};
  static const int groups[3][3][7] = {
      {{2, 64, 128, 256, 1024, 1, 1}, {2, 64, 128, 256, 256, 3, 1}, {2, 64, 128, 1024, 256, 1, 1}},
      {{2, 128, 256, 128, 512, 1, 1}, {2, 128, 256, 128, 128, 3, 1}, {2, 128, 256, 512, 128, 1, 1}},
      {{512, 7, 7, 2048, 512, 1, 1}, {512, 7, 7, 512, 512, 3, 1}, {512, 7, 7, 512, 2048, 1, 1}}};
  struct Setting { int mode, big; const char* name; const char* value; };
  static const Setting settings[] = {
      {0, 0, 0, 0}, {0, 1, 0, 0}, {0, 2, 0, 0}, {3, 0, 0, 0}, {3, 1, 0, 0}, {3, 2, 0, 0}, {4, 0, 0, 0}, {4, 1, 0, 0}, {4, 2, 0, 0},
      {4, 1, "DADET_STREAMK", "0"}, {4, 1, "DADET_STREAMK_SMALL", "1"}, {4, 1, "DADET_WS_1X1", "0"},
      {4, 1, "DADET_WS_K256_BN", "64"}, {4, 1, "DADET_BIG_SPLITS", "3"}, {4, 1, "DADET_BIG_TAIL", "0"},
      {4, 2, "DADET_BIG_TILE_N", "128"}, {4, 1, "DADET_WGRAD_SPLITS", "5"}, {4, 1, "DADET_WGRAD_BIG_SPLITS", "4"},
      {4, 1, "DADET_WGRAD_GROUP_ROWS", "128"}, {4, 1, "DADET_WGRAD_MIN_ROWS", "64"}, {4, 1, "DADET_EPILOGUE_V4", "0"}};
  for (const Setting& s : settings) {
    if (s.name) setenv(s.name, s.value, 1);
    for (const auto& m : maps)
      for (int cin : cins)
        for (int cout : couts)
          for (int k : {1, 3})
            for (int stride : {1, 2}) {
              const int pad = k / 2;
              one(desc(m[0], m[1], m[2], cin, cout, k, k, stride, pad, (m[1] + 2 * pad - k) / stride + 1,
                       (m[2] + 2 * pad - k) / stride + 1), s.mode, s.big);
            }
    one(desc(2, 256, 512, 4, 64, 7, 8, 2, 3, 128, 256), s.mode, s.big);      // the stem
    one(desc(0, 7, 7, 512, 512, 3, 3, 1, 1, 7, 7), s.mode, s.big);           // an empty batch
    for (const auto& g : groups) group(g, s.mode, s.big);
    if (s.name) unsetenv(s.name);
  }
  printf("%ld plans, checksum %016llx\n", plans, sum);
  return 0;
}
