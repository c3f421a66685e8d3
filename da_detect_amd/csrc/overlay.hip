// Detections drawn onto decoded uint8 RGB images on the device (gfx950): box tint, outline, label plate and glyph ink.
//
// What it replaces (host-side in the reference, per image): demo/predictor.py overlay_boxes / overlay_class_names ->
// cv2.rectangle / cv2.putText.  The placement decisions (corners, colours, label text and its cell origin) stay on the host
// (da_detect_amd/engine/overlay.py, which also states the per-pixel rule in numpy: render_host, what the tests hold this file
// to); this file applies a packed draw list.  The rule, per pixel, records in list order (include/dadet.h):
//   pass A  tint (a > 0, inside the box): v = (c * a + v * (256 - a) + 128) >> 8;  outline (inside the box, closer than w to
//           one of its edges): v = c
//   pass B  after ALL of pass A, records with a label: plate v = c, glyph ink v = white / black by the colour's luma
// Work split: one workgroup of 256 threads per 16 x 64 pixel tile; a thread owns 4 neighbouring pixels of one row (12 bytes:
// three aligned word accesses when the row's byte offset allows and the four pixels lie inside the image, bytes otherwise —
// W * 3 is in general no multiple of 4, so rows start at any alignment).  The grid runs over the tiles of every image that
// has records.  A workgroup walks its image's records twice, once per pass, kOvChunk at a time: every thread tests one
// record against the tile, the survivors are compacted IN ORDER into an LDS list (one ballot per wave, prefix by popcount,
// the waves' counts through LDS — no atomics), and all threads then apply the list to their pixels in registers.  Flushing
// the list after every chunk keeps the sequential order of pass A (the tint makes it order-dependent); the second walk
// starts only after the first has ended, so pass B lies over every record's pass A however many chunks there are.  The
// pixels are loaded at the first non-empty list and stored once at the end by the threads that changed something: a tile
// nothing reaches touches no image memory.
#include "common.h"

namespace dadet {

constexpr int kOvThreads = 256, kOvTileH = 16, kOvTileW = 64, kOvPx = 4;
constexpr int kOvChunk = DADET_OVERLAY_CHUNK, kOvInts = DADET_OVERLAY_RECORD_INTS, kOvMaxImages = DADET_OVERLAY_BATCH_MAX;
constexpr int kOvCellW = 6, kOvCellH = 11, kOvGlyphs = 95, kOvEntry = 8, kOvFar = 1 << 30;
static_assert(kOvChunk == kOvThreads, "a cull round tests one record per thread");
static_assert(kOvTileH * kOvTileW == kOvThreads * kOvPx, "a thread owns kOvPx pixels of the tile");

struct OverlayBatch {
  dadet_overlay_item it[kOvMaxImages];
  int tile_end[kOvMaxImages];                            // tiles of the items up to and including this one
  int n;
};

__device__ inline int ov_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the thread's npx pixels at p -> v (statically indexed: stays in registers)
__device__ inline void ov_load(const unsigned char* __restrict__ p, int npx, int* v) {
  if (npx == kOvPx && ((uintptr_t)p & 3) == 0) {
    const unsigned int* q = reinterpret_cast<const unsigned int*>(p);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const unsigned int word = q[k];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[4 * k + j] = (int)((word >> (8 * j)) & 255u);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 3 * kOvPx; ++k) v[k] = k < 3 * npx ? (int)p[k] : 0;
  }
}

__device__ inline void ov_store(unsigned char* __restrict__ p, int npx, const int* v) {
  if (npx == kOvPx && ((uintptr_t)p & 3) == 0) {
    unsigned int* q = reinterpret_cast<unsigned int*>(p);
#pragma unroll
    for (int k = 0; k < 3; ++k)
      q[k] = (unsigned)v[4 * k] | (unsigned)v[4 * k + 1] << 8 | (unsigned)v[4 * k + 2] << 16 | (unsigned)v[4 * k + 3] << 24;
  } else {
#pragma unroll
    for (int k = 0; k < 3 * kOvPx; ++k)
      if (k < 3 * npx) p[k] = (unsigned char)v[k];
  }
}

// One walk over the image's records.  kLabels false: pass A (entries x0 y0 x1 y1 rgb w a); true: pass B (entries tx ty len
// rgb ink text_offset).  Returns through loaded / dirty what it did to the thread's pixels.
template <bool kLabels>
__device__ inline void ov_walk(const dadet_overlay_item& d, const int* __restrict__ records,
                               const unsigned char* __restrict__ text, const unsigned char* __restrict__ glyphs, int tile_x0,
                               int tile_y0, int tile_x1, int tile_y1, int xb, int y, int npx, const unsigned char* p, int* v,
                               bool& loaded, bool& dirty, int (*s_list)[kOvEntry], int* s_wave) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  for (int base = 0; base < d.count; base += kOvChunk) {
    const int idx = base + t;
    bool keep = false;
    int e[kOvEntry] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (idx < d.count) {
      const int* __restrict__ r = records + (int64_t)(d.first + idx) * kOvInts;
      const int rgb = r[4] & 0xffffff;
      if (!kLabels) {
        const int x0 = ov_clamp(r[0], -kOvFar, kOvFar), y0 = ov_clamp(r[1], -kOvFar, kOvFar);
        const int x1 = ov_clamp(r[2], -kOvFar, kOvFar), y1 = ov_clamp(r[3], -kOvFar, kOvFar);
        const int w = ov_clamp(r[5], 1, 8), a = ov_clamp(r[6], 0, 256);
        keep = x0 <= x1 && y0 <= y1 && x0 <= tile_x1 && x1 >= tile_x0 && y0 <= tile_y1 && y1 >= tile_y0;
        // an untinted box whose outline lies wholly around the tile changes nothing in it
        if (a == 0 && tile_x0 >= x0 + w && tile_x1 <= x1 - w && tile_y0 >= y0 + w && tile_y1 <= y1 - w) keep = false;
        e[0] = x0, e[1] = y0, e[2] = x1, e[3] = y1, e[4] = rgb, e[5] = w, e[6] = a;
      } else {
        const int tx = ov_clamp(r[7], -kOvFar, kOvFar), ty = ov_clamp(r[8], -kOvFar, kOvFar);
        const int len = ov_clamp(r[10], 0, DADET_OVERLAY_MAX_LABEL);
        keep = len > 0 && tx - 1 <= tile_x1 && tx + kOvCellW * len >= tile_x0 && ty - 1 <= tile_y1 && ty + kOvCellH >= tile_y0;
        const int cr = rgb & 255, cg = (rgb >> 8) & 255, cb = rgb >> 16;
        const int luma = (cr * 19595 + cg * 38470 + cb * 7471 + 0x8000) >> 16;
        e[0] = tx, e[1] = ty, e[2] = len, e[3] = rgb, e[4] = luma < 128 ? 255 : 0, e[5] = r[9];
      }
    }
    const unsigned long long kept = __ballot(keep);
    if (lane == 0) s_wave[wave] = __popcll(kept);
    __syncthreads();
    int slot = __popcll(kept & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
    for (int k = 0; k < kOvThreads / 64; ++k) {
      const int c = s_wave[k];
      slot += k < wave ? c : 0;
      total += c;
    }
    if (keep) {
#pragma unroll
      for (int k = 0; k < kOvEntry; ++k) s_list[slot][k] = e[k];
    }
    __syncthreads();
    if (total > 0) {
      if (!loaded) {
        if (npx > 0) ov_load(p, npx, v);
        loaded = true;
      }
      for (int j = 0; j < total; ++j) {
        const int* q = s_list[j];
        if (npx <= 0) continue;
        if (!kLabels) {
          const int x0 = q[0], y0 = q[1], x1 = q[2], y1 = q[3], rgb = q[4], w = q[5], a = q[6];
          if (y < y0 || y > y1 || xb + kOvPx - 1 < x0 || xb > x1) continue;
          const int c[3] = {rgb & 255, (rgb >> 8) & 255, rgb >> 16};
          const bool y_edge = y - y0 < w || y1 - y < w;
#pragma unroll
          for (int i = 0; i < kOvPx; ++i) {
            const int x = xb + i;
            if (i >= npx || x < x0 || x > x1) continue;
            const bool edge = y_edge || x - x0 < w || x1 - x < w;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
              int val = v[3 * i + ch];
              if (a > 0) val = (c[ch] * a + val * (256 - a) + 128) >> 8;
              v[3 * i + ch] = edge ? c[ch] : val;
            }
            dirty = dirty || edge || a > 0;
          }
        } else {
          const int tx = q[0], ty = q[1], len = q[2], rgb = q[3], ink = q[4], off = q[5];
          const int right = tx + kOvCellW * len, dy = y - ty;
          if (dy < -1 || dy > kOvCellH || xb + kOvPx - 1 < tx - 1 || xb > right) continue;
          const int c[3] = {rgb & 255, (rgb >> 8) & 255, rgb >> 16};
#pragma unroll
          for (int i = 0; i < kOvPx; ++i) {
            const int dx = xb + i - tx;
            if (i >= npx || dx < -1 || dx > kOvCellW * len) continue;
            bool on = false;
            if (dx >= 0 && dx < kOvCellW * len && dy >= 0 && dy < kOvCellH) {
              const int cell = dx / kOvCellW, col = dx - cell * kOvCellW;
              int g = (int)text[(int64_t)off + cell] - 0x20;
              g = (unsigned)g < (unsigned)kOvGlyphs ? g : '?' - 0x20;
              on = (glyphs[g * kOvCellH + dy] >> (kOvCellW - 1 - col)) & 1;
            }
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) v[3 * i + ch] = on ? ink : c[ch];
            dirty = true;
          }
        }
      }
    }
    __syncthreads();                                     // the list and the counts are rewritten by the next round
  }
}

__global__ __launch_bounds__(kOvThreads) void overlay_kernel(OverlayBatch batch, const int* __restrict__ records,
                                                             const unsigned char* __restrict__ text,
                                                             const unsigned char* __restrict__ glyphs) {
  __shared__ int s_list[kOvChunk][kOvEntry];
  __shared__ int s_wave[kOvThreads / 64];
  int tile = blockIdx.x, k = 0;
  while (k + 1 < batch.n && tile >= batch.tile_end[k]) ++k;
  if (k > 0) tile -= batch.tile_end[k - 1];
  const dadet_overlay_item& d = batch.it[k];
  const int tiles_x = ceil_div(d.W, kOvTileW);
  const int tile_x0 = (tile % tiles_x) * kOvTileW, tile_y0 = (tile / tiles_x) * kOvTileH;
  const int tile_x1 = min(tile_x0 + kOvTileW, d.W) - 1, tile_y1 = min(tile_y0 + kOvTileH, d.H) - 1;
  const int t = threadIdx.x;
  const int y = tile_y0 + t / (kOvTileW / kOvPx), xb = tile_x0 + (t % (kOvTileW / kOvPx)) * kOvPx;
  const int npx = y < d.H ? ov_clamp(d.W - xb, 0, kOvPx) : 0;   // the thread's pixels inside the image
  unsigned char* p = (unsigned char*)d.image + ((int64_t)y * d.W + xb) * 3;   // dereferenced only where npx > 0
  int v[3 * kOvPx];
#pragma unroll
  for (int i = 0; i < 3 * kOvPx; ++i) v[i] = 0;
  bool loaded = false, dirty = false;
  ov_walk<false>(d, records, text, glyphs, tile_x0, tile_y0, tile_x1, tile_y1, xb, y, npx, p, v, loaded, dirty, s_list, s_wave);
  ov_walk<true>(d, records, text, glyphs, tile_x0, tile_y0, tile_x1, tile_y1, xb, y, npx, p, v, loaded, dirty, s_list, s_wave);
  if (dirty) ov_store(p, npx, v);
}

}  // namespace dadet

using namespace dadet;

extern "C" int dadet_overlay_batch(const dadet_overlay_item* items, int n, const int* records, const unsigned char* text,
                                   const unsigned char* glyphs, void* stream) {
  DADET_REQUIRE(n >= 0 && n <= kOvMaxImages, "overlay_batch: %d images (0 .. %d per call)", n, kOvMaxImages);
  DADET_REQUIRE(n == 0 || items, "overlay_batch: null pointer");
  OverlayBatch batch = {};
  int64_t tiles = 0;
  for (int i = 0; i < n; ++i) {
    const dadet_overlay_item& d = items[i];
    DADET_REQUIRE(d.image, "overlay_batch: image %d: null pointer", i);
    DADET_REQUIRE(d.H > 0 && d.W > 0 && (int64_t)d.H * d.W <= DADET_OVERLAY_MAX_PIXELS, "overlay_batch: image %d: bad dims %d x %d", i,
                  d.H, d.W);
    DADET_REQUIRE(d.count >= 0 && d.count <= DADET_OVERLAY_MAX_RECORDS, "overlay_batch: image %d: %d records (0 .. %d)", i, d.count,
                  DADET_OVERLAY_MAX_RECORDS);
    DADET_REQUIRE(d.first >= 0 && d.first <= INT32_MAX - d.count, "overlay_batch: image %d: first record %d", i, d.first);
    if (d.count == 0) continue;
    tiles += (int64_t)ceil_div(d.W, kOvTileW) * ceil_div(d.H, kOvTileH);
    batch.it[batch.n] = d;
    batch.tile_end[batch.n] = (int)tiles;
    ++batch.n;
  }
  if (batch.n == 0) return DADET_OK;
  DADET_REQUIRE(records && text && glyphs, "overlay_batch: null pointer");
  DADET_REQUIRE(((uintptr_t)records & 3) == 0, "overlay_batch: records must be 4-byte aligned");
  hipLaunchKernelGGL(overlay_kernel, dim3((unsigned)tiles), dim3(kOvThreads), 0, as_stream(stream), batch, records, text, glyphs);
  return check_launch("overlay_batch");
}
