// Instance boxes from Cityscapes instance-id maps on the device (gfx950).
//
// What it replaces (host-side, offline, through OpenCV and cityscapesscripts in the reference): the per-instance loop of
// tools/cityscapes/convert_cityscapes_to_coco.py / instances2dict_with_polygons.py — one full-image mask pass and a
// contour trace per instance.  Here every map of a batch is read ONCE and every instance id 24000 .. 33999 gets
//   {xmin, ymin, xmax, ymax, pixelCount, fragmented}
// where `fragmented` says that one of the id's 8-connected components has at most 2 pixels (the reference drops such an
// instance whole: a contour of <= 2 points).  That is a 5 x 5 stencil, not a labelling pass: with n(p) the number of
// same-id 8-neighbours of p, p lies in such a component iff n(p) == 0, or n(p) == 1 and its one neighbour q has n(q) == 1.
//
// Launches (one memset, two kernels, all on the caller's stream):
//   * clear of the table  int32 [n][6 fields][10000 slots]  (slot = id - 24000);
//   * instance_accumulate_kernel, one workgroup of 256 threads per 16 x 256 tile of one map.  The tile and its 2-pixel
//     halo go to LDS (0 = "no pixel" beyond the image; 0 is no instance id).  Rows are fetched as 16-byte vectors wherever
//     a vector lies inside its image row — the vectors are aligned in the PACKED buffer, so a map of odd width, whose rows
//     start at odd 2-byte offsets, takes the same path — and element by element at the row ends.  A wave then walks
//     64-pixel row segments with consecutive lanes on consecutive pixels: a ballot of "differs from the left
//     neighbour" splits the segment into runs, the first lane of a run of an instance id owns it and merges
//     (x, x + len - 1, y, len, any fragment pixel in the run) into a 128-entry LDS hash of the workgroup; at the end each
//     occupied entry issues its six global integer atomics.  A hash that fills up sends the run straight to the table.
//   * instance_compact_kernel, one workgroup of 1024 threads per map: ordered stream compaction of the non-empty slots
//     into rows [id, x0, y0, x1, y1, pixelCount, fragmented] and the per-map count.
// Only integer max / add / or take part, so the result does not depend on the order of arrival.  Minima are kept as
// maxima of (kInv - v), so that the one clear to zero is the neutral element of every field.
#include "common.h"

namespace dadet {

constexpr int kIbTileW = DADET_INSTANCE_BOXES_TILE_W, kIbTileH = DADET_INSTANCE_BOXES_TILE_H;
constexpr int kIbSeg = DADET_INSTANCE_BOXES_SEGMENT;         // one wave, one pixel per lane
constexpr int kIbThreads = 256, kIbWaves = kIbThreads / 64;
constexpr int kIbHalo = 2, kIbLdsW = kIbTileW + 2 * kIbHalo, kIbLdsH = kIbTileH + 2 * kIbHalo;
constexpr int kIbVec = 8;                                    // uint16 per 16-byte load
constexpr int kIbUnits = (kIbLdsW + kIbVec - 1 + kIbVec - 1) / kIbVec;   // vectors that cover any 260 elements: 34
constexpr int kIbSlots = DADET_INSTANCE_BOXES_SLOTS, kIbFirstId = DADET_INSTANCE_BOXES_FIRST_ID;
constexpr int kIbFields = 6, kIbCols = DADET_INSTANCE_BOXES_COLUMNS;
constexpr int kIbHash = 128;
constexpr int kIbInv = 0x7fff;                               // minima as maxima of kIbInv - v; H, W <= 32767
constexpr int kIbCompactThreads = 1024;
enum { kIbNX = 0, kIbNY, kIbX1, kIbY1, kIbCount, kIbFrag };
static_assert(kIbSeg == 64 && kIbTileW % kIbSeg == 0 && kIbTileH % kIbWaves == 0, "tile walk");
static_assert(kIbUnits * kIbVec >= kIbLdsW + kIbVec - 1, "vector cover of a halo row");

struct IbBatch {                                             // by value: no upload, no host wait
  int n;
  int H[DADET_INSTANCE_BOXES_MAX_BATCH], W[DADET_INSTANCE_BOXES_MAX_BATCH];
  int tile0[DADET_INSTANCE_BOXES_MAX_BATCH + 1];             // first workgroup of every map
  long long off[DADET_INSTANCE_BOXES_MAX_BATCH];             // first element of every map
};

struct IbHashLds {
  int key[kIbHash];                                          // slot + 1, 0 = free
  int val[kIbFields][kIbHash];
};

__device__ inline void ib_table_merge(int* __restrict__ table, int slot, int nx, int ny, int x1, int y1, int count, int frag) {
  atomicMax(table + kIbNX * kIbSlots + slot, nx);
  atomicMax(table + kIbNY * kIbSlots + slot, ny);
  atomicMax(table + kIbX1 * kIbSlots + slot, x1);
  atomicMax(table + kIbY1 * kIbSlots + slot, y1);
  atomicAdd(table + kIbCount * kIbSlots + slot, count);
  if (frag) atomicOr(table + kIbFrag * kIbSlots + slot, 1);
}

// same-id 8-neighbours of the tile cell at `at` (LDS index; the halo makes every neighbour addressable)
__device__ inline int ib_neighbours(const unsigned short* t, int at, unsigned short id) {
  int n = 0;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx)
      if (dy != 0 || dx != 0) n += t[at + dy * kIbLdsW + dx] == id;
  return n;
}

__global__ __launch_bounds__(kIbThreads) void instance_accumulate_kernel(const unsigned short* __restrict__ ids, IbBatch b,
                                                                         int* __restrict__ tables) {
  __shared__ __attribute__((aligned(16))) unsigned short tile[kIbLdsH * kIbLdsW];
  __shared__ IbHashLds hash;
  const int tid = threadIdx.x;
  int img = 0;
  while (img + 1 < b.n && (int)blockIdx.x >= b.tile0[img + 1]) ++img;
  const int H = b.H[img], W = b.W[img];
  const long long off = b.off[img];
  const int tiles_x = (W + kIbTileW - 1) / kIbTileW;
  const int t = blockIdx.x - b.tile0[img];
  const int x0 = (t % tiles_x) * kIbTileW, y0 = (t / tiles_x) * kIbTileH;
  int* __restrict__ table = tables + (size_t)img * kIbFields * kIbSlots;

  if (tid < kIbHash) {
    hash.key[tid] = 0;
#pragma unroll
    for (int f = 0; f < kIbFields; ++f) hash.val[f][tid] = 0;
  }
  // tile + halo -> LDS
  for (int u = tid; u < kIbLdsH * kIbUnits; u += kIbThreads) {
    const int lr = u / kIbUnits, k = u - lr * kIbUnits;
    const int y = y0 - kIbHalo + lr;
    const long long a = off + (long long)y * W + (x0 - kIbHalo);        // element of LDS column 0 (may lie before the row)
    const bool row_ok = y >= 0 && y < H;
    const long long row_lo = row_ok ? off + (long long)y * W : a, row_hi = row_ok ? row_lo + W : a;
    const long long e0 = (a & ~(long long)(kIbVec - 1)) + (long long)k * kIbVec;   // 16-byte aligned in the packed buffer
    unsigned short v[kIbVec];
    if (e0 >= row_lo && e0 + kIbVec <= row_hi) {
      const uint4 q = *reinterpret_cast<const uint4*>(ids + e0);
      const unsigned int w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int j = 0; j < kIbVec; ++j) v[j] = (unsigned short)(w[j >> 1] >> ((j & 1) * 16));
    } else {
#pragma unroll
      for (int j = 0; j < kIbVec; ++j) {
        const long long e = e0 + j;
        v[j] = (e >= row_lo && e < row_hi) ? ids[e] : (unsigned short)0;
      }
    }
    const int col0 = (int)(e0 - a);                                     // -7 .. 264
#pragma unroll
    for (int j = 0; j < kIbVec; ++j) {
      const int col = col0 + j;
      if (col >= 0 && col < kIbLdsW) tile[lr * kIbLdsW + col] = v[j];
    }
  }
  __syncthreads();

  const int wave = tid >> 6, lane = tid & 63;
  constexpr int kSegsPerRow = kIbTileW / kIbSeg, kRowsPerWave = kIbTileH / kIbWaves;
  for (int it = 0; it < kRowsPerWave * kSegsPerRow; ++it) {
    const int r = wave * kRowsPerWave + it / kSegsPerRow, c = (it % kSegsPerRow) * kIbSeg + lane;
    const int at = (r + kIbHalo) * kIbLdsW + c + kIbHalo;
    const unsigned short id = tile[at];
    const bool inst = (unsigned)((int)id - kIbFirstId) < (unsigned)kIbSlots;   // a cell beyond the image holds 0
    if (__ballot(inst) == 0ull) continue;                               // wave-uniform
    const bool edge = lane == 0 || tile[at - 1] != id;                  // a run starts here
    bool small = false;                                                 // p lies in a component of <= 2 pixels
    if (inst) {
      const int n = ib_neighbours(tile, at, id);
      if (n == 0) {
        small = true;
      } else if (n == 1) {
        int q = at;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
          for (int dx = -1; dx <= 1; ++dx)
            if ((dy != 0 || dx != 0) && tile[at + dy * kIbLdsW + dx] == id) q = at + dy * kIbLdsW + dx;
        small = ib_neighbours(tile, q, id) == 1;
      }
    }
    const unsigned long long edges = __ballot(edge), smalls = __ballot(small);
    if (inst && edge) {
      const unsigned long long above = lane == 63 ? 0ull : edges >> (lane + 1);
      const int len = above ? __builtin_ctzll(above) + 1 : 64 - lane;
      const unsigned long long run = (len == 64 ? ~0ull : ((1ull << len) - 1ull)) << lane;
      const int frag = (smalls & run) != 0ull;
      const int slot = (int)id - kIbFirstId, x = x0 + c, y = y0 + r;
      const int nx = kIbInv - x, ny = kIbInv - y, x1 = x + len - 1;
      unsigned int h = ((unsigned int)slot * 2654435761u) >> 25;        // 7 bits
      int tries = 0;
      for (; tries < kIbHash; ++tries, h = (h + 1) & (kIbHash - 1)) {
        const int old = atomicCAS(&hash.key[h], 0, slot + 1);
        if (old == 0 || old == slot + 1) break;
      }
      if (tries < kIbHash) {
        atomicMax(&hash.val[kIbNX][h], nx);
        atomicMax(&hash.val[kIbNY][h], ny);
        atomicMax(&hash.val[kIbX1][h], x1);
        atomicMax(&hash.val[kIbY1][h], y);
        atomicAdd(&hash.val[kIbCount][h], len);
        if (frag) atomicOr(&hash.val[kIbFrag][h], 1);
      } else {
        ib_table_merge(table, slot, nx, ny, x1, y, len, frag);
      }
    }
  }
  __syncthreads();
  if (tid < kIbHash && hash.key[tid] != 0)
    ib_table_merge(table, hash.key[tid] - 1, hash.val[kIbNX][tid], hash.val[kIbNY][tid], hash.val[kIbX1][tid],
                   hash.val[kIbY1][tid], hash.val[kIbCount][tid], hash.val[kIbFrag][tid]);
}

// ordered compaction of one map's slots; grid = maps
__global__ __launch_bounds__(kIbCompactThreads) void instance_compact_kernel(const int* __restrict__ tables,
                                                                             int* __restrict__ rows, int* __restrict__ counts) {
  __shared__ int wave_total[kIbCompactThreads / 64];
  const int img = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int* __restrict__ table = tables + (size_t)img * kIbFields * kIbSlots;
  int* __restrict__ out = rows + (size_t)img * kIbSlots * kIbCols;
  int running = 0;
  for (int base = 0; base < kIbSlots; base += kIbCompactThreads) {
    const int slot = base + tid;
    const int count = slot < kIbSlots ? table[kIbCount * kIbSlots + slot] : 0;
    const unsigned long long have = __ballot(count > 0);
    if (lane == 0) wave_total[wave] = __popcll(have);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kIbCompactThreads / 64; ++w) {
      const int v = wave_total[w];
      before += w < wave ? v : 0;
      total += v;
    }
    if (count > 0) {
      int* row = out + (size_t)(running + before + __popcll(have & ((1ull << lane) - 1ull))) * kIbCols;
      row[0] = kIbFirstId + slot;
      row[1] = kIbInv - table[kIbNX * kIbSlots + slot];
      row[2] = kIbInv - table[kIbNY * kIbSlots + slot];
      row[3] = table[kIbX1 * kIbSlots + slot];
      row[4] = table[kIbY1 * kIbSlots + slot];
      row[5] = count;
      row[6] = table[kIbFrag * kIbSlots + slot];
    }
    running += total;
    __syncthreads();
  }
  if (tid == 0) counts[img] = running;
}

}  // namespace dadet

using namespace dadet;

extern "C" int dadet_instance_boxes_workspace_bytes(int n, size_t* bytes_out) {
  DADET_REQUIRE(bytes_out, "instance_boxes_workspace_bytes: null pointer");
  DADET_REQUIRE(n >= 1 && n <= DADET_INSTANCE_BOXES_MAX_BATCH, "instance_boxes_workspace_bytes: %d maps (1 .. %d)", n,
                DADET_INSTANCE_BOXES_MAX_BATCH);
  *bytes_out = (size_t)n * kIbFields * kIbSlots * sizeof(int);
  return DADET_OK;
}

extern "C" int dadet_instance_boxes(const unsigned short* ids, long long total_elements, const int* hw_host,
                                    const long long* offsets_host, int n, int* rows_out, int* counts_out, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  DADET_REQUIRE(ids && hw_host && offsets_host && rows_out && counts_out && workspace, "instance_boxes: null pointer");
  size_t need = 0;
  const int rc = dadet_instance_boxes_workspace_bytes(n, &need);
  if (rc != DADET_OK) return rc;
  DADET_REQUIRE(workspace_bytes >= need, "instance_boxes: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  DADET_REQUIRE(((uintptr_t)ids & 15) == 0 && (((uintptr_t)workspace | (uintptr_t)rows_out | (uintptr_t)counts_out) & 3) == 0,
                "instance_boxes: ids must be 16-byte aligned, workspace, rows and counts 4-byte aligned");
  IbBatch b;
  b.n = n;
  long long tiles = 0;
  for (int i = 0; i < n; ++i) {
    const int H = hw_host[2 * i], W = hw_host[2 * i + 1];
    DADET_REQUIRE(H >= 1 && W >= 1 && H <= DADET_INSTANCE_BOXES_MAX_SIDE && W <= DADET_INSTANCE_BOXES_MAX_SIDE,
                  "instance_boxes: map %d is %d x %d (sides 1 .. %d)", i, H, W, DADET_INSTANCE_BOXES_MAX_SIDE);
    DADET_REQUIRE(offsets_host[i] >= 0 && offsets_host[i] + (long long)H * W <= total_elements,
                  "instance_boxes: map %d (offset %lld, %d x %d) leaves the buffer of %lld elements", i, offsets_host[i], H, W,
                  total_elements);
    b.H[i] = H;
    b.W[i] = W;
    b.off[i] = offsets_host[i];
    b.tile0[i] = (int)tiles;
    tiles += (long long)ceil_div(W, kIbTileW) * ceil_div(H, kIbTileH);
    DADET_REQUIRE(tiles <= 0x7fffffffLL, "instance_boxes: too many tiles in one batch");
  }
  for (int i = n; i <= DADET_INSTANCE_BOXES_MAX_BATCH; ++i) b.tile0[i] = (int)tiles;
  for (int i = n; i < DADET_INSTANCE_BOXES_MAX_BATCH; ++i) b.H[i] = b.W[i] = 0, b.off[i] = 0;
  hipError_t e = hipMemsetAsync(workspace, 0, need, as_stream(stream));
  if (e != hipSuccess) {
    set_error("instance_boxes: clearing the table: %s", hipGetErrorString(e));
    return DADET_ELAUNCH;
  }
  hipLaunchKernelGGL(instance_accumulate_kernel, dim3((unsigned)tiles), dim3(kIbThreads), 0, as_stream(stream), ids, b,
                     (int*)workspace);
  const int rca = check_launch("instance_boxes (accumulate)");
  if (rca != DADET_OK) return rca;
  hipLaunchKernelGGL(instance_compact_kernel, dim3(n), dim3(kIbCompactThreads), 0, as_stream(stream), (const int*)workspace,
                     rows_out, counts_out);
  return check_launch("instance_boxes (compact)");
}
