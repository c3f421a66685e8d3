// Colour jitter on the device: brightness, contrast, saturation and hue of decoded uint8 RGB images (gfx950), ahead of
// dadet_image_prepare_batch.
//
// What it replaces (host-side in the reference, per image and per worker): data/transforms/transforms.py ColorJitter ->
// torchvision.transforms.ColorJitter on a PIL image -> functional_pil adjust_brightness / adjust_contrast /
// adjust_saturation (Pillow's ImageEnhance: Image.blend of a degenerate image with the image) and adjust_hue (Pillow's
// convert("HSV"), the h plane shifted modulo 256, convert("RGB")).  The random draws stay on the host
// (da_detect_amd/data/transforms.py ColorJitter.draw); this file applies a drawn list.  Pillow's arithmetic restated
// (numpy statement: da_detect_amd/data/color_jitter.py jitter_host, which the tests hold this file to):
//   * Image.blend: t = f32(f32(d) + f32(a * f32(x - d))), truncated, saturated to 0 .. 255 (inside 0 <= a <= 1 the
//     saturation never acts, a = 0 gives d and a = 1 gives x exactly, so one formula serves Pillow's three branches);
//   * convert("L"): (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16;
//   * the contrast's grey level m = int(mean(L) + 0.5) = (2 * sum + count) / (2 * count) in integers;
//   * Convert.c rgb2hsv / hsv2rgb with their float / double placement (the file is built without fast-math and with
//     -ffp-contract=off: IEEE divisions, every product and sum rounded on its own).
// Launches: at most two for up to 8 images.  The sum pass (only the images whose list holds the contrast) applies the
// operators in front of the contrast per pixel in registers and adds up L: per thread, per wave (shuffles), per
// workgroup (LDS), then ONE 64-bit integer atomicAdd per workgroup — integer sums do not depend on the order, so the
// result is deterministic; 32 bits would overflow at 16.8 M white pixels.  The apply pass runs the whole list per pixel
// in registers and writes 8 bit.
// Work split: an image is a FLAT run of H * W pixels walked in groups of 16 pixels = 48 bytes = three aligned 16-byte
// loads and stores per thread (src and out are 16-byte aligned); the last, partial group goes byte by byte.  Grid =
// (workgroups, image), grid-strided over the groups of the image.
#include "common.h"

namespace dadet {

constexpr int kJitThreads = 256, kJitGroupPx = 16, kJitWords = kJitGroupPx * 3 / 4;
constexpr int kJitMaxImages = DADET_JITTER_BATCH_MAX, kJitMaxOps = DADET_JITTER_MAX_OPS;

struct JitterBatch {
  dadet_jitter_item it[kJitMaxImages];
  int sum_slot[kJitMaxImages];                           // the image's word of `sums`, -1: its list holds no contrast
};

__device__ inline int jit_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__device__ inline int jit_luma(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

__device__ inline int jit_blend(int d, int x, float a) {
  const float t = (float)d + a * (float)(x - d);
  return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

__device__ inline int jit_round8(float y) { return jit_clip8((int)floorf(y + 0.5f)); }

// Pillow's rgb2hsv, h += shift (mod 256), hsv2rgb
__device__ inline void jit_hue(int& r, int& g, int& b, int shift) {
  const int mx = max(r, max(g, b)), mn = min(r, min(g, b));
  int h = 0, s = 0;
  if (mx != mn) {
    const float cr = (float)(mx - mn);
    s = jit_clip8((int)((cr / (float)mx) * 255.f));
    const float rc = (float)(mx - r) / cr, gc = (float)(mx - g) / cr, bc = (float)(mx - b) / cr;
    float h0;
    if (r == mx) h0 = bc - gc;
    else if (g == mx) h0 = (float)((2.0 + (double)rc) - (double)bc);
    else h0 = (float)((4.0 + (double)gc) - (double)rc);
    double turn = (double)h0 / 6.0 + 1.0;                // in [5/6, 11/6]: fmod(turn, 1.0) is one exact subtraction
    turn = turn >= 1.0 ? turn - 1.0 : turn;
    const float h1 = (float)turn;
    h = jit_clip8((int)((double)h1 * 255.0));
  }
  h = (h + shift) & 255;
  const int v = mx;
  if (s == 0) {
    r = g = b = v;
    return;
  }
  const float hh = (float)(h * 6) / 255.f;
  const float fi = floorf(hh), fr = hh - fi, fs = (float)s / 255.f, fv = (float)v;
  const int p = jit_round8(fv * (1.f - fs));
  const int q = jit_round8(fv * (1.f - fs * fr));
  const int t = jit_round8(fv * (1.f - fs * (1.f - fr)));
  switch ((int)fi % 6) {
    case 0: r = v; g = t; b = p; break;
    case 1: r = q; g = v; b = p; break;
    case 2: r = p; g = v; b = t; break;
    case 3: r = p; g = q; b = v; break;
    case 4: r = t; g = p; b = v; break;
    default: r = v; g = p; b = q; break;
  }
}

// operators [0, count) of the list on one pixel; m: the contrast's grey level
__device__ inline void jit_pixel(const dadet_jitter_item& d, int count, int m, int& r, int& g, int& b) {
  for (int k = 0; k < count; ++k) {
    const float a = d.factor[k];
    switch (d.op[k]) {
      case DADET_JITTER_BRIGHTNESS:
        r = jit_blend(0, r, a);
        g = jit_blend(0, g, a);
        b = jit_blend(0, b, a);
        break;
      case DADET_JITTER_CONTRAST:
        r = jit_blend(m, r, a);
        g = jit_blend(m, g, a);
        b = jit_blend(m, b, a);
        break;
      case DADET_JITTER_SATURATION: {
        const int l = jit_luma(r, g, b);
        r = jit_blend(l, r, a);
        g = jit_blend(l, g, a);
        b = jit_blend(l, b, a);
        break;
      }
      default:
        jit_hue(r, g, b, d.hue_shift);
        break;
    }
  }
}

// the 48 bytes of the group that starts at pixel `first` -> w (statically indexed: the words stay in registers); bytes
// past the image read as 0
__device__ inline void jit_load(const unsigned char* __restrict__ src, int64_t first, int64_t total, unsigned int* w) {
  const unsigned char* p = src + first * 3;
  if (first + kJitGroupPx <= total) {
    const uint4* v = reinterpret_cast<const uint4*>(p);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const uint4 q = v[k];
      w[4 * k] = q.x;
      w[4 * k + 1] = q.y;
      w[4 * k + 2] = q.z;
      w[4 * k + 3] = q.w;
    }
  } else {
    const int nb = (int)(total - first) * 3;
#pragma unroll
    for (int k = 0; k < kJitWords; ++k) {
      unsigned int word = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (4 * k + j < nb) word |= (unsigned int)p[4 * k + j] << (8 * j);
      w[k] = word;
    }
  }
}

__device__ inline void jit_store(unsigned char* __restrict__ out, int64_t first, int64_t total, const unsigned int* w) {
  unsigned char* p = out + first * 3;
  if (first + kJitGroupPx <= total) {
    uint4* v = reinterpret_cast<uint4*>(p);
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
  } else {
    const int nb = (int)(total - first) * 3;
#pragma unroll
    for (int k = 0; k < kJitWords; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (4 * k + j < nb) p[4 * k + j] = (unsigned char)(w[k] >> (8 * j));
  }
}

__device__ inline int jit_byte(const unsigned int* w, int i) { return (int)((w[i >> 2] >> (8 * (i & 3))) & 255u); }

// sums[slot] += sum of L over the image after the operators in front of its contrast
__global__ __launch_bounds__(kJitThreads) void jitter_sum_kernel(JitterBatch batch, unsigned long long* __restrict__ sums) {
  __shared__ unsigned long long part[kJitThreads / 64];
  const dadet_jitter_item& d = batch.it[blockIdx.y];
  int front = 0;
  while (front < d.n_ops && d.op[front] != DADET_JITTER_CONTRAST) ++front;
  const int64_t total = (int64_t)d.H * d.W;
  const int64_t groups = ceil_div64(total, kJitGroupPx);
  const unsigned char* __restrict__ src = (const unsigned char*)d.src;
  unsigned long long acc = 0;
  for (int64_t grp = (int64_t)blockIdx.x * kJitThreads + threadIdx.x; grp < groups; grp += (int64_t)gridDim.x * kJitThreads) {
    const int64_t first = grp * kJitGroupPx;
    unsigned int w[kJitWords];
    jit_load(src, first, total, w);
    unsigned int group_sum = 0;
#pragma unroll
    for (int k = 0; k < kJitGroupPx; ++k) {
      int r = jit_byte(w, 3 * k), g = jit_byte(w, 3 * k + 1), b = jit_byte(w, 3 * k + 2);
      jit_pixel(d, front, 0, r, g, b);
      if (first + k < total) group_sum += (unsigned int)jit_luma(r, g, b);
    }
    acc += group_sum;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long block_sum = 0;
#pragma unroll
    for (int k = 0; k < kJitThreads / 64; ++k) block_sum += part[k];
    atomicAdd(&sums[batch.sum_slot[blockIdx.y]], block_sum);
  }
}

__global__ __launch_bounds__(kJitThreads) void jitter_apply_kernel(JitterBatch batch,
                                                                   const unsigned long long* __restrict__ sums) {
  const dadet_jitter_item& d = batch.it[blockIdx.y];
  const int64_t total = (int64_t)d.H * d.W;
  const int64_t groups = ceil_div64(total, kJitGroupPx);
  int m = 0;
  const int slot = batch.sum_slot[blockIdx.y];
  if (slot >= 0) m = (int)((2ull * sums[slot] + (unsigned long long)total) / (2ull * (unsigned long long)total));
  const unsigned char* __restrict__ src = (const unsigned char*)d.src;
  unsigned char* __restrict__ out = (unsigned char*)d.out;
  for (int64_t grp = (int64_t)blockIdx.x * kJitThreads + threadIdx.x; grp < groups; grp += (int64_t)gridDim.x * kJitThreads) {
    const int64_t first = grp * kJitGroupPx;
    unsigned int w[kJitWords], o[kJitWords];
    jit_load(src, first, total, w);
#pragma unroll
    for (int k = 0; k < kJitWords; ++k) o[k] = 0;
#pragma unroll
    for (int k = 0; k < kJitGroupPx; ++k) {
      int c[3] = {jit_byte(w, 3 * k), jit_byte(w, 3 * k + 1), jit_byte(w, 3 * k + 2)};
      jit_pixel(d, d.n_ops, m, c[0], c[1], c[2]);
#pragma unroll
      for (int j = 0; j < 3; ++j) o[(3 * k + j) >> 2] |= (unsigned int)c[j] << (8 * ((3 * k + j) & 3));
    }
    jit_store(out, first, total, o);
  }
}

}  // namespace dadet

using namespace dadet;

extern "C" int dadet_color_jitter_batch(const dadet_jitter_item* items, int n, unsigned long long* sums, void* stream) {
  DADET_REQUIRE(n >= 0 && n <= kJitMaxImages, "color_jitter_batch: %d images (0 .. %d per call)", n, kJitMaxImages);
  DADET_REQUIRE(n == 0 || items, "color_jitter_batch: null pointer");
  JitterBatch all = {}, with_contrast = {};
  int n_all = 0, n_contrast = 0;
  int64_t most = 0, most_contrast = 0;
  for (int i = 0; i < n; ++i) {
    const dadet_jitter_item& d = items[i];
    DADET_REQUIRE(d.n_ops >= 0 && d.n_ops <= kJitMaxOps, "color_jitter_batch: image %d: %d operators (0 .. %d)", i, d.n_ops,
                  kJitMaxOps);
    if (d.n_ops == 0) continue;
    DADET_REQUIRE(d.src && d.out && d.src != d.out, "color_jitter_batch: image %d: null pointer or out == src", i);
    DADET_REQUIRE((((uintptr_t)d.src | (uintptr_t)d.out) & 15) == 0, "color_jitter_batch: image %d: src and out must be 16-byte aligned", i);
    DADET_REQUIRE(d.H > 0 && d.W > 0 && (int64_t)d.H * d.W <= DADET_JITTER_MAX_PIXELS, "color_jitter_batch: image %d: bad dims %d x %d",
                  i, d.H, d.W);
    unsigned seen = 0;
    bool contrast = false;
    for (int k = 0; k < d.n_ops; ++k) {
      DADET_REQUIRE(d.op[k] >= DADET_JITTER_BRIGHTNESS && d.op[k] <= DADET_JITTER_HUE, "color_jitter_batch: image %d: operator code %d",
                    i, d.op[k]);
      DADET_REQUIRE(!(seen & (1u << d.op[k])), "color_jitter_batch: image %d: operator %d twice", i, d.op[k]);
      seen |= 1u << d.op[k];
      if (d.op[k] == DADET_JITTER_HUE)
        DADET_REQUIRE(d.hue_shift >= 0 && d.hue_shift <= 255, "color_jitter_batch: image %d: hue shift %d (0 .. 255)", i, d.hue_shift);
      else
        DADET_REQUIRE(d.factor[k] - d.factor[k] == 0.f, "color_jitter_batch: image %d: factor %d is not finite", i, k);
      contrast |= d.op[k] == DADET_JITTER_CONTRAST;
    }
    const int64_t groups = ceil_div64((int64_t)d.H * d.W, kJitGroupPx);
    all.it[n_all] = d;
    all.sum_slot[n_all] = -1;
    if (contrast) {
      all.sum_slot[n_all] = n_contrast;
      with_contrast.it[n_contrast] = d;
      with_contrast.sum_slot[n_contrast] = n_contrast;
      ++n_contrast;
      most_contrast = groups > most_contrast ? groups : most_contrast;
    }
    ++n_all;
    most = groups > most ? groups : most;
  }
  if (n_all == 0) return DADET_OK;
  auto blocks = [](int64_t groups) {
    const int64_t b = ceil_div64(groups, kJitThreads);
    return (unsigned)(b < kMaxStreamBlocks ? b : kMaxStreamBlocks);
  };
  if (n_contrast > 0) {
    DADET_REQUIRE(sums && ((uintptr_t)sums & 7) == 0, "color_jitter_batch: sums missing or not 8-byte aligned");
    const hipError_t e = hipMemsetAsync(sums, 0, sizeof(unsigned long long) * n_contrast, as_stream(stream));
    if (e != hipSuccess) {
      set_error("color_jitter_batch: clearing the sums: %s", hipGetErrorString(e));
      return DADET_ELAUNCH;
    }
    hipLaunchKernelGGL(jitter_sum_kernel, dim3(blocks(most_contrast), n_contrast), dim3(kJitThreads), 0, as_stream(stream),
                       with_contrast, sums);
    const int rc = check_launch("color_jitter_batch (sum)");
    if (rc != DADET_OK) return rc;
  }
  hipLaunchKernelGGL(jitter_apply_kernel, dim3(blocks(most), n_all), dim3(kJitThreads), 0, as_stream(stream), all,
                     (const unsigned long long*)sums);
  return check_launch("color_jitter_batch (apply)");
}
