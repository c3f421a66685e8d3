// Input pipeline on the device: Pillow-exact bilinear resize of a decoded RGB image, horizontal / vertical flip, BGR-255
// conversion and mean / std normalisation, written straight into the padded batch tensor (gfx950).
//
// What it replaces (all host-side in the reference, per image and per worker process):
//   maskrcnn_benchmark/data/transforms/transforms.py:32-62  Resize -> torchvision F.resize -> PIL Image.resize(BILINEAR)
//   transforms.py:65-74  RandomHorizontalFlip (the coin is tossed by the caller)       :77-79  ToTensor (u8 / 255)
//   transforms.py:82-97  Normalize with to_bgr255 (channel swap, * 255, - PIXEL_MEAN, / PIXEL_STD)
//   structures/image_list.py:49-91  to_image_list zero padding to SIZE_DIVISIBILITY
// Pillow's resample is integer arithmetic (8-bit pixels, 22-bit fixed-point triangle-filter coefficients, horizontal
// pass rounded to 8 bits, then vertical pass): it is reproduced bit for bit — the coefficient tables are computed
// on the host exactly as Pillow's precompute_coeffs / normalize_coeffs_8bpc do (double precision), the two passes
// below apply them.  HBM-bound byte work: lanes run along the output row, 3 channels per lane.
#include "common.h"

namespace dadet {

constexpr int kPrecisionBits = 32 - 8 - 2;

__device__ inline unsigned char clip8(int acc) {
  const int v = acc >> kPrecisionBits;
  return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// out[y][xx][c] = clip8(2^21 + sum_k in[y][xmin+k][c] * coeff[xx][k])
__global__ void resample_h_kernel(const unsigned char* __restrict__ in, int H, int W, const int* __restrict__ bounds,
                                  const int* __restrict__ coeffs, int ksize, int out_w,
                                  unsigned char* __restrict__ out) {
  const int xx = blockIdx.x * blockDim.x + threadIdx.x;
  const int y = blockIdx.y;
  if (xx >= out_w) return;
  const int xmin = bounds[2 * xx], n = bounds[2 * xx + 1];
  const int* k = coeffs + (size_t)xx * ksize;
  const unsigned char* row = in + ((size_t)y * W + xmin) * 3;
  int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
  for (int i = 0; i < n; ++i) {
    const int c = k[i];
    a0 += (int)row[3 * i] * c;
    a1 += (int)row[3 * i + 1] * c;
    a2 += (int)row[3 * i + 2] * c;
  }
  unsigned char* o = out + ((size_t)y * out_w + xx) * 3;
  o[0] = clip8(a0);
  o[1] = clip8(a1);
  o[2] = clip8(a2);
}

// vertical pass + flip + (BGR, * 255) + normalise; out is fp32 [out_h rows][row_stride pixels][3] (NHWC of a
// 3-channel image whose padded width is row_stride); bounds == nullptr: no vertical resampling
__global__ void resample_v_normalize_kernel(const unsigned char* __restrict__ in, int in_h, int w,
                                            const int* __restrict__ bounds, const int* __restrict__ coeffs,
                                            int ksize, int out_h, int flip, int to_bgr255, float m0, float m1,
                                            float m2, float s0, float s1, float s2, float* __restrict__ out,
                                            int row_stride) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  const int yy = blockIdx.y;
  if (x >= w) return;
  unsigned char r, g, b;
  if (bounds) {
    const int ymin = bounds[2 * yy], n = bounds[2 * yy + 1];
    const int* k = coeffs + (size_t)yy * ksize;
    int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
    for (int i = 0; i < n; ++i) {
      const unsigned char* p = in + ((size_t)(ymin + i) * w + x) * 3;
      const int c = k[i];
      a0 += (int)p[0] * c;
      a1 += (int)p[1] * c;
      a2 += (int)p[2] * c;
    }
    r = clip8(a0);
    g = clip8(a1);
    b = clip8(a2);
  } else {
    const unsigned char* p = in + ((size_t)yy * w + x) * 3;
    r = p[0];
    g = p[1];
    b = p[2];
  }
  // ToTensor: u8 / 255; Normalize(to_bgr255): [2,1,0] * 255, then (v - mean) / std — the reference's fp32 op order
  float c0 = (float)r / 255.f, c1 = (float)g / 255.f, c2 = (float)b / 255.f;
  if (to_bgr255) {
    const float t = c0;
    c0 = c2 * 255.f;
    c1 = c1 * 255.f;
    c2 = t * 255.f;
  }
  const int xo = (flip & DADET_FLIP_H) ? (w - 1 - x) : x;
  const int yo = (flip & DADET_FLIP_V) ? (out_h - 1 - yy) : yy;
  float* o = out + ((size_t)yo * row_stride + xo) * 3;
  o[0] = (c0 - m0) / s0;
  o[1] = (c1 - m1) / s1;
  o[2] = (c2 - m2) / s2;
}

// ---------------------------------------------------------------------------------------------- one launch per batch
// Both passes, the conversion and the zero padding of up to kPrepMaxImages images in one launch.  Grid = (tiles in x,
// tiles in y, image) over the PADDED canvas [Hp][Wp]; a workgroup owns one kPrepTileH x kPrepTileW tile of it and writes
// every pixel of that tile once: image pixels inside [out_h, out_w] (mirrored columns stay inside [0, out_w), mirrored
// rows inside [0, out_h): the workgroups then write each other's image pixels, every pixel still once), zeros beyond.  Inside the image the workgroup runs the horizontal pass for the input rows its output rows draw from into
// LDS (8-bit, rounded with clip8 like resample_h_kernel: Pillow rounds between the passes), then the vertical pass
// from LDS in registers.  The input rows are walked in chunks of kPrepChunkRows: a tile of 16 output rows draws from
// 15 * f + 2 * ceil(f) + 1 input rows at a vertical factor f = H / out_h, so one chunk holds the tile up to f = 3 (the
// DA yamls' 1024 -> 600 is 1.71: 31 rows); above that the integer accumulators carry over from chunk to chunk, which
// is exact because the sum is an integer one.  LDS: 64 rows x 64 pixels x 4 B (a pixel padded to one dword, so a wave
// reads and writes one bank row per input row without conflicts) = 16 KiB per workgroup of 256 threads — the five
// workgroups a CU holds at 89 registers take half its LDS; the kernel is bound by the unaligned byte loads of the horizontal pass.
constexpr int kPrepMaxImages = DADET_IMAGE_BATCH_MAX;
constexpr int kPrepTileH = 16, kPrepTileW = 64, kPrepChunkRows = 64, kPrepThreads = 256;
constexpr int kPrepPixelsPerThread = kPrepTileH * kPrepTileW / kPrepThreads;

struct PrepBatch {
  dadet_image_item it[kPrepMaxImages];
};

__global__ __launch_bounds__(kPrepThreads) void prepare_batch_kernel(PrepBatch batch, int to_bgr255, float m0, float m1,
                                                                     float m2, float s0, float s1, float s2,
                                                                     float* __restrict__ out, int Hp, int Wp) {
  __shared__ uchar4 rows[kPrepChunkRows][kPrepTileW];
  const dadet_image_item& d = batch.it[blockIdx.z];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * kPrepTileW, y0 = blockIdx.y * kPrepTileH;
  const int tw = min(kPrepTileW, Wp - x0), th = min(kPrepTileH, Hp - y0);        // the tile clipped to the canvas
  const int vw = max(0, min(tw, d.out_w - x0)), vh = max(0, min(th, d.out_h - y0));   // its part inside the image
  float* __restrict__ slot = out + (size_t)d.slot * Hp * Wp * 3;
  const int px = tid % kPrepTileW, py0 = tid / kPrepTileW;       // this thread's pixels: (py0 + 4 * k, px)
  constexpr int kRowStep = kPrepThreads / kPrepTileW;

  for (int k = 0; k < kPrepPixelsPerThread; ++k) {               // the padding of this tile
    const int py = py0 + kRowStep * k;
    if (py < th && px < tw && (py >= vh || px >= vw)) {
      float* o = slot + ((size_t)(y0 + py) * Wp + (x0 + px)) * 3;
      o[0] = 0.f;
      o[1] = 0.f;
      o[2] = 0.f;
    }
  }
  if (vw == 0 || vh == 0) return;                                // (uniform over the workgroup)

  const unsigned char* __restrict__ src = (const unsigned char*)d.src;
  const int* __restrict__ hb = (const int*)d.h_bounds;
  const int* __restrict__ hc = (const int*)d.h_coeffs;
  const int* __restrict__ vb = (const int*)d.v_bounds;
  const int* __restrict__ vc = (const int*)d.v_coeffs;
  // input rows [rmin, rmax) feed the output rows [y0, y0 + vh); Pillow's bounds grow with the output index
  int rmin = y0, rmax = y0 + vh;
  if (vb) {
    rmin = vb[2 * y0];
    rmax = vb[2 * (y0 + vh - 1)] + vb[2 * (y0 + vh - 1) + 1];
  }
  constexpr int kHalf = 1 << (kPrecisionBits - 1);
  int acc[kPrepPixelsPerThread][3];
  int ymin[kPrepPixelsPerThread], yn[kPrepPixelsPerThread];
  for (int k = 0; k < kPrepPixelsPerThread; ++k) {
    acc[k][0] = acc[k][1] = acc[k][2] = vb ? kHalf : 0;
    const int py = py0 + kRowStep * k;
    ymin[k] = 0;
    yn[k] = 0;
    if (py < vh && px < vw) {
      ymin[k] = vb ? vb[2 * (y0 + py)] : y0 + py;
      yn[k] = vb ? vb[2 * (y0 + py) + 1] : 1;
    }
  }
  // the horizontal taps of this thread's column (px is the same in every iteration of the loops below)
  int xmin = x0 + px, xn = 0;
  const int* hk = nullptr;
  if (px < vw && hb) {
    xmin = hb[2 * (x0 + px)];
    xn = hb[2 * (x0 + px) + 1];
    hk = hc + (size_t)(x0 + px) * d.h_ksize;
  }

  for (int c0 = rmin; c0 < rmax; c0 += kPrepChunkRows) {
    const int nr = min(kPrepChunkRows, rmax - c0);
    if (px < vw) {
      for (int r = py0; r < nr; r += kRowStep) {                 // horizontal pass: input row c0 + r, output column px
        const unsigned char* p = src + ((size_t)(c0 + r) * d.W + xmin) * 3;
        uchar4 v;
        if (hb) {
          int a0 = kHalf, a1 = kHalf, a2 = kHalf;
          for (int i = 0; i < xn; ++i) {
            const int c = hk[i];
            a0 += (int)p[3 * i] * c;
            a1 += (int)p[3 * i + 1] * c;
            a2 += (int)p[3 * i + 2] * c;
          }
          v = make_uchar4(clip8(a0), clip8(a1), clip8(a2), 0);
        } else {                                                 // out_w == W: Pillow skips the pass
          v = make_uchar4(p[0], p[1], p[2], 0);
        }
        rows[r][px] = v;
      }
    }
    __syncthreads();
    for (int k = 0; k < kPrepPixelsPerThread; ++k) {             // vertical pass: the taps that fall into this chunk
      const int lo = max(ymin[k], c0), hi = min(ymin[k] + yn[k], c0 + nr);
      for (int i = lo; i < hi; ++i) {
        const uchar4 v = rows[i - c0][px];
        const int c = vb ? vc[(size_t)(y0 + py0 + kRowStep * k) * d.v_ksize + (i - ymin[k])] : 1;
        acc[k][0] += (int)v.x * c;
        acc[k][1] += (int)v.y * c;
        acc[k][2] += (int)v.z * c;
      }
    }
    __syncthreads();                                             // the next chunk overwrites the rows
  }

  for (int k = 0; k < kPrepPixelsPerThread; ++k) {
    const int py = py0 + kRowStep * k;
    if (py >= vh || px >= vw) continue;
    unsigned char r, g, b;
    if (vb) {
      r = clip8(acc[k][0]);
      g = clip8(acc[k][1]);
      b = clip8(acc[k][2]);
    } else {                                                     // out_h == H: the pixel itself
      r = (unsigned char)acc[k][0];
      g = (unsigned char)acc[k][1];
      b = (unsigned char)acc[k][2];
    }
    // ToTensor: u8 / 255; Normalize(to_bgr255): [2,1,0] * 255, then (v - mean) / std — the reference's fp32 op order
    float c0 = (float)r / 255.f, c1 = (float)g / 255.f, c2 = (float)b / 255.f;
    if (to_bgr255) {
      const float t = c0;
      c0 = c2 * 255.f;
      c1 = c1 * 255.f;
      c2 = t * 255.f;
    }
    const int x = x0 + px;
    const int y = y0 + py;
    const int xo = (d.flip & DADET_FLIP_H) ? (d.out_w - 1 - x) : x;
    const int yo = (d.flip & DADET_FLIP_V) ? (d.out_h - 1 - y) : y;       // mirrored rows stay inside [0, out_h)
    float* o = slot + ((size_t)yo * Wp + xo) * 3;
    o[0] = (c0 - m0) / s0;
    o[1] = (c1 - m1) / s1;
    o[2] = (c2 - m2) / s2;
  }
}

}  // namespace dadet

using namespace dadet;

extern "C" int dadet_image_resample_h(const unsigned char* image_hwc, int H, int W, const int* bounds, const int* coeffs,
                                      int ksize, int out_w, unsigned char* out_hwc, void* stream) {
  DADET_REQUIRE(H > 0 && W > 0 && out_w > 0 && ksize > 0, "image_resample_h: bad dims");
  DADET_REQUIRE(image_hwc && bounds && coeffs && out_hwc, "image_resample_h: null pointer");
  hipLaunchKernelGGL(resample_h_kernel, dim3(ceil_div(out_w, 256), H), dim3(256), 0, as_stream(stream), image_hwc, H, W,
                     bounds, coeffs, ksize, out_w, out_hwc);
  return check_launch("image_resample_h");
}

extern "C" int dadet_image_resample_v_normalize(const unsigned char* image_hwc, int in_h, int w, const int* bounds,
                                                const int* coeffs, int ksize, int out_h, int flip, int to_bgr255,
                                                const float* mean3, const float* std3, float* out_hw3,
                                                int out_row_stride, void* stream) {
  DADET_REQUIRE(in_h > 0 && w > 0 && out_h > 0 && out_row_stride >= w, "image_resample_v_normalize: bad dims");
  DADET_REQUIRE(image_hwc && mean3 && std3 && out_hw3, "image_resample_v_normalize: null pointer");
  DADET_REQUIRE(bounds || out_h == in_h, "image_resample_v_normalize: no coefficient table but out_h != in_h");
  DADET_REQUIRE(!bounds || (coeffs && ksize > 0), "image_resample_v_normalize: missing coefficients");
  DADET_REQUIRE(flip >= 0 && flip <= (DADET_FLIP_H | DADET_FLIP_V), "image_resample_v_normalize: flip mask %d (0 .. 3)", flip);
  hipLaunchKernelGGL(resample_v_normalize_kernel, dim3(ceil_div(w, 256), out_h), dim3(256), 0, as_stream(stream),
                     image_hwc, in_h, w, bounds, coeffs, ksize, out_h, flip, to_bgr255 ? 1 : 0, mean3[0],
                     mean3[1], mean3[2], std3[0], std3[1], std3[2], out_hw3, out_row_stride);
  return check_launch("image_resample_v_normalize");
}

extern "C" int dadet_image_prepare_batch(const dadet_image_item* items, int n, int to_bgr255, const float* mean3,
                                         const float* std3, float* out, int n_slots, int Hp, int Wp, void* stream) {
  DADET_REQUIRE(items && mean3 && std3 && out, "image_prepare_batch: null pointer");
  DADET_REQUIRE(n > 0 && n <= kPrepMaxImages, "image_prepare_batch: %d images (1 .. %d per launch)", n, kPrepMaxImages);
  DADET_REQUIRE(n_slots > 0 && Hp > 0 && Wp > 0, "image_prepare_batch: bad batch dims");
  DADET_REQUIRE(ceil_div(Hp, kPrepTileH) <= 65535, "image_prepare_batch: canvas too tall");
  PrepBatch batch = {};
  for (int i = 0; i < n; ++i) {
    const dadet_image_item& d = items[i];
    DADET_REQUIRE(d.src && d.H > 0 && d.W > 0 && d.out_h > 0 && d.out_w > 0, "image_prepare_batch: image %d: bad dims", i);
    DADET_REQUIRE(d.out_h <= Hp && d.out_w <= Wp, "image_prepare_batch: image %d: %d x %d does not fit the %d x %d canvas",
                  i, d.out_h, d.out_w, Hp, Wp);
    DADET_REQUIRE(d.flip >= 0 && d.flip <= (DADET_FLIP_H | DADET_FLIP_V), "image_prepare_batch: image %d: flip mask %d (0 .. 3)", i,
                  d.flip);
    DADET_REQUIRE(d.slot >= 0 && d.slot < n_slots, "image_prepare_batch: image %d: slot %d of %d", i, d.slot, n_slots);
    DADET_REQUIRE(d.h_bounds ? (d.h_coeffs && d.h_ksize > 0) : d.out_w == d.W,
                  "image_prepare_batch: image %d: horizontal table missing or incomplete", i);
    DADET_REQUIRE(d.v_bounds ? (d.v_coeffs && d.v_ksize > 0) : d.out_h == d.H,
                  "image_prepare_batch: image %d: vertical table missing or incomplete", i);
    for (int j = 0; j < i; ++j)
      DADET_REQUIRE(items[j].slot != d.slot, "image_prepare_batch: images %d and %d share slot %d", j, i, d.slot);
    batch.it[i] = d;
  }
  hipLaunchKernelGGL(prepare_batch_kernel, dim3(ceil_div(Wp, kPrepTileW), ceil_div(Hp, kPrepTileH), n), dim3(kPrepThreads),
                     0, as_stream(stream), batch, to_bgr255 ? 1 : 0, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2],
                     out, Hp, Wp);
  return check_launch("image_prepare_batch");
}
