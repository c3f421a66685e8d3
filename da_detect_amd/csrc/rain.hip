// Rain synthesis on the device: the auxiliary (rainy) rendering of a source image from a rain-mask image (gfx950).
//
// What it replaces (host-side, offline and through OpenCV in the reference): efficientderain-master/
// generate_rainy_cityscape.py rain_aug -> augment_and_mix.augment_and_mix(layer, severity=3, width=3, depth=-1) ->
// augmentations.py (rotate / shear / translate / zoom through Pillow's Image.transform(AFFINE, BILINEAR)), then the
// screen blend img + R - img * R written as an 8-bit image.  The random draws stay on the host
// (da_detect_amd/data/rain.py draw_rain_plan); this file applies a drawn plan:
//   * three chains of `depth` affine warps of the 8-bit mask, each warp Pillow's Geometry.c bilinear affine in float64
//     (affine_transform + bilinear_filter32RGB: pixel centres at +0.5, 0 outside the image, clamped neighbours,
//     truncation to 8 bits) — the library is built with -ffp-contract=off, so every product and sum rounds on its own;
//   * the mix  mix = f32(f64(mix) + f64(ws_i) * (u_i / 255.))  chain after chain,  R = f32(c0 * L) + f32(c1 * mix);
//   * the composite  t = ((img + R) - img * R) * 255  in fp32, rounded half to even and saturated to 0 .. 255.
// k / 255 in float64 and in fp32 comes from two 256-entry tables folded by the HOST compiler (IEEE division), so no
// device division takes part.
// Launches: one warp launch per operator position except the last (the three chains in grid.y, 8 bit -> 8 bit,
// ping-ponging between the two halves of the scratch buffer), then one launch that evaluates the last warp of the three
// chains per pixel, mixes, composites and writes 8 bit: depth 3 is three launches, no float image ever reaches HBM.
// Work split: the image is walked as a FLAT run of H * W pixels; a thread owns kRainPx = 4 consecutive pixels (12
// bytes = three aligned dword stores), a wave 256 consecutive pixels, a workgroup kRainTile = 1024.  For the
// identity-like operators (translate, zoom, small shears) a wave therefore reads and writes contiguous row segments.
#include "common.h"

namespace dadet {

constexpr int kRainThreads = 256, kRainPx = 4, kRainTile = kRainThreads * kRainPx;
constexpr int kRainChains = DADET_RAIN_CHAINS;

struct RainDivD { double v[256]; };
struct RainDivF { float v[256]; };
constexpr RainDivD rain_div_d() {
  RainDivD t{};
  for (int k = 0; k < 256; ++k) t.v[k] = (double)k / 255.0;
  return t;
}
constexpr RainDivF rain_div_f() {
  RainDivF t{};
  for (int k = 0; k < 256; ++k) t.v[k] = (float)k / 255.0f;
  return t;
}
__device__ const RainDivD kRainDivD = rain_div_d();      // numpy's  uint8 / 255.  (float64)
__device__ const RainDivF kRainDivF = rain_div_f();      // numpy's  float32(uint8) / 255.0  (fp32)

struct RainAffine {
  double a[kRainChains][6];                              // Pillow's AFFINE data, per chain
};
struct RainSources {
  const unsigned char* p[kRainChains];
};

// Pillow's bilinear affine for output pixel (x, y) of a W x H 3-channel image -> out[3]
__device__ inline void rain_warp_pixel(const unsigned char* __restrict__ src, int W, int H, const double* a, int x, int y,
                                       unsigned char* out) {
  const double xc = (double)x + 0.5, yc = (double)y + 0.5;
  double xin = (a[0] * xc + a[1] * yc) + a[2];
  double yin = (a[3] * xc + a[4] * yc) + a[5];
  if (!(xin >= 0.0 && xin < (double)W && yin >= 0.0 && yin < (double)H)) {
    out[0] = out[1] = out[2] = 0;
    return;
  }
  xin -= 0.5;
  yin -= 0.5;
  const int xf = xin >= 0.0 ? (int)xin : (int)floor(xin);
  const int yf = yin >= 0.0 ? (int)yin : (int)floor(yin);
  const double dx = xin - (double)xf, dy = yin - (double)yf;
  const int x0 = min(max(xf, 0), W - 1) * 3, x1 = min(max(xf + 1, 0), W - 1) * 3;
  const unsigned char* r0 = src + (size_t)min(max(yf, 0), H - 1) * W * 3;
  const bool below = yf + 1 >= 0 && yf + 1 < H;
  const unsigned char* r1 = src + (size_t)(below ? yf + 1 : 0) * W * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int p0 = r0[x0 + c], p1 = r0[x1 + c];
    const double v1 = (double)p0 + (double)(p1 - p0) * dx;
    double v2 = v1;
    if (below) {
      const int q0 = r1[x0 + c], q1 = r1[x1 + c];
      v2 = (double)q0 + (double)(q1 - q0) * dx;
    }
    const double v = v1 + (v2 - v1) * dy;
    out[c] = (unsigned char)(int)v;
  }
}

// 12 bytes of kRainPx pixels starting at flat pixel `first` -> out; whole groups as three dword stores (the base is
// 4-byte aligned and 12 * group is a multiple of 4), the last, partial group byte by byte
__device__ inline void rain_store(unsigned char* __restrict__ out, int first, int total, const unsigned char* px) {
  if (first + kRainPx <= total) {
    unsigned int* o = reinterpret_cast<unsigned int*>(out + (size_t)first * 3);
#pragma unroll
    for (int k = 0; k < 3; ++k)
      o[k] = (unsigned int)px[4 * k] | ((unsigned int)px[4 * k + 1] << 8) | ((unsigned int)px[4 * k + 2] << 16) |
             ((unsigned int)px[4 * k + 3] << 24);
  } else {
    for (int k = 0; k < (total - first) * 3; ++k) out[(size_t)first * 3 + k] = px[k];
  }
}

// one operator position of the three chains: dst[chain] = warp(src[chain]); grid = (tiles, chains)
__global__ __launch_bounds__(kRainThreads) void rain_warp_kernel(RainSources src, RainAffine coeffs, int H, int W,
                                                                 unsigned char* __restrict__ dst, size_t plane) {
  const int chain = blockIdx.y;
  const int total = H * W;
  const int first = (blockIdx.x * kRainThreads + threadIdx.x) * kRainPx;
  if (first >= total) return;
  const unsigned char* __restrict__ s = src.p[chain];
  unsigned char px[kRainPx * 3];
  int y = first / W, x = first - y * W;
#pragma unroll
  for (int k = 0; k < kRainPx; ++k) {
    if (first + k < total) rain_warp_pixel(s, W, H, coeffs.a[chain], x, y, px + 3 * k);
    if (++x == W) {
      x = 0;
      ++y;
    }
  }
  rain_store(dst + plane * chain, first, total, px);
}

// the last operator of every chain, the mix, the composite
__global__ __launch_bounds__(kRainThreads) void rain_final_kernel(RainSources src, RainAffine coeffs, int H, int W,
                                                                  const unsigned char* __restrict__ image,
                                                                  const unsigned char* __restrict__ mask, float ws0,
                                                                  float ws1, float ws2, float c0, float c1,
                                                                  unsigned char* __restrict__ out) {
  __shared__ double div_d[256];
  __shared__ float div_f[256];
  div_d[threadIdx.x] = kRainDivD.v[threadIdx.x];
  div_f[threadIdx.x] = kRainDivF.v[threadIdx.x];
  __syncthreads();
  const int total = H * W;
  const int first = (blockIdx.x * kRainThreads + threadIdx.x) * kRainPx;
  if (first >= total) return;
  const float ws[kRainChains] = {ws0, ws1, ws2};
  unsigned char px[kRainPx * 3];
  int y = first / W, x = first - y * W;
#pragma unroll
  for (int k = 0; k < kRainPx; ++k) {
    if (first + k < total) {
      float mix[3] = {0.f, 0.f, 0.f};
#pragma unroll
      for (int chain = 0; chain < kRainChains; ++chain) {
        unsigned char u[3];
        rain_warp_pixel(src.p[chain], W, H, coeffs.a[chain], x, y, u);
#pragma unroll
        for (int c = 0; c < 3; ++c) mix[c] = (float)((double)mix[c] + (double)ws[chain] * div_d[u[c]]);
      }
      const size_t at = (size_t)(first + k) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float layer = div_f[mask[at + c]];
        const float r = c0 * layer + c1 * mix[c];            // (no contraction: two rounded products, one sum)
        const float img = div_f[image[at + c]];
        float t = ((img + r) - img * r) * 255.f;
        t = rintf(t);                                        // half to even, then saturate
        t = t < 0.f ? 0.f : (t > 255.f ? 255.f : t);
        px[3 * k + c] = (unsigned char)(int)t;
      }
    }
    if (++x == W) {
      x = 0;
      ++y;
    }
  }
  rain_store(out, first, total, px);
}

inline size_t rain_plane_bytes(int H, int W) { return ((size_t)H * W * 3 + 255) / 256 * 256; }

}  // namespace dadet

using namespace dadet;

extern "C" int dadet_rain_scratch_bytes(int H, int W, int depth, size_t* bytes) {
  DADET_REQUIRE(bytes, "rain_scratch_bytes: null pointer");
  DADET_REQUIRE(H > 0 && W > 0 && (int64_t)H * W <= DADET_RAIN_MAX_PIXELS, "rain_scratch_bytes: bad dims %d x %d", H, W);
  DADET_REQUIRE(depth >= 1 && depth <= DADET_RAIN_MAX_DEPTH, "rain_scratch_bytes: depth %d (1 .. %d)", depth,
                DADET_RAIN_MAX_DEPTH);
  // depth 1: no intermediate; depth 2: one set of three planes; deeper: two sets taking turns
  *bytes = (size_t)(depth == 1 ? 0 : (depth == 2 ? 1 : 2)) * kRainChains * rain_plane_bytes(H, W);
  return DADET_OK;
}

extern "C" int dadet_rain_synthesize(const unsigned char* image_hwc, const unsigned char* mask_hwc, int H, int W, int depth,
                                     const double* coeffs, const float* ws3, float c0, float c1, unsigned char* out_hwc,
                                     void* scratch, size_t scratch_bytes, void* stream) {
  DADET_REQUIRE(image_hwc && mask_hwc && coeffs && ws3 && out_hwc, "rain_synthesize: null pointer");
  size_t need = 0;
  const int rc = dadet_rain_scratch_bytes(H, W, depth, &need);
  if (rc != DADET_OK) return rc;
  DADET_REQUIRE(need == 0 || (scratch && scratch_bytes >= need), "rain_synthesize: scratch of %zu bytes, %zu needed",
                scratch_bytes, need);
  DADET_REQUIRE(((uintptr_t)out_hwc & 3) == 0 && ((uintptr_t)scratch & 3) == 0,
                "rain_synthesize: out and scratch must be 4-byte aligned");
  for (int i = 0; i < kRainChains * depth * 6; ++i)
    DADET_REQUIRE(coeffs[i] == coeffs[i] && coeffs[i] - coeffs[i] == 0.0, "rain_synthesize: coefficient %d is not finite", i);
  const size_t plane = rain_plane_bytes(H, W);
  const int tiles = (int)ceil_div64((int64_t)H * W, kRainTile);
  unsigned char* sets[2] = {(unsigned char*)scratch, (unsigned char*)scratch + kRainChains * plane};
  RainSources src;
  for (int c = 0; c < kRainChains; ++c) src.p[c] = mask_hwc;
  for (int pos = 0; pos < depth; ++pos) {
    RainAffine a;
    for (int c = 0; c < kRainChains; ++c)
      for (int k = 0; k < 6; ++k) a.a[c][k] = coeffs[((size_t)c * depth + pos) * 6 + k];
    if (pos == depth - 1) {
      hipLaunchKernelGGL(rain_final_kernel, dim3(tiles), dim3(kRainThreads), 0, as_stream(stream), src, a, H, W, image_hwc,
                         mask_hwc, ws3[0], ws3[1], ws3[2], c0, c1, out_hwc);
      return check_launch("rain_synthesize (final)");
    }
    unsigned char* dst = sets[pos & 1];
    hipLaunchKernelGGL(rain_warp_kernel, dim3(tiles, kRainChains), dim3(kRainThreads), 0, as_stream(stream), src, a, H, W,
                       dst, plane);
    const int rcl = check_launch("rain_synthesize (warp)");
    if (rcl != DADET_OK) return rcl;
    for (int c = 0; c < kRainChains; ++c) src.p[c] = dst + plane * c;
  }
  return DADET_OK;
}
