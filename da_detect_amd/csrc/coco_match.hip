// COCO box matching for a whole dataset in one launch: one workgroup per (image, category) pair.
//
//   1) every thread fills the pair's IoU matrix [D][G] in float64, in the stated operation order (the library is built with
//      -ffp-contract=off, so the values are those of a host float64 evaluation of the same expressions, bit for bit);
//   2) lane l < T * A of the first wave runs the sequential greedy pass of (threshold l / A, area range l % A) over that
//      matrix: the variants are independent, each walks detections and ground truths in the same fixed order;
//   3) one matched and one ignored byte per (threshold, area, detection), one count of non-ignored ground truths per
//      (pair, area).
//
// The pair's scratch (matrix, one flag byte per ground truth, one "taken" byte per ground truth and variant) lives in LDS when
// it fits the 160 KiB of a CU and in the caller's workspace otherwise; the launch asks for the LDS of the largest pair
// that fits.  No atomics, nothing depends on timing: every byte of the output has exactly one writer.
#include "pair_tables.h"

namespace dadet {
namespace {

constexpr int kCocoThreads = 256;
constexpr int kCocoMaxDet = 100;         // detections per pair after the cut
constexpr int kCocoMaxThr = 16;
constexpr int kCocoMaxArea = 4;
constexpr int kCocoMaxLanes = 64;        // T * A variants: one wave
constexpr size_t kCocoLdsLimit = 160 * 1024;
constexpr unsigned char kCrowdBit = 0x80;

struct CocoParams {
  double thr[kCocoMaxThr];
  double lo[kCocoMaxArea];
  double hi[kCocoMaxArea];
  int n_thr, n_area;
};

// scratch of one pair: iou double[D * G] | flags u8[G] | taken u8[G * lanes], padded to 8 bytes
__host__ __device__ inline size_t coco_scratch_bytes(int D, int G, int lanes) {
  const size_t raw = sizeof(double) * (size_t)D * (size_t)G + (size_t)G * (size_t)(1 + lanes);
  return (raw + 7) & ~(size_t)7;
}

__global__ __launch_bounds__(kCocoThreads) void coco_match_kernel(
    const double* __restrict__ det_box, const double* __restrict__ gt_box, const double* __restrict__ gt_area,
    const int* __restrict__ gt_crowd, const int* __restrict__ det_off, const int* __restrict__ gt_off,
    const long long* __restrict__ ws_off, unsigned char* __restrict__ ws, CocoParams prm, int n_det,
    unsigned char* __restrict__ matched, unsigned char* __restrict__ ignored, int* __restrict__ npig) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int p = blockIdx.x;
  const int d0 = det_off[p], D = det_off[p + 1] - d0;
  const int g0 = gt_off[p], G = gt_off[p + 1] - g0;
  const int A = prm.n_area, lanes = prm.n_thr * prm.n_area;
  const long long off = ws_off[p];
  unsigned char* base = off >= 0 ? ws + off : reinterpret_cast<unsigned char*>(smem);
  double* iou = reinterpret_cast<double*>(base);
  unsigned char* flags = base + sizeof(double) * (size_t)D * (size_t)G;
  unsigned char* taken = flags + G;

  // per ground truth: bit a = ignored in area range a (crowd, or area outside [lo, hi]); bit 7 = crowd
  for (int g = threadIdx.x; g < G; g += kCocoThreads) {
    const double ar = gt_area[g0 + g];
    const bool crowd = gt_crowd[g0 + g] != 0;
    unsigned f = crowd ? kCrowdBit : 0u;
    for (int a = 0; a < A; ++a)
      if (crowd || ar < prm.lo[a] || ar > prm.hi[a]) f |= 1u << a;
    flags[g] = (unsigned char)f;
  }
  for (size_t i = threadIdx.x; i < (size_t)G * lanes; i += kCocoThreads) taken[i] = 0;
  // IoU, boxes xywh: i = max(w, 0) * max(h, 0), iou = i / ((da + ga) - i), for a crowd ground truth i / da; an empty
  // intersection is 0 (also where both areas are 0)
  for (size_t e = threadIdx.x; e < (size_t)D * G; e += kCocoThreads) {
    const int d = (int)(e / G), g = (int)(e - (size_t)d * G);
    const double* db = det_box + 4 * (size_t)(d0 + d);
    const double* gb = gt_box + 4 * (size_t)(g0 + g);
    const double dx = db[0], dy = db[1], dw = db[2], dh = db[3];
    const double gx = gb[0], gy = gb[1], gw = gb[2], gh = gb[3];
    const double w = fmin(dx + dw, gx + gw) - fmax(dx, gx);
    const double h = fmin(dy + dh, gy + gh) - fmax(dy, gy);
    const double inter = fmax(w, 0.0) * fmax(h, 0.0);
    const double da = dw * dh, ga = gw * gh;
    const double uni = gt_crowd[g0 + g] != 0 ? da : (da + ga) - inter;
    iou[e] = inter > 0.0 ? inter / uni : 0.0;
  }
  __syncthreads();

  const int l = threadIdx.x;
  if (l >= lanes) return;
  const int t = l / A, a = l - t * A;
  const unsigned abit = 1u << a;
  const double lo = prm.lo[a], hi = prm.hi[a];
  if (t == 0) {
    int n = 0;
    for (int g = 0; g < G; ++g) n += (flags[g] & abit) ? 0 : 1;
    npig[(size_t)p * A + a] = n;
  }
  unsigned char* mine = taken + (size_t)l * G;
  const size_t row = (size_t)l * (size_t)n_det + (size_t)d0;
  const double start = fmin(prm.thr[t], 1.0 - 1e-10);
  for (int d = 0; d < D; ++d) {
    const double* r = iou + (size_t)d * G;
    double best = start;
    int m = -1;
    // the non-ignored ground truths in annotation order (none of them is crowd) ...
    for (int g = 0; g < G; ++g) {
      if ((flags[g] & abit) || mine[g]) continue;
      const double v = r[g];
      if (v < best) continue;
      best = v;
      m = g;
    }
    // ... then, only while no match is held, the ignored ones; a crowd box can be matched again and again
    if (m < 0) {
      for (int g = 0; g < G; ++g) {
        const unsigned f = flags[g];
        if (!(f & abit) || (mine[g] && !(f & kCrowdBit))) continue;
        const double v = r[g];
        if (v < best) continue;
        best = v;
        m = g;
      }
    }
    bool ign;
    if (m >= 0) {
      ign = (flags[m] & abit) != 0;
      if (!(flags[m] & kCrowdBit)) mine[m] = 1;
    } else {
      const double* db = det_box + 4 * (size_t)(d0 + d);
      const double da = db[2] * db[3];
      ign = da < lo || da > hi;
    }
    matched[row + d] = m >= 0 ? 1 : 0;
    ignored[row + d] = ign ? 1 : 0;
  }
}

// The checks shared by the query and the launch: the threshold and area counts, then the offset tables (pair_tables.h), where
// no pair may hold more than kCocoMaxDet detections.
int coco_layout(const int* det_off_host, const int* gt_off_host, int pairs, int n_det, int n_gt, int n_thr, int n_area,
                PairLayout* out) {
  DADET_REQUIRE(n_thr >= 1 && n_thr <= kCocoMaxThr && n_area >= 1 && n_area <= kCocoMaxArea && n_thr * n_area <= kCocoMaxLanes,
                "coco_match: %d thresholds x %d area ranges; at most %d x %d and %d variants", n_thr, n_area, kCocoMaxThr,
                kCocoMaxArea, kCocoMaxLanes);
  const int lanes = n_thr * n_area;
  return pair_layout("coco_match", kCocoLdsLimit, det_off_host, gt_off_host, pairs, n_det, n_gt,
                     [lanes](int p, int D, int G, size_t* need) {
                       DADET_REQUIRE(D <= kCocoMaxDet, "coco_match: pair %d has %d detections; at most %d after the cut", p, D,
                                     kCocoMaxDet);
                       *need = coco_scratch_bytes(D, G, lanes);
                       return DADET_OK;
                     },
                     out);
}

}  // namespace
}  // namespace dadet

using namespace dadet;

extern "C" int dadet_coco_match_workspace_bytes(const int* det_off_host, const int* gt_off_host, int pairs, int n_det, int n_gt,
                                                int n_thr, int n_area, size_t* bytes_out) {
  DADET_REQUIRE(bytes_out, "coco_match_workspace_bytes: null output");
  PairLayout lay;
  const int rc = coco_layout(det_off_host, gt_off_host, pairs, n_det, n_gt, n_thr, n_area, &lay);
  if (rc != DADET_OK) return rc;
  *bytes_out = lay.total;
  return DADET_OK;
}

extern "C" int dadet_coco_match(const double* det_box, const double* gt_box, const double* gt_area, const int* gt_crowd,
                                const int* det_off_host, const int* gt_off_host, int pairs, int n_det, int n_gt,
                                const double* iou_thr_host, int n_thr, const double* area_rng_host, int n_area, void* workspace,
                                size_t workspace_bytes, unsigned char* matched_out, unsigned char* ignored_out, int* npig_out,
                                void* stream) {
  PairLayout lay;
  int rc = coco_layout(det_off_host, gt_off_host, pairs, n_det, n_gt, n_thr, n_area, &lay);
  if (rc != DADET_OK) return rc;
  DADET_REQUIRE(iou_thr_host && area_rng_host, "coco_match: null threshold / area table");
  if (pairs == 0) return DADET_OK;
  DADET_REQUIRE(n_det == 0 || (det_box && matched_out && ignored_out), "coco_match: null detection buffer");
  DADET_REQUIRE(n_gt == 0 || (gt_box && gt_area && gt_crowd), "coco_match: null ground-truth buffer");
  DADET_REQUIRE(npig_out && workspace, "coco_match: null output / workspace");
  DADET_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "coco_match: workspace must be 8-byte aligned");
  if (workspace_bytes < lay.total) {
    set_error("coco_match: workspace %zu B < %zu B", workspace_bytes, lay.total);
    return DADET_EWORKSPACE;
  }
  CocoParams prm;
  for (int t = 0; t < kCocoMaxThr; ++t) prm.thr[t] = t < n_thr ? iou_thr_host[t] : 0.0;
  for (int a = 0; a < kCocoMaxArea; ++a) {
    prm.lo[a] = a < n_area ? area_rng_host[2 * a] : 0.0;
    prm.hi[a] = a < n_area ? area_rng_host[2 * a + 1] : 0.0;
  }
  prm.n_thr = n_thr;
  prm.n_area = n_area;

  hipStream_t st = as_stream(stream);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  const int *d_det_off, *d_gt_off;
  const long long* d_ws_off;
  rc = pair_tables_upload("coco_match", lay, det_off_host, gt_off_host, pairs, ws, st, &d_det_off, &d_gt_off, &d_ws_off);
  if (rc != DADET_OK) return rc;
  if (lay.lds > 48 * 1024) {
    rc = raise_lds("coco_match", coco_match_kernel, lay.lds);
    if (rc != DADET_OK) return rc;
  }
  hipLaunchKernelGGL(coco_match_kernel, dim3((unsigned)pairs), dim3(kCocoThreads), lay.lds, st, det_box, gt_box, gt_area, gt_crowd,
                     d_det_off, d_gt_off, d_ws_off, ws, prm, n_det, matched_out, ignored_out, npig_out);
  return check_launch("coco_match");
}
