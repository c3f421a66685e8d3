// PASCAL VOC box matching for a whole dataset in one launch: one workgroup per (image, class) pair.
//
// The rule (the reference's calc_detection_voc_prec_rec): every detection has ONE candidate, the ground truth of its pair
// with the largest IoU (first index on ties), whatever earlier detections took; below the threshold it has none.  A
// candidate that is `difficult` gives -1; otherwise the best-ranked detection with that candidate gives 1 and every later
// one 0.  "Best-ranked with candidate g" is the SMALLEST detection index whose candidate is g, so nothing is sequential:
//
//   1) the pair's ground truths go to LDS: box (x2, y2 already + 1) | first[t][g] = INT_MAX | difficult byte;
//   2) threads stride over the detections; each scans the ground truths for its running argmax in float32, in the stated
//      operation order (the library is built with -ffp-contract=off and fp32 division is correctly rounded, so the values
//      are those of a host float32 evaluation of the same expressions, bit for bit), writes gt_index / iou_max and does
//      atomicMin(&first[t][g], d) for every threshold the maximum reaches;
//   3) after a barrier each thread reads its own gt_index / iou_max back and writes its match bytes.
//
// A minimum does not depend on the order of arrival, so the result is deterministic; every output byte has one writer.  No
// D x G matrix exists and D is not capped.  A pair whose ground truths do not fit the 160 KiB of a CU keeps the same scratch
// in the caller's workspace (the atomics then go to global memory, for that pair only).
#include <climits>

#include "pair_tables.h"

namespace dadet {
namespace {

constexpr int kVocThreads = 256;
constexpr int kVocMaxThr = 16;
constexpr size_t kVocLdsLimit = 160 * 1024 - 16;      // the 160 KiB of a CU less the kernel's one static counter

struct VocParams {
  double thr[kVocMaxThr];
  int n_thr;
};

// scratch of one pair: box float4[G] | first int[T * G] | difficult u8[G], padded to 16 bytes
__host__ __device__ inline size_t voc_scratch_bytes(int G, int T) {
  const size_t raw = (size_t)G * (size_t)(16 + 1 + 4 * T);
  return (raw + 15) & ~(size_t)15;
}

__global__ __launch_bounds__(kVocThreads) void voc_match_kernel(
    const float* __restrict__ det_box, const float* __restrict__ gt_box, const unsigned char* __restrict__ gt_difficult,
    const int* __restrict__ det_off, const int* __restrict__ gt_off, const long long* __restrict__ ws_off,
    unsigned char* __restrict__ ws, VocParams prm, int n_det, signed char* __restrict__ match, int* __restrict__ n_pos,
    int* gt_index, float* iou_max) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ int pos_count;
  const int p = blockIdx.x;
  const int d0 = det_off[p], D = det_off[p + 1] - d0;
  const int g0 = gt_off[p], G = gt_off[p + 1] - g0;
  const int T = prm.n_thr;
  const long long off = ws_off[p];
  unsigned char* base = off >= 0 ? ws + off : reinterpret_cast<unsigned char*>(smem);
  float4* box = reinterpret_cast<float4*>(base);
  int* first = reinterpret_cast<int*>(base + sizeof(float4) * (size_t)G);
  unsigned char* difficult = base + (size_t)G * (size_t)(16 + 4 * T);

  if (threadIdx.x == 0) pos_count = 0;
  __syncthreads();
  int mine = 0;
  for (int g = threadIdx.x; g < G; g += kVocThreads) {
    const float* gb = gt_box + 4 * (size_t)(g0 + g);
    box[g] = make_float4(gb[0], gb[1], gb[2] + 1.0f, gb[3] + 1.0f);     // "VOC evaluation follows integer typed boxes"
    const unsigned char df = gt_difficult[g0 + g] != 0 ? 1 : 0;
    difficult[g] = df;
    mine += df ? 0 : 1;
  }
  for (size_t i = threadIdx.x; i < (size_t)T * G; i += kVocThreads)
    __hip_atomic_store(first + i, INT_MAX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (mine) atomicAdd(&pos_count, mine);
  __syncthreads();
  if (threadIdx.x == 0) n_pos[p] = pos_count;

  // IoU of the "+1" convention on boxes whose x2, y2 were already raised by 1: area = (x2 - x1 + 1) * (y2 - y1 + 1),
  // wh = max(min(rb) - max(lt) + 1, 0), iou = inter / ((area_d + area_g) - inter).  numpy's argmax: the first maximum, and a
  // NaN (only degenerate boxes make one) counts as the largest value.
  for (int d = threadIdx.x; d < D; d += kVocThreads) {
    const float* db = det_box + 4 * (size_t)(d0 + d);
    const float dx1 = db[0], dy1 = db[1], dx2 = db[2] + 1.0f, dy2 = db[3] + 1.0f;
    const float da = (dx2 - dx1 + 1.0f) * (dy2 - dy1 + 1.0f);
    float best = 0.0f;
    int m = -1;
    for (int g = 0; g < G; ++g) {
      const float4 b = box[g];
      const float ga = (b.z - b.x + 1.0f) * (b.w - b.y + 1.0f);
      const float w = fmaxf(fminf(dx2, b.z) - fmaxf(dx1, b.x) + 1.0f, 0.0f);
      const float h = fmaxf(fminf(dy2, b.w) - fmaxf(dy1, b.y) + 1.0f, 0.0f);
      const float inter = w * h;
      const float v = inter / ((da + ga) - inter);
      if (g == 0 || v > best || (v != v && best == best)) {
        best = v;
        m = g;
      }
    }
    gt_index[d0 + d] = m;
    iou_max[d0 + d] = best;
    if (m >= 0 && !difficult[m])
      for (int t = 0; t < T; ++t)
        if (!((double)best < prm.thr[t])) atomicMin(first + (size_t)t * G + m, d);
  }
  __syncthreads();

  for (int d = threadIdx.x; d < D; d += kVocThreads) {
    const int m = gt_index[d0 + d];                   // this thread's own stores above
    const float best = iou_max[d0 + d];
    for (int t = 0; t < T; ++t) {
      signed char r = 0;
      if (m >= 0 && !((double)best < prm.thr[t])) {
        if (difficult[m])
          r = -1;
        else
          r = __hip_atomic_load(first + (size_t)t * G + m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == d ? 1 : 0;
      }
      match[(size_t)t * (size_t)n_det + (size_t)(d0 + d)] = r;
    }
  }
}

// The checks shared by the query and the launch: the threshold count, then the offset tables (pair_tables.h).
int voc_layout(const int* det_off_host, const int* gt_off_host, int pairs, int n_det, int n_gt, int n_thr, PairLayout* out) {
  DADET_REQUIRE(n_thr >= 1 && n_thr <= kVocMaxThr, "voc_match: %d thresholds; 1 to %d", n_thr, kVocMaxThr);
  return pair_layout("voc_match", kVocLdsLimit, det_off_host, gt_off_host, pairs, n_det, n_gt,
                     [n_thr](int, int, int G, size_t* need) {
                       *need = voc_scratch_bytes(G, n_thr);
                       return DADET_OK;
                     },
                     out);
}

}  // namespace
}  // namespace dadet

using namespace dadet;

extern "C" int dadet_voc_match_workspace_bytes(const int* det_off_host, const int* gt_off_host, int pairs, int n_det, int n_gt,
                                               int n_thr, size_t* bytes_out) {
  DADET_REQUIRE(bytes_out, "voc_match_workspace_bytes: null output");
  PairLayout lay;
  const int rc = voc_layout(det_off_host, gt_off_host, pairs, n_det, n_gt, n_thr, &lay);
  if (rc != DADET_OK) return rc;
  *bytes_out = lay.total;
  return DADET_OK;
}

extern "C" int dadet_voc_match(const float* det_box, const float* gt_box, const unsigned char* gt_difficult,
                               const int* det_off_host, const int* gt_off_host, int pairs, int n_det, int n_gt,
                               const double* iou_thr_host, int n_thr, void* workspace, size_t workspace_bytes,
                               signed char* match_out, int* n_pos_out, int* gt_index_out, float* iou_max_out, void* stream) {
  PairLayout lay;
  int rc = voc_layout(det_off_host, gt_off_host, pairs, n_det, n_gt, n_thr, &lay);
  if (rc != DADET_OK) return rc;
  DADET_REQUIRE(iou_thr_host, "voc_match: null threshold table");
  if (pairs == 0) return DADET_OK;
  DADET_REQUIRE(n_det == 0 || (det_box && match_out && gt_index_out && iou_max_out), "voc_match: null detection buffer");
  DADET_REQUIRE(n_gt == 0 || (gt_box && gt_difficult), "voc_match: null ground-truth buffer");
  DADET_REQUIRE(n_pos_out && workspace, "voc_match: null output / workspace");
  DADET_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "voc_match: workspace must be 16-byte aligned");
  if (workspace_bytes < lay.total) {
    set_error("voc_match: workspace %zu B < %zu B", workspace_bytes, lay.total);
    return DADET_EWORKSPACE;
  }
  VocParams prm;
  for (int t = 0; t < kVocMaxThr; ++t) prm.thr[t] = t < n_thr ? iou_thr_host[t] : 0.0;
  prm.n_thr = n_thr;

  hipStream_t st = as_stream(stream);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  const int *d_det_off, *d_gt_off;
  const long long* d_ws_off;
  rc = pair_tables_upload("voc_match", lay, det_off_host, gt_off_host, pairs, ws, st, &d_det_off, &d_gt_off, &d_ws_off);
  if (rc != DADET_OK) return rc;
  if (lay.lds > 48 * 1024) {
    rc = raise_lds("voc_match", voc_match_kernel, lay.lds);
    if (rc != DADET_OK) return rc;
  }
  hipLaunchKernelGGL(voc_match_kernel, dim3((unsigned)pairs), dim3(kVocThreads), lay.lds, st, det_box, gt_box, gt_difficult,
                     d_det_off, d_gt_off, d_ws_off, ws, prm, n_det, match_out, n_pos_out, gt_index_out, iou_max_out);
  return check_launch("voc_match");
}
