// Error breakdown of detections for a whole dataset in one launch: one workgroup per IMAGE, which sees the
// ground truths of all classes at once — what tells a classification error (right place, wrong label) from background.
//
// The rule sits on top of voc_match.hip's.  Every detection d (ranked by descending score) keeps three running maxima of the
// float32 "+1" IoU over its image's ground truths, first maximum wins, 0.0 / -1 without a candidate:
//   cand: ground truths of d's class, difficult ones included (the VOC candidate);
//   s:    the non-difficult ground truths of d's class;        o: the non-difficult ground truths of every other class.
// With "v >= t" read as !((double)v < t):  ignored (1) when cand is difficult and IoU(cand) >= t_f;  TP (0) when IoU(cand) >=
// t_f, cand is not difficult and d is the best-ranked detection with that cand.  Every other detection is a false positive
// of the first kind that holds:  Loc (3) t_b <= s < t_f;  Cls (2) o >= t_f;  Dupe (5) s >= t_f;  Bkg (6) s < t_b and o < t_b;
// Both (4) otherwise.  det_gt: cand for TP / ignored / Dupe, argmax s for Loc, argmax o for Cls / Both, -1 for Bkg.  det_fix:
// the best-ranked Loc (and, separately, the best-ranked Cls) detection of a ground truth that has no TP.  gt_state: 0 detected
// (gt_det = its TP), 1 difficult, 2 covered (not detected, but the det_gt of a Loc or Cls detection), 3 missed.
//
// "Best-ranked" is the smallest detection index, an atomicMin, so nothing is sequential:
//   1) the image's ground truths go to LDS: box (x2, y2 already + 1) | label | claim[3][g] = INT_MAX (TP, Loc, Cls) |
//      difficult byte — 33 bytes each;
//   2) threads stride over the detections: the scan, iou_same / iou_other, every kind that does not hang on a claim, and the
//      TP claim of a detection whose candidate qualifies;
//   3) after a barrier the claimants learn whether they won (a loser is Cls or Dupe; only the Cls one scans again, for the
//      argmax of o it did not keep), and Loc / Cls detections of a ground truth without TP make their fix claims;
//   4) after a second barrier det_fix, gt_state and gt_det are read off the claim words.
// A minimum does not depend on the order of arrival and every output byte has one writer: the result is deterministic.
// Detections per image are not capped.  An image whose ground truths do not fit the 160 KiB of a CU keeps the same scratch
// in the caller's workspace (the atomics then go to global memory, for that image only).
#include <climits>

#include "pair_tables.h"

namespace dadet {
namespace {

constexpr int kErrThreads = 256;
constexpr size_t kErrLdsLimit = 160 * 1024;
constexpr int kErrGtBytes = 16 + 4 + 3 * 4 + 1;

enum : unsigned char { kTP = 0, kIgnored = 1, kCls = 2, kLoc = 3, kBoth = 4, kDupe = 5, kBkg = 6, kClaimant = 255 };
enum : unsigned char { kDetected = 0, kDifficult = 1, kCovered = 2, kMissed = 3 };

// scratch of one image: box float4[G] | label int[G] | claim int[3 * G] | difficult u8[G], padded to 16 bytes
__host__ __device__ inline size_t err_scratch_bytes(int G) {
  const size_t raw = (size_t)G * (size_t)kErrGtBytes;
  return (raw + 15) & ~(size_t)15;
}

struct ErrScan {
  float cand, same, other;
  int cand_g, same_g, other_g;
};

// The three maxima of one detection.  IoU: voc_match.hip's expression on boxes whose x2, y2 were already raised by 1.
__device__ inline ErrScan err_scan(const float* __restrict__ db, int label, const float4* box, const int* gt_label,
                                   const unsigned char* difficult, int G) {
  const float dx1 = db[0], dy1 = db[1], dx2 = db[2] + 1.0f, dy2 = db[3] + 1.0f;
  const float da = (dx2 - dx1 + 1.0f) * (dy2 - dy1 + 1.0f);
  ErrScan r = {0.0f, 0.0f, 0.0f, -1, -1, -1};
  for (int g = 0; g < G; ++g) {
    const float4 b = box[g];
    const float ga = (b.z - b.x + 1.0f) * (b.w - b.y + 1.0f);
    const float w = fmaxf(fminf(dx2, b.z) - fmaxf(dx1, b.x) + 1.0f, 0.0f);
    const float h = fmaxf(fminf(dy2, b.w) - fmaxf(dy1, b.y) + 1.0f, 0.0f);
    const float inter = w * h;
    const float v = inter / ((da + ga) - inter);
    const bool hard = difficult[g] != 0;
    if (gt_label[g] == label) {
      if (r.cand_g < 0 || v > r.cand) r.cand = v, r.cand_g = g;
      if (!hard && (r.same_g < 0 || v > r.same)) r.same = v, r.same_g = g;
    } else if (!hard && (r.other_g < 0 || v > r.other)) {
      r.other = v, r.other_g = g;
    }
  }
  return r;
}

__device__ inline bool reaches(float v, double t) { return !((double)v < t); }

// kind of a false positive from its two maxima, in the order Loc, Cls, Dupe, Bkg, Both
__device__ inline unsigned char err_fp_kind(float same, float other, double tf, double tb) {
  if (reaches(same, tb) && !reaches(same, tf)) return kLoc;
  if (reaches(other, tf)) return kCls;
  if (reaches(same, tf)) return kDupe;
  if (!reaches(same, tb) && !reaches(other, tb)) return kBkg;
  return kBoth;
}

__device__ inline int claim_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(kErrThreads) void error_match_kernel(
    const float* __restrict__ det_box, const int* __restrict__ det_label, const float* __restrict__ gt_box,
    const int* __restrict__ gt_label_in, const unsigned char* __restrict__ gt_difficult, const int* __restrict__ det_off,
    const int* __restrict__ gt_off, const long long* __restrict__ ws_off, unsigned char* __restrict__ ws, double tf, double tb,
    unsigned char* det_kind, int* det_gt, float* __restrict__ iou_same, float* __restrict__ iou_other,
    unsigned char* __restrict__ det_fix, unsigned char* __restrict__ gt_state, int* __restrict__ gt_det) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int p = blockIdx.x;
  const int d0 = det_off[p], D = det_off[p + 1] - d0;
  const int g0 = gt_off[p], G = gt_off[p + 1] - g0;
  const long long off = ws_off[p];
  unsigned char* base = off >= 0 ? ws + off : reinterpret_cast<unsigned char*>(smem);
  float4* box = reinterpret_cast<float4*>(base);
  int* label = reinterpret_cast<int*>(base + sizeof(float4) * (size_t)G);
  int* claim_tp = label + G;
  int* claim_loc = claim_tp + G;
  int* claim_cls = claim_loc + G;
  unsigned char* difficult = base + (size_t)G * (size_t)(kErrGtBytes - 1);

  for (int g = threadIdx.x; g < G; g += kErrThreads) {
    const float* gb = gt_box + 4 * (size_t)(g0 + g);
    box[g] = make_float4(gb[0], gb[1], gb[2] + 1.0f, gb[3] + 1.0f);
    label[g] = gt_label_in[g0 + g];
    difficult[g] = gt_difficult[g0 + g] != 0 ? 1 : 0;
    __hip_atomic_store(claim_tp + g, INT_MAX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(claim_loc + g, INT_MAX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(claim_cls + g, INT_MAX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();

  for (int d = threadIdx.x; d < D; d += kErrThreads) {
    const ErrScan r = err_scan(det_box + 4 * (size_t)(d0 + d), det_label[d0 + d], box, label, difficult, G);
    iou_same[d0 + d] = r.same;
    iou_other[d0 + d] = r.other;
    unsigned char kind;
    int g;
    if (r.cand_g >= 0 && reaches(r.cand, tf)) {
      g = r.cand_g;
      if (difficult[g]) {
        kind = kIgnored;
      } else {
        kind = kClaimant;                                 // TP if it wins the claim, else Cls or Dupe: decided below
        atomicMin(claim_tp + g, d);
      }
    } else {
      kind = err_fp_kind(r.same, r.other, tf, tb);
      g = kind == kLoc ? r.same_g : (kind == kCls || kind == kBoth) ? r.other_g : kind == kDupe ? r.cand_g : -1;
    }
    det_kind[d0 + d] = kind;
    det_gt[d0 + d] = g >= 0 ? g0 + g : -1;
  }
  __syncthreads();

  for (int d = threadIdx.x; d < D; d += kErrThreads) {
    unsigned char kind = det_kind[d0 + d];                // this thread's own stores above
    int g = det_gt[d0 + d] - g0;
    if (kind == kClaimant) {
      if (claim_load(claim_tp + g) == d) {
        kind = kTP;
      } else {
        kind = err_fp_kind(iou_same[d0 + d], iou_other[d0 + d], tf, tb);      // s = IoU(cand) >= t_f: Cls or Dupe
        if (kind == kCls) {
          g = err_scan(det_box + 4 * (size_t)(d0 + d), det_label[d0 + d], box, label, difficult, G).other_g;
          det_gt[d0 + d] = g0 + g;
        }
      }
      det_kind[d0 + d] = kind;
    }
    if ((kind == kLoc || kind == kCls) && claim_load(claim_tp + g) == INT_MAX) atomicMin((kind == kLoc ? claim_loc : claim_cls) + g, d);
  }
  __syncthreads();

  for (int d = threadIdx.x; d < D; d += kErrThreads) {
    const unsigned char kind = det_kind[d0 + d];
    unsigned char fix = 0;
    if (kind == kLoc || kind == kCls) {
      const int g = det_gt[d0 + d] - g0;
      fix = claim_load(claim_tp + g) == INT_MAX && claim_load((kind == kLoc ? claim_loc : claim_cls) + g) == d ? 1 : 0;
    }
    det_fix[d0 + d] = fix;
  }
  for (int g = threadIdx.x; g < G; g += kErrThreads) {
    const int tp = claim_load(claim_tp + g);
    unsigned char state;
    if (difficult[g])
      state = kDifficult;
    else if (tp != INT_MAX)
      state = kDetected;
    else
      state = claim_load(claim_loc + g) != INT_MAX || claim_load(claim_cls + g) != INT_MAX ? kCovered : kMissed;
    gt_state[g0 + g] = state;
    gt_det[g0 + g] = state == kDetected ? d0 + tp : -1;
  }
}

int err_layout(const int* det_off_host, const int* gt_off_host, int images, int n_det, int n_gt, PairLayout* out) {
  return pair_layout("error_match", kErrLdsLimit, det_off_host, gt_off_host, images, n_det, n_gt,
                     [](int, int, int G, size_t* need) {
                       *need = err_scratch_bytes(G);
                       return DADET_OK;
                     },
                     out);
}

}  // namespace
}  // namespace dadet

using namespace dadet;

extern "C" int dadet_error_match_workspace_bytes(const int* det_off_host, const int* gt_off_host, int images, int n_det, int n_gt,
                                                 size_t* bytes_out) {
  DADET_REQUIRE(bytes_out, "error_match_workspace_bytes: null output");
  PairLayout lay;
  const int rc = err_layout(det_off_host, gt_off_host, images, n_det, n_gt, &lay);
  if (rc != DADET_OK) return rc;
  *bytes_out = lay.total;
  return DADET_OK;
}

extern "C" int dadet_error_match(const float* det_box, const int* det_label, const float* gt_box, const int* gt_label,
                                 const unsigned char* gt_difficult, const int* det_off_host, const int* gt_off_host, int images,
                                 int n_det, int n_gt, double pos_thr, double bg_thr, void* workspace, size_t workspace_bytes,
                                 unsigned char* det_kind, int* det_gt, float* iou_same, float* iou_other, unsigned char* det_fix,
                                 unsigned char* gt_state, int* gt_det, void* stream) {
  PairLayout lay;
  int rc = err_layout(det_off_host, gt_off_host, images, n_det, n_gt, &lay);
  if (rc != DADET_OK) return rc;
  DADET_REQUIRE(0.0 < bg_thr && bg_thr < pos_thr && pos_thr <= 1.0, "error_match: thresholds need 0 < bg (%g) < pos (%g) <= 1", bg_thr,
                pos_thr);
  if (images == 0) return DADET_OK;
  DADET_REQUIRE(n_det == 0 || (det_box && det_label && det_kind && det_gt && iou_same && iou_other && det_fix),
                "error_match: null detection buffer");
  DADET_REQUIRE(n_gt == 0 || (gt_box && gt_label && gt_difficult && gt_state && gt_det), "error_match: null ground-truth buffer");
  DADET_REQUIRE(workspace, "error_match: null workspace");
  DADET_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "error_match: workspace must be 16-byte aligned");
  if (workspace_bytes < lay.total) {
    set_error("error_match: workspace %zu B < %zu B", workspace_bytes, lay.total);
    return DADET_EWORKSPACE;
  }

  hipStream_t st = as_stream(stream);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  const int *d_det_off, *d_gt_off;
  const long long* d_ws_off;
  rc = pair_tables_upload("error_match", lay, det_off_host, gt_off_host, images, ws, st, &d_det_off, &d_gt_off, &d_ws_off);
  if (rc != DADET_OK) return rc;
  if (lay.lds > 48 * 1024) {
    rc = raise_lds("error_match", error_match_kernel, lay.lds);
    if (rc != DADET_OK) return rc;
  }
  hipLaunchKernelGGL(error_match_kernel, dim3((unsigned)images), dim3(kErrThreads), lay.lds, st, det_box, det_label, gt_box,
                     gt_label, gt_difficult, d_det_off, d_gt_off, d_ws_off, ws, pos_thr, bg_thr, det_kind, det_gt, iou_same,
                     iou_other, det_fix, gt_state, gt_det);
  return check_launch("error_match");
}
