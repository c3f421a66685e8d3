// Host-side scaffold of the per-(image, class) pair matchers (coco_match.hip, voc_match.hip): the checks of the
// two offset tables, the workspace layout and the upload of the validated tables.
//
// Workspace: det_off int[pairs + 1] | gt_off int[pairs + 1] | (to 8 bytes) ws_off i64[max(pairs, 1)] | (to 256 bytes) the
// scratch of every pair that does not fit LDS, back to back.  ws_off[p] is that pair's byte offset, or -1 for "in LDS".
#pragma once
#include <algorithm>
#include <vector>

#include "common.h"

namespace dadet {

struct PairLayout {
  size_t total;           // bytes of the whole workspace
  size_t lds;             // dynamic LDS of the launch: the largest pair that fits
  std::vector<long long> ws_off;
};

inline size_t pair_tables_head(int pairs) { return (sizeof(int) * 2 * (size_t)(pairs + 1) + 7) & ~(size_t)7; }

// Both tables start at 0, never decrease, stay inside and end at the array sizes.  scratch(p, D, G, &bytes) gives the
// scratch of pair p or refuses the pair (it sets the error and returns its status).  Fills the layout.
template <typename Scratch>
int pair_layout(const char* who, size_t lds_limit, const int* det_off_host, const int* gt_off_host, int pairs, int n_det, int n_gt,
                Scratch scratch, PairLayout* out) {
  DADET_REQUIRE(pairs >= 0 && n_det >= 0 && n_gt >= 0, "%s: negative size (pairs %d, n_det %d, n_gt %d)", who, pairs, n_det, n_gt);
  DADET_REQUIRE(det_off_host && gt_off_host, "%s: null offset table", who);
  DADET_REQUIRE(det_off_host[0] == 0 && gt_off_host[0] == 0, "%s: offset tables must start at 0 (%d, %d)", who, det_off_host[0],
                gt_off_host[0]);
  const size_t tables = pair_tables_head(pairs) + sizeof(long long) * (size_t)std::max(pairs, 1);
  size_t at = (tables + 255) & ~(size_t)255, lds = 0;
  out->ws_off.assign((size_t)std::max(pairs, 1), -1);
  for (int p = 0; p < pairs; ++p) {
    const int D = det_off_host[p + 1] - det_off_host[p], G = gt_off_host[p + 1] - gt_off_host[p];
    DADET_REQUIRE(D >= 0 && G >= 0, "%s: offsets decrease at pair %d", who, p);
    DADET_REQUIRE(det_off_host[p + 1] <= n_det && gt_off_host[p + 1] <= n_gt,
                  "%s: offsets of pair %d (%d, %d) run past the arrays (%d, %d)", who, p, det_off_host[p + 1], gt_off_host[p + 1],
                  n_det, n_gt);
    size_t need = 0;
    const int rc = scratch(p, D, G, &need);
    if (rc != DADET_OK) return rc;
    if (need <= lds_limit) {
      lds = std::max(lds, need);
    } else {
      out->ws_off[p] = (long long)at;
      at += need;
    }
  }
  DADET_REQUIRE(det_off_host[pairs] == n_det && gt_off_host[pairs] == n_gt,
                "%s: offset tables end at (%d, %d), the arrays hold (%d, %d)", who, det_off_host[pairs], gt_off_host[pairs], n_det,
                n_gt);
  out->total = at;
  out->lds = lds;
  return DADET_OK;
}

// The validated tables themselves go to the device: what the kernel indexes with is what pair_layout checked.  lay.ws_off
// dies with the caller, so the upload is waited for (the tables are a few KB; the one host wait of a matcher's launch).
// Needs pairs >= 1 and a workspace of lay.total bytes, 8-byte aligned.
inline int pair_tables_upload(const char* who, const PairLayout& lay, const int* det_off_host, const int* gt_off_host, int pairs,
                              unsigned char* ws, hipStream_t st, const int** d_det_off, const int** d_gt_off,
                              const long long** d_ws_off) {
  int* det = reinterpret_cast<int*>(ws);
  int* gt = det + (pairs + 1);
  long long* off = reinterpret_cast<long long*>(ws + pair_tables_head(pairs));
  if (hipMemcpyAsync(det, det_off_host, sizeof(int) * (size_t)(pairs + 1), hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(gt, gt_off_host, sizeof(int) * (size_t)(pairs + 1), hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(off, lay.ws_off.data(), sizeof(long long) * (size_t)pairs, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess) {
    (void)hipGetLastError();
    set_error("%s: upload of the offset tables failed", who);
    return DADET_ELAUNCH;
  }
  *d_det_off = det;
  *d_gt_off = gt;
  *d_ws_off = off;
  return DADET_OK;
}

}  // namespace dadet
