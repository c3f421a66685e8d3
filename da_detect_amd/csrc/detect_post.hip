// Detection filtering of the evaluation path entirely on the device (gfx950): score threshold, per-class greedy NMS,
// reference output order and the detections_per_img cut for a whole batch in one fixed sequence of launches.
//
// Replaces the per-image, per-class Python loop of PostProcessor.filter_results (reference:
// maskrcnn_benchmark/modeling/roi_heads/box_head/inference.py:108-149 — per class a nonzero, two gathers, _C.nms and a
// full, then kthvalue on the host), whose cost is about two host waits per class and image.
//
// Differences in HOW (results are the reference's, bit for bit):
//   a) rank: one workgroup per (image, foreground class) segment bitonic-sorts 64-bit keys in LDS.  A candidate
//      (score > thresh, strict) carries (score descending, row ascending); every other row sorts behind all candidates,
//      by row.  The candidates are therefore the first cand[s] ranks — no compaction — and their order is the one
//      _C.nms gives them (nms.hip: key_before).  LDS is sized by the batch's largest row count, not by the limit;
//   b) suppress: dadet_nms_batch on the ranked sets, at most 64 segments per call.  Either over ALL rows of a segment
//      (no host read: a lower-ranked box never changes the fate of a higher-ranked one, so the kept positions below
//      cand[s] are exactly the candidates' kept set) or, after ONE host read of cand[], over the candidates only;
//   c) emit: kept positions -> rows through the rank -> row map into an LDS bit set, per-segment scan (ascending rows),
//      per-image offsets in class order, MSB-first radix select of the detections_per_img-th largest score and a second
//      fixed-order compaction with score >= cut.  Integer LDS atomics only (bit set, histogram): the output is deterministic.
#include <vector>

#include "common.h"

namespace dadet {

constexpr int kPostMaxImages = 64;       // per-image tables travel by value with the launches
constexpr int kPostMaxRows = 16384;      // dadet_nms_batch's limit per ranked set; also 128 KiB of LDS keys
constexpr int kPostNmsChunk = 64;        // segments per dadet_nms_batch call (its by-value count table)

struct PostImages {
  int rows[kPostMaxImages];              // R_i
  int row_off[kPostMaxImages];           // sum of R_k, k < i
};

// ascending in the result <=> ascending as floats (no NaN reaches here: a candidate satisfies score > thresh)
__device__ __forceinline__ unsigned float_orderable(float f) {
  f += 0.0f;                             // -0 -> +0: the two compare equal as floats
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// ---- a) rank -----------------------------------------------------------------------------------------------------
// key = (~orderable(score) << 32) | row for a candidate, (0xFFFFFFFF << 32) | row for any other row, all ones for
// padding; ascending keys = candidates by (score desc, row asc), then the rest by row, then padding.
// (a candidate's high word is never 0xFFFFFFFF: that needs orderable == 0, the bits of a negative NaN)
__global__ __launch_bounds__(1024) void post_rank_kernel(const float4* __restrict__ boxes, const float* __restrict__ scores,
                                                         PostImages imgs, int num_classes, int n_max, float score_thresh,
                                                         float4* __restrict__ ranked, int* __restrict__ rowmap,
                                                         int* __restrict__ cand) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem);
  __shared__ int s_cand;
  const int seg = blockIdx.x;
  const int fg = num_classes - 1;
  const int img = seg / fg, cls = seg % fg + 1;
  const int n = imgs.rows[img];
  const size_t row0 = (size_t)imgs.row_off[img];
  if (threadIdx.x == 0) s_cand = 0;
  if (n == 0) {
    if (threadIdx.x == 0) cand[seg] = 0;
    return;
  }
  int npow2 = 1;
  while (npow2 < n) npow2 <<= 1;
  __syncthreads();
  int mine = 0;
  for (int i = threadIdx.x; i < npow2; i += blockDim.x) {
    unsigned long long k = ~0ULL;
    if (i < n) {
      const float s = scores[(row0 + i) * num_classes + cls];
      unsigned hi = 0xFFFFFFFFu;
      if (s > score_thresh) {
        hi = ~float_orderable(s);
        ++mine;
      }
      k = ((unsigned long long)hi << 32) | (unsigned)i;
    }
    keys[i] = k;
  }
  if (mine) atomicAdd(&s_cand, mine);
  __syncthreads();
  for (int size = 2; size <= npow2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = threadIdx.x; t < (npow2 >> 1); t += blockDim.x) {
        const int lo = 2 * t - (t & (stride - 1));
        const int hi = lo + stride;
        const bool up = ((lo & size) == 0);
        const unsigned long long a = keys[lo], b = keys[hi];
        if (up ? (b < a) : (a < b)) {
          keys[lo] = b;
          keys[hi] = a;
        }
      }
      __syncthreads();
    }
  }
  float4* out = ranked + (size_t)seg * n_max;
  int* map = rowmap + (size_t)seg * n_max;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int row = (int)(unsigned)keys[i];
    map[i] = row;
    out[i] = boxes[(row0 + row) * num_classes + cls];
  }
  if (threadIdx.x == 0) cand[seg] = s_cand;
}

// ---- c) emit -----------------------------------------------------------------------------------------------------
// One workgroup per segment: the kept candidates' rows as a bit set in LDS, then their ascending list.
// keep == nullptr: no suppression ran (nms_thresh <= 0), every candidate is kept.
__global__ __launch_bounds__(256) void post_rows_kernel(const int64_t* __restrict__ keep, const int* __restrict__ num_keep,
                                                        const int* __restrict__ rowmap, const int* __restrict__ cand,
                                                        PostImages imgs, int num_classes, int n_max,
                                                        int* __restrict__ krow, int* __restrict__ seg_kept) {
  __shared__ unsigned s_bits[kPostMaxRows / 32];
  __shared__ int s_scan[256];
  const int seg = blockIdx.x;
  const int n = imgs.rows[seg / (num_classes - 1)];
  const int nc = cand[seg];
  const int words = (n + 31) >> 5;
  for (int i = threadIdx.x; i < words; i += 256) s_bits[i] = 0u;
  __syncthreads();
  const int* map = rowmap + (size_t)seg * n_max;
  if (keep) {
    const int64_t* kp = keep + (size_t)seg * n_max;
    const int nk = min(num_keep[seg], n);
    for (int k = threadIdx.x; k < nk; k += 256) {
      const int pos = (int)kp[k];
      if (pos < nc) {
        const int row = map[pos];
        atomicOr(&s_bits[row >> 5], 1u << (row & 31));
      }
    }
  } else {
    for (int pos = threadIdx.x; pos < nc; pos += 256) {
      const int row = map[pos];
      atomicOr(&s_bits[row >> 5], 1u << (row & 31));
    }
  }
  __syncthreads();
  // thread t owns the words [t * per, (t + 1) * per): consecutive, so the list ascends with the thread
  const int per = (words + 255) >> 8;
  const int w0 = threadIdx.x * per, w1 = min(w0 + per, words);
  int mine = 0;
  for (int w = w0; w < w1; ++w) mine += __popc(s_bits[w]);
  s_scan[threadIdx.x] = mine;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {       // inclusive Hillis-Steele scan
    const int add = (int)threadIdx.x >= off ? s_scan[threadIdx.x - off] : 0;
    __syncthreads();
    s_scan[threadIdx.x] += add;
    __syncthreads();
  }
  int at = s_scan[threadIdx.x] - mine;
  int* out = krow + (size_t)seg * n_max;
  for (int w = w0; w < w1; ++w) {
    unsigned b = s_bits[w];
    while (b) {
      out[at++] = w * 32 + (__ffs((int)b) - 1);
      b &= b - 1u;
    }
  }
  if (threadIdx.x == 255) seg_kept[seg] = s_scan[255];
}

// One workgroup per segment: the segment's detections at their place in the image's (class, row) order.  An image that
// needs no cut is written to the output at once, any other to the staging arrays the cut reads.
__global__ __launch_bounds__(256) void post_gather_kernel(const float4* __restrict__ boxes, const float* __restrict__ scores,
                                                          const int* __restrict__ krow, const int* __restrict__ seg_kept,
                                                          PostImages imgs, int num_classes, int n_max, int det_per_img,
                                                          float4* __restrict__ stage_boxes, float* __restrict__ stage_scores,
                                                          int* __restrict__ stage_labels, float4* __restrict__ out_boxes,
                                                          float* __restrict__ out_scores, int64_t* __restrict__ out_labels) {
  __shared__ int s_before, s_total;
  const int seg = blockIdx.x;
  const int fg = num_classes - 1;
  const int img = seg / fg, cls = seg % fg + 1;
  if (threadIdx.x == 0) {
    s_before = 0;
    s_total = 0;
  }
  __syncthreads();
  int before = 0, total = 0;
  for (int c = threadIdx.x; c < fg; c += 256) {
    const int k = seg_kept[img * fg + c];
    total += k;
    if (c < cls - 1) before += k;
  }
  if (total) atomicAdd(&s_total, total);
  if (before) atomicAdd(&s_before, before);
  __syncthreads();
  const int n_det = s_total;
  const size_t row0 = (size_t)imgs.row_off[img];
  const size_t base = row0 * fg + s_before;
  const bool cut = det_per_img > 0 && n_det > det_per_img;
  const int mine = seg_kept[seg];
  const int* rows = krow + (size_t)seg * n_max;
  for (int k = threadIdx.x; k < mine; k += 256) {
    const size_t g = (row0 + rows[k]) * num_classes + cls;
    if (cut) {
      stage_boxes[base + k] = boxes[g];
      stage_scores[base + k] = scores[g];
      stage_labels[base + k] = cls;
    } else {
      out_boxes[base + k] = boxes[g];
      out_scores[base + k] = scores[g];
      out_labels[base + k] = (int64_t)cls;
    }
  }
}

// One workgroup per image: the count, and where n > detections_per_img > 0 the cut.  The cut value is the
// detections_per_img-th largest score (torch.kthvalue(scores, n - k + 1), inference.py:143-147), found by an MSB-first
// radix select over the order-preserving integer image of the scores; everything >= it stays, in order.
__global__ __launch_bounds__(256) void post_cut_kernel(const int* __restrict__ seg_kept, PostImages imgs, int num_classes,
                                                       int det_per_img, const float4* __restrict__ stage_boxes,
                                                       const float* __restrict__ stage_scores,
                                                       const int* __restrict__ stage_labels, float4* __restrict__ out_boxes,
                                                       float* __restrict__ out_scores, int64_t* __restrict__ out_labels,
                                                       int* __restrict__ out_counts) {
  __shared__ int s_total;
  __shared__ int s_hist[256];
  __shared__ unsigned s_prefix;
  __shared__ int s_want;
  __shared__ int s_wave[4];
  const int img = blockIdx.x;
  const int fg = num_classes - 1;
  if (threadIdx.x == 0) s_total = 0;
  __syncthreads();
  int total = 0;
  for (int c = threadIdx.x; c < fg; c += 256) total += seg_kept[img * fg + c];
  if (total) atomicAdd(&s_total, total);
  __syncthreads();
  const int n = s_total;
  if (!(det_per_img > 0 && n > det_per_img)) {
    if (threadIdx.x == 0) out_counts[img] = n;
    return;
  }
  const size_t base = (size_t)imgs.row_off[img] * fg;
  const float* sc = stage_scores + base;
  // the key v with count(keys > v) < k <= count(keys >= v), eight bits per pass from the top
  if (threadIdx.x == 0) {
    s_prefix = 0u;
    s_want = det_per_img;
  }
  for (int shift = 24; shift >= 0; shift -= 8) {
    s_hist[threadIdx.x] = 0;
    __syncthreads();
    const unsigned prefix = s_prefix;
    const unsigned himask = shift == 24 ? 0u : (0xFFFFFFFFu << (shift + 8));
    for (int i = threadIdx.x; i < n; i += 256) {
      const unsigned key = float_orderable(sc[i]);
      if ((key & himask) == prefix) atomicAdd(&s_hist[(key >> shift) & 255u], 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int want = s_want, d = 255;
      for (; d > 0; --d) {
        if (s_hist[d] >= want) break;
        want -= s_hist[d];
      }
      s_prefix = prefix | ((unsigned)d << shift);
      s_want = want;
    }
    __syncthreads();
  }
  const unsigned cutkey = s_prefix;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int done = 0;
  for (int start = 0; start < n; start += 256) {
    const int i = start + threadIdx.x;
    const bool pass = i < n && float_orderable(sc[i]) >= cutkey;
    const unsigned long long ballot = __ballot(pass);
    if (lane == 0) s_wave[wave] = __popcll(ballot);
    __syncthreads();
    int at = done + __popcll(ballot & ((1ULL << lane) - 1ULL));
    for (int w = 0; w < wave; ++w) at += s_wave[w];
    if (pass) {
      out_boxes[base + at] = stage_boxes[base + i];
      out_scores[base + at] = sc[i];
      out_labels[base + at] = (int64_t)stage_labels[base + i];
    }
    done += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    __syncthreads();
  }
  if (threadIdx.x == 0) out_counts[img] = done;
}

struct PostLayout {
  size_t ranked_off, rowmap_off, cand_off, keep_off, numkeep_off, krow_off, segkept_off, sbox_off, sscore_off, slabel_off,
      nms_off, nms_slice, total;
  int chunk;       // segments per dadet_nms_batch call
};

static int post_layout(int batch, const int* rows_host, int num_classes, PostLayout* lay, int* n_max_out,
                       long long* total_rows_out) {
  int n_max = 0;
  long long total_rows = 0;
  for (int i = 0; i < batch; ++i) {
    if (rows_host[i] > n_max) n_max = rows_host[i];
    total_rows += rows_host[i];
  }
  *n_max_out = n_max;
  *total_rows_out = total_rows;
  const size_t S = (size_t)batch * (num_classes - 1);
  const size_t det = (size_t)total_rows * (num_classes - 1);
  auto align = [](size_t x) { return (x + 255) & ~(size_t)255; };
  size_t off = 0;
  lay->ranked_off = off;   off = align(off + sizeof(float4) * S * n_max);
  lay->rowmap_off = off;   off = align(off + sizeof(int) * S * n_max);
  lay->cand_off = off;     off = align(off + sizeof(int) * S);
  lay->keep_off = off;     off = align(off + sizeof(int64_t) * S * n_max);
  lay->numkeep_off = off;  off = align(off + sizeof(int) * S);
  lay->krow_off = off;     off = align(off + sizeof(int) * S * n_max);
  lay->segkept_off = off;  off = align(off + sizeof(int) * S);
  lay->sbox_off = off;     off = align(off + sizeof(float4) * det);
  lay->sscore_off = off;   off = align(off + sizeof(float) * det);
  lay->slabel_off = off;   off = align(off + sizeof(int) * det);
  size_t slice = 0;
  if (n_max > 0) {
    const int rc = dadet_nms_batch_workspace_bytes(1, n_max, &slice);
    if (rc != DADET_OK) return rc;
  }
  // (the IoU bit matrix of 16 384 boxes is 32 MB: many classes of very long lists go through in smaller chunks)
  size_t chunk = kPostNmsChunk;
  const size_t budget = (size_t)1 << 30;
  if (slice > 0 && chunk * slice > budget) chunk = budget / slice ? budget / slice : 1;
  if (chunk > S) chunk = S ? S : 1;
  lay->chunk = (int)chunk;
  lay->nms_slice = slice;
  lay->nms_off = off;      off = align(off + chunk * slice);
  lay->total = off;
  return DADET_OK;
}

static int post_check_shape(const int* rows_host, int batch, int num_classes, const char* who) {
  DADET_REQUIRE(batch >= 0 && batch <= kPostMaxImages, "%s: batch must be in 0..%d", who, kPostMaxImages);
  DADET_REQUIRE(num_classes >= 2, "%s: num_classes=%d needs a foreground class", who, num_classes);
  DADET_REQUIRE(batch == 0 || rows_host, "%s: rows_host is null", who);
  long long total = 0;
  for (int i = 0; i < batch; ++i) {
    DADET_REQUIRE(rows_host[i] >= 0 && rows_host[i] <= kPostMaxRows, "%s: rows[%d]=%d outside 0..%d", who, i, rows_host[i],
                  kPostMaxRows);
    total += rows_host[i];
  }
  DADET_REQUIRE(total * (long long)num_classes < (1LL << 31), "%s: %lld rows x %d classes exceed the index range", who, total,
                num_classes);
  return DADET_OK;
}

}  // namespace dadet

using namespace dadet;

extern "C" int dadet_detect_post_workspace_bytes(const int* rows_host, int batch, int num_classes, size_t* bytes_out) {
  DADET_REQUIRE(bytes_out, "detect_post_workspace_bytes: bytes_out is null");
  const int rc = post_check_shape(rows_host, batch, num_classes, "detect_post_workspace_bytes");
  if (rc != DADET_OK) return rc;
  PostLayout lay;
  int n_max;
  long long total_rows;
  const int rc2 = post_layout(batch, rows_host, num_classes, &lay, &n_max, &total_rows);
  if (rc2 != DADET_OK) return rc2;
  *bytes_out = lay.total;
  return DADET_OK;
}

extern "C" int dadet_detect_post(const float* boxes, const float* scores, const int* rows_host, int batch, int num_classes,
                                 float score_thresh, float nms_thresh, int tie_rule, int detections_per_img, int read_counts,
                                 void* workspace, size_t workspace_bytes, float* out_boxes, float* out_scores,
                                 int64_t* out_labels, int* out_counts, void* stream) {
  const int rc = post_check_shape(rows_host, batch, num_classes, "detect_post");
  if (rc != DADET_OK) return rc;
  if (batch == 0) return DADET_OK;
  DADET_REQUIRE(out_counts, "detect_post: out_counts is null");
  DADET_REQUIRE(tie_rule == 0 || tie_rule == 1, "detect_post: tie_rule must be 0 (>=) or 1 (>)");
  hipStream_t st = as_stream(stream);
  PostLayout lay;
  int n_max;
  long long total_rows;
  const int rc2 = post_layout(batch, rows_host, num_classes, &lay, &n_max, &total_rows);
  if (rc2 != DADET_OK) return rc2;
  if (n_max == 0) {
    (void)hipMemsetAsync(out_counts, 0, sizeof(int) * (size_t)batch, st);
    return check_launch("detect_post(empty)");
  }
  DADET_REQUIRE(boxes && scores && workspace && out_boxes && out_scores && out_labels, "detect_post: null pointer");
  DADET_REQUIRE(((reinterpret_cast<uintptr_t>(boxes) | reinterpret_cast<uintptr_t>(out_boxes) |
                  reinterpret_cast<uintptr_t>(workspace)) & 15) == 0,
                "detect_post: boxes, out_boxes and workspace must be 16-byte aligned");
  if (workspace_bytes < lay.total) {
    set_error("detect_post: workspace %zu < required %zu", workspace_bytes, lay.total);
    return DADET_EWORKSPACE;
  }
  PostImages imgs;
  int off = 0;
  for (int i = 0; i < kPostMaxImages; ++i) {
    imgs.rows[i] = i < batch ? rows_host[i] : 0;
    imgs.row_off[i] = off;
    off += imgs.rows[i];
  }
  const int fg = num_classes - 1;
  const int S = batch * fg;
  char* base = static_cast<char*>(workspace);
  float4* ranked = reinterpret_cast<float4*>(base + lay.ranked_off);
  int* rowmap = reinterpret_cast<int*>(base + lay.rowmap_off);
  int* cand = reinterpret_cast<int*>(base + lay.cand_off);
  int64_t* keep = reinterpret_cast<int64_t*>(base + lay.keep_off);
  int* num_keep = reinterpret_cast<int*>(base + lay.numkeep_off);
  int* krow = reinterpret_cast<int*>(base + lay.krow_off);
  int* seg_kept = reinterpret_cast<int*>(base + lay.segkept_off);
  float4* sbox = reinterpret_cast<float4*>(base + lay.sbox_off);
  float* sscore = reinterpret_cast<float*>(base + lay.sscore_off);
  int* slabel = reinterpret_cast<int*>(base + lay.slabel_off);
  const float4* boxes4 = reinterpret_cast<const float4*>(boxes);
  float4* out_boxes4 = reinterpret_cast<float4*>(out_boxes);

  // a) rank
  int p2 = 1;
  while (p2 < n_max) p2 <<= 1;
  const int threads = p2 / 2 >= 1024 ? 1024 : (p2 / 2 < 64 ? 64 : p2 / 2);
  const size_t lds = sizeof(unsigned long long) * (size_t)p2;
  if (lds > 48 * 1024)
    if (const int rc = raise_lds("detect_post", post_rank_kernel, lds); rc != DADET_OK) return rc;
  hipLaunchKernelGGL(post_rank_kernel, dim3(S), dim3(threads), lds, st, boxes4, scores, imgs, num_classes, n_max,
                     score_thresh, ranked, rowmap, cand);

  // b) suppress
  const bool suppress = nms_thresh > 0.f;            // boxlist_nms returns its input otherwise (boxlist_ops.py:24-25)
  if (suppress) {
    std::vector<int> n_seg((size_t)S);
    if (read_counts) {
      if (hipMemcpyAsync(n_seg.data(), cand, sizeof(int) * (size_t)S, hipMemcpyDeviceToHost, st) != hipSuccess ||
          hipStreamSynchronize(st) != hipSuccess)
        return check_launch("detect_post(read counts)");
      for (int s = 0; s < S; ++s)
        DADET_REQUIRE(n_seg[s] >= 0 && n_seg[s] <= rows_host[s / fg], "detect_post: candidate count %d of segment %d", n_seg[s], s);
    } else {
      for (int s = 0; s < S; ++s) n_seg[(size_t)s] = rows_host[s / fg];
    }
    for (int c0 = 0; c0 < S; c0 += lay.chunk) {
      const int m = S - c0 < lay.chunk ? S - c0 : lay.chunk;
      const int rcn = dadet_nms_batch(reinterpret_cast<const float*>(ranked + (size_t)c0 * n_max), n_seg.data() + c0, m, n_max,
                                      nms_thresh, tie_rule, -1, base + lay.nms_off, (size_t)m * lay.nms_slice,
                                      keep + (size_t)c0 * n_max, num_keep + c0, stream);
      if (rcn != DADET_OK) return rcn;
    }
  }

  // c) emit
  hipLaunchKernelGGL(post_rows_kernel, dim3(S), dim3(256), 0, st, suppress ? keep : nullptr, num_keep, rowmap, cand, imgs,
                     num_classes, n_max, krow, seg_kept);
  hipLaunchKernelGGL(post_gather_kernel, dim3(S), dim3(256), 0, st, boxes4, scores, krow, seg_kept, imgs, num_classes, n_max,
                     detections_per_img, sbox, sscore, slabel, out_boxes4, out_scores, out_labels);
  hipLaunchKernelGGL(post_cut_kernel, dim3(batch), dim3(256), 0, st, seg_kept, imgs, num_classes, detections_per_img, sbox,
                     sscore, slabel, out_boxes4, out_scores, out_labels, out_counts);
  return check_launch("detect_post");
}
