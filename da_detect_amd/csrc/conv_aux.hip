// What the convolution GEMMs need around them: the reduction passes over split partial results (weight gradient, split-K),
// the weight transposes of the data gradient, the operand maxima of contraction mode 4, the non-finite guard's host side,
// and the per-stream scratch / counter / slot tables.  Kernels, their launchers and the C entry points that only launch them.
#include <atomic>
#include <cstdlib>
#include <mutex>
#include <stdlib.h>
#include <unordered_map>
#include "conv_common.h"

namespace dadet {

__global__ void wgrad_reduce_kernel(const float4* __restrict__ part, const float* __restrict__ out_scale,
                                    float4* __restrict__ dw, int64_t total4, int K4, int splits,
                                    int accumulate) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4;
       i += (int64_t)gridDim.x * blockDim.x) {
    float4 s = part[i];
    for (int p = 1; p < splits; ++p) {
      const float4 v = part[(int64_t)p * total4 + i];
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    if (out_scale) {
      const float sc = out_scale[i / K4];
      s.x *= sc; s.y *= sc; s.z *= sc; s.w *= sc;
    }
    if (accumulate) {
      const float4 o = dw[i];
      s.x += o.x; s.y += o.y; s.z += o.z; s.w += o.w;
    }
    dw[i] = s;
  }
}

// The same reduction for up to kReduceBatch (32: a step's deferred passes go out in two launches) weight gradients in ONE launch (dadet_conv_wgrad_reduce_batch): a residual
// block's backward produces 3 - 4 split weight gradients of 0.3 - 9 MB each; one reduction pass per tensor is a
// 10 - 40 us launch that runs at ~1.5 TB/s because it is over before it fills the chip (45 launches, 1.2 ms per step).
// Block b belongs to the item whose block range contains it; within an item the arithmetic is wgrad_reduce_kernel's.
constexpr int kReduceBatch = 32;
struct ReduceItem {
  const float4* part;
  const float* out_scale;
  float4* dw;
  long long total4;
  int K4, splits, accumulate, first_block;
};
struct ReduceBatch {
  ReduceItem item[kReduceBatch];
  int n;
};

__global__ __launch_bounds__(256) void wgrad_reduce_batch_kernel(const ReduceBatch batch) {
  int k = 0;
#pragma unroll
  for (int i = 1; i < kReduceBatch; ++i)
    if (i < batch.n && (int)blockIdx.x >= batch.item[i].first_block) k = i;
  const ReduceItem& it = batch.item[k];
  const int nblocks = (k + 1 < batch.n ? batch.item[k + 1].first_block : (int)gridDim.x) - it.first_block;
  for (int64_t i = (int64_t)((int)blockIdx.x - it.first_block) * 256 + threadIdx.x; i < it.total4;
       i += (int64_t)nblocks * 256) {
    float4 s = it.part[i];
    for (int p = 1; p < it.splits; ++p) {
      const float4 v = it.part[(int64_t)p * it.total4 + i];
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    if (it.out_scale) {
      const float sc = it.out_scale[i / it.K4];
      s.x *= sc; s.y *= sc; s.z *= sc; s.w *= sc;
    }
    if (it.accumulate) {
      const float4 o = it.dw[i];
      s.x += o.x; s.y += o.y; s.z += o.z; s.w += o.w;
    }
    it.dw[i] = s;
  }
}

// wt[ci][KH-1-r][KW-1-s][co] = w[co][r][s][ci] * scale[co]
// 32x32 LDS tile transpose between the co axis and the ci axis for one (r,s) tap.
__global__ __launch_bounds__(256) void weight_transpose_kernel(const float* __restrict__ w,
                                                               const float* __restrict__ scale,
                                                               float* __restrict__ wt, int Cout, int KH,
                                                               int KW, int Cin, int CoutPad) {
  // CoutPad >= Cout: the output rows are CoutPad wide, the columns co >= Cout are zeros (a weight whose output channels the
  // forward pads to a multiple of four — the offset branch of a deformable block)
  __shared__ float tile[32][33];
  const int tap = blockIdx.z;
  const int r = tap / KW, s = tap % KW;
  const int tapT = (KH - 1 - r) * KW + (KW - 1 - s);
  const int ci0 = blockIdx.x * 32, co0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const int64_t K = (int64_t)KH * KW * Cin, Kt = (int64_t)KH * KW * CoutPad;
  for (int j = ty; j < 32; j += 8) {
    const int co = co0 + j, ci = ci0 + tx;
    float v = 0.f;
    if (co < Cout && ci < Cin) {
      v = w[(int64_t)co * K + (int64_t)tap * Cin + ci];
      if (scale) v = v * scale[co];
    }
    tile[j][tx] = v;
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    const int ci = ci0 + j, co = co0 + tx;
    if (co < CoutPad && ci < Cin) wt[(int64_t)ci * Kt + (int64_t)tapT * CoutPad + co] = tile[tx][j];
  }
}

// Every registered weight in ONE launch (dadet_conv_weight_transpose_batch): the backward pass of a step needs the
// transposed, FrozenBN-folded form of ~44 convolution weights, and producing each right in front of its data-gradient GEMM
// put 42 launches of ~5 us (plus their dispatch gaps) into the serial GEMM chain (rocprofv3 timeline of round 3: 0.22 ms
// per step with nothing else running).  The table lives in device memory; block b serves the item whose block range holds it.
struct TransposeItem {
  const float* w;
  const float* scale;
  float* wt;
  int Cout, KH, KW, Cin;
  int first_block, blocks_ci, blocks_co;
  int cout_pad;     // width of the output rows (>= Cout; 0: Cout), see weight_transpose_kernel
};

__global__ __launch_bounds__(256) void weight_transpose_batch_kernel(const TransposeItem* __restrict__ items, int n) {
  __shared__ float tile[32][33];
  __shared__ int s_item;
  if (threadIdx.x == 0) {
    int lo = 0, hi = n - 1;                 // last item whose first_block <= blockIdx.x
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (items[mid].first_block <= (int)blockIdx.x) lo = mid;
      else hi = mid - 1;
    }
    s_item = lo;
  }
  __syncthreads();
  const TransposeItem it = items[s_item];
  int b = (int)blockIdx.x - it.first_block;
  const int bx = b % it.blocks_ci;
  b /= it.blocks_ci;
  const int by = b % it.blocks_co, tap = b / it.blocks_co;
  const int r = tap / it.KW, sidx = tap % it.KW;
  const int tapT = (it.KH - 1 - r) * it.KW + (it.KW - 1 - sidx);
  const int ci0 = bx * 32, co0 = by * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const int cout_pad = it.cout_pad > it.Cout ? it.cout_pad : it.Cout;
  const int64_t K = (int64_t)it.KH * it.KW * it.Cin, Kt = (int64_t)it.KH * it.KW * cout_pad;
  for (int j = ty; j < 32; j += 8) {
    const int co = co0 + j, ci = ci0 + tx;
    float v = 0.f;
    if (co < it.Cout && ci < it.Cin) {
      v = it.w[(int64_t)co * K + (int64_t)tap * it.Cin + ci];
      if (it.scale) v = v * it.scale[co];
    }
    tile[j][tx] = v;
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    const int ci = ci0 + j, co = co0 + tx;
    if (co < cout_pad && ci < it.Cin) it.wt[(int64_t)ci * Kt + (int64_t)tapT * cout_pad + co] = tile[tx][j];
  }
}

}  // namespace dadet

using namespace dadet;

static bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the reduce pass of split-K (conv_plan.h: splitk_plan): sums the partial results in split order and applies the epilogue
__global__ void splitk_reduce_kernel(const float4* __restrict__ partial, int splits, size_t stride4,
                                     const float4* __restrict__ scale, const float4* __restrict__ bias,
                                     const float4* __restrict__ addend, const float4* __restrict__ mask,
                                     float4* __restrict__ y, int64_t total4, int C4, int relu_mode,
                                     unsigned* __restrict__ amax_y) {
  float mx = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4;
       i += (int64_t)gridDim.x * blockDim.x) {
    float4 v = partial[i];
    for (int p = 1; p < splits; ++p) {
      const float4 q = partial[(size_t)p * stride4 + i];
      v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w;
    }
    const int c = (int)(i % C4);
    if (scale) { const float4 q = scale[c]; v.x *= q.x; v.y *= q.y; v.z *= q.z; v.w *= q.w; }
    if (bias) { const float4 q = bias[c]; v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w; }
    if (addend) { const float4 q = addend[i]; v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w; }
    if (relu_mode == 1) {
      v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
    } else if (relu_mode == 2) {
      const float4 q = mask[i];
      v.x = q.x > 0.f ? v.x : 0.f; v.y = q.y > 0.f ? v.y : 0.f;
      v.z = q.z > 0.f ? v.z : 0.f; v.w = q.w > 0.f ? v.w : 0.f;
    }
    y[i] = v;
    mx = fmaxf(fmaxf(mx, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
  }
  if (amax_y) amax_publish(amax_y, mx);
}

// max|x| over a tensor, merged into *slot (mode 4: a GEMM operand whose producer left no maximum).  Bits of non-negative
// floats order like unsigned integers; amax_publish: at most one atomic per workgroup, sharded by XCD.
__global__ __launch_bounds__(256) void amax_kernel(const float* __restrict__ x, int64_t n, unsigned* __restrict__ slot) {
  float mx = 0.f;
  const int64_t n4 = n / 4;
  const float4* x4 = reinterpret_cast<const float4*>(x);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 v = x4[i];
    mx = fmaxf(fmaxf(mx, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
  }
  if (blockIdx.x == 0 && threadIdx.x < (unsigned)(n - n4 * 4)) mx = fmaxf(mx, fabsf(x[n4 * 4 + threadIdx.x]));
  amax_publish(slot, mx);
}

// the same for many tensors in one launch (the weights of a model once per optimizer step): item i owns the workgroups
// [first_block, first_block + blocks)
__global__ __launch_bounds__(256) void amax_batch_kernel(const dadet_amax_item* __restrict__ items, int n) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {          // last item whose first_block <= blockIdx.x
    const int mid = (lo + hi + 1) >> 1;
    if (items[mid].first_block <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const dadet_amax_item it = items[lo];
  const int b = (int)blockIdx.x - it.first_block;
  const float* x = reinterpret_cast<const float*>(it.x);
  const float4* x4 = reinterpret_cast<const float4*>(x);
  const int64_t n4 = it.n / 4;
  float mx = 0.f;
  // four loads in flight per lane and round (one dependent load per round ran this launch at 1.6 TB/s)
  const int64_t stride = (int64_t)it.blocks * 256;
  int64_t i = (int64_t)b * 256 + threadIdx.x;
  for (; i + 3 * stride < n4; i += 4 * stride) {
    const float4 v0 = x4[i], v1 = x4[i + stride], v2 = x4[i + 2 * stride], v3 = x4[i + 3 * stride];
    mx = fmaxf(mx, fmaxf(fmaxf(fmaxf(fabsf(v0.x), fabsf(v0.y)), fmaxf(fabsf(v0.z), fabsf(v0.w))),
                         fmaxf(fmaxf(fabsf(v1.x), fabsf(v1.y)), fmaxf(fabsf(v1.z), fabsf(v1.w)))));
    mx = fmaxf(mx, fmaxf(fmaxf(fmaxf(fabsf(v2.x), fabsf(v2.y)), fmaxf(fabsf(v2.z), fabsf(v2.w))),
                         fmaxf(fmaxf(fabsf(v3.x), fabsf(v3.y)), fmaxf(fabsf(v3.z), fabsf(v3.w)))));
  }
  for (; i < n4; i += stride) {
    const float4 v = x4[i];
    mx = fmaxf(fmaxf(mx, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
  }
  if (b == 0 && threadIdx.x < (unsigned)(it.n - n4 * 4)) mx = fmaxf(mx, fabsf(x[n4 * 4 + threadIdx.x]));
  amax_publish(reinterpret_cast<unsigned*>(it.slot), mx);
}

// ---- non-finite guard: device words + a ring of recent launch records (conv_common.h: nf_check) -------------------------
__device__ unsigned g_nf_words[2];
__device__ unsigned g_nf_taken[2];
// read-and-clear in one atomic step per word: a record set while the host polls is either in this poll or in the next
__global__ void nf_take_kernel() {
  g_nf_taken[1] = atomicExch(&g_nf_words[1], 0u);
  g_nf_taken[0] = atomicExch(&g_nf_words[0], 0u);
}
namespace {
struct NfRecord { unsigned id; char kind[24]; int M, N, K, KH; };
constexpr int kNfRing = 8192;
NfRecord g_nf_ring[kNfRing];
std::atomic<unsigned> g_nf_next{0};
}  // namespace
namespace dadet {
unsigned nf_next_launch(const char* kind, int M, int N, int K, int KH) {
  const unsigned id = g_nf_next.fetch_add(1);
  NfRecord& r = g_nf_ring[id % kNfRing];
  r.id = id;
  snprintf(r.kind, sizeof(r.kind), "%s", kind);
  r.M = M; r.N = N; r.K = K; r.KH = KH;
  return id;
}
unsigned* nf_flag_ptr() {
  static unsigned* p = [] {
    void* q = nullptr;
    return hipGetSymbolAddress(&q, HIP_SYMBOL(g_nf_words)) == hipSuccess ? static_cast<unsigned*>(q) : nullptr;
  }();
  static const bool off = getenv("DADET_NONFINITE_GUARD") && getenv("DADET_NONFINITE_GUARD")[0] == '0';
  return off ? nullptr : p;
}

// ---- per-stream tables ----------------------------------------------------------------------------------------------
namespace {
struct Scratch { void* p = nullptr; size_t bytes = 0; };
std::mutex g_scratch_mutex;
std::unordered_map<hipStream_t, Scratch> g_scratch;
}  // namespace

// scratch of `bytes` for work queued on `st`; contents are only valid in stream order
void* stream_scratch(hipStream_t st, size_t bytes) {
  std::lock_guard<std::mutex> lock(g_scratch_mutex);
  Scratch& s = g_scratch[st];
  if (s.bytes < bytes) {
    if (s.p) {
      (void)hipStreamSynchronize(st);   // the old buffer may still be read by queued work
      (void)hipFree(s.p);
      s.p = nullptr;
      s.bytes = 0;
    }
    const size_t want = bytes < (size_t)(8u << 20) ? (size_t)(8u << 20) : bytes * 2;
    if (hipMalloc(&s.p, want) != hipSuccess) {
      s.p = nullptr;
      return nullptr;
    }
    s.bytes = want;
  }
  return s.p;
}

// arrival counters of the stream-K tail: one persistent zero-initialised buffer per stream (work queued on a stream is
// ordered, so one launch owns it at a time); the workgroup that completes a tile resets that tile's counter
constexpr int kSkCounters = plan::kSkCounters;
int* stream_counters(hipStream_t st) {
  static std::mutex m;
  static std::unordered_map<hipStream_t, int*> table;
  std::lock_guard<std::mutex> lock(m);
  int*& p = table[st];
  if (!p) {
    if (hipMalloc(reinterpret_cast<void**>(&p), sizeof(int) * kSkCounters) != hipSuccess) {
      p = nullptr;
      return nullptr;
    }
    if (hipMemset(p, 0, sizeof(int) * kSkCounters) != hipSuccess) return nullptr;
  }
  return p;
}

// mode 4 through the plain entry points (no maxima handed in): two slots per stream that the library fills itself
unsigned* stream_amax_slots(hipStream_t st) {
  static std::mutex m;
  static std::unordered_map<hipStream_t, unsigned*> table;
  std::lock_guard<std::mutex> lock(m);
  unsigned*& p = table[st];
  if (!p && hipMalloc(reinterpret_cast<void**>(&p), sizeof(unsigned) * (7 * (size_t)kAmaxStride + 4)) != hipSuccess)
    p = nullptr;
  return p;
}
// zero the eight shards of `n` adjacent slots
hipError_t zero_slots(unsigned* first, int n, hipStream_t st) {
  return hipMemset2DAsync(first, sizeof(unsigned) * kAmaxStride, 0, sizeof(unsigned) * n, 8, st);
}

int launch_amax(const float* x, int64_t n, unsigned* slot, hipStream_t st) {
  int64_t blocks = ceil_div64(n / 4 > 0 ? n / 4 : 1, 256 * 4);
  if (blocks > kMaxStreamBlocks) blocks = kMaxStreamBlocks;
  hipLaunchKernelGGL(amax_kernel, dim3((int)blocks), dim3(256), 0, st, x, n, slot);
  return check_launch("amax");
}

int launch_splitk_reduce(const float* partial, int splits, const ConvArgs& a, hipStream_t st) {
  const size_t per = (size_t)a.M * a.Cout;
  const int64_t total4 = (int64_t)per / 4;
  int64_t blocks = ceil_div64(total4, 256);
  if (blocks > kMaxStreamBlocks) blocks = kMaxStreamBlocks;
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3((int)blocks), dim3(256), 0, st,
                     reinterpret_cast<const float4*>(partial), splits, per / 4,
                     reinterpret_cast<const float4*>(a.scale), reinterpret_cast<const float4*>(a.bias),
                     reinterpret_cast<const float4*>(a.addend), reinterpret_cast<const float4*>(a.mask_ref),
                     reinterpret_cast<float4*>(a.y), total4, a.Cout / 4, a.relu_mode, a.amax_y);
  return check_launch("conv_forward(split-K reduce)");
}

int launch_wgrad_reduce(const float* partials, const float* out_scale, float* dw, int Cout, int K, int splits,
                        int accumulate, hipStream_t st) {
  const int64_t total4 = (int64_t)Cout * K / 4;
  int64_t blocks = ceil_div64(total4, 256);
  if (blocks > kMaxStreamBlocks) blocks = kMaxStreamBlocks;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((int)blocks), dim3(256), 0, st,
                     reinterpret_cast<const float4*>(partials), out_scale, reinterpret_cast<float4*>(dw),
                     total4, K / 4, splits, accumulate);
  return check_launch("conv_wgrad(reduce)");
}
}  // namespace dadet

extern "C" int dadet_amax(const float* x, long long n, float* slot, void* stream) {
  DADET_REQUIRE(n >= 0 && slot && (n == 0 || (x && al16(x))), "amax: bad arguments");
  if (n == 0) return DADET_OK;
  return launch_amax(x, n, reinterpret_cast<unsigned*>(slot), as_stream(stream));
}

extern "C" int dadet_amax_batch(const dadet_amax_item* items_dev, int n, int total_blocks, void* stream) {
  DADET_REQUIRE(n >= 0 && (n == 0 || (items_dev && total_blocks > 0)), "amax_batch: bad arguments");
  if (n == 0) return DADET_OK;
  hipLaunchKernelGGL(amax_batch_kernel, dim3(total_blocks), dim3(256), 0, as_stream(stream), items_dev, n);
  return check_launch("amax_batch");
}

extern "C" int dadet_nonfinite_poll(char* msg, int cap) {
  unsigned w[2] = {0, 0};
  unsigned* dev = nf_flag_ptr();
  if (!dev) { if (msg && cap > 0) msg[0] = 0; return 0; }
  // every stream of the process first (PyTorch's side streams and the weight-gradient lane are non-blocking: the null
  // stream does not order against them), then one exchange kernel, then its two words
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  hipLaunchKernelGGL(nf_take_kernel, dim3(1), dim3(1), 0, 0);
  if (hipMemcpyFromSymbol(w, HIP_SYMBOL(g_nf_taken), sizeof(w), 0, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  if (w[1] == 0) { if (msg && cap > 0) msg[0] = 0; return 0; }
  if (msg && cap > 0) {
    const unsigned id = w[0] - 1u;
    const NfRecord& r = g_nf_ring[id % kNfRing];
    if (w[0] != 0 && r.id == id)
      snprintf(msg, cap, "%s launch #%u (M=%d N=%d K=%d, %dx%d taps): non-finite sums in %u wavefront(s) — an operand's "
               "largest-magnitude slot below its data overflows the fp16 split (contraction mode 4)", r.kind, id, r.M, r.N,
               r.K, r.KH, r.KH, w[1]);
    else
      snprintf(msg, cap, "GEMM launch #%u: non-finite sums in %u wavefront(s) (launch record no longer in the ring)", id, w[1]);
  }
  return (int)w[1];
}

extern "C" int dadet_conv_wgrad_reduce_batch(const dadet_wgrad_pending* items, int n, void* stream) {
  DADET_REQUIRE(n >= 0 && (n == 0 || items), "conv_wgrad_reduce_batch: bad arguments");
  hipStream_t st = as_stream(stream);
  for (int base = 0; base < n; base += kReduceBatch) {
    ReduceBatch b;
    b.n = 0;
    int blocks_total = 0;
    for (int i = base; i < n && b.n < kReduceBatch; ++i) {
      const dadet_wgrad_pending& p = items[i];
      if (p.splits <= 1) continue;       // nothing pending for this one (splits == 1 wrote dw itself)
      DADET_REQUIRE(p.partials && p.dw && p.count > 0 && p.count % 4 == 0 && p.K > 0 && p.K % 4 == 0,
                    "conv_wgrad_reduce_batch: item %d is malformed", i);
      ReduceItem& it = b.item[b.n++];
      it.part = reinterpret_cast<const float4*>(p.partials);
      it.out_scale = p.out_scale;
      it.dw = reinterpret_cast<float4*>(p.dw);
      it.total4 = p.count / 4;
      it.K4 = p.K / 4;
      it.splits = p.splits;
      it.accumulate = p.accumulate;
      it.first_block = blocks_total;
      int64_t blocks = ceil_div64(it.total4, 256);
      if (blocks > kMaxStreamBlocks) blocks = kMaxStreamBlocks;
      blocks_total += (int)blocks;
    }
    if (b.n == 0) continue;
    hipLaunchKernelGGL(wgrad_reduce_batch_kernel, dim3(blocks_total), dim3(256), 0, st, b);
    int rc = check_launch("conv_wgrad_reduce_batch");
    if (rc) return rc;
  }
  return DADET_OK;
}

static int weight_transpose_impl(const float* w, const float* scale, float* wt, int Cout, int KH, int KW, int Cin,
                                 int cout_pad, void* stream) {
  DADET_REQUIRE(w && wt && Cout > 0 && KH > 0 && KW > 0 && Cin > 0, "conv_weight_transpose: bad args");
  DADET_REQUIRE(KH * KW <= 65535, "conv_weight_transpose: kernel too large");
  DADET_REQUIRE(cout_pad >= Cout, "conv_weight_transpose: cout_pad=%d < Cout=%d", cout_pad, Cout);
  hipLaunchKernelGGL(weight_transpose_kernel, dim3(ceil_div(Cin, 32), ceil_div(cout_pad, 32), KH * KW),
                     dim3(256), 0, as_stream(stream), w, scale, wt, Cout, KH, KW, Cin, cout_pad);
  return check_launch("conv_weight_transpose");
}

extern "C" int dadet_conv_weight_transpose(const float* w, const float* scale, float* wt, int Cout, int KH,
                                           int KW, int Cin, void* stream) {
  return weight_transpose_impl(w, scale, wt, Cout, KH, KW, Cin, Cout, stream);
}

extern "C" int dadet_conv_weight_transpose_padded(const float* w, const float* scale, float* wt, int Cout, int KH,
                                                  int KW, int Cin, int cout_pad, void* stream) {
  return weight_transpose_impl(w, scale, wt, Cout, KH, KW, Cin, cout_pad, stream);
}

extern "C" int dadet_conv_weight_transpose_batch(const dadet_transpose_item* items_dev, int n, int total_blocks,
                                                 void* stream) {
  static_assert(sizeof(dadet_transpose_item) == sizeof(dadet::TransposeItem), "transpose item layout");
  DADET_REQUIRE(n >= 0 && total_blocks >= 0, "conv_weight_transpose_batch: bad args");
  if (n == 0 || total_blocks == 0) return DADET_OK;
  DADET_REQUIRE(items_dev, "conv_weight_transpose_batch: null table");
  hipLaunchKernelGGL(weight_transpose_batch_kernel, dim3(total_blocks), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<const dadet::TransposeItem*>(items_dev), n);
  return check_launch("conv_weight_transpose_batch");
}
