// Dispatch of the convolution GEMMs (forward / data gradient, weight gradient, grouped weight gradient) and their C entry
// points.  Host code only: a call validates its arguments, asks conv_plan.h for the plan, fills the kernel's argument
// struct from the descriptor and the plan, takes the scratch the plan asks for and calls the launcher of the plan's kernel
// family (conv_common.h).  The query entry points hand out views of the same plans.
#include "conv_common.h"

namespace dadet {

// contraction mode (dadet_set_gemm_mode) and large-tile mode (dadet_set_big_gemm; DADET_BIG_GEMM sets the start-up value)
static int g_gemm_mode = 4;
static int g_big_mode = plan::big_gemm_default();
int gemm_mode() { return g_gemm_mode; }

static int conv_desc_check(const dadet_conv_desc* d, const char* who) {
  DADET_REQUIRE(d, "%s: null descriptor", who);
  DADET_REQUIRE(d->N >= 0 && d->H > 0 && d->W > 0 && d->Cin > 0 && d->Cout > 0 && d->KH > 0 && d->KW > 0 &&
                    d->stride > 0 && d->pad >= 0 && d->Ho > 0 && d->Wo > 0,
                "%s: bad dims", who);
  DADET_REQUIRE(d->Cin % 4 == 0, "%s: Cin=%d must be a multiple of 4 (pad the channel axis)", who, d->Cin);
  DADET_REQUIRE((int64_t)d->N * d->H * d->W * d->Cin < (1LL << 31) &&
                    (int64_t)d->N * d->Ho * d->Wo < (1LL << 31),
                "%s: tensor too large for 32-bit pixel indexing", who);
  return DADET_OK;
}

// one buffer descriptor addresses less than 4 GB
static int extents_check(uint64_t a, uint64_t b, uint64_t c, const char* who) {
  DADET_REQUIRE(a < 0xFFFFFFF0ull && b < 0xFFFFFFF0ull && c < 0xFFFFFFF0ull,
                "%s: tensors of 4 GB or more are not addressable through one buffer descriptor", who);
  return DADET_OK;
}

static bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// descriptor + plan -> kernel arguments (pointers, maxima and the guard are the caller's)
static void fill_conv_args(const dadet_conv_desc* d, const plan::Gemm& g, const plan::FwdPlan& p, ConvArgs* a) {
  *a = ConvArgs();
  a->N = d->N; a->H = d->H; a->W = d->W; a->Cin = d->Cin; a->Cout = d->Cout; a->KH = d->KH; a->KW = d->KW;
  a->stride = d->stride; a->pad = d->pad; a->Ho = d->Ho; a->Wo = d->Wo; a->OutH = d->OutH; a->OutW = d->OutW;
  a->os = g.os; a->relu_mode = d->relu_mode;
  a->M = g.M; a->K = g.K;
  a->x_bytes = (unsigned)g.x_bytes; a->w_bytes = (unsigned)g.w_bytes; a->y_bytes = (unsigned)g.y_bytes;
  a->ablate = plan::ablate();
  a->epi_v4 = p.epi_v4;
  a->tiles_m = p.tiles_m; a->tiles_n = p.tiles_n;
  a->sk_dp_tiles = p.sk.dp_tiles; a->sk_tiles = p.sk.sk_tiles; a->sk_units = p.sk.units; a->sk_iters = p.sk.iters;
  a->sk_max_parts = p.sk.max_parts;
  a->big_splits = p.big_splits; a->big_body = p.big_body;
}

// descriptor + the plan's tiles_co / tiles_kc / splits / rows_per_split -> kernel arguments (pointers, maxima, the guard and
// direct / out are the caller's)
static void fill_wgrad_args(const dadet_conv_desc* d, int gy_ld, int tiles_co, int tiles_kc, int splits, int rows,
                            WgradArgs* a) {
  *a = WgradArgs();
  const plan::Gemm g = plan::gemm_of(d);
  a->gy_ld = gy_ld;
  a->N = d->N; a->H = d->H; a->W = d->W; a->Cin = d->Cin; a->Cout = d->Cout; a->KH = d->KH; a->KW = d->KW;
  a->stride = d->stride; a->pad = d->pad; a->Ho = d->Ho; a->Wo = d->Wo;
  a->M = g.M; a->K = g.K;
  a->x_bytes = (unsigned)g.x_bytes; a->gy_bytes = (unsigned)((uint64_t)g.M * gy_ld * 4);
  a->tiles_co = tiles_co; a->tiles_kc = tiles_kc; a->splits = splits; a->rows_per_split = rows;
}

static void fill_pending(dadet_wgrad_pending* p, const void* workspace, const float* out_scale, float* dw, int Cout, int K,
                         int splits, int accumulate) {
  p->partials = static_cast<const float*>(workspace);
  p->out_scale = out_scale;
  p->dw = dw;
  p->count = (long long)Cout * K;
  p->K = K;
  p->splits = splits;
  p->accumulate = accumulate;
}

static int conv_forward_impl(const dadet_conv_desc* d, const float* x, const float* w,
                             const float* scale, const float* bias, const float* addend,
                             const float* mask_ref, float* y, const float* amax_x, const float* amax_w,
                             float* amax_y, void* stream) {
  int rc = conv_desc_check(d, "conv_forward");
  if (rc) return rc;
  if (d->N == 0) return DADET_OK;
  DADET_REQUIRE(x && w && y && al16(x) && al16(w), "conv_forward: x / w must be non-null and 16-byte aligned");
  DADET_REQUIRE(d->relu_mode >= 0 && d->relu_mode <= 2, "conv_forward: relu_mode");
  DADET_REQUIRE(d->relu_mode != 2 || mask_ref, "conv_forward: relu_mode 2 needs mask_ref");
  const plan::Gemm g = plan::gemm_of(d);
  DADET_REQUIRE(g.os == 1 ? (d->OutH == d->Ho && d->OutW == d->Wo)
                          : ((d->Ho - 1) * g.os < d->OutH && (d->Wo - 1) * g.os < d->OutW),
                "conv_forward: OutH/OutW inconsistent with Ho/Wo and out_spatial_stride");
  rc = extents_check(g.x_bytes, g.w_bytes, g.y_bytes, "conv_forward");
  if (rc) return rc;
  const int mode = g_gemm_mode;
  const bool aligned16 = al16(y) && (!addend || al16(addend)) && (!mask_ref || al16(mask_ref)) && (!scale || al16(scale)) &&
                         (!bias || al16(bias));
  const plan::FwdPlan p = plan::plan_forward(d, aligned16, mode, g_big_mode);
  ConvArgs a;
  fill_conv_args(d, g, p, &a);
  a.x = x; a.w = w; a.scale = scale; a.bias = bias; a.addend = addend; a.mask_ref = mask_ref; a.y = y;
  hipStream_t st = as_stream(stream);
  if (mode == 4) {
    // operand maxima: the caller's slots, or (plain entry point) two per-stream slots filled here
    if (!amax_x || !amax_w) {
      unsigned* own = stream_amax_slots(st);
      if (!own) { set_error("conv_forward: could not allocate the operand-maximum slots"); return DADET_ELAUNCH; }
      if (zero_slots(own, 2, st) != hipSuccess) return check_launch("conv_forward(amax memset)");
      if (!amax_x) {
        rc = launch_amax(x, (int64_t)(g.x_bytes / 4), own, st);
        if (rc) return rc;
        amax_x = reinterpret_cast<const float*>(own);
      }
      if (!amax_w) {
        rc = launch_amax(w, (int64_t)(g.w_bytes / 4), own + 1, st);
        if (rc) return rc;
        amax_w = reinterpret_cast<const float*>(own + 1);
      }
    }
    a.amax_x = amax_x; a.amax_w = amax_w;
    a.amax_y = reinterpret_cast<unsigned*>(amax_y);
    a.nf_flag = nf_flag_ptr();
    a.launch_id = a.nf_flag ? nf_next_launch("conv_forward", a.M, a.Cout, a.K, a.KH) : 0;
  }   // (the other modes neither read nor leave maxima)
  // per-stream scratch (reused in stream order) and arrival counters, where the plan wants them
  float* ws = p.workspace_bytes ? static_cast<float*>(stream_scratch(st, p.workspace_bytes)) : nullptr;
  int* counters = p.counters ? stream_counters(st) : nullptr;
  if ((p.workspace_bytes && !ws) || (p.counters && !counters)) {
    set_error("conv_forward: could not allocate %zu bytes of %s scratch", p.workspace_bytes,
              p.family == plan::kFwdSplitSk ? "stream-K" : p.family == plan::kFwdSplitK ? "split-K" : "split-reduction");
    return DADET_ELAUNCH;
  }
  switch (p.family) {
    case plan::kFwdWs: return launch_fwd_ws(a, p, mode, st);
    case plan::kFwdBig256:
    case plan::kFwdBig128:
      a.sk_ws = ws;
      a.sk_counters = counters;
      return launch_fwd_big(a, p, st);
    case plan::kFwdSplitSk:
      a.sk_ws = ws;
      a.sk_counters = counters;
      return launch_fwd_split_sk(a, mode, st);
    case plan::kFwdSplitK: {
      ConvArgs part = a;
      part.scale = part.bias = part.addend = part.mask_ref = nullptr;
      part.amax_y = nullptr;          // the reduce pass sees the final values
      part.relu_mode = 0;
      part.y = ws;
      part.ksplit = p.ksplit;
      part.split_stride = (unsigned)((size_t)a.M * a.Cout);
      rc = launch_fwd_split(part, p, mode, st);
      return rc ? rc : launch_splitk_reduce(ws, p.splits, a, st);
    }
    case plan::kFwdSplit: return launch_fwd_split(a, p, mode, st);
    default: return launch_fwd_exact(a, p, st);
  }
}

// Weight gradient.  (measured and removed, round 2: the last-arriving split of a tile summing the partials inside the GEMM
// kernel — 32.1 ms against 28.8 ms per step: every one of the ~800 workgroups of a launch had to publish its 64 KB tile
// write-through, where the separate pass reads partials that mostly still sit in L2 / MALL)
static int conv_wgrad_impl(const dadet_conv_desc* d, const float* x, const float* gy, const float* out_scale, float* dw,
                           int accumulate, void* workspace, size_t workspace_bytes, dadet_wgrad_pending* pending,
                           void* stream, int gy_ld = 0, const float* amax_x = nullptr, const float* amax_gy = nullptr) {
  if (pending) pending->splits = 0;
  int rc = conv_desc_check(d, "conv_wgrad");
  if (rc) return rc;
  DADET_REQUIRE(dw, "conv_wgrad: null dw");
  hipStream_t st = as_stream(stream);
  const int K = d->KH * d->KW * d->Cin;
  if (d->N == 0) {
    if (!accumulate) (void)hipMemsetAsync(dw, 0, sizeof(float) * (size_t)d->Cout * K, st);
    return check_launch("conv_wgrad(empty)");
  }
  DADET_REQUIRE(x && gy && al16(x) && al16(gy) && al16(dw), "conv_wgrad: pointers must be 16-byte aligned");
  // gy_ld: rows of gy padded to a multiple of four channels (the offset branch of a deformable block: 18 / 27 channels in
  // rows of 20 / 28) — the padding columns are read with the last channel quad and never stored
  if (gy_ld == 0) gy_ld = d->Cout;
  DADET_REQUIRE(gy_ld % 4 == 0 && gy_ld >= d->Cout && gy_ld - d->Cout < 4,
                "conv_wgrad: gy rows of %d floats for Cout=%d (need a multiple of 4, less than 4 above Cout)", gy_ld, d->Cout);
  DADET_REQUIRE(K % 4 == 0, "conv_wgrad: KH*KW*Cin=%d must be a multiple of 4", K);
  const plan::Gemm g = plan::gemm_of(d);
  const uint64_t gb = (uint64_t)g.M * gy_ld * 4;
  rc = extents_check(g.x_bytes, gb, 0, "conv_wgrad");
  if (rc) return rc;
  const int mode = g_gemm_mode;
  const plan::WgradPlan p = plan::plan_wgrad(d, gy_ld, mode, g_big_mode);
  WgradArgs a;
  fill_wgrad_args(d, gy_ld, p.tiles_co, p.tiles_kc, p.splits, p.rows_per_split, &a);
  a.x = x; a.gy = gy; a.out_scale = out_scale;
  a.accumulate = accumulate;
  if (mode == 4) {
    if (!amax_x || !amax_gy) {
      unsigned* own = stream_amax_slots(st);
      if (!own) { set_error("conv_wgrad: could not allocate the operand-maximum slots"); return DADET_ELAUNCH; }
      if (zero_slots(own + 2, 2, st) != hipSuccess) return check_launch("conv_wgrad(amax memset)");
      if (!amax_x) {
        rc = launch_amax(x, (int64_t)(g.x_bytes / 4), own + 2, st);
        if (rc) return rc;
        amax_x = reinterpret_cast<const float*>(own + 2);
      }
      if (!amax_gy) {
        rc = launch_amax(gy, (int64_t)(gb / 4), own + 3, st);
        if (rc) return rc;
        amax_gy = reinterpret_cast<const float*>(own + 3);
      }
    }
    a.amax_x = amax_x; a.amax_gy = amax_gy;
    a.nf_flag = nf_flag_ptr();
    a.launch_id = a.nf_flag ? nf_next_launch("conv_wgrad", a.M, a.Cout, a.K, a.KH) : 0;
  }
  if (p.splits == 1) {
    a.direct = 1;
    a.out = dw;
  } else {
    if (!workspace || workspace_bytes < p.workspace_bytes) {
      set_error("conv_wgrad: workspace %zu < required %zu", workspace_bytes, p.workspace_bytes);
      return DADET_EWORKSPACE;
    }
    a.direct = 0;
    a.out = static_cast<float*>(workspace);
  }
  switch (p.family) {
    case plan::kWgradBig: rc = launch_wgrad_big(a, st); break;
    case plan::kWgradExact: rc = launch_wgrad_exact(a, st); break;
    default: rc = launch_wgrad_split(a, p.family == plan::kWgradSplitSmallMap, mode, st);
  }
  if (rc || p.splits == 1) return rc;
  if (pending) {      // the caller batches the reduction passes
    fill_pending(pending, workspace, out_scale, dw, d->Cout, K, p.splits, accumulate);
    return DADET_OK;
  }
  return launch_wgrad_reduce(static_cast<const float*>(workspace), out_scale, dw, d->Cout, K, p.splits, accumulate, st);
}

// the descriptors of a group are valid and non-empty (what plan_wgrad_group takes for granted)
static bool group_descs_ok(const dadet_conv_desc* descs, int n) {
  if (n < 1 || n > kWgradGroupMax) return false;
  for (int i = 0; i < n; ++i)
    if (conv_desc_check(&descs[i], "conv_wgrad_group") || descs[i].N == 0) return false;
  return true;
}

}  // namespace dadet

using namespace dadet;

// 4 = 2-term fp16 split under per-tensor power-of-two scales (3 MFMAs / K=16, fp32-class accuracy); 3 = 3-term bf16 split
// (6 MFMAs / K=16, fp32-class accuracy, no scales); 0 = exact fp32 MFMA; 2 = 2-term bf16 split (3 MFMAs / K=16, ~2^-16)
extern "C" int dadet_set_gemm_mode(int mode) {
  if (mode != 0 && mode != 2 && mode != 3 && mode != 4) {
    set_error("set_gemm_mode: mode must be 0, 2, 3 or 4");
    return DADET_EINVAL;
  }
  g_gemm_mode = mode;
  return DADET_OK;
}
extern "C" int dadet_get_gemm_mode(void) { return g_gemm_mode; }

// 0: never, 1: where the plan expects a gain, 2: wherever the large-tile kernels are applicable (tests)
extern "C" int dadet_set_big_gemm(int mode) {
  if (mode < 0 || mode > 2) {
    set_error("set_big_gemm: mode must be 0 (off), 1 (planned) or 2 (wherever applicable)");
    return DADET_EINVAL;
  }
  g_big_mode = mode;
  return DADET_OK;
}
extern "C" int dadet_get_big_gemm(void) { return g_big_mode; }

extern "C" int dadet_conv_forward(const dadet_conv_desc* d, const float* x, const float* w,
                                  const float* scale, const float* bias, const float* addend,
                                  const float* mask_ref, float* y, void* stream) {
  return conv_forward_impl(d, x, w, scale, bias, addend, mask_ref, y, nullptr, nullptr, nullptr, stream);
}

extern "C" int dadet_conv_forward_scaled(const dadet_conv_desc* d, const float* x, const float* w,
                                         const float* scale, const float* bias, const float* addend,
                                         const float* mask_ref, float* y, const float* amax_x, const float* amax_w,
                                         float* amax_y, void* stream) {
  return conv_forward_impl(d, x, w, scale, bias, addend, mask_ref, y, amax_x, amax_w, amax_y, stream);
}

// ---- queries: views of the plan -----------------------------------------------------------------------------------------
extern "C" int dadet_conv_forward_plan(const dadet_conv_desc* d, dadet_conv_plan_info* out) {
  int rc = conv_desc_check(d, "conv_forward_plan");
  if (rc) return rc;
  DADET_REQUIRE(out, "conv_forward_plan: null out");
  const plan::Gemm g = plan::gemm_of(d);
  rc = extents_check(g.x_bytes, g.w_bytes, g.y_bytes, "conv_forward_plan");
  if (rc) return rc;
  const plan::FwdPlan p = plan::plan_forward(d, true, g_gemm_mode, g_big_mode);
  plan::fill_info(p, out);
  // variant and name are the label dadet_conv_forward_variant stands for: it has always assumed the 16-byte epilogue, also
  // under DADET_EPILOGUE_V4=0 (where the launch, and the other fields, fall back to the tiled kernels)
  if (!p.epi_v4 && g.os == 1 && d->Cout % 4 == 0) {
    const plan::FwdPlan label = plan::plan_forward_epi(d, true, true, g_gemm_mode, g_big_mode);
    out->variant = label.variant;
    snprintf(out->name, sizeof(out->name), "%s", label.name);
  }
  return DADET_OK;
}

extern "C" int dadet_conv_forward_variant(const dadet_conv_desc* d) {
  if (!d) return -1;
  const int os = d->out_spatial_stride > 0 ? d->out_spatial_stride : 1;
  // (assuming 16-byte aligned tensors, as torch allocates them, and the 16-byte epilogue)
  return plan::fwd_label(d, plan::gemm_of(d), os == 1 && d->Cout % 4 == 0, g_gemm_mode, g_big_mode);
}

extern "C" int dadet_conv_wgrad_plan(const dadet_conv_desc* d, int gy_ld, dadet_conv_plan_info* out) {
  int rc = conv_desc_check(d, "conv_wgrad_plan");
  if (rc) return rc;
  DADET_REQUIRE(out, "conv_wgrad_plan: null out");
  plan::fill_info(plan::plan_wgrad(d, gy_ld ? gy_ld : d->Cout, g_gemm_mode, g_big_mode), out);
  return DADET_OK;
}

extern "C" int dadet_conv_wgrad_variant(const dadet_conv_desc* d) {
  if (!d) return -1;
  return plan::plan_wgrad(d, d->Cout, g_gemm_mode, g_big_mode).family == plan::kWgradBig ? 1 : 0;
}

extern "C" int dadet_conv_wgrad_workspace_bytes(const dadet_conv_desc* d, size_t* bytes_out) {
  int rc = conv_desc_check(d, "conv_wgrad_workspace_bytes");
  if (rc) return rc;
  DADET_REQUIRE(bytes_out, "conv_wgrad_workspace_bytes: null out");
  if (d->N == 0) { *bytes_out = 0; return DADET_OK; }
  // The query does not know gy's row pitch: the plan for dense rows and the one for padded rows (which never takes the
  // 256 x 256 kernel), and the LARGER need of the two, so that whichever kernel runs finds its space
  const plan::WgradPlan dense = plan::plan_wgrad(d, d->Cout, g_gemm_mode, g_big_mode);
  *bytes_out = dense.workspace_bytes;
  if (dense.family == plan::kWgradBig) {      // (otherwise the dense plan is the padded one)
    const size_t padded = plan::plan_wgrad(d, d->Cout + 4, g_gemm_mode, g_big_mode).workspace_bytes;
    if (padded > *bytes_out) *bytes_out = padded;
  }
  return DADET_OK;
}

extern "C" int dadet_conv_wgrad(const dadet_conv_desc* d, const float* x, const float* gy,
                                const float* out_scale, float* dw, int accumulate, void* workspace,
                                size_t workspace_bytes, void* stream) {
  return conv_wgrad_impl(d, x, gy, out_scale, dw, accumulate, workspace, workspace_bytes, nullptr, stream);
}

extern "C" int dadet_conv_wgrad_partials(const dadet_conv_desc* d, const float* x, const float* gy,
                                         const float* out_scale, float* dw, int accumulate, void* workspace,
                                         size_t workspace_bytes, dadet_wgrad_pending* pending_out, void* stream) {
  DADET_REQUIRE(pending_out, "conv_wgrad_partials: null pending_out");
  return conv_wgrad_impl(d, x, gy, out_scale, dw, accumulate, workspace, workspace_bytes, pending_out, stream);
}

extern "C" int dadet_conv_wgrad_partials_ld(const dadet_conv_desc* d, const float* x, const float* gy, int gy_ld,
                                            const float* out_scale, float* dw, int accumulate, void* workspace,
                                            size_t workspace_bytes, dadet_wgrad_pending* pending_out, void* stream) {
  DADET_REQUIRE(pending_out, "conv_wgrad_partials_ld: null pending_out");
  return conv_wgrad_impl(d, x, gy, out_scale, dw, accumulate, workspace, workspace_bytes, pending_out, stream, gy_ld);
}

extern "C" int dadet_conv_wgrad_scaled(const dadet_conv_desc* d, const float* x, const float* gy, int gy_ld,
                                       const float* out_scale, float* dw, int accumulate, void* workspace,
                                       size_t workspace_bytes, dadet_wgrad_pending* pending_out, const float* amax_x,
                                       const float* amax_gy, void* stream) {
  return conv_wgrad_impl(d, x, gy, out_scale, dw, accumulate, workspace, workspace_bytes, pending_out, stream, gy_ld,
                         amax_x, amax_gy);
}

// ---- several weight gradients in one launch (conv_big.hip: conv_wgrad_big_group_kernel; conv_split.hip: its 128 x 128 form)
extern "C" int dadet_conv_wgrad_group_plan(const dadet_conv_desc* descs, int n, int* splits_out, size_t* workspace_bytes_out) {
  DADET_REQUIRE(descs && n >= 1 && splits_out && workspace_bytes_out, "conv_wgrad_group_plan: bad arguments");
  if (!group_descs_ok(descs, n)) return 0;
  const plan::WgradGroupPlan p = plan::plan_wgrad_group(descs, n, g_gemm_mode, g_big_mode);
  for (int i = 0; i < n && p.kind; ++i) {
    splits_out[i] = p.splits[i];
    workspace_bytes_out[i] = p.workspace_bytes[i];
  }
  return p.kind;
}

extern "C" int dadet_conv_wgrad_group(const dadet_conv_desc* descs, int n, const float* const* x, const float* const* gy,
                                      const float* const* out_scale, float* const* dw, const int* accumulate,
                                      void* const* workspace, const size_t* workspace_bytes,
                                      dadet_wgrad_pending* pending_out, const float* const* amax_x,
                                      const float* const* amax_gy, void* stream) {
  DADET_REQUIRE(descs && n >= 1 && n <= kWgradGroupMax && x && gy && dw && accumulate && workspace && workspace_bytes &&
                    pending_out && amax_x && amax_gy, "conv_wgrad_group: bad arguments (1 - 4 problems, every array non-null)");
  DADET_REQUIRE(g_gemm_mode == 4, "conv_wgrad_group: contraction mode 4 only (mode %d is set)", g_gemm_mode);
  hipStream_t st = as_stream(stream);
  const plan::WgradGroupPlan p = group_descs_ok(descs, n) ? plan::plan_wgrad_group(descs, n, g_gemm_mode, g_big_mode)
                                                           : plan::WgradGroupPlan();
  DADET_REQUIRE(p.kind != 0, "conv_wgrad_group: these problems do not form a grouped launch (dadet_conv_wgrad_group_plan)");
  for (int i = 0; i < n; ++i) {
    DADET_REQUIRE(x[i] && gy[i] && dw[i] && amax_x[i] && amax_gy[i] && al16(x[i]) && al16(gy[i]) && al16(dw[i]),
                  "conv_wgrad_group: problem %d: null or misaligned pointer", i);
    for (int j = 0; j < i; ++j)
      DADET_REQUIRE(dw[i] != dw[j], "conv_wgrad_group: problems %d and %d write the same dw", j, i);
  }
  WgradArgs a[kWgradGroupMax];
  for (int i = 0; i < n; ++i) {
    const dadet_conv_desc* d = &descs[i];
    WgradArgs& w = a[i];
    fill_wgrad_args(d, d->Cout, p.tiles_co[i], p.tiles_kc[i], p.splits[i], p.rows, &w);
    w.x = x[i]; w.gy = gy[i]; w.out_scale = out_scale ? out_scale[i] : nullptr;
    w.accumulate = accumulate[i];
    w.amax_x = amax_x[i]; w.amax_gy = amax_gy[i];
    w.nf_flag = nf_flag_ptr();
    w.launch_id = w.nf_flag ? nf_next_launch("conv_wgrad_group", w.M, w.Cout, w.K, w.KH) : 0;
    pending_out[i].splits = 0;
    if (p.splits[i] == 1) {
      w.direct = 1;
      w.out = dw[i];
    } else {
      if (!workspace[i] || workspace_bytes[i] < p.workspace_bytes[i]) {
        set_error("conv_wgrad_group: problem %d: workspace %zu < required %zu", i, workspace_bytes[i], p.workspace_bytes[i]);
        return DADET_EWORKSPACE;
      }
      w.direct = 0;
      w.out = static_cast<float*>(workspace[i]);
    }
  }
  int rc = p.kind == 256 ? launch_wgrad_big_group(a, n, st) : launch_wgrad_split_group(a, n, p.small_map != 0, st);
  if (rc) return rc;
  for (int i = 0; i < n; ++i)
    if (p.splits[i] > 1)
      fill_pending(&pending_out[i], workspace[i], out_scale ? out_scale[i] : nullptr, dw[i], descs[i].Cout, a[i].K,
                   p.splits[i], accumulate[i]);
  return DADET_OK;
}
