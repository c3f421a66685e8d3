// Implicit-GEMM convolution (forward / data-gradient / weight-gradient) on the gfx950 fp32 matrix
// pipe (v_mfma_f32_32x32x2_f32: exact fp32, k-ordered fmaf chain — guide §3), NHWC activations,
// [Cout][KH][KW][Cin] weights.
//
// Stands in for the ATen conv2d / linear calls of the reference hot path and fuses what the reference
// runs as separate elementwise passes around them:
//   forward : conv -> FrozenBatchNorm2d affine (layers/batch_norm.py:19-24) -> (+ residual) -> relu_
//             (modeling/backbone/resnet.py:294-314, :331-336), conv + bias + relu (rpn/rpn.py:39-46,
//             da_heads/da_heads.py:32-37), nn.Linear (+relu) (da_heads.py:61-68, roi_box_predictors.py:28-33)
//   dgrad   : the same kernel run on the output gradient with the flipped/transposed weights, with the
//             upstream ReLU gating and the residual-gradient add fused into the epilogue
//   wgrad   : dW = gY^T * im2col(X), split over the (huge) N*Ho*Wo reduction axis, deterministic two-pass.
//
// GEMM view (forward): C[m][n] = sum_k A[m][k] * B[n][k],  m = (img, ho, wo), n = cout, k = (r, s, cin).
// Both operands are K-contiguous in HBM (NHWC rows / KRSC rows), so a K-tile of 32 is one 128-byte run
// per row: each lane moves 16 B, a wavefront covers 8 rows x 128 B.  Tiles are staged through LDS with a
// +4-float row pad (row stride 36 floats): the MFMA fragment reads are ds_read_b128 (4 consecutive k per
// lane, the k-slot order is permuted identically for A and B so the product is unchanged) and are
// bank-conflict free for the 16-lane service groups of ds_read_b128 (36*i mod 64 is a permutation of the
// 16 quad-slots); the staging writes are ds_write_b128 of 8 contiguous lanes per row.
// A 256-thread workgroup = 4 wavefronts as 2x2, each wavefront owns a (TM*32)x(TN*32) block of the
// output tile, accumulators live in registers (16 fp32 per 32x32 block).  K loop: the global loads of
// tile t+1 are issued into registers before the MFMAs of tile t and written to the (single) LDS buffer
// after them; at ~36 KB of LDS and 144 registers three workgroups are resident per CU (12 waves), and it is
// this cross-workgroup overlap that keeps the matrix pipe fed across the two barriers of a K-tile (PMC on
// the double-buffered / 2-workgroup variant: 38% of wave cycles parked in s_waitcnt/s_barrier).
// Workgroup ids are remapped so that each XCD (private L2) walks a contiguous range of m-tiles.
#include "conv_common.h"

namespace dadet {

template <int TM, int TN>
__global__ __launch_bounds__(256, 3) void conv_fwd_kernel(const ConvArgs a) {
  constexpr int BM = 2 * TM * 32, BN = 2 * TN * 32;
  constexpr int A_LOADS = BM / 32, B_LOADS = BN / 32;  // float4 loads per thread per K-tile
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* As = reinterpret_cast<float*>(smem);                 // [BM][LDS_STRIDE]
  float* Bs = As + BM * LDS_STRIDE;                           // [BN][LDS_STRIDE]

  const int nwg = a.tiles_m * a.tiles_n;
  const int tile = xcd_remap(blockIdx.x, nwg);
  const int bm0 = (tile / a.tiles_n) * BM;
  const int bn0 = (tile % a.tiles_n) * BN;

  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int lcol = t & 7;    // float4 column of the K-tile this thread stages
  const int lrow = t >> 3;   // first staged row (0..31)

  const __amdgpu_buffer_rsrc_t xr = make_rsrc(a.x, a.x_bytes);
  const __amdgpu_buffer_rsrc_t wr = make_rsrc(a.w, a.w_bytes);

  // per staged A row: image pixel base and top-left input coordinate
  int pixbase[A_LOADS], hi0[A_LOADS], wi0[A_LOADS];
  const int HoWo = a.Ho * a.Wo;
#pragma unroll
  for (int i = 0; i < A_LOADS; ++i) {
    const int m = bm0 + lrow + 32 * i;
    if (m < a.M) {
      const int img = m / HoWo;
      const int rem = m - img * HoWo;
      const int ho = rem / a.Wo;
      const int wo = rem - ho * a.Wo;
      pixbase[i] = img * a.H * a.W;
      hi0[i] = ho * a.stride - a.pad;
      wi0[i] = wo * a.stride - a.pad;
    } else {
      pixbase[i] = 0;
      hi0[i] = -(1 << 28);  // fails every bounds check
      wi0[i] = 0;
    }
  }
  // weight rows of this thread (byte offsets of column 0), out-of-range rows read as zero
  unsigned wrow[B_LOADS];
#pragma unroll
  for (int i = 0; i < B_LOADS; ++i) {
    const int n = bn0 + lrow + 32 * i;
    wrow[i] = n < a.Cout ? (unsigned)n * (unsigned)a.K * 4u : kOOB;
  }

  float4 ra[A_LOADS], rb[B_LOADS];

  // (r, s, c) of this thread's float4 column, advanced incrementally from K-tile to K-tile
  int kk = lcol * 4;
  int tap = kk / a.Cin;
  int kc = kk - tap * a.Cin;
  int kr = tap / a.KW;
  int ks = tap - kr * a.KW;

  auto load_tile = [&]() {
    const bool kvalid = kk < a.K;
#pragma unroll
    for (int i = 0; i < A_LOADS; ++i) {
      const int hi = hi0[i] + kr, wi = wi0[i] + ks;
      const bool ok = kvalid && (unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W;
      const unsigned off = ((unsigned)(pixbase[i] + hi * a.W + wi) * (unsigned)a.Cin + (unsigned)kc) * 4u;
      ra[i] = buf_load4(xr, ok ? off : kOOB);
    }
#pragma unroll
    for (int i = 0; i < B_LOADS; ++i)
      rb[i] = buf_load4(wr, (kvalid && wrow[i] != kOOB) ? wrow[i] + (unsigned)kk * 4u : kOOB);
    // advance to the next K-tile
    kk += BK;
    kc += BK;
    while (kc >= a.Cin) {
      kc -= a.Cin;
      if (++ks == a.KW) {
        ks = 0;
        ++kr;
      }
    }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int i = 0; i < A_LOADS; ++i)
      *reinterpret_cast<float4*>(As + (lrow + 32 * i) * LDS_STRIDE + lcol * 4) = ra[i];
#pragma unroll
    for (int i = 0; i < B_LOADS; ++i)
      *reinterpret_cast<float4*>(Bs + (lrow + 32 * i) * LDS_STRIDE + lcol * 4) = rb[i];
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  const int nk = (a.K + BK - 1) / BK;
  load_tile();
  store_tile();
  __syncthreads();

  const int frag_row = lane & 31;        // row of the 32-row fragment this lane feeds
  const int frag_k = (lane >> 5) * 4;    // which 4-float half of each 8-float k-group
  const float* Ab = As + (wm * TM * 32 + frag_row) * LDS_STRIDE + frag_k;
  const float* Bb = Bs + (wn * TN * 32 + frag_row) * LDS_STRIDE + frag_k;
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) load_tile();  // buffer loads in flight during the MFMAs below
#pragma unroll
    for (int j = 0; j < BK / 8; ++j) {
      float4 fa[TM], fb[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i)
        fa[i] = *reinterpret_cast<const float4*>(Ab + i * 32 * LDS_STRIDE + j * 8);
#pragma unroll
      for (int i = 0; i < TN; ++i)
        fb[i] = *reinterpret_cast<const float4*>(Bb + i * 32 * LDS_STRIDE + j * 8);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
#pragma unroll
        for (int im = 0; im < TM; ++im)
#pragma unroll
          for (int in = 0; in < TN; ++in) {
            const float av = e == 0 ? fa[im].x : e == 1 ? fa[im].y : e == 2 ? fa[im].z : fa[im].w;
            const float bv = e == 0 ? fb[in].x : e == 1 ? fb[in].y : e == 2 ? fb[in].z : fb[in].w;
            acc[im][in] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[im][in], 0, 0, 0);
          }
      }
    }
    // one LDS buffer (36 KB for the 128x128 tile): three workgroups share a CU, so another workgroup's MFMAs
    // cover this one's staging; the price is a second barrier per K-tile
    if (kt + 1 < nk) {
      __syncthreads();
      store_tile();
      __syncthreads();
    }
  }

  // epilogue: D layout of the 32x32 MFMA — col = lane & 31, row = (reg & 3) + 8*(reg >> 2) + 4*(lane >> 5).
  // Ragged edges are handled by out-of-range buffer offsets (loads give 0, stores are dropped).
  const __amdgpu_buffer_rsrc_t yr = make_rsrc(a.y, a.y_bytes);
  const __amdgpu_buffer_rsrc_t ar = make_rsrc(a.addend ? a.addend : a.y, a.addend ? a.y_bytes : 0u);
  const __amdgpu_buffer_rsrc_t mr = make_rsrc(a.mask_ref ? a.mask_ref : a.y, a.mask_ref ? a.y_bytes : 0u);
  const int col_in = lane & 31;
  const int row_hi = 4 * (lane >> 5);
#pragma unroll
  for (int in = 0; in < TN; ++in) {
    const int n = bn0 + wn * TN * 32 + in * 32 + col_in;
    const bool nvalid = n < a.Cout;
    const float sc = (a.scale && nvalid) ? a.scale[n] : 1.f;
    const float bi = (a.bias && nvalid) ? a.bias[n] : 0.f;
#pragma unroll
    for (int im = 0; im < TM; ++im) {
      // four rows (one accumulator row-group) at a time keeps the epilogue's live registers small; the
      // scheduling barrier stops hipcc from interleaving all 16 groups (which cost 200+ VGPRs and occupancy)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        unsigned offs[4];
        float add[4], msk[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int m = bm0 + wm * TM * 32 + im * 32 + q + 8 * g + row_hi;
          unsigned orow = (unsigned)m;
          if (a.os != 1) {
            const int img = m / HoWo;
            const int rem = m - img * HoWo;
            const int ho = rem / a.Wo;
            const int wo = rem - ho * a.Wo;
            orow = (unsigned)((img * a.OutH + ho * a.os) * a.OutW + wo * a.os);
          }
          offs[q] = (nvalid && m < a.M) ? (orow * (unsigned)a.Cout + (unsigned)n) * 4u : kOOB;
        }
        if (a.addend) {
#pragma unroll
          for (int q = 0; q < 4; ++q) add[q] = buf_load1(ar, offs[q]);
        }
        if (a.relu_mode == 2) {
#pragma unroll
          for (int q = 0; q < 4; ++q) msk[q] = buf_load1(mr, offs[q]);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float v = acc[im][in][g * 4 + q];
          if (a.scale) v = v * sc;
          if (a.bias) v = v + bi;
          if (a.addend) v = v + add[q];
          if (a.relu_mode == 1) v = fmaxf(v, 0.f);
          else if (a.relu_mode == 2) v = (msk[q] > 0.f) ? v : 0.f;
          buf_store1(yr, offs[q], v);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// weight gradient.  GEMM view: D[co][kc] = sum_m gY[m][co] * Xg[m][kc], kc = (r, s, ci).
// Both operands are staged as [32 m-rows][128 columns] (their natural HBM orientation, 16 B per lane
// along the channel axis); MFMA fragments are ds_read_b32 down the columns — consecutive lanes hit
// consecutive banks, so no padding is needed.  grid = (co tiles * kc tiles, m splits).

__global__ __launch_bounds__(256, 3) void conv_wgrad_kernel(const WgradArgs a) {
  constexpr int TILE = 128, RK = 32;  // output tile 128x128, 32 m-rows per step
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* Gs = reinterpret_cast<float*>(smem);   // [RK][TILE]  gY rows
  float* Xs = Gs + RK * TILE;                   // [RK][TILE]  gathered X rows

  const int tile = xcd_remap(blockIdx.x, a.tiles_co * a.tiles_kc);
  const int co0 = (tile / a.tiles_kc) * TILE;
  const int kc0 = (tile % a.tiles_kc) * TILE;
  const int split = blockIdx.y;
  const int m_begin = split * a.rows_per_split;
  int m_end = m_begin + a.rows_per_split;
  if (m_end > a.M) m_end = a.M;

  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int lcol = t & 31;   // float4 column (0..31) of the 128-wide row
  const int lrow = t >> 5;   // 0..7 ; rows lrow + 8*i

  // this thread's X column -> (tap, channel) is fixed for the whole kernel
  const int kk = kc0 + lcol * 4;
  const bool kvalid = kk < a.K;
  const int tap = kk / a.Cin;
  const int ci = kk - tap * a.Cin;
  const int r = tap / a.KW;
  const int s = tap - r * a.KW;
  const int co = co0 + lcol * 4;
  const bool covalid = co < a.Cout;  // Cout % 4 == 0 is required by the host wrapper
  const int HoWo = a.Ho * a.Wo;

  const __amdgpu_buffer_rsrc_t xr = make_rsrc(a.x, a.x_bytes);
  const __amdgpu_buffer_rsrc_t gr = make_rsrc(a.gy, a.gy_bytes);
  float4 rg[4], rx[4];
  const unsigned co_off = covalid ? (unsigned)co * 4u : kOOB;
  // (img, ho, wo) of this thread's four rows, advanced by RK rows per step
  int r_img[4], r_ho[4], r_wo[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m_begin + lrow + 8 * i;
    r_img[i] = m / HoWo;
    const int rem = m - r_img[i] * HoWo;
    r_ho[i] = rem / a.Wo;
    r_wo[i] = rem - r_ho[i] * a.Wo;
  }
  const int d_img = RK / HoWo, d_ho = (RK - d_img * HoWo) / a.Wo, d_wo = RK - d_img * HoWo - d_ho * a.Wo;
  int m_cur = m_begin;
  auto load_tile = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m_cur + lrow + 8 * i;
      const bool mv = m < m_end;
      rg[i] = buf_load4(gr, (mv && covalid) ? (unsigned)m * (unsigned)a.gy_ld * 4u + co_off : kOOB);
      const int hi = r_ho[i] * a.stride - a.pad + r;
      const int wi = r_wo[i] * a.stride - a.pad + s;
      const bool ok = mv && kvalid && (unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W;
      const unsigned off = ((unsigned)((r_img[i] * a.H + hi) * a.W + wi) * (unsigned)a.Cin + (unsigned)ci) * 4u;
      rx[i] = buf_load4(xr, ok ? off : kOOB);
      // advance this row by RK output pixels
      int wo = r_wo[i] + d_wo;
      const int cw = wo >= a.Wo;
      wo -= cw ? a.Wo : 0;
      int ho = r_ho[i] + d_ho + cw;
      const int ch = ho >= a.Ho;
      ho -= ch ? a.Ho : 0;
      r_wo[i] = wo;
      r_ho[i] = ho;
      r_img[i] += d_img + ch;
    }
    m_cur += RK;
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<float4*>(Gs + (lrow + 8 * i) * TILE + lcol * 4) = rg[i];
      *reinterpret_cast<float4*>(Xs + (lrow + 8 * i) * TILE + lcol * 4) = rx[i];
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  const int nsteps = (m_end - m_begin + RK - 1) / RK;
  if (nsteps > 0) {
    load_tile();
    store_tile();
  }
  __syncthreads();
  const int fcol = lane & 31, fk = lane >> 5;
  const float* Gb = Gs + wm * 64 + fcol;
  const float* Xb = Xs + wn * 64 + fcol;
  for (int st = 0; st < nsteps; ++st) {
    if (st + 1 < nsteps) load_tile();
#pragma unroll
    for (int k2 = 0; k2 < RK / 2; ++k2) {
      const int row = 2 * k2 + fk;
      const float g0 = Gb[row * TILE], g1 = Gb[row * TILE + 32];
      const float x0 = Xb[row * TILE], x1 = Xb[row * TILE + 32];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(g0, x0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(g0, x1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(g1, x0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(g1, x1, acc[1][1], 0, 0, 0);
    }
    if (st + 1 < nsteps) {
      __syncthreads();
      store_tile();
      __syncthreads();
    }
  }

  float* out = a.direct ? a.out : a.out + (size_t)split * a.Cout * a.K;
  const int col_in = lane & 31, row_hi = 4 * (lane >> 5);
#pragma unroll
  for (int in = 0; in < 2; ++in) {
    const int kc = kc0 + wn * 64 + in * 32 + col_in;
    if (kc >= a.K) continue;
#pragma unroll
    for (int im = 0; im < 2; ++im)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int c = co0 + wm * 64 + im * 32 + (reg & 3) + 8 * (reg >> 2) + row_hi;
        if (c >= a.Cout) continue;
        const size_t off = (size_t)c * a.K + kc;
        float v = acc[im][in][reg];
        if (a.direct) {
          if (a.out_scale) v = v * a.out_scale[c];
          if (a.accumulate) v = v + out[off];
        }
        out[off] = v;
      }
  }
}

template <int TM, int TN>
static int launch_fwd(ConvArgs& a, hipStream_t st) {
  constexpr int BM = 2 * TM * 32, BN = 2 * TN * 32;
  const size_t lds = sizeof(float) * (BM + BN) * LDS_STRIDE;
  static bool attr_set = false;
  if (lds > 48 * 1024)
    if (const int rc = raise_lds_once(&attr_set, "conv_forward", conv_fwd_kernel<TM, TN>, lds); rc != DADET_OK) return rc;
  hipLaunchKernelGGL((conv_fwd_kernel<TM, TN>), dim3(a.tiles_m * a.tiles_n), dim3(256), lds, st, a);
  return check_launch("conv_forward");
}

int launch_fwd_exact(ConvArgs& a, const plan::FwdPlan& p, hipStream_t st) {
  if (p.tm == 2) return p.tn == 2 ? launch_fwd<2, 2>(a, st) : launch_fwd<2, 1>(a, st);
  return launch_fwd<1, 1>(a, st);
}

int launch_wgrad_exact(WgradArgs& a, hipStream_t st) {
  const size_t lds = sizeof(float) * 2 * 32 * 128;  // 32 KB: three workgroups per CU
  static bool attr_set = false;
  if (const int rc = raise_lds_once(&attr_set, "conv_wgrad", conv_wgrad_kernel, lds); rc != DADET_OK) return rc;
  hipLaunchKernelGGL(conv_wgrad_kernel, dim3(a.tiles_co * a.tiles_kc, a.splits), dim3(256), lds, st, a);
  return check_launch("conv_wgrad");
}

}  // namespace dadet
