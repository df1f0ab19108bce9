// Distance objective of the reference's *_spe_do configs (distance_loss / distance_target): the auxiliary loss over the
// FINAL edge channels e_L [B,N,N,De].
//   target   lib/models/graph_model_base.py:66-76     sum of the first T clipped hop matrices, an integer in [0, T]
//   head     graph_model_base.py:83-94, graph_xformer_model_base.py:343-372
//            logits = Dense_t(act(Dense_1(act(Dense_0(edge_norm_final(e))))))      De -> M0 -> M1 -> C = T + 1
//   loss     lib/base/genutil/loss_layers.py:38-67    per_graph[b] = sum_ij CE(logits, target) * (target > 0)
// One kernel per direction.  A wave owns a 16-pair tile (tiles are cut per graph: the last tile of a graph is ragged, none
// straddles two graphs); a tile whose 16 targets are all 0 is skipped before anything of e is loaded.  The three products run
// on v_mfma_f32_16x16x4_f32 tiles with the LayerNorm-folded, zero-padded weights (M0 -> 32, M1 -> 16, C -> 16 columns)
// resident in LDS; the activations of a tile go through a per-wave LDS image in [pair][feature] layout, which is the
// A operand of the next product and -- transposed -- of the weight-gradient products of the backward.  The backward recomputes
// the forward from e (nothing is saved).  Loss and parameter-gradient partials are per workgroup, reduced in a fixed order by
// k_edge_head_reduce / k_edge_head_finish: no atomics, two runs are bitwise equal.
#include "egt_common.h"
#include <cstring>

typedef float v4f_h __attribute__((ext_vector_type(4)));
#define HMFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

#define EH_NW 4      // waves per workgroup
#define EH_P0 36     // LDS pitch of W0f rows / of the x1 image  (32 columns + 4: the transposed reads stay conflict-free)
#define EH_P1 20     // LDS pitch of W1 / Wt rows, of the x2 and d_logits images (16 columns + 4)

// LDS hand-offs inside one wavefront: DS operations of a wave complete in order (egt_tile.h lds_sync)
__device__ __forceinline__ void eh_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// geometry of one instance: DET = 16-column tiles of the (zero-padded) edge width
template <int DET>
struct EhGeo {
  static constexpr int DEP = 16 * DET;                     // padded De
  static constexpr int PE = DEP + 4;                       // pitch of the e image
  static constexpr int W0 = 0;                             // [DEP][EH_P0]   gamma-folded
  static constexpr int W1 = W0 + DEP * EH_P0;              // [32][EH_P1]
  static constexpr int WT = W1 + 32 * EH_P1;               // [16][EH_P1]
  static constexpr int B0 = WT + 16 * EH_P1;               // [32]           beta-folded
  static constexpr int B1 = B0 + 32;                       // [16]
  static constexpr int BT = B1 + 16;                       // [16]
  static constexpr int IMG = BT + 16;                      // floats of the prepared weight image
  // per-wave activations
  static constexpr int XE = 0;                             // [16][PE]
  static constexpr int X1 = XE + 16 * PE;                  // [16][EH_P0]
  static constexpr int X2 = X1 + 16 * EH_P0;               // [16][EH_P1]
  static constexpr int DL = X2 + 16 * EH_P1;               // [16][EH_P1]
  static constexpr int RS = DL + 16 * EH_P1;               // [16] rstd
  static constexpr int WAVE = RS + 16;
  // gradient image of a workgroup / of the reduction (dense)
  static constexpr int G0 = 0;                             // dW0f [DEP][32]
  static constexpr int G1 = G0 + DEP * 32;                 // dW1  [32][16]
  static constexpr int GT = G1 + 32 * 16;                  // dWt  [16][16]
  static constexpr int GB0 = GT + 16 * 16;                 // [32]
  static constexpr int GB1 = GB0 + 32;                     // [16]
  static constexpr int GBT = GB1 + 16;                     // [16]
  static constexpr int PG = GBT + 16;
};
static inline int eh_det(int De) { return De <= 16 ? 1 : De / 16; }
static inline int eh_img(int det) { return 16 * det * EH_P0 + 32 * EH_P1 + 16 * EH_P1 + 64; }
static inline int eh_pg(int det) { return 16 * det * 32 + 32 * 16 + 16 * 16 + 64; }

// ---- weight image: gamma folded into W0, beta into b0, everything zero-padded to the tile widths (one wave) ----
__global__ void __launch_bounds__(64) k_edge_head_prep(const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       const float* __restrict__ W0, const float* __restrict__ b0,
                                                       const float* __restrict__ W1, const float* __restrict__ b1,
                                                       const float* __restrict__ Wt, const float* __restrict__ bt,
                                                       float* __restrict__ img, int De, int DEP, int M0, int M1, int C, int ln) {
  const int oW1 = DEP * EH_P0, oWT = oW1 + 32 * EH_P1, oB0 = oWT + 16 * EH_P1, oB1 = oB0 + 32, oBT = oB1 + 16;
  for (int i = threadIdx.x; i < DEP * EH_P0; i += 64) {
    const int k = i / EH_P0, j = i % EH_P0;
    img[i] = (k < De && j < M0) ? (ln ? gamma[k] : 1.f) * W0[k * M0 + j] : 0.f;
  }
  for (int i = threadIdx.x; i < 32 * EH_P1; i += 64) {
    const int k = i / EH_P1, j = i % EH_P1;
    img[oW1 + i] = (k < M0 && j < M1) ? W1[k * M1 + j] : 0.f;
  }
  for (int i = threadIdx.x; i < 16 * EH_P1; i += 64) {
    const int k = i / EH_P1, j = i % EH_P1;
    img[oWT + i] = (k < M1 && j < C) ? Wt[k * C + j] : 0.f;
  }
  for (int j = threadIdx.x; j < 32; j += 64) {
    float s = 0.f;
    if (j < M0) {
      s = b0[j];
      if (ln)
        for (int k = 0; k < De; ++k) s = fmaf(beta[k], W0[k * M0 + j], s);
    }
    img[oB0 + j] = s;
  }
  for (int j = threadIdx.x; j < 16; j += 64) {
    img[oB1 + j] = j < M1 ? b1[j] : 0.f;
    img[oBT + j] = j < C ? bt[j] : 0.f;
  }
}

// ---- MFMA products on LDS images; lane (i = lane & 15, q = lane >> 4); D: row 4 q + r, column i ----
// acc += A[16 x K] . B[K x 16]: A rows at A[i * pa + k] (one 16-byte read = 4 contraction steps, the contraction index of step s
// is 16 g + 4 q + s on both sides), B at B[k * pb + i]
template <int K>
__device__ __forceinline__ v4f_h eh_mm_nn(const float* A, int pa, const float* B, int pb, int i, int q, v4f_h acc) {
#pragma unroll
  for (int g = 0; g < K / 16; ++g) {
    const v4f_h a4 = *reinterpret_cast<const v4f_h*>(A + i * pa + 16 * g + 4 * q);
    const float* bp = B + (16 * g + 4 * q) * pb + i;
    acc = HMFMA(a4[0], bp[0], acc);
    acc = HMFMA(a4[1], bp[pb], acc);
    acc = HMFMA(a4[2], bp[2 * pb], acc);
    acc = HMFMA(a4[3], bp[3 * pb], acc);
  }
  return acc;
}
// acc += A[16 x K] . W^T: B[k][column] = W[column * pw + k] (the backward through a Dense kernel)
template <int K>
__device__ __forceinline__ v4f_h eh_mm_nt(const float* A, int pa, const float* W, int pw, int i, int q, v4f_h acc) {
#pragma unroll
  for (int g = 0; g < K / 16; ++g) {
    const v4f_h a4 = *reinterpret_cast<const v4f_h*>(A + i * pa + 16 * g + 4 * q);
    const v4f_h b4 = *reinterpret_cast<const v4f_h*>(W + i * pw + 16 * g + 4 * q);
    acc = HMFMA(a4[0], b4[0], acc);
    acc = HMFMA(a4[1], b4[1], acc);
    acc = HMFMA(a4[2], b4[2], acc);
    acc = HMFMA(a4[3], b4[3], acc);
  }
  return acc;
}
// acc += X^T . Y over the 16 pairs of the tile: A[row][k] = X[k * px + row], B[k][column] = Y[k * py + column]
__device__ __forceinline__ v4f_h eh_mm_tn(const float* X, int px, const float* Y, int py, int i, int q, v4f_h acc) {
#pragma unroll
  for (int s = 0; s < 4; ++s) acc = HMFMA(X[(4 * q + s) * px + i], Y[(4 * q + s) * py + i], acc);
  return acc;
}

__device__ __forceinline__ float eh_act(float x, int act) {
  return act == EGT_ACT_ELU ? (x > 0.f ? x : expm1f(x)) : fmaxf(x, 0.f);
}
// act'(x) from y = act(x): elu' = 1 (x > 0) or exp(x) = y + 1; relu' = [y > 0]
__device__ __forceinline__ float eh_dact(float y, int act) {
  return y > 0.f ? 1.f : (act == EGT_ACT_ELU ? y + 1.f : 0.f);
}
__device__ __forceinline__ float eh_sum_q(float v) { return sum_xor32(sum_xor16(v)); }

// a 4-channel slot of e as loaded (bf16: the raw bits, widened only when the slot goes into the LDS image, so that a
// prefetched tile stays in flight)
__device__ __forceinline__ float4 eh_ld_raw(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ uint2 eh_ld_raw(const uint16_t* p) { return *reinterpret_cast<const uint2*>(p); }
__device__ __forceinline__ float4 eh_widen(float4 v) { return v; }
__device__ __forceinline__ float4 eh_widen(uint2 v) { return bf4_to_f4(v); }
template <typename T> struct EhRaw { typedef float4 type; };
template <> struct EhRaw<uint16_t> { typedef uint2 type; };
__device__ __forceinline__ void eh_zero(float4& v) { v = make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ void eh_zero(uint2& v) { v = make_uint2(0u, 0u); }
__device__ __forceinline__ void eh_st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ void eh_st4(uint16_t* p, float4 v) { *reinterpret_cast<uint2*>(p) = f4_to_bf4(v); }

// ---- the 16-row tile of both heads: set-up, forward, backward from d_logits, workgroup partials ----
// A wave's view of the workgroup's LDS and of its rows: `width` is the real row width (De / W), DET gives the padded one.
template <int DET>
struct EhTile {
  float *XE, *X1, *X2, *DL, *RS;        // the wave's activation images
  const float *wsm, *W0, *W1, *WT;      // the weight image
  int lane, wave, i, q;
  int width, C4, NF4;                   // 16-byte (fp32) slots per row / per tile
  float inv;                            // 1 / width
};
// the parameter-gradient accumulators of a wave
template <int DET>
struct EhGrad {
  v4f_h W0[DET][2], W1[2], Wt;
  float b0[2], b1, bt;
};
template <int DET>
__device__ __forceinline__ void eh_zero(EhGrad<DET>& g) {
#pragma unroll
  for (int a = 0; a < DET; ++a) g.W0[a][0] = g.W0[a][1] = (v4f_h){0.f, 0.f, 0.f, 0.f};
  g.W1[0] = g.W1[1] = g.Wt = (v4f_h){0.f, 0.f, 0.f, 0.f};
  g.b0[0] = g.b0[1] = g.b1 = g.bt = 0.f;
}

// weight image -> wsm, the per-wave activation area zeroed (the pad columns of the row image stay 0); ends on a workgroup barrier
template <int DET>
__device__ __forceinline__ EhTile<DET> eh_setup(float* wsm, float* asm_, const float* __restrict__ img, int width) {
  using Z = EhGeo<DET>;
  EhTile<DET> L;
  L.lane = threadIdx.x & 63, L.wave = threadIdx.x >> 6, L.i = L.lane & 15, L.q = L.lane >> 4;
  for (int k = threadIdx.x; k < Z::IMG; k += EH_NW * 64) wsm[k] = img[k];
  float* const my = asm_ + L.wave * Z::WAVE;
  for (int k = L.lane; k < Z::WAVE; k += 64) my[k] = 0.f;
  __syncthreads();
  L.XE = my + Z::XE, L.X1 = my + Z::X1, L.X2 = my + Z::X2, L.DL = my + Z::DL, L.RS = my + Z::RS;
  L.wsm = wsm, L.W0 = wsm + Z::W0, L.W1 = wsm + Z::W1, L.WT = wsm + Z::WT;
  L.width = width, L.C4 = width >> 2, L.NF4 = 4 * width;
  L.inv = 1.0f / (float)width;
  return L;
}

// `valid` rows of `src` -> the XE image (rows >= valid: zeros), the optional LayerNorm (rstd -> RS), the three products.
// a1 / a2: the activations x1 / x2 (also left in X1 / X2), z: the logits
template <int DET, typename T>
__device__ __forceinline__ void eh_tile_fwd(const EhTile<DET>& L, const T* src, int valid, int act, int ln, float eps,
                                            v4f_h (&a1)[2], v4f_h& a2, v4f_h& z) {
  using Z = EhGeo<DET>;
  constexpr int PE = Z::PE;
  const int lane = L.lane, i = L.i, q = L.q, C4 = L.C4;
  float* const XE = L.XE;
  for (int f = lane; f < L.NF4; f += 64) {
    const int row = f / C4, c4 = f % C4;
    const float4 v = row < valid ? eh_widen(eh_ld_raw(src + (size_t)f * 4)) : make_float4(0.f, 0.f, 0.f, 0.f);
    *reinterpret_cast<float4*>(XE + row * PE + 4 * c4) = v;
  }
  eh_sync();
  // ---- LayerNorm: two-pass moments; 4 lanes per row ----
  if (ln) {
    const int row = lane >> 2, pt = lane & 3;
    float s = 0.f;
    for (int c4 = pt; c4 < C4; c4 += 4) {
      const float4 v = *reinterpret_cast<const float4*>(XE + row * PE + 4 * c4);
      s += (v.x + v.y) + (v.z + v.w);
    }
    s += lane_xor<1>(s); s += lane_xor<2>(s);
    const float mu = s * L.inv;
    float vs = 0.f;
    for (int c4 = pt; c4 < C4; c4 += 4) {
      const float4 v = *reinterpret_cast<const float4*>(XE + row * PE + 4 * c4);
      const float d0 = v.x - mu, d1 = v.y - mu, d2 = v.z - mu, d3 = v.w - mu;
      vs = fmaf(d0, d0, vs); vs = fmaf(d1, d1, vs); vs = fmaf(d2, d2, vs); vs = fmaf(d3, d3, vs);
    }
    vs += lane_xor<1>(vs); vs += lane_xor<2>(vs);
    const float rstd = rsqrtf(vs * L.inv + eps);
    for (int c4 = pt; c4 < C4; c4 += 4) {
      float4 v = *reinterpret_cast<const float4*>(XE + row * PE + 4 * c4);
      v.x = (v.x - mu) * rstd; v.y = (v.y - mu) * rstd; v.z = (v.z - mu) * rstd; v.w = (v.w - mu) * rstd;
      *reinterpret_cast<float4*>(XE + row * PE + 4 * c4) = v;
    }
    if (pt == 0) L.RS[row] = rstd;
    eh_sync();
  }
  // ---- x1 = act(xhat . W0f + b0f) ----
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    const float bb = L.wsm[Z::B0 + 16 * ct + i];
    v4f_h acc = (v4f_h){bb, bb, bb, bb};
    acc = eh_mm_nn<Z::DEP>(XE, PE, L.W0 + 16 * ct, EH_P0, i, q, acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      acc[r] = eh_act(acc[r], act);
      L.X1[(4 * q + r) * EH_P0 + 16 * ct + i] = acc[r];
    }
    a1[ct] = acc;
  }
  eh_sync();
  // ---- x2 = act(x1 . W1 + b1) ----
  {
    const float bb = L.wsm[Z::B1 + i];
    v4f_h acc = (v4f_h){bb, bb, bb, bb};
    acc = eh_mm_nn<32>(L.X1, EH_P0, L.W1, EH_P1, i, q, acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      acc[r] = eh_act(acc[r], act);
      L.X2[(4 * q + r) * EH_P1 + i] = acc[r];
    }
    a2 = acc;
  }
  eh_sync();
  // ---- logits ----
  {
    const float bb = L.wsm[Z::BT + i];
    z = (v4f_h){bb, bb, bb, bb};
    z = eh_mm_nn<16>(L.X2, EH_P1, L.WT, EH_P1, i, q, z);
  }
}

// The backward of a tile from its d_logits: the parameter gradients are added to g, the gradient of the tile's rows is left in
// the XE image (behind a wave sync, for the kernel's store)
template <int DET>
__device__ __forceinline__ void eh_tile_bwd(const EhTile<DET>& L, v4f_h dl, const v4f_h (&a1)[2], v4f_h a2, int act, int ln,
                                            EhGrad<DET>& g) {
  using Z = EhGeo<DET>;
  constexpr int PE = Z::PE;
  const int i = L.i, q = L.q;
  float *const XE = L.XE, *const X1 = L.X1, *const X2 = L.X2, *const DL = L.DL;
  g.bt += (dl[0] + dl[1]) + (dl[2] + dl[3]);
#pragma unroll
  for (int r = 0; r < 4; ++r) DL[(4 * q + r) * EH_P1 + i] = dl[r];
  eh_sync();
  g.Wt = eh_mm_tn(X2, EH_P1, DL, EH_P1, i, q, g.Wt);                                    // dWt += x2^T . dl
  v4f_h d2 = eh_mm_nt<16>(DL, EH_P1, L.WT, EH_P1, i, q, (v4f_h){0.f, 0.f, 0.f, 0.f});   // dx2 = dl . Wt^T
#pragma unroll
  for (int r = 0; r < 4; ++r) d2[r] *= eh_dact(a2[r], act);
  g.b1 += (d2[0] + d2[1]) + (d2[2] + d2[3]);
  eh_sync();                                                                           // x2 has been read
#pragma unroll
  for (int r = 0; r < 4; ++r) X2[(4 * q + r) * EH_P1 + i] = d2[r];
  eh_sync();
  v4f_h d1[2];
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    g.W1[ct] = eh_mm_tn(X1 + 16 * ct, EH_P0, X2, EH_P1, i, q, g.W1[ct]);               // dW1 += x1^T . dx2pre
    d1[ct] = eh_mm_nt<16>(X2, EH_P1, L.W1 + 16 * ct * EH_P1, EH_P1, i, q, (v4f_h){0.f, 0.f, 0.f, 0.f});
#pragma unroll
    for (int r = 0; r < 4; ++r) d1[ct][r] *= eh_dact(a1[ct][r], act);
    g.b0[ct] += (d1[ct][0] + d1[ct][1]) + (d1[ct][2] + d1[ct][3]);
  }
  eh_sync();                                                                           // x1 has been read
#pragma unroll
  for (int ct = 0; ct < 2; ++ct)
#pragma unroll
    for (int r = 0; r < 4; ++r) X1[(4 * q + r) * EH_P0 + 16 * ct + i] = d1[ct][r];
  eh_sync();
  v4f_h gx[DET];
#pragma unroll
  for (int a = 0; a < DET; ++a) {
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
      g.W0[a][ct] = eh_mm_tn(XE + 16 * a, PE, X1 + 16 * ct, EH_P0, i, q, g.W0[a][ct]);  // dW0f += xhat^T . dx1pre
    gx[a] = eh_mm_nt<32>(X1, EH_P0, L.W0 + 16 * a * EH_P0, EH_P0, i, q, (v4f_h){0.f, 0.f, 0.f, 0.f});   // dxhat = dx1pre . W0f^T
  }
  // ---- LayerNorm backward per row: dx = rstd (g - mean(g) - xhat mean(g xhat)) ----
  if (ln) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 4 * q + r;
      float xh[DET], s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int a = 0; a < DET; ++a) {
        xh[a] = XE[row * PE + 16 * a + i];
        s1 += gx[a][r];
        s2 = fmaf(gx[a][r], xh[a], s2);
      }
      s1 = row_sum16(s1) * L.inv;
      s2 = row_sum16(s2) * L.inv;
      const float rstd = L.RS[row];
#pragma unroll
      for (int a = 0; a < DET; ++a) gx[a][r] = rstd * (gx[a][r] - s1 - xh[a] * s2);
    }
  }
  eh_sync();                                                                           // xhat has been read
#pragma unroll
  for (int a = 0; a < DET; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (16 * a + i < L.width) XE[(4 * q + r) * PE + 16 * a + i] = gx[a][r];           // (width 8: the pad columns stay 0)
  eh_sync();
}

// the waves' parameter gradients added in index order in the (now free) activation area -> part[blockIdx.x * PG ..]
template <int DET>
__device__ __forceinline__ void eh_wg_partials(const EhTile<DET>& L, EhGrad<DET>& g, float* red, float* __restrict__ part) {
  using Z = EhGeo<DET>;
  static_assert(EH_NW * Z::WAVE >= Z::PG, "the gradient image is reduced in the activation area");
  const int i = L.i, q = L.q;
  g.b0[0] = eh_sum_q(g.b0[0]); g.b0[1] = eh_sum_q(g.b0[1]); g.b1 = eh_sum_q(g.b1); g.bt = eh_sum_q(g.bt);
  __syncthreads();   // every wave is done with its activation image
  for (int w = 0; w < EH_NW; ++w) {
    if (L.wave == w) {
      const bool first = w == 0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int a = 0; a < DET; ++a)
#pragma unroll
          for (int ct = 0; ct < 2; ++ct) {
            float* p = red + Z::G0 + (16 * a + 4 * q + r) * 32 + 16 * ct + i;
            *p = (first ? 0.f : *p) + g.W0[a][ct][r];
          }
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
          float* p = red + Z::G1 + (16 * ct + 4 * q + r) * 16 + i;
          *p = (first ? 0.f : *p) + g.W1[ct][r];
        }
        float* p = red + Z::GT + (4 * q + r) * 16 + i;
        *p = (first ? 0.f : *p) + g.Wt[r];
      }
      if (q == 0) {
        float* p = red + Z::GB0 + i;
        p[0] = (first ? 0.f : p[0]) + g.b0[0];
        p[16] = (first ? 0.f : p[16]) + g.b0[1];
        p = red + Z::GB1 + i;
        *p = (first ? 0.f : *p) + g.b1;
        p = red + Z::GBT + i;
        *p = (first ? 0.f : *p) + g.bt;
      }
    }
    __syncthreads();
  }
  float* out = part + (size_t)blockIdx.x * Z::PG;
  for (int k = threadIdx.x; k < Z::PG; k += EH_NW * 64) out[k] = red[k];
}

// ---- edge head: the rows are the pairs of a graph ----
// grid = B * G workgroups; workgroup (b, g) owns the tiles [g * chunk, (g + 1) * chunk) of graph b, wave w every EH_NW-th of them.
// BWD == false: loss_part[b * G + g] = the workgroup's share of per_graph[b].
// BWD == true:  de = d per_graph / d e (zeros on skipped tiles), part[(b * G + g) * PG ..] = the workgroup's parameter gradients
template <int DET, typename T, bool BWD>
__global__ void __launch_bounds__(EH_NW * 64) k_edge_head(const T* __restrict__ e, const uint8_t* __restrict__ target,
                                                          const float* __restrict__ img, const float* __restrict__ sgrad,
                                                          T* __restrict__ de, float* __restrict__ loss_part,
                                                          float* __restrict__ part, int N, int G, int chunk, int De, int C, int act,
                                                          int ln, float eps) {
  using Z = EhGeo<DET>;
  constexpr int PE = Z::PE;
  __shared__ __attribute__((aligned(16))) float wsm[Z::IMG];
  __shared__ __attribute__((aligned(16))) float asm_[EH_NW * Z::WAVE];
  __shared__ float lsm[EH_NW];
  const int b = blockIdx.x / G, g = blockIdx.x % G;
  const int NN = N * N, TPG = (NN + 15) / 16;
  const int t0 = g * chunk, t1 = min(TPG, t0 + chunk);
  const EhTile<DET> L = eh_setup<DET>(wsm, asm_, img, De);
  const int lane = L.lane, i = L.i, q = L.q, C4 = L.C4, NF4 = L.NF4;
  const float sb = BWD ? sgrad[b] : 0.f;

  float lossacc = 0.f;
  EhGrad<DET> gr;
  eh_zero(gr);

  for (int t = t0 + L.wave; t < t1; t += EH_NW) {
    const int valid = min(16, NN - 16 * t);
    const size_t p0 = (size_t)b * NN + (size_t)16 * t;       // first pair of the tile
    const int my_t = lane < valid ? (int)target[p0 + lane] : 0;
    if (__ballot(my_t != 0) == 0ull) {                         // nothing to learn here: no e load, no arithmetic
      if (BWD) {
        T* dt = de + p0 * De;
        for (int f = lane; f < NF4; f += 64)
          if (f / C4 < valid) eh_st4(dt + (size_t)f * 4, make_float4(0.f, 0.f, 0.f, 0.f));
      }
      continue;
    }
    v4f_h a1[2], a2, z;
    eh_tile_fwd<DET>(L, e + p0 * De, valid, act, ln, eps, a1, a2, z);
    // ---- max-subtracted log-sum-exp over the C real columns, gather, mask ----
    v4f_h dl;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int tr = __shfl(my_t, 4 * q + r, 64);
      const bool real = i < C;
      const float m = row_max16(real ? z[r] : -INFINITY);
      const float ex = real ? expf(z[r] - m) : 0.f;
      const float se = row_sum16(ex);
      const float zt = row_sum16(i == tr ? z[r] : 0.f);
      if (!BWD) {
        if (i == 0 && tr > 0) lossacc += (m + logf(se)) - zt;
      } else {
        dl[r] = (tr > 0 && real) ? (ex / se - (i == tr ? 1.f : 0.f)) * sb : 0.f;
      }
    }
    if (!BWD) continue;
    eh_tile_bwd<DET>(L, dl, a1, a2, act, ln, gr);
    {
      T* dt = de + p0 * De;                                    // (a target-0 row of a live tile stores what was computed: dl = 0 there)
      for (int f = lane; f < NF4; f += 64) {
        const int row = f / C4, c4 = f % C4;
        if (row < valid) eh_st4(dt + (size_t)f * 4, *reinterpret_cast<const float4*>(L.XE + row * PE + 4 * c4));
      }
    }
    eh_sync();   // the image is free for the next tile (its pad columns are untouched)
  }

  if (!BWD) {   // the workgroup's loss, waves added in index order
    const float l = eh_sum_q(lossacc);   // (lanes i == 0 carry the rows)
    if (lane == 0) lsm[L.wave] = l;
    __syncthreads();
    if (threadIdx.x == 0) loss_part[blockIdx.x] = ((lsm[0] + lsm[1]) + lsm[2]) + lsm[3];
    return;
  }
  eh_wg_partials<DET>(L, gr, asm_, part);
}

// per_graph[b] = sum_g loss_part[b][g], in index order
__global__ void __launch_bounds__(64) k_edge_head_loss(const float* __restrict__ loss_part, float* __restrict__ per_graph, int B,
                                                       int G) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  float s = 0.f;
  for (int g = 0; g < G; ++g) s += loss_part[(size_t)b * G + g];
  per_graph[b] = s;
}

// red[k] = sum over the workgroups' partials in a fixed order: 4 contiguous segments of workgroups per element, then the 4
__global__ void __launch_bounds__(256) k_edge_head_reduce(const float* __restrict__ part, float* __restrict__ red, int nwg, int PG) {
  __shared__ float sm[4][64];
  const int k = blockIdx.x * 64 + (threadIdx.x & 63), sg = threadIdx.x >> 6;
  const int per = (nwg + 3) / 4, w0 = sg * per, w1 = min(nwg, w0 + per);
  float s = 0.f;
  if (k < PG)
    for (int w = w0; w < w1; ++w) s += part[(size_t)w * PG + k];
  sm[sg][threadIdx.x & 63] = s;
  __syncthreads();
  if (sg == 0 && k < PG) red[k] = ((sm[0][threadIdx.x] + sm[1][threadIdx.x]) + sm[2][threadIdx.x]) + sm[3][threadIdx.x];
}

// the reduced (folded, padded) gradients -> the eight parameter gradients: W0f = gamma (.) W0, b0f = b0 + beta . W0
// (so W0 collects gamma[k] dW0f[k][j] + beta[k] db0f[j])
__global__ void __launch_bounds__(256) k_edge_head_finish(const float* __restrict__ red, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, const float* __restrict__ W0, float* __restrict__ d_gamma,
                                                          float* __restrict__ d_beta, float* __restrict__ d_W0,
                                                          float* __restrict__ d_b0, float* __restrict__ d_W1,
                                                          float* __restrict__ d_b1, float* __restrict__ d_Wt,
                                                          float* __restrict__ d_bt, int De, int DEP, int M0, int M1, int C, int ln) {
  const int oG1 = DEP * 32, oGT = oG1 + 512, oB0 = oGT + 256, oB1 = oB0 + 32, oBT = oB1 + 16;
  const int tid = threadIdx.x;
  for (int x = tid; x < De * M0; x += 256) {
    const int k = x / M0, j = x % M0;
    d_W0[x] = ln ? fmaf(gamma[k], red[k * 32 + j], beta[k] * red[oB0 + j]) : red[k * 32 + j];
  }
  if (ln)
    for (int k = tid; k < De; k += 256) {
      float sg = 0.f, sbt = 0.f;
      for (int j = 0; j < M0; ++j) {
        const float w = W0[k * M0 + j];
        sg = fmaf(red[k * 32 + j], w, sg);
        sbt = fmaf(red[oB0 + j], w, sbt);
      }
      d_gamma[k] = sg;
      d_beta[k] = sbt;
    }
  for (int x = tid; x < M0 * M1; x += 256) d_W1[x] = red[oG1 + (x / M1) * 16 + x % M1];
  for (int x = tid; x < M1 * C; x += 256) d_Wt[x] = red[oGT + (x / C) * 16 + x % C];
  for (int j = tid; j < M0; j += 256) d_b0[j] = red[oB0 + j];
  for (int j = tid; j < M1; j += 256) d_b1[j] = red[oB1 + j];
  for (int j = tid; j < C; j += 256) d_bt[j] = red[oBT + j];
}

// ---- node-classification head (the PATTERN / CLUSTER readout: sbm_pattern/dc.py, sbm_cluster/dc.py) ----
//   z = Dense_t(act(Dense_1(act(Dense_0(node_norm_final(h))))))                   W -> M0 -> M1 -> C
//   stats = (sum mask w[y] CE(z, y), sum mask [argmax z == y], sum mask)          lib/base/genutil/losses.py:41-118
// The same tile with another row source and epilogue: the rows are the R = B N flattened (graph, node) slots of h,
// workgroup g owns the tiles [g chunk, (g + 1) chunk); a tile whose 16 rows are all masked is skipped before h is loaded, and
// the target of a masked row is never used as a class.  The weight image and the parameter-gradient route
// (per-workgroup partials -> k_edge_head_reduce -> k_edge_head_finish) are the edge head's.
// BWD == false: stat_part[3 g ..] = the workgroup's (loss, hits, rows); hits and rows are integers (stored as their bit patterns).
// BWD == true:  dh = sgrad[0] d stats[0] / d h (exact zeros on masked rows), part[g * PG ..] = the parameter gradients.
template <int DET, bool BWD>
__global__ void __launch_bounds__(EH_NW * 64) k_node_head(const float* __restrict__ h, const int32_t* __restrict__ target,
                                                          const uint8_t* __restrict__ mask, const float* __restrict__ cw,
                                                          const float* __restrict__ img, const float* __restrict__ sgrad,
                                                          float* __restrict__ dh, float* __restrict__ stat_part,
                                                          float* __restrict__ part, int R, int chunk, int W, int C, int act, int ln,
                                                          float eps) {
  using Z = EhGeo<DET>;
  constexpr int PE = Z::PE;
  __shared__ __attribute__((aligned(16))) float wsm[Z::IMG];
  __shared__ __attribute__((aligned(16))) float asm_[EH_NW * Z::WAVE];
  __shared__ float lsm[EH_NW];
  __shared__ int csm[2 * EH_NW];
  __shared__ float cws[16];
  const int TPG = (R >> 4) + ((R & 15) != 0);
  const int t0 = min(TPG, (int)blockIdx.x * chunk), t1 = min(TPG, t0 + chunk);
  if (threadIdx.x < 16) cws[threadIdx.x] = (int)threadIdx.x < C ? cw[threadIdx.x] : 0.f;
  const EhTile<DET> L = eh_setup<DET>(wsm, asm_, img, W);
  const int lane = L.lane, i = L.i, q = L.q, C4 = L.C4, NF4 = L.NF4;
  const float sb = BWD ? sgrad[0] : 0.f;

  float lossacc = 0.f;
  int hits = 0, rows = 0;
  EhGrad<DET> gr;
  eh_zero(gr);

  for (int t = t0 + L.wave; t < t1; t += EH_NW) {
    const size_t r0 = (size_t)16 * t;                           // first row of the tile
    const int valid = (int)min((size_t)16, (size_t)R - r0);
    const bool lv = lane < valid && mask[r0 + lane] != 0;
    const unsigned long long lvm = __ballot(lv);                // bit r: row r of the tile is a real node
    if (lvm == 0ull) {                                          // nothing to learn here: no h load, no arithmetic
      if (BWD) {
        float* dt = dh + r0 * W;
        for (int f = lane; f < NF4; f += 64)
          if (f / C4 < valid) eh_st4(dt + (size_t)f * 4, make_float4(0.f, 0.f, 0.f, 0.f));
      }
      continue;
    }
    const int my_t = lv ? target[r0 + lane] : -1;               // a masked row has no class
    v4f_h a1[2], a2, z;
    eh_tile_fwd<DET>(L, h + r0 * W, valid, act, ln, eps, a1, a2, z);
    // ---- max-subtracted log-sum-exp over the C real columns, class weight, gather, arg-max (lowest index wins) ----
    v4f_h dl;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int tr = __shfl(my_t, 4 * q + r, 64);
      const bool live = (lvm >> (4 * q + r)) & 1ull;
      const bool real = i < C;
      const float m = row_max16(real ? z[r] : -INFINITY);
      const float ex = real ? expf(z[r] - m) : 0.f;
      const float se = row_sum16(ex);
      const float zt = row_sum16(i == tr ? z[r] : 0.f);
      const float wt = live ? cws[min(max(tr, 0), 15)] : 0.f;
      if (!BWD) {
        const float am = -row_max16((real && z[r] == m) ? -(float)i : -16.f);
        if (i == 0 && live) {
          lossacc += wt * ((m + logf(se)) - zt);
          hits += am == (float)tr ? 1 : 0;
          rows += 1;
        }
      } else {
        dl[r] = (live && real) ? (ex / se - (i == tr ? 1.f : 0.f)) * (wt * sb) : 0.f;
      }
    }
    if (!BWD) continue;
    eh_tile_bwd<DET>(L, dl, a1, a2, act, ln, gr);
    {
      float* dt = dh + r0 * W;
      for (int f = lane; f < NF4; f += 64) {
        const int row = f / C4, c4 = f % C4;
        if (row < valid) {
          const bool on = (lvm >> row) & 1ull;                                         // a masked row gets exact zeros
          eh_st4(dt + (size_t)f * 4, on ? *reinterpret_cast<const float4*>(L.XE + row * PE + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f));
        }
      }
    }
    eh_sync();   // the image is free for the next tile (its pad columns are untouched)
  }

  if (!BWD) {   // the workgroup's (loss, hits, rows), waves added in index order
    const float l = eh_sum_q(lossacc);   // (lanes i == 0 carry the rows)
    hits += __shfl_xor(hits, 16, 64); hits += __shfl_xor(hits, 32, 64);
    rows += __shfl_xor(rows, 16, 64); rows += __shfl_xor(rows, 32, 64);
    if (lane == 0) { lsm[L.wave] = l; csm[2 * L.wave] = hits; csm[2 * L.wave + 1] = rows; }
    __syncthreads();
    if (threadIdx.x == 0) {
      float* o = stat_part + (size_t)blockIdx.x * 3;
      o[0] = ((lsm[0] + lsm[1]) + lsm[2]) + lsm[3];
      o[1] = __int_as_float(csm[0] + csm[2] + csm[4] + csm[6]);
      o[2] = __int_as_float(csm[1] + csm[3] + csm[5] + csm[7]);
    }
    return;
  }
  eh_wg_partials<DET>(L, gr, asm_, part);
}

// stats = the workgroups' (loss, hits, rows) added in a fixed order: 64 contiguous segments, then the 64; the two counts in integers
__global__ void __launch_bounds__(64) k_node_head_stats(const float* __restrict__ stat_part, float* __restrict__ stats, int G) {
  __shared__ float ls[64];
  __shared__ long long hs[64], rs[64];
  const int per = (G + 63) / 64, w0 = threadIdx.x * per, w1 = min(G, w0 + per);
  float l = 0.f;
  long long hh = 0, rr = 0;
  for (int w = w0; w < w1; ++w) {
    l += stat_part[3 * (size_t)w];
    hh += __float_as_int(stat_part[3 * (size_t)w + 1]);
    rr += __float_as_int(stat_part[3 * (size_t)w + 2]);
  }
  ls[threadIdx.x] = l; hs[threadIdx.x] = hh; rs[threadIdx.x] = rr;
  __syncthreads();
  if (threadIdx.x == 0) {
    l = 0.f; hh = 0; rr = 0;
    for (int k = 0; k < 64; ++k) { l += ls[k]; hh += hs[k]; rr += rs[k]; }
    stats[0] = l; stats[1] = (float)hh; stats[2] = (float)rr;
  }
}

// ---- distance target: target = round(sum_{k=1..T} hop_k), hop_1 = A, hop_k = clip(A . hop_{k-1}, 0, 1) ----
// k_hop_chain's scheme (egt_embed.hip): a workgroup owns CT column tiles of one graph, keeps the zero-padded adjacency
// ([R16][R16 + 4]) and its column block of the current hop ([R16][16 CT + 4]) in LDS, and walks the hops without another global
// read; the running sum stays in the MFMA tiles' registers.  Sums of 0/1 products are exact in any order.  HP: the hop plane's row
// padding (4 floats against bank conflicts; 0 where the padded plane does not fit next to the adjacency: R16 = 192).
#define DT_NW 8
#define DT_MAXT 8
__global__ void __launch_bounds__(DT_NW * 64) k_dist_target(const float* __restrict__ adj, uint8_t* __restrict__ target, int N, int T,
                                                            int NB, int CT, int HP) {
  extern __shared__ __attribute__((aligned(16))) float dsm[];
  const int RT = (N + 15) / 16, R16 = RT * 16, PA = R16 + 4, PH = 16 * CT + HP;
  float* As = dsm;
  float* Hs = As + R16 * PA;
  const int b = blockIdx.x / NB, c0 = (blockIdx.x % NB) * CT * 16;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, kq = lane >> 4;
  const float* A = adj + (size_t)b * N * N;
  for (int x = threadIdx.x; x < R16 * PA; x += DT_NW * 64) {
    const int r = x / PA, c = x % PA;
    As[x] = (r < N && c < N) ? A[(size_t)r * N + c] : 0.f;
  }
  for (int x = threadIdx.x; x < R16 * PH; x += DT_NW * 64) {
    const int r = x / PH, c = c0 + x % PH;
    Hs[x] = (r < N && c < N && (x % PH) < 16 * CT) ? A[(size_t)r * N + c] : 0.f;
  }
  __syncthreads();
  const int ntile = RT * CT;
  v4f_h sum[DT_MAXT];
#pragma unroll
  for (int ti = 0; ti < DT_MAXT; ++ti) {
    sum[ti] = (v4f_h){0.f, 0.f, 0.f, 0.f};
    const int t = wave + DT_NW * ti;
    if (t < ntile)
#pragma unroll
      for (int r = 0; r < 4; ++r) sum[ti][r] = Hs[(16 * (t / CT) + 4 * kq + r) * PH + 16 * (t % CT) + m];   // hop 1
  }
  for (int k = 2; k <= T; ++k) {
    v4f_h acc[DT_MAXT];
#pragma unroll
    for (int ti = 0; ti < DT_MAXT; ++ti) {
      acc[ti] = (v4f_h){0.f, 0.f, 0.f, 0.f};
      const int t = wave + DT_NW * ti;
      if (t < ntile) {
        const float* ap = As + (16 * (t / CT) + m) * PA + 4 * kq;
        const float* bp = Hs + (4 * kq) * PH + 16 * (t % CT) + m;
        v4f_h c = acc[ti];
        for (int g = 0; g < RT; ++g) {
          const v4f_h a4 = *reinterpret_cast<const v4f_h*>(ap + 16 * g);
          const float* bg = bp + 16 * g * PH;
          c = HMFMA(a4[0], bg[0], c);
          c = HMFMA(a4[1], bg[PH], c);
          c = HMFMA(a4[2], bg[2 * PH], c);
          c = HMFMA(a4[3], bg[3 * PH], c);
        }
        acc[ti] = c;
      }
    }
    __syncthreads();   // every wave has read the old plane
#pragma unroll
    for (int ti = 0; ti < DT_MAXT; ++ti) {
      const int t = wave + DT_NW * ti;
      if (t < ntile)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float x = fminf(fmaxf(acc[ti][r], 0.f), 1.f);
          Hs[(16 * (t / CT) + 4 * kq + r) * PH + 16 * (t % CT) + m] = x;
          sum[ti][r] += x;
        }
    }
    __syncthreads();
  }
#pragma unroll
  for (int ti = 0; ti < DT_MAXT; ++ti) {
    const int t = wave + DT_NW * ti;
    if (t < ntile)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * (t / CT) + 4 * kq + r, col = c0 + 16 * (t % CT) + m;
        if (row < N && col < N) target[((size_t)b * N + row) * N + col] = (uint8_t)(int)fminf(fmaxf(rintf(sum[ti][r]), 0.f), 255.f);
      }
  }
}

// =================================== host ===================================
#define DT_MAX_N 192   // the adjacency ([R16][R16 + 4] fp32) plus one column tile of a hop ([R16][16], unpadded at this size) fill the 160 KB of LDS

extern "C" int egt_distance_target(const float* adj, int32_t B, int32_t N, int32_t T, uint8_t* target, void* stream) {
  if (B < 1 || N < 1 || (long)B * N * N > 2147483647L) EGT_FAIL(EGT_E_SHAPE, "distance target: B, N >= 1 and B*N*N inside 32 bits (got B=%d N=%d)", B, N);
  if (N > DT_MAX_N) EGT_FAIL(EGT_E_SHAPE, "distance target: N <= %d (the graph's adjacency stays in LDS); got %d", DT_MAX_N, N);
  if (T < 1 || T > 255) EGT_FAIL(EGT_E_SHAPE, "distance target: 1 <= T <= 255 (got %d)", T);
  if (!adj || !target) EGT_FAIL(EGT_E_NULL, "adj/target is NULL");
  const int RT = (N + 15) / 16, R16 = RT * 16;
  int ct = (int)((long)RT * B / 256);
  ct = ct < 1 ? 1 : (ct > RT ? RT : ct);
  int hp = 4;
  auto lds_of = [&](int c) { return (size_t)(R16 * (R16 + 4) + R16 * (16 * c + hp)) * sizeof(float); };
  while (ct > 1 && (RT * ct > DT_NW * DT_MAXT || lds_of(ct) > 160 * 1024)) --ct;
  if (lds_of(ct) > 160 * 1024) hp = 0;   // N in 177..192: one unpadded column tile (165888 bytes with the padding, 162816 without)
                                          // (PH = 16 then: the hop-1 load and the B-operand reads bg[k * PH] hit LDS bank conflicts; B = 64, T = 8
                                          //  on one MI355X: 151 us at N = 176, 187 us at N = 192 -- 1.24x for 1.30x the MFMA work, so they do not show)
  if (RT * ct > DT_NW * DT_MAXT || lds_of(ct) > 160 * 1024) EGT_FAIL(EGT_E_SHAPE, "distance target: N=%d does not fit", N);
  const int NB = (RT + ct - 1) / ct;
  EGT_MAX_LDS_ONCE(k_dist_target);
  EGT_LAUNCH("k_dist_target", k_dist_target, dim3((unsigned)(B * NB)), dim3(DT_NW * 64), lds_of(ct), (hipStream_t)stream, adj, target,
             N, T, NB, ct, hp);
  EGT_HIP_LAUNCH_CHECK("egt_distance_target");
  return EGT_OK;
}

// ---- what the two heads share on the host: one shape of the MLP, one block of the eight parameter pointers ----
struct EhShape {
  const char *who, *ln_flag;   // "edge head" / "node head" (the prefix of every message) and the name of its LayerNorm flag
  int width, det, M0, M1, C, act, ln;
  float eps;
};
struct EhParams { float* p[8]; };   // gamma, beta, W0, b0, W1, b1, Wt, bt: the order of egt_head_params and of egt_node_head_params
static_assert(sizeof(egt_head_params) == sizeof(EhParams) && sizeof(egt_node_head_params) == sizeof(EhParams),
              "both parameter structs are eight pointers");

static int eh_mlp_check(const char* who, int M0, int M1, int C, int act) {
  if (!((M0 == 24 && M1 == 12) || (M0 == 32 && M1 == 16)))
    EGT_FAIL(EGT_E_SHAPE, "%s covers (M0, M1) in {(24,12), (32,16)}: model widths 48 / 64 (got %d, %d)", who, M0, M1);
  if (C < 2 || C > 16) EGT_FAIL(EGT_E_SHAPE, "%s covers 2 <= C <= 16 classes (got %d)", who, C);
  if (act != EGT_ACT_ELU && act != EGT_ACT_RELU)
    EGT_FAIL(EGT_E_SHAPE, "%s activation is EGT_ACT_ELU or EGT_ACT_RELU (got %d)", who, act);
  return EGT_OK;
}
// P: egt_head_params or egt_node_head_params (`what`: "params" / "grads")
template <typename P>
static int eh_params(const EhShape& s, const P* p, const char* what, EhParams* out) {
  if (!p) EGT_FAIL(EGT_E_NULL, "%s: %s is NULL", s.who, what);
  memcpy(out, p, sizeof(EhParams));
  if (s.ln && (!out->p[0] || !out->p[1])) EGT_FAIL(EGT_E_NULL, "%s: %s set but %s gamma/beta is NULL", s.who, s.ln_flag, what);
  for (int k = 2; k < 8; ++k)
    if (!out->p[k]) EGT_FAIL(EGT_E_NULL, "%s: a kernel / bias pointer of %s is NULL", s.who, what);
  return EGT_OK;
}
static void eh_prep(const char* label, const EhShape& s, const EhParams& P, float* img, hipStream_t st) {
  float* const* p = P.p;
  EGT_LAUNCH(label, k_edge_head_prep, dim3(1), dim3(64), 0, st, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], img, s.width,
             16 * s.det, s.M0, s.M1, s.C, s.ln);
}
// the workgroups' gradient partials -> the eight gradients of G
static void eh_reduce_finish(const char* label, const EhShape& s, const EhParams& P, const EhParams& G, const float* part, float* red,
                             int nwg, hipStream_t st) {
  const int PG = eh_pg(s.det);
  float* const* g = G.p;
  EGT_LAUNCH(label, k_edge_head_reduce, dim3((unsigned)((PG + 63) / 64)), dim3(256), 0, st, part, red, nwg, PG);
  EGT_LAUNCH(label, k_edge_head_finish, dim3(1), dim3(256), 0, st, red, P.p[0], P.p[1], P.p[2],
             g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], s.width, 16 * s.det, s.M0, s.M1, s.C, s.ln);
}

// =================================== edge head: host ===================================
static int head_check(const egt_head_desc* d) {
  if (!d) EGT_FAIL(EGT_E_NULL, "desc is NULL");
  if ((d->flags & ~(int32_t)EGT_EH_LAYERNORM) != 0 || d->reserved != 0)
    EGT_FAIL(EGT_E_FLAGS, "edge head: unknown flag bits 0x%x / reserved %d", (unsigned)d->flags, d->reserved);
  if (d->dtype != EGT_F32 && d->dtype != EGT_BF16) EGT_FAIL(EGT_E_DTYPE, "edge head: e is fp32 or bf16 (dtype %d)", d->dtype);
  if (d->B < 1 || d->N < 1 || (long)d->B * d->N * d->N > 2147483647L)
    EGT_FAIL(EGT_E_SHAPE, "edge head: B, N >= 1 and B*N*N inside 32-bit indexing (B=%d N=%d)", d->B, d->N);
  if (!(d->De == 8 || d->De == 16 || d->De == 32 || d->De == 48 || d->De == 64))
    EGT_FAIL(EGT_E_SHAPE, "edge head covers De in {8,16,32,48,64} (got %d)", d->De);
  return eh_mlp_check("edge head", d->M0, d->M1, d->C, d->activation);
}
static EhShape head_shape(const egt_head_desc* d) {
  return {"edge head", "EGT_EH_LAYERNORM", d->De, eh_det(d->De), d->M0, d->M1, d->C, d->activation,
          (d->flags & EGT_EH_LAYERNORM) ? 1 : 0, d->ln_eps};
}
extern "C" int egt_edge_head_supported(const egt_head_desc* d) { return head_check(d) == EGT_OK ? 1 : 0; }

// workgroups per graph: about four workgroups per CU over the batch, at least 8 tiles each (the 13 KB weight image is
// loaded once per workgroup)
static int head_chunks(const egt_head_desc* d) {
  const int tpg = (d->N * d->N + 15) / 16;
  int g = 1024 / d->B;
  const int cap = tpg / 8;
  g = g > cap ? cap : g;
  return g < 1 ? 1 : g;
}
// workspace (floats): weight image | loss partials [B G] | gradient partials [B G][PG] | reduced gradients [PG]
extern "C" size_t egt_edge_head_workspace_bytes(const egt_head_desc* d) {
  if (head_check(d) != EGT_OK) return 0;
  const int det = eh_det(d->De);
  const size_t nwg = (size_t)d->B * head_chunks(d);
  return sizeof(float) * ((size_t)eh_img(det) + nwg + nwg * eh_pg(det) + eh_pg(det));
}

template <int DET, typename T, bool BWD>
static void head_launch(const egt_head_desc* d, const EhShape& s, const void* e, const uint8_t* target, const float* img,
                        const float* sg, void* de, float* loss_part, float* part, hipStream_t st) {
  const int G = head_chunks(d), tpg = (d->N * d->N + 15) / 16, chunk = (tpg + G - 1) / G;
  EGT_LAUNCH(BWD ? "k_edge_head_bwd" : "k_edge_head_fwd", (k_edge_head<DET, T, BWD>), dim3((unsigned)(d->B * G)), dim3(EH_NW * 64),
             0, st, (const T*)e, target, img, sg, (T*)de, loss_part, part, d->N, G, chunk, s.width, s.C, s.act, s.ln, s.eps);
}
template <bool BWD>
static void head_dispatch(const egt_head_desc* d, const EhShape& s, const void* e, const uint8_t* target, const float* img,
                          const float* sg, void* de, float* loss_part, float* part, hipStream_t st) {
  const bool bf = d->dtype == EGT_BF16;
  switch (s.det) {
#define EH_CASE(DET_)                                                                                 \
  case DET_:                                                                                          \
    if (bf) head_launch<DET_, uint16_t, BWD>(d, s, e, target, img, sg, de, loss_part, part, st);       \
    else head_launch<DET_, float, BWD>(d, s, e, target, img, sg, de, loss_part, part, st);             \
    break;
    EH_CASE(1) EH_CASE(2) EH_CASE(3) EH_CASE(4)
#undef EH_CASE
  }
}

extern "C" int egt_edge_head_fwd(const egt_head_desc* d, const egt_head_params* params, const void* e, const uint8_t* target,
                                 float* per_graph_loss, void* workspace, void* stream) {
  int rc = head_check(d);
  if (rc) return rc;
  const EhShape s = head_shape(d);
  EhParams P;
  if ((rc = eh_params(s, params, "params", &P))) return rc;
  if (!e || !target || !per_graph_loss || !workspace) EGT_FAIL(EGT_E_NULL, "edge head: e/target/per_graph_loss/workspace is NULL");
  hipStream_t st = (hipStream_t)stream;
  const int G = head_chunks(d);
  float* img = (float*)workspace;
  float* loss_part = img + eh_img(s.det);
  eh_prep("k_edge_head_prep", s, P, img, st);
  head_dispatch<false>(d, s, e, target, img, nullptr, nullptr, loss_part, nullptr, st);
  EGT_LAUNCH("k_edge_head_finish", k_edge_head_loss, dim3((unsigned)((d->B + 63) / 64)), dim3(64), 0, st, (const float*)loss_part,
             per_graph_loss, d->B, G);
  EGT_HIP_LAUNCH_CHECK("egt_edge_head_fwd");
  return EGT_OK;
}

extern "C" int egt_edge_head_bwd(const egt_head_desc* d, const egt_head_params* params, const void* e, const uint8_t* target,
                                 const float* d_per_graph, void* d_e, const egt_head_params* grads, void* workspace,
                                 void* stream) {
  int rc = head_check(d);
  if (rc) return rc;
  const EhShape s = head_shape(d);
  EhParams P, Gr;
  if ((rc = eh_params(s, params, "params", &P))) return rc;
  if ((rc = eh_params(s, grads, "grads", &Gr))) return rc;
  if (!e || !target || !d_per_graph || !d_e || !workspace) EGT_FAIL(EGT_E_NULL, "edge head: e/target/d_per_graph/d_e/workspace is NULL");
  hipStream_t st = (hipStream_t)stream;
  const int nwg = d->B * head_chunks(d);
  float* img = (float*)workspace;
  float* part = img + eh_img(s.det) + nwg;
  float* red = part + (size_t)nwg * eh_pg(s.det);
  eh_prep("k_edge_head_prep", s, P, img, st);
  head_dispatch<true>(d, s, e, target, img, d_per_graph, d_e, nullptr, part, st);
  eh_reduce_finish("k_edge_head_finish", s, P, Gr, part, red, nwg, st);
  EGT_HIP_LAUNCH_CHECK("egt_edge_head_bwd");
  return EGT_OK;
}

// =================================== node-classification head: host ===================================
static int node_head_check(const egt_node_head_desc* d) {
  if (!d) EGT_FAIL(EGT_E_NULL, "desc is NULL");
  if ((d->flags & ~(int32_t)EGT_NH_LAYERNORM) != 0 || d->reserved != 0)
    EGT_FAIL(EGT_E_FLAGS, "node head: unknown flag bits 0x%x / reserved %d", (unsigned)d->flags, d->reserved);
  if (d->B < 1 || d->N < 1 || (long)d->B * d->N > 2147483647L)
    EGT_FAIL(EGT_E_SHAPE, "node head: B, N >= 1 and B*N inside 32-bit indexing (B=%d N=%d)", d->B, d->N);
  if (!(d->W == 16 || d->W == 32 || d->W == 48 || d->W == 64))
    EGT_FAIL(EGT_E_SHAPE, "node head covers W in {16,32,48,64} (got %d)", d->W);
  return eh_mlp_check("node head", d->M0, d->M1, d->C, d->activation);
}
static EhShape node_head_shape(const egt_node_head_desc* d) {
  return {"node head", "EGT_NH_LAYERNORM", d->W, d->W / 16, d->M0, d->M1, d->C, d->activation,
          (d->flags & EGT_NH_LAYERNORM) ? 1 : 0, d->ln_eps};
}
extern "C" int egt_node_head_supported(const egt_node_head_desc* d) { return node_head_check(d) == EGT_OK ? 1 : 0; }

// workgroups: one 16-row tile per wave and pass, so at least 4 tiles each; at most 1024 (the weight image is loaded once per
// workgroup, and every workgroup leaves one gradient partial)
static int node_head_tiles(const egt_node_head_desc* d) { return (int)(((long)d->B * d->N + 15) / 16); }
static int node_head_groups(const egt_node_head_desc* d) {
  int g = node_head_tiles(d) / EH_NW;
  g = g > 1024 ? 1024 : g;
  return g < 1 ? 1 : g;
}
// workspace (floats): weight image | stat partials [G][3] | gradient partials [G][PG] | reduced gradients [PG]
extern "C" size_t egt_node_head_workspace_bytes(const egt_node_head_desc* d) {
  if (node_head_check(d) != EGT_OK) return 0;
  const int det = d->W / 16;
  const size_t G = (size_t)node_head_groups(d);
  return sizeof(float) * ((size_t)eh_img(det) + 3 * G + G * eh_pg(det) + eh_pg(det));
}

template <bool BWD>
static void node_head_dispatch(const egt_node_head_desc* d, const EhShape& s, const float* h, const int32_t* target,
                               const uint8_t* mask, const float* cw, const float* img, const float* sg, float* dh, float* stat_part,
                               float* part, hipStream_t st) {
  const int G = node_head_groups(d), tiles = node_head_tiles(d), chunk = (tiles + G - 1) / G;
  const int R = d->B * d->N;
  switch (s.det) {
#define NH_CASE(DET_)                                                                                                          \
  case DET_:                                                                                                                   \
    EGT_LAUNCH(BWD ? "k_node_head_bwd" : "k_node_head_fwd", (k_node_head<DET_, BWD>), dim3((unsigned)G), dim3(EH_NW * 64), 0, st, \
               h, target, mask, cw, img, sg, dh, stat_part, part, R, chunk, s.width, s.C, s.act, s.ln, s.eps);                  \
    break;
    NH_CASE(1) NH_CASE(2) NH_CASE(3) NH_CASE(4)
#undef NH_CASE
  }
}

extern "C" int egt_node_head_fwd(const egt_node_head_desc* d, const egt_node_head_params* params, const float* h,
                                 const int32_t* target, const uint8_t* mask, const float* class_weights, float* stats,
                                 void* workspace, void* stream) {
  int rc = node_head_check(d);
  if (rc) return rc;
  const EhShape s = node_head_shape(d);
  EhParams P;
  if ((rc = eh_params(s, params, "params", &P))) return rc;
  if (!h || !target || !mask || !class_weights || !stats || !workspace)
    EGT_FAIL(EGT_E_NULL, "node head: h/target/mask/class_weights/stats/workspace is NULL");
  hipStream_t st = (hipStream_t)stream;
  float* img = (float*)workspace;
  float* stat_part = img + eh_img(s.det);
  eh_prep("k_node_head_prep", s, P, img, st);
  node_head_dispatch<false>(d, s, h, target, mask, class_weights, img, nullptr, nullptr, stat_part, nullptr, st);
  EGT_LAUNCH("k_node_head_finish", k_node_head_stats, dim3(1), dim3(64), 0, st, (const float*)stat_part, stats, node_head_groups(d));
  EGT_HIP_LAUNCH_CHECK("egt_node_head_fwd");
  return EGT_OK;
}

extern "C" int egt_node_head_bwd(const egt_node_head_desc* d, const egt_node_head_params* params, const float* h,
                                 const int32_t* target, const uint8_t* mask, const float* class_weights, const float* d_loss,
                                 float* d_h, const egt_node_head_params* grads, void* workspace, void* stream) {
  int rc = node_head_check(d);
  if (rc) return rc;
  const EhShape s = node_head_shape(d);
  EhParams P, Gr;
  if ((rc = eh_params(s, params, "params", &P))) return rc;
  if ((rc = eh_params(s, grads, "grads", &Gr))) return rc;
  if (!h || !target || !mask || !class_weights || !d_loss || !d_h || !workspace)
    EGT_FAIL(EGT_E_NULL, "node head: h/target/mask/class_weights/d_loss/d_h/workspace is NULL");
  hipStream_t st = (hipStream_t)stream;
  const int G = node_head_groups(d);
  float* img = (float*)workspace;
  float* part = img + eh_img(s.det) + 3 * (size_t)G;
  float* red = part + (size_t)G * eh_pg(s.det);
  eh_prep("k_node_head_prep", s, P, img, st);
  node_head_dispatch<true>(d, s, h, target, mask, class_weights, img, d_loss, d_h, nullptr, part, st);
  eh_reduce_finish("k_node_head_finish", s, P, Gr, part, red, G, st);
  EGT_HIP_LAUNCH_CHECK("egt_node_head_bwd");
  return EGT_OK;
}
