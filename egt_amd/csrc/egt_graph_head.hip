// Graph-level readout of the ZINC / ZINC-full / CIFAR10 / MNIST models and its loss (include/egt_amd.h, "graph-level readout
// head"):
//   x      = node_norm_final(h)                                              h [B,N',W] fp32, N' = nv + N
//   pooled = nv == 0 ? masked mean of x over the nodes                       lib/models/zinc/dc.py:109
//                    : the nv virtual rows of x, flattened                   zinc/dc.py:105-108
//   y      = Dense_t(act(Dense_1(act(Dense_0(pooled)))))                     max(nv,1) W -> M0 -> M1 -> C
//   stats  = MAE { sum |y - t|, 0, B C }  /  XENT { sum CE, sum [argmax y == t], B }
// One workgroup per graph and direction.  A 16-lane row of a wave owns one node row (float4 per lane, the lanes past W idle), so
// the LayerNorm moments are DPP reductions inside the row and a wave takes four node rows per pass; the pooled sum stays in
// registers and meets the other rows / waves in one fixed-order exchange.  The MLP of the graph's ONE pooled row follows in the
// same launch from LDS (a 16-row MFMA tile would be 15/16 padding).  The backward recomputes all of it, pushes the gradient
// down to the pooled row, writes d_h in a second pass over the graph's rows and leaves one record per graph (the MLP's
// activations, their gradients, the gamma / beta partials); k_graph_head_wgrad sums the records over the graphs in a fixed
// order, one thread per parameter element.  No atomics anywhere: two runs are bitwise equal.
#include "egt_common.h"
#include <cstring>

#define GH_NW 4                   // waves per workgroup
#define GH_NT (GH_NW * 64)
#define GH_MAX_NV 4               // virtual rows the readout flattens
#define GH_KMAX (GH_MAX_NV * 64)  // widest Dense_0 input
#define GH_PARTS (GH_NT / 32)     // slices of Dense_0's input dimension

struct GhParams { float* p[8]; };   // gamma, beta, W0, b0, W1, b1, Wt, bt: the order of egt_node_head_params
static_assert(sizeof(egt_node_head_params) == sizeof(GhParams), "the parameter struct is eight pointers");

struct GhGeo {
  int NP, W, nv, K, M0, M1, C, loss, act, ln;
  float eps;
};

__device__ __forceinline__ float gh_act(float x, int act) { return act == EGT_ACT_ELU ? (x > 0.f ? x : expm1f(x)) : fmaxf(x, 0.f); }
// derivative of the activation at the pre-activation a
__device__ __forceinline__ float gh_dact(float a, int act) { return a > 0.f ? 1.f : (act == EGT_ACT_ELU ? expf(a) : 0.f); }
__device__ __forceinline__ float gh_sum4(float4 v) { return (v.x + v.y) + (v.z + v.w); }
__device__ __forceinline__ float gh_wave_sum4(float v) { return sum_xor32(sum_xor16(v)); }   // over the four 16-lane rows of a wave

// LayerNorm statistics of one node row spread over a 16-lane row (idle lanes hold zeros and stay zero): x -> (x - mean) rstd
__device__ __forceinline__ float4 gh_ln(float4 x, bool col, float invW, float eps, float& rstd) {
  const float mean = row_sum16(gh_sum4(x)) * invW;
  float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
  if (col) d = make_float4(x.x - mean, x.y - mean, x.z - mean, x.w - mean);
  const float var = row_sum16((d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w)) * invW;
  rstd = 1.0f / sqrtf(var + eps);
  return make_float4(d.x * rstd, d.y * rstd, d.z * rstd, d.w * rstd);
}
// four consecutive floats of a parameter (element alignment only: scalar loads)
__device__ __forceinline__ float4 gh_ld4(const float* p) { return make_float4(p[0], p[1], p[2], p[3]); }

// record of one graph for k_graph_head_wgrad (floats): x0 [K] | x1 [M0] | x2 [M1] | da1 [M0] | da2 [M1] | dy [C] | dgamma [W] | dbeta [W]
__host__ __device__ inline int gh_stride(int K, int W, int M0, int M1, int C) { return K + 2 * M0 + 2 * M1 + C + 2 * W; }

template <bool BWD>
__global__ void __launch_bounds__(GH_NT) k_graph_head(const float* __restrict__ h, const void* __restrict__ target,
                                                      const uint8_t* __restrict__ mask, const GhParams P,
                                                      const float* __restrict__ d_loss, float* __restrict__ pred,
                                                      float* __restrict__ d_h, float* __restrict__ loss_part,
                                                      float* __restrict__ rec_all, const GhGeo g) {
  __shared__ __attribute__((aligned(16))) float s_pw[GH_NW][64];
  __shared__ __attribute__((aligned(16))) float s_pb[GH_NW][64];
  __shared__ __attribute__((aligned(16))) float s_x0[GH_KMAX];
  __shared__ __attribute__((aligned(16))) float s_dx0[GH_KMAX];
  __shared__ float s_cnt[GH_NW];
  __shared__ float s_red[GH_PARTS][32];
  __shared__ float s_a1[32], s_x1[32], s_da1[32];
  __shared__ float s_a2[16], s_x2[16], s_da2[16], s_y[16], s_dy[16];

  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, sub = lane >> 4, q = lane & 15;
  const int W = g.W, NP = g.NP, nv = g.nv, K = g.K, M0 = g.M0, M1 = g.M1, C = g.C;
  const bool col = 4 * q < W;
  const float invW = 1.0f / (float)W;
  const float* hb = h + (size_t)b * NP * W;
  const uint8_t* mb = mask + (size_t)b * NP;
  const float *W0 = P.p[2], *b0 = P.p[3], *W1 = P.p[4], *b1 = P.p[5], *Wt = P.p[6], *bt = P.p[7];

  float4 gam = make_float4(1.f, 1.f, 1.f, 1.f), bet = make_float4(0.f, 0.f, 0.f, 0.f);
  if (g.ln && col) { gam = gh_ld4(P.p[0] + 4 * q); bet = gh_ld4(P.p[1] + 4 * q); }

  // ---- pass 1: node_norm_final and the pooling ----
  const int npool = nv > 0 ? nv : NP;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  float cnt = 0.f;
  for (int r0 = wave * 4; r0 < npool; r0 += GH_NW * 4) {
    const int r = r0 + sub;
    const bool live = r < npool && (nv > 0 || mb[r] != 0);      // a masked row is never loaded
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live && col) x = *reinterpret_cast<const float4*>(hb + (size_t)r * W + 4 * q);
    if (g.ln) {
      float rstd;
      const float4 xh = gh_ln(x, col, invW, g.eps, rstd);
      x = make_float4(xh.x * gam.x + bet.x, xh.y * gam.y + bet.y, xh.z * gam.z + bet.z, xh.w * gam.w + bet.w);
    }
    if (nv > 0) {
      if (live && col) *reinterpret_cast<float4*>(&s_x0[r * W + 4 * q]) = x;
    } else if (live) {
      acc.x += x.x; acc.y += x.y; acc.z += x.z; acc.w += x.w;
      cnt += 1.f;
    }
  }
  if (nv == 0) {
    acc.x = gh_wave_sum4(acc.x); acc.y = gh_wave_sum4(acc.y); acc.z = gh_wave_sum4(acc.z); acc.w = gh_wave_sum4(acc.w);
    cnt = gh_wave_sum4(cnt);
    if (sub == 0 && col) *reinterpret_cast<float4*>(&s_pw[wave][4 * q]) = acc;
    if (lane == 0) s_cnt[wave] = cnt;
  }
  __syncthreads();
  float real = 1.f;
  if (nv == 0) {
    real = ((s_cnt[0] + s_cnt[1]) + s_cnt[2]) + s_cnt[3];
    if (tid < W) s_x0[tid] = (((s_pw[0][tid] + s_pw[1][tid]) + s_pw[2][tid]) + s_pw[3][tid]) / real;
    __syncthreads();
  }

  // ---- the MLP of the pooled row ----
  {
    const int j = tid & 31, part = tid >> 5;
    float a = 0.f;
    if (j < M0)
      for (int k = part; k < K; k += GH_PARTS) a = fmaf(s_x0[k], W0[k * M0 + j], a);
    s_red[part][j] = a;
  }
  __syncthreads();
  if (tid < M0) {
    float a = b0[tid];
    for (int p = 0; p < GH_PARTS; ++p) a += s_red[p][tid];
    s_a1[tid] = a;
    s_x1[tid] = gh_act(a, g.act);
  }
  __syncthreads();
  if (tid < M1) {
    float a = b1[tid];
    for (int k = 0; k < M0; ++k) a = fmaf(s_x1[k], W1[k * M1 + tid], a);
    s_a2[tid] = a;
    s_x2[tid] = gh_act(a, g.act);
  }
  __syncthreads();
  if (tid < C) {
    float a = bt[tid];
    for (int k = 0; k < M1; ++k) a = fmaf(s_x2[k], Wt[k * C + tid], a);
    s_y[tid] = a;
    if (!BWD) pred[(size_t)b * C + tid] = a;
  }
  __syncthreads();

  // ---- loss of the graph (C <= 16 values: one thread) ----
  if (tid == 0) {
    const float up = BWD ? d_loss[0] : 0.f;
    float l = 0.f, hit = 0.f;
    if (g.loss == EGT_GH_MAE) {
      const float* t = reinterpret_cast<const float*>(target) + (size_t)b * C;
      for (int c = 0; c < C; ++c) {
        const float d = s_y[c] - t[c];
        l += fabsf(d);
        if (BWD) s_dy[c] = d > 0.f ? up : (d < 0.f ? -up : 0.f);
      }
    } else {
      const int t = reinterpret_cast<const int32_t*>(target)[b];
      const int tc = t < 0 ? 0 : (t >= C ? C - 1 : t);
      float m = s_y[0];
      int am = 0;
      for (int c = 1; c < C; ++c)
        if (s_y[c] > m) { m = s_y[c]; am = c; }      // strict: the lowest class wins a tie
      float se = 0.f;
      for (int c = 0; c < C; ++c) se += expf(s_y[c] - m);
      l = (m + logf(se)) - s_y[tc];
      hit = am == t ? 1.f : 0.f;
      if (BWD)
        for (int c = 0; c < C; ++c) s_dy[c] = up * (expf(s_y[c] - m) / se - (c == tc ? 1.f : 0.f));
    }
    if (!BWD) { loss_part[2 * (size_t)b] = l; loss_part[2 * (size_t)b + 1] = hit; }
  }
  if (!BWD) return;

  // ---- backward of the MLP ----
  __syncthreads();
  if (tid < M1) {
    float d = 0.f;
    for (int c = 0; c < C; ++c) d = fmaf(Wt[tid * C + c], s_dy[c], d);
    s_da2[tid] = d * gh_dact(s_a2[tid], g.act);
  }
  __syncthreads();
  if (tid < M0) {
    float d = 0.f;
    for (int j = 0; j < M1; ++j) d = fmaf(W1[tid * M1 + j], s_da2[j], d);
    s_da1[tid] = d * gh_dact(s_a1[tid], g.act);
  }
  __syncthreads();
  float* rec = rec_all + (size_t)b * gh_stride(K, W, M0, M1, C);
  for (int k = tid; k < K; k += GH_NT) {
    float d = 0.f;
    for (int j = 0; j < M0; ++j) d = fmaf(W0[k * M0 + j], s_da1[j], d);
    s_dx0[k] = d;
    rec[k] = s_x0[k];
  }
  if (tid < M0) { rec[K + tid] = s_x1[tid]; rec[K + M0 + M1 + tid] = s_da1[tid]; }
  if (tid < M1) { rec[K + M0 + tid] = s_x2[tid]; rec[K + 2 * M0 + M1 + tid] = s_da2[tid]; }
  if (tid < C) rec[K + 2 * M0 + 2 * M1 + tid] = s_dy[tid];
  __syncthreads();

  // ---- pass 2: d_h of every row of the graph (exact zeros where no gradient arrives), gamma / beta partials ----
  const float inv = nv > 0 ? 1.f : 1.0f / real;
  float4 gg = make_float4(0.f, 0.f, 0.f, 0.f), gb = make_float4(0.f, 0.f, 0.f, 0.f);
  float* dhb = d_h + (size_t)b * NP * W;
  for (int r0 = wave * 4; r0 < NP; r0 += GH_NW * 4) {
    const int r = r0 + sub;
    const bool inside = r < NP;
    const bool live = inside && (nv > 0 ? r < nv : mb[r] != 0);
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f), dx = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live && col) {
      x = *reinterpret_cast<const float4*>(hb + (size_t)r * W + 4 * q);
      const float4 s = *reinterpret_cast<const float4*>(&s_dx0[(nv > 0 ? r * W : 0) + 4 * q]);
      dx = make_float4(s.x * inv, s.y * inv, s.z * inv, s.w * inv);
    }
    float4 dh = dx;
    if (g.ln) {
      float rstd;
      const float4 xh = gh_ln(x, col, invW, g.eps, rstd);
      const float4 dxh = make_float4(dx.x * gam.x, dx.y * gam.y, dx.z * gam.z, dx.w * gam.w);
      const float m1 = row_sum16(gh_sum4(dxh)) * invW;
      const float m2 = row_sum16((dxh.x * xh.x + dxh.y * xh.y) + (dxh.z * xh.z + dxh.w * xh.w)) * invW;
      dh = make_float4(rstd * (dxh.x - m1 - xh.x * m2), rstd * (dxh.y - m1 - xh.y * m2), rstd * (dxh.z - m1 - xh.z * m2),
                       rstd * (dxh.w - m1 - xh.w * m2));
      gg.x += dx.x * xh.x; gg.y += dx.y * xh.y; gg.z += dx.z * xh.z; gg.w += dx.w * xh.w;
      gb.x += dx.x; gb.y += dx.y; gb.z += dx.z; gb.w += dx.w;
    }
    if (!live) dh = make_float4(0.f, 0.f, 0.f, 0.f);
    if (inside && col) *reinterpret_cast<float4*>(dhb + (size_t)r * W + 4 * q) = dh;
  }
  if (g.ln) {
    gg.x = gh_wave_sum4(gg.x); gg.y = gh_wave_sum4(gg.y); gg.z = gh_wave_sum4(gg.z); gg.w = gh_wave_sum4(gg.w);
    gb.x = gh_wave_sum4(gb.x); gb.y = gh_wave_sum4(gb.y); gb.z = gh_wave_sum4(gb.z); gb.w = gh_wave_sum4(gb.w);
    if (sub == 0 && col) {
      *reinterpret_cast<float4*>(&s_pw[wave][4 * q]) = gg;
      *reinterpret_cast<float4*>(&s_pb[wave][4 * q]) = gb;
    }
    __syncthreads();
    if (tid < W) {
      float* rg = rec + K + 2 * M0 + 2 * M1 + C;
      rg[tid] = ((s_pw[0][tid] + s_pw[1][tid]) + s_pw[2][tid]) + s_pw[3][tid];
      rg[W + tid] = ((s_pb[0][tid] + s_pb[1][tid]) + s_pb[2][tid]) + s_pb[3][tid];
    }
  }
}

// stats = { sum_b loss, sum_b hit, count }: one wave, graphs strided over the lanes, then a fixed butterfly
__global__ void __launch_bounds__(64) k_graph_head_stats(const float* __restrict__ loss_part, float* __restrict__ stats, int B,
                                                         float count) {
  float l = 0.f, hit = 0.f;
  for (int b = threadIdx.x; b < B; b += 64) { l += loss_part[2 * (size_t)b]; hit += loss_part[2 * (size_t)b + 1]; }
  l = gh_wave_sum4(row_sum16(l));
  hit = gh_wave_sum4(row_sum16(hit));
  if (threadIdx.x == 0) { stats[0] = l; stats[1] = hit; stats[2] = count; }
}

// The eight parameter gradients from the graphs' records: one thread per element, the graphs summed in index order (four
// interleaved chains, combined in a fixed order).
__device__ __forceinline__ float gh_dot_b(const float* __restrict__ a, const float* __restrict__ c, int B, int stride) {
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int b = 0;
  for (; b + 4 <= B; b += 4) {
    const size_t o = (size_t)b * stride;
    s0 = fmaf(a[o], c ? c[o] : 1.f, s0);
    s1 = fmaf(a[o + stride], c ? c[o + stride] : 1.f, s1);
    s2 = fmaf(a[o + 2 * (size_t)stride], c ? c[o + 2 * (size_t)stride] : 1.f, s2);
    s3 = fmaf(a[o + 3 * (size_t)stride], c ? c[o + 3 * (size_t)stride] : 1.f, s3);
  }
  for (; b < B; ++b) {
    const size_t o = (size_t)b * stride;
    s0 = fmaf(a[o], c ? c[o] : 1.f, s0);
  }
  return (s0 + s1) + (s2 + s3);
}
__global__ void __launch_bounds__(256) k_graph_head_wgrad(const float* __restrict__ rec, const GhParams G, int B, int K, int W, int M0,
                                                          int M1, int C, int ln) {
  const int stride = gh_stride(K, W, M0, M1, C);
  const int oX1 = K, oX2 = K + M0, oA1 = K + M0 + M1, oA2 = K + 2 * M0 + M1, oDY = K + 2 * M0 + 2 * M1, oG = oDY + C;
  int i = blockIdx.x * 256 + threadIdx.x;
  if (i < K * M0) { G.p[2][i] = gh_dot_b(rec + i / M0, rec + oA1 + i % M0, B, stride); return; }
  i -= K * M0;
  if (i < M0) { G.p[3][i] = gh_dot_b(rec + oA1 + i, nullptr, B, stride); return; }
  i -= M0;
  if (i < M0 * M1) { G.p[4][i] = gh_dot_b(rec + oX1 + i / M1, rec + oA2 + i % M1, B, stride); return; }
  i -= M0 * M1;
  if (i < M1) { G.p[5][i] = gh_dot_b(rec + oA2 + i, nullptr, B, stride); return; }
  i -= M1;
  if (i < M1 * C) { G.p[6][i] = gh_dot_b(rec + oX2 + i / C, rec + oDY + i % C, B, stride); return; }
  i -= M1 * C;
  if (i < C) { G.p[7][i] = gh_dot_b(rec + oDY + i, nullptr, B, stride); return; }
  i -= C;
  if (ln && i < 2 * W) G.p[i < W ? 0 : 1][i < W ? i : i - W] = gh_dot_b(rec + oG + i, nullptr, B, stride);
}
static inline int gh_wgrad_elems(int K, int W, int M0, int M1, int C, int ln) {
  return K * M0 + M0 + M0 * M1 + M1 + M1 * C + C + (ln ? 2 * W : 0);
}

// =================================== host ===================================
static int graph_head_check(const egt_graph_head_desc* d) {
  if (!d) EGT_FAIL(EGT_E_NULL, "desc is NULL");
  if ((d->flags & ~(int32_t)EGT_GH_LAYERNORM) != 0 || d->reserved != 0)
    EGT_FAIL(EGT_E_FLAGS, "graph head: unknown flag bits 0x%x / reserved %d", (unsigned)d->flags, d->reserved);
  if (d->loss != EGT_GH_MAE && d->loss != EGT_GH_XENT)
    EGT_FAIL(EGT_E_FLAGS, "graph head: loss is EGT_GH_MAE or EGT_GH_XENT (got %d)", d->loss);
  if (d->nv < 0 || d->nv > GH_MAX_NV) EGT_FAIL(EGT_E_SHAPE, "graph head covers 0 <= nv <= %d virtual nodes (got %d)", GH_MAX_NV, d->nv);
  if (d->B < 1 || d->N < 1 || (long)d->B * ((long)d->nv + d->N) > 2147483647L)
    EGT_FAIL(EGT_E_SHAPE, "graph head: B, N >= 1 and B*(nv+N) inside 32-bit indexing (B=%d N=%d nv=%d)", d->B, d->N, d->nv);
  if (!(d->W == 48 || d->W == 64)) EGT_FAIL(EGT_E_SHAPE, "graph head covers W in {48,64} (got %d)", d->W);
  if (!((d->M0 == 24 && d->M1 == 12) || (d->M0 == 32 && d->M1 == 16)))
    EGT_FAIL(EGT_E_SHAPE, "graph head covers (M0, M1) in {(24,12), (32,16)}: model widths 48 / 64 (got %d, %d)", d->M0, d->M1);
  if (d->C < 1 || d->C > 16) EGT_FAIL(EGT_E_SHAPE, "graph head covers 1 <= C <= 16 outputs (got %d)", d->C);
  if (d->activation != EGT_ACT_ELU && d->activation != EGT_ACT_RELU)
    EGT_FAIL(EGT_E_SHAPE, "graph head activation is EGT_ACT_ELU or EGT_ACT_RELU (got %d)", d->activation);
  return EGT_OK;
}
static GhGeo graph_head_geo(const egt_graph_head_desc* d) {
  return {d->nv + d->N, d->W, d->nv, (d->nv > 0 ? d->nv : 1) * d->W, d->M0, d->M1, d->C, d->loss, d->activation,
          (d->flags & EGT_GH_LAYERNORM) ? 1 : 0, d->ln_eps};
}
static int graph_head_params(const GhGeo& g, const egt_node_head_params* p, const char* what, GhParams* out) {
  if (!p) EGT_FAIL(EGT_E_NULL, "graph head: %s is NULL", what);
  memcpy(out, p, sizeof(GhParams));
  if (g.ln && (!out->p[0] || !out->p[1])) EGT_FAIL(EGT_E_NULL, "graph head: EGT_GH_LAYERNORM set but %s gamma/beta is NULL", what);
  for (int k = 2; k < 8; ++k)
    if (!out->p[k]) EGT_FAIL(EGT_E_NULL, "graph head: a kernel / bias pointer of %s is NULL", what);
  return EGT_OK;
}
extern "C" int egt_graph_head_supported(const egt_graph_head_desc* d) { return graph_head_check(d) == EGT_OK ? 1 : 0; }

// workspace (floats): loss / hit of every graph [B][2] | the graphs' records [B][stride]
extern "C" size_t egt_graph_head_workspace_bytes(const egt_graph_head_desc* d) {
  if (graph_head_check(d) != EGT_OK) return 0;
  const GhGeo g = graph_head_geo(d);
  return sizeof(float) * ((size_t)d->B * 2 + (size_t)d->B * gh_stride(g.K, g.W, g.M0, g.M1, g.C));
}

extern "C" int egt_graph_head_fwd(const egt_graph_head_desc* d, const egt_node_head_params* params, const float* h,
                                  const void* target, const uint8_t* mask, float* stats, float* pred, void* workspace,
                                  void* stream) {
  int rc = graph_head_check(d);
  if (rc) return rc;
  const GhGeo g = graph_head_geo(d);
  GhParams P;
  if ((rc = graph_head_params(g, params, "params", &P))) return rc;
  if (!h || !target || !mask || !stats || !pred || !workspace)
    EGT_FAIL(EGT_E_NULL, "graph head: h/target/mask/stats/pred/workspace is NULL");
  hipStream_t st = (hipStream_t)stream;
  float* loss_part = (float*)workspace;
  EGT_LAUNCH("k_graph_head_fwd", (k_graph_head<false>), dim3((unsigned)d->B), dim3(GH_NT), 0, st, h, target, mask, P,
             (const float*)nullptr, pred, (float*)nullptr, loss_part, (float*)nullptr, g);
  EGT_LAUNCH("k_graph_head_finish", k_graph_head_stats, dim3(1), dim3(64), 0, st, (const float*)loss_part, stats, d->B,
             d->loss == EGT_GH_MAE ? (float)d->B * (float)d->C : (float)d->B);
  EGT_HIP_LAUNCH_CHECK("egt_graph_head_fwd");
  return EGT_OK;
}

extern "C" int egt_graph_head_bwd(const egt_graph_head_desc* d, const egt_node_head_params* params, const float* h,
                                  const void* target, const uint8_t* mask, const float* d_loss, float* d_h,
                                  const egt_node_head_params* grads, void* workspace, void* stream) {
  int rc = graph_head_check(d);
  if (rc) return rc;
  const GhGeo g = graph_head_geo(d);
  GhParams P, Gr;
  if ((rc = graph_head_params(g, params, "params", &P))) return rc;
  if ((rc = graph_head_params(g, grads, "grads", &Gr))) return rc;
  if (!h || !target || !mask || !d_loss || !d_h || !workspace)
    EGT_FAIL(EGT_E_NULL, "graph head: h/target/mask/d_loss/d_h/workspace is NULL");
  hipStream_t st = (hipStream_t)stream;
  float* rec = (float*)workspace + (size_t)d->B * 2;
  EGT_LAUNCH("k_graph_head_bwd", (k_graph_head<true>), dim3((unsigned)d->B), dim3(GH_NT), 0, st, h, target, mask, P, d_loss,
             (float*)nullptr, d_h, (float*)nullptr, rec, g);
  const int n = gh_wgrad_elems(g.K, g.W, g.M0, g.M1, g.C, g.ln);
  EGT_LAUNCH("k_graph_head_finish", k_graph_head_wgrad, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)rec, Gr,
             d->B, g.K, g.W, g.M0, g.M1, g.C, g.ln);
  EGT_HIP_LAUNCH_CHECK("egt_graph_head_bwd");
  return EGT_OK;
}
