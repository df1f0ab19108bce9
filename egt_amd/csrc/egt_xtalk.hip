// Edge side of the channel FFN with node<->edge cross-talk (node2edge_xtalk / edge2node_xtalk of the reference's
// transform_embeddings, lib/models/graph_xformer_model_base.py:227-324), for gfx950, ffn_multiplier 2, fp32, exact fp32 MFMAs:
//   pre = Dense_1(LayerNorm(e))                               [B,N,N,H], H = 2 De, no activation yet
//   pre = [ er (s_e) | ec (s_e) | tail (H - 2 s_e) ]
//   hn[b,n,c] = divide_no_nan( sum_i m[b,i] er[b,i,n,c] + sum_j m[b,j] ec[b,n,j,c], sum m[b,:] )      (edge -> node)
//   z = [ tail | hr[b,i,:] + hc[b,j,:] ]                      width K2 = H - 2 s_e + s_n              (node -> edge)
//   e' = e + Dense_2(act(z))
// The [B,N,N,H] hidden tensor and the [B,N,N,s_n] broadcast never exist in HBM: e is read once per direction.
//
// Tiles and fragments are those of egt_ffn.hip: a wave owns 16 pairs (b, i, 16 jt .. 16 jt + 15), pairs sit on the MFMA column
// axis, lane (p = lane & 15, q = lane >> 4) keeps pair p's channels 16 t + 4 q + {0..3}, the weights are the A operand out of
// LDS slabs [tile][k-tile][lane] float4.  s_e and s_n are multiples of 4, so the four values of a lane's fragment always lie in
// ONE of the segments er / ec / tail.  Dense_2 contracts over the "kx space" of KT = TH + SNT 16-wide tiles: kx < H is hidden
// channel h = kx (rows below 2 s_e carry zero weights and zero activations), kx >= H is exchange channel kx - H (SNT tiles,
// zero past s_n); k_xtalk_prep lays W2's K2 rows out in that space.
//
// Work split: a wave owns a block of RB rows i of one graph and walks jt outermost, its rows innermost.
//   row sums    (ec over j; d hr over j): complete inside the wave.  The lane (p = 0, q) that owns a channel group adds its
//               tile's masked sum to a global slot that ONLY it ever touches (first jt writes, later ones add): a fixed order.
//   column sums (er over i; d hc over i): the wave keeps the sum over ITS rows in registers and stores one partial per
//               (row block, column); k_xtalk_colsum adds the row blocks in index order.
//   weight gradients: per-wave MFMA accumulators over the wave's pairs, the four waves of a workgroup added in wave order
//               through LDS, k_xtalk_sum adds the workgroups in index order.
// No atomics anywhere: two runs are bitwise equal.
#include <stdlib.h>

#include "egt_tile.h"

struct XtArgs {
  int B, N, W, se, sn, relu;
  int RB, NBLK, WPG;   // rows per wave, row blocks per graph, workgroups per graph (4 row blocks each)
  float ln_eps;
  const float *e, *dy, *mask, *hr, *hc, *dhn;
  float *y, *de, *hn, *dhr, *dhc;
  const float *gamma, *beta, *W1, *b1, *W2, *b2;          // Keras layout: kernel [in, out]
  float *slab1, *slab2, *slab3, *slab4, *b1p;             // prepared operands (workspace)
  float *colp;     // column partials [B][NBLK][N][cw]: er sums (forward, cw = s_e) / d hc sums (backward, cw = s_n)
  float *rowacc;   // forward: ec row sums [B][N][s_e]
  float *part, *red;
  float *g_gamma, *g_beta, *g_W1, *g_b1, *g_W2, *g_b2;
  int nwg, part_len, snt;
  int guard;   // always 0: opaque phase guards of the backward (see k_xtalk_bwd)
};

// W: edge width; SNT: 16-wide tiles of the exchange channels hr + hc (s_n <= 16 SNT)
#define XT_GEO(W, SNT)                                                                                           \
  constexpr int FW = (W), FH = 2 * (W), TW = (W) / 16, TH = 2 * TW, KT = TH + (SNT), TILEF = 16 * (W),           \
                S1F = FW * FH, S2F = KT * 16 * FW, XT_PART = S1F + S2F + FH + FW;                                \
  (void)TILEF; (void)XT_PART
#define XT_TB 320   // the 16 x 16 transposition buffer of a wave, row pitch 20 floats

// W2 in kx space: row kx of the zero-padded [KT*16][W] operand
__device__ __forceinline__ float xt_w2x(const XtArgs& a, int kx, int o) {
  const int FH = 2 * a.W, T = FH - 2 * a.se;
  if (kx < FH) return kx >= 2 * a.se ? a.W2[(size_t)(kx - 2 * a.se) * a.W + o] : 0.f;
  const int k = kx - FH;
  return k < a.sn ? a.W2[(size_t)(T + k) * a.W + o] : 0.f;
}

// The prepared operands, once per call (lane = 16 q + pl, u = 0..3):
//   slab1[j][t][lane].u  = gamma[c] W1[c][16j+pl],        c = 16t+4q+u    (A operand of  pre   = W1p^T . xhat)
//   slab4[i][j][lane].u  = gamma[16i+pl] W1[16i+pl][16j+4q+u]             (A operand of  dxhat = W1p . dpre)
//   slab2[i][kt][lane].u = W2x[16kt+4q+u][16i+pl]                         (A operand of  y     = W2x^T . act(z))
//   slab3[kt][t][lane].u = W2x[16kt+pl][16t+4q+u]                         (A operand of  dz    = W2x . dy)
//   b1p[h] = b1[h] + sum_c beta[c] W1[c][h]
__global__ void __launch_bounds__(256) k_xtalk_prep(XtArgs a) {
  const int FW = a.W, FH = 2 * a.W, TW = FW / 16, TH = 2 * TW, KT = TH + a.snt;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int u = idx & 3, lane = (idx >> 2) & 63, pl = lane & 15, q = lane >> 4, blk = idx >> 8;
  if (idx < FW * FH) {
    {
      const int t = blk % TW, j = blk / TW, c = 16 * t + 4 * q + u;
      a.slab1[idx] = a.gamma[c] * a.W1[c * FH + 16 * j + pl];
    }
    {
      const int j = blk % TH, i = blk / TH;
      a.slab4[idx] = a.gamma[16 * i + pl] * a.W1[(16 * i + pl) * FH + 16 * j + 4 * q + u];
    }
  }
  if (idx < KT * 16 * FW) {
    {
      const int kt = blk % KT, i = blk / KT;
      a.slab2[idx] = xt_w2x(a, 16 * kt + 4 * q + u, 16 * i + pl);
    }
    {
      const int t = blk % TW, kt = blk / TW;
      a.slab3[idx] = xt_w2x(a, 16 * kt + pl, 16 * t + 4 * q + u);
    }
  }
  if (idx < FH) {
    float s = a.b1[idx];
    for (int c = 0; c < FW; ++c) s = fmaf(a.beta[c], a.W1[c * FH + idx], s);
    a.b1p[idx] = s;
  }
}

// relu, or elu with the Keras default alpha = 1.  expm1f, not the fast exp minus 1: that difference cancels for |v| << 1 (6e-8
// absolute on a value of |v|; tests/test_conditioning_gpu.py small_weights4).  xt_dact's hid + 1 is exp(v) to the same accuracy.
__device__ __forceinline__ float xt_act(float v, int relu) {
  return v > 0.f ? v : (relu ? 0.f : expm1f(v));
}
__device__ __forceinline__ float xt_dact(float hid, int relu) {   // derivative from the activation's OUTPUT
  return hid > 0.f ? 1.f : (relu ? 0.f : hid + 1.0f);
}
__device__ __forceinline__ v4f xt_act4(v4f v, int relu) {
  return (v4f){xt_act(v[0], relu), xt_act(v[1], relu), xt_act(v[2], relu), xt_act(v[3], relu)};
}

__device__ __forceinline__ void xt_to_lds(float* dst, const float* src, int nfloats) {
  for (int i = threadIdx.x; i < nfloats / 4; i += 256)
    reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(src)[i];
}

// acc += sum_n A[n] . B[n] over N consecutive [lane] float4 slab blocks (1 KiB apart): 4 N MFMAs
template <int N>
__device__ __forceinline__ v4f xt_gemm(const float* slab_lane, const v4f* b, v4f acc) {
#pragma unroll
  for (int n = 0; n < N; ++n) {
    const float4 w = *reinterpret_cast<const float4*>(slab_lane + n * 256);
    acc = MFMA(w.x, b[n][0], acc);
    acc = MFMA(w.y, b[n][1], acc);
    acc = MFMA(w.z, b[n][2], acc);
    acc = MFMA(w.w, b[n][3], acc);
  }
  return acc;
}

// the lane's fragment v (pair p, channels 4q + {0..3} of one 16-wide tile) -> o[s] = channel pl of pair q + 4s: the row-axis
// operand of the weight-gradient products
__device__ __forceinline__ void xt_transpose(float* tb, v4f v, int p, int q, float (&o)[4]) {
  lds_sync();
  *reinterpret_cast<v4f*>(tb + p * 20 + 4 * q) = v;
  lds_sync();
#pragma unroll
  for (int s = 0; s < 4; ++s) o[s] = tb[(q + 4 * s) * 20 + p];
}

// the lane's four exchange channels 16 kt + 4 q + {0..3} of node row `row` (zero past s_n)
__device__ __forceinline__ v4f xt_node4(const float* t, size_t row, int sn, int kt, int q, bool ok) {
  v4f v = {0.f, 0.f, 0.f, 0.f};
  const int k = 16 * kt + 4 * q;
  if (ok && k < sn) {
    const float* s = t + row * sn + k;
    v = (v4f){s[0], s[1], s[2], s[3]};
  }
  return v;
}

// ================================================================== forward =====
template <int W, int SNT>
__global__ void __launch_bounds__(256) k_xtalk_fwd(XtArgs a) {
  XT_GEO(W, SNT);
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* s1 = sm;
  float* s2 = s1 + S1F;
  float* b1s = s2 + S2F;   // [2W]
  float* b2s = b1s + FH;   // [W]
  float* tiles = b2s + FW; // [4 waves][16 W]
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int p = lane & 15, q = lane >> 4;
  xt_to_lds(s1, a.slab1, S1F);
  xt_to_lds(s2, a.slab2, S2F);
  if (threadIdx.x < FH) b1s[threadIdx.x] = a.b1p[threadIdx.x];
  if (threadIdx.x < FW) b2s[threadIdx.x] = a.b2[threadIdx.x];
  __syncthreads();
  float* tl = tiles + wave * TILEF;
  const int N = a.N, se = a.se, sn = a.sn, relu = a.relu;
  const int b = blockIdx.x / a.WPG, blk = (blockIdx.x % a.WPG) * 4 + wave;
  if (blk >= a.NBLK) return;   // (no workgroup barrier below)
  const int i0 = blk * a.RB, i1 = min(N, i0 + a.RB);
  const int njt = (N + 15) / 16;
  const float* mb = a.mask + (size_t)b * N;
  for (int jt = 0; jt < njt; ++jt) {
    const int jv = min(16, N - jt * 16);
    const int jcol = jt * 16 + p;
    const bool pok = p < jv;
    const float mj = pok ? mb[jcol] : 0.f;
    v4f hcv[SNT > 0 ? SNT : 1];
#pragma unroll
    for (int kt = 0; kt < SNT; ++kt) hcv[kt] = xt_node4(a.hc, (size_t)b * N + jcol, sn, kt, q, pok);
    v4f racc[TW];   // er summed over the wave's rows (s_e <= De: the er channels lie in the first TW hidden tiles)
#pragma unroll
    for (int j = 0; j < TW; ++j) racc[j] = (v4f){0.f, 0.f, 0.f, 0.f};
    for (int i = i0; i < i1; ++i) {
      const float mi = mb[i];
      const size_t toff = (((size_t)b * N + i) * N + (size_t)jt * 16) * FW;
      TileRegs<FW> tr;
      tile_gload<FW, true>(tr, a.e + toff, lane, jv);
      lds_sync();
      tile_lds_put<FW>(tl, tr, lane, jv);
      lds_sync();
      float4 x[TW];
#pragma unroll
      for (int t = 0; t < TW; ++t) x[t] = frag_read<FW>(tl, p, q, t);
      ln_frags<W>(x, q, a.ln_eps);
      v4f xv[TW], h[KT];
#pragma unroll
      for (int t = 0; t < TW; ++t) xv[t] = (v4f){x[t].x, x[t].y, x[t].z, x[t].w};
#pragma unroll
      for (int j = 0; j < TH; ++j) {                                   // fnn_lr1, the exchange, the activation
        const float4 bj = *reinterpret_cast<const float4*>(b1s + 16 * j + 4 * q);
        v4f pre = {bj.x, bj.y, bj.z, bj.w};
        pre = xt_gemm<TW>(s1 + (j * TW * 64 + lane) * 4, xv, pre);
        const int hb = 16 * j + 4 * q;
        if (16 * j < 2 * se) {   // (uniform) a tile with exchanged channels
          const bool er = hb < se, ec = !er && hb < 2 * se;
          const float fi = er ? mi : 0.f;
          if (j < TW) racc[j] += pre * fi;
          float cs[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) cs[r] = row_sum16(pre[r] * mj);
          if (ec && p == 0) {
            float* dst = a.rowacc + ((size_t)b * N + i) * se + (hb - se);
#pragma unroll
            for (int r = 0; r < 4; ++r) dst[r] = jt ? dst[r] + cs[r] : cs[r];
          }
        }
        h[j] = hb >= 2 * se ? xt_act4(pre, relu) : (v4f){0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int kt = 0; kt < SNT; ++kt)                                 // hr[i] + hc[j]  (act(0) = 0 past s_n)
        h[TH + kt] = xt_act4(xt_node4(a.hr, (size_t)b * N + i, sn, kt, q, true) + hcv[kt], relu);
#pragma unroll
      for (int o = 0; o < TW; ++o) {                                   // fnn_lr2 + residual (joined after the chain, as k_ffn_fwd)
        const float4 xr = frag_read<FW>(tl, p, q, o);
        const float4 bo = *reinterpret_cast<const float4*>(b2s + 16 * o + 4 * q);
        v4f acc = {bo.x, bo.y, bo.z, bo.w};
        acc = xt_gemm<KT>(s2 + (o * KT * 64 + lane) * 4, h, acc);
        frag_write<FW>(tl, p, q, o, make_float4(acc[0] + xr.x, acc[1] + xr.y, acc[2] + xr.z, acc[3] + xr.w));
      }
      lds_sync();
      tile_from_lds<FW>(tl, a.y + toff, lane, jv);
    }
    if (pok) {   // this row block's er partial of columns 16 jt .. + 15
      float* dst = a.colp + (((size_t)b * a.NBLK + blk) * N + jcol) * se;
#pragma unroll
      for (int j = 0; j < TW; ++j) {
        const int hb = 16 * j + 4 * q;
        if (hb < se) *reinterpret_cast<float4*>(dst + hb) = make_float4(racc[j][0], racc[j][1], racc[j][2], racc[j][3]);
      }
    }
  }
}

// sum over the row blocks in index order.  mode 0: hn = divide_no_nan(colp sums + rowacc, sum of the mask); mode 1: d hc = colp sums
__global__ void __launch_bounds__(256) k_xtalk_colsum(XtArgs a, int mode) {
  const int cw = mode ? a.sn : a.se;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x, total = (size_t)a.B * a.N * cw;
  if (idx >= total) return;
  const int c = (int)(idx % cw), n = (int)((idx / cw) % a.N), b = (int)(idx / ((size_t)cw * a.N));
  float v = 0.f;
  for (int blk = 0; blk < a.NBLK; ++blk) v += a.colp[(((size_t)b * a.NBLK + blk) * a.N + n) * cw + c];
  if (mode) { a.dhc[idx] = v; return; }
  float cnt = 0.f;
  for (int k = 0; k < a.N; ++k) cnt += a.mask[(size_t)b * a.N + k];
  v += a.rowacc[idx];
  a.hn[idx] = cnt != 0.f ? v / cnt : 0.f;
}

// ================================================================= backward =====
// Recomputes the forward from e, as k_ffn_bwd does.  Per tile: (A) xhat, pre, act(z); (T2) hid^T . dy; (B) dz = W2x . dy, dpre
// (tail: dz act'; er: m_i d hn[j] / count; ec: m_j d hn[i] / count), the d hr / d hc sums; (T1) xhat^T . dpre; (D) dxhat = W1p . dpre,
// LayerNorm backward, de = dy + ... .  One wave per SIMD: the weight-gradient tiles (TW TH + KT TW accumulators) stay in
// registers for the wave's whole row block.
// W = 64 with three or four exchange tiles: 304 / 320 accumulator registers beside the tile phases' working set pass a wave's 512
// (13 / 96 spilled registers in the row loop when built that way).  Those instances keep only the hidden rows of T2 (K1 = TH tiles)
// through the main walk and take the exchange rows of T2 in a second walk over the wave's pairs that needs only dy, hr and hc
// (no product besides the 4 SNT TW weight-gradient MFMAs per tile, a working set of ~40 registers): e is still read once, d e' twice.
// Every tile phase opens with its own copy of the lane's (p, q), opaque to the compiler, and sits behind an opaque always-true
// guard (a.guard == 0), as in k_ffn_bwd: the phase's operands and LDS address math stay inside the phase instead of stretching
// across the tile next to the weight-gradient accumulators.
#define XT_PHASE_PQ int p = p0, q = q0; asm volatile("" : "+v"(p), "+v"(q))
template <int W, int SNT>
__global__ void __launch_bounds__(256, 1) k_xtalk_bwd(XtArgs a) {
  XT_GEO(W, SNT);
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* s1 = sm;
  float* s3 = s1 + S1F;
  float* s4 = s3 + S2F;
  float* b1s = s4 + S1F;     // [2W]
  float* tiles = b1s + FH;   // [4 waves][e / xhat | dy / de | transposition buffer]
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int p0 = lane & 15, q0 = lane >> 4;
  xt_to_lds(s1, a.slab1, S1F);
  xt_to_lds(s3, a.slab3, S2F);
  xt_to_lds(s4, a.slab4, S1F);
  if (threadIdx.x < FH) b1s[threadIdx.x] = a.b1p[threadIdx.x];
  __syncthreads();
  float* et = tiles + wave * (2 * TILEF + XT_TB);
  float* dt = et + TILEF;
  float* tb = dt + TILEF;
  constexpr int EN1 = (W == 64 && SNT >= 3) ? 0 : SNT, K1 = TH + EN1, ENX = SNT - EN1;   // exchange tiles of T2 in the main walk / the second
  v4f accT1[TW * TH], accT2[K1 * TW];   // T1[in 16t+4q+r][hid 16j+pl] = accT1[t*TH+j][r] ; T2[kx 16kt+4q+r][out 16o+pl] = accT2[kt*TW+o][r]
#pragma unroll
  for (int k = 0; k < TW * TH; ++k) accT1[k] = (v4f){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < K1 * TW; ++k) accT2[k] = (v4f){0.f, 0.f, 0.f, 0.f};
  float sp[TH], sd[TW];   // bias-gradient sums over pairs q + 4s: dpre column 16j + pl, dy column 16o + pl
#pragma unroll
  for (int j = 0; j < TH; ++j) sp[j] = 0.f;
#pragma unroll
  for (int t = 0; t < TW; ++t) sd[t] = 0.f;

  const int N = a.N, se = a.se, sn = a.sn, relu = a.relu;
  const int b = blockIdx.x / a.WPG, blk = (blockIdx.x % a.WPG) * 4 + wave;
  const int i0 = blk * a.RB, i1 = blk < a.NBLK ? min(N, i0 + a.RB) : i0;   // (a wave past the last row block only joins the final sum)
  const int njt = i1 > i0 ? (N + 15) / 16 : 0;
  const float* mb = a.mask + (size_t)b * N;
  float cnt = 0.f;
  if (se > 0) {
    for (int k = lane; k < N; k += 64) cnt += mb[k];
    cnt = sum_over_q(row_sum16(cnt));
  }
  const float ginv = cnt != 0.f ? 1.0f / cnt : 0.f;   // divide_no_nan: no gradient through an empty graph's mean
  for (int jt = 0; jt < njt; ++jt) {
    const int jv = min(16, N - jt * 16);
    const int jcol = jt * 16 + p0;
    const bool pok = p0 < jv;
    const float mj = pok ? mb[jcol] : 0.f;
    v4f cacc[SNT > 0 ? SNT : 1];
#pragma unroll
    for (int kt = 0; kt < SNT; ++kt) cacc[kt] = (v4f){0.f, 0.f, 0.f, 0.f};
    for (int i = i0; i < i1; ++i) {
      const float mi = mb[i];
      const size_t toff = (((size_t)b * N + i) * N + (size_t)jt * 16) * FW;
      {
        TileRegs<FW> te, td;
        tile_gload<FW, true>(te, a.e + toff, lane, jv);
        tile_gload<FW, true>(td, a.dy + toff, lane, jv);
        lds_sync();
        tile_lds_put<FW>(et, te, lane, jv);   // pairs past the end are zero: they add nothing to the sums
        tile_lds_put<FW>(dt, td, lane, jv);
        lds_sync();
      }
      // ---- (A) recompute: xhat, act(z) ----
      float rstd;
      v4f h[KT];
      {
        XT_PHASE_PQ;
        float4 x[TW];
#pragma unroll
        for (int t = 0; t < TW; ++t) x[t] = frag_read<FW>(et, p, q, t);
        rstd = ln_frags<W>(x, q, a.ln_eps);
#pragma unroll
        for (int t = 0; t < TW; ++t) frag_write<FW>(et, p, q, t, x[t]);   // xhat: row-axis operand of T1, LayerNorm backward
        v4f xv[TW];
#pragma unroll
        for (int t = 0; t < TW; ++t) xv[t] = (v4f){x[t].x, x[t].y, x[t].z, x[t].w};
#pragma unroll
        for (int j = 0; j < TH; ++j) {
          const float4 bj = *reinterpret_cast<const float4*>(b1s + 16 * j + 4 * q);
          v4f pre = {bj.x, bj.y, bj.z, bj.w};
          pre = xt_gemm<TW>(s1 + (j * TW * 64 + lane) * 4, xv, pre);
          h[j] = 16 * j + 4 * q >= 2 * se ? xt_act4(pre, relu) : (v4f){0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int kt = 0; kt < SNT; ++kt)
          h[TH + kt] = xt_act4(xt_node4(a.hr, (size_t)b * N + i, sn, kt, q, true) +
                              xt_node4(a.hc, (size_t)b * N + jcol, sn, kt, q, pok), relu);
      }
      lds_sync();
      // ---- (T2) += act(z)^T . dy over the 16 pairs (pair index rho = q + 4s) ----
      if (a.guard == 0) {
        XT_PHASE_PQ;
        float bdy[TW][4];   // dy[rho][16o+pl]
#pragma unroll
        for (int o = 0; o < TW; ++o)
#pragma unroll
          for (int s = 0; s < 4; ++s) bdy[o][s] = elem_read<FW>(dt, q + 4 * s, 16 * o + p);
#pragma unroll
        for (int o = 0; o < TW; ++o) sd[o] += (bdy[o][0] + bdy[o][1]) + (bdy[o][2] + bdy[o][3]);
#pragma unroll
        for (int kt = 0; kt < K1; ++kt) {
          float ah[4];
          xt_transpose(tb, h[kt], p, q, ah);
#pragma unroll
          for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int o = 0; o < TW; ++o) accT2[kt * TW + o] = MFMA(ah[s], bdy[o][s], accT2[kt * TW + o]);
        }
      }
      // ---- (B) dz = W2x . dy ; dpre, in place over act(z) ----
      if (a.guard == 0) {
        XT_PHASE_PQ;
        v4f dv[TW];
#pragma unroll
        for (int t = 0; t < TW; ++t) {
          const float4 dyf = frag_read<FW>(dt, p, q, t);
          dv[t] = (v4f){dyf.x, dyf.y, dyf.z, dyf.w};
        }
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
          v4f acc = {0.f, 0.f, 0.f, 0.f};
          acc = xt_gemm<TW>(s3 + (kt * TW * 64 + lane) * 4, dv, acc);
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[r] *= xt_dact(h[kt][r], relu);
          if (kt < TH) {
            const int hb = 16 * kt + 4 * q;
            if (hb < se) {              // er[i][j] entered hn[j] with weight m_i
              acc = (v4f){0.f, 0.f, 0.f, 0.f};
              if (pok) {
                const float* g = a.dhn + ((size_t)b * N + jcol) * se + hb;
                const float f = mi * ginv;
                acc = (v4f){g[0] * f, g[1] * f, g[2] * f, g[3] * f};
              }
            } else if (hb < 2 * se) {   // ec[i][j] entered hn[i] with weight m_j (0 past the end)
              const float* g = a.dhn + ((size_t)b * N + i) * se + (hb - se);
              const float f = mj * ginv;
              acc = (v4f){g[0] * f, g[1] * f, g[2] * f, g[3] * f};
            }
          } else {                      // exchange channels: d hr[i] sums over j, d hc[j] over i
            cacc[kt - TH > 0 ? kt - TH : 0] += acc;
            float rs[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) rs[r] = row_sum16(acc[r]);
            const int k = 16 * (kt - TH) + 4 * q;
            if (p == 0 && k < sn) {
              float* dst = a.dhr + ((size_t)b * N + i) * sn + k;
#pragma unroll
              for (int r = 0; r < 4; ++r) dst[r] = jt ? dst[r] + rs[r] : rs[r];
            }
          }
          h[kt] = acc;
        }
      }
      // ---- (T1) += xhat^T . dpre ----
      if (a.guard == 0) {
        XT_PHASE_PQ;
        float axh[TW][4];   // xhat[rho][16t+pl]
#pragma unroll
        for (int t = 0; t < TW; ++t)
#pragma unroll
          for (int s = 0; s < 4; ++s) axh[t][s] = elem_read<FW>(et, q + 4 * s, 16 * t + p);
#pragma unroll
        for (int j = 0; j < TH; ++j) {
          float bd[4];
          xt_transpose(tb, h[j], p, q, bd);
          sp[j] += (bd[0] + bd[1]) + (bd[2] + bd[3]);
#pragma unroll
          for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int t = 0; t < TW; ++t) accT1[t * TH + j] = MFMA(axh[t][s], bd[s], accT1[t * TH + j]);
        }
      }
      // ---- (D) dxhat = W1p . dpre ; LayerNorm backward ; de = dy + ... (in place over the dy tile) ----
      if (a.guard == 0) {
        XT_PHASE_PQ;
        float4 dxh[TW], x[TW];
        float m1 = 0.f, m2 = 0.f;
#pragma unroll
        for (int o = 0; o < TW; ++o) {
          x[o] = frag_read<FW>(et, p, q, o);   // xhat
          v4f acc = {0.f, 0.f, 0.f, 0.f};
          acc = xt_gemm<TH>(s4 + (o * TH * 64 + lane) * 4, h, acc);
          dxh[o] = make_float4(acc[0], acc[1], acc[2], acc[3]);
          m1 += (acc[0] + acc[1]) + (acc[2] + acc[3]);
          m2 = fmaf(acc[0], x[o].x, m2); m2 = fmaf(acc[1], x[o].y, m2);
          m2 = fmaf(acc[2], x[o].z, m2); m2 = fmaf(acc[3], x[o].w, m2);
        }
        m1 = sum_over_q(m1) * (1.0f / FW); m2 = sum_over_q(m2) * (1.0f / FW);
#pragma unroll
        for (int o = 0; o < TW; ++o) {
          const float4 dyv = frag_read<FW>(dt, p, q, o);
          float4 r;
          r.x = dyv.x + rstd * (dxh[o].x - m1 - x[o].x * m2);
          r.y = dyv.y + rstd * (dxh[o].y - m1 - x[o].y * m2);
          r.z = dyv.z + rstd * (dxh[o].z - m1 - x[o].z * m2);
          r.w = dyv.w + rstd * (dxh[o].w - m1 - x[o].w * m2);
          frag_write<FW>(dt, p, q, o, r);
        }
      }
      lds_sync();
      tile_from_lds<FW>(dt, a.de + toff, lane, jv);
    }
    if (pok) {   // this row block's d hc partial of columns 16 jt .. + 15
#pragma unroll
      for (int kt = 0; kt < SNT; ++kt) {
        const int k = 16 * kt + 4 * q0;
        if (k < sn)
          *reinterpret_cast<float4*>(a.colp + (((size_t)b * a.NBLK + blk) * N + jcol) * sn + k) =
              make_float4(cacc[kt][0], cacc[kt][1], cacc[kt][2], cacc[kt][3]);
      }
    }
  }

  // ---- the exchange rows of T2 that the main walk left out: T2[H + 16 kt ..] += act(hr[i] + hc[j])^T . dy ----
  v4f accX[ENX > 0 ? ENX * TW : 1];
  if constexpr (ENX > 0) {
#pragma unroll
    for (int k = 0; k < ENX * TW; ++k) accX[k] = (v4f){0.f, 0.f, 0.f, 0.f};
    for (int jt = 0; jt < njt; ++jt) {
      const int jv = min(16, N - jt * 16);
      const int jcol = jt * 16 + p0;
      const bool pok = p0 < jv;
      for (int i = i0; i < i1; ++i) {
        XT_PHASE_PQ;
        const size_t toff = (((size_t)b * N + i) * N + (size_t)jt * 16) * FW;
        TileRegs<FW> td;
        tile_gload<FW, true>(td, a.dy + toff, lane, jv);
        lds_sync();
        tile_lds_put<FW>(dt, td, lane, jv);   // pairs past the end: dy = 0
        lds_sync();
        float bdy[TW][4];
#pragma unroll
        for (int o = 0; o < TW; ++o)
#pragma unroll
          for (int s = 0; s < 4; ++s) bdy[o][s] = elem_read<FW>(dt, q + 4 * s, 16 * o + p);
#pragma unroll
        for (int kt = 0; kt < ENX; ++kt) {
          const v4f az = xt_act4(xt_node4(a.hr, (size_t)b * N + i, sn, EN1 + kt, q, true) +
                                 xt_node4(a.hc, (size_t)b * N + jcol, sn, EN1 + kt, q, pok), relu);
          float ah[4];
          xt_transpose(tb, az, p, q, ah);
#pragma unroll
          for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int o = 0; o < TW; ++o) accX[kt * TW + o] = MFMA(ah[s], bdy[o][s], accX[kt * TW + o]);
        }
      }
    }
  }

  // ---- per-workgroup partial in canonical order [T1 | T2 (kx space) | s1 | s2]: wave 0 writes the LDS image, waves 1..3 add ----
  const int p = p0, q = q0;
  float* img = sm;
#pragma unroll 1
  for (int w = 0; w < 4; ++w) {
    __syncthreads();   // (first pass: every wave is done with the operand slabs the image overwrites)
    if (wave == w) {
#pragma unroll
      for (int k = 0; k < TW * TH; ++k)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float* d = img + (16 * (k / TH) + 4 * q + r) * FH + 16 * (k % TH) + p;
          *d = w ? *d + accT1[k][r] : accT1[k][r];
        }
#pragma unroll
      for (int k = 0; k < KT * TW; ++k)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float* d = img + S1F + (16 * (k / TW) + 4 * q + r) * FW + 16 * (k % TW) + p;
          const float v = k < K1 * TW ? accT2[k < K1 * TW ? k : 0][r] : accX[k >= K1 * TW ? k - K1 * TW : 0][r];
          *d = w ? *d + v : v;
        }
#pragma unroll
      for (int j = 0; j < TH; ++j) {
        const float v = sum_over_q(sp[j]);
        float* d = img + S1F + S2F + 16 * j + p;
        if (q == 0) *d = w ? *d + v : v;
      }
#pragma unroll
      for (int t = 0; t < TW; ++t) {
        const float v = sum_over_q(sd[t]);
        float* d = img + S1F + S2F + FH + 16 * t + p;
        if (q == 0) *d = w ? *d + v : v;
      }
    }
  }
  __syncthreads();
  float* out = a.part + (size_t)blockIdx.x * XT_PART;
  for (int i = threadIdx.x; i < XT_PART; i += 256) out[i] = img[i];
}

// deterministic sum over the workgroup partials (the shape of k_ffn_sum: 64 outputs per workgroup, 16 waves over the partial axis)
__global__ void __launch_bounds__(1024) k_xtalk_sum(XtArgs a) {
  __shared__ float red[16][64];
  const int l = threadIdx.x & 63, o = blockIdx.x * 64 + l, pg = threadIdx.x >> 6;
  float v = 0.f;
  if (o < a.part_len)
    for (int pi = pg; pi < a.nwg; pi += 16) v += a.part[(size_t)pi * a.part_len + o];
  red[pg][l] = v;
  __syncthreads();
  if (pg == 0 && o < a.part_len) {
    float s = 0.f;
#pragma unroll
    for (int g = 0; g < 16; ++g) s += red[g][l];
    a.red[o] = s;
  }
}

// T1 = sum xhat^T.dpre, T2 = sum act(z)^T.dy (kx space), s1 = sum dpre, s2 = sum dy (a.red)  ->  parameter gradients
//   dW1[c][h] = gamma_c T1[c][h] + beta_c s1[h] ; dgamma_c = sum_h W1[c][h] T1[c][h] ; dbeta_c = sum_h W1[c][h] s1[h]
//   db1 = s1 ; dW2[k] = T2[kx(k)] ; db2 = s2
__global__ void __launch_bounds__(1024) k_xtalk_param_grads(XtArgs a) {
  const int FW = a.W, FH = 2 * a.W, S1F = FW * FH, S2F = (2 * (FW / 16) + a.snt) * 16 * FW, t = threadIdx.x;
  const int T = FH - 2 * a.se, K2 = T + a.sn;
  const float* T1 = a.red;
  const float* T2 = a.red + S1F;
  const float* s1 = T2 + S2F;
  const float* s2 = s1 + FH;
  float dg = 0.f, db = 0.f;
  const int c = t >> 4, part = t & 15;   // 16 lanes per channel
  if (t < FW * 16) {
    for (int h = part; h < FH; h += 16) {
      const float w = a.W1[c * FH + h];
      dg = fmaf(w, T1[c * FH + h], dg);
      db = fmaf(w, s1[h], db);
    }
    dg = row_sum16(dg); db = row_sum16(db);
  }
  for (int i = t; i < S1F; i += 1024) a.g_W1[i] = fmaf(a.gamma[i / FH], T1[i], a.beta[i / FH] * s1[i % FH]);
  for (int i = t; i < K2 * FW; i += 1024) {
    const int k = i / FW, kx = k < T ? k + 2 * a.se : FH + (k - T);
    a.g_W2[i] = T2[kx * FW + i % FW];
  }
  if (t < FH) a.g_b1[t] = s1[t];
  if (t < FW) a.g_b2[t] = s2[t];
  if (t < FW * 16 && part == 0) { a.g_gamma[c] = dg; a.g_beta[c] = db; }
}

// ================================================================== C ABI =====
// One coverage predicate behind egt_xtalk_supported and the entry points (`report`: leave the reason with egt_set_error).
static int xtalk_check(const egt_xtalk_desc* d, bool report) {
  if (!d) EGT_BAD(EGT_E_NULL, "xtalk desc is NULL");
  if (d->dtype != EGT_F32) EGT_BAD(EGT_E_DTYPE, "cross-talk FFN takes fp32 edge tensors (got dtype %d)", d->dtype);
  if (d->flags != 0 || d->reserved != 0) EGT_BAD(EGT_E_FLAGS, "xtalk desc: flags and reserved must be 0 (got %d, %d)", d->flags, d->reserved);
  if (d->activation != EGT_ACT_RELU && d->activation != EGT_ACT_ELU)
    EGT_BAD(EGT_E_FLAGS, "cross-talk FFN activation must be EGT_ACT_RELU or EGT_ACT_ELU (got %d)", d->activation);
  if (d->B < 1 || d->N < 1) EGT_BAD(EGT_E_SHAPE, "cross-talk FFN needs B >= 1 and N >= 1 (got B %d, N %d)", d->B, d->N);
  if (d->De != 16 && d->De != 32 && d->De != 64) EGT_BAD(EGT_E_SHAPE, "cross-talk FFN covers De in {16, 32, 64} (got %d)", d->De);
  if (d->Dh != 48 && d->Dh != 64) EGT_BAD(EGT_E_SHAPE, "cross-talk FFN covers node widths 48 and 64 (got %d)", d->Dh);
  if (d->s_e < 0 || d->s_e % 4 || 2 * d->s_e > 2 * d->De)
    EGT_BAD(EGT_E_SHAPE, "s_e must be a multiple of 4 with 2 s_e <= 2 De (got s_e %d, De %d)", d->s_e, d->De);
  if (d->s_n < 0 || d->s_n % 4 || 2 * d->s_n > 2 * d->Dh)
    EGT_BAD(EGT_E_SHAPE, "s_n must be a multiple of 4 with 2 s_n <= 2 Dh (got s_n %d, Dh %d)", d->s_n, d->Dh);
  if (d->s_e == 0 && d->s_n == 0) EGT_BAD(EGT_E_SHAPE, "no cross-talk (s_e = s_n = 0): that is egt_ffn_fwd");
  if (2 * d->De - 2 * d->s_e + d->s_n == 0) EGT_BAD(EGT_E_SHAPE, "fnn_lr2_edge would have no input (2 De - 2 s_e + s_n = 0)");
  if ((long long)d->B * (((d->N + 7) / 8 + 3) / 4) > 0x7FFFFFFFll) EGT_BAD(EGT_E_SHAPE, "B * N is too large for one launch (B %d, N %d)", d->B, d->N);
  return EGT_OK;
}

extern "C" int egt_xtalk_supported(const egt_xtalk_desc* d) { return xtalk_check(d, false) == EGT_OK; }

// Every launch and workspace decision, once per call.  Workspace in floats (every section a multiple of 64):
//   [slab1 | slab2 | slab3 | slab4 | b1p | red | rowacc B N s_e | colp B NBLK N max(s_e, s_n) | part x backward workgroups]
struct XtPlan {
  int W, snt;
  size_t s1f, s2f, part_len;
  size_t slab1, slab2, slab3, slab4, b1p, red, rowacc, colp, part, total;
  int rb_f, nblk_f, wpg_f, rb_b, nblk_b, wpg_b;
  EgtLaunch prep, fwd, bwd;
};
static size_t xt_al(size_t n) { return (n + 63) / 64 * 64; }
#define XT_BWD_WG_CAP 512   // backward workgroups (= weight-gradient partials): rows per wave grow past it

static XtPlan plan_xtalk(const egt_xtalk_desc* d) {
  XtPlan P{};
  const size_t W = P.W = d->De, TW = W / 16, TH = 2 * TW;
  P.snt = (d->s_n + 15) / 16;
  const size_t KT = TH + P.snt;
  P.s1f = 2 * W * W; P.s2f = KT * 16 * W; P.part_len = P.s1f + P.s2f + 3 * W;
  P.rb_f = 8; P.nblk_f = (d->N + P.rb_f - 1) / P.rb_f; P.wpg_f = (P.nblk_f + 3) / 4;
  P.rb_b = 8;
  for (;;) {
    P.nblk_b = (d->N + P.rb_b - 1) / P.rb_b; P.wpg_b = (P.nblk_b + 3) / 4;
    if ((long long)d->B * P.wpg_b <= XT_BWD_WG_CAP || P.rb_b >= d->N) break;
    P.rb_b += 8;
  }
  const size_t cw = d->s_e > d->s_n ? d->s_e : d->s_n;
  P.slab1 = 0; P.slab2 = P.slab1 + P.s1f; P.slab3 = P.slab2 + P.s2f; P.slab4 = P.slab3 + P.s2f; P.b1p = P.slab4 + P.s1f;
  P.red = P.b1p + xt_al(2 * W); P.rowacc = P.red + xt_al(P.part_len);
  P.colp = P.rowacc + xt_al((size_t)d->B * d->N * d->s_e);
  P.part = P.colp + xt_al((size_t)d->B * P.nblk_f * d->N * cw);
  P.total = P.part + (size_t)d->B * P.wpg_b * P.part_len;
  const size_t slabmax = P.s1f > P.s2f ? P.s1f : P.s2f;
  P.prep = {(int)((slabmax + 255) / 256), 256, 0};
  P.fwd = {d->B * P.wpg_f, 256, (P.s1f + P.s2f + 3 * W + 4 * 16 * W) * sizeof(float)};
  P.bwd = {d->B * P.wpg_b, 256, (2 * P.s1f + P.s2f + 2 * W + 4 * (2 * 16 * W + XT_TB)) * sizeof(float)};
  return P;
}

extern "C" size_t egt_xtalk_workspace_bytes(const egt_xtalk_desc* d) {
  if (!egt_xtalk_supported(d)) return 0;
  return plan_xtalk(d).total * sizeof(float);
}

// The launch plan plan_xtalk chose for `d`, as text:
//   "fwd=k_xtalk_fwd<W,SNT>/rb8/g<grid> bwd=k_xtalk_bwd<W,SNT>/rb<rows per wave>/g<grid>[/walk2]"
// (/walk2: the W = 64, SNT >= 3 instances, whose backward takes the exchange rows of T2 in its second walk).  For tests and
// bench lines that must not assume which instance and row block a shape reaches.  Thread-local string; NULL when `d` is not covered.
extern "C" const char* egt_xtalk_launch_form(const egt_xtalk_desc* d) {
  if (!egt_xtalk_supported(d)) return nullptr;
  const XtPlan P = plan_xtalk(d);
  static thread_local char buf[128];
  snprintf(buf, sizeof buf, "fwd=k_xtalk_fwd<%d,%d>/rb%d/g%d bwd=k_xtalk_bwd<%d,%d>/rb%d/g%d%s", P.W, P.snt, P.rb_f, P.fwd.grid,
           P.W, P.snt, P.rb_b, P.bwd.grid, P.W == 64 && P.snt >= 3 ? "/walk2" : "");
  return buf;
}

static int xtalk_fill(const egt_xtalk_desc* d, const egt_ffn_params* p, const void* e, const void* mask, const void* hr,
                      const void* hc, void* ws, XtPlan& P, XtArgs& a) {
  if (!d || !p || !ws) EGT_FAIL(EGT_E_NULL, "desc/params/workspace is NULL");
  const int rc = xtalk_check(d, true);
  if (rc) return rc;
  if (!p->norm_gamma || !p->norm_beta || !p->lr1_kernel || !p->lr1_bias || !p->lr2_kernel || !p->lr2_bias)
    EGT_FAIL(EGT_E_NULL, "an FFN parameter pointer is NULL");
  if (!e || !mask) EGT_FAIL(EGT_E_NULL, "e/mask is NULL");
  if (d->s_n > 0 && (!hr || !hc)) EGT_FAIL(EGT_E_NULL, "hr/hc is NULL with s_n > 0");
  P = plan_xtalk(d);
  a = XtArgs{};
  a.B = d->B; a.N = d->N; a.W = d->De; a.se = d->s_e; a.sn = d->s_n; a.relu = d->activation == EGT_ACT_RELU;
  a.ln_eps = d->ln_eps; a.snt = P.snt;
  a.e = (const float*)e; a.mask = (const float*)mask; a.hr = (const float*)hr; a.hc = (const float*)hc;
  a.gamma = (const float*)p->norm_gamma; a.beta = (const float*)p->norm_beta;
  a.W1 = (const float*)p->lr1_kernel; a.b1 = (const float*)p->lr1_bias;
  a.W2 = (const float*)p->lr2_kernel; a.b2 = (const float*)p->lr2_bias;
  float* w = (float*)ws;
  a.slab1 = w + P.slab1; a.slab2 = w + P.slab2; a.slab3 = w + P.slab3; a.slab4 = w + P.slab4; a.b1p = w + P.b1p;
  a.red = w + P.red; a.rowacc = w + P.rowacc; a.colp = w + P.colp; a.part = w + P.part;
  a.part_len = (int)P.part_len;
  return EGT_OK;
}

template <int W, int SNT>
static void xtalk_launch_ws(const XtPlan& P, const XtArgs& a, bool bwd, hipStream_t st) {
  if (bwd) egt_launch_planned<k_xtalk_bwd<W, SNT>>("k_xtalk_bwd", P.bwd, st, a);
  else egt_launch_planned<k_xtalk_fwd<W, SNT>>("k_xtalk_fwd", P.fwd, st, a);
}
template <int W>
static void xtalk_launch_w(const XtPlan& P, const XtArgs& a, bool bwd, hipStream_t st) {
  switch (P.snt) {   // (s_n <= Dh <= 64: at most four exchange tiles)
    case 0: xtalk_launch_ws<W, 0>(P, a, bwd, st); break;
    case 1: xtalk_launch_ws<W, 1>(P, a, bwd, st); break;
    case 2: xtalk_launch_ws<W, 2>(P, a, bwd, st); break;
    case 3: xtalk_launch_ws<W, 3>(P, a, bwd, st); break;
    default: xtalk_launch_ws<W, 4>(P, a, bwd, st); break;
  }
}
static void xtalk_launch(const XtPlan& P, const XtArgs& a, bool bwd, hipStream_t st) {
  EGT_LAUNCH("k_xtalk_prep", k_xtalk_prep, dim3(P.prep.grid), dim3(P.prep.block), P.prep.lds, st, a);
  switch (P.W) {   // (xtalk_check has passed: these are all the widths)
    case 16: xtalk_launch_w<16>(P, a, bwd, st); break;
    case 32: xtalk_launch_w<32>(P, a, bwd, st); break;
    default: xtalk_launch_w<64>(P, a, bwd, st); break;
  }
}

extern "C" int egt_xtalk_fwd(const egt_xtalk_desc* desc, const egt_ffn_params* params, const void* e, const void* mask,
                             const void* hr, const void* hc, void* e_out, void* hn, void* workspace, void* stream) {
  XtPlan P; XtArgs a;
  int rc = xtalk_fill(desc, params, e, mask, hr, hc, workspace, P, a);
  if (rc) return rc;
  if (!e_out) EGT_FAIL(EGT_E_NULL, "e_out is NULL");
  if (desc->s_e > 0 && !hn) EGT_FAIL(EGT_E_NULL, "hn is NULL with s_e > 0");
  a.y = (float*)e_out; a.hn = (float*)hn;
  a.RB = P.rb_f; a.NBLK = P.nblk_f; a.WPG = P.wpg_f;
  hipStream_t st = (hipStream_t)stream;
  xtalk_launch(P, a, false, st);
  if (desc->s_e > 0) {
    const size_t n = (size_t)a.B * a.N * a.se;
    EGT_LAUNCH("k_xtalk_colsum", k_xtalk_colsum, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, 0);
  }
  EGT_HIP_LAUNCH_CHECK("egt_xtalk_fwd");
  return EGT_OK;
}

extern "C" int egt_xtalk_bwd(const egt_xtalk_desc* desc, const egt_ffn_params* params, const void* e, const void* mask,
                             const void* hr, const void* hc, const void* d_e_out, const void* d_hn, void* d_e, void* d_hr,
                             void* d_hc, const egt_ffn_params* grads, void* workspace, void* stream) {
  XtPlan P; XtArgs a;
  int rc = xtalk_fill(desc, params, e, mask, hr, hc, workspace, P, a);
  if (rc) return rc;
  if (!d_e_out || !d_e || !grads) EGT_FAIL(EGT_E_NULL, "d_e_out/d_e/grads is NULL");
  if (desc->s_e > 0 && !d_hn) EGT_FAIL(EGT_E_NULL, "d_hn is NULL with s_e > 0");
  if (desc->s_n > 0 && (!d_hr || !d_hc)) EGT_FAIL(EGT_E_NULL, "d_hr/d_hc is NULL with s_n > 0");
  if (!grads->norm_gamma || !grads->norm_beta || !grads->lr1_kernel || !grads->lr1_bias || !grads->lr2_kernel || !grads->lr2_bias)
    EGT_FAIL(EGT_E_NULL, "an FFN gradient pointer is NULL");
  a.dy = (const float*)d_e_out; a.dhn = (const float*)d_hn; a.de = (float*)d_e; a.dhr = (float*)d_hr; a.dhc = (float*)d_hc;
  a.g_gamma = (float*)grads->norm_gamma; a.g_beta = (float*)grads->norm_beta;
  a.g_W1 = (float*)grads->lr1_kernel; a.g_b1 = (float*)grads->lr1_bias;
  a.g_W2 = (float*)grads->lr2_kernel; a.g_b2 = (float*)grads->lr2_bias;
  a.RB = P.rb_b; a.NBLK = P.nblk_b; a.WPG = P.wpg_b; a.nwg = P.bwd.grid;
  hipStream_t st = (hipStream_t)stream;
  xtalk_launch(P, a, true, st);
  if (desc->s_n > 0) {
    const size_t n = (size_t)a.B * a.N * a.sn;
    EGT_LAUNCH("k_xtalk_colsum", k_xtalk_colsum, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, 1);
  }
  EGT_LAUNCH("k_xtalk_sum", k_xtalk_sum, dim3((a.part_len + 63) / 64), dim3(1024), 0, st, a);
  EGT_LAUNCH("k_xtalk_param_grads", k_xtalk_param_grads, dim3(1), dim3(1024), 0, st, a);
  EGT_HIP_LAUNCH_CHECK("egt_xtalk_bwd");
  return EGT_OK;
}
