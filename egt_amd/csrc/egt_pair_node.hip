// The large-head block (d = 64, H = 8, Dh = 512, De = 32) as ONE C-ABI operator: the node side of mha_block
// (graph_xformer_model_base.py:106-145) on exact-fp32 MFMA GEMMs around the fused pair operator (egt_pair_fwd / egt_pair_bwd).
//
//   forward   k_pn_stats   per-row mean / rstd of h (two passes: mean, then the centred variance)            -> saved [R,2]
//             k_pn_qkv     QKV = LN(h).Wqkv + bqkv: h rows are normalised WHILE the A tile is staged           -> saved [R,1536]
//             egt_pair_fwd                                                                                    -> V_att, e', rowstats
//             k_pn_out     h' = V_att.Wo + bo + h
//   backward  k_pn_dvatt   dV_att = dh'.Wo^T
//             egt_pair_bwd                                                                                    -> dQKV, de, 8 edge-side gradients
//             k_pn_dln     d(LN out) = dQKV.Wqkv^T (K = 1536)
//             k_pn_lnbwd   dh = dh' + LN_bwd(d(LN out)); per-64-row partial column sums for d gamma / d beta
//             k_pn_wgrad   dWqkv = LN(h)^T.dQKV, dWo = V_att^T.dh' as per-row-chunk partials (LN again while staging);
//                          the workgroups of the first row tile also sum the columns of their dQKV / dh' tiles (dbqkv, dbo)
//             k_pn_reduce  every partial kind summed over its chunks in chunk order, written to the six gradient sinks
//
// No [R,512] LN(h) tensor exists in HBM in either direction, no floating-point atomics: every sum has one fixed order.
// All GEMMs: 128x128x32 block, 4 waves, 2x2 tiles of v_mfma_f32_32x32x2_f32 per wave, operands staged through LDS in the
// orientation their source is contiguous in ([tile dim][33] or [k][128] with a 32-column swizzle on odd k), so that every MFMA
// operand read is one bank per lane.  Dh = 512 is a compile-time constant, R = B N the run-time dimension (plan_pn).
#include <math.h>

#include "egt_common.h"

namespace {
constexpr int DH = 512, D3 = 1536, TM = 128, TK = 32, NT = 256, LDR = 33, TILE_F = TM * LDR;   // (>= TK * 128)
constexpr int LN_ROWS = 64;                                                                    // rows per k_pn_lnbwd workgroup
constexpr size_t P_WQKV = 0, P_BQKV = (size_t)DH * D3, P_WO = P_BQKV + D3, P_BO = P_WO + (size_t)DH * DH, P_STRIDE = P_BO + DH;
typedef float v16f __attribute__((ext_vector_type(16)));

// ---- launch plan: a pure function of R ------------------------------------------------------------------------------
struct PnPlan {
  int R, tiles, rpc, chunks, ln_parts;
  bool tile_ragged, chunk_ragged;
  size_t sv_qkv, sv_vatt, sv_rowstats, sv_ln, sv_pair, sv_total;       // floats
  size_t ws_dvatt, ws_dqkv, ws_dln, ws_wpart, ws_lnpart, ws_total;     // floats
};
PnPlan plan_pn(int R, size_t pair_ws_floats) {
  PnPlan P{};
  P.R = R;
  P.tiles = (R + TM - 1) / TM;
  P.tile_ragged = R % TM != 0;
  // weight gradients: 64 output tiles per chunk; at most 8 chunks of at least 256 rows (a multiple of the k step)
  const int per8 = ((R + 7) / 8 + TK - 1) / TK * TK;
  P.rpc = per8 > 256 ? per8 : 256;
  P.chunks = (R + P.rpc - 1) / P.rpc;
  P.chunk_ragged = R % P.rpc != 0;
  P.ln_parts = (R + LN_ROWS - 1) / LN_ROWS;
  const size_t r = (size_t)R;
  P.sv_qkv = 0;
  P.sv_vatt = P.sv_qkv + r * D3;
  P.sv_rowstats = P.sv_vatt + r * DH;
  P.sv_ln = P.sv_rowstats + r * 32;
  P.sv_pair = P.sv_ln + ((r * 2 + 3) & ~(size_t)3);
  P.sv_total = P.sv_pair + pair_ws_floats;
  P.ws_dvatt = 0;
  P.ws_dqkv = P.ws_dvatt + r * DH;
  P.ws_dln = P.ws_dqkv + r * D3;
  P.ws_wpart = P.ws_dln + r * DH;
  P.ws_lnpart = P.ws_wpart + (size_t)P.chunks * P_STRIDE;
  P.ws_total = P.ws_lnpart + (size_t)P.ln_parts * 2 * DH;
  return P;
}

// ---- operand staging ---------------------------------------------------------------------------------------------------
// RM: the source's rows are the tile's 128 rows and it is contiguous along k -> LDS [128][33].
// KM: the source's rows are k and it is contiguous along the tile's 128 columns -> LDS [32][128], columns ^ 32 on odd k.
// LN (A operands only): the value staged is fma((x - mean) * rstd, gamma, beta) of its h row; mean / rstd from `stats`.
struct Stage {
  float4 v[4];
  float g[4], b[4];    // LN: gamma / beta of the thread's four channels (RM: reloaded per k step; KM: fixed)
  float mu[4], rs[4];  // LN: mean / rstd of the thread's four rows       (RM: fixed;               KM: reloaded per k step)
};
__device__ __forceinline__ float4 ld4(const float* p, bool al) {
  if (al) return *reinterpret_cast<const float4*>(p);
  return make_float4(p[0], p[1], p[2], p[3]);
}
__device__ __forceinline__ float ln1(float x, float mu, float rs, float g, float b) { return fmaf((x - mu) * rs, g, b); }

template <bool LN>
__device__ __forceinline__ void rm_init(Stage& s, const float* stats, int r0, int rows) {
  if (LN) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int row = r0 + ((threadIdx.x + NT * u) >> 3);
      const float2 st = *reinterpret_cast<const float2*>(stats + 2 * (size_t)(row < rows ? row : 0));
      s.mu[u] = st.x; s.rs[u] = st.y;
    }
  }
}
template <bool LN>
__device__ __forceinline__ void rm_load(Stage& s, const float* src, int ld, bool al, int r0, int rows, int k0, const float* gamma, const float* beta) {
  const int k4 = threadIdx.x & 7;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int row = r0 + ((threadIdx.x + NT * u) >> 3);
    s.v[u] = ld4(src + (size_t)(row < rows ? row : 0) * ld + k0 + k4 * 4, al);
  }
  if (LN) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { s.g[j] = gamma[k0 + k4 * 4 + j]; s.b[j] = beta[k0 + k4 * 4 + j]; }
  }
}
template <bool LN>
__device__ __forceinline__ void rm_commit(const Stage& s, float* S, int r0, int rows) {
  const int k4 = threadIdx.x & 7;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int lr = (threadIdx.x + NT * u) >> 3;
    const bool ok = r0 + lr < rows;
    float x[4] = {s.v[u].x, s.v[u].y, s.v[u].z, s.v[u].w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (LN) x[j] = ln1(x[j], s.mu[u], s.rs[u], s.g[j], s.b[j]);
      S[lr * LDR + k4 * 4 + j] = ok ? x[j] : 0.f;
    }
  }
}

template <bool LN>
__device__ __forceinline__ void km_init(Stage& s, int c0, const float* gamma, const float* beta) {
  if (LN) {
    const int c = c0 + (threadIdx.x & 31) * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) { s.g[j] = gamma[c + j]; s.b[j] = beta[c + j]; }
  }
}
template <bool LN>
__device__ __forceinline__ void km_load(Stage& s, const float* src, int ld, bool al, int c0, int k0, int kend, const float* stats) {
  const int c4 = threadIdx.x & 31;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int k = k0 + ((threadIdx.x + NT * u) >> 5);
    const size_t kr = (size_t)(k < kend ? k : k0);   // (k0 < kend always)
    s.v[u] = ld4(src + kr * ld + c0 + c4 * 4, al);
    if (LN) {
      const float2 st = *reinterpret_cast<const float2*>(stats + 2 * kr);
      s.mu[u] = st.x; s.rs[u] = st.y;
    }
  }
}
template <bool LN>
__device__ __forceinline__ void km_commit(const Stage& s, float* S, int k0, int kend) {
  const int c4 = threadIdx.x & 31;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int lk = (threadIdx.x + NT * u) >> 5;
    const bool ok = k0 + lk < kend;
    float x[4] = {s.v[u].x, s.v[u].y, s.v[u].z, s.v[u].w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (LN) x[j] = ln1(x[j], s.mu[u], s.rs[u], s.g[j], s.b[j]);
      if (!ok) x[j] = 0.f;
    }
    *reinterpret_cast<float4*>(S + lk * 128 + ((c4 * 4) ^ ((lk & 1) << 5))) = make_float4(x[0], x[1], x[2], x[3]);
  }
}

// one k step of the 128x128 tile: wave (wm, wn) owns 64x64 = 2x2 MFMA tiles; lane l: A[i = l & 31][k = l >> 5], B[k][j = l & 31]
template <bool A_KM, bool B_KM>
__device__ __forceinline__ void mma_step(const float* As, const float* Bs, int wm, int wn, int lane, v16f (&acc)[2][2]) {
  const int i = lane & 31, hh = lane >> 5;
#pragma unroll
  for (int kk = 0; kk < TK / 2; ++kk) {
    const int k = 2 * kk + hh;
    float a[2], b[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int ra = wm * 64 + t * 32 + i, rb = wn * 64 + t * 32 + i;
      a[t] = A_KM ? As[k * 128 + (ra ^ (hh << 5))] : As[ra * LDR + k];
      b[t] = B_KM ? Bs[k * 128 + (rb ^ (hh << 5))] : Bs[rb * LDR + k];
    }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mt], b[nt], acc[mt][nt], 0, 0, 0);
  }
}

// ---- C[M, N] = A'[M, K] . B'[K, N] (+ bias (+ residual)), rows M ragged, N and K multiples of the tile ------------------
//   A: [M][lda] activations (16-byte aligned), LN: normalised while staged.
//   B_T = false: B'[k][n] = W[k][n] (W [K][ldb]);  B_T = true: B'[k][n] = W[n][k] (W [N][ldb]).  W may be 4-byte aligned only.
struct GemmArgs {
  const float *A, *W, *stats, *gamma, *beta, *bias, *res;
  float* C;
  int lda, ldb, ldc, M, N, K;
};
enum { EPI_PLAIN = 0, EPI_BIAS = 1, EPI_BIAS_RES = 2 };

template <bool LN, bool B_T, int EPI>
__device__ __forceinline__ void gemm_rows(const GemmArgs& g) {
  __shared__ __attribute__((aligned(16))) float As[TILE_F];
  __shared__ __attribute__((aligned(16))) float Bs[TILE_F];
  const int m0 = blockIdx.x * TM, n0 = blockIdx.y * 128;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1;
  const bool w_al = (reinterpret_cast<uintptr_t>(g.W) & 15) == 0;
  Stage sa, sb;
  rm_init<LN>(sa, g.stats, m0, g.M);
  v16f acc[2][2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;
  auto load = [&](int k0) {
    rm_load<LN>(sa, g.A, g.lda, true, m0, g.M, k0, g.gamma, g.beta);
    if (B_T) rm_load<false>(sb, g.W, g.ldb, w_al, n0, g.N, k0, nullptr, nullptr);
    else km_load<false>(sb, g.W, g.ldb, w_al, n0, k0, g.K, nullptr);
  };
  load(0);
  for (int k0 = 0; k0 < g.K; k0 += TK) {
    __syncthreads();
    rm_commit<LN>(sa, As, m0, g.M);
    if (B_T) rm_commit<false>(sb, Bs, n0, g.N);
    else km_commit<false>(sb, Bs, k0, g.K);
    __syncthreads();
    if (k0 + TK < g.K) load(k0 + TK);
    mma_step<false, !B_T>(As, Bs, wm, wn, lane, acc);
  }
  const int i = lane & 31, hh = lane >> 5;
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int col = n0 + wn * 64 + nt * 32 + i;
    const float bias = EPI != EPI_PLAIN ? g.bias[col] : 0.f;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm * 64 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
        if (row < g.M) {
          const size_t o = (size_t)row * g.ldc + col;
          float v = acc[mt][nt][r];
          if (EPI != EPI_PLAIN) v += bias;
          if (EPI == EPI_BIAS_RES) v += g.res[o];
          g.C[o] = v;
        }
      }
  }
}

__global__ void __launch_bounds__(NT) k_pn_qkv(GemmArgs g) { gemm_rows<true, false, EPI_BIAS>(g); }
__global__ void __launch_bounds__(NT) k_pn_out(GemmArgs g) { gemm_rows<false, false, EPI_BIAS_RES>(g); }
__global__ void __launch_bounds__(NT) k_pn_dvatt(GemmArgs g) { gemm_rows<false, true, EPI_PLAIN>(g); }
__global__ void __launch_bounds__(NT) k_pn_dln(GemmArgs g) { gemm_rows<false, true, EPI_PLAIN>(g); }

// ---- per-row LayerNorm statistics: one wave per row, two passes ---------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__global__ void __launch_bounds__(NT) k_pn_stats(const float* h, float* stats, int R, float eps) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const float* x = h + (size_t)row * DH;
  const float4 a = *reinterpret_cast<const float4*>(x + lane * 4), b = *reinterpret_cast<const float4*>(x + 256 + lane * 4);
  float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) s += v[j];
  const float mu = wave_sum(s) / DH;
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) { v[j] -= mu; ss = fmaf(v[j], v[j], ss); }
  const float rstd = rsqrtf(wave_sum(ss) / DH + eps);
  if (lane == 0) *reinterpret_cast<float2*>(stats + 2 * (size_t)row) = make_float2(mu, rstd);
}

// ---- LayerNorm backward + residual; partial column sums of d gamma / d beta per 64-row workgroup -------------------------
struct LnBwdArgs {
  const float *dln, *h, *stats, *gamma, *dh_out;
  float *dh, *part;   // part [ln_parts][2 * 512]: d gamma | d beta
  int R;
};
__global__ void __launch_bounds__(NT) k_pn_lnbwd(LnBwdArgs a) {
  __shared__ float red[4][2 * DH];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c[2] = {lane * 4, 256 + lane * 4};
  float g[8], dg[8], db[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { g[j] = a.gamma[c[j >> 2] + (j & 3)]; dg[j] = 0.f; db[j] = 0.f; }
  for (int lr = wave; lr < LN_ROWS; lr += 4) {
    const int row = blockIdx.x * LN_ROWS + lr;
    if (row >= a.R) break;
    const size_t o = (size_t)row * DH;
    const float2 st = *reinterpret_cast<const float2*>(a.stats + 2 * (size_t)row);
    float dy[8], x[8], up[8];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const float4 d4 = *reinterpret_cast<const float4*>(a.dln + o + c[p]), h4 = *reinterpret_cast<const float4*>(a.h + o + c[p]);
      const float4 u4 = *reinterpret_cast<const float4*>(a.dh_out + o + c[p]);
      dy[4 * p] = d4.x; dy[4 * p + 1] = d4.y; dy[4 * p + 2] = d4.z; dy[4 * p + 3] = d4.w;
      x[4 * p] = h4.x; x[4 * p + 1] = h4.y; x[4 * p + 2] = h4.z; x[4 * p + 3] = h4.w;
      up[4 * p] = u4.x; up[4 * p + 1] = u4.y; up[4 * p + 2] = u4.z; up[4 * p + 3] = u4.w;
    }
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      x[j] = (x[j] - st.x) * st.y;   // x hat
      dg[j] = fmaf(dy[j], x[j], dg[j]);
      db[j] += dy[j];
      dy[j] *= g[j];
      s1 += dy[j];
      s2 = fmaf(dy[j], x[j], s2);
    }
    s1 = wave_sum(s1) / DH; s2 = wave_sum(s2) / DH;
    float r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = up[j] + st.y * (dy[j] - s1 - x[j] * s2);
    *reinterpret_cast<float4*>(a.dh + o + c[0]) = make_float4(r[0], r[1], r[2], r[3]);
    *reinterpret_cast<float4*>(a.dh + o + c[1]) = make_float4(r[4], r[5], r[6], r[7]);
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) { red[wave][c[j >> 2] + (j & 3)] = dg[j]; red[wave][DH + c[j >> 2] + (j & 3)] = db[j]; }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * DH; i += NT) a.part[(size_t)blockIdx.x * 2 * DH + i] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
}

// ---- weight gradients: per-row-chunk partials of dWqkv = LN(h)^T.dQKV and dWo = V_att^T.dh', plus the bias column sums ---
struct WgradArgs {
  const float *h, *stats, *gamma, *beta, *dqkv, *vatt, *dh_out;
  float* part;   // [chunks][P_STRIDE]
  int R, rpc;
};
template <bool LN>
__device__ __forceinline__ void wgrad_tile(const float* X, const float* Y, int ldy, int m0, int n0, int kbeg, int kend, const WgradArgs& w,
                                           float* outW, float* outB, float* As, float* Bs) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1;
  Stage sa, sb;
  km_init<LN>(sa, m0, w.gamma, w.beta);
  v16f acc[2][2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;
  float colsum = 0.f;
  km_load<LN>(sa, X, DH, true, m0, kbeg, kend, w.stats);
  km_load<false>(sb, Y, ldy, true, n0, kbeg, kend, nullptr);
  for (int k0 = kbeg; k0 < kend; k0 += TK) {
    __syncthreads();
    km_commit<LN>(sa, As, k0, kend);
    km_commit<false>(sb, Bs, k0, kend);
    __syncthreads();
    if (k0 + TK < kend) {
      km_load<LN>(sa, X, DH, true, m0, k0 + TK, kend, w.stats);
      km_load<false>(sb, Y, ldy, true, n0, k0 + TK, kend, nullptr);
    }
    if (outB && threadIdx.x < 128) {   // (workgroup-uniform outB) the tile's column sums, rows in order
#pragma unroll
      for (int k = 0; k < TK; ++k) colsum += Bs[k * 128 + ((int)threadIdx.x ^ ((k & 1) << 5))];
    }
    mma_step<true, true>(As, Bs, wm, wn, lane, acc);
  }
  const int i = lane & 31, hh = lane >> 5;
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm * 64 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh, col = n0 + wn * 64 + nt * 32 + i;
        outW[(size_t)row * ldy + col] = acc[mt][nt][r];
      }
  if (outB && threadIdx.x < 128) outB[n0 + threadIdx.x] = colsum;
}
__global__ void __launch_bounds__(NT) k_pn_wgrad(WgradArgs w) {
  __shared__ __attribute__((aligned(16))) float As[TILE_F];
  __shared__ __attribute__((aligned(16))) float Bs[TILE_F];
  const int job = blockIdx.x, chunk = blockIdx.y;
  const int kbeg = chunk * w.rpc, kend = min(w.R, kbeg + w.rpc);
  float* part = w.part + (size_t)chunk * P_STRIDE;
  if (job < 48) {
    const int mt = job / 12, nt = job % 12;
    wgrad_tile<true>(w.h, w.dqkv, D3, mt * 128, nt * 128, kbeg, kend, w, part + P_WQKV, mt == 0 ? part + P_BQKV : nullptr, As, Bs);
  } else {
    const int mt = (job - 48) / 4, nt = (job - 48) % 4;
    wgrad_tile<false>(w.vatt, w.dh_out, DH, mt * 128, nt * 128, kbeg, kend, w, part + P_WO, mt == 0 ? part + P_BO : nullptr, As, Bs);
  }
}

// ---- fixed-order reduction of every partial kind into its gradient sink (sinks may be 4-byte aligned) -------------------
struct RedSeg { const float* part; float* out; unsigned n, stride, count, blk0; };
struct RedArgs { RedSeg s[6]; };
__global__ void __launch_bounds__(NT) k_pn_reduce(RedArgs a) {
  int si = 0;
#pragma unroll
  for (int j = 1; j < 6; ++j) if (blockIdx.x >= a.s[j].blk0) si = j;
  const RedSeg s = a.s[si];
  const unsigned i = (blockIdx.x - s.blk0) * NT + threadIdx.x;
  if (i >= s.n) return;
  float sum = 0.f;
  for (unsigned c = 0; c < s.count; ++c) sum += s.part[(size_t)c * s.stride + i];
  s.out[i] = sum;
}

// ---- host -----------------------------------------------------------------------------------------------------------------
egt_block_desc shared_desc(const egt_block_desc* d) { egt_block_desc p = *d; p.reserved = EGT_ATTN_WS_SHARED; return p; }
PnPlan plan_of(const egt_block_desc* d) {
  const egt_block_desc p = shared_desc(d);
  return plan_pn(d->B * d->N, egt_pair_workspace_bytes(&p) / sizeof(float));
}
int check_call(const egt_block_desc* d, const egt_block_params* P, const void* h, const void* e, const void* saved, const void* ws) {
  if (!egt_pair_block_supported(d)) EGT_FAIL(EGT_E_SHAPE, "configuration not covered by the large-head block (d = 64, De = 32, H = 8, gated, fp32, host seed)");
  if (d->reserved) EGT_FAIL(EGT_E_FLAGS, "egt_block_desc.reserved: unknown bits 0x%x (the block shares the pair workspace itself)", d->reserved);
  if (!P || !h || !e || !saved || !ws) EGT_FAIL(EGT_E_NULL, "params/h/e/saved/workspace is NULL");
  const void* const* pp = reinterpret_cast<const void* const*>(P);
  for (int i = 0; i < 14; ++i)
    if (!pp[i]) EGT_FAIL(EGT_E_NULL, "parameter pointer #%d is NULL", i);
  return EGT_OK;
}
template <auto K>
void launch_gemm(const char* name, const GemmArgs& g, hipStream_t st) {
  EGT_LAUNCH(name, K, dim3((g.M + TM - 1) / TM, g.N / 128), dim3(NT), 0, st, g);
}
}  // namespace

static_assert(sizeof(egt_block_params) == 14 * sizeof(void*), "egt_block_params is fourteen pointers");

extern "C" int egt_pair_block_supported(const egt_block_desc* d) { return egt_pair_supported(d); }

// "tile=<rows per row tile>r/<row tiles>t[/ragged] wgrad=<rows per chunk>r/<chunks>c[/ragged] ln=<rows>r/<partials>p reduce=<launches>"
extern "C" const char* egt_pair_block_launch_form(const egt_block_desc* d) {
  if (!egt_pair_block_supported(d)) return nullptr;
  const PnPlan P = plan_pn(d->B * d->N, 0);
  static thread_local char buf[128];
  snprintf(buf, sizeof buf, "tile=%dr/%dt%s wgrad=%dr/%dc%s ln=%dr/%dp reduce=1", TM, P.tiles, P.tile_ragged ? "/ragged" : "", P.rpc, P.chunks,
           P.chunk_ragged ? "/ragged" : "", LN_ROWS, P.ln_parts);
  return buf;
}
extern "C" size_t egt_pair_block_saved_bytes(const egt_block_desc* d) {
  return egt_pair_block_supported(d) ? plan_of(d).sv_total * sizeof(float) : 0;
}
extern "C" size_t egt_pair_block_workspace_bytes(const egt_block_desc* d) {
  return egt_pair_block_supported(d) ? plan_of(d).ws_total * sizeof(float) : 0;
}

extern "C" int egt_pair_block_fwd(const egt_block_desc* desc, const egt_block_params* params, const void* h, const void* e,
                                  const uint8_t* key_mask, void* h_out, void* e_out, void* saved, void* workspace, void* stream) {
  int rc = check_call(desc, params, h, e, saved, workspace);
  if (rc) return rc;
  if (!h_out || !e_out) EGT_FAIL(EGT_E_NULL, "h_out/e_out is NULL");
  const PnPlan P = plan_of(desc);
  const egt_block_desc pd = shared_desc(desc);
  hipStream_t st = (hipStream_t)stream;
  float* sv = (float*)saved;
  EGT_LAUNCH("k_pn_stats", k_pn_stats, dim3((P.R + 3) / 4), dim3(NT), 0, st, (const float*)h, sv + P.sv_ln, P.R, desc->ln_eps);
  GemmArgs g{};
  g.A = (const float*)h; g.lda = DH; g.W = (const float*)params->dense_qkv_kernel; g.ldb = D3; g.C = sv + P.sv_qkv; g.ldc = D3;
  g.M = P.R; g.N = D3; g.K = DH; g.stats = sv + P.sv_ln;
  g.gamma = (const float*)params->norm_mha_gamma; g.beta = (const float*)params->norm_mha_beta; g.bias = (const float*)params->dense_qkv_bias;
  launch_gemm<k_pn_qkv>("k_pn_qkv", g, st);
  EGT_HIP_LAUNCH_CHECK("egt_pair_block_fwd");
  rc = egt_pair_fwd(&pd, params, sv + P.sv_qkv, e, key_mask, sv + P.sv_vatt, e_out, sv + P.sv_rowstats, sv + P.sv_pair, stream);
  if (rc) return rc;
  g = GemmArgs{};
  g.A = sv + P.sv_vatt; g.lda = DH; g.W = (const float*)params->dense_mha_kernel; g.ldb = DH; g.C = (float*)h_out; g.ldc = DH;
  g.M = P.R; g.N = DH; g.K = DH; g.bias = (const float*)params->dense_mha_bias; g.res = (const float*)h;
  launch_gemm<k_pn_out>("k_pn_out", g, st);
  EGT_HIP_LAUNCH_CHECK("egt_pair_block_fwd");
  return EGT_OK;
}

// `saved` is the forward's buffer (slot 3 of its attention row statistics and the pair workspace's backward part are completed here).
extern "C" int egt_pair_block_bwd(const egt_block_desc* desc, const egt_block_params* params, const void* h, const void* e,
                                  const uint8_t* key_mask, const void* saved, const void* d_h_out, const void* d_e_out, void* d_h,
                                  void* d_e, const egt_block_params* grads, void* workspace, void* stream) {
  int rc = check_call(desc, params, h, e, saved, workspace);
  if (rc) return rc;
  if (!d_h_out || !d_e_out || !d_h || !d_e || !grads) EGT_FAIL(EGT_E_NULL, "d_h_out/d_e_out/d_h/d_e/grads is NULL");
  if (d_h == d_h_out) EGT_FAIL(EGT_E_NULL, "d_h must not alias d_h_out");
  const void* const* gp = reinterpret_cast<const void* const*>(grads);
  for (int i = 0; i < 14; ++i)
    if (!gp[i]) EGT_FAIL(EGT_E_NULL, "gradient pointer #%d is NULL", i);
  const PnPlan P = plan_of(desc);
  const egt_block_desc pd = shared_desc(desc);
  hipStream_t st = (hipStream_t)stream;
  float* sv = (float*)const_cast<void*>(saved);
  float* ws = (float*)workspace;
  GemmArgs g{};
  g.A = (const float*)d_h_out; g.lda = DH; g.W = (const float*)params->dense_mha_kernel; g.ldb = DH; g.C = ws + P.ws_dvatt; g.ldc = DH;
  g.M = P.R; g.N = DH; g.K = DH;
  launch_gemm<k_pn_dvatt>("k_pn_dvatt", g, st);
  EGT_HIP_LAUNCH_CHECK("egt_pair_block_bwd");
  rc = egt_pair_bwd(&pd, params, sv + P.sv_qkv, e, key_mask, sv + P.sv_vatt, sv + P.sv_rowstats, ws + P.ws_dvatt, d_e_out, ws + P.ws_dqkv, d_e,
                    grads, sv + P.sv_pair, stream);
  if (rc) return rc;
  g = GemmArgs{};
  g.A = ws + P.ws_dqkv; g.lda = D3; g.W = (const float*)params->dense_qkv_kernel; g.ldb = D3; g.C = ws + P.ws_dln; g.ldc = DH;
  g.M = P.R; g.N = DH; g.K = D3;
  launch_gemm<k_pn_dln>("k_pn_dln", g, st);
  LnBwdArgs l{};
  l.dln = ws + P.ws_dln; l.h = (const float*)h; l.stats = sv + P.sv_ln; l.gamma = (const float*)params->norm_mha_gamma;
  l.dh_out = (const float*)d_h_out; l.dh = (float*)d_h; l.part = ws + P.ws_lnpart; l.R = P.R;
  EGT_LAUNCH("k_pn_lnbwd", k_pn_lnbwd, dim3(P.ln_parts), dim3(NT), 0, st, l);
  WgradArgs w{};
  w.h = (const float*)h; w.stats = sv + P.sv_ln; w.gamma = (const float*)params->norm_mha_gamma; w.beta = (const float*)params->norm_mha_beta;
  w.dqkv = ws + P.ws_dqkv; w.vatt = sv + P.sv_vatt; w.dh_out = (const float*)d_h_out; w.part = ws + P.ws_wpart; w.R = P.R; w.rpc = P.rpc;
  EGT_LAUNCH("k_pn_wgrad", k_pn_wgrad, dim3(64, P.chunks), dim3(NT), 0, st, w);
  RedArgs r{};
  const float* wp = ws + P.ws_wpart;
  const float* lp = ws + P.ws_lnpart;
  r.s[0] = {wp + P_WQKV, (float*)grads->dense_qkv_kernel, (unsigned)(DH * D3), (unsigned)P_STRIDE, (unsigned)P.chunks, 0};
  r.s[1] = {wp + P_BQKV, (float*)grads->dense_qkv_bias, (unsigned)D3, (unsigned)P_STRIDE, (unsigned)P.chunks, 0};
  r.s[2] = {wp + P_WO, (float*)grads->dense_mha_kernel, (unsigned)(DH * DH), (unsigned)P_STRIDE, (unsigned)P.chunks, 0};
  r.s[3] = {wp + P_BO, (float*)grads->dense_mha_bias, (unsigned)DH, (unsigned)P_STRIDE, (unsigned)P.chunks, 0};
  r.s[4] = {lp, (float*)grads->norm_mha_gamma, (unsigned)DH, (unsigned)(2 * DH), (unsigned)P.ln_parts, 0};
  r.s[5] = {lp + DH, (float*)grads->norm_mha_beta, (unsigned)DH, (unsigned)(2 * DH), (unsigned)P.ln_parts, 0};
  unsigned blk = 0;
  for (int i = 0; i < 6; ++i) { r.s[i].blk0 = blk; blk += (r.s[i].n + NT - 1) / NT; }
  EGT_LAUNCH("k_pn_reduce", k_pn_reduce, dim3(blk), dim3(NT), 0, st, r);
  EGT_HIP_LAUNCH_CHECK("egt_pair_block_bwd");
  return EGT_OK;
}
