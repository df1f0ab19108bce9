// Fused channel FFN of the reference's ffn_block, for gfx950:
//   y = x + Dense_2( act( Dense_1( LayerNorm(x) ) ) )        width W in {16,32,48,64}, hidden 2W  (W = 8: k_ffn8_*, below)
//   lib/models/graph_xformer_model_base.py:230-258 (ffnlr1 / ffnact / ffnlr2, pre-norm, no
//   cross-talk), applied to the edge channels [B,N,N,De] and the node channels [B,N,Dh] (:309-324).
// At De = 64 this is the largest FLOP consumer of the model (24*W^2 flop per row fwd+bwd) and
// a true dense contraction: MFMA-bound (fp32 v_mfma_f32_16x16x4_f32, 256 flop/clk/CU).
//
// One wave owns 16 rows ("tile": 4 KiB of contiguous HBM).  Rows sit on the MFMA COLUMN axis
// and the weights are the A operand, so (as in egt_block.hip) lane (p = lane&15, q = lane>>4)
// keeps row p's channels 16t + 4q + {0..3}: the accumulator layout of the first GEMM IS the B
// operand layout of the second one (contraction order kappa = 16j + 4q + u on both operands) --
// the 128 hidden activations of a row never leave the registers of its four lanes.  The
// LN-folded weights live in LDS as [tile][k-tile][lane] float4 slabs (conflict-free
// ds_read_b128, four contraction steps per read), built once per call by k_ffn_prep.
// One kernel per role for the three product modes of egt_ffn_desc.matmul: k_ffn_prep<W, MM>, k_ffn_fwd<W, ACT, MM, T>,
// k_ffn_bwd<W, ACT, MM, T>.  MM sizes the staged slabs (FFN_SLABS) and picks the products behind `if constexpr`: f32_gemm on the fp32
// slabs, or split_tiles / bf_gemm (egt_tile.h) on the bf16 hi | lo slabs; everything around the products is written once.
//   forward : 256 MFMA / tile, 2 waves per SIMD, tiles streamed through ping-pong LDS buffers.
//   backward: recompute + dHid + dXhat (384 MFMA) and the two weight-gradient contractions over
//             the row axis (256 MFMA) in ONE kernel: 1 wave per SIMD so that a wave owns 512
//             registers and keeps all 64 weight-gradient tiles (256 accumulator registers)
//             for its whole row range; per-workgroup partials are reduced deterministically.
#include <stdlib.h>

#include "egt_tile.h"

// Cache-policy hint (egt_tile.h): the FFN kernels read their input tiles (x; x and dy in the backward) once -- non-temporal loads, so
// that what they WRITE (the next launch's input) stays in the memory-side cache.
#ifndef EGT_NT_FFN
#define EGT_NT_FFN true
#endif

// geometry of width W (multiple of 16, <= 64): TW channel tiles, hidden 2W = TH tiles
#define FFN_GEO(W)                                                                          \
  constexpr int FW = (W), FH = 2 * (W), TW = (W) / 16, TH = 2 * TW, SLABF = FW * FH,        \
                TILEF = 16 * (W), FFN_PART = 2 * SLABF + FH + FW;                           \
  (void)TW; (void)TH; (void)TILEF; (void)FFN_PART   /* slab = W*2W floats; partial = T1 | T2 | s1 | s2 */

struct FfnArgs {
  long rows;
  float ln_eps;
  const float *x, *dy;
  float *y, *dx;
  // parameters (Keras layout: kernel [in,out])
  const float *gamma, *beta, *W1, *b1, *W2, *b2;
  // prepared operands (workspace)
  float *slab1, *slab2, *slab3, *slab4, *b1p;
  uint16_t *sA1, *sA2;   // EGT_MM_BF16X3 / EGT_MM_BF16: bf16 (hi | lo) A-operand slabs of the two forward GEMMs
  uint16_t *sA3, *sA4;   // ... and of the backward's dhid = W2 . dy and dxhat = W1p . dpre
  float *x16;            // workspace: the prepared operands of the width-8 kernels (F8_* offsets, k_ffn8_prep)
  float *part, *red;   // backward: per-workgroup partials, reduced sums
  float *g_gamma, *g_beta, *g_W1, *g_b1, *g_W2, *g_b2;
  int nwg;
  int part_len;   // floats per workgroup partial (k_ffn_sum)
  int row8;       // width 8 on the row-per-lane kernels (k_ffn8_*)
  int W;       // channel width (host copy for the run-time-sized helper kernels)
  int guard;   // always 0: opaque phase guards of the backward (see k_ffn_bwd)
};

// slab sizes of product mode MM in floats: S1F of the W -> 2W operands (slab1 / slab3, sA1 / sA3), S2F of the 2W -> W ones (slab2 /
// slab4, sA2 / sA4).  A bf16 slab holds ceil(TW / 2) (resp. TW) 32-deep steps per output tile as [part][lane] blocks of 1 KiB.
#define FFN_SLABS(MM)                                                                        \
  constexpr int NS1 = (TW + 1) / 2, S1F = (MM) ? TH * NS1 * 2 * 256 : SLABF, S2F = (MM) ? TW * TW * 2 * 256 : SLABF; \
  (void)NS1

// v as its hi | lo bfloat16 terms (hi = bf16(v), lo = bf16(v - hi)) into slot i of the lane, in both parts of slab block blk
__device__ __forceinline__ void bf_slab_put(uint16_t* slab, int blk, int lane, int i, float v) {
  const uint32_t h = pk_bf16(v, 0.f) & 0xFFFFu;
  slab[((size_t)(blk * 2 + 0) * 64 + lane) * 8 + i] = (uint16_t)h;
  slab[((size_t)(blk * 2 + 1) * 64 + lane) * 8 + i] = (uint16_t)(pk_bf16(v - __uint_as_float(h << 16), 0.f) & 0xFFFFu);
}

// The prepared operands, once per call.  EGT_MM_F32 writes the fp32 slabs:
//   slab1[j][t][lane].u = gamma[c] W1[c][16j+pl],            c = 16t+4q+u     (A operand of  pre  = W1p^T . xhat)
//   slab2[i][j][lane].u = W2[16j+4q+u][16i+pl]                                (A operand of  y    = W2^T . hid)
//   slab3[j][t][lane].u = W2[16j+pl][16t+4q+u]                                (A operand of  dhid = W2 . dy)
//   slab4[i][j][lane].u = gamma[16i+pl] W1[16i+pl][16j+4q+u]                  (A operand of  dxhat= W1p . dpre)
// EGT_MM_BF16X3 / EGT_MM_BF16 write the bf16 slabs ONLY (the same four operands; one 16x16x32 step contracts the 8 values a lane
// holds of channel tiles 2s and 2s+1: slot i <-> tile 2s + (i >> 2), offset i & 3; part 0 = hi, 1 = lo):
//   sA1[j][s][part][lane][i] = bf16_part( gamma[c] W1[c][16j + pl] ),  c = 16 (2s + (i >> 2)) + 4q + (i & 3)   (0 past W)
//   sA3[j][s][part][lane][i] = bf16_part( W2[16j + pl][c] )                                                     (0 past W)
//   sA2[o][s][part][lane][i] = bf16_part( W2[hc][16o + pl] ),         hc = 16 (2s + (i >> 2)) + 4q + (i & 3)
//   sA4[o][s][part][lane][i] = bf16_part( gamma[16o + pl] W1[16o + pl][hc] )
// Every mode writes b1p[h] = b1[h] + sum_c beta[c] W1[c][h].
template <int W, int MM>
__global__ void __launch_bounds__(256) k_ffn_prep(FfnArgs a) {
  FFN_GEO(W);
  FFN_SLABS(MM);
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if constexpr (MM == EGT_MM_F32) {
    if (idx < SLABF) {
      const int u = idx & 3, lane = (idx >> 2) & 63, pl = lane & 15, q = lane >> 4, blk = idx >> 8;
      {
        const int t = blk % TW, j = blk / TW;
        const int c = 16 * t + 4 * q + u;
        a.slab1[idx] = a.gamma[c] * a.W1[c * FH + 16 * j + pl];
        a.slab3[idx] = a.W2[(16 * j + pl) * FW + c];
      }
      {
        const int j = blk % TH, i = blk / TH;
        const int hc = 16 * j + 4 * q + u;
        a.slab2[idx] = a.W2[hc * FW + 16 * i + pl];
        a.slab4[idx] = a.gamma[16 * i + pl] * a.W1[(16 * i + pl) * FH + hc];
      }
    }
  } else {   // one thread per (block, lane, i)
    const int i = idx & 7, lane = (idx >> 3) & 63, pl = lane & 15, q = lane >> 4, blk = idx >> 9;
    if (idx < S1F) {   // (a block is 512 slots = 512 floats of both parts)
      const int s = blk % NS1, j = blk / NS1, t = 2 * s + (i >> 2);
      const int c = 16 * t + 4 * q + (i & 3);
      bf_slab_put(a.sA1, blk, lane, i, t < TW ? a.gamma[c] * a.W1[c * FH + 16 * j + pl] : 0.f);
      bf_slab_put(a.sA3, blk, lane, i, t < TW ? a.W2[(16 * j + pl) * FW + c] : 0.f);
    }
    if (idx < S2F) {
      const int s = blk % TW, o = blk / TW;
      const int hc = 16 * (2 * s + (i >> 2)) + 4 * q + (i & 3);
      bf_slab_put(a.sA2, blk, lane, i, a.W2[hc * FW + 16 * o + pl]);
      bf_slab_put(a.sA4, blk, lane, i, a.gamma[16 * o + pl] * a.W1[(16 * o + pl) * FH + hc]);
    }
  }
  if (idx < FH) {
    float s = a.b1[idx];
    for (int c = 0; c < FW; ++c) s = fmaf(a.beta[c], a.W1[c * FH + idx], s);
    a.b1p[idx] = s;
  }
}

template <int ACT>   // EGT_ACT_RELU (2), EGT_ACT_ELU (3, Keras default alpha = 1)
__device__ __forceinline__ float ffn_act(float v) {
  if (ACT == EGT_ACT_RELU) return fmaxf(v, 0.f);
  // The difference cancels for |v| << 1 (6e-8 absolute on a value of |v|: DESIGN.md, gaps; the strict XFAIL entries of
  // tests/test_conditioning_gpu.py).  Kept: expm1f costs 10 %, a degree-4 polynomial above -1/16 8 % of the layers-scope step.
  return v > 0.f ? v : __expf(v) - 1.0f;
}
template <int ACT>   // derivative from the activation's OUTPUT (hid > 0 <=> pre > 0 for both)
__device__ __forceinline__ float ffn_dact(float hid) {
  if (ACT == EGT_ACT_RELU) return hid > 0.f ? 1.f : 0.f;
  return hid > 0.f ? 1.f : hid + 1.0f;
}

__device__ __forceinline__ void slab_to_lds(float* dst, const float* src, int nfloats, int nthreads) {
  for (int i = threadIdx.x; i < nfloats / 4; i += nthreads)
    reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(src)[i];
}

// N consecutive [lane] float4 slabs (1 KiB apart) of one MFMA group in ONE LDS round trip.  hipcc,
// short of registers, emits ds_read_b128 -> s_waitcnt -> 4 MFMA per slab (one exposed LDS latency
// per four MFMAs at one wave per SIMD); the asm issues the group's reads back to back and
// waits once.
template <int N>
__device__ __forceinline__ void slab_read(v4f (&w)[N], const float* slab_lane) {
  const unsigned addr = (unsigned)(size_t)slab_lane;   // LDS byte offset = low 32 bits of the flat address
  static_assert(N >= 1 && N <= 8, "slab group size");
  if constexpr (N == 1)
    asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(w[0]) : "v"(addr));
  else if constexpr (N == 2)
    asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:1024\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(w[0]), "=&v"(w[1]) : "v"(addr));
  else if constexpr (N == 3)
    asm volatile("ds_read_b128 %0, %3\n\tds_read_b128 %1, %3 offset:1024\n\tds_read_b128 %2, %3 offset:2048\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(w[0]), "=&v"(w[1]), "=&v"(w[2]) : "v"(addr));
  else if constexpr (N == 4)
    asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:1024\n\tds_read_b128 %2, %4 offset:2048\n\t"
                 "ds_read_b128 %3, %4 offset:3072\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(w[0]), "=&v"(w[1]), "=&v"(w[2]), "=&v"(w[3]) : "v"(addr));
  else if constexpr (N == 6)
    asm volatile("ds_read_b128 %0, %6\n\tds_read_b128 %1, %6 offset:1024\n\tds_read_b128 %2, %6 offset:2048\n\t"
                 "ds_read_b128 %3, %6 offset:3072\n\tds_read_b128 %4, %6 offset:4096\n\tds_read_b128 %5, %6 offset:5120\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&v"(w[0]), "=&v"(w[1]), "=&v"(w[2]), "=&v"(w[3]), "=&v"(w[4]), "=&v"(w[5]) : "v"(addr));
  else if constexpr (N == 8)
    asm volatile("ds_read_b128 %0, %8\n\tds_read_b128 %1, %8 offset:1024\n\tds_read_b128 %2, %8 offset:2048\n\t"
                 "ds_read_b128 %3, %8 offset:3072\n\tds_read_b128 %4, %8 offset:4096\n\tds_read_b128 %5, %8 offset:5120\n\t"
                 "ds_read_b128 %6, %8 offset:6144\n\tds_read_b128 %7, %8 offset:7168\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(w[0]), "=&v"(w[1]), "=&v"(w[2]), "=&v"(w[3]), "=&v"(w[4]), "=&v"(w[5]), "=&v"(w[6]), "=&v"(w[7])
                 : "v"(addr));
  else {
#pragma unroll
    for (int n = 0; n < N; ++n) {
      const float4 t = *reinterpret_cast<const float4*>(slab_lane + n * 256);
      w[n] = (v4f){t.x, t.y, t.z, t.w};
    }
  }
}

// fp32 products, the twin of bf_gemm: acc += sum_n A[n] . B[n] over the N [lane] float4 slab blocks at slab_lane (one slab_read), 4 N MFMAs.
// TWO: two alternating accumulators, summed at the end.  A chain of MFMAs on ONE accumulator issues every 40 cycles (dependent
// latency) instead of every 32; k_ffn_bwd runs one wave per SIMD and nothing else fills the gap.  The forward's two waves per SIMD
// cover each other: it keeps the single chain -- and its bit pattern.
template <int N, bool TWO>
__device__ __forceinline__ v4f f32_gemm(const float* slab_lane, const v4f (&b)[N], v4f acc) {
  v4f w[N];
  slab_read<N>(w, slab_lane);
  if constexpr (TWO) {
    v4f acc2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int n = 0; n < N; ++n) {
      acc = MFMA(w[n][0], b[n][0], acc);
      acc2 = MFMA(w[n][1], b[n][1], acc2);
      acc = MFMA(w[n][2], b[n][2], acc);
      acc2 = MFMA(w[n][3], b[n][3], acc2);
    }
    return acc + acc2;
  } else {
#pragma unroll
    for (int n = 0; n < N; ++n) {
      acc = MFMA(w[n][0], b[n][0], acc);
      acc = MFMA(w[n][1], b[n][1], acc);
      acc = MFMA(w[n][2], b[n][2], acc);
      acc = MFMA(w[n][3], b[n][3], acc);
    }
    return acc;
  }
}

// ================================================================== forward =====
// T: storage type of x / y (float, or uint16_t = bfloat16 bits for EGT_BF16; the LDS tiles and the arithmetic stay fp32)
// MM: egt_ffn_desc.matmul, how the two GEMMs are evaluated.  EGT_MM_F32: exact fp32 MFMAs.
// EGT_MM_BF16X3: every fp32 operand v is split into two bfloat16 terms,
// v = hi + lo (hi = bf16(v), lo = bf16(v - hi): 16 mantissa bits survive), and a product a.b is
// evaluated as a_hi.b_hi + a_lo.b_hi + a_hi.b_lo on v_mfma_f32_16x16x32_bf16 with fp32 accumulation
// (the dropped a_lo.b_lo term is 2^-18 relative; every bf16 x bf16 product is exact in fp32).  Per-product
// error <= 2^-16 instead of fp32's 2^-24 -- the outputs stay inside the fp32 parity tolerances of the
// test-suite (tests/test_ffn_gpu.py runs the SAME tolerances on this mode) -- at 3/16 of the fp32 MFMA
// cost: 96 bf16 MFMAs of 16 cycles per 16-row tile instead of 256 fp32 MFMAs of 32 cycles, which turns
// the FFN from MFMA-bound (0.46 of the fp32 matrix peak) into an HBM-bound streaming kernel.
// EGT_MM_BF16 keeps only the hi terms (plain bf16 products, fp32 accumulate; tolerance rtol 2e-2).
// Same tile flow and fragment layout in every mode: lane (p, q) holds row p's channels 16t + 4q + {0..3};
// one 16x16x32 step contracts the 8 values a lane holds of channel tiles 2s and 2s+1 -- both operands use
// that order (k_ffn_prep), so the accumulators of GEMM 1 are again the B operand of GEMM 2 without leaving the lane.
template <int W, int ACT, int MM, typename T>
__global__ void __launch_bounds__(512, 2) k_ffn_fwd(FfnArgs a) {
  FFN_GEO(W);
  FFN_SLABS(MM);
  constexpr bool SPLIT = MM == EGT_MM_BF16X3;
  const T* xg = reinterpret_cast<const T*>(a.x);
  T* yg = reinterpret_cast<T*>(a.y);
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* s1 = sm;
  float* s2 = s1 + S1F;
  float* b1s = s2 + S2F;            // [2W]
  float* b2s = b1s + FH;            // [W]
  float* tiles = b2s + FW;          // [8 waves][2][16 W]
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int p = lane & 15, q = lane >> 4;
  slab_to_lds(s1, MM ? reinterpret_cast<const float*>(a.sA1) : a.slab1, S1F, 512);
  slab_to_lds(s2, MM ? reinterpret_cast<const float*>(a.sA2) : a.slab2, S2F, 512);
  if (threadIdx.x < FH) b1s[threadIdx.x] = a.b1p[threadIdx.x];
  if (threadIdx.x < FW) b2s[threadIdx.x] = a.b2[threadIdx.x];
  __syncthreads();
  float* tl0 = tiles + wave * 2 * TILEF;
  const long ntiles = (a.rows + 15) / 16;
  const long stride = (long)gridDim.x * 8;
  long tile = (long)blockIdx.x * 8 + wave;
  typename TileIn<FW, T>::type tr;
  if (tile < ntiles) tile_gload<FW, EGT_NT_FFN>(tr, xg + tile * TILEF, lane, (int)min(16L, a.rows - tile * 16));
  long prev = -1;
  for (int it = 0; tile < ntiles; tile += stride, ++it) {
    const int rows_valid = (int)min(16L, a.rows - tile * 16);
    float* tl = tl0 + (it & 1) * TILEF;
    lds_sync();
    if (prev >= 0)   // stream out the previous tile's y from the other buffer
      tile_from_lds<FW>(tl0 + ((it - 1) & 1) * TILEF, yg + prev * TILEF, lane, (int)min(16L, a.rows - prev * 16));
    tile_lds_put<FW>(tl, tr, lane, rows_valid);
    const long nxt = tile + stride;
    if (nxt < ntiles) tile_gload<FW, EGT_NT_FFN>(tr, xg + nxt * TILEF, lane, (int)min(16L, a.rows - nxt * 16));
    lds_sync();
    float4 x[TW];
#pragma unroll
    for (int t = 0; t < TW; ++t) x[t] = frag_read<FW>(tl, p, q, t);
    ln_frags<W>(x, q, a.ln_eps);                            // norm_fnn (gamma/beta folded into the weights)
    v4f xv[TW], h[TH];
    Bf8 xh[NS1], xl[NS1];
#pragma unroll
    for (int t = 0; t < TW; ++t) xv[t] = (v4f){x[t].x, x[t].y, x[t].z, x[t].w};
    if constexpr (MM != 0) split_tiles<TW, SPLIT>(xv, xh, xl);
#pragma unroll
    for (int j = 0; j < TH; ++j) {                                    // fnn_lr1 + activation
      const float4 bj = *reinterpret_cast<const float4*>(b1s + 16 * j + 4 * q);
      v4f pre = {bj.x, bj.y, bj.z, bj.w};
      if constexpr (MM != 0) pre = bf_gemm<NS1, SPLIT>(s1, j * NS1, lane, xh, xl, pre);
      else pre = f32_gemm<TW, false>(s1 + (j * TW * 64 + lane) * 4, xv, pre);
      h[j] = (v4f){ffn_act<ACT>(pre[0]), ffn_act<ACT>(pre[1]), ffn_act<ACT>(pre[2]), ffn_act<ACT>(pre[3])};
    }
    Bf8 hh[TW], hl[TW];
    if constexpr (MM != 0) split_tiles<TH, SPLIT>(h, hh, hl);
#pragma unroll
    for (int i = 0; i < TW; ++i) {                                    // fnn_lr2 + res_fnn
      const float4 xr = frag_read<FW>(tl, p, q, i);
      const float4 b = *reinterpret_cast<const float4*>(b2s + 16 * i + 4 * q);
      // the residual joins AFTER the chain: with x in the accumulator each of the 2W accumulations rounds at ulp(x), which at
      // |x| ~ 100 is 1.2 - 1.5 of the forward tolerance on the update y - x (tests/test_conditioning_gpu.py, big / outliers;
      // 0.93 of it on the bf16 pipe)
      v4f acc = {b.x, b.y, b.z, b.w};
      if constexpr (MM != 0) acc = bf_gemm<TW, SPLIT>(s2, i * TW, lane, hh, hl, acc);
      else acc = f32_gemm<TH, false>(s2 + (i * TH * 64 + lane) * 4, h, acc);
      frag_write<FW>(tl, p, q, i, make_float4(acc[0] + xr.x, acc[1] + xr.y, acc[2] + xr.z, acc[3] + xr.w));
    }
    prev = tile;
    if (nxt >= ntiles) {   // last tile of this wave: flush
      lds_sync();
      tile_from_lds<FW>(tl, yg + tile * TILEF, lane, rows_valid);
    }
  }
}

// ================================================================= backward =====
// MM: egt_ffn_desc.matmul.  EGT_MM_BF16X3 / EGT_MM_BF16 move the three channel contractions (recompute,
// dhid = W2 . dy, dxhat = W1p . dpre: 384 of the 640 fp32 MFMAs of a tile) to the bf16 matrix pipe (144 / 48
// MFMAs of 16 cycles); the weight-gradient contractions over the ROW axis stay exact fp32 (their operands are
// read transposed out of the fp32 LDS tiles).
// Every tile phase opens with its own copy of the lane's (p, q), opaque to the compiler: the phase's LDS address math stays inside
// the phase (no hoisting out of the tile loop).
#define FFN_PHASE_PQ int p = p0, q = q0; asm volatile("" : "+v"(p), "+v"(q))
template <int W, int ACT, int MM, typename T>
__global__ void __launch_bounds__(256, 1) k_ffn_bwd(FfnArgs a) {
  FFN_GEO(W);
  const T* xg = reinterpret_cast<const T*>(a.x);
  const T* dyg = reinterpret_cast<const T*>(a.dy);
  T* dxg = reinterpret_cast<T*>(a.dx);
  FFN_SLABS(MM);
  constexpr bool SPLIT = MM == EGT_MM_BF16X3;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* s1 = sm;
  float* s3 = s1 + S1F;
  float* s4 = s3 + S1F;
  float* b1s = s4 + S2F;            // [2W]
  float* tiles = b1s + FH;          // [4 waves][x | dy | hid/dpre half][TILEF]
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int p0 = lane & 15, q0 = lane >> 4;
  slab_to_lds(s1, MM ? reinterpret_cast<const float*>(a.sA1) : a.slab1, S1F, 256);
  slab_to_lds(s3, MM ? reinterpret_cast<const float*>(a.sA3) : a.slab3, S1F, 256);
  slab_to_lds(s4, MM ? reinterpret_cast<const float*>(a.sA4) : a.slab4, S2F, 256);
  if (threadIdx.x < FH) b1s[threadIdx.x] = a.b1p[threadIdx.x];
  __syncthreads();
  float* et = tiles + wave * 3 * TILEF;
  float* dt = et + TILEF;
  float* hd = dt + TILEF;
  v4f accT1[TW * TH], accT2[TH * TW];   // T1[in 16t+4q+r][hid 16j+pl] = accT1[t*8+j][r] ; T2[hid 16j+4q+r][out 16i+pl] = accT2[j*4+i][r]
#pragma unroll
  for (int k = 0; k < TW * TH; ++k) { accT1[k] = (v4f){0.f, 0.f, 0.f, 0.f}; accT2[k] = (v4f){0.f, 0.f, 0.f, 0.f}; }
  // bias-gradient sums, taken from the ROW-axis operands of the weight-gradient products (the lane already holds column 16j + pl of
  // rows q + 4s there): one register per column tile instead of four per fragment -- 12 registers instead of 48 in a kernel whose
  // 256 weight-gradient accumulators leave no slack (the W = 64 fp32 instance spilled 20-40 registers before)
  float sp[TH];                // sums of dpre over rows q + 4s, column hid 16j + pl
  float sd[TW];                // sums of dy   over rows q + 4s, column out 16i + pl
#pragma unroll
  for (int j = 0; j < TH; ++j) sp[j] = 0.f;
#pragma unroll
  for (int t = 0; t < TW; ++t) sd[t] = 0.f;

  const long ntiles = (a.rows + 15) / 16;
  const long stride = (long)gridDim.x * 4;
  long tile = (long)blockIdx.x * 4 + wave;
  typename TileIn<FW, T>::type te, td;
  if (tile < ntiles) {
    const int rv = (int)min(16L, a.rows - tile * 16);
    tile_gload<FW, EGT_NT_FFN>(te, xg + tile * TILEF, lane, rv);
    tile_gload<FW, EGT_NT_FFN>(td, dyg + tile * TILEF, lane, rv);
  }
  long prev = -1;
  for (; tile < ntiles; tile += stride) {
    const int rows_valid = (int)min(16L, a.rows - tile * 16);
    lds_sync();
    if (prev >= 0) tile_from_lds<FW>(dt, dxg + prev * TILEF, lane, (int)min(16L, a.rows - prev * 16));   // dx of the previous tile
    lds_sync();
    tile_lds_put<FW>(et, te, lane, rows_valid);     // rows past the end are zero: they add nothing to the sums
    tile_lds_put<FW>(dt, td, lane, rows_valid);
    const long nxt = tile + stride;
    if (nxt < ntiles) {
      const int rv = (int)min(16L, a.rows - nxt * 16);
      tile_gload<FW, EGT_NT_FFN>(te, xg + nxt * TILEF, lane, rv);
      tile_gload<FW, EGT_NT_FFN>(td, dyg + nxt * TILEF, lane, rv);
    }
    lds_sync();
    // The phases below sit behind opaque always-true guards (a.guard == 0): the uniform branches
    // split the tile body into basic blocks so that hipcc keeps every phase's operands local
    // (re-read from the LDS tiles) instead of stretching 200+ live registers across the tile.
    // ---- recompute: xhat, hid ----
    float rstd;
    v4f h[TH], dp[TH];
    {
      FFN_PHASE_PQ;
      float4 x[TW];
#pragma unroll
      for (int t = 0; t < TW; ++t) x[t] = frag_read<FW>(et, p, q, t);
      rstd = ln_frags<W>(x, q, a.ln_eps);
#pragma unroll
      for (int t = 0; t < TW; ++t) frag_write<FW>(et, p, q, t, x[t]);   // xhat: A operand of T1 (other rows) + LN backward
      v4f xv[TW];
      Bf8 xh[NS1], xl[NS1];
#pragma unroll
      for (int t = 0; t < TW; ++t) xv[t] = (v4f){x[t].x, x[t].y, x[t].z, x[t].w};
      if constexpr (MM != 0) split_tiles<TW, SPLIT>(xv, xh, xl);
#pragma unroll
      for (int j = 0; j < TH; ++j) {
        const float4 bj = *reinterpret_cast<const float4*>(b1s + 16 * j + 4 * q);
        v4f pre = {bj.x, bj.y, bj.z, bj.w};
        if constexpr (MM != 0) pre = bf_gemm<NS1, SPLIT>(s1, j * NS1, lane, xh, xl, pre);
        else pre = f32_gemm<TW, (W < 64)>(s1 + (j * TW * 64 + lane) * 4, xv, pre);   // (W = 64: the extra accumulator would spill)
        h[j] = (v4f){ffn_act<ACT>(pre[0]), ffn_act<ACT>(pre[1]), ffn_act<ACT>(pre[2]), ffn_act<ACT>(pre[3])};
      }
    }
    lds_sync();
    // ---- dhid = W2 . dy ; dpre = dhid * act'(pre) ----
    if (a.guard == 0) {
      FFN_PHASE_PQ;
      v4f dv[TW];
#pragma unroll
      for (int t = 0; t < TW; ++t) {
        const float4 dyf = frag_read<FW>(dt, p, q, t);
        dv[t] = (v4f){dyf.x, dyf.y, dyf.z, dyf.w};
      }
      Bf8 dyh[NS1], dyl[NS1];
      if constexpr (MM != 0) split_tiles<TW, SPLIT>(dv, dyh, dyl);
#pragma unroll
      for (int j = 0; j < TH; ++j) {
        v4f acc = {0.f, 0.f, 0.f, 0.f};
        if constexpr (MM != 0) acc = bf_gemm<NS1, SPLIT>(s3, j * NS1, lane, dyh, dyl, acc);
        else acc = f32_gemm<TW, true>(s3 + (j * TW * 64 + lane) * 4, dv, acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] *= ffn_dact<ACT>(h[j][r]);
        dp[j] = acc;
      }
    }
    // ---- weight gradients: contractions over the 16 rows of the tile (row index rho = q + 4s) ----
    if (a.guard == 0) {                             // T2 += hid^T . dy
      FFN_PHASE_PQ;
      float bdy[TW][4];   // dy[rho][16i+pl]
#pragma unroll
      for (int i = 0; i < TW; ++i)
#pragma unroll
        for (int s = 0; s < 4; ++s) bdy[i][s] = elem_read<FW>(dt, q + 4 * s, 16 * i + p);
#pragma unroll
      for (int i = 0; i < TW; ++i) sd[i] += (bdy[i][0] + bdy[i][1]) + (bdy[i][2] + bdy[i][3]);
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        lds_sync();
#pragma unroll
        for (int jj = 0; jj < TW; ++jj)
          frag_write<FW>(hd, p, q, jj, make_float4(h[TW * half + jj][0], h[TW * half + jj][1], h[TW * half + jj][2], h[TW * half + jj][3]));
        lds_sync();
#pragma unroll
        for (int jj = 0; jj < TW; ++jj)
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const float ah = elem_read<FW>(hd, q + 4 * s, 16 * jj + p);
#pragma unroll
            for (int i = 0; i < TW; ++i) accT2[(TW * half + jj) * TW + i] = MFMA(ah, bdy[i][s], accT2[(TW * half + jj) * TW + i]);
          }
      }
    }
    if (a.guard == 0) {                             // T1 += xhat^T . dpre
      FFN_PHASE_PQ;
      float axh[TW][4];   // xhat[rho][16t+pl]
#pragma unroll
      for (int t = 0; t < TW; ++t)
#pragma unroll
        for (int s = 0; s < 4; ++s) axh[t][s] = elem_read<FW>(et, q + 4 * s, 16 * t + p);
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        lds_sync();
#pragma unroll
        for (int jj = 0; jj < TW; ++jj)
          frag_write<FW>(hd, p, q, jj, make_float4(dp[TW * half + jj][0], dp[TW * half + jj][1], dp[TW * half + jj][2], dp[TW * half + jj][3]));
        lds_sync();
#pragma unroll
        for (int jj = 0; jj < TW; ++jj)
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const float bd = elem_read<FW>(hd, q + 4 * s, 16 * jj + p);
            sp[TW * half + jj] += bd;
#pragma unroll
            for (int t = 0; t < TW; ++t) accT1[t * TH + TW * half + jj] = MFMA(axh[t][s], bd, accT1[t * TH + TW * half + jj]);
          }
      }
    }
    // ---- dxhat = W1p . dpre ; LayerNorm backward ; dx = dy + ... (in place over the dy tile) ----
    if (a.guard == 0) {
      FFN_PHASE_PQ;
      float4 dxh[TW], x[TW];
      float m1 = 0.f, m2 = 0.f;
      Bf8 dph[TW], dpl[TW];
      if constexpr (MM != 0) split_tiles<TH, SPLIT>(dp, dph, dpl);
#pragma unroll
      for (int i = 0; i < TW; ++i) {
        x[i] = frag_read<FW>(et, p, q, i);          // xhat
        v4f acc = {0.f, 0.f, 0.f, 0.f};
        if constexpr (MM != 0) acc = bf_gemm<TW, SPLIT>(s4, i * TW, lane, dph, dpl, acc);
        else acc = f32_gemm<TH, true>(s4 + (i * TH * 64 + lane) * 4, dp, acc);
        dxh[i] = make_float4(acc[0], acc[1], acc[2], acc[3]);
        m1 += (acc[0] + acc[1]) + (acc[2] + acc[3]);
        m2 = fmaf(acc[0], x[i].x, m2); m2 = fmaf(acc[1], x[i].y, m2);
        m2 = fmaf(acc[2], x[i].z, m2); m2 = fmaf(acc[3], x[i].w, m2);
      }
      m1 = sum_over_q(m1) * (1.0f / FW); m2 = sum_over_q(m2) * (1.0f / FW);
#pragma unroll
      for (int i = 0; i < TW; ++i) {
        const float4 dyv = frag_read<FW>(dt, p, q, i);
        float4 o;
        o.x = dyv.x + rstd * (dxh[i].x - m1 - x[i].x * m2);
        o.y = dyv.y + rstd * (dxh[i].y - m1 - x[i].y * m2);
        o.z = dyv.z + rstd * (dxh[i].z - m1 - x[i].z * m2);
        o.w = dyv.w + rstd * (dxh[i].w - m1 - x[i].w * m2);
        frag_write<FW>(dt, p, q, i, o);
      }
    }
    prev = tile;
  }
  lds_sync();
  if (prev >= 0) tile_from_lds<FW>(dt, dxg + prev * TILEF, lane, (int)min(16L, a.rows - prev * 16));

  // ---- per-workgroup partial: (wave 0 + wave 2) + (wave 1 + wave 3), a pairwise tree through two LANE-LINEAR LDS images
  //      (accumulator tile k of lane l at float4 slot k*64 + l: conflict-free b128 moves, no read-modify-write).  The
  //      canonical [row][col] layout is only formed by the final gather, which all four waves share.  (The first version
  //      added the waves one after the other into a canonical image: 4-way bank conflicts on ~520 b32 read-modify-writes
  //      per wave, 7 us per wave = 28 of the 73 us the kernel takes on the node channels.) ----
  const int p = p0, q = q0;
  __syncthreads();
  constexpr int NT = TW * TH;
  float* img0 = sm;
  float* img1 = img0 + 2 * NT * 256;
  float* ssum = img1 + 2 * NT * 256;   // [4 waves][FH + FW]: bias-gradient sums in canonical order
  auto img_put = [&](float* img) {
#pragma unroll
    for (int k = 0; k < NT; ++k) {
      *reinterpret_cast<v4f*>(img + (k * 64 + lane) * 4) = accT1[k];
      *reinterpret_cast<v4f*>(img + ((NT + k) * 64 + lane) * 4) = accT2[k];
    }
  };
  auto img_add = [&](const float* img) {
#pragma unroll
    for (int k = 0; k < NT; ++k) {
      accT1[k] += *reinterpret_cast<const v4f*>(img + (k * 64 + lane) * 4);
      accT2[k] += *reinterpret_cast<const v4f*>(img + ((NT + k) * 64 + lane) * 4);
    }
  };
  {
    float* sw = ssum + wave * (FH + FW);
#pragma unroll
    for (int j = 0; j < TH; ++j) {
      const float v = sum_over_q(sp[j]);       // the four lane rows hold rows q, q + 4, q + 8, q + 12 of every tile
      if (q == 0) sw[16 * j + p] = v;
    }
#pragma unroll
    for (int t = 0; t < TW; ++t) {
      const float v = sum_over_q(sd[t]);
      if (q == 0) sw[FH + 16 * t + p] = v;
    }
  }
  if (wave == 2) img_put(img0);
  if (wave == 3) img_put(img1);
  __syncthreads();
  if (wave == 0) img_add(img0);
  if (wave == 1) { img_add(img1); img_put(img1); }   // (a lane rewrites the slots it has just read: in order within the wave)
  __syncthreads();
  if (wave == 0) { img_add(img1); img_put(img0); }
  __syncthreads();
  float* out = a.part + (size_t)blockIdx.x * FFN_PART;
  for (int i = threadIdx.x; i < FFN_PART; i += 256) {
    float v;
    if (i < SLABF) {                 // T1[row = 16t + 4q + r][col = 16j + p]
      const int row = i / FH, col = i % FH;
      v = img0[(((row >> 4) * TH + (col >> 4)) * 64 + 4 * (row & 12) + (col & 15)) * 4 + (row & 3)];
    } else if (i < 2 * SLABF) {      // T2[row = 16j + 4q + r][col = 16i + p]
      const int e = i - SLABF, row = e / FW, col = e % FW;
      v = img0[((NT + (row >> 4) * TW + (col >> 4)) * 64 + 4 * (row & 12) + (col & 15)) * 4 + (row & 3)];
    } else {
      const int e = i - 2 * SLABF;
      v = ((ssum[e] + ssum[(FH + FW) + e]) + ssum[2 * (FH + FW) + e]) + ssum[3 * (FH + FW) + e];
    }
    out[i] = v;
  }
}

// T1 = sum xhat^T.dpre, s1 = sum dpre, T2 = sum hid^T.dy, s2 = sum dy (a.red)  ->  parameter gradients
//   dW1[c][h] = gamma_c T1[c][h] + beta_c s1[h] ; dgamma_c = sum_h W1[c][h] T1[c][h] ; dbeta_c = sum_h W1[c][h] s1[h]
//   db1 = s1 ; dW2 = T2 ; db2 = s2          (width 8 keeps T2 transposed: T2^T[o][h])
// One workgroup of 1024 threads, 16 lanes per channel for the gamma / beta contractions.  (Folding this into k_ffn_sum behind
// a last-workgroup ticket was tried: the device-scope fences cost more than the launch, 20 us against 7 + 10 as two launches.)
__global__ void __launch_bounds__(1024) k_ffn_param_grads(FfnArgs a) {
  const int FW = a.W, FH = 2 * a.W, SLABF = FW * FH, t = threadIdx.x;
  const float* T1 = a.red;
  const float* T2 = a.red + SLABF;
  const float* s1 = a.red + 2 * SLABF;
  const float* s2 = s1 + FH;
  // every load before the first store (the gradient pointers may alias anything as far as the compiler knows: a store
  // inside the loops would make each iteration its own memory round trip)
  float w1v[8], w2v[8];   // SLABF <= 64 * 128 = 8 x 1024
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int i = t + 1024 * u;
    if (i < SLABF) {
      w1v[u] = fmaf(a.gamma[i / FH], T1[i], a.beta[i / FH] * s1[i % FH]);
      w2v[u] = a.row8 ? T2[(i % FW) * FH + i / FW] : T2[i];
    }
  }
  const float b1v = t < FH ? s1[t] : 0.f, b2v = t < FW ? s2[t] : 0.f;
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
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int i = t + 1024 * u;
    if (i < SLABF) { a.g_W1[i] = w1v[u]; a.g_W2[i] = w2v[u]; }
  }
  if (t < FH) a.g_b1[t] = b1v;
  if (t < FW) a.g_b2[t] = b2v;
  if (t < FW * 16 && part == 0) { a.g_gamma[c] = dg; a.g_beta[c] = db; }
}

// deterministic sum over the workgroup partials: 64 outputs per workgroup, partial axis over 16 waves with 8 loads in
// flight each (the loop is a chain of HBM round trips: 1024 partials are 8 trips per thread)
__global__ void __launch_bounds__(1024) k_ffn_sum(FfnArgs a) {
  const int FFN_PART = a.part_len;
  __shared__ float red[16][64];
  const int l = threadIdx.x & 63, o = blockIdx.x * 64 + l, pg = threadIdx.x >> 6;
  float v[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) v[u] = 0.f;
  if (o < FFN_PART) {
    int pi = pg;
    for (; pi + 112 < a.nwg; pi += 128)
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] += a.part[(size_t)(pi + 16 * u) * FFN_PART + o];
    for (; pi < a.nwg; pi += 16) v[0] += a.part[(size_t)pi * FFN_PART + o];
  }
  red[pg][l] = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
  __syncthreads();
  if (pg == 0 && o < FFN_PART) {
    float s = 0.f;
#pragma unroll
    for (int g = 0; g < 16; ++g) s += red[g][l];
    a.red[o] = s;
  }
}

// ============================================== width 8: one row per lane =====
// De = 8 (configs 3/4: the CIFAR10 / PATTERN edge channels).  A 16x16 MFMA tile is the wrong shape for an 8 -> 16 -> 8
// FFN (two 8-wide rows riding in one 16-wide row behind block-diagonal weights: half of every MFMA multiplies zeros, and the
// tile round trips through LDS made the W = 16 backward VALU/latency-bound at 0.18 of the HBM roof).  Here a lane owns one
// whole row: LayerNorm and the three channel contractions (128 FMAs each) are in-lane VALU work on v_pk_fma_f32 with the
// weights as wave-uniform SGPR pairs (s_load from the constant address space, re-fetched per chunk), x/dy/dx move as two
// 16-byte accesses per lane (a wave covers 2 KiB of contiguous HBM), and only the two weight-gradient contractions over the
// ROW axis go to the matrix pipe: the wave transposes [xhat | dy] and dpre / hid through a padded LDS image ([16][68] floats:
// conflict-free b32 column writes and b128 row reads) and contracts its 64 rows with 16 + 16 v_mfma_f32_16x16x4_f32.
typedef float v2f __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(4))) float* cfp;   // constant address space: uniform reads become s_load
#define F8_W1P 0      // gamma[c] W1[c][h]            [8][16]   (pairs over h: pre)
#define F8_W1PT 128   // gamma[c] W1[c][h] as [h][c]  [16][8]   (pairs over c: dxhat)
#define F8_W2T 256    // W2[h][o] as [o][h]           [8][16]   (pairs over h: dhid)
#define F8_W2 384     // W2[h][o]                     [16][8]   (pairs over o: y)
#define F8_B1P 512    // b1[h] + sum_c beta[c] W1[c][h]
#define F8_B2 528
#define F8_PREP_FLOATS 536
#define F8_PART 280   // per-workgroup partial: T1[c][h] 128 | T2^T[o][h] 128 | s1[h] 16 | s2[o] 8
#define F8_LD 68      // row pitch of the transposed LDS images (floats)

__global__ void __launch_bounds__(128) k_ffn8_prep(FfnArgs a) {
  const int t = threadIdx.x;
  float* w = a.x16;
  const int c = t >> 4, h = t & 15;
  const float v = a.gamma[c] * a.W1[c * 16 + h];
  w[F8_W1P + c * 16 + h] = v;
  w[F8_W1PT + h * 8 + c] = v;
  const float u = a.W2[h * 8 + c];   // (h, o = c)
  w[F8_W2 + h * 8 + c] = u;
  w[F8_W2T + c * 16 + h] = u;
  if (t < 16) {
    float s = a.b1[t];
    for (int k = 0; k < 8; ++k) s = fmaf(a.beta[k], a.W1[k * 16 + t], s);
    w[F8_B1P + t] = s;
  }
  if (t < 8) w[F8_B2 + t] = a.b2[t];
}

__device__ __forceinline__ v2f splat2(float v) { return (v2f){v, v}; }
__device__ __forceinline__ v2f ldw2(cfp w, int i) { return (v2f){w[i], w[i + 1]}; }

// the lane's row: two-pass moments, x -> xhat in place, returns rstd
__device__ __forceinline__ float ffn8_ln(float (&x)[8], float eps) {
  const float mu = (((x[0] + x[1]) + (x[2] + x[3])) + ((x[4] + x[5]) + (x[6] + x[7]))) * 0.125f;
  float v = 0.f;
#pragma unroll
  for (int c = 0; c < 8; ++c) { x[c] -= mu; v = fmaf(x[c], x[c], v); }
  const float rstd = rsqrtf(fmaf(v, 0.125f, eps));
#pragma unroll
  for (int c = 0; c < 8; ++c) x[c] *= rstd;
  return rstd;
}
// hid = act(W1p^T . xhat + b1p)
template <int ACT>
__device__ __forceinline__ void ffn8_hidden(cfp w, const float (&xh)[8], float (&hid)[16]) {
  v2f pre[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) pre[k] = ldw2(w, F8_B1P + 2 * k);
#pragma unroll
  for (int c = 0; c < 8; ++c)
#pragma unroll
    for (int k = 0; k < 8; ++k) pre[k] = ldw2(w, F8_W1P + c * 16 + 2 * k) * splat2(xh[c]) + pre[k];
#pragma unroll
  for (int k = 0; k < 8; ++k) { hid[2 * k] = ffn_act<ACT>(pre[k][0]); hid[2 * k + 1] = ffn_act<ACT>(pre[k][1]); }
}
__device__ __forceinline__ void ffn8_load(const float* src, long row, bool ok, float (&v)[8]) {
  float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
  if (ok) {
    lo = *reinterpret_cast<const float4*>(src + row * 8);
    hi = *reinterpret_cast<const float4*>(src + row * 8 + 4);
  }
  v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w; v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
}
// bf16 rows (EGT_BF16): 16 bytes, ONE access per lane
__device__ __forceinline__ void ffn8_load(const uint16_t* src, long row, bool ok, float (&v)[8]) {
  uint4 u = make_uint4(0u, 0u, 0u, 0u);
  if (ok) u = *reinterpret_cast<const uint4*>(src + row * 8);
  const float4 lo = bf4_to_f4(make_uint2(u.x, u.y)), hi = bf4_to_f4(make_uint2(u.z, u.w));
  v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w; v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
}
__device__ __forceinline__ void ffn8_store(float* dst, long row, float4 lo, float4 hi) {
  *reinterpret_cast<float4*>(dst + row * 8) = lo;
  *reinterpret_cast<float4*>(dst + row * 8 + 4) = hi;
}
__device__ __forceinline__ void ffn8_store(uint16_t* dst, long row, float4 lo, float4 hi) {   // rounded once, here (RNE)
  const uint2 l = f4_to_bf4(lo), h = f4_to_bf4(hi);
  *reinterpret_cast<uint4*>(dst + row * 8) = make_uint4(l.x, l.y, h.x, h.y);
}

template <int ACT, typename T>   // T: storage type of x / y (float, or uint16_t = bfloat16 bits)
__global__ void __launch_bounds__(256, 4) k_ffn8_fwd(FfnArgs a) {
  const int lane = threadIdx.x & 63;
  const long nchunk = (a.rows + 63) / 64, stride = (long)gridDim.x * 4;
  for (long ch = (long)blockIdx.x * 4 + (threadIdx.x >> 6); ch < nchunk; ch += stride) {
    const long row = ch * 64 + lane;
    const bool ok = row < a.rows;
    float x[8], xh[8], hid[16];
    ffn8_load(reinterpret_cast<const T*>(a.x), row, ok, x);
    cfp w = (cfp)a.x16;
    asm volatile("" : "+s"(w));   // per-chunk copy of the base: the weight fetches stay inside the loop (272 SGPRs do not exist)
#pragma unroll
    for (int c = 0; c < 8; ++c) xh[c] = x[c];
    ffn8_ln(xh, a.ln_eps);
    ffn8_hidden<ACT>(w, xh, hid);
    v2f y[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) y[k] = ldw2(w, F8_B2 + 2 * k);
#pragma unroll
    for (int h = 0; h < 16; ++h)
#pragma unroll
      for (int k = 0; k < 4; ++k) y[k] = ldw2(w, F8_W2 + h * 8 + 2 * k) * splat2(hid[h]) + y[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) y[k] = y[k] + (v2f){x[2 * k], x[2 * k + 1]};   // the residual joins after the chain, as in k_ffn_fwd
    if (ok)
      ffn8_store(reinterpret_cast<T*>(a.y), row, make_float4(y[0][0], y[0][1], y[1][0], y[1][1]),
                 make_float4(y[2][0], y[2][1], y[3][0], y[3][1]));
  }
}

#ifndef F8_BWD_OCC
#define F8_BWD_OCC 3   // waves per SIMD: 4 (128 registers) spills ~20 values per chunk
#endif
template <int ACT, typename T>
__global__ void __launch_bounds__(256, F8_BWD_OCC) k_ffn8_bwd(FfnArgs a) {
  __shared__ __attribute__((aligned(16))) float sm[4 * 2 * 16 * F8_LD];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m = lane & 15, kq = lane >> 4;
  float* tA = sm + wave * 2 * 16 * F8_LD;   // [xhat 0-7 | dy 8-15][row]
  float* tB = tA + 16 * F8_LD;              // dpre, then hid: [h][row]
  v4f accT1[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};   // [xhat | dy]^T . dpre : rows 0-7 = T1[c][h]
  v4f accT2[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};   // [xhat | dy]^T . hid  : rows 8-15 = T2^T[o][h]
  // bias gradients from the transposed images too: lane (m, kq) adds up the 16 rows it reads of dpre[h = m] and of
  // [xhat | dy][m] (one register each instead of 24 per-row accumulators)
  v4f sp4 = {0.f, 0.f, 0.f, 0.f}, sd4 = {0.f, 0.f, 0.f, 0.f};
  const long nchunk = (a.rows + 63) / 64, stride = (long)gridDim.x * 4;
  for (long ch = (long)blockIdx.x * 4 + wave; ch < nchunk; ch += stride) {
    const long row = ch * 64 + lane;
    const bool ok = row < a.rows;
    float xh[8], dy[8], hid[16], dp[16];
    ffn8_load(reinterpret_cast<const T*>(a.x), row, ok, xh);     // rows past the end are zero: xhat = dy = dpre = 0 add nothing to the sums
    ffn8_load(reinterpret_cast<const T*>(a.dy), row, ok, dy);
    cfp w = (cfp)a.x16;
    asm volatile("" : "+s"(w));
    const float rstd = ffn8_ln(xh, a.ln_eps);
    ffn8_hidden<ACT>(w, xh, hid);
    {   // dhid = W2 . dy ; dpre = dhid * act'(pre)
      v2f dh[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) dh[k] = splat2(0.f);
#pragma unroll
      for (int o = 0; o < 8; ++o)
#pragma unroll
        for (int k = 0; k < 8; ++k) dh[k] = ldw2(w, F8_W2T + o * 16 + 2 * k) * splat2(dy[o]) + dh[k];
#pragma unroll
      for (int h = 0; h < 16; ++h) dp[h] = dh[h >> 1][h & 1] * ffn_dact<ACT>(hid[h]);
    }
    // ---- weight gradients: transpose through LDS, contract the wave's 64 rows on the matrix pipe ----
    lds_sync();
#pragma unroll
    for (int c = 0; c < 8; ++c) { tA[c * F8_LD + lane] = xh[c]; tA[(8 + c) * F8_LD + lane] = dy[c]; }
#pragma unroll
    for (int h = 0; h < 16; ++h) tB[h * F8_LD + lane] = dp[h];
    lds_sync();
    v4f av[4], bv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      av[j] = *reinterpret_cast<const v4f*>(tA + m * F8_LD + 16 * kq + 4 * j);
      bv[j] = *reinterpret_cast<const v4f*>(tB + m * F8_LD + 16 * kq + 4 * j);
    }
    lds_sync();
    sp4 += (bv[0] + bv[1]) + (bv[2] + bv[3]);
    sd4 += (av[0] + av[1]) + (av[2] + av[3]);
#pragma unroll
    for (int h = 0; h < 16; ++h) tB[h * F8_LD + lane] = hid[h];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int u = 0; u < 4; ++u) accT1[u & 1] = MFMA(av[j][u], bv[j][u], accT1[u & 1]);
    lds_sync();
#pragma unroll
    for (int j = 0; j < 4; ++j) bv[j] = *reinterpret_cast<const v4f*>(tB + m * F8_LD + 16 * kq + 4 * j);
    // ---- dxhat = W1p . dpre ; LayerNorm backward ; dx = dy + ... ----
    v2f dxh[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) dxh[k] = splat2(0.f);
#pragma unroll
    for (int h = 0; h < 16; ++h)
#pragma unroll
      for (int k = 0; k < 4; ++k) dxh[k] = ldw2(w, F8_W1PT + h * 8 + 2 * k) * splat2(dp[h]) + dxh[k];
    float m1 = 0.f, m2 = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) { const float d = dxh[c >> 1][c & 1]; m1 += d; m2 = fmaf(d, xh[c], m2); }
    m1 *= 0.125f; m2 *= 0.125f;
    float o8[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) o8[c] = dy[c] + rstd * (dxh[c >> 1][c & 1] - m1 - xh[c] * m2);
    if (ok) ffn8_store(reinterpret_cast<T*>(a.dx), row, make_float4(o8[0], o8[1], o8[2], o8[3]), make_float4(o8[4], o8[5], o8[6], o8[7]));
    lds_sync();
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int u = 0; u < 4; ++u) accT2[u & 1] = MFMA(av[j][u], bv[j][u], accT2[u & 1]);
  }
  // ---- per-workgroup partial: the four waves add into one LDS image, one after the other (fixed order) ----
  __syncthreads();
  float* red = sm;   // [F8_PART]
  const v4f t1 = accT1[0] + accT1[1], t2 = accT2[0] + accT2[1];
  const v4f tt = kq < 2 ? t1 : t2;   // D[mrow = 4 kq + r][n = m]: rows 0-7 of T1, rows 8-15 of T2^T  ->  image index 16 mrow + n
  const float s1m = sum_over_q((sp4[0] + sp4[1]) + (sp4[2] + sp4[3]));   // s1[h = m]
  const float s2m = sum_over_q((sd4[0] + sd4[1]) + (sd4[2] + sd4[3]));   // m >= 8: s2[o = m - 8]
  for (int wv = 0; wv < 4; ++wv) {
    if (wave == wv) {
      const bool first = wv == 0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float* d = red + 16 * (4 * kq + r) + m;
        *d = first ? tt[r] : *d + tt[r];
      }
      if (kq == 0) {
        red[256 + m] = first ? s1m : red[256 + m] + s1m;
        if (m >= 8) red[264 + m] = first ? s2m : red[264 + m] + s2m;
      }
    }
    __syncthreads();
  }
  float* out = a.part + (size_t)blockIdx.x * F8_PART;
  for (int i = threadIdx.x; i < F8_PART; i += 256) out[i] = red[i];
}

// ------------------------------------------------------------------ host glue --
#define FFN_NWG 256   // W >= 48: at most one backward workgroup per CU (4 waves, 1 per SIMD: the 512-register kernel)
// narrower rows need < 128 registers and ~20 KB of LDS per workgroup: several workgroups per CU hide each other's latency
static size_t ffn_nwg_cap(size_t W) { return W <= 16 ? 1024 : (W <= 32 ? 512 : FFN_NWG); }   // (measured: 256 -> 1024 workgroups: 128 -> 96 us at De = 8; 1280/2048 no better)

static size_t ffn_al(size_t x) { return (x + 63) & ~(size_t)63; }

extern "C" int egt_ffn_supported(const egt_ffn_desc* d) {
  if (!d || (d->dtype != EGT_F32 && d->dtype != EGT_BF16) || d->rows <= 0) return 0;   // EGT_BF16: x, y, dy, dx in bf16
  if (d->matmul != EGT_MM_F32 && d->matmul != EGT_MM_BF16X3 && d->matmul != EGT_MM_BF16) return 0;
  if (d->width == 8) return d->matmul == EGT_MM_F32 && (d->activation == EGT_ACT_RELU || d->activation == EGT_ACT_ELU);   // VALU kernels: exact fp32 only
  if (d->width != 16 && d->width != 32 && d->width != 48 && d->width != 64) return 0;
  return d->activation == EGT_ACT_RELU || d->activation == EGT_ACT_ELU;
}

// Every launch and workspace decision of the fused FFN is made in ONE place, plan_ffn, once per C-ABI call: the size query returns
// its total, ffn_fill binds the workspace from it, the entry points launch from it.  Workspace, in floats (width 8 lays out as 16):
//   [slab1 slab2 slab3 slab4 | b1p | red | part x ffn_nwg_cap | sA1 sA2 sA3 sA4 (bf16 modes) | x16 (width 8: F8_* operands)]
// The storage dtype changes only the kernel instances (x / y / dy / dx as T): the workspace holds fp32 operands and partials in
// both, so an EGT_BF16 descriptor has the same plan sizes as its fp32 twin.
enum FfnFamily { FFN_ROW8, FFN_TILE };   // k_ffn8_* (one row per lane) | k_ffn_* (16-row tiles, every product mode)
struct FfnPlan {
  FfnFamily fam;
  bool bf16;   // desc.dtype == EGT_BF16: the uint16_t (bfloat16) storage instances
  int W;   // layout width
  int mm;  // desc.matmul: the product mode of the tile kernels' instances
  size_t slab, b1p, red, part, sA1, sA2, sA3, sA4, x16, total;
  int part_len;                 // floats per backward workgroup partial
  EgtLaunch prep, fwd, bwd;     // bwd.grid: backward workgroups (= partials)
};

static FfnPlan plan_ffn(const egt_ffn_desc* d) {
  FfnPlan P{};
  P.fam = d->width == 8 ? FFN_ROW8 : FFN_TILE;
  P.bf16 = d->dtype == EGT_BF16;
  P.mm = d->matmul;
  const size_t W = P.W = d->width == 8 ? 16 : d->width, TW = W / 16, NS1 = (TW + 1) / 2;
  const size_t slab = 2 * W * W, part = 2 * slab + 3 * W;                     // slab = W*2W floats; partial = T1 | T2 | s1 | s2
  const size_t a1 = 2 * TW * NS1 * 2 * 256, a2 = TW * TW * 2 * 256;           // sA1, sA3: [TH][NS1][2][256]; sA2, sA4: [TW][TW][2][256]
  P.slab = slab; P.b1p = 4 * slab; P.red = P.b1p + ffn_al(2 * W); P.part = P.red + ffn_al(part);
  P.sA1 = P.part + ffn_nwg_cap(W) * part; P.sA2 = P.sA1 + a1; P.sA3 = P.sA2 + a2; P.sA4 = P.sA3 + a1; P.x16 = P.sA4 + a2;
  P.total = P.x16 + 1280;
  auto clamp = [](long v, long hi) { return (int)(v < 1 ? 1 : (v > hi ? hi : v)); };
  const long tiles = (d->rows + 15) / 16;
  if (P.fam == FFN_ROW8) {   // one row per lane: 64-row waves, 4 per workgroup
    const long want = (((d->rows + 63) / 64) + 3) / 4;
    P.part_len = F8_PART;
    P.prep = {1, 128, 0};
    P.fwd = {clamp(want, 2048), 256, 0};
    P.bwd = {clamp(want, 1024), 256, 0};
    return P;
  }
  P.part_len = (int)part;
  // the slabs the kernels stage (FFN_SLABS): s1f floats each of the W -> 2W operands, s2f of the 2W -> W ones.  The bf16 modes' forward
  // is HBM-bound and takes twice the workgroups.
  const bool bf = P.mm != EGT_MM_F32;
  const size_t s1f = bf ? a1 : slab, s2f = bf ? a2 : slab;
  P.prep = {(int)(((s1f > s2f ? s1f : s2f) + 255) / 256), 256, 0};
  P.fwd = {clamp((tiles + 7) / 8, bf ? 512 : 256), 512, (s1f + s2f + 3 * W + 8 * 2 * 16 * W) * 4};
  // backward workgroups: one per CU for large inputs; small inputs (node channels) one tile per wave (a tile is ~16 us of dependent
  // work: spreading beats amortising the slab staging).  LDS: the operand slabs, with the partial staged over them at the end
  const size_t slabs = 2 * s1f + s2f;
  P.bwd = {clamp((tiles + 3) / 4, (long)ffn_nwg_cap(W)), 256, ((slabs > part ? slabs : part) + 2 * W + 4 * 3 * 16 * W) * 4};
  return P;
}

extern "C" size_t egt_ffn_workspace_bytes(const egt_ffn_desc* d) {
  if (!egt_ffn_supported(d)) return 0;
  return plan_ffn(d).total * sizeof(float);
}

static int ffn_fill(const egt_ffn_desc* d, const egt_ffn_params* p, void* ws, FfnPlan& P, FfnArgs& a) {
  if (!d || !p || !ws) EGT_FAIL(EGT_E_NULL, "desc/params/workspace is NULL");
  if (!egt_ffn_supported(d))
    EGT_FAIL(d->dtype != EGT_F32 && d->dtype != EGT_BF16 ? EGT_E_DTYPE : EGT_E_SHAPE,
             "fused FFN covers widths 16/32/48/64 (and 8 with exact fp32 products), fp32 or bf16 x/y, relu/elu "
             "(got width %d, rows %lld, dtype %d, act %d, matmul %d)", d->width, (long long)d->rows, d->dtype, d->activation, d->matmul);
  if (!p->norm_gamma || !p->norm_beta || !p->lr1_kernel || !p->lr1_bias || !p->lr2_kernel || !p->lr2_bias)
    EGT_FAIL(EGT_E_NULL, "an FFN parameter pointer is NULL");
  P = plan_ffn(d);
  a = FfnArgs{};
  a.rows = d->rows; a.ln_eps = d->ln_eps; a.W = d->width;
  a.gamma = (const float*)p->norm_gamma; a.beta = (const float*)p->norm_beta;
  a.W1 = (const float*)p->lr1_kernel; a.b1 = (const float*)p->lr1_bias;
  a.W2 = (const float*)p->lr2_kernel; a.b2 = (const float*)p->lr2_bias;
  float* w = (float*)ws;
  a.slab1 = w; a.slab2 = w + P.slab; a.slab3 = w + 2 * P.slab; a.slab4 = w + 3 * P.slab;
  a.b1p = w + P.b1p; a.red = w + P.red; a.part = w + P.part;
  a.sA1 = reinterpret_cast<uint16_t*>(w + P.sA1); a.sA2 = reinterpret_cast<uint16_t*>(w + P.sA2);
  a.sA3 = reinterpret_cast<uint16_t*>(w + P.sA3); a.sA4 = reinterpret_cast<uint16_t*>(w + P.sA4);
  a.x16 = w + P.x16;
  a.part_len = P.part_len; a.row8 = P.fam == FFN_ROW8; a.nwg = P.bwd.grid;
  return EGT_OK;
}

// one instance of the tile kernels: width W, activation ACT, products MM, storage T of x / y / dy / dx
template <int W, int ACT, int MM, typename T>
static void ffn_launch_tiles(const FfnPlan& P, const FfnArgs& a, bool bwd, bool prep, hipStream_t st) {
  if (prep) EGT_LAUNCH("k_ffn_prep", (k_ffn_prep<W, MM>), dim3(P.prep.grid), dim3(P.prep.block), P.prep.lds, st, a);
  if (bwd) egt_launch_planned<k_ffn_bwd<W, ACT, MM, T>>("k_ffn_bwd", P.bwd, st, a);
  else egt_launch_planned<k_ffn_fwd<W, ACT, MM, T>>("k_ffn_fwd", P.fwd, st, a);
}
// the planned family's instance for storage T: the row-per-lane kernels by activation, the tile kernels by (W, MM, ACT)
template <typename T>
static void ffn_launch_t(const FfnPlan& P, const FfnArgs& a, int act, bool bwd, bool prep, hipStream_t st) {
  const bool relu = act == EGT_ACT_RELU;
  if (P.fam == FFN_ROW8) {
    if (prep) EGT_LAUNCH("k_ffn_prep", k_ffn8_prep, dim3(P.prep.grid), dim3(P.prep.block), P.prep.lds, st, a);
    const EgtLaunch& s = bwd ? P.bwd : P.fwd;
    if (bwd && relu) EGT_LAUNCH("k_ffn_bwd", (k_ffn8_bwd<EGT_ACT_RELU, T>), dim3(s.grid), dim3(s.block), s.lds, st, a);
    else if (bwd) EGT_LAUNCH("k_ffn_bwd", (k_ffn8_bwd<EGT_ACT_ELU, T>), dim3(s.grid), dim3(s.block), s.lds, st, a);
    else if (relu) EGT_LAUNCH("k_ffn_fwd", (k_ffn8_fwd<EGT_ACT_RELU, T>), dim3(s.grid), dim3(s.block), s.lds, st, a);
    else EGT_LAUNCH("k_ffn_fwd", (k_ffn8_fwd<EGT_ACT_ELU, T>), dim3(s.grid), dim3(s.block), s.lds, st, a);
    return;
  }
#define FFN_TILE_CASE(W, MM)                                                                              \
  case (W) * 4 + (MM):                                                                                    \
    if (relu) ffn_launch_tiles<W, EGT_ACT_RELU, MM, T>(P, a, bwd, prep, st);                              \
    else ffn_launch_tiles<W, EGT_ACT_ELU, MM, T>(P, a, bwd, prep, st);                                    \
    break;
#define FFN_TILE_CASES(W) FFN_TILE_CASE(W, EGT_MM_F32) FFN_TILE_CASE(W, EGT_MM_BF16X3) FFN_TILE_CASE(W, EGT_MM_BF16)
  switch (P.W * 4 + P.mm) {   // (egt_ffn_supported has passed: the widths and modes below are all there are)
    FFN_TILE_CASES(16) FFN_TILE_CASES(32) FFN_TILE_CASES(48) FFN_TILE_CASES(64)
  }
#undef FFN_TILE_CASES
#undef FFN_TILE_CASE
}
// prep (unless a backward finds its workspace prepared), then the planned family's forward / backward instance
static void ffn_launch(const FfnPlan& P, const FfnArgs& a, int act, bool bwd, bool prep, hipStream_t st) {
  if (P.bf16) ffn_launch_t<uint16_t>(P, a, act, bwd, prep, st);
  else ffn_launch_t<float>(P, a, act, bwd, prep, st);
}

extern "C" int egt_ffn_fwd(const egt_ffn_desc* desc, const egt_ffn_params* params, const void* x, void* y,
                           void* workspace, void* stream) {
  FfnPlan P; FfnArgs a;
  int rc = ffn_fill(desc, params, workspace, P, a);
  if (rc) return rc;
  if (!x || !y) EGT_FAIL(EGT_E_NULL, "x/y is NULL");
  a.x = (const float*)x; a.y = (float*)y;
  ffn_launch(P, a, desc->activation, false, true, (hipStream_t)stream);
  EGT_HIP_LAUNCH_CHECK("egt_ffn_fwd");
  return EGT_OK;
}

extern "C" int egt_ffn_bwd(const egt_ffn_desc* desc, const egt_ffn_params* params, const void* x, const void* dy,
                           void* dx, const egt_ffn_params* grads, void* workspace, void* stream) {
  FfnPlan P; FfnArgs a;
  int rc = ffn_fill(desc, params, workspace, P, a);
  if (rc) return rc;
  if (!x || !dy || !dx || !grads) EGT_FAIL(EGT_E_NULL, "x/dy/dx/grads is NULL");
  if (!grads->norm_gamma || !grads->norm_beta || !grads->lr1_kernel || !grads->lr1_bias || !grads->lr2_kernel || !grads->lr2_bias)
    EGT_FAIL(EGT_E_NULL, "an FFN gradient pointer is NULL");
  a.x = (const float*)x; a.dy = (const float*)dy; a.dx = (float*)dx;
  a.g_gamma = (float*)grads->norm_gamma; a.g_beta = (float*)grads->norm_beta;
  a.g_W1 = (float*)grads->lr1_kernel; a.g_b1 = (float*)grads->lr1_bias;
  a.g_W2 = (float*)grads->lr2_kernel; a.g_b2 = (float*)grads->lr2_bias;
  hipStream_t st = (hipStream_t)stream;
  // EGT_FFN_WS_PREPARED: the forward's workspace, its prepared operands are still there (the bf16 modes read their own slabs and b1p
  // only: k_ffn_prep<W, MM> writes all of that)
  ffn_launch(P, a, desc->activation, true, !(desc->flags & EGT_FFN_WS_PREPARED), st);
  EGT_LAUNCH("k_ffn_sum", k_ffn_sum, dim3((P.part_len + 63) / 64), dim3(1024), 0, st, a);
  EGT_LAUNCH("k_ffn_param_grads", k_ffn_param_grads, dim3(1), dim3(1024), 0, st, a);
  EGT_HIP_LAUNCH_CHECK("egt_ffn_bwd");
  return EGT_OK;
}
