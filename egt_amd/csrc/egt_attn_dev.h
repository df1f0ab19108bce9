// Device side of the d in {16,32,64}, H = 8 family: what the MFMA inner-op kernels (egt_attn_kernels.h: k_attn_mfma_fwd / _bwd_kv /
// _bwd_q, one body each for the exact-fp32 and the bf16-product operand form) and the fused pair operator (egt_pair.h: k_pair_fwd /
// k_pair_bwd) share -- arguments, LDS layouts, LDS-DMA, and ONE copy of every attention phase: the key terms of a slot, the forward
// and the backward elementwise unit, the fp32 MFMA contractions and the bf16 form's primitives, the backward's operand addresses, the
// forward's finalize.  The phases are pure arithmetic, LDS accesses and MFMAs: every wait, barrier, priority change, scheduling
// fence and stamp stays in the kernel bodies, whose instruction order is pinned there.
#pragma once
#include <limits.h>

#include "egt_common.h"
#include "egt_stamps.h"

typedef float v4f __attribute__((ext_vector_type(4)));

#define AH 8
#define L2E 1.4426950408889634f
#define KEY_OFF (-3.0e38f)   // additive term of key slots past N (below every masked logit, above -inf)

// packed operand arrays, each B*H*NP*d floats, in workspace order: Q rows (pre-scaled), K rows, V^T (what the forward
// reads), V rows, K^T, dO rows (the backward's); then stats2 and dA (the layout: plan_attn).  A forward launched with
// EGT_ATTN_WS_SHARED packs the five q/k/v arrays once and the backward, given the same workspace, adds only dO.
enum { PK_QH = 0, PK_KH, PK_VT, PK_FWD_COUNT, PK_VH = PK_FWD_COUNT, PK_KT, PK_OH, PK_COUNT };
enum { PACK_Q = 1, PACK_KH = 2, PACK_KT = 4, PACK_VT = 8, PACK_VH = 16, PACK_O = 32 };

struct AttnMfmaArgs {
  int B, N, NP, d;
  uint32_t flags;
  float clip_lo, clip_hi, scale;
  uint32_t rm_thr, s0, s1;
  int rng_rm;
  const float *qkv, *E, *G, *M;
  const uint8_t *km, *rm;
  float *v_att, *h_hat, *rowstats;
  float* pk;   // packed arrays
  // backward
  const float *v_att_in, *d_v_att, *d_h_ext;
  float *d_qkv, *d_E, *d_G, *ws_dA, *stats2;
  int pack_what;   // PACK_* bits
};

// Phase stamps (egt_stamps.h; measurement builds only).  Slots of this unit: a kernel's compute / attention waves and the pair kernels'
// edge waves stamp different phases (the loader waves of k_attn_mfma_fwd / _bwd_kv do not stamp)
enum { ST_ATTN_FWD, ST_ATTN_BWD_KV, ST_PAIR_FWD_ATT, ST_PAIR_FWD_EDGE, ST_PAIR_BWD_ATT, ST_PAIR_BWD_EDGE, ST_COUNT };
EGT_STAMP_UNIT(ST_COUNT);
// timing ablations (results are wrong): -DEGT_ATTN_ABL=<bits>: 1 no operand DMA, 2 no pair loads / scatter, 4 no output stores,
// 8 no MFMAs (MFMA becomes one multiply-add), 32 no dA DMA in k_attn_mfma_bwd_q
#ifndef EGT_ATTN_ABL
#define EGT_ATTN_ABL 0
#endif
#define ABL(bit) ((EGT_ATTN_ABL & (bit)) == 0)
#if EGT_ATTN_ABL & 8
__device__ __forceinline__ v4f MFMA(float a, float b, v4f c) { c[0] += a * b; return c; }
#else
#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)
#endif

// ---- the bf16 operand form (MM = 1: egt_attn_desc.reserved & EGT_ATTN_MM_BF16): products on v_mfma_f32_16x16x16_bf16 / _16x16x32_bf16,
// fp32 accumulate.  The fp32 form's contraction order kappa(T, u, q) = 16 T + 4 q + u gives a lane (row, q) the four consecutive
// channels 16 T + 4 q .. + 3 of its row in one 16-byte fragment: exactly the K = 16 bf16 operand (lane l: A[l & 15][4 (l >> 4) + j]).
// Four fp32 MFMAs (u = 0..3) become ONE bf16 MFMA on the fragment packed with v_cvt_pk_bf16_f32.
typedef short v4s __attribute__((ext_vector_type(4)));
typedef short v8s __attribute__((ext_vector_type(8)));
typedef __bf16 v2b __attribute__((ext_vector_type(2)));
typedef float v2f __attribute__((ext_vector_type(2)));
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x16bf16_1k((a), (b), (c), 0, 0, 0)
#define MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16((a), (b), (c), 0, 0, 0)
// (lo, hi) -> one dword of two bf16, round to nearest even (v_cvt_pk_bf16_f32)
__device__ __forceinline__ unsigned pk_bf16(float lo, float hi) {
  const v2f x = {lo, hi};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(x, v2b));
}
__device__ __forceinline__ float bf16_round(float x) { return __uint_as_float(pk_bf16(x, x) << 16); }
__device__ __forceinline__ v4s bf4(float x0, float x1, float x2, float x3) {
  union { unsigned u[2]; v4s s; } r;
  r.u[0] = pk_bf16(x0, x1); r.u[1] = pk_bf16(x2, x3);
  return r.s;
}
__device__ __forceinline__ v4s bf4(const float4& v) { return bf4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ v4s bf4(const float (&v)[4]) { return bf4(v[0], v[1], v[2], v[3]); }
__device__ __forceinline__ v8s cat8(v4s a, v4s b) { return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7); }
// c += sum over the d channels of a lane's fragments: a[T], b[T] = channels 16 T + 4 q .. + 3 of the lane's row.  Two channel blocks
// pair into one K = 32 MFMA for d >= 32 (both operands take the same (2 T', 2 T' + 1) pairing: the contraction order is free);
// d = 16 is one K = 16 MFMA -- no zero padding.
template <int KT>
__device__ __forceinline__ v4f dot_d(const v4s (&a)[KT], const v4s (&b)[KT], v4f c) {
  if constexpr (KT == 1) {
    return MFMA16(a[0], b[0], c);
  } else {
#pragma unroll
    for (int t = 0; t < KT / 2; ++t) c = MFMA32(cat8(a[2 * t], a[2 * t + 1]), cat8(b[2 * t], b[2 * t + 1]), c);
    return c;
  }
}

// What the operand form MM of a kernel decides beside its contractions: the type of a fragment that stays in registers across the
// trips (Frag: K / V of the backward), of a dA element in the workspace (DA), and how a fragment read from the operand arrays takes
// its form (cvt).
template <int MM> struct AttnForm;
template <> struct AttnForm<0> {
  typedef float4 Frag;
  typedef float DA;
  static __device__ __forceinline__ const float4& cvt(const float4& v) { return v; }
};
template <> struct AttnForm<1> {
  typedef v4s Frag;
  typedef unsigned short DA;
  static __device__ __forceinline__ v4s cvt(const float4& v) { return bf4(v.x, v.y, v.z, v.w); }
};
// a lane's four dA values of its tile (element offset in `dst`): 16 bytes of fp32, or the 8 bytes packed for dK
__device__ __forceinline__ void da_store(float* dst, const float (&da)[4]) { *reinterpret_cast<float4*>(dst) = make_float4(da[0], da[1], da[2], da[3]); }
__device__ __forceinline__ void da_store(unsigned short* dst, v4s da) {
  union { v4s s; uint2 u; } pk;
  pk.s = da;
  *reinterpret_cast<uint2*>(dst) = pk.u;
}

// LDS hand-off between the waves of a workgroup WITHOUT draining vector memory: __syncthreads() is
// s_waitcnt vmcnt(0) lgkmcnt(0) + s_barrier on gfx950; the operand prefetches and the output stores of
// these kernels must stay in flight across the barrier, and nothing here communicates through global memory.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__device__ __forceinline__ float pair_max_q(float v) {   // max over lanes l, l+16, l+32, l+48
  auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
  auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}
__device__ __forceinline__ float pair_sum_q(float v) { return sum_xor32(sum_xor16(v)); }
__device__ __forceinline__ float exp2_fast(float x) { return __builtin_amdgcn_exp2f(x); }

// Feature set of a kernel instance.  V = 0 reads every switch at run time (any combination);
// V = 1 / 2 are the straight-line instances of the main configuration (edge bias + gates + key
// padding + clip, no attention-mask tensor, no injected mask bytes; 2 = in-kernel random mask).
// (The pair kernels are V = 1 / 2 only and take `clip` from the flags all the same.)
template <int V>
struct Feat {
  bool E, G, M, km, clip, rmb, rng, X;
  __device__ __forceinline__ Feat(const AttnMfmaArgs& a) {
    E = V ? true : a.E != nullptr;
    G = V ? true : (a.flags & EGT_F_GATE_INPUT) != 0;
    M = V ? false : a.M != nullptr;
    km = V ? true : a.km != nullptr;
    clip = V ? true : (a.flags & EGT_F_CLIP) != 0;
    rmb = V ? false : a.rm != nullptr;
    rng = V == 2 ? true : (V == 1 ? false : a.rng_rm != 0);
    X = V ? true : a.d_h_ext != nullptr;
  }
};

// ---- pair-tile planes: a [16 rows][16 cols x 8 heads] tile of a [B,N,N,8] tensor lives in LDS HEAD-MAJOR: eight planes of stride PT_PL.
//   forward planes  [query row][key]: the wave that owns head h reads the four consecutive keys of its lane with
//     one ds_read_b128; rows 4..7 / 12..15 pair-swapped, 4-column chunks XORed with (row>>1)&3;
//   backward planes [key][query row]: lane (key, q) moves query rows 4q..4q+3 with one b128; chunk XOR (0,2,3,1)[key>>2].
// tools/lds_bank_check.py enumerates every pattern against the gfx950 lane-group tables: all conflict free except the
// backward's 4 x b32 cooperative scatter / gather (4-way: 8 array cycles under a 4-cycle issue, 2 x).
#define PT_PL 260

__device__ __forceinline__ int pt_off(int row, int m) {
  return ((row ^ ((row >> 2) & 1)) << 4) + ((((m >> 2) ^ (row >> 1)) & 3) << 2) + (m & 3);
}
__device__ __forceinline__ int ptT_off(int row, int col) {
  const int c2 = col >> 2;
  const int a = (0x78 >> (2 * c2)) & 3;   // (0, 2, 3, 1)[c2]
  return (col << 4) + ((((row >> 2) ^ a) & 3) << 2) + (row & 3);
}

// ---- producer / consumer split (tools/micro/mfma_stream.hip, profiles/r04_attn5_microbench.md) ----------------
// One global_load in an fp32 MFMA stream costs the issuing wave ~80 cycles (= 2.5 MFMAs), a ds_read_b128 ~7; LDS-DMA
// loader waves on the same SIMDs move 18 TB/s without slowing a compute wave's MFMA stream (33.7 vs 32 cycles per
// MFMA).  So a workgroup is 4 COMPUTE waves (one per SIMD, one head each: ds_read + MFMA + VALU only) and 4 LOADER
// waves: operand tiles by LDS-DMA (global_load_lds_dwordx4: no VGPR, no ds_write) one iteration ahead, pair tiles
// HBM -> registers -> head-major planes two iterations ahead, output planes -> HBM one iteration behind.  One
// s_barrier per iteration, which does not drain vector memory.
//
// Operand tile in LDS: the packed [T][16 rows][16 channels] block with the four 16-byte chunks of a row XORed by
// (0,2,3,1)[row >> 2] (done by the DMA's lane -> source mapping: LDS slot s of a 1 KB piece receives row s >> 2,
// chunk (s & 3) ^ a[s >> 4]): the row-form fragment reads (lane (row, q): ds_read_b128 of chunk q) are bank-conflict
// free and the transposed reads (lane (channel, q): ds_read_b32 of rows 4q + r) 2-way (tools/lds_bank_check.py).
__device__ __forceinline__ unsigned lds_addr(const void* p) { return (unsigned)(uintptr_t)p; }   // LDS byte address of a __shared__ pointer
__device__ __forceinline__ int chunk_xor(int row) { return (0x78 >> (2 * (row >> 2))) & 3; }      // (0, 2, 3, 1)[row >> 2]
// one 1 KB piece HBM -> LDS (any LDS address: tools/micro/dma_hi.hip): lane i lands at lds + 16 i and fetches src + off
__device__ __forceinline__ void dma_piece(unsigned lds, const float* src, unsigned off) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %1\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "s"(src), "v"(off), "s"(lds) : "memory");
}
__device__ __forceinline__ unsigned dma_lane_off(int lane) {   // source byte offset (inside a 1 KB block) of the chunk that lands in slot `lane`
  return (unsigned)((lane >> 2) * 64 + (((lane & 3) ^ chunk_xor(lane >> 2)) << 4));
}
#define OPS_STAGE 32768   // bytes of one operand stage: 4 heads x (two 4 KB tiles)
#define OPS_BYTES (2 * OPS_STAGE)
// launch geometry of the inner-op kernels (egt_attn_kernels.h, both operand forms: one plan, plan_attn)
#define FQ 2         // forward: query tiles per compute wave
#define BK 2         // backward: key tiles per compute wave
#define QW_TILES 8   // dQ: query tiles per workgroup
#define QW_STAGES 4  // dQ: LDS ring; the DMA of a stage is issued QW_STAGES - 1 trips ahead of its use (issue -> landed is ~1.1 us, a trip ~1 us)

// ================================================================ the phases =====
// element (graph b, query row l, key m, head h) of a [B,N,N,8] tensor: the index of the mask bytes and of the mask hash (< 2^32: *_supported)
__device__ __forceinline__ uint32_t pair_elem(int b, int N, int l, int m, int h) { return (uint32_t)((((size_t)b * N + l) * N + m) * AH + h); }

// additive mask of one element beyond its key term, in the reference's order (egt_layers.py:96-108); Feat<1> reduces it to nothing,
// Feat<2> to the hash
template <int V>
__device__ __forceinline__ float mask_extra(const AttnMfmaArgs& a, const Feat<V>& f, float mval, uint32_t gi) {
  float add = 0.f;
  if (f.M) add += (mval - 1.0f) * EGT_NEG;
  if (f.rmb || f.rng) {
    const bool hit = f.rmb ? (a.rm[gi] != 0) : ((egt_hash32(gi, a.s0, a.s1) >> 8) < a.rm_thr);
    add += hit ? -EGT_NEG : 0.0f;
  }
  return add;
}

// Key terms of key slot m of graph b (km: the [B,N] key-mask bytes, read only if has_km): ka is added to the logit (0, -EGT_NEG for a
// masked key, KEY_OFF past N: no selects in the loops), kg to the gate's exponent (-ka log2 e; past N the gate is rcp(1 + exp2(3e38)) = 0).
__device__ __forceinline__ void key_terms(int b, int m, int N, bool has_km, const uint8_t* km, float& ka, float& kg) {
  float t = 0.f;   // (a local: ka may be an LDS slot, which the byte load below could alias)
  if (m >= N) t = KEY_OFF;
  else if (has_km && km[(size_t)b * N + m] == 0) t = -EGT_NEG;
  ka = t;
  kg = m >= N ? 3.0e38f : -t * L2E;
}

// Forward elementwise unit: one 16 x 16 tile of logits of one (query tile | head) in a lane's S^T layout (keys mk0 + r of query row lq;
// key indices clamped to mmax for the mask lookups): clip, + E -> H_hat (hv4: post-clip, pre-mask, egt_layers.py:85-86), additive masks,
// gate, online softmax over the 16 keys (in-lane over r, then across q), rescale of the O accumulators.  pa: gated, unnormalised
// probabilities = the B operand of A.V.  kg4 is read by V = 1 only (elsewhere the gate's exponent needs the whole additive term).
template <int V, int KT>
__device__ __forceinline__ void attn_fwd_unit(const AttnMfmaArgs& a, const Feat<V>& f, bool clip, bool gated, const v4f& s, const float4& e4,
                                              const float4& g4, const float4& m4, const float4& ka4, const float4& kg4, int b, int lq, int mk0,
                                              int mmax, int h, float& mrun, float& lrun, v4f (&oacc)[KT], float (&pa)[4], float (&hv4)[4]) {
  float x[4];
  float tmax = KEY_OFF;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float ah = s[r];
    if (clip) ah = __builtin_amdgcn_fmed3f(ah, a.clip_lo, a.clip_hi);
    const float hv = ah + f4get(e4, r);
    hv4[r] = hv;
    float add = f4get(ka4, r);
    if (V != 1) add += mask_extra(a, f, f4get(m4, r), pair_elem(b, a.N, lq, min(mk0 + r, mmax), h));
    x[r] = hv + add;
    tmax = fmaxf(tmax, x[r]);
    if (gated) {   // sigmoid(G + add); masked -> exp2(+1.4e9) = inf -> rcp = 0 exactly, as the reference's fp32 path
      const float tg = V == 1 ? exp2_fast(fmaf(f4get(g4, r), -L2E, f4get(kg4, r))) : exp2_fast((f4get(g4, r) + add) * -L2E);
      pa[r] = __builtin_amdgcn_rcpf(1.0f + tg);
    } else {
      pa[r] = 1.0f;
    }
  }
  tmax = pair_max_q(tmax);
  const float mnew = fmaxf(mrun, tmax);
  const float alpha = exp2_fast((mrun - mnew) * L2E);
  float psum = 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float pexp = exp2_fast((x[r] - mnew) * L2E);   // keys past N: exp2(-inf) = 0
    psum += pexp;
    pa[r] *= pexp;
  }
  psum = pair_sum_q(psum);
  lrun = fmaf(lrun, alpha, psum);
  mrun = mnew;
#pragma unroll
  for (int kt = 0; kt < KT; ++kt) {
    v4f o = oacc[kt];
    o[0] *= alpha; o[1] *= alpha; o[2] *= alpha; o[3] *= alpha;
    oacc[kt] = o;
  }
}

// Backward elementwise unit: one 16 x 16 tile of one (key tile | head) in a lane's S layout (key mc, query rows lq0 + r clamped to mmax
// for the mask lookups; stc[r] = (m, 1/l, delta) of row r): clip, masks, S = exp2((x - m) log2 e) / l, gate, then at = S g (B operand of
// dV), dH -> dE4, da = dH where the clip passes the gradient (B operand of dK; the dA tile), dG4; hv4 = H_hat again (the pair kernel's
// dense_edge_r backward reads it).  An attention-mask tensor arrives folded into e4 / g4.
template <int V>
__device__ __forceinline__ void attn_bwd_unit(const AttnMfmaArgs& a, const Feat<V>& f, bool clip, bool gated, const v4f& s, const v4f& dp,
                                              const float4& e4, const float4& g4, const float4& x4, const float4 (&stc)[4], float ka, float kg,
                                              int b, int lq0, int mc, int mmax, int h, float (&at)[4], float (&da)[4], float (&dE4)[4],
                                              float (&dG4)[4], float (&hv4)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float araw = s[r];
    float ah = araw;
    if (clip) ah = __builtin_amdgcn_fmed3f(araw, a.clip_lo, a.clip_hi);
    float add = ka;
    if (V != 1) add += mask_extra(a, f, 1.0f, pair_elem(b, a.N, min(lq0 + r, mmax), mc, h));
    const float hv = ah + f4get(e4, r);
    const float xx = hv + add;
    const float S = exp2_fast((xx - stc[r].x) * L2E) * stc[r].y;   // rows past N: 1/l = 0; keys past N: exp2(-inf) = 0
    float g = 1.0f;
    if (gated) {
      const float tg = V == 1 ? exp2_fast(fmaf(f4get(g4, r), -L2E, kg)) : exp2_fast((f4get(g4, r) + add) * -L2E);
      g = __builtin_amdgcn_rcpf(1.0f + tg);
    }
    const float dAt_ = dp[r];
    const float Sg = S * g;
    const float dH = fmaf(S, fmaf(dAt_, g, -stc[r].z), f4get(x4, r));
    at[r] = Sg;
    da[r] = (clip && ah != araw) ? 0.f : dH;   // clip passes the gradient where lo <= x <= hi
    dE4[r] = dH;
    dG4[r] = gated ? dAt_ * Sg * (1.0f - g) : 0.f;
    hv4[r] = hv;
  }
}

// ---- MFMA contractions.  U units (query tiles / key tiles / heads) run side by side; contraction order kappa(T, u, q) = 16 T + 4 q + u.
// Forward: the streamed fragments (K rows, V^T) are shared by the units (NF = 1: the two query tiles of k_attn_mfma_fwd, every register
// feeds two MFMAs) or one per unit (NF = U: the two heads of k_pair_fwd).
//   S^T[m][l] = sum_k K[m][k] (d^-1/2 Q)[l][k]
template <int U, int NF, int KT>
__device__ __forceinline__ void mfma_s(const float4 (&kc)[NF][KT], const float (&Qr)[U][4 * KT], v4f (&s)[U]) {
  static_assert(NF == 1 || NF == U, "shared fragments or one per unit");
#pragma unroll
  for (int i = 0; i < U; ++i) s[i] = (v4f){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int T = 0; T < KT; ++T)
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int i = 0; i < U; ++i) s[i] = MFMA(f4get(kc[NF == 1 ? 0 : i][T], u), Qr[i][4 * T + u], s[i]);
}
//   O^T[k][l] += sum_m V^T[k][m] P^T[m][l]  (contraction order m = 4q + r)
template <int U, int NF, int KT>
__device__ __forceinline__ void mfma_pv(const float4 (&vc)[NF][KT], const float (&pa)[U][4], v4f (&oacc)[U][KT]) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
      for (int i = 0; i < U; ++i) oacc[i][kt] = MFMA(f4get(vc[NF == 1 ? 0 : i][kt], r), pa[i][r], oacc[i][kt]);
}
// Backward: the Q / dO fragments of the query tile are shared by the U units (the two key tiles of k_attn_mfma_bwd_kv; k_pair_bwd works
// on one head at a time: U = 1), whose K / V fragments and accumulators are rows of the callers' arrays.
//   S[l][m] = sum_k (d^-1/2 Q)[l][k] K[m][k] ; dP[l][m] = sum_k dO[l][k] V[m][k]
template <int U, int KT>
__device__ __forceinline__ void mfma_s_dp(const float4 (&qa)[KT], const float4 (&oa)[KT], const float4 (*Kr)[KT], const float4 (*Vr)[KT], v4f* s,
                                          v4f* dp) {
#pragma unroll
  for (int i = 0; i < U; ++i) { s[i] = (v4f){0.f, 0.f, 0.f, 0.f}; dp[i] = (v4f){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
  for (int T = 0; T < KT; ++T)
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int i = 0; i < U; ++i) {
        s[i] = MFMA(f4get(qa[T], u), f4get(Kr[i][T], u), s[i]);
        dp[i] = MFMA(f4get(oa[T], u), f4get(Vr[i][T], u), dp[i]);
      }
}
//   dV^T[k][m] += sum_l dO[l][k] A[l][m] ; dK^T[k][m] += sum_l (d^-1/2 Q)[l][k] dA[l][m]: the transposed operands from the same LDS
//   tiles (Q tile, then dO tile KT blocks behind it), just in time
template <int U, int KT>
__device__ __forceinline__ void mfma_dv_dk(const float* opt_e, const float* opt_o, const float (*at)[4], const float (*da)[4], v4f (*dVacc)[KT],
                                           v4f (*dKacc)[KT]) {
#pragma unroll
  for (int kt = 0; kt < KT; ++kt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float* opt = (r & 1) ? opt_o : opt_e;
      const float qq = opt[kt * 256 + r * 16];
      const float oo = opt[KT * 256 + kt * 256 + r * 16];
#pragma unroll
      for (int i = 0; i < U; ++i) {
        dVacc[i][kt] = MFMA(oo, at[i][r], dVacc[i][kt]);
        dKacc[i][kt] = MFMA(qq, da[i][r], dKacc[i][kt]);
      }
    }
}

// Backward operand tiles (Q, then dO) of one head at `base`, lane (mm = lane & 15, q): row form = lane (row mm, chunk q), one b128 per
// k-tile; transposed form = lane (channel mm, q): rows 4q + r, dword mm & 3 of chunk mm >> 2, one b32 per step.
// Tile row rho lives in LDS row rho ^ ((rho >> 2) & 1) (rows 4-7 and 12-15 swapped in pairs; the DMA's lane -> source mapping does it
// for free: dma_lane_off_swapped): the transposed b32 reads of a 32-lane group touch tile rows r and 4 + r, which 16-float rows put on the
// same 16 banks (2-way on the 32 reads of a tile); swapped, row 4 + r sits in an odd-even exchanged line and the group covers 32 banks.
// Step r of a lane still reads tile row 4q + r: from LDS row 4q + (r ^ (q & 1)) = 4q + r +- (q & 1) -- two base addresses, no
// arithmetic in the loop.
struct BwdOperands { const float *row, *t_e, *t_o; };   // row form; transposed form of steps 0, 2 / of steps 1, 3
__device__ __forceinline__ BwdOperands bwd_operands(const float* base, int mm, int q) {
  BwdOperands o;
  o.row = base + (mm ^ ((mm >> 2) & 1)) * 16 + ((q ^ chunk_xor(mm)) << 2);
  const float* optr = base + (4 * q) * 16 + (((mm >> 2) ^ chunk_xor(4 * q)) << 2) + (mm & 3);
  o.t_e = optr + (q & 1) * 16;   // LDS row 4q + r + (q & 1)
  o.t_o = optr - (q & 1) * 16;   // LDS row 4q + r - (q & 1)
  return o;
}
// LDS slot of row sigma <- source row sigma ^ ((sigma >> 2) & 1) (the same chunk XOR: it depends on sigma >> 2 only)
__device__ __forceinline__ unsigned dma_lane_off_swapped(int lane) { return dma_lane_off(lane ^ (((lane >> 4) & 1) << 2)); }

// Forward finalize of one (query row, head): O[l][k] / l_run into the (now idle) operand stage at `sm` as [row][k][HSTR heads] (slot
// hslot of the workgroup's HSTR heads); row statistics (m, l, -, -) for the backward from the q = 0 lanes.
template <int HSTR, int KT>
__device__ __forceinline__ void attn_fwd_finalize(const AttnMfmaArgs& a, float* sm, int row, int q, int hslot, int b, int l, int h,
                                                  const v4f (&oacc)[KT], float mrun, float lrun) {
  const float inv = 1.0f / lrun;
  float* vs = sm + (row * (16 * KT) + 4 * q) * HSTR + hslot;
#pragma unroll
  for (int kt = 0; kt < KT; ++kt)
#pragma unroll
    for (int r = 0; r < 4; ++r) vs[(16 * kt + r) * HSTR] = oacc[kt][r] * inv;
  if (l < a.N && q == 0)
    *reinterpret_cast<float4*>(a.rowstats + (((size_t)b * a.N + l) * AH + h) * 4) = make_float4(mrun, lrun, 0.f, 0.f);
}

// ---- egt_attn_bf16.hip: the MM = 1 instances of egt_attn_kernels.h (egt_attn_desc.reserved & EGT_ATTN_MM_BF16) behind their two
// entry points, launched from plan_attn's geometry; var: the Feat instance of the direction
void egt_attn_bf16_launch_fwd(int var, const EgtLaunch& pack, const EgtLaunch& fwd, const AttnMfmaArgs& a, hipStream_t st);
void egt_attn_bf16_launch_bwd(int var, const EgtLaunch& pack, const EgtLaunch& kv, const EgtLaunch& q, const AttnMfmaArgs& a, hipStream_t st);
