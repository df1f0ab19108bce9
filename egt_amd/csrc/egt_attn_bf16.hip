// Inner op on MFMA tiles, opt-in bf16 products (egt_attn_desc.reserved & EGT_ATTN_MM_BF16): the kernels of egt_attn_mfma.hip with
// QK^T, A.V and their backward products on v_mfma_f32_16x16x32_bf16 / v_mfma_f32_16x16x16_bf16, fp32 accumulate.
//
// The arithmetic contract (include/egt_amd.h): exactly s.Q, K, V, dV_att, the gated probabilities P that enter A.V and P^T.dV_att,
// and the logit gradient dS are rounded to bfloat16 (round to nearest even), each once; every accumulator, the whole elementwise
// skeleton (scale, clip, +E, masks, exp, softmax max / sum, sigmoid, delta, dA, H_hat, dE, dG) is fp32 on unrounded values.
//
// Structure: workgroup roles, LDS layouts, staging, barriers and launch geometry are those of the fp32 kernels (one plan: plan_attn);
// what differs is the operand form.
//   * k_attn_bf16_pack rounds when it writes the operand arrays.  The arrays keep their fp32 containers in this first cut (every
//     element is a bf16 value held in a float): tile addresses, LDS-DMA pieces and swizzles are the fp32 kernels', which are tested.
//   * The fp32 kernels' contraction order kappa(T, u, q) = 16 T + 4 q + u gives a lane (row, q) the four consecutive channels
//     16 T + 4 q .. + 3 of its row in one 16-byte fragment: exactly the K = 16 bf16 operand (lane l: A[l & 15][4 (l >> 4) + j]).  Four
//     fp32 MFMAs (u = 0..3) become ONE bf16 MFMA on the fragment packed with v_cvt_pk_bf16_f32 (exact: the values are bf16 already).
//   * Contractions over d (S = Q.K^T, dP = dO.V^T) pair two channel blocks into one K = 32 MFMA for d >= 32 (both operands take
//     the same (2 T', 2 T' + 1) pairing: the contraction order is free); d = 16 is one K = 16 MFMA -- no zero padding.
//   * Contractions over the 16 keys / query rows of a tile (A.V, dV, dK) are K = 16: the S^T accumulators (lane (l, q): keys
//     4 q + r), converted pairwise, are the B fragment of the next MFMA with no lane movement.  dQ pairs the two key tiles of a
//     trip into one K = 32 MFMA.
//   * dS is rounded once in k_attn_bf16_bwd_kv: the packed value feeds dK, and the same packed value IS the dA hand-off that
//     k_attn_bf16_bwd_q reads: the dA tiles are bf16 in the workspace ([ltile][mtile][16 keys][16 queries], 512 bytes a tile: half
//     the fp32 mode's hand-off, which is most of its workspace and a fifth of the backward's HBM bytes).
#include "egt_attn_dev.h"

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

// c += sum over the d channels of a lane's fragments: a[T], b[T] = channels 16 T + 4 q .. + 3 of the lane's row
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

// ------------------------------------------------------------------- pack --------
// k_attn_pack of egt_attn_mfma.hip with the rounding: the head planes in LDS hold the fp32 values (Q scaled in fp32; delta is the
// fp32 sum over the UNROUNDED dO), every element of an operand array is rounded as it is written.
__device__ __forceinline__ float4 round4(float4 v) { return make_float4(bf16_round(v.x), bf16_round(v.y), bf16_round(v.z), bf16_round(v.w)); }

template <int D>
__global__ void __launch_bounds__(512) k_attn_bf16_pack(AttnMfmaArgs a) {
  constexpr int DH = D * AH, RS = D == 16 ? 16 : 80, RP = 16 * RS + 4, NPC = 16 * DH / 4 / 512;   // pieces per thread and section
  static_assert((16 * DH / 4) % 512 == 0, "whole pieces per thread");
  extern __shared__ __attribute__((aligned(16))) float sm[];   // [8 heads][RP]
  const int N = a.N, NP = a.NP, tid = threadIdx.x;
  const int tiles = NP / 16;
  const int b = blockIdx.x / tiles, n0 = (blockIdx.x % tiles) * 16;
  int secs[4], nsec = 0;   // sections of this launch, in order q, k, v, dO
  if (a.pack_what & PACK_Q) secs[nsec++] = 0;
  if (a.pack_what & (PACK_KH | PACK_KT)) secs[nsec++] = 1;
  if (a.pack_what & (PACK_VT | PACK_VH)) secs[nsec++] = 2;
  if (a.pack_what & PACK_O) secs[nsec++] = 3;
  const size_t arr = (size_t)a.B * AH * NP * D;
  auto load = [&](int sec, float4 (&v)[NPC]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NPC; ++i) {
      const int p = tid + 512 * i, r = p / (DH / 4), c = (p % (DH / 4)) * 4, n = n0 + r;
      v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (n < N)
        v[i] = sec < 3 ? *reinterpret_cast<const float4*>(a.qkv + ((size_t)b * N + n) * 3 * DH + sec * DH + c)
                       : *reinterpret_cast<const float4*>(a.d_v_att + ((size_t)b * N + n) * DH + c);
    }
  };
  auto scatter = [&](const float4 (&v)[NPC], float mul) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NPC; ++i) {
      const int p = tid + 512 * i, r = p / (DH / 4), c4 = p % (DH / 4), k = c4 >> 1, h0 = 4 * (c4 & 1);
      float* o = sm + h0 * RP + r * RS + k;
      o[0] = v[i].x * mul; o[RP] = v[i].y * mul; o[2 * RP] = v[i].z * mul; o[3 * RP] = v[i].w * mul;
    }
  };
  auto put_rows = [&](int which) __attribute__((always_inline)) {   // planes -> [b,h,n/16,k/16,16 nodes,16 channels]
    float* dst = a.pk + (size_t)which * arr;
    for (int i = tid; i < AH * 16 * (D / 4); i += 512) {
      const int j = i & 3, r = (i >> 2) & 15, T = (i >> 6) % (D / 16), h = i / (4 * D);
      *reinterpret_cast<float4*>(dst + ((size_t)b * AH + h) * NP * D + (size_t)n0 * D + T * 256 + r * 16 + j * 4) =
          round4(*reinterpret_cast<const float4*>(sm + h * RP + r * RS + 16 * T + 4 * j));
    }
  };
  auto put_cols = [&](int which) __attribute__((always_inline)) {   // planes -> transposed, tile-major [b,h,n/16,k,16]
    float* dst = a.pk + (size_t)which * arr;
    for (int i = tid; i < AH * D * 4; i += 512) {
      const int r4 = i & 3, k = (i >> 2) % D, h = i / (4 * D);
      const float* src = sm + h * RP + (r4 * 4) * RS + k;
      *reinterpret_cast<float4*>(dst + ((size_t)b * AH + h) * D * NP + (size_t)n0 * D + k * 16 + r4 * 4) =
          round4(make_float4(src[0], src[RS], src[2 * RS], src[3 * RS]));
    }
  };
  float4 cur[NPC], nxt[NPC];
  load(secs[0], cur);
  for (int si = 0; si < nsec; ++si) {
    const int sec = secs[si];
    if (si + 1 < nsec) load(secs[si + 1], nxt);
    if (si > 0) __syncthreads();          // the previous section's readers are done with the planes
    scatter(cur, sec == 0 ? a.scale : 1.0f);   // Q is scaled in fp32 and rounded after: bf16(fl32(s Q))
    __syncthreads();
    if (sec == 0) put_rows(PK_QH);
    else if (sec == 1) {
      if (a.pack_what & PACK_KH) put_rows(PK_KH);
      if (a.pack_what & PACK_KT) put_cols(PK_KT);
    } else if (sec == 2) {
      if (a.pack_what & PACK_VT) put_cols(PK_VT);
      if (a.pack_what & PACK_VH) put_rows(PK_VH);
    } else {
      put_rows(PK_OH);
      // per-row constants of the backward, head-major [b,h,n,4] = (m, 1/l, delta, 0); delta from the unrounded dO and O
      const int r = (tid >> 5) & 15, hh = (tid >> 2) & 7, part = tid & 3, n = n0 + r;   // 4 lanes per (row, head)
      float sdel = 0.f;
      if (n < N) {
        const float* vo = a.v_att_in + ((size_t)b * N + n) * DH + hh;
        const float* dr = sm + hh * RP + r * RS;
#pragma unroll 4
        for (int k = part * (D / 4); k < (part + 1) * (D / 4); ++k) sdel = fmaf(dr[k], vo[k * AH], sdel);
      }
      sdel += __shfl_xor(sdel, 1, 64);
      sdel += __shfl_xor(sdel, 2, 64);
      if (part == 0) {
        float4 s2 = make_float4(3.0e38f, 0.f, 0.f, 0.f);   // rows past N: exp2(-inf) * 0
        if (n < N) {
          float* rs = a.rowstats + (((size_t)b * N + n) * AH + hh) * 4;
          rs[3] = sdel;
          s2 = make_float4(rs[0], __builtin_amdgcn_rcpf(rs[1]), sdel, 0.f);
        }
        *reinterpret_cast<float4*>(a.stats2 + (((size_t)b * AH + hh) * NP + n) * 4) = s2;
      }
    }
#pragma unroll
    for (int i = 0; i < NPC; ++i) cur[i] = nxt[i];
  }
}

// ================================================================== forward =====
// k_attn_mfma_fwd with bf16 operands: the loader waves are the fp32 kernel's; a compute wave packs its K / V^T fragments and its
// gated probabilities pairwise and issues (d / 32 or 1) + d / 16 MFMAs per query tile and key tile where the fp32 kernel issues d / 2.
template <int D, int V>
__global__ void __launch_bounds__(512, 2) k_attn_bf16_fwd(AttnMfmaArgs a) {
  constexpr int KT = D / 16, DH = D * AH, NIN = V ? 2 : 3, TS = FQ * 4 * PT_PL;   // TS: one tensor, one stage of planes
  static_assert(KT * 1024 * 2 * 4 <= OPS_STAGE, "operand stage");
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool loader = wv >= 4;
  const int w = wv & 3;
  const int N = a.N, NP = a.NP;
  const int lgroups = (NP / 16 + FQ - 1) / FQ;
  const int KA = (NP + 16 + 3) & ~3;
  float* kaddL = sm + OPS_BYTES / 4;   // [NP + 16] additive key term of the logits
  float* kaddG = kaddL + KA;           // ... of the gate's exponent
  float* In = kaddG + KA;              // [2 stages][E | G | M][TS]
  float* Hout = In + 2 * NIN * TS;     // [2][TS]
  const int wg = egt_xcd_remap(blockIdx.x, gridDim.x);
  const int hg = wg & 1, grp = wg >> 1;
  const int b = grp / lgroups, l0 = (grp % lgroups) * 16 * FQ;
  const int h = 4 * hg + w;
  const Feat<V> f(a);
  const int mtiles = NP / 16;
  const size_t arr = (size_t)a.B * AH * NP * D;

  if (loader) {
    // ------------------------------------------------------------------ loader waves ----
    const int lt = tid - 256;                   // 0..255
    const int crow = lt >> 4, ccol = lt & 15;   // pair-tile transfers: row crow, key ccol of every 16 x 16 sub-tile, 4 heads (16 bytes)
    for (int m = lt; m < NP + 16; m += 256) key_terms(b, m, N, f.km, a.km, kaddL[m], kaddG[m]);
    const float* Kh = a.pk + PK_KH * arr + ((size_t)b * AH + h) * NP * D;   // [NP/16][D/16][16][16]
    const float* VT = a.pk + PK_VT * arr + ((size_t)b * AH + h) * D * NP;   // [NP/16][D][16]
    const unsigned doff = dma_lane_off(lane);
    const unsigned ops0 = lds_addr(sm) + w * (KT * 2048);   // head w: K tile, then V^T tile
    auto dma_ops = [&](int mt, int stage) __attribute__((always_inline)) {
      const float* ks = Kh + (size_t)mt * 16 * D;
      const float* vs = VT + (size_t)mt * 16 * D;
      const unsigned dst = ops0 + stage * OPS_STAGE;
#pragma unroll
      for (int T = 0; T < KT; ++T) dma_piece(dst + T * 1024, ks + T * 256, doff);
#pragma unroll
      for (int T = 0; T < KT; ++T) dma_piece(dst + KT * 1024 + T * 1024, vs + T * 256, doff);
    };
    const size_t gbase = ((size_t)b * N + l0) * N * AH;
    uint32_t rowoff[FQ];
#pragma unroll
    for (int qt = 0; qt < FQ; ++qt) rowoff[qt] = (uint32_t)(min(l0 + 16 * qt + crow, N - 1) - l0) * N * AH + 4 * hg;
    auto pload = [&](const float* src, int qt, int mcol) __attribute__((always_inline)) {
      return *reinterpret_cast<const float4*>(src + gbase + rowoff[qt] + (uint32_t)min(mcol + ccol, N - 1) * AH);
    };
    const int sc_off = pt_off(crow, ccol);
    auto scatter = [&](float* tl, int qt, float4 v) __attribute__((always_inline)) {
      float* p = tl + qt * 4 * PT_PL + sc_off;
      p[0] = v.x; p[PT_PL] = v.y; p[2 * PT_PL] = v.z; p[3 * PT_PL] = v.w;
    };
    auto hstore = [&](int itp) __attribute__((always_inline)) {   // H_hat tiles of iteration itp: planes -> 16-byte pieces of the [N,N,8] rows
      const float* Hp = Hout + (itp & 1) * TS;
      const int mp = 16 * itp;
#pragma unroll
      for (int qt = 0; qt < FQ; ++qt)
        if (l0 + 16 * qt + crow < N && mp + ccol < N) {
          const float* p = Hp + qt * 4 * PT_PL + sc_off;
          *reinterpret_cast<float4*>(a.h_hat + gbase + rowoff[qt] + (uint32_t)(mp + ccol) * AH) = make_float4(p[0], p[PT_PL], p[2 * PT_PL], p[3 * PT_PL]);
        }
    };
    dma_ops(0, 0);
    float4 pe[FQ], pg[FQ], pm[FQ];
    {
      float4 fe[FQ], fg[FQ], fm[FQ];
      const int m1 = min(16, NP - 16);
#pragma unroll
      for (int qt = 0; qt < FQ; ++qt) {   // both tiles' requests before the first use: one HBM round trip, not two
        if (f.E) fe[qt] = pload(a.E, qt, 0);
        if (f.G) fg[qt] = pload(a.G, qt, 0);
        if (f.M) fm[qt] = pload(a.M, qt, 0);
      }
#pragma unroll
      for (int qt = 0; qt < FQ; ++qt) {
        pe[qt] = pg[qt] = pm[qt] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (f.E) pe[qt] = pload(a.E, qt, m1);
        if (f.G) pg[qt] = pload(a.G, qt, m1);
        if (f.M) pm[qt] = pload(a.M, qt, m1);
      }
#pragma unroll
      for (int qt = 0; qt < FQ; ++qt) {
        if (f.E) scatter(In + 0 * TS, qt, fe[qt]);
        if (f.G) scatter(In + 1 * TS, qt, fg[qt]);
        if (f.M) scatter(In + 2 * TS, qt, fm[qt]);
      }
    }
    if (V) vm_wait<FQ * NIN>(); else vm_wait<0>();   // the DMA pieces are older than the register loads just issued
    lds_barrier();
    for (int it = 0; it < mtiles; ++it) {
      {   // pair tiles of iteration it+1 (requested one iteration ago) into the other stage: its last readers passed the previous barrier
        float* nx = In + ((it + 1) & 1) * NIN * TS;
#pragma unroll
        for (int qt = 0; qt < FQ; ++qt) {
          if (f.E) scatter(nx + 0 * TS, qt, pe[qt]);
          if (f.G) scatter(nx + 1 * TS, qt, pg[qt]);
          if (f.M) scatter(nx + 2 * TS, qt, pm[qt]);
        }
      }
      if (it > 0) hstore(it - 1);
      dma_ops(min(it + 1, mtiles - 1), (it + 1) & 1);
      {
        const int m2 = min(16 * (it + 2), NP - 16);
#pragma unroll
        for (int qt = 0; qt < FQ; ++qt) {
          if (f.E) pe[qt] = pload(a.E, qt, m2);
          if (f.G) pg[qt] = pload(a.G, qt, m2);
          if (f.M) pm[qt] = pload(a.M, qt, m2);
        }
      }
      // exactly the register loads above are younger than the DMA pieces (the generic instance drains)
      if (V) vm_wait<FQ * NIN>(); else vm_wait<0>();
      lds_barrier();
    }
    hstore(mtiles - 1);
  } else {
  // -------------------------------------------------------------------- compute waves ----
  const int ll = lane & 15, q = lane >> 4;
  const bool gated = f.G, clip = f.clip;
  // Q fragments (B operand of S^T = K.Q^T): bf16(d^-1/2 Q)[l][16T + 4q .. + 3]
  v4s Qb[FQ][KT];
  {
    const float* Qh = a.pk + PK_QH * arr + ((size_t)b * AH + h) * NP * D;
#pragma unroll
    for (int qt = 0; qt < FQ; ++qt) {
      const int ltile = min((l0 >> 4) + qt, mtiles - 1);
#pragma unroll
      for (int T = 0; T < KT; ++T) Qb[qt][T] = bf4(*reinterpret_cast<const float4*>(Qh + (size_t)ltile * 16 * D + 256 * T + ll * 16 + 4 * q));
    }
  }
  v4f oacc[FQ][KT];
  float mrun[FQ], lrun[FQ];
#pragma unroll
  for (int qt = 0; qt < FQ; ++qt) {
    mrun[qt] = KEY_OFF; lrun[qt] = 0.f;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) oacc[qt][kt] = (v4f){0.f, 0.f, 0.f, 0.f};
  }
  const int po4 = w * PT_PL + pt_off(ll, 4 * q);   // this lane's keys 4q..4q+3 of row ll inside a sub-tile: one 16-byte access
  const float* opl = sm + w * (KT * 512) + ll * 16 + ((q ^ chunk_xor(ll)) << 2);
  lds_barrier();
  for (int it = 0; it < mtiles; ++it) {
    const int m0 = 16 * it;
    const float* ops = opl + (it & 1) * (OPS_STAGE / 4);
    const float* Inb = In + (it & 1) * NIN * TS;
    float* Hb2 = Hout + (it & 1) * TS;
    float4 kc[KT], vc[KT];   // one K / V^T fragment set for both query tiles
#pragma unroll
    for (int T = 0; T < KT; ++T) kc[T] = *reinterpret_cast<const float4*>(ops + T * 256);
    float4 e4[FQ], g4[FQ], m4[FQ], ka4, kg4 = make_float4(0.f, 0.f, 0.f, 0.f);
    ka4 = *reinterpret_cast<const float4*>(kaddL + m0 + 4 * q);
    if (V == 1) kg4 = *reinterpret_cast<const float4*>(kaddG + m0 + 4 * q);
#pragma unroll
    for (int qt = 0; qt < FQ; ++qt) {
      e4[qt] = g4[qt] = make_float4(0.f, 0.f, 0.f, 0.f);
      m4[qt] = make_float4(1.f, 1.f, 1.f, 1.f);
      if (f.E) e4[qt] = *reinterpret_cast<const float4*>(Inb + 0 * TS + qt * 4 * PT_PL + po4);
      if (f.G) g4[qt] = *reinterpret_cast<const float4*>(Inb + 1 * TS + qt * 4 * PT_PL + po4);
      if (f.M) m4[qt] = *reinterpret_cast<const float4*>(Inb + 2 * TS + qt * 4 * PT_PL + po4);
    }
    __builtin_amdgcn_sched_barrier(0);   // every LDS request of the S phase is in flight before its first MFMA
    // ---- S^T[m][l] = sum_k K[m][k] (d^-1/2 Q)[l][k]: every K fragment feeds the two query tiles ----
    v4s kb4[KT];
#pragma unroll
    for (int T = 0; T < KT; ++T) kb4[T] = bf4(kc[T]);
    v4f s[FQ];
#pragma unroll
    for (int qt = 0; qt < FQ; ++qt) s[qt] = dot_d<KT>(kb4, Qb[qt], (v4f){0.f, 0.f, 0.f, 0.f});
#pragma unroll
    for (int T = 0; T < KT; ++T) vc[T] = *reinterpret_cast<const float4*>(ops + KT * 256 + T * 256);   // V^T fragments: requested behind the S MFMAs
    __builtin_amdgcn_sched_barrier(0);
    float pa[FQ][4];
#pragma unroll
    for (int qt = 0; qt < FQ; ++qt) {
      float hv4[4];
      attn_fwd_unit<V, KT>(a, f, clip, gated, s[qt], e4[qt], g4[qt], m4[qt], ka4, kg4, b, min(l0 + 16 * qt + ll, N - 1), m0 + 4 * q, N - 1, h,
                           mrun[qt], lrun[qt], oacc[qt], pa[qt], hv4);
      *reinterpret_cast<float4*>(Hb2 + qt * 4 * PT_PL + po4) = make_float4(hv4[0], hv4[1], hv4[2], hv4[3]);   // H_hat: post-clip, pre-mask
    }
    __builtin_amdgcn_sched_barrier(0);
    // ---- O^T[k][l] += sum_m V^T[k][m] bf16(P^T)[m][l]: the lane's four keys 4q + r are one K = 16 B fragment ----
    v4s pb[FQ];
#pragma unroll
    for (int qt = 0; qt < FQ; ++qt) pb[qt] = bf4(pa[qt]);
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      const v4s vb = bf4(vc[kt]);
#pragma unroll
      for (int qt = 0; qt < FQ; ++qt) oacc[qt][kt] = MFMA16(vb, pb[qt], oacc[qt][kt]);
    }
    lds_barrier();
  }
  // ---- finalize: O[l][k] / l_run into the (now idle) operand stages as [row][k][4 heads]; row statistics for the backward ----
#pragma unroll
  for (int qt = 0; qt < FQ; ++qt) attn_fwd_finalize<4, KT>(a, sm, 16 * qt + ll, q, w, b, l0 + 16 * qt + ll, h, oacc[qt], mrun[qt], lrun[qt]);
  }
  // V_att[l][k*8 + h]: all eight waves store 16-byte pieces (the group's 4 heads of one channel)
  lds_barrier();
  for (int p = tid; p < 16 * FQ * D; p += 512) {
    const int row = p / D, k = p % D;
    if (l0 + row < N)
      *reinterpret_cast<float4*>(a.v_att + ((size_t)b * N + l0 + row) * DH + k * AH + 4 * hg) = *reinterpret_cast<const float4*>(sm + (size_t)p * 4);
  }
}

// ================================================================= backward =====
// k_attn_mfma_bwd_kv with bf16 operands.  Compute lane (mm = lane&15, q): keys m0 + 16 kb + mm; in every query tile rows l0 + 4q + r.
template <int D, int V>
__global__ void __launch_bounds__(512, 2) k_attn_bf16_bwd_kv(AttnMfmaArgs a) {
  constexpr int KT = D / 16, DH = D * AH, NIN = 3, TS = BK * 4 * PT_PL;   // planes E | G | X (an attention-mask tensor is folded into E and G by the loaders)
  static_assert(KT * 1024 * 2 * 4 <= OPS_STAGE, "operand stage");
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool loader = wv >= 4;
  const int w = wv & 3;
  const int N = a.N, NP = a.NP;
  const int mtiles = NP / 16, mgroups = (mtiles + BK - 1) / BK;
  float* statL = sm + OPS_BYTES / 4;   // [2 stages][4 heads][16 rows][4]
  float* In = statL + 2 * 4 * 64;      // [2][E | G | X][TS], key-major planes
  float* Out = In + 2 * NIN * TS;      // [2][dE | dG][TS]
  const int wg = egt_xcd_remap(blockIdx.x, gridDim.x);
  const int hg = wg & 1, grp = wg >> 1;
  const int b = grp / mgroups, m0 = (grp % mgroups) * 16 * BK;
  const int h = 4 * hg + w;
  const Feat<V> f(a);
  const size_t arr = (size_t)a.B * AH * NP * D;
  const size_t hb = ((size_t)b * AH + h) * NP * D;
  const size_t gb = (size_t)b * N * N * AH;

  if (loader) {
    // ------------------------------------------------------------------ loader waves ----
    const int lt = tid - 256;
    const int crow = lt >> 4, ccol = lt & 15;   // query row, key of each 16 x 16 sub-tile; the group's 4 heads (16 bytes)
    const float* Qh = a.pk + PK_QH * arr + hb;  // this loader wave feeds head h
    const float* Oh = a.pk + PK_OH * arr + hb;
    const unsigned doff = dma_lane_off_swapped(lane);   // (operand-tile rows pair-swapped in LDS: bwd_operands)
    const unsigned ops0 = lds_addr(sm) + w * (KT * 2048);   // head w: Q tile, then dO tile
    auto dma_ops = [&](int ltile, int stage) __attribute__((always_inline)) {
      const float* qs = Qh + (size_t)ltile * 16 * D;
      const float* os = Oh + (size_t)ltile * 16 * D;
      const unsigned dst = ops0 + stage * OPS_STAGE;
#pragma unroll
      for (int T = 0; T < KT; ++T) dma_piece(dst + T * 1024, qs + T * 256, doff);
#pragma unroll
      for (int T = 0; T < KT; ++T) dma_piece(dst + KT * 1024 + T * 1024, os + T * 256, doff);
    };
    const float* st2 = a.stats2 + ((size_t)b * AH + h) * NP * 4;
    uint32_t coff[BK];
#pragma unroll
    for (int kb = 0; kb < BK; ++kb) coff[kb] = (uint32_t)min(m0 + 16 * kb + ccol, N - 1) * AH + 4 * hg;   // + row * N * 8
    auto cload = [&](const float* src, int l0, int kb) __attribute__((always_inline)) {
      return *reinterpret_cast<const float4*>(src + gb + (size_t)min(l0 + crow, N - 1) * N * AH + coff[kb]);
    };
    struct Pair { float4 e, g, x; };
    // tensors past their valid range read a valid address; only dH_ext must be ZERO there (it is added to dH).  An
    // attention-mask tensor enters the backward only through the additive term of logit and gate: folded into E and G here.
    auto pair_load = [&](int l0, int kb) __attribute__((always_inline)) {
      Pair p;
      p.e = p.g = p.x = make_float4(0.f, 0.f, 0.f, 0.f);
      if (f.E) p.e = cload(a.E, l0, kb);
      if (f.G) p.g = cload(a.G, l0, kb);
      if (f.X) {
        p.x = cload(a.d_h_ext, l0, kb);
        if (!(l0 + crow < N && m0 + 16 * kb + ccol < N)) p.x = make_float4(0.f, 0.f, 0.f, 0.f);
      }
      if (f.M) {
        const float4 mk = cload(a.M, l0, kb);
        p.e.x += (mk.x - 1.0f) * EGT_NEG; p.e.y += (mk.y - 1.0f) * EGT_NEG; p.e.z += (mk.z - 1.0f) * EGT_NEG; p.e.w += (mk.w - 1.0f) * EGT_NEG;
        p.g.x += (mk.x - 1.0f) * EGT_NEG; p.g.y += (mk.y - 1.0f) * EGT_NEG; p.g.z += (mk.z - 1.0f) * EGT_NEG; p.g.w += (mk.w - 1.0f) * EGT_NEG;
      }
      return p;
    };
    const int sc_off = ptT_off(crow, ccol);
    auto scatter = [&](float* tl, int kb, float4 v) __attribute__((always_inline)) {
      float* p = tl + kb * 4 * PT_PL + sc_off;
      p[0] = v.x; p[PT_PL] = v.y; p[2 * PT_PL] = v.z; p[3 * PT_PL] = v.w;
    };
    auto pair_put = [&](float* st, int kb, const Pair& p) __attribute__((always_inline)) {
      scatter(st + 0 * TS, kb, p.e);
      if (f.G) scatter(st + 1 * TS, kb, p.g);
      scatter(st + 2 * TS, kb, p.x);
    };
    auto gstore = [&](int itp) __attribute__((always_inline)) {   // dE / dG tiles of iteration itp: planes -> 16-byte pieces of the [N,N,8] rows
      const int lp = 16 * itp;
      const float* o = Out + (itp & 1) * 2 * TS;
#pragma unroll
      for (int kb = 0; kb < BK; ++kb)
        if (lp + crow < N && m0 + 16 * kb + ccol < N) {
          const float* p = o + kb * 4 * PT_PL + sc_off;
          const size_t go = gb + (size_t)(lp + crow) * N * AH + coff[kb];
          if (f.E) *reinterpret_cast<float4*>(a.d_E + go) = make_float4(p[0], p[PT_PL], p[2 * PT_PL], p[3 * PT_PL]);
          if (f.G) *reinterpret_cast<float4*>(a.d_G + go) = make_float4(p[TS], p[TS + PT_PL], p[TS + 2 * PT_PL], p[TS + 3 * PT_PL]);
        }
    };
    auto stat_load = [&](int ltile) __attribute__((always_inline)) {   // (every lane loads: the count of register loads per trip stays fixed)
      return *reinterpret_cast<const float4*>(st2 + (size_t)(ltile * 16 + (lane & 15)) * 4);
    };
    auto stat_put = [&](float4 v, int stage) __attribute__((always_inline)) {
      if (lane < 16) *reinterpret_cast<float4*>(statL + ((stage * 4 + w) * 16 + lane) * 4) = v;
    };
    dma_ops(0, 0);
    Pair pr[BK];
    {
      Pair p0[BK];
#pragma unroll
      for (int kb = 0; kb < BK; ++kb) p0[kb] = pair_load(0, kb);   // both tiles' requests before the first use: one HBM round trip
#pragma unroll
      for (int kb = 0; kb < BK; ++kb) pr[kb] = pair_load(min(16, NP - 16), kb);
      stat_put(stat_load(0), 0);
#pragma unroll
      for (int kb = 0; kb < BK; ++kb) pair_put(In, kb, p0[kb]);
    }
    float4 stn = stat_load(min(1, mtiles - 1));
    vm_wait<0>();
    lds_barrier();
    for (int it = 0; it < mtiles; ++it) {
      {   // pair tiles of query tile it+1 (requested one iteration ago) into the other stage
        float* nx = In + ((it + 1) & 1) * NIN * TS;
#pragma unroll
        for (int kb = 0; kb < BK; ++kb) pair_put(nx, kb, pr[kb]);
      }
      stat_put(stn, (it + 1) & 1);
      if (it > 0) gstore(it - 1);
      dma_ops(min(it + 1, mtiles - 1), (it + 1) & 1);
      {
        const int l2 = min(16 * (it + 2), NP - 16);
#pragma unroll
        for (int kb = 0; kb < BK; ++kb) pr[kb] = pair_load(l2, kb);
        stn = stat_load(l2 >> 4);
      }
      if (V) vm_wait<BK * 3 + 1>(); else vm_wait<0>();   // exactly the BK * 3 + 1 register loads above are younger than the DMA pieces
      lds_barrier();
    }
    gstore(mtiles - 1);
  } else {
  // -------------------------------------------------------------------- compute waves ----
  const int mm = lane & 15, q = lane >> 4;
  const bool gated = f.G, clip = f.clip;
  const uint32_t ooff = mm * 16 + 4 * q;
  // K / V fragments of this lane's keys (B operands of S = Q.K^T and dP = dO.V^T), packed once; key rows past N are zero in the
  // pack, a key tile past NP re-reads the last one and is switched off by its additive term
  v4s Kb[BK][KT], Vb[BK][KT];
  float kadd[BK], kaddg[BK];
  bool tile_ok[BK];
  unsigned short* dAb[BK];   // bf16 dA tiles: the fp32 kernel's element indices, two bytes an element
  {
    const float* Kh = a.pk + PK_KH * arr + hb;
    const float* Vh = a.pk + PK_VH * arr + hb;
#pragma unroll
    for (int kb = 0; kb < BK; ++kb) {
      const int mt = (m0 >> 4) + kb, mtc = min(mt, mtiles - 1);
      tile_ok[kb] = mt < mtiles;
      dAb[kb] = reinterpret_cast<unsigned short*>(a.ws_dA) + (((size_t)b * AH + h) * mtiles * mtiles + (size_t)mtc) * 256;   // + ltile * mtiles * 256
#pragma unroll
      for (int T = 0; T < KT; ++T) {
        Kb[kb][T] = bf4(*reinterpret_cast<const float4*>(Kh + (size_t)mtc * 16 * D + 256 * T + ooff));
        Vb[kb][T] = bf4(*reinterpret_cast<const float4*>(Vh + (size_t)mtc * 16 * D + 256 * T + ooff));
      }
      key_terms(b, m0 + 16 * kb + mm, N, f.km, a.km, kadd[kb], kaddg[kb]);
    }
  }
  v4f dKacc[BK][KT], dVacc[BK][KT];
#pragma unroll
  for (int kb = 0; kb < BK; ++kb)
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) { dKacc[kb][kt] = (v4f){0.f, 0.f, 0.f, 0.f}; dVacc[kb][kt] = (v4f){0.f, 0.f, 0.f, 0.f}; }
  const int po4 = w * PT_PL + ptT_off(4 * q, mm);   // this lane's query rows 4q..4q+3 of key mm inside a sub-tile: one 16-byte access
  const BwdOperands op = bwd_operands(sm + w * (KT * 512), mm, q);   // operand tiles of head w (Q, then dO)
  lds_barrier();
  for (int l0 = 0, it = 0; it < mtiles; l0 += 16, ++it) {
    const float* opr = op.row + (it & 1) * (OPS_STAGE / 4);
    const float* opt_e = op.t_e + (it & 1) * (OPS_STAGE / 4);
    const float* opt_o = op.t_o + (it & 1) * (OPS_STAGE / 4);
    const float* Inb = In + (it & 1) * NIN * TS;
    float* Ob = Out + (it & 1) * 2 * TS;
    float4 qa[KT], oa[KT];   // row operands first: the S / dP MFMAs start as soon as they land
#pragma unroll
    for (int T = 0; T < KT; ++T) {
      qa[T] = *reinterpret_cast<const float4*>(opr + T * 256);
      oa[T] = *reinterpret_cast<const float4*>(opr + KT * 256 + T * 256);
    }
    float4 e4[BK], g4[BK], x4[BK], stc[4];
#pragma unroll
    for (int kb = 0; kb < BK; ++kb) {
      e4[kb] = *reinterpret_cast<const float4*>(Inb + 0 * TS + kb * 4 * PT_PL + po4);
      g4[kb] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (f.G) g4[kb] = *reinterpret_cast<const float4*>(Inb + 1 * TS + kb * 4 * PT_PL + po4);
      x4[kb] = *reinterpret_cast<const float4*>(Inb + 2 * TS + kb * 4 * PT_PL + po4);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) stc[r] = *reinterpret_cast<const float4*>(statL + (((it & 1) * 4 + w) * 16 + 4 * q + r) * 4);
    __builtin_amdgcn_sched_barrier(0);   // every LDS request of the first two phases is in flight before the first MFMA
    // ---- S[l][m] = sum_k (d^-1/2 Q)[l][k] K[m][k] ; dP[l][m] = sum_k dO[l][k] V[m][k]: every Q / dO fragment feeds two key tiles ----
    v4s qb[KT], ob[KT];
#pragma unroll
    for (int T = 0; T < KT; ++T) { qb[T] = bf4(qa[T]); ob[T] = bf4(oa[T]); }
    v4f s[BK], dp[BK];
#pragma unroll
    for (int kb = 0; kb < BK; ++kb) {
      s[kb] = dot_d<KT>(qb, Kb[kb], (v4f){0.f, 0.f, 0.f, 0.f});
      dp[kb] = dot_d<KT>(ob, Vb[kb], (v4f){0.f, 0.f, 0.f, 0.f});
    }
    __builtin_amdgcn_sched_barrier(0);
    v4s atb[BK], dab[BK];   // bf16(P), bf16(dS): the B fragments of dV and dK
#pragma unroll
    for (int kb = 0; kb < BK; ++kb) {
      float at[4], da[4], dE4[4], dG4[4], hv4[4];   // (hv4: dropped, H_hat left in the forward)
      attn_bwd_unit<V>(a, f, clip, gated, s[kb], dp[kb], e4[kb], g4[kb], x4[kb], stc, kadd[kb], kaddg[kb], b, l0 + 4 * q,
                       min(m0 + 16 * kb + mm, N - 1), N - 1, h, at, da, dE4, dG4, hv4);   // (the mask tensor arrives inside E / G)
      if (f.E) *reinterpret_cast<float4*>(Ob + kb * 4 * PT_PL + po4) = make_float4(dE4[0], dE4[1], dE4[2], dE4[3]);
      if (f.G) *reinterpret_cast<float4*>(Ob + TS + kb * 4 * PT_PL + po4) = make_float4(dG4[0], dG4[1], dG4[2], dG4[3]);
      atb[kb] = bf4(at);
      dab[kb] = bf4(da);
      // dA tile [key][query] of (head, query tile, key tile): the lane's own four rows as packed for dK, one 8-byte store
      if (tile_ok[kb]) {
        union { v4s s; uint2 u; } pk;
        pk.s = dab[kb];
        *reinterpret_cast<uint2*>(dAb[kb] + (size_t)it * mtiles * 256 + ooff) = pk.u;
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    // ---- dV^T[k][m] += sum_l dO[l][k] P[l][m] ; dK^T[k][m] += sum_l (d^-1/2 Q)[l][k] dS[l][m]: transposed operands from the same
    // tiles, the lane's four query rows 4q + r are one K = 16 fragment ----
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      float qq[4], oo[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float* opt = (r & 1) ? opt_o : opt_e;
        qq[r] = opt[kt * 256 + r * 16];
        oo[r] = opt[KT * 256 + kt * 256 + r * 16];
      }
      const v4s qT = bf4(qq), oT = bf4(oo);
#pragma unroll
      for (int kb = 0; kb < BK; ++kb) {
        dVacc[kb][kt] = MFMA16(oT, atb[kb], dVacc[kb][kt]);
        dKacc[kb][kt] = MFMA16(qT, dab[kb], dKacc[kb][kt]);
      }
    }
    lds_barrier();
  }
  // dK / dV into the (now idle) operand stages as [key][k][4 heads], dK in stage 0, dV in stage 1
#pragma unroll
  for (int kb = 0; kb < BK; ++kb) {
    float* ks = sm + ((16 * kb + mm) * D + 4 * q) * 4 + w;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        ks[(16 * kt + r) * 4] = dKacc[kb][kt][r];
        ks[OPS_STAGE / 4 + (16 * kt + r) * 4] = dVacc[kb][kt][r];
      }
  }
  }
  // dK / dV rows of d_qkv: all eight waves store 16-byte pieces (the group's 4 heads of one channel)
  lds_barrier();
  for (int p = tid; p < 16 * BK * D; p += 512) {
    const int row = p / D, k = p % D;
    if (m0 + row < N) {
      float* o = a.d_qkv + ((size_t)b * N + m0 + row) * 3 * DH + k * AH + 4 * hg;
      *reinterpret_cast<float4*>(o + DH) = *reinterpret_cast<const float4*>(sm + (size_t)p * 4);
      *reinterpret_cast<float4*>(o + 2 * DH) = *reinterpret_cast<const float4*>(sm + OPS_STAGE / 4 + (size_t)p * 4);
    }
  }
}

// dQ: k_attn_mfma_bwd_q with bf16 operands: the two key tiles of a trip are one K = 32 contraction (an odd tile count ends with
// one K = 16 MFMA on the first tile alone).  The dA tiles are bf16: the two key tiles of a (query tile, trip) are adjacent in the
// workspace and arrive as ONE 1 KB piece (half the fp32 kernel's dA pieces and LDS); a lane reads its four keys 4q + u of query ll
// with four 16-bit LDS reads into two packed registers.
template <int D>
__global__ void __launch_bounds__(512, 2) k_attn_bf16_bwd_q(AttnMfmaArgs a) {
  constexpr int KT = D / 16, DH = D * AH, NPIECE = 2 * KT + QW_TILES, STG = NPIECE * 256;   // 1 KB pieces / floats per stage
  constexpr int PPW = (NPIECE + 3) / 4;                                                      // DMA pieces per loader wave and stage (upper bound)

  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int N = a.N, NP = a.NP;
  const int mtiles = NP / 16, qgroups = (mtiles + QW_TILES - 1) / QW_TILES;
  const int wg = egt_xcd_remap(blockIdx.x, gridDim.x);
  const int b = wg / (AH * qgroups), h = (wg / qgroups) % AH, lt0 = (wg % qgroups) * QW_TILES;
  const size_t arr = (size_t)a.B * AH * NP * D;
  const float* KTp = a.pk + PK_KT * arr + ((size_t)b * AH + h) * D * NP;           // [mtile][D][16 keys]
  const float* dAh = a.ws_dA + ((size_t)b * AH + h) * mtiles * mtiles * 128;       // [ltile][mtile][16 keys][16 queries] bf16: 128 floats a tile
  const int nit = (mtiles + 1) / 2;
  if (wv >= 4) {
    // ---- loaders: piece p of a stage: p < 2 KT: K^T block (kb = p / KT, T = p % KT); else the two dA tiles (key tiles 2 it, 2 it + 1) of
    // query tile ltile = p - 2 KT
    const int j = wv - 4;
    const unsigned doff = dma_lane_off(lane), lin = lane * 16, lin_first = (lane & 31) * 16;
    const float* base[PPW];
    int stride[PPW];
    unsigned voff[PPW];
    bool second[PPW];   // K^T block of the second key tile of a trip (absent in the last trip of an odd tile count)
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
      const int p = j + 4 * i;
      if (p < 2 * KT) {
        base[i] = KTp + (size_t)(p / KT) * 16 * D + (p % KT) * 256; stride[i] = 32 * D; voff[i] = doff; second[i] = p / KT != 0;
      } else {
        const int ltile = min(lt0 + (p - 2 * KT), mtiles - 1);
        base[i] = dAh + (size_t)ltile * mtiles * 128; stride[i] = 256; voff[i] = lin; second[i] = false;
      }
    }
    auto stage_in = [&](int it, int stage) __attribute__((always_inline)) {
      const unsigned dst = lds_addr(sm) + stage * (STG * 4);
      // the second key tile of the last trip of an odd tile count does not exist: the K^T block re-reads the first tile's and the
      // upper half of a dA piece re-reads the first tile (nothing past tile (ltile, mtiles - 1) is touched); those fragments are not used
      const bool odd_last = 2 * it + 1 >= mtiles;
#pragma unroll
      for (int i = 0; i < PPW; ++i) {
        const int p = j + 4 * i;
        if (p < NPIECE) {
          const float* src = base[i] + (size_t)it * stride[i];
          if (odd_last && second[i]) src -= 16 * D;
          dma_piece(dst + p * 1024, src, (p >= 2 * KT && odd_last) ? lin_first : voff[i]);
        }
      }
    };
    const bool full = j + 4 * (PPW - 1) < NPIECE;   // this wave issues PPW (else PPW - 1) pieces per stage
    auto wait_ring = [&]() __attribute__((always_inline)) {
      if (full) vm_wait<(QW_STAGES - 2) * PPW>(); else vm_wait<(QW_STAGES - 2) * (PPW - 1)>();
    };
#pragma unroll
    for (int t = 0; t < QW_STAGES - 1; ++t) if (t < nit) stage_in(t, t);
    if (nit >= QW_STAGES - 1) wait_ring(); else vm_wait<0>();
    lds_barrier();
    for (int it = 0; it < nit; ++it) {
      const int tn = it + QW_STAGES - 1;
      if (tn < nit) { stage_in(tn, tn % QW_STAGES); wait_ring(); }
      else vm_wait<0>();   // the ring drains: nothing is in flight when the stages are reused by the epilogue
      lds_barrier();
    }
  } else {
    const int ll = lane & 15, q = lane >> 4;
    v4f dQ[2][KT];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj)
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) dQ[jj][kt] = (v4f){0.f, 0.f, 0.f, 0.f};
    const float* kfrag = sm + ll * 16 + ((q ^ chunk_xor(ll)) << 2);                 // + stage, + (kb KT + kt) * 256
    // dA[key 4q + u][query ll] of (query tile 2 wv + jj, key tile kb), in bf16 elements: + stage * 2 STG, + jj * 512 + kb * 256 + u * 16
    const unsigned short* dfrag = reinterpret_cast<const unsigned short*>(sm + 2 * KT * 256) + (2 * wv) * 512 + (4 * q) * 16 + ll;
    struct Frag { float4 kc[2][KT]; unsigned da[2][2][2]; };
    auto fetch = [&](int stage, Frag& fr) __attribute__((always_inline)) {
      const float* kf = kfrag + stage * STG;
      const unsigned short* df = dfrag + stage * (2 * STG);
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) fr.kc[kb][kt] = *reinterpret_cast<const float4*>(kf + (kb * KT + kt) * 256);
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            const unsigned short* e = df + jj * 512 + kb * 256 + 2 * u * 16;
            fr.da[kb][jj][u] = (unsigned)e[0] | ((unsigned)e[16] << 16);
          }
    };
    // dQ^T[k][l] += sum_m K^T[k][m] dS[l][m] over the keys 4q + u of both tiles (K^T holds bf16 values: its packing is exact)
    auto mma = [&](int it, const Frag& fr) __attribute__((always_inline)) {
      v4s db[2][2];
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
          union { unsigned u[2]; v4s s; } pk;
          pk.u[0] = fr.da[kb][jj][0]; pk.u[1] = fr.da[kb][jj][1];
          db[kb][jj] = pk.s;
        }
      if (2 * it + 1 < mtiles) {
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
          const v8s kk = cat8(bf4(fr.kc[0][kt]), bf4(fr.kc[1][kt]));
#pragma unroll
          for (int jj = 0; jj < 2; ++jj) dQ[jj][kt] = MFMA32(kk, cat8(db[0][jj], db[1][jj]), dQ[jj][kt]);
        }
      } else {
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
          const v4s kk = bf4(fr.kc[0][kt]);
#pragma unroll
          for (int jj = 0; jj < 2; ++jj) dQ[jj][kt] = MFMA16(kk, db[0][jj], dQ[jj][kt]);
        }
      }
    };
    // The MFMAs lag one trip behind the LDS requests; two named register sets swap roles.
    Frag fa, fb;
    lds_barrier();
    fetch(0, fa);
    int it = 0;
    for (; it + 1 < nit; it += 2) {
      lds_barrier(); fetch((it + 1) % QW_STAGES, fb); mma(it, fa);
      lds_barrier(); fetch((it + 2) % QW_STAGES, fa); mma(it + 1, fb);
    }
    if (it < nit) { lds_barrier(); mma(it, fa); }
    // d^-1/2 dQ into the (now idle) stages as [query row 128][channel]
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      float* o = sm + ((2 * wv + jj) * 16 + ll) * D + 4 * q;
#pragma unroll
      for (int kt = 0; kt < KT; ++kt)
        *reinterpret_cast<float4*>(o + 16 * kt) = make_float4(dQ[jj][kt][0] * a.scale, dQ[jj][kt][1] * a.scale, dQ[jj][kt][2] * a.scale, dQ[jj][kt][3] * a.scale);
    }
  }
  // dQ rows of d_qkv (channel k*8 + h): consecutive lanes consecutive channels of one row
  lds_barrier();
  for (int p = tid; p < 16 * QW_TILES * D; p += 512) {
    const int row = p / D, k = p % D, l = lt0 * 16 + row;
    if (l < N) a.d_qkv[((size_t)b * N + l) * 3 * DH + k * AH + h] = sm[p];
  }
}

// ------------------------------------------------------------------ host glue --
// Launched from plan_attn's geometry (egt_attn_mfma.hip): the fp32 kernels' grids, blocks and LDS sizes, k_attn_bf16_bwd_q's smaller stages apart.
template <int D>
static void launch_fwd(int var, const EgtLaunch& pack, const EgtLaunch& fwd, const AttnMfmaArgs& a, hipStream_t st) {
  egt_launch_planned<k_attn_bf16_pack<D>>("k_attn_bf16_pack", pack, st, a);
  switch (var) {
    case 1: egt_launch_planned<k_attn_bf16_fwd<D, 1>>("k_attn_bf16_fwd", fwd, st, a); break;
    case 2: egt_launch_planned<k_attn_bf16_fwd<D, 2>>("k_attn_bf16_fwd", fwd, st, a); break;
    default: egt_launch_planned<k_attn_bf16_fwd<D, 0>>("k_attn_bf16_fwd", fwd, st, a); break;
  }
}
template <int D>
static void launch_bwd(int var, const EgtLaunch& pack, const EgtLaunch& kv, const EgtLaunch& q, const AttnMfmaArgs& a, hipStream_t st) {
  egt_launch_planned<k_attn_bf16_pack<D>>("k_attn_bf16_pack", pack, st, a);   // (also the per-row constants)
  switch (var) {
    case 1: egt_launch_planned<k_attn_bf16_bwd_kv<D, 1>>("k_attn_bf16_bwd_kv", kv, st, a); break;
    case 2: egt_launch_planned<k_attn_bf16_bwd_kv<D, 2>>("k_attn_bf16_bwd_kv", kv, st, a); break;
    default: egt_launch_planned<k_attn_bf16_bwd_kv<D, 0>>("k_attn_bf16_bwd_kv", kv, st, a); break;
  }
  egt_launch_planned<k_attn_bf16_bwd_q<D>>("k_attn_bf16_bwd_q", q, st, a);
}

void egt_attn_bf16_launch_fwd(int var, const EgtLaunch& pack, const EgtLaunch& fwd, const AttnMfmaArgs& a, hipStream_t st) {
  switch (a.d) {
    case 16: launch_fwd<16>(var, pack, fwd, a, st); break;
    case 32: launch_fwd<32>(var, pack, fwd, a, st); break;
    default: launch_fwd<64>(var, pack, fwd, a, st); break;
  }
}
void egt_attn_bf16_launch_bwd(int var, const EgtLaunch& pack, const EgtLaunch& kv, const EgtLaunch& q, const AttnMfmaArgs& a, hipStream_t st) {
  switch (a.d) {
    case 16: launch_bwd<16>(var, pack, kv, q, a, st); break;
    case 32: launch_bwd<32>(var, pack, kv, q, a, st); break;
    default: launch_bwd<64>(var, pack, kv, q, a, st); break;
  }
}
