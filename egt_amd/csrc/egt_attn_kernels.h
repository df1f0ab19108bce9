// The four kernels of the MFMA inner op (structure and measurements: egt_attn_mfma.hip's header), ONE body each for
// both operand forms, and their launchers.  MM = 0: every contraction exact fp32 on v_mfma_f32_16x16x4_f32 (egt_attn_mfma.hip
// instantiates it, the pair operator shares its pack and dQ kernels); MM = 1: bf16 products, fp32 accumulate (egt_attn_bf16.hip).
//
// Workgroup roles, LDS layouts, staging, waits, barriers and launch geometry do not depend on the form.  The form decides the type of
// the fragments a compute wave keeps (AttnForm), their conversion when they are read, the contractions and the dA hand-off from
// k_attn_mfma_bwd_kv to k_attn_mfma_bwd_q, each under `if constexpr (MM)` where it is used.  The fp32 contractions are the functions of
// egt_attn_dev.h that the pair kernels share; the bf16 ones are a few lines on that header's primitives (bf4, dot_d, MFMA16 / 32)
// and stay in the bodies: moved behind a by-reference function boundary like the fp32 ones, the same arithmetic compiles to other
// instruction streams in every MM = 1 instance of fwd and bwd_kv, and both forms' streams are kept as they were measured.  The MM = 1
// contract (include/egt_amd.h): exactly s.Q, K, V, dV_att, the gated
// probabilities P that enter A.V and P^T.dV_att, and the logit gradient dS are rounded to bfloat16 (round to nearest even), each
// once; every accumulator and the whole elementwise skeleton (scale, clip, +E, masks, exp, softmax max / sum, sigmoid, delta, dA,
// H_hat, dE, dG) is fp32 on unrounded values.
//   * The pack rounds when it writes the operand arrays, which keep their fp32 containers (every element is a bf16 value held in a
//     float): tile addresses, LDS-DMA pieces and swizzles are one set; packing a fragment with v_cvt_pk_bf16_f32 is exact.
//   * dS is rounded once in k_attn_mfma_bwd_kv: the packed value feeds dK, and the same packed value IS the dA hand-off: the dA tiles
//     are bf16 in the workspace ([ltile][mtile][16 keys][16 queries], 512 bytes a tile: half the fp32 form's hand-off, which is most
//     of its workspace and a fifth of the backward's HBM bytes).
#pragma once
#include <type_traits>

#include "egt_attn_dev.h"

// ------------------------------------------------------------------- pack --------
// workgroup = (graph, 16 node rows), 512 threads: every section of the launch ([q | k | v | dO]) is de-interleaved
// through LDS and leaves head-major.  Channel index of the source: c = s*d*H + k*H + h (egt_layers.py:70-76).
// A thread loads 16 bytes = 4 heads of one channel k of one row and scatters them into head planes [h][row][k]
// (row stride D + 16, plane stride = 16 rows + 4: the 4 x ds_write_b32 and the 16-byte row reads are bank-conflict
// free); the next section's loads are in flight while the current one is written out (one launch = one wave of
// workgroups and, per section, one overlapped HBM round trip: the one-section-per-workgroup kernel took 18 us).
// MM = 1 rounds every element of an operand array as it is written: the head planes in LDS hold the fp32 values (Q scaled in fp32 and
// rounded after: bf16(fl32(s Q)); delta is the fp32 sum over the UNROUNDED dO).
__device__ __forceinline__ float4 round4(float4 v) { return make_float4(bf16_round(v.x), bf16_round(v.y), bf16_round(v.z), bf16_round(v.w)); }

template <int D, int MM = 0>
__global__ void __launch_bounds__(512) k_attn_pack(AttnMfmaArgs a) {
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
  // planes -> [b,h,n/16,k/16,16 nodes,16 channels] array `which`: a wave's operand fetch (16 nodes x 16 channels of
  // one k-tile) is ONE contiguous 1 KB block; lanes walk the 16-byte chunks of a block in order
  auto put_rows = [&](int which) __attribute__((always_inline)) {
    float* dst = a.pk + (size_t)which * arr;
    for (int i = tid; i < AH * 16 * (D / 4); i += 512) {
      const int j = i & 3, r = (i >> 2) & 15, T = (i >> 6) % (D / 16), h = i / (4 * D);
      float4 v = *reinterpret_cast<const float4*>(sm + h * RP + r * RS + 16 * T + 4 * j);
      if constexpr (MM) v = round4(v);
      *reinterpret_cast<float4*>(dst + ((size_t)b * AH + h) * NP * D + (size_t)n0 * D + T * 256 + r * 16 + j * 4) = v;
    }
  };
  // planes -> transposed, tile-major [b,h,n/16,k,16] array: the 16 nodes of a tile are contiguous per channel and a
  // tile is one 64*D-byte block
  auto put_cols = [&](int which) __attribute__((always_inline)) {
    float* dst = a.pk + (size_t)which * arr;
    for (int i = tid; i < AH * D * 4; i += 512) {
      const int r4 = i & 3, k = (i >> 2) % D, h = i / (4 * D);
      const float* src = sm + h * RP + (r4 * 4) * RS + k;
      float4 v = make_float4(src[0], src[RS], src[2 * RS], src[3 * RS]);
      if constexpr (MM) v = round4(v);
      *reinterpret_cast<float4*>(dst + ((size_t)b * AH + h) * D * NP + (size_t)n0 * D + k * 16 + r4 * 4) = v;
    }
  };
  float4 cur[NPC], nxt[NPC];
  load(secs[0], cur);
  for (int si = 0; si < nsec; ++si) {
    const int sec = secs[si];
    if (si + 1 < nsec) load(secs[si + 1], nxt);
    if (si > 0) __syncthreads();          // the previous section's readers are done with the planes
    scatter(cur, sec == 0 ? a.scale : 1.0f);   // Q leaves pre-scaled: S = (d^-1/2 Q).K^T, dK = dA^T.(d^-1/2 Q)
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
      // per-row constants of the backward, head-major [b,h,n,4] = (m, 1/l, delta, 0) with
      // delta[row,h] = sum_k dO[row,k,h] * O[row,k,h] (flash-style); rows past N get 1/l = 0 (their probabilities vanish)
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
// workgroup = (graph b, 32 query rows, 4 heads); compute wave w = head 4 hg + w.  Lane (ll = lane&15, q = lane>>4)
// owns query rows l0 + 16 qt + ll (two query tiles: every K / V^T operand register feeds two MFMAs) and, in the key
// tile of an iteration, keys m0 + 4q + r.  S^T = K.Q^T puts the key index on the MFMA row axis: the softmax
// reductions over keys are in-lane ops + two permlane swaps, the online-softmax rescale is lane-uniform, and the
// gated probabilities feed the A.V MFMA as its B operand in place.
// MM = 1: a compute wave issues (d / 32 or 1) + d / 16 MFMAs per query tile and key tile where the fp32 form issues d / 2.
template <int D, int V, int MM>
__global__ void __launch_bounds__(512, 2) k_attn_mfma_fwd(AttnMfmaArgs a) {
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
  const int wg = egt_xcd_remap(blockIdx.x, gridDim.x);   // the two head groups of a row block and a graph's K / V^T share an XCD's L2
  const int hg = wg & 1, grp = wg >> 1;
  const int b = grp / lgroups, l0 = (grp % lgroups) * 16 * FQ;
  const int h = 4 * hg + w;
  const Feat<V> f(a);
  const int mtiles = NP / 16;
  const size_t arr = (size_t)a.B * AH * NP * D;
  EGT_STAMP_DECL;

  if (loader) {
    // ------------------------------------------------------------------ loader waves ----
    const int lt = tid - 256;                   // 0..255
    const int crow = lt >> 4, ccol = lt & 15;   // pair-tile transfers: row crow, key ccol of every 16 x 16 sub-tile, 4 heads (16 bytes)
    for (int m = lt; m < NP + 16; m += 256) key_terms(b, m, N, f.km, a.km, kaddL[m], kaddG[m]);
    const float* Kh = a.pk + PK_KH * arr + ((size_t)b * AH + h) * NP * D;   // [NP/16][D/16][16][16]   (this loader wave feeds head h)
    const float* VT = a.pk + PK_VT * arr + ((size_t)b * AH + h) * D * NP;   // [NP/16][D][16]
    const unsigned doff = dma_lane_off(lane);
    const unsigned ops0 = lds_addr(sm) + w * (KT * 2048);   // head w: K tile, then V^T tile
    auto dma_ops = [&](int mt, int stage) __attribute__((always_inline)) {
      const float* ks = Kh + (size_t)mt * 16 * D;
      const float* vs = VT + (size_t)mt * 16 * D;
      const unsigned dst = ops0 + stage * OPS_STAGE;
#pragma unroll
      for (int T = 0; T < KT; ++T) if (ABL(1)) dma_piece(dst + T * 1024, ks + T * 256, doff);
#pragma unroll
      for (int T = 0; T < KT; ++T) if (ABL(1)) dma_piece(dst + KT * 1024 + T * 1024, vs + T * 256, doff);
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
    auto hstore = [&](int itp) __attribute__((always_inline)) {   // H_hat tiles of iteration itp: planes -> whole 16-byte pieces of the [N,N,8] rows
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
        for (int qt = 0; qt < FQ; ++qt) if (ABL(2)) {
          if (f.E) scatter(nx + 0 * TS, qt, pe[qt]);
          if (f.G) scatter(nx + 1 * TS, qt, pg[qt]);
          if (f.M) scatter(nx + 2 * TS, qt, pm[qt]);
        }
      }
      if (it > 0 && ABL(4)) hstore(it - 1);
      dma_ops(min(it + 1, mtiles - 1), (it + 1) & 1);
      if (ABL(2)) {
        const int m2 = min(16 * (it + 2), NP - 16);
#pragma unroll
        for (int qt = 0; qt < FQ; ++qt) {
          if (f.E) pe[qt] = pload(a.E, qt, m2);
          if (f.G) pg[qt] = pload(a.G, qt, m2);
          if (f.M) pm[qt] = pload(a.M, qt, m2);
        }
      }
      // exactly the register loads above are younger than the DMA pieces (their count is a template constant for the
      // straight-line instances; the generic instance drains)
      if (V && EGT_ATTN_ABL == 0) vm_wait<FQ * NIN>(); else vm_wait<0>();
      lds_barrier();
    }
    hstore(mtiles - 1);
  } else {
  // -------------------------------------------------------------------- compute waves ----
  const int ll = lane & 15, q = lane >> 4;
  const bool gated = f.G, clip = f.clip;
  // Q fragments (B operand of S^T = K.Q^T), pre-scaled: d^-1/2 Q[l][16T + 4q + u]; MM = 1: one packed fragment per channel block
  std::conditional_t<MM == 0, float[FQ][4 * KT], v4s[FQ][KT]> Qr;
  {
    const float* Qh = a.pk + PK_QH * arr + ((size_t)b * AH + h) * NP * D;
#pragma unroll
    for (int qt = 0; qt < FQ; ++qt) {
      const int ltile = min((l0 >> 4) + qt, mtiles - 1);
#pragma unroll
      for (int T = 0; T < KT; ++T) {
        const float4* src = reinterpret_cast<const float4*>(Qh + (size_t)ltile * 16 * D + 256 * T + ll * 16 + 4 * q);
        if constexpr (MM) {
          Qr[qt][T] = AttnForm<MM>::cvt(*src);
        } else {
          const float4 v = *src;
          Qr[qt][4 * T + 0] = v.x; Qr[qt][4 * T + 1] = v.y; Qr[qt][4 * T + 2] = v.z; Qr[qt][4 * T + 3] = v.w;
        }
      }
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
  // operand fragment address: row ll, chunk q of the k-tile blocks of head w's tiles (+ stage, + 1024 T, + KT*1024 for V^T)
  const float* opl = sm + w * (KT * 512) + ll * 16 + ((q ^ chunk_xor(ll)) << 2);
  lds_barrier();
  EGT_STAMP(0);
  for (int it = 0; it < mtiles; ++it) {
    const int m0 = 16 * it;
    const float* ops = opl + (it & 1) * (OPS_STAGE / 4);
    const float* Inb = In + (it & 1) * NIN * TS;
    float* Hb2 = Hout + (it & 1) * TS;
    float4 kc[1][KT], vc[1][KT];   // one K / V^T fragment set for both query tiles
#pragma unroll
    for (int T = 0; T < KT; ++T) kc[0][T] = *reinterpret_cast<const float4*>(ops + T * 256);
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
    EGT_STAMP(1);
    // ---- S^T[m][l] = sum_k K[m][k] (d^-1/2 Q)[l][k]: every K register feeds the two query tiles ----
    v4f s[FQ];
    if constexpr (MM) {   // (d / 32 or 1) MFMAs a query tile
      v4s kb[KT];
#pragma unroll
      for (int T = 0; T < KT; ++T) kb[T] = bf4(kc[0][T]);
#pragma unroll
      for (int qt = 0; qt < FQ; ++qt) s[qt] = dot_d<KT>(kb, Qr[qt], (v4f){0.f, 0.f, 0.f, 0.f});
    } else {
      mfma_s<FQ, 1, KT>(kc, Qr, s);
    }
#pragma unroll
    for (int T = 0; T < KT; ++T) vc[0][T] = *reinterpret_cast<const float4*>(ops + KT * 256 + T * 256);   // V^T fragments: requested behind the S MFMAs, landed long before P.V
    __builtin_amdgcn_sched_barrier(0);
    EGT_STAMP(2);
    float pa[FQ][4];
#pragma unroll
    for (int qt = 0; qt < FQ; ++qt) {
      float hv4[4];
      attn_fwd_unit<V, KT>(a, f, clip, gated, s[qt], e4[qt], g4[qt], m4[qt], ka4, kg4, b, min(l0 + 16 * qt + ll, N - 1), m0 + 4 * q, N - 1, h,
                           mrun[qt], lrun[qt], oacc[qt], pa[qt], hv4);
      *reinterpret_cast<float4*>(Hb2 + qt * 4 * PT_PL + po4) = make_float4(hv4[0], hv4[1], hv4[2], hv4[3]);   // H_hat: post-clip, pre-mask
    }
    __builtin_amdgcn_sched_barrier(0);
    EGT_STAMP(3);
    // ---- O^T[k][l] += sum_m V^T[k][m] P^T[m][l]  (contraction order m = 4q + t): every V^T register feeds two MFMAs ----
    if constexpr (MM) {   // the lane's four keys 4q + r are one K = 16 B fragment: the S^T accumulators' layout, rounded pairwise
      v4s pb[FQ];
#pragma unroll
      for (int qt = 0; qt < FQ; ++qt) pb[qt] = bf4(pa[qt]);
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) {
        const v4s vb = bf4(vc[0][kt]);
#pragma unroll
        for (int qt = 0; qt < FQ; ++qt) oacc[qt][kt] = MFMA16(vb, pb[qt], oacc[qt][kt]);
      }
    } else {
      mfma_pv<FQ, 1, KT>(vc, pa, oacc);
    }
    EGT_STAMP(4);
    lds_barrier();
    EGT_STAMP(6);
  }
  // ---- finalize: O[l][k] / l_run into the (now idle) operand stages as [row][k][4 heads]; row statistics for the backward ----
#pragma unroll
  for (int qt = 0; qt < FQ; ++qt) attn_fwd_finalize<4, KT>(a, sm, 16 * qt + ll, q, w, b, l0 + 16 * qt + ll, h, oacc[qt], mrun[qt], lrun[qt]);
  EGT_STAMP(7);
  EGT_STAMP_OUT(ST_ATTN_FWD);
  }
  // V_att[l][k*8 + h]: all eight waves store 16-byte pieces (the group's 4 heads of one channel), consecutive threads
  // consecutive channels (a dword store per lane and channel costs ~300 cycles each: 19 k cycles per workgroup before)
  lds_barrier();
  for (int p = tid; p < 16 * FQ * D; p += 512) {
    const int row = p / D, k = p % D;
    if (l0 + row < N)
      *reinterpret_cast<float4*>(a.v_att + ((size_t)b * N + l0 + row) * DH + k * AH + 4 * hg) = *reinterpret_cast<const float4*>(sm + (size_t)p * 4);
  }
}

// ================================================================= backward =====
// Launches (flash-attention style, the [N,N,H] probabilities are recomputed):
//   k_attn_pack        : head-major operand arrays of Q (pre-scaled), K, V, dV_att; the per-row constants
//                        (m, 1/l, delta = sum_k dO*O) head-major
//   k_attn_mfma_bwd_kv : workgroup = (graph, 32 keys, 4 heads): compute wave = head, K / V fragments and the dK / dV
//                        accumulators of TWO key tiles in registers while the workgroup walks the query tiles; the loader
//                        waves stage the Q / dO tiles of a query tile by LDS-DMA (the compute waves read BOTH operand forms
//                        from that one tile), the pair tiles (E, G, dH_ext) into key-major planes, and store dE / dG;
//                        per tile S = Q.K^T and dP = dO.V^T on MFMA, softmax / gate / clip backward on the VALU, then
//                        dV^T += dO^T.A and dK^T += Q^T.dA on MFMA with the probabilities as B operands in place;
//                        dA = dH*c leaves in the lane's own layout (one 16-byte store per key tile)
//   k_attn_mfma_bwd_q  : wave = (graph, head, 32 query rows), walks the key tiles: dQ^T += K^T.dA^T straight from the
//                        dA tiles and the packed K^T
// Compute lane (mm = lane&15, q): keys m0 + 16 kb + mm; in every query tile rows l0 + 4q + r.
template <int D, int V, int MM>
__global__ void __launch_bounds__(512, 2) k_attn_mfma_bwd_kv(AttnMfmaArgs a) {
  typedef AttnForm<MM> F;
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
  EGT_STAMP_DECL;

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
      for (int T = 0; T < KT; ++T) if (ABL(1)) dma_piece(dst + T * 1024, qs + T * 256, doff);
#pragma unroll
      for (int T = 0; T < KT; ++T) if (ABL(1)) dma_piece(dst + KT * 1024 + T * 1024, os + T * 256, doff);
    };
    // per-row constants of the query tile: one float4 per (head, row) -- lanes 0..15 of each loader wave
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
    auto stat_load = [&](int ltile) __attribute__((always_inline)) {   // (every lane loads: lanes >= 16 re-read rows 0..15 -- the count of register loads per trip stays fixed)
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
        for (int kb = 0; kb < BK; ++kb) if (ABL(2)) pair_put(nx, kb, pr[kb]);
      }
      stat_put(stn, (it + 1) & 1);
      if (it > 0 && ABL(4)) gstore(it - 1);
      dma_ops(min(it + 1, mtiles - 1), (it + 1) & 1);
      if (ABL(2)) {
        const int l2 = min(16 * (it + 2), NP - 16);
#pragma unroll
        for (int kb = 0; kb < BK; ++kb) pr[kb] = pair_load(l2, kb);
        stn = stat_load(l2 >> 4);
      }
      if (V && EGT_ATTN_ABL == 0) vm_wait<BK * 3 + 1>(); else vm_wait<0>();   // exactly the BK * 3 + 1 register loads above are younger than the DMA pieces
      lds_barrier();
    }
    gstore(mtiles - 1);
  } else {
  // -------------------------------------------------------------------- compute waves ----
  const int mm = lane & 15, q = lane >> 4;
  const bool gated = f.G, clip = f.clip;
  const uint32_t ooff = mm * 16 + 4 * q;
  // K / V fragments of this lane's keys (B operands of S = Q.K^T and dP = dO.V^T); key rows past N are zero in the pack,
  // a key tile past NP re-reads the last one and is switched off by its additive term
  typename F::Frag Kr[BK][KT], Vr[BK][KT];   // (MM = 1: packed once)
  float kadd[BK], kaddg[BK];
  bool tile_ok[BK];
  typename F::DA* dAb[BK];   // dA tiles: one element index in both forms
  {
    const float* Kh = a.pk + PK_KH * arr + hb;
    const float* Vh = a.pk + PK_VH * arr + hb;
#pragma unroll
    for (int kb = 0; kb < BK; ++kb) {
      const int mt = (m0 >> 4) + kb, mtc = min(mt, mtiles - 1);
      tile_ok[kb] = mt < mtiles;
      dAb[kb] = reinterpret_cast<typename F::DA*>(a.ws_dA) + (((size_t)b * AH + h) * mtiles * mtiles + (size_t)mtc) * 256;   // + ltile * mtiles * 256
#pragma unroll
      for (int T = 0; T < KT; ++T) {
        Kr[kb][T] = F::cvt(*reinterpret_cast<const float4*>(Kh + (size_t)mtc * 16 * D + 256 * T + ooff));
        Vr[kb][T] = F::cvt(*reinterpret_cast<const float4*>(Vh + (size_t)mtc * 16 * D + 256 * T + ooff));
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
  EGT_STAMP(0);
  for (int l0 = 0, it = 0; it < mtiles; l0 += 16, ++it) {
    const float* opr = op.row + (it & 1) * (OPS_STAGE / 4);
    const float* opt_e = op.t_e + (it & 1) * (OPS_STAGE / 4);
    const float* opt_o = op.t_o + (it & 1) * (OPS_STAGE / 4);
    const float* Inb = In + (it & 1) * NIN * TS;
    float* Ob = Out + (it & 1) * 2 * TS;
    float4 qa[KT], oa[KT];   // row operands first: the S / dP MFMAs start as soon as they land, everything else lands behind them
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
    EGT_STAMP(1);
    // ---- S[l][m] = sum_k (d^-1/2 Q)[l][k] K[m][k] ; dP[l][m] = sum_k dO[l][k] V[m][k]: every Q / dO register feeds two MFMAs ----
    v4f s[BK], dp[BK];
    if constexpr (MM) {
      v4s qb[KT], ob[KT];
#pragma unroll
      for (int T = 0; T < KT; ++T) { qb[T] = bf4(qa[T]); ob[T] = bf4(oa[T]); }
#pragma unroll
      for (int kb = 0; kb < BK; ++kb) {
        s[kb] = dot_d<KT>(qb, Kr[kb], (v4f){0.f, 0.f, 0.f, 0.f});
        dp[kb] = dot_d<KT>(ob, Vr[kb], (v4f){0.f, 0.f, 0.f, 0.f});
      }
    } else {
      mfma_s_dp<BK, KT>(qa, oa, Kr, Vr, s, dp);
    }
    __builtin_amdgcn_sched_barrier(0);
    EGT_STAMP(2);
    float at[BK][4], da[BK][4];   // P, dS: the B fragments of dV and dK
    v4s atb[BK], dab[BK];         // ... MM = 1: rounded, each once
#pragma unroll
    for (int kb = 0; kb < BK; ++kb) {
      float dE4[4], dG4[4], hv4[4];   // (hv4: dropped, H_hat left in the forward)
      attn_bwd_unit<V>(a, f, clip, gated, s[kb], dp[kb], e4[kb], g4[kb], x4[kb], stc, kadd[kb], kaddg[kb], b, l0 + 4 * q,
                       min(m0 + 16 * kb + mm, N - 1), N - 1, h, at[kb], da[kb], dE4, dG4, hv4);   // (the mask tensor arrives inside E / G)
      if (f.E) *reinterpret_cast<float4*>(Ob + kb * 4 * PT_PL + po4) = make_float4(dE4[0], dE4[1], dE4[2], dE4[3]);
      if (f.G) *reinterpret_cast<float4*>(Ob + TS + kb * 4 * PT_PL + po4) = make_float4(dG4[0], dG4[1], dG4[2], dG4[3]);
      if constexpr (MM) { atb[kb] = bf4(at[kb]); dab[kb] = bf4(da[kb]); }
      // dA tile [key][query] of (head, query tile, key tile): the lane's own four rows as they enter dK, one 16-byte (MM = 1: 8-byte) store
      if (tile_ok[kb] && ABL(4)) {
        if constexpr (MM) da_store(dAb[kb] + (size_t)it * mtiles * 256 + ooff, dab[kb]);
        else da_store(dAb[kb] + (size_t)it * mtiles * 256 + ooff, da[kb]);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    EGT_STAMP(3);
    // ---- dV^T[k][m] += sum_l dO[l][k] A[l][m] ; dK^T[k][m] += sum_l (d^-1/2 Q)[l][k] dA[l][m]: transposed operands from the same tiles ----
    if constexpr (MM) {   // the lane's four query rows 4q + r are one K = 16 fragment
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
    } else {
      mfma_dv_dk<BK, KT>(opt_e, opt_o, at, da, dVacc, dKacc);
    }
    EGT_STAMP(4);
    lds_barrier();
    EGT_STAMP(6);
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
  EGT_STAMP(7);
  EGT_STAMP_OUT(ST_ATTN_BWD_KV);
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

// dQ: workgroup = (graph, head, 128 query rows): 4 compute waves (32 query rows = two tiles each) + 4 loader waves.  Per
// iteration the loaders stage two key tiles by LDS-DMA: their K^T tiles (shared by the four compute waves) and the sixteen
// dA tiles (query tile x key tile) -- the register-direct version issued 24 global loads per 64 MFMAs, i.e. as many issue
// cycles of loads as of MFMAs.  Compute lane (ll = lane&15, q): query rows 16 j + ll of its tiles; keys 4q + u as the
// contraction index: K^T fragments by ds_read_b128 (chunk-swizzled like every operand tile), dA[key][query] read
// transposed by ds_read_b32.
// MM = 1: the dA tiles are bf16, so the two key tiles of a (query tile, trip) are adjacent in the workspace and arrive as ONE 1 KB
// piece (half the fp32 form's dA pieces and LDS); a lane reads its four keys 4q + u of query ll with four 16-bit LDS reads into two
// packed registers, and the two key tiles of a trip are one K = 32 contraction (an odd tile count ends with one K = 16 MFMA on the
// first tile alone).
template <int D, int MM = 0>
__global__ void __launch_bounds__(512, 2) k_attn_mfma_bwd_q(AttnMfmaArgs a) {
  typedef typename AttnForm<MM>::DA DA;
  constexpr int DAT = 256 * sizeof(DA) / 4, DAP = MM ? 1 : 2;                               // floats per dA tile; dA pieces per query tile and trip
  constexpr int KT = D / 16, DH = D * AH, NPIECE = 2 * KT + DAP * QW_TILES, STG = NPIECE * 256;   // 1 KB pieces / floats per stage
  constexpr int PPW = (NPIECE + 3) / 4;                                                      // DMA pieces per loader wave and stage (upper bound)

  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int N = a.N, NP = a.NP;
  const int mtiles = NP / 16, qgroups = (mtiles + QW_TILES - 1) / QW_TILES;
  const int wg = egt_xcd_remap(blockIdx.x, gridDim.x);
  const int b = wg / (AH * qgroups), h = (wg / qgroups) % AH, lt0 = (wg % qgroups) * QW_TILES;
  const size_t arr = (size_t)a.B * AH * NP * D;
  const float* KTp = a.pk + PK_KT * arr + ((size_t)b * AH + h) * D * NP;           // [mtile][D][16 keys]
  const float* dAh = a.ws_dA + ((size_t)b * AH + h) * mtiles * mtiles * DAT;       // [ltile][mtile][16 keys][16 queries] of DA
  const int nit = (mtiles + 1) / 2;
  if (wv >= 4) {
    // ---- loaders: piece p of a stage: p < 2 KT: K^T block (kb = p / KT, T = p % KT); else dA piece t = p - 2 KT: the tile (ltile = t >> 1,
    // kb = t & 1), MM = 1: both key tiles of ltile = t
    const int j = wv - 4;
    const unsigned doff = dma_lane_off(lane), lin = lane * 16, lin_first = (lane & 31) * 16;
    // piece i of this wave: p = j + 4 i; its source address advances by a constant per trip (two key tiles): K^T blocks by
    // 32 D floats, dA pieces by two tiles -- bases and strides are hoisted (the address arithmetic of a piece was ~45 scalar
    // instructions, six pieces per trip: the loaders were SALU-bound)
    const float* base[PPW];
    int stride[PPW];
    unsigned voff[PPW];
    bool second[PPW];   // piece belongs to the second key tile of a trip (absent in the last trip of an odd tile count)
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
      const int p = j + 4 * i;
      if (p < 2 * KT) {
        base[i] = KTp + (size_t)(p / KT) * 16 * D + (p % KT) * 256; stride[i] = 32 * D; voff[i] = doff; second[i] = p / KT != 0;
      } else {
        const int t = p - 2 * KT, ltile = min(lt0 + t / DAP, mtiles - 1);
        base[i] = dAh + ((size_t)ltile * mtiles + t % DAP) * DAT; stride[i] = 2 * DAT; voff[i] = lin; second[i] = t % DAP != 0;
      }
    }
    auto stage_in = [&](int it, int stage) __attribute__((always_inline)) {
      const unsigned dst = lds_addr(sm) + stage * (STG * 4);
      // the second key tile of the last trip of an odd tile count does not exist: its pieces re-read the first tile's, MM = 1: the upper
      // half of a dA piece re-reads the first tile (nothing past tile (ltile, mtiles - 1) is touched); those fragments are not used
      const bool odd_last = 2 * it + 1 >= mtiles;
#pragma unroll
      for (int i = 0; i < PPW; ++i) {
        const int p = j + 4 * i;
        if (p < NPIECE) {
          const float* src = base[i] + (size_t)it * stride[i];
          if (odd_last && second[i]) src -= (MM || p < 2 * KT) ? 16 * D : DAT;   // (MM = 1: only K^T blocks are second)
          if (p < 2 * KT ? ABL(1) : ABL(32)) dma_piece(dst + p * 1024, src, (MM && p >= 2 * KT && odd_last) ? lin_first : voff[i]);
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
    // dA[key 4q + u][query ll] of (query tile 2 wv + jj, key tile kb), in elements: + stage, + jj * 512 + kb * 256 + u * 16
    const DA* dfrag = reinterpret_cast<const DA*>(sm + 2 * KT * 256) + (2 * wv) * 512 + (4 * q) * 16 + ll;
    struct Frag { float4 kc[2][KT]; std::conditional_t<MM == 0, float[4], unsigned[2]> da[2][2]; };   // (MM = 1: two bf16 a register)
    auto fetch = [&](int stage, Frag& fr) __attribute__((always_inline)) {
      const float* kf = kfrag + stage * STG;
      const DA* df = dfrag + stage * (STG * 256 / DAT);
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) fr.kc[kb][kt] = *reinterpret_cast<const float4*>(kf + (kb * KT + kt) * 256);
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
          const DA* e = df + jj * 512 + kb * 256;
          if constexpr (MM) {
#pragma unroll
            for (int u = 0; u < 2; ++u) fr.da[kb][jj][u] = (unsigned)e[2 * u * 16] | ((unsigned)e[2 * u * 16 + 16] << 16);
          } else {
#pragma unroll
            for (int u = 0; u < 4; ++u) fr.da[kb][jj][u] = e[u * 16];
          }
        }
    };
    // dQ^T[k][l] += sum_m K^T[k][m] dA[l][m]  (a key tile past the end -- odd tile counts -- is skipped); MM = 1: over the keys 4q + u of
    // both tiles at once (K^T holds bf16 values: its packing is exact)
    auto mma = [&](int it, const Frag& fr) __attribute__((always_inline)) {
      if constexpr (MM) {
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
      } else {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
          if (2 * it + kb < mtiles) {
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
              for (int kt = 0; kt < KT; ++kt) {
                const float kk = u == 0 ? fr.kc[kb][kt].x : u == 1 ? fr.kc[kb][kt].y : u == 2 ? fr.kc[kb][kt].z : fr.kc[kb][kt].w;
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) dQ[jj][kt] = MFMA(kk, fr.da[kb][jj][u], dQ[jj][kt]);
              }
          }
      }
    };
    // The MFMAs lag one trip behind the LDS requests: behind barrier it the fragments of stage it+1 are requested, then the
    // MFMAs of trip it run from the registers filled a trip ago -- the LDS latency never faces an idle matrix pipe.  Two
    // named register sets swap roles.
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
    if (l < N && ABL(4)) a.d_qkv[((size_t)b * N + l) * 3 * DH + k * AH + h] = sm[p];
  }
}

// ------------------------------------------------------------------ launchers --
// From plan_attn's geometry (egt_attn_mfma.hip); var: the Feat instance of the direction.  The launch profiler's names are per form.
template <int MM, int D>
static void attn_launch_fwd(int var, const EgtLaunch& pack, const EgtLaunch& fwd, const AttnMfmaArgs& a, hipStream_t st) {
  constexpr const char* name = MM ? "k_attn_bf16_fwd" : "k_attn_mfma_fwd";
  egt_launch_planned<k_attn_pack<D, MM>>(MM ? "k_attn_bf16_pack" : "k_attn_pack", pack, st, a);
  switch (var) {
    case 1: egt_launch_planned<k_attn_mfma_fwd<D, 1, MM>>(name, fwd, st, a); break;
    case 2: egt_launch_planned<k_attn_mfma_fwd<D, 2, MM>>(name, fwd, st, a); break;
    default: egt_launch_planned<k_attn_mfma_fwd<D, 0, MM>>(name, fwd, st, a); break;
  }
}
template <int MM, int D>
static void attn_launch_bwd(int var, const EgtLaunch& pack, const EgtLaunch& kv, const EgtLaunch& q, const AttnMfmaArgs& a, hipStream_t st) {
  constexpr const char* name = MM ? "k_attn_bf16_bwd_kv" : "k_attn_mfma_bwd_kv";
  egt_launch_planned<k_attn_pack<D, MM>>(MM ? "k_attn_bf16_pack" : "k_attn_pack", pack, st, a);   // (also the per-row constants, delta = sum_k dO*O among them)
  switch (var) {
    case 1: egt_launch_planned<k_attn_mfma_bwd_kv<D, 1, MM>>(name, kv, st, a); break;
    case 2: egt_launch_planned<k_attn_mfma_bwd_kv<D, 2, MM>>(name, kv, st, a); break;
    default: egt_launch_planned<k_attn_mfma_bwd_kv<D, 0, MM>>(name, kv, st, a); break;
  }
  egt_launch_planned<k_attn_mfma_bwd_q<D, MM>>(MM ? "k_attn_bf16_bwd_q" : "k_attn_mfma_bwd_q", q, st, a);
}
template <int MM>
static void attn_launch_fwd(int var, const EgtLaunch& pack, const EgtLaunch& fwd, const AttnMfmaArgs& a, hipStream_t st) {
  switch (a.d) {
    case 16: attn_launch_fwd<MM, 16>(var, pack, fwd, a, st); break;
    case 32: attn_launch_fwd<MM, 32>(var, pack, fwd, a, st); break;
    default: attn_launch_fwd<MM, 64>(var, pack, fwd, a, st); break;
  }
}
template <int MM>
static void attn_launch_bwd(int var, const EgtLaunch& pack, const EgtLaunch& kv, const EgtLaunch& q, const AttnMfmaArgs& a, hipStream_t st) {
  switch (a.d) {
    case 16: attn_launch_bwd<MM, 16>(var, pack, kv, q, a, st); break;
    case 32: attn_launch_bwd<MM, 32>(var, pack, kv, q, a, st); break;
    default: attn_launch_bwd<MM, 64>(var, pack, kv, q, a, st); break;
  }
}
