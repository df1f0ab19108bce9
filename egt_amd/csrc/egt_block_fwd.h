// Forward pair kernels of the fused attention block (included by egt_block.hip, which holds the dispatch):
// k_block_fwd<De,KVL,ML,FULL,BF,SD,DO> and the four-rows-per-iteration k_block_fwd_r4<De,FULL,NW,BF,SD,DO> for narrow edge channels
// (SD = true: the degree-scaler instances, instantiated by egt_block_sd.hip; DO = true: the attention-dropout instances, egt_block_do.hip),
// and k_block_fwd_s64, k_block_fwd written for the headline descriptor alone (everything the generic kernel tests per tile is a constant there).
// The phases of the per-pair body (lane-constant operands, logits, online softmax and A.V, dense_edge_r, the row finish) are the
// fwd_* functions below, with kv_frags / frag16 / key_mask_add of egt_block_dev.h; a kernel is its LDS carve-up, its staging and
// prefetch, and its loop around them (profiles/fwd_phases_kres.txt has the register counts of this split against the pasted copies).
// Two phases keep a pasted copy in one kernel each, because the shared function measured slower there than the parent's text (DESIGN 4.1
// has the figures): k_block_fwd_r4 its online softmax x gate, A.V, the mask-tensor instances (ML) of k_block_fwd their row finish.  A change to fwd_softmax_av or
// fwd_row_finish is made in that copy too.
#pragma once
// Cache-policy hints of the streamed tiles (egt_tile.h).  k_block_fwd reads e_l ONCE: non-temporal, so that it does not push e_{l+1} --
// which this launch writes and the next one reads, 134 MB of the 256 MB memory-side cache at the headline batch -- out.  Measured
// (tools/ab.sh, same box): k_block_fwd 60.7 -> 59.0 us; the stores non-temporal instead (nothing retained): 67 us.
#ifndef EGT_NT_FWD_E
#define EGT_NT_FWD_E true
#endif
#ifndef EGT_NT_FWD_ST
#define EGT_NT_FWD_ST false
#endif

// ================================================ tile phases of the forward =====
// Every phase of the per-pair body, once.  Lane = (p, q) = (lane & 15, lane >> 4): key p of the tile, head pair q (heads 2q + j).
// Row state of a (wave, query row): running max `mx` and sum `sum` per head j, O[2k + j] = channel k of head 2q + j of A.V.

// lane-constant MFMA operands: projection weights wA and bias c2r (a.pw), dense_edge_r weights wrA and bias brv
template <int DE>
__device__ __forceinline__ void fwd_lane_weights(const BlockArgs& a, int p, int q, float (&wA)[4 * Geo<DE>::TILES], float (&c2r)[4],
                                                 float (&wrA)[Geo<DE>::TILES][2], float4 (&brv)[Geo<DE>::TILES]) {
  using G = Geo<DE>;
#pragma unroll
  for (int t = 0; t < 4 * G::TILES; ++t) wA[t] = a.pw[(16 * (t >> 2) + 4 * q + (t & 3)) * 16 + p];
#pragma unroll
  for (int r = 0; r < 4; ++r) c2r[r] = a.pw[G::DEP * 16 + 4 * q + r];
#pragma unroll
  for (int t = 0; t < G::TILES; ++t) {
    const int c = 16 * t + p;
    wrA[t][0] = c < DE ? a.Wr[(2 * q + 0) * DE + c] : 0.f;
    wrA[t][1] = c < DE ? a.Wr[(2 * q + 1) * DE + c] : 0.f;
    const int cb = 16 * t + 4 * q;   // scalar loads: parameter tensors need not be 16-byte aligned
    brv[t] = (cb < DE) ? make_float4(a.br[cb], a.br[cb + 1], a.br[cb + 2], a.br[cb + 3])
                       : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

__device__ __forceinline__ void fwd_row_init(float (&mx)[2], float (&sum)[2], float (&O)[16]) {
  mx[0] = mx[1] = -3.0e38f; sum[0] = sum[1] = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) O[i] = 0.f;
}

// scaled QK^T, clip, + E (egt_layers.py:79-86): hh = H_hat of the pair (what dense_edge_r reads), xl = the logits the masks are
// added to, gl = the gate logits.  acc = the projection of the pair: acc[2j] = G, acc[2j + 1] = E of head 2q + j.
__device__ __forceinline__ void fwd_pair_logits(const BlockArgs& a, bool clip, const float (&Qf)[16], const float (&Kf)[16], const v4f& acc,
                                                float (&hh)[2], float (&xl)[2], float (&gl)[2]) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) dot = fmaf(Qf[2 * k + j], Kf[2 * k + j], dot);
    float ah = dot * a.scale;
    if (clip) ah = fminf(fmaxf(ah, a.clip_lo), a.clip_hi);
    hh[j] = ah + acc[2 * j + 1];
    xl[j] = hh[j];
    gl[j] = acc[2 * j];
  }
}

// online softmax x gate, A.V (per lane); a key past N (!valid) leaves max and sum alone and weighs 0
__device__ __forceinline__ void fwd_softmax_av(bool valid, bool gated, const float (&xl)[2], const float (&gl)[2], const float (&Vf)[16],
                                               float (&mx)[2], float (&sum)[2], float (&O)[16]) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const float xv = xl[j];
    const float mn = valid ? fmaxf(mx[j], xv) : mx[j];
    const float alpha = __expf(mx[j] - mn);
    const float pe = valid ? __expf(xv - mn) : 0.f;
    mx[j] = mn;
    sum[j] = fmaf(sum[j], alpha, pe);
    const float av = gated ? pe * egt_sigmoid(gl[j]) : pe;
#pragma unroll
    for (int k = 0; k < 8; ++k) O[2 * k + j] = fmaf(O[2 * k + j], alpha, av * Vf[2 * k + j]);
  }
}

// dense_edge_r + res_edge on the LDS tile: e' = e + H_hat.Wr + br (H_hat of a key past N reads as 0)
template <int DE>
__device__ __forceinline__ void fwd_edge_update(float* tl, int p, int q, bool valid, const float (&hh)[2],
                                                const float (&wrA)[Geo<DE>::TILES][2], const float4 (&brv)[Geo<DE>::TILES]) {
  const float h0 = valid ? hh[0] : 0.f, h1 = valid ? hh[1] : 0.f;
#pragma unroll
  for (int t = 0; t < Geo<DE>::TILES; ++t) {
    v4f d = {brv[t].x, brv[t].y, brv[t].z, brv[t].w};
    d = MFMA(wrA[t][0], h0, d);
    d = MFMA(wrA[t][1], h1, d);
    const float4 ev = frag_read<DE>(tl, p, q, t);
    frag_write<DE>(tl, p, q, t, make_float4(ev.x + d[0], ev.y + d[1], ev.z + d[2], ev.w + d[3]));
  }
}

// end of query row `rowl` ([B * N] row index): merge the 16 key lanes (same q), max first, then the sums; V_att and the row statistics
// (max, sum per head) to HBM.  keep: V_att also into the row's Q slot `qrow` in LDS for the node epilogue (the row's Q is dead).
__device__ __forceinline__ void fwd_row_finish(const BlockArgs& a, size_t rowl, int p, int q, float (&mx)[2], float (&sum)[2], float (&O)[16],
                                               bool keep, float* qrow) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const float mr2 = row_max16(mx[j]);
    const float f = __expf(mx[j] - mr2);
    mx[j] = mr2;
    sum[j] = row_sum16(sum[j] * f);
#pragma unroll
    for (int k = 0; k < 8; ++k) O[2 * k + j] *= f;
  }
  const float o = reduce16_keep_own(O, p);
  // element i = p: k = p>>1, j = p&1 -> head 2q + j
  const int k = p >> 1, j = p & 1;
  const float sj = j ? sum[1] : sum[0];
  const float vo = o / sj;
  if (k < a.DK) a.v_att[rowl * a.Dh + k * BH + 2 * q + j] = vo;
  if (keep) qrow[k * BH + 2 * q + j] = vo;
  if (p < 2) {
    float* st = a.stats + (rowl * BH + 2 * q + p) * 4;
    st[0] = p ? mx[1] : mx[0];
    st[1] = sj;
  }
}

// ---- degree scalers (EGT_BF_SCALE_DEGREE, egt_layers.py:122-136): the SD instances of the two kernels below ----
// deg of (row, head) = the sum of the gates over the keys; V_att leaves the row finish multiplied by s(deg), so dense_mha (node
// epilogue, k_node_post) and the dWo contraction read V_att' from where they read V_att.  Slot 3 of the row statistics keeps deg
// for the backward (bwd_sd_rows).  The unflagged instances call neither function.
__device__ __forceinline__ float egt_degree_scaler(float deg, bool linear) { return linear ? deg : log1pf(deg); }

// fwd_softmax_av of a gated block, with the degree: a key past N adds 0, a masked key's gate IS 0 (egt_sigmoid(-1e9))
__device__ __forceinline__ void fwd_softmax_av_sd(bool valid, const float (&xl)[2], const float (&gl)[2], const float (&Vf)[16],
                                                  float (&mx)[2], float (&sum)[2], float (&deg)[2], float (&O)[16]) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const float xv = xl[j];
    const float mn = valid ? fmaxf(mx[j], xv) : mx[j];
    const float alpha = __expf(mx[j] - mn);
    const float pe = valid ? __expf(xv - mn) : 0.f;
    const float g = valid ? egt_sigmoid(gl[j]) : 0.f;
    mx[j] = mn;
    sum[j] = fmaf(sum[j], alpha, pe);
    deg[j] += g;
    const float av = pe * g;
#pragma unroll
    for (int k = 0; k < 8; ++k) O[2 * k + j] = fmaf(O[2 * k + j], alpha, av * Vf[2 * k + j]);
  }
}

// fwd_row_finish with the degree merged over the 16 key lanes: V_att' = s(deg) V_att to HBM (and the Q slot), deg into slot 3.
// The scaler is evaluated here, once per (row, head), with log1pf (deg reaches 1e-5, where log(1 + deg) has lost its digits).
__device__ __forceinline__ void fwd_row_finish_sd(const BlockArgs& a, size_t rowl, int p, int q, float (&mx)[2], float (&sum)[2],
                                                  float (&deg)[2], float (&O)[16], bool keep, float* qrow) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const float mr2 = row_max16(mx[j]);
    const float f = __expf(mx[j] - mr2);
    mx[j] = mr2;
    sum[j] = row_sum16(sum[j] * f);
    deg[j] = row_sum16(deg[j]);
#pragma unroll
    for (int k = 0; k < 8; ++k) O[2 * k + j] *= f;
  }
  const float o = reduce16_keep_own(O, p);
  const int k = p >> 1, j = p & 1;
  const float sj = j ? sum[1] : sum[0];
  const float dj = j ? deg[1] : deg[0];
  const float vo = (o / sj) * egt_degree_scaler(dj, (a.flags & EGT_BF_SCALER_LINEAR) != 0);
  if (k < a.DK) a.v_att[rowl * a.Dh + k * BH + 2 * q + j] = vo;
  if (keep) qrow[k * BH + 2 * q + j] = vo;
  if (p < 2) {
    float* st = a.stats + (rowl * BH + 2 * q + p) * 4;
    st[0] = p ? mx[1] : mx[0];
    st[1] = sj;
    st[3] = dj;
  }
}

// ---- attention dropout (EGT_BF_ATTN_DROPOUT, egt_layers.py:116-117): the DO instances of the two kernels below ----
// fwd_softmax_av with the keep factor of (pair, head) on av = p . g before it enters O: V_att is the dropped sum.  The softmax sum
// (and with it H_hat, the edge update and the row statistics) does not see the mask.  idx8 = the pair's element index x 8 heads.
__device__ __forceinline__ void fwd_softmax_av_do(const BlockArgs& a, size_t idx8, int q, bool valid, bool gated, const float (&xl)[2],
                                                  const float (&gl)[2], const float (&Vf)[16], float (&mx)[2], float (&sum)[2], float (&O)[16]) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const float xv = xl[j];
    const float mn = valid ? fmaxf(mx[j], xv) : mx[j];
    const float alpha = __expf(mx[j] - mn);
    const float pe = valid ? __expf(xv - mn) : 0.f;
    mx[j] = mn;
    sum[j] = fmaf(sum[j], alpha, pe);
    const float av = (gated ? pe * egt_sigmoid(gl[j]) : pe) * attn_drop_factor(a, idx8, q, j);
#pragma unroll
    for (int k = 0; k < 8; ++k) O[2 * k + j] = fmaf(O[2 * k + j], alpha, av * Vf[2 * k + j]);
  }
}

// ================================================================= forward =====
// Workgroup = (graph b, 16 query rows); wave w owns rows l = 16*lg + w + 4*i.
// KVL: K/V of the graph, Q of the 16 rows and the key-mask adds are staged in LDS.
// ML: attention-mask / injected-random-mask byte streams are present (their loads are
// compiled out of the headline kernel).
// FULL: N is a multiple of 16 (no ragged key tile): validity selects and address clamps fold away.
// SD: EGT_BF_SCALE_DEGREE (gated blocks, fp32 edge tensors): the degree rides next to the softmax sum (fwd_softmax_av_sd / fwd_row_finish_sd).
// DO: EGT_BF_ATTN_DROPOUT: the keep factor on av (fwd_softmax_av_do); never together with SD.
template <int DE, bool KVL, bool ML, bool FULL, bool BF, bool SD = false, bool DO = false>
__global__ void __launch_bounds__(256, ((DE <= 16 && !KVL) ? 4 : 2)) k_block_fwd(BlockArgs a) {   // narrow tiles without K/V in LDS: more resident waves (with K/V in LDS the LDS footprint caps a CU at two workgroups anyway)
  seed_from_device(a);
  using G = Geo<DE>;
  typedef typename EdgeT<BF>::type ET;   // element type of the edge tensors in HBM
  const ET* e_in = reinterpret_cast<const ET*>(a.e);
  ET* e_o = reinterpret_cast<ET*>(a.e_out);
  const ET* dey_in = reinterpret_cast<const ET*>(a.de_out);
  ET* dex_o = reinterpret_cast<ET*>(a.de);
  (void)e_in; (void)e_o; (void)dey_in; (void)dex_o;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = lane & 15, q = lane >> 4;
  const int N = a.N;
  const int RG = a.RGF;   // query rows per workgroup (<= 16; launch_fwd: fewer when the launch would leave workgroup slots empty)
  const int lgroups = (N + RG - 1) / RG;
  const int wg = a.xcd ? egt_xcd_remap(blockIdx.x, gridDim.x) : (int)blockIdx.x;
  const int b = wg / lgroups, lg = wg % lgroups;
  const int l0 = lg * RG, nlr = min(RG, N - l0);   // the group's rows [l0, l0 + nlr)
  float* tl0 = sm + wave * 2 * G::TILE_FLOATS;  // two tiles per wave (ping-pong)
  float* kvs = sm + 8 * G::TILE_FLOATS;         // [N][KV_LD]   (KVL)
  float* qs = kvs + (KVL ? N * KV_LD : 0);     // [16][QS_LD]  (KVL)
  float* kms = qs + (KVL ? 16 * QS_LD : 0);    // [N]          (KVL)
  const bool gated = (a.flags & EGT_BF_GATE) != 0;
  const bool clip = (a.flags & EGT_BF_CLIP) != 0;

  // Start-up loads in as few memory round trips as possible (round 5: hipcc compiled the staging loops as load -> wait -> LDS store
  // per iteration, eight dependent round trips per thread at N = 64, and the 44 weight loads of a lane as one more behind them):
  // the K / V rows go in batches of eight 16-byte loads per thread, the Q rows and the key-mask adds ride in the first batch, and
  // the lane-constant MFMA operands below are requested BEFORE the first batch is waited for.
  float4 kvb[8], qb = make_float4(0.f, 0.f, 0.f, 0.f);
  float kmb = 0.f;
  const float* kvsrc = a.qkvp + (size_t)b * N * QKVP;
  if (KVL) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = threadIdx.x + 256 * u, row = min(i >> 5, N - 1), f = i & 31;
      kvb[u] = *reinterpret_cast<const float4*>(kvsrc + (size_t)row * QKVP + 64 + f * 4);
    }
    {
      const int row = threadIdx.x >> 4, f = threadIdx.x & 15, l = min(l0 + row, N - 1);
      qb = *reinterpret_cast<const float4*>(kvsrc + (size_t)l * QKVP + f * 4);
    }
    if ((int)threadIdx.x < N) kmb = key_mask_add(a, (size_t)b * N + threadIdx.x);
  }
  // lane-constant MFMA operands
  float wA[4 * G::TILES], wrA[G::TILES][2], c2r[4];
  float4 brv[G::TILES];
  fwd_lane_weights<DE>(a, p, q, wA, c2r, wrA, brv);
  if (KVL) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = threadIdx.x + 256 * u, row = i >> 5, f = i & 31;
      if (i < N * 32) *reinterpret_cast<float4*>(kvs + row * KV_LD + f * 4) = kvb[u];
    }
    *reinterpret_cast<float4*>(qs + (threadIdx.x >> 4) * QS_LD + (threadIdx.x & 15) * 4) = qb;
    if ((int)threadIdx.x < N) kms[threadIdx.x] = kmb;
    for (int i = 2048 + threadIdx.x; i < N * 32; i += 256) {   // N > 64: the keys past the first batch
      const int row = i >> 5, f = i & 31;
      *reinterpret_cast<float4*>(kvs + row * KV_LD + f * 4) = *reinterpret_cast<const float4*>(kvsrc + (size_t)row * QKVP + 64 + f * 4);
    }
    for (int i = 256 + threadIdx.x; i < N; i += 256) kms[i] = key_mask_add(a, (size_t)b * N + i);
    __syncthreads();
  }

  const int ntile = (N + 15) / 16;
  int nrows = 0;
  for (int li = 0; li < 4; ++li) nrows += (wave + 4 * li < nlr) ? 1 : 0;
  const int total = nrows * ntile;

  // e tiles in flight per wave.  A De <= 16 tile is 0.5 - 1 KB, so narrow tiles travel PFD
  // iterations ahead in a ring of register sets (more bytes in flight per CU).  The ring is indexed
  // statically (loop unrolled by PFD); the iterations that pad the last group re-run the last tile
  // with every global write predicated off, which keeps the body straight-line (exact waits).
  constexpr int PFD = (DE <= 16 && KVL) ? 4 : 1;   // measured: +3.5 % at De = 8, N = 120; without K/V in LDS the extra registers spill
  TileRegs<DE> ring[PFD];
  auto prefetch = [&](TileRegs<DE>& tr, int it) {
    if (PFD > 1) it = min(it, total - 1);
    const int l = l0 + wave + 4 * (it / ntile), m0 = (it % ntile) * 16;
    const size_t pair0 = ((size_t)b * N + l) * N + m0;
    tile_gload<DE, EGT_NT_FWD_E>(tr, e_in + pair0 * DE, lane, FULL ? 16 : min(16, N - m0));
  };
  if (total > 0) {
#pragma unroll
    for (int k = 0; k < PFD; ++k) prefetch(ring[k], k);
  }

  float Qf[16], mx[2], sum[2], O[16];
  float deg[2] = {0.f, 0.f};   // (SD)
  (void)deg;
  auto step = [&](const int it_, TileRegs<DE>& tr) __attribute__((always_inline)) {
    const bool live = PFD == 1 || it_ < total;
    const int it = PFD == 1 ? it_ : min(it_, total - 1);
    const int li = it / ntile, mt = it % ntile;
    const int l = l0 + wave + 4 * li, m0 = mt * 16, m = m0 + p;
    const bool valid = FULL ? true : (m < N);
    const int rows_valid = FULL ? 16 : min(16, N - m0);
    const size_t rowl = (size_t)b * N + l;
    const size_t pair0 = rowl * N + m0;
    if (mt == 0) {
      frag16(KVL ? reinterpret_cast<const float4*>(qs + (wave + 4 * li) * QS_LD + q * 16)
                 : reinterpret_cast<const float4*>(a.qkvp + rowl * QKVP + q * 16), Qf);
      fwd_row_init(mx, sum, O);
      if constexpr (SD) deg[0] = deg[1] = 0.f;
    }
    // ---- stage this tile, start the next one's loads ----
    MaskRegs mr{make_float2(1.f, 1.f), 0};   // issued before the prefetch, consumed after the MFMAs
    mask_gload<ML>(a, mr, pair0 + (valid ? p : 0), q);
    // Memory order per step: [stores of tile it-1] then [loads of tile it+1]; the wait in front
    // of the next LDS staging therefore never covers a store younger than the loads it needs.
    float* tl = tl0 + (it_ & 1) * G::TILE_FLOATS;
    lds_sync();
    if (it_ > 0 && live) {   // stream out e' of the previous tile from the other buffer
      const int itp = it - 1, lp = l0 + wave + 4 * (itp / ntile), m0p = (itp % ntile) * 16;
      tile_from_lds<DE, EGT_NT_FWD_ST>(tl0 + (itp & 1) * G::TILE_FLOATS, e_o + (((size_t)b * N + lp) * N + m0p) * DE,
                                       lane, FULL ? 16 : min(16, N - m0p));
    }
    tile_lds_put<DE>(tl, tr, lane, rows_valid);
    if (PFD == 1) { if (it + 1 < total) prefetch(tr, it + 1); }
    else prefetch(tr, it_ + PFD);   // this slot's next tile (clamped past the end)
    lds_sync();
    float4 x[G::TILES];
#pragma unroll
    for (int t = 0; t < G::TILES; ++t) x[t] = frag_read<DE>(tl, p, q, t);
    // ---- K/V fragments of key m ----
    float Kf[16], Vf[16], kadd = 0.f;
    {
      const int mc = valid ? m : 0;
      if (KVL) {
        kv_frags(reinterpret_cast<const float4*>(kvs + mc * KV_LD + q * 16),
                 reinterpret_cast<const float4*>(kvs + mc * KV_LD + 64 + q * 16), Kf, Vf);
        kadd = kms[mc];
      } else {
        const size_t rowm = (size_t)b * N + mc;
        kv_frags_row(a, rowm, q, Kf, Vf);
        kadd = key_mask_add(a, rowm);
      }
    }
    // ---- norm_edge + [attention_gates | dense_edge_b] ----
    v4f acc = {c2r[0], c2r[1], c2r[2], c2r[3]};
    {
      ln_frags<DE>(x, q, a.ln_eps, (a.flags & EGT_BF_NO_EDGE_LN) == 0);
      acc = project<DE>(x, wA, acc);
    }
    float hh[2] = {0.f, 0.f}, xl[2] = {0.f, 0.f}, gl[2] = {0.f, 0.f};
    fwd_pair_logits(a, clip, Qf, Kf, acc, hh, xl, gl);
    apply_masks<ML>(a, kadd, mr, (pair0 + p) * BH, q, xl, gl);
    if constexpr (SD) fwd_softmax_av_sd(valid, xl, gl, Vf, mx, sum, deg, O);
    else if constexpr (DO) fwd_softmax_av_do(a, (pair0 + p) * BH, q, valid, gated, xl, gl, Vf, mx, sum, O);
    else fwd_softmax_av(valid, gated, xl, gl, Vf, mx, sum, O);
    fwd_edge_update<DE>(tl, p, q, valid, hh, wrA, brv);
    if (it_ + 1 == total) {   // last tile of the wave: flush
      lds_sync();
      tile_from_lds<DE, EGT_NT_FWD_ST>(tl, e_o + pair0 * DE, lane, rows_valid);
    }
    if (mt == ntile - 1 && live) {
      // the row's Q is dead (read at mt == 0 by this wave only): its slot keeps V_att for the epilogue
      if constexpr (SD) fwd_row_finish_sd(a, rowl, p, q, mx, sum, deg, O, KVL && a.epi, qs + (wave + 4 * li) * QS_LD);
      else if (!ML) fwd_row_finish(a, rowl, p, q, mx, sum, O, KVL && a.epi, qs + (wave + 4 * li) * QS_LD);
      else {
        // Own copy of fwd_row_finish in the mask-tensor instances: with the shared one <64, true, true, false, false> (attention mask,
        // h [128, 64, 64]) ran 69.8 us against the parent's 66.4 (its max - min over three runs: 0.5), with this copy 66.8.  In the
        // instances without mask tensors it is the copy that costs: <64, false, false, false, false> (h [32, 90, 64]) 56.4 us against
        // the parent's 54.0 (1.0) where the shared function ran 51.0 against 56.1 (1.8) in another visit.
        // ---- merge the 16 key lanes (same q): max, then sums ----
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const float mr2 = row_max16(mx[j]);
          const float f = __expf(mx[j] - mr2);
          mx[j] = mr2;
          sum[j] = row_sum16(sum[j] * f);
#pragma unroll
          for (int k = 0; k < 8; ++k) O[2 * k + j] *= f;
        }
        const float o = reduce16_keep_own(O, p);
        // element i = p: k = p>>1, j = p&1 -> head 2q + j
        const int k = p >> 1, j = p & 1;
        const float sj = j ? sum[1] : sum[0];
        const float vo = o / sj;
        if (k < a.DK) a.v_att[rowl * a.Dh + k * BH + 2 * q + j] = vo;
        if (KVL && a.epi) qs[(wave + 4 * li) * QS_LD + k * BH + 2 * q + j] = vo;
        if (p < 2) {
          float* st = a.stats + (rowl * BH + 2 * q + p) * 4;
          st[0] = p ? mx[1] : mx[0];
          st[1] = sj;
        }
      }
    }
  };
  if (PFD == 1) {
    for (int it = 0; it < total; ++it) step(it, ring[0]);
  } else {
    for (int it0 = 0; it0 < total; it0 += PFD) {
#pragma unroll
      for (int k = 0; k < PFD; ++k) step(it0 + k, ring[k]);
    }
  }

  // ---- node-side epilogue (Dh = 64): the workgroup holds V_att of its 16 rows ----
  //   epi >= 1: h' = V_att.Wo + bo + h                      (dense_mha + res_mha, :136,140)
  //   epi == 2: qkv of the NEXT block = LN(h').Wqkv' + bqkv' (norm_mha + dense_qkv, :109,113), packed
  // Contraction order k = 4s + q on both MFMA operands; weights come straight from L2.
  if (KVL && a.epi) fwd_node_epilogue(a, sm, qs, b, l0, nlr, N, wave, p, q);
}

// ---------------------------------------------------------------- forward, narrow edge channels ---
// k_block_fwd walks (row, key tile) pairs one 16-pair tile at a time; for De <= 16 such a tile is
// 0.5 - 1 KB and a third of the time is the per-iteration skeleton (staging, LDS hand-offs, index
// arithmetic), the rest a chain of short dependent phases (see the ablation in DESIGN.md).  This
// variant turns the loop inside out: one iteration = ONE key tile for all FOUR rows of the wave.
// The K / V fragments and the key-mask add are fetched once per iteration and shared by the four
// rows, the four e tiles are staged with one pair of LDS hand-offs, and the four rows' LN ->
// projection -> softmax -> A.V -> dense_edge_r chains are independent, so the scheduler interleaves
// them (ILP x4 instead of one latency-bound chain).  Q stays in LDS (re-read per key tile), the
// running softmax state of the four rows lives in registers.  K/V of the graph in LDS (KVL) only;
// no mask tensors (the ML variants stay on k_block_fwd).
// NW = 4: 16 rows per workgroup, two workgroups per CU; NW = 8: 32 rows (two 16-row halves), ONE
// workgroup per CU -- same occupancy, but K/V of a graph up to N ~ 250 still fits in LDS and is staged
// once per 32 rows.
template <int DE, bool FULL, int NW, bool BF, bool SD = false, bool DO = false>
__global__ void __launch_bounds__(64 * NW, 2) k_block_fwd_r4(BlockArgs a) {
  seed_from_device(a);
  typedef typename EdgeT<BF>::type ET;   // element type of the edge tensors in HBM
  constexpr int RW = 4 * NW, NT = 64 * NW;   // rows / threads per workgroup
  using G = Geo<DE>;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = lane & 15, q = lane >> 4;
  const int hf = wave >> 2, wv = wave & 3;   // 16-row half of the workgroup, wave inside it
  const int N = a.N;
  const int lgroups = (N + RW - 1) / RW;
  const int wg = a.xcd ? egt_xcd_remap(blockIdx.x, gridDim.x) : (int)blockIdx.x;
  const int b = wg / lgroups, lg = wg % lgroups;
  float* tl = sm + wave * 4 * G::TILE_FLOATS;    // the wave's four tiles (one per row)
  float* kvs = sm + 4 * NW * G::TILE_FLOATS;     // [N][KV_LD]
  float* qs = kvs + N * KV_LD;                   // [RW][QS_LD]
  float* kms = qs + RW * QS_LD;                  // [N]
  const bool gated = (a.flags & EGT_BF_GATE) != 0;
  const bool clip = (a.flags & EGT_BF_CLIP) != 0;
  {
    const float* src = a.qkvp + (size_t)b * N * QKVP;
    fwd_stage_kv<NT>(kvs, src, N);
    for (int i = threadIdx.x; i < RW * 16; i += NT) {
      const int row = i >> 4, f = i & 15, l = min(lg * RW + row, N - 1);
      *reinterpret_cast<float4*>(qs + row * QS_LD + f * 4) =
          *reinterpret_cast<const float4*>(src + (size_t)l * QKVP + f * 4);
    }
    for (int i = threadIdx.x; i < N; i += NT) kms[i] = key_mask_add(a, (size_t)b * N + i);
  }
  float wA[4 * G::TILES], wrA[G::TILES][2], c2r[4];
  float4 brv[G::TILES];
  fwd_lane_weights<DE>(a, p, q, wA, c2r, wrA, brv);
  __syncthreads();

  const int ntile = (N + 15) / 16;
  int nrows = 0;
  const int row0 = hf * 16 + wv;   // the wave's rows inside the workgroup: row0 + 4i
#pragma unroll
  for (int i = 0; i < 4; ++i) nrows += (lg * RW + row0 + 4 * i < N) ? 1 : 0;   // rows i < nrows exist
  if (nrows > 0) {
    const ET* e_in = reinterpret_cast<const ET*>(a.e);
    ET* e_o = reinterpret_cast<ET*>(a.e_out);
    size_t rowl[4];   // rows past the end alias the last real row: loaded, never computed or stored
#pragma unroll
    for (int i = 0; i < 4; ++i) rowl[i] = (size_t)b * N + lg * RW + row0 + 4 * min(i, nrows - 1);
    TileRegs<DE> tr[4];
    auto prefetch = [&](int mt) {
      const int m0 = mt * 16;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        tile_gload<DE>(tr[i], e_in + (rowl[i] * N + m0) * DE, lane, FULL ? 16 : min(16, N - m0));
    };
    prefetch(0);
    float mx[4][2], sum[4][2], O[4][16];
    float deg[4][2] = {};   // (SD)
    (void)deg;
#pragma unroll
    for (int i = 0; i < 4; ++i) fwd_row_init(mx[i], sum[i], O[i]);
    for (int mt = 0; mt < ntile; ++mt) {
      const int m0 = mt * 16, m = m0 + p;
      const bool valid = FULL ? true : (m < N);
      const int rows_valid = FULL ? 16 : min(16, N - m0);
      lds_sync();   // the e' tiles of the previous key tile have left the LDS tiles
#pragma unroll
      for (int i = 0; i < 4; ++i) tile_lds_put<DE>(tl + i * G::TILE_FLOATS, tr[i], lane, rows_valid);
      if (mt + 1 < ntile) prefetch(mt + 1);
      lds_sync();
      // ---- K/V fragments of key m: shared by the four rows ----
      float Kf[16], Vf[16];
      const int mc = valid ? m : 0;
      kv_frags(reinterpret_cast<const float4*>(kvs + mc * KV_LD + q * 16),
               reinterpret_cast<const float4*>(kvs + mc * KV_LD + 64 + q * 16), Kf, Vf);
      const float kadd = kms[mc];
      const MaskRegs mr{make_float2(1.f, 1.f), 0};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (i < nrows) {
          float* tli = tl + i * G::TILE_FLOATS;
          float4 x[G::TILES];
#pragma unroll
          for (int t = 0; t < G::TILES; ++t) x[t] = frag_read<DE>(tli, p, q, t);
          // ---- norm_edge + [attention_gates | dense_edge_b] ----
          ln_frags<DE>(x, q, a.ln_eps, (a.flags & EGT_BF_NO_EDGE_LN) == 0);
          v4f acc = {c2r[0], c2r[1], c2r[2], c2r[3]};
          acc = project<DE>(x, wA, acc);
          // ---- scaled QK^T, clip, + E (egt_layers.py:79-86); Q of the row from LDS ----
          float Qf[16];
          frag16(reinterpret_cast<const float4*>(qs + (row0 + 4 * i) * QS_LD + q * 16), Qf);
          float hh[2], xl[2], gl[2];
          fwd_pair_logits(a, clip, Qf, Kf, acc, hh, xl, gl);
          apply_masks<false>(a, kadd, mr, (rowl[i] * N + m0 + p) * BH, q, xl, gl);
          // ---- online softmax x gate, A.V (per lane).  Own copy of fwd_softmax_av: with the shared one r4<8, false, 8, false> ran
          // 165.5 us against the parent's 161.4 (max - min 0.7) and r4<8, false, 4, false> 98.5 against 97.2 (0.3); with this copy
          // 160.4 and 96.2 ----
          if constexpr (SD) fwd_softmax_av_sd(valid, xl, gl, Vf, mx[i], sum[i], deg[i], O[i]);
          else if constexpr (DO) fwd_softmax_av_do(a, (rowl[i] * N + m0 + p) * BH, q, valid, gated, xl, gl, Vf, mx[i], sum[i], O[i]);
          else
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const float xv = xl[j];
            const float mn = valid ? fmaxf(mx[i][j], xv) : mx[i][j];
            const float alpha = __expf(mx[i][j] - mn);
            const float pe = valid ? __expf(xv - mn) : 0.f;
            mx[i][j] = mn;
            sum[i][j] = fmaf(sum[i][j], alpha, pe);
            const float av = gated ? pe * egt_sigmoid(gl[j]) : pe;
#pragma unroll
            for (int k = 0; k < 8; ++k) O[i][2 * k + j] = fmaf(O[i][2 * k + j], alpha, av * Vf[2 * k + j]);
          }
          fwd_edge_update<DE>(tli, p, q, valid, hh, wrA, brv);
        }
      }
      lds_sync();   // stream out the four e' tiles
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (i < nrows) tile_from_lds<DE>(tl + i * G::TILE_FLOATS, e_o + (rowl[i] * N + m0) * DE, lane, rows_valid);
    }
    // ---- per row: 16-lane merge, V_att (also into the row's Q slot: dead from here on), statistics ----
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < nrows) {
        if constexpr (SD) fwd_row_finish_sd(a, rowl[i], p, q, mx[i], sum[i], deg[i], O[i], a.epi != 0, qs + (row0 + 4 * i) * QS_LD);
        else fwd_row_finish(a, rowl[i], p, q, mx[i], sum[i], O[i], a.epi != 0, qs + (row0 + 4 * i) * QS_LD);
      }
  }
  // each 16-row half runs the 4-wave epilogue on its own rows (staging area hs = its own tiles)
  if (a.epi) fwd_node_epilogue(a, sm + hf * 16 * QS_LD, qs + hf * 16 * QS_LD, b, lg * RW + hf * 16, min(16, N - (lg * RW + hf * 16)), N, wv, p, q);
}


// ---------------------------------------------------------------- forward, the headline shape at compile time ---
// k_block_fwd<64, true, false, true, false> for ONE descriptor, with everything the generic kernel tests per tile known to the
// compiler: N = 64 (four key tiles per row), De = 64, d = 8 (Dh = 64), gate + clip + edge LayerNorm, training with the in-kernel
// random mask, a key mask, no mask tensors, 16-row groups, the node epilogue on (plan_for / launch_tile_fwd check every one of these;
// any other call takes the generic instance).  Same LDS carve-up, same staging, same phase functions in the same order on the same
// operands -- the results are bit-identical -- but the wave's loop is written per row with its four key tiles unrolled: the Q fragment,
// fwd_row_init and fwd_row_finish sit outside the tile body, the first tile of the wave (no previous e' to store) and the last one (flush,
// no prefetch) are peeled, the LDS ping-pong buffer of a tile is a constant, and a global address is a wave-uniform base plus a 32-bit
// lane offset.  The launch constants reach the phase functions through `a` itself: the kernel overwrites its own copy of those fields
// with the literals.  (One row loop that tests the row index at its first and last tile instead of the peeled rows measured 55.2 us
// per launch against 54.7; the generic instance 57.3.)  DE = 64 is the only instance.
template <int DE>
__global__ void __launch_bounds__(256, 2) k_block_fwd_s64(BlockArgs a) {
  static_assert(DE == 64, "k_block_fwd_s64 is written for the headline shape");
  seed_from_device(a);
  constexpr int N = 64, NTILE = N / 16;
  using G = Geo<DE>;
  a.N = N; a.De = DE; a.DK = 8; a.Dh = 64;
  a.flags = EGT_BF_GATE | EGT_BF_CLIP | EGT_BF_TRAINING;
  a.rng_rm = 1; a.rm = nullptr; a.M = nullptr;
  __builtin_assume(a.km != nullptr);
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int p = lane & 15, q = lane >> 4;
  const int wg = a.xcd ? egt_xcd_remap(blockIdx.x, gridDim.x) : (int)blockIdx.x;
  const int b = wg / NTILE, l0 = (wg % NTILE) * 16;   // four 16-row groups per graph
  float* tl0 = sm + wave * 2 * G::TILE_FLOATS;  // two tiles per wave (ping-pong)
  float* kvs = sm + 8 * G::TILE_FLOATS;         // [N][KV_LD]
  float* qs = kvs + N * KV_LD;                  // [16][QS_LD]
  float* kms = qs + 16 * QS_LD;                 // [N]

  // start-up loads as in k_block_fwd: one batch of K / V rows, the Q rows and the key-mask adds, the lane-constant operands behind them
  float4 kvb[8], qb;
  float kmb = 0.f;
  const float* kvsrc = a.qkvp + (size_t)b * N * QKVP;
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int i = threadIdx.x + 256 * u, row = i >> 5, f = i & 31;
    kvb[u] = *reinterpret_cast<const float4*>(kvsrc + row * QKVP + 64 + f * 4);
  }
  qb = *reinterpret_cast<const float4*>(kvsrc + (l0 + (threadIdx.x >> 4)) * QKVP + (threadIdx.x & 15) * 4);
  if ((int)threadIdx.x < N) kmb = key_mask_add(a, (size_t)b * N + threadIdx.x);
  float wA[4 * G::TILES], wrA[G::TILES][2], c2r[4];
  float4 brv[G::TILES];
  fwd_lane_weights<DE>(a, p, q, wA, c2r, wrA, brv);
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int i = threadIdx.x + 256 * u, row = i >> 5, f = i & 31;
    *reinterpret_cast<float4*>(kvs + row * KV_LD + f * 4) = kvb[u];
  }
  *reinterpret_cast<float4*>(qs + (threadIdx.x >> 4) * QS_LD + (threadIdx.x & 15) * 4) = qb;
  if ((int)threadIdx.x < N) kms[threadIdx.x] = kmb;
  __syncthreads();

  // the wave's rows: l0 + wave + 4 li, li < 4.  Tile (li, mt) of e / e' lies ROW * li + 16 * DE * mt floats behind the wave's base.
  constexpr int ROW = 4 * N * DE;
  const uint32_t row0 = (uint32_t)(b * N + l0 + wave);             // [B * N] index of row li = 0 (wave-uniform)
  const float* e_w = a.e + (size_t)row0 * N * DE;
  float* eo_w = a.e_out + (size_t)row0 * N * DE;
  const float* kvl = kvs + p * KV_LD + q * 16;                     // the lane's key of tile 0
  const uint32_t lane8 = (uint32_t)p * BH;                         // the lane's part of the mask counter (pair index x 8 heads)
  TileRegs<DE> tr;
  tile_gload<DE, EGT_NT_FWD_E>(tr, e_w, lane, 16);

  float Qf[16], mx[2], sum[2], O[16];
  // one key tile.  Memory order as in k_block_fwd: [store of the previous tile's e'] then [loads of the next tile]
  auto tile = [&](const int li, const int mt, const bool first, const bool last) __attribute__((always_inline)) {
    float* tl = tl0 + (mt & 1) * G::TILE_FLOATS;
    float* tlp = tl0 + ((mt & 1) ^ 1) * G::TILE_FLOATS;
    const int off = li * ROW + mt * 16 * DE;   // (< 2^20 floats)
    lds_sync();
    if (!first) tile_from_lds<DE, EGT_NT_FWD_ST>(tlp, eo_w + (off - (mt ? 16 * DE : ROW - 3 * 16 * DE)), lane, 16);
    tile_lds_put<DE>(tl, tr, lane, 16);
    if (!last) tile_gload<DE, EGT_NT_FWD_E>(tr, e_w + (off + (mt < NTILE - 1 ? 16 * DE : ROW - 3 * 16 * DE)), lane, 16);
    lds_sync();
    float4 x[G::TILES];
#pragma unroll
    for (int t = 0; t < G::TILES; ++t) x[t] = frag_read<DE>(tl, p, q, t);
    float Kf[16], Vf[16];
    kv_frags(reinterpret_cast<const float4*>(kvl + mt * 16 * KV_LD), reinterpret_cast<const float4*>(kvl + mt * 16 * KV_LD + 64), Kf, Vf);
    const float kadd = kms[mt * 16 + p];
    // ---- norm_edge + [attention_gates | dense_edge_b] ----
    v4f acc = {c2r[0], c2r[1], c2r[2], c2r[3]};
    ln_frags<DE>(x, q, a.ln_eps, true);
    acc = project<DE>(x, wA, acc);
    float hh[2] = {0.f, 0.f}, xl[2] = {0.f, 0.f}, gl[2] = {0.f, 0.f};
    fwd_pair_logits(a, true, Qf, Kf, acc, hh, xl, gl);
    const MaskRegs mr{make_float2(1.f, 1.f), 0};
    const uint32_t idx8 = ((row0 + 4u * li) * N + 16u * mt) * BH + lane8;   // == (uint32_t)((pair0 + p) * BH) of k_block_fwd
    apply_masks<false>(a, kadd, mr, (size_t)idx8, q, xl, gl);
    fwd_softmax_av(true, true, xl, gl, Vf, mx, sum, O);
    fwd_edge_update<DE>(tl, p, q, true, hh, wrA, brv);
    if (last) {   // last tile of the wave: flush
      lds_sync();
      tile_from_lds<DE, EGT_NT_FWD_ST>(tl, eo_w + off, lane, 16);
    }
  };
  auto row = [&](const int li, const bool first, const bool last) __attribute__((always_inline)) {
    float* qrow = qs + (wave + 4 * li) * QS_LD;
    frag16(reinterpret_cast<const float4*>(qrow + q * 16), Qf);
    fwd_row_init(mx, sum, O);
    tile(li, 0, first, false);
    tile(li, 1, false, false);
    tile(li, 2, false, false);
    tile(li, 3, false, last);
    // the row's Q is dead (read above by this wave only): its slot keeps V_att for the epilogue
    fwd_row_finish(a, (size_t)(row0 + 4u * li), p, q, mx, sum, O, true, qrow);
  };
  row(0, true, false);
#pragma unroll 1
  for (int li = 1; li < 3; ++li) row(li, false, false);
  row(3, false, true);
  fwd_node_epilogue(a, sm, qs, b, l0, 16, N, wave, p, q);
}
