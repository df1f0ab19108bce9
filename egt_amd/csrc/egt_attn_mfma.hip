// Inner op on MFMA tiles (flash-style) for the large-head geometry (d in {16,32,64}, H = 8):
//   (V_att, H_hat) = EGT([QKV, E?, G?, M?], mask)     lib/models/egt_layers.py:57-213
// and its backward (SURVEY.md appendix A / egt_layers.py semantics under autodiff).
// This is the shape where QK^T / A.V carry the arithmetic (BASELINE config 5: N = 512, d = 64: fp32
// arithmetic intensity at the ridge), so every contraction runs on v_mfma_f32_16x16x4_f32 (exact fp32)
// and the N x N probabilities never exist outside registers.
//
// The kernels are in egt_attn_kernels.h, ONE body each for two operand forms: this unit instantiates MM = 0 (what is described
// here) and holds the plan and the C ABI of both; egt_attn_bf16.hip instantiates MM = 1 (bf16 products, opt-in) of the same bodies.
//
// Round-4 structure (what bounds an fp32 MFMA kernel on gfx950: DESIGN.md 4.0 -- MFMA and VALU issue
// ADD on a SIMD, everything else can hide):
//   * a pack kernel rewrites Q (pre-scaled by d^-1/2), K, V, dV_att head-major and tile-major, row form
//     [B,H,NP/16,d/16,16,16] and transposed form [B,H,NP/16,d,16]: EVERY MFMA operand that comes from
//     them is one aligned 16-byte global load per four contraction steps, straight into the lane that
//     feeds the matrix core (contraction order kappa(T,u,q) = 16T + 4q + u on both operands);
//   * workgroup = (32-row block, 4 heads): 4 COMPUTE waves (one per SIMD, one head each) whose instruction
//     stream is ds_read + MFMA + VALU only, and 4 LOADER waves that own every vector-memory instruction
//     (one global_load in an fp32 MFMA stream costs its wave ~80 cycles of issue, a ds_read_b128 ~7; LDS-DMA
//     loaders beside the compute waves cost them nothing: tools/micro/mfma_stream.hip).  A compute wave
//     works on two 16-row tiles at once, so every operand fragment read from LDS feeds two MFMAs.  The
//     [N,N,8] pair tensors cross the heads <-> pairs layout change through head-major LDS planes: a
//     loader thread moves 16 bytes (4 heads of one pair) per tensor and 16 x 16 sub-tile, two iterations ahead;
//   * ONE barrier per iteration and it does not drain the vector-memory queue (s_waitcnt lgkmcnt(0) +
//     s_barrier, not __syncthreads): operand prefetches and output stores stay in flight across it;
//   * the elementwise skeleton is cut to the arithmetic: additive masks from a per-key LDS table
//     (0 / -1e9 / -3e38 for keys past N: no selects), v_med3 clip, exp2 with folded constants,
//     v_rcp sigmoid, Q pre-scaled;
//   * backward: K / V fragments and the dK / dV accumulators of two key tiles stay in registers while the
//     workgroup walks the query tiles; the Q / dO tile of a query tile is staged ONCE by LDS-DMA and read
//     in BOTH operand forms (row form b128, transposed form b32: no transposing MFMAs, no transposed
//     arrays); planes are key-major there so a lane moves its four query rows with one ds_read_b128;
//     dA = dH*c leaves in the lane's own layout (one 16-byte store) for k_attn_mfma_bwd_q, which is a
//     pure operand-streaming MFMA kernel (no LDS, no barrier).
// Attributes outside this cover (dropout, degree scalers, A_tild output, H != 8, other d) use the
// general kernels of egt_attn.hip.
#include <stdlib.h>

#include "egt_attn_kernels.h"   // the inner op's four kernels: this unit instantiates their exact-fp32 form (MM = 0)
#include "egt_pair.h"   // the fused pair operator of the same geometry (k_pair_fwd / k_pair_bwd)

// ------------------------------------------------------------------ host glue --
extern "C" int egt_attn_mfma_supported(const egt_attn_desc* d, int need_a_tild) {
  if (!d || d->dtype != EGT_F32 || d->H != AH) return 0;
  if (d->d != 16 && d->d != 32 && d->d != 64) return 0;
  if (d->flags & EGT_F_SCALE_DEGREE) return 0;
  if ((d->flags & EGT_F_TRAINING) && d->attn_dropout > 0.0f) return 0;
  if (need_a_tild) return 0;
  if ((size_t)d->B * d->N * d->N * d->H > 0xFFFFFFFFull) return 0;
  if (d->N > 2048) return 0;   // the forward keeps two per-key tables of N floats in LDS beside its stages
  return 1;
}

static int np_of(int N) { return (N + 15) & ~15; }

// Every launch and workspace decision of this file is made in ONE place, plan_attn, once per C-ABI call: the size queries return
// its totals, fill / pair_fill check the descriptor and bind the call's pointers, the entry points bind the workspace and launch
// from it.  Workspace, in floats: the packed operand arrays (PK_* order, B*H*NP*d each; a forward alone needs only the first
// PK_FWD_COUNT), stats2 [B,H,NP,4], dA [B,H,NP,NP]; the pair operator appends its parameter-gradient partials, nwg + 1 of each
// kind (the last one: the reduced image), the 1 KB store dump (PairArgs::dump) and the prepared weight table (PairArgs::wprep).
// EGT_ATTN_MM_BF16 (the kernels' MM = 1 form) keeps the layout and every launch shape but the dA tiles: those are bf16 there (half the
// bytes, half the dA pieces of a k_attn_mfma_bwd_q stage); the operand arrays keep fp32 containers.
struct AttnPlan {
  int NP;
  size_t stats2, dA, fwd_total, total;   // fwd_total: egt_attn_mfma_fwd's workspace (all of it with EGT_ATTN_WS_SHARED)
  int nwg;                               // pair: workgroups of k_pair_fwd / k_pair_bwd = partials of each kind
  size_t part_proj, red_proj, part_upd, red_upd, dump, wprep;
  int pack_fwd, pack_bwd;                // PACK_* bits of each direction's k_attn_pack: a shared workspace packs q / k / v once
  int var_fwd, var_bwd;                  // attention: 1 / 2 the straight-line instances (see Feat), 0 the run-time-switched one; pair: V
  bool bf16;                             // attention: EGT_ATTN_MM_BF16 -- the MM = 1 instances, in egt_attn_bf16.hip (same geometry; bf16 dA tiles)
  bool full;                             // pair: N is a multiple of 16 (k_pair_* FULL)
  EgtLaunch pack, fwd, bwd_kv, bwd_q, prep, pair_fwd, pair_bwd;
};

static AttnPlan plan_attn(int B, int N, int D, int reserved, bool pair, int var_fwd, int var_bwd) {
  constexpr int DE = 32, HS = (64 / 16) * 256;   // the pair operator's geometry (d = 64)
  constexpr size_t PSZ1 = DE * 16 + 16, PSZ2 = AH * DE + DE, WTABLE = (3 * (DE / 16) + 1) * 64 * 4;
  const bool shared = (reserved & EGT_ATTN_WS_SHARED) != 0;
  AttnPlan P{};
  const int NP = P.NP = np_of(N);
  const size_t arr = (size_t)B * AH * NP * D;
  P.bf16 = !pair && (reserved & EGT_ATTN_MM_BF16) != 0;
  P.stats2 = PK_COUNT * arr;
  P.dA = P.stats2 + (size_t)B * AH * NP * 4;
  P.total = P.dA + (size_t)B * AH * NP * NP / (P.bf16 ? 2 : 1);   // (bf16 dA tiles: NP is a multiple of 16)
  P.fwd_total = shared ? P.total : PK_FWD_COUNT * arr;
  P.nwg = B * (NP / 16);
  if (pair) {
    P.part_proj = P.total;
    P.red_proj = P.part_proj + (size_t)P.nwg * PSZ1;
    P.part_upd = P.red_proj + PSZ1;
    P.red_upd = P.part_upd + (size_t)P.nwg * PSZ2;
    P.dump = P.red_upd + PSZ2;
    P.wprep = P.dump + 256;
    P.total = P.wprep + WTABLE;
  }
  P.pack_fwd = PACK_Q | PACK_KH | PACK_VT | (shared ? (PACK_KT | PACK_VH) : 0);
  P.pack_bwd = PACK_O | (shared ? 0 : (PACK_Q | PACK_KH | PACK_KT | PACK_VH));
  P.var_fwd = var_fwd; P.var_bwd = var_bwd;
  P.full = N % 16 == 0;
  const size_t keys = (size_t)((NP + 16 + 3) & ~3);   // the forwards' two per-key LDS tables
  P.pack = {B * (NP / 16), 512, (size_t)AH * (16 * (D == 16 ? 16 : 80) + 4) * 4};
  P.fwd = {B * ((NP / 16 + FQ - 1) / FQ) * 2, 512, OPS_BYTES + (2 * keys + (size_t)(2 * (var_fwd ? 2 : 3) + 2) * FQ * 4 * PT_PL) * 4};
  P.bwd_kv = {B * ((NP / 16 + BK - 1) / BK) * 2, 512, OPS_BYTES + ((size_t)2 * 4 * 64 + (size_t)(2 * 3 + 4) * BK * 4 * PT_PL) * 4};
  P.bwd_q = {B * AH * ((NP / 16 + QW_TILES - 1) / QW_TILES), 512, (size_t)QW_STAGES * (2 * (D / 16) + (P.bf16 ? 1 : 2) * QW_TILES) * 1024};   // (bf16: both key tiles of a trip in one dA piece)
  P.prep = {1, 64, 0};
  P.pair_fwd = {P.nwg, 64 * PR_WAVES, ((size_t)2 * AH * HS + 2 * keys + (size_t)6 * AH * PT_PL + 16 + DE) * sizeof(float)};
  P.pair_bwd = {P.nwg, 64 * PR_WAVES, ((size_t)2 * 4 * 2 * HS + (size_t)2 * 3 * AH * PT_PL + (size_t)2 * AH * 64 + (size_t)4 * 2 * 16 * DE +
                                       (size_t)3 * (DE / 16) * 64 * 4 + 64 * 4 + 4 * 2 * 4 * 16) * sizeof(float)};
  return P;
}
// The attention's instances depend on which optional pointers the call passes: a = its bound arguments (nullptr: a size query).
// EGT_ATTN_GENERIC (tests) forces the run-time-switched instance; it is read at the first launch.
static AttnPlan plan_attn(const egt_attn_desc* d, const AttnMfmaArgs* a = nullptr) {
  if (!a) return plan_attn(d->B, d->N, d->d, d->reserved, false, 0, 0);
  static const bool generic = getenv("EGT_ATTN_GENERIC") != nullptr;
  const bool main_cfg = !generic && a->E && (a->flags & EGT_F_GATE_INPUT) && a->G && !a->M && a->km && (a->flags & EGT_F_CLIP) && !a->rm;
  const int v = main_cfg ? (a->rng_rm ? 2 : 1) : 0;
  return plan_attn(d->B, d->N, d->d, d->reserved, false, v, (a->d_h_ext && a->d_E && a->d_G) ? v : 0);
}
static AttnPlan plan_attn(const egt_block_desc* d) {   // the pair operator: V = 2 with the in-kernel random mask
  const int v = ((d->flags & EGT_BF_TRAINING) && d->random_mask_prob > 0.0f) ? 2 : 1;
  return plan_attn(d->B, d->N, d->d, d->reserved, true, v, v);
}

extern "C" size_t egt_attn_mfma_workspace_bytes(const egt_attn_desc* d) {
  return egt_attn_mfma_supported(d, 0) ? plan_attn(d).total * sizeof(float) : 0;
}
extern "C" size_t egt_attn_mfma_fwd_workspace_bytes(const egt_attn_desc* d) {
  return egt_attn_mfma_supported(d, 0) ? plan_attn(d).fwd_total * sizeof(float) : 0;
}

static int fill(const egt_attn_desc* desc, const void* qkv, const void* E, const void* G,
                const uint8_t* key_mask, const void* attn_mask, const uint8_t* rand_mask, void* workspace,
                AttnMfmaArgs& a) {
  if (!egt_attn_mfma_supported(desc, 0)) EGT_FAIL(EGT_E_SHAPE, "configuration not covered by the MFMA inner-op kernel");
  if (!qkv || !workspace) EGT_FAIL(EGT_E_NULL, "qkv/workspace is NULL");
  if (desc->reserved & ~(EGT_ATTN_WS_SHARED | EGT_ATTN_MM_BF16))
    EGT_FAIL(EGT_E_FLAGS, "egt_attn_desc.reserved: unknown bits 0x%x (EGT_ATTN_WS_SHARED | EGT_ATTN_MM_BF16 are defined)", desc->reserved);
  if ((desc->flags & EGT_F_EDGE_INPUT) && !E) EGT_FAIL(EGT_E_NULL, "edge_input set but E is NULL");
  if ((desc->flags & EGT_F_GATE_INPUT) && !G) EGT_FAIL(EGT_E_NULL, "gate_input set but G is NULL");
  if ((desc->flags & EGT_F_ATTN_MASK) && !attn_mask) EGT_FAIL(EGT_E_NULL, "attn_mask set but M is NULL");
  a = AttnMfmaArgs{};
  a.B = desc->B; a.N = desc->N; a.NP = np_of(desc->N); a.d = desc->d; a.flags = desc->flags;
  a.clip_lo = desc->clip_lo; a.clip_hi = desc->clip_hi;
  a.scale = 1.0f / sqrtf((float)desc->d);
  a.rm_thr = egt_threshold24(desc->random_mask_prob);
  a.s0 = (uint32_t)(desc->seed & 0xFFFFFFFFull); a.s1 = (uint32_t)(desc->seed >> 32);
  a.qkv = (const float*)qkv;
  a.E = (desc->flags & EGT_F_EDGE_INPUT) ? (const float*)E : nullptr;
  a.G = (desc->flags & EGT_F_GATE_INPUT) ? (const float*)G : nullptr;
  a.M = (desc->flags & EGT_F_ATTN_MASK) ? (const float*)attn_mask : nullptr;
  a.km = key_mask;
  if ((desc->flags & EGT_F_TRAINING) && desc->random_mask_prob > 0.0f) {
    if (rand_mask) a.rm = rand_mask; else a.rng_rm = 1;
  }
  a.pk = (float*)workspace;
  return EGT_OK;
}

extern "C" int egt_attn_mfma_fwd(const egt_attn_desc* desc, const void* qkv, const void* E,
                                 const void* G, const uint8_t* key_mask, const void* attn_mask,
                                 const uint8_t* rand_mask, void* v_att, void* h_hat, void* rowstats,
                                 void* workspace, void* stream) {
  AttnMfmaArgs a;
  int rc = fill(desc, qkv, E, G, key_mask, attn_mask, rand_mask, workspace, a);
  if (rc) return rc;
  if (!v_att || !h_hat || !rowstats) EGT_FAIL(EGT_E_NULL, "v_att/h_hat/rowstats is NULL");
  a.v_att = (float*)v_att; a.h_hat = (float*)h_hat; a.rowstats = (float*)rowstats;
  const AttnPlan P = plan_attn(desc, &a);
  a.pack_what = P.pack_fwd;
  if (P.bf16) egt_attn_bf16_launch_fwd(P.var_fwd, P.pack, P.fwd, a, (hipStream_t)stream);   // (the MM = 1 instances: egt_attn_bf16.hip)
  else attn_launch_fwd<0>(P.var_fwd, P.pack, P.fwd, a, (hipStream_t)stream);
  EGT_HIP_LAUNCH_CHECK("egt_attn_mfma_fwd");
  return EGT_OK;
}

// rowstats is read AND written (slot 3 receives delta); workspace: egt_attn_mfma_workspace_bytes()
extern "C" int egt_attn_mfma_bwd(const egt_attn_desc* desc, const void* qkv, const void* E,
                                 const void* G, const uint8_t* key_mask, const void* attn_mask,
                                 const uint8_t* rand_mask, const void* v_att, void* rowstats,
                                 const void* d_v_att, const void* d_h_ext, void* d_qkv, void* d_E,
                                 void* d_G, void* workspace, void* stream) {
  AttnMfmaArgs a;
  int rc = fill(desc, qkv, E, G, key_mask, attn_mask, rand_mask, workspace, a);
  if (rc) return rc;
  if (!v_att || !rowstats || !d_v_att || !d_qkv) EGT_FAIL(EGT_E_NULL, "v_att/rowstats/d_v_att/d_qkv is NULL");
  if ((desc->flags & EGT_F_EDGE_INPUT) && !d_E) EGT_FAIL(EGT_E_NULL, "edge_input set but d_E is NULL");
  if ((desc->flags & EGT_F_GATE_INPUT) && !d_G) EGT_FAIL(EGT_E_NULL, "gate_input set but d_G is NULL");
  a.v_att_in = (const float*)v_att; a.rowstats = (float*)rowstats;
  a.d_v_att = (const float*)d_v_att; a.d_h_ext = (const float*)d_h_ext;
  a.d_qkv = (float*)d_qkv;
  a.d_E = (desc->flags & EGT_F_EDGE_INPUT) ? (float*)d_E : nullptr;
  a.d_G = (desc->flags & EGT_F_GATE_INPUT) ? (float*)d_G : nullptr;
  const AttnPlan P = plan_attn(desc, &a);
  a.stats2 = a.pk + P.stats2; a.ws_dA = a.pk + P.dA;
  a.pack_what = P.pack_bwd;
  if (P.bf16) egt_attn_bf16_launch_bwd(P.var_bwd, P.pack, P.bwd_kv, P.bwd_q, a, (hipStream_t)stream);
  else attn_launch_bwd<0>(P.var_bwd, P.pack, P.bwd_kv, P.bwd_q, a, (hipStream_t)stream);
  EGT_HIP_LAUNCH_CHECK("egt_attn_mfma_bwd");
  return EGT_OK;
}

// ---- fused pair operator (egt_pair.h): (V_att, e') = pair(QKV, e, mask) and its backward -------------------------------
extern "C" int egt_pair_supported(const egt_block_desc* d) {
  if (!d || d->dtype != EGT_F32 || d->H != AH) return 0;
  if (d->d != 64 || d->De != 32) return 0;                                   // the instantiated geometry (BASELINE config 5)
  if (!(d->flags & EGT_BF_GATE)) return 0;                                    // gated attention with edge bias ('residual' edge channels)
  if (d->flags & (EGT_BF_ATTN_MASK | EGT_BF_NO_EDGE_LN | EGT_BF_SEED_DEVICE | EGT_BF_STATIC_EDGE | EGT_BF_SCALE_DEGREE | EGT_BF_SCALER_LINEAR | EGT_BF_ATTN_DROPOUT)) return 0;
  if (d->B < 1 || d->N < 1 || d->N > 2048) return 0;
  if ((size_t)d->B * d->N * d->N * AH > 0xFFFFFFFFull) return 0;              // 32-bit element index of the mask hash
  return 1;
}

// the attention's workspace plus the pair operator's tail (plan_attn).  The forward writes the q / k / v arrays; with
// desc->reserved & EGT_ATTN_WS_SHARED the caller hands the SAME untouched workspace to egt_pair_bwd, which then adds only dO
extern "C" size_t egt_pair_workspace_bytes(const egt_block_desc* d) {
  return egt_pair_supported(d) ? plan_attn(d).total * sizeof(float) : 0;
}

static int pair_fill(const egt_block_desc* d, const egt_block_params* P, const void* qkv, const void* e, const uint8_t* key_mask,
                     void* workspace, AttnPlan& plan, AttnMfmaArgs& a, PairArgs& pa) {
  if (!egt_pair_supported(d)) EGT_FAIL(EGT_E_SHAPE, "configuration not covered by the fused pair operator (d = 64, De = 32, H = 8, gated, fp32)");
  if (!P || !qkv || !e || !workspace) EGT_FAIL(EGT_E_NULL, "params/qkv/e/workspace is NULL");
  if (!P->norm_edge_gamma || !P->norm_edge_beta || !P->attention_gates_kernel || !P->attention_gates_bias || !P->dense_edge_b_kernel ||
      !P->dense_edge_b_bias || !P->dense_edge_r_kernel || !P->dense_edge_r_bias)
    EGT_FAIL(EGT_E_NULL, "an edge-side parameter pointer is NULL");
  if (d->reserved & ~EGT_ATTN_WS_SHARED) EGT_FAIL(EGT_E_FLAGS, "egt_block_desc.reserved: unknown bits 0x%x", d->reserved);
  plan = plan_attn(d);
  a = AttnMfmaArgs{};
  a.B = d->B; a.N = d->N; a.NP = np_of(d->N); a.d = d->d;
  a.flags = EGT_F_EDGE_INPUT | EGT_F_GATE_INPUT | ((d->flags & EGT_BF_CLIP) ? EGT_F_CLIP : 0);
  a.clip_lo = d->clip_lo; a.clip_hi = d->clip_hi;
  a.scale = 1.0f / sqrtf((float)d->d);
  a.rm_thr = egt_threshold24(d->random_mask_prob);
  a.s0 = (uint32_t)(d->seed & 0xFFFFFFFFull); a.s1 = (uint32_t)(d->seed >> 32);
  a.rng_rm = ((d->flags & EGT_BF_TRAINING) && d->random_mask_prob > 0.0f) ? 1 : 0;
  a.qkv = (const float*)qkv; a.km = key_mask;
  a.pk = (float*)workspace;
  pa = PairArgs{};
  pa.De = d->De; pa.ln_eps = d->ln_eps;
  pa.e = (const float*)e;
  pa.gamma = (const float*)P->norm_edge_gamma; pa.beta = (const float*)P->norm_edge_beta;
  pa.Wg = (const float*)P->attention_gates_kernel; pa.bg = (const float*)P->attention_gates_bias;
  pa.We = (const float*)P->dense_edge_b_kernel; pa.be = (const float*)P->dense_edge_b_bias;
  pa.Wr = (const float*)P->dense_edge_r_kernel; pa.br = (const float*)P->dense_edge_r_bias;
  pa.wprep = a.pk + plan.wprep; pa.dump = a.pk + plan.dump;
  return EGT_OK;
}

extern "C" int egt_pair_fwd(const egt_block_desc* desc, const egt_block_params* params, const void* qkv, const void* e,
                            const uint8_t* key_mask, void* v_att, void* e_out, void* rowstats, void* workspace, void* stream) {
  AttnPlan P; AttnMfmaArgs a; PairArgs pa;
  int rc = pair_fill(desc, params, qkv, e, key_mask, workspace, P, a, pa);
  if (rc) return rc;
  if (!v_att || !e_out || !rowstats) EGT_FAIL(EGT_E_NULL, "v_att/e_out/rowstats is NULL");
  a.v_att = (float*)v_att; a.rowstats = (float*)rowstats;
  pa.e_out = (float*)e_out;
  a.pack_what = P.pack_fwd;
  hipStream_t st = (hipStream_t)stream;
  egt_launch_planned<k_attn_pack<64>>("k_attn_pack", P.pack, st, a);
  EGT_LAUNCH("k_pair_prep", k_pair_prep<32>, dim3(P.prep.grid), dim3(P.prep.block), P.prep.lds, st, pa);
  switch (2 * P.var_fwd + P.full) {   // V, FULL
    case 5: egt_launch_planned<k_pair_fwd<64, 32, 2, true>>("k_pair_fwd", P.pair_fwd, st, a, pa); break;
    case 4: egt_launch_planned<k_pair_fwd<64, 32, 2, false>>("k_pair_fwd", P.pair_fwd, st, a, pa); break;
    case 3: egt_launch_planned<k_pair_fwd<64, 32, 1, true>>("k_pair_fwd", P.pair_fwd, st, a, pa); break;
    default: egt_launch_planned<k_pair_fwd<64, 32, 1, false>>("k_pair_fwd", P.pair_fwd, st, a, pa); break;
  }
  EGT_HIP_LAUNCH_CHECK("egt_pair_fwd");
  return EGT_OK;
}

// rowstats is read AND written (slot 3 receives delta).  Every edge-side pointer of `grads` is written; d_e may alias d_e_out.
extern "C" int egt_pair_bwd(const egt_block_desc* desc, const egt_block_params* params, const void* qkv, const void* e,
                            const uint8_t* key_mask, const void* v_att, void* rowstats, const void* d_v_att, const void* d_e_out,
                            void* d_qkv, void* d_e, const egt_block_params* grads, void* workspace, void* stream) {
  AttnPlan P; AttnMfmaArgs a; PairArgs pa;
  int rc = pair_fill(desc, params, qkv, e, key_mask, workspace, P, a, pa);
  if (rc) return rc;
  if (!v_att || !rowstats || !d_v_att || !d_e_out || !d_qkv || !d_e || !grads) EGT_FAIL(EGT_E_NULL, "v_att/rowstats/d_v_att/d_e_out/d_qkv/d_e/grads is NULL");
  if (!grads->norm_edge_gamma || !grads->norm_edge_beta || !grads->attention_gates_kernel || !grads->attention_gates_bias ||
      !grads->dense_edge_b_kernel || !grads->dense_edge_b_bias || !grads->dense_edge_r_kernel || !grads->dense_edge_r_bias)
    EGT_FAIL(EGT_E_NULL, "an edge-side gradient pointer is NULL");
  a.v_att_in = (const float*)v_att; a.rowstats = (float*)rowstats;
  a.d_v_att = (const float*)d_v_att; a.d_qkv = (float*)d_qkv;
  pa.d_e_out = (const float*)d_e_out; pa.d_e = (float*)d_e;
  a.stats2 = a.pk + P.stats2; a.ws_dA = a.pk + P.dA;
  pa.part_proj = a.pk + P.part_proj; pa.part_upd = a.pk + P.part_upd;
  a.pack_what = P.pack_bwd;
  hipStream_t st = (hipStream_t)stream;
  egt_launch_planned<k_attn_pack<64>>("k_attn_pack", P.pack, st, a);   // (also the per-row constants, delta = sum_k dO*O among them)
  if (!(desc->reserved & EGT_ATTN_WS_SHARED))   // (a shared workspace still holds the forward's table: same parameter values by contract)
    EGT_LAUNCH("k_pair_prep", k_pair_prep<32>, dim3(P.prep.grid), dim3(P.prep.block), P.prep.lds, st, pa);
  switch (2 * P.var_bwd + P.full) {   // V, FULL
    case 5: egt_launch_planned<k_pair_bwd<64, 32, 2, true>>("k_pair_bwd", P.pair_bwd, st, a, pa); break;
    case 4: egt_launch_planned<k_pair_bwd<64, 32, 2, false>>("k_pair_bwd", P.pair_bwd, st, a, pa); break;
    case 3: egt_launch_planned<k_pair_bwd<64, 32, 1, true>>("k_pair_bwd", P.pair_bwd, st, a, pa); break;
    default: egt_launch_planned<k_pair_bwd<64, 32, 1, false>>("k_pair_bwd", P.pair_bwd, st, a, pa); break;
  }
  egt_launch_planned<k_attn_mfma_bwd_q<64>>("k_attn_mfma_bwd_q", P.bwd_q, st, a);
  egt_edge_finish_param_grads(32, pa.gamma, pa.beta, pa.Wg, pa.We, pa.part_proj, pa.part_upd, P.nwg, a.pk + P.red_proj, a.pk + P.red_upd,
                              (float*)grads->norm_edge_gamma, (float*)grads->norm_edge_beta, (float*)grads->attention_gates_kernel,
                              (float*)grads->attention_gates_bias, (float*)grads->dense_edge_b_kernel, (float*)grads->dense_edge_b_bias,
                              (float*)grads->dense_edge_r_kernel, (float*)grads->dense_edge_r_bias, st);
  EGT_HIP_LAUNCH_CHECK("egt_pair_bwd");
  return EGT_OK;
}

#ifdef EGT_STAMPS
static const char* const g_attn_names[] = {"setup", "top: pair loads, out stores, LDS reads", "MFMA 1 + operand reloads", "elementwise", "MFMA 2 + reloads", nullptr, "barrier", "epilogue"};
static const EgtStampKernel g_attn_stamped[ST_COUNT] = {
    {"k_attn_mfma_fwd (compute waves)", g_attn_names, 8},     {"k_attn_mfma_bwd_kv (compute waves)", g_attn_names, 8},
    {"k_pair_fwd (attention waves)", g_pair_fwd_att_names, 8}, {"k_pair_fwd (edge waves)", g_pair_fwd_edge_names, 9},
    {"k_pair_bwd (attention waves)", g_pair_bwd_att_names, 9}, {"k_pair_bwd (edge waves)", g_pair_bwd_edge_names, 10}};
EGT_STAMP_REGISTER(g_attn_stamped);
#endif
