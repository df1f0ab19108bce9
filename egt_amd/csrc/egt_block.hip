// Fused EGT attention block for gfx950 — the data-parallel hot path.
//   (h', e') = edge_update_residual(h, e) around mha_block, pre-norm
//   (lib/models/graph_xformer_model_base.py:192-223 + :106-145, inner op
//    lib/models/egt_layers.py:57-143).
//
// Data flow per 16-pair tile (one query row l, 16 consecutive keys m; the
// [B,N,N,De] edge tensor makes that 16*De*4 contiguous bytes):
//   HBM --coalesced 16B loads--> LDS tile (XOR-swizzled 16B slots)
//   LDS --ds_read_b128--> MFMA B-fragments: lane (p = lane&15, q = lane>>4) owns
//        pair p and channels {16*t + 4*q + r}
//   LayerNorm (norm_edge) in registers (two-pass moments; 2 cross-lane adds)
//   v_mfma_f32_16x16x4_f32 x (De/4):  [Wg|We]^T(16 x De) . ehat^T(De x 16 pairs)
//        -> lane (p,q) receives G,E of pair p for heads 2q,2q+1  (no shuffles)
//   QK^T (d <= 8: 16 FMAs/lane), clip, +E, additive masks, per-lane ONLINE
//   softmax x sigmoid gate, A.V accumulated per lane; merged across the 16 key
//   lanes once per query row.
//   v_mfma x (De/16*2): Wr^T . H_hat^T -> residual update written back into the
//   LDS tile, streamed out with coalesced 16B stores.
// E, G, H_hat, A_tild never touch HBM.  Backward recomputes all of it from e,
// keeps per-(row,head) softmax statistics + V_att from the forward (flash-style
// delta), and does every weight gradient as MFMA contractions over the pair
// axis with deterministic per-workgroup partials.
// The node side of the block (norm_mha, dense_qkv, dense_mha + residual and their backward) is
// row-local, so it rides along: the forward's epilogue finishes h' and already produces the next
// block's packed QKV, the backward's prologue turns the dQ/dK/dV partials of the block above into
// dh and this block's dV_att / delta -- one launch per layer per direction.
//
// Lane roles follow the 16x16x4 f32 MFMA register maps (A: row=lane&15,
// k=lane>>4; B: k=lane>>4, col=lane&15; D: row=4*(lane>>4)+reg, col=lane&15).
#include "egt_common.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "egt_block.h"
#include "egt_tile.h"

#include "egt_block_dev.h"
#include "egt_dma.h"

#include "egt_block_fwd.h"   // k_block_fwd, k_block_fwd_r4, k_block_fwd_s64
#include "egt_block_bwd.h"   // k_block_bwd_v4, k_block_bwd_v5, k_block_bwd_v4r

// ================================================================ host glue ====


// Run-time switches of the fused block, read ONCE per process (the launch path does no getenv()) -- the complete list, see README.md:
//   EGT_NO_NARROW / EGT_NO_NARROW_FWD / EGT_NO_NARROW_BWD: De = 8 falls back from the De = 8 pair kernels (egt_narrow.hip) to the
//     MFMA-tile kernels (tests exercise both);  EGT_BWD_MATMUL=bf16x3: the backward's channel contractions as 3-term bf16 split
//     products (opt-in; default exact fp32);  EGT_BWD_TL / EGT_FWD_ROWS = 4 .. 16: query rows per backward / forward workgroup
//     (tests, sweeps; other values are ignored);  EGT_NRW_FWD_WAVES / EGT_NRW_BWD_WAVES = 4 | 8: waves per De = 8 workgroup, and
//     EGT_NRW_FWD_HALF = 0 | 1: eight-row forward workgroups when that runs eight waves (tests, A/B; other values keep the rule);
//     EGT_NO_STATIC: the headline descriptor takes the generic k_block_fwd instance instead of k_block_fwd_s64 (tests, A/B).
struct EgtBlockEnv {
  bool no_narrow_fwd, no_narrow_bwd, no_static;
  int bwd_mm;
  int bwd_tl, fwd_rows;                            // 0 when unset
  int nrw_fwd_waves, nrw_bwd_waves, nrw_fwd_half;  // 0 when unset; nrw_fwd_half -1
};
static bool env_flag_raw(const char* name) {
  const char* v = getenv(name);
  return v && v[0] && v[0] != '0';
}
static int env_int(const char* name, int unset) {
  const char* v = getenv(name);
  return v ? atoi(v) : unset;
}
static const EgtBlockEnv& block_env() {
  static const EgtBlockEnv e = [] {
    EgtBlockEnv v{};
    v.no_narrow_fwd = env_flag_raw("EGT_NO_NARROW_FWD") || env_flag_raw("EGT_NO_NARROW");
    v.no_narrow_bwd = env_flag_raw("EGT_NO_NARROW_BWD") || env_flag_raw("EGT_NO_NARROW");
    v.no_static = env_flag_raw("EGT_NO_STATIC");
    const char* mm = getenv("EGT_BWD_MATMUL");
    v.bwd_mm = (mm && !strcmp(mm, "bf16x3")) ? EGT_MM_BF16X3 : EGT_MM_F32;
    v.bwd_tl = env_int("EGT_BWD_TL", 0);
    v.fwd_rows = env_int("EGT_FWD_ROWS", 0);
    v.nrw_fwd_waves = env_int("EGT_NRW_FWD_WAVES", 0);
    v.nrw_bwd_waves = env_int("EGT_NRW_BWD_WAVES", 0);
    v.nrw_fwd_half = env_int("EGT_NRW_FWD_HALF", -1);
    return v;
  }();
  return e;
}
// compute units of the current device (dispatch decisions that depend on whether a launch fills the chip)
int egt_device_cus() {
  static const int n = [] {
    int dev = 0, cu = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev);
    return cu > 0 ? cu : 256;
  }();
  return n;
}

// EGT_BF_ATTN_DROPOUT: the rate travels as its fp32 bit pattern in desc->reserved
static float block_drop_rate(const egt_block_desc* d) {
  float r;
  memcpy(&r, &d->reserved, sizeof r);
  return r;
}

static int block_check(const egt_block_desc* d, bool report) {
  if (!d) EGT_BAD(EGT_E_NULL, "desc is NULL");
  if (d->dtype != EGT_F32 && d->dtype != EGT_BF16) EGT_BAD(EGT_E_DTYPE, "dtype must be EGT_F32 or EGT_BF16 (got %d)", d->dtype);
  if (d->B <= 0 || d->N <= 0) EGT_BAD(EGT_E_SHAPE, "B and N must be positive");
  if (d->H != BH) EGT_BAD(EGT_E_SHAPE, "fused block is built for num_heads=8 (got %d)", d->H);
  if (d->d < 1 || d->d > 8) EGT_BAD(EGT_E_SHAPE, "fused block covers per-head dim <= 8 (got %d)", d->d);
  switch (d->De) {
    case 8: case 16: case 32: case 48: case 64: break;
    default: EGT_BAD(EGT_E_SHAPE, "fused block covers edge_width in {8,16,32,48,64} (got %d)", d->De);
  }
  if ((size_t)d->B * d->N * d->N * d->H > 0xFFFFFFFFull) EGT_BAD(EGT_E_SHAPE, "B*N*N*H exceeds the 32-bit RNG counter");
  if ((d->flags & EGT_BF_SEED_DEVICE) && !d->seed_device) EGT_BAD(EGT_E_NULL, "EGT_BF_SEED_DEVICE set but seed_device is NULL");
  if (d->flags & EGT_BF_STATIC_EDGE) {   // the static-edge mode lives in the De = 8 pair kernels (egt_narrow.hip) and nowhere else
    if (!(d->flags & EGT_BF_NO_EDGE_LN)) EGT_BAD(EGT_E_FLAGS, "EGT_BF_STATIC_EDGE is only valid together with EGT_BF_NO_EDGE_LN");
    if (d->flags & EGT_BF_ATTN_MASK) EGT_BAD(EGT_E_FLAGS, "EGT_BF_STATIC_EDGE does not take EGT_BF_ATTN_MASK");
    if (d->De != 8) EGT_BAD(EGT_E_SHAPE, "EGT_BF_STATIC_EDGE covers edge_width 8 (got %d)", d->De);
    if (block_env().no_narrow_fwd || block_env().no_narrow_bwd) EGT_BAD(EGT_E_FLAGS, "EGT_BF_STATIC_EDGE needs the De = 8 pair kernels (EGT_NO_NARROW* is set)");
  }
  if ((d->flags & EGT_BF_SCALER_LINEAR) && !(d->flags & EGT_BF_SCALE_DEGREE))
    EGT_BAD(EGT_E_FLAGS, "EGT_BF_SCALER_LINEAR is only valid together with EGT_BF_SCALE_DEGREE");
  if (d->flags & EGT_BF_SCALE_DEGREE) {   // degree scalers: the SD instances of the MFMA-tile kernels (egt_block_sd.hip)
    if (!(d->flags & EGT_BF_GATE)) EGT_BAD(EGT_E_FLAGS, "EGT_BF_SCALE_DEGREE needs EGT_BF_GATE (scale_degree only works with gate_attention)");
    if (d->flags & EGT_BF_STATIC_EDGE) EGT_BAD(EGT_E_FLAGS, "EGT_BF_SCALE_DEGREE does not take EGT_BF_STATIC_EDGE");
    if (d->dtype == EGT_BF16) EGT_BAD(EGT_E_DTYPE, "EGT_BF_SCALE_DEGREE with bf16 edge tensors is not covered (fp32 edge tensors only)");
  }
  if (d->flags & EGT_BF_ATTN_DROPOUT) {   // attention dropout: the DO instances of the MFMA-tile kernels (egt_block_do.hip)
    if (!(d->flags & EGT_BF_TRAINING)) EGT_BAD(EGT_E_FLAGS, "EGT_BF_ATTN_DROPOUT needs EGT_BF_TRAINING (dropout acts in training only; clear the flag for evaluation)");
    if (d->flags & EGT_BF_SCALE_DEGREE) EGT_BAD(EGT_E_FLAGS, "EGT_BF_ATTN_DROPOUT does not take EGT_BF_SCALE_DEGREE");
    if (d->flags & EGT_BF_STATIC_EDGE) EGT_BAD(EGT_E_FLAGS, "EGT_BF_ATTN_DROPOUT does not take EGT_BF_STATIC_EDGE");
    const float rate = block_drop_rate(d);
    if (!(rate > 0.0f && rate < 1.0f)) EGT_BAD(EGT_E_FLAGS, "EGT_BF_ATTN_DROPOUT needs a rate in (0, 1) in desc->reserved (fp32 bits; got %g)", (double)rate);
  }
  return EGT_OK;
}

extern "C" int egt_block_supported(const egt_block_desc* d) { return block_check(d, false) == EGT_OK; }

static size_t al(size_t x) { return (x + 63) & ~(size_t)63; }  // in floats

// ------------------------------------------------------------------------------------------------------- launch plan ----
// How the fused block runs for one descriptor -- the kernel family and instance of each direction, the launch shapes, the
// buffer layout -- is decided in ONE place, plan_block, once per C-ABI call (the layers of a stack call differ only by seed).
// launch_fwd / launch_bwd (and the De = 8 launchers in egt_narrow.hip) execute the plan; egt_block_bwd_kernel and the
// *_bytes queries read it.  Families:
enum class FwdKernel { narrow, r4, tile };      // k_narrow_fwd {NW, half rows} | k_block_fwd_r4 {NW} | k_block_fwd {KVL, ML, FULL}
enum class BwdKernel { narrow, v4r, v5, v4 };   // k_narrow_bwd {NW} | k_block_bwd_v4r | k_block_bwd_v5 {MM} | k_block_bwd_v4 {ML}
static const char* const g_bwd_kernel_name[] = {"k_narrow_bwd", "k_block_bwd_v4r", "k_block_bwd_v5", "k_block_bwd_v4"};

struct BlockPlan {
  bool dro;    // EGT_BF_ATTN_DROPOUT: the DO instances (egt_block_do.hip) of the MFMA-tile kernels; never the De = 8 VALU kernels
  bool sd;     // EGT_BF_SCALE_DEGREE: the SD instances (egt_block_sd.hip) of the MFMA-tile kernels; never the De = 8 VALU kernels
  bool ml;     // a mask TENSOR is read: the attention mask or a host random-mask buffer (the in-kernel random mask is not one)
  bool full;   // N is a multiple of 16 (else the kernels' ragged forms)
  bool stat;   // the descriptor is the headline one that k_block_fwd_s64 is compiled for (plan_for has the list); EGT_NO_STATIC clears it
  FwdKernel fwd;
  EgtLaunch fl;
  int fwd_nw;      // k_narrow_fwd / k_block_fwd_r4: waves per workgroup
  bool fwd_half;   // k_narrow_fwd: eight-row workgroups
  bool kvl;        // k_block_fwd: the graph's K / V rows stay in LDS
  bool epi_ok;     // the geometry allows the pair kernel's node-side epilogue (else k_node_post finishes h')
  int RGF;         // k_block_fwd: query rows per workgroup (BlockArgs::RGF, set for every forward)
  BwdKernel bwd;
  EgtLaunch bl;    // grid = nwg_bwd
  int bwd_nw;      // k_narrow_bwd: waves per workgroup
  int mm;          // k_block_bwd_v5: EGT_MM_*
  int TL, NLR, nwg_bwd, EP;   // query rows per backward workgroup, row groups per graph, workgroups (= edge-parameter partials), floats per partial
  // buffers, in floats.  saved: pw_sv = LN-folded edge weights, wfrag_sv = fragment-major Wqkv / Wo -- prepared by the forward,
  // reused by the backward.  workspace = [common: dvp dqp[2] dkvp[2]] + per layer [pw epart spart sbo wpart ered dqkv dhbuf]
  // (dqp / dkvp alternate by layer parity: the prologue of layer l-1 reads layer l's partials while
  //  other workgroups of that launch already write their own)
  size_t v_att, stats, qkvp, pw_sv, wfrag_sv, saved_total;
  size_t dvp, dqp, dkvp, dqp_sz, dkvp_sz, common_total;
  size_t pw, epart, spart, sbo, wpart, ered, dqkv, dhbuf, layer_total;
};

template <int DE>
static BlockPlan plan_for(const egt_block_desc* d, bool ml) {
  using GG = Geo<DE>;
  const EgtBlockEnv& E = block_env();
  const int B = d->B, N = d->N, cus = egt_device_cus();
  const int groups = (N + BWD_TL - 1) / BWD_TL;   // 16-row groups per graph
  // degree scalers, attention dropout: MFMA-tile kernels only (De = 8 as under EGT_NO_NARROW)
  const bool dro = (d->flags & EGT_BF_ATTN_DROPOUT) != 0;
  const bool sd = (d->flags & EGT_BF_SCALE_DEGREE) != 0;
  const bool tile_only = sd || dro;
  BlockPlan P{};
  P.ml = ml;
  P.sd = sd;
  P.dro = dro;
  P.full = (N % 16) == 0;

  // Row groups per graph of the MFMA-tile kernels (two workgroups per CU), where the forward and backward row rules start:
  // a launch that leaves slots empty takes more, shorter groups while they still fit one round and keep 8 rows (ZINC-100K, B = 128,
  // N = 37: backward 3 x 13 rows = 384 workgroups on 512 slots -> 4 x 10 rows: k_block_bwd 73.6 -> 64.3 us; 5 x 8 rows = 640
  // workgroups is a second round: 92.9 us) ... and 4 rows when even four-row groups leave every CU at most ONE workgroup (B = 16 per
  // GPU at the headline shapes -- a global batch of 128 over 8 GPUs: 64 sixteen-row workgroups on 512 slots -> 256 four-row ones:
  // 23.8 k -> 30.1 k graphs/s with the forward's same rule; at B = 24 / 32 four rows measure the same as / below eight:
  // profiles/r06_pair_abl2.txt)
  int tg = 2 * cus / B;
  {
    const int cap = B * ((N + 3) / 4) <= cus ? (N + 3) / 4 : (N + 7) / 8;
    if (tg > cap) tg = cap;
  }

  // ---- forward
  // k_block_fwd: 16 query rows per workgroup (four per wave); more groups than that take whole multiples of four rows, so the
  // waves stay balanced (ZINC-100K, B = 128, N = 37: 3 x 16 rows = 384 workgroups -> 4 x 12 rows = 512: the longest wave walks
  // 3 rows instead of 4).  EGT_FWD_ROWS = 4 .. 16 overrides (tests).
  P.RGF = tg > groups ? (((N + tg - 1) / tg + 3) / 4) * 4 : 16;
  if (E.fwd_rows >= 4 && E.fwd_rows <= 16) P.RGF = E.fwd_rows;
  const size_t lds_tiles = (size_t)8 * GG::TILE_FLOATS * 4;
  const size_t lds_kv = ((size_t)N * KV_LD + 16 * QS_LD + N) * 4;
  P.kvl = lds_tiles + lds_kv <= 80 * 1024 - 512;   // two workgroups per CU keep their K/V in LDS
  // narrow edge channels: four rows per iteration (k_block_fwd_r4).  16-row workgroups when K/V + tiles fit
  // twice in a CU, else 32-row workgroups (one per CU) as long as K/V fits at all
  const size_t lds_r4 = (size_t)16 * GG::TILE_FLOATS * 4 + lds_kv;
  const size_t lds_r8 = (size_t)32 * GG::TILE_FLOATS * 4 + ((size_t)N * KV_LD + 32 * QS_LD + N) * 4;
  const bool r4 = lds_r4 <= 80 * 1024 - 512, r8 = !r4 && lds_r8 <= 156 * 1024;
  if (DE == 8 && !ml && !E.no_narrow_fwd && !tile_only) {
    // VALU pair kernel (egt_narrow.hip): lane = (row, head/channel pair), 4 key quarters per workgroup.  At most one 16-row
    // workgroup per CU: eight key ranges (eight waves); ... per two CUs: eight-row workgroups.  A forced wave count wins over the
    // rule; EGT_NRW_FWD_HALF only matters with eight waves.
    const int grid16 = B * groups;
    P.fwd = FwdKernel::narrow;
    P.fwd_nw = E.nrw_fwd_waves == 8 || (E.nrw_fwd_waves != 4 && grid16 <= cus && N >= 64) ? 8 : 4;
    P.fwd_half = P.fwd_nw == 8 && (E.nrw_fwd_half == 1 || (E.nrw_fwd_half != 0 && 2 * grid16 <= cus));
    P.fl = {P.fwd_half ? B * ((N + 7) / 8) : grid16, 64 * P.fwd_nw, egt_narrow_fwd_lds(P.fwd_nw)};
  } else if (DE <= 16 && !ml && (r4 || r8)) {   // (wider channels would not fit the four rows' state in 256 VGPRs: not instantiated)
    P.fwd = FwdKernel::r4;
    P.fwd_nw = r4 ? 4 : 8;
    P.fl = {B * ((N + 4 * P.fwd_nw - 1) / (4 * P.fwd_nw)), 64 * P.fwd_nw, r4 ? lds_r4 : lds_r8};
  } else {
    P.fwd = FwdKernel::tile;
    P.fl = {B * ((N + P.RGF - 1) / P.RGF), 256, lds_tiles + (P.kvl ? lds_kv : 0)};
  }
  P.epi_ok = P.fwd != FwdKernel::tile || P.kvl;
  // the compile-time instance of the headline shape (k_block_fwd_s64): exactly ZINC-500K's descriptor -- N = 64, De = 64, d = 8, fp32,
  // gate + clip + edge LayerNorm, training with the in-kernel random mask, no mask tensor, no scalers / dropout, 16-row groups.  What
  // a descriptor does not say (a key mask is passed, the node epilogue runs) launch_tile_fwd checks on the call.
  P.stat = !E.no_static && DE == 64 && N == 64 && d->d == 8 && d->dtype == EGT_F32 && !ml && d->random_mask_prob > 0.0f &&
           (d->flags & ~EGT_BF_SEED_DEVICE) == (EGT_BF_GATE | EGT_BF_CLIP | EGT_BF_TRAINING) &&
           P.fwd == FwdKernel::tile && P.kvl && P.RGF == 16;

  // ---- backward
  // Query rows per backward workgroup (<= 16: the MFMA tiles of the node-side prologue):
  //  * equal groups: N = 150 is ten groups of 15 rather than nine of 16 and one of 6 -- same workgroup count, no short group
  //    (config 3: 225 -> 216 us per launch; N = 120: 162 -> 156 us);
  //  * MFMA-tile kernels: the row groups above, at least `groups` of them (16 rows whenever N is a multiple of 16 and the launch
  //    fills the slots).  (N = 6 / 9 at small B come out at 3 rows.)
  //  * De = 8: a launch of at most one 16-row workgroup per CU (BASELINE config 4 as specified: B = 16, N = 120 -> 128 workgroups
  //    on 256 CUs) takes 8 rows per workgroup: twice the partial slots, each prologue on a half-filled tile, every CU busy
  //    (pattern500k_n120, per launch: B = 16: 59.0 us at 16 rows, 43.3 at 8, 47.9 at 6; B = 32: 63.0 / 59.5 / 65.5) -- round 6, with
  //    the eight-wave k_narrow_bwd for such launches: the shortest groups of >= 8 rows that keep the launch at ONE workgroup per CU
  //    (N = 120: B = 16 -> 8 rows (240 workgroups), B = 24 -> 12 rows: 51.5 -> 42.5 us, B = 32 -> 15 rows: 54.0 -> 48.4 us against
  //    8 rows; N = 188: B = 16 -> 12 rows (256; with 8 rows the launch was 368 four-wave workgroups: 71.4 us against 58.4,
  //    `pattern500k_n188` 9.4 k -> 10.9 k graphs/s)).  Smaller groups never pay beyond that: the per-workgroup work that does not
  //    shrink with the rows (prologue, K / V tiles, partial sums) takes over (B = 128, N = 150: 225 us at 16 rows, 253 at 12, 295 at 8).
  // EGT_BWD_TL = 4 .. 16 overrides, for every De (tests, sweeps: tools/dbg/nrw_tlsweep.sh).
  if (E.bwd_tl >= 4 && E.bwd_tl <= BWD_TL) P.TL = E.bwd_tl;
  else if (DE != 8) {
    const int g = tg > groups ? tg : groups;
    P.TL = (N + g - 1) / g;
  } else if (B * groups <= cus) {
    P.TL = BWD_TL;
    if (N > 8)
      for (int tl = 8; tl < BWD_TL; ++tl)
        if (B * ((N + tl - 1) / tl) <= cus) { P.TL = tl; break; }
  } else P.TL = (N + groups - 1) / groups;
  P.NLR = (N + P.TL - 1) / P.TL;
  P.nwg_bwd = B * P.NLR;
  P.EP = GG::EP;
  if (DE == 8 && !ml && !E.no_narrow_bwd && !tile_only) {
    // De = 8 pair kernel (egt_narrow.hip: k_narrow_bwd, three workgroups per CU), ragged N included.  Measured at config 3
    // against v4r / the round-2 quad-lane kernel (two waves per SIMD both): bf16 edge tensors 226 vs 314 us, fp32 243 vs 320 us.
    // At most one workgroup per CU: eight waves share its key tiles (a forced wave count wins).
    P.bwd = BwdKernel::narrow;
    P.bwd_nw = E.nrw_bwd_waves == 8 || (E.nrw_bwd_waves != 4 && P.nwg_bwd <= cus && N >= 64) ? 8 : 4;
    P.bl = {P.nwg_bwd, 64 * P.bwd_nw, egt_narrow_bwd_lds(P.bwd_nw)};
  } else if (DE <= 16 && !ml) {   // narrow edge channels: V4R_RR rows per iteration, ragged N included
    constexpr int PWR = V4R_RR * (2 * GG::TILE_FLOATS + 256 + 192);
    P.bwd = BwdKernel::v4r;
    P.bl = {P.nwg_bwd, 256,
            ((size_t)(4 * PWR > BWD_PRO_WS ? 4 * PWR : BWD_PRO_WS) + (size_t)BWD_TL * QD_LD + 3 * GG::TILES * 256 + 3 * 2048 + 4) * 4};
  } else if (DE >= 32 && !ml && d->dtype != EGT_BF16) {   // LDS-DMA staged e tiles, ragged N included
    P.bwd = BwdKernel::v5;
    P.mm = E.bwd_mm;
    P.bl = {P.nwg_bwd, 256, ((size_t)V5_AREA(DE) + (size_t)BWD_TL * QD_LD + 3 * ((GG::TILES + 1) / 2) * 512 + 4) * 4};   // (+ 4: the parked-partial flags)
  } else {
    constexpr int PW = 3 * GG::TILE_FLOATS + 256 + 192;
    P.bwd = BwdKernel::v4;
    P.bl = {P.nwg_bwd, 256,   // slabs padded to whole 32-channel steps (bf16 operands)
            ((size_t)(4 * PW > BWD_PRO_WS ? 4 * PW : BWD_PRO_WS) + (size_t)BWD_TL * QD_LD + 3 * ((GG::TILES + 1) / 2) * 512) * 4};
  }

  // ---- buffers
  const size_t rows = (size_t)B * N;
  const int Dh = d->d * d->H;
  size_t o = 0;
  P.v_att = o; o += al(rows * Dh);
  P.stats = o; o += al(rows * BH * 4);
  P.qkvp = o; o += al(rows * QKVP);
  P.pw_sv = o; o += al((size_t)GG::DEP * 16 + 16);
  P.wfrag_sv = o; o += al(Dh <= 64 ? WFRAG_FLOATS : 0);
  P.saved_total = o;
  o = 0;
  P.dvp = o; o += al(rows * 64);
  P.dqp_sz = al(rows * 64 * (size_t)groups);
  P.dkvp_sz = al((size_t)P.nwg_bwd * N * 128);
  P.dqp = o; o += 2 * P.dqp_sz;
  P.dkvp = o; o += 2 * P.dkvp_sz;
  P.common_total = o;
  o = 0;
  P.pw = o; o += al((size_t)GG::DEP * 16 + 16);
  P.epart = o; o += al((size_t)P.nwg_bwd * P.EP);
  {
    const int node_wg = B * ((N + NODE_RC - 1) / NODE_RC);
    const size_t nmax = (size_t)(P.nwg_bwd > node_wg ? P.nwg_bwd : node_wg);
    P.spart = o; o += al(nmax * (5 * Dh));
    P.sbo = o; o += al(nmax * Dh);
  }
  P.wpart = o; o += al((size_t)egt_node_wgrad_chunks((int)rows, 1) * (Dh * 3 * Dh + Dh * Dh));
  P.ered = o; o += al(P.EP);
  P.dqkv = o; o += al(rows * 3 * Dh);
  P.dhbuf = o; o += al(rows * Dh);
  P.layer_total = o;
  return P;
}

#define DISPATCH_BDE(De, CALL)                        \
  switch (De) {                                       \
    case 8: { constexpr int DE = 8; CALL; } break;    \
    case 16: { constexpr int DE = 16; CALL; } break;  \
    case 32: { constexpr int DE = 32; CALL; } break;  \
    case 48: { constexpr int DE = 48; CALL; } break;  \
    default: { constexpr int DE = 64; CALL; } break;  \
  }

static BlockPlan plan_block(const egt_block_desc* d, bool ml) {
  DISPATCH_BDE(d->De, return plan_for<DE>(d, ml));
}

// the call passes a host random-mask buffer the kernels read (else they draw the random mask themselves)
static bool host_rand_mask(const egt_block_desc* d, const uint8_t* rm) {
  return rm && (d->flags & EGT_BF_TRAINING) && d->random_mask_prob > 0.0f;
}
static bool mask_tensor(const egt_block_desc* d, const uint8_t* rm) {
  return (d->flags & EGT_BF_ATTN_MASK) || host_rand_mask(d, rm);
}

// workspace pointers of one layer: `wc` = common region, `wl` = that layer's region
static void bind_ws(const BlockPlan& P, BlockArgs& a, float* wc, float* wl, int parity = 0) {
  a.dvp = wc + P.dvp; a.dqp = wc + P.dqp + parity * P.dqp_sz; a.dkvp = wc + P.dkvp + parity * P.dkvp_sz;
  a.epart = wl + P.epart; a.spart = wl + P.spart; a.sbo = wl + P.sbo; a.wpart = wl + P.wpart;
  a.spart_n = a.sbo_n = a.B * ((a.N + NODE_RC - 1) / NODE_RC);   // k_node_bwd's workgroups (prologue path overrides)
  a.ered = wl + P.ered; a.dqkv_sv = wl + P.dqkv;
  a.TL = P.TL; a.NLR = P.NLR; a.NQP = 1;
  a.xcd = 1;
}

// Which backward pair kernel launch_bwd takes for `d` when no mask TENSOR is passed (the in-kernel random mask is not one) and
// the node side is fused: the families of DESIGN.md section 4 by name.  For tests and bench lines; NULL when `d` is not covered.
extern "C" const char* egt_block_bwd_kernel(const egt_block_desc* d) {
  if (block_check(d, false)) return nullptr;
  return g_bwd_kernel_name[(int)plan_block(d, mask_tensor(d, nullptr)).bwd];
}

// The launch forms plan_block chose for `d` (no mask tensor), as text: "fwd=<family>/<waves>w[/half] bwd=<family>/<waves>w/tl<rows>".
// For tests and bench lines that must not assume which form a batch reaches.  Thread-local string; NULL when `d` is not covered.
extern "C" const char* egt_block_launch_form(const egt_block_desc* d) {
  if (block_check(d, false)) return nullptr;
  const BlockPlan P = plan_block(d, mask_tensor(d, nullptr));
  static const char* const fwd_name[] = {"k_narrow_fwd", "k_block_fwd_r4", "k_block_fwd"};
  static thread_local char buf[128];
  snprintf(buf, sizeof buf, "fwd=%s/%dw%s bwd=%s/%dw/tl%d", fwd_name[(int)P.fwd], P.fwd == FwdKernel::tile ? 4 : P.fwd_nw,
           P.fwd_half ? "/half" : "", g_bwd_kernel_name[(int)P.bwd], P.bwd == BwdKernel::narrow ? P.bwd_nw : 4, P.TL);
  return buf;
}

// every pointer of a parameter / gradient table (the gate's two, #2 and #3, only when the block is gated)
// (EGT_BF_STATIC_EDGE: norm_edge, #0 and #1, and dense_edge_r, #12 and #13, are neither read nor written)
static int check_table(const egt_block_params* t, uint32_t flags, const char* what, int layer = -1) {
  const void* const* tp = reinterpret_cast<const void* const*>(t);
  for (int i = 0; i < 14; ++i) {
    if (tp[i] || (!(flags & EGT_BF_GATE) && (i == 2 || i == 3))) continue;
    if ((flags & EGT_BF_STATIC_EDGE) && (i < 2 || i >= 12)) continue;
    if (layer < 0) EGT_FAIL(EGT_E_NULL, "%s #%d is NULL", what, i);
    EGT_FAIL(EGT_E_NULL, "layer %d %s #%d is NULL", layer, what, i);
  }
  return EGT_OK;
}

// descriptor and parameters of one layer (checked by check_call / bind_chain)
static void fill_block(const egt_block_desc* d, const egt_block_params* p, BlockArgs& a) {
  a = BlockArgs{};
  a.B = d->B; a.N = d->N; a.De = d->De; a.DK = d->d; a.Dh = d->d * d->H;
  a.flags = d->flags;
  a.bf16 = d->dtype == EGT_BF16;
  a.clip_lo = d->clip_lo; a.clip_hi = d->clip_hi;
  a.scale = 1.0f / sqrtf((float)d->d);
  a.ln_eps = d->ln_eps;
  a.rm_thr = egt_threshold24(d->random_mask_prob);
  if (d->flags & EGT_BF_ATTN_DROPOUT) {   // (block_check: training, rate in (0, 1)); as fill_args of egt_attn.hip
    const float rate = block_drop_rate(d);
    a.dk_thr = egt_threshold24(rate);
    a.dk_scale = 1.0f / (1.0f - rate);
  }
  a.s0 = (uint32_t)(d->seed & 0xFFFFFFFFull);
  a.s1 = (uint32_t)(d->seed >> 32);
  a.sd = (d->flags & EGT_BF_SEED_DEVICE) ? (const uint32_t*)d->seed_device : nullptr;
  a.ne_g = (const float*)p->norm_edge_gamma; a.ne_b = (const float*)p->norm_edge_beta;
  a.Wg = (const float*)p->attention_gates_kernel; a.bg = (const float*)p->attention_gates_bias;
  a.We = (const float*)p->dense_edge_b_kernel; a.be = (const float*)p->dense_edge_b_bias;
  a.nm_g = (const float*)p->norm_mha_gamma; a.nm_b = (const float*)p->norm_mha_beta;
  a.Wqkv = (const float*)p->dense_qkv_kernel; a.bqkv = (const float*)p->dense_qkv_bias;
  a.Wo = (const float*)p->dense_mha_kernel; a.bo = (const float*)p->dense_mha_bias;
  a.Wr = (const float*)p->dense_edge_r_kernel; a.br = (const float*)p->dense_edge_r_bias;
  if (d->flags & EGT_BF_STATIC_EDGE) a.ne_g = a.ne_b = a.Wr = a.br = nullptr;   // never read: whatever the caller left there
}

static void bind_grads(BlockArgs& a, const egt_block_params* g) {
  a.g_ne_g = (float*)g->norm_edge_gamma; a.g_ne_b = (float*)g->norm_edge_beta;
  a.g_Wg = (float*)g->attention_gates_kernel; a.g_bg = (float*)g->attention_gates_bias;
  a.g_We = (float*)g->dense_edge_b_kernel; a.g_be = (float*)g->dense_edge_b_bias;
  a.g_nm_g = (float*)g->norm_mha_gamma; a.g_nm_b = (float*)g->norm_mha_beta;
  a.g_Wqkv = (float*)g->dense_qkv_kernel; a.g_bqkv = (float*)g->dense_qkv_bias;
  a.g_Wo = (float*)g->dense_mha_kernel; a.g_bo = (float*)g->dense_mha_bias;
  a.g_Wr = (float*)g->dense_edge_r_kernel; a.g_br = (float*)g->dense_edge_r_bias;
  if (a.flags & EGT_BF_STATIC_EDGE) a.g_ne_g = a.g_ne_b = a.g_Wr = a.g_br = nullptr;   // never written
}

// what the layers of a call share: its masks and its random-mask source (bind_layer binds a layer's own regions)
static void bind_common(const egt_block_desc* d, BlockArgs& a, const uint8_t* km, const void* M, const uint8_t* rm) {
  a.km = km;
  a.M = (d->flags & EGT_BF_ATTN_MASK) ? (const float*)M : nullptr;
  a.rm = nullptr; a.rng_rm = 0;
  if ((d->flags & EGT_BF_TRAINING) && d->random_mask_prob > 0.0f) {
    if (rm) a.rm = rm; else a.rng_rm = 1;
  }
  a.prep = 1;
}

// The node side inside the pair kernels (fwd_node_epilogue / bwd_node_prologue): H = 8 heads of DK <= 8 channels, i.e. node width
// Dh = 8 DK <= 64 as a zero-padded 64-wide row.  (Wo / Wqkv reach those kernels through the fragment-major copies the preparation
// writes with scalar loads -- WFRAG_*, egt_block.h -- so parameter views that are not 16-byte aligned are covered as well.)
static bool node_fused_ok(const BlockArgs& a) {
  return a.Dh == BH * a.DK && a.DK >= 1 && a.DK <= 8 && a.wfrag != nullptr;
}

// The kernel instances of the planned launches: the run-time choices of the plan as template arguments.
template <int DE, bool BF>
static void launch_r4(BlockArgs& a, const BlockPlan& P, hipStream_t st) {
  if (P.fwd_nw == 4) {
    if (P.full) egt_launch_planned<k_block_fwd_r4<DE, true, 4, BF>>("k_block_fwd", P.fl, st, a);
    else egt_launch_planned<k_block_fwd_r4<DE, false, 4, BF>>("k_block_fwd", P.fl, st, a);
  } else {
    if (P.full) egt_launch_planned<k_block_fwd_r4<DE, true, 8, BF>>("k_block_fwd", P.fl, st, a);
    else egt_launch_planned<k_block_fwd_r4<DE, false, 8, BF>>("k_block_fwd", P.fl, st, a);
  }
}
template <int DE, bool BF>   // k_block_fwd<DE, KVL, ML, FULL, BF>: five forms, FULL only for the headline one (K/V in LDS, no mask tensor)
static void launch_tile_fwd(BlockArgs& a, const BlockPlan& P, hipStream_t st) {
  if constexpr (DE == 64 && !BF) {
    if (P.stat && a.km && a.rng_rm && a.epi) {   // the headline descriptor, called the headline way: the compile-time instance
      egt_launch_planned<k_block_fwd_s64<DE>>("k_block_fwd", P.fl, st, a);
      return;
    }
  }
  if (!P.kvl) {
    if (P.ml) egt_launch_planned<k_block_fwd<DE, false, true, false, BF>>("k_block_fwd", P.fl, st, a);
    else egt_launch_planned<k_block_fwd<DE, false, false, false, BF>>("k_block_fwd", P.fl, st, a);
  } else if (P.ml) egt_launch_planned<k_block_fwd<DE, true, true, false, BF>>("k_block_fwd", P.fl, st, a);
  else if (P.full) egt_launch_planned<k_block_fwd<DE, true, false, true, BF>>("k_block_fwd", P.fl, st, a);
  else egt_launch_planned<k_block_fwd<DE, true, false, false, BF>>("k_block_fwd", P.fl, st, a);
}
template <int DE>
static void launch_v5(BlockArgs& a, const BlockPlan& P, hipStream_t st) {
  if (P.mm == EGT_MM_BF16X3) {
    if (P.full) egt_launch_planned<k_block_bwd_v5<DE, EGT_MM_BF16X3, false>>("k_block_bwd", P.bl, st, a);
    else egt_launch_planned<k_block_bwd_v5<DE, EGT_MM_BF16X3, true>>("k_block_bwd", P.bl, st, a);
  } else {
    if (P.full) egt_launch_planned<k_block_bwd_v5<DE, EGT_MM_F32, false>>("k_block_bwd", P.bl, st, a);
    else egt_launch_planned<k_block_bwd_v5<DE, EGT_MM_F32, true>>("k_block_bwd", P.bl, st, a);
  }
}
template <int DE, bool BF>
static void launch_v4(BlockArgs& a, const BlockPlan& P, hipStream_t st) {
  if (P.ml) {
    if (P.full) egt_launch_planned<k_block_bwd_v4<DE, true, BF, false>>("k_block_bwd", P.bl, st, a);
    else egt_launch_planned<k_block_bwd_v4<DE, true, BF, true>>("k_block_bwd", P.bl, st, a);
  } else {
    if (P.full) egt_launch_planned<k_block_bwd_v4<DE, false, BF, false>>("k_block_bwd", P.bl, st, a);
    else egt_launch_planned<k_block_bwd_v4<DE, false, BF, true>>("k_block_bwd", P.bl, st, a);
  }
}

// Forward of one block.  `skip_pre`: qkvp (and pw) of this block were already produced (by the
// previous block's epilogue / k_edge_prep).  a.epi is the epilogue the caller would like; the
// value actually used is returned (0 when the geometry is outside the epilogue's cover, in
// which case k_node_post runs and the next block needs its own k_node_pre).
template <int DE>
static int launch_fwd(BlockArgs& a, const BlockPlan& P, hipStream_t st, bool skip_pre) {
  if (!skip_pre) egt_node_launch_pre(a, st);   // norm_mha + dense_qkv (packed) [+ edge-weight prep]
  if (!(P.epi_ok && node_fused_ok(a))) a.epi = 0;
  a.guard = 0;   // (the always-taken phase branches of the kernels only shape hipcc's scheduling regions)
  a.RGF = P.RGF;
  if (P.sd) egt_block_sd_launch_fwd(a, P.fwd == FwdKernel::r4 ? P.fwd_nw : 0, P.kvl, P.ml, P.full, P.fl, st);
  else if (P.dro) egt_block_do_launch_fwd(a, P.fwd == FwdKernel::r4 ? P.fwd_nw : 0, P.kvl, P.ml, P.full, P.fl, st);
  else switch (P.fwd) {
    case FwdKernel::narrow: egt_narrow_launch_fwd(a, P.fwd_nw, P.fwd_half, P.fl, st); break;
    case FwdKernel::r4:
      if constexpr (DE <= 16) { if (a.bf16) launch_r4<DE, true>(a, P, st); else launch_r4<DE, false>(a, P, st); }
      break;
    case FwdKernel::tile: if (a.bf16) launch_tile_fwd<DE, true>(a, P, st); else launch_tile_fwd<DE, false>(a, P, st); break;
  }
  if (a.epi == 0) egt_node_launch_post(a, st);  // dense_mha + res_mha
  return a.epi;
}

// Backward of one block.  `top`: first block of the chain (its dV_att / delta come from an own
// launch); otherwise they were produced by the node kernel of the block above.  `below`: the
// next block of the chain (NULL at the bottom), whose dV_att / delta this block's node kernel
// produces.  GEMM-shaped weight gradients and all partial reductions are left to the caller
// (the pair kernel writes P.nwg_bwd edge-parameter partials into a.epart).
template <int DE>
static void launch_bwd(BlockArgs& a, const BlockPlan& P, hipStream_t st, bool top, BlockArgs* below, BlockArgs* above, bool fuse) {
  static_assert(DE % 16 == 0 || DE == 8, "edge widths of the pair kernels");
  // node-side prologue inside the pair kernel (see bwd_node_prologue)
  const bool pro = fuse;   // node_fused_ok() of EVERY block of the chain (every backward kernel and the prologue take N that is not a multiple of 16)
  a.pro = 0;
  if (pro) {
    a.pro = top ? 1 : 2;
    a.sbo_n = P.nwg_bwd;
    if (!top) {
      a.up_h = above->h; a.up_nm_g = above->nm_g; a.up_Wqkv = above->Wqkv; a.up_wfrag = above->wfrag; a.up_dh_out = above->dh_out;
      a.up_dqp = above->dqp; a.up_dkvp = above->dkvp; a.up_dqkv_sv = above->dqkv_sv; a.up_spart = above->spart;
      above->spart_n = P.nwg_bwd;
    }
    if (a.prep) egt_node_launch_prep(&a, 1, st);   // single-block call: the LN-folded edge weights of this layer
  } else if (top) {
    egt_node_launch_bwd(a, &a, false, st);  // dV_att (packed), delta, dbo sums [+ edge-weight prep]
  }
  a.NQP = (a.N + 15) / 16;
  a.guard = 0;   // (the always-taken phase branches of the kernels only shape hipcc's scheduling regions)
  if (P.sd)
    egt_block_sd_launch_bwd(a, P.bwd == BwdKernel::v4r ? EGT_SD_BWD_V4R : P.bwd == BwdKernel::v5 ? EGT_SD_BWD_V5 : EGT_SD_BWD_V4, P.mm, P.ml, P.full, P.bl, st);
  else if (P.dro)
    egt_block_do_launch_bwd(a, P.bwd == BwdKernel::v4r ? EGT_SD_BWD_V4R : P.bwd == BwdKernel::v5 ? EGT_SD_BWD_V5 : EGT_SD_BWD_V4, P.mm, P.ml, P.full, P.bl, st);
  else switch (P.bwd) {
    case BwdKernel::narrow: egt_narrow_launch_bwd(a, P.bwd_nw, P.bl, st); break;
    case BwdKernel::v4r:
      if constexpr (DE <= 16) {
        if (a.bf16) egt_launch_planned<k_block_bwd_v4r<DE, true, V4R_RR>>("k_block_bwd", P.bl, st, a);
        else egt_launch_planned<k_block_bwd_v4r<DE, false, V4R_RR>>("k_block_bwd", P.bl, st, a);
      }
      break;
    case BwdKernel::v5:
      if constexpr (DE >= 32) launch_v5<DE>(a, P, st);
      break;
    case BwdKernel::v4: if (a.bf16) launch_v4<DE, true>(a, P, st); else launch_v4<DE, false>(a, P, st); break;
  }
  if (!pro) egt_node_launch_bwd(a, below, true, st);   // dQKV -> dh, bias/LN sums; dV_att + delta of the block below
  else if (!below) egt_node_launch_bwd(a, nullptr, true, st);   // bottom of the chain: only dQKV -> dh is left
}

// ===================================================== one call: block or layer stack =====
// A call runs a chain of `layers` blocks.  egt_stack_* chains model_height of them; egt_block_* is the one-layer chain of the
// same layout (stack_layout puts `blk` at offset 0 then) with the caller's seed as it is and, optionally, a host random mask.
// The argument checks (check_call) and the binding of the chain (bind_chain) are shared; an entry point keeps its outputs /
// incoming gradients and its launch sequence.
static uint64_t layer_seed(uint64_t seed, int l) { return seed ^ (0x9E3779B97F4A7C15ull * (uint64_t)(l + 1)); }

struct StackLayout {
  size_t h_act, e_act, blk, saved_total;      // floats
  size_t ws_total;
  size_t h_sz, e_sz;
};

// egt_stack_* keeps a layer's e' as the next layer's input: the static-edge mode is a per-block one (egt_block_fwd / _bwd)
static int stack_flags_check(const egt_block_desc* d, bool report) {
  if (d && (d->flags & EGT_BF_STATIC_EDGE)) {
    if (report) egt_set_error("egt_stack_* does not take EGT_BF_STATIC_EDGE (use egt_block_fwd / egt_block_bwd per layer)");
    return EGT_E_FLAGS;
  }
  if (d && (d->flags & (EGT_BF_SCALE_DEGREE | EGT_BF_SCALER_LINEAR))) {   // the chained epilogue / prologue of a stack carry no degree
    if (report) egt_set_error("egt_stack_* does not take EGT_BF_SCALE_DEGREE (use egt_block_fwd / egt_block_bwd per layer)");
    return EGT_E_FLAGS;
  }
  if (d && (d->flags & EGT_BF_ATTN_DROPOUT)) {   // a stack call has one seed per layer for the random mask only
    if (report) egt_set_error("egt_stack_* does not take EGT_BF_ATTN_DROPOUT (use egt_block_fwd / egt_block_bwd per layer)");
    return EGT_E_FLAGS;
  }
  return EGT_OK;
}

static StackLayout stack_layout(const egt_block_desc* d, const BlockPlan& P, int layers) {
  StackLayout S{};
  S.h_sz = al((size_t)d->B * d->N * d->d * d->H);
  S.e_sz = al((size_t)d->B * d->N * d->N * d->De / (d->dtype == EGT_BF16 ? 2 : 1));   // in floats
  size_t o = 0;
  S.h_act = o; o += S.h_sz * (size_t)(layers > 1 ? layers - 1 : 0);
  S.e_act = o; o += S.e_sz * (size_t)(layers > 1 ? layers - 1 : 0);
  S.blk = o; o += P.saved_total * (size_t)layers;
  S.saved_total = o;
  S.ws_total = P.common_total + P.layer_total * (size_t)layers;
  return S;
}

// 1 when plan_block gives `d` (no mask tensor) the compile-time instance of the headline shape, k_block_fwd_s64 -- which a call then
// runs if it passes a key mask and the geometry takes the node epilogue; else 0 (EGT_NO_STATIC, any other descriptor, NULL or not
// covered).  For tests and bench lines that must know which form ran.
extern "C" int egt_block_plan_static(const egt_block_desc* d) {
  if (block_check(d, false)) return 0;
  return plan_block(d, mask_tensor(d, nullptr)).stat ? 1 : 0;
}

// saved / workspace bytes of a chain of `layers` blocks (0: not covered)
static size_t chain_bytes(const egt_block_desc* d, int layers, bool stack, bool ws) {
  if ((stack && stack_flags_check(d, false)) || block_check(d, false) || layers < 1) return 0;
  const StackLayout S = stack_layout(d, plan_block(d, mask_tensor(d, nullptr)), layers);
  return (ws ? S.ws_total : S.saved_total) * sizeof(float);
}
extern "C" size_t egt_block_saved_bytes(const egt_block_desc* d) { return chain_bytes(d, 1, false, false); }
extern "C" size_t egt_block_workspace_bytes(const egt_block_desc* d) { return chain_bytes(d, 1, false, true); }
extern "C" size_t egt_stack_saved_bytes(const egt_block_desc* d, int32_t layers) { return chain_bytes(d, layers, true, false); }
extern "C" size_t egt_stack_workspace_bytes(const egt_block_desc* d, int32_t layers) { return chain_bytes(d, layers, true, true); }

// The launch plane of egt_stack_bwd's tail for `d` and `layers` (no mask tensor), as text:
// "wgrad=<rows per workgroup>r/<chunks>c partials=<edge-parameter partials> reduce=<k_sum_segments launches>
//  epg=<k_edge_param_grads launches> prep=<stack16|stack40|edge_prep>", e.g. "wgrad=160r/27c partials=384 reduce=2 epg=1 prep=stack16".
// Every figure comes from the function the launch itself calls.  Thread-local string; NULL when the call is not covered.
extern "C" const char* egt_stack_tail_form(const egt_block_desc* d, int32_t layers) {
  if (stack_flags_check(d, false) || block_check(d, false) || layers < 1 || layers > 64) return nullptr;
  const BlockPlan P = plan_block(d, mask_tensor(d, nullptr));
  const int rows = d->B * d->N, slots = egt_node_pre_stack_slots(layers);
  static thread_local char buf[128];
  snprintf(buf, sizeof buf, "wgrad=%dr/%dc partials=%d reduce=%d epg=%d prep=%s", egt_node_wgrad_rows(rows, layers),
           egt_node_wgrad_chunks(rows, layers), P.nwg_bwd, egt_node_reduce_launches(layers), egt_node_edge_grad_launches(layers),
           slots == 16 ? "stack16" : slots == 40 ? "stack40" : "edge_prep");
  return buf;
}

// the saved / workspace regions of layer l
static void bind_layer(const StackLayout& S, const BlockPlan& P, int l, BlockArgs& a, float* saved, float* ws) {
  float* bs = saved + S.blk + P.saved_total * (size_t)l;
  a.v_att = bs + P.v_att; a.stats = bs + P.stats; a.qkvp = bs + P.qkvp;
  // per-layer workspace: block l's epilogue must not race block l+1's prepared weights, and the
  // deferred reductions / weight gradients need every layer's partials and dQKV rows at the end
  bind_ws(P, a, ws, ws + P.common_total + P.layer_total * (size_t)l, l & 1);
  a.pw = bs + P.pw_sv;
  a.wfrag = a.Dh <= 64 ? bs + P.wfrag_sv : nullptr;
}

// what the four entry points hand to check_call and bind_chain
struct ChainCall {
  const egt_block_desc* d;
  int layers;
  bool stack, bwd;
  const egt_block_params *params, *grads;   // grads: backward only
  const void *h, *e;
  const uint8_t* km;
  const void* M;
  const uint8_t* rm;                        // host random mask: block calls only
  float *saved, *ws;
};

// The argument checks of a call, in the order the entry points have always answered in.  `ptrs_ok`: none of the tensors the
// entry point needs (`names`) is NULL; `alias`: d_h is d_h_out.  The parameter / gradient tables of a stack call are checked
// layer by layer in bind_chain.
static int check_call(const ChainCall& c, bool ptrs_ok, const char* names, bool alias) {
  const egt_block_desc* d = c.d;
  int rc;
  if (c.stack) {   // flags and layer count before the pointers: a descriptor-only answer
    if ((rc = stack_flags_check(d, true))) return rc;
    if (c.layers < 1) EGT_FAIL(EGT_E_SHAPE, "layers must be >= 1");
    if (c.bwd && c.layers > 64) EGT_FAIL(EGT_E_SHAPE, "at most 64 layers per stack call");
    if (!ptrs_ok) EGT_FAIL(EGT_E_NULL, "params/%s is NULL", names);
    if ((rc = block_check(d, true))) return rc;
  } else {
    if ((rc = block_check(d, true))) return rc;
    if (!c.params) EGT_FAIL(EGT_E_NULL, "params is NULL");
    if ((rc = check_table(c.params, d->flags, "block parameter"))) return rc;
    if (!ptrs_ok) EGT_FAIL(EGT_E_NULL, "%s is NULL", names);
  }
  if ((d->flags & EGT_BF_ATTN_MASK) && !c.M) EGT_FAIL(EGT_E_NULL, "ATTN_MASK set but attn_mask is NULL");
  if ((d->flags & EGT_BF_STATIC_EDGE) && host_rand_mask(d, c.rm))
    EGT_FAIL(EGT_E_FLAGS, "EGT_BF_STATIC_EDGE takes the in-kernel random mask only (rand_mask must be NULL)");
  if (c.layers > 64) EGT_FAIL(EGT_E_SHAPE, "at most 64 layers per stack call");   // (the forward's place for it)
  // every layer's dh' is read again after dh was written (deferred dWo contraction): no in-place dh
  if (alias) EGT_FAIL(EGT_E_FLAGS, "d_h must not alias d_h_out (d_e may alias d_e_out)");
  return EGT_OK;
}

// Layers 0 .. layers-1 of a call bound into as[]: seed, parameters, input / activation addresses, masks, saved and workspace
// regions, gradient tables.  A NULL table slot is reported for the layer the direction reaches first.
static int bind_chain(const ChainCall& c, const BlockPlan& P, BlockArgs* as) {
  const StackLayout S = stack_layout(c.d, P, c.layers);
  for (int i = 0; i < c.layers; ++i) {
    const int l = c.bwd ? c.layers - 1 - i : i;
    int rc = c.stack ? check_table(c.params + l, c.d->flags, "block parameter") : EGT_OK;   // (a block call's: check_call)
    if (!rc && c.bwd) rc = check_table(c.grads + l, c.d->flags, "gradient pointer", c.stack ? l : -1);
    if (rc) return rc;
    egt_block_desc dl = *c.d;
    if (c.stack) dl.seed = layer_seed(c.d->seed, l);
    BlockArgs& a = as[l];
    fill_block(&dl, c.params + l, a);
    a.h = l == 0 ? (const float*)c.h : c.saved + S.h_act + S.h_sz * (size_t)(l - 1);
    a.e = l == 0 ? (const float*)c.e : c.saved + S.e_act + S.e_sz * (size_t)(l - 1);
    bind_common(&dl, a, c.km, c.M, c.rm);
    bind_layer(S, P, l, a, c.saved, c.ws);
    if (c.bwd) bind_grads(a, c.grads + l);
  }
  return EGT_OK;
}

extern "C" int egt_block_fwd(const egt_block_desc* desc, const egt_block_params* params,
                             const void* h, const void* e, const uint8_t* key_mask,
                             const void* attn_mask, const uint8_t* rand_mask, void* h_out,
                             void* e_out, void* saved, void* workspace, void* stream) {
  const bool se = desc && (desc->flags & EGT_BF_STATIC_EDGE);   // e is an input only: e_out is not written (may be NULL)
  const ChainCall c{desc, 1, false, false, params, nullptr, h, e, key_mask, attn_mask, rand_mask, (float*)saved, (float*)workspace};
  int rc = check_call(c, h && e && h_out && (e_out || se) && saved && workspace, "h/e/h_out/e_out/saved/workspace", false);
  if (rc) return rc;
  const BlockPlan P = plan_block(desc, mask_tensor(desc, rand_mask));
  BlockArgs a;
  if ((rc = bind_chain(c, P, &a))) return rc;
  a.h_out = (float*)h_out; a.e_out = se ? nullptr : (float*)e_out;
  a.epi = 1;
  DISPATCH_BDE(desc->De, launch_fwd<DE>(a, P, (hipStream_t)stream, false));
  EGT_HIP_LAUNCH_CHECK("egt_block_fwd");
  return EGT_OK;
}

extern "C" int egt_block_bwd(const egt_block_desc* desc, const egt_block_params* params,
                             const void* h, const void* e, const uint8_t* key_mask,
                             const void* attn_mask, const uint8_t* rand_mask, const void* saved,
                             const void* d_h_out, const void* d_e_out, void* d_h, void* d_e,
                             const egt_block_params* grads, void* workspace, void* stream) {
  const bool se = desc && (desc->flags & EGT_BF_STATIC_EDGE);   // d_e_out NULL = zeros (not read)
  const ChainCall c{desc, 1, false, true, params, grads, h, e, key_mask, attn_mask, rand_mask, (float*)saved, (float*)workspace};
  int rc = check_call(c, h && e && saved && d_h_out && (d_e_out || se) && d_h && d_e && grads && workspace,
                      "h/e/saved/d_h_out/d_e_out/d_h/d_e/grads/workspace", d_h == d_h_out);
  if (rc) return rc;
  const BlockPlan P = plan_block(desc, mask_tensor(desc, rand_mask));
  BlockArgs a;
  if ((rc = bind_chain(c, P, &a))) return rc;
  a.prep = 0;   // prepared by the forward, kept in `saved`
  a.dh_out = (const float*)d_h_out; a.de_out = (const float*)d_e_out;
  a.dh = (float*)d_h; a.de = (float*)d_e;
  DISPATCH_BDE(desc->De, launch_bwd<DE>(a, P, (hipStream_t)stream, true, nullptr, nullptr, node_fused_ok(a)));
  egt_node_launch_wgrads(&a, 1, (hipStream_t)stream);
  egt_node_launch_reduce(&a, 1, P.nwg_bwd, P.EP, (hipStream_t)stream);  // partial sums + edge param grads
  EGT_HIP_LAUNCH_CHECK("egt_block_bwd");
  return EGT_OK;
}


// ============================================================ layer stack =====
// The model_height loop over attention blocks (graph_xformer_model_base.py:336-339) as ONE
// call per direction: Ly x {node_pre, block_fwd, node_post} enqueued back to back, and in
// backward the per-workgroup partial sums of ALL layers reduced by a single launch at the end
// (they are off the dh/de critical path).  Layer l draws its random mask from
// seed ^ golden * (l + 1)  (layer_seed).
extern "C" int egt_stack_fwd(const egt_block_desc* desc, int32_t layers, const egt_block_params* params,
                             const void* h, const void* e, const uint8_t* key_mask,
                             const void* attn_mask, void* h_out, void* e_out, void* saved,
                             void* workspace, void* stream) {
  const ChainCall c{desc, layers, true, false, params, nullptr, h, e, key_mask, attn_mask, nullptr, (float*)saved, (float*)workspace};
  int rc = check_call(c, params && h && e && h_out && e_out && saved && workspace, "h/e/h_out/e_out/saved/workspace", false);
  if (rc) return rc;
  const BlockPlan P = plan_block(desc, mask_tensor(desc, nullptr));
  BlockArgs as[64];
  if ((rc = bind_chain(c, P, as))) return rc;
  for (int l = 0; l < layers; ++l) {   // a layer writes the next layer's inputs (activations kept in `saved`)
    as[l].h_out = l == layers - 1 ? (float*)h_out : const_cast<float*>(as[l + 1].h);
    as[l].e_out = l == layers - 1 ? (float*)e_out : const_cast<float*>(as[l + 1].e);
  }
  // edge weights of every layer in one launch; each block's epilogue then finishes the node side
  // (dense_mha + residual) and already produces the next block's packed QKV, so a layer is ONE
  // launch wherever the epilogue covers the geometry
  // (the preparation rides along with layer 0's k_node_pre as extra workgroups: one launch less in front of every step)
  for (int l = 0; l < layers; ++l) as[l].prep = 0;
  int prev_epi = 0;
  if (egt_node_launch_pre_stack(as, layers, (hipStream_t)stream)) prev_epi = 2;   // layer 0's packed QKV rows exist
  else egt_node_launch_prep(as, layers, (hipStream_t)stream);
  for (int l = 0; l < layers; ++l) {
    BlockArgs& a = as[l];
    a.epi = 1;
    if (l + 1 < layers) {
      const BlockArgs& nx = as[l + 1];
      a.epi = 2;
      a.nx_nm_g = nx.nm_g; a.nx_nm_b = nx.nm_b; a.nx_Wqkv = nx.Wqkv; a.nx_wfrag = nx.wfrag; a.nx_bqkv = nx.bqkv;
      a.nx_qkvp = nx.qkvp;
    }
    DISPATCH_BDE(desc->De, prev_epi = launch_fwd<DE>(a, P, (hipStream_t)stream, prev_epi == 2));
  }
  EGT_HIP_LAUNCH_CHECK("egt_stack_fwd");
  return EGT_OK;
}

extern "C" int egt_stack_bwd(const egt_block_desc* desc, int32_t layers, const egt_block_params* params,
                             const void* h, const void* e, const uint8_t* key_mask,
                             const void* attn_mask, const void* saved, const void* d_h_out,
                             const void* d_e_out, void* d_h, void* d_e,
                             const egt_block_params* grads, void* workspace, void* stream) {
  const ChainCall c{desc, layers, true, true, params, grads, h, e, key_mask, attn_mask, nullptr, (float*)saved, (float*)workspace};
  int rc = check_call(c, params && grads && h && e && saved && d_h_out && d_e_out && d_h && d_e && workspace,
                      "grads/h/e/saved/d_h_out/d_e_out/d_h/d_e/workspace", d_h == d_h_out);
  if (rc) return rc;
  const BlockPlan P = plan_block(desc, mask_tensor(desc, nullptr));
  BlockArgs as[64];
  if ((rc = bind_chain(c, P, as))) return rc;
  for (int l = 0; l < layers; ++l) {
    BlockArgs& a = as[l];
    // d_e flows in place below the top layer; every layer keeps its own dh (the deferred dWo
    // contraction reads dh' of each layer at the end)
    auto dhbuf = [&](int ll) { return (float*)workspace + P.common_total + P.layer_total * (size_t)ll + P.dhbuf; };
    a.dh_out = l == layers - 1 ? (const float*)d_h_out : (const float*)dhbuf(l + 1);
    a.de_out = l == layers - 1 ? (const float*)d_e_out : (const float*)d_e;
    a.dh = l == 0 ? (float*)d_h : dhbuf(l);
    a.de = (float*)d_e;
  }
  bool fuse = true;
  for (int l = 0; l < layers; ++l) fuse = fuse && node_fused_ok(as[l]);
  for (int l = layers - 1; l >= 0; --l) {
    as[l].prep = 0;   // the LN-folded edge weights were prepared by the forward and live in `saved`
    DISPATCH_BDE(desc->De, launch_bwd<DE>(as[l], P, (hipStream_t)stream, l == layers - 1, l > 0 ? &as[l - 1] : nullptr,
                                          l + 1 < layers ? &as[l + 1] : nullptr, fuse));
  }
  egt_node_launch_wgrads(as, layers, (hipStream_t)stream);
  egt_node_launch_reduce(as, layers, P.nwg_bwd, P.EP, (hipStream_t)stream);
  EGT_HIP_LAUNCH_CHECK("egt_stack_bwd");
  return EGT_OK;
}
