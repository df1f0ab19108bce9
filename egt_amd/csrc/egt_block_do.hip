// Attention dropout (attn_dropout, EGT_BF_ATTN_DROPOUT) on the MFMA-tile pair kernels of the fused attention block: the DO = true
// instances of k_block_fwd / k_block_fwd_r4 (egt_block_fwd.h) and k_block_bwd_v4 / k_block_bwd_v5 / k_block_bwd_v4r
// (egt_block_bwd.h), in a translation unit of their own so that they compile beside egt_block.hip, which keeps the plan
// (plan_block) and calls the two launchers below with what the plan chose.  fp32 and bf16 edge tensors (a.bf16), gated and ungated
// attention (a run-time flag inside the instances), every De of the block (De = 8 runs on r4 / v4r: the De = 8 VALU kernels of
// egt_narrow.hip draw no dropout), d <= 8, full and ragged N, with and without a mask tensor, v5 in both matmul forms.
//   keep(b, l, m, h) <=> (egt_hash32(((b N + l) N + m) H + h, s0, s1 ^ EGT_DROPOUT_STREAM) >> 8) >= egt_threshold24(rate); a kept
//   element is scaled by 1 / (1 - rate).  (s0, s1): the effective seed of the call -- the random mask draws from the same seed on
//   its own stream.  Nothing is stored: both directions recompute the factor from the counter (attn_drop_factor, egt_block_dev.h).
//   forward : av = p . g of (pair, head) is multiplied by the factor before it enters O (fwd_softmax_av_do); the softmax sum,
//             H_hat, the edge update and the row statistics do not see the mask
//   backward: bwd_pair_grad<.., DO> multiplies dA_t by the factor before dS, dG and the softmax backward, and hands the dropped
//             A_tild to dV; delta stays as the node side computes it
// SD and DO together are not instantiated (block_check refuses the two flags together).
#include "egt_common.h"

#include "egt_block.h"
#include "egt_tile.h"

#include "egt_block_dev.h"
#include "egt_dma.h"

#include "egt_block_fwd.h"
#include "egt_block_bwd.h"

#define DISPATCH_DO_DE(De, CALL)                      \
  switch (De) {                                       \
    case 8: { constexpr int DE = 8; CALL; } break;    \
    case 16: { constexpr int DE = 16; CALL; } break;  \
    case 32: { constexpr int DE = 32; CALL; } break;  \
    case 48: { constexpr int DE = 48; CALL; } break;  \
    default: { constexpr int DE = 64; CALL; } break;  \
  }

template <int DE, bool BF>
static void do_fwd(BlockArgs& a, int r4_waves, bool kvl, bool ml, bool full, const EgtLaunch& s, hipStream_t st) {
  if (r4_waves) {
    if constexpr (DE <= 16) {
      if (r4_waves == 4) {
        if (full) egt_launch_planned<k_block_fwd_r4<DE, true, 4, BF, false, true>>("k_block_fwd", s, st, a);
        else egt_launch_planned<k_block_fwd_r4<DE, false, 4, BF, false, true>>("k_block_fwd", s, st, a);
      } else {
        if (full) egt_launch_planned<k_block_fwd_r4<DE, true, 8, BF, false, true>>("k_block_fwd", s, st, a);
        else egt_launch_planned<k_block_fwd_r4<DE, false, 8, BF, false, true>>("k_block_fwd", s, st, a);
      }
    }
    return;
  }
  // the five forms of launch_tile_fwd (egt_block.hip)
  if (!kvl) {
    if (ml) egt_launch_planned<k_block_fwd<DE, false, true, false, BF, false, true>>("k_block_fwd", s, st, a);
    else egt_launch_planned<k_block_fwd<DE, false, false, false, BF, false, true>>("k_block_fwd", s, st, a);
  } else if (ml) egt_launch_planned<k_block_fwd<DE, true, true, false, BF, false, true>>("k_block_fwd", s, st, a);
  else if (full) egt_launch_planned<k_block_fwd<DE, true, false, true, BF, false, true>>("k_block_fwd", s, st, a);
  else egt_launch_planned<k_block_fwd<DE, true, false, false, BF, false, true>>("k_block_fwd", s, st, a);
}

template <int DE, bool BF>
static void do_bwd(BlockArgs& a, int family, int mm, bool ml, bool full, const EgtLaunch& s, hipStream_t st) {
  if (family == EGT_SD_BWD_V4R) {
    if constexpr (DE <= 16) egt_launch_planned<k_block_bwd_v4r<DE, BF, V4R_RR, false, true>>("k_block_bwd", s, st, a);
  } else if (family == EGT_SD_BWD_V5) {   // fp32 edge tensors only (plan_for)
    if constexpr (DE >= 32 && !BF) {
      if (mm == EGT_MM_BF16X3) {
        if (full) egt_launch_planned<k_block_bwd_v5<DE, EGT_MM_BF16X3, false, false, true>>("k_block_bwd", s, st, a);
        else egt_launch_planned<k_block_bwd_v5<DE, EGT_MM_BF16X3, true, false, true>>("k_block_bwd", s, st, a);
      } else {
        if (full) egt_launch_planned<k_block_bwd_v5<DE, EGT_MM_F32, false, false, true>>("k_block_bwd", s, st, a);
        else egt_launch_planned<k_block_bwd_v5<DE, EGT_MM_F32, true, false, true>>("k_block_bwd", s, st, a);
      }
    }
  } else if (ml) {   // v4: a mask tensor, any De and edge type
    if (full) egt_launch_planned<k_block_bwd_v4<DE, true, BF, false, false, true>>("k_block_bwd", s, st, a);
    else egt_launch_planned<k_block_bwd_v4<DE, true, BF, true, false, true>>("k_block_bwd", s, st, a);
  } else {           // v4 without a mask tensor: bf16 edge tensors on the wide tiles (plan_for: fp32 goes to v5, De <= 16 to v4r)
    if constexpr (DE >= 32 && BF) {
      if (full) egt_launch_planned<k_block_bwd_v4<DE, false, true, false, false, true>>("k_block_bwd", s, st, a);
      else egt_launch_planned<k_block_bwd_v4<DE, false, true, true, false, true>>("k_block_bwd", s, st, a);
    }
  }
}

void egt_block_do_launch_fwd(BlockArgs& a, int r4_waves, bool kvl, bool ml, bool full, const EgtLaunch& s, hipStream_t st) {
  if (a.bf16) { DISPATCH_DO_DE(a.De, (do_fwd<DE, true>(a, r4_waves, kvl, ml, full, s, st))); }
  else { DISPATCH_DO_DE(a.De, (do_fwd<DE, false>(a, r4_waves, kvl, ml, full, s, st))); }
}

void egt_block_do_launch_bwd(BlockArgs& a, int family, int mm, bool ml, bool full, const EgtLaunch& s, hipStream_t st) {
  if (a.bf16) { DISPATCH_DO_DE(a.De, (do_bwd<DE, true>(a, family, mm, ml, full, s, st))); }
  else { DISPATCH_DO_DE(a.De, (do_bwd<DE, false>(a, family, mm, ml, full, s, st))); }
}
