// Degree scalers (scale_degree, EGT_BF_SCALE_DEGREE) on the MFMA-tile pair kernels of the fused attention block: the SD = true
// instances of k_block_fwd / k_block_fwd_r4 (egt_block_fwd.h) and k_block_bwd_v4 / k_block_bwd_v5 / k_block_bwd_v4r
// (egt_block_bwd.h), in a translation unit of their own so that they compile beside egt_block.hip, which keeps the plan
// (plan_block) and calls the two launchers below with what the plan chose.  fp32 edge tensors, gated attention; every De of the
// block (De = 8 runs on r4 / v4r: the De = 8 VALU kernels of egt_narrow.hip have no degree), d <= 8, full and ragged N, with and
// without a mask tensor.  The scaler type is a run-time flag inside the instances (EGT_BF_SCALER_LINEAR).
//   forward : deg = sum of the gates rides next to the softmax sum; V_att' = s(deg) V_att is what leaves the row finish (HBM and
//             the node epilogue's LDS rows), deg goes to slot 3 of the row statistics
//   backward: bwd_sd_rows turns the staged (dV_att', delta, deg) of a row into (s dV_att', delta, d deg) after the node-side
//             prologue; bwd_pair_grad adds d deg . g (1 - g) to every key's gate-logit gradient
#include "egt_common.h"

#include "egt_block.h"
#include "egt_tile.h"

#include "egt_block_dev.h"
#include "egt_dma.h"

#include "egt_block_fwd.h"
#include "egt_block_bwd.h"

#define DISPATCH_SD_DE(De, CALL)                      \
  switch (De) {                                       \
    case 8: { constexpr int DE = 8; CALL; } break;    \
    case 16: { constexpr int DE = 16; CALL; } break;  \
    case 32: { constexpr int DE = 32; CALL; } break;  \
    case 48: { constexpr int DE = 48; CALL; } break;  \
    default: { constexpr int DE = 64; CALL; } break;  \
  }

template <int DE>
static void sd_fwd(BlockArgs& a, int r4_waves, bool kvl, bool ml, bool full, const EgtLaunch& s, hipStream_t st) {
  if (r4_waves) {
    if constexpr (DE <= 16) {
      if (r4_waves == 4) {
        if (full) egt_launch_planned<k_block_fwd_r4<DE, true, 4, false, true>>("k_block_fwd", s, st, a);
        else egt_launch_planned<k_block_fwd_r4<DE, false, 4, false, true>>("k_block_fwd", s, st, a);
      } else {
        if (full) egt_launch_planned<k_block_fwd_r4<DE, true, 8, false, true>>("k_block_fwd", s, st, a);
        else egt_launch_planned<k_block_fwd_r4<DE, false, 8, false, true>>("k_block_fwd", s, st, a);
      }
    }
    return;
  }
  // the five forms of launch_tile_fwd (egt_block.hip)
  if (!kvl) {
    if (ml) egt_launch_planned<k_block_fwd<DE, false, true, false, false, true>>("k_block_fwd", s, st, a);
    else egt_launch_planned<k_block_fwd<DE, false, false, false, false, true>>("k_block_fwd", s, st, a);
  } else if (ml) egt_launch_planned<k_block_fwd<DE, true, true, false, false, true>>("k_block_fwd", s, st, a);
  else if (full) egt_launch_planned<k_block_fwd<DE, true, false, true, false, true>>("k_block_fwd", s, st, a);
  else egt_launch_planned<k_block_fwd<DE, true, false, false, false, true>>("k_block_fwd", s, st, a);
}

template <int DE>
static void sd_bwd(BlockArgs& a, int family, int mm, bool ml, bool full, const EgtLaunch& s, hipStream_t st) {
  if (family == EGT_SD_BWD_V4R) {
    if constexpr (DE <= 16) egt_launch_planned<k_block_bwd_v4r<DE, false, V4R_RR, true>>("k_block_bwd", s, st, a);
  } else if (family == EGT_SD_BWD_V5) {
    if constexpr (DE >= 32) {
      if (mm == EGT_MM_BF16X3) {
        if (full) egt_launch_planned<k_block_bwd_v5<DE, EGT_MM_BF16X3, false, true>>("k_block_bwd", s, st, a);
        else egt_launch_planned<k_block_bwd_v5<DE, EGT_MM_BF16X3, true, true>>("k_block_bwd", s, st, a);
      } else {
        if (full) egt_launch_planned<k_block_bwd_v5<DE, EGT_MM_F32, false, true>>("k_block_bwd", s, st, a);
        else egt_launch_planned<k_block_bwd_v5<DE, EGT_MM_F32, true, true>>("k_block_bwd", s, st, a);
      }
    }
  } else {   // v4: with fp32 edge tensors the plan takes it for a mask tensor only (ml; plan_for)
    (void)ml;
    if (full) egt_launch_planned<k_block_bwd_v4<DE, true, false, false, true>>("k_block_bwd", s, st, a);
    else egt_launch_planned<k_block_bwd_v4<DE, true, false, true, true>>("k_block_bwd", s, st, a);
  }
}

void egt_block_sd_launch_fwd(BlockArgs& a, int r4_waves, bool kvl, bool ml, bool full, const EgtLaunch& s, hipStream_t st) {
  DISPATCH_SD_DE(a.De, sd_fwd<DE>(a, r4_waves, kvl, ml, full, s, st));
}

void egt_block_sd_launch_bwd(BlockArgs& a, int family, int mm, bool ml, bool full, const EgtLaunch& s, hipStream_t st) {
  DISPATCH_SD_DE(a.De, sd_bwd<DE>(a, family, mm, ml, full, s, st));
}
