// Inner op on MFMA tiles, opt-in bf16 products (egt_attn_desc.reserved & EGT_ATTN_MM_BF16): the MM = 1 instances of the four kernels of
// egt_attn_kernels.h (QK^T, A.V and their backward products on v_mfma_f32_16x16x32_bf16 / v_mfma_f32_16x16x16_bf16, fp32 accumulate)
// behind their two entry points.  The kernel bodies, the arithmetic contract and what the operand form changes are described there;
// the contractions on packed fragments stand beside the fp32 ones in egt_attn_dev.h.  A translation unit of its own: it builds beside
// egt_attn_mfma.hip, and that unit's measurement flags (ablations, stamps) do not reach these instances.
#include "egt_attn_kernels.h"

void egt_attn_bf16_launch_fwd(int var, const EgtLaunch& pack, const EgtLaunch& fwd, const AttnMfmaArgs& a, hipStream_t st) {
  attn_launch_fwd<1>(var, pack, fwd, a, st);
}
void egt_attn_bf16_launch_bwd(int var, const EgtLaunch& pack, const EgtLaunch& kv, const EgtLaunch& q, const AttnMfmaArgs& a, hipStream_t st) {
  attn_launch_bwd<1>(var, pack, kv, q, a, st);
}
