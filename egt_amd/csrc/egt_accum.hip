// egt_accumulate — epoch sums of (metric sum, count) pairs kept on the device.
//
// A training step that never synchronises cannot hand its loss and metric sums to the host one by one.  The step's fp32
// results stay where the step wrote them and ONE launch of one wave adds each of them to an fp64 accumulator: lane k owns
// item k and the pair acc[2k], acc[2k+1].  The additions of one pair happen in launch order, so the accumulator holds what
// `a += float(x)` on the host would after the same sequence.  Plain loads and stores, no atomics, capturable.
#include "egt_common.h"

namespace {
constexpr int ACC_MAX_ITEMS = 32;

__global__ __launch_bounds__(64) void k_accumulate(double* __restrict__ acc, const egt_acc_item* __restrict__ items, int K) {
  const int k = threadIdx.x;
  if (blockIdx.x != 0 || k >= K) return;
  const egt_acc_item it = items[k];
  const double s = (double)*it.sum;
  const double c = it.count ? (double)*it.count : (double)it.count_value;
  acc[2 * k] += s;
  acc[2 * k + 1] += c;
}
}  // namespace

extern "C" int egt_accumulate(double* acc, const egt_acc_item* items, int32_t K, void* stream) {
  if (!acc) EGT_FAIL(EGT_E_NULL, "acc is NULL");
  if (!items) EGT_FAIL(EGT_E_NULL, "items is NULL");
  if (K < 1 || K > ACC_MAX_ITEMS) EGT_FAIL(EGT_E_SHAPE, "egt_accumulate: K %d outside 1..%d", K, ACC_MAX_ITEMS);
  if ((reinterpret_cast<uintptr_t>(acc) | reinterpret_cast<uintptr_t>(items)) & 7) EGT_FAIL(EGT_E_SHAPE, "acc and items must be 8-byte aligned");
  EGT_LAUNCH("k_accumulate", k_accumulate, dim3(1), dim3(64), 0, (hipStream_t)stream, acc, items, (int)K);
  EGT_HIP_LAUNCH_CHECK("egt_accumulate");
  return EGT_OK;
}
