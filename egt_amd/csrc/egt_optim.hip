// egt_optim_* — the parameter update of a training step as two launches: Adam / RMSprop / SGD over the flat gradient buffer.
//
// What torch.optim does for the training driver today in chunks of multi-tensor launches (about ten elementwise passes for
// Adam, each moving a few hundred kilobytes), as ONE stream over gradients, moments and parameters.  The gradients and the
// moments are flat fp32 buffers in the layout of FlatGradAllReduce (running sum of numel(), no padding); the parameters stay
// where they are and are reached through a device-resident table of work items {param pointer, flat offset, count} that the
// host cut so that no item straddles a parameter.  One workgroup takes one item.
//
// Alignment.  An item starts at any float offset of the flat buffers and at any 4-byte-aligned parameter address.  The flat
// side decides the split: dword accesses up to the first 16-byte boundary of the flat offset, dwordx4 from there, dword
// accesses for the rest.  The parameter moves as dwordx4 in the middle part when its address is 16-byte aligned there, else
// as four dwords.  Nothing outside [0, count) of an item is read or written.
//
// Arithmetic: torch.optim's (the multi-tensor path), one copy (optim_elem) for every access form, with the contractions
// written out, so that an element's result does not depend on the item it falls into or on its lane.
//   Adam     m = m + (1-b1) (g - m);  v = b2 v + (1-b2) (g g);  p -= step_size * (m / (sqrt(v) / bc2_sqrt + eps))
//   RMSprop  sq = a sq + (1-a) (g g);  p -= lr * (g / (sqrt(sq) + eps))
//   SGD      p -= lr g
// Everything that changes from step to step lives in the state block (kernel arguments are frozen when a hipGraph is
// captured): k_optim_prepare, one thread in front of the step kernel, advances the step count and forms the bias
// corrections in fp64 -- 1 - 0.999^t in fp32 carries a relative error of about 3e-5 at small t -- and leaves the fp32
// scalars the step kernel reads.  The step kernel writes no state.
#include <math.h>

#include "egt_common.h"

namespace {
struct OptimState {          // EGT_OPTIM_STATE_BYTES; the first 24 bytes are the host's (include/egt_amd.h)
  int64_t t;                 // steps taken: k_optim_prepare increments it
  double lr;                 // host
  float grad_scale;          // host
  float pad0;
  float step_size;           // k_optim_prepare: lr / (1 - beta1^t)      (lr where the algorithm has no first moment)
  float bc2_sqrt;            //                  sqrt(1 - beta2^t)       (1 likewise)
  float lr_f;                //                  (float)lr
  float grad_scale_f;        //                  grad_scale
  float pad1[6];
};
static_assert(sizeof(OptimState) == EGT_OPTIM_STATE_BYTES, "include/egt_amd.h: EGT_OPTIM_STATE_BYTES");
static_assert(sizeof(egt_optim_segment) == 24, "egt_optim_segment is 24 bytes");

struct OptimConst {          // per launch, from the descriptor
  float w1, beta2, w2, eps, clip;   // w1 = 1 - beta1, w2 = 1 - beta2 (formed in double on the host, as torch.optim forms them)
};

constexpr int OPT_THREADS = 256;

__global__ void k_optim_prepare(OptimState* st, int algo, double beta1, double beta2) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int64_t t = st->t + 1;
  const double lr = st->lr;
  double bc1 = 1.0, bc2 = 1.0;
  if (algo == EGT_OPT_ADAM) {
    bc1 = 1.0 - pow(beta1, (double)t);
    bc2 = 1.0 - pow(beta2, (double)t);
  }
  st->t = t;
  st->step_size = (float)(lr / bc1);
  st->bc2_sqrt = (float)sqrt(bc2);
  st->lr_f = (float)lr;
  st->grad_scale_f = st->grad_scale;
}

struct OptimScal { float step_size, bc2_sqrt, lr, grad_scale; };

// one element; `m` / `v` are dead where the algorithm has none
template <int ALGO, bool CLIP>
__device__ __forceinline__ void optim_elem(float& p, float g, float& m, float& v, const OptimConst& c, const OptimScal& s) {
#pragma clang fp contract(off)
  g = g * s.grad_scale;
  if (CLIP) g = g < -c.clip ? -c.clip : (g > c.clip ? c.clip : g);   // NaN passes, as through clamp_
  if (ALGO == EGT_OPT_SGD) {
    p = fmaf(-s.lr, g, p);
    return;
  }
  v = fmaf(c.w2, g * g, v * c.beta2);
  if (ALGO == EGT_OPT_ADAM) {
    m = fmaf(c.w1, g - m, m);
    const float den = sqrtf(v) / s.bc2_sqrt + c.eps;
    p = fmaf(-s.step_size, m / den, p);
  } else {
    const float den = sqrtf(v) + c.eps;
    p = fmaf(-s.lr, g / den, p);
  }
}

template <int ALGO, bool CLIP, bool ZERO>
__device__ __forceinline__ void optim_one(float* p, float* grad, float* m, float* v, int64_t f, const OptimConst& c, const OptimScal& s) {
  float pv = *p, mv = 0.f, vv = 0.f;
  const float g = grad[f];
  if (ALGO == EGT_OPT_ADAM) mv = m[f];
  if (ALGO != EGT_OPT_SGD) vv = v[f];
  optim_elem<ALGO, CLIP>(pv, g, mv, vv, c, s);
  *p = pv;
  if (ALGO == EGT_OPT_ADAM) m[f] = mv;
  if (ALGO != EGT_OPT_SGD) v[f] = vv;
  if (ZERO) grad[f] = 0.f;
}

template <int ALGO, bool CLIP, bool ZERO>
__global__ __launch_bounds__(OPT_THREADS) void k_optim_step(const egt_optim_segment* __restrict__ table, float* __restrict__ grad,
                                                            float* __restrict__ m, float* __restrict__ v,
                                                            const OptimState* __restrict__ st, OptimConst c) {
  const egt_optim_segment seg = table[blockIdx.x];
  float* const p = seg.param;
  const int64_t off = seg.offset, n = seg.count;
  const OptimScal s = {st->step_size, st->bc2_sqrt, st->lr_f, st->grad_scale_f};
  const int tid = threadIdx.x;
  // [0, head) dwords, [head, head + 4 nv) dwordx4 on the flat side, [head + 4 nv, n) dwords
  int64_t head = (4 - (off & 3)) & 3;
  if (head > n) head = n;
  const int64_t nv = (n - head) >> 2;
  const int64_t tail0 = head + 4 * nv;
  if (tid < head) optim_one<ALGO, CLIP, ZERO>(p + tid, grad, m, v, off + tid, c, s);
  const bool pvec = ((reinterpret_cast<uintptr_t>(p + head)) & 15) == 0;   // uniform over the workgroup
  for (int64_t q = tid; q < nv; q += OPT_THREADS) {
    const int64_t i = head + 4 * q, f = off + i;
    float4 pv, mv = make_float4(0.f, 0.f, 0.f, 0.f), vv = mv;
    const float4 g = *reinterpret_cast<const float4*>(grad + f);
    if (ALGO == EGT_OPT_ADAM) mv = *reinterpret_cast<const float4*>(m + f);
    if (ALGO != EGT_OPT_SGD) vv = *reinterpret_cast<const float4*>(v + f);
    if (pvec) pv = *reinterpret_cast<const float4*>(p + i);
    else pv = make_float4(p[i], p[i + 1], p[i + 2], p[i + 3]);
    optim_elem<ALGO, CLIP>(pv.x, g.x, mv.x, vv.x, c, s);
    optim_elem<ALGO, CLIP>(pv.y, g.y, mv.y, vv.y, c, s);
    optim_elem<ALGO, CLIP>(pv.z, g.z, mv.z, vv.z, c, s);
    optim_elem<ALGO, CLIP>(pv.w, g.w, mv.w, vv.w, c, s);
    if (pvec) *reinterpret_cast<float4*>(p + i) = pv;
    else { p[i] = pv.x; p[i + 1] = pv.y; p[i + 2] = pv.z; p[i + 3] = pv.w; }
    if (ALGO == EGT_OPT_ADAM) *reinterpret_cast<float4*>(m + f) = mv;
    if (ALGO != EGT_OPT_SGD) *reinterpret_cast<float4*>(v + f) = vv;
    if (ZERO) *reinterpret_cast<float4*>(grad + f) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (tid < n - tail0) optim_one<ALGO, CLIP, ZERO>(p + tail0 + tid, grad, m, v, off + tail0 + tid, c, s);
}

// one text behind egt_optim_supported and the two entry points
int optim_desc_check(const egt_optim_desc* d, bool report) {
  if (!d) EGT_BAD(EGT_E_NULL, "desc is NULL");
  if (d->algo != EGT_OPT_ADAM && d->algo != EGT_OPT_RMSPROP && d->algo != EGT_OPT_SGD)
    EGT_BAD(EGT_E_FLAGS, "egt_optim_desc.algo %d: EGT_OPT_ADAM, EGT_OPT_RMSPROP or EGT_OPT_SGD", d->algo);
  if (d->flags & ~(EGT_OPT_CLIP | EGT_OPT_ZERO_GRAD)) EGT_BAD(EGT_E_FLAGS, "egt_optim_desc.flags 0x%x has unknown bits", d->flags);
  if (d->reserved != 0) EGT_BAD(EGT_E_FLAGS, "egt_optim_desc.reserved must be 0");
  if ((d->flags & EGT_OPT_CLIP) && !(d->clip_value > 0.f)) EGT_BAD(EGT_E_FLAGS, "EGT_OPT_CLIP needs clip_value > 0 (got %g)", d->clip_value);
  if (d->num_segments < 1) EGT_BAD(EGT_E_SHAPE, "num_segments must be >= 1 (got %d)", d->num_segments);
  if (d->total < d->num_segments) EGT_BAD(EGT_E_SHAPE, "total %lld is less than one element per segment (%d segments)", (long long)d->total, d->num_segments);
  if (d->algo != EGT_OPT_SGD) {
    if (d->algo == EGT_OPT_ADAM && !(d->beta1 >= 0.0 && d->beta1 < 1.0)) EGT_BAD(EGT_E_SHAPE, "beta1 %g outside [0, 1)", d->beta1);
    if (!(d->beta2 >= 0.0 && d->beta2 < 1.0)) EGT_BAD(EGT_E_SHAPE, "beta2 / alpha %g outside [0, 1)", d->beta2);
    if (!(d->eps >= 0.f)) EGT_BAD(EGT_E_SHAPE, "eps %g is negative", d->eps);
  }
  return EGT_OK;
}

template <int ALGO, bool CLIP>
void launch_step(const egt_optim_desc* d, const egt_optim_segment* table, float* grad, float* m, float* v, const OptimState* st,
                 const OptimConst& c, hipStream_t s) {
  const dim3 grid((unsigned)d->num_segments), block(OPT_THREADS);
  if (d->flags & EGT_OPT_ZERO_GRAD) EGT_LAUNCH("k_optim_step", (k_optim_step<ALGO, CLIP, true>), grid, block, 0, s, table, grad, m, v, st, c);
  else EGT_LAUNCH("k_optim_step", (k_optim_step<ALGO, CLIP, false>), grid, block, 0, s, table, grad, m, v, st, c);
}
template <int ALGO>
void launch_step_clip(const egt_optim_desc* d, const egt_optim_segment* table, float* grad, float* m, float* v, const OptimState* st,
                      const OptimConst& c, hipStream_t s) {
  if (d->flags & EGT_OPT_CLIP) launch_step<ALGO, true>(d, table, grad, m, v, st, c, s);
  else launch_step<ALGO, false>(d, table, grad, m, v, st, c, s);
}
}  // namespace

extern "C" int egt_optim_supported(const egt_optim_desc* desc) { return optim_desc_check(desc, false) == EGT_OK ? 1 : 0; }

extern "C" int egt_optim_prepare(const egt_optim_desc* desc, void* state, void* stream) {
  const int rc = optim_desc_check(desc, true);
  if (rc != EGT_OK) return rc;
  if (!state) EGT_FAIL(EGT_E_NULL, "state is NULL");
  if (reinterpret_cast<uintptr_t>(state) & 7) EGT_FAIL(EGT_E_SHAPE, "state must be 8-byte aligned");
  EGT_LAUNCH("k_optim_prepare", k_optim_prepare, dim3(1), dim3(1), 0, (hipStream_t)stream, (OptimState*)state, (int)desc->algo,
             desc->beta1, desc->beta2);
  EGT_HIP_LAUNCH_CHECK("egt_optim_prepare");
  return EGT_OK;
}

extern "C" int egt_optim_step(const egt_optim_desc* desc, const egt_optim_segment* table, float* grad, float* m, float* v,
                              void* state, void* stream) {
  const int rc = optim_desc_check(desc, true);
  if (rc != EGT_OK) return rc;
  if (!table) EGT_FAIL(EGT_E_NULL, "table is NULL");
  if (!grad) EGT_FAIL(EGT_E_NULL, "grad is NULL");
  if (!state) EGT_FAIL(EGT_E_NULL, "state is NULL");
  if (desc->algo == EGT_OPT_ADAM && !m) EGT_FAIL(EGT_E_NULL, "m is NULL (EGT_OPT_ADAM keeps a first moment)");
  if (desc->algo != EGT_OPT_SGD && !v) EGT_FAIL(EGT_E_NULL, "v is NULL (EGT_OPT_ADAM / EGT_OPT_RMSPROP keep a second moment)");
  if (desc->algo != EGT_OPT_ADAM) m = nullptr;
  if (desc->algo == EGT_OPT_SGD) v = nullptr;
  if ((reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v)) & 15)
    EGT_FAIL(EGT_E_SHAPE, "grad, m and v must be 16-byte aligned (flat buffers; the parameters need 4)");
  if ((reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(state)) & 7) EGT_FAIL(EGT_E_SHAPE, "table and state must be 8-byte aligned");
  const OptimConst c = {(float)(1.0 - desc->beta1), (float)desc->beta2, (float)(1.0 - desc->beta2), desc->eps, desc->clip_value};
  const OptimState* st = (const OptimState*)state;
  hipStream_t s = (hipStream_t)stream;
  switch (desc->algo) {
    case EGT_OPT_ADAM: launch_step_clip<EGT_OPT_ADAM>(desc, table, grad, m, v, st, c, s); break;
    case EGT_OPT_RMSPROP: launch_step_clip<EGT_OPT_RMSPROP>(desc, table, grad, m, v, st, c, s); break;
    default: launch_step_clip<EGT_OPT_SGD>(desc, table, grad, m, v, st, c, s); break;
  }
  EGT_HIP_LAUNCH_CHECK("egt_optim_step");
  return EGT_OK;
}
