// Phase stamps of the hand-scheduled kernels: where a wave's cycles go, section by section.  Measurement builds only
// (-DEGT_STAMPS through build.py's per-unit flags or its EGT_STAMPS=1 shortcut); without the flag every macro below is empty
// and nothing of this header reaches the object.  tools/stamps.py runs a workload and prints the tables.
//   EGT_STAMP_UNIT(n)        once per translation unit, before its kernels: n slots (one per stamped kernel, or per wave role of one)
//   EGT_STAMP_DECL;          in a kernel: the wave's clock and its per-phase cycle sums
//   EGT_STAMP(i);            the cycles since the previous stamp go to phase i (a phase stamped in a loop accumulates)
//   EGT_STAMP_OUT(k);        once per wave, at its end: lane 0 adds the wave's sums to slot k (atomicAdd) and counts the wave
//   EGT_STAMP_REGISTER(tab)  once per unit, after the phase-name tables: hands the unit's slots to egt_stamps_read
// Clock: __builtin_readcyclecounter() (s_memtime, 64 bits) for every kernel.
// A slot holds the sums over EVERY stamping wave of EVERY workgroup since the last read, and the number of such waves: the tool
// prints means per wave.  Not comparable with figures of the earlier workgroup-0-only stamps of the MFMA inner op and the pair
// kernels (one workgroup's eight waves, one launch), nor exactly with the earlier De = 8 section timers (waves 0-3 only).
// Caveats: the clock reads are scalar and the compiler moves unpinned work across them; a stamp between two MFMA groups times
// their issue, not their completion.  The sums live in scalar registers: a stamps build adds no VGPR spill and no scratch to any
// kernel (tools/kres.py on both units), but hipcc spills SGPRs to VGPR lanes (.sgpr_spill_count) in the run-time-switched and the
// eight-wave k_narrow_bwd instances (<., -1, 4>: 4, <., -1, 8>: 8, <., 3, 8>: 2) and in k_attn_mfma_bwd_kv<32 | 64, 0> (3) --
// v_writelane / v_readlane pairs inside the stamped sections; the instances tools/stamps.py runs have none.
#pragma once
#ifdef EGT_STAMPS
#define EGT_STAMP_PHASES 16
struct EgtStampSlot { unsigned long long sum[EGT_STAMP_PHASES], waves; };
struct EgtStampKernel { const char* kernel; const char* const* names; int nphase; };   // names[i] == nullptr: phase i is not stamped
#define EGT_STAMP_UNIT(n) static __device__ EgtStampSlot g_egt_stamps[n]
#define EGT_STAMP_DECL unsigned long long st_last__ = __builtin_readcyclecounter(), st_acc__[EGT_STAMP_PHASES] = {}
#define EGT_STAMP(i) do { const unsigned long long t__ = __builtin_readcyclecounter(); st_acc__[i] += t__ - st_last__; st_last__ = t__; } while (0)
#define EGT_STAMP_OUT(k)                                                                                                      \
  do {                                                                                                                        \
    if ((threadIdx.x & 63) == 0) {                                                                                            \
      _Pragma("unroll") for (int i__ = 0; i__ < EGT_STAMP_PHASES; ++i__)                                                      \
        if (st_acc__[i__]) atomicAdd(&g_egt_stamps[k].sum[i__], st_acc__[i__]);                                               \
      atomicAdd(&g_egt_stamps[k].waves, 1ull);                                                                                \
    }                                                                                                                         \
  } while (0)

// ---- host: the units of the library and their one reader (exported in stamps builds only; not part of include/egt_amd.h) ----
struct EgtStampUnit { const void* symbol; const EgtStampKernel* kernels; int nslot; };
inline EgtStampUnit g_egt_stamp_units[4];
inline int g_egt_stamp_nunits = 0;
struct EgtStampRegistration {
  EgtStampRegistration(const void* symbol, const EgtStampKernel* kernels, int nslot) { g_egt_stamp_units[g_egt_stamp_nunits++] = {symbol, kernels, nslot}; }
};
#define EGT_STAMP_REGISTER(tab) static const EgtStampRegistration g_egt_stamp_registration(HIP_SYMBOL(g_egt_stamps), tab, (int)(sizeof(tab) / sizeof(tab[0])))
// Slot k of the library (units in registration order): its kernel, phase names, sums[EGT_STAMP_PHASES] and wave count; the slot is
// zeroed on the device.  Returns 0, 1 when k is past the last slot, -1 on a HIP error.
extern "C" __attribute__((used, visibility("default"))) inline int egt_stamps_read(int k, const char** kernel, const char* const** names, int* nphase,
                                                                                  unsigned long long* sums, unsigned long long* waves) {
  for (int u = 0; u < g_egt_stamp_nunits; ++u) {
    const EgtStampUnit& U = g_egt_stamp_units[u];
    if (k >= U.nslot) { k -= U.nslot; continue; }
    EgtStampSlot s;
    const EgtStampSlot zero = {};
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpyFromSymbol(&s, U.symbol, sizeof(s), k * sizeof(s)) != hipSuccess ||
        hipMemcpyToSymbol(U.symbol, &zero, sizeof(zero), k * sizeof(zero)) != hipSuccess) return -1;
    *kernel = U.kernels[k].kernel; *names = U.kernels[k].names; *nphase = U.kernels[k].nphase; *waves = s.waves;
    for (int i = 0; i < EGT_STAMP_PHASES; ++i) sums[i] = s.sum[i];
    return 0;
  }
  return 1;
}
#else
#define EGT_STAMP_UNIT(n)
#define EGT_STAMP_DECL
#define EGT_STAMP(i)
#define EGT_STAMP_OUT(k)
#define EGT_STAMP_REGISTER(tab)
#endif
