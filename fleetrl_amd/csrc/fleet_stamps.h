// fleet_stamps.h -- diagnostic time stamps inside the step kernels (FLEET_STAMPS builds only: tools/stamps.py).
//
// Provides FLEET_STAMP(k) (shader clock), FLEET_STAMP_RT(k) (wall clock) and FLEET_STAMP_WHERE() (which die / CU / SIMD), and the
// host reader fleet_debug_read_stamps.  In the product build all three macros expand to nothing.  Restates nothing of the reference.
// Expects of its includer: FLEET_KBLOCK (threads per workgroup, fleet_kernels.hip) is defined where a stamp macro is EXPANDED; the
// macros are only used inside kernels of kBlock-thread workgroups.
#pragma once
#include <hip/hip_runtime.h>

#ifdef FLEET_STAMPS
// Diagnostic build only (tools/stamps.py): s_memtime stamps of every wave (the first 4096) at fixed points of the step,
// written to a buffer nothing else reads.  Never compiled into the product library.
__device__ unsigned long long fleet_stamp_buf[4096 * 32];
#define FLEET_STAMP(k)                                                                                   \
  do {                                                                                                   \
    __builtin_amdgcn_sched_barrier(0);                                                                   \
    unsigned long long _t;                                                                               \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(_t)::"memory");                           \
    __builtin_amdgcn_sched_barrier(0);                                                                   \
    const unsigned _w = blockIdx.x * (FLEET_KBLOCK / 64) + threadIdx.x / 64;                             \
    if ((threadIdx.x & 63) == 0 && _w < 4096) fleet_stamp_buf[_w * 32 + (k)] = _t;                       \
  } while (0)
// wall-clock stamps (s_memrealtime: 100 MHz, one counter for the whole chip) at a wave's entry (slot 9) and exit (slot 10):
// the launch's timeline across dies, which the per-die shader-clock stamps cannot give
#define FLEET_STAMP_RT(k)                                                                                \
  do {                                                                                                   \
    const unsigned long long _t = __builtin_amdgcn_s_memrealtime();                                      \
    const unsigned _w = blockIdx.x * (FLEET_KBLOCK / 64) + threadIdx.x / 64;                             \
    if ((threadIdx.x & 63) == 0 && _w < 4096) fleet_stamp_buf[_w * 32 + (k)] = _t;                       \
  } while (0)
// where the wavefront runs (slot 16: HW_REG_HW_ID = wave / SIMD / CU / SH / SE ids; slot 17: HW_REG_XCC_ID): does the tail of slow
// wavefronts belong to a die, a CU, a SIMD?
#define FLEET_STAMP_WHERE()                                                                              \
  do {                                                                                                   \
    const unsigned _hw = __builtin_amdgcn_s_getreg((4) | (0 << 6) | (31 << 11));                         \
    const unsigned _xc = __builtin_amdgcn_s_getreg((20) | (0 << 6) | (31 << 11));                        \
    const unsigned _w = blockIdx.x * (FLEET_KBLOCK / 64) + threadIdx.x / 64;                             \
    if ((threadIdx.x & 63) == 0 && _w < 4096) {                                                          \
      fleet_stamp_buf[_w * 32 + 16] = _hw;                                                               \
      fleet_stamp_buf[_w * 32 + 17] = _xc;                                                               \
    }                                                                                                    \
  } while (0)
extern "C" int fleet_debug_read_stamps(unsigned long long* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(fleet_stamp_buf), sizeof(fleet_stamp_buf));
}
#else
#define FLEET_STAMP(k) do {} while (0)
#define FLEET_STAMP_RT(k) do {} while (0)
#define FLEET_STAMP_WHERE() do {} while (0)
#endif
