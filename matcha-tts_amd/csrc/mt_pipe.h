// The LDS-DMA pipeline primitives of the persistent kernels (mt_vconv, mt_rbconv, mt_ffn and the ResBlock pair
// kernels), one definition each: the 16-byte global -> LDS DMA, the runtime vmcnt wait, the two workgroup barriers,
// the compile-time loop, the MFMA-layout swap and the host-side CU count. (The buffer-resource forms buf_rsrc /
// buf_lds16 / buf_store16 are mt_common.h's.)
#pragma once
#include <type_traits>

#include "mt_common.h"

namespace mt {

// 16 bytes per lane from src (per lane) into lds_wave_base + 16 * lane (global_load_lds_dwordx4)
__device__ __forceinline__ void glds16(const void* src, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// s_waitcnt vmcnt(k) for a wave-uniform runtime bound n, with k the largest of {0,2,4,7,10,15,23,31} <= n:
// waiting for fewer outstanding operations than allowed is always correct (only stricter), and a
// three-level branch tree keeps the scalar cost per step small (a 64-way switch was ~40 SALU + branches)
__device__ __forceinline__ void wait_vmcnt(int n) {
  if (n < 7) {
    if (n < 2) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if (n < 4) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  } else if (n < 15) {
    if (n < 10) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
  } else {
    if (n < 23) asm volatile("s_waitcnt vmcnt(15)" ::: "memory");
    else if (n < 31) asm volatile("s_waitcnt vmcnt(23)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(31)" ::: "memory");
  }
}

// the draining barrier: every LDS operation of this wave (writes other waves will read, reads of what they will
// overwrite) has completed before the workgroup meets; nothing is scheduled across it
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}
// a K-loop step's barrier: publishes LDS-DMA data (each wave waited for its own with vmcnt) and frees the ring slot
// of two steps back. No LDS write is in flight there, and the reads still in flight (the next step's first K-slice)
// touch neither the slot the step's DMA overwrites nor anything another wave writes, so no lgkmcnt drain: the
// compiler waits for them where the MFMAs use them
__device__ __forceinline__ void step_barrier() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// compile-time loop: f(integral_constant<int, I>) for I in [I0, N)
template <int I, int N, class F>
__device__ __forceinline__ void vc_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    vc_for<I + 1, N>(f);
  }
}

// Epilogue I/O is 16 bytes per lane: MFMA blocks X = (fm, fn) and Y = (fm + 1, fn) hold, per lane, 4 channels of one
// frame each; v_permlane16_swap (odd 16-lane rows of x <-> even rows of y) turns them into 8 consecutive channels
// per lane (row g4: X or Y by g4 & 1, channels +8 by g4 >> 1). An involution: loaded words go back the same way.
__device__ __forceinline__ void swap16(uint32_t& x, uint32_t& y) {
  const auto r = __builtin_amdgcn_permlane16_swap(x, y, false, false);
  x = r[0];
  y = r[1];
}

// words [X|Y][dword] in accumulator layout -> the lane's 16 bytes in store layout (o is left swapped), and back
__device__ __forceinline__ u32x4 pack16(uint32_t (&o)[2][2]) {
  swap16(o[0][0], o[1][0]);
  swap16(o[0][1], o[1][1]);
  return u32x4{o[0][0], o[0][1], o[1][0], o[1][1]};
}
__device__ __forceinline__ void unpack16(const u32x4& v, uint32_t (&o)[2][2]) {
  o[0][0] = v[0], o[0][1] = v[1], o[1][0] = v[2], o[1][1] = v[3];
  swap16(o[0][0], o[1][0]);
  swap16(o[0][1], o[1][1]);
}

// compute units of the current device (the persistent kernels' grid bound), queried once; 256 if the query fails
inline int cu_count() {
  static int n = 0;
  if (n == 0) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
  }
  return n;
}

}  // namespace mt
