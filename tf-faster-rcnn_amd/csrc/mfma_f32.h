// What the direct-to-LDS slab-ring kernels share: the 32x32 MFMA accumulator type, the LDS address space, the counted vector-memory
// wait and the direct-to-LDS load (conv_igemm.hip, wgrad_tn.hip, gemm_x3.hip; wgrad_h2.hip takes the accumulator type only).
#pragma once
#include <hip/hip_runtime.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define LDS_AS __attribute__((address_space(3)))

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// One direct-to-LDS load: 64 lanes x 16 B from per-lane global addresses to LDS [lds_base, +1 KiB),
// lane-linear.  Issued from inline asm on purpose: hipcc tracks builtin LDS-DMA conservatively and
// puts `s_waitcnt vmcnt(0)` in front of the first ds_read of every k-step (it cannot prove the ring
// slots disjoint), which would drain the NS-deep pipeline; asm loads are invisible to its scoreboard,
// so the counted waits of the callers are the only ones.  M0 (LDS base) is saved/restored inside the statement.
__device__ __forceinline__ void glds16(const void* gsrc, unsigned lds_base) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, off\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(gsrc), "s"(lds_base)
      : "memory");
}
