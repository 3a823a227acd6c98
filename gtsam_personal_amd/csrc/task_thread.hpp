#pragma once
#include <hip/hip_runtime.h>

namespace lmgpu {

// The thread index of a role of a chained task (kernels_step.hpp, kernels_potrf.hpp, kernels_dense.hpp: syrk_tile).  The product:
// threadIdx.x.  The test library runs those roles in a loop (chain_kernel, resident form), and there everything a role derives from
// threadIdx.x alone (lane masks, LDS offsets) would be computed once in front of the loop and held across the update tile, which has
// no register to spare; an empty asm makes the index a new value to the compiler at every call.
__device__ __forceinline__ int task_thread() {
  int t = (int)threadIdx.x;
#ifdef LMGPU_TEST_HOOKS
  asm volatile("" : "+v"(t));
#endif
  return t;
}

}  // namespace lmgpu
