// wave_sync.hpp -- the hand-off through LDS inside ONE wavefront.
#pragma once

// The block is one wavefront: its lanes run in lockstep and the LDS serves one wave's instructions in order, so a hand-off through LDS
// needs no s_barrier -- only a compiler fence.  (A __syncthreads() would also drain vmcnt(0), i.e. stall every phase on the record
// prefetches and P_k stores in flight.)
#define WSYNC()                                                  \
    do {                                                         \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   \
        __builtin_amdgcn_wave_barrier();                         \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   \
    } while (0)
