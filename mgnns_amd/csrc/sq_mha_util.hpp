// Helpers of the unit-queue attention cores -- sq_mha_bf16.hip, sq_mha32_bf16.hip and sq_mha_split_bf16.hip, each through a
// `using namespace mg_mha;` in its anonymous namespace: compile-time loops (also imgbank_bf16.hip's), the packed-weight stream
// through a buffer resource, LDS hand-over counters, the transposing four-value row reduction, the phase-trace stamp.
#pragma once
#include "common.hpp"

// In-kernel phase trace of a core (each behind its own build flag, off by default): s_memtime stamps of wave 0 / wave 4 of
// workgroups 0 and 129 at the phase boundaries, into `arr` = a __device__ unsigned long long [4][64] of the core's file.
#define MG_MHA_STAMP(arr, slot)                                                                                           \
    do {                                                                                                                  \
        if ((threadIdx.x & 255) == 0 && (blockIdx.x == 0 || blockIdx.x == 129) && blockIdx.y == 0 && (slot) < 64)         \
            arr[(blockIdx.x ? 2 : 0) + (threadIdx.x >> 8)][(slot)] = __builtin_amdgcn_s_memtime();                        \
    } while (0)

namespace mg_mha {

// compile-time loop: f(IC<0>{}), f(IC<1>{}), ... -- the index is a constant expression inside f (immediate offsets / counts of
// inline-asm instructions need one)
template <int N> struct IC { static constexpr int v = N; };
template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(IC<I>{});
        static_for<I + 1, N>(f);
    }
}

// Packed weights through a buffer resource: one VGPR (lane * 16) addresses every fragment, the fragment is selected by a
// wave-uniform byte offset in an SGPR.  (64-bit per-lane pointers for the two live weight streams cost sq_mha_bf16's 13-tile
// class enough registers to spill its head-pair loop state.)
struct WStream {
    __amdgpu_buffer_rsrc_t rsrc;
    int voff;                                   // lane * 16
};
__device__ __forceinline__ uint4 wfrag(const WStream& w, int soff) {
    return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(w.rsrc, w.voff, soff, 0));
}

// Sum over the four 16-lane rows of the wave for FOUR values at once (a transposing reduction): on return the rows of the
// result hold the row sums of [a, c, b, d] -- row 0: a, row 1: c, row 2: b, row 3: d.  v_permlane32_swap exchanges the upper
// half of its first operand with the lower half of its second, v_permlane16_swap the odd rows of the first with the even rows
// of the second, so one swap + one add folds TWO values by one level: 3 swaps + 3 adds for four tiles (the one-value form, both
// operands the same register, cost 2 swaps + 2 adds per tile).  Inline asm: both registers of a swap are read AND written (hipcc
// 7.2's builtin loses the second result here); the s_nop 1 on either side cover the VALU-write -> swap-read and swap-write ->
// VALU-read hazards, which the compiler's hazard recogniser does not see through an asm block.
__device__ __forceinline__ float rows4_sum4(float a, float b, float c, float d) {
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\tv_permlane32_swap_b32 %2, %3\n\ts_nop 1"
                 : "+v"(a), "+v"(b), "+v"(c), "+v"(d));      // a = [a.lo, b.lo], b = [a.hi, b.hi] (same for c, d)
    float ab = a + b, cd = c + d;                             // halves: [a: r0+r2, r1+r3 | b: r0+r2, r1+r3]
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1" : "+v"(ab), "+v"(cd));
    return ab + cd;                                           // rows: [a, c, b, d]
}

// Cross-wave hand-over inside a workgroup through LDS counters (no s_barrier).  LDS operations of a wave complete in order:
// lgkmcnt(0) in front of an arrival publishes this wave's LDS writes to whoever sees the count.
__device__ __forceinline__ int lds_arrive(int* ctr, int lane) {          // -> the count before this arrival (wave-uniform)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    int old = 0;
    if (lane == 0) old = __hip_atomic_fetch_add(ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return __builtin_amdgcn_readfirstlane(old);
}
__device__ __forceinline__ void lds_wait_ge(int* ctr, int target) {
    while (__builtin_amdgcn_readfirstlane(__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) < target)
        __builtin_amdgcn_s_sleep(1);
    asm volatile("" ::: "memory");
}

}  // namespace mg_mha
