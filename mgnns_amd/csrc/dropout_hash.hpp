// Counter-based dropout masks shared by the training kernels (mha_train.hip, model_train.hip): element `idx` of site `site`
// is kept iff hash(seed, site, idx) >= rate, kept values are scaled by 1 / (1 - rate).  Nothing is stored to reproduce a
// mask: a second launch with the same seed draws the same one.  Site ids: include/mgnns_hip.h (MGNNS_DROP_*).
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

// splitmix64 finaliser of (seed, site, index) -> uniform in [0, 1) with 24 bits; kept iff u >= rate
__device__ __forceinline__ bool mg_keep(uint64_t seed, int site, uint64_t idx, float rate) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * ((((uint64_t)site) << 48) + idx + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (float)(uint32_t)(z >> 40) * (1.0f / 16777216.0f) >= rate;
}

__host__ __device__ inline float keep_scale(float rate) { return rate < 1.0f ? 1.0f / (1.0f - rate) : 0.0f; }
