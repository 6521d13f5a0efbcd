// fp32 <-> bf16 conversions of every kernel, one definition each (the bf16x8 fragment type is in common.hpp).  A new kernel
// takes its conversion from here.  Two forms of round-to-nearest-even exist and a call site's choice is part of its kernel's
// instruction stream:
//   instruction form  mg_bf16x2 / mg_bf16: ONE v_cvt_pk_bf16_f32 (there is no builtin for it on gfx950) for one or two
//                     values -- the hot paths, where every VALU instruction of a latency-bound phase or an epilogue shows;
//   integer form      mg_bf16_rne / mg_bf16_rne_finite: five VALU operations per value -- set-up kernels written before the
//                     instruction form was in use (weight packs, casts), kept as they are.
#pragma once
#include "common.hpp"

// two values -> packed bf16x2: bf16(a) | bf16(b) << 16
__device__ __forceinline__ unsigned int mg_bf16x2(float a, float b) {
    unsigned int r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ unsigned short mg_bf16(float x) {
    unsigned int r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %1" : "=v"(r) : "v"(x));
    return (unsigned short)r;
}
// bf16 bits in the low 16 of h (anything above is shifted out) -> fp32, exact
__device__ __forceinline__ float mg_bf16_f32(unsigned int h) { return __uint_as_float(h << 16); }

// integer form, FINITE inputs: the rounding carry of a NaN with a large payload runs into the exponent and the sign
__device__ __forceinline__ unsigned int mg_bf16_rne_finite(float x) {
    unsigned int u = __float_as_uint(x);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return u >> 16;
}
// integer form, any input: a NaN stays a quiet NaN
__device__ __forceinline__ unsigned short mg_bf16_rne(float x) {
    const unsigned int u = __float_as_uint(x);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (unsigned short)((u >> 16) | 0x40u);
    return (unsigned short)mg_bf16_rne_finite(x);
}

// Split-bf16 operands: an fp32 x travels as hi = bf16(x), lo = bf16(x - hi) (x - hi is exact in fp32), instruction form.
__device__ __forceinline__ void mg_split(float x, unsigned short& hi, unsigned short& lo) {
    const unsigned short h = mg_bf16(x);
    hi = h;
    lo = mg_bf16(x - mg_bf16_f32(h));
}
// ... into hi[idx], lo[idx]
__device__ __forceinline__ void mg_split_store(unsigned short* hi, unsigned short* lo, int idx, float x) {
    const unsigned short h = mg_bf16(x);
    hi[idx] = h;
    lo[idx] = mg_bf16(x - mg_bf16_f32(h));
}
// ... of two values, packed like mg_bf16x2
__device__ __forceinline__ void mg_split2(float a, float b, unsigned int& hi, unsigned int& lo) {
    const unsigned int h = mg_bf16x2(a, b);
    hi = h;
    lo = mg_bf16x2(a - __uint_as_float(h << 16), b - __uint_as_float(h & 0xFFFF0000u));
}
// ... of 8 values -> the hi and lo 16-byte chunks
__device__ __forceinline__ void mg_split8(const float (&x)[8], uint4& hi, uint4& lo) {
    unsigned int h[4], l[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) mg_split2(x[2 * q], x[2 * q + 1], h[q], l[q]);
    hi = uint4{h[0], h[1], h[2], h[3]};
    lo = uint4{l[0], l[1], l[2], l[3]};
}
