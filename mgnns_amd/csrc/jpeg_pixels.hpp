// Baseline JPEG, sample half: libjpeg's jidctint 8x8 inverse DCT ("islow"), the "fancy" chroma upsampling and YCbCr -> RGB, as
// functions that compile for host and device (jpeg_decode.hip's kernels; tools/dev/jpeg_host_check.cpp on the CPU).  Integer
// arithmetic throughout; sums and products are formed in uint32_t so that a corrupt file's huge coefficients wrap instead of
// overflowing a signed integer (a sound file's stay far inside 32 bits).
#pragma once
#include <stdint.h>

#include "jpeg_entropy.hpp"

// One 1-D pass of jidctint on eight inputs: CONST_BITS = 13, DESCALE(x, shift) = (x + (1 << (shift - 1))) >> shift.
MG_HD void mg_jpeg_idct8(const int32_t in[8], int shift, int32_t out[8]) {
    typedef uint32_t u;
    const u i0 = (u)in[0], i1 = (u)in[1], i2 = (u)in[2], i3 = (u)in[3], i4 = (u)in[4], i5 = (u)in[5], i6 = (u)in[6], i7 = (u)in[7];
    u z1 = (i2 + i6) * 4433u;
    u tmp2 = z1 - i6 * 15137u;
    u tmp3 = z1 + i2 * 6270u;
    u tmp0 = (i0 + i4) << 13;
    u tmp1 = (i0 - i4) << 13;
    const u tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = i7;
    tmp1 = i5;
    tmp2 = i3;
    tmp3 = i1;
    z1 = tmp0 + tmp3;
    u z2 = tmp1 + tmp2, z3 = tmp0 + tmp2, z4 = tmp1 + tmp3;
    const u z5 = (z3 + z4) * 9633u;
    tmp0 *= 2446u;
    tmp1 *= 16819u;
    tmp2 *= 25172u;
    tmp3 *= 12299u;
    z1 *= (u)-7373;
    z2 *= (u)-20995;
    z3 = z3 * (u)-16069 + z5;
    z4 = z4 * (u)-3196 + z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    const u r = 1u << (shift - 1);
    out[0] = (int32_t)(tmp10 + tmp3 + r) >> shift;
    out[7] = (int32_t)(tmp10 - tmp3 + r) >> shift;
    out[1] = (int32_t)(tmp11 + tmp2 + r) >> shift;
    out[6] = (int32_t)(tmp11 - tmp2 + r) >> shift;
    out[2] = (int32_t)(tmp12 + tmp1 + r) >> shift;
    out[5] = (int32_t)(tmp12 - tmp1 + r) >> shift;
    out[3] = (int32_t)(tmp13 + tmp0 + r) >> shift;
    out[4] = (int32_t)(tmp13 - tmp0 + r) >> shift;
}

// pass 1 of one column: dequantise coef[8 r + c] and transform down the column -> ws[r] (PASS1_BITS = 2 extra bits: shift 11)
MG_HD void mg_jpeg_idct_column(const int16_t* coef, const uint8_t* quant, int c, int32_t ws[8]) {
    int32_t in[8];
    for (int r = 0; r < 8; ++r) in[r] = (int32_t)coef[8 * r + c] * (int32_t)quant[8 * r + c];
    mg_jpeg_idct8(in, 11, ws);
}

// pass 2 of one row (shift 13 + 2 + 3 = 18), level shift and clamp -> 8 samples
MG_HD void mg_jpeg_idct_row(const int32_t ws[8], uint8_t out[8]) {
    int32_t o[8];
    mg_jpeg_idct8(ws, 18, o);
    for (int x = 0; x < 8; ++x) {
        const int32_t v = o[x] + 128;
        out[x] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
    }
}

// The chroma sample at full-resolution (x, y) of a plane with dw x dh real samples (pitch bytes per row), sampled 1 / hs by 1 / vs:
// libjpeg's "fancy" triangle filters.  Edges replicate the first / last REAL sample or row.  0 <= x < hs dw, 0 <= y < vs dh.
// replicate: the plane is at most two samples wide and its samples are to be repeated, not filtered, as libjpeg does for such planes
// (jdsample.c filters only where downsampled_width > 2).  The progressive decoder passes dw <= 2; the baseline decoder passes false
// and keeps the pixels it always gave for files of width 2..4 ("Progressive files").
MG_HD int mg_jpeg_chroma(const uint8_t* plane, int pitch, int dw, int dh, int hs, int vs, int x, int y, bool replicate = false) {
    if (hs == 1) return plane[(size_t)y * pitch + x];             // (vs == 1 too: 1x2 is not accepted)
    if (replicate) return plane[(size_t)(vs == 2 ? y >> 1 : y) * pitch + (x >> 1)];
    const int i = x >> 1, odd = x & 1;
    const int in = odd ? (i + 1 < dw ? i + 1 : dw - 1) : (i > 0 ? i - 1 : 0);       // the neighbour this output leans towards
    const bool edge = x == 0 || x == 2 * dw - 1;
    if (vs == 1) {
        const uint8_t* row = plane + (size_t)y * pitch;
        return edge ? row[i] : (3 * row[i] + row[in] + 1 + odd) >> 2;
    }
    const int r = y >> 1, lower = y & 1;
    const int rn = lower ? (r + 1 < dh ? r + 1 : dh - 1) : (r > 0 ? r - 1 : 0);
    const uint8_t* r0 = plane + (size_t)r * pitch, * r1 = plane + (size_t)rn * pitch;
    const int cs = 3 * r0[i] + r1[i], csn = 3 * r0[in] + r1[in];
    return edge ? (4 * cs + 8 - odd) >> 4 : (3 * cs + csn + 8 - odd) >> 4;
}

MG_HD void mg_jpeg_rgb(int y, int cb, int cr, uint8_t* rgb) {
    cb -= 128;
    cr -= 128;
    const int r = y + ((91881 * cr + 32768) >> 16);
    const int g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16);
    const int b = y + ((116130 * cb + 32768) >> 16);
    rgb[0] = (uint8_t)(r < 0 ? 0 : (r > 255 ? 255 : r));
    rgb[1] = (uint8_t)(g < 0 ? 0 : (g > 255 ? 255 : g));
    rgb[2] = (uint8_t)(b < 0 ? 0 : (b > 255 ? 255 : b));
}
