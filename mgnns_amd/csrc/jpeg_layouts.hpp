// Other component layouts ("Other component layouts"): the entropy decoder of ONE independent segment of a scan that
// interleaves 1, 3 or 4 components with any sampling factors h, v in 1..4 (at most 10 blocks per MCU), the upsampling forms of
// libjpeg-turbo's jdsample.c and the colour models of jdcolor.c / Pillow's convert('RGB').  Plain C++17 without a HIP header: the
// same functions are the bodies of jpeg_decode.hip's layout kernels and what tools/dev/jpeg_layouts_host_check.cpp runs on the CPU
// under the sanitizers.  The reader and the symbol loop are mg_jpeg_decode_segment's (jpeg_entropy.hpp); what differs is the walk
// over the MCU's block list, the sum of h_i v_i blocks, with up to four predictors and four coefficient planes.  A segment is
// decoded by one lane from its first byte to its last: these segments are never split over lanes (jpeg_split.hpp knows the
// baseline block list only), so a restart-free file of these layouts decodes at the one-lane rate.
#pragma once
#include <stdint.h>

#include "jpeg_entropy.hpp"
#include "jpeg_pixels.hpp"

// the colour models, as jpeg_parse.hpp numbers them
enum { MG_JPEG_MODEL_GRAY = 0, MG_JPEG_MODEL_YCC = 1, MG_JPEG_MODEL_RGB = 2, MG_JPEG_MODEL_CMYK = 3, MG_JPEG_MODEL_YCCK = 4 };

// Per-component fields are packed, a nibble (h, v) or two bits (table ids) per component, so that nothing here indexes an array
// with a run-time index: the lane's state stays in registers.
struct MgJpegLayoutSegment {
    int ncomp;                               // 1, 3 or 4
    uint32_t h, v;                           // nibble c: the sampling factors of component c, 1..4 (one component: 1 x 1)
    uint32_t td, ta;                         // bits 2c, 2c + 1: DC / AC table id of component c
    int mcux, mcu_total;                     // MCUs per row, MCUs of the image
    int mcu0, nmcu;                          // this segment's MCUs: [mcu0, mcu0 + nmcu), inside [0, mcu_total)
};

MG_HD int mg_jpeg_nibble(uint32_t packed, int c) { return (int)((packed >> (4 * c)) & 15u); }

// blocks per MCU of a layout, 0 if it is none the decoder takes
MG_HD int mg_jpeg_layout_mcu_blocks(int ncomp, uint32_t h, uint32_t v) {
    if (ncomp != 1 && ncomp != 3 && ncomp != 4) return 0;
    int blocks = 0, hmax = 1, vmax = 1;
    for (int c = 0; c < ncomp; ++c) {
        const int hc = mg_jpeg_nibble(h, c), vc = mg_jpeg_nibble(v, c);
        if (hc < 1 || hc > 4 || vc < 1 || vc > 4) return 0;
        hmax = hc > hmax ? hc : hmax, vmax = vc > vmax ? vc : vmax;
        blocks += hc * vc;
    }
    for (int c = 0; c < ncomp; ++c)
        if (hmax % mg_jpeg_nibble(h, c) || vmax % mg_jpeg_nibble(v, c)) return 0;
    if (ncomp == 1 && blocks != 1) return 0;
    return blocks <= 10 ? blocks : 0;
}

// Decode one segment's bytes [p, end) into quantised coefficients, int16 [block][64] in natural order per component, component c
// at mcux h_c blocks per block row and mcuy v_c block rows.  mg_jpeg_decode_segment's guarantees: the workspace is zero beforehand;
// only non-zero AC coefficients and every DC are written, only into blocks of the segment's own MCUs and never at an index above
// 63; reads stay inside [p, end), past the end -- or past a marker -- the reader feeds zero bits; one symbol per trip and at most 64
// trips per block, so at most nmcu * blocks * 64 trips; a record that is no layout, or whose MCU range is not inside the image,
// is MG_JPEG_SEG_BAD_RECORD and nothing is written.  -> the segment's status word, one of the five.
MG_HD int mg_jpeg_decode_layout_segment(const uint8_t* p, const uint8_t* end, const MgJpegTables* T, const MgJpegLayoutSegment& g,
                                        int16_t* coef0, int16_t* coef1, int16_t* coef2, int16_t* coef3) {
    static constexpr uint8_t NATURAL[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                            41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                            30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    const int bpm = mg_jpeg_layout_mcu_blocks(g.ncomp, g.h, g.v);
    if (bpm == 0 || g.nmcu <= 0 || g.mcu0 < 0 || g.mcu0 > g.mcu_total - g.nmcu || g.mcux < 1) return MG_JPEG_SEG_BAD_RECORD;
    // the MCU's block list, six bits per block: component, column and row of the block inside the component's share of the MCU
    uint64_t list = 0;
    {
        int at = 0;
        for (int c = 0; c < g.ncomp; ++c)
            for (int by = 0; by < mg_jpeg_nibble(g.v, c); ++by)
                for (int bx = 0; bx < mg_jpeg_nibble(g.h, c); ++bx, ++at) list |= (uint64_t)(uint32_t)(c | bx << 2 | by << 4) << (6 * at);
    }
    uint64_t acc = 0;        // the next nbits bits of the stream are its low bits
    int nbits = 0, pad = 0;  // pad: how many zero bits were fed past the end of the data; they are the lowest bits of acc
    int pred0 = 0, pred1 = 0, pred2 = 0, pred3 = 0;
    int status = MG_JPEG_SEG_OK;
    int mcu = g.mcu0, bi = 0, k = 0, c = 0;
    const int mcu_end = g.mcu0 + g.nmcu;
    auto block = [&](int mcu_, int bi_, int& c_) -> int16_t* {
        const int d = (int)((list >> (6 * bi_)) & 63u);
        c_ = d & 3;
        const int bx = (d >> 2) & 3, by = d >> 4, h = mg_jpeg_nibble(g.h, c_), v = mg_jpeg_nibble(g.v, c_);
        const int my = mcu_ / g.mcux, mx = mcu_ - my * g.mcux;
        int16_t* const base = c_ == 0 ? coef0 : (c_ == 1 ? coef1 : (c_ == 2 ? coef2 : coef3));
        return base + ((size_t)(my * v + by) * (size_t)(g.mcux * h) + (size_t)(mx * h + bx)) * 64;
    };
    int16_t* blk = block(mcu, bi, c);
    const MgJpegHuff* dct = &T->dc[(g.td >> (2 * c)) & 3u], * act = &T->ac[(g.ta >> (2 * c)) & 3u];
    // the next byte of [p, end): eight at a time wherever eight of them lie inside the segment, as mg_jpeg_walk reads them
    uint64_t cache = 0;
    int cache_n = 0;
    auto next_byte = [&](uint32_t& b) -> bool {
        if (cache_n == 0) {
            if (p >= end) return false;
            if ((reinterpret_cast<uintptr_t>(p) & 7u) == 0 && end - p >= 8) {
                __builtin_memcpy(&cache, __builtin_assume_aligned(p, 8), 8);      // little-endian: the first byte is the lowest
                cache_n = 8;
            } else {
                cache = *p;
                cache_n = 1;
            }
            p += cache_n;
        }
        b = (uint32_t)(cache & 0xFF);
        cache >>= 8;
        --cache_n;
        return true;
    };
    const long long max_symbols = (long long)g.nmcu * bpm * 64;
    for (long long it = 0; it < max_symbols; ++it) {
        while (nbits <= 56) {                                    // refill: at least 57 bits, a symbol takes at most 16 + 15
            uint32_t b = 0, b2 = 0;
            bool real = false;
            if (next_byte(b)) {
                if (b != 0xFF || (next_byte(b2) && b2 == 0)) {   // an ordinary byte, or a stuffed FF
                    real = true;
                } else {
                    p = end;                                     // a marker, or FF as the last byte: the data ends here
                    cache_n = 0;
                }
            }
            if (!real) {
                b = 0;
                pad = pad < (1 << 30) ? pad + 8 : pad;
            }
            acc = (acc << 8) | b;
            nbits += 8;
        }
        const MgJpegHuff* const H = k == 0 ? dct : act;
        const uint32_t peek = (uint32_t)(acc >> (nbits - 16)) & 0xFFFFu;
        const uint32_t e = H->look[peek >> (16 - MG_JPEG_LOOK_BITS)];
        int len = (int)(e >> 8), sym = (int)(e & 0xFF);
        if (e == 0) {
            len = MG_JPEG_LOOK_BITS + 1;
            while (len <= 16 && (int32_t)(peek >> (16 - len)) > H->maxcode[len]) ++len;
            if (len > 16) {
                status = MG_JPEG_SEG_INVALID_CODE;
                break;
            }
            sym = H->huffval[((int32_t)(peek >> (16 - len)) + H->valoffset[len]) & 0xFF];
        }
        nbits -= len;
        const int r = sym >> 4, size = sym & 15;
        int v = (int)((uint32_t)(acc >> (nbits - size)) & ((1u << size) - 1u));     // size = 0: nothing
        nbits -= size;
        if (size && v < (1 << (size - 1))) v -= (1 << size) - 1;                    // extend()
        if (k == 0) {
            if (r) {
                status = MG_JPEG_SEG_INVALID_CODE;                                   // a DC category above 15
                break;
            }
            int pr = c == 0 ? pred0 : (c == 1 ? pred1 : (c == 2 ? pred2 : pred3));
            pr = (int)((uint32_t)pr + (uint32_t)v);
            if (c == 0) pred0 = pr; else if (c == 1) pred1 = pr; else if (c == 2) pred2 = pr; else pred3 = pr;
            blk[0] = (int16_t)(uint16_t)(uint32_t)pr;
            k = 1;
        } else if (size == 0) {
            k = r == 15 ? k + 16 : 64;                                               // ZRL, or EOB
            if (k > 64) {
                status = MG_JPEG_SEG_COEF_OVERFLOW;
                break;
            }
        } else {
            k += r;
            if (k > 63) {
                status = MG_JPEG_SEG_COEF_OVERFLOW;
                break;
            }
            blk[NATURAL[k]] = (int16_t)v;
            ++k;
        }
        if (k >= 64) {
            k = 0;
            if (++bi == bpm) {
                bi = 0;
                if (++mcu == mcu_end) break;
            }
            blk = block(mcu, bi, c);
            dct = &T->dc[(g.td >> (2 * c)) & 3u], act = &T->ac[(g.ta >> (2 * c)) & 3u];
        }
    }
    return nbits < pad ? MG_JPEG_SEG_OUT_OF_DATA : status;       // bits from beyond the data were consumed: that is the cause
}

// The sample at full-resolution (x, y) of a component plane with dw x dh real samples (pitch bytes per row) that is sampled 1 / hr
// by 1 / vr of the largest: libjpeg-turbo's jdsample.c with fancy upsampling.
//   1 x 1            the sample itself
//   2 x 1, 2 x 2     the triangle filters of mg_jpeg_chroma; a plane at most two samples wide is replicated
//   1 x 2            out[2r] = (3 p[r] + p[r-1] + 1) >> 2, out[2r+1] = (3 p[r] + p[r+1] + 2) >> 2 down the column, the first and the
//                    last REAL row repeated at the edges; at every width
//   other ratios     replication
MG_HD int mg_jpeg_layout_sample(const uint8_t* plane, int pitch, int dw, int dh, int hr, int vr, int x, int y) {
    if (hr == 1 && vr == 1) return plane[(size_t)y * pitch + x];
    if (hr == 2 && vr <= 2) return mg_jpeg_chroma(plane, pitch, dw, dh, 2, vr, x, y, dw <= 2);
    if (hr == 1 && vr == 2) {
        const int r = y >> 1, lower = y & 1;
        const int rn = lower ? (r + 1 < dh ? r + 1 : dh - 1) : (r > 0 ? r - 1 : 0);
        return (3 * plane[(size_t)r * pitch + x] + plane[(size_t)rn * pitch + x] + 1 + lower) >> 2;
    }
    return plane[(size_t)(y / vr) * pitch + x / hr];
}

// Four samples of one pixel -> Pillow's RGB.  GRAY repeats s0, YCC is mg_jpeg_rgb, RGB is stored as it is.  CMYK: Pillow reads the
// four bytes as inverted ink (CMYK;I) and converts with integer arithmetic, out_c = clip8(nk - muldiv255(in_c, nk)) with
// in_c = 255 - s_c, nk = 255 - K = s3 and muldiv255(a, b) = (t + (t >> 8)) >> 8, t = a b + 128.  YCCK first becomes CMYK as
// jdcolor.c's ycck_cmyk_convert does it: C, M, Y = 255 - (R, G, B) of (s0, s1, s2), K = s3.
MG_HD void mg_jpeg_layout_rgb(int model, int s0, int s1, int s2, int s3, uint8_t* rgb) {
    if (model == MG_JPEG_MODEL_GRAY) {
        rgb[0] = rgb[1] = rgb[2] = (uint8_t)s0;
    } else if (model == MG_JPEG_MODEL_YCC) {
        mg_jpeg_rgb(s0, s1, s2, rgb);
    } else if (model == MG_JPEG_MODEL_RGB) {
        rgb[0] = (uint8_t)s0, rgb[1] = (uint8_t)s1, rgb[2] = (uint8_t)s2;
    } else {
        int ink[3] = {s0, s1, s2};
        if (model == MG_JPEG_MODEL_YCCK) {
            uint8_t t[3];
            mg_jpeg_rgb(s0, s1, s2, t);
            ink[0] = 255 - t[0], ink[1] = 255 - t[1], ink[2] = 255 - t[2];
        }
        for (int c = 0; c < 3; ++c) {
            const int t = (255 - ink[c]) * s3 + 128;
            const int o = s3 - ((t + (t >> 8)) >> 8);
            rgb[c] = (uint8_t)(o < 0 ? 0 : (o > 255 ? 255 : o));
        }
    }
}
