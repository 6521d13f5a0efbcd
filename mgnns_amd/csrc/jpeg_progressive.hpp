// Progressive JPEG (SOF2), entropy-decoding half: the Huffman decoder of ONE independent segment of ONE progressive scan -- a whole
// scan, or the stretch between two restart markers -- by the four procedures of T.81 Annex G (libjpeg's jdphuff.c): DC first, DC
// refinement, AC first, AC refinement.  Plain C++17 without a HIP header: the same function body is the lane's loop of
// jpeg_progressive_kernel (jpeg_decode.hip) and what tools/dev/jpeg_progressive_host_check.cpp runs on the CPU under the sanitizers.
// The bit reader is the baseline decoder's (jpeg_entropy.hpp): a 64-bit buffer, aligned eight-byte refills, FF 00 unstuffing, zero
// bits past the end or past a marker, a 9-bit look-ahead with the maxcode walk behind it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "jpeg_entropy.hpp"

// One segment of one scan.  A unit is an MCU in a scan of several components, and a single block in a scan of one component: such
// a scan walks ceil(w_c / 8) x ceil(h_c / 8) blocks in raster order, w_c = ceil(W h_c / h_max) -- not the MCU-padded counts, while
// the row stride of the coefficient workspace stays the MCU-padded one.
struct MgJpegProgSegment {
    int ncomp, hs, vs;                       // the frame: 1 component, or 3 with Y sampled hs x vs and Cb = Cr = 1 x 1
    int W, H, mcux, mcuy;
    int comps;                               // mask of the frame's components in this scan (bit c)
    int ss, se, ah, al;
    int unit0, nunits;                       // this segment's units: [unit0, unit0 + nunits), inside the scan's
};

// units of a whole scan; 0 for a record that is no scan
MG_HD long long mg_jpeg_prog_units(const MgJpegProgSegment& g) {
    const int c = g.comps;
    if (c != 1 && c != 2 && c != 4) return (long long)g.mcux * g.mcuy;
    const int h = c == 1 ? g.hs : 1, v = c == 1 ? g.vs : 1;
    const int wc = (g.W * h + g.hs - 1) / g.hs, hc = (g.H * v + g.vs - 1) / g.vs;
    return (long long)((wc + 7) / 8) * ((hc + 7) / 8);
}

// Decode one segment's bytes [p, end) into the int16 [block][64] natural-order workspace the baseline decoder fills (zero before
// the image's first scan).  dc0..dc2: the DC tables of components 0..2 (read by a DC first scan only, for the components of the
// scan), ac: the AC table (AC scans only).  Reads stay inside [p, end); a write goes only to blocks of the segment's own units, in
// the scan's components, at zigzag indices inside [ss, se] -- two segments that run at the same time differ in one of the three.  An
// AC refinement also READS its blocks whole, 16 bytes at a time, and looks only at its own band of what it read.  Every loop runs
// at most a count computed from the record.  -> the segment's status word.
MG_HD int mg_jpeg_decode_progressive_segment(const uint8_t* p, const uint8_t* end, const MgJpegHuff* dc0, const MgJpegHuff* dc1,
                                             const MgJpegHuff* dc2, const MgJpegHuff* ac, const MgJpegProgSegment& g, int16_t* coef0,
                                             int16_t* coef1, int16_t* coef2) {
    static constexpr uint8_t NATURAL[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                            41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                            30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    // zigzag index of every natural position (the inverse of NATURAL)
    static constexpr uint8_t ZIGZAG_OF[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                                              41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                                              46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};
    // ---- the record, re-checked ----
    const bool gray = g.ncomp == 1;
    if ((g.ncomp != 1 && g.ncomp != 3) || (g.hs != 1 && g.hs != 2) || (g.vs != 1 && g.vs != 2) || (gray && (g.hs != 1 || g.vs != 1)) ||
        (g.hs == 1 && g.vs == 2) || g.W < 1 || g.H < 1 || g.mcux != (g.W + 8 * g.hs - 1) / (8 * g.hs) ||
        g.mcuy != (g.H + 8 * g.vs - 1) / (8 * g.vs) || g.comps < 1 || g.comps > (gray ? 1 : 7))
        return MG_JPEG_SEG_BAD_RECORD;
    const bool dc = g.ss == 0, single = g.comps == 1 || g.comps == 2 || g.comps == 4;
    if (dc ? g.se != 0 : (g.ss < 1 || g.se < g.ss || g.se > 63 || !single)) return MG_JPEG_SEG_BAD_RECORD;
    if (g.al < 0 || g.al > 13 || (g.ah != 0 && g.ah != g.al + 1)) return MG_JPEG_SEG_BAD_RECORD;
    const long long scan_units = mg_jpeg_prog_units(g);
    if (g.nunits < 1 || g.unit0 < 0 || g.unit0 > scan_units - g.nunits) return MG_JPEG_SEG_BAD_RECORD;
    if (dc && g.ah == 0 && (((g.comps & 1) && !dc0) || ((g.comps & 2) && !dc1) || ((g.comps & 4) && !dc2))) return MG_JPEG_SEG_BAD_RECORD;
    if (!dc && !ac) return MG_JPEG_SEG_BAD_RECORD;

    // ---- where a block lies ----
    const int sc = g.comps == 2 ? 1 : (g.comps == 4 ? 2 : 0);                  // the component of a single-component scan
    const int bwc = sc == 0 ? ((g.W + 7) / 8) : (((g.W + g.hs - 1) / g.hs + 7) / 8);   // its block columns (Y: w_c = W)
    const int hs = g.hs, vs = g.vs, mcux = g.mcux;
    // (everything by value: a choice among three pointers captured by reference becomes a choice among their addresses, in scratch)
    auto block = [=](int unit, int c, int bi) -> int16_t* {
        const int h = c == 0 ? hs : 1, v = c == 0 ? vs : 1;
        int16_t* const base = c == 0 ? coef0 : (c == 1 ? coef1 : coef2);
        if (single) {
            const int by = unit / bwc, bx = unit - by * bwc;
            return base + ((size_t)by * (size_t)(mcux * h) + (size_t)bx) * 64;
        }
        const int my = unit / mcux, mx = unit - my * mcux;
        const int by = bi / h, bx = bi - by * h;
        return base + ((size_t)(my * v + by) * (size_t)(mcux * h) + (size_t)(mx * h + bx)) * 64;
    };

    // ---- the bit reader (jpeg_entropy.hpp's) ----
    uint64_t acc = 0;        // the next nbits bits of the stream are its low bits
    int nbits = 0, pad = 0;  // pad: how many zero bits were fed past the end of the data; they are the lowest bits of acc
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
    auto fill = [&]() {                                          // at least 57 bits
        while (nbits <= 56) {
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
    };
    auto get = [&](int n) -> int {                               // n = 0..16 bits; the caller has them
        const int v = (int)((uint32_t)(acc >> (nbits - n)) & ((1u << n) - 1u));
        nbits -= n;
        return v;
    };
    auto symbol = [&](const MgJpegHuff* H) -> int {              // at most 16 bits; -> -1 for no code
        const uint32_t peek = (uint32_t)(acc >> (nbits - 16)) & 0xFFFFu;
        const uint32_t e = H->look[peek >> (16 - MG_JPEG_LOOK_BITS)];
        int len = (int)(e >> 8), sym = (int)(e & 0xFF);
        if (e == 0) {
            len = MG_JPEG_LOOK_BITS + 1;
            while (len <= 16 && (int32_t)(peek >> (16 - len)) > H->maxcode[len]) ++len;
            if (len > 16) return -1;
            sym = H->huffval[((int32_t)(peek >> (16 - len)) + H->valoffset[len]) & 0xFF];
        }
        nbits -= len;
        return sym;
    };

    int status = MG_JPEG_SEG_OK;
    const int unit_end = g.unit0 + g.nunits;
    const int p1 = 1 << g.al;

    if (dc) {
        // ---- DC first / DC refinement: one block per trip ----
        const int first_c = (g.comps & 1) ? 0 : ((g.comps & 2) ? 1 : 2);
        const int ybl = g.hs * g.vs;
        int bpu = 0;                                             // blocks per unit
        if (single) bpu = 1;
        else bpu = ((g.comps & 1) ? ybl : 0) + ((g.comps & 2) ? 1 : 0) + ((g.comps & 4) ? 1 : 0);
        int pred0 = 0, pred1 = 0, pred2 = 0;
        int unit = g.unit0, c = first_c, bi = 0;
        const long long trips = (long long)g.nunits * bpu;
        for (long long it = 0; it < trips; ++it) {
            fill();
            int16_t* const blk = block(unit, c, bi);
            if (g.ah == 0) {
                const int s = symbol(c == 0 ? dc0 : (c == 1 ? dc1 : dc2));
                if (s < 0 || s > 15) {                           // no code, or a DC category above 15
                    status = MG_JPEG_SEG_INVALID_CODE;
                    break;
                }
                int v = get(s);
                if (s && v < (1 << (s - 1))) v -= (1 << s) - 1;  // extend()
                int pr = c == 0 ? pred0 : (c == 1 ? pred1 : pred2);
                pr = (int)((uint32_t)pr + (uint32_t)v);
                if (c == 0) pred0 = pr; else if (c == 1) pred1 = pr; else pred2 = pr;
                blk[0] = (int16_t)(uint16_t)((uint32_t)pr << g.al);
            } else if (get(1)) {
                blk[0] = (int16_t)(uint16_t)((uint32_t)(uint16_t)blk[0] | (uint32_t)p1);
            }
            // the next block: of this component, of the scan's next component, of the next unit
            const int nb = single ? 1 : (c == 0 ? ybl : 1);
            if (++bi == nb) {
                bi = 0;
                int nc = c + 1;
                while (nc < 3 && !((g.comps >> nc) & 1)) ++nc;
                if (single || nc >= 3) {
                    c = first_c;
                    ++unit;
                } else {
                    c = nc;
                }
            }
        }
        return nbits < pad ? MG_JPEG_SEG_OUT_OF_DATA : status;
    }

    const int band = g.se - g.ss + 1;
    if (g.ah == 0) {
        // ---- AC first: one symbol per trip; an end-of-band run skips whole blocks ----
        int unit = g.unit0, k = g.ss;
        int16_t* blk = block(unit, sc, 0);
        const long long trips = (long long)g.nunits * band + g.nunits;
        for (long long it = 0; it < trips; ++it) {
            fill();
            const int sym = symbol(ac);
            if (sym < 0) {
                status = MG_JPEG_SEG_INVALID_CODE;
                break;
            }
            const int r = sym >> 4, size = sym & 15;
            if (size) {
                int v = get(size);
                if (v < (1 << (size - 1))) v -= (1 << size) - 1;
                k += r;
                if (k > g.se) {
                    status = MG_JPEG_SEG_COEF_OVERFLOW;
                    break;
                }
                blk[NATURAL[k]] = (int16_t)(uint16_t)((uint32_t)v << g.al);
                ++k;
            } else if (r == 15) {
                k += 16;
                if (k > g.se + 1) {
                    status = MG_JPEG_SEG_COEF_OVERFLOW;
                    break;
                }
            } else {                                             // EOBr: this block and (1 << r) + bits - 1 more end here
                long long run = (1 << r) + get(r);
                if (run > unit_end - unit) run = unit_end - unit;          // clipped to the segment's remaining blocks
                unit += (int)run - 1;
                k = g.se + 1;
            }
            if (k > g.se) {
                k = g.ss;
                if (++unit >= unit_end) break;
                blk = block(unit, sc, 0);
            }
        }
        return nbits < pad ? MG_JPEG_SEG_OUT_OF_DATA : status;
    }

    // ---- AC refinement.  A trip reads at most one symbol (16 + 14 bits) and then at most 24 correction bits, one for every
    // coefficient of the band that is already non-zero, up to the symbol's target: the r-th coefficient that is still zero (a
    // new +-(1 << al)), 16 zero ones (ZRL) or the end of the band (EOB, and every block of an EOB run).  Which coefficients of the
    // block are non-zero is read once per block, 128 bytes in eight loads, into a mask in zigzag order; the walk then loads only
    // the coefficients it corrects.
    uint64_t bandmask = 0;
    for (int k = g.ss; k <= g.se; ++k) bandmask |= 1ull << k;
    auto nonzero = [&](const int16_t* blk) -> uint64_t {
        uint64_t w[16];
        __builtin_memcpy(w, __builtin_assume_aligned(blk, 16), 128);
        uint64_t nz = 0;
#if defined(__clang__)
#pragma unroll                                                   // (constant shifts: w[] stays in registers)
#endif
        for (int n = 0; n < 64; ++n) nz |= (uint64_t)(((w[n >> 2] >> (16 * (n & 3))) & 0xFFFFu) != 0) << ZIGZAG_OF[n];
        return nz & bandmask;
    };
    int unit = g.unit0, k = g.ss, r = 0, newv = 0;
    long long eobrun = 0;
    bool walking = false, to_end = false;                        // to_end: the walk's target is the end of the band
    int16_t* blk = block(unit, sc, 0);
    uint64_t nz = nonzero(blk);
    const long long trips = (long long)g.nunits * (band + 4) + g.nunits;
    for (long long it = 0; it < trips; ++it) {
        fill();
        if (!walking) {
            newv = 0;
            if (eobrun > 0) {                                    // a block inside an end-of-band run: corrections only
                r = 64, to_end = true;
            } else {
                const int sym = symbol(ac);
                if (sym < 0) {
                    status = MG_JPEG_SEG_INVALID_CODE;
                    break;
                }
                r = sym >> 4, to_end = false;
                const int size = sym & 15;
                if (size) {
                    if (size != 1) {                             // a refinement adds one bit: any other size is no code of this scan
                        status = MG_JPEG_SEG_INVALID_CODE;
                        break;
                    }
                    newv = get(1) ? p1 : -p1;
                } else if (r != 15) {                            // EOBr: this block and (1 << r) + bits - 1 more
                    eobrun = (1 << r) + get(r);
                    if (eobrun > unit_end - unit) eobrun = unit_end - unit;    // clipped to the segment's remaining blocks
                    r = 64, to_end = true;
                }
            }
            walking = true;
        }
        bool reached = false;                                    // the target, a coefficient that is still zero, is at k
        int budget = 24;
        for (int step = 0; step < 64; ++step) {                  // (every step passes a coefficient or leaves)
            const uint64_t rem = k <= 63 ? nz >> k : 0;
            const int z = rem ? __builtin_ctzll(rem) : g.se + 1 - k;           // zero coefficients from k up to the next non-zero one
            if (r < z) {
                k += r;
                reached = true;
                break;
            }
            r -= z;
            k += z;
            if (k > g.se || budget == 0) break;
            --budget;
            if (get(1)) {
                int16_t* const q = blk + NATURAL[k];
                const int v = *q;
                if ((v & p1) == 0) *q = (int16_t)(v >= 0 ? v + p1 : v - p1);
            }
            ++k;
        }
        if (!reached && k <= g.se) continue;                     // this trip's correction bits are used up: the walk goes on
        walking = false;
        if (reached) {
            if (newv) blk[NATURAL[k]] = (int16_t)newv;
            ++k;
        } else if (!to_end) {                                    // a new coefficient or a ZRL whose target lies beyond se
            status = MG_JPEG_SEG_COEF_OVERFLOW;
            break;
        }
        if (k > g.se) {
            if (eobrun > 0) --eobrun;
            k = g.ss;
            if (++unit >= unit_end) break;
            blk = block(unit, sc, 0);
            nz = nonzero(blk);
        }
    }
    return nbits < pad ? MG_JPEG_SEG_OUT_OF_DATA : status;
}
