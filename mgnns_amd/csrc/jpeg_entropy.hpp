// Baseline JPEG, entropy-decoding half: the derived tables the host parser builds (jpeg_parse.hpp) and the Huffman decoder of ONE
// independent segment -- a whole scan, or the stretch between two restart markers.  Plain C++17 without a HIP header: the same
// function body is the lane's loop of jpeg_entropy_kernel (jpeg_decode.hip) and what tools/dev/jpeg_host_check.cpp runs on the
// CPU under the sanitizers.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MG_HD __host__ __device__ __forceinline__
#else
#define MG_HD inline
#endif

// status word of a segment (one int32 per segment; ops.jpeg_decode turns a non-zero word into a ValueError)
enum { MG_JPEG_SEG_OK = 0, MG_JPEG_SEG_OUT_OF_DATA = 1, MG_JPEG_SEG_INVALID_CODE = 2, MG_JPEG_SEG_COEF_OVERFLOW = 3, MG_JPEG_SEG_BAD_RECORD = 4 };

constexpr int MG_JPEG_LOOK_BITS = 9;

// One Huffman table as the decoder reads it (1424 bytes).  A code of up to 9 bits is found with one look-up of the next 9 bits;
// longer ones walk maxcode[] as libjpeg's slow path does.
struct MgJpegHuff {
    uint16_t look[1 << MG_JPEG_LOOK_BITS];   // (code length << 8) | symbol for every 9-bit prefix of a code of <= 9 bits; 0 = none
    int32_t maxcode[18];                     // [l] = largest code of length l, -1 if there is none (l = 1..16)
    int32_t valoffset[18];                   // [l] = index into huffval of the first code of length l, minus that code
    uint8_t huffval[256];                    // the symbols in code order
};

// The tables of one file, by table id (11648 bytes).  Only the tables the scan refers to are filled, the rest is zero, so that two
// files with the same tables in use give the same bytes: a batch keeps one copy per distinct content.
struct MgJpegTables {
    uint8_t quant[4][64];                    // natural (row-major) order
    MgJpegHuff dc[4], ac[4];
};

struct MgJpegSegment {
    int ncomp, hs, vs;                       // 1 component, or 3 with Y sampled hs x vs and Cb = Cr = 1 x 1
    int mcux, mcu_total;                     // MCUs per row, MCUs of the image
    int mcu0, nmcu;                          // this segment's MCUs: [mcu0, mcu0 + nmcu), inside [0, mcu_total)
    int td[3], ta[3];                        // DC / AC table id per component (0..3)
};

// Decode one segment's bytes [p, end) into quantised coefficients, int16 [block][64] in natural order per component, at MCU-padded
// block counts (component 0: mcux * hs blocks per block row).  The workspace is zero beforehand; only non-zero AC coefficients
// and every DC are written, only into the segment's own blocks, and never at an index above 63.  Reads stay inside [p, end);
// past the end -- or past a marker, which a sound segment does not contain -- the reader feeds zero bits.  The loop runs one
// symbol per trip and at most 64 trips per block.  -> the segment's status word.
MG_HD int mg_jpeg_decode_segment(const uint8_t* p, const uint8_t* end, const MgJpegTables* T, const MgJpegSegment& g,
                                 int16_t* coef0, int16_t* coef1, int16_t* coef2) {
    static constexpr uint8_t NATURAL[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                            41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                            30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    const bool gray = g.ncomp == 1;
    const int ybl = gray ? 1 : g.hs * g.vs, bpm = gray ? 1 : ybl + 2;
    if (g.nmcu <= 0 || g.mcu0 < 0 || g.mcu0 > g.mcu_total - g.nmcu || g.mcux < 1 || (g.hs != 1 && g.hs != 2) || (g.vs != 1 && g.vs != 2))
        return MG_JPEG_SEG_BAD_RECORD;
    const MgJpegHuff* const dc0 = &T->dc[g.td[0] & 3], * const ac0 = &T->ac[g.ta[0] & 3];
    const MgJpegHuff* const dc1 = &T->dc[g.td[1] & 3], * const ac1 = &T->ac[g.ta[1] & 3];
    const MgJpegHuff* const dc2 = &T->dc[g.td[2] & 3], * const ac2 = &T->ac[g.ta[2] & 3];

    uint64_t acc = 0;        // the next nbits bits of the stream are its low bits
    int nbits = 0, pad = 0;  // pad: how many zero bits were fed past the end of the data; they are the lowest bits of acc
    int pred0 = 0, pred1 = 0, pred2 = 0;
    int status = MG_JPEG_SEG_OK;
    int mcu = g.mcu0, bi = 0, k = 0, c = 0;
    const int mcu_end = g.mcu0 + g.nmcu;
    auto block = [&](int mcu_, int bi_, int& c_) -> int16_t* {
        const int my = mcu_ / g.mcux, mx = mcu_ - my * g.mcux;
        if (bi_ < ybl) {
            c_ = 0;
            const int by = bi_ / (gray ? 1 : g.hs), bx = bi_ - by * (gray ? 1 : g.hs);
            const int h = gray ? 1 : g.hs, v = gray ? 1 : g.vs;
            return coef0 + ((size_t)(my * v + by) * (size_t)(g.mcux * h) + (size_t)(mx * h + bx)) * 64;
        }
        c_ = bi_ - ybl + 1;
        return (c_ == 1 ? coef1 : coef2) + (size_t)mcu_ * 64;
    };
    int16_t* blk = block(mcu, bi, c);
    // The next byte of [p, end).  Bytes come eight at a time, one aligned 8-byte load, wherever eight of them lie inside the segment
    // (a dependent byte load per byte is what a lane would otherwise wait for); the ends of the segment are read byte by byte.
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
        const MgJpegHuff* const H = k == 0 ? (c == 0 ? dc0 : (c == 1 ? dc1 : dc2)) : (c == 0 ? ac0 : (c == 1 ? ac1 : ac2));
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
            int pr = c == 0 ? pred0 : (c == 1 ? pred1 : pred2);
            pr = (int)((uint32_t)pr + (uint32_t)v);
            if (c == 0) pred0 = pr; else if (c == 1) pred1 = pr; else pred2 = pr;
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
        }
    }
    return nbits < pad ? MG_JPEG_SEG_OUT_OF_DATA : status;       // bits from beyond the data were consumed: that is the cause
}
