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

// The forms of the decoder's loop.  SERIAL is mg_jpeg_decode_segment.  SCAN and WRITE walk one CHUNK of a segment for the split
// decoder (jpeg_split.hpp) from an entry state to the chunk's end: SCAN stores nothing and leaves its exit state, the blocks that
// ended on its way and the sums of the DC differences it read; WRITE stores what the serial decoder stores there.
enum { MG_JPEG_WALK_SERIAL = 0, MG_JPEG_WALK_SCAN = 1, MG_JPEG_WALK_WRITE = 2 };

// What two decoders of one stream have to agree on, packed: the raw position of the next unread bit (8 x the byte's offset from
// the segment's first byte + the bits of it already read; it never points at the 00 of a stuffed FF 00), the block's index in its
// MCU and the zigzag index.
constexpr uint64_t MG_JPEG_STATE_INVALID = ~0ull;
MG_HD uint64_t mg_jpeg_state(uint32_t bit, int bi, int k) { return (uint64_t)bit | (uint64_t)(uint32_t)bi << 32 | (uint64_t)(uint32_t)k << 40; }

struct MgJpegWalk {
    uint64_t entry;          // in: the state to start from (not MG_JPEG_STATE_INVALID)
    uint32_t limit;          // in: the chunk's end, a byte offset from the segment's first byte: a symbol that starts there ends the walk
    uint32_t block0;         // in, WRITE: the blocks of the segment that ended before the entry
    uint64_t exit;           // out, SCAN: the state at the chunk's end; invalid if the walk met an error or the end of the data
    uint32_t blocks;         // out, SCAN: blocks that ended on the way
    uint32_t failed;         // out, SCAN: 1 if the walk met an error.  It went on all the same: behind a wrong guess a walk falls into
                             // step again and its exit is the next lane's better guess, so an error must not end it; behind the TRUE
                             // walk's error nothing is written, which the carry step sees to
    uint32_t dc[3];          // in, WRITE: the predictors at the entry; out, SCAN: the sum of the DC differences read, per component
};

// The decoder's loop in its three forms; mg_jpeg_decode_segment below states what it reads and writes.  A chunk walk (w != null)
// ends at the first symbol whose first bit lies at or behind w->limit.  A walk that has been fed a byte from beyond the data is the
// segment's last: SCAN ends there with an invalid exit, WRITE runs on over zero bits until the MCUs are complete, as SERIAL does.
template <int MODE>
MG_HD int mg_jpeg_walk(const uint8_t* p, const uint8_t* end, const MgJpegTables* T, const MgJpegSegment& g, int16_t* coef0, int16_t* coef1,
                       int16_t* coef2, MgJpegWalk* w) {
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
    const uint8_t* const base = p;                 // (chunk walks) positions count from here
    uint32_t marks = 0;                            // (chunk walks) bit j: the byte fed j bytes ago was a stuffed FF, two raw bytes
    int skip = 0;                                  // (chunk walks) bits of the entry's byte that lie before the entry
    uint32_t ended = 0;                            // (SCAN) blocks that ended; the predictors, starting at zero, are the DC sums
    if constexpr (MODE != MG_JPEG_WALK_SERIAL) {
        if constexpr (MODE == MG_JPEG_WALK_SCAN) w->exit = MG_JPEG_STATE_INVALID, w->blocks = 0, w->failed = 0, w->dc[0] = w->dc[1] = w->dc[2] = 0;
        if (w->entry == MG_JPEG_STATE_INVALID) return MG_JPEG_SEG_OK;                // behind the segment's last walk: nothing
        const uint32_t bit = (uint32_t)w->entry;
        p = (size_t)(bit >> 3) < (size_t)(end - base) ? base + (bit >> 3) : end;
        skip = (int)(bit & 7u);
        bi = (int)((w->entry >> 32) & 0xFF), k = (int)((w->entry >> 40) & 63);
        if (bi >= bpm) bi = 0;
        if constexpr (MODE == MG_JPEG_WALK_WRITE) {
            mcu = g.mcu0 + (int)(w->block0 / (uint32_t)bpm);
            pred0 = (int)w->dc[0], pred1 = (int)w->dc[1], pred2 = (int)w->dc[2];
            if (mcu >= mcu_end) return MG_JPEG_SEG_OK;
        }
    }
    auto block = [&](int mcu_, int bi_, int& c_) -> int16_t* {
        if constexpr (MODE == MG_JPEG_WALK_SCAN) {                                   // no stores: the component alone
            c_ = bi_ < ybl ? 0 : bi_ - ybl + 1;
            return nullptr;
        }
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
    // one symbol per trip: at most 64 per block, and at least a bit each up to the chunk's end
    const long long max_symbols = MODE == MG_JPEG_WALK_SERIAL ? (long long)g.nmcu * bpm * 64
                                  : MODE == MG_JPEG_WALK_WRITE ? ((long long)g.nmcu * bpm - w->block0) * 64
                                                               : ((long long)w->limit + 16) * 8;

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
            if constexpr (MODE != MG_JPEG_WALK_SERIAL) marks = (marks << 1) | (uint32_t)(real && b == 0xFF);
        }
        if constexpr (MODE != MG_JPEG_WALK_SERIAL) {
            nbits -= skip;
            skip = 0;
            const uint32_t fed = (uint32_t)(p - base) - (uint32_t)cache_n;           // raw bytes taken from the segment
            if (pad != 0) {                                                          // beyond the data: this walk is the segment's last
                if constexpr (MODE == MG_JPEG_WALK_SCAN) break;
            } else if (fed >= w->limit) {
                // The byte that holds the next unread bit: the unread bits lie in the last `held` bytes fed, each one raw byte and
                // a stuffed FF two.
                const uint32_t held = (uint32_t)(nbits + 7) >> 3;
                const uint32_t at = fed - held - (uint32_t)__builtin_popcount(marks & ((1u << held) - 1u));
                if (at >= w->limit) {
                    if constexpr (MODE == MG_JPEG_WALK_SCAN) {
                        w->exit = mg_jpeg_state(at * 8u + ((8u - ((uint32_t)nbits & 7u)) & 7u), bi, k);
                        w->blocks = ended, w->failed = status != MG_JPEG_SEG_OK, w->dc[0] = (uint32_t)pred0, w->dc[1] = (uint32_t)pred1, w->dc[2] = (uint32_t)pred2;
                    }
                    break;
                }
            }
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
                if constexpr (MODE == MG_JPEG_WALK_SCAN) {       // a wrong guess, most likely: drop a bit and begin a block
                    nbits -= 1, k = 0;
                    continue;
                }
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
                if constexpr (MODE == MG_JPEG_WALK_SCAN) continue;                   // (the bits are read: begin a block)
                break;
            }
            int pr = c == 0 ? pred0 : (c == 1 ? pred1 : pred2);
            pr = (int)((uint32_t)pr + (uint32_t)v);
            if (c == 0) pred0 = pr; else if (c == 1) pred1 = pr; else pred2 = pr;
            if constexpr (MODE != MG_JPEG_WALK_SCAN) blk[0] = (int16_t)(uint16_t)(uint32_t)pr;
            k = 1;
        } else if (size == 0) {
            k = r == 15 ? k + 16 : 64;                                               // ZRL, or EOB
            if (k > 64) {
                status = MG_JPEG_SEG_COEF_OVERFLOW;
                if constexpr (MODE == MG_JPEG_WALK_SCAN) {
                    k = 0;
                    continue;
                }
                break;
            }
        } else {
            k += r;
            if (k > 63) {
                status = MG_JPEG_SEG_COEF_OVERFLOW;
                if constexpr (MODE == MG_JPEG_WALK_SCAN) {
                    k = 0;
                    continue;
                }
                break;
            }
            if constexpr (MODE != MG_JPEG_WALK_SCAN) blk[NATURAL[k]] = (int16_t)v;
            ++k;
        }
        if (k >= 64) {
            k = 0;
            if constexpr (MODE == MG_JPEG_WALK_SCAN) ++ended;
            if (++bi == bpm) {
                bi = 0;
                if constexpr (MODE != MG_JPEG_WALK_SCAN)
                    if (++mcu == mcu_end) break;
            }
            blk = block(mcu, bi, c);
        }
    }
    if constexpr (MODE == MG_JPEG_WALK_SCAN) return MG_JPEG_SEG_OK;                  // (errors met while scanning are no errors)
    return nbits < pad ? MG_JPEG_SEG_OUT_OF_DATA : status;       // bits from beyond the data were consumed: that is the cause
}

// Decode one segment's bytes [p, end) into quantised coefficients, int16 [block][64] in natural order per component, at MCU-padded
// block counts (component 0: mcux * hs blocks per block row).  The workspace is zero beforehand; only non-zero AC coefficients
// and every DC are written, only into the segment's own blocks, and never at an index above 63.  Reads stay inside [p, end);
// past the end -- or past a marker, which a sound segment does not contain -- the reader feeds zero bits.  The loop runs one
// symbol per trip and at most 64 trips per block.  -> the segment's status word.
MG_HD int mg_jpeg_decode_segment(const uint8_t* p, const uint8_t* end, const MgJpegTables* T, const MgJpegSegment& g,
                                 int16_t* coef0, int16_t* coef1, int16_t* coef2) {
    return mg_jpeg_walk<MG_JPEG_WALK_SERIAL>(p, end, T, g, coef0, coef1, coef2, nullptr);
}
