// Baseline JPEG, host half: the marker parser.  Plain C++17 without a HIP header (it also compiles with the host compiler alone:
// tools/dev/jpeg_host_check.cpp); exported from the library as mgnns_jpeg_parse, which makes no GPU call.  Every read is checked
// against the file's length; a file that is malformed, or that the GPU decoder does not cover, gets a reason code.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "jpeg_entropy.hpp"

// reason codes (info[MG_JPEG_I_REASON]); info[MG_JPEG_I_DETAIL] holds what was found (a marker, a count, a byte offset)
enum {
    MG_JPEG_OK = 0,
    MG_JPEG_NOT_JPEG = 1,          // no SOI at the start
    MG_JPEG_MALFORMED = 2,         // a segment runs past the end of the file, or contradicts another
    MG_JPEG_UNSUPPORTED_SOF = 3,   // progressive (SOF2) or another SOFn; detail = the marker
    MG_JPEG_ARITHMETIC = 4,        // SOF9..15 or DAC
    MG_JPEG_PRECISION = 5,         // 12-bit samples (detail 12) or 16-bit quantisation tables (detail 16)
    MG_JPEG_COMPONENTS = 6,        // neither 1 nor 3 components (CMYK / YCCK: 4)
    MG_JPEG_ADOBE_TRANSFORM = 7,   // Adobe APP14 with transform 0 on three components (RGB, not YCbCr)
    MG_JPEG_RGB_IDS = 8,           // component ids 'R','G','B'
    MG_JPEG_SAMPLING = 9,          // sampling factors other than 1x1 / 2x1 / 2x2 for Y with 1x1 chroma
    MG_JPEG_SCANS = 10,            // more than one scan, or a scan that does not interleave all components
    MG_JPEG_DNL = 11,              // the height comes in a DNL segment
    MG_JPEG_EXTENT = 12,           // width or height outside 1..max_extent
    MG_JPEG_MISSING_TABLES = 13,   // the scan refers to a table no segment defined; detail = the component
};

// fields of info[MG_JPEG_INFO_INTS]
enum {
    MG_JPEG_I_REASON = 0, MG_JPEG_I_DETAIL, MG_JPEG_I_WIDTH, MG_JPEG_I_HEIGHT, MG_JPEG_I_NCOMP, MG_JPEG_I_HS, MG_JPEG_I_VS,
    MG_JPEG_I_TQ = 7,              // 3: quantisation-table id per component
    MG_JPEG_I_TD = 10,             // 3: DC table id per component
    MG_JPEG_I_TA = 13,             // 3: AC table id per component
    MG_JPEG_I_RI = 16,             // restart interval in MCUs, 0 = none
    MG_JPEG_I_RESTARTS = 17,       // RSTn markers found in the entropy-coded data
    MG_JPEG_I_NSEG = 18,           // independent segments of the scan: ceil(nMCU / Ri), or 1
    MG_JPEG_I_MCUX = 19, MG_JPEG_I_MCUY = 20,
    MG_JPEG_INFO_INTS = 24,
};

namespace mgjpeg {

struct Reader {
    const uint8_t* d;
    size_t n;
    bool has(size_t pos, size_t k) const { return pos <= n && k <= n - pos; }
    int u16(size_t pos) const { return (d[pos] << 8) | d[pos + 1]; }
};

// libjpeg's jdhuff.c derivation: canonical codes from the 16 counts; -> false if the counts are no prefix code
inline bool derive(const uint8_t* bits, const uint8_t* vals, int nvals, MgJpegHuff* h) {
    memset(h, 0, sizeof(*h));
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        const int cnt = bits[l - 1];
        if (code + cnt > (1 << l)) return false;
        if (cnt) {
            h->valoffset[l] = k - code;
            for (int i = 0; i < cnt; ++i, ++k, ++code) {
                if (l <= MG_JPEG_LOOK_BITS) {
                    const int first = code << (MG_JPEG_LOOK_BITS - l);
                    for (int j = 0; j < (1 << (MG_JPEG_LOOK_BITS - l)); ++j) h->look[first + j] = (uint16_t)((l << 8) | vals[k]);
                }
            }
            h->maxcode[l] = code - 1;
        } else {
            h->maxcode[l] = -1;
        }
        code <<= 1;
    }
    h->maxcode[0] = h->maxcode[17] = -1;
    if (k != nvals) return false;
    memcpy(h->huffval, vals, (size_t)nvals);
    return true;
}

}  // namespace mgjpeg

// Parse one file.  info: MG_JPEG_INFO_INTS int32 (above); range: the entropy-coded data's [begin, end) byte offsets; seg: [seg_cap][2]
// byte ranges of the scan's independent segments (as many as fit; info[NSEG] says how many there are -- call again with a larger
// buffer if it is more than seg_cap); tables: the file's tables in use.  Segment j covers MCUs [j Ri, (j+1) Ri).  Restart markers are
// found by scanning for FF D0..D7; a sound file has NSEG - 1 of them.  With fewer, the last segments get an empty byte range; with
// more, the surplus is ignored: either way the decoder ends those segments with a status word, never out of range.
// Returns the reason code (also in info[0]); everything but info[0..1] is meaningful only for MG_JPEG_OK.
inline int mg_jpeg_parse(const uint8_t* data, size_t n, int max_extent, int32_t* info, int64_t* range, int64_t* seg, size_t seg_cap,
                         MgJpegTables* tables) {
    using namespace mgjpeg;
    const Reader R{data, n};
    memset(info, 0, sizeof(int32_t) * MG_JPEG_INFO_INTS);
    memset(tables, 0, sizeof(*tables));
    range[0] = range[1] = 0;
    auto refuse = [&](int reason, long long detail) {
        info[MG_JPEG_I_REASON] = reason;
        info[MG_JPEG_I_DETAIL] = (int32_t)(detail > 0x7fffffffLL ? 0x7fffffffLL : detail);
        return reason;
    };
    if (n < 2 || data[0] != 0xFF || data[1] != 0xD8) return refuse(MG_JPEG_NOT_JPEG, 0);

    uint8_t quant[4][64];
    uint8_t hbits[2][4][16], hvals[2][4][256];
    int hcount[2][4];
    bool have_q[4] = {false, false, false, false}, have_h[2][4] = {{false, false, false, false}, {false, false, false, false}};
    bool have_frame = false;
    int width = 0, height = 0, ncomp = 0, comp_id[3] = {0, 0, 0}, comp_h[3] = {1, 1, 1}, comp_v[3] = {1, 1, 1}, comp_tq[3] = {0, 0, 0};
    int td[3] = {0, 0, 0}, ta[3] = {0, 0, 0}, ri = 0, adobe = -1;
    static const uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                       41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                       30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    size_t pos = 2;
    for (;;) {
        if (!R.has(pos, 2) || data[pos] != 0xFF) return refuse(MG_JPEG_MALFORMED, (long long)pos);
        while (pos + 1 < n && data[pos + 1] == 0xFF) ++pos;                  // fill bytes
        if (!R.has(pos, 2)) return refuse(MG_JPEG_MALFORMED, (long long)pos);
        const int m = data[pos + 1];
        pos += 2;
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;    // stand-alone markers
        if (m == 0xD9) return refuse(MG_JPEG_MALFORMED, (long long)pos);     // EOI before any scan
        if (!R.has(pos, 2)) return refuse(MG_JPEG_MALFORMED, (long long)pos);
        const int ln = R.u16(pos);
        if (ln < 2 || !R.has(pos, (size_t)ln)) return refuse(MG_JPEG_MALFORMED, (long long)pos);
        const size_t body = pos + 2, end = pos + (size_t)ln;
        if (m == 0xDB) {
            size_t p = body;
            while (p < end) {
                const int pq = data[p] >> 4, tq = data[p] & 15;
                if (pq != 0) return refuse(MG_JPEG_PRECISION, 16);
                if (tq > 3 || p + 65 > end) return refuse(MG_JPEG_MALFORMED, (long long)p);
                for (int k = 0; k < 64; ++k) quant[tq][ZIGZAG[k]] = data[p + 1 + k];
                have_q[tq] = true;
                p += 65;
            }
        } else if (m == 0xC4) {
            size_t p = body;
            while (p < end) {
                if (p + 17 > end) return refuse(MG_JPEG_MALFORMED, (long long)p);
                const int tc = data[p] >> 4, th = data[p] & 15;
                int cnt = 0;
                for (int i = 0; i < 16; ++i) cnt += data[p + 1 + i];
                if (tc > 1 || th > 3 || cnt > 256 || p + 17 + (size_t)cnt > end) return refuse(MG_JPEG_MALFORMED, (long long)p);
                int code = 0;
                for (int l = 1; l <= 16; ++l) {
                    code += data[p + l];
                    if (code > (1 << l)) return refuse(MG_JPEG_MALFORMED, (long long)p);
                    code <<= 1;
                }
                memcpy(hbits[tc][th], data + p + 1, 16);
                memcpy(hvals[tc][th], data + p + 17, (size_t)cnt);
                hcount[tc][th] = cnt;
                have_h[tc][th] = true;
                p += 17 + (size_t)cnt;
            }
        } else if (m == 0xDD) {
            if (ln != 4) return refuse(MG_JPEG_MALFORMED, (long long)pos);
            ri = R.u16(body);
        } else if (m == 0xCC || (m >= 0xC9 && m <= 0xCF)) {
            return refuse(MG_JPEG_ARITHMETIC, m);
        } else if (m == 0xC1 || m == 0xC2 || m == 0xC3 || m == 0xC5 || m == 0xC6 || m == 0xC7 || m == 0xC8) {
            return refuse(MG_JPEG_UNSUPPORTED_SOF, m);
        } else if (m == 0xC0) {
            if (have_frame || ln < 8) return refuse(MG_JPEG_MALFORMED, (long long)pos);
            const int prec = data[body], nf = data[body + 5];
            height = R.u16(body + 1);
            width = R.u16(body + 3);
            if (prec != 8) return refuse(MG_JPEG_PRECISION, prec);
            if (ln != 8 + 3 * nf) return refuse(MG_JPEG_MALFORMED, (long long)pos);
            if (nf != 1 && nf != 3) return refuse(MG_JPEG_COMPONENTS, nf);
            if (height == 0) return refuse(MG_JPEG_DNL, 0);
            if (width < 1 || width > max_extent || height > max_extent) return refuse(MG_JPEG_EXTENT, width > max_extent ? width : height);
            ncomp = nf;
            for (int i = 0; i < nf; ++i) {
                comp_id[i] = data[body + 6 + 3 * i];
                comp_h[i] = data[body + 7 + 3 * i] >> 4;
                comp_v[i] = data[body + 7 + 3 * i] & 15;
                comp_tq[i] = data[body + 8 + 3 * i];
            }
            if (nf == 3 && comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B') return refuse(MG_JPEG_RGB_IDS, 0);
            for (int i = 0; i < nf; ++i)
                if (comp_tq[i] > 3) return refuse(MG_JPEG_MALFORMED, (long long)pos);
            const int hv = comp_h[0] * 16 + comp_v[0];
            if (nf == 1) {
                if (hv != 0x11) return refuse(MG_JPEG_SAMPLING, hv);
            } else if ((hv != 0x11 && hv != 0x21 && hv != 0x22) || comp_h[1] != 1 || comp_v[1] != 1 || comp_h[2] != 1 || comp_v[2] != 1) {
                return refuse(MG_JPEG_SAMPLING, hv);
            }
            have_frame = true;
        } else if (m == 0xDC) {
            return refuse(MG_JPEG_DNL, 0);
        } else if (m == 0xEE && ln >= 14 && memcmp(data + body, "Adobe", 5) == 0) {
            adobe = data[body + 11];
        } else if (m == 0xDA) {
            if (!have_frame) return refuse(MG_JPEG_MALFORMED, (long long)pos);
            const int ns = ln >= 3 ? data[body] : 0;
            if (ns != ncomp) return refuse(MG_JPEG_SCANS, ns);
            if (ln != 6 + 2 * ns) return refuse(MG_JPEG_MALFORMED, (long long)pos);
            for (int i = 0; i < ns; ++i) {
                if (data[body + 1 + 2 * i] != comp_id[i]) return refuse(MG_JPEG_MALFORMED, (long long)pos);
                td[i] = data[body + 2 + 2 * i] >> 4;
                ta[i] = data[body + 2 + 2 * i] & 15;
                if (td[i] > 3 || ta[i] > 3) return refuse(MG_JPEG_MALFORMED, (long long)pos);
            }
            if (data[body + 1 + 2 * ns] != 0 || data[body + 2 + 2 * ns] != 63 || data[body + 3 + 2 * ns] != 0)
                return refuse(MG_JPEG_MALFORMED, (long long)pos);
            if (adobe == 0 && ns == 3) return refuse(MG_JPEG_ADOBE_TRANSFORM, 0);
            for (int i = 0; i < ns; ++i)
                if (!have_q[comp_tq[i]] || !have_h[0][td[i]] || !have_h[1][ta[i]]) return refuse(MG_JPEG_MISSING_TABLES, i);
            pos = end;
            break;
        }
        pos = end;
    }

    // the entropy-coded data: up to the first marker that is neither a stuffed FF, a fill byte nor RSTn
    const int hs = comp_h[0], vs = comp_v[0];
    const int mcux = (width + 8 * hs - 1) / (8 * hs), mcuy = (height + 8 * vs - 1) / (8 * vs);
    const long long nmcu = (long long)mcux * mcuy;
    const long long nseg = ri ? (nmcu + ri - 1) / ri : 1;
    const size_t begin = pos;
    size_t i = pos, seg_begin = pos;
    long long found = 0;
    auto put = [&](long long j, size_t b, size_t e) {
        if (j < nseg && (size_t)j < seg_cap) {
            seg[2 * j] = (int64_t)b;
            seg[2 * j + 1] = (int64_t)e;
        }
    };
    for (;;) {
        while (i < n && data[i] != 0xFF) ++i;
        if (i + 1 >= n) {
            i = n;
            break;
        }
        const int b = data[i + 1];
        if (b == 0) {
            i += 2;
        } else if (b == 0xFF) {
            i += 1;
        } else if (b >= 0xD0 && b <= 0xD7) {
            put(found, seg_begin, i);
            ++found;
            i += 2;
            seg_begin = i;
        } else {
            break;
        }
    }
    const size_t ecs_end = i;
    put(found, seg_begin, ecs_end);
    for (long long j = found + 1; j < nseg; ++j) put(j, ecs_end, ecs_end);
    // what follows: another scan or DNL is refused; anything else (EOI, nothing, rubbish) ends the file
    while (i + 1 < n && data[i] == 0xFF) {
        const int b = data[i + 1];
        if (b == 0xFF) {
            ++i;
            continue;
        }
        if (b == 0xD9) break;
        if (b == 0xDA) return refuse(MG_JPEG_SCANS, 2);
        if (b == 0xDC) return refuse(MG_JPEG_DNL, 0);
        if (i + 4 > n) break;
        i += 2 + (size_t)R.u16(i + 2);
    }

    for (int c = 0; c < ncomp; ++c) {
        memcpy(tables->quant[comp_tq[c]], quant[comp_tq[c]], 64);
        if (!mgjpeg::derive(hbits[0][td[c]], hvals[0][td[c]], hcount[0][td[c]], &tables->dc[td[c]]) ||
            !mgjpeg::derive(hbits[1][ta[c]], hvals[1][ta[c]], hcount[1][ta[c]], &tables->ac[ta[c]]))
            return refuse(MG_JPEG_MALFORMED, c);
    }
    info[MG_JPEG_I_WIDTH] = width;
    info[MG_JPEG_I_HEIGHT] = height;
    info[MG_JPEG_I_NCOMP] = ncomp;
    info[MG_JPEG_I_HS] = hs;
    info[MG_JPEG_I_VS] = vs;
    for (int c = 0; c < 3; ++c) {
        info[MG_JPEG_I_TQ + c] = comp_tq[c];
        info[MG_JPEG_I_TD + c] = td[c];
        info[MG_JPEG_I_TA + c] = ta[c];
    }
    info[MG_JPEG_I_RI] = ri;
    info[MG_JPEG_I_RESTARTS] = (int32_t)(found > 0x7fffffffLL ? 0x7fffffffLL : found);
    info[MG_JPEG_I_NSEG] = (int32_t)nseg;
    info[MG_JPEG_I_MCUX] = mcux;
    info[MG_JPEG_I_MCUY] = mcuy;
    range[0] = (int64_t)begin;
    range[1] = (int64_t)ecs_end;
    return MG_JPEG_OK;
}

// ---- progressive files (SOF2) ---------------------------------------------------------------------------------------------------
// further reason codes, of mg_jpeg_parse_progressive alone
enum {
    MG_JPEG_INCOMPLETE_PROGRESSION = 14,   // at EOI / the end of the file a coefficient has not reached Al = 0; detail = 64 c + k
    MG_JPEG_ILLEGAL_PROGRESSION = 15,      // Ss / Se / Ah / Al contradict T.81 G.1.1.1.1 or the scans before; detail = the scan
    MG_JPEG_TOO_MANY_SCANS = 16,           // more than MG_JPEG_MAX_SCANS scans
};
// further fields of info[] (the baseline fields TQ / TD / TA / RI / RESTARTS stay zero: they are per scan here; NSEG counts the
// segments of all scans)
enum { MG_JPEG_I_NSCANS = 21, MG_JPEG_I_NTABLES = 22, MG_JPEG_I_NLEVELS = 23 };
// fields of one scan record, int64 scan[MG_JPEG_SCAN_INTS]
enum {
    MG_JPEG_S_NS = 0,                      // components in the scan
    MG_JPEG_S_COMPS = 1,                   // mask of the frame's components in it (bit c)
    MG_JPEG_S_SS = 2, MG_JPEG_S_SE, MG_JPEG_S_AH, MG_JPEG_S_AL,
    MG_JPEG_S_RI = 6,                      // the restart interval in force at its SOS, in units (MCUs, or blocks of its one component)
    MG_JPEG_S_LEVEL = 7,
    MG_JPEG_S_DC = 8,                      // 3: index into the table pool of the frame component's DC table, -1 = none read
    MG_JPEG_S_AC = 11,                     // index of the AC table, -1 = none read
    MG_JPEG_S_SEG0 = 12, MG_JPEG_S_NSEG,   // its segments in seg[]
    MG_JPEG_S_UNITS = 14,                  // units of the whole scan
    MG_JPEG_S_BEGIN = 15, MG_JPEG_S_END,   // [begin, end) of its entropy-coded data
    MG_JPEG_S_RESTARTS = 17,               // RSTn markers found in it
    MG_JPEG_SCAN_INTS = 18,
};
constexpr int MG_JPEG_MAX_SCANS = 32;
constexpr int MG_JPEG_POOL_TABLES = 3 * MG_JPEG_MAX_SCANS;     // no file needs more: a scan reads at most three tables

// Parse one progressive file: SOF2, 8 bit, Huffman, the baseline decoder's component layouts, any legal progression script of at
// most 32 scans with DHT / DQT / DRI between them.  A file that is not SOF2 gets the reason mg_jpeg_parse gives it (a baseline
// file: MG_JPEG_UNSUPPORTED_SOF with detail 0xC0 -- parse it with mg_jpeg_parse).
//  info   as mg_jpeg_parse, with the fields above.
//  scan   [MG_JPEG_MAX_SCANS][MG_JPEG_SCAN_INTS] int64, in file order.  The LEVEL of a scan is 0 if no earlier scan touches a
//         (component, coefficient) it touches, else 1 + the largest level among those that do; an AC scan also counts as touching
//         what the component's first DC scan did (T.81 orders them so).  Scans of one level write different int16 elements.
//  seg    [seg_cap][4] int64: begin, end (bytes), first unit, units of every independent segment, scan after scan; as many as fit
//         (info[NSEG] says how many there are).  With fewer restart markers than the interval asks for, the last segments are empty.
//  pool   [MG_JPEG_POOL_TABLES] MgJpegHuff: the distinct tables the scans read; info[NTABLES] of them are filled, the rest is zero.
//  quant  [3][64]: per component, in natural order, the quantisation table in force at the component's first scan.
// After the first scan, anything that cannot be read as a marker segment ends the file, as EOI does.
inline int mg_jpeg_parse_progressive(const uint8_t* data, size_t n, int max_extent, int32_t* info, int64_t* scan, int64_t* seg,
                                     size_t seg_cap, MgJpegHuff* pool, uint8_t* quant_out) {
    using namespace mgjpeg;
    const Reader R{data, n};
    memset(info, 0, sizeof(int32_t) * MG_JPEG_INFO_INTS);
    memset(scan, 0, sizeof(int64_t) * MG_JPEG_MAX_SCANS * MG_JPEG_SCAN_INTS);
    memset(pool, 0, sizeof(MgJpegHuff) * MG_JPEG_POOL_TABLES);
    memset(quant_out, 0, 3 * 64);
    auto refuse = [&](int reason, long long detail) {
        info[MG_JPEG_I_REASON] = reason;
        info[MG_JPEG_I_DETAIL] = (int32_t)(detail > 0x7fffffffLL ? 0x7fffffffLL : detail);
        return reason;
    };
    if (n < 2 || data[0] != 0xFF || data[1] != 0xD8) return refuse(MG_JPEG_NOT_JPEG, 0);

    uint8_t quant[4][64];
    uint8_t hbits[2][4][16], hvals[2][4][256];
    int hcount[2][4], hpool[2][4];                   // hpool: where the table in force lies in the pool, -1 = not derived yet
    bool have_q[4] = {false, false, false, false}, have_h[2][4] = {{false, false, false, false}, {false, false, false, false}};
    bool have_frame = false, latched[3] = {false, false, false};
    int width = 0, height = 0, ncomp = 0, comp_id[3] = {0, 0, 0}, comp_h[3] = {1, 1, 1}, comp_v[3] = {1, 1, 1}, comp_tq[3] = {0, 0, 0};
    int ri = 0, adobe = -1, nscans = 0, ntables = 0, nlevels = 0;
    int bits_left[3][64], level_of[3][64], dc_level[3] = {-1, -1, -1};      // Al a coefficient stands at (-1: never sent); last level
    for (int c = 0; c < 3; ++c)
        for (int k = 0; k < 64; ++k) bits_left[c][k] = level_of[c][k] = -1;
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 4; ++b) hpool[a][b] = -1, hcount[a][b] = 0;
    long long nseg_total = 0;
    static const uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                       41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                       30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    // the table (tc, th) in force, as a pool index: derived once, shared with an earlier table of the same content; -1 = no prefix code
    auto pooled = [&](int tc, int th) -> int {
        if (hpool[tc][th] >= 0) return hpool[tc][th];
        if (ntables >= MG_JPEG_POOL_TABLES) return -1;
        MgJpegHuff* const h = pool + ntables;
        if (!derive(hbits[tc][th], hvals[tc][th], hcount[tc][th], h)) {
            memset(h, 0, sizeof(*h));
            return -1;
        }
        for (int i = 0; i < ntables; ++i)
            if (memcmp(pool + i, h, sizeof(*h)) == 0) {
                memset(h, 0, sizeof(*h));
                return hpool[tc][th] = i;
            }
        return hpool[tc][th] = ntables++;
    };
    size_t pos = 2;
    for (;;) {
        // ---- the next marker segment; after the first scan, what cannot be read ends the file ----
        if (!R.has(pos, 2) || data[pos] != 0xFF) {
            if (nscans) break;
            return refuse(MG_JPEG_MALFORMED, (long long)pos);
        }
        while (pos + 1 < n && data[pos + 1] == 0xFF) ++pos;                  // fill bytes
        if (!R.has(pos, 2)) {
            if (nscans) break;
            return refuse(MG_JPEG_MALFORMED, (long long)pos);
        }
        const int m = data[pos + 1];
        pos += 2;
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;    // stand-alone markers
        if (m == 0xD9) {
            if (nscans) break;
            return refuse(MG_JPEG_MALFORMED, (long long)pos);                // EOI before any scan
        }
        if (!R.has(pos, 2) || R.u16(pos) < 2 || !R.has(pos, (size_t)R.u16(pos))) {
            if (nscans) break;
            return refuse(MG_JPEG_MALFORMED, (long long)pos);
        }
        const int ln = R.u16(pos);
        const size_t body = pos + 2, end = pos + (size_t)ln;
        if (m == 0xDB) {
            size_t p = body;
            while (p < end) {
                const int pq = data[p] >> 4, tq = data[p] & 15;
                if (pq != 0) return refuse(MG_JPEG_PRECISION, 16);
                if (tq > 3 || p + 65 > end) return refuse(MG_JPEG_MALFORMED, (long long)p);
                for (int k = 0; k < 64; ++k) quant[tq][ZIGZAG[k]] = data[p + 1 + k];
                have_q[tq] = true;
                p += 65;
            }
        } else if (m == 0xC4) {
            size_t p = body;
            while (p < end) {
                if (p + 17 > end) return refuse(MG_JPEG_MALFORMED, (long long)p);
                const int tc = data[p] >> 4, th = data[p] & 15;
                int cnt = 0;
                for (int i = 0; i < 16; ++i) cnt += data[p + 1 + i];
                if (tc > 1 || th > 3 || cnt > 256 || p + 17 + (size_t)cnt > end) return refuse(MG_JPEG_MALFORMED, (long long)p);
                int code = 0;
                for (int l = 1; l <= 16; ++l) {
                    code += data[p + l];
                    if (code > (1 << l)) return refuse(MG_JPEG_MALFORMED, (long long)p);
                    code <<= 1;
                }
                memcpy(hbits[tc][th], data + p + 1, 16);
                memcpy(hvals[tc][th], data + p + 17, (size_t)cnt);
                hcount[tc][th] = cnt;
                have_h[tc][th] = true;
                hpool[tc][th] = -1;
                p += 17 + (size_t)cnt;
            }
        } else if (m == 0xDD) {
            if (ln != 4) return refuse(MG_JPEG_MALFORMED, (long long)pos);
            ri = R.u16(body);
        } else if (m == 0xCC || (m >= 0xC9 && m <= 0xCF)) {
            return refuse(MG_JPEG_ARITHMETIC, m);
        } else if (m == 0xC0 || m == 0xC1 || m == 0xC3 || m == 0xC5 || m == 0xC6 || m == 0xC7 || m == 0xC8) {
            return refuse(MG_JPEG_UNSUPPORTED_SOF, m);
        } else if (m == 0xC2) {
            if (have_frame || ln < 8) return refuse(MG_JPEG_MALFORMED, (long long)pos);
            const int prec = data[body], nf = data[body + 5];
            height = R.u16(body + 1);
            width = R.u16(body + 3);
            if (prec != 8) return refuse(MG_JPEG_PRECISION, prec);
            if (ln != 8 + 3 * nf) return refuse(MG_JPEG_MALFORMED, (long long)pos);
            if (nf != 1 && nf != 3) return refuse(MG_JPEG_COMPONENTS, nf);
            if (height == 0) return refuse(MG_JPEG_DNL, 0);
            if (width < 1 || width > max_extent || height > max_extent) return refuse(MG_JPEG_EXTENT, width > max_extent ? width : height);
            ncomp = nf;
            for (int i = 0; i < nf; ++i) {
                comp_id[i] = data[body + 6 + 3 * i];
                comp_h[i] = data[body + 7 + 3 * i] >> 4;
                comp_v[i] = data[body + 7 + 3 * i] & 15;
                comp_tq[i] = data[body + 8 + 3 * i];
            }
            if (nf == 3 && comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B') return refuse(MG_JPEG_RGB_IDS, 0);
            for (int i = 0; i < nf; ++i)
                if (comp_tq[i] > 3) return refuse(MG_JPEG_MALFORMED, (long long)pos);
            const int hv = comp_h[0] * 16 + comp_v[0];
            if (nf == 1) {
                if (hv != 0x11) return refuse(MG_JPEG_SAMPLING, hv);
            } else if ((hv != 0x11 && hv != 0x21 && hv != 0x22) || comp_h[1] != 1 || comp_v[1] != 1 || comp_h[2] != 1 || comp_v[2] != 1) {
                return refuse(MG_JPEG_SAMPLING, hv);
            }
            have_frame = true;
        } else if (m == 0xDC) {
            return refuse(MG_JPEG_DNL, 0);
        } else if (m == 0xEE && ln >= 14 && memcmp(data + body, "Adobe", 5) == 0) {
            adobe = data[body + 11];
        } else if (m == 0xDA) {
            if (!have_frame) return refuse(MG_JPEG_MALFORMED, (long long)pos);
            if (nscans == MG_JPEG_MAX_SCANS) return refuse(MG_JPEG_TOO_MANY_SCANS, nscans + 1);
            const int ns = ln >= 3 ? data[body] : 0;
            if (ns < 1 || ns > ncomp || ln != 6 + 2 * ns) return refuse(MG_JPEG_MALFORMED, (long long)pos);
            int sc_comp[3] = {0, 0, 0}, td[3] = {0, 0, 0}, ta[3] = {0, 0, 0}, mask = 0;
            for (int i = 0, c = 0; i < ns; ++i, ++c) {                       // the frame's components, in the frame's order
                while (c < ncomp && comp_id[c] != data[body + 1 + 2 * i]) ++c;
                if (c >= ncomp) return refuse(MG_JPEG_MALFORMED, (long long)pos);
                sc_comp[i] = c;
                mask |= 1 << c;
                td[i] = data[body + 2 + 2 * i] >> 4;
                ta[i] = data[body + 2 + 2 * i] & 15;
                if (td[i] > 3 || ta[i] > 3) return refuse(MG_JPEG_MALFORMED, (long long)pos);
            }
            const int ss = data[body + 1 + 2 * ns], se = data[body + 2 + 2 * ns], ah = data[body + 3 + 2 * ns] >> 4, al = data[body + 3 + 2 * ns] & 15;
            if (adobe == 0 && ncomp == 3) return refuse(MG_JPEG_ADOBE_TRANSFORM, 0);
            // T.81 G.1.1.1.1, and the scans before this one
            bool legal = ss == 0 ? se == 0 : (ss <= se && se <= 63 && ns == 1);
            if (ah != 0 && al != ah - 1) legal = false;
            if (al > 13) legal = false;
            for (int i = 0; legal && i < ns; ++i) {
                const int c = sc_comp[i];
                if (ss != 0 && bits_left[c][0] < 0) legal = false;           // AC before the component's DC
                for (int k = ss; k <= se; ++k)
                    if (bits_left[c][k] < 0 ? ah != 0 : (ah == 0 || ah != bits_left[c][k])) legal = false;
            }
            if (!legal) return refuse(MG_JPEG_ILLEGAL_PROGRESSION, nscans);
            int64_t* const S = scan + (size_t)nscans * MG_JPEG_SCAN_INTS;
            for (int c = 0; c < 3; ++c) S[MG_JPEG_S_DC + c] = -1;
            S[MG_JPEG_S_AC] = -1;
            int level = 0;
            for (int i = 0; i < ns; ++i) {
                const int c = sc_comp[i];
                if (!latched[c]) {                                           // the quantisation table in force at its first scan
                    if (!have_q[comp_tq[c]]) return refuse(MG_JPEG_MISSING_TABLES, c);
                    memcpy(quant_out + 64 * c, quant[comp_tq[c]], 64);
                    latched[c] = true;
                }
                if (ah == 0) {                                               // a refinement of DC reads no table
                    const int tc = ss == 0 ? 0 : 1, th = ss == 0 ? td[i] : ta[i];
                    if (!have_h[tc][th]) return refuse(MG_JPEG_MISSING_TABLES, c);
                    const int at = pooled(tc, th);
                    if (at < 0) return refuse(MG_JPEG_MALFORMED, c);
                    S[ss == 0 ? MG_JPEG_S_DC + c : MG_JPEG_S_AC] = at;
                } else if (ss != 0) {
                    if (!have_h[1][ta[i]]) return refuse(MG_JPEG_MISSING_TABLES, c);
                    const int at = pooled(1, ta[i]);
                    if (at < 0) return refuse(MG_JPEG_MALFORMED, c);
                    S[MG_JPEG_S_AC] = at;
                }
                if (ss != 0 && dc_level[c] + 1 > level) level = dc_level[c] + 1;
                for (int k = ss; k <= se; ++k)
                    if (level_of[c][k] + 1 > level) level = level_of[c][k] + 1;
            }
            for (int i = 0; i < ns; ++i) {
                const int c = sc_comp[i];
                if (ss == 0 && dc_level[c] < 0) dc_level[c] = level;
                for (int k = ss; k <= se; ++k) bits_left[c][k] = al, level_of[c][k] = level;
            }
            if (level + 1 > nlevels) nlevels = level + 1;
            // units: MCUs, or the blocks of the one component
            const int hs = comp_h[0], vs = comp_v[0];
            long long units;
            if (ns > 1) {
                units = (long long)((width + 8 * hs - 1) / (8 * hs)) * ((height + 8 * vs - 1) / (8 * vs));
            } else {
                const int c = sc_comp[0], h = comp_h[c], v = comp_v[c];
                const int wc = (width * h + hs - 1) / hs, hc = (height * v + vs - 1) / vs;
                units = (long long)((wc + 7) / 8) * ((hc + 7) / 8);
            }
            const long long nseg = ri ? (units + ri - 1) / ri : 1;
            // the entropy-coded data: up to the first marker that is neither a stuffed FF, a fill byte nor RSTn
            size_t i = end, seg_begin = end;
            long long found = 0;
            auto put = [&](long long j, size_t b, size_t e) {
                if (j < nseg && (size_t)(nseg_total + j) < seg_cap) {
                    int64_t* const g = seg + 4 * (size_t)(nseg_total + j);
                    g[0] = (int64_t)b, g[1] = (int64_t)e;
                    g[2] = ri ? j * ri : 0;
                    g[3] = ri ? (units - j * ri < ri ? units - j * ri : ri) : units;
                }
            };
            for (;;) {
                while (i < n && data[i] != 0xFF) ++i;
                if (i + 1 >= n) {
                    i = n;
                    break;
                }
                const int b = data[i + 1];
                if (b == 0) {
                    i += 2;
                } else if (b == 0xFF) {
                    i += 1;
                } else if (b >= 0xD0 && b <= 0xD7) {
                    put(found, seg_begin, i);
                    ++found;
                    i += 2;
                    seg_begin = i;
                } else {
                    break;
                }
            }
            put(found, seg_begin, i);
            for (long long j = found + 1; j < nseg; ++j) put(j, i, i);
            S[MG_JPEG_S_NS] = ns, S[MG_JPEG_S_COMPS] = mask, S[MG_JPEG_S_SS] = ss, S[MG_JPEG_S_SE] = se, S[MG_JPEG_S_AH] = ah, S[MG_JPEG_S_AL] = al;
            S[MG_JPEG_S_RI] = ri, S[MG_JPEG_S_LEVEL] = level, S[MG_JPEG_S_SEG0] = nseg_total, S[MG_JPEG_S_NSEG] = nseg, S[MG_JPEG_S_UNITS] = units;
            S[MG_JPEG_S_BEGIN] = (int64_t)end, S[MG_JPEG_S_END] = (int64_t)i, S[MG_JPEG_S_RESTARTS] = found;
            nseg_total += nseg;
            if (nseg_total > 0x7fffffffLL) return refuse(MG_JPEG_MALFORMED, (long long)pos);
            ++nscans;
            pos = i;
            continue;
        }
        pos = end;
    }
    for (int c = 0; c < ncomp; ++c)
        for (int k = 0; k < 64; ++k)
            if (bits_left[c][k] != 0) return refuse(MG_JPEG_INCOMPLETE_PROGRESSION, 64 * c + k);
    info[MG_JPEG_I_WIDTH] = width;
    info[MG_JPEG_I_HEIGHT] = height;
    info[MG_JPEG_I_NCOMP] = ncomp;
    info[MG_JPEG_I_HS] = comp_h[0];
    info[MG_JPEG_I_VS] = comp_v[0];
    info[MG_JPEG_I_NSEG] = (int32_t)nseg_total;
    info[MG_JPEG_I_MCUX] = (width + 8 * comp_h[0] - 1) / (8 * comp_h[0]);
    info[MG_JPEG_I_MCUY] = (height + 8 * comp_v[0] - 1) / (8 * comp_v[0]);
    info[MG_JPEG_I_NSCANS] = nscans;
    info[MG_JPEG_I_NTABLES] = ntables;
    info[MG_JPEG_I_NLEVELS] = nlevels;
    return MG_JPEG_OK;
}

// ---- other component layouts ("Other component layouts") -----------------------------------------------------------
// further reason codes, of mg_jpeg_parse_layout alone
enum {
    MG_JPEG_FRACTIONAL_SAMPLING = 17,      // a sampling factor that is no integral fraction of the largest (libjpeg fails on it too); detail = h v
    MG_JPEG_SAMPLING_RANGE = 18,           // a sampling factor outside 1..4 (detail = h v), or more than 10 blocks per MCU (detail = the count)
};
// the colour model of the components, by libjpeg's default_decompress_parms
enum { MG_JPEG_COLOUR_GRAY = 0, MG_JPEG_COLOUR_YCC = 1, MG_JPEG_COLOUR_RGB = 2, MG_JPEG_COLOUR_CMYK = 3, MG_JPEG_COLOUR_YCCK = 4 };
// fields of info[MG_JPEG_LAYOUT_INFO_INTS]; 0..4 are REASON, DETAIL, WIDTH, HEIGHT, NCOMP as above
enum {
    MG_JPEG_L_HMAX = 5, MG_JPEG_L_VMAX = 6,
    MG_JPEG_L_H = 7, MG_JPEG_L_V = 11,     // 4 each: the sampling factors per component (a one-component file: 1, whatever it says)
    MG_JPEG_L_TQ = 15, MG_JPEG_L_TD = 19, MG_JPEG_L_TA = 23,       // 4 each: table ids per component
    MG_JPEG_L_RI = 27, MG_JPEG_L_RESTARTS = 28, MG_JPEG_L_NSEG = 29, MG_JPEG_L_MCUX = 30, MG_JPEG_L_MCUY = 31,
    MG_JPEG_L_COLOUR = 32,                 // MG_JPEG_COLOUR_*
    MG_JPEG_L_SOF = 33,                    // 0xC0 or 0xC1
    MG_JPEG_L_BLOCKS = 34,                 // blocks per MCU: the sum of h v over the components
    MG_JPEG_LAYOUT_INFO_INTS = 40,
};
constexpr int MG_JPEG_MAX_MCU_BLOCKS = 10;                     // T.81 B.2.3

// Parse one file of SOF0 or SOF1, 8 bit, Huffman, one scan that interleaves all of its 1, 3 or 4 components, each sampled h x v
// with h, v in 1..4 that divide the largest, at most 10 blocks per MCU.  The segment logic, range, seg and tables are
// mg_jpeg_parse's; an MCU covers 8 hmax x 8 vmax pixels and segment j the MCUs [j Ri, (j+1) Ri).  The colour model follows
// libjpeg: three components are YCbCr with a JFIF segment, else what an Adobe segment's transform says (0: RGB), else RGB if the
// ids are 'R','G','B', else YCbCr; four are YCCK if an Adobe segment's transform is not 0, else CMYK.  A progressive file gets
// reason 3 with detail 0xC2.
inline int mg_jpeg_parse_layout(const uint8_t* data, size_t n, int max_extent, int32_t* info, int64_t* range, int64_t* seg, size_t seg_cap,
                                MgJpegTables* tables) {
    using namespace mgjpeg;
    const Reader R{data, n};
    memset(info, 0, sizeof(int32_t) * MG_JPEG_LAYOUT_INFO_INTS);
    memset(tables, 0, sizeof(*tables));
    range[0] = range[1] = 0;
    auto refuse = [&](int reason, long long detail) {
        info[MG_JPEG_I_REASON] = reason;
        info[MG_JPEG_I_DETAIL] = (int32_t)(detail > 0x7fffffffLL ? 0x7fffffffLL : detail);
        return reason;
    };
    if (n < 2 || data[0] != 0xFF || data[1] != 0xD8) return refuse(MG_JPEG_NOT_JPEG, 0);

    uint8_t quant[4][64];
    uint8_t hbits[2][4][16], hvals[2][4][256];
    int hcount[2][4];
    bool have_q[4] = {false, false, false, false}, have_h[2][4] = {{false, false, false, false}, {false, false, false, false}};
    bool have_frame = false, jfif = false;
    int width = 0, height = 0, ncomp = 0, sof = 0, comp_id[4] = {0, 0, 0, 0}, comp_h[4] = {1, 1, 1, 1}, comp_v[4] = {1, 1, 1, 1};
    int comp_tq[4] = {0, 0, 0, 0}, td[4] = {0, 0, 0, 0}, ta[4] = {0, 0, 0, 0}, ri = 0, adobe = -1, hmax = 1, vmax = 1, mcu_blocks = 1;
    static const uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                       41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                       30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    size_t pos = 2;
    for (;;) {
        if (!R.has(pos, 2) || data[pos] != 0xFF) return refuse(MG_JPEG_MALFORMED, (long long)pos);
        while (pos + 1 < n && data[pos + 1] == 0xFF) ++pos;                  // fill bytes
        if (!R.has(pos, 2)) return refuse(MG_JPEG_MALFORMED, (long long)pos);
        const int m = data[pos + 1];
        pos += 2;
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;    // stand-alone markers
        if (m == 0xD9) return refuse(MG_JPEG_MALFORMED, (long long)pos);     // EOI before any scan
        if (!R.has(pos, 2)) return refuse(MG_JPEG_MALFORMED, (long long)pos);
        const int ln = R.u16(pos);
        if (ln < 2 || !R.has(pos, (size_t)ln)) return refuse(MG_JPEG_MALFORMED, (long long)pos);
        const size_t body = pos + 2, end = pos + (size_t)ln;
        if (m == 0xDB) {
            size_t p = body;
            while (p < end) {
                const int pq = data[p] >> 4, tq = data[p] & 15;
                if (pq != 0) return refuse(MG_JPEG_PRECISION, 16);
                if (tq > 3 || p + 65 > end) return refuse(MG_JPEG_MALFORMED, (long long)p);
                for (int k = 0; k < 64; ++k) quant[tq][ZIGZAG[k]] = data[p + 1 + k];
                have_q[tq] = true;
                p += 65;
            }
        } else if (m == 0xC4) {
            size_t p = body;
            while (p < end) {
                if (p + 17 > end) return refuse(MG_JPEG_MALFORMED, (long long)p);
                const int tc = data[p] >> 4, th = data[p] & 15;
                int cnt = 0;
                for (int i = 0; i < 16; ++i) cnt += data[p + 1 + i];
                if (tc > 1 || th > 3 || cnt > 256 || p + 17 + (size_t)cnt > end) return refuse(MG_JPEG_MALFORMED, (long long)p);
                int code = 0;
                for (int l = 1; l <= 16; ++l) {
                    code += data[p + l];
                    if (code > (1 << l)) return refuse(MG_JPEG_MALFORMED, (long long)p);
                    code <<= 1;
                }
                memcpy(hbits[tc][th], data + p + 1, 16);
                memcpy(hvals[tc][th], data + p + 17, (size_t)cnt);
                hcount[tc][th] = cnt;
                have_h[tc][th] = true;
                p += 17 + (size_t)cnt;
            }
        } else if (m == 0xDD) {
            if (ln != 4) return refuse(MG_JPEG_MALFORMED, (long long)pos);
            ri = R.u16(body);
        } else if (m == 0xCC || (m >= 0xC9 && m <= 0xCF)) {
            return refuse(MG_JPEG_ARITHMETIC, m);
        } else if (m == 0xC2 || m == 0xC3 || m == 0xC5 || m == 0xC6 || m == 0xC7 || m == 0xC8) {
            return refuse(MG_JPEG_UNSUPPORTED_SOF, m);
        } else if (m == 0xC0 || m == 0xC1) {
            if (have_frame || ln < 8) return refuse(MG_JPEG_MALFORMED, (long long)pos);
            const int prec = data[body], nf = data[body + 5];
            height = R.u16(body + 1);
            width = R.u16(body + 3);
            if (prec != 8) return refuse(MG_JPEG_PRECISION, prec);
            if (ln != 8 + 3 * nf) return refuse(MG_JPEG_MALFORMED, (long long)pos);
            if (nf != 1 && nf != 3 && nf != 4) return refuse(MG_JPEG_COMPONENTS, nf);
            if (height == 0) return refuse(MG_JPEG_DNL, 0);
            if (width < 1 || width > max_extent || height > max_extent) return refuse(MG_JPEG_EXTENT, width > max_extent ? width : height);
            ncomp = nf, sof = m;
            for (int i = 0; i < nf; ++i) {
                comp_id[i] = data[body + 6 + 3 * i];
                comp_h[i] = data[body + 7 + 3 * i] >> 4;
                comp_v[i] = data[body + 7 + 3 * i] & 15;
                comp_tq[i] = data[body + 8 + 3 * i];
            }
            for (int i = 0; i < nf; ++i)
                if (comp_tq[i] > 3) return refuse(MG_JPEG_MALFORMED, (long long)pos);
            for (int i = 0; i < nf; ++i)
                if (comp_h[i] < 1 || comp_h[i] > 4 || comp_v[i] < 1 || comp_v[i] > 4) return refuse(MG_JPEG_SAMPLING_RANGE, comp_h[i] * 16 + comp_v[i]);
            if (nf == 1) comp_h[0] = comp_v[0] = 1;                          // one component: its factors mean nothing (T.81 A.2.2)
            hmax = vmax = 1, mcu_blocks = 0;
            for (int i = 0; i < nf; ++i) {
                hmax = comp_h[i] > hmax ? comp_h[i] : hmax;
                vmax = comp_v[i] > vmax ? comp_v[i] : vmax;
                mcu_blocks += comp_h[i] * comp_v[i];
            }
            for (int i = 0; i < nf; ++i)
                if (hmax % comp_h[i] || vmax % comp_v[i]) return refuse(MG_JPEG_FRACTIONAL_SAMPLING, comp_h[i] * 16 + comp_v[i]);
            if (mcu_blocks > MG_JPEG_MAX_MCU_BLOCKS) return refuse(MG_JPEG_SAMPLING_RANGE, mcu_blocks);
            have_frame = true;
        } else if (m == 0xDC) {
            return refuse(MG_JPEG_DNL, 0);
        } else if (m == 0xE0 && ln >= 16 && memcmp(data + body, "JFIF", 5) == 0) {
            jfif = true;
        } else if (m == 0xEE && ln >= 14 && memcmp(data + body, "Adobe", 5) == 0) {
            adobe = data[body + 11];
        } else if (m == 0xDA) {
            if (!have_frame) return refuse(MG_JPEG_MALFORMED, (long long)pos);
            const int ns = ln >= 3 ? data[body] : 0;
            if (ns != ncomp) return refuse(MG_JPEG_SCANS, ns);
            if (ln != 6 + 2 * ns) return refuse(MG_JPEG_MALFORMED, (long long)pos);
            for (int i = 0; i < ns; ++i) {
                if (data[body + 1 + 2 * i] != comp_id[i]) return refuse(MG_JPEG_MALFORMED, (long long)pos);
                td[i] = data[body + 2 + 2 * i] >> 4;
                ta[i] = data[body + 2 + 2 * i] & 15;
                if (td[i] > 3 || ta[i] > 3) return refuse(MG_JPEG_MALFORMED, (long long)pos);
            }
            if (data[body + 1 + 2 * ns] != 0 || data[body + 2 + 2 * ns] != 63 || data[body + 3 + 2 * ns] != 0)
                return refuse(MG_JPEG_MALFORMED, (long long)pos);
            for (int i = 0; i < ns; ++i)
                if (!have_q[comp_tq[i]] || !have_h[0][td[i]] || !have_h[1][ta[i]]) return refuse(MG_JPEG_MISSING_TABLES, i);
            pos = end;
            break;
        }
        pos = end;
    }

    // the entropy-coded data: up to the first marker that is neither a stuffed FF, a fill byte nor RSTn
    const int mcux = (width + 8 * hmax - 1) / (8 * hmax), mcuy = (height + 8 * vmax - 1) / (8 * vmax);
    const long long nmcu = (long long)mcux * mcuy;
    const long long nseg = ri ? (nmcu + ri - 1) / ri : 1;
    const size_t begin = pos;
    size_t i = pos, seg_begin = pos;
    long long found = 0;
    auto put = [&](long long j, size_t b, size_t e) {
        if (j < nseg && (size_t)j < seg_cap) {
            seg[2 * j] = (int64_t)b;
            seg[2 * j + 1] = (int64_t)e;
        }
    };
    for (;;) {
        while (i < n && data[i] != 0xFF) ++i;
        if (i + 1 >= n) {
            i = n;
            break;
        }
        const int b = data[i + 1];
        if (b == 0) {
            i += 2;
        } else if (b == 0xFF) {
            i += 1;
        } else if (b >= 0xD0 && b <= 0xD7) {
            put(found, seg_begin, i);
            ++found;
            i += 2;
            seg_begin = i;
        } else {
            break;
        }
    }
    const size_t ecs_end = i;
    put(found, seg_begin, ecs_end);
    for (long long j = found + 1; j < nseg; ++j) put(j, ecs_end, ecs_end);
    // what follows: another scan or DNL is refused; anything else (EOI, nothing, rubbish) ends the file
    while (i + 1 < n && data[i] == 0xFF) {
        const int b = data[i + 1];
        if (b == 0xFF) {
            ++i;
            continue;
        }
        if (b == 0xD9) break;
        if (b == 0xDA) return refuse(MG_JPEG_SCANS, 2);
        if (b == 0xDC) return refuse(MG_JPEG_DNL, 0);
        if (i + 4 > n) break;
        i += 2 + (size_t)R.u16(i + 2);
    }

    for (int c = 0; c < ncomp; ++c) {
        memcpy(tables->quant[comp_tq[c]], quant[comp_tq[c]], 64);
        if (!mgjpeg::derive(hbits[0][td[c]], hvals[0][td[c]], hcount[0][td[c]], &tables->dc[td[c]]) ||
            !mgjpeg::derive(hbits[1][ta[c]], hvals[1][ta[c]], hcount[1][ta[c]], &tables->ac[ta[c]]))
            return refuse(MG_JPEG_MALFORMED, c);
    }
    int colour = MG_JPEG_COLOUR_GRAY;
    if (ncomp == 3) {
        const bool ids_rgb = comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B';
        colour = jfif ? MG_JPEG_COLOUR_YCC : adobe >= 0 ? (adobe == 0 ? MG_JPEG_COLOUR_RGB : MG_JPEG_COLOUR_YCC)
                                                        : (ids_rgb ? MG_JPEG_COLOUR_RGB : MG_JPEG_COLOUR_YCC);
    } else if (ncomp == 4) {
        colour = adobe > 0 ? MG_JPEG_COLOUR_YCCK : MG_JPEG_COLOUR_CMYK;
    }
    info[MG_JPEG_I_WIDTH] = width;
    info[MG_JPEG_I_HEIGHT] = height;
    info[MG_JPEG_I_NCOMP] = ncomp;
    info[MG_JPEG_L_HMAX] = hmax;
    info[MG_JPEG_L_VMAX] = vmax;
    for (int c = 0; c < 4; ++c) {
        info[MG_JPEG_L_H + c] = c < ncomp ? comp_h[c] : 0;
        info[MG_JPEG_L_V + c] = c < ncomp ? comp_v[c] : 0;
        info[MG_JPEG_L_TQ + c] = comp_tq[c];
        info[MG_JPEG_L_TD + c] = td[c];
        info[MG_JPEG_L_TA + c] = ta[c];
    }
    info[MG_JPEG_L_RI] = ri;
    info[MG_JPEG_L_RESTARTS] = (int32_t)(found > 0x7fffffffLL ? 0x7fffffffLL : found);
    info[MG_JPEG_L_NSEG] = (int32_t)nseg;
    info[MG_JPEG_L_MCUX] = mcux;
    info[MG_JPEG_L_MCUY] = mcuy;
    info[MG_JPEG_L_COLOUR] = colour;
    info[MG_JPEG_L_SOF] = sof;
    info[MG_JPEG_L_BLOCKS] = mcu_blocks;
    range[0] = (int64_t)begin;
    range[1] = (int64_t)ecs_end;
    return MG_JPEG_OK;
}
