// The progressive JPEG decoder's host-side run: the progressive parser (csrc/jpeg_parse.hpp) and the very decoder body the GPU
// lanes run (csrc/jpeg_progressive.hpp), then the IDCT and colour functions of csrc/jpeg_pixels.hpp, on the CPU.  Every buffer is an
// exact-size heap allocation, so under AddressSanitizer one byte read or written out of range is a report.  Scans run level by
// level, as the GPU launches them.  CPU only -- never run it on a GPU machine.
//
//   python tools/dev/jpeg_progressive_host_check.py     dumps the golden files, builds this with -fsanitize=address,undefined, runs it
//   tests/test_jpeg_progressive_cpu.py                  builds it with -O1 alone and compares pixels and statuses
//
//   jpeg_progressive_host_check FILE.jpg [FILE.rgb]  [--truncate] [--mutations N]
// decodes the file (comparing with the raw RGB8 pixels in FILE.rgb if given), then every truncation length of it (--truncate) and N
// seeded single-byte and burst mutations.  Every input must end in a documented reason code or segment status; exit status 0.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../mgnns_amd/csrc/jpeg_parse.hpp"
#include "../../mgnns_amd/csrc/jpeg_pixels.hpp"
#include "../../mgnns_amd/csrc/jpeg_progressive.hpp"

static std::vector<uint8_t> read_file(const char* path) {
    std::vector<uint8_t> v;
    FILE* f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        exit(2);
    }
    uint8_t buf[4096];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + k);
    fclose(f);
    return v;
}

struct Outcome {
    int reason = 0;
    int worst = 0;                 // largest segment status
    int scans = 0, levels = 0;
    long segments = 0;
    std::vector<uint8_t> rgb;
    int w = 0, h = 0;
};

static long g_reasons[MG_JPEG_TOO_MANY_SCANS + 1], g_status[8];

// the whole pipeline on one input, every buffer of exact size
static Outcome decode(const uint8_t* src, size_t n) {
    Outcome o;
    uint8_t* data = (uint8_t*)malloc(n ? n : 1);          // an exact-size copy: the parser must not read data[n]
    memcpy(data, src, n);
    int32_t info[MG_JPEG_INFO_INTS];
    int64_t* scans = (int64_t*)malloc(sizeof(int64_t) * MG_JPEG_MAX_SCANS * MG_JPEG_SCAN_INTS);
    MgJpegHuff* pool = (MgJpegHuff*)malloc(sizeof(MgJpegHuff) * MG_JPEG_POOL_TABLES);
    uint8_t* quant = (uint8_t*)malloc(3 * 64);
    std::vector<int64_t> seg(4);
    o.reason = mg_jpeg_parse_progressive(data, n, 8192, info, scans, seg.data(), 1, pool, quant);
    if (o.reason == MG_JPEG_OK && info[MG_JPEG_I_NSEG] > 1) {
        seg.assign(4 * (size_t)info[MG_JPEG_I_NSEG], 0);
        o.reason = mg_jpeg_parse_progressive(data, n, 8192, info, scans, seg.data(), seg.size() / 4, pool, quant);
    }
    if (o.reason < 0 || o.reason > MG_JPEG_TOO_MANY_SCANS) {
        fprintf(stderr, "undocumented reason %d\n", o.reason);
        exit(1);
    }
    g_reasons[o.reason]++;
    if (o.reason == MG_JPEG_OK) {
        const int W = info[MG_JPEG_I_WIDTH], H = info[MG_JPEG_I_HEIGHT], nc = info[MG_JPEG_I_NCOMP], hs = info[MG_JPEG_I_HS], vs = info[MG_JPEG_I_VS];
        const int mcux = info[MG_JPEG_I_MCUX], mcuy = info[MG_JPEG_I_MCUY];
        const size_t nmcu = (size_t)mcux * mcuy;
        o.scans = info[MG_JPEG_I_NSCANS], o.levels = info[MG_JPEG_I_NLEVELS], o.segments = info[MG_JPEG_I_NSEG];
        int16_t* coef[3] = {nullptr, nullptr, nullptr};
        size_t blocks[3] = {nmcu * hs * vs, nmcu, nmcu};
        for (int c = 0; c < nc; ++c) coef[c] = (int16_t*)aligned_alloc(16, blocks[c] * 64 * sizeof(int16_t));
        for (int c = 0; c < nc; ++c) memset(coef[c], 0, blocks[c] * 64 * sizeof(int16_t));
        for (int level = 0; level < o.levels; ++level)
            for (int s = 0; s < o.scans; ++s) {
                const int64_t* S = scans + (size_t)s * MG_JPEG_SCAN_INTS;
                if (S[MG_JPEG_S_LEVEL] != level) continue;
                for (int64_t j = S[MG_JPEG_S_SEG0]; j < S[MG_JPEG_S_SEG0] + S[MG_JPEG_S_NSEG]; ++j) {
                    MgJpegProgSegment g;
                    g.ncomp = nc, g.hs = hs, g.vs = vs, g.W = W, g.H = H, g.mcux = mcux, g.mcuy = mcuy;
                    g.comps = (int)S[MG_JPEG_S_COMPS], g.ss = (int)S[MG_JPEG_S_SS], g.se = (int)S[MG_JPEG_S_SE];
                    g.ah = (int)S[MG_JPEG_S_AH], g.al = (int)S[MG_JPEG_S_AL];
                    g.unit0 = (int)seg[4 * j + 2], g.nunits = (int)seg[4 * j + 3];
                    const size_t sb = (size_t)seg[4 * j], se = (size_t)seg[4 * j + 1];
                    // the segment alone, ending where its allocation ends: a read past its end is a report.  It starts at the misalignment
                    // it has in the file (files sit on 16-byte boundaries on the GPU), so the byte-wise and the 8-byte reads both run.
                    const size_t mis = sb & 7;
                    uint8_t* const alloc = (uint8_t*)malloc(mis + (se - sb) ? mis + (se - sb) : 1);
                    uint8_t* const piece = alloc + mis;
                    memcpy(piece, data + sb, se - sb);
                    // every table on its own, at its exact size
                    MgJpegHuff* T[4] = {nullptr, nullptr, nullptr, nullptr};
                    for (int t = 0; t < 4; ++t) {
                        const int64_t at = S[MG_JPEG_S_DC + t];            // (S_AC follows the three S_DC)
                        if (at < 0) continue;
                        T[t] = (MgJpegHuff*)malloc(sizeof(MgJpegHuff));
                        memcpy(T[t], pool + at, sizeof(MgJpegHuff));
                    }
                    const int st = mg_jpeg_decode_progressive_segment(piece, piece + (se - sb), T[0], T[1], T[2], T[3], g, coef[0], coef[1], coef[2]);
                    for (int t = 0; t < 4; ++t) free(T[t]);
                    free(alloc);
                    if (st < 0 || st > MG_JPEG_SEG_COEF_OVERFLOW) {        // (a record the parser made is never a bad record)
                        fprintf(stderr, "undocumented status %d (scan %d)\n", st, s);
                        exit(1);
                    }
                    g_status[st]++;
                    if (st > o.worst) o.worst = st;
                }
            }
        // planes at block-padded size, then pixels
        uint8_t* plane[3] = {nullptr, nullptr, nullptr};
        int pitch[3];
        for (int c = 0; c < nc; ++c) {
            const int bw = mcux * (c ? 1 : hs), bh = mcuy * (c ? 1 : vs);
            pitch[c] = 8 * bw;
            plane[c] = (uint8_t*)malloc((size_t)64 * bw * bh);
            const uint8_t* q = quant + 64 * c;
            for (int by = 0; by < bh; ++by)
                for (int bx = 0; bx < bw; ++bx) {
                    const int16_t* blk = coef[c] + ((size_t)by * bw + bx) * 64;
                    int32_t ws[8][8], col[8];
                    for (int x = 0; x < 8; ++x) {
                        mg_jpeg_idct_column(blk, q, x, col);
                        for (int r = 0; r < 8; ++r) ws[r][x] = col[r];
                    }
                    for (int r = 0; r < 8; ++r) mg_jpeg_idct_row(ws[r], plane[c] + (size_t)(8 * by + r) * pitch[c] + 8 * bx);
                }
        }
        o.w = W, o.h = H;
        o.rgb.resize((size_t)W * H * 3);
        const int dw = (W + hs - 1) / hs, dh = (H + vs - 1) / vs;
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const int Y = plane[0][(size_t)y * pitch[0] + x];
                uint8_t* px = &o.rgb[((size_t)y * W + x) * 3];
                if (nc == 1) {
                    px[0] = px[1] = px[2] = (uint8_t)Y;
                } else {
                    mg_jpeg_rgb(Y, mg_jpeg_chroma(plane[1], pitch[1], dw, dh, hs, vs, x, y, dw <= 2), mg_jpeg_chroma(plane[2], pitch[2], dw, dh, hs, vs, x, y, dw <= 2), px);
                }
            }
        for (int c = 0; c < nc; ++c) {
            free(coef[c]);
            free(plane[c]);
        }
    }
    free(quant);
    free(pool);
    free(scans);
    free(data);
    return o;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: jpeg_progressive_host_check FILE.jpg [FILE.rgb] [--truncate] [--mutations N]\n");
        return 2;
    }
    const char* rgb_path = nullptr;
    bool truncate = false;
    long mutations = 0;
    for (int a = 2; a < argc; ++a) {
        const std::string s = argv[a];
        if (s == "--truncate") truncate = true;
        else if (s == "--mutations" && a + 1 < argc) mutations = atol(argv[++a]);
        else rgb_path = argv[a];
    }
    const std::vector<uint8_t> file = read_file(argv[1]);
    const Outcome whole = decode(file.data(), file.size());
    printf("%s: %zu bytes, reason %d, worst status %d, %dx%d, %d scans, %d levels, %ld segments", argv[1], file.size(), whole.reason, whole.worst,
           whole.w, whole.h, whole.scans, whole.levels, whole.segments);
    if (rgb_path) {
        const std::vector<uint8_t> want = read_file(rgb_path);
        if (whole.reason != MG_JPEG_OK || whole.worst != 0 || want != whole.rgb) {
            printf("\nMISMATCH against %s\n", rgb_path);
            return 1;
        }
        printf(", pixels equal");
    }
    if (truncate)
        for (size_t n = 0; n < file.size(); ++n) decode(file.data(), n);
    uint64_t s = 0x9E3779B97F4A7C15ull ^ file.size();
    auto rnd = [&]() {                                     // xorshift64*
        s ^= s >> 12, s ^= s << 25, s ^= s >> 27;
        return (uint32_t)((s * 0x2545F4914F6CDD1Dull) >> 32);
    };
    std::vector<uint8_t> m;
    for (long t = 0; t < mutations && !file.empty(); ++t) {
        m = file;
        const size_t at = rnd() % m.size();
        if (t & 1) {                                       // a burst of up to 16 bytes: random, all ones or all zero
            const size_t len = 1 + rnd() % 16;
            const uint32_t kind = rnd() % 3;
            for (size_t i = at; i < at + len && i < m.size(); ++i) m[i] = kind == 0 ? (uint8_t)rnd() : (kind == 1 ? 0xFF : 0x00);
        } else {
            m[at] = (uint8_t)rnd();
        }
        decode(m.data(), m.size());
    }
    printf("; reasons");
    for (int i = 0; i <= MG_JPEG_TOO_MANY_SCANS; ++i) printf(" %ld", g_reasons[i]);
    printf("; statuses");
    for (int i = 0; i <= MG_JPEG_SEG_COEF_OVERFLOW; ++i) printf(" %ld", g_status[i]);
    printf("\n");
    return 0;
}
