// The host-side run of the decoder of other component layouts: the routing of images.parse_jpeg(..., layouts=True) -- the baseline
// marker parser, then mg_jpeg_parse_layout after its refusals 3 (0xC1), 6, 7, 8, 9 (csrc/jpeg_parse.hpp) -- then every segment
// through mg_jpeg_decode_layout_segment and the planes through the IDCT of csrc/jpeg_pixels.hpp and the upsampling and colour
// functions of csrc/jpeg_layouts.hpp: the functions the GPU kernels run.  Every buffer is an exact-size heap allocation, so under
// AddressSanitizer one byte read or written out of range is a report.  CPU only -- never run it on a GPU machine.
//
//   python tools/dev/jpeg_layouts_host_check.py   dumps the golden files, builds this with -fsanitize=address,undefined, runs it
//   tests/test_jpeg_layouts_cpu.py                builds it with -O1 alone
//
//   jpeg_layouts_host_check FILE.jpg [FILE.rgb] [--truncate] [--mutations N]
// decodes the file (comparing with the raw RGB8 pixels in FILE.rgb if given), then every truncation length of it (--truncate) and N
// seeded single-byte and burst mutations.  A file the baseline parser accepts is the baseline decoder's and is only counted.
// Exit status 0 unless the pixels differ or a reason or status outside the documented ones turns up.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../mgnns_amd/csrc/jpeg_layouts.hpp"
#include "../../mgnns_amd/csrc/jpeg_parse.hpp"

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
    int reason = 0, detail = 0;
    bool baseline = false;         // the baseline parser accepted the file: not decoded here
    int worst = 0, nseg = 0;
    std::string statuses;          // one digit per segment
    std::vector<uint8_t> rgb;
    int w = 0, h = 0, ncomp = 0, colour = 0, hmax = 0, vmax = 0;
};

static long g_reasons[19], g_status[8], g_inputs, g_baseline;

static uint32_t pack(const int32_t* v, int n, int bits) {
    uint32_t p = 0;
    for (int c = 0; c < n; ++c) p |= (uint32_t)v[c] << (bits * c);
    return p;
}

// the whole pipeline on one input, every buffer of exact size
static Outcome decode(const uint8_t* src, size_t n) {
    Outcome o;
    ++g_inputs;
    uint8_t* data = (uint8_t*)malloc(n ? n : 1);          // an exact-size copy: the parser must not read data[n]
    memcpy(data, src, n);
    int32_t info[MG_JPEG_LAYOUT_INFO_INTS];
    int64_t range[2];
    MgJpegTables* T = (MgJpegTables*)malloc(sizeof(MgJpegTables));
    std::vector<int64_t> seg(2);
    o.reason = mg_jpeg_parse(data, n, 8192, info, range, seg.data(), 1, T);
    o.detail = info[MG_JPEG_I_DETAIL];
    if (o.reason == MG_JPEG_OK) {
        o.baseline = true;
        ++g_baseline;
    } else if ((o.reason >= MG_JPEG_COMPONENTS && o.reason <= MG_JPEG_SAMPLING) || (o.reason == MG_JPEG_UNSUPPORTED_SOF && o.detail == 0xC1)) {
        o.reason = mg_jpeg_parse_layout(data, n, 8192, info, range, seg.data(), 1, T);
        if (o.reason == MG_JPEG_OK && info[MG_JPEG_L_NSEG] > 1) {
            seg.assign(2 * (size_t)info[MG_JPEG_L_NSEG], 0);
            o.reason = mg_jpeg_parse_layout(data, n, 8192, info, range, seg.data(), seg.size() / 2, T);
        }
        o.detail = info[MG_JPEG_I_DETAIL];
    }
    if (o.reason < 0 || o.reason > MG_JPEG_SAMPLING_RANGE || (o.reason > MG_JPEG_MISSING_TABLES && o.reason < MG_JPEG_FRACTIONAL_SAMPLING)) {
        fprintf(stderr, "undocumented reason %d\n", o.reason);
        exit(1);
    }
    g_reasons[o.reason]++;
    if (o.reason == MG_JPEG_OK && !o.baseline) {
        const int W = info[MG_JPEG_I_WIDTH], H = info[MG_JPEG_I_HEIGHT], nc = info[MG_JPEG_I_NCOMP], hmax = info[MG_JPEG_L_HMAX], vmax = info[MG_JPEG_L_VMAX];
        const int mcux = info[MG_JPEG_L_MCUX], mcuy = info[MG_JPEG_L_MCUY], ri = info[MG_JPEG_L_RI];
        const int32_t* const ch = info + MG_JPEG_L_H, * const cv = info + MG_JPEG_L_V;
        const size_t nmcu = (size_t)mcux * mcuy;
        o.w = W, o.h = H, o.ncomp = nc, o.colour = info[MG_JPEG_L_COLOUR], o.hmax = hmax, o.vmax = vmax, o.nseg = info[MG_JPEG_L_NSEG];
        int16_t* coef[4] = {nullptr, nullptr, nullptr, nullptr};
        for (int c = 0; c < nc; ++c) coef[c] = (int16_t*)calloc(nmcu * ch[c] * cv[c] * 64, sizeof(int16_t));
        for (int j = 0; j < info[MG_JPEG_L_NSEG]; ++j) {
            MgJpegLayoutSegment g;
            g.ncomp = nc, g.h = pack(ch, nc, 4), g.v = pack(cv, nc, 4), g.td = pack(info + MG_JPEG_L_TD, nc, 2), g.ta = pack(info + MG_JPEG_L_TA, nc, 2);
            g.mcux = mcux, g.mcu_total = (int)nmcu;
            g.mcu0 = ri ? j * ri : 0;
            g.nmcu = ri ? (int)((nmcu - g.mcu0) < (size_t)ri ? nmcu - g.mcu0 : ri) : (int)nmcu;
            const size_t sb = (size_t)seg[2 * j], se = (size_t)seg[2 * j + 1];
            // the segment alone, ending where its allocation ends: a read past its end is a report.  It keeps the misalignment it
            // has in the file, so the 8-byte loads fall where the kernel's fall.
            const size_t mis = sb & 7;
            uint8_t* const alloc = (uint8_t*)malloc(mis + (se - sb) ? mis + (se - sb) : 1);
            uint8_t* const piece = alloc + mis;
            memcpy(piece, data + sb, se - sb);
            const int st = mg_jpeg_decode_layout_segment(piece, piece + (se - sb), T, g, coef[0], coef[1], coef[2], coef[3]);
            free(alloc);
            if (st < 0 || st > MG_JPEG_SEG_COEF_OVERFLOW) {
                fprintf(stderr, "undocumented status %d\n", st);
                exit(1);
            }
            g_status[st]++;
            if (o.statuses.size() < 64) o.statuses += (char)('0' + st);
            if (st > o.worst) o.worst = st;
        }
        // planes at block-padded size, then pixels
        uint8_t* plane[4] = {nullptr, nullptr, nullptr, nullptr};
        int pitch[4] = {0, 0, 0, 0};
        for (int c = 0; c < nc; ++c) {
            const int bw = mcux * ch[c], bh = mcuy * cv[c];
            pitch[c] = 8 * bw;
            plane[c] = (uint8_t*)malloc((size_t)64 * bw * bh);
            const uint8_t* q = T->quant[info[MG_JPEG_L_TQ + c]];
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
        o.rgb.resize((size_t)W * H * 3);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                int s[4] = {0, 0, 0, 0};
                for (int c = 0; c < nc; ++c)
                    s[c] = mg_jpeg_layout_sample(plane[c], pitch[c], (W * ch[c] + hmax - 1) / hmax, (H * cv[c] + vmax - 1) / vmax, hmax / ch[c],
                                                 vmax / cv[c], x, y);
                mg_jpeg_layout_rgb(o.colour, s[0], s[1], s[2], s[3], &o.rgb[((size_t)y * W + x) * 3]);
            }
        for (int c = 0; c < nc; ++c) {
            free(coef[c]);
            free(plane[c]);
        }
    }
    free(T);
    free(data);
    return o;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: jpeg_layouts_host_check FILE.jpg [FILE.rgb] [--truncate] [--mutations N]\n");
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
    printf("%s: %zu bytes, reason %d, detail %d, baseline %d, %dx%d, %d components %dx%d, colour %d, %d segments, statuses [%s], worst status %d",
           argv[1], file.size(), whole.reason, whole.detail, (int)whole.baseline, whole.w, whole.h, whole.ncomp, whole.hmax, whole.vmax, whole.colour,
           whole.nseg, whole.statuses.c_str(), whole.worst);
    if (rgb_path) {
        const std::vector<uint8_t> want = read_file(rgb_path);
        if (whole.reason != MG_JPEG_OK || whole.baseline || whole.worst != 0 || want != whole.rgb) {
            printf("\nMISMATCH against %s\n", rgb_path);
            return 1;
        }
        printf(", pixels equal");
    }
    uint64_t s = 0x9E3779B97F4A7C15ull ^ file.size();
    auto rnd = [&]() {                                     // xorshift64*
        s ^= s >> 12, s ^= s << 25, s ^= s >> 27;
        return (uint32_t)((s * 0x2545F4914F6CDD1Dull) >> 32);
    };
    if (truncate)
        for (size_t n = 0; n < file.size(); ++n) decode(file.data(), n);
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
    printf("\n  %ld inputs, %ld of them the baseline parser's; reasons", g_inputs, g_baseline);
    for (int i = 0; i <= MG_JPEG_SAMPLING_RANGE; ++i) printf(" %ld", g_reasons[i]);
    printf("; statuses");
    for (int i = 0; i <= MG_JPEG_SEG_COEF_OVERFLOW; ++i) printf(" %ld", g_status[i]);
    printf("\n");
    return 0;
}
