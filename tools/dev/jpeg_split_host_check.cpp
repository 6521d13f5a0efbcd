// The split-scan decoder's host-side run: the marker parser (csrc/jpeg_parse.hpp), then every segment twice -- through
// mg_jpeg_decode_segment and through mg_jpeg_decode_segment_split_host (csrc/jpeg_split.hpp: the chunk walks the GPU lanes run, in
// the rounds' order) -- and the IDCT and colour functions of csrc/jpeg_pixels.hpp on the split decoder's coefficients.  The two
// coefficient workspaces and the two status words must be equal byte for byte on EVERY input, sound or not.  Every buffer is an
// exact-size heap allocation, so under AddressSanitizer one byte read or written out of range is a report.  CPU only -- never run
// it on a GPU machine.
//
//   python tools/dev/jpeg_split_host_check.py     dumps the golden files, builds this with -fsanitize=address,undefined, runs it
//   tests/test_jpeg_split_cpu.py                  builds it with -O1 alone
//
//   jpeg_split_host_check FILE.jpg [FILE.rgb] [--chunks 8,64] [--lanes 4,1024] [--guess BI K] [--truncate] [--mutations N]
// decodes the file with every chunk size x lane count (comparing with the raw RGB8 pixels in FILE.rgb if given), then every
// truncation length of it (--truncate) and N seeded single-byte and burst mutations.  --guess: the speculative start state of
// every lane but the first, which the result must not depend on.  Exit status 0 if the two decoders agreed everywhere.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../mgnns_amd/csrc/jpeg_parse.hpp"
#include "../../mgnns_amd/csrc/jpeg_pixels.hpp"
#include "../../mgnns_amd/csrc/jpeg_split.hpp"

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
    int split = 0;                 // segments that were split
    int chunks = 0, rounds = 0;    // the largest of any segment
    int grown = 0;                 // segments whose chunk grew: more chunks than lanes
    int in_pair = 0;               // chunk boundaries on the 00 of a stuffed FF 00
    std::vector<uint8_t> rgb;
    int w = 0, h = 0;
};

static long g_reasons[16], g_status[8], g_inputs;
static int g_guess_bi = 0, g_guess_k = 0;

// the whole pipeline on one input, every buffer of exact size
static Outcome decode(const uint8_t* src, size_t n, int chunk_bytes, int lanes) {
    Outcome o;
    ++g_inputs;
    uint8_t* data = (uint8_t*)malloc(n ? n : 1);          // an exact-size copy: the parser must not read data[n]
    memcpy(data, src, n);
    int32_t info[MG_JPEG_INFO_INTS];
    int64_t range[2];
    MgJpegTables* T = (MgJpegTables*)malloc(sizeof(MgJpegTables));
    std::vector<int64_t> seg(2);
    o.reason = mg_jpeg_parse(data, n, 8192, info, range, seg.data(), 1, T);
    if (o.reason == MG_JPEG_OK && info[MG_JPEG_I_NSEG] > 1) {
        seg.assign(2 * (size_t)info[MG_JPEG_I_NSEG], 0);
        o.reason = mg_jpeg_parse(data, n, 8192, info, range, seg.data(), seg.size() / 2, T);
    }
    if (o.reason < 0 || o.reason > MG_JPEG_MISSING_TABLES) {
        fprintf(stderr, "undocumented reason %d\n", o.reason);
        exit(1);
    }
    g_reasons[o.reason]++;
    if (o.reason == MG_JPEG_OK) {
        const int W = info[MG_JPEG_I_WIDTH], H = info[MG_JPEG_I_HEIGHT], nc = info[MG_JPEG_I_NCOMP], hs = info[MG_JPEG_I_HS], vs = info[MG_JPEG_I_VS];
        const int mcux = info[MG_JPEG_I_MCUX], mcuy = info[MG_JPEG_I_MCUY], ri = info[MG_JPEG_I_RI];
        const size_t nmcu = (size_t)mcux * mcuy;
        int16_t* serial[3] = {nullptr, nullptr, nullptr}, * coef[3] = {nullptr, nullptr, nullptr};
        size_t blocks[3] = {nmcu * hs * vs, nmcu, nmcu};
        for (int c = 0; c < nc; ++c) serial[c] = (int16_t*)calloc(blocks[c] * 64, sizeof(int16_t)), coef[c] = (int16_t*)calloc(blocks[c] * 64, sizeof(int16_t));
        MgJpegSplitLane* lane = (MgJpegSplitLane*)malloc(sizeof(MgJpegSplitLane) * (size_t)lanes);
        for (int j = 0; j < info[MG_JPEG_I_NSEG]; ++j) {
            MgJpegSegment g;
            g.ncomp = nc, g.hs = hs, g.vs = vs, g.mcux = mcux, g.mcu_total = (int)nmcu;
            g.mcu0 = ri ? j * ri : 0;
            g.nmcu = ri ? (int)((nmcu - g.mcu0) < (size_t)ri ? nmcu - g.mcu0 : ri) : (int)nmcu;
            for (int c = 0; c < 3; ++c) g.td[c] = info[MG_JPEG_I_TD + c], g.ta[c] = info[MG_JPEG_I_TA + c];
            const size_t sb = (size_t)seg[2 * j], se = (size_t)seg[2 * j + 1];
            // the segment alone, ending where its allocation ends: a read past its end is a report.  It starts at the misalignment
            // it has in the file (files sit on 16-byte boundaries on the GPU), so the chunk boundaries fall where the kernel's fall.
            const size_t mis = sb & 7;
            uint8_t* const alloc = (uint8_t*)malloc(mis + (se - sb) ? mis + (se - sb) : 1);
            uint8_t* const piece = alloc + mis;
            memcpy(piece, data + sb, se - sb);
            const int want = mg_jpeg_decode_segment(piece, piece + (se - sb), T, g, serial[0], serial[1], serial[2]);
            int rounds = 0, chunks = 1;
            const int st = mg_jpeg_decode_segment_split_host(piece, piece + (se - sb), T, g, coef[0], coef[1], coef[2], chunk_bytes, lanes, lane,
                                                             g_guess_bi, g_guess_k, &rounds, &chunks);
            if (chunks > 1) {
                const MgJpegSplit s = mg_jpeg_split_geometry(reinterpret_cast<uintptr_t>(piece), (long long)(se - sb), chunk_bytes, lanes);
                ++o.split;
                if (s.chunk != (uint32_t)chunk_bytes) ++o.grown;
                for (int t = 1; t < s.chunks; ++t)
                    if (s.begin(t) < s.len && piece[s.begin(t) - 1] == 0xFF && piece[s.begin(t)] == 0) ++o.in_pair;
                if (rounds > chunks) {
                    fprintf(stderr, "%d rounds for %d chunks\n", rounds, chunks);
                    exit(1);
                }
            }
            free(alloc);
            if (st != want) {
                fprintf(stderr, "segment %d: status %d, the serial decoder's is %d (chunk %d, %d lanes, %zu bytes)\n", j, st, want, chunk_bytes, lanes, n);
                exit(1);
            }
            if (st < 0 || st > MG_JPEG_SEG_COEF_OVERFLOW) {
                fprintf(stderr, "undocumented status %d\n", st);
                exit(1);
            }
            g_status[st]++;
            if (st > o.worst) o.worst = st;
            if (chunks > o.chunks) o.chunks = chunks;
            if (rounds > o.rounds) o.rounds = rounds;
        }
        free(lane);
        for (int c = 0; c < nc; ++c)
            if (memcmp(serial[c], coef[c], blocks[c] * 64 * sizeof(int16_t)) != 0) {
                fprintf(stderr, "component %d: the coefficients differ from the serial decoder's (chunk %d, %d lanes, %zu bytes)\n", c, chunk_bytes, lanes, n);
                exit(1);
            }
        // planes at block-padded size, then pixels
        uint8_t* plane[3] = {nullptr, nullptr, nullptr};
        int pitch[3];
        for (int c = 0; c < nc; ++c) {
            const int bw = mcux * (c ? 1 : hs), bh = mcuy * (c ? 1 : vs);
            pitch[c] = 8 * bw;
            plane[c] = (uint8_t*)malloc((size_t)64 * bw * bh);
            const uint8_t* q = T->quant[info[MG_JPEG_I_TQ + c]];
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
                    mg_jpeg_rgb(Y, mg_jpeg_chroma(plane[1], pitch[1], dw, dh, hs, vs, x, y), mg_jpeg_chroma(plane[2], pitch[2], dw, dh, hs, vs, x, y), px);
                }
            }
        for (int c = 0; c < nc; ++c) {
            free(serial[c]);
            free(coef[c]);
            free(plane[c]);
        }
    }
    free(T);
    free(data);
    return o;
}

static std::vector<int> int_list(const char* s) {
    std::vector<int> v;
    for (const char* q = s; *q;) {
        char* e;
        v.push_back((int)strtol(q, &e, 10));
        if (e == q) break;
        q = *e == ',' ? e + 1 : e;
    }
    return v;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: jpeg_split_host_check FILE.jpg [FILE.rgb] [--chunks 8,64] [--lanes 4,1024] [--guess BI K] [--truncate] [--mutations N]\n");
        return 2;
    }
    const char* rgb_path = nullptr;
    bool truncate = false;
    long mutations = 0;
    std::vector<int> chunk_list = {8, 64}, lane_list = {1024};
    for (int a = 2; a < argc; ++a) {
        const std::string s = argv[a];
        if (s == "--truncate") truncate = true;
        else if (s == "--mutations" && a + 1 < argc) mutations = atol(argv[++a]);
        else if (s == "--chunks" && a + 1 < argc) chunk_list = int_list(argv[++a]);
        else if (s == "--lanes" && a + 1 < argc) lane_list = int_list(argv[++a]);
        else if (s == "--guess" && a + 2 < argc) g_guess_bi = atoi(argv[a + 1]), g_guess_k = atoi(argv[a + 2]), a += 2;
        else rgb_path = argv[a];
    }
    for (int c : chunk_list)
        if (c < MG_JPEG_SPLIT_MIN_CHUNK || c > (1 << 20) || c % 8) {
            fprintf(stderr, "a chunk size is a multiple of 8\n");
            return 2;
        }
    for (int l : lane_list)
        if (l < 2 || l > MG_JPEG_SPLIT_MAX_LANES) {
            fprintf(stderr, "2..%d lanes\n", MG_JPEG_SPLIT_MAX_LANES);
            return 2;
        }
    const std::vector<uint8_t> file = read_file(argv[1]);
    std::vector<uint8_t> want;
    if (rgb_path) want = read_file(rgb_path);
    printf("%s: %zu bytes", argv[1], file.size());
    for (int chunk : chunk_list)
        for (int lanes : lane_list) {
            const Outcome whole = decode(file.data(), file.size(), chunk, lanes);
            printf("\n  chunk %d, %d lanes: reason %d, worst status %d, %dx%d, %d split, %d chunks, %d rounds, %d grown, %d in a pair", chunk, lanes,
                   whole.reason, whole.worst, whole.w, whole.h, whole.split, whole.chunks, whole.rounds, whole.grown, whole.in_pair);
            if (rgb_path) {
                if (whole.reason != MG_JPEG_OK || whole.worst != 0 || want != whole.rgb) {
                    printf("\nMISMATCH against %s\n", rgb_path);
                    return 1;
                }
                printf(", pixels equal");
            }
        }
    uint64_t s = 0x9E3779B97F4A7C15ull ^ file.size();
    auto rnd = [&]() {                                     // xorshift64*
        s ^= s >> 12, s ^= s << 25, s ^= s >> 27;
        return (uint32_t)((s * 0x2545F4914F6CDD1Dull) >> 32);
    };
    for (int chunk : chunk_list)
        for (int lanes : lane_list) {
            if (truncate)
                for (size_t n = 0; n < file.size(); ++n) decode(file.data(), n, chunk, lanes);
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
                decode(m.data(), m.size(), chunk, lanes);
            }
        }
    printf("\n  %ld inputs equal to the serial decoder; reasons", g_inputs);
    for (int i = 0; i <= MG_JPEG_MISSING_TABLES; ++i) printf(" %ld", g_reasons[i]);
    printf("; statuses");
    for (int i = 0; i <= MG_JPEG_SEG_COEF_OVERFLOW; ++i) printf(" %ld", g_status[i]);
    printf("\n");
    return 0;
}
