// Baseline JPEG, split scans ("Split scans"): one restart-free segment decoded on many lanes with the result of
// mg_jpeg_decode_segment, byte for byte.  A Huffman-coded scan self-synchronises, and what has to agree between two decoders is
// small -- the position of the next unread bit, the block's index in its MCU, the zigzag index -- while DC predictors and block
// numbers are sums that are carried forward afterwards.  The segment's bytes are cut into chunks; lane t owns the symbols whose
// first bit lies in chunk t (mg_jpeg_walk of jpeg_entropy.hpp, the serial decoder's own loop, in its scanning and writing forms):
//   1. speculate   lane 0 walks from the segment's true state, every other lane from a guess, storing nothing
//   2. synchronise every lane takes its predecessor's exit state as its entry and walks again if that entry is new, until a round
//                  changes nothing: lane 0 is right from the start and lane t is right once lane t - 1 is, so the fixed point is
//                  the serial decoder's state at every boundary whatever the guesses were, after at most as many rounds as chunks
//   3. carry       exclusive prefix sums of the blocks ended, of the DC differences per component and of the walks that failed
//   4. write       every lane with a valid entry and no failed walk before it walks a last time and stores what the serial
//                  decoder stores; the status word is this pass's
// Plain C++17 without a HIP header: jpeg_split_kernel (jpeg_decode.hip) runs these steps with a lane per chunk, through LDS and
// workgroup barriers; mg_jpeg_decode_segment_split_host runs them serially, in the rounds' order, for tools/dev/jpeg_split_host_check.cpp.
#pragma once
#include "jpeg_entropy.hpp"

constexpr int MG_JPEG_SPLIT_MAX_LANES = 1024;
constexpr int MG_JPEG_SPLIT_MIN_CHUNK = 8, MG_JPEG_SPLIT_MAX_CHUNK = 65536;
constexpr long long MG_JPEG_SPLIT_MAX_BYTES = 1LL << 28;      // a bit position then fits 31 bits of the packed state

// Routing.  A segment of `len` bytes is split when it is at least two chunks long and its positions fit the state's field;
// chunk_bytes = 0: never.  jpeg_entropy_kernel skips exactly the segments jpeg_split_kernel takes.
MG_HD bool mg_jpeg_split_takes(long long len, int chunk_bytes) {
    return chunk_bytes >= MG_JPEG_SPLIT_MIN_CHUNK && len >= 2LL * chunk_bytes && len < MG_JPEG_SPLIT_MAX_BYTES;
}

// Chunk geometry.  Boundaries lie on 8-byte boundaries of the data buffer (`lead` = the misalignment of the segment's first
// byte, 0..7), so a lane's aligned 8-byte loads start at once; with more chunks than lanes the chunk grows.  Chunk t covers the
// offsets [begin(t), end(t)) from the segment's first byte.
struct MgJpegSplit {
    uint32_t len, lead, chunk;
    int chunks;
    MG_HD uint32_t begin(int t) const { return t == 0 ? 0u : (uint32_t)t * chunk - lead; }
    MG_HD uint32_t end(int t) const {
        const uint64_t e = (uint64_t)(t + 1) * chunk - lead;
        return e < len ? (uint32_t)e : len;
    }
};

MG_HD MgJpegSplit mg_jpeg_split_geometry(uintptr_t first_byte, long long len, int chunk_bytes, int lanes) {
    MgJpegSplit s;
    s.len = (uint32_t)len, s.lead = (uint32_t)(first_byte & 7u);
    const uint64_t span = (uint64_t)s.lead + (uint64_t)len;
    uint64_t chunk = (uint64_t)chunk_bytes;
    if ((span + chunk - 1) / chunk > (uint64_t)lanes) chunk = ((span + lanes - 1) / lanes + 7) & ~7ull;
    s.chunk = (uint32_t)chunk;
    s.chunks = (int)((span + chunk - 1) / chunk);
    return s;
}

// The speculative entry of lane t > 0: its chunk's first bit as block `bi` of an MCU at zigzag index `k` (the kernel guesses
// 0, 0).  A position never points at the 00 of a stuffed FF 00: there the guess starts one byte later.
MG_HD uint64_t mg_jpeg_split_guess(const uint8_t* p, const MgJpegSplit& s, int t, int bi, int k) {
    uint32_t at = s.begin(t);
    if (at > 0 && at < s.len && p[at - 1] == 0xFF && p[at] == 0) ++at;
    return mg_jpeg_state(at * 8u, bi, k);
}

// One lane's LDS record on the host.
struct MgJpegSplitLane {
    uint64_t entry, exit;
    uint32_t blocks, failed, dc[3];
};

// Steps 1-4 for one segment on the CPU, serially and in the rounds' order, with `lanes` lanes and chunks of `chunk_bytes`
// (a segment mg_jpeg_split_takes refuses goes to mg_jpeg_decode_segment).  `lane` holds `lanes` records.  guess_bi / guess_k:
// the speculative start state, 0 / 0 in the kernel -- the result does not depend on it.  -> the status word; *rounds, *chunks: the
// synchronisation rounds run (the last one changes nothing) and the chunks.
inline int mg_jpeg_decode_segment_split_host(const uint8_t* p, const uint8_t* end, const MgJpegTables* T, const MgJpegSegment& g, int16_t* coef0,
                                             int16_t* coef1, int16_t* coef2, int chunk_bytes, int lanes, MgJpegSplitLane* lane, int guess_bi,
                                             int guess_k, int* rounds, int* chunks) {
    *rounds = 0, *chunks = 1;
    if (lanes < 2 || lanes > MG_JPEG_SPLIT_MAX_LANES || !mg_jpeg_split_takes(end - p, chunk_bytes))
        return mg_jpeg_decode_segment(p, end, T, g, coef0, coef1, coef2);
    if (g.nmcu <= 0 || g.mcu0 < 0 || g.mcu0 > g.mcu_total - g.nmcu || g.mcux < 1 || (g.hs != 1 && g.hs != 2) || (g.vs != 1 && g.vs != 2))
        return MG_JPEG_SEG_BAD_RECORD;
    const MgJpegSplit s = mg_jpeg_split_geometry(reinterpret_cast<uintptr_t>(p), end - p, chunk_bytes, lanes);
    const int n = *chunks = s.chunks;
    const int bpm = g.ncomp == 1 ? 1 : g.hs * g.vs + 2;
    auto scan = [&](int t) {
        MgJpegWalk w;
        w.entry = lane[t].entry, w.limit = s.end(t);
        mg_jpeg_walk<MG_JPEG_WALK_SCAN>(p, end, T, g, nullptr, nullptr, nullptr, &w);
        lane[t].exit = w.exit, lane[t].blocks = w.blocks, lane[t].failed = w.failed;
        for (int c = 0; c < 3; ++c) lane[t].dc[c] = w.dc[c];
    };
    for (int t = 0; t < n; ++t) {                                            // 1. speculate
        lane[t].entry = t == 0 ? mg_jpeg_state(0, 0, 0) : mg_jpeg_split_guess(p, s, t, guess_bi % bpm, guess_k & 63);
        scan(t);
    }
    for (;;) {                                                               // 2. synchronise: a round reads every exit, then writes
        ++*rounds;
        bool changed = false;
        uint64_t prev = lane[0].exit;
        for (int t = 1; t < n; ++t) {
            const uint64_t in = prev, before = lane[t].exit;
            prev = before;
            if (in == lane[t].entry) continue;
            lane[t].entry = in;
            scan(t);
            changed |= lane[t].exit != before;
        }
        if (!changed) break;
    }
    int status = MG_JPEG_SEG_OK;
    uint32_t block0 = 0, failed = 0, pred[3] = {0, 0, 0};
    for (int t = 0; t < n; ++t) {                                            // 3. carry and 4. write, lane after lane
        if (lane[t].entry != MG_JPEG_STATE_INVALID && failed == 0 && (long long)block0 < (long long)g.nmcu * bpm) {
            MgJpegWalk w;
            w.entry = lane[t].entry, w.limit = s.end(t), w.block0 = block0;
            for (int c = 0; c < 3; ++c) w.dc[c] = pred[c];
            const int st = mg_jpeg_walk<MG_JPEG_WALK_WRITE>(p, end, T, g, coef0, coef1, coef2, &w);
            if (status == MG_JPEG_SEG_OK) status = st;                       // the lowest lane's
        }
        block0 += lane[t].blocks, failed += lane[t].failed;
        for (int c = 0; c < 3; ++c) pred[c] += lane[t].dc[c];
    }
    return status;
}
