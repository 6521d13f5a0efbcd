// f4 (file half): baseline JPEG files -> the packed RGB8 pixel buffer image_prep.hip reads, bit for bit what Pillow / libjpeg-turbo
// decode.  The host parses the markers (jpeg_parse.hpp: no GPU call) and ships the compressed bytes, one record per
// image, one per independent segment and the distinct table sets; three launches on the caller's stream do the rest:
//   1. jpeg_entropy_kernel   one LANE per segment (a whole scan, or the stretch between two restart markers): Huffman decoding is
//                            serial within a segment, so the parallelism is across segments.  Quantised coefficients go as int16
//                            [block][64] in natural order into a zeroed workspace; one status word per segment.
//   2. jpeg_idct_kernel      dequantise + libjpeg's jidctint 8x8: eight threads per block, a column each, then a row each
//                            -> uint8 component planes at block-padded size.
//   3. jpeg_colour_kernel    one thread per pixel: "fancy" h2v1 / h2v2 chroma upsampling, YCbCr -> RGB, crop to W x H, interleaved
//                            RGB8 at the image's 16-byte-aligned offset; the padding behind the image is zeroed.
// The decoder body and the sample arithmetic live in jpeg_entropy.hpp / jpeg_pixels.hpp as host + device functions: the CPU run of
// tools/dev/jpeg_host_check.cpp under the sanitizers executes the same code.  Every record is re-checked on the device (a record
// buffer can change under a captured graph): a bad one gives status MG_JPEG_SEG_BAD_RECORD and writes nothing.
//
// Progressive files (SOF2; mgnns_jpeg_decode_progressive_fwd, DESIGN.md 17, "Progressive files") share the workspace, the pixel layout and stages 2
// and 3.  Their entropy stage is jpeg_progressive_kernel (jpeg_progressive.hpp), one lane per segment of one SCAN, launched once
// per LEVEL of the batch: scans of one level touch different (component, coefficient) pairs, so their lanes write different int16
// elements of a block and need neither atomics nor a fence; the stream orders the levels.
//
// Split scans (mgnns_jpeg_decode_split_fwd, DESIGN.md 17, "Split scans"): a long baseline segment -- a restart-free scan is one --
// gets a WORKGROUP of jpeg_split_kernel, a lane per chunk of its bytes (jpeg_split.hpp), and the serial decoder's result byte for
// byte; jpeg_entropy_kernel decodes the short ones, one lane each, in the same status array.
#include "common.hpp"
#include "../../include/mgnns_jpeg_progressive.h"
#include "../../include/mgnns_jpeg_split.h"
#include "../../include/mgnns_jpeg_layouts.h"
#include "jpeg_parse.hpp"
#include "jpeg_pixels.hpp"
#include "jpeg_progressive.hpp"
#include "jpeg_split.hpp"
#include "jpeg_layouts.hpp"

namespace {

constexpr int IMG = 16;         // int64 per image record
constexpr int SEG = 5;          // int64 per segment record
constexpr int PSEG = 12;        // int64 per segment record of a progressive scan
constexpr int QSET = 3 * 64;    // bytes of one latched quantisation set: a table per component
constexpr int MAXEXT = 8192;
constexpr int NT = 256;
constexpr int IDCT_BLOCKS = NT / 8;
constexpr int ENT_NT = 64;      // the entropy kernel's workgroup: one wave, of which the first `lanes` lanes decode a segment each
constexpr int LDS_SETS = 2;     // table sets kept in LDS (11 648 bytes each)
#ifndef MG_JPEG_SPLIT_LANES     // (an instrumented build for the sweep of DESIGN.md 17: MGNNS_HIPCC_FLAGS=-DMG_JPEG_SPLIT_LANES=256)
#define MG_JPEG_SPLIT_LANES 512
#endif
constexpr int SPLIT_NT = MG_JPEG_SPLIT_LANES;   // lanes of the split kernel's workgroup; a multiple of 64 up to MG_JPEG_SPLIT_MAX_LANES
static_assert(SPLIT_NT % 64 == 0 && SPLIT_NT <= MG_JPEG_SPLIT_MAX_LANES, "whole waves, one lane per LDS record");
static_assert(sizeof(MgJpegTables) % 16 == 0, "table sets are copied 16 bytes at a time");

struct Img {
    int kind, W, H, ncomp, hs, vs, mcux, mcuy, set;
    int tq[3], td[3], ta[3];
    long long coef_off, plane_off, pix_off, pix_end;
    long long nmcu, blocks0, blocks;      // MCUs; blocks of component 0; blocks of all components
};

// kind 0: pixels staged by the host; 1: baseline; 2: progressive -- `set` then counts the latched quantisation sets (n_q of them),
// a table per component, and the table ids are not read
__device__ __forceinline__ bool load_img(const int64_t* __restrict__ r, int n_sets, size_t coef_elems, size_t plane_bytes,
                                         size_t pixel_bytes, Img& m, int n_q = 0) {
    const long long kind = r[0], W = r[1], H = r[2], nc = r[3], hs = r[4], vs = r[5], mcux = r[6], mcuy = r[7], set = r[11];
    m.coef_off = r[12], m.plane_off = r[13], m.pix_off = r[14], m.pix_end = r[15];
    if (kind != 0 && kind != 1 && !(kind == 2 && n_q > 0)) return false;
    if (W < 1 || W > MAXEXT || H < 1 || H > MAXEXT) return false;
    if (m.pix_off < 0 || (m.pix_off & 15) || m.pix_end < m.pix_off || (unsigned long long)m.pix_end > pixel_bytes ||
        W * H * 3 > m.pix_end - m.pix_off)
        return false;
    m.kind = (int)kind, m.W = (int)W, m.H = (int)H;
    if (kind == 0) return true;                 // pixels staged by the host: nothing else is read
    if (!((nc == 1 && hs == 1 && vs == 1) || (nc == 3 && ((hs == 1 && vs == 1) || (hs == 2 && (vs == 1 || vs == 2)))))) return false;
    if (mcux != (W + 8 * hs - 1) / (8 * hs) || mcuy != (H + 8 * vs - 1) / (8 * vs)) return false;
    if (set < 0 || set >= (kind == 2 ? n_q : n_sets)) return false;
    m.ncomp = (int)nc, m.hs = (int)hs, m.vs = (int)vs, m.mcux = (int)mcux, m.mcuy = (int)mcuy, m.set = (int)set;
    m.nmcu = mcux * mcuy;
    m.blocks0 = m.nmcu * hs * vs;
    m.blocks = nc == 1 ? m.blocks0 : m.blocks0 + 2 * m.nmcu;
    if (m.coef_off < 0 || (m.coef_off & 63) || (unsigned long long)m.coef_off + (unsigned long long)m.blocks * 64 > coef_elems) return false;
    if (m.plane_off < 0 || (m.plane_off & 63) || (unsigned long long)m.plane_off + (unsigned long long)m.blocks * 64 > plane_bytes) return false;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        m.tq[c] = (int)((r[8] >> (8 * c)) & 3);
        m.td[c] = (int)((r[9] >> (8 * c)) & 3);
        m.ta[c] = (int)((r[10] >> (8 * c)) & 3);
    }
    return true;
}

// Which of the two baseline entropy kernels decodes the segment of bytes [b, e): the split kernel takes a record whose byte range is
// sound and long enough (jpeg_split.hpp); every other one -- a bad range too, which is status 4 -- is the one-lane kernel's.
__device__ __forceinline__ bool split_takes(long long b, long long e, size_t data_bytes, int split_chunk) {
    return b >= 0 && b <= e && (unsigned long long)e <= data_bytes && mg_jpeg_split_takes(e - b, split_chunk);
}

__global__ __launch_bounds__(ENT_NT) void jpeg_entropy_kernel(const uint8_t* __restrict__ data, size_t data_bytes,
                                    const int64_t* __restrict__ img, int B, const int64_t* __restrict__ seg, int S, int lanes,
                                    const MgJpegTables* __restrict__ tables, int n_sets,
                                    int16_t* __restrict__ coef, size_t coef_elems, size_t plane_bytes, size_t pixel_bytes,
                                    int32_t* __restrict__ status, int split_chunk) {
    // The batch's first LDS_SETS table sets -- nearly always all of them -- are copied into LDS: the look-up of a symbol is the one
    // load every trip of the loop waits for, and it depends on the bits just read.  A lane of another set reads global memory.
    __shared__ __attribute__((aligned(16))) MgJpegTables s_tables[LDS_SETS];
    {
        const int n16 = (n_sets < LDS_SETS ? n_sets : LDS_SETS) * (int)(sizeof(MgJpegTables) / 16);
        const u32x4* const src = reinterpret_cast<const u32x4*>(tables);
        u32x4* const dst = reinterpret_cast<u32x4*>(s_tables);
        for (int i = threadIdx.x; i < n16; i += ENT_NT) dst[i] = src[i];
    }
    __syncthreads();
    const long long s = (long long)blockIdx.x * lanes + threadIdx.x;
    if ((int)threadIdx.x >= lanes || s >= S) return;
    const int64_t* const r = seg + s * SEG;
    const long long im = r[0], b = r[1], e = r[2], mcu0 = r[3], nmcu = r[4];
    if (split_takes(b, e, data_bytes, split_chunk)) return;      // jpeg_split_kernel's (split_chunk = 0: none)
    Img m;
    int st = MG_JPEG_SEG_BAD_RECORD;
    if (im >= 0 && im < B && b >= 0 && b <= e && (unsigned long long)e <= data_bytes && mcu0 >= 0 && nmcu >= 1 &&
        load_img(img + im * IMG, n_sets, coef_elems, plane_bytes, pixel_bytes, m) && m.kind == 1 && mcu0 <= m.nmcu - nmcu) {
        MgJpegSegment g;
        g.ncomp = m.ncomp, g.hs = m.hs, g.vs = m.vs, g.mcux = m.mcux, g.mcu_total = (int)m.nmcu, g.mcu0 = (int)mcu0, g.nmcu = (int)nmcu;
#pragma unroll
        for (int c = 0; c < 3; ++c) g.td[c] = m.td[c], g.ta[c] = m.ta[c];
        int16_t* const c0 = coef + m.coef_off;
        int16_t* const c1 = c0 + m.blocks0 * 64;
        int16_t* const c2 = c1 + m.nmcu * 64;
        const MgJpegTables* const T = m.set < LDS_SETS ? &s_tables[m.set] : tables + m.set;
        st = mg_jpeg_decode_segment(data + b, data + e, T, g, c0, c1, c2);
    }
    status[s] = st;
}

// Inclusive prefix sum over the wave's 64 lanes.
__device__ __forceinline__ uint32_t wave_prefix(uint32_t v) {
    const int l = (int)(threadIdx.x & 63);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(v, d, 64);
        if (l >= d) v += o;
    }
    return v;
}

// One WORKGROUP per baseline segment record the routing gives it (the others return at once), a lane per chunk: the four steps of
// jpeg_split.hpp through LDS and workgroup barriers -- no flag in global memory, no wait on another workgroup.  Every barrier is
// reached by the whole workgroup: what a lane skips is its walk, never a barrier, and the synchronisation loop's trip count comes
// from the barrier's own OR, so it is uniform.  It is bounded by the number of chunks.
__global__ __launch_bounds__(SPLIT_NT) void jpeg_split_kernel(const uint8_t* __restrict__ data, size_t data_bytes,
                                    const int64_t* __restrict__ img, int B, const int64_t* __restrict__ seg, int S,
                                    const MgJpegTables* __restrict__ tables, int n_sets,
                                    int16_t* __restrict__ coef, size_t coef_elems, size_t plane_bytes, size_t pixel_bytes,
                                    int32_t* __restrict__ status, int split_chunk) {
    __shared__ __attribute__((aligned(16))) MgJpegTables s_tables[LDS_SETS];
    __shared__ uint64_t s_exit[SPLIT_NT];                 // a lane's exit state: the next lane's entry
    __shared__ uint32_t s_wave[5][SPLIT_NT / 64];         // the waves' totals of the carry step
    __shared__ int s_status;
    const long long s = blockIdx.x;
    const int lane = (int)threadIdx.x;
    if (s >= S) return;
    const int64_t* const r = seg + s * SEG;
    const long long im = r[0], b = r[1], e = r[2], mcu0 = r[3], nmcu = r[4];
    if (!split_takes(b, e, data_bytes, split_chunk)) return;     // jpeg_entropy_kernel's (uniform over the workgroup)
    {
        const int n16 = (n_sets < LDS_SETS ? n_sets : LDS_SETS) * (int)(sizeof(MgJpegTables) / 16);
        const u32x4* const src = reinterpret_cast<const u32x4*>(tables);
        u32x4* const dst = reinterpret_cast<u32x4*>(s_tables);
        for (int i = lane; i < n16; i += SPLIT_NT) dst[i] = src[i];
    }
    if (lane == 0) s_status = 0x7fffffff;
    Img m;
    if (!(im >= 0 && im < B && mcu0 >= 0 && nmcu >= 1 && load_img(img + im * IMG, n_sets, coef_elems, plane_bytes, pixel_bytes, m) &&
          m.kind == 1 && mcu0 <= m.nmcu - nmcu)) {               // (uniform: every lane read the same record)
        if (lane == 0) status[s] = MG_JPEG_SEG_BAD_RECORD;
        return;
    }
    MgJpegSegment g;
    g.ncomp = m.ncomp, g.hs = m.hs, g.vs = m.vs, g.mcux = m.mcux, g.mcu_total = (int)m.nmcu, g.mcu0 = (int)mcu0, g.nmcu = (int)nmcu;
#pragma unroll
    for (int c = 0; c < 3; ++c) g.td[c] = m.td[c], g.ta[c] = m.ta[c];
    int16_t* const c0 = coef + m.coef_off;
    int16_t* const c1 = c0 + m.blocks0 * 64;
    int16_t* const c2 = c1 + m.nmcu * 64;
    const MgJpegTables* const T = m.set < LDS_SETS ? &s_tables[m.set] : tables + m.set;
    const uint8_t* const p = data + b, * const end = data + e;
    const MgJpegSplit sp = mg_jpeg_split_geometry(reinterpret_cast<uintptr_t>(p), e - b, split_chunk, SPLIT_NT);
    const int n = sp.chunks;                                     // 2..SPLIT_NT
    const bool active = lane < n;
    __syncthreads();                                             // the tables are in LDS

    // 1. speculate
    MgJpegWalk w;
    uint64_t entry = MG_JPEG_STATE_INVALID;
    w.exit = MG_JPEG_STATE_INVALID, w.blocks = 0, w.failed = 0, w.dc[0] = w.dc[1] = w.dc[2] = 0;
    w.limit = active ? sp.end(lane) : 0;
    if (active) {
        entry = lane == 0 ? mg_jpeg_state(0, 0, 0) : mg_jpeg_split_guess(p, sp, lane, 0, 0);
        w.entry = entry;
        mg_jpeg_walk<MG_JPEG_WALK_SCAN>(p, end, T, g, nullptr, nullptr, nullptr, &w);
    }
    s_exit[lane] = w.exit;
    __syncthreads();
    // 2. synchronise
    for (int round = 0; round < n; ++round) {
        const uint64_t in = active && lane > 0 ? s_exit[lane - 1] : entry;
        __syncthreads();                                         // every exit is read before one is replaced
        int changed = 0;
        if (in != entry) {
            const uint64_t before = w.exit;
            w.entry = entry = in;
            mg_jpeg_walk<MG_JPEG_WALK_SCAN>(p, end, T, g, nullptr, nullptr, nullptr, &w);
            s_exit[lane] = w.exit;
            changed = w.exit != before;
        }
        if (!__syncthreads_or(changed)) break;
    }
    // 3. carry: exclusive prefix sums over the lanes
    uint32_t own[5] = {w.blocks, w.failed, w.dc[0], w.dc[1], w.dc[2]}, sum[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        sum[i] = wave_prefix(own[i]);
        if ((lane & 63) == 63) s_wave[i][lane >> 6] = sum[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        uint32_t before = 0;
        for (int j = 0; j < (lane >> 6); ++j) before += s_wave[i][j];
        sum[i] += before - own[i];
    }
    // 4. write
    if (active && entry != MG_JPEG_STATE_INVALID && sum[1] == 0) {
        w.block0 = sum[0], w.dc[0] = sum[2], w.dc[1] = sum[3], w.dc[2] = sum[4];
        const int st = mg_jpeg_walk<MG_JPEG_WALK_WRITE>(p, end, T, g, c0, c1, c2, &w);
        if (st != MG_JPEG_SEG_OK) atomicMin(&s_status, (lane << 3) | st);        // the lowest lane's
    }
    __syncthreads();
    if (lane == 0) status[s] = s_status == 0x7fffffff ? MG_JPEG_SEG_OK : (s_status & 7);
}

// One lane per segment of a progressive scan, segments [first, first + count) of pseg: one level of the batch.  A record:
// image, begin, end (bytes in the data buffer), first unit, units, component mask, Ss, Se, Ah, Al, the pool indices of the DC tables
// of components 0..2 and of the AC table (16 bits each, 0xFFFF = none), the scan's number in its file (not read here).  The tables
// are read from global memory: the lanes of a level use many different ones, and one look-ahead table is 1 KB that stays in the
// lane's cache lines.
__global__ __launch_bounds__(ENT_NT) void jpeg_progressive_kernel(const uint8_t* __restrict__ data, size_t data_bytes,
                                    const int64_t* __restrict__ img, int B, const int64_t* __restrict__ pseg, int first, int count, int lanes,
                                    const MgJpegHuff* __restrict__ pool, int n_pool, int n_sets, int n_q,
                                    int16_t* __restrict__ coef, size_t coef_elems, size_t plane_bytes, size_t pixel_bytes,
                                    int32_t* __restrict__ status) {
    const long long s = (long long)blockIdx.x * lanes + threadIdx.x;
    if ((int)threadIdx.x >= lanes || s >= count) return;
    const int64_t* const r = pseg + (first + s) * PSEG;
    const long long im = r[0], b = r[1], e = r[2], unit0 = r[3], nunits = r[4], comps = r[5], ss = r[6], se = r[7], ah = r[8], al = r[9], tabs = r[10];
    Img m;
    int st = MG_JPEG_SEG_BAD_RECORD;
    const int t0 = (int)(tabs & 0xFFFF), t1 = (int)((tabs >> 16) & 0xFFFF), t2 = (int)((tabs >> 32) & 0xFFFF), ta = (int)((tabs >> 48) & 0xFFFF);
    auto table_ok = [&](int t) { return t == 0xFFFF || t < n_pool; };
    if (im >= 0 && im < B && b >= 0 && b <= e && (unsigned long long)e <= data_bytes && unit0 >= 0 && nunits >= 1 && unit0 <= 0x7fffffffLL &&
        nunits <= 0x7fffffffLL && comps >= 1 && comps <= 7 && ss >= 0 && ss <= 63 && se >= 0 && se <= 63 && ah >= 0 && ah <= 14 && al >= 0 &&
        al <= 13 && table_ok(t0) && table_ok(t1) && table_ok(t2) && table_ok(ta) &&
        load_img(img + im * IMG, n_sets, coef_elems, plane_bytes, pixel_bytes, m, n_q) && m.kind == 2) {
        MgJpegProgSegment g;
        g.ncomp = m.ncomp, g.hs = m.hs, g.vs = m.vs, g.W = m.W, g.H = m.H, g.mcux = m.mcux, g.mcuy = m.mcuy;
        g.comps = (int)comps, g.ss = (int)ss, g.se = (int)se, g.ah = (int)ah, g.al = (int)al, g.unit0 = (int)unit0, g.nunits = (int)nunits;
        int16_t* const c0 = coef + m.coef_off;
        int16_t* const c1 = c0 + m.blocks0 * 64;
        int16_t* const c2 = c1 + m.nmcu * 64;
        auto table = [&](int t) -> const MgJpegHuff* { return t == 0xFFFF ? nullptr : pool + t; };
        // (the function checks the unit range against the scan's own count, the tables it needs against null, and the rest of g)
        st = mg_jpeg_decode_progressive_segment(data + b, data + e, table(t0), table(t1), table(t2), table(ta), g, c0, c1, c2);
    }
    status[first + s] = st;
}

__global__ __launch_bounds__(NT) void jpeg_idct_kernel(const int64_t* __restrict__ img, const MgJpegTables* __restrict__ tables, int n_sets,
                                                       const int16_t* __restrict__ coef, size_t coef_elems, uint8_t* __restrict__ planes,
                                                       size_t plane_bytes, size_t pixel_bytes, const uint8_t* __restrict__ qsets = nullptr,
                                                       int n_q = 0) {
    __shared__ int32_t s_ws[IDCT_BLOCKS][8][9];
    Img m;
    const bool ok = load_img(img + (size_t)blockIdx.y * IMG, n_sets, coef_elems, plane_bytes, pixel_bytes, m, n_q) && m.kind != 0;   // (block-uniform)
    if (!ok || (long long)blockIdx.x * IDCT_BLOCKS >= m.blocks) return;
    const int lb = threadIdx.x >> 3, t = threadIdx.x & 7;
    const long long gb = (long long)blockIdx.x * IDCT_BLOCKS + lb;
    const bool live = gb < m.blocks;
    const int c = gb < m.blocks0 ? 0 : (gb < m.blocks0 + m.nmcu ? 1 : 2);
    if (live) {
        int32_t ws[8];
        const uint8_t* const q = m.kind == 2 ? qsets + (size_t)m.set * QSET + 64 * c : tables[m.set].quant[c == 0 ? m.tq[0] : (c == 1 ? m.tq[1] : m.tq[2])];
        mg_jpeg_idct_column(coef + m.coef_off + gb * 64, q, t, ws);
#pragma unroll
        for (int r = 0; r < 8; ++r) s_ws[lb][r][t] = ws[r];
    }
    __syncthreads();
    if (live) {
        int32_t ws[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) ws[x] = s_ws[lb][t][x];
        union {
            uint8_t b[8];
            uint2 v;
        } o;
        mg_jpeg_idct_row(ws, o.b);
        const long long first = c == 0 ? 0 : (c == 1 ? m.blocks0 : m.blocks0 + m.nmcu);      // the component's first block
        const long long bi = gb - first;
        const int bw = c == 0 ? m.mcux * m.hs : m.mcux;
        const long long by = bi / bw, bx = bi - by * bw;
        // 8 bytes at a multiple of 8: plane offsets are multiples of 64, the pitch 8 bw
        *reinterpret_cast<uint2*>(planes + m.plane_off + first * 64 + (by * 8 + t) * (8LL * bw) + bx * 8) = o.v;
    }
}

__global__ __launch_bounds__(NT) void jpeg_colour_kernel(const int64_t* __restrict__ img, int n_sets, size_t coef_elems,
                                                         const uint8_t* __restrict__ planes, size_t plane_bytes, uint8_t* __restrict__ pixels,
                                                         size_t pixel_bytes, int n_q = 0) {
    Img m;
    const bool ok = load_img(img + (size_t)blockIdx.y * IMG, n_sets, coef_elems, plane_bytes, pixel_bytes, m, n_q) && m.kind != 0;
    if (!ok) return;
    const long long npix = (long long)m.W * m.H, p = (long long)blockIdx.x * NT + threadIdx.x;
    if (blockIdx.x == 0) {                              // the padding up to the next image's start (behind the last: the slack too)
        const long long z = m.pix_off + npix * 3 + threadIdx.x;
        if (z < m.pix_end) pixels[z] = 0;               // (NT bytes at most: ops.jpeg_decode refuses a longer gap)
    }
    if (p >= npix) return;
    const int y = (int)(p / m.W), x = (int)(p - (long long)y * m.W);
    const uint8_t* const p0 = planes + m.plane_off;
    const int pitch0 = 8 * m.mcux * m.hs;
    const int Y = p0[(size_t)y * pitch0 + x];
    uint8_t* const o = pixels + m.pix_off + p * 3;
    if (m.ncomp == 1) {
        o[0] = o[1] = o[2] = (uint8_t)Y;
        return;
    }
    const uint8_t* const p1 = p0 + m.blocks0 * 64, * const p2 = p1 + m.nmcu * 64;
    const int dw = (m.W + m.hs - 1) / m.hs, dh = (m.H + m.vs - 1) / m.vs, pitch = 8 * m.mcux;
    uint8_t rgb[3];
    int cb, cr;
    if (m.kind == 2 && dw <= 2) {                       // (uniform over the image's workgroups; baseline images: never)
        cb = mg_jpeg_chroma(p1, pitch, dw, dh, m.hs, m.vs, x, y, true), cr = mg_jpeg_chroma(p2, pitch, dw, dh, m.hs, m.vs, x, y, true);
    } else {
        cb = mg_jpeg_chroma(p1, pitch, dw, dh, m.hs, m.vs, x, y), cr = mg_jpeg_chroma(p2, pitch, dw, dh, m.hs, m.vs, x, y);
    }
    mg_jpeg_rgb(Y, cb, cr, rgb);
    o[0] = rgb[0];
    o[1] = rgb[1];
    o[2] = rgb[2];
}

// ---- other component layouts (jpeg_layouts.hpp; DESIGN.md 17, "Other component layouts") -----------------------------------------
// An image record of kind 3, with a check of its own: load_img and the kernels above do not know the kind and skip the record.
struct LImg {
    int W, H, ncomp, model, mcux, mcuy, set, hmax, vmax;
    uint32_t h, v, tq, td, ta;            // h, v: a nibble per component; the table ids: a byte per component in the record, 0..3
    long long coef_off, plane_off, pix_off, pix_end;
    long long nmcu, blocks;               // MCUs; blocks of all components
    long long nb0, nb1, nb2, nb3;         // blocks per component, 0 for one the image does not have
};

__device__ __forceinline__ bool load_layout_img(const int64_t* __restrict__ r, int n_sets, size_t coef_elems, size_t plane_bytes,
                                                size_t pixel_bytes, LImg& m) {
    const long long kind = r[0], W = r[1], H = r[2], nm = r[3], hp = r[4], vp = r[5], mcux = r[6], mcuy = r[7], set = r[11];
    m.coef_off = r[12], m.plane_off = r[13], m.pix_off = r[14], m.pix_end = r[15];
    if (kind != 3) return false;
    if (W < 1 || W > MAXEXT || H < 1 || H > MAXEXT) return false;
    if (m.pix_off < 0 || (m.pix_off & 15) || m.pix_end < m.pix_off || (unsigned long long)m.pix_end > pixel_bytes ||
        W * H * 3 > m.pix_end - m.pix_off)
        return false;
    const long long nc = nm & 0xFF, model = nm >> 8;
    if (nm < 0 || hp < 0 || hp > 0xFFFF || vp < 0 || vp > 0xFFFF) return false;
    const int bpm = mg_jpeg_layout_mcu_blocks((int)nc, (uint32_t)hp, (uint32_t)vp);
    if (bpm == 0) return false;
    if (!((nc == 1 && model == MG_JPEG_MODEL_GRAY) || (nc == 3 && (model == MG_JPEG_MODEL_YCC || model == MG_JPEG_MODEL_RGB)) ||
          (nc == 4 && (model == MG_JPEG_MODEL_CMYK || model == MG_JPEG_MODEL_YCCK))))
        return false;
    m.W = (int)W, m.H = (int)H, m.ncomp = (int)nc, m.model = (int)model, m.h = (uint32_t)hp, m.v = (uint32_t)vp;
    m.hmax = m.vmax = 1;
    long long nb[4] = {0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (c < m.ncomp) {
            const int hc = mg_jpeg_nibble(m.h, c), vc = mg_jpeg_nibble(m.v, c);
            m.hmax = hc > m.hmax ? hc : m.hmax, m.vmax = vc > m.vmax ? vc : m.vmax;
            nb[c] = (long long)hc * vc;
        }
    if (mcux != (W + 8 * m.hmax - 1) / (8 * m.hmax) || mcuy != (H + 8 * m.vmax - 1) / (8 * m.vmax)) return false;
    if (set < 0 || set >= n_sets) return false;
    m.mcux = (int)mcux, m.mcuy = (int)mcuy, m.set = (int)set;
    m.nmcu = mcux * mcuy;
    m.nb0 = nb[0] * m.nmcu, m.nb1 = nb[1] * m.nmcu, m.nb2 = nb[2] * m.nmcu, m.nb3 = nb[3] * m.nmcu;
    m.blocks = m.nmcu * bpm;
    if (m.coef_off < 0 || (m.coef_off & 63) || (unsigned long long)m.coef_off + (unsigned long long)m.blocks * 64 > coef_elems) return false;
    if (m.plane_off < 0 || (m.plane_off & 63) || (unsigned long long)m.plane_off + (unsigned long long)m.blocks * 64 > plane_bytes) return false;
    m.tq = m.td = m.ta = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        m.tq |= (uint32_t)((r[8] >> (8 * c)) & 3) << (2 * c);
        m.td |= (uint32_t)((r[9] >> (8 * c)) & 3) << (2 * c);
        m.ta |= (uint32_t)((r[10] >> (8 * c)) & 3) << (2 * c);
    }
    return true;
}

// One lane per segment record of lseg, placed as jpeg_entropy_kernel places its lanes, with the batch's first table sets in LDS.
// A segment is one lane's from its first byte to its last: these segments are never split.
__global__ __launch_bounds__(ENT_NT) void jpeg_layout_entropy_kernel(const uint8_t* __restrict__ data, size_t data_bytes,
                                    const int64_t* __restrict__ img, int B, const int64_t* __restrict__ seg, int S, int lanes,
                                    const MgJpegTables* __restrict__ tables, int n_sets,
                                    int16_t* __restrict__ coef, size_t coef_elems, size_t plane_bytes, size_t pixel_bytes,
                                    int32_t* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) MgJpegTables s_tables[LDS_SETS];
    {
        const int n16 = (n_sets < LDS_SETS ? n_sets : LDS_SETS) * (int)(sizeof(MgJpegTables) / 16);
        const u32x4* const src = reinterpret_cast<const u32x4*>(tables);
        u32x4* const dst = reinterpret_cast<u32x4*>(s_tables);
        for (int i = threadIdx.x; i < n16; i += ENT_NT) dst[i] = src[i];
    }
    __syncthreads();
    const long long s = (long long)blockIdx.x * lanes + threadIdx.x;
    if ((int)threadIdx.x >= lanes || s >= S) return;
    const int64_t* const r = seg + s * SEG;
    const long long im = r[0], b = r[1], e = r[2], mcu0 = r[3], nmcu = r[4];
    LImg m;
    int st = MG_JPEG_SEG_BAD_RECORD;
    if (im >= 0 && im < B && b >= 0 && b <= e && (unsigned long long)e <= data_bytes && mcu0 >= 0 && nmcu >= 1 &&
        load_layout_img(img + im * IMG, n_sets, coef_elems, plane_bytes, pixel_bytes, m) && mcu0 <= m.nmcu - nmcu) {
        MgJpegLayoutSegment g;
        g.ncomp = m.ncomp, g.h = m.h, g.v = m.v, g.td = m.td, g.ta = m.ta;
        g.mcux = m.mcux, g.mcu_total = (int)m.nmcu, g.mcu0 = (int)mcu0, g.nmcu = (int)nmcu;
        int16_t* const c0 = coef + m.coef_off;
        int16_t* const c1 = c0 + m.nb0 * 64;
        int16_t* const c2 = c1 + m.nb1 * 64;
        int16_t* const c3 = c2 + m.nb2 * 64;
        const MgJpegTables* const T = m.set < LDS_SETS ? &s_tables[m.set] : tables + m.set;
        st = mg_jpeg_decode_layout_segment(data + b, data + e, T, g, c0, c1, c2, c3);
    }
    status[s] = st;
}

// jpeg_idct_kernel over the images of kind 3: component c's blocks lie behind those of component c - 1, mcux h_c to a block row
__global__ __launch_bounds__(NT) void jpeg_layout_idct_kernel(const int64_t* __restrict__ img, const MgJpegTables* __restrict__ tables, int n_sets,
                                                              const int16_t* __restrict__ coef, size_t coef_elems, uint8_t* __restrict__ planes,
                                                              size_t plane_bytes, size_t pixel_bytes) {
    __shared__ int32_t s_ws[IDCT_BLOCKS][8][9];
    LImg m;
    const bool ok = load_layout_img(img + (size_t)blockIdx.y * IMG, n_sets, coef_elems, plane_bytes, pixel_bytes, m);   // (block-uniform)
    if (!ok || (long long)blockIdx.x * IDCT_BLOCKS >= m.blocks) return;
    const int lb = threadIdx.x >> 3, t = threadIdx.x & 7;
    const long long gb = (long long)blockIdx.x * IDCT_BLOCKS + lb;
    const bool live = gb < m.blocks;
    const int c = gb < m.nb0 ? 0 : (gb < m.nb0 + m.nb1 ? 1 : (gb < m.nb0 + m.nb1 + m.nb2 ? 2 : 3));
    if (live) {
        int32_t ws[8];
        mg_jpeg_idct_column(coef + m.coef_off + gb * 64, tables[m.set].quant[(m.tq >> (2 * c)) & 3u], t, ws);
#pragma unroll
        for (int r = 0; r < 8; ++r) s_ws[lb][r][t] = ws[r];
    }
    __syncthreads();
    if (live) {
        int32_t ws[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) ws[x] = s_ws[lb][t][x];
        union {
            uint8_t b[8];
            uint2 v;
        } o;
        mg_jpeg_idct_row(ws, o.b);
        const long long first = c == 0 ? 0 : (c == 1 ? m.nb0 : (c == 2 ? m.nb0 + m.nb1 : m.nb0 + m.nb1 + m.nb2));
        const long long bi = gb - first;
        const int bw = m.mcux * mg_jpeg_nibble(m.h, c);
        const long long by = bi / bw, bx = bi - by * bw;
        // 8 bytes at a multiple of 8: plane offsets are multiples of 64, the pitch 8 bw
        *reinterpret_cast<uint2*>(planes + m.plane_off + first * 64 + (by * 8 + t) * (8LL * bw) + bx * 8) = o.v;
    }
}

// One thread per pixel of an image of kind 3: every component upsampled to the largest, the colour model, RGB8 at the image's
// offset; the padding behind the image is zeroed.
__global__ __launch_bounds__(NT) void jpeg_layout_colour_kernel(const int64_t* __restrict__ img, int n_sets, size_t coef_elems,
                                                                const uint8_t* __restrict__ planes, size_t plane_bytes,
                                                                uint8_t* __restrict__ pixels, size_t pixel_bytes) {
    LImg m;
    if (!load_layout_img(img + (size_t)blockIdx.y * IMG, n_sets, coef_elems, plane_bytes, pixel_bytes, m)) return;
    const long long npix = (long long)m.W * m.H, p = (long long)blockIdx.x * NT + threadIdx.x;
    if (blockIdx.x == 0) {                              // the padding up to the next image's start (behind the last: the slack too)
        const long long z = m.pix_off + npix * 3 + threadIdx.x;
        if (z < m.pix_end) pixels[z] = 0;               // (NT bytes at most: ops.jpeg_decode_layouts refuses a longer gap)
    }
    if (p >= npix) return;
    const int y = (int)(p / m.W), x = (int)(p - (long long)y * m.W);
    const uint8_t* plane = planes + m.plane_off;
    const long long nb[4] = {m.nb0, m.nb1, m.nb2, m.nb3};
    int s[4] = {0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (c < m.ncomp) {
            const int hc = mg_jpeg_nibble(m.h, c), vc = mg_jpeg_nibble(m.v, c);
            const int dw = (m.W * hc + m.hmax - 1) / m.hmax, dh = (m.H * vc + m.vmax - 1) / m.vmax;
            s[c] = mg_jpeg_layout_sample(plane, 8 * m.mcux * hc, dw, dh, m.hmax / hc, m.vmax / vc, x, y);
            plane += nb[c] * 64;
        }
    uint8_t rgb[3];
    mg_jpeg_layout_rgb(m.model, s[0], s[1], s[2], s[3], rgb);
    uint8_t* const o = pixels + m.pix_off + p * 3;
    o[0] = rgb[0];
    o[1] = rgb[1];
    o[2] = rgb[2];
}

}  // namespace

extern "C" size_t mgnns_jpeg_tableset_bytes(void) { return sizeof(MgJpegTables); }

extern "C" int mgnns_jpeg_parse(const void* data, size_t bytes, int max_extent, int32_t* info, int64_t* range, int64_t* seg, size_t seg_cap,
                                void* tables) {
    MG_REQUIRE(info && range && tables && (seg || seg_cap == 0) && (data || bytes == 0), "mgnns_jpeg_parse: null pointer");
    MG_REQUIRE(max_extent >= 1 && max_extent <= MAXEXT, "mgnns_jpeg_parse: max_extent=%d (1..%d)", max_extent, MAXEXT);
    static const uint8_t none = 0;
    mg_jpeg_parse(data ? (const uint8_t*)data : &none, bytes, max_extent, info, range, seg, seg_cap, (MgJpegTables*)tables);
    return 0;
}

extern "C" int mgnns_jpeg_decode_fwd(const void* data, size_t data_bytes, const int64_t* img, int B, const int64_t* seg, int S,
                                     const void* tables, int n_sets, void* coef, size_t coef_elems, void* planes, size_t plane_bytes,
                                     void* pixels, size_t pixel_bytes, long long max_blocks, long long max_pixels, int stages,
                                     int32_t* status, mgnns_stream_t stream) {
    MG_REQUIRE(B >= 0 && B <= 65535 && S >= 0, "mgnns_jpeg_decode_fwd: B=%d (0..65535), S=%d", B, S);
    MG_REQUIRE(stages >= 1 && stages <= 7, "mgnns_jpeg_decode_fwd: stages=%d is no mask of 1 (entropy), 2 (IDCT), 4 (colour)", stages);
    if (B == 0 || S == 0) return 0;                // nothing to decode (every image staged by the host, or none at all)
    MG_REQUIRE(data && img && seg && tables && coef && planes && pixels && status, "mgnns_jpeg_decode_fwd: null pointer");
    MG_REQUIRE(n_sets >= 1, "mgnns_jpeg_decode_fwd: no table set");
    MG_REQUIRE(mg_aligned16(coef) && mg_aligned16(planes) && mg_aligned16(pixels) && mg_aligned16(tables),
               "mgnns_jpeg_decode_fwd: coef, planes, pixels and tables must be 16-byte aligned");
    MG_REQUIRE(max_blocks >= 1 && max_blocks <= 6LL * (MAXEXT / 8) * (MAXEXT / 8) && max_pixels >= 1 && max_pixels <= (long long)MAXEXT * MAXEXT,
               "mgnns_jpeg_decode_fwd: max_blocks=%lld, max_pixels=%lld", max_blocks, max_pixels);
    hipStream_t st = (hipStream_t)stream;
    if (stages & 1) {
        hipError_t e = hipMemsetAsync(coef, 0, coef_elems * sizeof(int16_t), st);
        if (e != hipSuccess) {
            mgnns_set_error("mgnns_jpeg_decode_fwd: hipMemsetAsync: %s", hipGetErrorString(e));
            return MGNNS_ERR_LAUNCH;
        }
        // Lanes of one wave serialise wherever their streams diverge, lanes of different waves do not: spread the segments over
        // the SIMDs (4 per CU) before a wave gets a second lane.
        const int cus = mg_cu_count();
        if (cus <= 0) return MGNNS_ERR_LAUNCH;
        int lanes = 1;
        while (lanes < 64 && (long long)lanes * 4 * cus < S) lanes *= 2;
        hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)((S + lanes - 1) / lanes)), dim3(ENT_NT), 0, st, (const uint8_t*)data,
                           data_bytes, img, B, seg, S, lanes, (const MgJpegTables*)tables, n_sets, (int16_t*)coef, coef_elems, plane_bytes,
                           pixel_bytes, status, 0);
        MG_CHECK_LAUNCH("mgnns_jpeg_decode_fwd (entropy)");
    }
    if (stages & 2) {
        hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((max_blocks + IDCT_BLOCKS - 1) / IDCT_BLOCKS), (unsigned)B), dim3(NT), 0, st, img,
                           (const MgJpegTables*)tables, n_sets, (const int16_t*)coef, coef_elems, (uint8_t*)planes, plane_bytes, pixel_bytes);
        MG_CHECK_LAUNCH("mgnns_jpeg_decode_fwd (idct)");
    }
    if (stages & 4) {
        hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)((max_pixels + NT - 1) / NT), (unsigned)B), dim3(NT), 0, st, img, n_sets,
                           coef_elems, (const uint8_t*)planes, plane_bytes, (uint8_t*)pixels, pixel_bytes);
        MG_CHECK_LAUNCH("mgnns_jpeg_decode_fwd (colour)");
    }
    return 0;
}

extern "C" size_t mgnns_jpeg_huff_bytes(void) { return sizeof(MgJpegHuff); }

extern "C" int mgnns_jpeg_parse_progressive(const void* data, size_t bytes, int max_extent, int32_t* info, int64_t* scans, int64_t* seg,
                                            size_t seg_cap, void* pool, void* quant) {
    MG_REQUIRE(info && scans && pool && quant && (seg || seg_cap == 0) && (data || bytes == 0), "mgnns_jpeg_parse_progressive: null pointer");
    MG_REQUIRE(max_extent >= 1 && max_extent <= MAXEXT, "mgnns_jpeg_parse_progressive: max_extent=%d (1..%d)", max_extent, MAXEXT);
    static const uint8_t none = 0;
    mg_jpeg_parse_progressive(data ? (const uint8_t*)data : &none, bytes, max_extent, info, scans, seg, seg_cap, (MgJpegHuff*)pool, (uint8_t*)quant);
    return 0;
}

// The launch sequence of a batch that may mix baseline and progressive files, for mgnns_jpeg_decode_progressive_fwd (split_chunk = 0)
// and mgnns_jpeg_decode_split_fwd: zero the workspace; the baseline segments -- with split_chunk, jpeg_split_kernel over the
// segments mg_jpeg_split_takes takes and jpeg_entropy_kernel over the others, each skipping the other's; the progressive levels;
// IDCT; colour.  `who` names the entry point in error messages.
#define MG_JPEG_LAUNCHED(stage)                                  \
    do {                                                         \
        char where_[96];                                         \
        snprintf(where_, sizeof where_, "%s (" stage ")", who);  \
        MG_CHECK_LAUNCH(where_);                                 \
    } while (0)

static int jpeg_decode_batch(const char* who, int split_chunk, const void* data, size_t data_bytes, const int64_t* img, int B, const int64_t* seg,
                             int S, const void* tables, int n_sets, const int64_t* pseg, const int32_t* level_counts, int n_levels,
                             const void* pool, int n_pool, const void* qsets, int n_q, void* coef, size_t coef_elems, void* planes,
                             size_t plane_bytes, void* pixels, size_t pixel_bytes, long long max_blocks, long long max_pixels, int stages,
                             int32_t* status, mgnns_stream_t stream) {
    MG_REQUIRE(stages >= 1 && stages <= 7, "%s: stages=%d is no mask of 1 (entropy), 2 (IDCT), 4 (colour)", who, stages);
    MG_REQUIRE(B >= 0 && B <= 65535 && S >= 0 && n_levels >= 0 && n_levels <= 64, "%s: B=%d (0..65535), S=%d, n_levels=%d (0..64)", who,
               B, S, n_levels);
    MG_REQUIRE(n_sets >= 0 && n_pool >= 0 && n_q >= 0, "%s: n_sets=%d, n_pool=%d, n_q=%d", who, n_sets, n_pool, n_q);
    MG_REQUIRE(n_levels == 0 || level_counts, "%s: null level_counts", who);
    long long P = 0;
    for (int l = 0; l < n_levels; ++l) {
        MG_REQUIRE(level_counts[l] >= 0, "%s: level_counts[%d]=%d", who, l, level_counts[l]);
        P += level_counts[l];
    }
    MG_REQUIRE(S + P <= 0x7fffffffLL, "%s: %lld segments", who, S + P);
    if (B == 0 || S + P == 0) return 0;            // nothing to decode (every image staged by the host, or none at all)
    MG_REQUIRE(data && img && coef && planes && pixels && status, "%s: null pointer", who);
    MG_REQUIRE(S == 0 || (seg && tables && n_sets >= 1), "%s: baseline segments without a table set", who);
    MG_REQUIRE(P == 0 || (pseg && pool && n_pool >= 1 && n_pool < 0xFFFF && qsets && n_q >= 1),
               "%s: progressive segments without a table pool or quantisation sets", who);
    MG_REQUIRE(mg_aligned16(coef) && mg_aligned16(planes) && mg_aligned16(pixels) && mg_aligned16(tables) && mg_aligned16(pool),
               "%s: coef, planes, pixels, tables and pool must be 16-byte aligned", who);
    MG_REQUIRE(max_blocks >= 1 && max_blocks <= 6LL * (MAXEXT / 8) * (MAXEXT / 8) && max_pixels >= 1 && max_pixels <= (long long)MAXEXT * MAXEXT,
               "%s: max_blocks=%lld, max_pixels=%lld", who, max_blocks, max_pixels);
    hipStream_t st = (hipStream_t)stream;
    if (stages & 1) {
        hipError_t e = hipMemsetAsync(coef, 0, coef_elems * sizeof(int16_t), st);
        if (e != hipSuccess) {
            mgnns_set_error("%s: hipMemsetAsync: %s", who, hipGetErrorString(e));
            return MGNNS_ERR_LAUNCH;
        }
    }
    const int cus = mg_cu_count();
    if (cus <= 0) return MGNNS_ERR_LAUNCH;
    auto lanes_for = [&](long long n) {            // one lane per wave until every SIMD (4 per CU) has one
        int lanes = 1;
        while (lanes < 64 && (long long)lanes * 4 * cus < n) lanes *= 2;
        return lanes;
    };
    if ((stages & 1) && S > 0 && split_chunk > 0) {
        hipLaunchKernelGGL(jpeg_split_kernel, dim3((unsigned)S), dim3(SPLIT_NT), 0, st, (const uint8_t*)data, data_bytes, img, B, seg, S,
                           (const MgJpegTables*)tables, n_sets, (int16_t*)coef, coef_elems, plane_bytes, pixel_bytes, status, split_chunk);
        MG_JPEG_LAUNCHED("split entropy");
    }
    if ((stages & 1) && S > 0) {
        const int lanes = lanes_for(S);
        hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)((S + lanes - 1) / lanes)), dim3(ENT_NT), 0, st, (const uint8_t*)data,
                           data_bytes, img, B, seg, S, lanes, (const MgJpegTables*)tables, n_sets, (int16_t*)coef, coef_elems, plane_bytes,
                           pixel_bytes, status, split_chunk);
        MG_JPEG_LAUNCHED("baseline entropy");
    }
    int first = 0;
    for (int l = 0; (stages & 1) && l < n_levels; ++l) {
        const int count = level_counts[l];
        if (count == 0) continue;
        const int lanes = lanes_for(count);
        hipLaunchKernelGGL(jpeg_progressive_kernel, dim3((unsigned)((count + lanes - 1) / lanes)), dim3(ENT_NT), 0, st, (const uint8_t*)data,
                           data_bytes, img, B, pseg, first, count, lanes, (const MgJpegHuff*)pool, n_pool, n_sets, n_q, (int16_t*)coef, coef_elems,
                           plane_bytes, pixel_bytes, status + S);
        MG_JPEG_LAUNCHED("progressive entropy");
        first += count;
    }
    if (stages & 2) {
        hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((max_blocks + IDCT_BLOCKS - 1) / IDCT_BLOCKS), (unsigned)B), dim3(NT), 0, st, img,
                           (const MgJpegTables*)tables, n_sets, (const int16_t*)coef, coef_elems, (uint8_t*)planes, plane_bytes, pixel_bytes,
                           (const uint8_t*)qsets, n_q);
        MG_JPEG_LAUNCHED("idct");
    }
    if (stages & 4) {
        hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)((max_pixels + NT - 1) / NT), (unsigned)B), dim3(NT), 0, st, img, n_sets, coef_elems,
                           (const uint8_t*)planes, plane_bytes, (uint8_t*)pixels, pixel_bytes, n_q);
        MG_JPEG_LAUNCHED("colour");
    }
    return 0;
}

#undef MG_JPEG_LAUNCHED

extern "C" int mgnns_jpeg_decode_progressive_fwd(const void* data, size_t data_bytes, const int64_t* img, int B, const int64_t* seg, int S,
                                                 const void* tables, int n_sets, const int64_t* pseg, const int32_t* level_counts, int n_levels,
                                                 const void* pool, int n_pool, const void* qsets, int n_q, void* coef, size_t coef_elems,
                                                 void* planes, size_t plane_bytes, void* pixels, size_t pixel_bytes, long long max_blocks,
                                                 long long max_pixels, int stages, int32_t* status, mgnns_stream_t stream) {
    return jpeg_decode_batch("mgnns_jpeg_decode_progressive_fwd", 0, data, data_bytes, img, B, seg, S, tables, n_sets, pseg, level_counts, n_levels,
                             pool, n_pool, qsets, n_q, coef, coef_elems, planes, plane_bytes, pixels, pixel_bytes, max_blocks, max_pixels, stages,
                             status, stream);
}

extern "C" int mgnns_jpeg_decode_split_fwd(const void* data, size_t data_bytes, const int64_t* img, int B, const int64_t* seg, int S,
                                           const void* tables, int n_sets, const int64_t* pseg, const int32_t* level_counts, int n_levels,
                                           const void* pool, int n_pool, const void* qsets, int n_q, void* coef, size_t coef_elems, void* planes,
                                           size_t plane_bytes, void* pixels, size_t pixel_bytes, long long max_blocks, long long max_pixels,
                                           int stages, int32_t* status, mgnns_stream_t stream, int chunk_bytes) {
    MG_REQUIRE(chunk_bytes >= MG_JPEG_SPLIT_MIN_CHUNK && chunk_bytes <= MG_JPEG_SPLIT_MAX_CHUNK && chunk_bytes % 8 == 0,
               "mgnns_jpeg_decode_split_fwd: chunk_bytes=%d is no multiple of 8 in %d..%d", chunk_bytes, MG_JPEG_SPLIT_MIN_CHUNK,
               MG_JPEG_SPLIT_MAX_CHUNK);
    return jpeg_decode_batch("mgnns_jpeg_decode_split_fwd", chunk_bytes, data, data_bytes, img, B, seg, S, tables, n_sets, pseg, level_counts,
                             n_levels, pool, n_pool, qsets, n_q, coef, coef_elems, planes, plane_bytes, pixels, pixel_bytes, max_blocks, max_pixels,
                             stages, status, stream);
}

extern "C" int mgnns_jpeg_parse_layout(const void* data, size_t bytes, int max_extent, int32_t* info, int64_t* range, int64_t* seg,
                                       size_t seg_cap, void* tables) {
    MG_REQUIRE(info && range && tables && (seg || seg_cap == 0) && (data || bytes == 0), "mgnns_jpeg_parse_layout: null pointer");
    MG_REQUIRE(max_extent >= 1 && max_extent <= MAXEXT, "mgnns_jpeg_parse_layout: max_extent=%d (1..%d)", max_extent, MAXEXT);
    static const uint8_t none = 0;
    mg_jpeg_parse_layout(data ? (const uint8_t*)data : &none, bytes, max_extent, info, range, seg, seg_cap, (MgJpegTables*)tables);
    return 0;
}

extern "C" int mgnns_jpeg_decode_layouts_fwd(const void* data, size_t data_bytes, const int64_t* img, int B, const int64_t* seg, int S,
                                             const void* tables, int n_sets, const int64_t* pseg, const int32_t* level_counts, int n_levels,
                                             const void* pool, int n_pool, const void* qsets, int n_q, const int64_t* lseg, int L, void* coef,
                                             size_t coef_elems, void* planes, size_t plane_bytes, void* pixels, size_t pixel_bytes,
                                             long long max_blocks, long long max_pixels, long long lmax_blocks, long long lmax_pixels,
                                             int stages, int32_t* status, mgnns_stream_t stream, int chunk_bytes) {
    const char* const who = "mgnns_jpeg_decode_layouts_fwd";
    MG_REQUIRE(chunk_bytes == 0 || (chunk_bytes >= MG_JPEG_SPLIT_MIN_CHUNK && chunk_bytes <= MG_JPEG_SPLIT_MAX_CHUNK && chunk_bytes % 8 == 0),
               "%s: chunk_bytes=%d is neither 0 nor a multiple of 8 in %d..%d", who, chunk_bytes, MG_JPEG_SPLIT_MIN_CHUNK, MG_JPEG_SPLIT_MAX_CHUNK);
    MG_REQUIRE(L >= 0 && S >= 0 && n_levels >= 0, "%s: L=%d, S=%d, n_levels=%d", who, L, S, n_levels);
    // the images of kind 0, 1 and 2: the launches of the earlier entry points, unchanged (none if there is no such segment)
    const int rc = jpeg_decode_batch(who, chunk_bytes, data, data_bytes, img, B, seg, S, tables, n_sets, pseg, level_counts, n_levels, pool, n_pool,
                                     qsets, n_q, coef, coef_elems, planes, plane_bytes, pixels, pixel_bytes, max_blocks, max_pixels, stages, status,
                                     stream);
    if (rc != 0 || B == 0 || L == 0) return rc;
    long long P = 0;
    for (int l = 0; l < n_levels; ++l) P += level_counts[l];
    MG_REQUIRE(S + P + L <= 0x7fffffffLL, "%s: %lld segments", who, S + P + L);
    MG_REQUIRE(data && img && lseg && tables && n_sets >= 1 && coef && planes && pixels && status, "%s: null pointer or no table set", who);
    MG_REQUIRE(mg_aligned16(coef) && mg_aligned16(planes) && mg_aligned16(pixels) && mg_aligned16(tables),
               "%s: coef, planes, pixels and tables must be 16-byte aligned", who);
    MG_REQUIRE(lmax_blocks >= 1 && lmax_blocks <= 16LL * (MAXEXT / 8) * (MAXEXT / 8) && lmax_pixels >= 1 && lmax_pixels <= (long long)MAXEXT * MAXEXT,
               "%s: lmax_blocks=%lld, lmax_pixels=%lld", who, lmax_blocks, lmax_pixels);
    hipStream_t st = (hipStream_t)stream;
    if ((stages & 1) && S + P == 0) {              // (with S + P > 0 the launches above have zeroed the workspace)
        hipError_t e = hipMemsetAsync(coef, 0, coef_elems * sizeof(int16_t), st);
        if (e != hipSuccess) {
            mgnns_set_error("%s: hipMemsetAsync: %s", who, hipGetErrorString(e));
            return MGNNS_ERR_LAUNCH;
        }
    }
    if (stages & 1) {
        const int cus = mg_cu_count();
        if (cus <= 0) return MGNNS_ERR_LAUNCH;
        int lanes = 1;                             // one lane per wave until every SIMD (4 per CU) has one
        while (lanes < 64 && (long long)lanes * 4 * cus < L) lanes *= 2;
        hipLaunchKernelGGL(jpeg_layout_entropy_kernel, dim3((unsigned)((L + lanes - 1) / lanes)), dim3(ENT_NT), 0, st, (const uint8_t*)data,
                           data_bytes, img, B, lseg, L, lanes, (const MgJpegTables*)tables, n_sets, (int16_t*)coef, coef_elems, plane_bytes,
                           pixel_bytes, status + S + P);
        MG_CHECK_LAUNCH("mgnns_jpeg_decode_layouts_fwd (layout entropy)");
    }
    if (stages & 2) {
        hipLaunchKernelGGL(jpeg_layout_idct_kernel, dim3((unsigned)((lmax_blocks + IDCT_BLOCKS - 1) / IDCT_BLOCKS), (unsigned)B), dim3(NT), 0, st,
                           img, (const MgJpegTables*)tables, n_sets, (const int16_t*)coef, coef_elems, (uint8_t*)planes, plane_bytes, pixel_bytes);
        MG_CHECK_LAUNCH("mgnns_jpeg_decode_layouts_fwd (layout idct)");
    }
    if (stages & 4) {
        hipLaunchKernelGGL(jpeg_layout_colour_kernel, dim3((unsigned)((lmax_pixels + NT - 1) / NT), (unsigned)B), dim3(NT), 0, st, img, n_sets,
                           coef_elems, (const uint8_t*)planes, plane_bytes, (uint8_t*)pixels, pixel_bytes);
        MG_CHECK_LAUNCH("mgnns_jpeg_decode_layouts_fwd (layout colour)");
    }
    return 0;
}
