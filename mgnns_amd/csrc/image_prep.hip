// f4 (input half): the reference's image transforms in front of the trunks, one launch per batch.
//   eval   (utils/Multi_GCN_Co_att_dataset.py:259-264): Warp(S) -> ToTensor -> Normalize
//   train  (engine/Multi_GCN_Multihead_Att_engine.py:273-299): MultiScaleCrop -> RandomHorizontalFlip -> ToTensor -> Normalize
// Both resizes are PIL.Image.resize(..., BILINEAR) on 8-bit channels (utils/util.py:73,93), which is integer arithmetic:
//   horizontal pass over every source row:  t[r][x] = clip8((2^21 + sum_j kx[x][j] * src[r][lo_x[x] + j]) >> 22)   (uint8)
//   vertical pass over its result:          v[y][x] = clip8((2^21 + sum_j ky[y][j] * t[lo_y[y] + j][x]) >> 22)
// with 22-bit fixed-point taps that the host computes in float64 exactly as Pillow does (mgnns_amd/images.py: one plan per
// distinct (extent, S)).  A crop is the sub-array -- taps never reach outside the crop rectangle -- the flip mirrors the
// output columns, and ToTensor + Normalize is a [3,256] table look-up.
//
// Layout.  A workgroup owns a tile of TY x TX output pixels (all three channels) of one image.  Thread (tx, c) owns one
// output column and channel and keeps the tile's TY vertical accumulators in registers.  The workgroup streams the source
// rows the tile's vertical windows cover; of each row only the pixels the tile's horizontal windows cover.  A step moves
// one 16-byte global load per lane: R rows of the segment at once (448-wide output of a photograph: 8 to 16 rows), or, when
// the segment is longer than CHPX pixels, one chunk of one row.  A row is fetched from its start rounded DOWN to 16 bytes
// -- an image starts on a 16-byte boundary, so that never leaves it -- to its end rounded up, at most 15 bytes past the
// image, which is why the buffer is over-allocated.  Registers -> LDS (two buffers, one barrier per step, the next step's
// loads in flight while this one is used).  The horizontal pass reads the 3-byte-pitch pixels from LDS as bytes: the three
// channel threads of a pixel read adjacent bytes of one dword.  A finished row value is multiplied into all TY
// accumulators by the step's [R][TY] matrix of vertical weights (zero outside a row's window), which the threads fetch
// one entry each along with the pixels and read back as LDS broadcasts.  Nothing is sized by the reduction factor:
// 8192 -> 1 just runs more chunks and more rows through the same 17 KB of LDS.  The finished tile goes through LDS once
// more so that a lane stores four consecutive fp32 of one output row (16 bytes) when S_w % 4 == 0.
#include "common.hpp"

namespace {

constexpr int TX = 64;          // output columns of a tile
constexpr int TY = 16;          // output rows of a tile
constexpr int NT = 256;         // threads: 3 * TX of them compute, all of them load and store
constexpr int CHB = 16 * NT;    // bytes of one chunk buffer: one 16-byte load per lane
constexpr int CHPX = (CHB - 16) / 3 / 16 * 16;   // pixels of a chunk: 3 * CHPX + 15 bytes of misalignment fit in CHB
constexpr int RMAX = NT / TY;   // source rows of a step at most: thread wi * TY + wty stages one vertical weight
constexpr int KLDS = 16;        // horizontal plans of up to this many taps per output are staged in LDS
constexpr int MAXEXT = 8192;
constexpr int MAXS = 1024;
constexpr int DESC = 10;

static_assert(3 * CHPX + 15 <= CHB, "a chunk and its misalignment must fit in one buffer");
static_assert(3 * TX <= NT, "one thread per (column, channel)");

struct Plan {
    const int32_t* bounds;      // [S][2]: first source index, tap count
    const int32_t* taps;        // [S][ks]
    int ks;
};

__device__ __forceinline__ bool load_plan(const int32_t* __restrict__ table, int n_plans, const int32_t* __restrict__ data,
                                          size_t plan_ints, long long idx, long long n, int S, Plan& p) {
    if (idx < 0 || idx >= n_plans) return false;
    const int32_t* e = table + 4 * idx;
    const long long off = e[0], ks = e[1];
    if (off < 0 || ks < 1 || ks > 2 * MAXEXT + 1 || e[2] != n || e[3] != S) return false;
    if ((unsigned long long)off + (unsigned long long)S * (2 + ks) > plan_ints) return false;
    p.bounds = data + off;
    p.taps = data + off + 2 * S;
    p.ks = (int)ks;
    return true;
}

__device__ __forceinline__ int clip8(int acc) {
    const int v = (acc + (1 << 21)) >> 22;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// A tap has 22 fractional bits and a pixel 8: the products fit the full-rate 24-bit multiply (v_mad_i32_i24) exactly; a 32-bit
// integer multiply runs at a quarter of that rate.
__device__ __forceinline__ int hpass(const uint8_t* __restrict__ rows, int o, const int32_t* __restrict__ taps, int jb, int je) {
    int acc = 0;
    o += 3 * jb;
    for (int j = jb; j < je; ++j, o += 3) acc += __mul24(taps[j], (int)rows[o]);      // (a 32-bit LDS offset, no pointer arithmetic)
    return acc;
}

__global__ __launch_bounds__(NT) void image_prep_kernel(const uint8_t* __restrict__ pixels, size_t pixel_bytes,
                                                        const int64_t* __restrict__ desc, const int32_t* __restrict__ plan_table,
                                                        int n_plans, const int32_t* __restrict__ plan_data, size_t plan_ints,
                                                        const float* __restrict__ lut, int S_h, int S_w, int tiles_x, int tiles_y,
                                                        float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint8_t s_row[2][CHB];
    __shared__ int32_t s_xtap[TX * KLDS];
    __shared__ __attribute__((aligned(16))) int32_t s_wy[2][RMAX * TY];
    __shared__ uint8_t s_out[3][TY][TX];

    const int tid = threadIdx.x;
    int bid = blockIdx.x;
    const int X0 = (bid % tiles_x) * TX;
    bid /= tiles_x;
    const int Y0 = (bid % tiles_y) * TY;
    const int b = bid / tiles_y;
    const int nxt = min(TX, S_w - X0), nyt = min(TY, S_h - Y0);
    float* const out_b = out + (size_t)b * 3 * S_h * S_w;
    const bool vec = (S_w & 3) == 0;

    // ---- the descriptor, re-checked (wave-uniform: scalar loads and branches) ----
    const int64_t* d = desc + (size_t)b * DESC;
    const long long off = d[0], H = d[1], W = d[2], cx = d[3], cy = d[4], cw = d[5], ch = d[6];
    const bool flip = d[7] != 0;
    Plan px, py;
    bool ok = (off >= 0) && ((off & 15) == 0) && H >= 1 && H <= MAXEXT && W >= 1 && W <= MAXEXT && cx >= 0 && cy >= 0 &&
              cw >= 1 && ch >= 1 && cw <= W && ch <= H && cx <= W - cw && cy <= H - ch &&      // (no sum that a huge cx could wrap)
              (unsigned long long)off + (unsigned long long)(H * W * 3) + 16 <= pixel_bytes;
    ok = ok && load_plan(plan_table, n_plans, plan_data, plan_ints, d[8], cw, S_w, px) &&
         load_plan(plan_table, n_plans, plan_data, plan_ints, d[9], ch, S_h, py);
    if (!ok) {
        const float nan = __builtin_nanf("");
        for (int s = tid; s < 3 * TY * TX; s += NT) {
            const int c = s / (TY * TX), ty = (s / TX) % TY, tx = s % TX;
            if (ty < nyt && tx < nxt) out_b[((size_t)c * S_h + Y0 + ty) * S_w + X0 + tx] = nan;
        }
        return;
    }
    const int n_x = (int)cw, n_y = (int)ch;

    // ---- vertical windows: the source rows [r_begin, r_end) the tile needs (wave-uniform), and this thread's share of a step's
    // vertical weights: thread wi * TY + wty holds the tap that source row wi of the step has in output row wty of the tile ----
    auto ywindow = [&](int ty, int& lo_, int& cnt_) {
        lo_ = min(max(py.bounds[2 * (Y0 + ty)], 0), n_y - 1);
        cnt_ = min(max(py.bounds[2 * (Y0 + ty) + 1], 0), min(py.ks, n_y - lo_));
    };
    int r_begin = n_y, r_end = 0;
    for (int ty = 0; ty < nyt; ++ty) {
        int lo_, cnt_;
        ywindow(ty, lo_, cnt_);
        r_begin = min(r_begin, lo_);
        r_end = max(r_end, lo_ + cnt_);
    }
    const int wi = tid / TY, wty = tid % TY;
    int wlo = 0, wcnt = 0;
    if (wty < nyt) ywindow(wty, wlo, wcnt);
    const int32_t* const wtaps = py.taps + (size_t)(Y0 + (wty < nyt ? wty : 0)) * py.ks;

    // ---- horizontal windows: the tile's source segment [seg_lo, seg_hi) and this thread's own window inside it ----
    const int xr_first = flip ? S_w - 1 - (X0 + nxt - 1) : X0;       // resize columns of the tile, ascending
    const int xr_last = xr_first + nxt - 1;
    const int seg_lo = min(max(px.bounds[2 * xr_first], 0), n_x - 1);
    const int seg_hi = min(max(px.bounds[2 * xr_last] + px.bounds[2 * xr_last + 1], seg_lo + 1), n_x);
    const int tx = tid / 3, c = tid - 3 * tx;
    const bool active = tid < 3 * TX && tx < nxt;
    const int xr = flip ? S_w - 1 - (X0 + tx) : X0 + tx;               // this thread's resize column (output column X0 + tx)
    int lo = seg_lo, cnt = 0;
    if (active) {
        lo = min(max(px.bounds[2 * xr], seg_lo), seg_hi - 1);
        cnt = min(max(px.bounds[2 * xr + 1], 0), min(px.ks, seg_hi - lo));
    }
    const bool lds_taps = px.ks <= KLDS;
    if (lds_taps) {
        for (int s = tid; s < nxt * px.ks; s += NT) {
            const int t = s / px.ks, j = s - t * px.ks;
            const int r = flip ? S_w - 1 - (X0 + t) : X0 + t;
            s_xtap[t * KLDS + j] = px.taps[(size_t)r * px.ks + j];
        }
    }
    const int32_t* const my_gtaps = px.taps + (size_t)(active ? xr : 0) * px.ks;
    const int32_t* const my_ltaps = s_xtap + (active ? tx : 0) * KLDS;

    int acc[TY];
#pragma unroll
    for (int ty = 0; ty < TY; ++ty) acc[ty] = 0;

    // ---- stream the source rows.  A step is one chunk of R rows: a row's chunk spans nb 16-byte blocks (its bytes plus up to 15
    // of misalignment), thread li * nb + lb loads block lb of row li, and R rows fill the NT loads of a step.  A segment longer
    // than a chunk runs one row per step, chunk by chunk. ----
    const int seg = seg_hi - seg_lo;
    const int nch = (seg + CHPX - 1) / CHPX;
    const int nb = nch > 1 ? NT : (3 * seg + 30) / 16;
    const int R = nch > 1 ? 1 : min(NT / nb, RMAX);
    const int li = tid / nb, lb = tid - li * nb;
    const int steps = (max(r_end - r_begin, 0) + R - 1) / R * nch;
    const size_t row_pitch = (size_t)W * 3;
    const size_t origin = (size_t)off + ((size_t)cy * W + cx) * 3;     // byte address of the crop's first pixel

    // step (r0, k) = rows r0 .. r0 + R - 1, pixels [p0, p1) of the crop; a row's bytes are fetched from their start rounded
    // down to 16
    auto fetch = [&](int r0, int k, u32x4& v, int& w) {
        v = u32x4{0u, 0u, 0u, 0u};
        w = 0;
        const int r = r0 + li;
        if (li < R && r < r_end) {
            const int p0 = seg_lo + k * CHPX, p1 = min(seg_hi, p0 + CHPX);
            const size_t rowb = origin + (size_t)r * row_pitch;
            const size_t g0 = rowb + (size_t)p0 * 3, g1 = rowb + (size_t)p1 * 3;
            const size_t a = (g0 & ~(size_t)15) + 16 * (size_t)lb;
            if (a < g1) v = *reinterpret_cast<const u32x4*>(pixels + a);   // a + 16 <= g1 + 15 < pixel_bytes (checked above)
        }
        const int dy = r0 + wi - wlo;                                    // (a row at or past r_end is past every window)
        if (wi < R && (unsigned)dy < (unsigned)wcnt) w = wtaps[dy];
    };

    int r0 = r_begin, k = 0, hacc = 0, prew = 0;
    u32x4 pre = {0u, 0u, 0u, 0u};
    if (steps > 0) fetch(r0, k, pre, prew);
    for (int s = 0; s < steps; ++s) {
        uint8_t* const buf = s_row[s & 1];
        int32_t* const wy = s_wy[s & 1];
        *reinterpret_cast<u32x4*>(buf + 16 * tid) = pre;
        wy[tid] = prew;
        __syncthreads();                                             // publishes buf and wy (and, at s == 0, s_xtap)
        int rn = r0, kn = k + 1;
        if (kn == nch) {
            kn = 0;
            rn += R;
        }
        if (s + 1 < steps) fetch(rn, kn, pre, prew);

        const int p0 = seg_lo + k * CHPX, p1 = min(seg_hi, p0 + CHPX);
        const int jb = max(0, p0 - lo), je = min(cnt, p1 - lo);
        const int rows = min(R, r_end - r0);
        for (int i = 0; i < rows; ++i) {
            // pixel lo + j, channel c of row r0 + i sits at byte 16 * nb * i + (g0 & 15) + 3 * (lo + j - p0) + c of the step's buffer
            // (only the row start's low four bits matter: 32-bit arithmetic keeps them)
            const unsigned g0 = (unsigned)origin + (unsigned)(r0 + i) * (unsigned)row_pitch + 3u * (unsigned)p0;
            const int src = (s & 1) * CHB + 16 * nb * i + (int)(g0 & 15u) + 3 * (lo - p0) + c;
            if (k == 0) hacc = 0;
            hacc += lds_taps ? hpass(&s_row[0][0], src, my_ltaps, jb, je) : hpass(&s_row[0][0], src, my_gtaps, jb, je);
            if (k == nch - 1) {
                const int h = clip8(hacc);
                const i32x4* const w4 = reinterpret_cast<const i32x4*>(wy + TY * i);   // wave-uniform address: a broadcast
#pragma unroll
                for (int q = 0; q < TY / 4; ++q) {
                    const i32x4 w = w4[q];
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[4 * q + e] += __mul24(w[e], h);
                }
            }
        }
        r0 = rn;
        k = kn;
    }

    // ---- table look-up and store, four columns of one output row per lane ----
    if (active) {
#pragma unroll
        for (int ty = 0; ty < TY; ++ty) s_out[c][ty][tx] = (uint8_t)clip8(acc[ty]);
    }
    __syncthreads();
    for (int s = tid; s < 3 * TY * (TX / 4); s += NT) {
        const int cc = s / (TY * (TX / 4)), ty = (s / (TX / 4)) % TY, x4 = (s % (TX / 4)) * 4;
        if (ty >= nyt || x4 >= nxt) continue;
        const float* const t = lut + 256 * cc;
        float* const o = out_b + ((size_t)cc * S_h + Y0 + ty) * S_w + X0 + x4;
        const uint8_t* const v = &s_out[cc][ty][x4];
        if (vec) {                                                   // S_w % 4 == 0: x4 + 3 < nxt and o is 16-byte aligned
            f32x4 q = {t[v[0]], t[v[1]], t[v[2]], t[v[3]]};
            *reinterpret_cast<f32x4*>(o) = q;
        } else {
            for (int i = 0; i < 4 && x4 + i < nxt; ++i) o[i] = t[v[i]];
        }
    }
}

}  // namespace

extern "C" int mgnns_image_prep_fwd(const void* pixels, size_t pixel_bytes, const int64_t* desc, int B, const int32_t* plan_table,
                                    int n_plans, const int32_t* plan_data, size_t plan_ints, const float* lut, int S_h, int S_w,
                                    float* out, mgnns_stream_t stream) {
    MG_REQUIRE(B >= 0, "mgnns_image_prep_fwd: B=%d", B);
    MG_REQUIRE(S_h >= 1 && S_h <= MAXS && S_w >= 1 && S_w <= MAXS, "mgnns_image_prep_fwd: output %dx%d unsupported (1..%d)", S_h, S_w,
               MAXS);
    if (B == 0) return 0;                  // an empty batch has no storage: its data pointers are null
    MG_REQUIRE(pixels && desc && plan_table && plan_data && lut && out, "mgnns_image_prep_fwd: null pointer");
    MG_REQUIRE(n_plans >= 1 && plan_ints >= 1, "mgnns_image_prep_fwd: no plans");
    MG_REQUIRE(mg_aligned16(pixels) && mg_aligned16(out), "mgnns_image_prep_fwd: pixels and out must be 16-byte aligned");
    MG_REQUIRE(pixel_bytes >= 16 + 3, "mgnns_image_prep_fwd: pixel buffer of %zu bytes holds no image", pixel_bytes);
    const int tiles_x = (S_w + TX - 1) / TX, tiles_y = (S_h + TY - 1) / TY;
    const long long blocks = (long long)B * tiles_x * tiles_y;
    MG_REQUIRE(blocks <= 0x7fffffffLL, "mgnns_image_prep_fwd: B=%d at %dx%d is too many tiles for one launch", B, S_h, S_w);
    hipLaunchKernelGGL(image_prep_kernel, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, (const uint8_t*)pixels,
                       pixel_bytes, desc, plan_table, n_plans, plan_data, plan_ints, lut, S_h, S_w, tiles_x, tiles_y, out);
    MG_CHECK_LAUNCH("mgnns_image_prep_fwd");
    return 0;
}
