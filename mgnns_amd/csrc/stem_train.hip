// Backward of the trunks' stem: conv1 7x7 / stride 2 / pad 3 (3 -> 64) and MaxPool2d(3, 2, 1).  The forward is
// stem_conv7_kernel of conv_bf16.hip -- the fp32 NCHW image rounded to bf16 when its patch is staged, fp32 accumulation -- and
// maxpool3x3s2_kernel; these kernels give their gradients:
//
//   stem_wgrad_kernel         dW'[o, (kh, kw, c)] = sum over output pixels (b, oh, ow) of g[b, oh, ow, o] bf16(img[b, c, 2 oh + kh - 3,
//                             2 ow + kw - 3]) and db'[o] = sum g[b, oh, ow, o] on v_mfma_f32_16x16x32_bf16 with the pixels as the
//                             contraction.  A workgroup walks a contiguous run of 8 x 32 output-pixel tiles; per tile the 21 x 69 x 3
//                             patch is staged in LDS as bf16 (the forward's patch[], the forward's rounding) and the tile of g is
//                             staged TRANSPOSED ([row][channel][pixel], two pixels per 32-bit word, as conv_wgrad_kernel does).  A wave
//                             owns two output rows of the tile and keeps the WHOLE 64 x 160 accumulator (k padded from 147; 40 MFMA
//                             tiles, 160 registers) across all its tiles: per 32 pixels it reads four 16-byte g fragments and ten
//                             patch fragments (8 consecutive output pixels of one tap = 8 LDS reads of 16 bits at stride 2) for 40
//                             MFMAs.  Column k = 147 of the patch operand is the constant 1, so db' is row sums on the same pipe.
//                             At the end the four waves add their accumulators in wave order through LDS and the workgroup writes
//                             one partial [64, 160] to the workspace;
//   stem_wgrad_reduce_kernel  adds the partials in a fixed order and drops the padding: no float atomics, bit-identical from call to
//                             call;
//   maxpool3x3s2_bwd_kernel   gather form: one thread = one INPUT pixel x 8 channels; the pixel lies in at most 2 x 2 windows and takes
//                             g_y of those whose FIRST maximum it is (row-major scan of the valid positions with a strict >: torch's
//                             rule; finite inputs).  The argmax is recomputed from x, once per window and workgroup, and lives in LDS
//                             only: no saved index tensor, no atomics.  fp32 sum in window order, one bf16 rounding, optionally
//                             zeroed where x <= 0 (the stem's ReLU, whose output x is).
//
// MFMA operand map (as in conv_train.hip): lane = (fr = lane & 15, fg = lane >> 4) holds index fr and contraction elements
// 8 fg .. 8 fg + 7 of either operand; D = mfma(P, Q, D) gives the lane D[r] = sum P[4 fg + r, .] Q[fr, .].
#include "common.hpp"
#include "bf16.hpp"

namespace {

typedef unsigned short u16;

constexpr int SW_ROWS = 8, SW_COLS = 32;                       // output pixels of a tile: a wave owns two rows, a row is one MFMA k-step
constexpr int SW_PR = 2 * SW_ROWS + 5, SW_PC = 2 * SW_COLS + 5;   // the tile's input patch: 21 x 69 per channel
constexpr int SW_NE = 3 * SW_PR * SW_PC;                       // 4347 patch elements
constexpr int SW_K = 160, SW_KV = 147;                         // k = (kh, kw, c) padded to ten 16-wide MFMA tiles; column 147 = ones
constexpr int SW_LDW = 20;                                     // words per transposed g row: 16 pixel pairs + 4 (16-byte aligned rows)
constexpr int SW_TG_WORDS = SW_ROWS * 64 * SW_LDW;             // 10240 words = 40 KB, also the waves' reduction buffer (40 x 64 x 4 floats)
constexpr int SW_MAX_WG = 256;                                 // partials at most: the accumulator leaves room for one workgroup per CU

struct StemWgradArgs {
    const float* img;     // [B, 3, H, W]
    const u16* g;         // [B, OH, OW, 64]
    float* ws;            // [nwg][64, 160]
    int H, W, OH, OW, ntr, ntc, ntiles, tpw;
};

__global__ __launch_bounds__(256) void stem_wgrad_kernel(const StemWgradArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned int Tg[SW_TG_WORDS];
    __shared__ u16 patch[SW_NE + 5];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fg = lane >> 4;

    // the lane's tap per k tile: k = 16 t + fr = (kh, kw, c)
    int koff[10];
#pragma unroll
    for (int t = 0; t < 10; ++t) {
        const int k = t * 16 + fr;
        const int kh = k / 21, kw = (k % 21) / 3, c = k % 3;
        koff[t] = k < SW_KV ? (c * SW_PR + kh) * SW_PC + kw : 0;
    }
    // tile 9 holds k = 144 .. 159: 144 .. 146 are taps, 147 is the constant 1 (db'), the rest is padding
    const unsigned int tail_and = fr < 3 ? 0xFFFFFFFFu : 0u;
    const unsigned int tail_or = fr == 3 ? 0x3F803F80u : 0u;

    f32x4 acc[10][4];
#pragma unroll
    for (int t = 0; t < 10; ++t)
#pragma unroll
        for (int ot = 0; ot < 4; ++ot) acc[t][ot] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int tile_begin = blockIdx.x * a.tpw;
    const int tile_end = min(a.ntiles, tile_begin + a.tpw);
    constexpr int NIT = (SW_NE + 255) / 256;
    float pv[NIT];
    u32x4 gu[4][2];
    // every global load of a tile at once, into registers: the next tile's are in flight while this tile's MFMAs run
    auto fetch = [&](int tile) {
        const int tc = tile % a.ntc, rest = tile / a.ntc;
        const int tr = rest % a.ntr, b = rest / a.ntr;
        const int or0 = tr * SW_ROWS, oc0 = tc * SW_COLS;
        const int ir0 = 2 * or0 - 3, ic0 = 2 * oc0 - 3;
        const float* src = a.img + (size_t)b * 3 * a.H * a.W;
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            const int e = tid + 256 * i;
            const int c = e / (SW_PR * SW_PC), rem = e - c * (SW_PR * SW_PC);
            const int r = rem / SW_PC, cc = rem - r * SW_PC;
            const int ir = ir0 + r, ic = ic0 + cc;
            pv[i] = 0.f;
            if (e < SW_NE && (unsigned)ir < (unsigned)a.H && (unsigned)ic < (unsigned)a.W) pv[i] = src[((size_t)c * a.H + ir) * a.W + ic];
        }
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int item = tid + 256 * it;                       // (pixel pair, 8-channel chunk) of the tile
            const int chunk = item & 7, pair = item >> 3;
            const int orow = or0 + (pair >> 4), ocol = oc0 + 2 * (pair & 15);
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                gu[it][e] = u32x4{0u, 0u, 0u, 0u};
                if (orow < a.OH && ocol + e < a.OW)
                    gu[it][e] = *reinterpret_cast<const u32x4*>(a.g + (((size_t)b * a.OH + orow) * a.OW + ocol + e) * 64 + chunk * 8);
            }
        }
    };
    // registers -> LDS: the patch as bf16 (the forward's rounding), g transposed with two pixels per word
    auto stash = [&]() {
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            const int e = tid + 256 * i;
            if (e < SW_NE) patch[e] = (u16)mg_bf16x2(pv[i], 0.f);
        }
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int item = tid + 256 * it;
            const int chunk = item & 7, pair = item >> 3;
            unsigned int* dst = Tg + (pair >> 4) * (64 * SW_LDW) + (chunk * 8) * SW_LDW + (pair & 15);
            const u32x4 u0 = gu[it][0], u1 = gu[it][1];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                dst[(2 * i) * SW_LDW] = (u0[i] & 0xFFFFu) | (u1[i] << 16);
                dst[(2 * i + 1) * SW_LDW] = (u0[i] >> 16) | (u1[i] & 0xFFFF0000u);
            }
        }
    };
    fetch(tile_begin);
    for (int tile = tile_begin; tile < tile_end; ++tile) {
        const int or0 = ((tile / a.ntc) % a.ntr) * SW_ROWS;
        stash();
        __syncthreads();
        if (tile + 1 < tile_end) fetch(tile + 1);
#pragma unroll 1
        for (int rr = 0; rr < 2; ++rr) {
            const int orl = 2 * wave + rr;
            if (or0 + orl >= a.OH) break;                          // wave uniform: the row's g is zero
            u32x4 gf[4];
#pragma unroll
            for (int ot = 0; ot < 4; ++ot)
                gf[ot] = *reinterpret_cast<const u32x4*>(Tg + orl * (64 * SW_LDW) + (ot * 16 + fr) * SW_LDW + fg * 4);
            const u16* prow = patch + (2 * orl) * SW_PC + 16 * fg;
#pragma unroll
            for (int t = 0; t < 10; ++t) {
                const u16* p = prow + koff[t];
                unsigned int e[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) e[j] = p[2 * j];
                u32x4 xf;
                xf[0] = e[0] | (e[1] << 16);
                xf[1] = e[2] | (e[3] << 16);
                xf[2] = e[4] | (e[5] << 16);
                xf[3] = e[6] | (e[7] << 16);
                if (t == 9) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) xf[i] = (xf[i] & tail_and) | tail_or;
                }
#pragma unroll
                for (int ot = 0; ot < 4; ++ot)
                    acc[t][ot] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, xf), __builtin_bit_cast(bf16x8, gf[ot]),
                                                                        acc[t][ot], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // acc[t][ot][r] = dW'[o = 16 ot + fr][k = 16 t + 4 fg + r] of this wave's rows: add the four waves in wave order
    float* red = reinterpret_cast<float*>(Tg);
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int t = 0; t < 10; ++t)
#pragma unroll
                for (int ot = 0; ot < 4; ++ot) {
                    f32x4* slot = reinterpret_cast<f32x4*>(red) + (t * 4 + ot) * 64 + lane;
                    *slot = w == 0 ? acc[t][ot] : *slot + acc[t][ot];
                }
        }
        __syncthreads();
    }
    float* out = a.ws + (size_t)blockIdx.x * 64 * SW_K;
    for (int i = tid; i < 40 * 64; i += 256) {
        const int f = i >> 6, l = i & 63;
        const int t = f >> 2, ot = f & 3;
        *reinterpret_cast<f32x4*>(out + (ot * 16 + (l & 15)) * SW_K + t * 16 + (l >> 4) * 4) = reinterpret_cast<const f32x4*>(red)[i];
    }
}

// one block = 32 16-byte columns of the [64, 160] partial x 8 classes of partials (p = y, y + 8, ...), added in class order
__global__ __launch_bounds__(256) void stem_wgrad_reduce_kernel(const float* __restrict__ ws, int npart, float* __restrict__ dW,
                                                                float* __restrict__ db) {
    __shared__ f32x4 part[8][32];
    const int x = threadIdx.x & 31, y = threadIdx.x >> 5;
    const int col = blockIdx.x * 32 + x;                           // < 64 * 160 / 4 = 2560 (the grid is exact)
    f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int p = y; p < npart; p += 8) s += *reinterpret_cast<const f32x4*>(ws + (size_t)p * 64 * SW_K + col * 4);
    part[y][x] = s;
    __syncthreads();
    if (y == 0) {
        for (int j = 1; j < 8; ++j) s += part[j][x];
        const int o = (col * 4) / SW_K, k = (col * 4) % SW_K;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (k + r < SW_KV) dW[o * SW_KV + k + r] = s[r];
            else if (k + r == SW_KV) db[o] = s[r];
        }
    }
}

// the split of the tiles over workgroups: a function of the shape alone, so the summation order is too
void stem_wgrad_split(int B, int OH, int OW, int& ntr, int& ntc, int& ntiles, int& tpw, int& nwg) {
    ntr = (OH + SW_ROWS - 1) / SW_ROWS;
    ntc = (OW + SW_COLS - 1) / SW_COLS;
    ntiles = B * ntr * ntc;
    tpw = (ntiles + SW_MAX_WG - 1) / SW_MAX_WG;
    if (tpw < 1) tpw = 1;
    nwg = (ntiles + tpw - 1) / tpw;
}

int stem_wgrad_geometry(const char* who, int B, int H, int W, int& OH, int& OW) {
    MG_REQUIRE(B >= 0 && H >= 7 && W >= 7, "%s: bad dims B=%d H=%d W=%d (the stem takes images of at least 7 x 7)", who, B, H, W);
    OH = (H - 1) / 2 + 1;
    OW = (W - 1) / 2 + 1;
    MG_REQUIRE((long long)B * H * W < (1ll << 31) - 256, "%s: B*H*W = %lld does not fit 31 bits", who, (long long)B * H * W);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// One workgroup = 8 x 16 input pixels x 64 channels (8 groups of 8) of one image, in two phases.
//  1. The 5 x 9 windows that touch the tile (4 x 8 own it, one more row and column for the odd pixels at its edges): a thread scans
//     one window x 8 channels in row-major order with a strict > and leaves the position of the first maximum, 4 bits per channel,
//     and the window's g_y in LDS.  Positions outside the image count as -inf; a window outside the pooled map gets position 15,
//     which no pixel has.  The nine loads of a window are unconditional (clamped to the window's own centre) and issued together.
//  2. Every pixel gathers: round k of four takes the pixels of parity class (h & 1, w & 1) = (k >> 1, k & 1), which fixes how many
//     windows a pixel lies in ((1 + h & 1) x (1 + w & 1)) and its position in each at compile time, so a wave never diverges.
// The argmax therefore is computed once per window and workgroup -- 45 scans for 128 pixels -- not once per pixel and window.
constexpr int PB_ROWS = 8, PB_COLS = 16;                       // pixel tile
constexpr int PB_WR = PB_ROWS / 2 + 1, PB_WC = PB_COLS / 2 + 1, PB_NWIN = PB_WR * PB_WC;     // 5 x 9 windows
constexpr unsigned int NEG_INF2 = 0xFF80FF80u;                 // two bf16 -inf

template <bool RELU_MASK>
__global__ __launch_bounds__(256) void maxpool3x3s2_bwd_kernel(const u16* __restrict__ x, const u16* __restrict__ gy, int B, int H, int W,
                                                               int C, int OH, int OW, int ntr, int ntc, int ncb, u16* __restrict__ gx) {
    __shared__ uint4 win_g[PB_NWIN][8];
    __shared__ unsigned int win_idx[PB_NWIN][8];
    const int tid = threadIdx.x;
    int t = blockIdx.x;
    const int cb = t % ncb;
    t /= ncb;
    const int tc = t % ntc;
    t /= ntc;
    const int tr = t % ntr, b = t / ntr;
    const int cgi = tid & 7;
    const int c0 = (cb * 8 + cgi) * 8;                             // this thread's first channel
    const bool cok = c0 < C;
    const u16* xb = x + (size_t)b * H * W * C + c0;
    // ---- phase 1: first maximum of every window of the tile
    for (int it = tid; it < PB_NWIN * 8; it += 256) {
        const int win = it >> 3;
        const int wr = win / PB_WC, wc = win - wr * PB_WC;
        const int oh = tr * (PB_ROWS / 2) + wr, ow = tc * (PB_COLS / 2) + wc;
        unsigned int packed = 0xFFFFFFFFu;
        uint4 gv = uint4{0u, 0u, 0u, 0u};
        if (cok && oh < OH && ow < OW) {
            const size_t centre = ((size_t)(2 * oh) * W + 2 * ow) * C;          // (2 oh, 2 ow) always lies inside the image
            uint4 v[9];
#pragma unroll
            for (int pos = 0; pos < 9; ++pos) {
                const int dh = pos / 3 - 1, dw = pos % 3 - 1;
                const bool valid = (unsigned)(2 * oh + dh) < (unsigned)H && (unsigned)(2 * ow + dw) < (unsigned)W;
                v[pos] = *reinterpret_cast<const uint4*>(xb + centre + (valid ? (dh * W + dw) * C : 0));
                if (!valid) v[pos] = uint4{NEG_INF2, NEG_INF2, NEG_INF2, NEG_INF2};
            }
            gv = *reinterpret_cast<const uint4*>(gy + (((size_t)b * OH + oh) * OW + ow) * C + c0);
            float m[8];
            unsigned int idx[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                m[j] = -INFINITY;
                idx[j] = 15u;
            }
#pragma unroll
            for (int pos = 0; pos < 9; ++pos) {
                const unsigned int u[4] = {v[pos].x, v[pos].y, v[pos].z, v[pos].w};
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float q = (j & 1) ? mg_bf16_f32(u[j >> 1] >> 16) : mg_bf16_f32(u[j >> 1] & 0xFFFFu);
                    const bool better = q > m[j];
                    m[j] = better ? q : m[j];
                    idx[j] = better ? (unsigned)pos : idx[j];
                }
            }
            packed = 0u;
#pragma unroll
            for (int j = 0; j < 8; ++j) packed |= idx[j] << (4 * j);
        }
        win_idx[win][cgi] = packed;
        win_g[win][cgi] = gv;
    }
    __syncthreads();
    // ---- phase 2: every pixel takes g_y of the windows whose first maximum it is
    const int c2 = (tid >> 3) & 7, r2 = tid >> 6;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ph = k >> 1, pw = k & 1;
        const int h = tr * PB_ROWS + 2 * r2 + ph, w = tc * PB_COLS + 2 * c2 + pw;
        if (!cok || h >= H || w >= W) continue;
        float sum[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) sum[j] = 0.f;
        // windows oh with 2 oh - 1 <= h <= 2 oh + 1: h / 2 for an even row, h / 2 and h / 2 + 1 for an odd one
#pragma unroll
        for (int wa = 0; wa <= ph; ++wa)
#pragma unroll
            for (int wb = 0; wb <= pw; ++wb) {
                const unsigned int mine = (unsigned)((ph + 1 - 2 * wa) * 3 + (pw + 1 - 2 * wb));   // this pixel's place in the window's scan
                const int win = (r2 + wa) * PB_WC + c2 + wb;
                const unsigned int packed = win_idx[win][cgi];
                const uint4 gv = win_g[win][cgi];
                const unsigned int gu[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float gj = (j & 1) ? mg_bf16_f32(gu[j >> 1] >> 16) : mg_bf16_f32(gu[j >> 1] & 0xFFFFu);
                    sum[j] += ((packed >> (4 * j)) & 15u) == mine ? gj : 0.f;
                }
            }
        const size_t self = ((size_t)h * W + w) * C;
        if (RELU_MASK) {
            const uint4 cv = *reinterpret_cast<const uint4*>(xb + self);
            const unsigned int cu[4] = {cv.x, cv.y, cv.z, cv.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float cj = (j & 1) ? mg_bf16_f32(cu[j >> 1] >> 16) : mg_bf16_f32(cu[j >> 1] & 0xFFFFu);
                if (!(cj > 0.f)) sum[j] = 0.f;
            }
        }
        uint4 o;
        o.x = mg_bf16x2(sum[0], sum[1]);
        o.y = mg_bf16x2(sum[2], sum[3]);
        o.z = mg_bf16x2(sum[4], sum[5]);
        o.w = mg_bf16x2(sum[6], sum[7]);
        *reinterpret_cast<uint4*>(gx + (size_t)b * H * W * C + self + c0) = o;
    }
}

}  // namespace

extern "C" size_t mgnns_stem_wgrad_workspace_bytes(int B, int H, int W) {
    int OH = 0, OW = 0;
    if (stem_wgrad_geometry("mgnns_stem_wgrad_workspace_bytes", B, H, W, OH, OW) || B == 0) return 0;
    int ntr, ntc, ntiles, tpw, nwg;
    stem_wgrad_split(B, OH, OW, ntr, ntc, ntiles, tpw, nwg);
    return (size_t)nwg * 64 * SW_K * sizeof(float);
}

extern "C" int mgnns_stem_wgrad(const float* img, const void* g, int B, int H, int W, float* dW, float* db, void* workspace,
                                size_t workspace_bytes, mgnns_stream_t stream) {
    int OH = 0, OW = 0;
    if (int rc = stem_wgrad_geometry("mgnns_stem_wgrad", B, H, W, OH, OW)) return rc;
    MG_REQUIRE(dW && db, "mgnns_stem_wgrad: null output");
    if (B == 0) {
        hipError_t e = hipMemsetAsync(dW, 0, (size_t)64 * SW_KV * sizeof(float), (hipStream_t)stream);
        if (e == hipSuccess) e = hipMemsetAsync(db, 0, (size_t)64 * sizeof(float), (hipStream_t)stream);
        MG_REQUIRE(e == hipSuccess, "mgnns_stem_wgrad: memset failed: %s", hipGetErrorString(e));
        return 0;
    }
    MG_REQUIRE(img && g && workspace, "mgnns_stem_wgrad: null pointer");
    MG_REQUIRE(mg_aligned16(g) && mg_aligned16(workspace), "mgnns_stem_wgrad: g and the workspace must be 16-byte aligned (B=%d H=%d W=%d)",
               B, H, W);
    StemWgradArgs a;
    int nwg;
    stem_wgrad_split(B, OH, OW, a.ntr, a.ntc, a.ntiles, a.tpw, nwg);
    const size_t need = (size_t)nwg * 64 * SW_K * sizeof(float);
    MG_REQUIRE(workspace_bytes >= need, "mgnns_stem_wgrad: workspace of %zu bytes, %zu needed (mgnns_stem_wgrad_workspace_bytes)",
               workspace_bytes, need);
    a.img = img;
    a.g = reinterpret_cast<const u16*>(g);
    a.ws = reinterpret_cast<float*>(workspace);
    a.H = H; a.W = W; a.OH = OH; a.OW = OW;
    hipLaunchKernelGGL(stem_wgrad_kernel, dim3(nwg), dim3(256), 0, (hipStream_t)stream, a);
    MG_CHECK_LAUNCH("mgnns_stem_wgrad");
    hipLaunchKernelGGL(stem_wgrad_reduce_kernel, dim3(64 * SW_K / 4 / 32), dim3(256), 0, (hipStream_t)stream, a.ws, nwg, dW, db);
    MG_CHECK_LAUNCH("mgnns_stem_wgrad (reduce)");
    return 0;
}

extern "C" int mgnns_maxpool3x3s2_nhwc_bwd(const void* x, const void* gy, int B, int H, int W, int C, int relu_mask, void* gx,
                                           mgnns_stream_t stream) {
    MG_REQUIRE(B >= 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, "mgnns_maxpool3x3s2_nhwc_bwd: need C %% 8 == 0 (B=%d H=%d W=%d C=%d)", B, H, W, C);
    if (B == 0) return 0;
    MG_REQUIRE(x && gy && gx, "mgnns_maxpool3x3s2_nhwc_bwd: null pointer");
    MG_REQUIRE(mg_aligned16(x) && mg_aligned16(gy) && mg_aligned16(gx), "mgnns_maxpool3x3s2_nhwc_bwd: operands must be 16-byte aligned");
    const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
    const int ntr = (H + PB_ROWS - 1) / PB_ROWS, ntc = (W + PB_COLS - 1) / PB_COLS, ncb = (C / 8 + 7) / 8;
    const long long blocks = (long long)B * ntr * ntc * ncb;
    MG_REQUIRE(blocks < (1ll << 31), "mgnns_maxpool3x3s2_nhwc_bwd: %lld tiles do not fit a launch (B=%d H=%d W=%d C=%d)", blocks, B, H, W, C);
    const u16* xp = reinterpret_cast<const u16*>(x);
    const u16* gp = reinterpret_cast<const u16*>(gy);
    if (relu_mask)
        hipLaunchKernelGGL(maxpool3x3s2_bwd_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, xp, gp, B, H, W, C, OH,
                           OW, ntr, ntc, ncb, reinterpret_cast<u16*>(gx));
    else
        hipLaunchKernelGGL(maxpool3x3s2_bwd_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, xp, gp, B, H, W, C, OH,
                           OW, ntr, ntc, ncb, reinterpret_cast<u16*>(gx));
    MG_CHECK_LAUNCH("mgnns_maxpool3x3s2_nhwc_bwd");
    return 0;
}
