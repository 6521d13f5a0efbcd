// Backward of the trunks' bottleneck convolutions (frozen-statistics fine-tuning): the forward is the eval
// forward of conv_bf16.hip -- BatchNorm folded into bf16 weights w'[o, (kh, kw, c)], NHWC bf16 activations -- and these
// kernels give its gradients on v_mfma_f32_16x16x32_bf16 with fp32 accumulation:
//
//   conv_transpose_pack_kernel  derived pack of the data gradient: wT[c, (kh, kw, o)] = w'[o, (kh, kw, c)]
//   conv_dgrad_kernel           dX[b, ih, iw, c] = sum over (kh, kw, o) of dY[b, oh, ow, o] wT[c, (kh, kw, o)] with
//                               oh * s - p + kh = ih, ow * s - p + kw = iw (a gather that also tests divisibility by s),
//                               epilogue dX = mask > 0 ? acc + add : 0, one bf16 rounding
//   conv_wgrad_kernel           dW'[o, (kh, kw, c)] = sum over pixels m of dY[m, o] X[pixel(m, kh, kw), c], db'[o] = sum_m dY[m, o]:
//                               the contraction runs over pixels while both operands are channel contiguous, so a step's
//                               32 pixels x 64 channels of each operand are written to LDS TRANSPOSED ([channel][pixel],
//                               two pixels per 32-bit word) and read back as 16-byte MFMA fragments.  The pixels are
//                               split into shares across workgroups; shares land in a workspace and
//   conv_wgrad_reduce_kernel    adds them in share order: no float atomics, bit-identical from call to call
//   conv_bn_unfold_kernel       gradients of the fp32 master parameters from dW' / db' (the bf16 rounding of w' is the identity)
//   map_grad_relu_kernel        the entry: g[b, p, c] = bf16(map[b, c, p] > 0 ? dmap[b, c, p] : 0), fp32 NCHW -> bf16 NHWC
//
// MFMA operand map (as in conv_bf16.hip): lane = (fr = lane & 15, fg = lane >> 4) holds index fr and k = 8 fg .. 8 fg + 7 of
// either operand; D = mfma(P, Q, D) gives the lane D[r] = sum_k P[4 fg + r, k] Q[fr, k].
#include "common.hpp"
#include "bf16.hpp"

namespace {

typedef unsigned short u16;

__global__ __launch_bounds__(256) void conv_transpose_pack_kernel(const u16* __restrict__ wt, int Cout, int Cin, int taps,
                                                                  u16* __restrict__ wT) {
    const size_t total = (size_t)Cout * taps * Cin;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int o = (int)(i % Cout);
        const size_t r = i / Cout;
        const int tap = (int)(r % taps), c = (int)(r / taps);
        wT[i] = wt[((size_t)o * taps + tap) * Cin + c];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Data gradient.  One workgroup = 128 input pixels x 64 input channels, a wave = 32 pixels x 64 channels (2 x 4 MFMA tiles);
// the fragments come straight from global memory (a dY row of a tap and a wT row are both contiguous in o).
struct DgradArgs {
    const u16* dy;      // [B, OH, OW, Cout]
    const u16* wT;      // [Cin, KH*KW*Cout]
    const u16* mask;    // [B, H, W, Cin] or null
    const u16* add;     // [B, H, W, Cin] or null
    u16* dx;            // [B, H, W, Cin]
    int H, W, Cin, OH, OW, Cout, KH, KW, stride, pad, M;
};

__global__ __launch_bounds__(256) void conv_dgrad_kernel(const DgradArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fr = lane & 15, fg = lane >> 4;
    const int n0 = blockIdx.y * 64;
    const int m0 = blockIdx.x * 128 + wave * 32;
    const int hw = a.H * a.W;
    int pb[2], ph[2], pw[2];
    bool pv[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = m0 + i * 16 + fr;
        pv[i] = m < a.M;
        const int mm = pv[i] ? m : 0;
        pb[i] = mm / hw;
        const int r = mm - pb[i] * hw;
        ph[i] = r / a.W;
        pw[i] = r - ph[i] * a.W;
    }
    f32x4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const size_t KT = (size_t)a.KH * a.KW * a.Cout;
    const u16* wrow[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) wrow[j] = a.wT + (size_t)(n0 + j * 16 + fr) * KT + fg * 8;

    for (int kh = 0; kh < a.KH; ++kh)
        for (int kw = 0; kw < a.KW; ++kw) {
            const u16* ap[2];
            bool ok[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int th = ph[i] + a.pad - kh, tw = pw[i] + a.pad - kw;
                const int oh = th / a.stride, ow = tw / a.stride;
                ok[i] = pv[i] && th >= 0 && tw >= 0 && oh * a.stride == th && ow * a.stride == tw && oh < a.OH && ow < a.OW;
                ap[i] = ok[i] ? a.dy + (((size_t)pb[i] * a.OH + oh) * a.OW + ow) * a.Cout + fg * 8 : a.dy;
            }
            if (!__any(ok[0] || ok[1])) continue;                  // wave uniform: no pixel of this wave meets the tap
            const size_t toff = (size_t)(kh * a.KW + kw) * a.Cout;
            for (int o0 = 0; o0 < a.Cout; o0 += 32) {
                u32x4 av[2], bv[4];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    av[i] = u32x4{0u, 0u, 0u, 0u};
                    if (ok[i]) av[i] = *reinterpret_cast<const u32x4*>(ap[i] + o0);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) bv[j] = *reinterpret_cast<const u32x4*>(wrow[j] + toff + o0);
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, bv[j]),
                                                                           __builtin_bit_cast(bf16x8, av[i]), acc[i][j], 0, 0, 0);
            }
        }
    // acc[i][j][r] = dX[pixel m0 + 16 i + fr][channel n0 + 16 j + 4 fg + r]
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        if (!pv[i]) continue;
        const size_t row = (size_t)(m0 + i * 16 + fr) * a.Cin;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const size_t off = row + n0 + j * 16 + fg * 4;
            float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
            if (a.add) {
                const uint2 u = *reinterpret_cast<const uint2*>(a.add + off);
                v[0] += mg_bf16_f32(u.x & 0xFFFFu);
                v[1] += mg_bf16_f32(u.x >> 16);
                v[2] += mg_bf16_f32(u.y & 0xFFFFu);
                v[3] += mg_bf16_f32(u.y >> 16);
            }
            if (a.mask) {
                const uint2 u = *reinterpret_cast<const uint2*>(a.mask + off);
                if (!(mg_bf16_f32(u.x & 0xFFFFu) > 0.f)) v[0] = 0.f;
                if (!(mg_bf16_f32(u.x >> 16) > 0.f)) v[1] = 0.f;
                if (!(mg_bf16_f32(u.y & 0xFFFFu) > 0.f)) v[2] = 0.f;
                if (!(mg_bf16_f32(u.y >> 16) > 0.f)) v[3] = 0.f;
            }
            uint2 o;
            o.x = mg_bf16x2(v[0], v[1]);
            o.y = mg_bf16x2(v[2], v[3]);
            *reinterpret_cast<uint2*>(a.dx + off) = o;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Weight gradient.  One workgroup = 64 output channels x 64 columns k = (tap, c) (inside one tap: Cin is a power of two >= 64)
// x one share of the pixels; a wave = 32 x 32 (2 x 2 MFMA tiles).  Per step of 32 pixels threads 0..127 stage dY and threads
// 128..255 stage X: a thread loads the same 8 channels of two neighbouring pixels and writes eight 32-bit words
// (pixel 2q | pixel 2q+1 << 16) into the [channel][pixel] image, rows of 16 words + 4 of padding.  The next step's global
// loads are in flight while this step's MFMAs run.  Workgroups of the first column tile also sum dY over pixels (db').
constexpr int WG_SHARE_MIN = 512;      // pixels below which the reduction is not split further
constexpr int WG_LDW = 20;             // words per LDS row: 16 pixel pairs + 4 (16-byte aligned rows)

struct WgradArgs {
    const u16* x;       // [B, H, W, Cin]
    const u16* dy;      // [M, Cout]
    float* out;         // [nshare][Cout, K] (the workspace) or dW' itself when nshare == 1
    float* dbout;       // [nshare][Cout] or db'
    int H, W, Cin, cin_shift, OH, OW, Cout, KW, stride, pad, M, K, share_len;
};

__global__ __launch_bounds__(256) void conv_wgrad_kernel(const WgradArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned int Tdy[64 * WG_LDW];
    __shared__ __attribute__((aligned(16))) unsigned int Tx[64 * WG_LDW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fg = lane >> 4;
    const int o0 = blockIdx.x * 64, k0 = blockIdx.y * 64, share = blockIdx.z;
    const int tap = k0 >> a.cin_shift, c0 = k0 & (a.Cin - 1);
    const int kh = tap / a.KW, kw = tap - kh * a.KW;
    const int p_begin = share * a.share_len;
    const int p_end = min(a.M, p_begin + a.share_len);
    const int nstep = p_end > p_begin ? (p_end - p_begin + 31) / 32 : 0;
    const int ohw = a.OH * a.OW;
    const bool is_x = tid >= 128;
    const int q = (tid & 127) >> 3, chunk = tid & 7;
    const bool want_db = blockIdx.y == 0;

    auto fetch = [&](int step, u32x4& u0, u32x4& u1) {
        u32x4 u[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            u[e] = u32x4{0u, 0u, 0u, 0u};
            const int m = p_begin + step * 32 + 2 * q + e;
            if (m >= p_end) continue;
            if (!is_x) {
                u[e] = *reinterpret_cast<const u32x4*>(a.dy + (size_t)m * a.Cout + o0 + chunk * 8);
            } else {
                const int b = m / ohw, r = m - b * ohw;
                const int oh = r / a.OW, ow = r - oh * a.OW;
                const int ih = oh * a.stride - a.pad + kh, iw = ow * a.stride - a.pad + kw;
                if ((unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W)
                    u[e] = *reinterpret_cast<const u32x4*>(a.x + (((size_t)b * a.H + ih) * a.W + iw) * a.Cin + c0 + chunk * 8);
            }
        }
        u0 = u[0];
        u1 = u[1];
    };

    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float dbacc = 0.f;
    const int wo = wave >> 1, wc = wave & 1;
    unsigned int* dst = (is_x ? Tx : Tdy) + (chunk * 8) * WG_LDW + q;
    u32x4 u0, u1;
    if (nstep > 0) fetch(0, u0, u1);
    for (int s = 0; s < nstep; ++s) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            dst[(2 * i) * WG_LDW] = (u0[i] & 0xFFFFu) | (u1[i] << 16);
            dst[(2 * i + 1) * WG_LDW] = (u0[i] >> 16) | (u1[i] & 0xFFFF0000u);
        }
        __syncthreads();
        if (s + 1 < nstep) fetch(s + 1, u0, u1);
        u32x4 xf[2], yf[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            xf[t] = *reinterpret_cast<const u32x4*>(Tx + (wc * 32 + t * 16 + fr) * WG_LDW + fg * 4);
            yf[t] = *reinterpret_cast<const u32x4*>(Tdy + (wo * 32 + t * 16 + fr) * WG_LDW + fg * 4);
        }
#pragma unroll
        for (int tc = 0; tc < 2; ++tc)
#pragma unroll
            for (int to = 0; to < 2; ++to)
                acc[tc][to] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, xf[tc]),
                                                                     __builtin_bit_cast(bf16x8, yf[to]), acc[tc][to], 0, 0, 0);
        if (want_db && tid < 64) {
#pragma unroll
            for (int w = 0; w < 16; ++w) {
                const unsigned int v = Tdy[tid * WG_LDW + w];
                dbacc += mg_bf16_f32(v & 0xFFFFu);
                dbacc += mg_bf16_f32(v >> 16);
            }
        }
        __syncthreads();
    }
    // acc[tc][to][r] = dW'[o0 + 32 wo + 16 to + fr][k0 + 32 wc + 16 tc + 4 fg + r]
    float* out = a.out + (size_t)share * a.Cout * a.K;
#pragma unroll
    for (int tc = 0; tc < 2; ++tc)
#pragma unroll
        for (int to = 0; to < 2; ++to)
            *reinterpret_cast<f32x4*>(out + (size_t)(o0 + wo * 32 + to * 16 + fr) * a.K + k0 + wc * 32 + tc * 16 + fg * 4) = acc[tc][to];
    if (want_db && tid < 64) a.dbout[(size_t)share * a.Cout + o0 + tid] = dbacc;
}

__global__ __launch_bounds__(256) void conv_wgrad_reduce_kernel(const float* __restrict__ ws, size_t n, int nshare,
                                                                float* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float s = ws[i];
        for (int k = 1; k < nshare; ++k) s += ws[(size_t)k * n + i];
        out[i] = s;
    }
}

// shares of the pixel reduction: enough workgroups to fill the chip, never shares below WG_SHARE_MIN pixels; a function of the
// shape alone, so the summation order is too
void wgrad_shares(long long M, int Cout, int K, int& nshare, int& share_len) {
    const long long tiles = (long long)(Cout / 64) * (K / 64);
    long long want = 1024 / tiles;
    if (want < 1) want = 1;
    long long most = (M + WG_SHARE_MIN - 1) / WG_SHARE_MIN;
    if (most < 1) most = 1;
    long long n = want < most ? want : most;
    long long len = ((M + n - 1) / n + 31) / 32 * 32;
    if (len < 32) len = 32;
    share_len = (int)len;
    nshare = (int)((M + len - 1) / len);
    if (nshare < 1) nshare = 1;
}

// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void conv_bn_unfold_kernel(const float* __restrict__ dwp, const float* __restrict__ dbp,
                                                             const float* __restrict__ w, const float* __restrict__ gamma,
                                                             const float* __restrict__ mean, const float* __restrict__ var,
                                                             float eps, int Cin, int KH, int KW, float* __restrict__ dw,
                                                             float* __restrict__ dgamma, float* __restrict__ dbeta) {
    __shared__ float red[256];
    const int o = blockIdx.x, K = KH * KW * Cin;
    const float r = 1.0f / sqrtf(var[o] + eps);
    const float scale = gamma[o] * r;
    float s = 0.f;
    for (int k = threadIdx.x; k < K; k += 256) {
        const int kh = k / (KW * Cin), kw = (k / Cin) % KW, c = k % Cin;
        const size_t wi = (((size_t)o * Cin + c) * KH + kh) * KW + kw;
        const float g = dwp[(size_t)o * K + k];
        s += w[wi] * g;
        if (dw) dw[wi] = scale * g;
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (dgamma) dgamma[o] = r * (red[0] - mean[o] * dbp[o]);
        if (dbeta) dbeta[o] = dbp[o];
    }
}

// one thread = one pixel x 8 channels; neighbouring threads take neighbouring pixels (the fp32 NCHW reads coalesce)
__global__ __launch_bounds__(256) void map_grad_relu_kernel(const float* __restrict__ map, const float* __restrict__ dmap,
                                                            int B, int C, int P, u16* __restrict__ g) {
    const int cg = C >> 3;
    const size_t total = (size_t)B * cg * P;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int p = (int)(i % P);
        const size_t r = i / P;
        const int c8 = (int)(r % cg), b = (int)(r / cg);
        const size_t src = ((size_t)b * C + c8 * 8) * P + p;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = map[src + (size_t)j * P] > 0.f ? dmap[src + (size_t)j * P] : 0.f;
        uint4 o;
        o.x = mg_bf16x2(v[0], v[1]);
        o.y = mg_bf16x2(v[2], v[3]);
        o.z = mg_bf16x2(v[4], v[5]);
        o.w = mg_bf16x2(v[6], v[7]);
        *reinterpret_cast<uint4*>(g + ((size_t)b * P + p) * C + c8 * 8) = o;
    }
}

unsigned eltwise_blocks(size_t total) {
    size_t blocks = (total + 255) / 256;
    if (blocks > 256 * 64) blocks = 256 * 64;
    if (blocks < 1) blocks = 1;
    return (unsigned)blocks;
}

bool pow2_ge64(int c) { return c >= 64 && (c & (c - 1)) == 0; }

// the geometry every entry point of this file accepts; OH / OW of the forward convolution
int conv_train_geometry(const char* who, int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int& OH,
                        int& OW) {
    MG_REQUIRE(B >= 0 && H > 0 && W > 0, "%s: bad dims B=%d H=%d W=%d", who, B, H, W);
    MG_REQUIRE(pow2_ge64(Cin) && pow2_ge64(Cout), "%s: C_in and C_out must be powers of two >= 64 (got C_in=%d C_out=%d, B=%d H=%d W=%d)",
               who, Cin, Cout, B, H, W);
    MG_REQUIRE((KH == 1 && KW == 1) || (KH == 3 && KW == 3), "%s: kernel must be 1x1 or 3x3 (got %dx%d, C_in=%d C_out=%d)", who, KH, KW,
               Cin, Cout);
    MG_REQUIRE((stride == 1 || stride == 2) && pad >= 0 && pad <= KH / 2, "%s: bad stride %d / padding %d (%dx%d, C_in=%d C_out=%d)", who,
               stride, pad, KH, KW, Cin, Cout);
    // an image smaller than the kernel has no output pixel; C's division truncates towards zero, so (H + 2 pad - KH) / stride + 1
    // alone calls H = 2, 3x3, pad 0, stride 2 one pixel
    MG_REQUIRE(H + 2 * pad >= KH && W + 2 * pad >= KW, "%s: empty output (H=%d W=%d k=%d stride=%d pad=%d)", who, H, W, KH, stride, pad);
    OH = (H + 2 * pad - KH) / stride + 1;
    OW = (W + 2 * pad - KW) / stride + 1;
    MG_REQUIRE((long long)B * H * W < (1ll << 31) - 256 && (long long)B * OH * OW < (1ll << 31) - 256,
               "%s: B*H*W = %lld does not fit 31 bits", who, (long long)B * H * W);
    return 0;
}

}  // namespace

extern "C" int mgnns_conv_transpose_pack_bf16(const void* wt, int Cout, int Cin, int KH, int KW, void* wT, mgnns_stream_t stream) {
    MG_REQUIRE(wt && wT, "mgnns_conv_transpose_pack_bf16: null pointer");
    MG_REQUIRE(Cout > 0 && Cin > 0 && KH > 0 && KW > 0, "mgnns_conv_transpose_pack_bf16: bad dims Cout=%d Cin=%d KH=%d KW=%d", Cout, Cin, KH, KW);
    const size_t total = (size_t)Cout * Cin * KH * KW;
    hipLaunchKernelGGL(conv_transpose_pack_kernel, dim3(eltwise_blocks(total)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const u16*>(wt), Cout, Cin, KH * KW, reinterpret_cast<u16*>(wT));
    MG_CHECK_LAUNCH("mgnns_conv_transpose_pack_bf16");
    return 0;
}

extern "C" int mgnns_conv_dgrad_bf16_nhwc(const void* dy, int B, int H, int W, int Cin, const void* wT, int Cout, int KH, int KW,
                                          int stride, int pad, const void* mask, const void* add, void* dx, mgnns_stream_t stream) {
    int OH = 0, OW = 0;
    if (int rc = conv_train_geometry("mgnns_conv_dgrad_bf16_nhwc", B, H, W, Cin, Cout, KH, KW, stride, pad, OH, OW)) return rc;
    if (B == 0) return 0;
    MG_REQUIRE(dy && wT && dx, "mgnns_conv_dgrad_bf16_nhwc: null pointer");
    MG_REQUIRE(mg_aligned16(dy) && mg_aligned16(wT) && mg_aligned16(dx) && (!mask || mg_aligned16(mask)) && (!add || mg_aligned16(add)),
               "mgnns_conv_dgrad_bf16_nhwc: operands must be 16-byte aligned (B=%d H=%d W=%d C_in=%d C_out=%d)", B, H, W, Cin, Cout);
    DgradArgs a;
    a.dy = reinterpret_cast<const u16*>(dy);
    a.wT = reinterpret_cast<const u16*>(wT);
    a.mask = reinterpret_cast<const u16*>(mask);
    a.add = reinterpret_cast<const u16*>(add);
    a.dx = reinterpret_cast<u16*>(dx);
    a.H = H; a.W = W; a.Cin = Cin; a.OH = OH; a.OW = OW; a.Cout = Cout; a.KH = KH; a.KW = KW; a.stride = stride; a.pad = pad;
    a.M = B * H * W;
    hipLaunchKernelGGL(conv_dgrad_kernel, dim3((a.M + 127) / 128, Cin / 64), dim3(256), 0, (hipStream_t)stream, a);
    MG_CHECK_LAUNCH("mgnns_conv_dgrad_bf16_nhwc");
    return 0;
}

extern "C" size_t mgnns_conv_wgrad_workspace_bytes(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad) {
    int OH = 0, OW = 0;
    if (conv_train_geometry("mgnns_conv_wgrad_workspace_bytes", B, H, W, Cin, Cout, KH, KW, stride, pad, OH, OW) || B == 0) return 0;
    int nshare, share_len;
    const int K = KH * KW * Cin;
    wgrad_shares((long long)B * OH * OW, Cout, K, nshare, share_len);
    return nshare > 1 ? (size_t)nshare * ((size_t)Cout * K + Cout) * sizeof(float) : 0;
}

extern "C" int mgnns_conv_wgrad_bf16_nhwc(const void* x, const void* dy, int B, int H, int W, int Cin, int Cout, int KH, int KW,
                                          int stride, int pad, float* dW, float* db, void* workspace, size_t workspace_bytes,
                                          mgnns_stream_t stream) {
    int OH = 0, OW = 0;
    if (int rc = conv_train_geometry("mgnns_conv_wgrad_bf16_nhwc", B, H, W, Cin, Cout, KH, KW, stride, pad, OH, OW)) return rc;
    MG_REQUIRE(dW && db, "mgnns_conv_wgrad_bf16_nhwc: null output");
    MG_REQUIRE(mg_aligned16(dW) && mg_aligned16(db), "mgnns_conv_wgrad_bf16_nhwc: outputs must be 16-byte aligned");
    const int K = KH * KW * Cin;
    if (B == 0) {
        hipError_t e = hipMemsetAsync(dW, 0, (size_t)Cout * K * sizeof(float), (hipStream_t)stream);
        if (e == hipSuccess) e = hipMemsetAsync(db, 0, (size_t)Cout * sizeof(float), (hipStream_t)stream);
        MG_REQUIRE(e == hipSuccess, "mgnns_conv_wgrad_bf16_nhwc: memset failed: %s", hipGetErrorString(e));
        return 0;
    }
    MG_REQUIRE(x && dy, "mgnns_conv_wgrad_bf16_nhwc: null pointer");
    MG_REQUIRE(mg_aligned16(x) && mg_aligned16(dy) && (!workspace || mg_aligned16(workspace)),
               "mgnns_conv_wgrad_bf16_nhwc: operands must be 16-byte aligned (B=%d H=%d W=%d C_in=%d C_out=%d)", B, H, W, Cin, Cout);
    int nshare, share_len;
    wgrad_shares((long long)B * OH * OW, Cout, K, nshare, share_len);
    const size_t need = nshare > 1 ? (size_t)nshare * ((size_t)Cout * K + Cout) * sizeof(float) : 0;
    MG_REQUIRE(need == 0 || (workspace && workspace_bytes >= need),
               "mgnns_conv_wgrad_bf16_nhwc: workspace of %zu bytes, %zu needed (mgnns_conv_wgrad_workspace_bytes)", workspace_bytes, need);
    WgradArgs a;
    a.x = reinterpret_cast<const u16*>(x);
    a.dy = reinterpret_cast<const u16*>(dy);
    float* ws = reinterpret_cast<float*>(workspace);
    a.out = nshare > 1 ? ws : dW;
    a.dbout = nshare > 1 ? ws + (size_t)nshare * Cout * K : db;
    a.H = H; a.W = W; a.Cin = Cin; a.cin_shift = __builtin_ctz((unsigned)Cin); a.OH = OH; a.OW = OW; a.Cout = Cout; a.KW = KW;
    a.stride = stride; a.pad = pad; a.M = B * OH * OW; a.K = K; a.share_len = share_len;
    hipLaunchKernelGGL(conv_wgrad_kernel, dim3(Cout / 64, K / 64, nshare), dim3(256), 0, (hipStream_t)stream, a);
    MG_CHECK_LAUNCH("mgnns_conv_wgrad_bf16_nhwc");
    if (nshare > 1) {
        const size_t n = (size_t)Cout * K;
        hipLaunchKernelGGL(conv_wgrad_reduce_kernel, dim3(eltwise_blocks(n)), dim3(256), 0, (hipStream_t)stream, a.out, n, nshare, dW);
        hipLaunchKernelGGL(conv_wgrad_reduce_kernel, dim3(eltwise_blocks((size_t)Cout)), dim3(256), 0, (hipStream_t)stream, a.dbout,
                           (size_t)Cout, nshare, db);
        MG_CHECK_LAUNCH("mgnns_conv_wgrad_bf16_nhwc (reduce)");
    }
    return 0;
}

extern "C" int mgnns_conv_bn_unfold(const float* dWp, const float* dbp, const float* w, const float* gamma, const float* mean,
                                    const float* var, float eps, int Cout, int Cin, int KH, int KW, float* dW, float* dgamma,
                                    float* dbeta, mgnns_stream_t stream) {
    MG_REQUIRE(dWp && dbp && w && gamma && mean && var, "mgnns_conv_bn_unfold: null pointer");
    MG_REQUIRE(Cout > 0 && Cin > 0 && KH > 0 && KW > 0, "mgnns_conv_bn_unfold: bad dims Cout=%d Cin=%d KH=%d KW=%d", Cout, Cin, KH, KW);
    hipLaunchKernelGGL(conv_bn_unfold_kernel, dim3(Cout), dim3(256), 0, (hipStream_t)stream, dWp, dbp, w, gamma, mean, var, eps, Cin,
                       KH, KW, dW, dgamma, dbeta);
    MG_CHECK_LAUNCH("mgnns_conv_bn_unfold");
    return 0;
}

extern "C" int mgnns_map_grad_relu_nhwc_bf16(const float* map, const float* dmap, int B, int C, int P, void* g, mgnns_stream_t stream) {
    MG_REQUIRE(B >= 0 && C > 0 && C % 8 == 0 && P > 0, "mgnns_map_grad_relu_nhwc_bf16: need C %% 8 == 0 (B=%d C=%d P=%d)", B, C, P);
    if (B == 0) return 0;
    MG_REQUIRE(map && dmap && g, "mgnns_map_grad_relu_nhwc_bf16: null pointer");
    MG_REQUIRE(mg_aligned16(g), "mgnns_map_grad_relu_nhwc_bf16: output must be 16-byte aligned (B=%d C=%d P=%d)", B, C, P);
    hipLaunchKernelGGL(map_grad_relu_kernel, dim3(eltwise_blocks((size_t)B * (C / 8) * P)), dim3(256), 0, (hipStream_t)stream, map, dmap,
                       B, C, P, reinterpret_cast<u16*>(g));
    MG_CHECK_LAUNCH("mgnns_map_grad_relu_nhwc_bf16");
    return 0;
}
