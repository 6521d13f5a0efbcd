// BatchNorm as a training operator over the trunks' NHWC bf16 activations (batch-statistics fine-tuning).  Every
// tensor is an [M, C] view (M = B * OH * OW pixels, C contiguous, C % 8 == 0); statistics and parameters are fp32:
//
//   bn_stats_kernel        per slab of rows and per channel the pair (mean, M2 = sum (z - mean)^2): a thread sums d = z - K and d^2
//                          about its own first value K (d is exact in fp32: both are bf16 values), so a channel whose mean is far
//                          from zero loses nothing to E[z^2] - mean^2; the threads of a workgroup are merged in thread order and
//   bn_stats_final_kernel  the slabs in slab order, about the first slab's mean K and in fp64: with d_k = mean_k - K, mean = K +
//                          sum n_k d_k / M and M2 = sum (M2_k + n_k d_k^2) - (sum n_k d_k)^2 / M; rstd = 1 / sqrt(M2 / M + eps),
//                          and the running buffers
//   bn_apply_kernel        y = relu?(a z + b + residual?), a = gamma rstd, b = beta - mean a, one rounding to bf16 NHWC
//   bn_apply_nchw_kernel   the same, unrounded, as the fp32 [B, C, P] map: 64 pixels x 64 channels turn round in LDS, so a wave
//                          reads whole 128-byte rows of z and writes 256-byte runs of the map
//   bn_bwd_reduce_kernel   per slab: sum g and sum g xhat, xhat = (z - mean) rstd;  bn_bwd_final_kernel adds the slabs in slab order
//   bn_bwd_apply_kernel    g_z = bf16(gamma rstd (g - dbeta / M - xhat dgamma / M))
//
// A thread owns 8 neighbouring channels (one 16-byte load per row) and walks rows; a workgroup is CGB channel groups x 256 / CGB
// rows (CGB up to 32 in the sweeps, up to 8 in the reductions).  Slabs, workgroup shape and every summation order are functions of (M, C) alone and nothing uses float atomics: results
// are bit-identical from call to call.  The merges across threads and slabs -- a few values per channel -- run in fp64.
#include "common.hpp"
#include "bf16.hpp"

namespace {

typedef unsigned short u16;

constexpr int BN_ROWS_MIN = 16;       // rows per thread below which the rows are not split into more slabs
constexpr int BN_SLABS_MAX = 256;
constexpr int BN_BLOCKS = 2048;       // workgroups the row split aims at

// workgroup shape and slabs of an [M, C] reduction or sweep
struct BnPlan {
    int cgb;         // channel groups (of 8) per workgroup: a power of two <= 32 (sweeps) or <= 8 (reductions)
    int ry;          // rows per step = 256 / cgb
    int gx;          // workgroups across the channels
    int nslab, slab_len;
};

// reduce: a reduction keeps a workgroup to 8 channel groups (whole 128-byte lines still), so that the workgroups that fill the chip
// come from the channels first and the slabs -- whose partials the finalising launch walks -- stay few
BnPlan bn_plan(int M, int C, bool reduce) {
    BnPlan p;
    const int cg = C / 8, widest = reduce ? 8 : 32;
    p.cgb = 1;
    while (p.cgb < cg && p.cgb < widest) p.cgb *= 2;
    p.ry = 256 / p.cgb;
    p.gx = (cg + p.cgb - 1) / p.cgb;
    long long want = BN_BLOCKS / p.gx;
    if (want < 1) want = 1;
    if (want > BN_SLABS_MAX) want = BN_SLABS_MAX;
    const long long step = (long long)p.ry * BN_ROWS_MIN;
    long long most = ((long long)M + step - 1) / step;
    if (most < 1) most = 1;
    const long long n = want < most ? want : most;
    long long len = (((long long)M + n - 1) / n + p.ry - 1) / p.ry * p.ry;
    if (len < p.ry) len = p.ry;
    p.slab_len = (int)len;
    p.nslab = (int)(((long long)M + len - 1) / len);
    if (p.nslab < 1) p.nslab = 1;
    return p;
}

__device__ __forceinline__ void unpack8(const uint4 u, float (&v)[8]) {
    v[0] = mg_bf16_f32(u.x & 0xFFFFu); v[1] = mg_bf16_f32(u.x >> 16);
    v[2] = mg_bf16_f32(u.y & 0xFFFFu); v[3] = mg_bf16_f32(u.y >> 16);
    v[4] = mg_bf16_f32(u.z & 0xFFFFu); v[5] = mg_bf16_f32(u.z >> 16);
    v[6] = mg_bf16_f32(u.w & 0xFFFFu); v[7] = mg_bf16_f32(u.w >> 16);
}

__device__ __forceinline__ uint4 pack8(const float (&v)[8]) {
    uint4 o;
    o.x = mg_bf16x2(v[0], v[1]);
    o.y = mg_bf16x2(v[2], v[3]);
    o.z = mg_bf16x2(v[4], v[5]);
    o.w = mg_bf16x2(v[6], v[7]);
    return o;
}

__device__ __forceinline__ void load8f(const float* p, float (&v)[8]) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
    v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
    v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
}

// rows of the slab [r0, r1) that the thread row `ty` of `ry` (a power of two) visits
__device__ __forceinline__ int rows_of(int r0, int r1, int ty, int ry) {
    const int len = r1 - r0;
    return (len >> (31 - __clz(ry))) + (ty < (len & (ry - 1)) ? 1 : 0);
}

// rows first, first + stride, ... below M
__device__ __forceinline__ int sweep_steps(int M, int first, int stride) {
    return first < M ? (int)(((long long)M - first + stride - 1) / stride) : 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// Statistics.  grid (gx, nslab); ws[slab][0][C] = mean, ws[slab][1][C] = M2 of the slab's rows.
__global__ __launch_bounds__(256) void bn_stats_kernel(const u16* __restrict__ z, int M, int C, int cgb, int slab_len,
                                                       float* __restrict__ ws) {
    __shared__ float s_mean[256 * 8];
    __shared__ float s_m2[256 * 8];
    const int tid = threadIdx.x, ry = 256 / cgb;
    const int tx = tid & (cgb - 1), ty = tid / cgb;
    const int cgi = blockIdx.x * cgb + tx;
    const bool live = cgi * 8 < C;
    const int r0 = blockIdx.y * slab_len;
    const int r1 = min(M, r0 + slab_len);
    const int wch = cgb * 8;                               // channels of this workgroup
    float mean[8], m2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) mean[j] = m2[j] = 0.f;
    if (live && r0 + ty < r1) {
        const u16* p = z + (size_t)(r0 + ty) * C + (size_t)cgi * 8;
        const size_t step = (size_t)ry * C;
        float k[8], s[8], q[8];
        unpack8(*reinterpret_cast<const uint4*>(p), k);
#pragma unroll
        for (int j = 0; j < 8; ++j) s[j] = q[j] = 0.f;
        int n = 1;
        p += step;
#pragma unroll 4
        for (int r = r0 + ty + ry; r < r1; r += ry, p += step, ++n) {
            float v[8];
            unpack8(*reinterpret_cast<const uint4*>(p), v);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float d = v[j] - k[j];
                s[j] += d;
                q[j] = fmaf(d, d, q[j]);
            }
        }
        const float inv = 1.0f / (float)n;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float ds = s[j] * inv;
            mean[j] = k[j] + ds;
            m2[j] = fmaxf(q[j] - s[j] * ds, 0.f);
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        s_mean[ty * wch + tx * 8 + j] = mean[j];
        s_m2[ty * wch + tx * 8 + j] = m2[j];
    }
    __syncthreads();
    // thread t < wch merges channel t of the workgroup over the thread rows, in row order
    const int c = blockIdx.x * wch + tid;
    if (tid < wch && c < C) {
        const double K = (double)s_mean[tid];              // thread row 0 always holds a row of the slab
        double S1 = 0.0, S2 = 0.0;
        int ntot = 0;
        for (int t = 0; t < ry; ++t) {
            const int n = rows_of(r0, r1, t, ry);
            if (n == 0) break;
            const double d = (double)s_mean[t * wch + tid] - K;
            S1 += (double)n * d;
            S2 += (double)s_m2[t * wch + tid] + (double)n * d * d;
            ntot += n;
        }
        const double mu = K + S1 / (double)ntot;
        const double Q = fmax(S2 - S1 * S1 / (double)ntot, 0.0);
        float* out = ws + (size_t)blockIdx.y * 2 * C;
        out[c] = (float)mu;
        out[C + c] = (float)Q;
    }
}

// grid (ceil(C / 32)); 256 threads = 32 channels x 8 parts of the slab range, the parts added in part order
__global__ __launch_bounds__(256) void bn_stats_final_kernel(const float* __restrict__ ws, int nslab, int slab_len, int M, int C,
                                                             float eps, double momentum, float* __restrict__ mean,
                                                             float* __restrict__ rstd, float* __restrict__ var,
                                                             float* __restrict__ running_mean, float* __restrict__ running_var) {
    __shared__ double red[2][8][32];
    const int tid = threadIdx.x, lane = tid & 31, part = tid >> 5;
    const int c = blockIdx.x * 32 + lane;
    const bool live = c < C;
    const int per = (nslab + 7) / 8;
    const int k0 = min(nslab, part * per), k1 = min(nslab, k0 + per);
    // one pass about K, the first slab's mean (inside the data's range): S1 = sum n_k d_k, S2 = sum (M2_k + n_k d_k^2), d_k = mean_k - K
    const double K = live ? (double)ws[c] : 0.0;
    double S1 = 0.0, S2 = 0.0;
    if (live) {
#pragma unroll 8
        for (int k = k0; k < k1; ++k) {
            const double n = (double)(min(M, (k + 1) * slab_len) - k * slab_len);
            const double d = (double)ws[(size_t)k * 2 * C + c] - K;
            S1 += n * d;
            S2 += (double)ws[(size_t)k * 2 * C + C + c] + n * d * d;
        }
    }
    red[0][part][lane] = S1;
    red[1][part][lane] = S2;
    __syncthreads();
    if (part == 0 && live) {
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            s1 += red[0][p][lane];
            s2 += red[1][p][lane];
        }
        const double mu = K + s1 / (double)M;
        const double m2 = fmax(s2 - s1 * s1 / (double)M, 0.0);  // fp64: the centre is within the data, nothing is lost
        const float muf = (float)mu;
        const float vb = (float)(m2 / (double)M);
        mean[c] = muf;
        rstd[c] = 1.0f / sqrtf(vb + eps);
        if (var) var[c] = vb;
        if (running_mean) {
            const double unbiased = (double)vb * (double)M / (double)(M - 1);
            running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * (double)muf);
            running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * unbiased);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Normalise and activate.  grid (gx, row blocks); a thread keeps a, b of its 8 channels and strides over rows.
__global__ __launch_bounds__(256) void bn_apply_kernel(const u16* __restrict__ z, int M, int C, int cgb,
                                                       const float* __restrict__ mean, const float* __restrict__ rstd,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       const u16* __restrict__ residual, int relu, u16* __restrict__ y) {
    const int tid = threadIdx.x, ry = 256 / cgb;
    const int tx = tid & (cgb - 1), ty = tid / cgb;
    const int cgi = blockIdx.x * cgb + tx;
    if (cgi * 8 >= C) return;
    float a[8], b[8], t[8];
    load8f(gamma + cgi * 8, a);
    load8f(rstd + cgi * 8, t);
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] *= t[j];
    load8f(beta + cgi * 8, b);
    load8f(mean + cgi * 8, t);
#pragma unroll
    for (int j = 0; j < 8; ++j) b[j] -= t[j] * a[j];
    const size_t step = (size_t)gridDim.y * ry * C;
    size_t off = ((size_t)blockIdx.y * ry + ty) * C + (size_t)cgi * 8;
    const int nit = sweep_steps(M, blockIdx.y * ry + ty, gridDim.y * ry);
    for (int it = 0; it < nit; ++it, off += step) {
        float v[8];
        unpack8(*reinterpret_cast<const uint4*>(z + off), v);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = fmaf(a[j], v[j], b[j]);
        if (residual) {
            float rr[8];
            unpack8(*reinterpret_cast<const uint4*>(residual + off), rr);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] += rr[j];
        }
        if (relu) {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = fmaxf(v[j], 0.f);
        }
        *reinterpret_cast<uint4*>(y + off) = pack8(v);
    }
}

// grid (ceil(P / 64), ceil(C / 64), B): 64 pixels x 64 channels of one image through LDS
constexpr int BN_TLD = 65;
__global__ __launch_bounds__(256) void bn_apply_nchw_kernel(const u16* __restrict__ z, int C, int P, const float* __restrict__ mean,
                                                            const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const u16* __restrict__ residual,
                                                            int relu, float* __restrict__ y) {
    __shared__ float tile[64 * BN_TLD];
    const int tid = threadIdx.x;
    const int p0 = blockIdx.x * 64, c0 = blockIdx.y * 64, img = blockIdx.z;
    const int cgx = tid & 7, c = c0 + cgx * 8;
    if (c < C) {
        float a[8], b[8], t[8];
        load8f(gamma + c, a);
        load8f(rstd + c, t);
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] *= t[j];
        load8f(beta + c, b);
        load8f(mean + c, t);
#pragma unroll
        for (int j = 0; j < 8; ++j) b[j] -= t[j] * a[j];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int pl = (tid >> 3) + 32 * i, p = p0 + pl;
            if (p >= P) continue;
            const size_t off = ((size_t)img * P + p) * C + c;
            float v[8];
            unpack8(*reinterpret_cast<const uint4*>(z + off), v);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = fmaf(a[j], v[j], b[j]);
            if (residual) {
                float rr[8];
                unpack8(*reinterpret_cast<const uint4*>(residual + off), rr);
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] += rr[j];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) tile[(cgx * 8 + j) * BN_TLD + pl] = relu ? fmaxf(v[j], 0.f) : v[j];
        }
    }
    __syncthreads();
    const int pl = tid & 63, p = p0 + pl;
    if (p < P) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int cl = i * 4 + (tid >> 6);
            if (c0 + cl < C) y[((size_t)img * C + c0 + cl) * P + p] = tile[cl * BN_TLD + pl];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Backward.  grid (gx, nslab); ws[slab][0][C] = sum g, ws[slab][1][C] = sum g xhat over the slab's rows.
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const u16* __restrict__ g, const u16* __restrict__ z, int M, int C, int cgb,
                                                            int slab_len, const float* __restrict__ mean,
                                                            const float* __restrict__ rstd, float* __restrict__ ws) {
    __shared__ float s_b[256 * 8];
    __shared__ float s_g[256 * 8];
    const int tid = threadIdx.x, ry = 256 / cgb;
    const int tx = tid & (cgb - 1), ty = tid / cgb;
    const int cgi = blockIdx.x * cgb + tx;
    const bool live = cgi * 8 < C;
    const int r0 = blockIdx.y * slab_len;
    const int r1 = min(M, r0 + slab_len);
    const int wch = cgb * 8;
    float sb[8], sg[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) sb[j] = sg[j] = 0.f;
    if (live) {
        float mu[8], rs[8];
        load8f(mean + cgi * 8, mu);
        load8f(rstd + cgi * 8, rs);
        size_t off = (size_t)(r0 + ty) * C + (size_t)cgi * 8;
        const size_t step = (size_t)ry * C;
#pragma unroll 2
        for (int r = r0 + ty; r < r1; r += ry, off += step) {
            float gv[8], zv[8];
            unpack8(*reinterpret_cast<const uint4*>(g + off), gv);
            unpack8(*reinterpret_cast<const uint4*>(z + off), zv);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                sb[j] += gv[j];
                sg[j] = fmaf(gv[j], (zv[j] - mu[j]) * rs[j], sg[j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        s_b[ty * wch + tx * 8 + j] = sb[j];
        s_g[ty * wch + tx * 8 + j] = sg[j];
    }
    __syncthreads();
    const int c = blockIdx.x * wch + tid;
    if (tid < wch && c < C) {
        double B = 0.0, G = 0.0;
        for (int t = 0; t < ry; ++t) {
            B += (double)s_b[t * wch + tid];
            G += (double)s_g[t * wch + tid];
        }
        float* out = ws + (size_t)blockIdx.y * 2 * C;
        out[c] = (float)B;
        out[C + c] = (float)G;
    }
}

// sums[0][C] = dbeta, sums[1][C] = dgamma (always: the sweep below reads them); dgamma / dbeta are the caller's copies, or null
__global__ __launch_bounds__(256) void bn_bwd_final_kernel(const float* __restrict__ ws, int nslab, int C, float* __restrict__ sums,
                                                           float* __restrict__ dgamma, float* __restrict__ dbeta) {
    __shared__ double red[2][8][32];
    const int tid = threadIdx.x, lane = tid & 31, part = tid >> 5;
    const int c = blockIdx.x * 32 + lane;
    const bool live = c < C;
    const int per = (nslab + 7) / 8;
    const int k0 = min(nslab, part * per), k1 = min(nslab, k0 + per);
    double B = 0.0, G = 0.0;
    if (live) {
#pragma unroll 8
        for (int k = k0; k < k1; ++k) {
            B += (double)ws[(size_t)k * 2 * C + c];
            G += (double)ws[(size_t)k * 2 * C + C + c];
        }
    }
    red[0][part][lane] = B;
    red[1][part][lane] = G;
    __syncthreads();
    if (part == 0 && live) {
        double b = 0.0, gsum = 0.0;
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            b += red[0][p][lane];
            gsum += red[1][p][lane];
        }
        sums[c] = (float)b;
        sums[C + c] = (float)gsum;
        if (dbeta) dbeta[c] = (float)b;
        if (dgamma) dgamma[c] = (float)gsum;
    }
}

__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const u16* __restrict__ g, const u16* __restrict__ z, int M, int C, int cgb,
                                                           const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           const float* __restrict__ gamma, const float* __restrict__ sums,
                                                           u16* __restrict__ gz) {
    const int tid = threadIdx.x, ry = 256 / cgb;
    const int tx = tid & (cgb - 1), ty = tid / cgb;
    const int cgi = blockIdx.x * cgb + tx;
    if (cgi * 8 >= C) return;
    float mu[8], rs[8], a[8], k1[8], k2[8];
    load8f(mean + cgi * 8, mu);
    load8f(rstd + cgi * 8, rs);
    load8f(gamma + cgi * 8, a);
    load8f(sums + cgi * 8, k1);
    load8f(sums + C + cgi * 8, k2);
    const float invM = 1.0f / (float)M;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        a[j] *= rs[j];
        k1[j] *= invM;
        k2[j] *= invM;
    }
    const size_t step = (size_t)gridDim.y * ry * C;
    size_t off = ((size_t)blockIdx.y * ry + ty) * C + (size_t)cgi * 8;
    const int nit = sweep_steps(M, blockIdx.y * ry + ty, gridDim.y * ry);
    for (int it = 0; it < nit; ++it, off += step) {
        float gv[8], zv[8];
        unpack8(*reinterpret_cast<const uint4*>(g + off), gv);
        unpack8(*reinterpret_cast<const uint4*>(z + off), zv);
#pragma unroll
        for (int j = 0; j < 8; ++j) gv[j] = a[j] * (gv[j] - k1[j] - (zv[j] - mu[j]) * rs[j] * k2[j]);
        *reinterpret_cast<uint4*>(gz + off) = pack8(gv);
    }
}

// row blocks of a sweep: enough workgroups to fill the chip, at least 4 rows per thread
unsigned sweep_blocks(int M, const BnPlan& p) {
    long long want = 4096 / p.gx;
    if (want < 1) want = 1;
    long long most = ((long long)M + p.ry * 4 - 1) / (p.ry * 4);
    if (most < 1) most = 1;
    return (unsigned)(want < most ? want : most);
}

int bn_shape(const char* who, int M, int C) {
    MG_REQUIRE(C > 0 && C % 8 == 0, "%s: C must be a positive multiple of 8 (got M=%d C=%d)", who, M, C);
    MG_REQUIRE(M >= 2, "%s: batch statistics need at least two values per channel (got M=%d C=%d)", who, M, C);
    MG_REQUIRE((long long)M < (1ll << 31) - 65536, "%s: M = %d does not fit 31 bits", who, M);
    return 0;
}

size_t bn_partial_bytes(int M, int C) { return (size_t)bn_plan(M, C, true).nslab * 2 * (size_t)C * sizeof(float); }

}  // namespace

extern "C" size_t mgnns_bn_stats_workspace_bytes(int M, int C) {
    if (bn_shape("mgnns_bn_stats_workspace_bytes", M, C)) return 0;
    return bn_partial_bytes(M, C);
}

extern "C" int mgnns_bn_stats_bf16(const void* z, int M, int C, float eps, double momentum, float* mean, float* rstd, float* var,
                                   float* running_mean, float* running_var, void* workspace, size_t workspace_bytes,
                                   mgnns_stream_t stream) {
    if (int rc = bn_shape("mgnns_bn_stats_bf16", M, C)) return rc;
    MG_REQUIRE(z && mean && rstd && workspace, "mgnns_bn_stats_bf16: null pointer");
    MG_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "mgnns_bn_stats_bf16: running_mean and running_var go together");
    MG_REQUIRE(eps >= 0.f && momentum >= 0.0 && momentum <= 1.0, "mgnns_bn_stats_bf16: bad eps %g / momentum %g", (double)eps, momentum);
    MG_REQUIRE(mg_aligned16(z) && mg_aligned16(workspace), "mgnns_bn_stats_bf16: z and workspace must be 16-byte aligned (M=%d C=%d)", M, C);
    const BnPlan p = bn_plan(M, C, true);
    const size_t need = bn_partial_bytes(M, C);
    MG_REQUIRE(workspace_bytes >= need, "mgnns_bn_stats_bf16: workspace of %zu bytes, %zu needed (mgnns_bn_stats_workspace_bytes)",
               workspace_bytes, need);
    float* ws = reinterpret_cast<float*>(workspace);
    hipLaunchKernelGGL(bn_stats_kernel, dim3(p.gx, p.nslab), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const u16*>(z), M, C,
                       p.cgb, p.slab_len, ws);
    hipLaunchKernelGGL(bn_stats_final_kernel, dim3((C + 31) / 32), dim3(256), 0, (hipStream_t)stream, ws, p.nslab, p.slab_len, M, C, eps,
                       momentum, mean, rstd, var, running_mean, running_var);
    MG_CHECK_LAUNCH("mgnns_bn_stats_bf16");
    return 0;
}

extern "C" int mgnns_bn_apply_bf16(const void* z, int M, int C, const float* mean, const float* rstd, const float* gamma,
                                   const float* beta, const void* residual, int relu, int out_nchw_f32, int P, void* y,
                                   mgnns_stream_t stream) {
    if (int rc = bn_shape("mgnns_bn_apply_bf16", M, C)) return rc;
    MG_REQUIRE(z && mean && rstd && gamma && beta && y, "mgnns_bn_apply_bf16: null pointer");
    MG_REQUIRE(mg_aligned16(z) && mg_aligned16(y) && (!residual || mg_aligned16(residual)) && mg_aligned16(mean) && mg_aligned16(rstd) &&
                   mg_aligned16(gamma) && mg_aligned16(beta),
               "mgnns_bn_apply_bf16: operands must be 16-byte aligned (M=%d C=%d)", M, C);
    const u16* zp = reinterpret_cast<const u16*>(z);
    const u16* rp = reinterpret_cast<const u16*>(residual);
    if (out_nchw_f32) {
        MG_REQUIRE(P > 0 && M % P == 0 && M / P <= 65535, "mgnns_bn_apply_bf16: the fp32 map needs M = B * P with B <= 65535 (M=%d P=%d)", M, P);
        hipLaunchKernelGGL(bn_apply_nchw_kernel, dim3((P + 63) / 64, (C + 63) / 64, M / P), dim3(256), 0, (hipStream_t)stream, zp, C, P,
                           mean, rstd, gamma, beta, rp, relu, reinterpret_cast<float*>(y));
    } else {
        const BnPlan p = bn_plan(M, C, false);
        hipLaunchKernelGGL(bn_apply_kernel, dim3(p.gx, sweep_blocks(M, p)), dim3(256), 0, (hipStream_t)stream, zp, M, C, p.cgb, mean, rstd,
                           gamma, beta, rp, relu, reinterpret_cast<u16*>(y));
    }
    MG_CHECK_LAUNCH("mgnns_bn_apply_bf16");
    return 0;
}

extern "C" size_t mgnns_bn_backward_workspace_bytes(int M, int C) {
    if (bn_shape("mgnns_bn_backward_workspace_bytes", M, C)) return 0;
    return bn_partial_bytes(M, C) + 2 * (size_t)C * sizeof(float);
}

extern "C" int mgnns_bn_backward_bf16(const void* g, const void* z, int M, int C, const float* mean, const float* rstd,
                                      const float* gamma, void* gz, float* dgamma, float* dbeta, void* workspace,
                                      size_t workspace_bytes, mgnns_stream_t stream) {
    if (int rc = bn_shape("mgnns_bn_backward_bf16", M, C)) return rc;
    MG_REQUIRE(g && z && mean && rstd && gamma && gz && workspace, "mgnns_bn_backward_bf16: null pointer");
    MG_REQUIRE(mg_aligned16(g) && mg_aligned16(z) && mg_aligned16(gz) && mg_aligned16(workspace) && mg_aligned16(mean) && mg_aligned16(rstd) &&
                   mg_aligned16(gamma),
               "mgnns_bn_backward_bf16: operands must be 16-byte aligned (M=%d C=%d)", M, C);
    const BnPlan p = bn_plan(M, C, true), q = bn_plan(M, C, false);
    const size_t part = bn_partial_bytes(M, C), need = part + 2 * (size_t)C * sizeof(float);
    MG_REQUIRE(workspace_bytes >= need, "mgnns_bn_backward_bf16: workspace of %zu bytes, %zu needed (mgnns_bn_backward_workspace_bytes)",
               workspace_bytes, need);
    float* ws = reinterpret_cast<float*>(workspace);
    float* sums = ws + part / sizeof(float);
    const u16* gp = reinterpret_cast<const u16*>(g);
    const u16* zp = reinterpret_cast<const u16*>(z);
    hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3(p.gx, p.nslab), dim3(256), 0, (hipStream_t)stream, gp, zp, M, C, p.cgb, p.slab_len, mean,
                       rstd, ws);
    hipLaunchKernelGGL(bn_bwd_final_kernel, dim3((C + 31) / 32), dim3(256), 0, (hipStream_t)stream, ws, p.nslab, C, sums, dgamma, dbeta);
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(q.gx, sweep_blocks(M, q)), dim3(256), 0, (hipStream_t)stream, gp, zp, M, C, q.cgb, mean,
                       rstd, gamma, sums, reinterpret_cast<u16*>(gz));
    MG_CHECK_LAUNCH("mgnns_bn_backward_bf16");
    return 0;
}
