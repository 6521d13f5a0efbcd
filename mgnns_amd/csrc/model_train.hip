// Training mode of the parts of Multi_GCN_Multihead_Att around the fusion stacks (MODEL:431-567), fp32 throughout:
//   * the image memory banks' weight gradient (liner_img_object / liner_img_place), the hot path of the backward:
//       dW[o, c] = sum_b sum_p dBank[b, p, o] X[b, c, p],   db[o] = sum_{b,p} dBank[b, p, o]
//     on the exact-f32 MFMA (v_mfma_f32_16x16x4_f32), reading the feature maps X in their native [B, K, P] layout;
//   * the label "attention" (MODEL:88-133) with dropout on softmax(energy) over each head's dh axis, forward and backward;
//   * plain dropout (the classifier's, after multi_linear_1) and the masks of any site as bytes (for tests and tools).
// DESIGN.md section 11 has the algebra.  Every reduction over samples runs in a fixed order (slabs + an ordered combine, no
// atomics): one seed gives bit-identical results.
#include "common.hpp"
#include "dropout_hash.hpp"

namespace {

// ---- image-bank weight gradient --------------------------------------------------------------------------------------------
// GEMM view: M = o (N <= 320 outputs), N = c (K channels), reduction index k = b * P + p over the flattened (sample, position)
// pairs of a slab.  A[o][k] = dBank[k][o] (row k of dBank is contiguous in o), B[k][c] = X[b][c][p] (contiguous in p).
// A workgroup (8 waves) owns all 320 o x 128 channels and one slab of k; it stages 32 k at a time in LDS (A as [k][o], B as
// [c][k]); wave w computes o tiles 10 (w & 1) .. +10 x channel tiles 2 (w >> 1) .. +2: 20 accumulators of 16 x 16.
// Each feature-map element is read by exactly one workgroup; dBank is re-read by the K / 128 channel blocks of a slab, which
// run next to each other (adjacent block ids) and find it in L2.
constexpr int BW_O = 320;                 // o rows per workgroup (20 MFMA tiles)
constexpr int BW_C = 128;                 // channels per workgroup (8 MFMA tiles)
constexpr int BW_K = 32;                  // k per LDS stage
constexpr int BW_NT = 512;
constexpr int AS_LD = 336;                // [k][o] row stride: 336 = 16 mod 64 banks, the 4 k rows of a read are disjoint
constexpr int BS_LD = 36;                 // [c][k] row stride: 36 c apart in 64 banks + 4 k -> no conflict
constexpr int A_PER_T = BW_K * BW_O / BW_NT;     // 20
constexpr int B_PER_T = BW_K * BW_C / BW_NT;     // 8

__global__ __launch_bounds__(BW_NT, 4) void imgbank_wgrad_kernel(const float* __restrict__ X, const float* __restrict__ dbank,
                                                                 int K, int P, int N, long KK, long kslab, int direct,
                                                                 float* __restrict__ dW, float* __restrict__ db,
                                                                 float* __restrict__ part, float* __restrict__ part_db) {
    __shared__ float As[BW_K * AS_LD];
    __shared__ float Bs[BW_C * BS_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c0 = blockIdx.x * BW_C;
    const int s = blockIdx.y;
    const long kb = (long)s * kslab;
    const long ke = kb + kslab < KK ? kb + kslab : KK;
    const int ow = (wave & 1) * 10, cw = (wave >> 1) * 2;
    const bool do_db = blockIdx.x == 0;

    f32x4 acc[10][2];
#pragma unroll
    for (int i = 0; i < 10; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float dbacc = 0.f;

    float ra[A_PER_T], rb[B_PER_T];
    // a stage: wave w loads A rows k = 4w .. 4w+3 (o = lane + 64 m, m < 5) and B element (c = tid / 32 + 16 i, k = tid % 32):
    // consecutive lanes, consecutive addresses
    const int bk = tid & (BW_K - 1), bc = tid >> 5;
    auto load = [&](long k0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long k = k0 + 4 * wave + r;
            const float* row = dbank + k * N;
#pragma unroll
            for (int m = 0; m < 5; ++m) {
                const int o = lane + 64 * m;
                ra[5 * r + m] = (k < ke && o < N) ? row[o] : 0.f;
            }
        }
        const long k = k0 + bk;
        const long b = k / P, p = k - b * P;
        const float* col = X + ((size_t)b * K + c0 + bc) * P + p;
#pragma unroll
        for (int i = 0; i < B_PER_T; ++i)
            rb[i] = (k < ke && c0 + bc + 16 * i < K) ? col[(size_t)16 * i * P] : 0.f;
    };
    auto store = [&]() {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int m = 0; m < 5; ++m) As[(4 * wave + r) * AS_LD + lane + 64 * m] = ra[5 * r + m];
#pragma unroll
        for (int i = 0; i < B_PER_T; ++i) Bs[(bc + 16 * i) * BS_LD + bk] = rb[i];
    };

    if (kb < ke) load(kb);
    for (long k0 = kb; k0 < ke; k0 += BW_K) {
        __syncthreads();                       // the previous stage's reads are done
        store();
        __syncthreads();
        if (k0 + BW_K < ke) load(k0 + BW_K);   // next stage in flight under the MFMAs
        if (do_db && tid < BW_O) {
#pragma unroll 8
            for (int kk = 0; kk < BW_K; ++kk) dbacc += As[kk * AS_LD + tid];
        }
#pragma unroll
        for (int ks = 0; ks < BW_K / 4; ++ks) {
            const int kr = 4 * ks + (lane >> 4);
            float a[10], bv[2];
#pragma unroll
            for (int i = 0; i < 10; ++i) a[i] = As[kr * AS_LD + (ow + i) * 16 + (lane & 15)];
#pragma unroll
            for (int j = 0; j < 2; ++j) bv[j] = Bs[((cw + j) * 16 + (lane & 15)) * BS_LD + kr];
#pragma unroll
            for (int i = 0; i < 10; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], bv[j], acc[i][j], 0, 0, 0);
        }
    }
    // C/D map of the 16x16 f32 MFMA: row 4 (lane >> 4) + r, column lane & 15
    float* out = direct ? dW : part + (size_t)s * N * K;
#pragma unroll
    for (int i = 0; i < 10; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int c = c0 + (cw + j) * 16 + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int o = (ow + i) * 16 + 4 * (lane >> 4) + r;
                if (o < N && c < K) out[(size_t)o * K + c] = acc[i][j][r];
            }
        }
    if (do_db && tid < N) {
        if (direct) db[tid] = dbacc;
        else part_db[(size_t)s * N + tid] = dbacc;
    }
}

// dW = sum_s part[s], db = sum_s part_db[s], slabs in order
__global__ void imgbank_wgrad_combine_kernel(const float* __restrict__ part, const float* __restrict__ part_db, int nslab,
                                             long nw, int N, float* __restrict__ dW, float* __restrict__ db) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nw + N; i += (long)gridDim.x * blockDim.x) {
        float v = 0.f;
        if (i < nw) {
            for (int s = 0; s < nslab; ++s) v += part[(size_t)s * nw + i];
            dW[i] = v;
        } else {
            const long o = i - nw;
            for (int s = 0; s < nslab; ++s) v += part_db[(size_t)s * N + o];
            db[o] = v;
        }
    }
}

int bank_wgrad_nslab(int B, int K, int P) {
    const long chunks = ((long)B * P + BW_K - 1) / BW_K;
    const int cblocks = (K + BW_C - 1) / BW_C;
    int cu = mg_cu_count();
    if (cu <= 0) cu = 256;
    long ns = (2L * cu + cblocks - 1) / cblocks;          // two workgroups per CU (61 KB of LDS each)
    if (ns > chunks) ns = chunks;
    if (ns > 64) ns = 64;
    return ns < 1 ? 1 : (int)ns;
}

// ---- label attention (MODEL:101-131), one wave per (sample b, head h), lane d < dh -----------------------------------------
//   e[n,d] = Q[n,h,d] K[b,h,d] / sqrt(dh);  p = softmax_d(e);  p' = dropout(p);  x[b,n,h,d] = p' V[b,h,d]
constexpr int LA_WAVES = 4;

__global__ __launch_bounds__(64 * LA_WAVES) void label_attn_train_fwd_kernel(const float* __restrict__ Q, const float* __restrict__ Kt,
                                                                          const float* __restrict__ V, int B, int NLQ, int H, int dh,
                                                                          uint64_t seed, float rate, float* __restrict__ x,
                                                                          float* __restrict__ P, uint8_t* __restrict__ keep) {
    const int w = blockIdx.x * LA_WAVES + (threadIdx.x >> 6), d = threadIdx.x & 63;
    if (w >= B * H) return;
    const int b = w / H, h = w - b * H, hid = H * dh;
    const bool on = d < dh;
    const float inv = 1.0f / sqrtf((float)dh), ks = keep_scale(rate);
    const float kv = on ? Kt[(size_t)b * hid + h * dh + d] : 0.f;
    const float vv = on ? V[(size_t)b * hid + h * dh + d] : 0.f;
    for (int n = 0; n < NLQ; ++n) {
        const float e = on ? Q[(size_t)n * hid + h * dh + d] * kv * inv : -INFINITY;
        const float m = wave_max(e);
        const float ex = on ? __expf(e - m) : 0.f;
        const float p = ex / wave_sum(ex);
        if (on) {
            const size_t i = ((size_t)b * NLQ + n) * hid + h * dh + d;
            const bool kp = mg_keep(seed, MGNNS_DROP_LABEL_ATTN, i, rate);
            x[i] = kp ? p * ks * vv : 0.f;
            P[i] = p;
            keep[i] = kp;
        }
    }
}

// backward: dV[b,h,d] = sum_n dx p';  dp = dx V keep / (1 - rate);  de = p (dp - sum_d p dp);
//           dK[b,h,d] = sum_n de Q / sqrt(dh);  dQ partial [b,n,h,d] = de K / sqrt(dh) (summed over b in order afterwards)
__global__ __launch_bounds__(64 * LA_WAVES) void label_attn_train_bwd_kernel(const float* __restrict__ dx, const float* __restrict__ Q,
                                                                          const float* __restrict__ Kt, const float* __restrict__ V,
                                                                          const float* __restrict__ P, const uint8_t* __restrict__ keep,
                                                                          int B, int NLQ, int H, int dh, float rate,
                                                                          float* __restrict__ dK, float* __restrict__ dV,
                                                                          float* __restrict__ dQp) {
    const int w = blockIdx.x * LA_WAVES + (threadIdx.x >> 6), d = threadIdx.x & 63;
    if (w >= B * H) return;
    const int b = w / H, h = w - b * H, hid = H * dh;
    const bool on = d < dh;
    const float inv = 1.0f / sqrtf((float)dh), ks = keep_scale(rate);
    const size_t j = (size_t)b * hid + h * dh + d;
    const float kv = on ? Kt[j] : 0.f, vv = on ? V[j] : 0.f;
    float dk = 0.f, dv = 0.f;
    for (int n = 0; n < NLQ; ++n) {
        const size_t i = ((size_t)b * NLQ + n) * hid + h * dh + d;
        float p = 0.f, g = 0.f, q = 0.f;
        bool kp = false;
        if (on) {
            p = P[i];
            kp = keep[i] != 0;
            g = dx[i];
            q = Q[(size_t)n * hid + h * dh + d];
        }
        dv += kp ? g * p * ks : 0.f;
        const float dp = kp ? g * vv * ks : 0.f;
        const float de = p * (dp - wave_sum(p * dp));
        dk += de * q * inv;
        if (on) dQp[i] = de * kv * inv;
    }
    if (on) {
        dK[j] = dk;
        dV[j] = dv;
    }
}

// out[j] = sum_r in[r][j] for r = 0..rows-1 in order
__global__ void column_sum_kernel(const float* __restrict__ in, int rows, long cols, float* __restrict__ out) {
    for (long j = (long)blockIdx.x * blockDim.x + threadIdx.x; j < cols; j += (long)gridDim.x * blockDim.x) {
        float v = 0.f;
        for (int r = 0; r < rows; ++r) v += in[(size_t)r * cols + j];
        out[j] = v;
    }
}

// ---- dropout --------------------------------------------------------------------------------------------------------------
__global__ void dropout_fwd_kernel(const float* __restrict__ x, long n, uint64_t seed, int site, float rate, float* __restrict__ y,
                                   uint8_t* __restrict__ keep) {
    const float ks = keep_scale(rate);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const bool kp = mg_keep(seed, site, (uint64_t)i, rate);
        y[i] = kp ? x[i] * ks : 0.f;
        keep[i] = kp;
    }
}

__global__ void dropout_bwd_kernel(const float* __restrict__ dy, const uint8_t* __restrict__ keep, long n, float rate,
                                   float* __restrict__ dx) {
    const float ks = keep_scale(rate);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        dx[i] = keep[i] ? dy[i] * ks : 0.f;
}

__global__ void dropout_mask_kernel(uint64_t seed, int site, float rate, long n, uint8_t* __restrict__ keep) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        keep[i] = mg_keep(seed, site, (uint64_t)i, rate);
}

unsigned grid_for(long n) {
    long g = (n + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

const char* label_attn_shape_error(int B, int NLQ, int H, int dh) {
    if (B < 0) return "B < 0";
    if (NLQ <= 0) return "need NLQ > 0";
    if (H <= 0) return "need H > 0";
    if (dh <= 0 || dh > 64) return "need 0 < dh <= 64";
    return nullptr;
}

}  // namespace

extern "C" size_t mgnns_imgbank_wgrad_workspace_bytes(int B, int K, int P, int N) {
    if (B <= 0 || K <= 0 || P <= 0 || N <= 0) return 64;
    const int ns = bank_wgrad_nslab(B, K, P);
    return ns > 1 ? sizeof(float) * (size_t)ns * N * ((size_t)K + 1) + 64 : 64;
}

extern "C" int mgnns_imgbank_wgrad(const float* X, const float* dbank, int B, int K, int P, int N, float* dW, float* db,
                                   void* workspace, size_t workspace_bytes, mgnns_stream_t stream) {
    MG_REQUIRE(dW && db && workspace && (B == 0 || (X && dbank)), "mgnns_imgbank_wgrad: null pointer");   // B = 0: empty maps
    MG_REQUIRE(B >= 0 && K > 0 && P > 0 && N > 0 && N <= BW_O, "mgnns_imgbank_wgrad: need B >= 0, K, P > 0, 0 < N <= %d "
               "(B=%d K=%d P=%d N=%d)", BW_O, B, K, P, N);
    MG_REQUIRE((long)B * K * P < (1L << 40), "mgnns_imgbank_wgrad: feature map too large");
    MG_REQUIRE(workspace_bytes >= mgnns_imgbank_wgrad_workspace_bytes(B, K, P, N), "mgnns_imgbank_wgrad: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    if (B == 0) {
        (void)hipMemsetAsync(dW, 0, sizeof(float) * N * K, s);
        (void)hipMemsetAsync(db, 0, sizeof(float) * N, s);
        MG_CHECK_LAUNCH("mgnns_imgbank_wgrad(B=0)");
        return 0;
    }
    const long KK = (long)B * P;
    const int ns = bank_wgrad_nslab(B, K, P);
    const long chunks = (KK + BW_K - 1) / BW_K;
    const long kslab = (chunks + ns - 1) / ns * BW_K;
    const int nslab = (int)((KK + kslab - 1) / kslab);
    float* part = reinterpret_cast<float*>(workspace);
    float* part_db = part + (size_t)nslab * N * K;
    dim3 grid((K + BW_C - 1) / BW_C, nslab);
    hipLaunchKernelGGL(imgbank_wgrad_kernel, grid, dim3(BW_NT), 0, s, X, dbank, K, P, N, KK, kslab, nslab == 1 ? 1 : 0, dW, db,
                       part, part_db);
    MG_CHECK_LAUNCH("mgnns_imgbank_wgrad");
    if (nslab > 1) {
        hipLaunchKernelGGL(imgbank_wgrad_combine_kernel, dim3(grid_for((long)N * K + N)), dim3(256), 0, s, (const float*)part,
                           (const float*)part_db, nslab, (long)N * K, N, dW, db);
        MG_CHECK_LAUNCH("mgnns_imgbank_wgrad(combine)");
    }
    return 0;
}

extern "C" int mgnns_label_attn_train_fwd(const float* Q, const float* K, const float* V, int B, int NLQ, int H, int dh,
                                          uint64_t seed, float rate, float* x, float* P, uint8_t* keep, mgnns_stream_t stream) {
    MG_REQUIRE(Q && (B == 0 || (K && V && x && P && keep)), "mgnns_label_attn_train_fwd: null pointer");   // B = 0: empty
    const char* bad = label_attn_shape_error(B, NLQ, H, dh);
    MG_REQUIRE(!bad, "mgnns_label_attn_train_fwd: %s (B=%d NLQ=%d H=%d dh=%d)", bad ? bad : "", B, NLQ, H, dh);
    MG_REQUIRE(rate >= 0.f && rate <= 1.f, "mgnns_label_attn_train_fwd: dropout rate %g outside [0, 1]", (double)rate);
    if (B == 0) return 0;
    hipLaunchKernelGGL(label_attn_train_fwd_kernel, dim3((B * H + LA_WAVES - 1) / LA_WAVES), dim3(64 * LA_WAVES), 0,
                       (hipStream_t)stream, Q, K, V, B, NLQ, H, dh, seed, rate, x, P, keep);
    MG_CHECK_LAUNCH("mgnns_label_attn_train_fwd");
    return 0;
}

extern "C" size_t mgnns_label_attn_train_bwd_workspace_bytes(int B, int NLQ, int H, int dh) {
    if (B <= 0 || NLQ <= 0 || H <= 0 || dh <= 0) return 64;
    return sizeof(float) * (size_t)B * NLQ * H * dh + 64;
}

extern "C" int mgnns_label_attn_train_bwd(const float* dx, const float* Q, const float* K, const float* V, const float* P,
                                          const uint8_t* keep, int B, int NLQ, int H, int dh, float rate, float* dQ, float* dK,
                                          float* dV, void* workspace, size_t workspace_bytes, mgnns_stream_t stream) {
    MG_REQUIRE(Q && dQ && workspace && (B == 0 || (dx && K && V && P && keep && dK && dV)),
               "mgnns_label_attn_train_bwd: null pointer");                                      // B = 0: per-sample tensors empty
    const char* bad = label_attn_shape_error(B, NLQ, H, dh);
    MG_REQUIRE(!bad, "mgnns_label_attn_train_bwd: %s (B=%d NLQ=%d H=%d dh=%d)", bad ? bad : "", B, NLQ, H, dh);
    MG_REQUIRE(rate >= 0.f && rate <= 1.f, "mgnns_label_attn_train_bwd: dropout rate %g outside [0, 1]", (double)rate);
    MG_REQUIRE(workspace_bytes >= mgnns_label_attn_train_bwd_workspace_bytes(B, NLQ, H, dh),
               "mgnns_label_attn_train_bwd: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const long cols = (long)NLQ * H * dh;
    if (B == 0) {
        (void)hipMemsetAsync(dQ, 0, sizeof(float) * cols, s);
        MG_CHECK_LAUNCH("mgnns_label_attn_train_bwd(B=0)");
        return 0;
    }
    float* dQp = reinterpret_cast<float*>(workspace);
    hipLaunchKernelGGL(label_attn_train_bwd_kernel, dim3((B * H + LA_WAVES - 1) / LA_WAVES), dim3(64 * LA_WAVES), 0, s, dx, Q, K,
                       V, P, keep, B, NLQ, H, dh, rate, dK, dV, dQp);
    MG_CHECK_LAUNCH("mgnns_label_attn_train_bwd");
    hipLaunchKernelGGL(column_sum_kernel, dim3(grid_for(cols)), dim3(256), 0, s, (const float*)dQp, B, cols, dQ);
    MG_CHECK_LAUNCH("mgnns_label_attn_train_bwd(dQ)");
    return 0;
}

extern "C" int mgnns_dropout_fwd(const float* x, int64_t n, uint64_t seed, int site, float rate, float* y, uint8_t* keep,
                                 mgnns_stream_t stream) {
    MG_REQUIRE(x && y && keep, "mgnns_dropout_fwd: null pointer");
    MG_REQUIRE(rate >= 0.f && rate <= 1.f, "mgnns_dropout_fwd: dropout rate %g outside [0, 1]", (double)rate);
    if (n <= 0) return 0;
    hipLaunchKernelGGL(dropout_fwd_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, x, (long)n, seed, site, rate, y,
                       keep);
    MG_CHECK_LAUNCH("mgnns_dropout_fwd");
    return 0;
}

extern "C" int mgnns_dropout_bwd(const float* dy, const uint8_t* keep, int64_t n, float rate, float* dx, mgnns_stream_t stream) {
    MG_REQUIRE(dy && keep && dx, "mgnns_dropout_bwd: null pointer");
    MG_REQUIRE(rate >= 0.f && rate <= 1.f, "mgnns_dropout_bwd: dropout rate %g outside [0, 1]", (double)rate);
    if (n <= 0) return 0;
    hipLaunchKernelGGL(dropout_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, dy, keep, (long)n, rate, dx);
    MG_CHECK_LAUNCH("mgnns_dropout_bwd");
    return 0;
}

extern "C" int mgnns_dropout_mask(uint64_t seed, int site, float rate, int64_t n, uint8_t* keep, mgnns_stream_t stream) {
    MG_REQUIRE(keep, "mgnns_dropout_mask: null pointer");
    MG_REQUIRE(rate >= 0.f && rate <= 1.f, "mgnns_dropout_mask: dropout rate %g outside [0, 1]", (double)rate);
    if (n <= 0) return 0;
    hipLaunchKernelGGL(dropout_mask_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, seed, site, rate, (long)n, keep);
    MG_CHECK_LAUNCH("mgnns_dropout_mask");
    return 0;
}
