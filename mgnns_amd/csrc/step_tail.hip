// The tail of a training step (include/mgnns_step.h): cross-entropy with its gradient, the global gradient
// norm over a table of chunks with its clip coefficient, and a fused Adam update over the same table.  Plain launches: no
// hand-over between workgroups, no atomics, every reduction in a fixed order -- the same inputs give the same bits.
//
// The Adam arithmetic is the specification: every fp32 operation is rounded on its own, in the order written in adam_element.
// Contraction is switched off for the whole file (and again by build.py's FILE_FLAGS): an FMA would round once where the
// specification rounds twice, and tests/step_tail_ref.py checks the kernel bit for bit.
#include "common.hpp"
#include "../../include/mgnns_step.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256;
constexpr int CHUNK = MGNNS_STEP_CHUNK;

struct Chunk {
    uint64_t p, g, m, v;
    int32_t n, group;
};
static_assert(sizeof(Chunk) == 40, "the chunk record of mgnns_step.h is 40 bytes");

struct Row {
    float neg_step, sqrt_bc2, omb1, b2, omb2, eps, wd, unused;
};
static_assert(sizeof(Row) == 4 * MGNNS_STEP_GROUP_FLOATS, "the scalar row of mgnns_step.h");

// sum of red[0..TPB) into red[0], as a fixed tree; every thread of the workgroup calls it
__device__ __forceinline__ void block_tree_sum(double* red) {
    __syncthreads();
#pragma unroll
    for (int s = TPB / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
}

// ---- cross-entropy ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void ce_loss_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target, int B, int NL,
                                                      float* __restrict__ loss, float* __restrict__ dlogits) {
    __shared__ double red[TPB];
    __shared__ int live_s[TPB], bad_s[TPB];
    const int tid = threadIdx.x;
    int live = 0, bad = 0;
    for (int b = tid; b < B; b += TPB) {
        const int64_t t = target[b];
        if (t != -100) {
            ++live;
            bad |= (t < 0 || t >= NL) ? 1 : 0;
        }
    }
    live_s[tid] = live;
    bad_s[tid] = bad;
    __syncthreads();
    for (int s = TPB / 2; s > 0; s >>= 1) {
        if (tid < s) {
            live_s[tid] += live_s[tid + s];
            bad_s[tid] |= bad_s[tid + s];
        }
        __syncthreads();
    }
    const double n_live = (double)live_s[0];
    const bool any_bad = bad_s[0] != 0;
    const double nan = __builtin_nan("");

    double acc = 0.0;                                   // this thread's rows, in row order
    for (int b = tid; b < B; b += TPB) {
        const int64_t t = target[b];
        const float* x = logits + (size_t)b * NL;
        float* d = dlogits + (size_t)b * NL;
        if (t == -100 || t < 0 || t >= NL) {             // ignored: a zero row; any other target outside [0, NL): a NaN row
            const float fill = t == -100 ? 0.0f : (float)nan;
            for (int j = 0; j < NL; ++j) d[j] = fill;
            continue;
        }
        double mx = (double)x[0];
        for (int j = 1; j < NL; ++j) {
            const double xj = (double)x[j];
            mx = (xj > mx || xj != xj) ? xj : mx;       // NaN propagates, as in torch
        }
        double sum = 0.0;
        for (int j = 0; j < NL; ++j) sum += exp((double)x[j] - mx);
        acc -= ((double)x[(int)t] - mx) - log(sum);
        for (int j = 0; j < NL; ++j) {
            const double pj = exp((double)x[j] - mx) / sum;
            d[j] = (float)((pj - (j == (int)t ? 1.0 : 0.0)) / n_live);
        }
    }
    red[tid] = acc;
    block_tree_sum(red);
    if (tid == 0) loss[0] = any_bad ? (float)nan : (float)(red[0] / n_live);        // no live row: 0 / 0 = NaN
}

// ---- sum of squares --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double sq(float x) { return (double)x * (double)x; }

// elements in front of the first 16-byte boundary of a 4-byte aligned address (0..3), at most n
__device__ __forceinline__ int head_elems(uint64_t addr, int n) {
    const int h = (int)(((16u - (unsigned)(addr & 15u)) & 15u) >> 2);
    return h < n ? h : n;
}

__global__ __launch_bounds__(TPB) void grad_sumsq_kernel(const Chunk* __restrict__ chunks, int n_chunks, double* __restrict__ partial) {
    __shared__ double red[TPB];
    const int tid = threadIdx.x;
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const Chunk ck = chunks[c];
        const int n = (ck.n >= 1 && ck.n <= CHUNK) ? ck.n : 0;
        const float* g = reinterpret_cast<const float*>(ck.g);
        double acc = 0.0;
        if ((ck.g & 3u) == 0) {
            const int head = head_elems(ck.g, n);
            const int nv = (n - head) >> 2;
            const int tail0 = head + (nv << 2);
            if (tid < head) acc += sq(g[tid]);
            const f32x4* gv = reinterpret_cast<const f32x4*>(g + head);
            for (int i = tid; i < nv; i += TPB) {
                const f32x4 x = gv[i];
                acc += sq(x.x);
                acc += sq(x.y);
                acc += sq(x.z);
                acc += sq(x.w);
            }
            if (tid < n - tail0) acc += sq(g[tail0 + tid]);
        } else {
            for (int i = tid; i < n; i += TPB) acc += sq(g[i]);
        }
        red[tid] = acc;
        block_tree_sum(red);
        if (tid == 0) partial[c] = red[0];
        __syncthreads();                                 // red is written again in the next round
    }
}

__global__ __launch_bounds__(TPB) void grad_clip_coef_kernel(const double* __restrict__ partial, int n_chunks, float max_norm,
                                                             float* __restrict__ out) {
    __shared__ double red[TPB];
    const int tid = threadIdx.x;
    const int per = (n_chunks + TPB - 1) / TPB;
    const int lo = tid * per < n_chunks ? tid * per : n_chunks, hi = lo + per < n_chunks ? lo + per : n_chunks;
    double acc = 0.0;
    for (int i = lo; i < hi; ++i) acc += partial[i];     // a run of consecutive partials in index order
    red[tid] = acc;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int t = 0; t < TPB; ++t) s += red[t];       // the runs in index order
        const float norm = (float)sqrt(s);
        const float c = max_norm / (norm + 1e-6f);
        out[0] = norm;
        out[1] = c > 1.0f ? 1.0f : c;                    // torch.clamp(c, max=1): NaN stays NaN
    }
}

// ---- Adam ------------------------------------------------------------------------------------------------------------------
// The specification, one rounding per operation (tests/step_tail_ref.py restates it in numpy).
__device__ __forceinline__ void adam_element(float& p, float g, float& m, float& v, const Row& r, float coef) {
    g = g * coef;
    if (r.wd != 0.0f) g = g + r.wd * p;
    m = m + (g - m) * r.omb1;
    v = v * r.b2 + (r.omb2 * g) * g;
    const float denom = sqrtf(v) / r.sqrt_bc2 + r.eps;
    p = p + r.neg_step * (m / denom);
}

// g[0..n) *= coef by the whole workgroup, 16 bytes at a time between a head and a tail of single elements
__device__ __forceinline__ void scale_run(float* g, int n, float coef) {
    const int tid = threadIdx.x;
    const uint64_t addr = reinterpret_cast<uint64_t>(g);
    if ((addr & 3u) != 0) {
        for (int i = tid; i < n; i += TPB) g[i] = g[i] * coef;
        return;
    }
    const int head = head_elems(addr, n);
    const int nv = (n - head) >> 2;
    const int tail0 = head + (nv << 2);
    if (tid < head) g[tid] = g[tid] * coef;
    f32x4* gv = reinterpret_cast<f32x4*>(g + head);
    for (int i = tid; i < nv; i += TPB) gv[i] = gv[i] * coef;
    if (tid < n - tail0) g[tail0 + tid] = g[tail0 + tid] * coef;
}

__global__ __launch_bounds__(TPB) void adam_step_kernel(const Chunk* __restrict__ chunks, int n_chunks, const Row* __restrict__ groups,
                                                        int n_groups, const float* __restrict__ clip_coef) {
    const int tid = threadIdx.x;
    const float coef = clip_coef[0];
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const Chunk ck = chunks[c];
        if (ck.n < 1 || ck.n > CHUNK) continue;
        if (ck.group == -1) {                            // counted in the norm only: g = g * coef in place, as clip_grad_norm_ leaves it
            scale_run(reinterpret_cast<float*>(ck.g), ck.n, coef);
            continue;
        }
        if (ck.group < 0 || ck.group >= n_groups) continue;
        const int n = ck.n;
        const Row r = groups[ck.group];
        float* p = reinterpret_cast<float*>(ck.p);
        const float* g = reinterpret_cast<const float*>(ck.g);
        float* m = reinterpret_cast<float*>(ck.m);
        float* v = reinterpret_cast<float*>(ck.v);
        // 16-byte accesses need the four runs to sit alike inside their 16-byte lines: a view at an odd offset next to freshly
        // allocated state does not, and goes element by element (coalesced all the same)
        const bool alike = (((ck.p ^ ck.g) | (ck.p ^ ck.m) | (ck.p ^ ck.v)) & 15u) == 0 && (ck.p & 3u) == 0;
        if (alike) {
            const int head = head_elems(ck.p, n);
            const int nv = (n - head) >> 2;
            const int tail0 = head + (nv << 2);
            if (tid < head) adam_element(p[tid], g[tid], m[tid], v[tid], r, coef);
            f32x4* pv = reinterpret_cast<f32x4*>(p + head);
            const f32x4* gv = reinterpret_cast<const f32x4*>(g + head);
            f32x4* mv = reinterpret_cast<f32x4*>(m + head);
            f32x4* vv = reinterpret_cast<f32x4*>(v + head);
            for (int i = tid; i < nv; i += TPB) {
                f32x4 P = pv[i], M = mv[i], V = vv[i];
                const f32x4 G = gv[i];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float pk = P[k], mk = M[k], vk = V[k];
                    adam_element(pk, G[k], mk, vk, r, coef);
                    P[k] = pk;
                    M[k] = mk;
                    V[k] = vk;
                }
                pv[i] = P;
                mv[i] = M;
                vv[i] = V;
            }
            if (tid < n - tail0) {
                const int i = tail0 + tid;
                adam_element(p[i], g[i], m[i], v[i], r, coef);
            }
        } else {
            for (int i = tid; i < n; i += TPB) adam_element(p[i], g[i], m[i], v[i], r, coef);
        }
    }
}

int chunk_grid(int n_chunks) {
    const int cus = mg_cu_count();
    if (cus <= 0) return 0;
    const int cap = cus * 8;                             // 8 workgroups of 256 lanes per CU; the loop strides over the rest
    return n_chunks < cap ? n_chunks : cap;
}

}  // namespace

extern "C" size_t mgnns_step_chunk_elems(void) { return MGNNS_STEP_CHUNK; }
extern "C" size_t mgnns_step_chunk_record_bytes(void) { return sizeof(Chunk); }
extern "C" size_t mgnns_step_chunk_table_bytes(int n_chunks) { return n_chunks > 0 ? sizeof(Chunk) * (size_t)n_chunks : 0; }
extern "C" size_t mgnns_step_group_table_bytes(int n_groups) { return n_groups > 0 ? sizeof(Row) * (size_t)n_groups : 0; }
extern "C" size_t mgnns_step_partials_bytes(int n_chunks) { return n_chunks > 0 ? sizeof(double) * (size_t)n_chunks : 0; }

extern "C" int mgnns_ce_loss_fwd_bwd(const float* logits, const int64_t* target, int B, int NL, float* loss, float* dlogits,
                                     mgnns_stream_t stream) {
    MG_REQUIRE(logits && target && loss && dlogits, "mgnns_ce_loss_fwd_bwd: null pointer");
    if (NL < 1 || NL > MGNNS_CE_MAX_NL || B < 1) {
        mgnns_set_error("mgnns_ce_loss_fwd_bwd: B=%d, NL=%d: takes B >= 1 and 1 <= NL <= %d", B, NL, MGNNS_CE_MAX_NL);
        return MGNNS_ERR_UNSUPP;
    }
    hipLaunchKernelGGL(ce_loss_kernel, dim3(1), dim3(TPB), 0, (hipStream_t)stream, logits, target, B, NL, loss, dlogits);
    MG_CHECK_LAUNCH("mgnns_ce_loss_fwd_bwd");
    return 0;
}

extern "C" int mgnns_grad_sumsq(const void* chunks, int n_chunks, double* partial, mgnns_stream_t stream) {
    MG_REQUIRE(n_chunks >= 0, "mgnns_grad_sumsq: n_chunks=%d", n_chunks);
    if (n_chunks == 0) return 0;
    MG_REQUIRE(chunks && partial, "mgnns_grad_sumsq: null pointer");
    MG_REQUIRE((reinterpret_cast<uintptr_t>(chunks) & 7u) == 0 && (reinterpret_cast<uintptr_t>(partial) & 7u) == 0,
               "mgnns_grad_sumsq: the chunk table and the partials must be 8-byte aligned");
    const int grid = chunk_grid(n_chunks);
    if (grid <= 0) return MGNNS_ERR_LAUNCH;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(grid), dim3(TPB), 0, (hipStream_t)stream, static_cast<const Chunk*>(chunks), n_chunks, partial);
    MG_CHECK_LAUNCH("mgnns_grad_sumsq");
    return 0;
}

extern "C" int mgnns_grad_clip_coef(const double* partial, int n_chunks, float max_norm, float* out, mgnns_stream_t stream) {
    MG_REQUIRE(n_chunks >= 0, "mgnns_grad_clip_coef: n_chunks=%d", n_chunks);
    MG_REQUIRE(out && (partial || n_chunks == 0), "mgnns_grad_clip_coef: null pointer");
    MG_REQUIRE(max_norm >= 0.0f, "mgnns_grad_clip_coef: max_norm=%g must be a number >= 0", (double)max_norm);
    MG_REQUIRE((reinterpret_cast<uintptr_t>(partial) & 7u) == 0, "mgnns_grad_clip_coef: the partials must be 8-byte aligned");
    hipLaunchKernelGGL(grad_clip_coef_kernel, dim3(1), dim3(TPB), 0, (hipStream_t)stream, partial, n_chunks, max_norm, out);
    MG_CHECK_LAUNCH("mgnns_grad_clip_coef");
    return 0;
}

extern "C" int mgnns_adam_step(const void* chunks, int n_chunks, const float* groups, int n_groups, const float* clip_coef,
                               mgnns_stream_t stream) {
    MG_REQUIRE(n_chunks >= 0 && n_groups >= 0, "mgnns_adam_step: n_chunks=%d, n_groups=%d", n_chunks, n_groups);
    if (n_chunks == 0) return 0;
    MG_REQUIRE(chunks && groups && clip_coef && n_groups >= 1, "mgnns_adam_step: null pointer or an empty scalar table");
    MG_REQUIRE((reinterpret_cast<uintptr_t>(chunks) & 7u) == 0 && (reinterpret_cast<uintptr_t>(groups) & 3u) == 0 &&
                   (reinterpret_cast<uintptr_t>(clip_coef) & 3u) == 0,
               "mgnns_adam_step: misaligned table");
    const int grid = chunk_grid(n_chunks);
    if (grid <= 0) return MGNNS_ERR_LAUNCH;
    hipLaunchKernelGGL(adam_step_kernel, dim3(grid), dim3(TPB), 0, (hipStream_t)stream, static_cast<const Chunk*>(chunks), n_chunks,
                       reinterpret_cast<const Row*>(groups), n_groups, clip_coef);
    MG_CHECK_LAUNCH("mgnns_adam_step");
    return 0;
}
