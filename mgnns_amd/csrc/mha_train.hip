// Training mode of one MyMultiHeadAttention layer (models/moudles.py:198-230, models/submodules.py:15-156), fp32 throughout:
// the attention core's forward with attention-probability dropout and its backward, the layer tails' dropout + residual +
// custom LayerNorm forward and backward, and a deterministic weight-gradient kernel.  DESIGN.md section 8 has the algebra.
//
// The core stays in the folded form of sq_mha_folded.hip (len_q == 1, K and V never exist).  Per sample b and head h, with
// a_h = W_k,h^T qh_h / T:
//   forward   s = X a_h (masked), p = softmax(s), p' = dropout(p), z_h = X^T p', o_h = W_v,h z_h + b_v,h sum_l p'_l
//   backward  u_h = W_v,h^T dO_h, c_h = b_v,h . dO_h, dp'_l = x_l . u_h + c_h, dp = dp' keep / (1 - rate),
//             ds = p (dp - sum_l p_l dp_l), r_h = X^T ds_h, dX_l = sum_h ds_h,l a_h + p'_h,l u_h
// Both kernels stream the bank of one sample per workgroup (8 waves, a wave per bank row): the forward reads X once (online
// softmax), the backward twice (dp' needs all of the row's dot products before ds exists; 196 x 300 fp32 rows do not fit in LDS).
//
// Dropout masks come from a counter-based hash of (seed, site, element index): nothing is stored to reproduce them, and a
// second launch with the same seed draws the same mask.  Every reduction over samples or rows runs in a fixed order (slabs +
// an ordered combine, no float atomics), so one seed gives bit-identical outputs and gradients.
#include "common.hpp"
#include "dropout_hash.hpp"

int mg_launch_gemm_batched(const float* X, int ldx, long sx, int M, int K, const float* W, long sw, int w_is_kn,
                           const float* bias, long sb, int N, float* Y, int ldy, long sy, int nbatch,
                           hipStream_t stream);

namespace {

constexpr int FD = 320;          // feature width handled (D <= 320, D % 4 == 0): 80 float4 chunks, two per lane
constexpr int MAXH = 8;
constexpr int MAXL = 208;
constexpr int WAVES = 8;
constexpr int NT = WAVES * 64;

__device__ __forceinline__ float dot4(f32x4 a, f32x4 b) { return (a[0] * b[0] + a[1] * b[1]) + (a[2] * b[2] + a[3] * b[3]); }

__device__ __forceinline__ f32x4 ld4(const float* p, bool ok) {
    return ok ? *reinterpret_cast<const f32x4*>(p) : f32x4{0.f, 0.f, 0.f, 0.f};
}

__device__ __forceinline__ bool row_live(const float* mask, int b, int L, int l) {
    return !mask || mask[(size_t)b * L + l] != 0.0f;
}

// ---- attention core, training forward: one workgroup per sample ------------------------------------------------------
// U [H][B][D] (W_k,h^T qh_h, unscaled); writes P [H][B][L] (softmax before dropout), A [H][B][L] (after dropout: the
// returned attn), keep [H][B][L] (bytes, optional), Z [H][B][D] (X^T p'), SP [H][B] (sum_l p').
__global__ __launch_bounds__(NT) void train_attn_fwd_kernel(const float* __restrict__ U, const float* __restrict__ X,
                                                            const float* __restrict__ mask, int B, int L, int D, int H,
                                                            float inv_temp, uint64_t seed, float rate,
                                                            float* __restrict__ P, float* __restrict__ A,
                                                            uint8_t* __restrict__ keep_out, float* __restrict__ Z,
                                                            float* __restrict__ SP) {
    __shared__ __attribute__((aligned(16))) float Us[MAXH][FD];
    __shared__ float s_all[MAXH][MAXL];
    __shared__ __attribute__((aligned(16))) float comb[WAVES][MAXH][FD];
    __shared__ float mz[2][WAVES][MAXH];
    __shared__ float fac[WAVES][MAXH];
    __shared__ float stat[2][MAXH];

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nc = D / 4;
    const int c0 = lane, c1 = lane + 64;
    const bool v0 = c0 < nc, v1 = c1 < nc;
    const float ks = keep_scale(rate);
    for (int i = tid; i < MAXH * FD; i += NT) {
        const int h = i / FD, d = i - h * FD;
        Us[h][d] = (h < H && d < D) ? U[((size_t)h * B + b) * D + d] * inv_temp : 0.f;
    }
    __syncthreads();

    float m[MAXH], zs[MAXH];
    f32x4 acc[MAXH][2];
#pragma unroll
    for (int h = 0; h < MAXH; ++h) {
        m[h] = -INFINITY;
        zs[h] = 0.f;
        acc[h][0] = acc[h][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int l = wave; l < L; l += WAVES) {
        const bool live = row_live(mask, b, L, l);
        if (!live) {                                            // masked rows: -inf score, the bank row is not read
            if (lane < H) s_all[lane][l] = -INFINITY;
            continue;
        }
        const float* xr = X + ((size_t)b * L + l) * D;
        const f32x4 x0 = ld4(xr + 4 * c0, v0), x1 = ld4(xr + 4 * c1, v1);
#pragma unroll
        for (int h = 0; h < MAXH; ++h) {
            if (h >= H) break;
            const f32x4 u0 = *reinterpret_cast<const f32x4*>(&Us[h][4 * (c0 < FD / 4 ? c0 : 0)]);
            const f32x4 u1 = v1 ? *reinterpret_cast<const f32x4*>(&Us[h][4 * c1]) : f32x4{0.f, 0.f, 0.f, 0.f};
            const float s = wave_sum_dpp(dot4(x0, u0) + dot4(x1, u1));
            if (lane == 0) s_all[h][l] = s;
            const float mn = fmaxf(m[h], s);
            const float sc = __expf(m[h] - mn);                // m == -inf -> 0
            const float w = __expf(s - mn);
            const float wk = mg_keep(seed, 0, ((uint64_t)h * B + b) * L + l, rate) ? w : 0.f;
            zs[h] = zs[h] * sc + w;
            acc[h][0] = acc[h][0] * sc + wk * x0;
            acc[h][1] = acc[h][1] * sc + wk * x1;
            m[h] = mn;
        }
    }
    // merge the waves: z_h = sum_w exp(m_w - M) acc_w / Z * ks
#pragma unroll
    for (int h = 0; h < MAXH; ++h) {
        if (h >= H) break;
        if (v0) *reinterpret_cast<f32x4*>(&comb[wave][h][4 * c0]) = acc[h][0];
        if (v1) *reinterpret_cast<f32x4*>(&comb[wave][h][4 * c1]) = acc[h][1];
        if (lane == 0) {
            mz[0][wave][h] = m[h];
            mz[1][wave][h] = zs[h];
        }
    }
    __syncthreads();
    if (tid < H) {
        const int h = tid;
        float M = -INFINITY;
        for (int w = 0; w < WAVES; ++w) M = fmaxf(M, mz[0][w][h]);
        float Zs = 0.f, f[WAVES];
        for (int w = 0; w < WAVES; ++w) {
            f[w] = (mz[0][w][h] == -INFINITY) ? 0.f : __expf(mz[0][w][h] - M);
            Zs += mz[1][w][h] * f[w];
        }
        // every row masked (a padded sample): P = A = Z = SP = 0, so o = 0 and the backward gives exact zeros.  The reference's
        // softmax would give NaN there, and 0 * NaN in the backward would reach every weight gradient of the step.
        const float iz = Zs > 0.f ? 1.0f / Zs : 0.f;
        for (int w = 0; w < WAVES; ++w) fac[w][h] = f[w] * iz * ks;
        stat[0][h] = M;
        stat[1][h] = iz;
    }
    __syncthreads();
    for (int i = tid; i < H * D; i += NT) {
        const int h = i / D, d = i - h * D;
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) v += comb[w][h][d] * fac[w][h];
        Z[((size_t)h * B + b) * D + d] = v;
    }
    for (int i = tid; i < H * L; i += NT) {
        const int h = i / L, l = i - h * L;
        const size_t e = ((size_t)h * B + b) * L + l;
        const float sv = s_all[h][l];
        const float p = (sv == -INFINITY) ? 0.f * stat[1][h] : __expf(sv - stat[0][h]) * stat[1][h];
        const bool kp = mg_keep(seed, 0, e, rate);
        const float pd = kp ? p * ks : 0.f;
        P[e] = p;
        A[e] = pd;
        if (keep_out) keep_out[e] = kp ? 1 : 0;
        s_all[h][l] = pd;
    }
    __syncthreads();
    if (wave < H) {
        float t = 0.f;
        for (int l = lane; l < L; l += 64) t += s_all[wave][l];
        t = wave_sum(t);
        if (lane == 0) SP[(size_t)wave * B + b] = t;
    }
}

// o[b, h*dk + j] += bv[h*dk + j] * SP[h][b]   (with dropout sum_l p'_l != 1)
__global__ void add_scaled_bias_kernel(float* __restrict__ o, const float* __restrict__ bv, const float* __restrict__ SP, int B,
                                       int H, int dk) {
    const size_t n = (size_t)B * H * dk;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int b = (int)(i / (H * dk)), hj = (int)(i - (size_t)b * H * dk), h = hj / dk;
        o[i] += bv[hj] * SP[(size_t)h * B + b];
    }
}

// ---- attention core, backward: one workgroup per sample ---------------------------------------------------------------
// Uu [H][B][D] = W_v,h^T dO_h; writes R [H][B][D] = X^T ds_h / T and, when dX != nullptr, dX [B][L][D].
__global__ __launch_bounds__(NT) void train_attn_bwd_kernel(const float* __restrict__ U, const float* __restrict__ Uu,
                                                            const float* __restrict__ dO, const float* __restrict__ bv,
                                                            const float* __restrict__ X, const float* __restrict__ mask,
                                                            const float* __restrict__ P, const float* __restrict__ A,
                                                            const uint8_t* __restrict__ keep, int B, int L, int D, int H,
                                                            int dk, float inv_temp, float rate, float* __restrict__ R,
                                                            float* __restrict__ dX) {
    __shared__ __attribute__((aligned(16))) float as[MAXH][FD];
    __shared__ __attribute__((aligned(16))) float us[MAXH][FD];
    __shared__ float ps[MAXH][MAXL];
    __shared__ float pds[MAXH][MAXL];
    __shared__ float dss[MAXH][MAXL];
    __shared__ __attribute__((aligned(16))) float comb[WAVES][MAXH][FD];
    __shared__ float ch[MAXH], tsum[MAXH];

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nc = D / 4;
    const int c0 = lane, c1 = lane + 64;
    const bool v0 = c0 < nc, v1 = c1 < nc;
    const float ks = keep_scale(rate);
    for (int i = tid; i < MAXH * FD; i += NT) {
        const int h = i / FD, d = i - h * FD;
        const bool ok = h < H && d < D;
        const size_t e = ((size_t)h * B + b) * D + d;
        as[h][d] = ok ? U[e] * inv_temp : 0.f;
        us[h][d] = ok ? Uu[e] : 0.f;
    }
    for (int i = tid; i < H * L; i += NT) {
        const int h = i / L, l = i - h * L;
        const size_t e = ((size_t)h * B + b) * L + l;
        ps[h][l] = P[e];
        pds[h][l] = A[e];
    }
    if (wave < H) {                                          // c_h = b_v,h . dO_h
        float t = 0.f;
        for (int j = lane; j < dk; j += 64) t += bv[wave * dk + j] * dO[(size_t)b * H * dk + wave * dk + j];
        t = wave_sum(t);
        if (lane == 0) ch[wave] = t;
    }
    __syncthreads();

    // pass 1: dp = (x_l . u_h + c_h) keep / (1 - rate)
    for (int l = wave; l < L; l += WAVES) {
        if (!row_live(mask, b, L, l)) {
            if (lane < H) dss[lane][l] = 0.f;
            continue;
        }
        const float* xr = X + ((size_t)b * L + l) * D;
        const f32x4 x0 = ld4(xr + 4 * c0, v0), x1 = ld4(xr + 4 * c1, v1);
#pragma unroll
        for (int h = 0; h < MAXH; ++h) {
            if (h >= H) break;
            const f32x4 u0 = *reinterpret_cast<const f32x4*>(&us[h][4 * (c0 < FD / 4 ? c0 : 0)]);
            const f32x4 u1 = v1 ? *reinterpret_cast<const f32x4*>(&us[h][4 * c1]) : f32x4{0.f, 0.f, 0.f, 0.f};
            const float dpd = wave_sum_dpp(dot4(x0, u0) + dot4(x1, u1)) + ch[h];
            if (lane == 0) dss[h][l] = keep[((size_t)h * B + b) * L + l] ? dpd * ks : 0.f;
        }
    }
    __syncthreads();
    if (wave < H) {                                          // sum_l p_l dp_l
        float t = 0.f;
        for (int l = lane; l < L; l += 64) t += ps[wave][l] * dss[wave][l];
        t = wave_sum(t);
        if (lane == 0) tsum[wave] = t;
    }
    __syncthreads();
    for (int i = tid; i < H * L; i += NT) {
        const int h = i / L, l = i - h * L;
        dss[h][l] = ps[h][l] * (dss[h][l] - tsum[h]);
    }
    __syncthreads();

    // pass 2: r_h += ds_h,l x_l;  dX_l = sum_h ds_h,l a_h + p'_h,l u_h
    f32x4 acc[MAXH][2];
#pragma unroll
    for (int h = 0; h < MAXH; ++h) acc[h][0] = acc[h][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int l = wave; l < L; l += WAVES) {
        float* dxr = dX ? dX + ((size_t)b * L + l) * D : nullptr;
        if (!row_live(mask, b, L, l)) {
            if (dxr) {
                if (v0) *reinterpret_cast<f32x4*>(dxr + 4 * c0) = f32x4{0.f, 0.f, 0.f, 0.f};
                if (v1) *reinterpret_cast<f32x4*>(dxr + 4 * c1) = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            continue;
        }
        const float* xr = X + ((size_t)b * L + l) * D;
        const f32x4 x0 = ld4(xr + 4 * c0, v0), x1 = ld4(xr + 4 * c1, v1);
        f32x4 g0 = f32x4{0.f, 0.f, 0.f, 0.f}, g1 = g0;
#pragma unroll
        for (int h = 0; h < MAXH; ++h) {
            if (h >= H) break;
            const float ds = dss[h][l], pd = pds[h][l];
            acc[h][0] += ds * x0;
            acc[h][1] += ds * x1;
            if (dxr) {
                const int k0 = 4 * (c0 < FD / 4 ? c0 : 0), k1 = 4 * (v1 ? c1 : 0);
                g0 += ds * *reinterpret_cast<const f32x4*>(&as[h][k0]) + pd * *reinterpret_cast<const f32x4*>(&us[h][k0]);
                g1 += ds * *reinterpret_cast<const f32x4*>(&as[h][k1]) + pd * *reinterpret_cast<const f32x4*>(&us[h][k1]);
            }
        }
        if (dxr) {
            if (v0) *reinterpret_cast<f32x4*>(dxr + 4 * c0) = g0;
            if (v1) *reinterpret_cast<f32x4*>(dxr + 4 * c1) = g1;
        }
    }
#pragma unroll
    for (int h = 0; h < MAXH; ++h) {
        if (h >= H) break;
        if (v0) *reinterpret_cast<f32x4*>(&comb[wave][h][4 * c0]) = acc[h][0];
        if (v1) *reinterpret_cast<f32x4*>(&comb[wave][h][4 * c1]) = acc[h][1];
    }
    __syncthreads();
    for (int i = tid; i < H * D; i += NT) {
        const int h = i / D, d = i - h * D;
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) v += comb[w][h][d];
        R[((size_t)h * B + b) * D + d] = v * inv_temp;
    }
}

// ---- weight gradient: dW_z[n, k] = sum_m dY_z[m, n] X_z[m, k];  db_z[n] = sum_m dY_z[m, n] xcol_z[m] (1 without xcol) --
// The bias is column K of a virtual [X | xcol].  Grid (k tiles, n tiles, nbatch * nslab): slab s reduces rows
// [s*rows, (s+1)*rows); with nslab > 1 the partials go to part[z][s][N][K+1] and wgrad_combine_kernel adds them in slab order.
constexpr int WT = 64, WM = 16;

struct WgradArgs {
    const float* dY; int ldy; long sy;
    const float* X; int ldx; long sx;
    const float* xcol; long sxc;
    int M, N, K, has_bias, nslab, rows;
    float* dW; int ldw; long sw;
    float* db; long sdb;
    float* part;
};

__global__ __launch_bounds__(256) void wgrad_kernel(WgradArgs a) {
    __shared__ float ys[WM][WT + 1];
    __shared__ float xs[WM][WT + 1];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int k0 = blockIdx.x * WT, n0 = blockIdx.y * WT;
    const int z = blockIdx.z / a.nslab, s = blockIdx.z - z * a.nslab;
    const float* dY = a.dY + (size_t)z * a.sy;
    const float* X = a.X + (size_t)z * a.sx;
    const float* xcol = a.xcol ? a.xcol + (size_t)z * a.sxc : nullptr;
    const int KC = a.K + a.has_bias;
    const int mb = s * a.rows, me = min(a.M, mb + a.rows);
    float acc[4][4] = {};
    for (int m0 = mb; m0 < me; m0 += WM) {
        for (int i = tid; i < WM * WT; i += 256) {
            const int r = i / WT, c = i - r * WT, m = m0 + r;
            const bool mv = m < me;
            const int n = n0 + c, k = k0 + c;
            ys[r][c] = (mv && n < a.N) ? dY[(size_t)m * a.ldy + n] : 0.f;
            float xv = 0.f;
            if (mv && k < a.K) xv = X[(size_t)m * a.ldx + k];
            else if (mv && k == a.K && a.has_bias) xv = xcol ? xcol[m] : 1.0f;
            xs[r][c] = xv;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < WM; ++r) {
            float yv[4], xv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                yv[i] = ys[r][ty * 4 + i];
                xv[i] = xs[r][tx * 4 + i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] += yv[i] * xv[j];
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int n = n0 + ty * 4 + i;
        if (n >= a.N) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = k0 + tx * 4 + j;
            if (k >= KC) continue;
            if (a.nslab > 1) {
                a.part[(((size_t)z * a.nslab + s) * a.N + n) * KC + k] = acc[i][j];
            } else if (k < a.K) {
                a.dW[(size_t)z * a.sw + (size_t)n * a.ldw + k] = acc[i][j];
            } else {
                a.db[(size_t)z * a.sdb + n] = acc[i][j];
            }
        }
    }
}

__global__ void wgrad_combine_kernel(WgradArgs a, int nbatch) {
    const int KC = a.K + a.has_bias;
    const size_t per = (size_t)a.N * KC, total = per * nbatch;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int z = (int)(i / per);
        const size_t e = i - (size_t)z * per;
        const int n = (int)(e / KC), k = (int)(e - (size_t)n * KC);
        float v = 0.f;
        for (int s = 0; s < a.nslab; ++s) v += a.part[((size_t)z * a.nslab + s) * per + e];
        if (k < a.K) a.dW[(size_t)z * a.sw + (size_t)n * a.ldw + k] = v;
        else a.db[(size_t)z * a.sdb + n] = v;
    }
}

int wgrad_nslab(int M) {
    const int ns = (M + 63) / 64;
    return ns < 1 ? 1 : (ns > 16 ? 16 : ns);
}

size_t wgrad_part_floats(int M, int N, int K, int nbatch) {
    const int ns = wgrad_nslab(M);
    return ns > 1 ? (size_t)nbatch * ns * N * (K + 1) : 0;
}

int launch_wgrad(WgradArgs a, int nbatch, hipStream_t s) {
    a.nslab = wgrad_nslab(a.M);
    a.rows = ((a.M + a.nslab - 1) / a.nslab + WM - 1) / WM * WM;
    a.nslab = (a.M + a.rows - 1) / a.rows;
    if (a.nslab < 1) a.nslab = 1;
    const int KC = a.K + a.has_bias;
    dim3 grid((KC + WT - 1) / WT, (a.N + WT - 1) / WT, nbatch * a.nslab);
    hipLaunchKernelGGL(wgrad_kernel, grid, dim3(256), 0, s, a);
    if (a.nslab > 1) {
        size_t blocks = ((size_t)nbatch * a.N * KC + 255) / 256;
        if (blocks > 2048) blocks = 2048;
        hipLaunchKernelGGL(wgrad_combine_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a, nbatch);
    }
    return 0;
}

// ---- dropout + residual + custom LayerNorm (one wave per row) ------------------------------------------------------------
//   v = dropout(x) + res;  y = gamma (v - mean) / (std_unbiased + eps) + beta;  saves xhat, std, keep
constexpr int LNC = 16;          // D <= 64 * LNC

__global__ __launch_bounds__(256) void drop_res_ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ res, int rows,
                                                              int D, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float eps, uint64_t seed,
                                                              int site, float rate, float* __restrict__ y,
                                                              float* __restrict__ xhat, float* __restrict__ sig,
                                                              uint8_t* __restrict__ keep) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float ks = keep_scale(rate);
    float v[LNC];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < LNC; ++i) {
        const int d = lane + 64 * i;
        v[i] = 0.f;
        if (d < D) {
            const size_t e = (size_t)r * D + d;
            const bool kp = mg_keep(seed, site, e, rate);
            keep[e] = kp ? 1 : 0;
            v[i] = (kp ? x[e] * ks : 0.f) + res[e];
            sum += v[i];
        }
    }
    const float mean = wave_sum(sum) / D;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < LNC; ++i) {
        const int d = lane + 64 * i;
        if (d < D) {
            v[i] -= mean;
            sq += v[i] * v[i];
        }
    }
    const float sd = sqrtf(wave_sum(sq) / (D - 1));
    const float inv = 1.0f / (sd + eps);
#pragma unroll
    for (int i = 0; i < LNC; ++i) {
        const int d = lane + 64 * i;
        if (d < D) {
            const size_t e = (size_t)r * D + d;
            const float xh = v[i] * inv;
            xhat[e] = xh;
            y[e] = gamma[d] * xh + beta[d];
        }
    }
    if (lane == 0) sig[r] = sd;
}

// g = (dy + dy2) gamma;  dv = (g - mean(g)) / (std + eps) - xhat sum(g xhat) / (std (D - 1));  dx = dv keep / (1 - rate)
__global__ __launch_bounds__(256) void drop_res_ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ dy2,
                                                              const float* __restrict__ xhat, const float* __restrict__ sig,
                                                              const uint8_t* __restrict__ keep, int rows, int D,
                                                              const float* __restrict__ gamma, float eps, float rate,
                                                              float* __restrict__ dres, float* __restrict__ dx) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float ks = keep_scale(rate);
    float g[LNC], xh[LNC];
    float sg = 0.f, sgx = 0.f;
#pragma unroll
    for (int i = 0; i < LNC; ++i) {
        const int d = lane + 64 * i;
        g[i] = xh[i] = 0.f;
        if (d < D) {
            const size_t e = (size_t)r * D + d;
            g[i] = (dy[e] + (dy2 ? dy2[e] : 0.f)) * gamma[d];
            xh[i] = xhat[e];
            sg += g[i];
            sgx += g[i] * xh[i];
        }
    }
    sg = wave_sum(sg) / D;
    sgx = wave_sum(sgx);
    const float sd = sig[r];
    const float inv = 1.0f / (sd + eps);
    const float k2 = sgx / (sd * (D - 1));
#pragma unroll
    for (int i = 0; i < LNC; ++i) {
        const int d = lane + 64 * i;
        if (d < D) {
            const size_t e = (size_t)r * D + d;
            const float dv = (g[i] - sg) * inv - xh[i] * k2;
            dres[e] = dv;
            dx[e] = keep[e] ? dv * ks : 0.f;
        }
    }
}

// dgamma[d] = sum_r (dy + dy2)[r, d] xhat[r, d];  dbeta[d] = sum_r (dy + dy2)[r, d]   (rows in order: deterministic)
__global__ void ln_param_grad_kernel(const float* __restrict__ dy, const float* __restrict__ dy2, const float* __restrict__ xhat,
                                     int rows, int D, float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= D) return;
    float sgm = 0.f, sb = 0.f;
    for (int r = 0; r < rows; ++r) {
        const size_t e = (size_t)r * D + d;
        const float g = dy[e] + (dy2 ? dy2[e] : 0.f);
        sgm += g * xhat[e];
        sb += g;
    }
    dgamma[d] = sgm;
    dbeta[d] = sb;
}

__global__ void eltwise_kernel(int op, const float* __restrict__ a, const float* __restrict__ b, long n, float* __restrict__ y) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        y[i] = op == MGNNS_ELT_ADD ? a[i] + b[i] : (b[i] > 0.f ? a[i] : (op == MGNNS_ELT_LRELU2_BWD ? 0.2f * a[i] : 0.f));
}

unsigned grid1d(size_t n) {
    size_t g = (n + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

}  // namespace

static const char* mha_train_shape_error(int B, int L, int D, int H, int dk) {
    if (B < 0) return "B < 0";
    if (L <= 0 || L > MAXL) return "need 0 < L <= 208";
    if (D <= 0 || D > FD || D % 4) return "need D <= 320, D % 4 == 0";
    if (H <= 0 || H > MAXH) return "need 0 < H <= 8";
    if (dk <= 0 || dk % 4) return "need dk % 4 == 0";
    return nullptr;
}

extern "C" int mgnns_mha_train_fwd(const float* qh, const float* bank, const float* mask, int B, int L, int D, int H, int dk,
                                   const float* Wk, const float* Wv, const float* bv, uint64_t seed, float rate, float* U,
                                   float* P, float* attn, uint8_t* keep, float* Z, float* SP, float* o, mgnns_stream_t stream) {
    MG_REQUIRE(qh && bank && Wk && Wv && bv && U && P && attn && Z && SP && o, "mgnns_mha_train_fwd: null pointer");
    const char* bad = mha_train_shape_error(B, L, D, H, dk);
    MG_REQUIRE(!bad, "mgnns_mha_train_fwd: %s (B=%d L=%d D=%d H=%d dk=%d)", bad ? bad : "", B, L, D, H, dk);
    MG_REQUIRE(rate >= 0.f && rate <= 1.f, "mgnns_mha_train_fwd: dropout rate %g outside [0, 1]", (double)rate);
    MG_REQUIRE(mg_aligned16(bank) && mg_aligned16(U) && mg_aligned16(Z), "mgnns_mha_train_fwd: bank/U/Z must be 16-byte aligned");
    if (B == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    mg_launch_gemm_batched(qh, H * dk, dk, B, dk, Wk, (long)dk * D, 1, nullptr, 0, D, U, D, (long)B * D, H, s);
    MG_CHECK_LAUNCH("mgnns_mha_train_fwd(U)");
    hipLaunchKernelGGL(train_attn_fwd_kernel, dim3(B), dim3(NT), 0, s, (const float*)U, bank, mask, B, L, D, H,
                       1.0f / sqrtf((float)dk), seed, rate, P, attn, keep, Z, SP);
    MG_CHECK_LAUNCH("mgnns_mha_train_fwd(attn)");
    mg_launch_gemm_batched(Z, D, (long)B * D, B, D, Wv, (long)dk * D, 0, nullptr, 0, dk, o, H * dk, dk, H, s);
    MG_CHECK_LAUNCH("mgnns_mha_train_fwd(o)");
    hipLaunchKernelGGL(add_scaled_bias_kernel, dim3(grid1d((size_t)B * H * dk)), dim3(256), 0, s, o, bv, (const float*)SP, B, H, dk);
    MG_CHECK_LAUNCH("mgnns_mha_train_fwd(bias)");
    return 0;
}

extern "C" size_t mgnns_mha_train_bwd_workspace_bytes(int B, int D, int H, int dk) {
    const size_t wk = wgrad_part_floats(B, dk, D, H);
    return sizeof(float) * (2 * (size_t)H * B * D + wk) + 64;
}

extern "C" int mgnns_mha_train_bwd(const float* dO, const float* qh, const float* bank, const float* mask, int B, int L, int D,
                                   int H, int dk, const float* Wk, const float* Wv, const float* bv, float rate, const float* U,
                                   const float* P, const float* attn, const uint8_t* keep, const float* Z, const float* SP,
                                   float* dqh, float* dWk, float* dWv, float* dbv, float* dbank, void* workspace,
                                   size_t workspace_bytes, mgnns_stream_t stream) {
    MG_REQUIRE(dO && qh && bank && Wk && Wv && bv && U && P && attn && keep && Z && SP && dqh && dWk && dWv && dbv && workspace,
               "mgnns_mha_train_bwd: null pointer");
    const char* bad = mha_train_shape_error(B, L, D, H, dk);
    MG_REQUIRE(!bad, "mgnns_mha_train_bwd: %s (B=%d L=%d D=%d H=%d dk=%d)", bad ? bad : "", B, L, D, H, dk);
    MG_REQUIRE(rate >= 0.f && rate <= 1.f, "mgnns_mha_train_bwd: dropout rate %g outside [0, 1]", (double)rate);
    MG_REQUIRE(mg_aligned16(bank) && mg_aligned16(U) && mg_aligned16(workspace) && (!dbank || mg_aligned16(dbank)),
               "mgnns_mha_train_bwd: bank/U/dbank/workspace must be 16-byte aligned");
    MG_REQUIRE(workspace_bytes >= mgnns_mha_train_bwd_workspace_bytes(B, D, H, dk), "mgnns_mha_train_bwd: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    if (B == 0) {
        (void)hipMemsetAsync(dWk, 0, sizeof(float) * H * dk * D, s);
        (void)hipMemsetAsync(dWv, 0, sizeof(float) * H * dk * D, s);
        (void)hipMemsetAsync(dbv, 0, sizeof(float) * H * dk, s);
        MG_CHECK_LAUNCH("mgnns_mha_train_bwd(B=0)");
        return 0;
    }
    float* Uu = reinterpret_cast<float*>(workspace);          // [H][B][D]  W_v,h^T dO_h
    float* R = Uu + (size_t)H * B * D;                        // [H][B][D]  X^T ds_h / T
    float* part = R + (size_t)H * B * D;
    mg_launch_gemm_batched(dO, H * dk, dk, B, dk, Wv, (long)dk * D, 1, nullptr, 0, D, Uu, D, (long)B * D, H, s);
    MG_CHECK_LAUNCH("mgnns_mha_train_bwd(u)");
    const float inv_temp = 1.0f / sqrtf((float)dk);
    hipLaunchKernelGGL(train_attn_bwd_kernel, dim3(B), dim3(NT), 0, s, U, (const float*)Uu, dO, bv, bank, mask, P, attn, keep, B,
                       L, D, H, dk, inv_temp, rate, R, dbank);
    MG_CHECK_LAUNCH("mgnns_mha_train_bwd(bank pass)");
    // dqh_h = W_k,h r_h / T  (R carries the 1/T)
    mg_launch_gemm_batched(R, D, (long)B * D, B, D, Wk, (long)dk * D, 0, nullptr, 0, dk, dqh, H * dk, dk, H, s);
    MG_CHECK_LAUNCH("mgnns_mha_train_bwd(dqh)");
    // dW_k,h = sum_b qh_h (x) r_h / T;   dW_v,h = sum_b dO_h (x) z_h,  db_v,h = sum_b dO_h sum_l p'
    WgradArgs a{qh, H * dk, dk, R, D, (long)B * D, nullptr, 0, B, dk, D, 0, 1, 0, dWk, D, (long)dk * D, nullptr, 0, part};
    launch_wgrad(a, H, s);
    MG_CHECK_LAUNCH("mgnns_mha_train_bwd(dWk)");
    WgradArgs v{dO, H * dk, dk, Z, D, (long)B * D, SP, B, B, dk, D, 1, 1, 0, dWv, D, (long)dk * D, dbv, dk, part};
    launch_wgrad(v, H, s);
    MG_CHECK_LAUNCH("mgnns_mha_train_bwd(dWv)");
    return 0;
}

extern "C" size_t mgnns_wgrad_workspace_bytes(int M, int N, int K) { return sizeof(float) * wgrad_part_floats(M, N, K, 1) + 64; }

extern "C" int mgnns_wgrad_fwd(const float* dY, int M, int N, const float* X, int K, float* dW, float* db, void* workspace,
                               size_t workspace_bytes, mgnns_stream_t stream) {
    MG_REQUIRE(dW && workspace && (M == 0 || (dY && X)), "mgnns_wgrad_fwd: null pointer");      // M = 0: dY, X may be empty
    MG_REQUIRE(M >= 0 && N > 0 && K > 0, "mgnns_wgrad_fwd: bad dims M=%d N=%d K=%d", M, N, K);
    MG_REQUIRE(workspace_bytes >= mgnns_wgrad_workspace_bytes(M, N, K), "mgnns_wgrad_fwd: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    if (M == 0) {
        (void)hipMemsetAsync(dW, 0, sizeof(float) * N * K, s);
        if (db) (void)hipMemsetAsync(db, 0, sizeof(float) * N, s);
        MG_CHECK_LAUNCH("mgnns_wgrad_fwd(M=0)");
        return 0;
    }
    WgradArgs a{dY, N, 0, X, K, 0, nullptr, 0, M, N, K, db ? 1 : 0, 1, 0, dW, K, 0, db, 0, reinterpret_cast<float*>(workspace)};
    launch_wgrad(a, 1, s);
    MG_CHECK_LAUNCH("mgnns_wgrad_fwd");
    return 0;
}

extern "C" int mgnns_drop_res_ln_fwd(const float* x, const float* res, int rows, int D, const float* gamma, const float* beta,
                                     float eps, uint64_t seed, int site, float rate, float* y, float* xhat, float* sig,
                                     uint8_t* keep, mgnns_stream_t stream) {
    MG_REQUIRE(x && res && gamma && beta && y && xhat && sig && keep, "mgnns_drop_res_ln_fwd: null pointer");
    MG_REQUIRE(rows >= 0 && D > 1 && D <= 64 * LNC, "mgnns_drop_res_ln_fwd: D=%d out of range (2..%d)", D, 64 * LNC);
    MG_REQUIRE(rate >= 0.f && rate <= 1.f, "mgnns_drop_res_ln_fwd: dropout rate %g outside [0, 1]", (double)rate);
    if (rows == 0) return 0;
    hipLaunchKernelGGL(drop_res_ln_fwd_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, res, rows, D, gamma,
                       beta, eps, seed, site, rate, y, xhat, sig, keep);
    MG_CHECK_LAUNCH("mgnns_drop_res_ln_fwd");
    return 0;
}

extern "C" int mgnns_drop_res_ln_bwd(const float* dy, const float* dy2, const float* xhat, const float* sig, const uint8_t* keep,
                                     int rows, int D, const float* gamma, float eps, float rate, float* dres, float* dx,
                                     float* dgamma, float* dbeta, mgnns_stream_t stream) {
    MG_REQUIRE(dy && xhat && sig && keep && gamma && dres && dx && dgamma && dbeta, "mgnns_drop_res_ln_bwd: null pointer");
    MG_REQUIRE(rows >= 0 && D > 1 && D <= 64 * LNC, "mgnns_drop_res_ln_bwd: D=%d out of range (2..%d)", D, 64 * LNC);
    hipStream_t s = (hipStream_t)stream;
    if (rows > 0)
        hipLaunchKernelGGL(drop_res_ln_bwd_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, dy, dy2, xhat, sig, keep, rows, D, gamma,
                           eps, rate, dres, dx);
    hipLaunchKernelGGL(ln_param_grad_kernel, dim3((D + 255) / 256), dim3(256), 0, s, dy, dy2, xhat, rows, D, dgamma, dbeta);
    MG_CHECK_LAUNCH("mgnns_drop_res_ln_bwd");
    return 0;
}

extern "C" int mgnns_train_eltwise(int op, const float* a, const float* b, int64_t n, float* y, mgnns_stream_t stream) {
    MG_REQUIRE(a && b && y, "mgnns_train_eltwise: null pointer");
    MG_REQUIRE(op == MGNNS_ELT_ADD || op == MGNNS_ELT_RELU_BWD || op == MGNNS_ELT_LRELU2_BWD, "mgnns_train_eltwise: unknown op %d",
               op);
    if (n <= 0) return 0;
    hipLaunchKernelGGL(eltwise_kernel, dim3(grid1d((size_t)n)), dim3(256), 0, (hipStream_t)stream, op, a, b, (long)n, y);
    MG_CHECK_LAUNCH("mgnns_train_eltwise");
    return 0;
}
