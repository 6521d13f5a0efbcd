// Gradient of the loss with respect to an image channel's feature map X [B, K, P] (MODEL:400-428, 450-455, 474), fp32.
// The map feeds the memory bank bank[b,p,:] = W X[b,:,p] + c and the max-pool pooled[b,k] = max_p X[b,k,p]:
//     dX[b,k,p] = sum_o W[o,k] dBank[b,p,o]  +  [p == arg[b,k]] dPooled[b,k]
// with arg[b,k] the FIRST p at which X[b,k,.] attains its maximum (torch's max_pool2d backward: a tie sends the whole gradient
// to the smallest index).  Two kernels: the argmax (one read of the map) and the data gradient on the exact-f32 MFMA
// (v_mfma_f32_16x16x4_f32) with the max-pool scatter folded into its epilogue.  Every output element is written by exactly
// one workgroup, the o reduction runs inside it in a fixed order: bit-identical from run to run.  DESIGN.md section 11.
#include "common.hpp"

namespace {

// ---- first-index argmax over p of every (b, k) row ------------------------------------------------------------------------
// A wave takes 4 consecutive rows at a time (their loads are issued together); lane l scans p = l, l + 64, .. (or four
// consecutive p per step when the rows are 16-byte aligned) in increasing order with a strict >, so it keeps its first
// maximum; the cross-lane reduction prefers the smaller index among equal values.
constexpr int AM_NT = 256;
constexpr int AM_ROWS = 4;

#define MG_DPP_I(v, ctrl) __builtin_amdgcn_update_dpp(0, (v), (ctrl), 0xF, 0xF, true)

__device__ __forceinline__ void argmax_take(float& best, int& bi, float v, int i) {
    if (v > best || (v == best && i < bi)) {
        best = v;
        bi = i;
    }
}

// -> wave-uniform (max, first index): DPP inside the four rows of 16 lanes, then the four row results through v_readlane
__device__ __forceinline__ int wave_argmax_first(float best, int bi) {
    argmax_take(best, bi, MG_DPP(best, 0xB1), MG_DPP_I(bi, 0xB1));
    argmax_take(best, bi, MG_DPP(best, 0x4E), MG_DPP_I(bi, 0x4E));
    argmax_take(best, bi, MG_DPP(best, 0x141), MG_DPP_I(bi, 0x141));
    argmax_take(best, bi, MG_DPP(best, 0x140), MG_DPP_I(bi, 0x140));
    float v = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, best), 0));
    int i = __builtin_amdgcn_readlane(bi, 0);
#pragma unroll
    for (int l = 16; l < 64; l += 16)
        argmax_take(v, i, __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, best), l)),
                    __builtin_amdgcn_readlane(bi, l));
    return i;
}

template <int VEC>
__global__ __launch_bounds__(AM_NT) void map_argmax_kernel(const float* __restrict__ X, long rows, int P, int* __restrict__ arg) {
    const int lane = threadIdx.x & 63;
    const long nw = (long)gridDim.x * (AM_NT / 64);
    const int n = P / VEC;                         // steps of VEC elements per row (VEC = 4: P % 4 == 0)
    for (long g = (long)blockIdx.x * (AM_NT / 64) + (threadIdx.x >> 6); g * AM_ROWS < rows; g += nw) {
        const long row0 = g * AM_ROWS;
        float best[AM_ROWS];
        int bi[AM_ROWS];
#pragma unroll
        for (int u = 0; u < AM_ROWS; ++u) {
            best[u] = -INFINITY;
            bi[u] = 0x7fffffff;
        }
        for (int c0 = 0; c0 < n; c0 += 64) {
            const int c = c0 + lane;
            if constexpr (VEC == 4) {
                float4 v[AM_ROWS];
#pragma unroll
                for (int u = 0; u < AM_ROWS; ++u)
                    v[u] = (c < n && row0 + u < rows) ? reinterpret_cast<const float4*>(X + (size_t)(row0 + u) * P)[c]
                                                      : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
                for (int u = 0; u < AM_ROWS; ++u) {
                    if (v[u].x > best[u]) { best[u] = v[u].x; bi[u] = 4 * c; }
                    if (v[u].y > best[u]) { best[u] = v[u].y; bi[u] = 4 * c + 1; }
                    if (v[u].z > best[u]) { best[u] = v[u].z; bi[u] = 4 * c + 2; }
                    if (v[u].w > best[u]) { best[u] = v[u].w; bi[u] = 4 * c + 3; }
                }
            } else {
                float v[AM_ROWS];
#pragma unroll
                for (int u = 0; u < AM_ROWS; ++u)
                    v[u] = (c < n && row0 + u < rows) ? X[(size_t)(row0 + u) * P + c] : -INFINITY;
#pragma unroll
                for (int u = 0; u < AM_ROWS; ++u)
                    if (v[u] > best[u]) { best[u] = v[u]; bi[u] = c; }
            }
        }
#pragma unroll
        for (int u = 0; u < AM_ROWS; ++u) {
            const int i = wave_argmax_first(best[u], bi[u]);
            if (lane == 0 && row0 + u < rows) arg[row0 + u] = i < P ? i : 0;      // a row of -inf only: index 0, as torch
        }
    }
}

// ---- data gradient of the image bank + max-pool scatter ------------------------------------------------------------------
// GEMM view per sample b: M = k (channels), N = p (positions), reduction over o <= 320.  A[k][o] = W[o][k] (row o of W is
// contiguous in k), B[o][p] = dBank[b][p][o] (row p of dBank is contiguous in o).  A workgroup (8 waves) owns 128 channels x
// 208 positions (13 MFMA tiles: all of P = 196) of one sample and the whole reduction: it stages 32 o at a time in LDS (A as
// [o][k], B as [p][o]); wave w computes channel tile w x the 13 position tiles: 13 accumulators of 16 x 16.
// The C/D map of the MFMA puts p on lane & 15, so a direct store would write 64-byte pieces.  Instead the accumulators of 64
// channels at a time go to LDS as [k][p] with the row stride of the output: with one position block (P <= 208) those 64 rows
// are one contiguous range of dX, which all 512 threads copy out 16 bytes per lane -- whole 128-byte lines.  The max-pool
// term is added in LDS before the copy (one thread per channel), so dX is written exactly once.
// Block ids: id & 7 picks the XCD on this chip, so sample b = 8 (..) + (id & 7) keeps all channel blocks of a sample -- the
// readers of dBank[b] -- on one XCD's L2 (a placement for speed only).
constexpr int DG_K = 128;                  // channels per workgroup (8 MFMA tiles)
constexpr int DG_PT = 13;                  // position tiles per workgroup
constexpr int DG_P = 16 * DG_PT;           // 208
constexpr int DG_O = 32;                   // o per LDS stage
constexpr int DG_OMAX = 320;
constexpr int DG_NT = 512;
constexpr int DG_AS_LD = 144;              // [o][k] row stride: 144 = 16 mod 64 banks, the 4 o rows of a read are disjoint
constexpr int DG_BS_LD = 36;               // [p][o] row stride: 36 p apart in 64 banks + 4 o -> no conflict
constexpr int DG_HALF = 64;                // channels staged per epilogue round
constexpr int DG_A_PER_T = DG_O * DG_K / DG_NT;      // 8
constexpr int DG_B_PER_T = DG_O * DG_P / DG_NT;      // 13
constexpr int DG_LDS = DG_HALF * DG_P > DG_O * DG_AS_LD + DG_P * DG_BS_LD ? DG_HALF * DG_P : DG_O * DG_AS_LD + DG_P * DG_BS_LD;

__global__ __launch_bounds__(DG_NT, 4) void imgbank_dgrad_kernel(const float* __restrict__ dbank, const float* __restrict__ W,
                                                                 const float* __restrict__ dpooled, const int* __restrict__ arg,
                                                                 int B, int K, int P, int N, int kblocks, int pblocks,
                                                                 float* __restrict__ dX) {
    __shared__ __attribute__((aligned(16))) float lds[DG_LDS];
    float* As = lds;
    float* Bs = lds + DG_O * DG_AS_LD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long slot = (long)blockIdx.x >> 3;
    const int tiles = kblocks * pblocks;
    const long b = slot / tiles * 8 + (blockIdx.x & 7);
    if (b >= B) return;
    const int t = (int)(slot % tiles);
    const int k0 = (t % kblocks) * DG_K, p0 = (t / kblocks) * DG_P;
    const int pw = P - p0 < DG_P ? P - p0 : DG_P;

    f32x4 acc[DG_PT];
#pragma unroll
    for (int j = 0; j < DG_PT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

    if (dbank) {
        const float* db = dbank + (size_t)b * P * N;
        float ra[DG_A_PER_T], rb[DG_B_PER_T];
        // a stage: A element (o = tid / 128 + 4 i, k = tid % 128), B element (p = tid / 32 + 16 i, o = tid % 32): consecutive
        // lanes, consecutive addresses
        const int ak = tid & (DG_K - 1), ao = tid >> 7;
        const int bo = tid & (DG_O - 1), bp = tid >> 5;
        auto load = [&](int o0) {
#pragma unroll
            for (int i = 0; i < DG_A_PER_T; ++i) {
                const int o = o0 + ao + 4 * i;
                ra[i] = (o < N && k0 + ak < K) ? W[(size_t)o * K + k0 + ak] : 0.f;
            }
#pragma unroll
            for (int i = 0; i < DG_B_PER_T; ++i) {
                const int p = p0 + bp + 16 * i;
                rb[i] = (p < P && o0 + bo < N) ? db[(size_t)p * N + o0 + bo] : 0.f;
            }
        };
        auto store = [&]() {
#pragma unroll
            for (int i = 0; i < DG_A_PER_T; ++i) As[(ao + 4 * i) * DG_AS_LD + ak] = ra[i];
#pragma unroll
            for (int i = 0; i < DG_B_PER_T; ++i) Bs[(bp + 16 * i) * DG_BS_LD + bo] = rb[i];
        };
        load(0);
        for (int o0 = 0; o0 < N; o0 += DG_O) {
            __syncthreads();                       // the previous stage's reads are done
            store();
            __syncthreads();
            if (o0 + DG_O < N) load(o0 + DG_O);    // next stage in flight under the MFMAs
#pragma unroll 1                           // (unrolled, the 13 B fragments of several steps are live at once and spill)
            for (int ks = 0; ks < DG_O / 4; ++ks) {
                const int kr = 4 * ks + (lane >> 4);
                const float a = As[kr * DG_AS_LD + wave * 16 + (lane & 15)];
                float bv[DG_PT];
#pragma unroll
                for (int j = 0; j < DG_PT; ++j) bv[j] = Bs[(j * 16 + (lane & 15)) * DG_BS_LD + kr];
#pragma unroll
                for (int j = 0; j < DG_PT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv[j], acc[j], 0, 0, 0);
            }
        }
    }

    // C/D map of the 16x16 f32 MFMA: row (channel) 4 (lane >> 4) + r, column (position) lane & 15
    float* St = lds;                               // [DG_HALF][pw]
#pragma unroll
    for (int h = 0; h < DG_K / DG_HALF; ++h) {
        __syncthreads();                           // the last stage's reads / the previous round's copy are done
        if ((wave >> 2) == h) {
#pragma unroll
            for (int j = 0; j < DG_PT; ++j) {
                const int col = 16 * j + (lane & 15);
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (col < pw) St[((wave & 3) * 16 + 4 * (lane >> 4) + r) * pw + col] = acc[j][r];
            }
        }
        __syncthreads();
        const int kh = k0 + h * DG_HALF;
        const int rows = K - kh < DG_HALF ? K - kh : DG_HALF;       // <= 0: nothing left
        if (dpooled) {
            if (tid < rows) {
                const int a = arg[(size_t)b * K + kh + tid] - p0;
                if ((unsigned)a < (unsigned)pw) St[tid * pw + a] += dpooled[(size_t)b * K + kh + tid];
            }
            __syncthreads();
        }
        const int n = rows * pw;
        if (pw == P) {                             // one position block: rows kh .. kh + rows are one contiguous range
            float* out = dX + ((size_t)b * K + kh) * P;
            int i0 = 0;
            if ((reinterpret_cast<uintptr_t>(out) & 15u) == 0) {
                for (int i = tid; i < n / 4; i += DG_NT)
                    reinterpret_cast<float4*>(out)[i] = reinterpret_cast<const float4*>(St)[i];
                i0 = n > 0 ? n / 4 * 4 : 0;
            }
            for (int i = i0 + tid; i < n; i += DG_NT) out[i] = St[i];
        } else {
            for (int i = tid; i < n; i += DG_NT) {
                const int row = i / pw, c = i - row * pw;
                dX[((size_t)b * K + kh + row) * P + p0 + c] = St[i];
            }
        }
    }
}

}  // namespace

extern "C" int mgnns_map_argmax(const float* X, int B, int K, int P, int32_t* arg, mgnns_stream_t stream) {
    MG_REQUIRE(B == 0 || (X && arg), "mgnns_map_argmax: null pointer");
    MG_REQUIRE(B >= 0 && K > 0 && P > 0, "mgnns_map_argmax: need B >= 0, K, P > 0 (B=%d K=%d P=%d)", B, K, P);
    MG_REQUIRE((long)B * K < (1L << 31) && (long)B * K * P < (1L << 40), "mgnns_map_argmax: feature map too large");
    if (B == 0) return 0;
    const long rows = (long)B * K;
    const long groups = (rows + AM_ROWS * (AM_NT / 64) - 1) / (AM_ROWS * (AM_NT / 64));
    const dim3 grid((unsigned)(groups < 65536 ? groups : 65536));
    if (P % 4 == 0 && mg_aligned16(X))
        hipLaunchKernelGGL(map_argmax_kernel<4>, grid, dim3(AM_NT), 0, (hipStream_t)stream, X, rows, P, arg);
    else
        hipLaunchKernelGGL(map_argmax_kernel<1>, grid, dim3(AM_NT), 0, (hipStream_t)stream, X, rows, P, arg);
    MG_CHECK_LAUNCH("mgnns_map_argmax");
    return 0;
}

extern "C" int mgnns_imgbank_dgrad(const float* dbank, const float* W, const float* dpooled, const int32_t* arg, int B, int K,
                                   int P, int N, float* dX, mgnns_stream_t stream) {
    MG_REQUIRE(B >= 0 && K > 0 && P > 0 && N > 0 && N <= DG_OMAX, "mgnns_imgbank_dgrad: need B >= 0, K, P > 0, 0 < N <= %d "
               "(B=%d K=%d P=%d N=%d)", DG_OMAX, B, K, P, N);
    MG_REQUIRE((dpooled == nullptr) == (arg == nullptr), "mgnns_imgbank_dgrad: dpooled and arg come together");
    MG_REQUIRE(B == 0 || (dX && (dbank || dpooled) && (!dbank || W)), "mgnns_imgbank_dgrad: null pointer");
    MG_REQUIRE((long)B * K * P < (1L << 40), "mgnns_imgbank_dgrad: feature map too large");
    if (B == 0) return 0;
    const int kblocks = (K + DG_K - 1) / DG_K, pblocks = (P + DG_P - 1) / DG_P;
    const long blocks = ((long)B + 7) / 8 * 8 * kblocks * pblocks;
    MG_REQUIRE(blocks < (1L << 31), "mgnns_imgbank_dgrad: too many blocks (B=%d K=%d P=%d)", B, K, P);
    hipLaunchKernelGGL(imgbank_dgrad_kernel, dim3((unsigned)blocks), dim3(DG_NT), 0, (hipStream_t)stream, dbank, W, dpooled,
                       (const int*)arg, B, K, P, N, kblocks, pblocks, dX);
    MG_CHECK_LAUNCH("mgnns_imgbank_dgrad");
    return 0;
}
