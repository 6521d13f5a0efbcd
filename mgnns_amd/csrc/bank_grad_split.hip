// Split-bf16 ("bf16x3") backward of the image memory banks: the fp32-class siblings of imgbank_wgrad_kernel (model_train.hip)
// and imgbank_dgrad_kernel (map_grad.hip) on the bf16 matrix pipe, with those kernels' contracts:
//     dW[o,c]   = sum_{b,p} dBank[b,p,o] X[b,c,p],   db[o] = sum_{b,p} dBank[b,p,o]
//     dX[b,k,p] = sum_o W[o,k] dBank[b,p,o]  +  [p == arg[b,k]] dPooled[b,k]
// Every fp32 operand x is carried as hi = bf16(x), lo = bf16(x - hi) (round to nearest even, bf16.hpp) and a product
// is a_hi b_lo + a_lo b_hi + a_hi b_hi on v_mfma_f32_16x16x32_bf16 into one fp32 accumulator: ~2^-16 relative per product.
// All inputs are plain fp32 in HBM in today's layouts; the split happens while a stage is written to LDS.  An operand fragment
// of the 16x16x32 MFMA is 8 consecutive reduction indices of one row per lane (16 bytes): LDS holds 16-byte chunks as
// [chunk of 8 reduction indices][row], so the 16 lanes of a ds_read_b128 group read 256 contiguous bytes and 8 consecutive
// lanes of a ds_write_b128 write 128 (no bank conflict on either side).  Fixed summation order everywhere: bit-identical
// from call to call.  DESIGN.md section 11.
#include <type_traits>
#include "common.hpp"
#include "bf16.hpp"


namespace {

__device__ __forceinline__ f32x4 bs_mfma(uint4 a, uint4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// ---- weight gradient -------------------------------------------------------------------------------------------------------
// GEMM view as the fp32 kernel's: M = o (<= 320), N = c, reduction k = b * P + p over a slab of the flattened (sample, position)
// pairs.  A workgroup (8 waves) owns 320 o x 128 channels and one slab; a stage is 32 k (one MFMA k-step), double buffered in
// LDS (one barrier per stage), the fp32 values of the next stage in registers under the MFMAs.  Wave w computes o tiles
// 5 (w & 3) .. +5 x channel tiles 4 (w >> 2) .. +4: 20 accumulators, 60 MFMAs per stage.
// Staging: a task is one chunk = 8 consecutive k of one row.  dBank (contiguous in o): lane = o, 8 loads a row of N apart
// (coalesced over the lanes) -- the transposition costs nothing.  X (contiguous in p inside a sample): two 16-byte loads per
// chunk where P % 4 == 0 (a quad then never crosses a sample), else 8 scalar loads with the (b, p) pair carried along.
constexpr int WS_O = 320;
constexpr int WS_C = 128;
constexpr int WS_K = 32;
constexpr int WS_NT = 512;
constexpr int WS_OT = 5, WS_CT = 4;                       // tiles per wave
constexpr int WS_A_TASKS = 4 * WS_O;                      // 1280 chunks of A per stage: 2.5 per thread
constexpr int WS_A_PER_T = (WS_A_TASKS + WS_NT - 1) / WS_NT;
constexpr int WS_STAGE = 4 * WS_O + 4 * WS_C;             // chunks per image (hi or lo) and stage
constexpr size_t WS_LDS = (size_t)2 * 2 * WS_STAGE * 16;  // 2 stages x (hi, lo): 114688 bytes

template <int VEC>
__global__ __launch_bounds__(WS_NT) void imgbank_wgrad_split_kernel(const float* __restrict__ X, const float* __restrict__ dbank,
                                                                    int K, int P, int N, long KK, long kslab, int direct,
                                                                    float* __restrict__ dW, float* __restrict__ db,
                                                                    float* __restrict__ part, float* __restrict__ part_db) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint4* lds = reinterpret_cast<uint4*>(smem);          // stage st: hi image at st * 2 * WS_STAGE, lo image WS_STAGE behind it;
                                                          // an image: A [4][320] then B [4][128]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fg = lane >> 4;
    const int c0 = blockIdx.x * WS_C;
    const int s = blockIdx.y;
    const long kb = (long)s * kslab;
    const long ke = kb + kslab < KK ? kb + kslab : KK;
    const int og = wave & 3, cg = wave >> 2;
    const bool do_db = blockIdx.x == 0;

    f32x4 acc[WS_OT][WS_CT];
#pragma unroll
    for (int i = 0; i < WS_OT; ++i)
#pragma unroll
        for (int j = 0; j < WS_CT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float dbacc[WS_A_PER_T];
#pragma unroll
    for (int i = 0; i < WS_A_PER_T; ++i) dbacc[i] = 0.f;

    // A tasks t = tid + 512 i < 1280: chunk kc = t / 320 of row o = t % 320 (a wave never straddles a chunk: 320 = 5 x 64)
    // B task: row c = 8 (tid >> 5) + (tid & 7), chunk kc = (tid >> 3) & 3 (8 consecutive lanes = 8 consecutive rows)
    const int bc = 8 * (tid >> 5) + (tid & 7), bkc = (tid >> 3) & 3;
    const bool bc_on = c0 + bc < K;
    // (b, p) of the B task's first k of the stage to load next
    long xb;
    int xp;
    {
        const long k = kb + 8 * bkc;
        xb = k / P;
        xp = (int)(k - xb * P);
    }
    float ra[WS_A_PER_T][8], rb[8];
    auto load = [&](long k0) {
#pragma unroll
        for (int i = 0; i < WS_A_PER_T; ++i) {
            const int t = tid + WS_NT * i;
            if (t < WS_A_TASKS) {                                   // (i = 2: waves 0-3 only, wave-uniform)
                const int kc = t / WS_O, o = t - kc * WS_O;
                const long k = k0 + 8 * kc;
#pragma unroll
                for (int j = 0; j < 8; ++j) ra[i][j] = (k + j < ke && o < N) ? dbank[(size_t)(k + j) * N + o] : 0.f;
            }
        }
        const long k = k0 + 8 * bkc;
        if constexpr (VEC == 4) {
            // P % 4 == 0, X 16-byte aligned, k % 4 == 0: a quad lies inside one sample, wholly in front of ke or behind it
            long b2 = xb;
            int p2 = xp;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
                if (bc_on && k + 4 * h < ke) v = *reinterpret_cast<const f32x4*>(X + ((size_t)b2 * K + c0 + bc) * P + p2);
#pragma unroll
                for (int j = 0; j < 4; ++j) rb[4 * h + j] = v[j];
                p2 += 4;
                if (p2 >= P) {
                    p2 -= P;
                    ++b2;
                }
            }
        } else {
            long b2 = xb;
            int p2 = xp;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                rb[j] = (bc_on && k + j < ke) ? X[((size_t)b2 * K + c0 + bc) * P + p2] : 0.f;
                if (++p2 == P) {
                    p2 = 0;
                    ++b2;
                }
            }
        }
        xp += WS_K;                                                 // the next stage's first k
        if (xp >= P) {
            const int q = xp / P;
            xb += q;
            xp -= q * P;
        }
    };
    auto store = [&](int st) {
        uint4* hi = lds + (size_t)st * 2 * WS_STAGE;
        uint4* lo = hi + WS_STAGE;
#pragma unroll
        for (int i = 0; i < WS_A_PER_T; ++i) {
            const int t = tid + WS_NT * i;
            if (t < WS_A_TASKS) {
                if (do_db) dbacc[i] += ((ra[i][0] + ra[i][1]) + (ra[i][2] + ra[i][3])) + ((ra[i][4] + ra[i][5]) + (ra[i][6] + ra[i][7]));
                uint4 h, l;
                mg_split8(ra[i], h, l);
                hi[t] = h;                                          // [kc][o] = kc * 320 + o = t
                lo[t] = l;
            }
        }
        uint4 h, l;
        mg_split8(rb, h, l);
        hi[4 * WS_O + bkc * WS_C + bc] = h;
        lo[4 * WS_O + bkc * WS_C + bc] = l;
    };

    if (kb < ke) {
        load(kb);
        store(0);
    }
    __syncthreads();
    int st = 0;
    for (long k0 = kb; k0 < ke; k0 += WS_K, st ^= 1) {
        const bool more = k0 + WS_K < ke;
        if (more) load(k0 + WS_K);                                  // in flight under the MFMAs
        const uint4* hi = lds + (size_t)st * 2 * WS_STAGE;
        const uint4* lo = hi + WS_STAGE;
        uint4 bh[WS_CT], bl[WS_CT];
#pragma unroll
        for (int j = 0; j < WS_CT; ++j) {
            const int at = 4 * WS_O + fg * WS_C + (cg * WS_CT + j) * 16 + fr;
            bh[j] = hi[at];
            bl[j] = lo[at];
        }
#pragma unroll
        for (int i = 0; i < WS_OT; ++i) {
            const int at = fg * WS_O + (og * WS_OT + i) * 16 + fr;
            const uint4 ah = hi[at], al = lo[at];
#pragma unroll
            for (int j = 0; j < WS_CT; ++j) acc[i][j] = bs_mfma(ah, bl[j], acc[i][j]);
#pragma unroll
            for (int j = 0; j < WS_CT; ++j) acc[i][j] = bs_mfma(al, bh[j], acc[i][j]);
#pragma unroll
            for (int j = 0; j < WS_CT; ++j) acc[i][j] = bs_mfma(ah, bh[j], acc[i][j]);
        }
        if (more) store(st ^ 1);                                    // (its last readers passed the barrier of the previous stage)
        __syncthreads();
    }

    // C/D map of the 16x16 MFMA: row (o) 4 (lane >> 4) + r, column (c) lane & 15
    float* out = direct ? dW : part + (size_t)s * N * K;
#pragma unroll
    for (int i = 0; i < WS_OT; ++i)
#pragma unroll
        for (int j = 0; j < WS_CT; ++j) {
            const int c = c0 + (cg * WS_CT + j) * 16 + fr;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int o = (og * WS_OT + i) * 16 + 4 * fg + r;
                if (o < N && c < K) out[(size_t)o * K + c] = acc[i][j][r];
            }
        }
    if (do_db) {
        // the four chunk columns of an o, in order (the loop's last barrier freed the LDS)
        float* red = reinterpret_cast<float*>(smem);
#pragma unroll
        for (int i = 0; i < WS_A_PER_T; ++i) {
            const int t = tid + WS_NT * i;
            if (t < WS_A_TASKS) red[t] = dbacc[i];
        }
        __syncthreads();
        if (tid < N) {
            const float v = (red[tid] + red[WS_O + tid]) + (red[2 * WS_O + tid] + red[3 * WS_O + tid]);
            if (direct) db[tid] = v;
            else part_db[(size_t)s * N + tid] = v;
        }
    }
}

// dW = sum_s part[s], db = sum_s part_db[s], slabs in order
__global__ void imgbank_wgrad_split_combine_kernel(const float* __restrict__ part, const float* __restrict__ part_db, int nslab,
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

// slabs of the reduction: one workgroup per CU (112 KB of LDS each), at most 64, at least one stage each
int wgrad_split_nslab(int B, int K, int P) {
    const long chunks = ((long)B * P + WS_K - 1) / WS_K;
    const int cblocks = (K + WS_C - 1) / WS_C;
    int cu = mg_cu_count();
    if (cu <= 0) cu = 256;
    long ns = ((long)cu + cblocks - 1) / cblocks;
    if (ns > chunks) ns = chunks;
    if (ns > 64) ns = 64;
    return ns < 1 ? 1 : (int)ns;
}

// ---- data gradient + max-pool scatter -------------------------------------------------------------------------------------
// GEMM view per sample as the fp32 kernel's: M = k (channels), N = p (positions), reduction over o <= 320 = 10 k-steps of 32.
// A[k][o] = W[o][k]: the transposed, split weight is made once per call by imgbank_wsplit_kernel into the workspace, as 16-byte
// chunks [o / 8][k] (k padded to whole blocks of 128, o to 320, zeros) -- an MFMA A fragment is then one 16-byte load per lane,
// 16 lanes 256 contiguous bytes, straight from L2 into registers one k-step ahead.  B[o][p] = dBank[b][p][o] is contiguous
// along the reduction: a chunk is 8 consecutive floats of a dBank row, split while it is staged to LDS (double buffered, one
// barrier per k-step).  A workgroup (8 waves) owns 128 channels x 208 positions of one sample and the whole reduction; wave w
// computes channel tiles 2 (w & 3), +1 x position tiles 7 (w >> 2) .. +7 (the 14th tile is padding: 13 x 16 = 208).
// Epilogue, block ids and XCD placement: those of imgbank_dgrad_kernel.
constexpr int DS_K = 128;
constexpr int DS_PT = 13;
constexpr int DS_P = 16 * DS_PT;           // 208
constexpr int DS_PR = 224;                 // LDS rows per chunk column (14 tiles)
constexpr int DS_PW = 7;                   // position tiles per wave
constexpr int DS_O = 32;
constexpr int DS_OMAX = 320;
constexpr int DS_OC = DS_OMAX / 8;         // 40 chunk rows of the split weight
constexpr int DS_NT = 512;
constexpr int DS_HALF = 64;                // channels staged per epilogue round
constexpr int DS_TASKS = 4 * DS_PR;        // 896 chunks of B per k-step
constexpr int DS_B_PER_T = (DS_TASKS + DS_NT - 1) / DS_NT;       // 2
constexpr int DS_STAGE = 4 * DS_PR;        // chunks per image and stage
constexpr int DS_LDS_BYTES = 2 * 2 * DS_STAGE * 16;              // 57344
static_assert(DS_HALF * DS_P * 4 <= DS_LDS_BYTES, "the epilogue tile fits the staging buffers");

// W [N, K] fp32 -> Wh, Wl [DS_OC][Kp] chunks: chunk (oc, k) = W[8 oc .. 8 oc + 7][k], zeros outside
__global__ void imgbank_wsplit_kernel(const float* __restrict__ W, int N, int K, int Kp, uint4* __restrict__ Wh, uint4* __restrict__ Wl) {
    const long n = (long)DS_OC * Kp;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int oc = (int)(i / Kp), k = (int)(i - (long)oc * Kp);
        float x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = (k < K && 8 * oc + j < N) ? W[(size_t)(8 * oc + j) * K + k] : 0.f;
        uint4 h, l;
        mg_split8(x, h, l);
        Wh[i] = h;
        Wl[i] = l;
    }
}

template <int VEC>
__global__ __launch_bounds__(DS_NT) void imgbank_dgrad_split_kernel(const float* __restrict__ dbank, const uint4* __restrict__ Wh,
                                                                    const uint4* __restrict__ Wl, const float* __restrict__ dpooled,
                                                                    const int* __restrict__ arg, int B, int K, int P, int N, int Kp,
                                                                    int kblocks, int pblocks, float* __restrict__ dX) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[DS_LDS_BYTES];
    uint4* lds = reinterpret_cast<uint4*>(smem);           // stage st: hi image [4][224] at st * 2 * DS_STAGE, lo image behind it
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fg = lane >> 4;
    const long slot = (long)blockIdx.x >> 3;
    const int tiles = kblocks * pblocks;
    const long b = slot / tiles * 8 + (blockIdx.x & 7);
    if (b >= B) return;
    const int t = (int)(slot % tiles);
    const int k0 = (t % kblocks) * DS_K, p0 = (t / kblocks) * DS_P;
    const int pw = P - p0 < DS_P ? P - p0 : DS_P;
    const int cg = wave & 3, ph = wave >> 2;
    const int nks = (N + DS_O - 1) / DS_O;

    f32x4 acc[2][DS_PW];
#pragma unroll
    for (int ci = 0; ci < 2; ++ci)
#pragma unroll
        for (int j = 0; j < DS_PW; ++j) acc[ci][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const float* dbs = dbank + (size_t)b * P * N;
    // B tasks u = tid + 512 i < 896: row p = 8 (u >> 5) + (u & 7), chunk oc = (u >> 3) & 3
    float rb[DS_B_PER_T][8];
    auto load = [&](int ks) {
#pragma unroll
        for (int i = 0; i < DS_B_PER_T; ++i) {
            const int u = tid + DS_NT * i;
            if (u < DS_TASKS) {
                const int p = 8 * (u >> 5) + (u & 7), o = ks * DS_O + 8 * ((u >> 3) & 3);
                const float* row = dbs + (size_t)(p0 + p) * N + o;
                const bool on = p < pw;
                if constexpr (VEC == 4) {                            // N % 4 == 0, dbank 16-byte aligned: whole quads
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
                        if (on && o + 4 * h < N) v = *reinterpret_cast<const f32x4*>(row + 4 * h);
#pragma unroll
                        for (int j = 0; j < 4; ++j) rb[i][4 * h + j] = v[j];
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) rb[i][j] = (on && o + j < N) ? row[j] : 0.f;
                }
            }
        }
    };
    auto store = [&](int st) {
        uint4* hi = lds + (size_t)st * 2 * DS_STAGE;
        uint4* lo = hi + DS_STAGE;
#pragma unroll
        for (int i = 0; i < DS_B_PER_T; ++i) {
            const int u = tid + DS_NT * i;
            if (u < DS_TASKS) {
                uint4 h, l;
                mg_split8(rb[i], h, l);
                const int at = ((u >> 3) & 3) * DS_PR + 8 * (u >> 5) + (u & 7);
                hi[at] = h;
                lo[at] = l;
            }
        }
    };
    // A fragments of this wave's two channel tiles: chunk row 4 ks + fg, channel k0 + 16 (2 cg + ci) + fr (< Kp: padded)
    uint4 ah[2][2], al[2][2];
    auto aload = [&](int ks, int slotA) {
#pragma unroll
        for (int ci = 0; ci < 2; ++ci) {
            const size_t at = (size_t)(4 * ks + fg) * Kp + k0 + 16 * (2 * cg + ci) + fr;
            ah[slotA][ci] = Wh[at];
            al[slotA][ci] = Wl[at];
        }
    };

    load(0);
    aload(0, 0);
    store(0);
    __syncthreads();
    auto kstep = [&](int ks, auto sa) {
        constexpr int SA = decltype(sa)::value;
        const int st = ks & 1;
        const bool more = ks + 1 < nks;
        if (more) {
            load(ks + 1);
            aload(ks + 1, SA ^ 1);
        }
        const uint4* hi = lds + (size_t)st * 2 * DS_STAGE;
        const uint4* lo = hi + DS_STAGE;
#pragma unroll
        for (int j = 0; j < DS_PW; ++j) {
            if (j == DS_PW - 1 && ph == 1) continue;                // the padding tile (wave-uniform)
            const int at = fg * DS_PR + (ph * DS_PW + j) * 16 + fr;
            const uint4 bh = hi[at], bl = lo[at];
            acc[0][j] = bs_mfma(ah[SA][0], bl, acc[0][j]);
            acc[1][j] = bs_mfma(ah[SA][1], bl, acc[1][j]);
            acc[0][j] = bs_mfma(al[SA][0], bh, acc[0][j]);
            acc[1][j] = bs_mfma(al[SA][1], bh, acc[1][j]);
            acc[0][j] = bs_mfma(ah[SA][0], bh, acc[0][j]);
            acc[1][j] = bs_mfma(ah[SA][1], bh, acc[1][j]);
        }
        if (more) store(st ^ 1);
        __syncthreads();
    };
    for (int ks = 0; ks < nks; ks += 2) {
        kstep(ks, std::integral_constant<int, 0>{});
        if (ks + 1 < nks) kstep(ks + 1, std::integral_constant<int, 1>{});
    }

    // C/D map of the 16x16 MFMA: row (channel) 4 (lane >> 4) + r, column (position) lane & 15
    float* St = reinterpret_cast<float*>(smem);            // [DS_HALF][pw]; the loop's last barrier freed the LDS
#pragma unroll
    for (int h = 0; h < DS_K / DS_HALF; ++h) {
        if (h) __syncthreads();                            // the previous round's copy is done
        if ((cg >> 1) == h) {
#pragma unroll
            for (int ci = 0; ci < 2; ++ci)
#pragma unroll
                for (int j = 0; j < DS_PW; ++j) {
                    const int col = (ph * DS_PW + j) * 16 + fr;
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (col < pw) St[(((cg & 1) * 2 + ci) * 16 + 4 * fg + r) * pw + col] = acc[ci][j][r];
                }
        }
        __syncthreads();
        const int kh = k0 + h * DS_HALF;
        const int rows = K - kh < DS_HALF ? K - kh : DS_HALF;       // <= 0: nothing left
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
                for (int i = tid; i < n / 4; i += DS_NT)
                    reinterpret_cast<float4*>(out)[i] = reinterpret_cast<const float4*>(St)[i];
                i0 = n > 0 ? n / 4 * 4 : 0;
            }
            for (int i = i0 + tid; i < n; i += DS_NT) out[i] = St[i];
        } else {
            for (int i = tid; i < n; i += DS_NT) {
                const int row = i / pw, c = i - row * pw;
                dX[((size_t)b * K + kh + row) * P + p0 + c] = St[i];
            }
        }
    }
}

unsigned bs_grid_for(long n) {
    long g = (n + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

}  // namespace

extern "C" size_t mgnns_imgbank_wgrad_split_workspace_bytes(int B, int K, int P, int N) {
    if (B <= 0 || K <= 0 || P <= 0 || N <= 0) return 64;
    const int ns = wgrad_split_nslab(B, K, P);
    return ns > 1 ? sizeof(float) * (size_t)ns * N * ((size_t)K + 1) + 64 : 64;
}

extern "C" int mgnns_imgbank_wgrad_split(const float* X, const float* dbank, int B, int K, int P, int N, float* dW, float* db,
                                         void* workspace, size_t workspace_bytes, mgnns_stream_t stream) {
    MG_REQUIRE(dW && db && workspace && (B == 0 || (X && dbank)), "mgnns_imgbank_wgrad_split: null pointer");   // B = 0: empty maps
    MG_REQUIRE(B >= 0 && K > 0 && P > 0 && N > 0 && N <= WS_O, "mgnns_imgbank_wgrad_split: need B >= 0, K, P > 0, 0 < N <= %d "
               "(B=%d K=%d P=%d N=%d)", WS_O, B, K, P, N);
    MG_REQUIRE((long)B * K * P < (1L << 40), "mgnns_imgbank_wgrad_split: feature map too large");
    MG_REQUIRE(workspace_bytes >= mgnns_imgbank_wgrad_split_workspace_bytes(B, K, P, N),
               "mgnns_imgbank_wgrad_split: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    if (B == 0) {
        (void)hipMemsetAsync(dW, 0, sizeof(float) * N * K, s);
        (void)hipMemsetAsync(db, 0, sizeof(float) * N, s);
        MG_CHECK_LAUNCH("mgnns_imgbank_wgrad_split(B=0)");
        return 0;
    }
    const long KK = (long)B * P;
    const int ns = wgrad_split_nslab(B, K, P);
    const long chunks = (KK + WS_K - 1) / WS_K;
    const long kslab = (chunks + ns - 1) / ns * WS_K;
    const int nslab = (int)((KK + kslab - 1) / kslab);
    float* part = reinterpret_cast<float*>(workspace);
    float* part_db = part + (size_t)nslab * N * K;
    dim3 grid((K + WS_C - 1) / WS_C, nslab);
    const int direct = nslab == 1 ? 1 : 0;
    if (P % 4 == 0 && mg_aligned16(X)) {
        MG_DYN_LDS(imgbank_wgrad_split_kernel<4>, WS_LDS);
        hipLaunchKernelGGL(imgbank_wgrad_split_kernel<4>, grid, dim3(WS_NT), WS_LDS, s, X, dbank, K, P, N, KK, kslab, direct, dW, db,
                           part, part_db);
    } else {
        MG_DYN_LDS(imgbank_wgrad_split_kernel<1>, WS_LDS);
        hipLaunchKernelGGL(imgbank_wgrad_split_kernel<1>, grid, dim3(WS_NT), WS_LDS, s, X, dbank, K, P, N, KK, kslab, direct, dW, db,
                           part, part_db);
    }
    MG_CHECK_LAUNCH("mgnns_imgbank_wgrad_split");
    if (nslab > 1) {
        hipLaunchKernelGGL(imgbank_wgrad_split_combine_kernel, dim3(bs_grid_for((long)N * K + N)), dim3(256), 0, s,
                           (const float*)part, (const float*)part_db, nslab, (long)N * K, N, dW, db);
        MG_CHECK_LAUNCH("mgnns_imgbank_wgrad_split(combine)");
    }
    return 0;
}

// the split, transposed weight: two images of DS_OC x Kp chunks
extern "C" size_t mgnns_imgbank_dgrad_split_workspace_bytes(int B, int K, int P, int N) {
    if (B <= 0 || K <= 0 || P <= 0 || N <= 0) return 64;
    const size_t Kp = ((size_t)K + DS_K - 1) / DS_K * DS_K;
    return (size_t)2 * DS_OC * Kp * 16 + 64;
}

extern "C" int mgnns_imgbank_dgrad_split(const float* dbank, const float* W, const float* dpooled, const int32_t* arg, int B,
                                         int K, int P, int N, float* dX, void* workspace, size_t workspace_bytes,
                                         mgnns_stream_t stream) {
    MG_REQUIRE(B >= 0 && K > 0 && P > 0 && N > 0 && N <= DS_OMAX, "mgnns_imgbank_dgrad_split: need B >= 0, K, P > 0, 0 < N <= %d "
               "(B=%d K=%d P=%d N=%d)", DS_OMAX, B, K, P, N);
    MG_REQUIRE((dpooled == nullptr) == (arg == nullptr), "mgnns_imgbank_dgrad_split: dpooled and arg come together");
    MG_REQUIRE(B == 0 || (dX && (dbank || dpooled) && (!dbank || W)), "mgnns_imgbank_dgrad_split: null pointer");
    MG_REQUIRE((long)B * K * P < (1L << 40), "mgnns_imgbank_dgrad_split: feature map too large");
    if (B == 0) return 0;
    if (!dbank) return mgnns_imgbank_dgrad(nullptr, W, dpooled, arg, B, K, P, N, dX, stream);   // no product: today's kernel
    MG_REQUIRE(workspace && mg_aligned16(workspace), "mgnns_imgbank_dgrad_split: the workspace must be a 16-byte aligned buffer");
    MG_REQUIRE(workspace_bytes >= mgnns_imgbank_dgrad_split_workspace_bytes(B, K, P, N),
               "mgnns_imgbank_dgrad_split: workspace too small");
    const int kblocks = (K + DS_K - 1) / DS_K, pblocks = (P + DS_P - 1) / DS_P;
    const int Kp = kblocks * DS_K;
    const long blocks = ((long)B + 7) / 8 * 8 * kblocks * pblocks;
    MG_REQUIRE(blocks < (1L << 31), "mgnns_imgbank_dgrad_split: too many blocks (B=%d K=%d P=%d)", B, K, P);
    hipStream_t s = (hipStream_t)stream;
    uint4* Wh = reinterpret_cast<uint4*>(workspace);
    uint4* Wl = Wh + (size_t)DS_OC * Kp;
    hipLaunchKernelGGL(imgbank_wsplit_kernel, dim3(bs_grid_for((long)DS_OC * Kp)), dim3(256), 0, s, W, N, K, Kp, Wh, Wl);
    MG_CHECK_LAUNCH("mgnns_imgbank_dgrad_split(weight)");
    if (N % 4 == 0 && mg_aligned16(dbank))
        hipLaunchKernelGGL(imgbank_dgrad_split_kernel<4>, dim3((unsigned)blocks), dim3(DS_NT), 0, s, dbank, (const uint4*)Wh,
                           (const uint4*)Wl, dpooled, (const int*)arg, B, K, P, N, Kp, kblocks, pblocks, dX);
    else
        hipLaunchKernelGGL(imgbank_dgrad_split_kernel<1>, dim3((unsigned)blocks), dim3(DS_NT), 0, s, dbank, (const uint4*)Wh,
                           (const uint4*)Wl, dpooled, (const int*)arg, B, K, P, N, Kp, kblocks, pblocks, dX);
    MG_CHECK_LAUNCH("mgnns_imgbank_dgrad_split");
    return 0;
}
