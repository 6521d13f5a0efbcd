// Training mode of the text encoders (fp32, wave64, no float atomics): the packed 2-layer BiLSTM of the text memory bank
// (MODEL:165-185, 366-398) and the text GCN (Text_GCN.py:142-275), each with a HIP backward.
//
// BiLSTM.  The training forward is the eval forward of lstm.hip (same packing, same input-projection GEMM, the same recurrence
// kernel: lstm_rec_kernel<true>) plus stores of what the backward needs: the post-activation gates [rows, 4H] and the cell state
// [rows, H] of every (layer, direction) in the packed sample-major row order (row = offs[b] + t), and layer 0's output.  Layer 1
// reads layer 0's output through the site-5 dropout mask (index (b*T + t)*2H + j).  The backward recurrence walks every chain in
// reverse: dh = dout_t + dh_rec, dc = dc_rec + dh o (1 - tanh^2 c), dz (pre-activation gates), dh_rec = W_hh^T dz, dc_rec = dc f.
// Its W_hh^T product uses the forward's register layout (lanes own gate rows, waves own hidden-unit slices) with the sum over
// the gate rows moved to the 64 lanes (DPP, a fixed order).  The weight and input gradients
// are GEMMs over the stored dz (python side: ops.wgrad, ops.matmul).
//
// Text GCN.  The training forward is the eval aggregation plus, for every (document node, feature), the source position of the
// winning in-edge (int16), and the pre-dropout sum.  Tie rule: among in-edges whose fp32 product equals the fp32 max, the one
// add_seq_edges builds first wins -- the smallest source position (a source's window edges come before its explicit self loop,
// which repeats its window edge to itself).  The backward re-derives the band, sends g w_e to the winner's node_hidden row and
// g h_u to its edge weight (summed per band slot over the features by DPP), as per-document partial rows that mgnns_keyed_row_sum adds up per key in a fixed order.
#include "common.hpp"
#include "dropout_hash.hpp"

int mg_launch_linear(const float* X, int M, int K, const float* W, const float* bias, int N, float* Y, int ldy,
                     const int32_t* gather_idx, const int32_t* m_dev, hipStream_t stream);
int mg_launch_lstm_rec_save(const float* Gx, const int32_t* offs, const int64_t* lens, int B, int T, const float* Whh_f,
                            const float* Whh_b, const float* bhh_f, const float* bhh_b, const int32_t* order, float* out,
                            float* gates, float* cells, int rows_cap, hipStream_t s);
int mg_lstm_pack(const int64_t* tok, const int64_t* lens, int B, int T, int V, int32_t* offs, int32_t* order, int32_t* pack_tok,
                 int32_t* pack_pos, hipStream_t s);

namespace {

constexpr int HID = 150;
constexpr int G4 = 4 * HID;
constexpr int TG_THREADS = 320;      // text GCN: one thread per feature (D <= 320)

unsigned grid_of(long n) {
    long g = (n + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > 65535 * 8 ? 65535 * 8 : g));
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float tanhf_(float x) { return 2.0f / (1.0f + expf(-2.0f * x)) - 1.0f; }

// y = x * keep / (1 - rate) at `site`, flat index i (the BiLSTM inter-layer dropout forward, and its backward on the gradient)
__global__ void drop_apply_kernel(const float* __restrict__ x, long n, uint64_t seed, int site, float rate, float* __restrict__ y) {
    const float sc = keep_scale(rate);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        y[i] = mg_keep(seed, site, (uint64_t)i, rate) ? x[i] * sc : 0.f;
}

// Backward recurrence of one layer: one workgroup per (sample, direction), longest chain first.  dout [B, T, 2H] (this layer's
// output gradient); gates / cells: this layer's saved [2][rows_cap][4H] / [2][rows_cap][H]; dz [rows, 2 * 4H] (row = offs[b] + t,
// columns dir * 4H + gate row).  Positions at or past len are never read.
// dh_rec = W_hh^T dz in the forward's register layout: wave w owns the hidden units k in [10 w, 10 w + 10), lane l the gate rows
// l + 64 i (100 weights in registers); each lane's 10 partials are summed over the 64 lanes by DPP + readlane (a fixed order,
// wave-uniform result).  (The row-slice layout -- 50 rows x 3 hidden units per lane in 12 waves -- needs 150 weight registers
// and spilled 95.)
constexpr int BT_THREADS = 1024;
constexpr int BT_KW = 10;            // hidden units per wave (16 x 10 = 160 >= 150)
constexpr int BT_RPL = 10;           // gate rows per lane (640 >= 600)
__global__ __launch_bounds__(BT_THREADS) void lstm_bwd_rec_kernel(const float* __restrict__ dout, const float* __restrict__ gates,
                                                                  const float* __restrict__ cells, const int32_t* __restrict__ offs,
                                                                  const int64_t* __restrict__ lens, int T,
                                                                  const float* __restrict__ Whh_f, const float* __restrict__ Whh_b,
                                                                  const int32_t* __restrict__ order, float* __restrict__ dz,
                                                                  int rows_cap) {
    __shared__ float s_dz[BT_RPL * 64];
    __shared__ float s_dh[16 * BT_KW];
    const int b = order[blockIdx.x >> 1], dir = blockIdx.x & 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long l = lens[b];
    const int len = (int)(l < 0 ? 0 : (l > T ? T : l));
    const int off = offs[b];
    if (off + len > rows_cap) return;                                  // (a row count the caller did not size for: uniform)
    const float* Whh = dir ? Whh_b : Whh_f;
    const float* gsave = gates + (size_t)dir * rows_cap * G4;
    const float* csave = cells + (size_t)dir * rows_cap * HID;

    float w[BT_RPL][BT_KW];
#pragma unroll
    for (int i = 0; i < BT_RPL; ++i) {
        const int row = lane + 64 * i;
#pragma unroll
        for (int kk = 0; kk < BT_KW; ++kk) {
            const int k = wave * BT_KW + kk;
            w[i][kk] = (row < G4 && k < HID) ? Whh[(size_t)row * HID + k] : 0.f;
        }
    }
    if (tid < BT_RPL * 64) s_dz[tid] = 0.f;                            // rows 600..639 stay zero
    const bool cell = tid < HID;
    float dh_rec = 0.f, dc_rec = 0.f;
    float ig = 0.f, fg = 0.f, gg = 0.f, og = 0.f, c = 0.f, cp = 0.f, dy = 0.f;
    auto load = [&](int s) {                                           // step s's gates, c of step s - 1, dout (prefetched one step ahead)
        const int t = dir ? len - 1 - s : s;
        const size_t row = (size_t)(off + t);
        ig = gsave[row * G4 + tid];
        fg = gsave[row * G4 + HID + tid];
        gg = gsave[row * G4 + 2 * HID + tid];
        og = gsave[row * G4 + 3 * HID + tid];
        cp = s > 0 ? csave[(size_t)(off + (dir ? t + 1 : t - 1)) * HID + tid] : 0.f;
        dy = dout[((size_t)b * T + t) * (2 * HID) + dir * HID + tid];
    };
    if (cell && len > 0) {
        load(len - 1);
        c = csave[(size_t)(off + (dir ? 0 : len - 1)) * HID + tid];
    }
    __syncthreads();
    for (int s = len - 1; s >= 0; --s) {
        if (cell) {
            const int t = dir ? len - 1 - s : s;
            const float dh = dy + dh_rec;
            const float tc = tanhf_(c);
            const float dc = dc_rec + dh * og * (1.f - tc * tc);
            const float zi = dc * gg * ig * (1.f - ig);
            const float zf = dc * cp * fg * (1.f - fg);
            const float zg = dc * ig * (1.f - gg * gg);
            const float zo = dh * tc * og * (1.f - og);
            dc_rec = dc * fg;
            s_dz[tid] = zi;
            s_dz[HID + tid] = zf;
            s_dz[2 * HID + tid] = zg;
            s_dz[3 * HID + tid] = zo;
            float* dzr = dz + (size_t)(off + t) * (2 * G4) + dir * G4;
            dzr[tid] = zi;
            dzr[HID + tid] = zf;
            dzr[2 * HID + tid] = zg;
            dzr[3 * HID + tid] = zo;
            c = cp;                                                    // the cell state of step s - 1
            if (s > 0) load(s - 1);
        }
        mg_lds_barrier();
        // two halves of the hidden units (5 partials live at a time: the whole product in one pass spilled 14 registers)
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
            float p[BT_KW / 2];
#pragma unroll
            for (int kk = 0; kk < BT_KW / 2; ++kk) p[kk] = 0.f;
#pragma unroll
            for (int i = 0; i < BT_RPL; ++i) {
                const float d = s_dz[lane + 64 * i];
#pragma unroll
                for (int kk = 0; kk < BT_KW / 2; ++kk) p[kk] = fmaf(w[i][h2 * (BT_KW / 2) + kk], d, p[kk]);
            }
#pragma unroll
            for (int kk = 0; kk < BT_KW / 2; ++kk) {
                const float v = wave_sum_dpp(p[kk]);
                if (lane == 0) s_dh[wave * BT_KW + h2 * (BT_KW / 2) + kk] = v;
            }
        }
        mg_lds_barrier();
        if (cell) dh_rec = s_dh[tid];
    }
}

// hprev [rows, 2H]: the recurrent input of every packed step (forward: h at t-1, reverse: h at t+1; 0 at a chain's first step)
__global__ __launch_bounds__(256) void lstm_hprev_kernel(const float* __restrict__ hout, const int32_t* __restrict__ offs,
                                                         const int64_t* __restrict__ lens, int T, float* __restrict__ hprev,
                                                         int rows_cap) {
    const int b = blockIdx.x;
    long long l = lens[b];
    const int len = (int)(l < 0 ? 0 : (l > T ? T : l));
    const int off = offs[b];
    if (off + len > rows_cap) return;
    for (int e = threadIdx.x; e < len * 2 * HID; e += blockDim.x) {
        const int t = e / (2 * HID), j = e - t * 2 * HID;
        const int src = j < HID ? t - 1 : t + 1;
        hprev[(size_t)(off + t) * 2 * HID + j] = (src >= 0 && src < len) ? hout[((size_t)b * T + src) * 2 * HID + j] : 0.f;
    }
}

// dst[r, :] = src[idx[r], :] for r < M
__global__ void gather_rows_kernel(const float* __restrict__ src, int n_src, int K, const int32_t* __restrict__ idx, long M,
                                   float* __restrict__ dst) {
    const long n = M * K;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
        const long r = e / K;
        const int k = (int)(e - r * K);
        const int i = idx[r];
        dst[e] = (i >= 0 && i < n_src) ? src[(size_t)i * K + k] : 0.f;
    }
}

// dout[pos[r], j] = dx[r, j] * keep(site 5, pos[r] * 2H + j) / (1 - rate): layer 1's input gradient back through the dropout
// into layer 0's output gradient (positions not listed stay as the caller zeroed them)
__global__ void lstm_unpack_drop_kernel(const float* __restrict__ dx, const int32_t* __restrict__ pos, long M, long n_pos,
                                        uint64_t seed, float rate, float* __restrict__ dout) {
    const float sc = keep_scale(rate);
    const long n = M * 2 * HID;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
        const long r = e / (2 * HID);
        const int j = (int)(e - r * 2 * HID);
        const long p = pos[r];
        if (p < 0 || p >= n_pos) continue;
        const uint64_t fi = (uint64_t)p * 2 * HID + j;
        dout[fi] = mg_keep(seed, MGNNS_DROP_LSTM, fi, rate) ? dx[e] * sc : 0.f;
    }
}

// out[key, :] = sum of values[perm[r], :] over the run of equal sorted keys, in sorted (stable) order; keys < skip_below
// contribute nothing.  One workgroup per sorted position; only a run's first position works.  D >= 64: a thread per column,
// rows in order, eight loads in flight.  D < 64 (the edge weights, where the "no PMI entry" id holds most band slots: runs of
// ~10^5 rows): the 256 threads take rows r0 + tid, r0 + tid + 256, .. (eight loads in flight), and thread 0 adds the 256 partials
// in order -- a fixed partition, so a fixed order.
constexpr int KS_THREADS = 256;
__global__ __launch_bounds__(KS_THREADS) void keyed_row_sum_kernel(const int64_t* __restrict__ skeys, const int64_t* __restrict__ perm,
                                                                   long M, const float* __restrict__ vals, int D, long n_vals,
                                                                   long skip_below, float* __restrict__ out, long K) {
    __shared__ float s_p[KS_THREADS];
    auto val = [&](long r, int d) {
        const long src = perm[r];
        return (src >= 0 && src < n_vals) ? vals[(size_t)src * D + d] : 0.f;
    };
    for (long r0 = blockIdx.x; r0 < M; r0 += gridDim.x) {
        const long key = skeys[r0];
        if (key < skip_below || key >= K || (r0 > 0 && skeys[r0 - 1] == key)) continue;
        long lo = r0 + 1, hi = M;                                      // end of the run: binary search (keys sorted)
        while (lo < hi) {
            const long mid = (lo + hi) >> 1;
            if (skeys[mid] == key) lo = mid + 1; else hi = mid;
        }
        const long r1 = lo;
        if (D >= 64) {
            for (int d = threadIdx.x; d < D; d += KS_THREADS) {
                float acc = 0.f;
                long r = r0;
                for (; r + 8 <= r1; r += 8) {
                    float v[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) v[u] = val(r + u, d);
#pragma unroll
                    for (int u = 0; u < 8; ++u) acc += v[u];
                }
                for (; r < r1; ++r) acc += val(r, d);
                out[(size_t)key * D + d] = acc;
            }
        } else {
            for (int d = 0; d < D; ++d) {
                float acc = 0.f;
                long r = r0 + threadIdx.x;
                for (; r + 7 * KS_THREADS < r1; r += 8 * KS_THREADS) {
                    float v[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) v[u] = val(r + (long)u * KS_THREADS, d);
#pragma unroll
                    for (int u = 0; u < 8; ++u) acc += v[u];
                }
                for (; r < r1; r += KS_THREADS) acc += val(r, d);
                s_p[threadIdx.x] = acc;
                __syncthreads();
                if (threadIdx.x == 0) {
                    float t = 0.f;
                    for (int i = 0; i < KS_THREADS; ++i) t += s_p[i];
                    out[(size_t)key * D + d] = t;
                }
                __syncthreads();
            }
        }
    }
}

// ---- text GCN ---------------------------------------------------------------------------------------------------------------
// edge id of (u -> v) in the PMI CSR (0 = no entry), the eval kernel's lookup (textgcn.hip pmi_weight) without the weight
__device__ int pmi_edge_id(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col, const int32_t* __restrict__ eid,
                           int n_edge_w, int u, int v) {
    int lo = row_ptr[u], hi = row_ptr[u + 1];
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (col[mid] < v) lo = mid + 1; else hi = mid;
    }
    int id = (lo < row_ptr[u + 1] && col[lo] == v) ? (eid ? eid[lo] : lo + 1) : 0;
    return (id < 0 || id >= n_edge_w) ? 0 : id;
}

// Shared per-document set-up of both text GCN kernels: compacted tokens, band of edge ids / weights, same-token chains.
struct TgDoc {
    int* tok;     // [Tm]
    int* next;    // [Tm] next position with the same token (INT_MAX: none)
    int* head;    // [Tm] first position with the same token
    int* eid;     // [Tm * W]
    float* w;     // [Tm * W]
    float* h;     // [Tm * D] staged node rows (or nullptr: read from the table)
};

__device__ int tg_setup(const int64_t* __restrict__ tok, int T, int Tm, int V, const float* __restrict__ node_hidden, int D,
                        const float* __restrict__ edge_w, int n_edge_w, const int32_t* __restrict__ rp,
                        const int32_t* __restrict__ col, const int32_t* __restrict__ eid, int g, const TgDoc& s, int* s_n) {
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int W = 2 * g + 1;
    if (tid < 64) {
        int n = 0;
        for (int p0 = 0; p0 < Tm; p0 += 64) {
            const int p = p0 + lane;
            long long id = p < Tm ? tok[(size_t)b * T + p] : 0;
            id = id < 0 ? 0 : (id >= V ? V - 1 : id);
            const bool nz = id != 0;
            const unsigned long long m = __ballot(nz);
            if (nz) s.tok[n + __popcll(m & ((1ull << lane) - 1ull))] = (int)id;
            n += __popcll(m);
        }
        if (lane == 0) *s_n = n;
    }
    __syncthreads();
    const int n = *s_n;
    for (int e = tid; e < n * W; e += blockDim.x) {
        const int j = e / W, o = e - j * W;
        const int i = j - g + o;
        int id = 0;
        if (i >= 0 && i < n) id = pmi_edge_id(rp, col, eid, n_edge_w, s.tok[i], s.tok[j]);
        s.eid[e] = (i >= 0 && i < n) ? id : -1;
        s.w[e] = (i >= 0 && i < n) ? edge_w[id] : 0.f;
    }
    for (int j = tid; j < n; j += blockDim.x) {
        const int v = s.tok[j];
        int nx = 0x7fffffff, hd = j;
        for (int k = n - 1; k > j; --k)
            if (s.tok[k] == v) nx = k;
        for (int k = j - 1; k >= 0; --k)
            if (s.tok[k] == v) hd = k;
        s.next[j] = nx;
        s.head[j] = hd;
    }
    if (s.h)
        for (int e = tid; e < n * D; e += blockDim.x) {
            const int i = e / D, d = e - i * D;
            s.h[e] = node_hidden[(size_t)s.tok[i] * D + d];
        }
    __syncthreads();
    return n;
}

// Training forward, one workgroup per document, a thread per feature d: h'_v[d] = max over in-edges, the winner's source
// position into win[b, first position of v, d] (other rows untouched), sum over nodes in first-occurrence order -> presum,
// out = relu(dropout_site6(presum)).
__global__ __launch_bounds__(TG_THREADS) void tg_train_fwd_kernel(const int64_t* __restrict__ tok, int T, int Tm,
                                                                  const float* __restrict__ node_hidden, int V, int D,
                                                                  const float* __restrict__ edge_w, int n_edge_w,
                                                                  const int32_t* __restrict__ rp, const int32_t* __restrict__ col,
                                                                  const int32_t* __restrict__ eid, int g, int stage, uint64_t seed,
                                                                  float rate, float* __restrict__ out, float* __restrict__ presum,
                                                                  int16_t* __restrict__ win) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int W = 2 * g + 1;
    TgDoc s;
    s.h = stage ? smem : nullptr;
    s.w = smem + (stage ? (size_t)Tm * D : 0);
    s.eid = reinterpret_cast<int*>(s.w + (size_t)Tm * W);
    s.tok = s.eid + (size_t)Tm * W;
    s.next = s.tok + Tm;
    s.head = s.next + Tm;
    int* s_n = s.head + Tm;
    const int n = tg_setup(tok, T, Tm, V, node_hidden, D, edge_w, n_edge_w, rp, col, eid, g, s, s_n);
    const int b = blockIdx.x, d = threadIdx.x;
    if (d >= D) return;
    float sum = 0.f;
    for (int j0 = 0; j0 < n; ++j0) {
        if (s.head[j0] != j0) continue;
        float mx = -INFINITY;
        int bi = 0x7fffffff;
        for (int j = j0; j < n; j = s.next[j]) {
            const int lo = max(0, j - g), hi = min(n, j + g + 1);
            for (int i = lo; i < hi; ++i) {
                const float h = s.h ? s.h[(size_t)i * D + d] : node_hidden[(size_t)s.tok[i] * D + d];
                const float p = s.w[(size_t)j * W + (i - (j - g))] * h;
                if (p > mx || (p == mx && i < bi)) { mx = p; bi = i; }
            }
        }
        sum += mx;
        win[((size_t)b * Tm + j0) * D + d] = (int16_t)bi;
    }
    presum[(size_t)b * D + d] = sum;
    const float y = mg_keep(seed, MGNNS_DROP_TEXT_GCN, (uint64_t)b * D + d, rate) ? sum * keep_scale(rate) : 0.f;
    out[(size_t)b * D + d] = fmaxf(y, 0.f);
}

// Backward, one workgroup per document.  g = dy [y > 0] keep / (1 - rate).  Nodes in first-occurrence order, the whole workgroup
// in step (the loop bounds live in LDS): per feature d, the winner i (source token u) of node v; its edge is taken at the first
// occurrence jj of v within i's window (every edge u -> v has the same id): R[b, i, d] += g w_e (the node_hidden row of u), and
// c = g h_u[d] goes to band slot (jj, i - jj + g).  Every slot of the node's occurrences takes the sum of its c over the wave's
// 64 features (DPP + readlane, a fixed order) into LDS; after the loop one thread per slot adds the wave sums in wave order ->
// Eg[b, jj, o].  Keys: keyR[b, i] = u (i < n, else -1), keyE[b, jj, o] = edge id (a real edge, else -1).
constexpr int TG_WAVES = TG_THREADS / 64;
__global__ __launch_bounds__(TG_THREADS) void tg_train_bwd_kernel(const int64_t* __restrict__ tok, int T, int Tm,
                                                                  const float* __restrict__ node_hidden, int V, int D,
                                                                  const float* __restrict__ edge_w, int n_edge_w,
                                                                  const int32_t* __restrict__ rp, const int32_t* __restrict__ col,
                                                                  const int32_t* __restrict__ eid, int g, int stage, uint64_t seed,
                                                                  float rate, const float* __restrict__ dy,
                                                                  const float* __restrict__ presum, const int16_t* __restrict__ win,
                                                                  float* __restrict__ R, int32_t* __restrict__ keyR,
                                                                  float* __restrict__ Eg, int32_t* __restrict__ keyE) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int W = 2 * g + 1;
    TgDoc s;
    s.h = stage ? smem : nullptr;
    s.w = smem + (stage ? (size_t)Tm * D : 0);
    s.eid = reinterpret_cast<int*>(s.w + (size_t)Tm * W);
    s.tok = s.eid + (size_t)Tm * W;
    s.next = s.tok + Tm;
    s.head = s.next + Tm;
    int* s_n = s.head + Tm;
    float* s_wp = reinterpret_cast<float*>(s_n + 4);                  // [TG_WAVES][Tm * W] per-wave slot sums
    const int n = tg_setup(tok, T, Tm, V, node_hidden, D, edge_w, n_edge_w, rp, col, eid, g, s, s_n);
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool live = tid < D;
    const int d = tid;
    float gd = 0.f;
    float* Rb = R + (size_t)b * Tm * D;
    if (live) {
        const float sum = presum[(size_t)b * D + d];
        const bool kp = mg_keep(seed, MGNNS_DROP_TEXT_GCN, (uint64_t)b * D + d, rate);
        const float sc = keep_scale(rate);
        const float y = kp ? sum * sc : 0.f;
        gd = (kp && y > 0.f) ? dy[(size_t)b * D + d] * sc : 0.f;
        for (int i = 0; i < n; ++i) Rb[(size_t)i * D + d] = 0.f;
    }
    float* wp = s_wp + (size_t)wave * Tm * W;
    for (int j0 = 0; j0 < n; ++j0) {
        if (s.head[j0] != j0) continue;                               // (uniform: LDS)
        int sl = -1;
        float cv = 0.f;
        if (live) {
            const int v = s.tok[j0];
            int i = win[((size_t)b * Tm + j0) * D + d];
            i = i < 0 ? 0 : (i >= n ? n - 1 : i);
            int jj = j0;
            for (int k = min(n - 1, i + g); k >= max(0, i - g); --k)
                if (s.tok[k] == v) jj = k;
            const int o = i - jj + g;
            sl = (o >= 0 && o < W) ? jj * W + o : -1;
            const float we = sl >= 0 ? s.w[sl] : 0.f;
            Rb[(size_t)i * D + d] += gd * we;
            const float h = s.h ? s.h[(size_t)i * D + d] : node_hidden[(size_t)s.tok[i] * D + d];
            cv = gd * h;
        }
        for (int jj = j0; jj < n; jj = s.next[jj])                   // the node's occurrences (uniform)
            for (int o = 0; o < W; ++o) {
                const float v = wave_sum_dpp(sl == jj * W + o ? cv : 0.f);
                if (lane == 0) wp[jj * W + o] = v;
            }
    }
    __syncthreads();
    for (int i = tid; i < Tm; i += blockDim.x) keyR[(size_t)b * Tm + i] = i < n ? s.tok[i] : -1;
    for (int sl = tid; sl < Tm * W; sl += blockDim.x) {
        const int jj = sl / W;
        float acc = 0.f;
        int key = -1;
        if (jj < n && s.eid[sl] >= 0) {
            for (int w = 0; w < TG_WAVES; ++w) acc += s_wp[(size_t)w * Tm * W + sl];
            key = s.eid[sl];
        }
        Eg[(size_t)b * Tm * W + sl] = acc;
        keyE[(size_t)b * Tm * W + sl] = key;
    }
}

size_t tg_lds(int Tm, int W, int D, bool stage, bool parts) {
    return (stage ? (size_t)Tm * D * sizeof(float) : 0) + (size_t)Tm * W * (sizeof(float) + sizeof(int)) + (3 * (size_t)Tm + 4) * sizeof(int) +
           (parts ? (size_t)TG_WAVES * Tm * W * sizeof(float) : 0);
}

}  // namespace

// ---- BiLSTM ------------------------------------------------------------------------------------------------------------------
extern "C" size_t mgnns_bilstm_train_workspace_bytes(int B, int T, int hidden) {
    return (((size_t)(B > 0 ? B : 0) * (T > 0 ? T : 0) * 8 * (size_t)(hidden > 0 ? hidden : 0) * sizeof(float)) + 255) & ~(size_t)255;
}

extern "C" int mgnns_bilstm_train_fwd(const int64_t* tok, const int64_t* lens, int B, int T, const float* emb_table, int V,
                                      int emb_dim, int hidden, int num_layers, const float* const* w_ih_cat,
                                      const float* const* b_ih_cat, const float* const* w_hh, const float* const* b_hh,
                                      uint64_t seed, float rate, int32_t* meta, int rows_cap, float* gates, float* cells,
                                      float* mid, float* mid_drop, float* out, void* workspace, size_t workspace_bytes,
                                      mgnns_stream_t stream) {
    MG_REQUIRE(tok && lens && emb_table && w_ih_cat && b_ih_cat && w_hh && b_hh && meta && gates && cells && out && workspace,
               "mgnns_bilstm_train_fwd: null pointer");
    MG_REQUIRE(hidden == HID, "mgnns_bilstm_train_fwd: hidden_size=%d unsupported (150 only)", hidden);
    MG_REQUIRE(num_layers >= 1 && num_layers <= 2, "mgnns_bilstm_train_fwd: num_layers=%d unsupported (1..2)", num_layers);
    MG_REQUIRE(B > 0 && T > 0 && V > 0 && emb_dim > 0 && rows_cap > 0, "mgnns_bilstm_train_fwd: bad dims B=%d T=%d V=%d E=%d rows=%d",
               B, T, V, emb_dim, rows_cap);
    MG_REQUIRE(num_layers == 1 || (mid && mid_drop), "mgnns_bilstm_train_fwd: null layer-0 output");
    MG_REQUIRE(rate >= 0.f && rate <= 1.f, "mgnns_bilstm_train_fwd: dropout rate %g outside [0, 1]", (double)rate);
    MG_REQUIRE(workspace_bytes >= mgnns_bilstm_train_workspace_bytes(B, T, hidden), "mgnns_bilstm_train_fwd: workspace too small");
    for (int i = 0; i < 2 * num_layers; ++i) MG_REQUIRE(w_hh[i] && b_hh[i], "mgnns_bilstm_train_fwd: null weight pointer %d", i);
    for (int i = 0; i < num_layers; ++i) MG_REQUIRE(w_ih_cat[i] && b_ih_cat[i], "mgnns_bilstm_train_fwd: null weight pointer %d", i);
    hipStream_t s = (hipStream_t)stream;
    const size_t rows = (size_t)B * T;
    int32_t* offs = meta;
    int32_t* order = offs + B + 1;
    int32_t* pack_tok = order + B + 8;
    int32_t* pack_pos = pack_tok + rows;
    float* Gx = reinterpret_cast<float*>(workspace);
    if (int rc = mg_lstm_pack(tok, lens, B, T, V, offs, order, pack_tok, pack_pos, s)) return rc;
    for (int layer = 0; layer < num_layers; ++layer) {
        const float* X = layer == 0 ? emb_table : mid_drop;
        const int K = layer == 0 ? emb_dim : 2 * HID;
        const int32_t* gidx = layer == 0 ? pack_tok : pack_pos;
        float* dst = (layer == num_layers - 1) ? out : mid;
        if (int rc = mg_launch_linear(X, (int)rows, K, w_ih_cat[layer], b_ih_cat[layer], 2 * G4, Gx, 2 * G4, gidx, offs + B, s)) return rc;
        if (int rc = mg_launch_lstm_rec_save(Gx, offs, lens, B, T, w_hh[2 * layer], w_hh[2 * layer + 1], b_hh[2 * layer], b_hh[2 * layer + 1],
                                             order, dst, gates + (size_t)2 * layer * rows_cap * G4,
                                             cells + (size_t)2 * layer * rows_cap * HID, rows_cap, s)) return rc;
        if (layer + 1 < num_layers)
            hipLaunchKernelGGL(drop_apply_kernel, dim3(grid_of((long)rows * 2 * HID)), dim3(256), 0, s, (const float*)mid,
                               (long)rows * 2 * HID, seed, (int)MGNNS_DROP_LSTM, rate, mid_drop);
    }
    MG_CHECK_LAUNCH("mgnns_bilstm_train_fwd");
    return 0;
}

extern "C" int mgnns_bilstm_train_bwd_rec(const float* dout, const int64_t* lens, int B, int T, const int32_t* meta, int rows_cap,
                                          const float* gates, const float* cells, const float* w_hh_f, const float* w_hh_r,
                                          float* dz, mgnns_stream_t stream) {
    MG_REQUIRE(dout && lens && meta && gates && cells && w_hh_f && w_hh_r && dz, "mgnns_bilstm_train_bwd_rec: null pointer");
    MG_REQUIRE(B > 0 && T > 0 && rows_cap > 0, "mgnns_bilstm_train_bwd_rec: bad dims B=%d T=%d rows=%d", B, T, rows_cap);
    const int32_t* offs = meta;
    const int32_t* order = offs + B + 1;
    hipLaunchKernelGGL(lstm_bwd_rec_kernel, dim3(2 * B), dim3(BT_THREADS), 0, (hipStream_t)stream, dout, gates, cells, offs, lens, T,
                       w_hh_f, w_hh_r, order, dz, rows_cap);
    MG_CHECK_LAUNCH("mgnns_bilstm_train_bwd_rec");
    return 0;
}

extern "C" int mgnns_bilstm_train_hprev(const float* hout, const int64_t* lens, int B, int T, const int32_t* meta, int rows_cap,
                                        float* hprev, mgnns_stream_t stream) {
    MG_REQUIRE(hout && lens && meta && hprev, "mgnns_bilstm_train_hprev: null pointer");
    MG_REQUIRE(B > 0 && T > 0 && rows_cap > 0, "mgnns_bilstm_train_hprev: bad dims B=%d T=%d rows=%d", B, T, rows_cap);
    hipLaunchKernelGGL(lstm_hprev_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, hout, meta, lens, T, hprev, rows_cap);
    MG_CHECK_LAUNCH("mgnns_bilstm_train_hprev");
    return 0;
}

extern "C" int mgnns_bilstm_train_unpack_drop(const float* dx, const int32_t* pack_pos, int64_t M, int B, int T, uint64_t seed,
                                              float rate, float* dout, mgnns_stream_t stream) {
    MG_REQUIRE(rate >= 0.f && rate <= 1.f, "mgnns_bilstm_train_unpack_drop: dropout rate %g outside [0, 1]", (double)rate);
    if (M <= 0) return 0;
    MG_REQUIRE(dx && pack_pos && dout, "mgnns_bilstm_train_unpack_drop: null pointer");
    hipLaunchKernelGGL(lstm_unpack_drop_kernel, dim3(grid_of((long)M * 2 * HID)), dim3(256), 0, (hipStream_t)stream, dx, pack_pos,
                       (long)M, (long)B * T, seed, rate, dout);
    MG_CHECK_LAUNCH("mgnns_bilstm_train_unpack_drop");
    return 0;
}

extern "C" int mgnns_gather_rows(const float* src, int n_src, int K, const int32_t* idx, int64_t M, float* dst, mgnns_stream_t stream) {
    if (M <= 0) return 0;
    MG_REQUIRE(src && idx && dst && K > 0 && n_src > 0, "mgnns_gather_rows: bad arguments");
    hipLaunchKernelGGL(gather_rows_kernel, dim3(grid_of((long)M * K)), dim3(256), 0, (hipStream_t)stream, src, n_src, K, idx, (long)M, dst);
    MG_CHECK_LAUNCH("mgnns_gather_rows");
    return 0;
}

extern "C" int mgnns_keyed_row_sum(const int64_t* sorted_keys, const int64_t* perm, int64_t M, const float* values, int D,
                                   int64_t n_values, int64_t skip_below, float* out, int64_t K, mgnns_stream_t stream) {
    if (M <= 0) return 0;
    MG_REQUIRE(sorted_keys && perm && values && out && D > 0 && K > 0, "mgnns_keyed_row_sum: bad arguments");
    const long grid = M < 65536 * 4 ? (long)M : 65536 * 4;
    hipLaunchKernelGGL(keyed_row_sum_kernel, dim3((unsigned)grid), dim3(KS_THREADS), 0, (hipStream_t)stream, sorted_keys, perm, (long)M, values,
                       D, (long)n_values, (long)skip_below, out, (long)K);
    MG_CHECK_LAUNCH("mgnns_keyed_row_sum");
    return 0;
}

// ---- text GCN ----------------------------------------------------------------------------------------------------------------
static int tg_check(const char* who, int B, int T, int V, int D, int n_edge_w, int ngram, int max_length, bool parts, int* Tm,
                    size_t* lds, int* stage) {
    MG_REQUIRE(B > 0 && T > 0 && V > 0 && n_edge_w > 0, "%s: bad dims B=%d T=%d V=%d", who, B, T, V);
    MG_REQUIRE(D > 0 && D <= TG_THREADS, "%s: D=%d unsupported (1..%d)", who, D, TG_THREADS);
    MG_REQUIRE(ngram >= 0 && ngram <= 15, "%s: ngram=%d unsupported (0..15)", who, ngram);
    MG_REQUIRE(max_length > 0, "%s: max_length=%d", who, max_length);
    *Tm = T < max_length ? T : max_length;
    const int W = 2 * ngram + 1;
    MG_REQUIRE((long)*Tm * W < 32768, "%s: min(T, max_length) x (2 ngram + 1) = %d does not fit the int16 winners", who, *Tm * W);
    *stage = tg_lds(*Tm, W, D, true, parts) <= 160 * 1024;
    *lds = tg_lds(*Tm, W, D, *stage != 0, parts);
    MG_REQUIRE(*lds <= 160 * 1024, "%s: min(T, max_length)=%d needs %zu B of LDS", who, *Tm, *lds);
    return 0;
}

// The shape limits of a text GCN training STEP as a predicate: the backward's (its per-wave slot sums make it the stricter of the two
// kernels), so a shape the forward takes is one the backward takes too.
extern "C" int mgnns_textgcn_train_supported(int T, int D, int ngram, int max_length) {
    if (!(T > 0 && D > 0 && D <= TG_THREADS && ngram >= 0 && ngram <= 15 && max_length > 0)) return 0;
    const int Tm = T < max_length ? T : max_length;
    const int W = 2 * ngram + 1;
    if ((long)Tm * W >= 32768) return 0;
    return tg_lds(Tm, W, D, false, true) <= 160 * 1024 ? 1 : 0;
}

extern "C" int mgnns_textgcn_train_fwd(const int64_t* tok, int B, int T, const float* node_hidden, int V, int D, const float* edge_w,
                                       int n_edge_w, const int32_t* pmi_row_ptr, const int32_t* pmi_col, const int32_t* pmi_eid,
                                       int ngram, int max_length, uint64_t seed, float rate, float* out, float* presum,
                                       int16_t* win, mgnns_stream_t stream) {
    MG_REQUIRE(rate >= 0.f && rate <= 1.f, "mgnns_textgcn_train_fwd: dropout rate %g outside [0, 1]", (double)rate);
    int Tm, stage;
    size_t lds;
    // (the shape first: at max_length = 0 the winners are an empty buffer, and the message should name max_length, not a pointer)
    if (int rc = tg_check("mgnns_textgcn_train_fwd", B, T, V, D, n_edge_w, ngram, max_length, false, &Tm, &lds, &stage)) return rc;
    MG_REQUIRE(tok && node_hidden && edge_w && pmi_row_ptr && pmi_col && out && presum && win, "mgnns_textgcn_train_fwd: null pointer");
    // a step this forward begins must be one the backward can finish: refuse here, before anything is launched
    MG_REQUIRE(mgnns_textgcn_train_supported(T, D, ngram, max_length),
               "mgnns_textgcn_train_fwd: min(T, max_length)=%d: the backward needs %zu B of LDS (> 160 KiB)", Tm,
               tg_lds(Tm, 2 * ngram + 1, D, false, true));
    MG_DYN_LDS(tg_train_fwd_kernel, 160 * 1024);
    hipLaunchKernelGGL(tg_train_fwd_kernel, dim3(B), dim3(TG_THREADS), lds, (hipStream_t)stream, tok, T, Tm, node_hidden, V, D, edge_w,
                       n_edge_w, pmi_row_ptr, pmi_col, pmi_eid, ngram, stage, seed, rate, out, presum, win);
    MG_CHECK_LAUNCH("mgnns_textgcn_train_fwd");
    return 0;
}

extern "C" int mgnns_textgcn_train_bwd(const int64_t* tok, int B, int T, const float* node_hidden, int V, int D, const float* edge_w,
                                       int n_edge_w, const int32_t* pmi_row_ptr, const int32_t* pmi_col, const int32_t* pmi_eid,
                                       int ngram, int max_length, uint64_t seed, float rate, const float* dy, const float* presum,
                                       const int16_t* win, float* R, int32_t* keyR, float* Eg, int32_t* keyE, mgnns_stream_t stream) {
    MG_REQUIRE(tok && node_hidden && edge_w && pmi_row_ptr && pmi_col && dy && presum && win && R && keyR && Eg && keyE,
               "mgnns_textgcn_train_bwd: null pointer");
    MG_REQUIRE(rate >= 0.f && rate <= 1.f, "mgnns_textgcn_train_bwd: dropout rate %g outside [0, 1]", (double)rate);
    int Tm, stage;
    size_t lds;
    if (int rc = tg_check("mgnns_textgcn_train_bwd", B, T, V, D, n_edge_w, ngram, max_length, true, &Tm, &lds, &stage)) return rc;
    MG_DYN_LDS(tg_train_bwd_kernel, 160 * 1024);
    hipLaunchKernelGGL(tg_train_bwd_kernel, dim3(B), dim3(TG_THREADS), lds, (hipStream_t)stream, tok, T, Tm, node_hidden, V, D, edge_w,
                       n_edge_w, pmi_row_ptr, pmi_col, pmi_eid, ngram, stage, seed, rate, dy, presum, win, R, keyR, Eg, keyE);
    MG_CHECK_LAUNCH("mgnns_textgcn_train_bwd");
    return 0;
}
