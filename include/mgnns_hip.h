/*
 * mgnns_hip.h -- C ABI of libmgnns_hip.so: the MI355X (gfx950) forward hot path of MGNNS.
 *
 * The reference has no native code and no FFI: its operators are Python nn.Modules that
 * dispatch to cuDNN/cuBLAS/DGL kernels.  Each entry point below replaces the device work
 * behind one reference call site (cited as file:line into the reference tree) and is what
 * a ctypes binding of that call site would bind.  See INTEGRATION.md for the Python stubs.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (row-major, contiguous);
 *     the library never allocates, frees or synchronises; workspaces are passed in;
 *   - `stream` is a hipStream_t (as void*); all work is enqueued on it, no hidden syncs;
 *   - return value 0 = enqueued, negative = rejected (mgnns_last_error() has the text);
 *   - fp32 everywhere unless an argument says otherwise; int64 token ids as PyTorch makes them.
 */
#ifndef MGNNS_HIP_H
#define MGNNS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mgnns_stream_t;
typedef struct mgnns_comm_s* mgnns_comm_t;      /* an RCCL communicator (one per rank / per device) */

/* activation codes for mgnns_linear_fwd / mgnns_matmul_fwd */
#define MGNNS_ACT_NONE   0
#define MGNNS_ACT_RELU   1   /* F.relu, submodules.py:135 */
#define MGNNS_ACT_LRELU2 2   /* nn.LeakyReLU(0.2), Multi_GCN_Multihead_att.py:306 */

#define MGNNS_ERR_ARG     (-1)
#define MGNNS_ERR_LAUNCH  (-2)
#define MGNNS_ERR_UNSUPP  (-3)

/* Status word of the persistent launches.  mgnns_label_gcn_fwd hands work between the workgroups of ONE launch through an
 * in-order item queue (the fused channel / layer tails pass partial results inside clusters of adjacent workgroups without
 * anybody waiting: the last arriver finishes the tile); nothing
 * needs the whole grid resident, and every wait is bounded: a wait that runs out (a device in trouble, a debugger
 * holding a wave) writes one of the codes below into the registered word and the launch drains instead of hanging.  The next
 * persistent launch of the process returns MGNNS_ERR_LAUNCH with the story in mgnns_last_error() and clears the word;
 * mgnns_take_status() reads-and-clears it explicitly (e.g. after a stream synchronise).
 * host_pinned: 4 bytes of host memory that the device can write (hipHostMalloc / a pinned torch tensor), alive until replaced;
 * NULL unregisters.  Without a registered word the waits are still bounded, only the report is lost. */
#define MGNNS_STATUS_LABEL_GCN_TIMEOUT 1
#define MGNNS_STATUS_CLUSTER_TIMEOUT   2      /* (no launch raises it any more: no cluster exchange waits) */
#define MGNNS_STATUS_BAD_PLAN          3      /* a masked attention launch was handed a plan of another kind / batch: it did nothing */
int mgnns_set_status_word(int32_t* host_pinned);
int mgnns_take_status(void);

/* Text of the last error on the calling thread ("" if none). */
const char* mgnns_last_error(void);
/* ABI version (bumped on any signature change). */
#define MGNNS_ABI_VERSION 26
int mgnns_abi_version(void);
/* 16 hex digits: sha256 over the sources this library was built from (every .hip and .hpp file of csrc and every header of
 * include; mgnns_amd/build.py generates the unit).  A measurement records it; the host side refuses to file a profile under
 * sources that differ. */
const char* mgnns_source_fingerprint(void);
/* Measurement, not an operator: does `blockIdx.x & 7` select the XCD on this device / runtime?  Several kernels place work that
 * way (SpMM feature slabs, the dense GEMM's row-block ranges) -- only their SPEED depends on it.  out9[0] = 1 / 0, out9[1 + k] =
 * the hardware XCC_ID observed for block indices with b & 7 == k (-1: more than one).  Synchronises the device. */
int mgnns_xcd_probe(int32_t* out9);

/* ---- a1: text-level GCN channel -------------------------------------------------------
 * Replaces Text_GCN.Model.forward (models/Text_GCN.py:213-275) including the host graph
 * construction seq_to_graph / add_seq_edges (Text_GCN.py:142-211):
 *   per document b: t = non-zero ids of tok[b, :min(T,max_length)];
 *   edge t_i -> t_j for |i-j| <= ngram (and the self loop), weight edge_w[pmi(t_i,t_j)];
 *   h'_v = max_e w_e * node_hidden[src_e];  out[b] = relu(sum over distinct v of h'_v).
 * tok [B,T] int64 (0 = PAD); node_hidden [V,D] (D <= 320); edge_w [n_edge_w] (seq_edge_w
 * [count,1] flattened); PMI map as CSR over V rows with sorted int32 columns and edge ids
 * (id 0 / absent = "no PMI entry", utils/pmi.py:86-97); out [B,D].
 * pmi_eid may be NULL: the id of the entry stored at CSR position k is then k + 1 -- the row-major
 * numbering utils/pmi.py:86-97 hands out -- and the lookup needs one dependent load less.
 * One 1024-thread workgroup per document; needs min(T,max_length)*(D+2*ngram+4)*4 + ~20 KB <= 160 KB of LDS.
 */
int mgnns_textgcn_fwd(const int64_t* tok, int B, int T,
                      const float* node_hidden, int V, int D,
                      const float* edge_w, int n_edge_w,
                      const int32_t* pmi_row_ptr, const int32_t* pmi_col, const int32_t* pmi_eid,
                      int ngram, int max_length, float* out, mgnns_stream_t stream);
/* Launch form of mgnns_textgcn_fwd (results agree to fp32 summation order; a test / measurement knob, process wide):
 * 0 = by batch and shape (default): batches of at least 64 documents run ONE launch of the lean kernel (256 threads, 8 KB of LDS,
 *     <= 64 registers, node rows read from L2: it fits beside an image-bank workgroup of the same forward),
 *     smaller ones one launch of 1024-thread workgroups with the document's node rows in LDS;
 * 1 = always that 1024-thread form, 2 = two launches (documents of <= 24 tokens on 256-thread workgroups, then the others on the
 *     1024-thread form; round 3-4's form for large batches), 3 = always the lean kernel (needs D % 4 == 0). */
int mgnns_textgcn_set_form(int form);

/* ---- a2: embedding gather ---------------------------------------------------------------
 * nn.Embedding lookups (Multi_GCN_Multihead_att.py:371; Text_GCN.py:184,206):
 * out[i,:] = table[idx[i],:], idx [n] int64 in [0,V), table [V,D], out [n,D].
 */
int mgnns_embedding_fwd(const int64_t* idx, int64_t n, const float* table, int V, int D,
                        float* out, mgnns_stream_t stream);

/* ---- a2 + a10: text memory bank = embedding gather + packed multi-layer bidirectional LSTM -----------
 * get_text_memory_bank (Multi_GCN_Multihead_att.py:366-398): embedding(text) -> pack_padded_sequence ->
 * nn.LSTM(hidden 150, bidirectional, batch_first) -> pad_packed_sequence(total_length=T).
 * tok [B,T] int64; lens [B] int64 ON THE DEVICE (valid tokens per sample, clamped to [0,T]);
 * emb_table [V,emb_dim]; per layer l: w_ih_cat[l] = [weight_ih_l{l} ; weight_ih_l{l}_reverse] stacked to
 * [2*4*hidden, in_l] and b_ih_cat[l] [2*4*hidden] (both directions' input projections run as one GEMM);
 * per (layer l, direction d) at index 2*l+d (d=1 is "_reverse"): w_hh [4*hidden, hidden], b_hh [4*hidden]
 * (gate order i,f,g,o); all passed as host arrays of device pointers; out [B,T,2*hidden] (zeros at t >= lens[b]);
 * out_bf16 (optional, may be NULL): the same bank as bf16 [B,T,ld_bf16], zero padded -- what
 * mgnns_sq_mha_core_bf16_fwd consumes.
 * workspace: >= mgnns_bilstm_workspace_bytes(B,T,hidden,num_layers) bytes of device memory.
 * hidden == 150, num_layers <= 2.
 */
size_t mgnns_bilstm_workspace_bytes(int B, int T, int hidden, int num_layers);
int mgnns_bilstm_fwd(const int64_t* tok, const int64_t* lens, int B, int T,
                     const float* emb_table, int V, int emb_dim, int hidden, int num_layers,
                     const float* const* w_ih_cat, const float* const* b_ih_cat,
                     const float* const* w_hh, const float* const* b_hh,
                     void* workspace, size_t workspace_bytes, float* out, void* out_bf16, int ld_bf16,
                     mgnns_stream_t stream);
/* Same contract, bf16-mode recurrence: the per-step W_hh . h on v_mfma_f32_4x4x4_16b_bf16 (W_hh and h rounded to bf16 for
 * the product; fp32 accumulation, gates and cell state; fast exp / rcp): ~2e-3 absolute on the bank, 2.5x shorter chain.  The
 * input projections stay on the exact-f32 GEMM. */
int mgnns_bilstm_bf16_fwd(const int64_t* tok, const int64_t* lens, int B, int T,
                     const float* emb_table, int V, int emb_dim, int hidden, int num_layers,
                     const float* const* w_ih_cat, const float* const* b_ih_cat,
                     const float* const* w_hh, const float* const* b_hh,
                     void* workspace, size_t workspace_bytes, float* out, void* out_bf16, int ld_bf16, const void* prepacked,
                     mgnns_stream_t stream);
/* Weights of the bf16 recurrence / projections in their kernel layouts (depends on the weights only: build once per weight
 * version, pass as `prepacked`; NULL = packed on the fly inside every call). */
size_t mgnns_bilstm_bf16_prepack_bytes(int hidden, int num_layers);
int mgnns_bilstm_bf16_prepack(const float* const* w_ih_cat, const float* const* w_hh, int emb_dim, int hidden, int num_layers,
                              void* packed, mgnns_stream_t stream);
/* The layer-0 input projection FOLDED into the embedding table (weights only, once per weight version; MODEL:366-398: the embedding
 * lookup feeds nn.LSTM's first W_ih and nothing else):
 *   table[v, :] = bf16(emb_table[v, :]) . bf16(w_ih_cat0)^T + b_ih_cat0     [V, 2 * 4 * hidden] fp32 (mgnns_bilstm_bf16_table_bytes)
 * by the same bf16 GEMM the forward would run on its gathered rows (same k order per element: bit-identical rows).
 * mgnns_bilstm_bf16_table_fwd = mgnns_bilstm_bf16_fwd reading its layer-0 projection rows out of `gx_table` by token id: no
 * gather / cast of embedding rows and no GEMM in front of the first recurrence.  workspace of the fold:
 * mgnns_bilstm_bf16_fold_workspace_bytes(V) bytes (the bf16 copies of the table and of W_ih). */
size_t mgnns_bilstm_bf16_table_bytes(int V, int hidden);
size_t mgnns_bilstm_bf16_fold_workspace_bytes(int V);
int mgnns_bilstm_bf16_fold_embedding(const float* emb_table, int V, int emb_dim, int hidden, const float* w_ih_cat0,
                                     const float* b_ih_cat0, void* workspace, size_t workspace_bytes, float* table,
                                     mgnns_stream_t stream);
int mgnns_bilstm_bf16_table_fwd(const int64_t* tok, const int64_t* lens, int B, int T,
                     const float* emb_table, int V, int emb_dim, int hidden, int num_layers,
                     const float* const* w_ih_cat, const float* const* b_ih_cat,
                     const float* const* w_hh, const float* const* b_hh,
                     void* workspace, size_t workspace_bytes, float* out, void* out_bf16, int ld_bf16, const void* prepacked,
                     const float* gx_table, mgnns_stream_t stream);

/* ---- a3: adjacency normalisation ----------------------------------------------------------
 * gen_adj (utils/util.py:421-426): d = rowsum(A)^-1/2; adj[i,j] = (A[j,i]*d[i])*d[j].
 * A, adj [C,C].  Also emits adj as CSR (row_ptr [C+1] int32, col/val [C*C] capacity,
 * ascending columns) for mgnns_spmm_csr_fwd; csr pointers may be NULL to skip.
 */
int mgnns_gen_adj(const float* A, int C, float* adj, float* work /* [C] floats */,
                  int32_t* csr_row_ptr, int32_t* csr_col, float* csr_val, mgnns_stream_t stream);

/* Dense [C,C] -> CSR (ascending columns; col/val capacity C*C): for GraphConvolution.forward(input, adj)
 * callers that hand over a dense adjacency (MODEL:52). */
int mgnns_dense_to_csr(const float* M, int C, int32_t* csr_row_ptr, int32_t* csr_col, float* csr_val,
                       mgnns_stream_t stream);

/* ---- a4: GraphConvolution = dense X*W then sparse adj*support --------------------------------
 * mgnns_matmul_fwd:   Y[M,N] = act(X[M,K] * W[K,N])      (GraphConvolution.weight layout
 *                     [in,out], Multi_GCN_Multihead_att.py:53)
 * mgnns_spmm_csr_fwd: Y[i,:] = act(sum_p val[p] * X[col[p],:]), p in row i   (MODEL:54 with
 *                     the adjacency in CSR; F % 4 == 0)
 */
int mgnns_matmul_fwd(const float* X, int M, int K, const float* W, int N, float* Y, int act,
                     void* workspace, size_t workspace_bytes, mgnns_stream_t stream);
int mgnns_spmm_csr_fwd(const int32_t* row_ptr, const int32_t* col, const float* val, int n_rows,
                       const float* X, int F, float* Y, int act, mgnns_stream_t stream);
/* GraphConvolution(bias=True) (MODEL:40-41,55-56): Y[i,:] = act(sum_p ... + bias[:]); bias [F] (the reference's
 * [1,1,F] parameter), NULL = the call above. */
int mgnns_spmm_csr_bias_fwd(const int32_t* row_ptr, const int32_t* col, const float* val, int n_rows,
                            const float* X, int F, const float* bias, float* Y, int act, mgnns_stream_t stream);

/* ---- a3/a4 at BASELINE configs[4] scale: bf16-feature sparse propagation ---------------------------------
 * Y[i,:] = act(sum_p val[p] * X[col[p],:]) as above (MODEL:54, adjacency of UTIL:421-426 held sparse) with the
 * adjacency values and X in bf16, fp32 accumulation in ascending column order, Y bf16 (y_bf16 = 1) or fp32.
 * Algorithmic bytes: nnz * (4 + 2) + n_cols * F * 2 + n_rows * F * 2.  X must be finite.
 *
 * mgnns_spmm_csr_bf16_fwd: one gather per non-zero from the XCD's L2 (feature slabs of 128 owned by XCDs); the path for
 *   PMI-like graphs (a few non-zeros per row).  F % 8 == 0; nnz = row_ptr[n_rows]; val_bf16 must be readable up to an
 *   even number of elements (the values travel as aligned dwords).  variant = 0 (default: the pipelined ring form) or a
 *   sweep code selecting one of the three kernel forms and its launch geometry (csrc/spmm_bf16.hip, tools/dev).
 *   row_map (optional, int32 [n_rows]): the CSR's row r is row row_map[r] of Y -- a static adjacency is handed over with its
 *   rows SORTED BY LENGTH (four rows share a wave instruction: with equal lengths nobody idles; ops.SparseAdjBf16 does it),
 *   the values of every row of Y are the same bits either way.  NULL: the CSR's row r is row r of Y.
 * mgnns_spmm_tiled_bf16_fwd: dense-ish graphs (tens of non-zeros per row): X staged through LDS tiles of `tile_cols`
 *   columns by LDS-DMA, a workgroup of 16 waves owns 16 * rows_per_wave rows x 32 * lane_bytes features of Y in
 *   registers.  The adjacency comes as the one-off re-ordered stream of mgnns_amd/spmm_plan.py (format documented
 *   there): wave_off [(ceil(n_rows / (16 rows_per_wave)) * 16) * (ceil(n_cols / tile_cols) + 1)] uint32, ent uint32
 *   (64 dwords of slack at the end).  Built geometries (lane_bytes, rows_per_wave, tile_cols): (8, 10, 128),
 *   (8, 20, 128), (4, 10, 256), (4, 20, 256).  F % (32 lane_bytes) == 0.
 * mgnns_cast_bf16: fp32 -> bf16 (round to nearest even), n elements (adjacency values, features).
 */
int mgnns_cast_bf16(const float* src, long long n, void* dst_bf16, mgnns_stream_t stream);
int mgnns_spmm_csr_bf16_fwd(const int32_t* row_ptr, const int32_t* col, const void* val_bf16, int n_rows, int nnz,
                            const void* X_bf16, int F, void* Y, int y_bf16, int act, int variant,
                            const int32_t* row_map, mgnns_stream_t stream);
int mgnns_spmm_tiled_bf16_fwd(const uint32_t* wave_off, const uint32_t* ent, int lane_bytes, int rows_per_wave,
                              int tile_cols, int n_rows, int n_cols, const void* X_bf16, int F, void* Y, int y_bf16,
                              int act, mgnns_stream_t stream);

/* ---- nn.Linear -------------------------------------------------------------------------------
 * Y[M,N] = act(X[M,K] * W[N,K]^T + bias[N]) (+ residual[M,N]);  bias/residual may be NULL.
 * Serves every nn.Linear / Conv1d(k=1) on the path (MODEL:78-82,320-335; submodules.py:24-26,
 * 34,126-127) and the read-out pooled*G^T (MODEL:474,500) with W = G [C,2048].
 */
int mgnns_linear_fwd(const float* X, int M, int K, const float* W, const float* bias, int N,
                     const float* residual, float* Y, int act,
                     void* workspace, size_t workspace_bytes, mgnns_stream_t stream);
/* Both GEMM entry points split the K dimension over extra workgroups when the 64x64 tiling alone would leave
 * most of the 256 CUs idle (M = batch = 256 layers); `workspace` (device, >= mgnns_gemm_workspace_bytes(), one
 * per stream in flight) receives the partial sums, reduced in a fixed order.  NULL workspace = no K split. */
size_t mgnns_gemm_workspace_bytes(void);

/* ---- a5+a6: image memory bank + global max-pool, one pass over the feature map ------------------
 * get_img_{object,place}_memory_bank (MODEL:400-428) fused with MaxPool2d(14,14) (MODEL:454-455):
 *   bank[b,p,:] = W * feat[b,:,p] + bias    feat [B,K,P] (NCHW map viewed [B,2048,196])
 *   pooled[b,k] = max_p feat[b,k,p]
 * Wt is the Linear weight TRANSPOSED and padded: [K, ldw] with ldw >= N, ldw % 16 == 0, columns
 * N..ldw-1 zero (build it once per weight version with mgnns_transpose_pad).  N <= 304, P <= 208,
 * K % 16 == 0.  bank [B,P,N]; pooled [B,K] (NULL to skip).
 */
int mgnns_imgbank_pool_fwd(const float* feat, int B, int K, int P,
                           const float* Wt, int ldw, const float* bias, int N,
                           float* bank, float* pooled, mgnns_stream_t stream);
/* bf16-operand variant (BASELINE config 3): same reads (the fp32 map crosses HBM once, max-pool exact fp32),
 * W pre-packed by mgnns_imgbank_pack_weights_bf16 into mgnns_imgbank_packed_weight_bytes(K) bytes, the bank is
 * emitted as bf16 [B, P, ld] with ld == 320 (zero padded) -- the layout mgnns_sq_mha_core_bf16_fwd consumes.
 * pooled_work: [B, 2, K] floats: two partial maxima whose max is the pooled value (pooled may be NULL: the caller then
 * consumes these itself, e.g. mgnns_label_tail_fwd with n_parts = 2).  16 <= P <= 208, P % 4 == 0, N <= 304, K % 64 == 0.
 * Two forms, chosen by the batch: one workgroup per sample streaming the map through an LDS-DMA ring (chip-filling batches),
 * two workgroups per sample (region halves; needs 104 < P <= 200, K % 128 == 0) up to half a chip of samples.
 * mgnns_imgbank_set_form: 0 = by batch (default), 1 = always the stream form, 2 = always the pair form
 * where its limits allow -- for tests and measurements; process-wide.  B = 0: the shape is checked, nothing is launched, the
 * tensors may be NULL.
 */
int mgnns_imgbank_set_form(int form);
size_t mgnns_imgbank_packed_weight_bytes(int K);
int mgnns_imgbank_pack_weights_bf16(const float* W, int N, int K, void* Wp, mgnns_stream_t stream);
int mgnns_imgbank_pool_bf16_fwd(const float* feat, int B, int K, int P, const void* Wp, const float* bias, int N,
                                void* bank_bf16, int ld, float* pooled, float* pooled_work, mgnns_stream_t stream);

/* Split-bf16 ("bf16x3") form of the same pass: fp32-class accuracy (every operand as bf16 hi + lo, three MFMAs per product,
 * fp32 accumulation: ~2^-16 relative per product) at bf16-MFMA speed -- the parity-grade mode's image bank.
 * (Wp_hi, Wp_lo) = mgnns_pack_weight_bf16_split of liner_img_*.weight [N,K]; bank [B,P,N] fp32 (+ bias);
 * pooled_halves [B,2,K] fp32 or NULL: exact maxima over the region halves [0,112) / [112,P) (-inf for an empty half).
 * bank_hi / bank_lo (both or neither; round 5): the same bank as split-bf16 images hi = bf16(x), lo = bf16(x - hi), bf16
 * [B,P,320] each, columns [N,320) zero -- what mgnns_sq_mha_core_split_fwd consumes; `bank` may then be NULL (N even).
 * K % 64 == 0, P % 4 == 0, P <= 224, N <= 304. */
int mgnns_imgbank_pool_split_fwd(const float* feat, int B, int K, int P, const void* Wp_hi, const void* Wp_lo,
                                 const float* bias, int N, float* bank, float* pooled_halves, void* bank_hi, void* bank_lo,
                                 mgnns_stream_t stream);

/* out[c, r] = in[r, c] for r < rows, c < cols; out is [cols, ld] with zero padding. */
int mgnns_transpose_pad(const float* in, int rows, int cols, float* out, int ld, mgnns_stream_t stream);

/* ---- a7: label-query attention core -----------------------------------------------------------------
 * The element-wise "attention" of Attention.forward (MODEL:101-131) between the projections:
 *   x[b,l,h*dh+d] = softmax_d(Q[l,h,d]*K[b,h,d]/sqrt(dh)) * V[b,h,d]
 * Q [NLQ,hid], K,V [B,hid] (already through w_q/w_k/w_v), x [B,NLQ,hid]; hid = n_heads*dh, dh <= 64.
 * Replaces the B-iteration torch.cat loop (MODEL:114-115).
 */
int mgnns_label_attn_core_fwd(const float* Q, const float* K, const float* V, int B, int NLQ,
                              int n_heads, int dh, float* x, mgnns_stream_t stream);
/* Attention.forward(mask=...) (MODEL:118-119): energy.masked_fill(mask == 0, -1e10) behind the scaling, in front of
 * the softmax over d.  mask = the byte image [B,NLQ,hid] of the caller's mask broadcast against the energy
 * [B,NLQ,heads,dh] (0 = masked); NULL = the call above. */
int mgnns_label_attn_core_masked_fwd(const float* Q, const float* K, const float* V, const unsigned char* mask,
                                     int B, int NLQ, int n_heads, int dh, float* x, mgnns_stream_t stream);

/* ---- a5 + a7 (fused): everything of an image channel behind the memory-bank kernel, one launch ----------------
 * Read-out (MODEL:454-455 max-pool halves + 474 `matmul(feature, x)`), Attention.forward (MODEL:88-133) without its
 * w_q, then linear_5 and x_linear (MODEL:477-479 / 504-506), optionally the query projection of the fusion stack the
 * result feeds (submodules.py:63-66):
 *   x = max_parts(pooled) . G^T                      (or x given: pass g_wp = NULL)
 *   K = w_k x + b_k, V = w_v x + b_v;  o[b,l] = softmax_d(Q[l] * K[b] / sqrt(dh)) * V[b] per head;
 *   y[b,l] = Wc o[b,l] + bc  with Wc = linear_5.weight . fc.weight [N5,hid], bc = linear_5.weight . fc.bias +
 *   linear_5.bias (the two maps have no non-linearity between them; composed by the caller);
 *   out[b] = x_linear(concat_l y[b,l]);   qh_next[b] = w_qs(out[b]) + b_qs  (wq_next_wp != NULL; needs n_out == hid).
 * pooled [B,n_parts,K_pool] (n_parts = 2: the memory-bank kernel's per-half maxima), g_wp = mgnns_pack_weight_f32
 * image of G [C,K_pool]; Q [NLQ,hid] = w_q(label query); wk_wp / wv_wp / wc_wp / xl_wp / wq_next_wp are
 * mgnns_pack_weight_f32 images of w_k [hid,C], w_v [hid,C], Wc [N5,hid], x_linear.weight [n_out, NLQ*N5],
 * w_qs.weight [HK_next, hid]; out [B,n_out].  hid = n_heads*dh <= 320, dh <= 64, N5 <= 128, NLQ*N5 >= 512 with G.
 * One workgroup per 16 samples; every contraction on the exact-f32 MFMA.
 */
int mgnns_label_tail_fwd(const float* x, int B, int C, const float* pooled, int n_parts, int K_pool,
                         const float* g_wp, const float* Q, int NLQ, int n_heads, int dh,
                         const float* wk_wp, const float* bk, const float* wv_wp, const float* bv,
                         const float* wc_wp, const float* bc, int N5, const float* xl_wp, const float* bxl,
                         int n_out, float* out, const float* wq_next_wp, const float* bq_next, int HK_next,
                         float* qh_next, mgnns_stream_t stream);

/* bf16 precision mode of the same chain, read-out always inside, every contraction on the bf16 MFMA (fp32 accumulation;
 * softmax, biases, attention products fp32).  terms = 1: plain bf16 operands; terms = 3: split-bf16 (hi + lo operands, three
 * MFMAs per product, fp32-class accuracy).  packed[12] = the (hi, lo) buffer pairs of mgnns_pack_weight_bf16_split for
 * G [C,K_pool], w_k, w_v [hid,C], Wc [N5,hid], x_linear.weight [n_out, NLQ*N5], w_qs.weight [HK_next, hid] (last pair may
 * be NULL; lo buffers are not read with terms = 1).  C <= 384, K_pool % 64 == 0, hid <= 320, N5 <= 128, n_out <= 384.
 * cluster_scratch / cluster_counters (both or neither; terms = 3 only): with them FOUR workgroups share each 16-sample
 * tile's read-out (K divided, partial read-outs passed through the scratch); the one that arrives LAST finishes the tile
 * alone (nobody waits), and the next query runs as a second small launch behind the tail, inside this call:
 * scratch >= ceil(B/16) * 4 * 24576 B, 16-byte aligned; counters = 2 * ceil(B/16) ints, ZERO before the first launch
 * (every launch leaves them zero).  One (scratch, counters) pair must not be shared by launches that may run concurrently.
 */
int mgnns_label_tail_bf16_fwd(const float* pooled, int B, int n_parts, int K_pool, int C, int terms,
                              const void* const* packed, const float* Q, int NLQ, int n_heads, int dh, const float* bk,
                              const float* bv, const float* bc, int N5, const float* bxl, int n_out, float* out,
                              const float* bq_next, int HK_next, float* qh_next, float* cluster_scratch,
                              int* cluster_counters, mgnns_stream_t stream);

/* ---- a8: single-query multi-head attention, K/V projection fused ---------------------------------------
 * MultiHeadAttention.forward + ScaledDotProductAttention.forward (submodules.py:55-119) for len_q == 1,
 * up to (not including) fc:  per (b,h)
 *   s[l] = qh[b,h,:] . (Wk_h bank[b,l,:] + bk_h) / sqrt(dk);  s[l] = -inf where mask[b,l] == 0
 *   p = softmax_l(s);  o[b,h,:] = sum_l p[l] (Wv_h bank[b,l,:] + bv_h)
 * K and V are never written to memory.  qh [B,H*dk] (already through w_qs); bank [B,L,D];
 * mask [B,L] float or NULL; Wk,Wv [H*dk, D]; o [B,H*dk]; attn [H*B, L] (row h*B+b, submodules.py:72-78)
 * or NULL.  dk == 128, D <= 320, L <= 208.
 */
int mgnns_sq_mha_core_fwd(const float* qh, const float* bank, const float* mask,
                          int B, int L, int D, int H, int dk,
                          const float* Wk, const float* bk, const float* Wv, const float* bv,
                          float* o, float* attn, mgnns_stream_t stream);

/* Head-difference term of MultiHeadAttention(is_regu=True) (models/submodules.py:38-52, 84-93): o [B, H*dv] = the per-head
 * attention outputs (the `o` of mgnns_sq_mha_core_*_fwd) -> out [B] = mean over ordered head pairs i != j of
 * cos^2(o_i, o_j) (n_head == 1: 0 / 0 = NaN, as in the reference).  H <= 16.
 */
int mgnns_head_diff_fwd(const float* o, int B, int H, int dv, float* out, mgnns_stream_t stream);

/* ---- a8, bf16-operand variant (BASELINE config 3: "bf16 MFMA") ------------------------------------------
 * Same contract as mgnns_sq_mha_core_fwd, but the projections run on v_mfma_f32_16x16x32_bf16 (bf16 operands,
 * fp32 accumulation; scores/softmax/weighted sum fp32).  The memory bank is bf16 [B, L, ld] with ld == 320
 * (model dim 300 zero padded; build with mgnns_cast_pad_bf16 or let mgnns_imgbank_pool_bf16_fwd emit it);
 * the K/V weights are pre-packed once per weight version by mgnns_sq_mha_pack_weights_bf16 into
 * mgnns_sq_mha_packed_weight_bytes(H) bytes (MFMA-fragment-major, 1 KiB per fragment).  L <= 208, H <= 16, D <= 320 at the packer.
 * mgnns_cast_pad_bf16: y [rows, ld] = bf16(x [rows, D]) zero padded, round to nearest even, a NaN stays a quiet NaN of its sign
 * whatever its payload; ld >= D, ld % 8 == 0.  B = 0 / rows = 0: the shape is checked, nothing is launched, the tensors may be NULL.
 */
size_t mgnns_sq_mha_packed_weight_bytes(int H);
int mgnns_sq_mha_pack_weights_bf16(const float* Wk, const float* Wv, int H, int dk, int D, void* Wp,
                                   mgnns_stream_t stream);
int mgnns_cast_pad_bf16(const float* x, int64_t rows, int D, int ld, void* y, mgnns_stream_t stream);
int mgnns_sq_mha_core_bf16_fwd(const float* qh, const void* bank_bf16, const float* mask,
                               int B, int L, int ld, int H, int dk,
                               const void* Wp, const float* bk, const float* bv,
                               float* o, float* attn, mgnns_stream_t stream);

/* ---- a8, bf16 operands on v_mfma_f32_32x32x16_bf16 (round 4) -----------------------------------------------
 * Same contract and inputs as mgnns_sq_mha_core_bf16_fwd (submodules.py:55-119, len_q == 1; moudles.py:207-230 calls it);
 * bank rows in tiles of 32, the model dim in 19 k-steps of 16 (300 -> 304), L <= 224.  The K/V weights are packed by
 * mgnns_sq_mha32_pack_weights_bf16 into mgnns_sq_mha32_packed_weight_bytes(H) bytes (a different fragment order from the
 * 16x16x32 form's).
 * `plan` (optional, needs a mask and L <= 128): the packing plan of the batch's mask -- mgnns_sq_mha32_plan_ints(B) int32 built
 * by mgnns_sq_mha32_plan(mask, B, L, plan) once per batch and shared by every launch on that mask (Multi_GCN_Multihead_att.py:
 * 509-527: both image->text stacks, every layer).  With a plan the live rows of several short samples share a workgroup
 * (8-row aligned, <= 128 rows and <= 16 samples per group): the weight stream is read once per group instead of once per
 * sample.  Same results as without a plan up to fp32 summation order.  plan == NULL: one workgroup per sample.
 * B = 0: the shape is checked, nothing is launched, the tensors may be NULL (mgnns_sq_mha32_plan: the mask may be NULL, the plan
 * is its four header ints).  H <= 16, D <= 304 at the packer, B <= 4096 at the plan.
 */
size_t mgnns_sq_mha32_packed_weight_bytes(int H);
int mgnns_sq_mha32_pack_weights_bf16(const float* Wk, const float* Wv, int H, int dk, int D, void* Wp,
                                     mgnns_stream_t stream);
size_t mgnns_sq_mha32_plan_ints(int B);
int mgnns_sq_mha32_plan(const float* mask, int B, int L, int32_t* plan, mgnns_stream_t stream);
int mgnns_sq_mha32_core_bf16_fwd(const float* qh, const void* bank_bf16, const float* mask,
                                 int B, int L, int ld, int H, int dk,
                                 const void* Wp, const float* bk, const float* bv,
                                 float* o, float* attn, const int32_t* plan, mgnns_stream_t stream);

/* ---- a8, split-bf16 operands ("bf16x3", round 5): the reference's formulation inside the 1e-4 parity gate on the bf16 pipe ----
 * Same contract as mgnns_sq_mha_core_fwd (models/submodules.py:55-119, len_q == 1: K and V projected from the memory bank,
 * scores / mask / softmax / weighted sum fp32, K and V never written to memory).  Every fp32 operand of the two projections is
 * carried as hi = bf16(x), lo = bf16(x - hi) and a product is three v_mfma_f32_16x16x32_bf16 (hi hi + lo hi + hi lo, fp32
 * accumulation, ~2^-16 relative per product).  The memory bank arrives as two bf16 images [B, L, ld], ld == 320 (model dim 300
 * zero padded): build them with mgnns_split_pad_bf16 from the fp32 bank.  The K/V weights are packed once per weight version by
 * mgnns_sq_mha_pack_weights_split into mgnns_sq_mha_split_packed_weight_bytes(H) bytes (hi image, then lo image, each in the
 * fragment-major order of mgnns_sq_mha_pack_weights_bf16).  The bank rows are walked in two halves of at most 112 (the two images
 * of 196 rows do not fit the 160 KB of LDS) joined by an exact fp32 online-softmax merge.  dk == 128, L <= 208, H <= 16.
 */
size_t mgnns_sq_mha_split_packed_weight_bytes(int H);
int mgnns_sq_mha_pack_weights_split(const float* Wk, const float* Wv, int H, int dk, int D, void* Wp,
                                    mgnns_stream_t stream);
int mgnns_split_pad_bf16(const float* x, int64_t rows, int D, int ld, void* hi, void* lo, mgnns_stream_t stream);
int mgnns_sq_mha_core_split_fwd(const float* qh, const void* bank_hi, const void* bank_lo, const float* mask,
                                int B, int L, int ld, int H, int dk,
                                const void* Wp, const float* bk, const float* bv,
                                float* o, float* attn, const int32_t* plan, mgnns_stream_t stream);
/* `plan` (optional: needs a mask, L <= 112, attn == NULL): the group plan of the batch's mask, mgnns_sq_mha32_plan_ints(B) int32 built
 * by mgnns_sq_mha_split_plan(mask, B, L, plan) once per batch (the layout of mgnns_sq_mha32_plan with other constants: samples in
 * whole tiles of 16 rows, at most 112 rows and 7 samples per group).  The samples of a group share one staging of the bank images
 * and one pass of the weight stream (Multi_GCN_Multihead_att.py:509-527: the text bank, mean 16 live rows of 100).  Same results
 * as without a plan up to fp32 summation order. */
int mgnns_sq_mha_split_plan(const float* mask, int B, int L, int32_t* plan, mgnns_stream_t stream);

/* ---- a8, folded variant: the K/V projections folded into the query side ---------------------------------
 * Same inputs and outputs as mgnns_sq_mha_core_fwd (submodules.py:55-119, len_q == 1) computed as
 *   U_h = Wk_h^T qh_h;   p = softmax_l(U_h . bank[b,l,:] / sqrt(dk)) (masked);   o_h = Wv_h (sum_l p_l bank[b,l,:]) + bv_h
 * which is algebraically the reference's result (q.bk is constant over l and drops out of the softmax; sum_l p_l = 1
 * carries bv through) at 1/100 of the FLOPs, all in fp32 (f32 MFMA): the folded attention of the fp32 / bf16x3 modes (the
 * faithful kernels above are what the MFMA-utilisation target is measured on; bf16 mode: mgnns_sq_mha_folded_bf16_fwd below).
 * bank: fp32 [B, L, D] (bank_is_bf16 == 0, ld_bank == D) or bf16 [B, L, ld_bank] zero padded (bank_is_bf16 == 1).
 * workspace: mgnns_sq_mha_folded_workspace_bytes(B, D, H) bytes.  D <= 320, D % 4 == 0, H <= 8, dk % 4 == 0, L <= 208.
 */
size_t mgnns_sq_mha_folded_workspace_bytes(int B, int D, int H);
int mgnns_sq_mha_folded_fwd(const float* qh, const void* bank, int bank_is_bf16, int ld_bank, const float* mask,
                            int B, int L, int D, int H, int dk, const float* Wk, const float* Wv, const float* bv,
                            void* workspace, size_t workspace_bytes, float* o, float* attn, mgnns_stream_t stream);

/* ---- a8, folded variant on the bf16 matrix pipe (bf16 precision mode) ----------------------------------------------
 * The same attention (submodules.py:55-119, len_q == 1) with ALL FOUR projections composed into the maps either side of it
 * (the host mirror builds them once per weight version, fusion.py):
 *   u_h = (Wk_h^T Wq_h) x + Wk_h^T bq_h                                     -- the previous tail's "next projection"
 *   p   = softmax_l(u_h . bank[b,l,:] / sqrt(dk)) (masked);   c_h = sum_l p_l bank[b,l,:]            -- this kernel
 *   fc(o) = sum_h (fc_h Wv_h) c_h + (fc bv + b_fc)                          -- the tail's first map (mgnns_mha_tail_c16_fwd)
 * U: fp32 [B, H*D] (head h at h*D); bank: bf16 [B, L, 320] zero padded; mask: fp32 [B, L] (0 = masked) or NULL;
 * C: bf16 [B, ldc] (ldc >= H*D, ldc % 8 == 0; head h at h*D, zeros behind H*D -- ldc = H*D rounded up to 32 is what
 * mgnns_mha_tail_c16_fwd takes); attn: fp32 [H*B, L] or NULL.  D <= 320, D % 4 == 0, H <= 8, L <= 208.  One read of the bank.
 * B = 0: the shape is checked, nothing is launched, the tensors may be NULL.
 */
int mgnns_sq_mha_folded_bf16_fwd(const float* U, const void* bank_bf16, const float* mask, int B, int L, int D, int H,
                                 float inv_temp, void* C_bf16, int ldc, float* attn, mgnns_stream_t stream);

/* ---- a8, rest of the layer: fc + residual + LayerNorm + position-wise FFN + residual + LayerNorm in ONE launch ----
 * MultiHeadAttention.forward after the attention (submodules.py:88-94) and PositionwiseFeedForward.forward
 * (submodules.py:132-139), optionally followed by the NEXT layer's query projection w_qs (submodules.py:68):
 *   y = LN1(fc(o) + q);  out = LN2(w_2 relu(w_1 y + b_1) + b_2 + y);  qh_next = w_qs'(out) + b'
 * o [B, HK] (HK = n_head*d_v), q [B, 300] (the layer's query = the residual), out [B, 300], qh_next [B, HK_next].
 * Every weight is passed PRE-PACKED by mgnns_pack_weight_f32 (MFMA-fragment-major fp32, one 16-B load = four
 * k-steps): fc [300, HK], w_1 / w_2 [300, 300] (Conv1d k=1 weight viewed 2-D), w_qs' [HK_next, 300].
 * wq_next_wp == NULL skips the last step.  Exact fp32.  d_model == 300; HK a multiple of 4, <= 1888 (16 rows of o and the two
 * activation tiles share the 160 KiB of LDS); HK_next any positive width.
 */
size_t mgnns_packed_f32_weight_bytes(int N, int K);
int mgnns_pack_weight_f32(const float* W, int N, int K, float* Wp, mgnns_stream_t stream);
int mgnns_mha_tail_fwd(const float* o, int HK, const float* q, int B, int d_model,
                       const float* fc_wp, const float* fc_b, const float* ln1_gamma, const float* ln1_beta,
                       const float* w1_wp, const float* b1, const float* w2_wp, const float* b2,
                       const float* ln2_gamma, const float* ln2_beta, float eps, float* out,
                       const float* wq_next_wp, const float* bq_next, int HK_next, float* qh_next,
                       mgnns_stream_t stream);

/* bf16-MFMA variant of the fused tail (bf16 precision mode).  terms = 1: bf16 operands; terms = 3: split-bf16
 * (x = hi + lo, a*b ~ a_hi*b_hi + a_hi*b_lo + a_lo*b_hi, fp32 accumulate: ~2^-16 relative per product).  Weights
 * pre-packed by mgnns_pack_weight_bf16_split into TWO buffers (hi, lo) of mgnns_packed_bf16_weight_bytes(N,K)
 * bytes each; `packed` = host array of 8 device pointers {fc_hi, fc_lo, w1_hi, w1_lo, w2_hi, w2_lo, wq'_hi, wq'_lo}
 * (the last two NULL to skip the next-layer projection).  Biases, residuals and LayerNorms are fp32.
 */
size_t mgnns_packed_bf16_weight_bytes(int N, int K);
int mgnns_pack_weight_bf16_split(const float* W, int N, int K, void* Whi, void* Wlo, mgnns_stream_t stream);
int mgnns_mha_tail_bf16_fwd(const float* o, int HK, const float* q, int B, int d_model, int terms,
                            const void* const* packed,
                            const float* fc_b, const float* ln1_gamma, const float* ln1_beta, const float* b1,
                            const float* b2, const float* ln2_gamma, const float* ln2_beta, float eps, float* out,
                            const float* bq_next, int HK_next, float* qh_next, int cluster, float* cluster_scratch,
                            int* cluster_counters, mgnns_stream_t stream);
/* cluster / cluster_scratch / cluster_counters as in mgnns_mha_tail_c16_fwd below (terms = 1 only; NULL buffers: every workgroup
 * of a tile's cluster streams all of fc and the ranks share the next layer's w_qs columns): with the buffers the ranks split the K
 * of fc (submodules.py:88), the last arriver finishes the tile and the next layer's w_qs runs as a second launch. */

/* The bf16 tail (terms = 1) behind mgnns_sq_mha_folded_bf16_fwd: `c` = bf16 [B, HC] (HC = n_head * d_model rounded up to a
 * multiple of 32, <= 2560; zeros behind n_head * d_model) instead of the fp32 head outputs; packed[0] = the composed map
 * fc . blockdiag(Wv) [d_model, n_head * d_model], fc_b = fc bv + b_fc; packed[6] / bq_next = the NEXT layer's composed query map
 * [HC_next, d_model] and its bias (NULL: none); only the hi buffers (even entries of `packed`) are read.
 * cluster: workgroups per 16-sample tile (0 = default: 4 with the exchange buffers; 1..8).  With cluster_scratch
 * (mgnns_mha_tail_c16_scratch_floats(B, 8) floats, 16-byte aligned) and cluster_counters (ceil(B/16) int32, ZERO before the
 * first launch; the kernel leaves them zero; one pair of buffers per concurrently running launch) the ranks split the K of the
 * first product, the rank that arrives LAST adds the partial sums and finishes the tile (nobody waits), and the next layer's
 * query map runs as a second launch behind it; without them every rank streams the whole composed map and takes a share of the
 * next one.  Everything else as mgnns_mha_tail_bf16_fwd.
 */
size_t mgnns_mha_tail_c16_scratch_floats(int B, int cluster);
int mgnns_mha_tail_c16_fwd(const void* c_bf16, int HC, const float* q, int B, int d_model, const void* const* packed,
                           const float* fc_b, const float* ln1_gamma, const float* ln1_beta, const float* b1,
                           const float* b2, const float* ln2_gamma, const float* ln2_beta, float eps, float* out,
                           const float* bq_next, int HC_next, float* u_next, int cluster, float* cluster_scratch,
                           int* cluster_counters, mgnns_stream_t stream);

/* ---- a3 + a4 (+ a7's w_q): one image channel's label GCN as ONE persistent launch ---------------------------------
 * gen_adj (utils/util.py:421-426) + GraphConvolution x 2 with LeakyReLU(0.2) between them
 * (Multi_GCN_Multihead_att.py:460-473 / 489-499, 42-58) + optionally w_q(label_query) (MODEL:97):
 *   adj = D^-1/2 A^T D^-1/2;  X1 = lrelu(adj @ (inp @ W1));  G = adj @ (X1 @ W2);  Q = label_query @ wq^T + bq
 * as a grid of `grid` (0: a quarter of the CUs, 64 on an MI355X -- the measured optimum with two channels' launches side by
 * side) workgroups that pull the phases' work items from one in-order queue
 * instead of 11-12 dependent launches.  split = 0: exact-fp32 MFMA, w1a / w2a = mgnns_pack_weight_f32 of W1^T [N1,K0] /
 * W2^T [N2,N1] (bit-equal to mgnns_gen_adj + mgnns_matmul_fwd + mgnns_spmm_csr_fwd); split = 1: split-bf16 operands
 * (fp32-class), (w1a, w1b) / (w2a, w2b) = the (hi, lo) buffers of mgnns_pack_weight_bf16_split.
 * A [C,C]; inp [C,K0]; G [C,N2]; Gp_hi / Gp_lo (both or neither): the mgnns_pack_weight_bf16_split image of G the fused
 * channel tail reads; Q [NLQ,HQ] or NULL.  C <= 512, K0 % 4 == 0, N1, N2 % 256 == 0, N1 <= 1024.
 * scratch: mgnns_label_gcn_scratch_bytes(C, N1, N2) bytes, 256-byte aligned, its first 256 bytes ZERO before the first
 * launch (every launch leaves them zero); one scratch must not be shared by launches that may run concurrently (it holds
 * the launch's intermediates).  The work items of the four phases are pulled in order from one ticket counter, so the
 * launch makes progress with ANY number of its workgroups resident: any grid, any neighbours (see the status word above).
 */
/* Shape limits of the three fused launches as predicates (1 = the launch takes these shapes): the host side routes
 * everything else to the chain of separate operators, which has no such limits.  K_pool = 0 for mgnns_label_tail_supported:
 * the read-out x is passed in. */
int mgnns_label_gcn_supported(int C, int K0, int N1, int N2, int split);
int mgnns_label_tail_supported(int C, int NLQ, int n_heads, int dh, int N5, int n_out, int K_pool, int with_next_q);
int mgnns_label_tail_bf16_supported(int C, int NLQ, int n_heads, int dh, int N5, int n_out, int K_pool, int terms, int with_next_q);
size_t mgnns_label_gcn_scratch_bytes(int C, int N1, int N2);
int mgnns_label_gcn_fwd(const float* A, int C, const float* inp, int K0, int split, const void* w1a, const void* w1b, int N1,
                        const void* w2a, const void* w2b, int N2, float* G, void* Gp_hi, void* Gp_lo,
                        const float* label_query, int NLQ, const float* wq, const float* bq, int HQ, float* Q,
                        void* scratch, size_t scratch_bytes, int grid, mgnns_stream_t stream);
/* The same launch with a MEMO: nothing it computes depends on the batch, so while inp (the label embedding table, the same tensor
 * for every batch of a dataset) and the weights stay what they were, G / Gp / Q of the previous launch are still right.
 * memo: mgnns_label_gcn_memo_bytes(C, K0) bytes, 256-byte aligned, its first 256 bytes ZERO before the first launch; it holds
 * three words (int32 [0] valid, [1] hit: the verdict of the last launch, 1 = nothing was computed, [2] internal) and, from
 * byte 256, a snapshot of the inp the outputs were computed from.  A small check launch compares inp with the snapshot on the
 * DEVICE, bitwise as integers (NaN equals NaN, -0 differs from +0), and the GCN launch behind it leaves at once on a hit --
 * correct under hipGraph replay, where no host code sees the inputs.  The caller keeps G, Gp_hi / Gp_lo, Q, scratch and memo
 * together and passes the SAME buffers every time (a hit writes nothing); one set per concurrently running launch.  The
 * weights (A, W1, W2, label_query, wq, bq) are NOT compared: after changing one, pass a fresh zeroed memo. */
size_t mgnns_label_gcn_memo_bytes(int C, int K0);
int mgnns_label_gcn_memo_fwd(const float* A, int C, const float* inp, int K0, int split, const void* w1a, const void* w1b, int N1,
                             const void* w2a, const void* w2b, int N2, float* G, void* Gp_hi, void* Gp_lo,
                             const float* label_query, int NLQ, const float* wq, const float* bq, int HQ, float* Q,
                             void* scratch, size_t scratch_bytes, void* memo, size_t memo_bytes, int grid, mgnns_stream_t stream);

/* ---- a9: classifier over the four fusion features (Multi_GCN_Multihead_att.py:560-566, eval: dropout is the identity) --
 * logits[b,:] = W [f0[b]; f1[b]; f2[b]; f3[b]] + bias without materialising the concatenation.  f_p [B,D]; W [NL, 4*D];
 * bias [NL]; logits [B,NL].  The host passes W = multi_linear_2.weight . multi_linear_1.weight (no non-linearity between
 * them in eval) or any single [NL, 4D] map.
 */
int mgnns_classifier_head_fwd(const float* f0, const float* f1, const float* f2, const float* f3, int B, int D,
                              const float* W, const float* bias, int NL, float* logits, mgnns_stream_t stream);
/* The same classifier as nparts launches, one behind each producer of a feature (the four fusion stacks run on different streams):
 * launch `part` adds  parts[part][b][:] = W[:, part*D:(part+1)*D] . f[b]  and the launch that finishes LAST adds the parts in index
 * order + bias into logits [B, NL] -- no launch (and no stream join) of its own behind the slowest stack.  parts [nparts, B, NL],
 * counter: one int32, zero before the first of the nparts launches (the last launch re-arms it).  All nparts launches must use the
 * same B, D, NL, parts, counter, logits.
 */
int mgnns_classifier_part_fwd(const float* f, int part, int nparts, int B, int D, const float* W, const float* bias,
                              int NL, float* parts, int* counter, float* logits, mgnns_stream_t stream);

/* ---- custom LayerNorm (submodules.py:153-156): unbiased std, eps added to std ---------------------------
 * y[r,:] = gamma * (x[r,:] - mean) / (std_unbiased + eps) + beta,  x,y [rows, D], D <= 1024.
 */
int mgnns_layernorm_fwd(const float* x, int rows, int D, const float* gamma, const float* beta,
                        float eps, float* y, mgnns_stream_t stream);

/* ---- training mode of one MyMultiHeadAttention layer (moudles.py:198-230, submodules.py:15-156), fp32 ----------------------
 * Dropout keeps element i of site s iff hash(seed, s, i) >= rate (a counter-based hash; the same seed draws the same mask) and
 * scales the kept values by 1 / (1 - rate).  Sites: 0 = attention probabilities (index (h*B + b)*L + l), 1 = after fc,
 * 2 = after w_2 (index r*D + d).  Every reduction over rows runs in a fixed order: one seed gives bit-identical results.
 *
 * mgnns_mha_train_fwd: the folded attention core with attention dropout.  qh [B, H*dk] = w_qs(q); bank fp32 [B, L, D]; mask
 * [B, L] (0 = masked) or NULL.  Outputs (all [H][B][...]): U [H,B,D] = W_k,h^T qh_h; P [H,B,L] softmax before dropout;
 * attn [H*B, L] after dropout (the reference's returned attn); keep [H,B,L] bytes or NULL; Z [H,B,D] = X^T p'; SP [H,B] =
 * sum_l p'; o [B, H*dk] = W_v,h z_h + b_v,h SP.  D <= 320, D % 4 == 0, H <= 8, dk % 4 == 0, L <= 208, 0 <= rate <= 1.
 * A sample without a live position (a padded row) is an empty contribution: P = attn = Z = SP = 0 and o = 0, and the backward
 * gives it exact zeros (the reference's softmax gives NaN there).
 * mgnns_mha_train_bwd: its backward from dO [B, H*dk] and the forward's saved tensors (keep required): dqh [B, H*dk],
 * dWk / dWv [H*dk, D], dbv [H*dk] (written, not accumulated), dbank [B, L, D] or NULL (masked rows: 0).  b_k has no gradient
 * (it drops out of the softmax).  workspace: mgnns_mha_train_bwd_workspace_bytes(B, D, H, dk) bytes, 16-byte aligned.
 */
int mgnns_mha_train_fwd(const float* qh, const float* bank, const float* mask, int B, int L, int D, int H, int dk,
                        const float* Wk, const float* Wv, const float* bv, uint64_t seed, float rate, float* U, float* P,
                        float* attn, uint8_t* keep, float* Z, float* SP, float* o, mgnns_stream_t stream);
size_t mgnns_mha_train_bwd_workspace_bytes(int B, int D, int H, int dk);
int mgnns_mha_train_bwd(const float* dO, const float* qh, const float* bank, const float* mask, int B, int L, int D, int H,
                        int dk, const float* Wk, const float* Wv, const float* bv, float rate, const float* U, const float* P,
                        const float* attn, const uint8_t* keep, const float* Z, const float* SP, float* dqh, float* dWk,
                        float* dWv, float* dbv, float* dbank, void* workspace, size_t workspace_bytes, mgnns_stream_t stream);
/* Weight gradient of a linear layer: dW[N,K] = dY[M,N]^T X[M,K], db[N] = column sums of dY (db NULL: none).  Row slabs + an
 * ordered combine, no atomics.  workspace: mgnns_wgrad_workspace_bytes(M, N, K) bytes.  M = 0: dW and db are zeroed, dY and X
 * may be NULL. */
size_t mgnns_wgrad_workspace_bytes(int M, int N, int K);
int mgnns_wgrad_fwd(const float* dY, int M, int N, const float* X, int K, float* dW, float* db, void* workspace,
                    size_t workspace_bytes, mgnns_stream_t stream);
/* v = dropout(x) + res;  y = gamma (v - mean) / (std_unbiased + eps) + beta  (rows x D, D <= 1024).  Saves xhat [rows, D],
 * sig [rows] (the unbiased std) and keep [rows, D] (bytes) for the backward. */
int mgnns_drop_res_ln_fwd(const float* x, const float* res, int rows, int D, const float* gamma, const float* beta, float eps,
                          uint64_t seed, int site, float rate, float* y, float* xhat, float* sig, uint8_t* keep,
                          mgnns_stream_t stream);
/* Its backward for dy (+ dy2 when not NULL): dres = dL/dv (the residual's gradient), dx = dres keep / (1 - rate),
 * dgamma / dbeta [D] (written). */
int mgnns_drop_res_ln_bwd(const float* dy, const float* dy2, const float* xhat, const float* sig, const uint8_t* keep, int rows,
                          int D, const float* gamma, float eps, float rate, float* dres, float* dx, float* dgamma, float* dbeta,
                          mgnns_stream_t stream);
/* y = a + b (MGNNS_ELT_ADD), y = a * (b > 0) (MGNNS_ELT_RELU_BWD: ReLU backward, b = the ReLU's output) or
 * y = b > 0 ? a : 0.2 a (MGNNS_ELT_LRELU2_BWD: LeakyReLU(0.2) backward, b = its output or input), n elements. */
#define MGNNS_ELT_ADD        0
#define MGNNS_ELT_RELU_BWD   1
#define MGNNS_ELT_LRELU2_BWD 2
int mgnns_train_eltwise(int op, const float* a, const float* b, int64_t n, float* y, mgnns_stream_t stream);

/* ---- training mode of the model around the fusion stacks (MODEL:431-567), fp32 -------------------------------------------
 * Dropout sites of the model (the hash above; index = flat element index of the tensor the site drops):
 * 3 = the label Attention's softmax(energy) [B, NLQ, H*dh], 4 = the classifier's dropout after multi_linear_1 [B, D].
 *
 * mgnns_imgbank_wgrad: weight gradient of an image memory bank bank[b,p,:] = W X[b,:,p] + c from dbank [B, P, N] and the feature
 * map X [B, K, P] in its native layout: dW[N, K] = sum_{b,p} dbank[b,p,:] (x) X[b,:,p], db[N] (written).  N <= 320.  Exact-f32
 * MFMA, the (b, p) reduction split into slabs combined in a fixed order.  workspace:
 * mgnns_imgbank_wgrad_workspace_bytes(B, K, P, N) bytes.  B = 0: dW and db are zeroed, X and dbank may be NULL.
 * mgnns_map_argmax: arg[b, k] (int32, written) = the FIRST p at which row X[b, k, :] of a feature map X [B, K, P] attains its
 * maximum -- where torch's max_pool2d backward sends the gradient of pooled[b, k] = max_p X[b, k, p] (a tie, e.g. a channel that
 * is zero over a whole image after the ReLU, goes to the smallest index).  NaN in X is not supported.  B = 0: nothing is launched,
 * X and arg may be NULL.
 * mgnns_imgbank_dgrad: gradient of the loss with respect to the feature map X [B, K, P] of an image memory bank:
 * dX[b,k,p] = sum_o W[o,k] dbank[b,p,o] + (p == arg[b,k] ? dpooled[b,k] : 0), written in full, from dbank [B, P, N], the
 * nn.Linear weight W [N, K], and the max-pool's gradient dpooled [B, K] with arg [B, K] from mgnns_map_argmax (entries outside
 * [0, P) add nothing).  dpooled and arg are both NULL (no pooled term) or both given; dbank may be NULL (the pooled term alone; W
 * is then not read), but not dbank and dpooled both.  N <= 320.  Exact-f32 MFMA; the o reduction runs inside one workgroup in a
 * fixed order, no workspace.  B = 0: nothing is launched, the tensors may be NULL.
 * mgnns_imgbank_wgrad_split / mgnns_imgbank_dgrad_split: the same two gradients on the bf16 matrix pipe at fp32-class accuracy
 * (split-bf16: every fp32 operand as hi = bf16(x), lo = bf16(x - hi), a product as hi*lo + lo*hi + hi*hi with fp32 accumulation,
 * ~2^-16 relative per product; db is summed from the unrounded dbank).  Same operands (plain fp32, same layouts), shapes, NULL
 * rules and determinism as the two entries above.  The wgrad's workspace: mgnns_imgbank_wgrad_split_workspace_bytes(B, K, P, N)
 * bytes (slab partials).  The dgrad's workspace, mgnns_imgbank_dgrad_split_workspace_bytes(B, K, P, N) bytes and 16-byte aligned,
 * receives the split, transposed image of W, written by a small launch of the same call (no state is kept between calls); with
 * dbank NULL (the pooled term alone) the call is mgnns_imgbank_dgrad's and the workspace is not touched.
 * mgnns_label_attn_train_fwd: the label attention between its projections with dropout: Q [NLQ, H*dh], K = w_k(x), V = w_v(x)
 * [B, H*dh] -> x [B, NLQ, H*dh] = dropout(softmax_dh(Q K / sqrt(dh))) V, and for the backward P (softmax before dropout) and
 * keep (bytes), both [B, NLQ, H*dh].  dh <= 64.
 * mgnns_label_attn_train_bwd: its backward from dx: dQ [NLQ, H*dh] (summed over the batch in order), dK, dV [B, H*dh].
 * workspace: mgnns_label_attn_train_bwd_workspace_bytes(B, NLQ, H, dh) bytes.  B = 0: dQ is zeroed, and the per-sample
 * tensors (K, V, x, P, keep, dx, dK, dV) may be NULL.
 * mgnns_dropout_fwd / _bwd: y = dropout(x) at `site` (keep written as bytes); dx = dy keep / (1 - rate).
 * mgnns_dropout_mask: the keep mask of elements 0..n-1 of a site as bytes (what the training kernels draw for that seed).
 */
#define MGNNS_DROP_LABEL_ATTN 3
#define MGNNS_DROP_HEAD       4
size_t mgnns_imgbank_wgrad_workspace_bytes(int B, int K, int P, int N);
int mgnns_imgbank_wgrad(const float* X, const float* dbank, int B, int K, int P, int N, float* dW, float* db, void* workspace,
                        size_t workspace_bytes, mgnns_stream_t stream);
int mgnns_map_argmax(const float* X, int B, int K, int P, int32_t* arg, mgnns_stream_t stream);
int mgnns_imgbank_dgrad(const float* dbank, const float* W, const float* dpooled, const int32_t* arg, int B, int K, int P, int N,
                        float* dX, mgnns_stream_t stream);
size_t mgnns_imgbank_wgrad_split_workspace_bytes(int B, int K, int P, int N);
int mgnns_imgbank_wgrad_split(const float* X, const float* dbank, int B, int K, int P, int N, float* dW, float* db,
                              void* workspace, size_t workspace_bytes, mgnns_stream_t stream);
size_t mgnns_imgbank_dgrad_split_workspace_bytes(int B, int K, int P, int N);
int mgnns_imgbank_dgrad_split(const float* dbank, const float* W, const float* dpooled, const int32_t* arg, int B, int K, int P,
                              int N, float* dX, void* workspace, size_t workspace_bytes, mgnns_stream_t stream);
int mgnns_label_attn_train_fwd(const float* Q, const float* K, const float* V, int B, int NLQ, int H, int dh, uint64_t seed,
                               float rate, float* x, float* P, uint8_t* keep, mgnns_stream_t stream);
size_t mgnns_label_attn_train_bwd_workspace_bytes(int B, int NLQ, int H, int dh);
int mgnns_label_attn_train_bwd(const float* dx, const float* Q, const float* K, const float* V, const float* P,
                               const uint8_t* keep, int B, int NLQ, int H, int dh, float rate, float* dQ, float* dK, float* dV,
                               void* workspace, size_t workspace_bytes, mgnns_stream_t stream);

/* ---- training mode of the text encoders (fp32): the packed 2-layer BiLSTM and the text GCN ----------------------------------
 * Two more dropout sites: 5 = the BiLSTM's inter-layer dropout on layer 0's output, index (b*T + t)*2H + j over [B, T, 2H];
 * 6 = the text GCN's dropout before its ReLU, index b*D + d over [B, D].
 * mgnns_bilstm_train_fwd: the eval forward (mgnns_bilstm_fwd, fp32 recurrence; bit for bit its bank at rate 0) with dropout(rate) at
 * site 5 between the layers, keeping for the backward: meta (int32: offs [B+1] | order [B+8] | pack_tok [B*T] | pack_pos [B*T]),
 * gates [num_layers][2][rows_cap][4H] (after the activations) and cells [num_layers][2][rows_cap][H] at row offs[b] + t,
 * mid / mid_drop [B, T, 2H] (layer 0's output before / after the dropout; unused with one layer).  rows_cap >= sum of the
 * clamped lengths.  workspace: mgnns_bilstm_train_workspace_bytes(B, T, hidden) bytes.
 * mgnns_bilstm_train_bwd_rec: one layer's backward recurrence from dout [B, T, 2H] -> dz [rows, 2 * 4H] (pre-activation gate
 * gradients, forward direction then reverse, row offs[b] + t); gates / cells: that layer's slices.
 * mgnns_bilstm_train_hprev: hprev [rows, 2H] = each packed step's recurrent input (forward: h at t-1, reverse: h at t+1, 0 at
 * a chain's first step) from a layer output hout [B, T, 2H].
 * mgnns_bilstm_train_unpack_drop: dout[pack_pos[r], :] = dx[r, :] through the site-5 mask (dout zeroed by the caller).
 * mgnns_gather_rows: dst[r, :] = src[idx[r], :] (r < M).
 * mgnns_keyed_row_sum: out[k, :] = sum of values[perm[r], :] over the sorted run of key k, in sorted order (a stable sort
 * makes the result deterministic); keys below skip_below and at or past K add nothing; rows of out without a key are left
 * as the caller set them.
 * mgnns_textgcn_train_fwd: mgnns_textgcn_fwd with dropout(rate) at site 6 before the ReLU; presum [B, D] (before the dropout) and
 * win [B, min(T, max_length), D] int16 (the source position of the winning in-edge, written at the first position of each
 * node) for the backward.  Tie rule: the smallest source position whose fp32 product equals the fp32 max.
 * mgnns_textgcn_train_bwd: from dy [B, D] the per-document partials: R [B, Tm, D] rows keyed by keyR [B, Tm] (the token id of
 * the source, -1 = none) for node_hidden; Eg [B, Tm, 2 ngram + 1] keyed by keyE (edge id, -1 = none) for seq_edge_w.
 * mgnns_textgcn_train_supported: whether a training step takes the shape (a host function, 1 / 0): D in 1..320, ngram in 0..15,
 * Tm (2 ngram + 1) < 32768 and the BACKWARD's LDS need at Tm = min(T, max_length) -- Tm (28 (2 ngram + 1) + 12) + 16 bytes -- within
 * 160 KiB (Tm <= 4095 at ngram 0, 186 at ngram 15).  mgnns_textgcn_train_fwd requires it, so a step that could not finish is refused
 * before anything is launched (added under ABI 26 without a bump: an addition).
 */
#define MGNNS_DROP_LSTM       5
#define MGNNS_DROP_TEXT_GCN   6
size_t mgnns_bilstm_train_workspace_bytes(int B, int T, int hidden);
int mgnns_bilstm_train_fwd(const int64_t* tok, const int64_t* lens, int B, int T, const float* emb_table, int V, int emb_dim,
                           int hidden, int num_layers, const float* const* w_ih_cat, const float* const* b_ih_cat,
                           const float* const* w_hh, const float* const* b_hh, uint64_t seed, float rate, int32_t* meta,
                           int rows_cap, float* gates, float* cells, float* mid, float* mid_drop, float* out, void* workspace,
                           size_t workspace_bytes, mgnns_stream_t stream);
int mgnns_bilstm_train_bwd_rec(const float* dout, const int64_t* lens, int B, int T, const int32_t* meta, int rows_cap,
                               const float* gates, const float* cells, const float* w_hh_f, const float* w_hh_r, float* dz,
                               mgnns_stream_t stream);
int mgnns_bilstm_train_hprev(const float* hout, const int64_t* lens, int B, int T, const int32_t* meta, int rows_cap, float* hprev,
                             mgnns_stream_t stream);
int mgnns_bilstm_train_unpack_drop(const float* dx, const int32_t* pack_pos, int64_t M, int B, int T, uint64_t seed, float rate,
                                   float* dout, mgnns_stream_t stream);
int mgnns_gather_rows(const float* src, int n_src, int K, const int32_t* idx, int64_t M, float* dst, mgnns_stream_t stream);
int mgnns_keyed_row_sum(const int64_t* sorted_keys, const int64_t* perm, int64_t M, const float* values, int D, int64_t n_values,
                        int64_t skip_below, float* out, int64_t K, mgnns_stream_t stream);
int mgnns_textgcn_train_supported(int T, int D, int ngram, int max_length);
int mgnns_textgcn_train_fwd(const int64_t* tok, int B, int T, const float* node_hidden, int V, int D, const float* edge_w,
                            int n_edge_w, const int32_t* pmi_row_ptr, const int32_t* pmi_col, const int32_t* pmi_eid, int ngram,
                            int max_length, uint64_t seed, float rate, float* out, float* presum, int16_t* win,
                            mgnns_stream_t stream);
int mgnns_textgcn_train_bwd(const int64_t* tok, int B, int T, const float* node_hidden, int V, int D, const float* edge_w,
                            int n_edge_w, const int32_t* pmi_row_ptr, const int32_t* pmi_col, const int32_t* pmi_eid, int ngram,
                            int max_length, uint64_t seed, float rate, const float* dy, const float* presum, const int16_t* win,
                            float* R, int32_t* keyR, float* Eg, int32_t* keyE, mgnns_stream_t stream);
int mgnns_dropout_fwd(const float* x, int64_t n, uint64_t seed, int site, float rate, float* y, uint8_t* keep,
                      mgnns_stream_t stream);
int mgnns_dropout_bwd(const float* dy, const uint8_t* keep, int64_t n, float rate, float* dx, mgnns_stream_t stream);
int mgnns_dropout_mask(uint64_t seed, int site, float rate, int64_t n, uint8_t* keep, mgnns_stream_t stream);

/* ---- dense bf16 GEMM (BASELINE configs[4] (i): dense [N,N] adjacency x support on the bf16 MFMA; any large X.W) ------
 * C[M,N] = act(A[M,K] . Bt[N,K]^T + bias): A and Bt are bf16 with K-contiguous rows of Kp elements (Kp % 64 == 0, zero
 * padded: build A with mgnns_cast_pad_bf16, Bt from a [K,N] fp32 matrix with mgnns_transpose_cast_bf16), C fp32
 * (c_bf16 = 0) or bf16 (c_bf16 = 1: the K-contiguous operand of the next product, no cast pass) with row stride ldc
 * elements.  N % 4 == 0, ldc % 4 == 0.  UTIL:421-426 (`adj @ support`), MODEL:52-58.
 */
int mgnns_transpose_cast_bf16(const float* x, int rows, int cols, int ld, void* y, mgnns_stream_t stream);
/* workspace (optional, mgnns_gemm_bf16_workspace_bytes() bytes, 16-byte aligned, one per concurrently running launch): with it, a
 * last PARTIAL round of tiles on the persistent workgroups (10 000 x 1024 on 256 compute units: 320 tiles of 256 x 128 = 1.25 rounds)
 * is cut along K over the idle workgroups, partial sums go to the workspace and a second, small launch on the same stream adds a
 * tile's parts in part order (deterministic: no counters, nobody waits) and stores C; and products with K >= 4096 and at least one
 * full round of 256 x 256 tiles per XCD run the 256 x 256-tile kernel (a third less L2 traffic per MAC), whose left-over tiles are
 * cut the same way.  NULL: every tile is computed whole by the 256 x 128 kernel. */
size_t mgnns_gemm_bf16_workspace_bytes(void);
/* c_bf16 (round 6: two bits): bit 0 = C is bf16 (else fp32); bit 1 = TRANSPOSED store: C is C^T [N, ldc >= M] (a product with a small M runs as
 * its transpose and still leaves the K-contiguous operand the next product needs; the 160 x 256 kernel only: ceil(M / 160) >= 8, N >= 256, K >= 320).
 * M == 0: nothing is launched, A and C may be NULL. */
int mgnns_gemm_bf16_nt_fwd(const void* A, const void* Bt, int M, int N, int Kp, const float* bias, void* C, int ldc,
                           int c_bf16, int act, void* workspace, size_t workspace_bytes, mgnns_stream_t stream);
/* Which tile shape mgnns_gemm_bf16_nt_fwd runs (tests and A/B timings; production leaves it alone; process-wide): 0 round 4's kernels
 * only (256 x 128, 256 x 256), 1 the 160 x 256 kernel whenever the shape fits it, 2 by the launcher's estimate (the default),
 * 3 the 320 x 256 kernel whenever the shape fits it; -1 = back to the default. */
int mgnns_gemm_bf16_set_form(int form);
/* The launcher's choice for a product, by its estimate (host arithmetic, no device call; n_cu = compute units of the device, 256 on
 * MI355X; with_workspace: the workspace of mgnns_gemm_bf16_workspace_bytes() is passed): 4 = 160 x 256 tiles, 5 = 320 x 256 tiles,
 * 0 = round 4's kernels (256 x 128, or 256 x 256 for K >= 4096 with at least a full round of tiles per XCD); < 0 = bad arguments. */
int mgnns_gemm_bf16_pick_form(int M, int N, int Kp, int with_workspace, int n_cu);

/* ---- f4 (metrics half): the evaluation tail after the logits (ENGINE:828-838) -------------------------------------
 * probs = softmax(logits, dim=1) (max-subtracted), pred = first arg-max of probs; when target (int64 [B]) and
 * confusion (int32 [NL, NL], rows = target, columns = prediction; ACCUMULATED, zero it per epoch) are given the batch
 * is added to the confusion matrix, from which accuracy and the micro / macro / weighted F1 of the engine follow
 * (mgnns_amd/metrics.py).  probs, pred, target + confusion may each be NULL.  NL <= 64.
 */
int mgnns_softmax_argmax_fwd(const float* logits, int B, int NL, float* probs, int32_t* pred, const int64_t* target,
                             int32_t* confusion, mgnns_stream_t stream);

/* ---- f4 (trunk half): torchvision-style ResNet trunks cut after layer4 (MODEL:274-294 `object_features` /
 * `place_features`, MODEL:586-595, 629-630), eval mode.  Activations NHWC bf16, fp32 accumulation.
 *  mgnns_conv_fold_bn_bf16   one-off: wt[o, k] = bf16(w[o,c,kh,kw] * gamma[o] / sqrt(var[o] + eps)) with k = (kh, kw, c)
 *                            (k_order 0, rows of ld >= KH*KW*Cin elements, zero padded) or k = (c, kh, kw) (k_order 1: the
 *                            stem, ld = 160); bias[o] = beta[o] + (conv_bias[o] - mean[o]) * scale.  gamma == NULL: no
 *                            BatchNorm (scale 1, bias = conv_bias or 0); conv_bias may be NULL.
 *  mgnns_stem_conv7_fwd      conv1 (7x7, stride 2, pad 3, 3 -> 64) + bn1 + ReLU: img [B,3,H,W] fp32 NCHW ->
 *                            y [B, H/2, W/2, 64] bf16 NHWC (OH = (H - 1) / 2 + 1).
 *  mgnns_maxpool3x3s2_nhwc_fwd  MaxPool2d(3, 2, 1): [B,H,W,C] -> [B,(H-1)/2+1,(W-1)/2+1,C], C % 8 == 0.
 *  mgnns_conv_bf16_nhwc_fwd  y = relu?(conv(x; wt) + bias + residual?) as an implicit GEMM: 1x1 or 3x3, any stride,
 *                            pad <= K/2, Cin a power of two >= 64, Cout % 8 == 0; residual [B,OH,OW,Cout] bf16 or NULL;
 *                            y [B,OH,OW,Cout] bf16, or -- out_nchw_f32 != 0 -- [B,Cout,OH,OW] fp32, the feature-map
 *                            layout mgnns_imgbank_pool_* read.
 *  B == 0 (the three forward entries above and mgnns_stem_conv7_raw_fwd): nothing is launched, and the activations (img / x / y / z)
 *  may be NULL -- an empty tensor has no address; the arguments are validated all the same.
 */
int mgnns_conv_fold_bn_bf16(const float* w, const float* conv_bias, int Cout, int Cin, int KH, int KW,
                            const float* gamma, const float* beta, const float* mean, const float* var, float eps,
                            int k_order, int ld, void* wt, float* bias, mgnns_stream_t stream);
int mgnns_stem_conv7_fwd(const float* img, int B, int H, int W, const void* wt, const float* bias, void* y,
                         mgnns_stream_t stream);
int mgnns_maxpool3x3s2_nhwc_fwd(const void* x, int B, int H, int W, int C, void* y, mgnns_stream_t stream);
int mgnns_conv_bf16_nhwc_fwd(const void* x, int B, int H, int W, int Cin, const void* wt, const float* bias, int Cout,
                             int KH, int KW, int stride, int pad, const void* residual, int relu, int out_nchw_f32,
                             void* y, mgnns_stream_t stream);

/* ---- f4 (trunk half, training; ABI 26): backward of the bottleneck convolutions for frozen-statistics fine-tuning
 * (csrc/conv_train.hip).  The forward is mgnns_conv_bf16_nhwc_fwd on the folded weights; these give its gradients on the bf16
 * matrix pipe with fp32 accumulation.  Geometry of all of them: 1x1 or 3x3, stride 1 or 2, pad <= k/2, C_in and C_out powers of
 * two >= 64; H, W are the extents of the convolution's INPUT, OH = (H + 2 pad - k) / stride + 1.  Operands 16-byte aligned.
 * Nothing uses float atomics: results are bit-identical from call to call.
 *  mgnns_conv_transpose_pack_bf16   the data gradient's derived pack: wT[c, (kh, kw, o)] = wt[o, (kh, kw, c)] (bf16, any dims).
 *  mgnns_conv_dgrad_bf16_nhwc       dx[b,ih,iw,c] = sum over (kh,kw,o) with oh*s - p + kh == ih, ow*s - p + kw == iw of
 *                                   dy[b,oh,ow,o] * wT[c,(kh,kw,o)]; then dx = mask > 0 ? dx + add : 0, rounded to bf16 once.
 *                                   dy [B,OH,OW,C_out], dx / mask / add [B,H,W,C_in], all bf16 NHWC; mask, add may be NULL.
 *                                   Input pixels no output pixel reads (stride 2) get exactly add (or 0).
 *  mgnns_conv_wgrad_bf16_nhwc       dW[o,(kh,kw,c)] = sum over output pixels m of dy[m,o] * x[pixel(m,kh,kw),c] (padding taps
 *                                   contribute zero), db[o] = sum_m dy[m,o]; x, dy bf16 NHWC, dW [C_out, k*k*C_in] and db fp32.
 *                                   The pixels are split into shares across workgroups, written to `workspace`
 *                                   (mgnns_conv_wgrad_workspace_bytes bytes, may be 0 / NULL for a single share) and added in
 *                                   share order.  B == 0 zeroes the outputs.
 *  mgnns_conv_bn_unfold             from dWp / dbp (the gradients of the FOLDED weight and bias), the fp32 w [C_out,C_in,KH,KW] and
 *                                   the BatchNorm's gamma, running mean / var, eps, with r = 1 / sqrt(var + eps):
 *                                   dW[o,c,kh,kw] = gamma[o] r[o] dWp[o,(kh,kw,c)], dgamma[o] = r[o] (sum_k w[o,k] dWp[o,k] -
 *                                   mean[o] dbp[o]), dbeta[o] = dbp[o]; each of dW, dgamma, dbeta may be NULL.
 *  mgnns_map_grad_relu_nhwc_bf16    the entry of the chain: g[b,p,c] = bf16(map[b,c,p] > 0 ? dmap[b,c,p] : 0) from the fp32
 *                                   NCHW map the last convolution wrote and its gradient; C % 8 == 0.
 */
int mgnns_conv_transpose_pack_bf16(const void* wt, int Cout, int Cin, int KH, int KW, void* wT, mgnns_stream_t stream);
int mgnns_conv_dgrad_bf16_nhwc(const void* dy, int B, int H, int W, int Cin, const void* wT, int Cout, int KH, int KW,
                               int stride, int pad, const void* mask, const void* add, void* dx, mgnns_stream_t stream);
size_t mgnns_conv_wgrad_workspace_bytes(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad);
int mgnns_conv_wgrad_bf16_nhwc(const void* x, const void* dy, int B, int H, int W, int Cin, int Cout, int KH, int KW,
                               int stride, int pad, float* dW, float* db, void* workspace, size_t workspace_bytes,
                               mgnns_stream_t stream);
int mgnns_conv_bn_unfold(const float* dWp, const float* dbp, const float* w, const float* gamma, const float* mean,
                         const float* var, float eps, int Cout, int Cin, int KH, int KW, float* dW, float* dgamma,
                         float* dbeta, mgnns_stream_t stream);
int mgnns_map_grad_relu_nhwc_bf16(const float* map, const float* dmap, int B, int C, int P, void* g, mgnns_stream_t stream);

/* ---- f4 (trunk half, training with batch statistics): BatchNorm as a training operator (csrc/bn_train.hip).  Added under ABI 26
 * without a bump: the change is additive -- no existing signature or behaviour moves, and a binding that does not know these
 * names is unaffected.  z, g, residual, y, gz are [M, C] views of NHWC bf16 activations (M = B*OH*OW >= 2, C % 8 == 0, 16-byte
 * aligned); mean, rstd, var, gamma, beta, the running buffers, dgamma, dbeta are fp32 [C].  Every reduction over rows goes through
 * per-slab partials in `workspace` that are added in slab order (slabs are a function of (M, C) alone); no float atomics:
 * results are bit-identical from call to call.
 *  mgnns_bn_stats_bf16     mean[c] and rstd[c] = 1 / sqrt(var_biased[c] + eps) of the stored bf16 z, from per-slab (mean, M2) about
 *                          local centres (never E[z^2] - mean^2); var (may be NULL) receives var_biased.  With running_mean /
 *                          running_var (both or neither) the same launch updates them in place: running_mean = (1 - momentum)
 *                          running_mean + momentum mean, running_var = (1 - momentum) running_var + momentum var_biased M / (M - 1).
 *  mgnns_bn_apply_bf16     y = relu?(a z + b + residual?), a = gamma rstd, b = beta - mean a in fp32, one rounding to bf16 [M, C];
 *                          with out_nchw_f32 the unrounded fp32 map [M / P, C, P] instead (P = OH*OW pixels per image; else unused).
 *  mgnns_bn_backward_bf16  with xhat = (z - mean) rstd: dbeta = sum g, dgamma = sum g xhat (each may be NULL: not returned), and
 *                          gz = bf16(gamma rstd (g - dbeta / M - xhat dgamma / M)), always.
 */
size_t mgnns_bn_stats_workspace_bytes(int M, int C);
int mgnns_bn_stats_bf16(const void* z, int M, int C, float eps, double momentum, float* mean, float* rstd, float* var,
                        float* running_mean, float* running_var, void* workspace, size_t workspace_bytes,
                        mgnns_stream_t stream);
int mgnns_bn_apply_bf16(const void* z, int M, int C, const float* mean, const float* rstd, const float* gamma,
                        const float* beta, const void* residual, int relu, int out_nchw_f32, int P, void* y,
                        mgnns_stream_t stream);
size_t mgnns_bn_backward_workspace_bytes(int M, int C);
int mgnns_bn_backward_bf16(const void* g, const void* z, int M, int C, const float* mean, const float* rstd,
                           const float* gamma, void* gz, float* dgamma, float* dbeta, void* workspace,
                           size_t workspace_bytes, mgnns_stream_t stream);

/* ---- f4 (trunk half, training): the stem -- conv1 7x7 / stride 2 / pad 3 (3 -> 64) and MaxPool2d(3, 2, 1) -- so that a trunk
 * fine-tunes end to end (csrc/stem_train.hip).  Added under ABI 26 without a bump, as the BatchNorm entries were:
 * the change is additive.  OH = (H - 1) / 2 + 1 throughout.  No float atomics: results are bit-identical from call to call.
 *  mgnns_stem_conv7_raw_fwd     z = conv1(bf16(img); wt) alone, no bias and no ReLU: img [B,3,H,W] fp32 NCHW -> z [B,OH,OW,64] bf16
 *                               NHWC; wt the stem pack of mgnns_conv_fold_bn_bf16 (k_order 1, ld 160) built with gamma == NULL.
 *                               mgnns_stem_conv7_fwd is the same kernel with its bias + ReLU epilogue and is unchanged.
 *  mgnns_stem_wgrad             dW[o,(kh,kw,c)] = sum over (b,oh,ow) of g[b,oh,ow,o] * bf16(img[b,c,2 oh + kh - 3,2 ow + kw - 3])
 *                               (zero outside the image; the image rounded as the forward rounds it), db[o] = sum g[b,oh,ow,o];
 *                               img [B,3,H,W] fp32, g [B,OH,OW,64] bf16 NHWC, dW [64,147] and db [64] fp32.  dW is in the order
 *                               mgnns_conv_bn_unfold reads.  Workgroups write one partial each to `workspace`
 *                               (mgnns_stem_wgrad_workspace_bytes bytes, a function of the shape alone; always needed when
 *                               B > 0) and a second launch adds them in order.  B == 0 zeroes the outputs.
 *  mgnns_maxpool3x3s2_nhwc_bwd  backward of mgnns_maxpool3x3s2_nhwc_fwd: x [B,H,W,C] (the pool's input) and gy [B,OH,OW,C] ->
 *                               gx [B,H,W,C], all bf16 NHWC, C % 8 == 0.  A pixel receives gy of every window whose FIRST
 *                               maximum (row-major scan, strict >; torch's rule) it is; the sum is fp32 and rounded once.
 *                               relu_mask != 0 zeroes gx where x <= 0.  x must hold no NaN.
 */
int mgnns_stem_conv7_raw_fwd(const float* img, int B, int H, int W, const void* wt, void* z, mgnns_stream_t stream);
size_t mgnns_stem_wgrad_workspace_bytes(int B, int H, int W);
int mgnns_stem_wgrad(const float* img, const void* g, int B, int H, int W, float* dW, float* db, void* workspace,
                     size_t workspace_bytes, mgnns_stream_t stream);
int mgnns_maxpool3x3s2_nhwc_bwd(const void* x, const void* gy, int B, int H, int W, int C, int relu_mask, void* gx,
                                mgnns_stream_t stream);

/* ---- f4 (input half): the reference's image transforms in front of the trunks (utils/util.py:67-146 Warp / MultiScaleCrop,
 * then RandomHorizontalFlip, ToTensor, Normalize; csrc/image_prep.hip).  Added under ABI 26 without a bump: the
 * change is additive.  One launch turns a batch of decoded uint8 images of DIFFERENT sizes into the fp32 [B,3,S_h,S_w] tensor
 * mgnns_stem_conv7_fwd reads: crop -> Pillow's 8-bit BILINEAR resize (integer arithmetic: horizontal pass over every source
 * row into uint8, then the vertical pass, each clip8((2^21 + sum k_j * pixel_j) >> 22)) -> mirror -> lut[c][v].  Integer
 * accumulation in a fixed order and no atomics: results are bit-identical from call to call.
 *  pixels      packed uint8 HWC (3 channels) images; pixel_bytes = size of the buffer.  Every image starts on a 16-byte boundary
 *              and ends at least 16 bytes before the end of the buffer (rows are fetched with 16-byte loads).
 *  desc        [B,10] int64 per image: byte offset, source height, source width, crop x, crop y, crop width, crop height,
 *              flip (0 / 1), index of the horizontal plan, index of the vertical plan.  1 <= height, width <= 8192; the crop
 *              lies inside the image.  The kernel re-checks a descriptor and fills the image's output with NaN if it is bad
 *              (the host wrapper refuses it before the launch; a descriptor buffer can change under a captured graph).
 *  plan_table  [n_plans,4] int32 per plan: offset into plan_data (in int32s), taps per output (ksize), input extent, output
 *              extent.  plan_data at that offset: (first source index, tap count) per output, then ksize int32 taps per
 *              output (22 fractional bits; Pillow's precompute_coeffs + normalize_coeffs_8bpc, built in float64 on the host).
 *              A horizontal plan's extents are (crop width, S_w), a vertical plan's (crop height, S_h).
 *  lut         [3,256] fp32: (v / 255 - mean_c) / std_c as torch computes it.
 *  out         [B,3,S_h,S_w] fp32, 1 <= S_h, S_w <= 1024.  B == 0 is a no-op.
 */
int mgnns_image_prep_fwd(const void* pixels, size_t pixel_bytes, const int64_t* desc, int B, const int32_t* plan_table,
                         int n_plans, const int32_t* plan_data, size_t plan_ints, const float* lut, int S_h, int S_w,
                         float* out, mgnns_stream_t stream);

/* ---- f4 (file half): baseline JPEG files -> the packed RGB8 pixel buffer above, bit for bit what Pillow / libjpeg-turbo decode
 * (csrc/jpeg_parse.hpp, jpeg_entropy.hpp, jpeg_pixels.hpp, jpeg_decode.hip).  Added under ABI 26 without a bump: the
 * change is additive.
 *
 * The parser is host code and makes no GPU call.  It fills, for one file:
 *  info    24 int32: reason code (0 = accepted; the MG_JPEG_* codes of csrc/jpeg_parse.hpp), detail, width, height, components,
 *          Y sampling h, v, quantisation-table id x 3, DC table id x 3, AC table id x 3, restart interval, restart markers found,
 *          independent segments (ceil(nMCU / Ri), or 1), MCUs per row, MCU rows.
 *  range   2 int64: [begin, end) of the entropy-coded data.
 *  seg     [seg_cap][2] int64: byte range of every independent segment, as many as fit (info says how many there are).
 *  tables  the tables in use as the kernels read them (the size getter's bytes, csrc/jpeg_entropy.hpp MgJpegTables): four 8-bit
 *          quantisation tables in natural order, then four DC and four AC decoding tables (a 9-bit look-ahead table, maxcode,
 *          valoffset, huffval); unused ones are zero.
 * It always returns 0 for valid arguments: a file it refuses is a reason code, not an error.
 */
size_t mgnns_jpeg_tableset_bytes(void);
int mgnns_jpeg_parse(const void* data, size_t bytes, int max_extent, int32_t* info, int64_t* range, int64_t* seg, size_t seg_cap,
                     void* tables);

/* Decode a batch: `stages` is a mask of 1 = zero the coefficient workspace and Huffman-decode (one lane per segment), 2 =
 * dequantise + jidctint 8x8 ("islow") into component planes, 4 = "fancy" chroma upsampling + YCbCr -> RGB + crop into the pixel
 * buffer (7 = all; the split exists for measurements).  All launches go on `stream`; nothing synchronises.
 *  data      the files' bytes, anywhere in one buffer.
 *  img       [B,16] int64 per image: kind (1 = decode, 0 = its pixels are staged by the caller and it is skipped), width, height,
 *            components, Y sampling h, v, MCUs per row, MCU rows, quantisation / DC / AC table ids (one byte per component
 *            each), table set, offset of its coefficients (int16 elements, a multiple of 64), of its planes (bytes, a multiple
 *            of 64), of its pixels (bytes, a multiple of 16) and the end of its pixels' padding, which is zeroed (at most 256
 *            bytes behind the image).  Coefficients and planes hold the components one after the other at MCU-padded block counts.
 *  seg       [S,5] int64 per segment: image, [begin, end) in `data`, first MCU, MCUs.
 *  tables    n_sets table sets (above).
 *  status    [S] int32, one word per segment: 0 ok, 1 ran out of data, 2 invalid Huffman code, 3 coefficient index above 63,
 *            4 a record the kernel refused on its own check.  A status never stops a kernel; the caller reads the words.
 *  max_blocks / max_pixels   the largest block count (all components) and pixel count of a decoded image: they size the grids.
 * B <= 65535.  B == 0 or S == 0 is a no-op.
 */
int mgnns_jpeg_decode_fwd(const void* data, size_t data_bytes, const int64_t* img, int B, const int64_t* seg, int S,
                          const void* tables, int n_sets, void* coef, size_t coef_elems, void* planes, size_t plane_bytes,
                          void* pixels, size_t pixel_bytes, long long max_blocks, long long max_pixels, int stages,
                          int32_t* status, mgnns_stream_t stream);

/* ---- measurement aid: a one-thread kernel that writes the GPU's constant-rate real-time counter (s_memrealtime,
 * 100 MHz) into slots[idx] when the stream reaches it.  Captured into the forward's hipGraph it gives the REAL
 * timeline of the concurrent branches of a replay (rocprofv3 serialises / perturbs them): tools/graph_timeline.py.
 */
int mgnns_debug_stamp(uint64_t* slots, int idx, mgnns_stream_t stream);

/* Access-pattern measurement aid (tools/dev/slabcopy_exp.py): copy / read / write a [n_rows, pitch] byte matrix in pieces of
 * `piece` bytes dealt to XCDs the way the slab SpMM kernels deal their row segments (mode: 0 copy, 1 read, 2 write; +16 plain
 * instead of non-temporal stores; +256 ignore XCDs).  wgx = workgroups per XCD. */
int mgnns_debug_slabcopy(const void* src, void* dst, int n_rows, int pitch, int piece, int mode, int wgx,
                         mgnns_stream_t stream);

/* One thread that spins for `microseconds` of the same counter, then (slots != NULL) stamps slots[idx].  Used once per
 * process by mgnns_amd.streams to find HIP streams that sit on DIFFERENT hardware queues: a stamp on stream Y that lands
 * before the end of a spin on stream X proves X and Y do not share an in-order queue.
 */
int mgnns_debug_spin(int microseconds, uint64_t* slots, int idx, mgnns_stream_t stream);

/* ---- e: the forward's one collective -------------------------------------------------------------------------
 * The reference runs on one GPU (hard-coded cuda:0, Multi_GCN_Multihead_att.py:85,465,493; the DataParallel line at
 * engine/Multi_GCN_Multihead_Att_engine.py:365 is commented out).  Its eval forward has no cross-sample reduction, so the
 * batch shards over ranks with replicated weights and ONE all-gather of the [rows_local, num_labels] logits restores the
 * single-process result exactly.  RCCL (over xGMI inside a node) is bound at run time -- the instance the process already
 * carries (torch's) or the system librccl.so.1; MGNNS_ERR_UNSUPP if neither loads.
 *   one process per GPU:  rank 0 calls mgnns_comm_unique_id and ships the 128 bytes to the other ranks by any host channel
 *                         (a torch.distributed store, MPI, a file); every rank, with its device current, calls
 *                         mgnns_comm_init_rank (collective: returns when all ranks have joined);
 *   one process, n GPUs:  mgnns_comm_init_all(n, devices or NULL for 0..n-1, comms[n]); a single thread that issues the
 *                         all-gathers of several devices brackets them with mgnns_comm_group_start / _end.
 * mgnns_allgather_logits enqueues on `stream` (no host sync; capturable into a hipGraph); `all` is
 * [world * rows_local, num_labels] in rank order; every rank passes the same rows_local.
 */
int mgnns_comm_unique_id(void* id, size_t bytes /* >= 128 */);
int mgnns_comm_init_rank(int world, int rank, const void* id, size_t bytes, mgnns_comm_t* comm);
int mgnns_comm_init_all(int ndev, const int* devices, mgnns_comm_t* comms);
int mgnns_comm_info(mgnns_comm_t comm, int* world, int* rank);
int mgnns_allgather_logits(mgnns_comm_t comm, const float* local, int rows_local, int num_labels, float* all,
                           mgnns_stream_t stream);
int mgnns_comm_group_start(void);   /* one thread driving several communicators brackets its per-device all-gathers with these */
int mgnns_comm_group_end(void);
int mgnns_comm_destroy(mgnns_comm_t comm);

#ifdef __cplusplus
}
#endif
#endif /* MGNNS_HIP_H */
