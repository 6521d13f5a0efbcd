/* mgnns_step.h -- extension of the C ABI of libmgnns_hip.so (include/mgnns_hip.h): the tail of a training step.
 *
 * Cross-entropy with its gradient, the global gradient norm and its clip coefficient, and a fused Adam update over a table of
 * chunks (csrc/step_tail.hip).  Added under ABI 26 without a bump: the change is additive, mgnns_hip.h and
 * the JPEG extension headers are as they were, and these entry points are declared in a header of their own with tables of
 * their own in mgnns_amd/_lib.py (STEP_SIGNATURES, STEP_SIZE_GETTERS).  The conventions are mgnns_hip.h's: every pointer is a
 * device address unless it says otherwise, every launch goes on `stream`, nothing synchronises, 0 is success.
 *
 * Every kernel is a plain launch and deterministic: the same inputs give the same bits.
 */
#ifndef MGNNS_STEP_H
#define MGNNS_STEP_H

#include "mgnns_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Elements of one chunk at most: a tensor of n elements is ceil(n / MGNNS_STEP_CHUNK) consecutive chunks. */
#define MGNNS_STEP_CHUNK 32768
/* Columns of the per-group scalar table (fp32): -(lr / bc1), sqrt(bc2), 1 - b1, b2, 1 - b2, eps, wd, (unused). */
#define MGNNS_STEP_GROUP_FLOATS 8
/* Largest NL mgnns_ce_loss_fwd_bwd takes. */
#define MGNNS_CE_MAX_NL 64

/* A chunk record is 40 bytes, little endian:
 *   uint64 p, g, m, v   addresses of the run's first element in the parameter, its gradient, exp_avg and exp_avg_sq (fp32; any
 *                       4-byte alignment: 16-byte accesses where the addresses allow, single elements where they do not)
 *   int32  n            elements of the run, 1..MGNNS_STEP_CHUNK (a record with another n is skipped)
 *   int32  group        row of the scalar table, or -1 for a run that only counts in the norm: mgnns_adam_step multiplies its g by
 *                       the coefficient in place and reads neither p, m nor v.  A record with any other row outside the table is skipped
 * The table is built and checked by the host (mgnns_amd/optim.py): the kernels trust its addresses.
 */
size_t mgnns_step_chunk_elems(void);                  /* MGNNS_STEP_CHUNK */
size_t mgnns_step_chunk_record_bytes(void);           /* 40 */
size_t mgnns_step_chunk_table_bytes(int n_chunks);    /* 40 * n_chunks; 0 for n_chunks < 0 */
size_t mgnns_step_group_table_bytes(int n_groups);    /* 4 * MGNNS_STEP_GROUP_FLOATS * n_groups; 0 for n_groups < 0 */
size_t mgnns_step_partials_bytes(int n_chunks);       /* 8 * n_chunks: one fp64 per chunk; 0 for n_chunks < 0 */

/* loss = mean over the live rows of -log softmax(logits[b])[target[b]], dlogits = (softmax - onehot) / n_live, one launch of one
 * workgroup.  The arithmetic is fp64 (exp, log, an ordered sum over the rows) and rounded once to fp32.
 *  logits [B, NL] fp32, target [B] int64, loss [1] fp32, dlogits [B, NL] fp32
 *  target -100 is ignored: a zero row that does not count; with no live row the loss is NaN (and every row of dlogits is zero)
 *  any other target outside [0, NL) makes the loss NaN and its own row NaN; nothing is read or written outside the row
 * 1 <= NL <= MGNNS_CE_MAX_NL and B >= 1, else MGNNS_ERR_UNSUPP.
 */
int mgnns_ce_loss_fwd_bwd(const float* logits, const int64_t* target, int B, int NL, float* loss, float* dlogits, mgnns_stream_t stream);

/* partial[c] = sum over chunk c of g * g in fp64 (the square of an fp32 value is exact there), a grid-stride loop over chunks. */
int mgnns_grad_sumsq(const void* chunks, int n_chunks, double* partial, mgnns_stream_t stream);

/* One workgroup: s = partial[0] + ... + partial[n_chunks - 1] in fp64 in a fixed order, out[0] = total_norm = (float)sqrt(s),
 * out[1] = clip_coef = c > 1 ? 1 : c with c = max_norm / (total_norm + 1e-6f) in fp32 (NaN stays NaN).  n_chunks = 0: norm 0, coefficient 1.
 */
int mgnns_grad_clip_coef(const double* partial, int n_chunks, float max_norm, float* out, mgnns_stream_t stream);

/* Adam over the chunk table, one pass: per element, with the row r = groups[group] and c = *clip_coef (read on the device),
 *   g = g * c;  if (wd != 0) g = g + wd * p;  m = m + (g - m) * (1 - b1);  v = v * b2 + ((1 - b2) * g) * g;
 *   p = p + (-(lr / bc1)) * (m / (sqrt(v) / sqrt(bc2) + eps))
 * every operation a separately rounded IEEE fp32 operation (no contraction), sqrt and / correctly rounded, denormals kept.
 * g is not written, except in the runs of group -1, which are only that: g = g * c.  Runs of different records must not overlap.
 *  groups [n_groups, MGNNS_STEP_GROUP_FLOATS] fp32, clip_coef [1] fp32 (pass a 1.0f for "no clipping")
 */
int mgnns_adam_step(const void* chunks, int n_chunks, const float* groups, int n_groups, const float* clip_coef, mgnns_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MGNNS_STEP_H */
