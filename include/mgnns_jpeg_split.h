/* mgnns_jpeg_split.h -- extension of the C ABI of libmgnns_hip.so (include/mgnns_hip.h): restart-free JPEG scans on many lanes.
 *
 * mgnns_hip.h is the surface of ABI 26 as it stood and mgnns_jpeg_progressive.h its first extension; this entry point was added
 * after both without an ABI bump and is declared in a header of its own, so that a caller built against the earlier headers sees
 * exactly what it saw.  The conventions are mgnns_hip.h's.  mgnns_amd/_lib.py derives the ctypes binding of this entry point from
 * this file as it derives the others from their headers (_lib.SPLIT_SIGNATURES).
 */
#ifndef MGNNS_JPEG_SPLIT_H
#define MGNNS_JPEG_SPLIT_H

#include "mgnns_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- f4 (file half), split scans (csrc/jpeg_split.hpp, jpeg_decode.hip; DESIGN.md 17, "Split scans").  Added under ABI 26
 * without a bump: the change is additive, and the entry points of the earlier headers behave as before.
 *
 * mgnns_jpeg_decode_progressive_fwd with one difference: a baseline segment of at least 2 * chunk_bytes bytes (below 2^28) is
 * decoded by one WORKGROUP, a lane per chunk of its bytes, instead of one lane -- a restart-free scan is one segment, so this is
 * what gives such a file more than one lane.  The lanes decode speculatively, take over each other's exit states until nothing
 * changes, carry block numbers and DC predictors forward by prefix sums, and write; the coefficient workspace, the status words
 * (one per segment record, same order, same five values) and so the pixels are those of mgnns_jpeg_decode_progressive_fwd byte for
 * byte, for corrupt and truncated scans too.  Shorter segments take the one-lane kernel as before, progressive scans are not
 * split, and the progressive arguments may be empty (NULL / 0).  All launches go on `stream`; nothing synchronises.
 *  chunk_bytes   a multiple of 8 in 8..65536; with more chunks than the workgroup has lanes the chunk grows.
 */
int mgnns_jpeg_decode_split_fwd(const void* data, size_t data_bytes, const int64_t* img, int B, const int64_t* seg, int S,
                                const void* tables, int n_sets, const int64_t* pseg, const int32_t* level_counts, int n_levels,
                                const void* pool, int n_pool, const void* qsets, int n_q, void* coef, size_t coef_elems, void* planes,
                                size_t plane_bytes, void* pixels, size_t pixel_bytes, long long max_blocks, long long max_pixels,
                                int stages, int32_t* status, mgnns_stream_t stream, int chunk_bytes);

#ifdef __cplusplus
}
#endif

#endif /* MGNNS_JPEG_SPLIT_H */
