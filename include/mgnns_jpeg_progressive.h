/* mgnns_jpeg_progressive.h -- extension of the C ABI of libmgnns_hip.so (include/mgnns_hip.h): progressive JPEG files.
 *
 * mgnns_hip.h is the surface of ABI 26 as it stood; entry points added to the library without an ABI bump are declared in an
 * extension header of their own, so that a caller built against mgnns_hip.h alone sees exactly what it saw.  The conventions are
 * mgnns_hip.h's: every int-returning entry point returns 0 or an MGNNS_ERR_* code with mgnns_last_error() set; size_t-returning
 * helpers give sizes of buffers the caller allocates.  mgnns_amd/_lib.py derives the ctypes binding of these entry points from this
 * file as it derives the others from mgnns_hip.h (_lib.EXTENSION_SIGNATURES / EXTENSION_SIZE_GETTERS).
 */
#ifndef MGNNS_JPEG_PROGRESSIVE_H
#define MGNNS_JPEG_PROGRESSIVE_H

#include "mgnns_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- f4 (file half), progressive files: SOF2, 8 bit, Huffman, the same component layouts, any legal progression script of at
 * most 32 scans (csrc/jpeg_parse.hpp, jpeg_progressive.hpp, jpeg_decode.hip; DESIGN.md 17, "Progressive files").  Added under ABI 26 without a bump:
 * the change is additive, and the entry points of mgnns_hip.h behave as before.
 *
 * The parser is host code and makes no GPU call.  A file that is not SOF2 gets the reason mgnns_jpeg_parse gives it (a baseline
 * file: reason 3 with detail 0xC0).  It fills, for one file:
 *  info    24 int32 as mgnns_jpeg_parse fills them; the table ids, the restart interval and the restart count are per scan here and stay zero; the
 *          segment count is that of all scans; [21] scans, [22] tables in the pool, [23] levels.  Further reasons: 14 incomplete
 *          progression (at EOI or the end of the file a coefficient has not reached Al = 0; detail = 64 component + coefficient),
 *          15 illegal progression (detail = the scan), 16 more than 32 scans.
 *  scans   [32][18] int64 in file order: components, component mask, Ss, Se, Ah, Al, restart interval in units (MCUs, or blocks of
 *          the scan's one component), level, pool index of the DC table of component 0, 1, 2 and of the AC table (-1 = none read),
 *          first segment, segments, units, begin and end of the entropy-coded data, restart markers found.  Scans of one level
 *          touch different (component, coefficient) pairs and may run at the same time; levels run in order.
 *  seg     [seg_cap][4] int64: begin, end, first unit, units of every independent segment, scan after scan; as many as fit.
 *  pool    96 tables of mgnns_jpeg_huff_bytes() each (csrc/jpeg_entropy.hpp MgJpegHuff): the distinct tables the scans read.
 *  quant   [3][64] uint8: per component, in natural order, the quantisation table in force at the component's first scan.
 */
size_t mgnns_jpeg_huff_bytes(void);
int mgnns_jpeg_parse_progressive(const void* data, size_t bytes, int max_extent, int32_t* info, int64_t* scans, int64_t* seg,
                                 size_t seg_cap, void* pool, void* quant);

/* Decode a batch that may mix baseline and progressive files: zero the workspace, mgnns_jpeg_decode_fwd's entropy kernel over the
 * S baseline segments, one launch of the progressive entropy kernel per level over that level's segments of all images, then the
 * IDCT and colour kernels over all images.  All launches go on `stream`; nothing synchronises.
 *  img       as for mgnns_jpeg_decode_fwd; kind 2 = progressive: the table ids are not read and the table-set field counts the latched quantisation
 *            sets (qsets) instead.
 *  seg       [S][5] baseline segments; tables / n_sets: their table sets (none: NULL, 0).
 *  pseg      [sum of level_counts][12] int64, sorted by level: image, begin, end, first unit, units, component mask, Ss, Se, Ah, Al,
 *            pool indices (16 bits each: DC of component 0, 1, 2, AC; 0xFFFF = none), the scan's number in its file.
 *  level_counts   HOST array [n_levels]: segments per level.  n_levels <= 64.
 *  pool      n_pool tables of mgnns_jpeg_huff_bytes() each; qsets: n_q sets of [3][64] uint8.
 *  status    [S + sum of level_counts] int32: the baseline segments' words, then the progressive ones' in pseg's order; the same
 *            five values (3: a coefficient index beyond Se).
 *  stages    the mask of mgnns_jpeg_decode_fwd: 1 = zero the workspace and run every entropy launch, 2 = IDCT, 4 = colour.
 */
int mgnns_jpeg_decode_progressive_fwd(const void* data, size_t data_bytes, const int64_t* img, int B, const int64_t* seg, int S,
                                      const void* tables, int n_sets, const int64_t* pseg, const int32_t* level_counts, int n_levels,
                                      const void* pool, int n_pool, const void* qsets, int n_q, void* coef, size_t coef_elems,
                                      void* planes, size_t plane_bytes, void* pixels, size_t pixel_bytes, long long max_blocks,
                                      long long max_pixels, int stages, int32_t* status, mgnns_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MGNNS_JPEG_PROGRESSIVE_H */
