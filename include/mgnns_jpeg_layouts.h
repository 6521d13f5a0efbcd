/* mgnns_jpeg_layouts.h -- extension of the C ABI of libmgnns_hip.so (include/mgnns_hip.h): JPEG files of other component layouts.
 *
 * mgnns_hip.h is the surface of ABI 26 as it stood, mgnns_jpeg_progressive.h and mgnns_jpeg_split.h its first two extensions;
 * these entry points were added after them without an ABI bump and are declared in a header of their own, so that a caller built
 * against the earlier headers sees exactly what it saw.  The conventions are mgnns_hip.h's.  mgnns_amd/_lib.py derives the ctypes
 * binding of these entry points from this file as it derives the others from their headers (_lib.LAYOUT_SIGNATURES).
 */
#ifndef MGNNS_JPEG_LAYOUTS_H
#define MGNNS_JPEG_LAYOUTS_H

#include "mgnns_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- f4 (file half), other component layouts (csrc/jpeg_layouts.hpp, jpeg_decode.hip; DESIGN.md 17, "Other component layouts").
 * Added under ABI 26 without a bump: the change is additive, and the entry points of the earlier headers behave as before.
 *
 * mgnns_jpeg_parse_layout: mgnns_jpeg_parse for SOF0 / SOF1 files of 1, 3 or 4 components with sampling factors 1..4 that divide
 * the largest and at most 10 blocks per MCU -- CMYK, YCCK, RGB, 4:4:0, 4:1:1 and the like.  No GPU call.
 *  info     int32 [40]: reason, detail, width, height, components, hmax, vmax, h[4], v[4], tq[4], td[4], ta[4], restart interval,
 *           restart markers found, segments, MCUs per row, MCU rows, colour model (0 gray, 1 YCbCr, 2 RGB, 3 CMYK, 4 YCCK), the SOF
 *           marker, blocks per MCU.  Reasons are mgnns_jpeg_parse's, and 17 (a sampling factor that is no integral fraction of the
 *           largest) and 18 (a factor outside 1..4, or more than 10 blocks per MCU).
 *  range, seg, seg_cap, tables   as mgnns_jpeg_parse; segment j covers MCUs [j Ri, (j+1) Ri) of 8 hmax x 8 vmax pixels.
 */
int mgnns_jpeg_parse_layout(const void* data, size_t bytes, int max_extent, int32_t* info, int64_t* range, int64_t* seg, size_t seg_cap,
                            void* tables);

/* mgnns_jpeg_decode_layouts_fwd: mgnns_jpeg_decode_progressive_fwd (chunk_bytes = 0) or mgnns_jpeg_decode_split_fwd (chunk_bytes a
 * multiple of 8 in 8..65536) -- the same launches in the same order for the images of kind 0, 1 and 2 -- and behind them three
 * launches for the images of kind 3, which the earlier kernels skip: the layout entropy kernel, one lane per record of lseg (these
 * segments are never split over lanes); dequantisation + jidctint with one table per component; upsampling of every component to
 * the largest and the colour model -> RGB8 in `pixels`.  All launches go on `stream`; nothing synchronises.
 *  img      [B][16] int64.  A record of kind 3: 3, width, height, components | colour model << 8, h and v (a nibble per component),
 *           MCUs per row, MCU rows, quantisation / DC / AC table ids (a byte per component), table set, coefficient / plane / pixel
 *           offset, end of the padding.  Component c lies behind component c - 1 in the workspaces, mcux h_c blocks per block row.
 *  lseg     [L][5] int64: image, begin, end (bytes in `data`), first MCU, MCUs -- the layout of seg.
 *  max_blocks, max_pixels     over the images of kind 1 and 2, as before;  lmax_blocks, lmax_pixels  over those of kind 3.
 *  status   int32 [S + P + L]: the words of seg, of pseg, of lseg.  The same five values; a record the device refuses is 4 and
 *           nothing is written for it.
 */
int mgnns_jpeg_decode_layouts_fwd(const void* data, size_t data_bytes, const int64_t* img, int B, const int64_t* seg, int S,
                                  const void* tables, int n_sets, const int64_t* pseg, const int32_t* level_counts, int n_levels,
                                  const void* pool, int n_pool, const void* qsets, int n_q, const int64_t* lseg, int L, void* coef,
                                  size_t coef_elems, void* planes, size_t plane_bytes, void* pixels, size_t pixel_bytes,
                                  long long max_blocks, long long max_pixels, long long lmax_blocks, long long lmax_pixels, int stages,
                                  int32_t* status, mgnns_stream_t stream, int chunk_bytes);

#ifdef __cplusplus
}
#endif

#endif /* MGNNS_JPEG_LAYOUTS_H */
