/* imm_compose.h - C-ABI of the compose entry point of libimm_hip.so (ABI 26; imm_amd/csrc/compose.hip, imm_amd/generation.py
 * ImageGenerator.repose): generated faces pasted back into the caller's u8 photographs.  Included by imm_hip.h, whose conventions hold
 * here: plain pointers and sizes, an explicit hipStream_t as void*, int status (0 = ok) and imm_last_error(). */
#ifndef IMM_COMPOSE_H
#define IMM_COMPOSE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* photos: the packed u8 HWC buffer of imm_resize_crop_u8 (offsets int64 [n_images], hw int32 [n_images, 2], three channels), composited
 * IN PLACE.  boxes int32 [n, 5] rows (image, y0, x0, y1, x1), half-open, possibly reaching outside the photo (imm_amd.keypoints.check_boxes);
 * a row whose image index lies outside [0, n_images) writes nothing.  faces f32 [n, image_size, image_size] pixels of pixel stride
 * ld >= 3 floats, channels 0..2 read (the generator's prediction buffer is wider).  With S = image_size, ih = y1 - y0, iw = x1 - x0, the
 * rows are applied IN ROW ORDER; row b changes every photo pixel (r, c) inside both box b and the photo:
 *   fy = (r - y0) * sy,  sy = (float)((double)(S - 1) / (double)(ih - 1)), 0 when ih == 1; fx, sx likewise from c, x0, iw: the exact
 *        inverse of the crop's align-corners map, the identity at ih == S
 *   g  = the bilinear sample of faces[b] at (fy, fx): taps floor and min(floor + 1, S - 1), evaluated as a + (b - a) * t along x, then
 *        along y, every operation rounded separately (no fma), then clipped to [0, 255]
 *   a  = wy * wx,  wy = min(1, (min(r - y0, y1 - 1 - r) + 0.5) * inv_ramp[b][0]),  wx = min(1, (min(c - x0, x1 - 1 - c) + 0.5) *
 *        inv_ramp[b][1]).  inv_ramp f32 [n, 2] comes from the host: 1 / (feather * ih) and 1 / (feather * iw), or any value >= 2 where
 *        that product is <= 0.5 (then a == 1: a hard paste).  The device never divides by a ramp.
 *   photo[r, c] = rint(p + a * (g - p)), to nearest even, stored as u8 AFTER EVERY ROW: a later row blends over the rounded result of an
 *        earlier one, so the same rows issued as several launches, in order, give the bytes of one launch.
 * Pixels of no box, photos without a box and the padding between photos are not written; a box wholly outside its photo writes nothing.
 * Overlapping boxes of one photo give the row-order result without atomics: links int32 [n, 2] holds per row (the previous row of the
 * same photo in THIS launch, the next one), -1 for none (imm_amd.generation.compose_links).  A pixel belongs to the first row of the launch
 * that covers it; that row's thread walks the later rows of the photo, keeps the running value in a register with the per-row rounding
 * and is the pixel's only reader and writer.  A previous link must be smaller and a next link larger than its row: the walks stop at a
 * link that is not (or that lies outside [0, n)), whatever the buffer holds.
 * max_box_pixels > 0 sizes the grid: the largest ih * iw of the rows (clipped to the photo or not); a larger box is still composited
 * whole, by a grid-stride loop.  0 < n <= 65535, 0 < image_size <= 8192.  Every pointer is read at the launch only, so the call can
 * follow a captured render program on its stream; arguments are validated before any HIP call (-1 and imm_last_error()). */
int imm_compose_u8(uint8_t* photos, const int64_t* offsets, const int32_t* hw, int n_images, const int32_t* boxes,
                   const int32_t* links, const float* inv_ramp, const float* faces, int ld, int n, int image_size, int max_box_pixels,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IMM_COMPOSE_H */
