/* imm_unalign.h - C-ABI of the unalign entry points of libimm_hip.so (ABI 27; imm_amd/csrc/unalign.hip, imm_amd/inference.py
 * LandmarkDetector.unalign, imm_amd/generation.py ImageGenerator.repose with a template): aligned faces pasted back into the caller's
 * u8 photographs through the inverse of their alignment maps.  Included by imm_hip.h, whose conventions hold here: plain pointers and
 * sizes, an explicit hipStream_t as void*, int status (0 = ok) and imm_last_error().
 *
 * THE PIXEL RULE
 *
 * Backward map.  For row b, imm_align_warp_u8 takes aligned pixel (i, j) of the So x So output to source pixel s of the photo, from
 * coef[b] f32 [3][2] (rows 1, q_y, q_x; columns y, x), geom[b] = (y0, x0, sy, sx), image_size = S and out_size = So.  For the
 * similarity and affine models (m3 == 3) that map is affine, s = B (i, j) + t:
 *     B[a][0] = geom[2 + a] * S * coef[1][a] / So
 *     B[a][1] = geom[2 + a] * S * coef[2][a] / So
 *     t[a]    = geom[a] + geom[2 + a] * S / 2 * (coef[0][a] + 1 - coef[1][a] - coef[2][a])           a = 0 (y), 1 (x)
 * Forward map.  Photo pixel (r, c) to aligned coordinate: (fi, fj) = B^-1 ((r, c) - t), stored per row as six floats
 * m00 m01 m02 m10 m11 m12 (fi = m00 r + m01 c + m02).
 *
 * Paste of row b at photo pixel (r, c).  All arithmetic is f32, every operation rounded separately (no fma):
 *   fi = (m00 * r + m01 * c) + m02,  fj = (m10 * r + m11 * c) + m12.  The pixel is COVERED iff 0 <= fi <= So - 1 and 0 <= fj <= So - 1;
 *        a NaN map covers nothing.
 *   g  = the bilinear sample of faces[b] at (fi, fj): taps floor and min(floor + 1, So - 1), evaluated as a + (b - a) * t along x, then
 *        along y (as imm_compose_u8 forms it), then clipped to [0, 255]
 *   a  = wy * wx,  wy = min(1, (min(fi, (So - 1) - fi) + 0.5) * inv_ramp),  wx likewise from fj.  inv_ramp comes from the host:
 *        1 / (feather * So), or any value >= 2 where feather * So <= 0.5 (then a == 1: a hard paste).  The device never divides by a
 *        ramp.
 *   photo[r, c] = rint(p + a * (g - p)), to nearest even, stored as u8 AFTER EVERY ROW, in row order: a later row blends over the
 *        rounded result of an earlier one, so the same rows issued as several launches, in order, give the bytes of one launch.
 * Overlapping rows of one photo use the links of imm_compose_u8 (int32 [n, 2]: per row the previous row of the same photo in THIS
 * launch and the next one, -1 for none; imm_amd.generation.compose_links over the rows' image indices).  A pixel belongs to the first
 * row of the launch that covers it; that row's thread walks the later rows of the photo, keeps the running value in a register with
 * the per-row rounding and is the pixel's only reader and writer.  No atomics.  "Covers" is the quad test above, evaluated with the
 * other row's map.  A previous link must be smaller and a next link larger than its row: the walks stop at a link that is not (or that
 * lies outside [0, n)), whatever the buffer holds.
 * Identity.  With an identity coef, geom = (y0, x0, 1, 1) and So == S the forward map is the exact translation fi = r - y0,
 * fj = c - x0, and pasting the float crop returns the photo bit for bit for every feather. */
#ifndef IMM_UNALIGN_H
#define IMM_UNALIGN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* fwd f32 [n][6] and bbox int32 [n][4] of n rows from the coefficients imm_align_coeffs wrote: coef f32 [n, 3, 2], geom f32 [n, 4],
 * boxes int32 [n, 5] (only the image index is read), hw int32 [n_images, 2].  One thread per row forms B and t and inverts in f64,
 * every operation rounded separately, in this order (k = (double)geom[2 + a] * S):
 *     B[a][0] = (k * coef[1][a]) / So,  B[a][1] = (k * coef[2][a]) / So,  t[a] = geom[a] + (k * 0.5) * (((coef[0][a] + 1) - coef[1][a]) - coef[2][a])
 *     det = B00 * B11 - B01 * B10;  m00 = B11 / det, m01 = -B01 / det, m10 = -B10 / det, m11 = B00 / det
 *     m02 = -(m00 * t0 + m01 * t1),  m12 = -(m10 * t0 + m11 * t1)
 * and rounds once to f32.  bbox is half-open (y0, x0, y1, x1): the four corners of [0, So - 1]^2 through B, t (corner (i, j) at
 * (B[a][0] * i + B[a][1] * j) + t[a]), floor(min) - 1 and ceil(max) + 2, clipped to the row's photo; (0, 0, 0, 0) when nothing is
 * left.  det == 0, a non-finite value or an image index outside [0, n_images) gives a NaN fwd and an empty bbox.
 * All pointers are read at the launch only: the call may follow imm_align_coeffs on its stream with no host round trip.
 * n > 0, n_images > 0, 0 < image_size <= 8192, 0 < out_size <= 8192; arguments are validated before any HIP call (-1 and imm_last_error()). */
int imm_unalign_maps(const float* coef, const float* geom, const int32_t* boxes, const int32_t* hw, int n_images, int n, int image_size,
                     int out_size, float* fwd, int32_t* bbox, void* stream);

/* The paste.  photos: the packed u8 HWC buffer of imm_resize_crop_u8 (offsets int64 [n_images], hw int32 [n_images, 2], three
 * channels), changed IN PLACE.  boxes int32 [n, 5]: only the image index of a row is used; a row whose index lies outside
 * [0, n_images) writes nothing.  fwd, bbox: what imm_unalign_maps wrote for these rows (bbox is clipped to the photo again; a pixel
 * outside it is not written by its row).  faces f32 [n, out_size, out_size] pixels of pixel stride ld >= 3 floats, channels 0..2 read
 * (the generator's prediction buffer can be read in place).  One thread per photo pixel of a row's bbox, the row in blockIdx.y;
 * max_pixels > 0 sizes the grid (the largest bbox area expected; larger ones are still pasted whole, by a grid-stride loop).
 * Pixels no row covers, photos without a row and the padding between photos are not written.  The photo accesses are byte-wide.
 * 0 < n <= 65535, 0 < out_size <= 8192, inv_ramp positive and finite.  Every pointer is read at the launch only; arguments are
 * validated before any HIP call (-1 and imm_last_error()). */
int imm_unalign_u8(uint8_t* photos, const int64_t* offsets, const int32_t* hw, int n_images, const int32_t* boxes, const int32_t* links,
                   const float* fwd, const int32_t* bbox, float inv_ramp, const float* faces, int ld, int n, int out_size, int max_pixels,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IMM_UNALIGN_H */
