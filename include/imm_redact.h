/* imm_redact.h - C-ABI of redaction of libimm_hip.so (ABI 37; imm_amd/csrc/redact.hip, imm_amd/redaction.py, imm_amd/inference.py
 * LandmarkDetector.redact and redact_clip): faces pixelated or smoothed inside their u8 photos.  Every other paste of this library
 * turns a face into another face; this one makes it unreadable: the box is cut into square cells, every cell is replaced by the mean
 * of the ORIGINAL pixels it covers (a mosaic), or by the bilinear interpolation of those means (a blur).  The cells are anchored to the
 * box, not to the photo, so the mosaic travels with a tracked face instead of shimmering under it.  Included by imm_hip.h, whose
 * conventions hold here: plain pointers and sizes, an explicit hipStream_t as void*, int status (0 = ok) and imm_last_error().  The
 * packed buffers, the box rows (image, y0, x0, y1, x1), links and inv_ramp are those of imm_warp.h.
 *
 * THE RULE
 *
 * A row is ACTIVE when 0 <= image < n_images, H > 0 and W > 0, with H = y1 - y0, W = x1 - x0 in 64 bits.  With 1 <= blocks <= 64, all
 * in 64-bit integers (/ is integer division):
 *     cell = max(1, (max(H, W) + blocks - 1) / blocks)            square cells, at most `blocks` of them along the longer side
 *     gy = (H + cell - 1) / cell,  gx = (W + cell - 1) / cell     both <= blocks
 *
 * Cells (imm_redact_cells_u8).  Cell (i, j) of an active row b, 0 <= i < gy, 0 <= j < gx, covers the box-relative rows
 * [i * cell, min((i + 1) * cell, H)) and the columns [j * cell, min((j + 1) * cell, W)), intersected with the photo.  Per channel
 *     sum  = the integer sum of the bytes of src over those pixels,  cnt = their number
 *     mean = (2 * sum + cnt) / (2 * cnt)                          rounds half up, exact;  cnt == 0: mean = 0
 * cells u8 [n, blocks * blocks * 3]: row b's grid lies dense as [gy, gx, 3] at the start of its slice.  EVERY byte of the n slices is
 * written: the bytes past gy * gx * 3 are zeros, and so is the whole slice of a row that is not active.  The buffer is a function of
 * the inputs alone, in any reduction order (the sums are integers).
 *
 * Paste (imm_redact_u8).  The skeleton of the paste kernels (imm_warp.h): one owner per photo pixel, the rows of a photo applied in
 * row order along links, a rint after every row.  Row q covers photo pixel (r, c) when q is ACTIVE and y0 <= r < y1, x0 <= c < x1.
 * Per covered pixel, in f32, every operation rounded separately (no fma), in this order.  The replacement value g, per channel:
 *     mode IMM_REDACT_PIXELATE (0):  g = cells_b[((r - y0) / cell) * gx + (c - x0) / cell]                          integer division
 *     mode IMM_REDACT_SMOOTH   (1):  inv = (float)(1.0 / (double)cell)
 *                                    fy = ((float)(r - y0) + 0.5f) * inv - 0.5f,  fx likewise from c, x0
 *                                    g = the bilinear sample of cells_b, read as a u8 photo [gy, gx, 3], at (fy, fx):
 *                                        taps floor and floor + 1, each clamped to the grid; a + (b - a) * t along x, then along y
 * (a box-filter downsample followed by a bilinear upsample).  The weight:
 *     ramp = the edge ramp of imm_compose.h from inv_ramp[b]
 *     without a mask (edges == NULL):  a = ramp
 *     with the mask:  w = hull_flags[b] != 0 ? 1.f : the weight of imm_hull.h from edges[b], inv_soft[b], K
 *                     if !(w > 0) the row leaves the pixel alone;  a = ramp * w              one rounded product
 *     v <- fminf(fmaxf(rintf(v + a * (g - v)), 0), 255)           imm_compose.h's blend: the difference, the product, the sum
 * Fail closed.  Where imm_morph_hull_u8 writes nothing for a row whose hull is flagged, this kernel redacts the row's WHOLE box: a
 * row whose hull_flags is not 0 (an empty box, landmarks that are not finite, no hull with an inside: imm_hull_fit's bits; a face a
 * tracker lost arrives with NaN landmarks) takes w = 1 at every pixel.  The kernel asks only whether the flag is 0, so a caller folds
 * any verdict of its own into it: LandmarkDetector.redact_clip sets bit 2 for a face its quality gate finds unsure on a frame, the
 * first frame included, where the tracker keeps such a face.  A face the detector is unsure of is never shown.
 * cells, edges, inv_soft and hull_flags never reach an address: whatever they hold, only bytes inside covered pixels change.  Only dst
 * is read and written for pixels; the cells were taken from src, so the rows of one call give the same bytes however they are split
 * into launches, provided the cells of all rows come from the original.
 *
 * Consequences of the order of operations.  (a) With cell == 1 (blocks >= max(H, W)) both modes return the photo bit for bit for
 * every weight: a cell's mean is its one pixel, and in the smooth mode fy is the integer r - y0 itself and t = 0.  (b) A flat photo
 * comes back bit for bit: every mean is the photo's value and g - v = 0.  This holds in the pixelate mode for every box, and in the
 * smooth mode for every box all of whose cells hold a pixel (any box inside the photo): a cell that lies wholly outside the photo
 * has the mean 0, and the smooth mode's taps mix that 0 into the pixels of the cells next to it, which come out darker: a box that
 * hangs over the photo's edge blurs towards black there.  (c) Where a == 1 (feather 0 and no mask, or deep inside the hull) the byte
 * IS the cell's mean in the pixelate mode: no original pixel value survives except through a mean of cnt pixels.
 * (d) blocks == 1 fills the box with its own mean. */
#ifndef IMM_REDACT_H
#define IMM_REDACT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IMM_REDACT_PIXELATE 0
#define IMM_REDACT_SMOOTH 1
#define IMM_REDACT_MAX_BLOCKS 64

/* The cell means.  src u8 (the packed photos), offsets int64 [n_images], hw int32 [n_images, 2], boxes int32 [n, 5], READ ONLY; writes
 * cells u8 [n, blocks * blocks * 3], every byte.  One wave per cell, four cells per workgroup of 256 threads, grid
 * (ceil(blocks * blocks / 4), n); the lanes stride over the pixels of the cell clipped to the photo, so the work is proportional to the
 * pixels that exist, whatever the box claims; no atomics, one writer per cell.  0 < n <= 65535, n_images > 0, 1 <= blocks <= 64.
 * Arguments are validated before any HIP call (-1 and imm_last_error()). */
int imm_redact_cells_u8(const uint8_t* src, const int64_t* offsets, const int32_t* hw, int n_images, const int32_t* boxes, int blocks, int n,
                        uint8_t* cells, void* stream);

/* The paste.  dst u8 (the packed photos, pasted into in place); offsets, hw, boxes, links int32 [n, 2], inv_ramp f32 [n, 2] as
 * imm_warp_u8 takes them; cells u8 [n, blocks * blocks * 3] (imm_redact_cells_u8's output for these rows and this `blocks`), READ ONLY,
 * never dst; mode IMM_REDACT_PIXELATE or IMM_REDACT_SMOOTH.  edges f32 [n, K, 3], inv_soft f32 [n] and hull_flags int32 [n]
 * (imm_hull_fit's output for these rows) are all NULL (no mask; K is not read) or all non-NULL, then 1 <= K <= 80.  The block's own
 * row keeps its cell grid (at most 12 288 bytes) and, with the mask, its 3 K lines and inv_soft (at most 964 bytes) in LDS; rows met
 * on a link walk read theirs from global memory.  0 < n <= 65535, n_images > 0, max_box_pixels > 0 (it sizes the grid only). */
int imm_redact_u8(uint8_t* dst, const int64_t* offsets, const int32_t* hw, int n_images, const int32_t* boxes, const int32_t* links,
                  const float* inv_ramp, const uint8_t* cells, int blocks, int mode, const float* edges, const float* inv_soft,
                  const int32_t* hull_flags, int K, int n, int max_box_pixels, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IMM_REDACT_H */
