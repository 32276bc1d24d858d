/* imm_hull.h - C-ABI of the landmark-hull mask of libimm_hip.so (ABI 33; imm_amd/csrc/hull.hip, imm_amd/csrc/morph.hip,
 * imm_amd/morphing.py, imm_amd/inference.py LandmarkDetector.morph(mask='hull')): a morph pastes only the face.  imm_morph_u8 blends
 * every pixel of a row's box, weighted by the rectangular edge ramp alone, so at shape = 0, texture = 1 (the swap) the donor's
 * background, hair and collar arrive with the face.  The mask is the convex hull of the row's K target landmarks, grown about their
 * centroid and softened inwards; it MULTIPLIES the box ramp, so the weight is never larger than imm_morph_u8's, and a pixel outside it
 * leaves the kernel before the spline is evaluated.  Included by imm_hip.h, whose conventions hold here: plain pointers and sizes, an
 * explicit hipStream_t as void*, int status (0 = ok) and imm_last_error().  The packed buffers and box rows are those of imm_morph.h.
 *
 * THE RULE
 *
 * Hull fit (imm_hull_fit).  One row per face.  poses f32 [n, K, 2]: the (y, x) of the row's target landmarks in the frame of its box
 * (the first half of imm_morph_poses' poses2, read in place); boxes int32 [n, 5]; grow f32 [n]; 1 <= K <= 80.  All arithmetic is f64
 * from the f32 inputs widened, every operation rounded separately (no fma), using only + - * / sqrt and comparisons, in this order, so
 * that numpy reproduces it in its bits:
 *     H = y1 - y0,  W = x1 - x0                                   in 64 bits
 *     vy_i = (py_i + 1) * (0.5 * H),  vx_i = (px_i + 1) * (0.5 * W)      box-relative pixel coordinates: the inverse of the paste
 *                                                                 kernels' q = (r - y0) * 2 / H - 1, no half-pixel offset; the box
 *                                                                 corner never enters, which keeps the per-pixel f32 arithmetic small
 *     cy = (((vy_0 + vy_1) + ...) + vy_{K-1}) / K,  cx likewise   summed in index order
 *     vy_i <- cy + g * (vy_i - cy),  vx_i likewise                g = (double)grow[b]
 * Slot i, for i = 0 .. K - 1 (declarative: no result depends on how the work is spread over threads):
 *     a CANDIDATE is a j with (ey, ex) = (vy_j - vy_i, vx_j - vx_i) != (0, 0) and
 *                 ey * (vx_k - vx_i) - ex * (vy_k - vy_i) >= 0    for EVERY k (the two products rounded, then their difference)
 *     the WINNER is the candidate with the largest ey * ey + ex * ex; ties go to the lowest j
 *     with a winner:     len = sqrt(ey * ey + ex * ex),  ny = -ex / len,  nx = ey / len,  d = -(ny * vy_i + nx * vx_i)
 *                        edges[b][i] = (ny, nx, d), each rounded once to f32
 *     without a winner:  edges[b][i] = (0, 0, +inf)
 * No compaction: no sorting, no vertex list, no count.  Collinear and duplicate points only yield redundant lines.
 * flags[b], int32:
 *     bit 0   H <= 0 or W <= 0, or any pose of the row or its grow not finite
 *     bit 1   fewer than 3 slots with a winner, or no winner's line has any point strictly on its inner side (the expression above
 *             is > 0 for no k of any winner): the points are all one point or all on one line, and the hull has no inside
 * A flagged row gets (0, 0, -inf) in every slot: its weight is 0 everywhere, so the row writes nothing.
 *
 * Weight.  Per photo pixel (r, c) of row b's box, in the morph kernel, in f32, every operation rounded separately, in this order:
 *     rr = (float)(r - y0),  cc = (float)(c - x0),  dist = +inf
 *     for k = 0 .. K - 1:   s = (ny_k * rr + nx_k * cc) + d_k;   dist = fminf(dist, s)        (numpy: fmin)
 *     w = fminf(fmaxf(dist * inv_soft[b], 0), 1)                  a NaN becomes 0 through the order of the two clamps
 *     if !(w > 0) the row leaves the pixel alone                  before the spline is evaluated and before any sample
 *     otherwise the blend weight is paste_ramp(...) * w           one rounded product, in place of paste_ramp(...)
 * inv_soft[b] = (float)(1 / max(1, mask_feather * min(H, W))), formed in f64 on the host: the weight is 0 on the grown hull's edge and
 * 1 that many pixels inside it.  A slot (0, 0, +inf) gives s = +inf and never lowers dist; a slot (0, 0, -inf) gives dist = -inf, w = 0.
 *
 * Morph with the mask (imm_morph_hull_u8).  imm_morph_u8 (imm_morph.h), or with gain != NULL imm_morph_colour_u8 (imm_colour.h), with
 * the weight above.  Everything else - ACTIVE rows, the ramp, the mix, the rounding after every row - is theirs.  Ownership does not
 * change: a row covers the pixels of its BOX, so ownership, row order and links behave exactly as before; a pixel a row owns and no
 * row gives a weight keeps its byte.  edges and inv_soft never reach an address: whatever they hold (NaN, inf, 1e30), only weights
 * change, and the blend's clamp keeps the result a byte.
 * Consequences of the order of operations.  (a) a hull that contains the whole box at a distance of 1 / inv_soft or more gives w = 1
 * at every pixel, the weight paste_ramp(...) * 1 = paste_ramp(...), and hence the bytes of imm_morph_u8 (of imm_morph_colour_u8 with
 * a gain).  (b) w <= 1 and paste_ramp(...) >= 0: the weight is never larger than imm_morph_u8's. */
#ifndef IMM_HULL_H
#define IMM_HULL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The hull fit.  poses f32 [n, K, 2], boxes int32 [n, 5], grow f32 [n], READ ONLY; writes edges f32 [n, K, 3] and flags int32 [n].
 * One workgroup of 256 threads per row: the K points in f64 in LDS, the K * K (i, j) pairs spread over the threads, each running the
 * predicate over k (K * K * K evaluations a row, at most 512 k), one thread per slot picking its winner.  0 < n <= 65535,
 * 1 <= K <= 80.  Arguments are validated before any HIP call (-1 and imm_last_error()). */
int imm_hull_fit(const float* poses, const int32_t* boxes, const float* grow, int K, int n, float* edges, int32_t* flags, void* stream);

/* The morph with the mask.  Every argument up to coef_b exactly as imm_morph_u8 takes it, with its bounds and refusals; gain f32
 * [n, 3, 2] as imm_morph_colour_u8 takes it, or NULL for the morph without colour matching; edges f32 [n, K, 3] (imm_hull_fit's
 * output for these rows) and inv_soft f32 [n], READ ONLY; 1 <= K <= 80.  The block's own row keeps its 3 K floats and its inv_soft
 * in LDS (at most 964 bytes) next to its control points and coefficients, read as broadcasts; rows met on a link walk read theirs
 * from global memory. */
int imm_morph_hull_u8(const uint8_t* src, uint8_t* dst, const int64_t* offsets, const int32_t* hw, int n_images, const uint8_t* donor,
                      const int64_t* donor_offsets, const int32_t* donor_hw, int n_donor_images, const int32_t* boxes,
                      const int32_t* donor_boxes, const int32_t* links, const float* inv_ramp, const float* texture, const float* ctrl,
                      const float* coef_a, const float* coef_b, const float* gain, const float* edges, const float* inv_soft, int K, int M,
                      int n, int max_box_pixels, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IMM_HULL_H */
