/* imm_seam.h - C-ABI of the seamless morph of libimm_hip.so (ABI 34; imm_amd/csrc/seam.hip, imm_amd/csrc/morph.hip, imm_amd/morphing.py,
 * imm_amd/inference.py LandmarkDetector.morph(mask='hull', seamless=...)): a mean-value membrane hides the seam of the hull mask.  The
 * hull mask pastes only the face, and colour matching gives the donor's pixels one gain and one offset per channel; where the two skins
 * still differ on the mask's outline the soft edge reads as a halo.  Here the donor's pixels keep their detail and a smooth correction
 * field is added that takes them onto the photo's own values on the outline: the mean-value-coordinates form of gradient-domain cloning
 * (Farbman et al., "Coordinates for Instant Image Cloning", 2009).  Every pixel is a closed-form weighted mean of the colour differences
 * at B samples of the outline: no iterations, pixels independent of one another, only + - * / sqrt.  Included by imm_hip.h, whose
 * conventions hold here: plain pointers and sizes, an explicit hipStream_t as void*, int status (0 = ok) and imm_last_error().  The
 * packed buffers and box rows are those of imm_morph.h, the lines (edges) and their flags those of imm_hull.h.
 *
 * THE RULE
 *
 * Seam fit (imm_seam_fit).  One row per face, B samples per row, 16 <= B <= 256.
 * Ring.  f64 from the f32 inputs widened, every operation rounded separately (no fma), only + - * / and comparisons, so that numpy
 * reproduces it in its bits:
 *     H, W, vy_i, vx_i and the centroid cy = (((vy_0 + vy_1) + ...) + vy_{K-1}) / K, cx likewise: exactly imm_hull_fit's (imm_hull.h),
 *     from the same poses and boxes, in the same order.  (Growing the points about their centroid does not move it; grow itself enters
 *     only through the lines.)
 *     The region is the grown hull cut with the box's pixel centres [0, H - 1] x [0, W - 1]: its lines are the row's K lines
 *     (ny, nx, d) = edges[b][k], widened, in slot order, and then the four sides (1, 0, 0), (-1, 0, H - 1), (0, 1, 0), (0, -1, W - 1).
 *     Per line:      s0 = (ny * cy + nx * cx) + d            (how far the centroid lies inside it)
 *     Sample s, direction (uy, ux) = dirs[s] (f64 [B, 2], formed on the host as (cos, sin) of 2 pi s / B: no transcendental function
 *     runs on the device), t = +inf, then per line in the order above:
 *                    g = ny * uy + nx * ux;   if g < 0:  t = fmin(t, s0 / (-g))
 *     ring[b][s] = (cy + t * uy, cx + t * ux), each coordinate rounded once to f32: box-relative pixels, as rr and cc of imm_hull.h.
 * flags[b], int32:
 *     bit 0   the hull's flags[b] != 0, or cy or cx not finite, or !(s0 > 0) for some line: the centroid is not strictly inside the
 *             region (a slot without a winner, (0, 0, +inf), has s0 = +inf and passes)
 *     bit 1   for some sample t is not finite or !(t > 0)
 * A flagged row gets diff = 0 everywhere and ring[b][s] = ((float)cy, (float)cx) for every s: it is pasted as the plain hull morph.
 * ORIENTATION.  uy = cos, ux = sin: the samples run from +y towards +x, and for a pixel p strictly inside the ring's polygon
 * py_s * px_s' - px_s * py_s' >= 0 for every pair of neighbours (s, s' = s + 1 mod B), where (py_s, px_s) = ring_s - p.
 * Difference.  f32, in the morph's order (imm_morph.h), at the fractional place (by, bx) = ring[b][s]:
 *     qy = by * ry - 1,  qx = bx * rx - 1                      (ry, rx = 2 / H, 2 / W as the morph forms them)
 *     DA, DB from (qy, qx) as the morph takes them
 *     sA = (((float)y0 + by) + hy * DA_y, ((float)x0 + bx) + hx * DA_x)      the morph's, with (float)r replaced by (float)y0 + by
 *     sB = the donor box's image of q + DB, as the morph forms it
 *     gA, and gB through the gain when there is one, then mix = gA + texture * (gB - gA): exactly as the morph takes them
 *     own = the bilinear sample of src at ((float)y0 + by, (float)x0 + bx)
 *     diff[b][s][ch] = own_ch - mix_ch
 * A sample any of whose places is not finite gets diff = 0, and so does every sample of a row that is not ACTIVE (imm_morph.h), whose
 * photo index is out of range, or whose photo or donor photo has no pixels.
 *
 * Morph with the membrane (imm_morph_seam_u8).  imm_morph_hull_u8 with, per pixel with w > 0, after mix, in f32, every operation
 * rounded separately, rr = (float)(r - y0), cc = (float)(c - x0), and s = 0 .. B - 1 in order (s' = s + 1 mod B, s- = s - 1 mod B):
 *     py_s = by_s - rr,  px_s = bx_s - cc,  l_s = sqrtf(py_s * py_s + px_s * px_s)
 *     cr = py_s * px_s' - px_s * py_s',  dt = py_s * py_s' + px_s * px_s',  th_s = cr / (l_s * l_s' + dt)        tan of half the angle
 *     w_s = (th_{s-} + th_s) / l_s
 *     R_ch = R_ch + w_s * diff_s,ch,   Wsum = Wsum + w_s                        (from 0)
 *     if some l_s == 0:                                r = diff_s of the lowest such s (the coordinates' own limit)
 *     otherwise, if Wsum > 0 and Wsum, R_0, R_1, R_2 are finite:    r_ch = R_ch / Wsum
 *     otherwise                                        r = 0
 *     mix_ch = mix_ch + seamless[b] * r_ch             (the product rounded, then the sum; not clamped: paste_blend clamps the byte)
 * sqrtf and / are the correctly rounded ones: hipcc's default, which the build's flags (-O3, no fast-math switch) leave alone, so the
 * f32 numpy restatement has the kernel's bits given the same mix.  Everything else is the hull morph's: the weight, the ramp, ownership,
 * links, the rounding after every row.  ring, diff and seamless never reach an address: whatever they hold (NaN, inf, 1e30), only the
 * bytes inside the boxes change.
 * Consequences.  (a) seamless[b] == 0 gives mix + 0 * r: with finite r the bytes of imm_morph_hull_u8 (the host issues the calls of
 * before when every row is 0).  (b) A flagged row has diff = 0 and hence r = 0: the bytes of the hull morph.  (c) Two flat photos of
 * different colours, swapped at texture = 1 and seamless = 1, with or without a gain: every diff is the same integer triple, r lies
 * within rounding of it, mix + r within rounding of the photo's byte, and the rint restores that byte at every weight: the photo comes
 * back bit for bit wherever the pixels with w > 0 lie inside the ring's polygon.  (d) Rows issued as several launches give the bytes of
 * one launch, as before.
 * What the rule does NOT do.  The ring's polygon is inscribed in the region: between two samples it cuts the region's corners, and on
 * a side of the box that binds, the outermost pixels lie on the polygon itself.  There the coordinates have no limit that the rule
 * forms (0 / 0, or a sum that is not positive): r = 0, the plain hull morph.  Elsewhere outside the polygon r is whatever the sums give. */
#ifndef IMM_SEAM_H
#define IMM_SEAM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The seam fit.  poses f32 [n, K, 2], boxes int32 [n, 5], edges f32 [n, K, 3], hull_flags int32 [n] (imm_hull_fit's inputs and
 * outputs for these rows), dirs f64 [B, 2], and the morph's own inputs exactly as imm_morph_hull_u8 takes them (gain f32 [n, 3, 2] or
 * NULL), all READ ONLY; grow f32 [n] is validated and not read.  Writes ring f32 [n, B, 2], diff f32 [n, B, 3] and flags int32 [n].  One
 * workgroup of B threads per row, one thread per sample.  0 < n <= 65535, 1 <= K <= 80, 3 <= M <= 80, 16 <= B <= 256.  Arguments are
 * validated before any HIP call (-1 and imm_last_error()). */
int imm_seam_fit(const float* poses, const int32_t* boxes, const float* grow, const float* edges, const int32_t* hull_flags,
                 const double* dirs, const uint8_t* src, const int64_t* offsets, const int32_t* hw, int n_images, const uint8_t* donor,
                 const int64_t* donor_offsets, const int32_t* donor_hw, int n_donor_images, const int32_t* donor_boxes,
                 const float* texture, const float* ctrl, const float* coef_a, const float* coef_b, const float* gain, int K, int M, int B,
                 int n, float* ring, float* diff, int32_t* flags, void* stream);

/* The morph with the membrane.  Every argument up to K exactly as imm_morph_hull_u8 takes it, with its bounds and refusals; ring f32
 * [n, B, 2], diff f32 [n, B, 3] (imm_seam_fit's output for these rows) and seamless f32 [n], READ ONLY; 16 <= B <= 256.  The block's own
 * row keeps its 5 B floats in LDS (at most 5 KB), read as broadcasts; rows met on a link walk read theirs from global memory. */
int imm_morph_seam_u8(const uint8_t* src, uint8_t* dst, const int64_t* offsets, const int32_t* hw, int n_images, const uint8_t* donor,
                      const int64_t* donor_offsets, const int32_t* donor_hw, int n_donor_images, const int32_t* boxes,
                      const int32_t* donor_boxes, const int32_t* links, const float* inv_ramp, const float* texture, const float* ctrl,
                      const float* coef_a, const float* coef_b, const float* gain, const float* edges, const float* inv_soft,
                      const float* ring, const float* diff, const float* seamless, int K, int M, int B, int n, int max_box_pixels,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IMM_SEAM_H */
