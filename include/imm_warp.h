/* imm_warp.h - C-ABI of the warp entry points of libimm_hip.so (ABI 30; imm_amd/csrc/warp.hip, imm_amd/warping.py, imm_amd/inference.py
 * LandmarkDetector.warp): faces re-posed inside their u8 photographs from the photo's OWN pixels, moved by a thin-plate spline whose
 * control points are the face's landmarks.  Included by imm_hip.h, whose conventions hold here: plain pointers and sizes, an explicit
 * hipStream_t as void*, int status (0 = ok) and imm_last_error().
 *
 * THE RULE
 *
 * Frame.  Row b has a box row (image, y0, x0, y1, x1), half-open, H = y1 - y0, W = x1 - x0.  Photo pixel (r, c) has the frame
 * coordinate q = (2 (r - y0) / H - 1, 2 (c - x0) / W - 1): the frame of the landmarks, the inverse of
 * imm_amd.keypoints.to_source_pixels over the box geometry.
 *
 * Control points.  ctrl_b = the row's K target landmarks p_b (poses) followed by A = 4 m anchors on the border of [-1, 1]^2, m per
 * side, equally spaced, corners included (imm_amd.warping.warp_anchors: from (-1, -1) along the top side, then the right, the bottom
 * and the left one).  The anchors are the same for every row and come from the host as f32 [A, 2]; m = 0: none.  M = K + A,
 * 3 <= M <= 80.
 *
 * Fit (imm_warp_fit).  The displacement spline D_b maps the TARGET frame to the SOURCE frame: its values are
 * d = strength * (mu_b - p_b) at the landmarks and 0 at the anchors,
 *     [[U(|ctrl_i - ctrl_j|^2) + lam I, 1, ctrl], [1^T, 0, 0], [ctrl^T, 0, 0]] . [w; a] = [d; 0],     U(d2) = d2 log d2, U(0) = 0,
 * one (M + 3) x (M + 3) system with two right-hand sides (y, x) per row.  One workgroup per row assembles it in f64 from the f32 inputs
 * widened (d = strength * ((double)mu - (double)p)) and solves it by Gaussian elimination with partial pivoting (the row of the largest
 * |value| of the column, the first of equals), every operation rounded separately; the coefficients are rounded ONCE to
 * coef f32 [n, M + 3, 2] (rows w_0 .. w_{M-1}, a_0, a_1 (q_y), a_2 (q_x); columns y, x) and the control points are written to
 * ctrl f32 [n, M, 2].  A row gets NaN coefficients and bit 0 of flags int32 [n] in two cases: an input (landmark, pose, anchor) that
 * is not finite, and a pivot that is zero or not finite (coincident control points at lam == 0, all points on one line); otherwise
 * its flag is 0.  The displacement form is deliberate: a zero right-hand side eliminates to exactly zero coefficients, so poses
 * equal to mu give the identity, bit for bit.
 *
 * Warp (imm_warp_u8).  Row b handles every photo pixel (r, c) inside both its box and its photo.  All arithmetic is f32, every
 * operation rounded separately (no fma), in this order:
 *   qy = (float)(r - y0) * ry - 1,  ry = (float)(2.0 / (double)H);  qx likewise from c, x0, W
 *   Dy = 0, Dx = 0; for j = 0 .. M - 1 in order:  dy = qy - ctrl[j][0], dx = qx - ctrl[j][1], d2 = dy * dy + dx * dx,
 *        u = d2 > 0 ? d2 * log(d2) : 0,  Dy = Dy + coef[j][0] * u,  Dx = Dx + coef[j][1] * u
 *   Dy = ((Dy + coef[M][0]) + coef[M + 1][0] * qy) + coef[M + 2][0] * qx;  Dx likewise from column 1
 *   s  = ((float)r + (0.5f * (float)H) * Dy, (float)c + (0.5f * (float)W) * Dx).  A pixel whose s is not finite is left alone (so a
 *        row whose coefficients are NaN writes nothing).
 *   g  = the bilinear sample of the ORIGINAL photo (src) at s: f = floor(s), t = s - f, taps f and f + 1, each clamped to
 *        [0, h - 1] x [0, w - 1] before any address is formed, evaluated as a + (b - a) * t along x, then along y
 *   a  = wy * wx,  wy = min(1, (min(r - y0, y1 - 1 - r) + 0.5) * inv_ramp[b][0]),  wx likewise with inv_ramp[b][1]: imm_compose_u8's
 *        weight (imm_amd.generation.compose_inv_ramp; the device never divides by a ramp)
 *   photo[r, c] = min(max(rint(p + a * (g - p)), 0), 255), to nearest even, p read from dst, stored as u8 AFTER EVERY ROW, in row
 *        order: a later row blends over the rounded result of an earlier one, so the same rows issued as several launches, in
 *        order, give the bytes of one launch.
 * log is the library logf (about one ulp), not the hardware's v_log_f32 approximation: with it the kernel stays within the cap of
 * the f64 restatement (tests/warp_reference.py) that the f32 numpy restatement itself meets; M logarithms per pixel are cheap next
 * to the photo traffic at the M <= 80 served here.
 * Overlapping rows of one photo use the links of imm_compose_u8 (int32 [n, 2]: per row the previous row of the same photo in THIS
 * launch and the next one, -1 for none; imm_amd.generation.compose_links).  A pixel belongs to the first row of the launch whose box
 * covers it; that row's thread walks the later rows of the photo, keeps the running value in a register with the per-row rounding
 * and is the pixel's only reader and writer in dst.  No atomics.  A previous link must be smaller and a next link larger than its
 * row: the walks stop at a link that is not (or that lies outside [0, n)), whatever the buffer holds.
 * Identity.  With zero coefficients s = (r, c) exactly, the sample is the pixel itself and the blend returns it for every feather. */
#ifndef IMM_WARP_H
#define IMM_WARP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The fit.  poses f32 [n, K, 2]: the target landmarks p; mu f32 [n, K, 2]: the faces' own landmarks (the pose head's buffer can be
 * read in place); anchors f32 [A, 2], NULL iff A == 0.  1 <= K, A >= 0 and a multiple of 4, 3 <= K + A <= 80, 0 < n <= 65535, strength
 * finite, lam finite and >= 0.  Writes coef f32 [n, K + A + 3, 2], ctrl f32 [n, K + A, 2] and flags int32 [n].  One workgroup of 256
 * threads per row; the augmented matrix (83 x 85 doubles at most) lives in static LDS.  All pointers are read at the launch only: the
 * call may follow the captured pose program on its stream with no host round trip.  Arguments are validated before any HIP call
 * (-1 and imm_last_error()). */
int imm_warp_fit(const float* poses, const float* mu, const float* anchors, int K, int A, int n, double strength, double lam, float* coef,
                 float* ctrl, int32_t* flags, void* stream);

/* The warp.  src: the packed u8 HWC buffer of imm_resize_crop_u8 (offsets int64 [n_images], hw int32 [n_images, 2], three channels),
 * READ ONLY; dst: a buffer of the same layout, the canvas, changed IN PLACE (it starts as a copy of src; it must not be src itself).
 * boxes int32 [n, 5], links int32 [n, 2], inv_ramp f32 [n, 2] as imm_compose_u8 takes them; ctrl f32 [n, M, 2] and coef f32
 * [n, M + 3, 2] as imm_warp_fit wrote them for these rows.  A row whose image index lies outside [0, n_images) writes nothing, nor does
 * a box wholly outside its photo.  Pixels of no box, photos without a row and the padding between photos are not written.  The grid is
 * (blocks, n) of 256 threads; max_box_pixels > 0 sizes it (the largest H * W of the rows; a larger box is still warped whole, by a
 * grid-stride loop).  The row's ctrl and coef sit in LDS (1.3 KB).  The photo accesses are byte-wide.  Nothing outside the packed
 * buffers is addressed, whatever ctrl, coef, boxes and links hold.  3 <= M <= 80, 0 < n <= 65535, n_images > 0.  Every pointer is read
 * at the launch only; arguments are validated before any HIP call (-1 and imm_last_error()). */
int imm_warp_u8(const uint8_t* src, uint8_t* dst, const int64_t* offsets, const int32_t* hw, int n_images, const int32_t* boxes,
                const int32_t* links, const float* inv_ramp, const float* ctrl, const float* coef, int M, int n, int max_box_pixels,
                void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IMM_WARP_H */
