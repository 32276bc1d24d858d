/* imm_morph.h - C-ABI of the morph entry points of libimm_hip.so (ABI 31; imm_amd/csrc/morph.hip, imm_amd/morphing.py, imm_amd/inference.py
 * LandmarkDetector.morph): two faces blended in SHAPE and in TEXTURE from their own pixels.  Row b has a face of its own (a box in a
 * photo of the packed buffer src) and a donor face (a box in a photo of a second packed buffer).  Two numbers per row say how far the
 * result goes from the one to the other: shape[b] moves the landmarks, texture[b] mixes the pixels.  shape = texture = t is the morph at
 * t; shape = 0, texture = 1 is the donor's face swapped in place; texture = 0 is imm_warp_u8 towards the blended pose.  Included by
 * imm_hip.h, whose conventions hold here: plain pointers and sizes, an explicit hipStream_t as void*, int status (0 = ok) and
 * imm_last_error().  The frame, the control points, the fit and the sampling are those of imm_warp.h; this header states what is added.
 *
 * THE RULE
 *
 * Poses (imm_morph_poses).  mu_a and mu_b f32 [n, K, 2] are the landmarks of the face itself and of its donor, each in the [-1, 1] frame
 * of its OWN box.  Per element, in f32, every operation rounded separately (no fma):
 *     p = (1 - s) * mu_a + s * mu_b,        s = shape[b]
 * so s = 0 gives mu_a and s = 1 gives mu_b as values (x * 1 + y * 0 for finite y), and a NaN input gives NaN.  poses2 f32 [2, n, K, 2]
 * holds p twice and mu2 f32 [2, n, K, 2] holds (mu_a, mu_b): the poses and mu arguments of ONE imm_warp_fit launch over 2 n rows with
 * strength 1, which writes ctrl [2, n, M, 2] (both halves equal: the splines share their control points, p and the anchors) and coef2
 * [2, n, M + 3, 2]: coef2[0] (coef_a) is the displacement spline target frame -> own frame, coef2[1] (coef_b) target frame -> donor frame.
 * shape outside [0, 1] extrapolates; the host refuses it.
 *
 * Morph (imm_morph_u8).  Row b handles every photo pixel (r, c) inside both its box and its photo.  All arithmetic is f32, every
 * operation rounded separately (no fma), in this order:
 *   qy, qx as in imm_warp.h, from the row's own box (y0, x0, y1, x1), H = y1 - y0, W = x1 - x0
 *   for j = 0 .. M - 1 in order:  dy, dx, d2 and u = d2 > 0 ? d2 * log(d2) : 0 as in imm_warp.h, computed ONCE with the library logf, then
 *        DAy = DAy + coef_a[j][0] * u,  DAx = DAx + coef_a[j][1] * u,  DBy = DBy + coef_b[j][0] * u,  DBx = DBx + coef_b[j][1] * u
 *   the affine tail of each spline as in imm_warp.h:  D = ((D + c[M]) + c[M + 1] * qy) + c[M + 2] * qx
 *   sA = ((float)r + hy * DAy, (float)c + hx * DAx),  hy = 0.5f * (float)H, hx = 0.5f * (float)W: the place in the row's OWN photo
 *   sB = ((float)y0_B + ((qy + DBy) + 1) * hy_B, (float)x0_B + ((qx + DBx) + 1) * hx_B), from the donor box row (image_B, y0_B, x0_B,
 *        y1_B, x1_B) with hy_B = 0.5f * (float)(y1_B - y0_B), hx_B likewise: the donor-frame point q + DB in the pixels of the DONOR photo
 *   if any of the four coordinates is not finite the pixel is left alone (so a row with NaN coefficients on either side writes nothing)
 *   gA = the bilinear sample of src's photo at sA, gB = the bilinear sample of the donor photo at sB, both as imm_warp_u8 samples: the
 *        float clamp before the int conversion, the taps clamped to the sampled photo before any address is formed, a + (b - a) * t
 *        along x, then along y
 *   mix = gA + texture[b] * (gB - gA), per channel
 *   a   = imm_warp_u8's ramp weight from inv_ramp[b];  photo[r, c] = min(max(rint(p + a * (mix - p)), 0), 255) with p read from dst,
 *        stored as u8 AFTER EVERY ROW, in row order
 * Rows and links.  A row is ACTIVE when its donor image index lies in [0, n_donor_images) and its donor box has H_B > 0 and W_B > 0.  A row
 * that is not active, a row whose own image index lies outside [0, n_images) and a row whose box lies wholly outside its photo write
 * nothing.  links int32 [n, 2] are imm_compose_u8's, as imm_warp_u8 reads them: a pixel belongs to the first ACTIVE row of the launch
 * whose box covers it; that row's thread walks the later rows of the photo (passing over rows that are not active), keeps the running
 * value in a register with the per-row rounding and is the pixel's only reader and writer in dst.  No atomics.  The same bounds hold on
 * the walks (a previous link must be smaller, a next link larger than its row, both inside [0, n)), so the same rows issued as several
 * launches, in order, give the bytes of one launch.  A donor box may reach outside the donor photo: the taps are clamped.
 * Consequences of the order of operations.  (a) texture[b] == 0 with finite coef_b: mix = gA + 0 = gA, the bytes of imm_warp_u8 with
 * coef_a.  (b) zero coefficients on both sides with the donor buffer, photo and box equal to the row's own: sA = (r, c) exactly and sB
 * lies within rounding of it, so every byte returns for every texture and feather.  (c) shape == 0 and texture == 0: coef_a == 0 (the
 * displacement fit of a zero right-hand side) and (a) give the photo bit for bit. */
#ifndef IMM_MORPH_H
#define IMM_MORPH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The pose blend.  mu_a, mu_b f32 [n, K, 2] (mu_a may be the pose head's buffer, read in place), shape f32 [n].  Writes poses2 f32
 * [2, n, K, 2] and mu2 f32 [2, n, K, 2].  1 <= K <= 80, 0 < n <= 32767 (the fit that follows takes 2 n <= 65535 rows).  One thread per
 * float.  All pointers are read at the launch only; arguments are validated before any HIP call (-1 and imm_last_error()). */
int imm_morph_poses(const float* mu_a, const float* mu_b, const float* shape, int K, int n, float* poses2, float* mu2, void* stream);

/* The morph.  src, dst, offsets, hw, n_images, boxes, links, inv_ramp, ctrl, M, n, max_box_pixels: exactly as imm_warp_u8 takes them
 * (src READ ONLY, dst a copy of it changed IN PLACE, src != dst).  donor: a second packed u8 HWC buffer of the same layout
 * (donor_offsets int64 [n_donor_images], donor_hw int32 [n_donor_images, 2]), READ ONLY; it may be src itself, never dst.  donor_boxes
 * int32 [n, 5] (image, y0, x0, y1, x1 in the donor buffer), texture f32 [n], coef_a and coef_b f32 [n, M + 3, 2] (the two halves of the
 * fit's output for these rows).  The grid is (blocks, n) of 256 threads with a grid-stride loop; the row's ctrl, coef_a and coef_b sit in
 * LDS (2 KB).  The photo accesses are byte-wide.  Nothing outside the two packed buffers is addressed, whatever ctrl, the coefficients,
 * texture, the box rows and links hold.  3 <= M <= 80, 0 < n <= 65535, n_images > 0, n_donor_images > 0.  Every pointer is read at the
 * launch only; arguments are validated before any HIP call (-1 and imm_last_error()). */
int imm_morph_u8(const uint8_t* src, uint8_t* dst, const int64_t* offsets, const int32_t* hw, int n_images, const uint8_t* donor,
                 const int64_t* donor_offsets, const int32_t* donor_hw, int n_donor_images, const int32_t* boxes, const int32_t* donor_boxes,
                 const int32_t* links, const float* inv_ramp, const float* texture, const float* ctrl, const float* coef_a,
                 const float* coef_b, int M, int n, int max_box_pixels, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IMM_MORPH_H */
