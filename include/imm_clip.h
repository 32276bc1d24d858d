/* imm_clip.h - C-ABI of the two clip-morph entry points of libimm_hip.so (ABI 35; imm_amd/csrc/clip.hip, imm_amd/clip.py,
 * imm_amd/inference.py LandmarkDetector.morph_clip): a donor's face follows a tracked face through a clip.  Every kernel of the morph
 * chain (imm_morph.h, imm_colour.h, imm_hull.h, imm_seam.h) takes its box rows, landmarks and settings as device pointers, so the
 * chain runs behind imm_track_step (imm_track.h) with nothing returning to the host.  What morph() forms on the host from host boxes
 * is formed here from the box rows the tracker left on the device (imm_clip_rows), and the colour gain and the membrane's differences,
 * which would otherwise jump from frame to frame, pass a first-order filter (imm_clip_ema).  Included by imm_hip.h, whose conventions
 * hold here: plain pointers and sizes, an explicit hipStream_t as void*, int status (0 = ok) and imm_last_error().
 *
 * THE RULE
 *
 * Rows (imm_clip_rows), per face f of one frame.  All arithmetic is f64, every operation rounded separately (no fma), in the order
 * written here; the only operations are + - * / fmin fmax isfinite and comparisons (fmin / fmax return the other operand when one is a
 * NaN), so that numpy reproduces it bit for bit; results are rounded once to f32.
 *     With this frame's row (image, y0, x0, y1, x1):  H = (double)y1 - (double)y0,  W = (double)x1 - (double)x0
 *     g(r) = r <= 0.5 ? 2 : 1 / fmax(r, 0.5)
 *     inv_ramp[f] = ((float)g(feather * H), (float)g(feather * W))                      the bits of generation.compose_inv_ramp
 *     inv_soft[f] = (float)(1 / fmax(1, (double)mask_feather[f] * fmin(H, W)))          the bits of morphing.hull_inv_soft
 *   own[f], the landmarks the morph blends, (y, x) in the frame of this frame's box:
 *     a LOST face (track_flags[f] bit 0):  every value is NaN.  This is how the row is dropped: imm_morph_poses carries the NaN,
 *         imm_warp_fit flags the row and gives it NaN coefficients, the paste then writes nothing in its box, and imm_hull_fit and
 *         imm_seam_fit flag it.
 *     otherwise, points == NULL:  the bits of mu[f].
 *     otherwise the inverse of step 1 of imm_track.h, from the tracker's (filtered) source pixels:
 *         sy = (double)((float)H / (float)S),  sx likewise with W
 *         v = ((((double)points[f][k][0] - (double)y0) / sy) / (double)S) * 2 - 1,   and x likewise with x0, sx
 *         a finite v is clamped, fmin(fmax(v, -1), 1), as imm_retarget clamps its poses; a v that is not finite is stored as it is
 *         (an empty box has sy = 0 and gives one).
 *
 * Filter (imm_clip_ema), per row i of n rows of `width` values, f32, every operation rounded separately:
 *     the row is SKIPPED when skip[i] != 0 (any bit of the row's own flags) or lost != NULL and lost[i] bit 0 is set:
 *         x, state and seen of that row are left alone.
 *     otherwise, per element j:   if seen[i] == 0:  state[i][j] = x[i][j]
 *                                 else:             state[i][j] = state[i][j] + alpha * (x[i][j] - state[i][j])
 *                                 then              x[i][j] = state[i][j]
 *     and after the row's elements seen[i] = 1.
 *   This is the box filter's convention of imm_track.h (s = s + a * (x - s)): alpha = 1 means no filter.
 * Consequences.  (a) The first value a row sees passes through in its bits.  (b) A constant input is a fixed point in its bits:
 * x - state is 0, the product is 0 and the sum is state (the one exception is -0, which becomes +0, the same value).  (c) A skipped frame does not age the state: the next unskipped frame is
 * filtered against the last unskipped one.  (d) A NaN that enters a row's state stays there: the row's values are NaN from then on. */
#ifndef IMM_CLIP_H
#define IMM_CLIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The rows of one frame, one workgroup of 64 threads per face.  Inputs, READ ONLY: boxes int32 [F, 5], the rows (image, y0, x0, y1, x1)
 * this frame was cut with (the image index is not read); track_flags int32 [F], imm_track_step's flags of this frame; mu f32 [F, K, 2],
 * the pose head's landmarks; points f32 [F, K, 2] (imm_track_step's points or points_smooth of this frame) or NULL; mask_feather f32 [F]
 * or NULL.  Outputs: own f32 [F, K, 2], inv_ramp f32 [F, 2], and inv_soft f32 [F], which is NULL exactly when mask_feather is.
 * 1 <= F <= 65535, 1 <= K <= 80, 0 < S <= 8192, feather in [0, 0.5].  No value a buffer holds reaches an address.  Arguments are
 * validated before any HIP call (-1 and imm_last_error()). */
int imm_clip_rows(const int32_t* boxes, const int32_t* track_flags, const float* mu, const float* points, int K, int S, int F,
                  double feather, const float* mask_feather, float* own, float* inv_ramp, float* inv_soft, void* stream);

/* The filter, one workgroup per row, so that seen[i] is read by all of it before one thread writes it.  x f32 [n, width] is filtered
 * in place; state f32 [n, width] and seen int32 [n] (zero at the start of a clip) are read and written; skip int32 [n] and lost int32
 * [n] (or NULL) are READ ONLY.  1 <= n <= 65535, 1 <= width <= 768 (6 for the colour gain, 3 * ring for the membrane), alpha in
 * (0, 1].  x and state must not overlap.  Arguments are validated before any HIP call (-1 and imm_last_error()). */
int imm_clip_ema(float* x, float* state, int32_t* seen, const int32_t* skip, const int32_t* lost, int n, int width, float alpha,
                 void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IMM_CLIP_H */
