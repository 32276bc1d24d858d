/* imm_score.h - C-ABI of the landmark-quality entry point of libimm_hip.so (ABI 36; imm_amd/csrc/score.hip, imm_amd/quality.py,
 * imm_amd/inference.py LandmarkDetector.quality, imm_amd/tracking.py FaceTracker with a gate): after a pose program, one small kernel
 * turns the soft-argmax marginals and the landmarks of every face into two scores - how widely the landmarks' probability is spread,
 * and how badly the K landmarks fit a reference shape under the best similarity - and, for the tracker, into landmarks that are NaN
 * for a face whose scores fail the caller's thresholds, so that imm_track_step's own lost rule (imm_track.h, step 3) takes it from
 * there.  Included by imm_hip.h, whose conventions hold here: plain pointers and sizes, an explicit hipStream_t as void*, int status
 * (0 = ok) and imm_last_error().
 *
 * Nobody has measured how well these scores tell a face from a non-face: the library ships no threshold.  +inf switches one off.
 *
 * THE RULE, per face f.  All arithmetic is f64, every operation rounded separately (no fma), in the order written here; the only
 * operations are + - * / sqrt fmax isfinite; every sum runs over ascending index from 0.0; results are rounded once to the stored
 * type.  No transcendental function runs on the device.
 *
 * 1. Spread.  lin_y(i) = -1.0 + (2.0 * i) / (h - 1), i = 0 .. h - 1;  lin_x(j) likewise with w.  Per landmark k:
 *     vy = sum_i (double)py[i][k] * (d * d)  with d = lin_y(i) - (double)mu[k][0];   vx likewise with px, lin_x and mu[k][1]
 *     spread[k] = sqrt(vy + vx)
 *     sbar = (sum_k spread[k]) / K          (over the f64 spreads)
 * 2. Points.  boxes == NULL:  p[k][a] = (double)mu[k][a].  Otherwise step 1 of imm_track.h, letter for letter: with the row
 *    (image, y0, x0, y1, x1):
 *     H = (double)y1 - (double)y0,  sy = (double)((float)H / (float)S),  W and sx likewise
 *     p[k][0] = (double)y0 + ((((double)mu[k][0] + 1.0) * 0.5) * S) * sy,   p[k][1] likewise with x0, sx
 * 3. Shape residual.  ref == NULL:  residual = 0.0.  Otherwise, with z0 := ref, as step 3 of imm_track.h:
 *     mz[a] = (sum_k z0[k][a]) / K,  mp[a] = (sum_k p[k][a]) / K
 *     per k:  u = z0[k] - mz,  v = p[k] - mp
 *             den += u0 * u0 + u1 * u1;   ar += u0 * v0 + u1 * v1;   ai += u0 * v1 - u1 * v0;   pv += v0 * v0 + v1 * v1
 *     den and pv not both finite and > 0:  residual = NaN.  Else
 *     r2 = 1.0 - (ar * ar + ai * ai) / (den * pv);   residual = sqrt(fmax(r2, 0.0)) when r2 is finite, else NaN
 *    the share of the points' scatter that the best similarity of the reference leaves unexplained: it lies in [0, 1] and is unchanged
 *    by rotating, scaling or shifting p.
 * 4. Flags, decided on the f64 values, not on the stored f32:  bit 0 = !(sbar <= max_spread),  bit 1 = !(residual <= max_residual).
 *    A NaN score therefore sets its bit; a score equal to its threshold passes.
 * 5. Gated landmarks.  mu_out[k][a] = the f32 quiet NaN 0x7fc00000 for every k of a face with blank && flags != 0; otherwise the
 *    bits of mu[k][a]. */
#ifndef IMM_SCORE_H
#define IMM_SCORE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The rule for F faces: one 64-lane workgroup per face, lane k < K walks landmark k's marginals, lane 0 forms the ordered sums over k.
 * Inputs: py f32 [F, h, K] and px f32 [F, w, K], the soft-argmax marginals; mu f32 [F, K, 2], the landmarks (y, x) in [-1, 1];
 * boxes int32 [F, 5], the rows (image, y0, x0, y1, x1) the faces were cut with, or NULL (the points are the landmarks themselves);
 * ref f64, the reference shape [K, 2] of face f at ref + f * ref_stride (ref_stride in doubles: 0 = one shape for all faces, else
 * >= 2 K; K * 2 values are read per face), or NULL (residual = 0); max_spread, max_residual: the thresholds, +inf = not applied, a NaN
 * is refused; blank: 0 or 1.
 * Outputs: spread f32 [F, K]; score f32 [F, 2] = ((float)sbar, (float)residual); qflags int32 [F]; mu_out f32 [F, K, 2], which may be
 * NULL when blank == 0 and must not overlap mu.
 * 0 < F <= 65535, 1 <= K <= 64, 2 <= h, w <= 64, 0 < S <= 8192.  Every pointer is read at the launch only; arguments are validated
 * before any HIP call (-1 and imm_last_error()). */
int imm_landmark_scores(const float* py, const float* px, const float* mu, const int32_t* boxes, const double* ref, int64_t ref_stride,
                        int K, int h, int w, int S, int F, double max_spread, double max_residual, int blank, float* spread,
                        float* score, int32_t* qflags, float* mu_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IMM_SCORE_H */
