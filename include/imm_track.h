/* imm_track.h - C-ABI of the face-tracking entry point of libimm_hip.so (ABI 28; imm_amd/csrc/track.hip, imm_amd/tracking.py,
 * imm_amd/inference.py LandmarkDetector.track / .tracker): after each frame's pose head, one small kernel turns the landmarks into
 * the next frame's box row on the device, so a whole clip is queued without a device -> host copy.  Included by imm_hip.h, whose
 * conventions hold here: plain pointers and sizes, an explicit hipStream_t as void*, int status (0 = ok) and imm_last_error().
 *
 * THE RULE, per face f.  All arithmetic is f64, every operation rounded separately (no fma), in the order written here; the only
 * operations are + - * / sqrt fabs fmin fmax rint isfinite (fmin / fmax return the other operand when one is a NaN; rint rounds ties
 * to even); results are rounded once to the stored type.  Sums over the K points run k = 0, 1, .., K - 1 from 0.0.
 *
 * State.  state f64 [F][5 + 6 K], persistent across the frames of a clip:
 *     [0] h0  [1] w0            the anchor box's sides
 *     [2] cy  [3] cx  [4] s     the box filter: centre and scale
 *     [5 + 2 k + a]             z0[k][a], the anchor shape (a = 0: y, 1: x), relative to the anchor box's centre
 *     [5 + 2 K + 2 k + a]       xhat[k][a]      the One-Euro pair of point coordinate (k, a)
 *     [5 + 4 K + 2 k + a]       dxhat[k][a]
 *
 * 1. Source pixels (keypoints.to_source_pixels over keypoints.box_geometry).  With this frame's row (image, y0, x0, y1, x1):
 *     H = (double)y1 - (double)y0,  sy = (double)((float)H / (float)S),  W and sx likewise
 *     p[k][0] = (double)y0 + ((((double)mu[k][0] + 1.0) * 0.5) * S) * sy,   p[k][1] likewise with x0, sx
 * 2. Start of a clip (init == 1):  ccy = ((double)y0 + (double)y1) * 0.5, ccx likewise;  h0 = H, w0 = W;  cy = ccy, cx = ccx, s = 1;
 *     z0[k][a] = p[k][a] - cc[a];  xhat = p;  dxhat = 0.
 * 3. Similarity fit of z0 onto p (alignment.fit_similarity, points as y + ix):
 *     mz[a] = (sum_k z0[k][a]) / K,  mp[a] = (sum_k p[k][a]) / K
 *     per k:  u = z0[k] - mz,  v = p[k] - mp
 *             den += u0 * u0 + u1 * u1;   ar += u0 * v0 + u1 * v1;   ai += u0 * v1 - u1 * v0
 *     a_r = ar / den,  a_i = ai / den
 *     my = mp0 - (a_r * mz0 - a_i * mz1),  mx = mp1 - (a_r * mz1 + a_i * mz0),  ms = sqrt(a_r * a_r + a_i * a_i)
 *    The face is LOST this frame when some mu of it is not finite, or den == 0, or my, mx, ms are not all finite with ms > 0.
 *    A lost face keeps its state as it is (after step 2): steps 4 and 6 are skipped.
 * 4. Box filter:  cy = cy + beta * (my - cy),  cx and s likewise with mx, ms.
 * 5. Next box, from the state (of a lost face: the unchanged one):
 *     h' = fmin(fmax(rint(s * h0), 2), 4194304),  w' likewise with w0
 *     y0' = fmin(fmax(rint(cy - h' * 0.5), -8388608), 8388608),  y1' = y0' + h',  x likewise
 *    so y1' > y0', x1' > x0' and every coordinate stays below 2^24 whatever the device buffers hold: the two things
 *    imm_resize_crop_u8 leaves to its caller.
 * 6. One-Euro filter per point coordinate, speeds in box heights per second:
 *     r(fc) = 1 / (1 + 1 / (c * fc));   rd = r(d_cutoff)
 *     dx = (p - xhat) / (te * H);  dxhat = dxhat + rd * (dx - dxhat);  fc = min_cutoff + beta_e * fabs(dxhat)
 *     xhat = xhat + r(fc) * (p - xhat)
 *    A non-finite p leaves its pair as it is.  On the first frame xhat == p and dxhat == 0, so the point passes through.
 *    With filter_off != 0 the pairs are not touched and points_smooth is p.
 *
 * No transcendental function runs on the device: c = 2 pi / fps and te = 1 / fps are formed on the host in f64. */
#ifndef IMM_TRACK_H
#define IMM_TRACK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One step of the rule for F faces, one thread per face, 64 per block.
 * Inputs: mu f32 [F, K, 2], the pose head's landmarks (y, x) in [-1, 1]; boxes int32 [F, 5], the rows (image, y0, x0, y1, x1) this
 * frame was cut with; hw int32 [n_images, 2], the sizes of the photos those rows index; state as above (read and written).
 * next_image: the image index written into the next rows (the index the next frame has in ITS packed buffer; the caller checks
 * it against that buffer).  init: 1 on the first frame of a clip, else 0.
 * Outputs, each at the pointer of this frame: points f32 [F, K, 2] = p; points_smooth f32 [F, K, 2] = xhat (p with filter_off);
 * boxes_next int32 [F, 5] = (next_image, y0', x0', y1', x1'), which may be the buffer `boxes` itself (a thread reads its row before
 * it writes it); geom_next f32 [F, 4] = ((float)y0', (float)x0', (float)h' / (float)S, (float)w' / (float)S), keypoints.box_geometry
 * of that row; flags int32 [F]: bit 0 lost, bit 1 the next box does not intersect the photo this frame was cut from (also set when
 * the row's image index lies outside [0, n_images): the sizes of the next frame need not be known yet).
 * 0 < F <= 65535, 1 <= K <= 64, 0 < S <= 8192, n_images > 0, next_image >= 0, init 0 or 1, 0 < box_smooth <= 1, min_cutoff, d_cutoff,
 * c and te finite and positive, beta_e finite and >= 0.  Every pointer is read at the launch only; arguments are validated before
 * any HIP call (-1 and imm_last_error()). */
int imm_track_step(const float* mu, const int32_t* boxes, const int32_t* hw, double* state, int K, int S, int F, int n_images,
                   int next_image, int init, double box_smooth, double min_cutoff, double beta_e, double d_cutoff, double c, double te,
                   int filter_off, float* points, float* points_smooth, int32_t* boxes_next, float* geom_next, int32_t* flags,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IMM_TRACK_H */
