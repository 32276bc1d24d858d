/* imm_retarget.h - C-ABI of the re-enactment entry point of libimm_hip.so (ABI 29; imm_amd/csrc/retarget.hip, imm_amd/reenact.py,
 * imm_amd/generation.py ImageGenerator.reenact): the tracked landmarks of ONE driving face become, per frame, the pose of n still source
 * faces, on the device, so a whole clip animates its photos without a device -> host copy.  Included by imm_hip.h, whose conventions
 * hold here: plain pointers and sizes, an explicit hipStream_t as void*, int status (0 = ok) and imm_last_error().
 *
 * THE RULE, per source face i.  All arithmetic is f64, every operation rounded separately (no fma), in the order written here; the only
 * operations are + - * / fabs fmin fmax isfinite (fmin / fmax return the other operand when one is a NaN); results are rounded once to
 * f32.  Sums over the K points run k = 0, 1, .., K - 1 from 0.0.  Points are (y, x), treated as the complex number y + i x;
 *     c (x) d = (c_r * d0 - c_i * d1,  c_r * d1 + c_i * d0)                         the complex product
 * and fit(z, p) is step 3 of imm_track.h, the least-squares similarity of the K points z onto the K points p:
 *     mz[a] = (sum_k z[k][a]) / K,  mp[a] = (sum_k p[k][a]) / K
 *     per k:  u = z[k] - mz,  v = p[k] - mp
 *             den += u0 * u0 + u1 * u1;   ar += u0 * v0 + u1 * v1;   ai += u0 * v1 - u1 * v0
 *     a_r = ar / den,  a_i = ai / den
 *     fit(z, p) = (a = (a_r, a_i), mz, mp, den)
 *
 * Names.  q f32 [K][2]: the driver's points of this frame, in the pixels of its clip.  q0 f64 [K][2]: the anchor, the driver's points
 * of the clip's first frame (with init == 1 the anchor is first set to (double)q).  m f32 [K][2]: the source face's own landmarks in
 * [-1, 1] of its box.  prev f32 [K][2]: the pose to hold.  f32 inputs enter as (double).
 *
 * 1. The driver's frame into the face's frame:  (a, mq0, mm, den_a) = fit(q0, m), the similarity that carries the driver's first-frame
 *    shape onto this face's landmarks.
 * 2. Head motion removed (rigid == 0):  (b, _, mq, den_b) = fit(q0, q);  nb = b_r * b_r + b_i * b_i;  per k:
 *     w = q[k] - mq
 *     q~[k] = mq0 + ((b_r * w0 + b_i * w1) / nb,  (b_r * w1 - b_i * w0) / nb)
 *    the current shape carried back into the anchor's frame (w / b), so that only the expression is left of the motion.
 *    With rigid == 1:  q~ = q.
 * 3. Target.   relative:  t[k] = m[k] + a (x) (q~[k] - q0[k])        the driver's motion since its first frame, added to the face
 *              absolute:  t[k] = mm   + a (x) (q~[k] - mq0)          the driver's shape itself, laid over the face
 * 4. Output.   o[k] = m[k] + gain * (t[k] - m[k]);   out[k] = fmin(fmax(o[k], -1), 1)
 * 5. HELD (flag bit 0): out = prev, copied bit for bit, when
 *     driver_flags & 1 (imm_track_step lost the driver on this frame), or
 *     some q, q0 or m of the face is not finite, or
 *     den_a == 0 (the driver's first-frame points coincide), or na = a_r * a_r + a_i * a_i == 0 (the face's own landmarks coincide:
 *     every v of the fit is then exactly 0, and so is a), or, with rigid == 0, den_b == 0 or nb == 0, or
 *     some o[k][a] is not finite (tested in front of the clamp, whose fmin / fmax would turn a NaN into a bound).
 *
 * What follows from the order of operations: a still driver (q == q0) gives out == m exactly in relative mode, and gain == 0 gives
 * out == m for every finite t. */
#ifndef IMM_RETARGET_H
#define IMM_RETARGET_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One frame of the rule for n source faces, one thread per face, 64 per block.
 * Inputs: q f32 [K, 2] (a frame's points or points_smooth row of the ONE driver face, as imm_track_step wrote it); anchor f64 [K, 2],
 * persistent across the frames of a clip (read; written only with init == 1, when no thread reads it); driver_flags int32 [1], that
 * frame's imm_track_step flags of the driver; m f32 [n, K, 2]; prev f32 [n, K, 2]; init: 1 on the first frame of a clip, else 0;
 * relative, rigid: 0 or 1; gain finite in [0, 4].
 * Outputs: out f32 [n, K, 2], which may be the buffer `prev` itself (a thread reads its row before it writes it; out overlaps no
 * other input); flags int32 [n], bit 0 held.
 * 0 < n <= 65535, 1 <= K <= 64.  Every pointer is read at the launch only; arguments are validated before any HIP call (-1 and
 * imm_last_error()). */
int imm_retarget(const float* q, double* anchor, const int32_t* driver_flags, const float* m, const float* prev, int K, int n, int init,
                 int relative, int rigid, double gain, float* out, int32_t* flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IMM_RETARGET_H */
