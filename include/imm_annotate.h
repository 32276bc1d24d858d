/* imm_annotate.h - C-ABI of annotation of libimm_hip.so (ABI 38; imm_amd/csrc/annotate.hip, imm_amd/annotation.py, imm_amd/inference.py
 * LandmarkDetector.annotate and annotate_clip): what the detector, the tracker, the quality gate and the hull mask decided, drawn into
 * the u8 photos on the device: the landmarks as markers, the trail of earlier frames, the box frame in the colour of the row's status,
 * the outline of the grown landmark hull and a number per face.  It is an instrument for choosing a gate, a grow or a box_smooth on
 * one's own footage, at the speed the frames are produced.  Included by imm_hip.h, whose conventions hold here: plain pointers and
 * sizes, an explicit hipStream_t as void*, int status (0 = ok) and imm_last_error().  The packed buffers, the box rows (image, y0, x0,
 * y1, x1) and links are those of imm_warp.h; the lines of a hull are imm_hull_fit's (imm_hull.h).
 *
 * THE RULE
 *
 * Points (imm_annotate_points).  The landmarks of a row move from the frame of its box to photo pixels, the convention of imm_hull.h
 * (the inverse of imm_track.h step 1, no half-pixel offset).  In f64 from the f32 and int32 inputs widened, every operation rounded
 * separately (no fma), rounded once to f32:
 *     H = y1 - y0,  W = x1 - x0
 *     py = y0 + (mu_y + 1) * (0.5 * H),  px = x0 + (mu_x + 1) * (0.5 * W)
 * A mu value that is not finite is stored as it is (its own bits), whatever the box.  An empty or inverted box is not special.
 *
 * Paste (imm_annotate_u8).  The skeleton of the paste kernels (imm_warp.h): one owner per photo pixel, the rows of a photo applied in
 * row order along links, a rint after every blend.  A row is ACTIVE when 0 <= image < n_images, H > 0 and W > 0 (in 64 bits).  Its EXTENT
 * is its box grown by pad pixels on every side, each bound saturated to int32; row q covers photo pixel (r, c) when q is ACTIVE and
 * (r, c) lies in its extent.  A blend is imm_compose.h's:
 *     v <- fminf(fmaxf(rintf(v + a * (g - v)), 0), 255)           per channel: the difference, the product, the sum
 * and clamp(x) = fminf(fmaxf(x, 0), 1), which turns a NaN into 0.  Per covered pixel the primitives draw_bits selects are applied in
 * this order; f32 arithmetic is rounded separately in the order written and uses only + - * fabs fmin fmax and comparisons; integer
 * arithmetic is in 64 bits.
 *
 * The row's colour.  s = status == NULL ? 0 : status[q];  i = s == 0 ? 0 : min(1 + the index of the lowest set bit of s, P - 1);
 * colour = palette[i] as floats.  A row is LOST when bit 0 of s is set (imm_track.h's meaning).
 *
 * 1. Box frame (IMM_ANNOTATE_BOX).  For a pixel inside the BOX with min(r - y0, y1 - 1 - r, c - x0, x1 - 1 - c) < thickness: a blend
 *    of the row's colour with a = 1.
 * 2. Hull outline (IMM_ANNOTATE_HULL), not for a LOST row.  With the row's lines (ny_k, nx_k, d_k) = edges[q][k]:
 *        rr = (float)(r - y0),  cc = (float)(c - x0),  dist = +inf
 *        for k = 0 .. K - 1:   s = (ny_k * rr + nx_k * cc) + d_k;   dist = fminf(dist, s)             imm_hull.h's weight, to here
 *        a = clamp((0.5f * (float)thickness + 0.5f) - fabsf(dist))
 *    and, if a > 0, a blend of the row's colour with a.  The outline is drawn over the whole extent.  A flagged hull (0, 0, -inf)
 *    gives dist = -inf and a = 0.
 * 3. and 4. Marks (IMM_ANNOTATE_POINTS), not for a LOST row.  marks[g][q][k] = (my, mx) in photo pixels; group_style[g] = (R, inv2R, h,
 *    alpha) with inv2R = 1 / (2 R) formed by the caller; mark_style[k] = (red, green, blue, shape).  For g = 0 .. G - 1, for k = 0 .. K - 1:
 *        dy = (float)r - my,  dx = (float)c - mx,  ay = fabsf(dy),  ax = fabsf(dx),  lim = R + 2.f
 *        the mark touches the pixel only if ay <= lim and ax <= lim        (a NaN coordinate fails the comparison: nothing is drawn)
 *    Trail groups g < G - 1 (the same landmarks on earlier frames, oldest first) are plain discs:
 *        s = (R * R - (dy * dy + dx * dx)) * inv2R;   a = alpha * clamp(s + 0.5f);   if a > 0, a blend of the mark's colour with a
 *    The markers of group G - 1 take their shape's inside-ness s(dy, dx) in pixels:
 *        shape 0 'v'   fminf(dy + R, ((R - dy) * 0.5f - ax) * 0.8944272f)
 *        shape 1 'o'   (R * R - (dy * dy + dx * dx)) * inv2R
 *        shape 2 's'   R - fmaxf(ay, ax)
 *        shape 3 'd'   (R - (ay + ax)) * 0.70710677f
 *        shape 4 '^'   shape 0 with -dy in place of dy
 *        shape 5 'x'   fminf(h - fminf(fabsf(dy - dx), fabsf(dy + dx)) * 0.70710677f, R - fmaxf(ay, ax))
 *        shape 6 '+'   fminf(h - fminf(ay, ax), R - fmaxf(ay, ax))
 *        any other shape byte draws nothing
 *    and two blends: white (255, 255, 255) with a = alpha * clamp(s + 1.5f) if that is > 0, then the mark's colour with
 *    a = alpha * clamp(s + 0.5f) if that is > 0.  The shapes are those of imm_amd/utils/plot_landmarks.py (MARKERS, in that order).
 * 5. Label (IMM_ANNOTATE_LABEL).  L = labels[q]; nothing is drawn unless 0 <= L <= 9999.  nd = the number of decimal digits of L
 *    (1 for 0), S = label_scale.  With u = (r - y0 - thickness) and t = (c - x0 - thickness): for a pixel inside the BOX with
 *    0 <= u < 9 S and 0 <= t < (6 nd + 1) S:  fr = u / S - 1,  tc = t / S - 1,  di = tc / 6,  fc = tc - 6 di (integer division; tc = -1
 *    is the left margin).  The pixel is white when 0 <= fr < 7, tc >= 0, fc < 5 and bit (4 - fc) of FONT[digit di of L, most
 *    significant first][fr] is set, otherwise the row's colour; a blend with a = 1.  FONT, seven rows of five bits per digit:
 *        0: 0E 11 13 15 19 11 0E   1: 04 0C 04 04 04 04 0E   2: 0E 11 01 02 04 08 1F   3: 1F 02 04 02 01 11 0E   4: 02 06 0A 12 1F 02 02
 *        5: 1F 10 1E 01 01 11 0E   6: 06 08 10 1E 11 11 0E   7: 1F 01 02 04 08 08 08   8: 0E 11 11 0E 11 11 0E   9: 0E 11 11 0F 01 02 0C
 *
 * A LOST row draws its frame and its label only: a lost face's landmarks are not to be believed.  A pixel a row owns and no primitive
 * touches keeps its byte.  status selects one of the P palette entries through the clamped index above, the shape byte selects a
 * formula and a label's digit a font row; nothing else a buffer holds reaches an address: whatever marks, group_style, edges, status and
 * labels hold, only bytes inside the extents of ACTIVE rows change.
 *
 * Consequences.  (a) draw_bits == 0 returns the photos bit for bit.  (b) With alpha == 1 a pixel with s >= 0.5 takes the mark's colour
 * exactly: at the centre of a mark placed on a pixel, every shape at R >= 2 and h >= 0.5.  (c) A pixel farther than R + 2 (Chebyshev)
 * from every mark, on no frame, label or hull line, keeps its byte; pad >= R + 2 lets every mark inside the box be drawn whole.
 * (d) For a mark on a pixel centre dy and dx are integers: shapes o, s, d, + and x are symmetric under both flips, ^ is v flipped. */
#ifndef IMM_ANNOTATE_H
#define IMM_ANNOTATE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IMM_ANNOTATE_POINTS 1
#define IMM_ANNOTATE_BOX 2
#define IMM_ANNOTATE_HULL 4
#define IMM_ANNOTATE_LABEL 8
#define IMM_ANNOTATE_MAX_GROUPS 16
#define IMM_ANNOTATE_MAX_PAD 64

/* The points.  mu f32 [n, K, 2] and boxes int32 [n, 5], READ ONLY; writes points f32 [n, K, 2], never mu.  One workgroup of 64 lanes per
 * row.  0 < n <= 65535, 1 <= K <= 80.  Arguments are validated before any HIP call (-1 and imm_last_error()). */
int imm_annotate_points(const float* mu, const int32_t* boxes, int K, int n, float* points, void* stream);

/* The paste.  dst u8 (the packed photos, drawn into in place); offsets, hw, boxes, links int32 [n, 2] as imm_warp_u8 takes them; marks f32
 * [G, n, K, 2], group_style f32 [G, 4] and mark_style u8 [K, 4] (needed with IMM_ANNOTATE_POINTS, else not read); edges f32 [n, K, 3]
 * (needed with IMM_ANNOTATE_HULL, else not read); status int32 [n] or NULL; palette u8 [P, 3], 1 <= P <= 32; labels int32 [n] (needed
 * with IMM_ANNOTATE_LABEL, else not read); all READ ONLY, never dst.  0 <= draw_bits < 16, 1 <= thickness <= 16, 0 <= pad <= 64,
 * 1 <= label_scale <= 8, 1 <= K <= 80, 1 <= G <= 16, 0 < n <= 65535, n_images > 0, max_box_pixels > 0 (it sizes the grid only: give the
 * largest extent).  The block's own row keeps its G * K marks (at most 10 240 bytes) and its 3 K lines (at most 960 bytes) in static
 * LDS; rows met on a link walk read theirs from global memory. */
int imm_annotate_u8(uint8_t* dst, const int64_t* offsets, const int32_t* hw, int n_images, const int32_t* boxes, const int32_t* links,
                    const float* marks, const float* group_style, const uint8_t* mark_style, const float* edges, const int32_t* status,
                    const uint8_t* palette, int P, const int32_t* labels, int draw_bits, int thickness, int pad, int label_scale, int K,
                    int G, int n, int max_box_pixels, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IMM_ANNOTATE_H */
