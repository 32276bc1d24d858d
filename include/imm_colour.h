/* imm_colour.h - C-ABI of the colour-matching entry points of libimm_hip.so (ABI 32; imm_amd/csrc/colour.hip, imm_amd/csrc/morph.hip,
 * imm_amd/morphing.py, imm_amd/inference.py LandmarkDetector.morph(colour=...) and LandmarkDetector.colour_stats): the donor's pixels
 * of a morph take the tone of the face they are blended into.  Two photographs are never lit alike; per row and colour channel the mean
 * and the spread of the face's region and of the donor's region give a gain and an offset, which imm_morph_colour_u8 applies to the
 * donor's sample in front of imm_morph_u8's mix.  Included by imm_hip.h, whose conventions hold here: plain pointers and sizes, an
 * explicit hipStream_t as void*, int status (0 = ok) and imm_last_error().  The packed buffers and box rows are those of imm_morph.h.
 *
 * THE RULE
 *
 * Region.  Row b = (image, y0, x0, y1, x1) of a packed u8 HWC buffer, H = y1 - y0, W = x1 - x0.  Its region is every pixel (r, c) of
 * the box that lies inside the photo, 0 <= r < h and 0 <= c < w, AND inside the ellipse inscribed in the box (the corners of a face box
 * are background), decided in integers so that host and device agree on every pixel:
 *     a = 2 (r - y0) + 1 - H,   b = 2 (c - x0) + 1 - W          (twice the distance of the pixel's centre from the box's centre)
 *     inside  iff  (a W)^2 + (b H)^2 <= (H W)^2                   in 64 bits: |a| < H and |b| < W, so every term is <= (H W)^2 <= 2^60
 * A row whose image index lies outside [0, n_images), whose box is empty (H <= 0 or W <= 0), whose H W > 2^30 (the bound that keeps the
 * test inside 64 bits) or that has no pixel in its photo has the empty region.
 *
 * Statistics (imm_colour_stats_u8).  sums uint64 [n, 7]: columns 0..2 the sum of v over the region per channel, columns 3..5 the sum of
 * v * v, column 6 the number of pixels.  All arithmetic is integer: the result does not depend on the order of the additions and equals
 * the host's exactly.  The empty region counts 0 and sums 0.
 *
 * Gain (imm_colour_gain).  Per row b and channel, in f64, every operation rounded separately (no fma), using only + - * / sqrt fmin fmax
 * and isfinite, in this order, for the face (a: sums_a) and its donor (b: sums_b):
 *     N = (double)count;  m = S1 / N;  q = S2 / N;  var = fmax(q - m * m, 0);  sd = sqrt(var)
 *     g = sd_b > 0 ? sd_a / sd_b : 1;   g = fmin(fmax(g, 1.0 / max_gain), max_gain)
 *     o = m_a - g * m_b
 *     t = (double)amount[b];   G = 1 + t * (g - 1);   O = t * o
 *     gain[b][ch] = ((float)G, (float)O)
 * A row with count 0 on either side or with an amount that is not finite gets (1, 0) in every channel and bit 0 of flags[b]; every
 * other row gets flags[b] = 0.
 * Consequences of the order of operations.  (a) amount == 0: G = 1 + 0 * (g - 1) = 1 and O = 0 * o = 0 for the finite g and o of a row
 * with pixels on both sides: exactly (1, 0) as values (the zero carries o's sign; gB + -0 = gB, so the bytes do not depend on it).  (b) a donor region equal to the face's own (the same sums): g = x / x = 1 for sd > 0 (and
 * 1 by the rule for sd == 0), o = m - 1 * m = 0: exactly (1, 0) for every amount.  (c) two flat regions of colours ca and cb: m = c N / N
 * = c exactly, sd = 0, g = 1, o = ca - cb, and with amount 1 the corrected donor colour cb * 1 + (ca - cb) is ca.
 *
 * Morph with colour (imm_morph_colour_u8).  imm_morph_u8 (imm_morph.h) with one step between the donor's sample gB and the mix, in f32,
 * per channel, every operation rounded separately (no fma):
 *     gB' = gB * G + O,        (G, O) = gain[b][ch]
 * and the mix takes gB' in place of gB: mix = gA + texture[b] * (gB' - gA).  Everything else - rows, links, ACTIVE rows, the ramp, the
 * rounding after every row - is imm_morph_u8's.  gain (1, 0) gives gB * 1 + 0 = gB and hence the bytes of imm_morph_u8.  gain never
 * reaches an address: whatever it holds (NaN and inf included) only pixel values change, and the final clamp keeps them bytes. */
#ifndef IMM_COLOUR_H
#define IMM_COLOUR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The statistics.  buf, offsets int64 [n_images], hw int32 [n_images, 2]: a packed u8 HWC buffer as imm_morph_u8 reads it, READ ONLY;
 * boxes int32 [n, 5].  sums uint64 [n, 7] is cleared on the stream in front of the launch and then accumulated into.  The grid is
 * (blocks, n) of 256 threads in the paste kernels' launch shape (consecutive lanes take consecutive pixels of a photo row, byte-wide
 * loads) with a grid-stride loop, so max_box_pixels (it sizes the grid only: a thread per eight pixels of that box) may understate the boxes.  Per-thread integer sums, a
 * reduction over the wave of 64 and over the block through LDS, then ONE 64-bit integer add per block and column.  No photo byte is
 * addressed outside [0, h) x [0, w) of a photo whose index passed 0 <= image < n_images, whatever the box rows hold.
 * 0 < n <= 65535, n_images > 0, max_box_pixels > 0.  Arguments are validated before any HIP call (-1 and imm_last_error()). */
int imm_colour_stats_u8(const uint8_t* buf, const int64_t* offsets, const int32_t* hw, int n_images, const int32_t* boxes, int n,
                        int max_box_pixels, uint64_t* sums, void* stream);

/* The gain.  sums_a, sums_b uint64 [n, 7] (the face's and the donor's statistics), amount f32 [n], max_gain finite and >= 1.  Writes
 * gain f32 [n, 3, 2] and flags int32 [n].  One thread per (row, channel).  0 < n <= 65535.  Arguments are validated before any HIP
 * call (-1 and imm_last_error()). */
int imm_colour_gain(const uint64_t* sums_a, const uint64_t* sums_b, const float* amount, double max_gain, int n, float* gain,
                    int32_t* flags, void* stream);

/* The morph with colour.  Every argument but gain exactly as imm_morph_u8 takes it, with its bounds and refusals; gain f32 [n, 3, 2]
 * (imm_colour_gain's output for these rows), READ ONLY.  The block's own row keeps its six floats in LDS next to its control points
 * and coefficients (2 KB + 24 bytes); rows met on a link walk read theirs from global memory. */
int imm_morph_colour_u8(const uint8_t* src, uint8_t* dst, const int64_t* offsets, const int32_t* hw, int n_images, const uint8_t* donor,
                        const int64_t* donor_offsets, const int32_t* donor_hw, int n_donor_images, const int32_t* boxes,
                        const int32_t* donor_boxes, const int32_t* links, const float* inv_ramp, const float* texture, const float* ctrl,
                        const float* coef_a, const float* coef_b, const float* gain, int M, int n, int max_box_pixels, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IMM_COLOUR_H */
