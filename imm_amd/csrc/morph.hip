// morph.hip — two faces blended in shape and texture from their own pixels on gfx950 (imm_amd/inference.py LandmarkDetector.morph,
// imm_amd/morphing.py).  The rule is stated once, in include/imm_morph.h; in short:
//
//   imm_morph_poses  p = (1 - s) mu_a + s mu_b per element, written twice (poses2 [2, n, K, 2]) next to (mu_a, mu_b) (mu2 [2, n, K, 2]): the
//                    inputs of ONE imm_warp_fit launch over 2 n rows, which fits the two displacement splines of every row (target frame ->
//                    own frame, target frame -> donor frame) on shared control points
//   imm_morph_u8     per photo pixel of a row's box: one basis evaluation u_j = U(|q - ctrl_j|^2) feeds both coefficient sets; the row's own
//                    photo sampled at (r, c) + (H/2, W/2) DA, the donor photo at the donor box's image of q + DB, the two samples mixed by
//                    texture[b] and blended over the canvas with imm_warp_u8's ramp, rounding, row order and links
//
// Poses: one thread per float, nothing shared.  Morph: the paste skeleton of paste_common.h, which states the launch shape, the ownership
// of a pixel and the addressing argument (the donor's taps are clamped to a photo whose index passed 0 <= donor image < n_donor_images).
// The row's ctrl [M][2], coef_a and coef_b [M + 3][2] sit in 2.0 KB of LDS, read by every lane at the same address (broadcasts).  The
// kernel is bound by its M logf per pixel, as imm_warp_u8 is: the second spline adds two multiply-adds per control point and four more
// byte taps per pixel, no logarithm.  Rows met on a link walk read their ctrl and coef through L2.
// A row is ACTIVE when its donor image index lies in [0, n_donor_images) and its donor box has H > 0 and W > 0; a row that is not writes
// nothing and owns nothing (the walks pass over it), so the rows of a call give the same bytes however they are split into launches.
// imm_morph_colour_u8 (include/imm_colour.h) is the same kernel in a second, compile-time instantiation: the donor's sample takes
// gB * G + O per channel in front of the mix, (G, O) = gain[b][ch] f32 [n, 3, 2].  The block's own row keeps its six floats in LDS, rows met
// on a link walk read theirs through L2; gain reaches no address.  imm_morph_u8's instantiation carries none of it.
// imm_morph_hull_u8 (include/imm_hull.h) is a third compile-time flag on the same kernel, with and without COLOUR: per pixel the row's K
// lines (ny, nx, d) = edges[b][k] f32 [n, K, 3] (imm_hull_fit's) give dist = min_k (ny rr + nx cc) + d and w = clamp(dist * inv_soft[b], 0, 1);
// a pixel with !(w > 0) is left alone BEFORE the spline is evaluated (it skips the M logf that bound the kernel), every other takes
// paste_ramp(...) * w for its blend weight.  covers() stays the box test, so ownership, row order and links are what they were.  The
// block's own row keeps its 3 K floats and its inv_soft in LDS (at most 964 bytes), rows met on a link walk read theirs through L2; edges
// and inv_soft reach no address.  The two instantiations without HULL carry none of it.
// imm_morph_seam_u8 (include/imm_seam.h) is a fourth compile-time flag, on the HULL instantiations, with and without COLOUR: per pixel
// with w > 0 the mean-value coordinates of the pixel in the row's ring [B][2] weigh the row's diff [B][3] into a correction r, and mix
// takes seamless[b] * r before the blend.  B sqrtf and 2 B divisions a pixel, all correctly rounded, on top of the M logf.  The block's own
// row keeps its 5 B floats in LDS (at most 5 KB), rows met on a link walk read theirs through L2; ring, diff and seamless reach no
// address.  The instantiations without SEAM carry none of it.
#include "morph_common.h"

__global__ __launch_bounds__(256) void morph_poses_kernel(const float* __restrict__ mu_a, const float* __restrict__ mu_b,
                                                          const float* __restrict__ shape, int K2, int64_t total, float* __restrict__ poses2,
                                                          float* __restrict__ mu2) {
#pragma clang fp contract(off)   // every operation rounded separately, as the host restatement's
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const float s = shape[i / K2];
  const float a = mu_a[i], b = mu_b[i];
  const float wa = 1.f - s;
  const float ta = wa * a, tb = s * b;
  const float p = ta + tb;
  poses2[i] = p; poses2[total + i] = p;
  mu2[i] = a; mu2[total + i] = b;
}

struct MorphColourRow : MorphRow {
  const float* g;             // its gain [3][2]: (G, O) per channel
};

template <class Base>
struct MorphHullRow : Base {
  const float* e;             // its lines [K][3]: (ny, nx, d) per slot
  const float* is;            // its inv_soft
};

template <class Base>
struct MorphSeamRow : Base {
  const float* rg;            // its ring [B][2]: (by, bx) per sample, box-relative pixels
  const float* df;            // its diff [B][3]
  float amt;                  // its seamless
};

// the membrane at photo pixel (r, c) of a row's box: the mean-value coordinates of the pixel in the ring weigh the ring's diffs.  th of
// the pair (s, s + 1) is tan of half the angle the pair subtends; it is formed once and carried to the next sample.
__device__ __forceinline__ void seam_field(const float* __restrict__ rg, const float* __restrict__ df, int B, const PasteBox& box, int r,
                                           int c, float (&out)[3]) {
#pragma clang fp contract(off)
  const float rr = (float)(r - box.y0), cc = (float)(c - box.x0);
  float py = rg[2 * (B - 1)] - rr, px = rg[2 * (B - 1) + 1] - cc;                       // sample B - 1
  float l = sqrtf(py * py + px * px);
  float ny = rg[0] - rr, nx = rg[1] - cc;                                              // sample 0
  float nl = sqrtf(ny * ny + nx * nx);
  float th;
  {
    const float cr = py * nx - px * ny, dt = py * ny + px * nx;
    th = cr / (l * nl + dt);
  }
  float R[3] = {0.f, 0.f, 0.f}, W = 0.f;
  int zero = -1;
  for (int s = 0; s < B; ++s) {
    const int s1 = s + 1 < B ? s + 1 : 0;
    py = ny; px = nx; l = nl;
    ny = rg[2 * s1] - rr; nx = rg[2 * s1 + 1] - cc;
    nl = sqrtf(ny * ny + nx * nx);
    const float cr = py * nx - px * ny, dt = py * ny + px * nx;
    const float tn = cr / (l * nl + dt);
    const float w = (th + tn) / l;
    th = tn;
    if (l == 0.f && zero < 0) zero = s;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) R[ch] = R[ch] + w * df[3 * s + ch];
    W = W + w;
  }
  if (zero >= 0) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) out[ch] = df[3 * zero + ch];
  } else if (W > 0.f && isfinite(W) && isfinite(R[0]) && isfinite(R[1]) && isfinite(R[2])) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) out[ch] = R[ch] / W;
  } else {
    out[0] = out[1] = out[2] = 0.f;
  }
}

// the hull weight of photo pixel (r, c) in a row's box: w = clamp(min_k ((ny_k rr + nx_k cc) + d_k) * inv_soft, 0, 1); a NaN s never
// lowers the minimum, a NaN product becomes 0 in the first clamp
__device__ __forceinline__ float hull_weight(const float* __restrict__ e, float inv_soft, int K, const PasteBox& box, int r, int c) {
#pragma clang fp contract(off)
  const float rr = (float)(r - box.y0), cc = (float)(c - box.x0);
  float dist = __builtin_huge_valf();
  for (int k = 0; k < K; ++k) {
    const float a = e[3 * k] * rr, b = e[3 * k + 1] * cc;
    const float s = (a + b) + e[3 * k + 2];
    dist = fminf(dist, s);
  }
  return fminf(fmaxf(dist * inv_soft, 0.f), 1.f);
}

template <bool COLOUR, bool HULL = false, bool SEAM = false>
struct MorphPolicy {
  static_assert(HULL || !SEAM, "the membrane goes with the hull mask");
  typedef typename std::conditional<COLOUR, MorphColourRow, MorphRow>::type BoxRow;
  typedef typename std::conditional<HULL, MorphHullRow<BoxRow>, BoxRow>::type MaskRow;
  typedef typename std::conditional<SEAM, MorphSeamRow<MaskRow>, MaskRow>::type Row;
  const int32_t *boxes, *dboxes;
  const float *inv_ramp, *texture, *ctrl, *coef_a, *coef_b, *gain, *edges, *inv_soft, *ring, *diff, *seamless;
  const uint8_t* sp;          // the row's photo in the ORIGINAL buffer
  const uint8_t* donor;
  const int64_t* doffs;
  const int32_t* dhw;
  int sh, sw, n_donor, M, K, B;
  Row own;

  // row j with its arrays at ct, ca, cb (and its gain at g, its lines at e, its inv_soft at is, its ring at rg, its diff at df)
  __device__ __forceinline__ Row row(int j, const float* ct, const float* ca, const float* cb, const float* g, const float* e,
                                     const float* is, const float* rg, const float* df) const {
    Row q;
    if constexpr (COLOUR) q.g = g;
    if constexpr (HULL) {
      q.e = e; q.is = is;
    }
    if constexpr (SEAM) {
      q.rg = rg; q.df = df;
      q.amt = seamless[j];
    }
    q.s = spline_row(boxes, inv_ramp, j, ct);
    q.ca = ca; q.cb = cb;
    q.tex = texture[j];
    morph_donor(dboxes, n_donor, j, q);
    return q;
  }
  __device__ __forceinline__ Row row(int j) const {
    return row(j, ctrl + (int64_t)j * 2 * M, coef_a + (int64_t)j * 2 * (M + 3), coef_b + (int64_t)j * 2 * (M + 3),
               COLOUR ? gain + (int64_t)j * 6 : nullptr, HULL ? edges + (int64_t)j * 3 * K : nullptr, HULL ? inv_soft + j : nullptr,
               SEAM ? ring + (int64_t)j * 2 * B : nullptr, SEAM ? diff + (int64_t)j * 3 * B : nullptr);
  }
  __device__ __forceinline__ bool covers(const Row& q, int r, int c) const { return q.dimg >= 0 && paste_inside(q.s.box, r, c); }
  // the row's own photo sampled at (r, c) + (H/2, W/2) DA, the donor photo at the donor box's image of q + DB (COLOUR: times its gain,
  // plus its offset), mixed by tex (HULL: only where the row's hull weight is > 0, and blended by the ramp times that weight; SEAM: the
  // mix takes the row's share of the membrane first)
  __device__ __forceinline__ void apply(const Row& q, int r, int c, float (&v)[3]) const {
#pragma clang fp contract(off)
    [[maybe_unused]] float w = 1.f;
    if constexpr (HULL) {
      w = hull_weight(q.e, *q.is, K, q.s.box, r, c);
      if (!(w > 0.f)) return;                                      // outside the hull: no spline, no sample
    }
    const float* const cf[2] = {q.ca, q.cb};
    float qy, qx, D[2][2], by, bx, mix[3];
    spline_displace<2>(q.s, cf, M, r, c, qy, qx, D);
    const float ay = (float)r + q.s.hy * D[0][0], ax = (float)c + q.s.hx * D[0][1];
    morph_donor_place(q, qy, qx, D[1], by, bx);
    if (!(isfinite(ay) && isfinite(ax) && isfinite(by) && isfinite(bx))) return;
    const float* g = nullptr;
    if constexpr (COLOUR) g = q.g;
    morph_mix<COLOUR>(sp, sh, sw, donor + doffs[q.dimg], dhw[2 * q.dimg], dhw[2 * q.dimg + 1], ay, ax, by, bx, g, q.tex, mix);
    if constexpr (SEAM) {
      float fr[3];
      seam_field(q.rg, q.df, B, q.s.box, r, c, fr);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float sr = q.amt * fr[ch];
        mix[ch] = mix[ch] + sr;
      }
    }
    const float ramp = paste_ramp(q.s.box, r, c, q.s.iry, q.s.irx);
    if constexpr (HULL) {
      paste_blend(v, mix, ramp * w);
    } else {
      paste_blend(v, mix, ramp);
    }
  }
};

template <bool COLOUR, bool HULL = false, bool SEAM = false>
__global__ __launch_bounds__(256) void morph_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                       const int64_t* __restrict__ offs, const int32_t* __restrict__ hw, int n_images,
                                                       const uint8_t* __restrict__ donor, const int64_t* __restrict__ doffs,
                                                       const int32_t* __restrict__ dhw, int n_donor, const int32_t* __restrict__ boxes,
                                                       const int32_t* __restrict__ dboxes, const int32_t* __restrict__ links,
                                                       const float* __restrict__ inv_ramp, const float* __restrict__ texture,
                                                       const float* __restrict__ ctrl, const float* __restrict__ coef_a,
                                                       const float* __restrict__ coef_b, const float* __restrict__ gain, int M, int n,
                                                       const float* __restrict__ edges, const float* __restrict__ inv_soft, int K,
                                                       const float* __restrict__ ring, const float* __restrict__ diff,
                                                       const float* __restrict__ seamless, int B) {
  __shared__ float ct_s[2 * SPLINE_MAX_M];
  __shared__ float ca_s[2 * SPLINE_MAX_N];
  __shared__ float cb_s[2 * SPLINE_MAX_N];
  __shared__ float g_s[COLOUR ? 6 : 1];                             // (without COLOUR: never referenced, takes no LDS)
  __shared__ float e_s[HULL ? 3 * SPLINE_MAX_M + 1 : 1];            // its lines, then its inv_soft (without HULL: likewise)
  __shared__ float m_s[SEAM ? 5 * SEAM_MAX_B : 1];                  // its ring [B][2], then its diff [B][3] (without SEAM: likewise)
  const int b = blockIdx.y;
  PastePhoto ph;
  if (!paste_photo(boxes, offs, hw, n_images, b, ph)) return;      // uniform over the block: no barrier is skipped by part of it
  MorphPolicy<COLOUR, HULL, SEAM> pol{boxes, dboxes, inv_ramp, texture, ctrl, coef_a, coef_b, gain, edges, inv_soft, ring, diff, seamless,
                                      src + ph.off, donor, doffs, dhw, ph.sh, ph.sw, n_donor, M, K, B};
  pol.own = pol.row(b, ct_s, ca_s, cb_s, g_s, e_s, e_s + 3 * SPLINE_MAX_M, m_s, m_s + 2 * SEAM_MAX_B);
  if (pol.own.dimg < 0) return;                                    // not active: uniform as well
  for (int i = threadIdx.x; i < 2 * M; i += 256) ct_s[i] = ctrl[(int64_t)b * 2 * M + i];
  for (int i = threadIdx.x; i < 2 * (M + 3); i += 256) {
    ca_s[i] = coef_a[(int64_t)b * 2 * (M + 3) + i];
    cb_s[i] = coef_b[(int64_t)b * 2 * (M + 3) + i];
  }
  if constexpr (COLOUR) {
    if (threadIdx.x < 6) g_s[threadIdx.x] = gain[(int64_t)b * 6 + threadIdx.x];
  }
  if constexpr (HULL) {
    for (int i = threadIdx.x; i < 3 * K; i += 256) e_s[i] = edges[(int64_t)b * 3 * K + i];
    if (threadIdx.x == 0) e_s[3 * SPLINE_MAX_M] = inv_soft[b];
  }
  if constexpr (SEAM) {
    for (int i = threadIdx.x; i < 2 * B; i += 256) m_s[i] = ring[(int64_t)b * 2 * B + i];
    for (int i = threadIdx.x; i < 3 * B; i += 256) m_s[2 * SEAM_MAX_B + i] = diff[(int64_t)b * 3 * B + i];
  }
  __syncthreads();
  paste_rows(pol, pol.own.s.box, ph, dst + ph.off, boxes, links, n);
}

extern "C" int imm_morph_poses(const float* mu_a, const float* mu_b, const float* shape, int K, int n, float* poses2, float* mu2,
                               void* stream) {
  IMM_REQUIRE(mu_a && mu_b && shape && poses2 && mu2, "morph_poses: null pointer");
  IMM_REQUIRE(n > 0 && n <= 32767, "morph_poses: 0 < n <= 32767 rows, so that one fit serves 2 n (got %d)", n);
  IMM_REQUIRE(K >= 1 && K <= SPLINE_MAX_M, "morph_poses: 1 <= K <= %d landmarks (got %d)", SPLINE_MAX_M, K);
  const int64_t total = (int64_t)n * K * 2;
  hipLaunchKernelGGL(morph_poses_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, mu_a, mu_b, shape, 2 * K,
                     total, poses2, mu2);
  IMM_CHECK_LAUNCH("imm_morph_poses");
  return 0;
}

// the checks and the launch of imm_morph_u8, imm_morph_colour_u8, imm_morph_hull_u8 and imm_morph_seam_u8 (gain != nullptr: the COLOUR
// instantiations; edges != nullptr: the HULL ones; ring != nullptr: the SEAM ones)
static int morph_launch(const char* name, const uint8_t* src, uint8_t* dst, const int64_t* offsets, const int32_t* hw, int n_images,
                        const uint8_t* donor, const int64_t* donor_offsets, const int32_t* donor_hw, int n_donor_images, const int32_t* boxes,
                        const int32_t* donor_boxes, const int32_t* links, const float* inv_ramp, const float* texture, const float* ctrl,
                        const float* coef_a, const float* coef_b, const float* gain, const float* edges, const float* inv_soft, int K, int M,
                        int n, int max_box_pixels, void* stream, const float* ring = nullptr, const float* diff = nullptr,
                        const float* seamless = nullptr, int B = 0) {
  IMM_REQUIRE(src && dst && offsets && hw && donor && donor_offsets && donor_hw && boxes && donor_boxes && links && inv_ramp && texture &&
                  ctrl && coef_a && coef_b, "%s: null pointer", name);
  IMM_REQUIRE(src != dst, "%s: dst must be a copy of src, not src itself (every row samples the original pixels)", name);
  IMM_REQUIRE(donor != dst, "%s: the donor buffer is read only and must not be dst", name);
  IMM_REQUIRE(n > 0 && n <= 65535 && n_images > 0 && n_donor_images > 0,
              "%s: 0 < n <= 65535 rows, n_images > 0, n_donor_images > 0 (got %d, %d, %d)", name, n, n_images, n_donor_images);
  IMM_REQUIRE(M >= 3 && M <= SPLINE_MAX_M, "%s: 3 <= M <= %d control points (got %d)", name, SPLINE_MAX_M, M);
  IMM_REQUIRE(max_box_pixels > 0, "%s: max_box_pixels > 0 (got %d)", name, max_box_pixels);
  const dim3 grid(paste_grid_x(max_box_pixels), n);
#define MORPH_LAUNCH(kernel)                                                                                                             \
  hipLaunchKernelGGL(kernel, grid, dim3(256), 0, (hipStream_t)stream, src, dst, offsets, hw, n_images, donor, donor_offsets, donor_hw,      \
                     n_donor_images, boxes, donor_boxes, links, inv_ramp, texture, ctrl, coef_a, coef_b, gain, M, n, edges, inv_soft, K, ring, \
                     diff, seamless, B)
  if (ring) {
    if (gain)
      MORPH_LAUNCH((morph_u8_kernel<true, true, true>));
    else
      MORPH_LAUNCH((morph_u8_kernel<false, true, true>));
  } else if (edges) {
    if (gain)
      MORPH_LAUNCH((morph_u8_kernel<true, true>));
    else
      MORPH_LAUNCH((morph_u8_kernel<false, true>));
  } else if (gain) {
    MORPH_LAUNCH(morph_u8_kernel<true>);
  } else {
    MORPH_LAUNCH(morph_u8_kernel<false>);
  }
#undef MORPH_LAUNCH
  return 0;
}

extern "C" int imm_morph_u8(const uint8_t* src, uint8_t* dst, const int64_t* offsets, const int32_t* hw, int n_images, const uint8_t* donor,
                            const int64_t* donor_offsets, const int32_t* donor_hw, int n_donor_images, const int32_t* boxes,
                            const int32_t* donor_boxes, const int32_t* links, const float* inv_ramp, const float* texture, const float* ctrl,
                            const float* coef_a, const float* coef_b, int M, int n, int max_box_pixels, void* stream) {
  const int rc = morph_launch("morph_u8", src, dst, offsets, hw, n_images, donor, donor_offsets, donor_hw, n_donor_images, boxes, donor_boxes,
                              links, inv_ramp, texture, ctrl, coef_a, coef_b, nullptr, nullptr, nullptr, 0, M, n, max_box_pixels, stream);
  if (rc) return rc;
  IMM_CHECK_LAUNCH("imm_morph_u8");
  return 0;
}

extern "C" int imm_morph_colour_u8(const uint8_t* src, uint8_t* dst, const int64_t* offsets, const int32_t* hw, int n_images,
                                   const uint8_t* donor, const int64_t* donor_offsets, const int32_t* donor_hw, int n_donor_images,
                                   const int32_t* boxes, const int32_t* donor_boxes, const int32_t* links, const float* inv_ramp,
                                   const float* texture, const float* ctrl, const float* coef_a, const float* coef_b, const float* gain, int M,
                                   int n, int max_box_pixels, void* stream) {
  IMM_REQUIRE(gain, "morph_colour_u8: null pointer");
  const int rc = morph_launch("morph_colour_u8", src, dst, offsets, hw, n_images, donor, donor_offsets, donor_hw, n_donor_images, boxes,
                              donor_boxes, links, inv_ramp, texture, ctrl, coef_a, coef_b, gain, nullptr, nullptr, 0, M, n, max_box_pixels, stream);
  if (rc) return rc;
  IMM_CHECK_LAUNCH("imm_morph_colour_u8");
  return 0;
}

extern "C" int imm_morph_hull_u8(const uint8_t* src, uint8_t* dst, const int64_t* offsets, const int32_t* hw, int n_images,
                                 const uint8_t* donor, const int64_t* donor_offsets, const int32_t* donor_hw, int n_donor_images,
                                 const int32_t* boxes, const int32_t* donor_boxes, const int32_t* links, const float* inv_ramp,
                                 const float* texture, const float* ctrl, const float* coef_a, const float* coef_b, const float* gain,
                                 const float* edges, const float* inv_soft, int K, int M, int n, int max_box_pixels, void* stream) {
  IMM_REQUIRE(edges && inv_soft, "morph_hull_u8: null pointer");
  IMM_REQUIRE(K >= 1 && K <= SPLINE_MAX_M, "morph_hull_u8: 1 <= K <= %d landmarks (got %d)", SPLINE_MAX_M, K);
  const int rc = morph_launch("morph_hull_u8", src, dst, offsets, hw, n_images, donor, donor_offsets, donor_hw, n_donor_images, boxes,
                              donor_boxes, links, inv_ramp, texture, ctrl, coef_a, coef_b, gain, edges, inv_soft, K, M, n, max_box_pixels,
                              stream);
  if (rc) return rc;
  IMM_CHECK_LAUNCH("imm_morph_hull_u8");
  return 0;
}

extern "C" int imm_morph_seam_u8(const uint8_t* src, uint8_t* dst, const int64_t* offsets, const int32_t* hw, int n_images,
                                 const uint8_t* donor, const int64_t* donor_offsets, const int32_t* donor_hw, int n_donor_images,
                                 const int32_t* boxes, const int32_t* donor_boxes, const int32_t* links, const float* inv_ramp,
                                 const float* texture, const float* ctrl, const float* coef_a, const float* coef_b, const float* gain,
                                 const float* edges, const float* inv_soft, const float* ring, const float* diff, const float* seamless,
                                 int K, int M, int B, int n, int max_box_pixels, void* stream) {
  IMM_REQUIRE(edges && inv_soft && ring && diff && seamless, "morph_seam_u8: null pointer");
  IMM_REQUIRE(K >= 1 && K <= SPLINE_MAX_M, "morph_seam_u8: 1 <= K <= %d landmarks (got %d)", SPLINE_MAX_M, K);
  IMM_REQUIRE(B >= SEAM_MIN_B && B <= SEAM_MAX_B, "morph_seam_u8: %d <= B <= %d ring samples (got %d)", SEAM_MIN_B, SEAM_MAX_B, B);
  const int rc = morph_launch("morph_seam_u8", src, dst, offsets, hw, n_images, donor, donor_offsets, donor_hw, n_donor_images, boxes,
                              donor_boxes, links, inv_ramp, texture, ctrl, coef_a, coef_b, gain, edges, inv_soft, K, M, n, max_box_pixels,
                              stream, ring, diff, seamless, B);
  if (rc) return rc;
  IMM_CHECK_LAUNCH("imm_morph_seam_u8");
  return 0;
}
