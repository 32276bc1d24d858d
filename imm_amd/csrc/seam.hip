// seam.hip — the ring of a seamless morph on gfx950 (imm_amd/inference.py LandmarkDetector.morph(mask='hull', seamless=...),
// imm_amd/morphing.py).  The rule is stated once, in include/imm_seam.h; in short:
//
//   imm_seam_fit   per row: B samples of the outline of the grown hull cut with the box, each where the ray from the landmarks' centroid
//                  along dirs[s] leaves the region (f64, every operation rounded separately, only + - * / and comparisons: bit-identical
//                  to the numpy restatement, as imm_hull_fit is), and at each sample the colour difference own photo - morph's mix (f32,
//                  through morph_common.h: the morph's own text and hence its order of operations)
//
// (imm_morph_seam_u8, which weighs the differences into a correction per pixel, is morph.hip's kernel in its SEAM instantiations.)
// One workgroup of B threads per row, one thread per sample; three phases with a barrier between them:
//   1 ring     the centroid (summed in index order by every thread for itself, as hull_grow does), s0 of every line, the sample's t
//   2 flags    every thread for itself from the B samples' verdicts in LDS; the ring point, or the centroid in a flagged row
//   3 diff     the two splines at the sample's place (M logf), five bilinear samples, own - mix
// B * (K + 4) line evaluations and B * M logf a row: not a hot path, and kept plain; ctrl and the coefficients are read from global
// memory at addresses the whole block shares.  Addressing: every index is formed from b < n, s < B, k < K and j < M alone and every
// sampling tap is clamped to a photo with pixels whose index passed its range check; what poses, boxes, edges, dirs, ctrl and the
// coefficients hold never reaches an address.
#include "morph_common.h"

struct SeamRing {
  double cy, cx, t;
  int bad;                     // bit 0 of the row's flags, as this thread sees it (every thread sees the same)
};

// one line (ny, nx, d) of the region against the centroid and the sample's direction: is the centroid strictly inside it, and where
// does the ray leave it
__device__ __forceinline__ void seam_line(SeamRing& o, double ny, double nx, double d, double uy, double ux) {
#pragma clang fp contract(off)   // every operation rounded separately, as the host restatement's
  const double a = ny * o.cy, c = nx * o.cx;
  const double s0 = (a + c) + d;
  if (!(s0 > 0.0)) o.bad = 1;
  const double gy = ny * uy, gx = nx * ux;
  const double g = gy + gx;
  if (g < 0.0) o.t = fmin(o.t, s0 / (-g));
}

// the centroid as hull_points and hull_grow form it, and the sample's t over the row's K lines and then the four sides
__device__ __forceinline__ SeamRing seam_ring(const float* __restrict__ poses, const int32_t* __restrict__ boxes,
                                              const float* __restrict__ edges, int hull_flag, double uy, double ux, int K, int b) {
#pragma clang fp contract(off)
  const double H = (double)((int64_t)boxes[5 * b + 3] - boxes[5 * b + 1]), W = (double)((int64_t)boxes[5 * b + 4] - boxes[5 * b + 2]);
  const double hh = 0.5 * H, hw = 0.5 * W;
  const float* p = poses + (int64_t)b * K * 2;
  double sy = ((double)p[0] + 1.0) * hh, sx = ((double)p[1] + 1.0) * hw;
  for (int i = 1; i < K; ++i) {
    sy = sy + ((double)p[2 * i] + 1.0) * hh;
    sx = sx + ((double)p[2 * i + 1] + 1.0) * hw;
  }
  SeamRing o;
  o.cy = sy / (double)K; o.cx = sx / (double)K;
  o.bad = hull_flag != 0 || !(__builtin_isfinite(o.cy) && __builtin_isfinite(o.cx));
  o.t = __builtin_huge_val();
  const float* e = edges + (int64_t)b * K * 3;
  for (int k = 0; k < K; ++k) seam_line(o, (double)e[3 * k], (double)e[3 * k + 1], (double)e[3 * k + 2], uy, ux);
  seam_line(o, 1.0, 0.0, 0.0, uy, ux);
  seam_line(o, -1.0, 0.0, H - 1.0, uy, ux);
  seam_line(o, 0.0, 1.0, 0.0, uy, ux);
  seam_line(o, 0.0, -1.0, W - 1.0, uy, ux);
  return o;
}

// the difference at the fractional place (by, bx) of row b's box: the own photo's sample minus the morph's mix there; out stays 0 where
// the row pastes nothing or a place is not finite
__device__ __forceinline__ void seam_diff(float by, float bx, int b, const int32_t* __restrict__ boxes, const uint8_t* __restrict__ src,
                                          const int64_t* __restrict__ offs, const int32_t* __restrict__ hw, int n_images,
                                          const uint8_t* __restrict__ donor, const int64_t* __restrict__ doffs,
                                          const int32_t* __restrict__ dhw, int n_donor, const int32_t* __restrict__ dboxes,
                                          const float* __restrict__ texture, const float* __restrict__ ctrl,
                                          const float* __restrict__ coef_a, const float* __restrict__ coef_b,
                                          const float* __restrict__ gain, int M, float* __restrict__ out) {
#pragma clang fp contract(off)
  PastePhoto ph;
  if (!paste_photo(boxes, offs, hw, n_images, b, ph) || ph.sh <= 0 || ph.sw <= 0) return;
  MorphRow q;
  q.s = spline_box(boxes, b, ctrl + (int64_t)b * 2 * M);
  q.ca = coef_a + (int64_t)b * 2 * (M + 3); q.cb = coef_b + (int64_t)b * 2 * (M + 3);
  q.tex = texture[b];
  morph_donor(dboxes, n_donor, b, q);
  if (q.dimg < 0) return;
  const int dh = dhw[2 * q.dimg], dw = dhw[2 * q.dimg + 1];
  if (dh <= 0 || dw <= 0) return;
  const float* const cf[2] = {q.ca, q.cb};
  float qy, qx, D[2][2], dy, dx, mix[3], own[3];
  spline_displace_at<2>(q.s, cf, M, by, bx, qy, qx, D);
  const float oy = (float)q.s.box.y0 + by, ox = (float)q.s.box.x0 + bx;
  const float ay = oy + q.s.hy * D[0][0], ax = ox + q.s.hx * D[0][1];
  morph_donor_place(q, qy, qx, D[1], dy, dx);
  if (!(isfinite(ay) && isfinite(ax) && isfinite(dy) && isfinite(dx) && isfinite(oy) && isfinite(ox))) return;
  const uint8_t* sp = src + ph.off;
  const uint8_t* dp = donor + doffs[q.dimg];
  if (gain)
    morph_mix<true>(sp, ph.sh, ph.sw, dp, dh, dw, ay, ax, dy, dx, gain + (int64_t)b * 6, q.tex, mix);
  else
    morph_mix<false>(sp, ph.sh, ph.sw, dp, dh, dw, ay, ax, dy, dx, nullptr, q.tex, mix);
  paste_sample_photo(sp, ph.sh, ph.sw, oy, ox, own);
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) out[ch] = own[ch] - mix[ch];
}

__global__ __launch_bounds__(SEAM_MAX_B) void seam_fit_kernel(
    const float* __restrict__ poses, const int32_t* __restrict__ boxes, const float* __restrict__ edges, const int32_t* __restrict__ hull_flags,
    const double* __restrict__ dirs, const uint8_t* __restrict__ src, const int64_t* __restrict__ offs, const int32_t* __restrict__ hw,
    int n_images, const uint8_t* __restrict__ donor, const int64_t* __restrict__ doffs, const int32_t* __restrict__ dhw, int n_donor,
    const int32_t* __restrict__ dboxes, const float* __restrict__ texture, const float* __restrict__ ctrl, const float* __restrict__ coef_a,
    const float* __restrict__ coef_b, const float* __restrict__ gain, int K, int M, int B, float* __restrict__ ring, float* __restrict__ diff,
    int32_t* __restrict__ flags) {
  __shared__ uint8_t bad_t[SEAM_MAX_B];                            // sample s: its t is not finite or not > 0
  const int b = blockIdx.x, s = threadIdx.x;                       // s < B: the block has B threads
  const double uy = dirs[2 * s], ux = dirs[2 * s + 1];
  const SeamRing rg = seam_ring(poses, boxes, edges, hull_flags[b], uy, ux, K, b);
  bad_t[s] = !(__builtin_isfinite(rg.t) && rg.t > 0.0);
  __syncthreads();
  int f = rg.bad ? 1 : 0;
  for (int i = 0; i < B; ++i) f |= bad_t[i] ? 2 : 0;
  float by, bx;
  {
#pragma clang fp contract(off)
    const double ty = rg.t * uy, tx = rg.t * ux;
    by = f ? (float)rg.cy : (float)(rg.cy + ty);
    bx = f ? (float)rg.cx : (float)(rg.cx + tx);
  }
  ring[((int64_t)b * B + s) * 2] = by;
  ring[((int64_t)b * B + s) * 2 + 1] = bx;
  if (s == 0) flags[b] = f;
  float* out = diff + ((int64_t)b * B + s) * 3;
  out[0] = out[1] = out[2] = 0.f;
  if (f) return;
  seam_diff(by, bx, b, boxes, src, offs, hw, n_images, donor, doffs, dhw, n_donor, dboxes, texture, ctrl, coef_a, coef_b, gain, M, out);
}

extern "C" int imm_seam_fit(const float* poses, const int32_t* boxes, const float* grow, const float* edges, const int32_t* hull_flags,
                            const double* dirs, const uint8_t* src, const int64_t* offsets, const int32_t* hw, int n_images,
                            const uint8_t* donor, const int64_t* donor_offsets, const int32_t* donor_hw, int n_donor_images,
                            const int32_t* donor_boxes, const float* texture, const float* ctrl, const float* coef_a, const float* coef_b,
                            const float* gain, int K, int M, int B, int n, float* ring, float* diff, int32_t* flags, void* stream) {
  IMM_REQUIRE(poses && boxes && grow && edges && hull_flags && dirs && src && offsets && hw && donor && donor_offsets && donor_hw &&
                  donor_boxes && texture && ctrl && coef_a && coef_b && ring && diff && flags, "seam_fit: null pointer");
  IMM_REQUIRE(n > 0 && n <= 65535 && n_images > 0 && n_donor_images > 0,
              "seam_fit: 0 < n <= 65535 rows, n_images > 0, n_donor_images > 0 (got %d, %d, %d)", n, n_images, n_donor_images);
  IMM_REQUIRE(K >= 1 && K <= SPLINE_MAX_M, "seam_fit: 1 <= K <= %d landmarks (got %d)", SPLINE_MAX_M, K);
  IMM_REQUIRE(M >= 3 && M <= SPLINE_MAX_M, "seam_fit: 3 <= M <= %d control points (got %d)", SPLINE_MAX_M, M);
  IMM_REQUIRE(B >= SEAM_MIN_B && B <= SEAM_MAX_B, "seam_fit: %d <= B <= %d ring samples (got %d)", SEAM_MIN_B, SEAM_MAX_B, B);
  hipLaunchKernelGGL(seam_fit_kernel, dim3(n), dim3(B), 0, (hipStream_t)stream, poses, boxes, edges, hull_flags, dirs, src, offsets, hw,
                     n_images, donor, donor_offsets, donor_hw, n_donor_images, donor_boxes, texture, ctrl, coef_a, coef_b, gain, K, M, B,
                     ring, diff, flags);
  IMM_CHECK_LAUNCH("imm_seam_fit");
  return 0;
}
