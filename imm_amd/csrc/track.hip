// track.hip — face tracking on gfx950: after each frame's pose head, the landmarks of every face become the box row the next frame
// is cut with, on the device (imm_amd/tracking.py, imm_amd/inference.py LandmarkDetector.track / .tracker).  The rule is stated
// once, in include/imm_track.h; in short, per face:
//
//   1. source pixels     p = box origin + (mu + 1) / 2 * S * (box side / S)         keypoints.to_source_pixels
//   2. init              anchor shape z0 = p - box centre, anchor sides, filters reset
//   3. similarity fit    a, b of z0 -> p (alignment.fit_similarity); measurement (b_y, b_x, |a|); lost when it is not usable
//   4. box filter        (cy, cx, s) += beta * (measurement - (cy, cx, s))
//   5. next box          sides rint(s * anchor sides) in [2, 2^22], origin rint(centre - side / 2) in [-2^23, 2^23]
//   6. One-Euro filter   per point coordinate, speeds in box heights per second
//
// One thread per face, 64 per block, f64, every operation rounded separately, in the order of the header (the numpy restatement
// of the tests follows it line by line), rounded once to the stored type.  A few microseconds of latency-bound work on at most
// 256 x 64 points: nothing here is tuned.  p is recomputed by source_pixel() in each of the three passes over the points instead of
// being held in 128 registers; the same operations on the same operands give the same bits.
// Addressing: a thread reads and writes only row f < F of every [F, ..] buffer, and hw[img] only after img is checked against
// [0, n_images); the values the device buffers hold never reach an address.
#include "common.h"

__device__ __forceinline__ double track_source_pixel(float mu, double origin, double dS, double scale) {
#pragma clang fp contract(off)
  double t = (double)mu + 1.0;
  t = t * 0.5;
  t = t * dS;
  t = t * scale;
  return origin + t;
}

__device__ __forceinline__ double track_alpha(double c, double fc) {
#pragma clang fp contract(off)
  double q = c * fc;
  q = 1.0 / q;
  q = 1.0 + q;
  return 1.0 / q;
}

__global__ __launch_bounds__(64) void track_step_kernel(const float* __restrict__ mu, const int32_t* boxes, const int32_t* __restrict__ hw,
                                                        double* __restrict__ state, int K, int S, int F, int n_images, int next_image,
                                                        int init, double beta, double min_cutoff, double beta_e, double d_cutoff,
                                                        double c, double te, int filter_off, float* __restrict__ points,
                                                        float* __restrict__ points_smooth, int32_t* boxes_next,
                                                        float* __restrict__ geom_next, int32_t* __restrict__ flags) {
#pragma clang fp contract(off)   // the stated order, every operation rounded separately: bit-identical to the f64 host restatement
  const int f = blockIdx.x * 64 + threadIdx.x;
  if (f >= F) return;
  const int img = boxes[5 * f];
  const double y0 = (double)boxes[5 * f + 1], x0 = (double)boxes[5 * f + 2], y1 = (double)boxes[5 * f + 3], x1 = (double)boxes[5 * f + 4];
  const float* m = mu + (int64_t)f * K * 2;
  double* st = state + (int64_t)f * (5 + 6 * K);
  double* z0 = st + 5;
  double* xhat = st + 5 + 2 * K;
  double* dxhat = st + 5 + 4 * K;
  float* pt = points + (int64_t)f * K * 2;
  float* ps = points_smooth + (int64_t)f * K * 2;
  const double dS = (double)S, dK = (double)K;
  // 1. the geometry of this frame's box
  const double H = y1 - y0, W = x1 - x0;
  // (float)H / (float)S, formed as the f64 quotient of the two floats rounded to f32: the same value (53 >= 2 * 24 + 2 bits)
  const double fS = (double)(float)S;
  const double sy = (double)(float)((double)(float)H / fS), sx = (double)(float)((double)(float)W / fS);
  // 2. start of a clip
  if (init) {
    const double ccy = (y0 + y1) * 0.5, ccx = (x0 + x1) * 0.5;
    st[0] = H; st[1] = W; st[2] = ccy; st[3] = ccx; st[4] = 1.0;
    for (int k = 0; k < K; ++k) {
      const double py = track_source_pixel(m[2 * k], y0, dS, sy), px = track_source_pixel(m[2 * k + 1], x0, dS, sx);
      z0[2 * k] = py - ccy; z0[2 * k + 1] = px - ccx;
      xhat[2 * k] = py; xhat[2 * k + 1] = px;
      dxhat[2 * k] = 0.0; dxhat[2 * k + 1] = 0.0;
    }
  }
  // 3. the similarity fit of z0 onto p; the points go out on the way
  bool finite = true;
  double mz0 = 0.0, mz1 = 0.0, mp0 = 0.0, mp1 = 0.0;
  for (int k = 0; k < K; ++k) {
    const float my_ = m[2 * k], mx_ = m[2 * k + 1];
    finite = finite && isfinite(my_) && isfinite(mx_);
    const double py = track_source_pixel(my_, y0, dS, sy), px = track_source_pixel(mx_, x0, dS, sx);
    pt[2 * k] = (float)py; pt[2 * k + 1] = (float)px;
    mz0 = mz0 + z0[2 * k]; mz1 = mz1 + z0[2 * k + 1];
    mp0 = mp0 + py; mp1 = mp1 + px;
  }
  mz0 = mz0 / dK; mz1 = mz1 / dK; mp0 = mp0 / dK; mp1 = mp1 / dK;
  double den = 0.0, ar = 0.0, ai = 0.0;
  for (int k = 0; k < K; ++k) {
    const double py = track_source_pixel(m[2 * k], y0, dS, sy), px = track_source_pixel(m[2 * k + 1], x0, dS, sx);
    const double u0 = z0[2 * k] - mz0, u1 = z0[2 * k + 1] - mz1;
    const double v0 = py - mp0, v1 = px - mp1;
    den = den + (u0 * u0 + u1 * u1);
    ar = ar + (u0 * v0 + u1 * v1);
    ai = ai + (u0 * v1 - u1 * v0);
  }
  const double a_r = ar / den, a_i = ai / den;
  const double my = mp0 - (a_r * mz0 - a_i * mz1);
  const double mx = mp1 - (a_r * mz1 + a_i * mz0);
  const double ms = sqrt(a_r * a_r + a_i * a_i);
  const bool lost = !finite || den == 0.0 || !(isfinite(my) && isfinite(mx) && isfinite(ms) && ms > 0.0);
  // 4. the box filter
  double cy = st[2], cx = st[3], s = st[4];
  if (!lost) {
    cy = cy + beta * (my - cy);
    cx = cx + beta * (mx - cx);
    s = s + beta * (ms - s);
    st[2] = cy; st[3] = cx; st[4] = s;
  }
  // 5. the next box: finite whatever the state holds (fmax / fmin drop a NaN), so the conversions never overflow
  const double hn = fmin(fmax(rint(s * st[0]), 2.0), 4194304.0);
  const double wn = fmin(fmax(rint(s * st[1]), 2.0), 4194304.0);
  const double ny0 = fmin(fmax(rint(cy - hn * 0.5), -8388608.0), 8388608.0);
  const double nx0 = fmin(fmax(rint(cx - wn * 0.5), -8388608.0), 8388608.0);
  const double ny1 = ny0 + hn, nx1 = nx0 + wn;
  int fl = lost ? 1 : 0;
  bool inside = false;
  if (img >= 0 && img < n_images) {
    const double sh = (double)hw[2 * img], sw = (double)hw[2 * img + 1];
    inside = ny0 < sh && ny1 > 0.0 && nx0 < sw && nx1 > 0.0;
  }
  if (!inside) fl |= 2;
  // 6. the One-Euro filter
  if (filter_off) {
    for (int k = 0; k < 2 * K; ++k) ps[k] = pt[k];            // this thread's own stores of pass 3
  } else {
    if (!lost) {
      const double rd = track_alpha(c, d_cutoff);
      const double th = te * H;
      for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int a = 0; a < 2; ++a) {
          const double p = a == 0 ? track_source_pixel(m[2 * k], y0, dS, sy) : track_source_pixel(m[2 * k + 1], x0, dS, sx);
          if (!isfinite(p)) continue;
          double xh = xhat[2 * k + a], dh = dxhat[2 * k + a];
          const double dx = (p - xh) / th;
          dh = dh + rd * (dx - dh);
          const double fc = min_cutoff + beta_e * fabs(dh);
          xh = xh + track_alpha(c, fc) * (p - xh);
          xhat[2 * k + a] = xh; dxhat[2 * k + a] = dh;
        }
      }
    }
    for (int k = 0; k < 2 * K; ++k) ps[k] = (float)xhat[k];
  }
  boxes_next[5 * f] = next_image;
  boxes_next[5 * f + 1] = (int32_t)ny0; boxes_next[5 * f + 2] = (int32_t)nx0;
  boxes_next[5 * f + 3] = (int32_t)ny1; boxes_next[5 * f + 4] = (int32_t)nx1;
  geom_next[4 * f] = (float)ny0; geom_next[4 * f + 1] = (float)nx0;
  geom_next[4 * f + 2] = (float)(hn / fS); geom_next[4 * f + 3] = (float)(wn / fS);               // hn, wn <= 2^22 are floats already
  flags[f] = fl;
}

extern "C" int imm_track_step(const float* mu, const int32_t* boxes, const int32_t* hw, double* state, int K, int S, int F, int n_images,
                              int next_image, int init, double box_smooth, double min_cutoff, double beta_e, double d_cutoff, double c,
                              double te, int filter_off, float* points, float* points_smooth, int32_t* boxes_next, float* geom_next,
                              int32_t* flags, void* stream) {
  IMM_REQUIRE(mu && boxes && hw && state && points && points_smooth && boxes_next && geom_next && flags, "track_step: null pointer");
  IMM_REQUIRE(F > 0 && F <= 65535 && K >= 1 && K <= 64, "track_step: 0 < F <= 65535 faces, 1 <= K <= 64 (got %d, %d)", F, K);
  IMM_REQUIRE(S > 0 && S <= 8192, "track_step: 0 < S <= 8192 (got %d)", S);
  IMM_REQUIRE(n_images > 0 && next_image >= 0, "track_step: n_images > 0, next_image >= 0 (got %d, %d)", n_images, next_image);
  IMM_REQUIRE(init == 0 || init == 1, "track_step: init must be 0 or 1 (got %d)", init);
  IMM_REQUIRE(box_smooth > 0.0 && box_smooth <= 1.0, "track_step: box_smooth must lie in (0, 1] (got %g)", box_smooth);
  IMM_REQUIRE(min_cutoff > 0.0 && min_cutoff <= 1.0e300 && d_cutoff > 0.0 && d_cutoff <= 1.0e300 && c > 0.0 && c <= 1.0e300 && te > 0.0 &&
                  te <= 1.0e300 && beta_e >= 0.0 && beta_e <= 1.0e300,
              "track_step: min_cutoff, d_cutoff, c, te must be finite and positive, beta finite and >= 0 (got %g, %g, %g, %g, %g)", min_cutoff,
              d_cutoff, c, te, beta_e);
  hipLaunchKernelGGL(track_step_kernel, dim3((F + 63) / 64), dim3(64), 0, (hipStream_t)stream, mu, boxes, hw, state, K, S, F, n_images,
                     next_image, init, box_smooth, min_cutoff, beta_e, d_cutoff, c, te, filter_off, points, points_smooth, boxes_next,
                     geom_next, flags);
  IMM_CHECK_LAUNCH("imm_track_step");
  return 0;
}
