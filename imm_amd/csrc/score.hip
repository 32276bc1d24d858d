// score.hip — landmark quality on gfx950: after a pose program, the soft-argmax marginals and the landmarks of every face become two
// scores and, for the tracker, the gated landmarks (imm_amd/quality.py, imm_amd/inference.py LandmarkDetector.quality,
// imm_amd/tracking.py FaceTracker with a gate).  The rule is stated once, in include/imm_score.h; in short, per face:
//
//   1. spread      per landmark sqrt of the marginals' second moments about mu; their mean over k
//   2. points      the landmarks themselves, or in source pixels as imm_track.h step 1 forms them
//   3. residual    sqrt(1 - |sum u conj v|^2 / (sum |u|^2 sum |v|^2)) of the reference shape against the points
//   4. flags       a score above its threshold, or NaN, sets its bit
//   5. mu_out      mu's bits, or the quiet NaN for every landmark of a flagged face when blank is set
//
// One 64-lane workgroup per face.  Lane k < K walks its landmark's marginals (the loads of one row i are K consecutive floats) and
// leaves spread[k], p[k] and ref[k] in LDS; after a barrier lane 0 forms the sums over k in ascending order, the scores and the flags;
// after a second barrier all lanes write mu_out.  f64, every operation rounded separately, in the order of the header (the numpy
// restatement of the tests follows it line by line), rounded once to the stored type.  At most 64 x 128 multiply-adds per face:
// latency-bound, nothing here is tuned.
// Addressing: a workgroup reads and writes only row f = blockIdx.x < F of every [F, ..] buffer and 2 K doubles at ref + f * ref_stride;
// the values the device buffers hold never reach an address.
#include "common.h"

__device__ __forceinline__ double score_source_pixel(float mu, double origin, double dS, double scale) {
#pragma clang fp contract(off)
  double t = (double)mu + 1.0;
  t = t * 0.5;
  t = t * dS;
  t = t * scale;
  return origin + t;
}

// sum_i (double)q[i * K] * (d * d), d = (-1.0 + (2.0 * i) / (n - 1)) - m
__device__ __forceinline__ double score_moment(const float* __restrict__ q, int n, int K, double m) {
#pragma clang fp contract(off)
  const double dn = (double)(n - 1);
  double v = 0.0;
  for (int i = 0; i < n; ++i) {
    double lin = 2.0 * (double)i;
    lin = lin / dn;
    lin = -1.0 + lin;
    const double d = lin - m;
    const double dd = d * d;
    v = v + (double)q[(int64_t)i * K] * dd;
  }
  return v;
}

__global__ __launch_bounds__(64) void landmark_scores_kernel(const float* __restrict__ py, const float* __restrict__ px,
                                                             const float* __restrict__ mu, const int32_t* __restrict__ boxes,
                                                             const double* __restrict__ ref, int64_t ref_stride, int K, int h, int w, int S,
                                                             double max_spread, double max_residual, int blank, float* __restrict__ spread,
                                                             float* __restrict__ score, int32_t* __restrict__ qflags,
                                                             float* __restrict__ mu_out) {
#pragma clang fp contract(off)   // the stated order, every operation rounded separately: bit-identical to the f64 host restatement
  __shared__ double s_spread[64];
  __shared__ double s_p[128];
  __shared__ double s_z[128];
  __shared__ int s_flags;
  const int f = blockIdx.x, k = threadIdx.x;
  const float* m = mu + (int64_t)f * K * 2;
  if (k < K) {
    const float my_ = m[2 * k], mx_ = m[2 * k + 1];
    // 1. the spread of landmark k
    const double vy = score_moment(py + (int64_t)f * h * K + k, h, K, (double)my_);
    const double vx = score_moment(px + (int64_t)f * w * K + k, w, K, (double)mx_);
    const double sp = sqrt(vy + vx);
    s_spread[k] = sp;
    spread[(int64_t)f * K + k] = (float)sp;
    // 2. its point
    if (boxes) {
      const double y0 = (double)boxes[5 * f + 1], x0 = (double)boxes[5 * f + 2], y1 = (double)boxes[5 * f + 3], x1 = (double)boxes[5 * f + 4];
      const double dS = (double)S, fS = (double)(float)S;
      const double H = y1 - y0, W = x1 - x0;
      // (float)H / (float)S, formed as the f64 quotient of the two floats rounded to f32: the same value (53 >= 2 * 24 + 2 bits)
      const double sy = (double)(float)((double)(float)H / fS), sx = (double)(float)((double)(float)W / fS);
      s_p[2 * k] = score_source_pixel(my_, y0, dS, sy);
      s_p[2 * k + 1] = score_source_pixel(mx_, x0, dS, sx);
    } else {
      s_p[2 * k] = (double)my_;
      s_p[2 * k + 1] = (double)mx_;
    }
    if (ref) {
      const double* z = ref + (int64_t)f * ref_stride;
      s_z[2 * k] = z[2 * k];
      s_z[2 * k + 1] = z[2 * k + 1];
    }
  }
  __syncthreads();
  if (k == 0) {
    const double dK = (double)K;
    double sbar = 0.0;
    for (int j = 0; j < K; ++j) sbar = sbar + s_spread[j];
    sbar = sbar / dK;
    // 3. the shape residual
    double residual = 0.0;
    if (ref) {
      double mz0 = 0.0, mz1 = 0.0, mp0 = 0.0, mp1 = 0.0;
      for (int j = 0; j < K; ++j) {
        mz0 = mz0 + s_z[2 * j]; mz1 = mz1 + s_z[2 * j + 1];
        mp0 = mp0 + s_p[2 * j]; mp1 = mp1 + s_p[2 * j + 1];
      }
      mz0 = mz0 / dK; mz1 = mz1 / dK; mp0 = mp0 / dK; mp1 = mp1 / dK;
      double den = 0.0, ar = 0.0, ai = 0.0, pv = 0.0;
      for (int j = 0; j < K; ++j) {
        const double u0 = s_z[2 * j] - mz0, u1 = s_z[2 * j + 1] - mz1;
        const double v0 = s_p[2 * j] - mp0, v1 = s_p[2 * j + 1] - mp1;
        den = den + (u0 * u0 + u1 * u1);
        ar = ar + (u0 * v0 + u1 * v1);
        ai = ai + (u0 * v1 - u1 * v0);
        pv = pv + (v0 * v0 + v1 * v1);
      }
      residual = __builtin_nan("");
      if (isfinite(den) && isfinite(pv) && den > 0.0 && pv > 0.0) {
        const double num = ar * ar + ai * ai;
        const double r2 = 1.0 - num / (den * pv);
        if (isfinite(r2)) residual = sqrt(fmax(r2, 0.0));
      }
    }
    // 4. the flags, on the f64 values
    int fl = 0;
    if (!(sbar <= max_spread)) fl |= 1;
    if (!(residual <= max_residual)) fl |= 2;
    score[2 * f] = (float)sbar;
    score[2 * f + 1] = (float)residual;
    qflags[f] = fl;
    s_flags = fl;
  }
  __syncthreads();
  // 5. the gated landmarks, as bits
  if (mu_out) {
    const bool gone = blank && s_flags != 0;
    const uint32_t* mb = reinterpret_cast<const uint32_t*>(m);
    uint32_t* ob = reinterpret_cast<uint32_t*>(mu_out + (int64_t)f * K * 2);
    for (int i = k; i < 2 * K; i += 64) ob[i] = gone ? 0x7fc00000u : mb[i];
  }
}

extern "C" int imm_landmark_scores(const float* py, const float* px, const float* mu, const int32_t* boxes, const double* ref,
                                   int64_t ref_stride, int K, int h, int w, int S, int F, double max_spread, double max_residual, int blank,
                                   float* spread, float* score, int32_t* qflags, float* mu_out, void* stream) {
  IMM_REQUIRE(py && px && mu && spread && score && qflags, "landmark_scores: null pointer");
  IMM_REQUIRE(F > 0 && F <= 65535 && K >= 1 && K <= 64, "landmark_scores: 0 < F <= 65535 faces, 1 <= K <= 64 (got %d, %d)", F, K);
  IMM_REQUIRE(h >= 2 && h <= 64 && w >= 2 && w <= 64, "landmark_scores: 2 <= h, w <= 64 (got %d, %d)", h, w);
  IMM_REQUIRE(S > 0 && S <= 8192, "landmark_scores: 0 < S <= 8192 (got %d)", S);
  IMM_REQUIRE(max_spread == max_spread && max_residual == max_residual,
              "landmark_scores: a threshold must not be NaN (+inf switches it off; got %g, %g)", max_spread, max_residual);
  IMM_REQUIRE(blank == 0 || blank == 1, "landmark_scores: blank must be 0 or 1 (got %d)", blank);
  IMM_REQUIRE(mu_out || blank == 0, "landmark_scores: mu_out may be NULL only with blank == 0");
  IMM_REQUIRE(!ref || ref_stride == 0 || ref_stride >= 2 * (int64_t)K,
              "landmark_scores: ref_stride must be 0 (one shape for all faces) or >= 2 K doubles (got %lld)", (long long)ref_stride);
  hipLaunchKernelGGL(landmark_scores_kernel, dim3(F), dim3(64), 0, (hipStream_t)stream, py, px, mu, boxes, ref, ref_stride, K, h, w, S,
                     max_spread, max_residual, blank, spread, score, qflags, mu_out);
  IMM_CHECK_LAUNCH("imm_landmark_scores");
  return 0;
}
