// retarget.hip — re-enactment on gfx950: the tracked points of ONE driving face become, per frame, the pose of n still source faces,
// on the device (imm_amd/reenact.py, imm_amd/generation.py ImageGenerator.reenact).  The rule is stated once, in
// include/imm_retarget.h; in short, per source face:
//
//   1. fit a             the similarity of the driver's first-frame shape q0 onto the face's own landmarks m
//   2. rigid == 0        the similarity b of q0 onto this frame's points q, divided out: q~ = mq0 + (q - mq) / b
//   3. target            relative: m + a (x) (q~ - q0);  absolute: mm + a (x) (q~ - mq0)
//   4. output            m + gain * (target - m), clamped to [-1, 1]
//   5. held              the previous pose, bit for bit, when the driver is lost or anything above is not usable
//
// One thread per face, 64 per block, f64, every operation rounded separately, in the order of the header (the numpy restatement of
// the tests follows it line by line), rounded once to f32.  A few microseconds of latency-bound work on at most 64 points per
// face: nothing here is tuned.  The target of a point is recomputed by retarget_value() in the test pass and in the store pass
// instead of being held in 128 registers; the same operations on the same operands give the same bits.
// Addressing: a thread reads and writes only row i < n of every [n, ..] buffer and the K rows of q and anchor; the values the
// device buffers hold never reach an address.  With init == 1 no thread reads the anchor (q0 is (double)q), and thread 0 of block 0
// writes it.
#include "common.h"

struct RetargetFit {
  double a_r, a_i, mz0, mz1, mp0, mp1, den;
};

// q0[k][a]: the anchor, or with init the points of this frame
__device__ __forceinline__ double retarget_q0(const float* q, const double* anchor, int init, int i) {
  return init ? (double)q[i] : anchor[i];
}

// step 3 of imm_track.h with z = q0 and p f32 [K, 2]
__device__ __forceinline__ RetargetFit retarget_fit(const float* q, const double* anchor, int init, const float* p, int K) {
#pragma clang fp contract(off)
  RetargetFit f;
  const double dK = (double)K;
  double mz0 = 0.0, mz1 = 0.0, mp0 = 0.0, mp1 = 0.0;
  for (int k = 0; k < K; ++k) {
    mz0 = mz0 + retarget_q0(q, anchor, init, 2 * k); mz1 = mz1 + retarget_q0(q, anchor, init, 2 * k + 1);
    mp0 = mp0 + (double)p[2 * k]; mp1 = mp1 + (double)p[2 * k + 1];
  }
  mz0 = mz0 / dK; mz1 = mz1 / dK; mp0 = mp0 / dK; mp1 = mp1 / dK;
  double den = 0.0, ar = 0.0, ai = 0.0;
  for (int k = 0; k < K; ++k) {
    const double u0 = retarget_q0(q, anchor, init, 2 * k) - mz0, u1 = retarget_q0(q, anchor, init, 2 * k + 1) - mz1;
    const double v0 = (double)p[2 * k] - mp0, v1 = (double)p[2 * k + 1] - mp1;
    den = den + (u0 * u0 + u1 * u1);
    ar = ar + (u0 * v0 + u1 * v1);
    ai = ai + (u0 * v1 - u1 * v0);
  }
  f.a_r = ar / den; f.a_i = ai / den;
  f.mz0 = mz0; f.mz1 = mz1; f.mp0 = mp0; f.mp1 = mp1; f.den = den;
  return f;
}

// steps 2 to 4 for point k in front of the clamp: o[k] = m[k] + gain * (t[k] - m[k])
__device__ __forceinline__ void retarget_value(const float* q, const double* anchor, int init, const float* m, int k, const RetargetFit& fa,
                                               const RetargetFit& fb, double nb, int relative, int rigid, double gain, double* o0,
                                               double* o1) {
#pragma clang fp contract(off)
  double s0 = (double)q[2 * k], s1 = (double)q[2 * k + 1];                                 // q~[k]
  if (!rigid) {
    const double w0 = s0 - fb.mp0, w1 = s1 - fb.mp1;
    s0 = fa.mz0 + (fb.a_r * w0 + fb.a_i * w1) / nb;
    s1 = fa.mz1 + (fb.a_r * w1 - fb.a_i * w0) / nb;
  }
  const double m0 = (double)m[2 * k], m1 = (double)m[2 * k + 1];
  double d0, d1, t0, t1;
  if (relative) {
    d0 = s0 - retarget_q0(q, anchor, init, 2 * k); d1 = s1 - retarget_q0(q, anchor, init, 2 * k + 1);
    t0 = m0 + (fa.a_r * d0 - fa.a_i * d1);
    t1 = m1 + (fa.a_r * d1 + fa.a_i * d0);
  } else {
    d0 = s0 - fa.mz0; d1 = s1 - fa.mz1;
    t0 = fa.mp0 + (fa.a_r * d0 - fa.a_i * d1);
    t1 = fa.mp1 + (fa.a_r * d1 + fa.a_i * d0);
  }
  *o0 = m0 + gain * (t0 - m0);
  *o1 = m1 + gain * (t1 - m1);
}

__global__ __launch_bounds__(64) void retarget_kernel(const float* __restrict__ q, double* anchor, const int32_t* __restrict__ driver_flags,
                                                      const float* m_all, const float* prev, int K, int n, int init, int relative,
                                                      int rigid, double gain, float* out, int32_t* __restrict__ flags) {
#pragma clang fp contract(off)   // the stated order, every operation rounded separately: bit-identical to the f64 host restatement
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const float* m = m_all + (int64_t)i * K * 2;
  const float* pv = prev + (int64_t)i * K * 2;
  float* o = out + (int64_t)i * K * 2;
  bool held = (driver_flags[0] & 1) != 0;
  bool finite = true;
  for (int k = 0; k < 2 * K; ++k)
    finite = finite && isfinite(q[k]) && isfinite(retarget_q0(q, anchor, init, k)) && isfinite(m[k]);
  held = held || !finite;
  // 1. the driver's first-frame shape onto the face's landmarks
  const RetargetFit fa = retarget_fit(q, anchor, init, m, K);
  const double na = fa.a_r * fa.a_r + fa.a_i * fa.a_i;
  held = held || fa.den == 0.0 || na == 0.0;
  // 2. the driver's first-frame shape onto its shape of this frame
  RetargetFit fb = fa;
  double nb = 1.0;
  if (!rigid) {
    fb = retarget_fit(q, anchor, init, q, K);
    nb = fb.a_r * fb.a_r + fb.a_i * fb.a_i;
    held = held || fb.den == 0.0 || nb == 0.0;
  }
  // 3, 4. every value in front of the clamp must be finite
  for (int k = 0; k < K; ++k) {
    double o0, o1;
    retarget_value(q, anchor, init, m, k, fa, fb, nb, relative, rigid, gain, &o0, &o1);
    held = held || !isfinite(o0) || !isfinite(o1);
  }
  // 5. the stores: the row of prev is read element by element in front of the store to the same index (out may be prev)
  if (held) {
    for (int k = 0; k < 2 * K; ++k) {
      const float v = pv[k];
      o[k] = v;
    }
  } else {
    for (int k = 0; k < K; ++k) {
      double o0, o1;
      retarget_value(q, anchor, init, m, k, fa, fb, nb, relative, rigid, gain, &o0, &o1);
      o[2 * k] = (float)fmin(fmax(o0, -1.0), 1.0);
      o[2 * k + 1] = (float)fmin(fmax(o1, -1.0), 1.0);
    }
  }
  flags[i] = held ? 1 : 0;
  if (init && i == 0)
    for (int k = 0; k < 2 * K; ++k) anchor[k] = (double)q[k];
}

extern "C" int imm_retarget(const float* q, double* anchor, const int32_t* driver_flags, const float* m, const float* prev, int K, int n,
                            int init, int relative, int rigid, double gain, float* out, int32_t* flags, void* stream) {
  IMM_REQUIRE(q && anchor && driver_flags && m && prev && out && flags, "retarget: null pointer");
  IMM_REQUIRE(n > 0 && n <= 65535 && K >= 1 && K <= 64, "retarget: 0 < n <= 65535 faces, 1 <= K <= 64 (got %d, %d)", n, K);
  IMM_REQUIRE(init == 0 || init == 1, "retarget: init must be 0 or 1 (got %d)", init);
  IMM_REQUIRE((relative == 0 || relative == 1) && (rigid == 0 || rigid == 1), "retarget: relative and rigid must be 0 or 1 (got %d, %d)",
              relative, rigid);
  IMM_REQUIRE(gain >= 0.0 && gain <= 4.0, "retarget: gain must be finite and lie in [0, 4] (got %g)", gain);
  hipLaunchKernelGGL(retarget_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, q, anchor, driver_flags, m, prev, K, n, init,
                     relative, rigid, gain, out, flags);
  IMM_CHECK_LAUNCH("imm_retarget");
  return 0;
}
