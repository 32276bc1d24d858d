// clip.hip — clip morph on gfx950: the two small kernels that let the morph chain run behind the tracker with nothing returning to
// the host (imm_amd/clip.py, imm_amd/inference.py LandmarkDetector.morph_clip).  The rule is stated once, in include/imm_clip.h:
//
//   imm_clip_rows   per face of a frame, from the box row the tracker left on the device: the edge ramp's reciprocals, the hull mask's
//                   reciprocal softness, and the face's landmarks in the frame of that box (NaN for a lost face: the row is dropped)
//   imm_clip_ema    s = s + alpha * (x - s) over the rows of the colour gain and of the membrane's differences, skipped rows left alone
//
// A few microseconds of latency-bound work on at most max_batch rows: nothing here is tuned.  Plain C++, every operation rounded
// separately in the order of the header (the numpy restatement of the tests follows it line by line).
// Addressing: a block reads and writes only row f < F (i < n) of every buffer; the values the buffers hold never reach an address.
#include "common.h"

#define CLIP_MAX_K 80                        // landmarks of a face: the bound of the morph chain (SPLINE_MAX_M)
#define CLIP_MAX_WIDTH 768                   // values of a filtered row: 3 * 256, the membrane's largest ring

__device__ __forceinline__ double clip_inv_ramp(double feather, double side) {
#pragma clang fp contract(off)
  const double r = feather * side;
  return r <= 0.5 ? 2.0 : 1.0 / fmax(r, 0.5);
}

__device__ __forceinline__ double clip_inv_soft(float mask_feather, double H, double W) {
#pragma clang fp contract(off)
  const double soft = (double)mask_feather * fmin(H, W);
  return 1.0 / fmax(1.0, soft);
}

// (float)side / (float)S, formed as the f64 quotient of the two floats rounded to f32: the same value (53 >= 2 * 24 + 2 bits)
__device__ __forceinline__ double clip_scale(double side, double fS) {
#pragma clang fp contract(off)
  return (double)(float)((double)(float)side / fS);
}

// a source pixel back into [-1, 1] of the box: the inverse of track_source_pixel
__device__ __forceinline__ float clip_landmark(float point, double origin, double scale, double dS) {
#pragma clang fp contract(off)
  double v = (double)point - origin;
  v = v / scale;
  v = v / dS;
  v = v * 2.0;
  v = v - 1.0;
  if (__builtin_isfinite(v)) v = fmin(fmax(v, -1.0), 1.0);
  return (float)v;
}

__global__ __launch_bounds__(64) void clip_rows_kernel(const int32_t* __restrict__ boxes, const int32_t* __restrict__ track_flags,
                                                       const float* __restrict__ mu, const float* __restrict__ points, int K, int S,
                                                       double feather, const float* __restrict__ mask_feather, float* __restrict__ own,
                                                       float* __restrict__ inv_ramp, float* __restrict__ inv_soft) {
#pragma clang fp contract(off)
  const int f = blockIdx.x;
  const double y0 = (double)boxes[5 * f + 1], x0 = (double)boxes[5 * f + 2], y1 = (double)boxes[5 * f + 3], x1 = (double)boxes[5 * f + 4];
  const double H = y1 - y0, W = x1 - x0;
  if (threadIdx.x == 0) {
    inv_ramp[2 * f] = (float)clip_inv_ramp(feather, H);
    inv_ramp[2 * f + 1] = (float)clip_inv_ramp(feather, W);
    if (mask_feather) inv_soft[f] = (float)clip_inv_soft(mask_feather[f], H, W);
  }
  const bool lost = (track_flags[f] & 1) != 0;
  const double dS = (double)S, fS = (double)(float)S;
  const double sy = clip_scale(H, fS), sx = clip_scale(W, fS);
  const int64_t base = (int64_t)f * K * 2;
  for (int i = threadIdx.x; i < 2 * K; i += 64) {
    float v;
    if (lost) v = __builtin_nanf("");
    else if (!points) v = mu[base + i];
    else v = (i & 1) ? clip_landmark(points[base + i], x0, sx, dS) : clip_landmark(points[base + i], y0, sy, dS);
    own[base + i] = v;
  }
}

__device__ __forceinline__ float clip_ema_one(float s, float x, float alpha) {
#pragma clang fp contract(off)
  const float d = x - s;
  const float m = alpha * d;
  return s + m;
}

__global__ __launch_bounds__(256) void clip_ema_kernel(float* x, float* state, int32_t* seen, const int32_t* __restrict__ skip,
                                                       const int32_t* __restrict__ lost, int width, float alpha) {
  const int i = blockIdx.x;
  // uniform over the block (the row's flags decide): no barrier is skipped by part of it
  if (skip[i] != 0 || (lost && (lost[i] & 1) != 0)) return;
  const int first = seen[i] == 0;
  __syncthreads();                                                     // every thread has read seen[i] before thread 0 writes it
  float* xr = x + (int64_t)i * width;
  float* sr = state + (int64_t)i * width;
  for (int j = threadIdx.x; j < width; j += 256) {
    const float v = xr[j];
    const float s = first ? v : clip_ema_one(sr[j], v, alpha);
    sr[j] = s;
    xr[j] = s;
  }
  if (threadIdx.x == 0) seen[i] = 1;
}

extern "C" int imm_clip_rows(const int32_t* boxes, const int32_t* track_flags, const float* mu, const float* points, int K, int S, int F,
                             double feather, const float* mask_feather, float* own, float* inv_ramp, float* inv_soft, void* stream) {
  IMM_REQUIRE(boxes && track_flags && mu && own && inv_ramp, "clip_rows: null pointer");
  IMM_REQUIRE((mask_feather == nullptr) == (inv_soft == nullptr), "clip_rows: inv_soft is given exactly when mask_feather is");
  IMM_REQUIRE(F >= 1 && F <= 65535 && K >= 1 && K <= CLIP_MAX_K, "clip_rows: 1 <= F <= 65535 faces, 1 <= K <= %d (got %d, %d)", CLIP_MAX_K,
              F, K);
  IMM_REQUIRE(S > 0 && S <= 8192, "clip_rows: 0 < S <= 8192 (got %d)", S);
  IMM_REQUIRE(feather >= 0.0 && feather <= 0.5, "clip_rows: feather must lie in [0, 0.5] (got %g)", feather);
  hipLaunchKernelGGL(clip_rows_kernel, dim3(F), dim3(64), 0, (hipStream_t)stream, boxes, track_flags, mu, points, K, S, feather,
                     mask_feather, own, inv_ramp, inv_soft);
  IMM_CHECK_LAUNCH("imm_clip_rows");
  return 0;
}

extern "C" int imm_clip_ema(float* x, float* state, int32_t* seen, const int32_t* skip, const int32_t* lost, int n, int width, float alpha,
                            void* stream) {
  IMM_REQUIRE(x && state && seen && skip, "clip_ema: null pointer");
  IMM_REQUIRE(n >= 1 && n <= 65535 && width >= 1 && width <= CLIP_MAX_WIDTH, "clip_ema: 1 <= n <= 65535 rows of 1 <= width <= %d (got %d, %d)",
              CLIP_MAX_WIDTH, n, width);
  IMM_REQUIRE(alpha > 0.f && alpha <= 1.f, "clip_ema: alpha must lie in (0, 1] (got %g)", (double)alpha);
  const size_t bytes = (size_t)n * width * sizeof(float);
  const uintptr_t a = (uintptr_t)x, b = (uintptr_t)state;
  IMM_REQUIRE(a + bytes <= b || b + bytes <= a, "clip_ema: x and state overlap");
  hipLaunchKernelGGL(clip_ema_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, x, state, seen, skip, lost, width, alpha);
  IMM_CHECK_LAUNCH("imm_clip_ema");
  return 0;
}
