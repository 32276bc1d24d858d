// hull.hip — the landmark-hull mask of a morph on gfx950 (imm_amd/inference.py LandmarkDetector.morph(mask='hull'),
// imm_amd/morphing.py).  The rule is stated once, in include/imm_hull.h; in short:
//
//   imm_hull_fit   per row: the K target landmarks in box-relative pixels, grown about their centroid; per slot i the supporting line
//                  through point i towards the farthest point j that has every point on its inner side, as (ny, nx, d) f32 [n, K, 3];
//                  f64 with every operation rounded separately, only + - * / sqrt and comparisons, bit-identical to the numpy
//                  restatement (as imm_track_step, imm_retarget and imm_colour_gain are)
//
// (imm_morph_hull_u8, which turns the lines into a weight per pixel, is morph.hip's kernel in its HULL instantiations.)
// One workgroup of 256 threads per row, five phases with a barrier between them; what a thread does in a phase is a __host__
// __device__ function of (row, thread) on the row's HullState, which is the block's LDS on the device, so that the same text compiles
// for the host, where a stand-alone program runs it thread by thread under the address and undefined-behaviour sanitizers.
//   1 points   thread i < K: pose i -> (vy_i, vx_i) before the grow; is the pose finite
//   2 grow     thread i < K: the centroid (summed in index order by every thread for itself: K broadcast reads), the grown point
//   3 pairs    the K * K (i, j) pairs spread over the threads: is j a candidate of slot i (the predicate over every k, points read
//              from LDS), and does any point lie strictly inside that line: two bytes per pair
//   4 slots    thread i < K: the largest candidate of slot i in a scan over j (strictly larger only: ties stay with the lowest j), its line
//   5 output   thread i < K: the row's flags from the K slots (every thread for itself), its slot's three floats; thread 0: flags[b]
// K * K * K predicate evaluations a row, at most 512 k at K = 80: not a hot path, and kept plain.  Addressing: every index is formed
// from b < n, i < K and j < K alone; what poses, boxes and grow hold never reaches an address.
#include "paste_common.h"

#define HULL_THREADS 256

struct HullState {
  double py[SPLINE_MAX_M], px[SPLINE_MAX_M];        // the points before the grow
  double vy[SPLINE_MAX_M], vx[SPLINE_MAX_M];        // and grown
  float line[SPLINE_MAX_M][3];                      // the slots' lines
  uint8_t cand[SPLINE_MAX_M * SPLINE_MAX_M];        // [i][j]: j is a candidate of slot i
  uint8_t inner[SPLINE_MAX_M * SPLINE_MAX_M];       // [i][j]: some point lies strictly inside the line i -> j
  uint8_t bad[SPLINE_MAX_M];                        // pose i is not finite
  uint8_t won[SPLINE_MAX_M];                        // slot i: 0 no winner, 1 a winner, 3 a winner with a point strictly inside
};

__host__ __device__ __forceinline__ void hull_points(HullState& st, const float* __restrict__ poses, const int32_t* __restrict__ boxes,
                                                     int K, int b, int t) {
#pragma clang fp contract(off)   // every operation rounded separately, as the host restatement's
  if (t >= K) return;
  const double H = (double)((int64_t)boxes[5 * b + 3] - boxes[5 * b + 1]), W = (double)((int64_t)boxes[5 * b + 4] - boxes[5 * b + 2]);
  const double y = (double)poses[((int64_t)b * K + t) * 2], x = (double)poses[((int64_t)b * K + t) * 2 + 1];
  const double hh = 0.5 * H, hw = 0.5 * W;
  st.py[t] = (y + 1.0) * hh;
  st.px[t] = (x + 1.0) * hw;
  st.bad[t] = !(__builtin_isfinite(y) && __builtin_isfinite(x));     // (the builtin: one spelling for the device and a host build)
}

__host__ __device__ __forceinline__ void hull_grow(HullState& st, const float* __restrict__ grow, int K, int b, int t) {
#pragma clang fp contract(off)
  if (t >= K) return;
  double sy = st.py[0], sx = st.px[0];
  for (int i = 1; i < K; ++i) {
    sy = sy + st.py[i];
    sx = sx + st.px[i];
  }
  const double cy = sy / (double)K, cx = sx / (double)K;
  const double g = (double)grow[b];
  const double ty = g * (st.py[t] - cy), tx = g * (st.px[t] - cx);
  st.vy[t] = cy + ty;
  st.vx[t] = cx + tx;
}

__host__ __device__ __forceinline__ void hull_pairs(HullState& st, int K, int t) {
#pragma clang fp contract(off)
  for (int p = t; p < K * K; p += HULL_THREADS) {
    const int i = p / K, j = p - i * K;
    const double iy = st.vy[i], ix = st.vx[i];
    const double ey = st.vy[j] - iy, ex = st.vx[j] - ix;
    bool ok = !(ey == 0.0 && ex == 0.0), strict = false;
    for (int k = 0; k < K && ok; ++k) {
      const double a = ey * (st.vx[k] - ix), c = ex * (st.vy[k] - iy);
      const double s = a - c;
      ok = s >= 0.0;
      strict = strict || s > 0.0;
    }
    st.cand[i * SPLINE_MAX_M + j] = ok;
    st.inner[i * SPLINE_MAX_M + j] = ok && strict;
  }
}

__host__ __device__ __forceinline__ void hull_slots(HullState& st, int K, int t) {
#pragma clang fp contract(off)
  if (t >= K) return;
  const double iy = st.vy[t], ix = st.vx[t];
  int win = -1;
  double best = 0.0, wy = 0.0, wx = 0.0;
  for (int j = 0; j < K; ++j) {
    if (!st.cand[t * SPLINE_MAX_M + j]) continue;
    const double ey = st.vy[j] - iy, ex = st.vx[j] - ix;
    const double l2 = ey * ey + ex * ex;
    if (win < 0 || l2 > best) {
      win = j; best = l2; wy = ey; wx = ex;
    }
  }
  if (win < 0) {
    st.line[t][0] = 0.f; st.line[t][1] = 0.f; st.line[t][2] = __builtin_huge_valf();
    st.won[t] = 0;
    return;
  }
  const double len = sqrt(best);
  const double ny = -wx / len, nx = wy / len;
  const double d = -(ny * iy + nx * ix);
  st.line[t][0] = (float)ny; st.line[t][1] = (float)nx; st.line[t][2] = (float)d;
  st.won[t] = st.inner[t * SPLINE_MAX_M + win] ? 3 : 1;
}

__host__ __device__ __forceinline__ void hull_output(const HullState& st, const int32_t* __restrict__ boxes,
                                                     const float* __restrict__ grow, int K, int b, int t, float* __restrict__ edges,
                                                     int32_t* __restrict__ flags) {
  if (t >= K) return;
  const int64_t H = (int64_t)boxes[5 * b + 3] - boxes[5 * b + 1], W = (int64_t)boxes[5 * b + 4] - boxes[5 * b + 2];
  bool bad = H <= 0 || W <= 0 || !__builtin_isfinite(grow[b]);
  int winners = 0, inside = 0;
  for (int i = 0; i < K; ++i) {
    bad = bad || st.bad[i];
    winners += st.won[i] & 1;
    inside |= st.won[i] & 2;
  }
  const int f = (bad ? 1 : 0) | ((winners < 3 || !inside) ? 2 : 0);
  float* e = edges + ((int64_t)b * K + t) * 3;
  if (f) {
    e[0] = 0.f; e[1] = 0.f; e[2] = -__builtin_huge_valf();
  } else {
    e[0] = st.line[t][0]; e[1] = st.line[t][1]; e[2] = st.line[t][2];
  }
  if (t == 0) flags[b] = f;
}

__global__ __launch_bounds__(HULL_THREADS) void hull_fit_kernel(const float* __restrict__ poses, const int32_t* __restrict__ boxes,
                                                                const float* __restrict__ grow, int K, float* __restrict__ edges,
                                                                int32_t* __restrict__ flags) {
  __shared__ HullState st;                                         // 16.5 KB
  const int b = blockIdx.x, t = threadIdx.x;
  hull_points(st, poses, boxes, K, b, t);
  __syncthreads();
  hull_grow(st, grow, K, b, t);
  __syncthreads();
  hull_pairs(st, K, t);
  __syncthreads();
  hull_slots(st, K, t);
  __syncthreads();
  hull_output(st, boxes, grow, K, b, t, edges, flags);
}

extern "C" int imm_hull_fit(const float* poses, const int32_t* boxes, const float* grow, int K, int n, float* edges, int32_t* flags,
                            void* stream) {
  IMM_REQUIRE(poses && boxes && grow && edges && flags, "hull_fit: null pointer");
  IMM_REQUIRE(n > 0 && n <= 65535, "hull_fit: 0 < n <= 65535 rows (got %d)", n);
  IMM_REQUIRE(K >= 1 && K <= SPLINE_MAX_M, "hull_fit: 1 <= K <= %d landmarks (got %d)", SPLINE_MAX_M, K);
  hipLaunchKernelGGL(hull_fit_kernel, dim3(n), dim3(HULL_THREADS), 0, (hipStream_t)stream, poses, boxes, grow, K, edges, flags);
  IMM_CHECK_LAUNCH("imm_hull_fit");
  return 0;
}
