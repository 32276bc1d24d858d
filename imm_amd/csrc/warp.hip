// warp.hip — faces re-posed from their own pixels on gfx950 (imm_amd/inference.py LandmarkDetector.warp, imm_amd/warping.py): a
// thin-plate spline whose control points are the face's landmarks, fitted per face on the device, moves the photo's pixels inside the
// face's box.  The rule is stated once, in include/imm_warp.h; in short:
//
//   imm_warp_fit   per row, ctrl = (target landmarks p, border anchors); the displacement spline with the values strength * (mu - p) at
//                  the landmarks and 0 at the anchors: an (M + 3) x (M + 3) system assembled and solved in f64 by Gaussian elimination
//                  with partial pivoting in LDS, the coefficients rounded once to f32
//   imm_warp_u8    per photo pixel of a row's box: q -> D(q) = sum_j w_j U(|q - ctrl_j|^2) + a_0 + a_1 q_y + a_2 q_x, the ORIGINAL photo
//                  sampled bilinearly at (r, c) + (H/2, W/2) D, blended over the canvas with imm_compose_u8's edge ramp and rounding
//
// Fit: one workgroup of 256 threads per row.  The augmented matrix [N][N + 2] doubles, N = M + 3 <= 83, is 56,440 bytes of static LDS
// (one workgroup per CU; the fit is a few hundred barriers of latency-bound work on a matrix that never leaves the CU, and rows run
// side by side on the chip's CUs).  The row stride N + 2 = 85 doubles is odd in 8-byte words, so a wave's column walks meet every bank.
// Per elimination step: thread 0 finds the pivot row, the rows are swapped, the multipliers of the column are formed ((N - 1 - k)
// divisions, not one per element), and the trailing block is updated by all threads; the back substitution is column oriented.
// Warp: the paste skeleton of paste_common.h, which states the launch shape, the ownership of a pixel (the first row of the launch whose
// box covers it) and the addressing argument.  The row's ctrl [M][2] and coef [M + 3][2] sit in 1.3 KB of LDS, read by every lane at the
// same address (a broadcast, no bank conflict); the kernel is bound by its M logf per pixel, not by the 6 bytes per pixel it moves.  Rows
// met on a link walk (overlapping boxes) read their ctrl and coef through L2, indexed by a row index in [0, n) and j < M + 3.
#include "paste_common.h"

__global__ __launch_bounds__(256) void warp_fit_kernel(const float* __restrict__ poses, const float* __restrict__ mu,
                                                       const float* __restrict__ anchors, int K, int A, double strength, double lam,
                                                       float* __restrict__ coef, float* __restrict__ ctrl_out, int32_t* __restrict__ flags) {
#pragma clang fp contract(off)   // every operation rounded separately, as the host restatement's
  __shared__ double a[SPLINE_MAX_N][SPLINE_MAX_N + 2];
  __shared__ double cp[SPLINE_MAX_M][2];
  __shared__ int piv_s, bad_s;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int M = K + A, N = M + 3, NC = N + 2;
  const float* p = poses + (int64_t)b * K * 2;
  const float* m = mu + (int64_t)b * K * 2;
  float* co = coef + (int64_t)b * N * 2;
  // the control points, and the finite test of every input
  int bad = 0;
  if (tid < M) {
    const float cy = tid < K ? p[2 * tid] : anchors[2 * (tid - K)];
    const float cx = tid < K ? p[2 * tid + 1] : anchors[2 * (tid - K) + 1];
    cp[tid][0] = (double)cy; cp[tid][1] = (double)cx;
    ctrl_out[((int64_t)b * M + tid) * 2] = cy; ctrl_out[((int64_t)b * M + tid) * 2 + 1] = cx;
    bad = !(isfinite(cy) && isfinite(cx));
    if (tid < K) bad = bad || !(isfinite(m[2 * tid]) && isfinite(m[2 * tid + 1]));
  }
  bad = __syncthreads_or(bad);
  // the augmented matrix
  if (!bad) {
    for (int idx = tid; idx < N * NC; idx += 256) {
      const int i = idx / NC, j = idx - i * NC;
      double v = 0.0;
      if (j >= N) {
        const int e = j - N;
        if (i < K) v = strength * ((double)m[2 * i + e] - cp[i][e]);
      } else if (i < M && j < M) {
        const double dy = cp[i][0] - cp[j][0], dx = cp[i][1] - cp[j][1];
        const double d2 = dy * dy + dx * dx;
        v = d2 > 0.0 ? d2 * log(d2) : 0.0;
        if (i == j) v = v + lam;
      } else if (i < M) {
        v = j == M ? 1.0 : cp[i][j - M - 1];
      } else if (j < M) {
        v = i == M ? 1.0 : cp[j][i - M - 1];
      }
      a[i][j] = v;
    }
    __syncthreads();
    for (int k = 0; k < N; ++k) {
      if (tid == 0) {
        int best = k;
        double big = fabs(a[k][k]);
        for (int i = k + 1; i < N; ++i) {
          const double v = fabs(a[i][k]);
          if (v > big) { big = v; best = i; }
        }
        const double pv = a[best][k];
        piv_s = best;
        bad_s = !(isfinite(pv) && pv != 0.0);
      }
      __syncthreads();
      const int piv = piv_s;
      if (bad_s) { bad = 1; break; }           // uniform: every thread reads the same LDS word
      if (piv != k) {
        for (int j = k + tid; j < NC; j += 256) {
          const double t = a[k][j];
          a[k][j] = a[piv][j];
          a[piv][j] = t;
        }
        __syncthreads();
      }
      const double pv = a[k][k];
      for (int i = k + 1 + tid; i < N; i += 256) a[i][k] = a[i][k] / pv;
      __syncthreads();
      const int nr = N - 1 - k, nc = NC - 1 - k;
      for (int idx = tid; idx < nr * nc; idx += 256) {
        const int i = k + 1 + idx / nc, j = k + 1 + idx % nc;
        a[i][j] = a[i][j] - a[i][k] * a[k][j];
      }
      __syncthreads();
    }
  }
  if (!bad) {
    // back substitution, column oriented: x_k, then its column leaves the right-hand sides of the rows above
    for (int k = N - 1; k >= 0; --k) {
      if (tid < 2) a[k][N + tid] = a[k][N + tid] / a[k][k];
      __syncthreads();
      for (int idx = tid; idx < 2 * k; idx += 256) {
        const int i = idx >> 1, e = idx & 1;
        a[i][N + e] = a[i][N + e] - a[i][k] * a[k][N + e];
      }
      __syncthreads();
    }
  }
  for (int idx = tid; idx < 2 * N; idx += 256)
    co[idx] = bad ? __builtin_nanf("") : (float)a[idx >> 1][N + (idx & 1)];
  if (tid == 0) flags[b] = bad ? 1 : 0;
}

struct WarpRow {
  SplineRow s;
  const float* cf;            // coef [M + 3][2]
};

struct WarpPolicy {
  typedef WarpRow Row;
  const int32_t* boxes;
  const float *inv_ramp, *ctrl, *coef;
  const uint8_t* sp;          // the row's photo in the ORIGINAL buffer
  int sh, sw, M;
  Row own;

  __device__ __forceinline__ Row row(int j) const {
    return Row{spline_row(boxes, inv_ramp, j, ctrl + (int64_t)j * 2 * M), coef + (int64_t)j * 2 * (M + 3)};
  }
  __device__ __forceinline__ bool covers(const Row& q, int r, int c) const { return paste_inside(q.s.box, r, c); }
  __device__ __forceinline__ void apply(const Row& q, int r, int c, float (&v)[3]) const {
#pragma clang fp contract(off)
    const float* const cf[1] = {q.cf};
    float qy, qx, D[1][2], g[3];
    spline_displace<1>(q.s, cf, M, r, c, qy, qx, D);
    const float sy = (float)r + q.s.hy * D[0][0], sx = (float)c + q.s.hx * D[0][1];
    if (!(isfinite(sy) && isfinite(sx))) return;
    paste_sample_photo(sp, sh, sw, sy, sx, g);
    paste_blend(v, g, paste_ramp(q.s.box, r, c, q.s.iry, q.s.irx));
  }
};

__global__ __launch_bounds__(256) void warp_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                      const int64_t* __restrict__ offs, const int32_t* __restrict__ hw, int n_images,
                                                      const int32_t* __restrict__ boxes, const int32_t* __restrict__ links,
                                                      const float* __restrict__ inv_ramp, const float* __restrict__ ctrl,
                                                      const float* __restrict__ coef, int M, int n) {
  __shared__ float ct_s[2 * SPLINE_MAX_M];
  __shared__ float cf_s[2 * SPLINE_MAX_N];
  const int b = blockIdx.y;
  PastePhoto ph;
  if (!paste_photo(boxes, offs, hw, n_images, b, ph)) return;      // uniform over the block: no barrier is skipped by part of it
  for (int i = threadIdx.x; i < 2 * M; i += 256) ct_s[i] = ctrl[(int64_t)b * 2 * M + i];
  for (int i = threadIdx.x; i < 2 * (M + 3); i += 256) cf_s[i] = coef[(int64_t)b * 2 * (M + 3) + i];
  __syncthreads();
  WarpPolicy pol{boxes, inv_ramp, ctrl, coef, src + ph.off, ph.sh, ph.sw, M};
  pol.own = WarpRow{spline_row(boxes, inv_ramp, b, ct_s), cf_s};
  paste_rows(pol, pol.own.s.box, ph, dst + ph.off, boxes, links, n);
}

extern "C" int imm_warp_fit(const float* poses, const float* mu, const float* anchors, int K, int A, int n, double strength, double lam,
                            float* coef, float* ctrl, int32_t* flags, void* stream) {
  IMM_REQUIRE(poses && mu && coef && ctrl && flags, "warp_fit: null pointer");
  IMM_REQUIRE(n > 0 && n <= 65535, "warp_fit: 0 < n <= 65535 rows (got %d)", n);
  IMM_REQUIRE(K >= 1 && A >= 0 && A % 4 == 0 && K <= SPLINE_MAX_M && A <= SPLINE_MAX_M && K + A >= 3 && K + A <= SPLINE_MAX_M,
              "warp_fit: K >= 1 landmarks and A = 4 m >= 0 anchors with 3 <= K + A <= %d (got %d, %d)", SPLINE_MAX_M, K, A);
  IMM_REQUIRE((A == 0) == (anchors == nullptr), "warp_fit: anchors must be NULL exactly when A == 0 (A = %d)", A);
  IMM_REQUIRE(strength - strength == 0.0, "warp_fit: strength must be finite (got %g)", strength);
  IMM_REQUIRE(lam >= 0.0 && lam - lam == 0.0, "warp_fit: lam must be finite and >= 0 (got %g)", lam);
  hipLaunchKernelGGL(warp_fit_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, poses, mu, anchors, K, A, strength, lam, coef, ctrl,
                     flags);
  IMM_CHECK_LAUNCH("imm_warp_fit");
  return 0;
}

extern "C" int imm_warp_u8(const uint8_t* src, uint8_t* dst, const int64_t* offsets, const int32_t* hw, int n_images, const int32_t* boxes,
                           const int32_t* links, const float* inv_ramp, const float* ctrl, const float* coef, int M, int n,
                           int max_box_pixels, void* stream) {
  IMM_REQUIRE(src && dst && offsets && hw && boxes && links && inv_ramp && ctrl && coef, "warp_u8: null pointer");
  IMM_REQUIRE(src != dst, "warp_u8: dst must be a copy of src, not src itself (every row samples the original pixels)");
  IMM_REQUIRE(n > 0 && n <= 65535 && n_images > 0, "warp_u8: 0 < n <= 65535 rows, n_images > 0 (got %d, %d)", n, n_images);
  IMM_REQUIRE(M >= 3 && M <= SPLINE_MAX_M, "warp_u8: 3 <= M <= %d control points (got %d)", SPLINE_MAX_M, M);
  IMM_REQUIRE(max_box_pixels > 0, "warp_u8: max_box_pixels > 0 (got %d)", max_box_pixels);
  hipLaunchKernelGGL(warp_u8_kernel, dim3(paste_grid_x(max_box_pixels), n), dim3(256), 0, (hipStream_t)stream, src, dst, offsets, hw, n_images,
                     boxes, links, inv_ramp, ctrl, coef, M, n);
  IMM_CHECK_LAUNCH("imm_warp_u8");
  return 0;
}
