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
// Warp: the launch shape of compose.hip, grid (blocks, n), one thread = one photo pixel (its three bytes), grid-stride loop.  The
// row's ctrl [M][2] and coef [M + 3][2] sit in 1.3 KB of LDS, read by every lane at the same address (a broadcast, no bank conflict);
// the kernel is bound by its M logf per pixel, not by the 6 bytes per pixel it moves.  Rows met on a link walk (overlapping boxes) read
// their ctrl and coef through L2.  Ownership of a pixel follows compose.hip: the first row of the launch whose box covers it.
// Addressing: a photo byte is addressed only through a tap clamped to [0, h - 1] x [0, w - 1] of a photo whose index passed
// 0 <= image < n_images; ctrl and coef are indexed by a row index in [0, n) and j < M + 3; the values they hold never reach an address.
#include "common.h"

#define WARP_MAX_M 80
#define WARP_MAX_N (WARP_MAX_M + 3)

__global__ __launch_bounds__(256) void warp_fit_kernel(const float* __restrict__ poses, const float* __restrict__ mu,
                                                       const float* __restrict__ anchors, int K, int A, double strength, double lam,
                                                       float* __restrict__ coef, float* __restrict__ ctrl_out, int32_t* __restrict__ flags) {
#pragma clang fp contract(off)   // every operation rounded separately, as the host restatement's
  __shared__ double a[WARP_MAX_N][WARP_MAX_N + 2];
  __shared__ double cp[WARP_MAX_M][2];
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
  int y0, x0, y1, x1;
  float ry, rx, hy, hx;
};

__device__ __forceinline__ WarpRow warp_row(const int32_t* __restrict__ boxes, int j) {
  WarpRow q;
  q.y0 = boxes[5 * j + 1]; q.x0 = boxes[5 * j + 2]; q.y1 = boxes[5 * j + 3]; q.x1 = boxes[5 * j + 4];
  const int ih = q.y1 - q.y0, iw = q.x1 - q.x0;
  // the correctly rounded float quotient of two small integers (an empty box covers no pixel: its scales are never used)
  q.ry = ih > 0 ? (float)(2.0 / (double)ih) : 0.f;
  q.rx = iw > 0 ? (float)(2.0 / (double)iw) : 0.f;
  q.hy = 0.5f * (float)ih; q.hx = 0.5f * (float)iw;
  return q;
}

// Row q at photo pixel (r, c): the running value v blended with the warped sample.  ct [M][2] and cf [M + 3][2] are the row's control
// points and coefficients (LDS for the block's own row, global memory for a row met on a link walk).
__device__ __forceinline__ void warp_apply(const WarpRow& q, const float* ct, const float* cf, int M, int r, int c, float iry, float irx,
                                           const uint8_t* __restrict__ sp, int sh, int sw, float (&v)[3]) {
#pragma clang fp contract(off)
  const float qy = (float)(r - q.y0) * q.ry - 1.f, qx = (float)(c - q.x0) * q.rx - 1.f;
  float Dy = 0.f, Dx = 0.f;
  for (int j = 0; j < M; ++j) {
    const float dy = qy - ct[2 * j], dx = qx - ct[2 * j + 1];
    const float d2 = dy * dy + dx * dx;
    const float u = d2 > 0.f ? d2 * logf(d2) : 0.f;
    Dy = Dy + cf[2 * j] * u;
    Dx = Dx + cf[2 * j + 1] * u;
  }
  Dy = ((Dy + cf[2 * M]) + cf[2 * M + 2] * qy) + cf[2 * M + 4] * qx;
  Dx = ((Dx + cf[2 * M + 1]) + cf[2 * M + 3] * qy) + cf[2 * M + 5] * qx;
  const float sy = (float)r + q.hy * Dy, sx = (float)c + q.hx * Dx;
  if (!(isfinite(sy) && isfinite(sx))) return;
  const float fy = floorf(sy), fx = floorf(sx);
  const float ty = sy - fy, tx = sx - fx;
  // clamped in float first (a finite s can lie far outside what an int holds), then to the photo
  const int iy = (int)fminf(fmaxf(fy, -1.f), (float)sh), ix = (int)fminf(fmaxf(fx, -1.f), (float)sw);
  const int yl = min(max(iy, 0), sh - 1), yh = min(max(iy + 1, 0), sh - 1);
  const int xl = min(max(ix, 0), sw - 1), xh = min(max(ix + 1, 0), sw - 1);
  const float wy = fminf(1.f, ((float)min(r - q.y0, q.y1 - 1 - r) + 0.5f) * iry);
  const float wx = fminf(1.f, ((float)min(c - q.x0, q.x1 - 1 - c) + 0.5f) * irx);
  const float al = wy * wx;
  const uint8_t* tlp = sp + ((int64_t)yl * sw + xl) * 3;
  const uint8_t* trp = sp + ((int64_t)yl * sw + xh) * 3;
  const uint8_t* blp = sp + ((int64_t)yh * sw + xl) * 3;
  const uint8_t* brp = sp + ((int64_t)yh * sw + xh) * 3;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float tl = (float)tlp[ch], tr = (float)trp[ch], bl = (float)blp[ch], br = (float)brp[ch];
    const float top = tl + (tr - tl) * tx;
    const float bot = bl + (br - bl) * tx;
    const float g = top + (bot - top) * ty;
    const float d = g - v[ch];
    const float mm = al * d;
    v[ch] = fminf(fmaxf(rintf(v[ch] + mm), 0.f), 255.f);
  }
}

__global__ __launch_bounds__(256) void warp_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                      const int64_t* __restrict__ offs, const int32_t* __restrict__ hw, int n_images,
                                                      const int32_t* __restrict__ boxes, const int32_t* __restrict__ links,
                                                      const float* __restrict__ inv_ramp, const float* __restrict__ ctrl,
                                                      const float* __restrict__ coef, int M, int n) {
  __shared__ float ct_s[2 * WARP_MAX_M];
  __shared__ float cf_s[2 * WARP_MAX_N];
  const int b = blockIdx.y;
  const int img = boxes[5 * b];
  if (img < 0 || img >= n_images) return;            // uniform over the block: no barrier is skipped by part of it
  const int sh = hw[2 * img], sw = hw[2 * img + 1];
  const WarpRow own = warp_row(boxes, b);
  // the part of box b inside the photo
  const int cy0 = max(own.y0, 0), cy1 = min(own.y1, sh), cx0 = max(own.x0, 0), cx1 = min(own.x1, sw);
  const int cw = cx1 - cx0, chh = cy1 - cy0;
  if (cw <= 0 || chh <= 0) return;
  for (int i = threadIdx.x; i < 2 * M; i += 256) ct_s[i] = ctrl[(int64_t)b * 2 * M + i];
  for (int i = threadIdx.x; i < 2 * (M + 3); i += 256) cf_s[i] = coef[(int64_t)b * 2 * (M + 3) + i];
  __syncthreads();
  const int64_t area = (int64_t)cw * chh;
  const uint8_t* sp = src + offs[img];
  uint8_t* photo = dst + offs[img];
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < area; p += (int64_t)gridDim.x * 256) {
    const int pr = (int)(p / cw);
    const int r = cy0 + pr, c = cx0 + (int)(p - (int64_t)pr * cw);
    // an earlier row of this launch that covers (r, c) in the same photo owns the pixel.  The chain must step strictly downwards
    // (upwards below): device data cannot make the walk leave [0, n) or loop.
    bool owned = true;
    for (int j = links[2 * b], last = b; j >= 0 && j < last; last = j, j = links[2 * j]) {
      if (boxes[5 * j] == img && r >= boxes[5 * j + 1] && r < boxes[5 * j + 3] && c >= boxes[5 * j + 2] && c < boxes[5 * j + 4]) {
        owned = false;
        break;
      }
    }
    if (!owned) continue;
    uint8_t* px = photo + ((int64_t)r * sw + c) * 3;
    float v[3] = {(float)px[0], (float)px[1], (float)px[2]};
    warp_apply(own, ct_s, cf_s, M, r, c, inv_ramp[2 * b], inv_ramp[2 * b + 1], sp, sh, sw, v);
    for (int j = b;;) {
      const int nx = links[2 * j + 1];
      if (nx <= j || nx >= n) break;
      j = nx;
      if (boxes[5 * j] != img) continue;             // a foreign row in the chain covers nothing
      const WarpRow q = warp_row(boxes, j);
      if (r >= q.y0 && r < q.y1 && c >= q.x0 && c < q.x1)
        warp_apply(q, ctrl + (int64_t)j * 2 * M, coef + (int64_t)j * 2 * (M + 3), M, r, c, inv_ramp[2 * j], inv_ramp[2 * j + 1], sp, sh,
                   sw, v);
    }
    px[0] = (uint8_t)v[0]; px[1] = (uint8_t)v[1]; px[2] = (uint8_t)v[2];
  }
}

extern "C" int imm_warp_fit(const float* poses, const float* mu, const float* anchors, int K, int A, int n, double strength, double lam,
                            float* coef, float* ctrl, int32_t* flags, void* stream) {
  IMM_REQUIRE(poses && mu && coef && ctrl && flags, "warp_fit: null pointer");
  IMM_REQUIRE(n > 0 && n <= 65535, "warp_fit: 0 < n <= 65535 rows (got %d)", n);
  IMM_REQUIRE(K >= 1 && A >= 0 && A % 4 == 0 && K <= WARP_MAX_M && A <= WARP_MAX_M && K + A >= 3 && K + A <= WARP_MAX_M,
              "warp_fit: K >= 1 landmarks and A = 4 m >= 0 anchors with 3 <= K + A <= %d (got %d, %d)", WARP_MAX_M, K, A);
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
  IMM_REQUIRE(M >= 3 && M <= WARP_MAX_M, "warp_u8: 3 <= M <= %d control points (got %d)", WARP_MAX_M, M);
  IMM_REQUIRE(max_box_pixels > 0, "warp_u8: max_box_pixels > 0 (got %d)", max_box_pixels);
  // the grid is sized by the caller's largest box; a row with more pixels than that is still covered (grid-stride loop)
  const int blocks = (int)((((int64_t)max_box_pixels + 255) / 256 < 65536) ? ((int64_t)max_box_pixels + 255) / 256 : 65536);
  hipLaunchKernelGGL(warp_u8_kernel, dim3(blocks, n), dim3(256), 0, (hipStream_t)stream, src, dst, offsets, hw, n_images, boxes, links,
                     inv_ramp, ctrl, coef, M, n);
  IMM_CHECK_LAUNCH("imm_warp_u8");
  return 0;
}
