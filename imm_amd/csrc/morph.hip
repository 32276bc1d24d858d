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
// Poses: one thread per float, nothing shared.  Morph: the launch shape of warp.hip, grid (blocks, n), one thread = one photo pixel (its
// three bytes), grid-stride loop; the row's ctrl [M][2], coef_a and coef_b [M + 3][2] sit in 2.0 KB of LDS, read by every lane at the same
// address (broadcasts).  The kernel is bound by its M logf per pixel, as imm_warp_u8 is: the second spline adds two multiply-adds per
// control point and four more byte taps per pixel, no logarithm.  Rows met on a link walk read their ctrl and coef through L2.
// A row is ACTIVE when its donor image index lies in [0, n_donor_images) and its donor box has H > 0 and W > 0; a row that is not writes
// nothing and owns nothing (the walks pass over it), so the rows of a call give the same bytes however they are split into launches.
// Addressing: a photo byte is addressed only through a tap clamped to [0, h - 1] x [0, w - 1] of a photo whose index passed
// 0 <= image < n_images (0 <= donor image < n_donor_images); ctrl and coef are indexed by a row index in [0, n) and j < M + 3; the values
// they hold never reach an address.
#include "common.h"

#define MORPH_MAX_M 80
#define MORPH_MAX_N (MORPH_MAX_M + 3)

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

struct MorphRow {
  int y0, x0, y1, x1;
  float ry, rx, hy, hx;       // the row's own box: frame scale and half sides
  float by, bx, dhy, dhx;     // the donor box: corner and half sides
  int dimg;                   // the donor photo, -1: the row is not active
};

__device__ __forceinline__ MorphRow morph_row(const int32_t* __restrict__ boxes, const int32_t* __restrict__ dboxes, int n_donor, int j) {
  MorphRow q;
  q.y0 = boxes[5 * j + 1]; q.x0 = boxes[5 * j + 2]; q.y1 = boxes[5 * j + 3]; q.x1 = boxes[5 * j + 4];
  const int ih = q.y1 - q.y0, iw = q.x1 - q.x0;
  // the correctly rounded float quotient of two small integers (an empty box covers no pixel: its scales are never used)
  q.ry = ih > 0 ? (float)(2.0 / (double)ih) : 0.f;
  q.rx = iw > 0 ? (float)(2.0 / (double)iw) : 0.f;
  q.hy = 0.5f * (float)ih; q.hx = 0.5f * (float)iw;
  const int di = dboxes[5 * j], dy0 = dboxes[5 * j + 1], dx0 = dboxes[5 * j + 2];
  // in 64 bits: the sides of a box row that holds anything
  const int64_t dh = (int64_t)dboxes[5 * j + 3] - dy0, dw = (int64_t)dboxes[5 * j + 4] - dx0;
  q.by = (float)dy0; q.bx = (float)dx0;
  q.dhy = 0.5f * (float)dh; q.dhx = 0.5f * (float)dw;
  q.dimg = (di >= 0 && di < n_donor && dh > 0 && dw > 0) ? di : -1;
  return q;
}

// The bilinear sample of photo sp [sh, sw, 3] at the finite place (sy, sx), imm_warp_u8's: clamped in float first (a finite s can lie far
// outside what an int holds), then every tap to the photo.
__device__ __forceinline__ void morph_sample(const uint8_t* __restrict__ sp, int sh, int sw, float sy, float sx, float (&g)[3]) {
#pragma clang fp contract(off)
  const float fy = floorf(sy), fx = floorf(sx);
  const float ty = sy - fy, tx = sx - fx;
  const int iy = (int)fminf(fmaxf(fy, -1.f), (float)sh), ix = (int)fminf(fmaxf(fx, -1.f), (float)sw);
  const int yl = min(max(iy, 0), sh - 1), yh = min(max(iy + 1, 0), sh - 1);
  const int xl = min(max(ix, 0), sw - 1), xh = min(max(ix + 1, 0), sw - 1);
  const uint8_t* tlp = sp + ((int64_t)yl * sw + xl) * 3;
  const uint8_t* trp = sp + ((int64_t)yl * sw + xh) * 3;
  const uint8_t* blp = sp + ((int64_t)yh * sw + xl) * 3;
  const uint8_t* brp = sp + ((int64_t)yh * sw + xh) * 3;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float tl = (float)tlp[ch], tr = (float)trp[ch], bl = (float)blp[ch], br = (float)brp[ch];
    const float top = tl + (tr - tl) * tx;
    const float bot = bl + (br - bl) * tx;
    g[ch] = top + (bot - top) * ty;
  }
}

// Active row q at photo pixel (r, c): the running value v blended with the mix of the two warped samples.  ct [M][2], ca and cb [M + 3][2]
// are the row's control points and its two coefficient sets (LDS for the block's own row, global memory for a row met on a link walk).
__device__ __forceinline__ void morph_apply(const MorphRow& q, const float* ct, const float* ca, const float* cb, int M, int r, int c,
                                            float iry, float irx, float tex, const uint8_t* __restrict__ sp, int sh, int sw,
                                            const uint8_t* __restrict__ dp, int dh, int dw, float (&v)[3]) {
#pragma clang fp contract(off)
  const float qy = (float)(r - q.y0) * q.ry - 1.f, qx = (float)(c - q.x0) * q.rx - 1.f;
  float Ay = 0.f, Ax = 0.f, By = 0.f, Bx = 0.f;
  for (int j = 0; j < M; ++j) {
    const float dy = qy - ct[2 * j], dx = qx - ct[2 * j + 1];
    const float d2 = dy * dy + dx * dx;
    const float u = d2 > 0.f ? d2 * logf(d2) : 0.f;
    Ay = Ay + ca[2 * j] * u;
    Ax = Ax + ca[2 * j + 1] * u;
    By = By + cb[2 * j] * u;
    Bx = Bx + cb[2 * j + 1] * u;
  }
  Ay = ((Ay + ca[2 * M]) + ca[2 * M + 2] * qy) + ca[2 * M + 4] * qx;
  Ax = ((Ax + ca[2 * M + 1]) + ca[2 * M + 3] * qy) + ca[2 * M + 5] * qx;
  By = ((By + cb[2 * M]) + cb[2 * M + 2] * qy) + cb[2 * M + 4] * qx;
  Bx = ((Bx + cb[2 * M + 1]) + cb[2 * M + 3] * qy) + cb[2 * M + 5] * qx;
  const float ay = (float)r + q.hy * Ay, ax = (float)c + q.hx * Ax;
  const float by = q.by + ((qy + By) + 1.f) * q.dhy, bx = q.bx + ((qx + Bx) + 1.f) * q.dhx;
  if (!(isfinite(ay) && isfinite(ax) && isfinite(by) && isfinite(bx))) return;
  float ga[3], gb[3];
  morph_sample(sp, sh, sw, ay, ax, ga);
  morph_sample(dp, dh, dw, by, bx, gb);
  const float wy = fminf(1.f, ((float)min(r - q.y0, q.y1 - 1 - r) + 0.5f) * iry);
  const float wx = fminf(1.f, ((float)min(c - q.x0, q.x1 - 1 - c) + 0.5f) * irx);
  const float al = wy * wx;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float e = gb[ch] - ga[ch];
    const float te = tex * e;
    const float mix = ga[ch] + te;
    const float d = mix - v[ch];
    const float mm = al * d;
    v[ch] = fminf(fmaxf(rintf(v[ch] + mm), 0.f), 255.f);
  }
}

__global__ __launch_bounds__(256) void morph_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                       const int64_t* __restrict__ offs, const int32_t* __restrict__ hw, int n_images,
                                                       const uint8_t* __restrict__ donor, const int64_t* __restrict__ doffs,
                                                       const int32_t* __restrict__ dhw, int n_donor, const int32_t* __restrict__ boxes,
                                                       const int32_t* __restrict__ dboxes, const int32_t* __restrict__ links,
                                                       const float* __restrict__ inv_ramp, const float* __restrict__ texture,
                                                       const float* __restrict__ ctrl, const float* __restrict__ coef_a,
                                                       const float* __restrict__ coef_b, int M, int n) {
  __shared__ float ct_s[2 * MORPH_MAX_M];
  __shared__ float ca_s[2 * MORPH_MAX_N];
  __shared__ float cb_s[2 * MORPH_MAX_N];
  const int b = blockIdx.y;
  const int img = boxes[5 * b];
  if (img < 0 || img >= n_images) return;            // uniform over the block: no barrier is skipped by part of it
  const MorphRow own = morph_row(boxes, dboxes, n_donor, b);
  if (own.dimg < 0) return;                          // not active: uniform as well
  const int sh = hw[2 * img], sw = hw[2 * img + 1];
  // the part of box b inside the photo
  const int cy0 = max(own.y0, 0), cy1 = min(own.y1, sh), cx0 = max(own.x0, 0), cx1 = min(own.x1, sw);
  const int cw = cx1 - cx0, chh = cy1 - cy0;
  if (cw <= 0 || chh <= 0) return;
  for (int i = threadIdx.x; i < 2 * M; i += 256) ct_s[i] = ctrl[(int64_t)b * 2 * M + i];
  for (int i = threadIdx.x; i < 2 * (M + 3); i += 256) {
    ca_s[i] = coef_a[(int64_t)b * 2 * (M + 3) + i];
    cb_s[i] = coef_b[(int64_t)b * 2 * (M + 3) + i];
  }
  __syncthreads();
  const int64_t area = (int64_t)cw * chh;
  const uint8_t* sp = src + offs[img];
  uint8_t* photo = dst + offs[img];
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < area; p += (int64_t)gridDim.x * 256) {
    const int pr = (int)(p / cw);
    const int r = cy0 + pr, c = cx0 + (int)(p - (int64_t)pr * cw);
    // an earlier ACTIVE row of this launch that covers (r, c) in the same photo owns the pixel.  The chain must step strictly downwards
    // (upwards below): device data cannot make the walk leave [0, n) or loop.
    bool owned = true;
    for (int j = links[2 * b], last = b; j >= 0 && j < last; last = j, j = links[2 * j]) {
      if (boxes[5 * j] == img && r >= boxes[5 * j + 1] && r < boxes[5 * j + 3] && c >= boxes[5 * j + 2] && c < boxes[5 * j + 4] &&
          morph_row(boxes, dboxes, n_donor, j).dimg >= 0) {
        owned = false;
        break;
      }
    }
    if (!owned) continue;
    uint8_t* px = photo + ((int64_t)r * sw + c) * 3;
    float v[3] = {(float)px[0], (float)px[1], (float)px[2]};
    morph_apply(own, ct_s, ca_s, cb_s, M, r, c, inv_ramp[2 * b], inv_ramp[2 * b + 1], texture[b], sp, sh, sw, donor + doffs[own.dimg],
                dhw[2 * own.dimg], dhw[2 * own.dimg + 1], v);
    for (int j = b;;) {
      const int nx = links[2 * j + 1];
      if (nx <= j || nx >= n) break;
      j = nx;
      if (boxes[5 * j] != img) continue;             // a foreign row in the chain covers nothing
      const MorphRow q = morph_row(boxes, dboxes, n_donor, j);
      if (q.dimg >= 0 && r >= q.y0 && r < q.y1 && c >= q.x0 && c < q.x1)
        morph_apply(q, ctrl + (int64_t)j * 2 * M, coef_a + (int64_t)j * 2 * (M + 3), coef_b + (int64_t)j * 2 * (M + 3), M, r, c,
                    inv_ramp[2 * j], inv_ramp[2 * j + 1], texture[j], sp, sh, sw, donor + doffs[q.dimg], dhw[2 * q.dimg],
                    dhw[2 * q.dimg + 1], v);
    }
    px[0] = (uint8_t)v[0]; px[1] = (uint8_t)v[1]; px[2] = (uint8_t)v[2];
  }
}

extern "C" int imm_morph_poses(const float* mu_a, const float* mu_b, const float* shape, int K, int n, float* poses2, float* mu2,
                               void* stream) {
  IMM_REQUIRE(mu_a && mu_b && shape && poses2 && mu2, "morph_poses: null pointer");
  IMM_REQUIRE(n > 0 && n <= 32767, "morph_poses: 0 < n <= 32767 rows, so that one fit serves 2 n (got %d)", n);
  IMM_REQUIRE(K >= 1 && K <= MORPH_MAX_M, "morph_poses: 1 <= K <= %d landmarks (got %d)", MORPH_MAX_M, K);
  const int64_t total = (int64_t)n * K * 2;
  hipLaunchKernelGGL(morph_poses_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, mu_a, mu_b, shape, 2 * K,
                     total, poses2, mu2);
  IMM_CHECK_LAUNCH("imm_morph_poses");
  return 0;
}

extern "C" int imm_morph_u8(const uint8_t* src, uint8_t* dst, const int64_t* offsets, const int32_t* hw, int n_images, const uint8_t* donor,
                            const int64_t* donor_offsets, const int32_t* donor_hw, int n_donor_images, const int32_t* boxes,
                            const int32_t* donor_boxes, const int32_t* links, const float* inv_ramp, const float* texture, const float* ctrl,
                            const float* coef_a, const float* coef_b, int M, int n, int max_box_pixels, void* stream) {
  IMM_REQUIRE(src && dst && offsets && hw && donor && donor_offsets && donor_hw && boxes && donor_boxes && links && inv_ramp && texture &&
                  ctrl && coef_a && coef_b, "morph_u8: null pointer");
  IMM_REQUIRE(src != dst, "morph_u8: dst must be a copy of src, not src itself (every row samples the original pixels)");
  IMM_REQUIRE(donor != dst, "morph_u8: the donor buffer is read only and must not be dst");
  IMM_REQUIRE(n > 0 && n <= 65535 && n_images > 0 && n_donor_images > 0,
              "morph_u8: 0 < n <= 65535 rows, n_images > 0, n_donor_images > 0 (got %d, %d, %d)", n, n_images, n_donor_images);
  IMM_REQUIRE(M >= 3 && M <= MORPH_MAX_M, "morph_u8: 3 <= M <= %d control points (got %d)", MORPH_MAX_M, M);
  IMM_REQUIRE(max_box_pixels > 0, "morph_u8: max_box_pixels > 0 (got %d)", max_box_pixels);
  // the grid is sized by the caller's largest box; a row with more pixels than that is still covered (grid-stride loop)
  const int blocks = (int)((((int64_t)max_box_pixels + 255) / 256 < 65536) ? ((int64_t)max_box_pixels + 255) / 256 : 65536);
  hipLaunchKernelGGL(morph_u8_kernel, dim3(blocks, n), dim3(256), 0, (hipStream_t)stream, src, dst, offsets, hw, n_images, donor,
                     donor_offsets, donor_hw, n_donor_images, boxes, donor_boxes, links, inv_ramp, texture, ctrl, coef_a, coef_b, M, n);
  IMM_CHECK_LAUNCH("imm_morph_u8");
  return 0;
}
