// paste_common.h — the one skeleton of the kernels that paste into the caller's u8 photographs: compose_u8_kernel (compose.hip),
// unalign_u8_kernel (unalign.hip), warp_u8_kernel (warp.hip) and morph_u8_kernel (morph.hip).  Each file states its own pixel rule as a
// small policy; the launch shape, the ownership of a pixel, the row order and the rounding are stated here, once.
//
// Launch: grid (paste_grid_x(largest box), n), 256 threads; blockIdx.y is the row, one thread = one photo pixel (its three bytes) of the
// row's box clipped to the photo, in a grid-stride loop, so a box larger than the caller's figure is still covered.  Lanes of a wave take
// consecutive pixels of a photo row: 192 contiguous bytes read and written per wave.  Photo rows start at any byte (3 * width is odd for
// odd widths) and a box edge can fall inside any dword, whose other bytes belong to no box or to another thread, so the accesses are
// byte-wide.
// Ownership: overlapping rows of one photo are resolved without atomics.  links[j] = (the previous row of j's photo, the next one).  The
// thread of (row b, pixel) skips the pixel if b does not cover it or if an earlier row of this launch (links[.][0], downwards) covers it
// in the same photo; otherwise it alone owns the pixel: it reads it once, applies b and then the later rows of the photo that cover it
// (links[.][1], upwards), keeps the running value in registers with a rint after EVERY row (a later row blends over the rounded value),
// and writes it once.  Every thread that looks at a pixel decides "covers" from the same arithmetic, so every pixel of the launch has
// exactly one writer and no reader but that writer.
// Addressing: the downward walk accepts only 0 <= j < the row before it and the upward walk only the row before it < j < n, so device
// data cannot make a walk leave [0, n) or loop; a row of another photo met on a walk is passed over.  A photo byte is addressed only
// inside [0, h) x [0, w) of a photo whose index passed 0 <= image < n_images: the box is clipped to the photo here, and every sampling
// tap is clamped.  What the device buffers hold beyond that (scales, maps, coefficients) never reaches an address.
//
// A policy P supplies the rows:
//   P::own                          the block's row; its arrays may sit in LDS (warp, morph)
//   P::row(j)                       row j of the launch, read from global memory (rows met on a walk)
//   P::covers(q, r, c)              does row q cover photo pixel (r, c), and is it active
//   P::apply(q, r, c, v)            blend row q over the running value v at a pixel it covers
// Every helper that does f32 arithmetic carries its own fp contract(off): the pragma does not follow code into another function, and
// every operation is rounded separately, in the order written, bit-identical to the f32 host restatements of the tests.
#pragma once
#include "common.h"

#define SPLINE_MAX_M 80                      // control points of a thin-plate spline (imm_warp_fit, imm_warp_u8, imm_morph_u8)
#define SPLINE_MAX_N (SPLINE_MAX_M + 3)      // with the affine part

// the x-dimension of the grid from the caller's largest box
static inline int paste_grid_x(int max_pixels) {
  const int64_t blocks = ((int64_t)max_pixels + 255) / 256;
  return (int)(blocks < 65536 ? blocks : 65536);
}

struct PasteBox {
  int y0, x0, y1, x1;                        // half-open
};

__device__ __forceinline__ PasteBox paste_box(const int32_t* __restrict__ boxes, int j) {
  return PasteBox{boxes[5 * j + 1], boxes[5 * j + 2], boxes[5 * j + 3], boxes[5 * j + 4]};
}

__device__ __forceinline__ bool paste_inside(const PasteBox& q, int r, int c) { return r >= q.y0 && r < q.y1 && c >= q.x0 && c < q.x1; }

struct PastePhoto {
  int img, sh, sw;
  int64_t off;                               // of the photo in the packed buffer
};

// the photo of row b; false (uniform over the block) when its image index is out of range
__device__ __forceinline__ bool paste_photo(const int32_t* __restrict__ boxes, const int64_t* __restrict__ offs,
                                            const int32_t* __restrict__ hw, int n_images, int b, PastePhoto& ph) {
  ph.img = boxes[5 * b];
  if (ph.img < 0 || ph.img >= n_images) return false;
  ph.sh = hw[2 * ph.img]; ph.sw = hw[2 * ph.img + 1];
  ph.off = offs[ph.img];
  return true;
}

// the linear edge ramp of a box: 1 in the middle, falling to (0.5 * inv_ramp) at the outermost pixel
__device__ __forceinline__ float paste_ramp(const PasteBox& q, int r, int c, float iry, float irx) {
#pragma clang fp contract(off)
  const float wy = fminf(1.f, ((float)min(r - q.y0, q.y1 - 1 - r) + 0.5f) * iry);
  const float wx = fminf(1.f, ((float)min(c - q.x0, q.x1 - 1 - c) + 0.5f) * irx);
  return wy * wx;
}

// v <- rint(v + a * (g - v)), nearest even.  In contract the sum is already in [0, 255]; the clamp keeps weights outside [0, 1] from
// wrapping the byte.
__device__ __forceinline__ void paste_blend(float (&v)[3], const float (&g)[3], float a) {
#pragma clang fp contract(off)
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float d = g[ch] - v[ch];
    const float m = a * d;
    v[ch] = fminf(fmaxf(rintf(v[ch] + m), 0.f), 255.f);
  }
}

// clip(bilinear(face, fy, fx), 0, 255) of an f32 face [S, S, ld]: taps floor and min(floor + 1, S - 1); a + (b - a) * t
__device__ __forceinline__ void paste_sample_face(const float* __restrict__ f, int S, int ld, float fy, float fx, float (&g)[3]) {
#pragma clang fp contract(off)
  const int yl = min(max((int)floorf(fy), 0), S - 1), xl = min(max((int)floorf(fx), 0), S - 1);
  const int yh = min(yl + 1, S - 1), xh = min(xl + 1, S - 1);
  const float ty = fy - (float)yl, tx = fx - (float)xl;
  const float* tlp = f + ((int64_t)yl * S + xl) * ld;
  const float* trp = f + ((int64_t)yl * S + xh) * ld;
  const float* blp = f + ((int64_t)yh * S + xl) * ld;
  const float* brp = f + ((int64_t)yh * S + xh) * ld;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float tl = tlp[ch], tr = trp[ch], bl = blp[ch], br = brp[ch];
    const float top = tl + (tr - tl) * tx;
    const float bot = bl + (br - bl) * tx;
    g[ch] = fminf(fmaxf(top + (bot - top) * ty, 0.f), 255.f);
  }
}

// bilinear(photo, sy, sx) of a u8 photo [sh, sw, 3] at a finite place: clamped in float first (a finite s can lie far outside what an
// int holds), then every tap to the photo
__device__ __forceinline__ void paste_sample_photo(const uint8_t* __restrict__ sp, int sh, int sw, float sy, float sx, float (&g)[3]) {
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

// The pixel loop of row blockIdx.y over span (its box or bounding box), as the header states it.  photo is the row's photo in the buffer
// that is written.
template <class P>
__device__ __forceinline__ void paste_rows(const P& pol, const PasteBox& span, const PastePhoto& ph, uint8_t* __restrict__ photo,
                                           const int32_t* __restrict__ boxes, const int32_t* __restrict__ links, int n) {
  const int b = blockIdx.y;
  const int cy0 = max(span.y0, 0), cy1 = min(span.y1, ph.sh), cx0 = max(span.x0, 0), cx1 = min(span.x1, ph.sw);
  const int cw = cx1 - cx0, chh = cy1 - cy0;
  if (cw <= 0 || chh <= 0) return;
  const int64_t area = (int64_t)cw * chh;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < area; p += (int64_t)gridDim.x * 256) {
    const int pr = (int)(p / cw);
    const int r = cy0 + pr, c = cx0 + (int)(p - (int64_t)pr * cw);
    if (!pol.covers(pol.own, r, c)) continue;
    bool owned = true;
    for (int j = links[2 * b], last = b; j >= 0 && j < last; last = j, j = links[2 * j]) {
      if (boxes[5 * j] == ph.img && pol.covers(pol.row(j), r, c)) {
        owned = false;
        break;
      }
    }
    if (!owned) continue;
    uint8_t* px = photo + ((int64_t)r * ph.sw + c) * 3;
    float v[3] = {(float)px[0], (float)px[1], (float)px[2]};
    pol.apply(pol.own, r, c, v);
    for (int j = b;;) {
      const int nx = links[2 * j + 1];
      if (nx <= j || nx >= n) break;
      j = nx;
      if (boxes[5 * j] != ph.img) continue;
      const typename P::Row q = pol.row(j);
      if (pol.covers(q, r, c)) pol.apply(q, r, c, v);
    }
    px[0] = (uint8_t)v[0]; px[1] = (uint8_t)v[1]; px[2] = (uint8_t)v[2];
  }
}

// ---- the thin-plate spline of imm_warp_u8 and imm_morph_u8 ----

struct SplineRow {
  PasteBox box;
  float ry, rx, hy, hx;                      // the box: frame scale 2 / H, 2 / W and half sides
  float iry, irx;                            // its edge ramp
  const float* ct;                           // its control points [M][2]
};

// row j's box and scales, without its edge ramp (imm_seam_fit blends nothing)
__device__ __forceinline__ SplineRow spline_box(const int32_t* __restrict__ boxes, int j, const float* ct) {
  SplineRow q;
  q.box = paste_box(boxes, j);
  const int ih = q.box.y1 - q.box.y0, iw = q.box.x1 - q.box.x0;
  // the correctly rounded float quotient of two small integers (an empty box covers no pixel: its scales are never used)
  q.ry = ih > 0 ? (float)(2.0 / (double)ih) : 0.f;
  q.rx = iw > 0 ? (float)(2.0 / (double)iw) : 0.f;
  q.hy = 0.5f * (float)ih; q.hx = 0.5f * (float)iw;
  q.iry = q.irx = 0.f;
  q.ct = ct;
  return q;
}

__device__ __forceinline__ SplineRow spline_row(const int32_t* __restrict__ boxes, const float* __restrict__ inv_ramp, int j,
                                                const float* ct) {
  SplineRow q = spline_box(boxes, j, ct);
  q.iry = inv_ramp[2 * j]; q.irx = inv_ramp[2 * j + 1];
  return q;
}

// For each of NS coefficient sets cf[s] [M + 3][2] on row q's control points, D[s] = sum_j w_j U(|q - ctrl_j|^2) + a_0 + a_1 q_y + a_2 q_x at
// the frame coordinate (qy, qx): one basis evaluation (one logf) feeds every set.
template <int NS>
__device__ __forceinline__ void spline_sum(const SplineRow& q, const float* const (&cf)[NS], int M, float qy, float qx, float (&D)[NS][2]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int s = 0; s < NS; ++s) D[s][0] = D[s][1] = 0.f;
  for (int j = 0; j < M; ++j) {
    const float dy = qy - q.ct[2 * j], dx = qx - q.ct[2 * j + 1];
    const float d2 = dy * dy + dx * dx;
    const float u = d2 > 0.f ? d2 * logf(d2) : 0.f;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      D[s][0] = D[s][0] + cf[s][2 * j] * u;
      D[s][1] = D[s][1] + cf[s][2 * j + 1] * u;
    }
  }
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    D[s][0] = ((D[s][0] + cf[s][2 * M]) + cf[s][2 * M + 2] * qy) + cf[s][2 * M + 4] * qx;
    D[s][1] = ((D[s][1] + cf[s][2 * M + 1]) + cf[s][2 * M + 3] * qy) + cf[s][2 * M + 5] * qx;
  }
}

// The frame coordinate (qy, qx) of photo pixel (r, c) in row q's box and the displacements D[s] there.
template <int NS>
__device__ __forceinline__ void spline_displace(const SplineRow& q, const float* const (&cf)[NS], int M, int r, int c, float& qy, float& qx,
                                                float (&D)[NS][2]) {
#pragma clang fp contract(off)
  qy = (float)(r - q.box.y0) * q.ry - 1.f; qx = (float)(c - q.box.x0) * q.rx - 1.f;
  spline_sum<NS>(q, cf, M, qy, qx, D);
}

// The same at a fractional place (fy, fx) of the box, in box-relative pixels (the ring samples of imm_seam_fit).
template <int NS>
__device__ __forceinline__ void spline_displace_at(const SplineRow& q, const float* const (&cf)[NS], int M, float fy, float fx, float& qy,
                                                   float& qx, float (&D)[NS][2]) {
#pragma clang fp contract(off)
  qy = fy * q.ry - 1.f; qx = fx * q.rx - 1.f;
  spline_sum<NS>(q, cf, M, qy, qx, D);
}
