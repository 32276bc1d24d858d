// compose.hip — the generator's last stage on gfx950: generated S x S faces pasted back into the caller's u8 photographs
// (imm_amd/generation.py ImageGenerator.repose).  The inverse of the box crop of image_io.hip: row b's face is resampled to the size of
// box b, blended over the photo's own pixels with a linear edge ramp and rounded back to u8, in place, in row order:
//
//   fy = (r - y0) * sy,  sy = (S - 1) / (ih - 1) as a double quotient rounded once (0 when ih == 1)      frame coordinate of photo
//   fx likewise                                                                                          pixel (r, c) of box b
//   g  = clip(bilinear(faces[b], fy, fx), 0, 255)         taps floor and min(floor + 1, S - 1); a + (b - a) * t, unfused
//   a  = wy * wx,  wy = min(1, (min(r - y0, y1 - 1 - r) + 0.5) * inv_ramp[b][0]),  wx with inv_ramp[b][1]
//   photo[r, c] = rint(p + a * (g - p))                   nearest even, after EVERY row: a later row blends over the rounded value
//
// The crop maps frame index o to box coordinate o * (ih - 1) / (S - 1) (align corners), so the map above is its exact inverse; at
// ih == S both scales are 1 and every photo pixel meets one face pixel with weight 1 on one tap.
//
// paste_common.h states the launch shape, the ownership of a pixel under overlapping boxes and the addressing argument.  The faces
// (f32, S * S * ld * 4 bytes per row, 256 KB at S = 128) are gathered through L2.  Algorithmic bytes: 6 per covered photo pixel (3 read,
// 3 written) plus each face once.
#include "paste_common.h"

struct ComposeRow {
  PasteBox box;
  float sy, sx, iry, irx;
  const float* face;
};

struct ComposePolicy {
  typedef ComposeRow Row;
  const int32_t* boxes;
  const float *inv_ramp, *faces;
  int ld, S;
  Row own;

  __device__ __forceinline__ Row row(int j) const {
    Row q;
    q.box = paste_box(boxes, j);
    const int ih = q.box.y1 - q.box.y0, iw = q.box.x1 - q.box.x0;
    // the correctly rounded float quotient of two small integers, formed as resize_crop_u8_kernel forms its own
    q.sy = ih > 1 ? (float)((double)(S - 1) / (double)(ih - 1)) : 0.f;
    q.sx = iw > 1 ? (float)((double)(S - 1) / (double)(iw - 1)) : 0.f;
    q.iry = inv_ramp[2 * j]; q.irx = inv_ramp[2 * j + 1];
    q.face = faces + (int64_t)j * S * S * ld;
    return q;
  }
  __device__ __forceinline__ bool covers(const Row& q, int r, int c) const { return paste_inside(q.box, r, c); }
  __device__ __forceinline__ void apply(const Row& q, int r, int c, float (&v)[3]) const {
#pragma clang fp contract(off)
    const float fy = (float)(r - q.box.y0) * q.sy, fx = (float)(c - q.box.x0) * q.sx;
    float g[3];
    paste_sample_face(q.face, S, ld, fy, fx, g);
    paste_blend(v, g, paste_ramp(q.box, r, c, q.iry, q.irx));
  }
};

__global__ __launch_bounds__(256) void compose_u8_kernel(uint8_t* __restrict__ photos, const int64_t* __restrict__ offs,
                                                         const int32_t* __restrict__ hw, int n_images,
                                                         const int32_t* __restrict__ boxes, const int32_t* __restrict__ links,
                                                         const float* __restrict__ inv_ramp, const float* __restrict__ faces, int ld,
                                                         int n, int S) {
  PastePhoto ph;
  if (!paste_photo(boxes, offs, hw, n_images, blockIdx.y, ph)) return;
  ComposePolicy pol{boxes, inv_ramp, faces, ld, S};
  pol.own = pol.row(blockIdx.y);
  paste_rows(pol, pol.own.box, ph, photos + ph.off, boxes, links, n);
}

extern "C" int imm_compose_u8(uint8_t* photos, const int64_t* offsets, const int32_t* hw, int n_images, const int32_t* boxes,
                              const int32_t* links, const float* inv_ramp, const float* faces, int ld, int n, int image_size,
                              int max_box_pixels, void* stream) {
  IMM_REQUIRE(photos && offsets && hw && boxes && links && inv_ramp && faces, "compose_u8: null pointer");
  IMM_REQUIRE(n > 0 && n <= 65535 && n_images > 0, "compose_u8: 0 < n <= 65535 rows, n_images > 0 (got %d, %d)", n, n_images);
  IMM_REQUIRE(image_size > 0 && image_size <= 8192 && ld >= 3, "compose_u8: 0 < image_size <= 8192, ld >= 3 (got %d, %d)", image_size, ld);
  IMM_REQUIRE(max_box_pixels > 0, "compose_u8: max_box_pixels > 0 (got %d)", max_box_pixels);
  hipLaunchKernelGGL(compose_u8_kernel, dim3(paste_grid_x(max_box_pixels), n), dim3(256), 0, (hipStream_t)stream, photos, offsets, hw,
                     n_images, boxes, links, inv_ramp, faces, ld, n, image_size);
  IMM_CHECK_LAUNCH("imm_compose_u8");
  return 0;
}
