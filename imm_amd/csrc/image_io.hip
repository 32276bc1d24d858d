// image_io.hip — ingest of decoded images on gfx950: the resize / central-crop / to-float stage of the reference's
// input pipelines (imm/datasets/celeba_dataset.py:136-174: tf.to_float -> tf.image.resize_images(BILINEAR,
// align_corners=True) to round(size/0.8) -> central crop; imm/datasets/aflw_dataset.py:81-114: resize straight to size).
// The reference runs this per image on CPU threads of tf.data; here the JPEG decoder's u8 HWC outputs (different sizes
// per image) are packed back to back into one staging buffer, copied to HBM once, and ONE launch produces the f32 NHWC
// batch — only the pixels that survive the crop are ever computed, and they can be written at a channel offset of a wider
// buffer (the mask||image stack the thin-plate-spline warp reads, imm/datasets/tps_dataset.py:79).
//
//   scale = (in - 1) / (resize - 1)      (TF1 align_corners; in / resize when resize == 1)
//   s = (crop0 + o) * scale;  lo = floor(s);  hi = min(ceil(s), in - 1);  t = s - lo
//   out = top + (bottom - top) * ty,  top = tl + (tr - tl) * tx,  bottom = bl + (br - bl) * tx     (float32, unfused)
// HBM-bound and tiny: B * (in_h*in_w*c bytes read at most) + B*oh*ow*c*4 bytes written.
//
// Box-crop mode (boxes != NULL): output row b is the half-open box boxes[b] = (image, y0, x0, y1, x1) cut from that image with
// zeros where it leaves the image (ImagePairDataset._crop_to_box(pad=True)), then resized and cropped as above.  The box takes the
// place of the image (in = the box's side) and a tap reads source pixel (y0 + lo, x0 + lo') or 0: the same f32 operations in the
// same order, so the result is bit-exact against that host composition.  Several rows may name one image (several faces).
#include "common.h"

template <bool BOX>
__global__ __launch_bounds__(256) void resize_crop_u8_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ offs,
                                                             const int32_t* __restrict__ hw, const int32_t* __restrict__ boxes,
                                                             int c, int rh, int rw, int y0, int x0, int oh, int ow,
                                                             float* __restrict__ dst, int ld_dst) {
#pragma clang fp contract(off)   // a fused a*s - floor(a*s) would differ from the separately rounded host evaluation
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= oh * ow) return;
  const int b = blockIdx.y;
  // BOX: the image of row b and the box that stands in for it (ih x iw = the box's side; by, bx = its corner in that image)
  const int img = BOX ? boxes[5 * b] : b;
  const int sh = hw[2 * img], sw = hw[2 * img + 1];
  const int by = BOX ? boxes[5 * b + 1] : 0, bx = BOX ? boxes[5 * b + 2] : 0;
  const int ih = BOX ? boxes[5 * b + 3] - by : sh, iw = BOX ? boxes[5 * b + 4] - bx : sw;
  const uint8_t* s = src + offs[img];
  const int oy = p / ow, ox = p - oy * ow;
  // every operation rounded separately (no fma contraction): bit-identical to a float32 host evaluation in the same order
  // (oracle/image_oracle.py)
  // the scale is the correctly rounded float quotient of two small integers: formed in double and rounded once (the
  // operands are < 2^24, so the double quotient can never sit within a double ulp of a float rounding boundary); the
  // device's float '/' may be the approximate-reciprocal form
  const float sy = rh > 1 ? (float)((double)(ih - 1) / (double)(rh - 1)) : (float)((double)ih / (double)rh);
  const float sx = rw > 1 ? (float)((double)(iw - 1) / (double)(rw - 1)) : (float)((double)iw / (double)rw);
  const float fy = (float)(y0 + oy) * sy, fx = (float)(x0 + ox) * sx;
  const int yl = (int)floorf(fy), xl = (int)floorf(fx);
  const int yh = min((int)ceilf(fy), ih - 1), xh = min((int)ceilf(fx), iw - 1);
  const float ty = fy - (float)yl, tx = fx - (float)xl;
  float* d = dst + ((int64_t)b * oh * ow + p) * ld_dst;
  if constexpr (BOX) {
    // the four taps in source pixels; a tap outside the image reads the zero padding
    const int r0 = by + yl, r1 = by + yh, c0 = bx + xl, c1 = bx + xh;
    const bool v0 = r0 >= 0 && r0 < sh, v1 = r1 >= 0 && r1 < sh, u0 = c0 >= 0 && c0 < sw, u1 = c1 >= 0 && c1 < sw;
    const uint8_t* q0 = s + (int64_t)(v0 ? r0 : 0) * sw * c;
    const uint8_t* q1 = s + (int64_t)(v1 ? r1 : 0) * sw * c;
    for (int ch = 0; ch < c; ++ch) {
      const float tl = (v0 && u0) ? (float)q0[c0 * c + ch] : 0.f, tr = (v0 && u1) ? (float)q0[c1 * c + ch] : 0.f;
      const float bl = (v1 && u0) ? (float)q1[c0 * c + ch] : 0.f, br = (v1 && u1) ? (float)q1[c1 * c + ch] : 0.f;
      const float top = tl + (tr - tl) * tx;
      const float bot = bl + (br - bl) * tx;
      d[ch] = top + (bot - top) * ty;
    }
  } else {
    const uint8_t* r0 = s + (int64_t)yl * iw * c;
    const uint8_t* r1 = s + (int64_t)yh * iw * c;
    for (int ch = 0; ch < c; ++ch) {
      const float tl = (float)r0[xl * c + ch], tr = (float)r0[xh * c + ch];
      const float bl = (float)r1[xl * c + ch], br = (float)r1[xh * c + ch];
      const float top = tl + (tr - tl) * tx;
      const float bot = bl + (br - bl) * tx;
      d[ch] = top + (bot - top) * ty;
    }
  }
}

extern "C" int imm_resize_crop_u8(const uint8_t* src, const int64_t* offsets, const int32_t* hw, const int32_t* boxes, int batch,
                                  int c, int resize_h, int resize_w, int crop_y0, int crop_x0, int out_h, int out_w, float* dst,
                                  int ld_dst, void* stream) {
  IMM_REQUIRE(src && offsets && hw && dst, "resize_crop_u8: null pointer");
  IMM_REQUIRE(batch > 0 && c >= 1 && c <= 4 && ld_dst >= c, "resize_crop_u8: batch > 0, 1 <= c <= 4, ld_dst >= c");
  IMM_REQUIRE(resize_h > 0 && resize_w > 0 && out_h > 0 && out_w > 0, "resize_crop_u8: sizes");
  IMM_REQUIRE(crop_y0 >= 0 && crop_x0 >= 0 && crop_y0 + out_h <= resize_h && crop_x0 + out_w <= resize_w,
              "resize_crop_u8: crop window [%d+%d, %d+%d] outside the resized image %dx%d", crop_y0, out_h, crop_x0, out_w,
              resize_h, resize_w);
  IMM_REQUIRE(batch <= 65535, "resize_crop_u8: batch %d > 65535", batch);
  const dim3 grid((out_h * out_w + 255) / 256, batch);
  // the box rows are device data: their image indices and y1 > y0, x1 > x0 are the caller's to check (imm_amd.keypoints.check_boxes)
  if (boxes != nullptr)
    hipLaunchKernelGGL(resize_crop_u8_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, src, offsets, hw, boxes, c, resize_h,
                       resize_w, crop_y0, crop_x0, out_h, out_w, dst, ld_dst);
  else
    hipLaunchKernelGGL(resize_crop_u8_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, src, offsets, hw, boxes, c, resize_h,
                       resize_w, crop_y0, crop_x0, out_h, out_w, dst, ld_dst);
  IMM_CHECK_LAUNCH("imm_resize_crop_u8");
  return 0;
}
