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
// One thread = one photo pixel (its three bytes) of one row's box, clipped to the photo; blockIdx.y is the row.  Overlapping boxes of
// one photo are resolved without atomics: the thread of (row b, pixel) returns if an earlier row of this launch covers the pixel in the
// same photo (links[b][0]: the previous row of that photo), otherwise it alone owns the pixel: it reads it once, walks b and the later
// rows of the photo (links[b][1]) that cover it, keeps the running value in a register with the per-row rint, and writes it once.  Every
// pixel of the launch therefore has exactly one writer and no reader but that writer.
// Lanes of a wave take consecutive pixels of a photo row: 192 contiguous bytes read and written per wave.  Photo rows start at any byte
// (3 * width is odd for odd widths) and a box edge can fall inside any dword, whose other bytes belong to no box or to another thread,
// so the accesses are byte-wide; the faces (f32, S * S * ld * 4 bytes per row, 256 KB at S = 128) are gathered through L2.
// Algorithmic bytes: 6 per covered photo pixel (3 read, 3 written) plus each face once.
#include "common.h"

struct ComposeRow {
  int y0, x0, y1, x1;
  float sy, sx;
};

__device__ __forceinline__ ComposeRow compose_row(const int32_t* __restrict__ boxes, int j, int S) {
  ComposeRow q;
  q.y0 = boxes[5 * j + 1]; q.x0 = boxes[5 * j + 2]; q.y1 = boxes[5 * j + 3]; q.x1 = boxes[5 * j + 4];
  const int ih = q.y1 - q.y0, iw = q.x1 - q.x0;
  // the correctly rounded float quotient of two small integers, formed as resize_crop_u8_kernel forms its own
  q.sy = ih > 1 ? (float)((double)(S - 1) / (double)(ih - 1)) : 0.f;
  q.sx = iw > 1 ? (float)((double)(S - 1) / (double)(iw - 1)) : 0.f;
  return q;
}

__global__ __launch_bounds__(256) void compose_u8_kernel(uint8_t* __restrict__ photos, const int64_t* __restrict__ offs,
                                                         const int32_t* __restrict__ hw, int n_images,
                                                         const int32_t* __restrict__ boxes, const int32_t* __restrict__ links,
                                                         const float* __restrict__ inv_ramp, const float* __restrict__ faces, int ld,
                                                         int n, int S) {
#pragma clang fp contract(off)   // every operation rounded separately: bit-identical to the f32 host restatement in the same order
  const int b = blockIdx.y;
  const int img = boxes[5 * b];
  if (img < 0 || img >= n_images) return;
  const int sh = hw[2 * img], sw = hw[2 * img + 1];
  const ComposeRow own = compose_row(boxes, b, S);
  // the part of box b inside the photo
  const int cy0 = max(own.y0, 0), cy1 = min(own.y1, sh), cx0 = max(own.x0, 0), cx1 = min(own.x1, sw);
  const int cw = cx1 - cx0, chh = cy1 - cy0;
  if (cw <= 0 || chh <= 0) return;
  const int64_t area = (int64_t)cw * chh;
  uint8_t* photo = photos + offs[img];
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
    float v0 = (float)px[0], v1 = (float)px[1], v2 = (float)px[2];
    ComposeRow q = own;
    for (int j = b;;) {
      if (r >= q.y0 && r < q.y1 && c >= q.x0 && c < q.x1) {
        const float fy = (float)(r - q.y0) * q.sy, fx = (float)(c - q.x0) * q.sx;
        const int yl = min(max((int)floorf(fy), 0), S - 1), xl = min(max((int)floorf(fx), 0), S - 1);
        const int yh = min(yl + 1, S - 1), xh = min(xl + 1, S - 1);
        const float ty = fy - (float)yl, tx = fx - (float)xl;
        const float wy = fminf(1.f, ((float)min(r - q.y0, q.y1 - 1 - r) + 0.5f) * inv_ramp[2 * j]);
        const float wx = fminf(1.f, ((float)min(c - q.x0, q.x1 - 1 - c) + 0.5f) * inv_ramp[2 * j + 1]);
        const float a = wy * wx;
        const float* f = faces + (int64_t)j * S * S * ld;
        const float* tlp = f + ((int64_t)yl * S + xl) * ld;
        const float* trp = f + ((int64_t)yl * S + xh) * ld;
        const float* blp = f + ((int64_t)yh * S + xl) * ld;
        const float* brp = f + ((int64_t)yh * S + xh) * ld;
        float v[3] = {v0, v1, v2};
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const float tl = tlp[ch], tr = trp[ch], bl = blp[ch], br = brp[ch];
          const float top = tl + (tr - tl) * tx;
          const float bot = bl + (br - bl) * tx;
          float g = top + (bot - top) * ty;
          g = fminf(fmaxf(g, 0.f), 255.f);
          const float d = g - v[ch];
          const float m = a * d;
          // in contract the sum is already in [0, 255]; the clamp keeps weights outside [0, 1] from wrapping the byte
          v[ch] = fminf(fmaxf(rintf(v[ch] + m), 0.f), 255.f);
        }
        v0 = v[0]; v1 = v[1]; v2 = v[2];
      }
      const int nx = links[2 * j + 1];
      if (nx <= j || nx >= n) break;
      j = nx;
      if (boxes[5 * j] != img) { q.y0 = q.y1 = 0; q.x0 = q.x1 = 0; continue; }      // a foreign row in the chain covers nothing
      q = compose_row(boxes, j, S);
    }
    px[0] = (uint8_t)v0; px[1] = (uint8_t)v1; px[2] = (uint8_t)v2;
  }
}

extern "C" int imm_compose_u8(uint8_t* photos, const int64_t* offsets, const int32_t* hw, int n_images, const int32_t* boxes,
                              const int32_t* links, const float* inv_ramp, const float* faces, int ld, int n, int image_size,
                              int max_box_pixels, void* stream) {
  IMM_REQUIRE(photos && offsets && hw && boxes && links && inv_ramp && faces, "compose_u8: null pointer");
  IMM_REQUIRE(n > 0 && n <= 65535 && n_images > 0, "compose_u8: 0 < n <= 65535 rows, n_images > 0 (got %d, %d)", n, n_images);
  IMM_REQUIRE(image_size > 0 && image_size <= 8192 && ld >= 3, "compose_u8: 0 < image_size <= 8192, ld >= 3 (got %d, %d)", image_size, ld);
  IMM_REQUIRE(max_box_pixels > 0, "compose_u8: max_box_pixels > 0 (got %d)", max_box_pixels);
  // the grid is sized by the caller's largest box; a row with more pixels than that is still covered (grid-stride loop)
  const int blocks = (int)((((int64_t)max_box_pixels + 255) / 256 < 65536) ? ((int64_t)max_box_pixels + 255) / 256 : 65536);
  hipLaunchKernelGGL(compose_u8_kernel, dim3(blocks, n), dim3(256), 0, (hipStream_t)stream, photos, offsets, hw, n_images, boxes, links,
                     inv_ramp, faces, ld, n, image_size);
  IMM_CHECK_LAUNCH("imm_compose_u8");
  return 0;
}
