// annotate.hip — landmarks, boxes, hulls and numbers drawn into u8 photos on gfx950 (imm_amd/inference.py LandmarkDetector.annotate and
// annotate_clip, imm_amd/annotation.py).  The rule is stated once, in include/imm_annotate.h; in short:
//
//   imm_annotate_points   per row the landmarks from the frame of the box to photo pixels, in f64, the convention of imm_hull.h
//   imm_annotate_u8       per photo pixel of a row's extent (its box grown by pad): the box frame in the colour of the row's status,
//                         the outline of the grown hull from imm_hull_fit's lines, the trail discs of earlier frames, the markers of
//                         the current one and a decimal label, each a blend of imm_compose_u8 with a rint after it, in that order
//
// Points: one workgroup of 64 lanes per row, a few microseconds of latency-bound work; plain C++, every operation rounded separately.
// Paste: the paste skeleton of paste_common.h, which states the launch shape, the ownership of a pixel and the addressing argument; the
// span of a block is its row's extent.  The block's own row keeps its G * K marks (at most 10 240 bytes) and its 3 K lines (960 bytes)
// in static LDS, read as broadcasts: every lane of a wave reads the same mark.  Rows met on a link walk read theirs through L2.
// A mark is compared against the pixel before anything else is computed (|dy|, |dx| <= R + 2), so the loop over G * K marks costs two
// subtractions and two comparisons a mark where nothing is drawn, which is nearly everywhere.  No division, square root or
// transcendental function runs per pixel in f32; the label's integer divisions run only inside its small rectangle.  The kernel moves
// 6 bytes a pixel.  status reaches the palette through an index clamped to [0, P); the shape byte and a label's digit select among
// constants; nothing else a buffer holds reaches an address.
#include "paste_common.h"

#include <limits.h>

// seven rows of five bits per digit (bit 4 is the left column): include/imm_annotate.h prints the same table
__constant__ uint8_t annot_font[10][7] = {
    {0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E}, {0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E}, {0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F},
    {0x1F, 0x02, 0x04, 0x02, 0x01, 0x11, 0x0E}, {0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02}, {0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E},
    {0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E}, {0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08}, {0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E},
    {0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C}};

__device__ __forceinline__ float annot_point(float mu, double origin, double side) {
#pragma clang fp contract(off)
  if (!__builtin_isfinite(mu)) return mu;                          // stored as it is
  const double half = 0.5 * side;
  const double a = (double)mu + 1.0;
  const double m = a * half;
  return (float)(origin + m);
}

__global__ __launch_bounds__(64) void annotate_points_kernel(const float* __restrict__ mu, const int32_t* __restrict__ boxes, int K,
                                                             float* __restrict__ points) {
  const int b = blockIdx.x;
  const double y0 = (double)boxes[5 * b + 1], x0 = (double)boxes[5 * b + 2], y1 = (double)boxes[5 * b + 3], x1 = (double)boxes[5 * b + 4];
  const double H = y1 - y0, W = x1 - x0;                           // exact: the difference of two int32 in f64
  const int64_t base = (int64_t)b * K * 2;
  for (int i = threadIdx.x; i < 2 * K; i += 64) points[base + i] = (i & 1) ? annot_point(mu[base + i], x0, W) : annot_point(mu[base + i], y0, H);
}

struct AnnotRow {
  PasteBox box, ext;          // the box, and the box grown by pad (each bound saturated)
  bool active, lost;          // H > 0 and W > 0; bit 0 of its status
  int label, nd;              // its label and the number of its digits; nd == 0: no label is drawn
  float col[3];               // its colour: the palette entry of its status
  const float* m;             // its marks: group g at m + g * gs, [K][2]
  int64_t gs;
  const float* e;             // its lines [K][3]
};

__device__ __forceinline__ int annot_sat(int64_t v) { return (int)(v < INT_MIN ? INT_MIN : v > INT_MAX ? INT_MAX : v); }

__device__ __forceinline__ float annot_clamp(float x) { return fminf(fmaxf(x, 0.f), 1.f); }

// the inside-ness of a marker in pixels, include/imm_annotate.h's table; a shape byte past the table: far outside
__device__ __forceinline__ float annot_shape(int shape, float dy, float dx, float ay, float ax, float R, float inv2R, float h) {
#pragma clang fp contract(off)
  switch (shape) {
    case 0: return fminf(dy + R, ((R - dy) * 0.5f - ax) * 0.8944272f);
    case 1: return (R * R - (dy * dy + dx * dx)) * inv2R;
    case 2: return R - fmaxf(ay, ax);
    case 3: return (R - (ay + ax)) * 0.70710677f;
    case 4: {
      const float ny = -dy;
      return fminf(ny + R, ((R - ny) * 0.5f - ax) * 0.8944272f);
    }
    case 5: return fminf(h - fminf(fabsf(dy - dx), fabsf(dy + dx)) * 0.70710677f, R - fmaxf(ay, ax));
    case 6: return fminf(h - fminf(ay, ax), R - fmaxf(ay, ax));
    default: return -__builtin_huge_valf();
  }
}

struct AnnotPolicy {
  typedef AnnotRow Row;
  const int32_t* boxes;
  const float *marks, *group_style;
  const uint8_t* mark_style;
  const float* edges;
  const int32_t* status;
  const uint8_t* palette;
  const int32_t* labels;
  int P, bits, thickness, pad, scale, K, G, n;
  Row own;

  // row j with its marks at m (group stride gs) and its lines at e
  __device__ __forceinline__ Row row(int j, const float* m, int64_t gs, const float* e) const {
    Row q;
    q.box = paste_box(boxes, j);
    const int64_t H = (int64_t)q.box.y1 - q.box.y0, W = (int64_t)q.box.x1 - q.box.x0;
    q.active = H > 0 && W > 0;
    q.ext = PasteBox{annot_sat((int64_t)q.box.y0 - pad), annot_sat((int64_t)q.box.x0 - pad), annot_sat((int64_t)q.box.y1 + pad),
                     annot_sat((int64_t)q.box.x1 + pad)};
    const int s = status ? status[j] : 0;
    q.lost = (s & 1) != 0;
    const int ci = s == 0 ? 0 : min(__ffs(s), P - 1);              // __ffs: 1 + the index of the lowest set bit; 0 <= ci < P
    q.col[0] = (float)palette[3 * ci]; q.col[1] = (float)palette[3 * ci + 1]; q.col[2] = (float)palette[3 * ci + 2];
    q.label = (bits & IMM_ANNOTATE_LABEL) ? labels[j] : -1;
    q.nd = q.label < 0 || q.label > 9999 ? 0 : q.label >= 1000 ? 4 : q.label >= 100 ? 3 : q.label >= 10 ? 2 : 1;
    q.m = m; q.gs = gs; q.e = e;
    return q;
  }
  __device__ __forceinline__ Row row(int j) const {
    return row(j, (bits & IMM_ANNOTATE_POINTS) ? marks + (int64_t)j * K * 2 : nullptr, (int64_t)n * K * 2,
               (bits & IMM_ANNOTATE_HULL) ? edges + (int64_t)j * K * 3 : nullptr);
  }
  __device__ __forceinline__ bool covers(const Row& q, int r, int c) const { return q.active && paste_inside(q.ext, r, c); }

  __device__ __forceinline__ void apply(const Row& q, int r, int c, float (&v)[3]) const {
#pragma clang fp contract(off)
    const bool in_box = paste_inside(q.box, r, c);
    // inside the box every difference below lies in [0, 2^32): 64 bits hold it
    const int64_t ry = (int64_t)r - q.box.y0, cx = (int64_t)c - q.box.x0;
    if ((bits & IMM_ANNOTATE_BOX) && in_box) {
      const int64_t fy = (int64_t)q.box.y1 - 1 - r, fx = (int64_t)q.box.x1 - 1 - c;
      const int64_t by = ry < fy ? ry : fy, bx = cx < fx ? cx : fx;
      if ((by < bx ? by : bx) < thickness) paste_blend(v, q.col, 1.f);
    }
    if (!q.lost) {
      if (bits & IMM_ANNOTATE_HULL) {
        const float rr = (float)ry, cc = (float)cx;
        float dist = __builtin_huge_valf();
        for (int k = 0; k < K; ++k) {
          const float a = q.e[3 * k] * rr, b = q.e[3 * k + 1] * cc;
          const float s = (a + b) + q.e[3 * k + 2];
          dist = fminf(dist, s);
        }
        const float half = 0.5f * (float)thickness + 0.5f;
        const float a = annot_clamp(half - fabsf(dist));
        if (a > 0.f) paste_blend(v, q.col, a);
      }
      if (bits & IMM_ANNOTATE_POINTS) {
        const float fr = (float)r, fc = (float)c;
        const float white[3] = {255.f, 255.f, 255.f};
        for (int g = 0; g < G; ++g) {
          const float R = group_style[4 * g], inv2R = group_style[4 * g + 1], h = group_style[4 * g + 2], alpha = group_style[4 * g + 3];
          const float lim = R + 2.f;
          const float* m = q.m + g * q.gs;
          const bool trail = g < G - 1;
          for (int k = 0; k < K; ++k) {
            const float dy = fr - m[2 * k], dx = fc - m[2 * k + 1];
            const float ay = fabsf(dy), ax = fabsf(dx);
            if (!(ay <= lim) || !(ax <= lim)) continue;            // a NaN mark fails here
            const uint8_t* st = mark_style + 4 * k;
            const float col[3] = {(float)st[0], (float)st[1], (float)st[2]};
            const float s = annot_shape(trail ? 1 : (int)st[3], dy, dx, ay, ax, R, inv2R, h);
            if (!trail) {
              const float aw = alpha * annot_clamp(s + 1.5f);
              if (aw > 0.f) paste_blend(v, white, aw);
            }
            const float ac = alpha * annot_clamp(s + 0.5f);
            if (ac > 0.f) paste_blend(v, col, ac);
          }
        }
      }
    }
    if (q.nd > 0 && in_box) {
      const int64_t u = ry - thickness, t = cx - thickness;
      if (u >= 0 && u < 9 * scale && t >= 0 && t < (6 * q.nd + 1) * scale) {
        const int frow = (int)(u / scale) - 1, tc = (int)(t / scale) - 1;      // tc <= 6 nd - 1
        bool on = false;
        if (frow >= 0 && frow < 7 && tc >= 0) {
          const int di = tc / 6, fcol = tc - 6 * di;                           // di <= nd - 1
          if (fcol < 5) {
            int p10 = 1;
            for (int i = q.nd - 1 - di; i > 0; --i) p10 *= 10;
            const int digit = (q.label / p10) % 10;                            // 0 .. 9: the label is not negative
            on = ((annot_font[digit][frow] >> (4 - fcol)) & 1) != 0;
          }
        }
        // one blend with a select per channel (as an if / else of two blends the compiled link walk lost one channel's select)
        const float g[3] = {on ? 255.f : q.col[0], on ? 255.f : q.col[1], on ? 255.f : q.col[2]};
        paste_blend(v, g, 1.f);
      }
    }
  }
};

__global__ __launch_bounds__(256) void annotate_u8_kernel(uint8_t* __restrict__ dst, const int64_t* __restrict__ offs,
                                                          const int32_t* __restrict__ hw, int n_images, const int32_t* __restrict__ boxes,
                                                          const int32_t* __restrict__ links, const float* __restrict__ marks,
                                                          const float* __restrict__ group_style, const uint8_t* __restrict__ mark_style,
                                                          const float* __restrict__ edges, const int32_t* __restrict__ status,
                                                          const uint8_t* __restrict__ palette, int P, const int32_t* __restrict__ labels,
                                                          int bits, int thickness, int pad, int scale, int K, int G, int n) {
  __shared__ float m_s[IMM_ANNOTATE_MAX_GROUPS * SPLINE_MAX_M * 2];
  __shared__ float e_s[3 * SPLINE_MAX_M];
  const int b = blockIdx.y;
  PastePhoto ph;
  if (!paste_photo(boxes, offs, hw, n_images, b, ph)) return;      // uniform over the block: no barrier is skipped by part of it
  AnnotPolicy pol{boxes, marks, group_style, mark_style, edges, status, palette, labels, P, bits, thickness, pad, scale, K, G, n};
  pol.own = pol.row(b, m_s, 2 * K, e_s);
  if (!pol.own.active) return;                                     // uniform as well
  if (bits & IMM_ANNOTATE_POINTS) {
    for (int i = threadIdx.x; i < G * 2 * K; i += 256) {           // i < 2560: inside m_s
      const int g = i / (2 * K);
      m_s[i] = marks[((int64_t)g * n + b) * 2 * K + (i - g * 2 * K)];
    }
  }
  if (bits & IMM_ANNOTATE_HULL) {
    for (int i = threadIdx.x; i < 3 * K; i += 256) e_s[i] = edges[(int64_t)b * 3 * K + i];
  }
  __syncthreads();
  paste_rows(pol, pol.own.ext, ph, dst + ph.off, boxes, links, n);
}

extern "C" int imm_annotate_points(const float* mu, const int32_t* boxes, int K, int n, float* points, void* stream) {
  IMM_REQUIRE(mu && boxes && points, "annotate_points: null pointer");
  IMM_REQUIRE(points != mu, "annotate_points: points must not be mu");
  IMM_REQUIRE(n > 0 && n <= 65535 && K >= 1 && K <= SPLINE_MAX_M, "annotate_points: 0 < n <= 65535 rows, 1 <= K <= %d (got %d, %d)",
              SPLINE_MAX_M, n, K);
  hipLaunchKernelGGL(annotate_points_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, mu, boxes, K, points);
  IMM_CHECK_LAUNCH("imm_annotate_points");
  return 0;
}

extern "C" int imm_annotate_u8(uint8_t* dst, const int64_t* offsets, const int32_t* hw, int n_images, const int32_t* boxes,
                               const int32_t* links, const float* marks, const float* group_style, const uint8_t* mark_style,
                               const float* edges, const int32_t* status, const uint8_t* palette, int P, const int32_t* labels, int draw_bits,
                               int thickness, int pad, int label_scale, int K, int G, int n, int max_box_pixels, void* stream) {
  IMM_REQUIRE(dst && offsets && hw && boxes && links && palette, "annotate_u8: null pointer");
  IMM_REQUIRE(n > 0 && n <= 65535 && n_images > 0, "annotate_u8: 0 < n <= 65535 rows, n_images > 0 (got %d, %d)", n, n_images);
  IMM_REQUIRE(draw_bits >= 0 && draw_bits < 16, "annotate_u8: draw_bits is a sum of 1 (points), 2 (box), 4 (hull), 8 (label) (got %d)", draw_bits);
  IMM_REQUIRE(thickness >= 1 && thickness <= 16, "annotate_u8: 1 <= thickness <= 16 (got %d)", thickness);
  IMM_REQUIRE(pad >= 0 && pad <= IMM_ANNOTATE_MAX_PAD, "annotate_u8: 0 <= pad <= %d (got %d)", IMM_ANNOTATE_MAX_PAD, pad);
  IMM_REQUIRE(label_scale >= 1 && label_scale <= 8, "annotate_u8: 1 <= label_scale <= 8 (got %d)", label_scale);
  IMM_REQUIRE(K >= 1 && K <= SPLINE_MAX_M, "annotate_u8: 1 <= K <= %d landmarks (got %d)", SPLINE_MAX_M, K);
  IMM_REQUIRE(G >= 1 && G <= IMM_ANNOTATE_MAX_GROUPS, "annotate_u8: 1 <= G <= %d groups (got %d)", IMM_ANNOTATE_MAX_GROUPS, G);
  IMM_REQUIRE(P >= 1 && P <= 32, "annotate_u8: 1 <= P <= 32 palette entries (got %d)", P);
  IMM_REQUIRE(max_box_pixels > 0, "annotate_u8: max_box_pixels > 0 (got %d)", max_box_pixels);
  if (draw_bits & IMM_ANNOTATE_POINTS)
    IMM_REQUIRE(marks && group_style && mark_style, "annotate_u8: points are drawn from marks, group_style and mark_style");
  if (draw_bits & IMM_ANNOTATE_HULL) IMM_REQUIRE(edges != nullptr, "annotate_u8: the hull is drawn from edges");
  if (draw_bits & IMM_ANNOTATE_LABEL) IMM_REQUIRE(labels != nullptr, "annotate_u8: the label is drawn from labels");
  IMM_REQUIRE((const void*)marks != (const void*)dst && (const void*)palette != (const void*)dst && (const void*)mark_style != (const void*)dst,
              "annotate_u8: marks, mark_style and palette are read only and must not be dst");
  hipLaunchKernelGGL(annotate_u8_kernel, dim3(paste_grid_x(max_box_pixels), n), dim3(256), 0, (hipStream_t)stream, dst, offsets, hw, n_images,
                     boxes, links, marks, group_style, mark_style, edges, status, palette, P, labels, draw_bits, thickness, pad, label_scale, K,
                     G, n);
  IMM_CHECK_LAUNCH("imm_annotate_u8");
  return 0;
}
