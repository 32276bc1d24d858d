// unalign.hip — alignment run backwards on gfx950: aligned So x So faces pasted back into the caller's u8 photographs through the
// inverse of their alignment maps (imm_amd/inference.py LandmarkDetector.unalign, imm_amd/generation.py ImageGenerator.repose with a
// template).  The rotated, scaled and sheared counterpart of compose.hip, which pastes into axis-aligned boxes only.  The pixel rule
// is stated once, in include/imm_unalign.h; in short:
//
//   backward map (imm_align_warp_u8, m3 == 3)   s = B (i, j) + t      aligned pixel (i, j) -> source pixel, from coef, geom, S, So
//   forward map  (imm_unalign_maps)             (fi, fj) = B^-1 ((r, c) - t), six f32 per row: m00 m01 m02 m10 m11 m12
//   paste        (imm_unalign_u8)               fi = (m00 r + m01 c) + m02, fj likewise; covered iff both lie in [0, So - 1]
//                                               g  = clip(bilinear(faces[b], fi, fj), 0, 255)      a + (b - a) * t, unfused
//                                               a  = wy wx, wy = min(1, (min(fi, (So - 1) - fi) + 0.5) * inv_ramp)
//                                               photo[r, c] = rint(p + a (g - p)), stored as u8 after EVERY row, in row order
//
// imm_unalign_maps: one thread per row, f64, every operation rounded separately, in the order written below (the numpy restatement
// of the tests follows it line by line), rounded once to f32.  It also writes the row's bounding box in the photo.
// imm_unalign_u8: the paste skeleton of paste_common.h, which states the launch shape, the ownership of a pixel and the addressing
// argument, over the row's bounding box.  "Covers" is the quad test above with a row's own map, so every thread that looks at a pixel
// decides its owner from the same f32 arithmetic; a covered coordinate lies in [0, So - 1] (its taps are clamped all the same).  The
// faces are gathered through L2.  Algorithmic bytes: 6 per covered photo pixel (3 read, 3 written) plus each face once.
#include "paste_common.h"

__global__ __launch_bounds__(64) void unalign_maps_kernel(const float* __restrict__ coef, const float* __restrict__ geom,
                                                          const int32_t* __restrict__ boxes, const int32_t* __restrict__ hw, int n_images,
                                                          int n, int S, int So, float* __restrict__ fwd, int32_t* __restrict__ bbox) {
#pragma clang fp contract(off)   // the stated order, every operation rounded separately: bit-identical to the f64 host restatement
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= n) return;
  const float* cf = coef + (int64_t)b * 6;             // rows 1, q_y, q_x; columns y, x
  const float* g = geom + (int64_t)b * 4;              // y0, x0, sy, sx
  const int img = boxes[5 * b];
  const double dS = (double)S, dSo = (double)So;
  double B[2][2], t[2];
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const double k = (double)g[2 + a] * dS;
    const double c0 = (double)cf[a], c1 = (double)cf[2 + a], c2 = (double)cf[4 + a];
    B[a][0] = (k * c1) / dSo;
    B[a][1] = (k * c2) / dSo;
    t[a] = (double)g[a] + (k * 0.5) * (((c0 + 1.0) - c1) - c2);
  }
  const double det = B[0][0] * B[1][1] - B[0][1] * B[1][0];
  double m[6];
  m[0] = B[1][1] / det;
  m[1] = -B[0][1] / det;
  m[3] = -B[1][0] / det;
  m[4] = B[0][0] / det;
  m[2] = -(m[0] * t[0] + m[1] * t[1]);
  m[5] = -(m[3] * t[0] + m[4] * t[1]);
  bool ok = img >= 0 && img < n_images && det != 0.0;
  float mf[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    mf[i] = (float)m[i];
    ok = ok && isfinite(mf[i]);
  }
  // the four corners of [0, So - 1]^2 through B, t
  const double e = dSo - 1.0;
  double lo[2], hi[2];
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const double p00 = t[a], p10 = B[a][0] * e + t[a], p01 = B[a][1] * e + t[a], p11 = (B[a][0] * e + B[a][1] * e) + t[a];
    lo[a] = fmin(fmin(p00, p10), fmin(p01, p11));
    hi[a] = fmax(fmax(p00, p10), fmax(p01, p11));
    ok = ok && isfinite(p00) && isfinite(p10) && isfinite(p01) && isfinite(p11);
  }
  int32_t bb[4] = {0, 0, 0, 0};
  if (ok) {
    const int sh = hw[2 * img], sw = hw[2 * img + 1];
    // one pixel outwards, half-open, clipped to the photo; the clip comes before the conversion, which therefore never overflows
    const double y0 = fmax(floor(lo[0]) - 1.0, 0.0), y1 = fmin(ceil(hi[0]) + 2.0, (double)sh);
    const double x0 = fmax(floor(lo[1]) - 1.0, 0.0), x1 = fmin(ceil(hi[1]) + 2.0, (double)sw);
    if (y1 > y0 && x1 > x0) { bb[0] = (int32_t)y0; bb[1] = (int32_t)x0; bb[2] = (int32_t)y1; bb[3] = (int32_t)x1; }
  }
  const float qnan = __builtin_nanf("");
#pragma unroll
  for (int i = 0; i < 6; ++i) fwd[(int64_t)b * 6 + i] = ok ? mf[i] : qnan;
#pragma unroll
  for (int i = 0; i < 4; ++i) bbox[(int64_t)b * 4 + i] = bb[i];
}

extern "C" int imm_unalign_maps(const float* coef, const float* geom, const int32_t* boxes, const int32_t* hw, int n_images, int n,
                                int image_size, int out_size, float* fwd, int32_t* bbox, void* stream) {
  IMM_REQUIRE(coef && geom && boxes && hw && fwd && bbox, "unalign_maps: null pointer");
  IMM_REQUIRE(n > 0 && n_images > 0, "unalign_maps: n > 0, n_images > 0 (got %d, %d)", n, n_images);
  IMM_REQUIRE(image_size > 0 && image_size <= 8192 && out_size > 0 && out_size <= 8192,
              "unalign_maps: 0 < image_size <= 8192, 0 < out_size <= 8192 (got %d, %d)", image_size, out_size);
  hipLaunchKernelGGL(unalign_maps_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, coef, geom, boxes, hw, n_images, n,
                     image_size, out_size, fwd, bbox);
  IMM_CHECK_LAUNCH("imm_unalign_maps");
  return 0;
}

struct UnalignRow {
  float m00, m01, m02, m10, m11, m12;
  const float* face;
};

struct UnalignPolicy {
  typedef UnalignRow Row;
  const float *fwd, *faces;
  float inv_ramp, edge;
  int ld, So;
  Row own;

  __device__ __forceinline__ Row row(int j) const {
    const float* m = fwd + (int64_t)j * 6;
    return Row{m[0], m[1], m[2], m[3], m[4], m[5], faces + (int64_t)j * So * So * ld};
  }
  // the aligned-frame coordinate of photo pixel (r, c)
  __device__ __forceinline__ void coord(const Row& q, int r, int c, float& fi, float& fj) const {
#pragma clang fp contract(off)
    const float rf = (float)r, cf = (float)c;
    fi = (q.m00 * rf + q.m01 * cf) + q.m02;
    fj = (q.m10 * rf + q.m11 * cf) + q.m12;
  }
  // the quad test; a NaN map covers nothing
  __device__ __forceinline__ bool covers(const Row& q, int r, int c) const {
    float fi, fj;
    coord(q, r, c, fi, fj);
    return fi >= 0.f && fi <= edge && fj >= 0.f && fj <= edge;
  }
  __device__ __forceinline__ void apply(const Row& q, int r, int c, float (&v)[3]) const {
#pragma clang fp contract(off)
    float fi, fj, g[3];
    coord(q, r, c, fi, fj);
    paste_sample_face(q.face, So, ld, fi, fj, g);
    const float wy = fminf(1.f, (fminf(fi, edge - fi) + 0.5f) * inv_ramp);
    const float wx = fminf(1.f, (fminf(fj, edge - fj) + 0.5f) * inv_ramp);
    paste_blend(v, g, wy * wx);
  }
};

__global__ __launch_bounds__(256) void unalign_u8_kernel(uint8_t* __restrict__ photos, const int64_t* __restrict__ offs,
                                                         const int32_t* __restrict__ hw, int n_images,
                                                         const int32_t* __restrict__ boxes, const int32_t* __restrict__ links,
                                                         const float* __restrict__ fwd, const int32_t* __restrict__ bbox, float inv_ramp,
                                                         const float* __restrict__ faces, int ld, int n, int So) {
  const int b = blockIdx.y;
  PastePhoto ph;
  if (!paste_photo(boxes, offs, hw, n_images, b, ph)) return;
  UnalignPolicy pol{fwd, faces, inv_ramp, (float)(So - 1), ld, So};
  pol.own = pol.row(b);
  // the row's bounding box, which paste_rows clips to the photo once more
  paste_rows(pol, PasteBox{bbox[4 * b], bbox[4 * b + 1], bbox[4 * b + 2], bbox[4 * b + 3]}, ph, photos + ph.off, boxes, links, n);
}

extern "C" int imm_unalign_u8(uint8_t* photos, const int64_t* offsets, const int32_t* hw, int n_images, const int32_t* boxes,
                              const int32_t* links, const float* fwd, const int32_t* bbox, float inv_ramp, const float* faces, int ld,
                              int n, int out_size, int max_pixels, void* stream) {
  IMM_REQUIRE(photos && offsets && hw && boxes && links && fwd && bbox && faces, "unalign_u8: null pointer");
  IMM_REQUIRE(n > 0 && n <= 65535 && n_images > 0, "unalign_u8: 0 < n <= 65535 rows, n_images > 0 (got %d, %d)", n, n_images);
  IMM_REQUIRE(out_size > 0 && out_size <= 8192 && ld >= 3, "unalign_u8: 0 < out_size <= 8192, ld >= 3 (got %d, %d)", out_size, ld);
  IMM_REQUIRE(inv_ramp > 0.f && inv_ramp <= 3.0e38f, "unalign_u8: inv_ramp must be positive and finite (got %g)", (double)inv_ramp);
  IMM_REQUIRE(max_pixels > 0, "unalign_u8: max_pixels > 0 (got %d)", max_pixels);
  hipLaunchKernelGGL(unalign_u8_kernel, dim3(paste_grid_x(max_pixels), n), dim3(256), 0, (hipStream_t)stream, photos, offsets, hw, n_images,
                     boxes, links, fwd, bbox, inv_ramp, faces, ld, n, out_size);
  IMM_CHECK_LAUNCH("imm_unalign_u8");
  return 0;
}
