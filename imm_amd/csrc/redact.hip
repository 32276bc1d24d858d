// redact.hip — faces pixelated or smoothed inside their u8 photos on gfx950 (imm_amd/inference.py LandmarkDetector.redact and
// redact_clip, imm_amd/redaction.py).  The rule is stated once, in include/imm_redact.h; in short:
//
//   imm_redact_cells_u8   per row the box is cut into gy x gx square cells of side cell = ceil(max(H, W) / blocks); every cell takes the
//                         mean, rounded half up in integers, of the ORIGINAL bytes it covers inside the photo
//   imm_redact_u8         per photo pixel of a row's box: the cell's mean (pixelate) or the bilinear sample of the grid of means
//                         (smooth), blended over the canvas with imm_compose_u8's ramp, rounding, row order and links; with the mask
//                         the ramp times the hull weight of imm_hull.h, and a row whose hull is FLAGGED takes the weight 1 over its
//                         whole box (redaction fails closed)
//
// Cells: one wave per cell, four cells per workgroup, grid (ceil(blocks^2 / 4), n).  The lanes stride over the pixels of the cell
// clipped to the photo, row-major (a cell row is 3 * cell contiguous bytes), so a box of side 100 000 around a small photo costs what
// the photo costs.  Integer sums in 64 bits, reduced over the wave by __shfl_xor: any order gives the same bits, one writer per cell,
// no atomics.  The waves of cell indices past gy * gx, and every wave of a row that is not active, write zeros: the whole buffer is
// written.  Byte-wide accesses, as in the other photo kernels (a cell row starts at any byte).
// Paste: the paste skeleton of paste_common.h, which states the launch shape, the ownership of a pixel and the addressing argument.
// The block's own row keeps its grid of means (gy * gx * 3 <= 12 288 bytes) and, with the mask, its 3 K lines and its inv_soft in
// static LDS; the lanes of a wave read neighbouring grid bytes, mostly the same ones.  Rows met on a link walk read theirs through L2.
// A grid index is formed from (r - y0) / cell < gy and (c - x0) / cell < gx of a pixel inside the box, and the smooth mode's taps are
// clamped to the grid: cells, edges, inv_soft and hull_flags hold values only and reach no address.  No logarithm and no spline: the
// kernel moves 6 bytes a pixel and is bound by that.
#include "paste_common.h"

struct RedactGrid {
  uint32_t cell;              // 0: the row is not active (an empty or inverted box)
  int gy, gx;
};

// the cell side and the grid of a box, in 64 bits: cell = max(1, ceil(max(H, W) / blocks)), gy = ceil(H / cell), gx = ceil(W / cell).
// max(H, W) < 2^32, so cell fits 32 unsigned bits and gy, gx <= blocks.
__device__ __forceinline__ RedactGrid redact_grid(const PasteBox& box, int blocks) {
  const int64_t H = (int64_t)box.y1 - box.y0, W = (int64_t)box.x1 - box.x0;
  if (H <= 0 || W <= 0) return RedactGrid{0u, 0, 0};
  const int64_t m = H > W ? H : W;
  int64_t cell = (m + blocks - 1) / blocks;
  if (cell < 1) cell = 1;
  return RedactGrid{(uint32_t)cell, (int)((H + cell - 1) / cell), (int)((W + cell - 1) / cell)};
}

__global__ __launch_bounds__(256) void redact_cells_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ offs,
                                                           const int32_t* __restrict__ hw, int n_images,
                                                           const int32_t* __restrict__ boxes, int blocks, uint8_t* __restrict__ cells) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int ci = blockIdx.x * 4 + (threadIdx.x >> 6);            // the wave's cell: the dense index i * gx + j
  if (ci >= blocks * blocks) return;                             // the whole wave
  uint8_t* out = cells + ((int64_t)b * blocks * blocks + ci) * 3;
  PastePhoto ph;
  const bool in_range = paste_photo(boxes, offs, hw, n_images, b, ph);
  const PasteBox box = paste_box(boxes, b);
  const RedactGrid g = redact_grid(box, blocks);
  unsigned long long s0 = 0, s1 = 0, s2 = 0, cnt = 0;
  if (in_range && g.cell && ci < g.gy * g.gx) {                  // uniform over the wave
    const int i = ci / g.gx, j = ci - i * g.gx;
    const int64_t H = (int64_t)box.y1 - box.y0, W = (int64_t)box.x1 - box.x0, cell = g.cell;
    const int64_t by1 = (i + 1) * cell < H ? (i + 1) * cell : H, bx1 = (j + 1) * cell < W ? (j + 1) * cell : W;
    // the cell in photo coordinates, clipped to the photo: after the clip every bound lies in [0, sh] or [0, sw]
    int64_t ry0 = box.y0 + i * cell, ry1 = box.y0 + by1, rx0 = box.x0 + j * cell, rx1 = box.x0 + bx1;
    ry0 = ry0 > 0 ? ry0 : 0; rx0 = rx0 > 0 ? rx0 : 0;
    ry1 = ry1 < ph.sh ? ry1 : ph.sh; rx1 = rx1 < ph.sw ? rx1 : ph.sw;
    if (ry1 > ry0 && rx1 > rx0) {
      const int ch = (int)(ry1 - ry0), cw = (int)(rx1 - rx0);
      const uint8_t* sp = src + ph.off;
      // lane l takes pixels l, l + 64, ... of the clipped cell, row-major; (pr, pc) advances by 64 pixels without a division
      const int qs = 64 / cw, rs = 64 - qs * cw;
      int pr = lane / cw, pc = lane - pr * cw;
      while (pr < ch) {
        const uint8_t* px = sp + ((int64_t)(ry0 + pr) * ph.sw + (rx0 + pc)) * 3;
        s0 += px[0]; s1 += px[1]; s2 += px[2];
        ++cnt;
        pr += qs; pc += rs;
        if (pc >= cw) { pc -= cw; ++pr; }
      }
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    s0 += __shfl_xor(s0, m, 64); s1 += __shfl_xor(s1, m, 64); s2 += __shfl_xor(s2, m, 64); cnt += __shfl_xor(cnt, m, 64);
  }
  if (lane == 0) {
    // mean = (2 sum + cnt) / (2 cnt): half up, exact; a cell without a pixel, a cell index past the grid, a row that is not active: 0
    out[0] = cnt ? (uint8_t)((2 * s0 + cnt) / (2 * cnt)) : (uint8_t)0;
    out[1] = cnt ? (uint8_t)((2 * s1 + cnt) / (2 * cnt)) : (uint8_t)0;
    out[2] = cnt ? (uint8_t)((2 * s2 + cnt) / (2 * cnt)) : (uint8_t)0;
  }
}

struct RedactRow {
  PasteBox box;
  RedactGrid g;
  float iry, irx;             // its edge ramp
  float inv;                  // (float)(1 / cell): the smooth mode's scale
  const uint8_t* cg;          // its grid of means [gy][gx][3]
  const float* e;             // with the mask: its lines [K][3]
  const float* is;            //                its inv_soft
  bool whole;                 //                its hull is flagged: the whole box is redacted
};

// The hull weight of photo pixel (r, c) in a row's box, the rule of include/imm_hull.h: w = clamp(min_k ((ny_k rr + nx_k cc) + d_k) *
// inv_soft, 0, 1).  A SECOND copy of morph.hip's hull_weight, on purpose: that definition is pinned where it is by the tests of the
// seam, and this file must not depend on morph.hip's internals.  tests/test_redact_gpu.py holds this copy bit for bit to
// tests/hull_reference.py, the restatement that holds the other.
__device__ __forceinline__ float redact_hull_weight(const float* __restrict__ e, float inv_soft, int K, float rr, float cc) {
#pragma clang fp contract(off)
  float dist = __builtin_huge_valf();
  for (int k = 0; k < K; ++k) {
    const float a = e[3 * k] * rr, b = e[3 * k + 1] * cc;
    const float s = (a + b) + e[3 * k + 2];
    dist = fminf(dist, s);
  }
  return fminf(fmaxf(dist * inv_soft, 0.f), 1.f);
}

template <bool HULL>
struct RedactPolicy {
  typedef RedactRow Row;
  const int32_t* boxes;
  const float* inv_ramp;
  const uint8_t* cells;
  const float *edges, *inv_soft;
  const int32_t* hull_flags;
  int blocks, mode, K;
  Row own;

  // row j with its grid at cg (and its lines at e, its inv_soft at is)
  __device__ __forceinline__ Row row(int j, const uint8_t* cg, const float* e, const float* is) const {
    Row q;
    q.box = paste_box(boxes, j);
    q.g = redact_grid(q.box, blocks);
    q.iry = inv_ramp[2 * j]; q.irx = inv_ramp[2 * j + 1];
    // the correctly rounded float quotient (a row that is not active covers no pixel: its scale is never used)
    q.inv = q.g.cell ? (float)(1.0 / (double)q.g.cell) : 0.f;
    q.cg = cg; q.e = e; q.is = is;
    q.whole = false;
    if constexpr (HULL) q.whole = hull_flags[j] != 0;
    return q;
  }
  __device__ __forceinline__ Row row(int j) const {
    return row(j, cells + (int64_t)j * blocks * blocks * 3, HULL ? edges + (int64_t)j * 3 * K : nullptr, HULL ? inv_soft + j : nullptr);
  }
  __device__ __forceinline__ bool covers(const Row& q, int r, int c) const { return q.g.cell != 0 && paste_inside(q.box, r, c); }
  // the cell's mean (or the bilinear sample of the grid of means) blended by the ramp (HULL: times the hull weight where that is
  // > 0; a flagged row: times 1, everywhere)
  __device__ __forceinline__ void apply(const Row& q, int r, int c, float (&v)[3]) const {
#pragma clang fp contract(off)
    // 0 <= r - y0 < 2^32 for a pixel inside the box: the unsigned difference is exact where the signed one could overflow
    const uint32_t dy = (uint32_t)r - (uint32_t)q.box.y0, dx = (uint32_t)c - (uint32_t)q.box.x0;
    [[maybe_unused]] float w = 1.f;
    if constexpr (HULL) {
      if (!q.whole) {
        w = redact_hull_weight(q.e, *q.is, K, (float)dy, (float)dx);
        if (!(w > 0.f)) return;                                    // outside the hull: the row leaves the pixel alone
      }
    }
    float g[3];
    if (mode == IMM_REDACT_PIXELATE) {
      const uint8_t* cp = q.cg + ((int)(dy / q.g.cell) * q.g.gx + (int)(dx / q.g.cell)) * 3;
      g[0] = (float)cp[0]; g[1] = (float)cp[1]; g[2] = (float)cp[2];
    } else {
      const float fy = ((float)dy + 0.5f) * q.inv - 0.5f, fx = ((float)dx + 0.5f) * q.inv - 0.5f;
      paste_sample_photo(q.cg, q.g.gy, q.g.gx, fy, fx, g);
    }
    const float ramp = paste_ramp(q.box, r, c, q.iry, q.irx);
    if constexpr (HULL) {
      paste_blend(v, g, ramp * w);
    } else {
      paste_blend(v, g, ramp);
    }
  }
};

template <bool HULL>
__global__ __launch_bounds__(256) void redact_u8_kernel(uint8_t* __restrict__ dst, const int64_t* __restrict__ offs,
                                                        const int32_t* __restrict__ hw, int n_images, const int32_t* __restrict__ boxes,
                                                        const int32_t* __restrict__ links, const float* __restrict__ inv_ramp,
                                                        const uint8_t* __restrict__ cells, int blocks, int mode,
                                                        const float* __restrict__ edges, const float* __restrict__ inv_soft,
                                                        const int32_t* __restrict__ hull_flags, int K, int n) {
  __shared__ uint8_t cg_s[IMM_REDACT_MAX_BLOCKS * IMM_REDACT_MAX_BLOCKS * 3];
  __shared__ float e_s[HULL ? 3 * SPLINE_MAX_M + 1 : 1];           // its lines, then its inv_soft (without HULL: never referenced)
  const int b = blockIdx.y;
  PastePhoto ph;
  if (!paste_photo(boxes, offs, hw, n_images, b, ph)) return;      // uniform over the block: no barrier is skipped by part of it
  RedactPolicy<HULL> pol{boxes, inv_ramp, cells, edges, inv_soft, hull_flags, blocks, mode, K};
  pol.own = pol.row(b, cg_s, HULL ? e_s : nullptr, HULL ? e_s + 3 * SPLINE_MAX_M : nullptr);
  if (!pol.own.g.cell) return;                                     // not active: uniform as well
  const int bytes = pol.own.g.gy * pol.own.g.gx * 3;               // <= blocks * blocks * 3
  for (int i = threadIdx.x; i < bytes; i += 256) cg_s[i] = cells[(int64_t)b * blocks * blocks * 3 + i];
  if constexpr (HULL) {
    for (int i = threadIdx.x; i < 3 * K; i += 256) e_s[i] = edges[(int64_t)b * 3 * K + i];
    if (threadIdx.x == 0) e_s[3 * SPLINE_MAX_M] = inv_soft[b];
  }
  __syncthreads();
  paste_rows(pol, pol.own.box, ph, dst + ph.off, boxes, links, n);
}

extern "C" int imm_redact_cells_u8(const uint8_t* src, const int64_t* offsets, const int32_t* hw, int n_images, const int32_t* boxes,
                                   int blocks, int n, uint8_t* cells, void* stream) {
  IMM_REQUIRE(src && offsets && hw && boxes && cells, "redact_cells_u8: null pointer");
  IMM_REQUIRE(cells != src, "redact_cells_u8: cells must not be src");
  IMM_REQUIRE(n > 0 && n <= 65535 && n_images > 0, "redact_cells_u8: 0 < n <= 65535 rows, n_images > 0 (got %d, %d)", n, n_images);
  IMM_REQUIRE(blocks >= 1 && blocks <= IMM_REDACT_MAX_BLOCKS, "redact_cells_u8: 1 <= blocks <= %d (got %d)", IMM_REDACT_MAX_BLOCKS, blocks);
  hipLaunchKernelGGL(redact_cells_kernel, dim3((blocks * blocks + 3) / 4, n), dim3(256), 0, (hipStream_t)stream, src, offsets, hw, n_images,
                     boxes, blocks, cells);
  IMM_CHECK_LAUNCH("imm_redact_cells_u8");
  return 0;
}

extern "C" int imm_redact_u8(uint8_t* dst, const int64_t* offsets, const int32_t* hw, int n_images, const int32_t* boxes,
                             const int32_t* links, const float* inv_ramp, const uint8_t* cells, int blocks, int mode, const float* edges,
                             const float* inv_soft, const int32_t* hull_flags, int K, int n, int max_box_pixels, void* stream) {
  IMM_REQUIRE(dst && offsets && hw && boxes && links && inv_ramp && cells, "redact_u8: null pointer");
  IMM_REQUIRE(cells != dst, "redact_u8: cells is read only and must not be dst");
  IMM_REQUIRE(n > 0 && n <= 65535 && n_images > 0, "redact_u8: 0 < n <= 65535 rows, n_images > 0 (got %d, %d)", n, n_images);
  IMM_REQUIRE(blocks >= 1 && blocks <= IMM_REDACT_MAX_BLOCKS, "redact_u8: 1 <= blocks <= %d (got %d)", IMM_REDACT_MAX_BLOCKS, blocks);
  IMM_REQUIRE(mode == IMM_REDACT_PIXELATE || mode == IMM_REDACT_SMOOTH, "redact_u8: mode must be 0 (pixelate) or 1 (smooth) (got %d)", mode);
  IMM_REQUIRE(max_box_pixels > 0, "redact_u8: max_box_pixels > 0 (got %d)", max_box_pixels);
  const bool mask = edges != nullptr;
  IMM_REQUIRE(mask == (inv_soft != nullptr) && mask == (hull_flags != nullptr),
              "redact_u8: edges, inv_soft and hull_flags are all NULL or all given");
  if (mask) IMM_REQUIRE(K >= 1 && K <= SPLINE_MAX_M, "redact_u8: 1 <= K <= %d landmarks (got %d)", SPLINE_MAX_M, K);
  const dim3 grid(paste_grid_x(max_box_pixels), n);
  if (mask)
    hipLaunchKernelGGL(redact_u8_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, dst, offsets, hw, n_images, boxes, links, inv_ramp,
                       cells, blocks, mode, edges, inv_soft, hull_flags, K, n);
  else
    hipLaunchKernelGGL(redact_u8_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, dst, offsets, hw, n_images, boxes, links, inv_ramp,
                       cells, blocks, mode, edges, inv_soft, hull_flags, 0, n);
  IMM_CHECK_LAUNCH("imm_redact_u8");
  return 0;
}
