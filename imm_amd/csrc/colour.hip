// colour.hip — colour matching between the two photographs of a morph on gfx950 (imm_amd/inference.py LandmarkDetector.morph(colour=...)
// and LandmarkDetector.colour_stats, imm_amd/morphing.py).  The rule is stated once, in include/imm_colour.h; in short:
//
//   imm_colour_stats_u8  per row: the sums of v and of v * v per channel and the pixel count over the pixels of the row's box that lie in
//                        its photo and in the ellipse inscribed in the box, as uint64 [n, 7]; integer arithmetic throughout, so the result
//                        is exact whatever order the chip adds in
//   imm_colour_gain      per (row, channel): the two regions' mean and spread -> (gain, offset) f32, in f64 with every operation rounded
//                        separately, bit-identical to the numpy restatement (as imm_track_step and imm_retarget are)
//
// (imm_morph_colour_u8, which applies the gain to the donor's sample, is morph.hip's kernel in its second instantiation.)
// Stats: the launch shape of the paste kernels (paste_common.h): grid (paste_grid_x(largest box / 8), n), 256 threads, blockIdx.y is
// the row, a thread takes photo pixels of the box clipped to the photo in a grid-stride loop (eight turns on the largest box), lanes of a
// wave on consecutive pixels of a photo row, byte-wide loads (a photo row starts at any byte).  Addressing: the box is clipped to [0, h) x [0, w) of a photo whose index
// passed 0 <= image < n_images before any pixel address is formed; the ellipse test only takes pixels away.
// What a thread does is a __host__ __device__ function of (block, thread, grid), so that the same text compiles for the host, where a
// stand-alone program runs it under the address and undefined-behaviour sanitizers on exact-size heap buffers.
#include "paste_common.h"

#define COLOUR_MAX_AREA ((int64_t)1 << 30)   // H * W of a row's box: (H W)^2 <= 2^60 keeps the ellipse test inside 64 bits
#define COLOUR_PER_THREAD 8                  // pixels of the largest box per thread: the grid is sized for that many turns of the loop, so
                                             // that the reduction and the seven adds of a block are paid once per 2048 pixels

struct ColourSums {
  // A thread of the smallest grid (ONE block of 256) takes at most 2^30 / 256 = 2^22 pixels: s1 <= 255 * 2^22 < 2^30 and cnt <= 2^22 fit
  // 32 bits; s2 <= 65025 * 2^22 < 2^38 does not, so it is 64 bits wide.  None of them can overflow.
  uint32_t s1[3], cnt;
  uint64_t s2[3];
};

// The part of row b's region that thread tx of block bx (of gx blocks) takes: false when the row has the empty region.
__host__ __device__ __forceinline__ bool colour_thread_sums(const uint8_t* __restrict__ buf, const int64_t* __restrict__ offs,
                                                            const int32_t* __restrict__ hw, int n_images, const int32_t* __restrict__ boxes,
                                                            int b, int bx, int tx, int gx, ColourSums& t) {
  t.s1[0] = t.s1[1] = t.s1[2] = t.cnt = 0;
  t.s2[0] = t.s2[1] = t.s2[2] = 0;
  const int img = boxes[5 * b];
  if (img < 0 || img >= n_images) return false;
  const int y0 = boxes[5 * b + 1], x0 = boxes[5 * b + 2], y1 = boxes[5 * b + 3], x1 = boxes[5 * b + 4];
  const int64_t H = (int64_t)y1 - y0, W = (int64_t)x1 - x0;         // in 64 bits: the sides of a box row that holds anything
  if (H <= 0 || W <= 0 || H > COLOUR_MAX_AREA || W > COLOUR_MAX_AREA || H * W > COLOUR_MAX_AREA) return false;
  const int sh = hw[2 * img], sw = hw[2 * img + 1];
  const int cy0 = y0 > 0 ? y0 : 0, cy1 = y1 < sh ? y1 : sh, cx0 = x0 > 0 ? x0 : 0, cx1 = x1 < sw ? x1 : sw;
  if (cy1 <= cy0 || cx1 <= cx0) return false;                      // no pixel in the photo
  const int cw = cx1 - cx0, chh = cy1 - cy0;
  // the clipped box is part of the box: area <= 2^30, and p stays below 2^30 + 2^24 (the stride is at most 65536 * 256): 32 bits
  const int area = cw * chh, stride = gx * 256;
  const uint8_t* const photo = buf + offs[img];
  const int64_t HW = H * W, HW2 = HW * HW;
  for (int p = bx * 256 + tx; p < area; p += stride) {
    const int pr = p / cw;
    const int r = cy0 + pr, c = cx0 + (p - pr * cw);
    const int64_t ea = (2 * ((int64_t)r - y0) + 1 - H) * W, eb = (2 * ((int64_t)c - x0) + 1 - W) * H;      // |.| < H W <= 2^30
    if (ea * ea + eb * eb > HW2) continue;
    const uint8_t* px = photo + ((int64_t)r * sw + c) * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const uint32_t v = px[ch];
      t.s1[ch] += v;
      t.s2[ch] += v * v;
    }
    t.cnt += 1;
  }
  return true;
}

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void colour_stats_u8_kernel(const uint8_t* __restrict__ buf, const int64_t* __restrict__ offs,
                                                              const int32_t* __restrict__ hw, int n_images,
                                                              const int32_t* __restrict__ boxes, unsigned long long* __restrict__ sums) {
  __shared__ uint64_t red[4][7];
  const int b = blockIdx.y;
  ColourSums t;
  // uniform over the block (the row's box and photo decide): no barrier is skipped by part of it
  if (!colour_thread_sums(buf, offs, hw, n_images, boxes, b, blockIdx.x, threadIdx.x, gridDim.x, t)) return;
  uint64_t v[7] = {t.s1[0], t.s1[1], t.s1[2], t.s2[0], t.s2[1], t.s2[2], t.cnt};
#pragma unroll
  for (int k = 0; k < 7; ++k) v[k] = wave_sum_u64(v[k]);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 7; ++k) red[wid][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < 7) {
    const uint64_t s = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    if (s) atomicAdd(sums + (int64_t)b * 7 + threadIdx.x, (unsigned long long)s);      // one add per block and column
  }
}

// (G, O) of one row and channel from the two rows of sums; true: the row is flagged and gets (1, 0)
__host__ __device__ __forceinline__ bool colour_gain_one(const uint64_t* __restrict__ sa, const uint64_t* __restrict__ sb, int ch, float amount,
                                                         double max_gain, float& G, float& O) {
#pragma clang fp contract(off)   // every operation rounded separately, as the host restatement's
  G = 1.f; O = 0.f;
  const double t = (double)amount;
  if (sa[6] == 0 || sb[6] == 0 || !__builtin_isfinite(t)) return true;    // (the builtin: one spelling for the device and a host build)
  const double Na = (double)sa[6], Nb = (double)sb[6];
  const double ma = (double)sa[ch] / Na, qa = (double)sa[3 + ch] / Na;
  const double mb = (double)sb[ch] / Nb, qb = (double)sb[3 + ch] / Nb;
  const double va = fmax(qa - ma * ma, 0.0), vb = fmax(qb - mb * mb, 0.0);
  const double sda = sqrt(va), sdb = sqrt(vb);
  double g = sdb > 0.0 ? sda / sdb : 1.0;
  g = fmin(fmax(g, 1.0 / max_gain), max_gain);
  const double gm = g * mb;
  const double o = ma - gm;
  const double tg = t * (g - 1.0), to = t * o;
  G = (float)(1.0 + tg);
  O = (float)to;
  return false;
}

__global__ __launch_bounds__(256) void colour_gain_kernel(const uint64_t* __restrict__ sums_a, const uint64_t* __restrict__ sums_b,
                                                          const float* __restrict__ amount, double max_gain, int n, float* __restrict__ gain,
                                                          int32_t* __restrict__ flags) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 3 * n) return;
  const int b = i / 3, ch = i - 3 * b;
  float G, O;
  const bool flagged = colour_gain_one(sums_a + (int64_t)b * 7, sums_b + (int64_t)b * 7, ch, amount[b], max_gain, G, O);
  gain[2 * i] = G; gain[2 * i + 1] = O;
  if (ch == 0) flags[b] = flagged ? 1 : 0;
}

extern "C" int imm_colour_stats_u8(const uint8_t* buf, const int64_t* offsets, const int32_t* hw, int n_images, const int32_t* boxes, int n,
                                   int max_box_pixels, uint64_t* sums, void* stream) {
  IMM_REQUIRE(buf && offsets && hw && boxes && sums, "colour_stats_u8: null pointer");
  IMM_REQUIRE(n > 0 && n <= 65535 && n_images > 0, "colour_stats_u8: 0 < n <= 65535 rows, n_images > 0 (got %d, %d)", n, n_images);
  IMM_REQUIRE(max_box_pixels > 0, "colour_stats_u8: max_box_pixels > 0 (got %d)", max_box_pixels);
  const hipError_t e = hipMemsetAsync(sums, 0, (size_t)n * 7 * sizeof(uint64_t), (hipStream_t)stream);
  if (e != hipSuccess) return imm_fail(IMM_E_HIP, "imm_colour_stats_u8: %s", hipGetErrorString(e));
  const int per_grid = (int)(((int64_t)max_box_pixels + COLOUR_PER_THREAD - 1) / COLOUR_PER_THREAD);
  hipLaunchKernelGGL(colour_stats_u8_kernel, dim3(paste_grid_x(per_grid), n), dim3(256), 0, (hipStream_t)stream, buf, offsets, hw, n_images,
                     boxes, (unsigned long long*)sums);
  IMM_CHECK_LAUNCH("imm_colour_stats_u8");
  return 0;
}

extern "C" int imm_colour_gain(const uint64_t* sums_a, const uint64_t* sums_b, const float* amount, double max_gain, int n, float* gain,
                               int32_t* flags, void* stream) {
  IMM_REQUIRE(sums_a && sums_b && amount && gain && flags, "colour_gain: null pointer");
  IMM_REQUIRE(n > 0 && n <= 65535, "colour_gain: 0 < n <= 65535 rows (got %d)", n);
  IMM_REQUIRE(max_gain >= 1.0 && max_gain - max_gain == 0.0, "colour_gain: max_gain must be finite and >= 1 (got %g)", max_gain);
  hipLaunchKernelGGL(colour_gain_kernel, dim3((unsigned)((3 * n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, sums_a, sums_b, amount,
                     max_gain, n, gain, flags);
  IMM_CHECK_LAUNCH("imm_colour_gain");
  return 0;
}
