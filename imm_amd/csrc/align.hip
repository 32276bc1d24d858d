// align.hip — alignment on gfx950: photos warped so that their landmarks land on a fixed template (imm_amd/alignment.py).
//
// The backward map T_b (template frame -> the sample's S x S landmark frame, T_b(t_c) ~= mu_b,c) of all three models
// (similarity, affine, thin-plate spline) is linear in the sample's landmarks, because the control points are the template:
//
//   coef[b] = F . vec(mu[b])                       imm_align_coeffs   (F f64 on the host, once per template / model / lam)
//   T_b(q)  = sum_j basis_j(q) * coef[b][j]        imm_align_warp_u8  (basis: U(|q - t_j|^2) for j < K, then 1, q_y, q_x)
//
// and the warp samples the u8 photo ONCE through T_b and the row's box geometry, keypoints()' conventions:
//
//   q = (-1 + 2 i / So, -1 + 2 j / So)             output pixel (i, j) in the template frame
//   c = (T_b(q) + 1) / 2 * S                       crop pixel coordinate of the S x S frame
//   s = (y0 + c_y sy, x0 + c_x sx)                 source-photo coordinate, geom[b] = (y0, x0, sy, sx)
//   out = bilinear(photo, s)                       taps floor(s), floor(s) + 1; a tap outside the photo reads 0; f32 in [0, 255]
//
// With a power-of-two S = So, an identity coef and geometry (0, 0, 1, 1) every step above is exact in f32 and s is the integer pixel
// index: the interpolation then takes weight 1 on one tap (a + (b - a) * 0) and the output equals the photo bit for bit.
//
// imm_align_warp_u8: one thread = one output pixel for AL_TB = 8 samples, as tps.hip does: a basis value (f32 [m3][So * So],
// shared by the whole batch, coalesced) is loaded once per tile and feeds 16 accumulators; coef sits in LDS (broadcast reads).
// m3 == 3 (similarity, affine) reads no basis: 1, q_y, q_x are formed in registers.  Algorithmic bytes: n * So * So * 12 written
// plus the 4 * m3 * So * So-byte basis per 8 samples; the photo taps are L2 hits (a 218 x 178 photo is 116 KB).
// Tap indices are clamped into the photo BEFORE an address is formed and the zero of an outside tap is applied afterwards, so
// nothing outside the packed buffer is ever addressed whatever coef holds (NaN and far-away coordinates read as outside).
#include "common.h"

#define AL_TB 8
#define AL_MAX_M3 67
#define AL_MAX_K 64

// coef[b][r] = sum_i mu[b][i] * ft[i][r]   (r < 2 m3, i < 2K; ft = F transposed, so the threads of a sample stream it coalesced).
// One workgroup per sample; mu is read once into LDS; plain f32 fma chain in the order i = 0, 1, ...
__global__ __launch_bounds__(192) void align_coeffs_kernel(const float* __restrict__ mu, const float* __restrict__ ft, int k2, int r2,
                                                           float* __restrict__ coef) {
  __shared__ float msh[2 * AL_MAX_K];
  const int b = blockIdx.x;
  for (int i = threadIdx.x; i < k2; i += 192) msh[i] = mu[(int64_t)b * k2 + i];
  __syncthreads();
  const int r = threadIdx.x;
  if (r >= r2) return;
  float acc = 0.f;
  for (int i = 0; i < k2; ++i) acc = fmaf(msh[i], ft[i * r2 + r], acc);
  coef[(int64_t)b * r2 + r] = acc;
}

extern "C" int imm_align_coeffs(const float* mu, const float* ft, int batch, int k, int m3, float* coef, void* stream) {
  IMM_REQUIRE(mu && ft && coef, "align_coeffs: null pointer");
  IMM_REQUIRE(batch > 0 && k >= 1 && k <= AL_MAX_K && m3 >= 3 && m3 <= AL_MAX_M3, "align_coeffs: batch > 0, 1 <= k <= %d, 3 <= m3 <= %d",
              AL_MAX_K, AL_MAX_M3);
  hipLaunchKernelGGL(align_coeffs_kernel, dim3(batch), dim3(192), 0, (hipStream_t)stream, mu, ft, 2 * k, 2 * m3, coef);
  IMM_CHECK_LAUNCH("imm_align_coeffs");
  return 0;
}

struct AlignSrc {
  const void* src;          // packed u8 HWC photos, or (F32SRC) f32 [n][S][S][3]
  const int64_t* offs;      // u8: start of image i in src
  const int32_t* hw;        // u8: (rows, columns) of image i
  const int32_t* boxes;     // u8: (image, y0, x0, y1, x1) per output row; only the image index is read here
  int n_images;
};

template <bool BASIS, bool F32SRC>
__global__ __launch_bounds__(256) void align_warp_kernel(AlignSrc in, const float* __restrict__ geom, const float* __restrict__ coef,
                                                         const float* __restrict__ basis_t, int m3, int batch, int S, int So,
                                                         float q_step, float* __restrict__ dst, int ld_dst) {
#pragma clang fp contract(off)   // the sampling arithmetic is written out: a + (b - a) * t must give a when t == 0 and stay unfused
  extern __shared__ float2 csh[];                      // [m3][AL_TB]: (y, x) coefficients of this block's samples (zeros beyond nb)
  const int npix = So * So;
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int b0 = blockIdx.y * AL_TB;
  const int nb = batch - b0 < AL_TB ? batch - b0 : AL_TB;
  for (int t = threadIdx.x; t < m3 * AL_TB; t += 256) {
    const int j = t / AL_TB, i = t - j * AL_TB;
    csh[t] = i < nb ? *(const float2*)(coef + ((int64_t)(b0 + i) * m3 + j) * 2) : make_float2(0.f, 0.f);
  }
  __syncthreads();
  if (p >= npix) return;
  const int oi = p / So, oj = p - oi * So;
  const float qy = fmaf((float)oi, q_step, -1.f), qx = fmaf((float)oj, q_step, -1.f);
  float ty[AL_TB], tx[AL_TB];
#pragma unroll
  for (int i = 0; i < AL_TB; ++i) { ty[i] = 0.f; tx[i] = 0.f; }
  const int nrad = m3 - 3;
  if constexpr (BASIS) {
    // the radial part, 8 basis loads in flight per thread; summation order j = 0, 1, ...
    int j = 0;
    for (; j + 8 <= nrad; j += 8) {
      float l[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) l[u] = basis_t[(int64_t)(j + u) * npix + p];
#pragma unroll
      for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int i = 0; i < AL_TB; ++i) {
          const float2 cv = csh[(j + u) * AL_TB + i];
          ty[i] = fmaf(l[u], cv.x, ty[i]);
          tx[i] = fmaf(l[u], cv.y, tx[i]);
        }
    }
    for (; j < nrad; ++j) {
      const float l = basis_t[(int64_t)j * npix + p];
#pragma unroll
      for (int i = 0; i < AL_TB; ++i) {
        const float2 cv = csh[j * AL_TB + i];
        ty[i] = fmaf(l, cv.x, ty[i]);
        tx[i] = fmaf(l, cv.y, tx[i]);
      }
    }
  }
  // the affine part 1, q_y, q_x from registers (its basis rows are never read)
#pragma unroll
  for (int i = 0; i < AL_TB; ++i) {
    const float2 c0 = csh[nrad * AL_TB + i], c1 = csh[(nrad + 1) * AL_TB + i], c2 = csh[(nrad + 2) * AL_TB + i];
    ty[i] = fmaf(qx, c2.x, fmaf(qy, c1.x, ty[i] + c0.x));
    tx[i] = fmaf(qx, c2.y, fmaf(qy, c1.y, tx[i] + c0.y));
  }
  const float half_s = 0.5f * (float)S;
#pragma unroll
  for (int i = 0; i < AL_TB; ++i) {
    if (i >= nb) break;
    const int b = b0 + i;
    const float4 g = *(const float4*)(geom + (int64_t)b * 4);
    const float fy = fmaf((ty[i] + 1.f) * half_s, g.z, g.x), fx = fmaf((tx[i] + 1.f) * half_s, g.w, g.y);
    int sh, sw;
    const uint8_t* s8 = nullptr;
    const float* s32 = nullptr;
    if constexpr (F32SRC) {
      sh = S; sw = S;
      s32 = (const float*)in.src + (int64_t)b * S * S * 3;
    } else {
      const int img = min(max(in.boxes[5 * b], 0), in.n_images - 1);
      sh = in.hw[2 * img]; sw = in.hw[2 * img + 1];
      s8 = (const uint8_t*)in.src + in.offs[img];
    }
    // NaN and far-away coordinates (the int conversion would overflow) are outside the photo
    const bool sane = fabsf(fy) < 1.0e9f && fabsf(fx) < 1.0e9f && sh > 0 && sw > 0;
    const float y0f = floorf(fy), x0f = floorf(fx);
    const float wy = fy - y0f, wx = fx - x0f;
    const int r0 = sane ? (int)y0f : -4, c0 = sane ? (int)x0f : -4;
    const int r1 = r0 + 1, c1 = c0 + 1;
    const bool v0 = sane && r0 >= 0 && r0 < sh, v1 = sane && r1 >= 0 && r1 < sh;
    const bool u0 = sane && c0 >= 0 && c0 < sw, u1 = sane && c1 >= 0 && c1 < sw;
    // clamped indices first, the zero of an outside tap afterwards
    const int shc = max(sh, 1), swc = max(sw, 1);
    const int64_t ra = (int64_t)min(max(r0, 0), shc - 1) * swc, rb = (int64_t)min(max(r1, 0), shc - 1) * swc;
    const int ca = min(max(c0, 0), swc - 1), cb = min(max(c1, 0), swc - 1);
    float* d = dst + ((int64_t)b * npix + p) * ld_dst;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      float tl, tr, bl, br;
      if constexpr (F32SRC) {
        tl = s32[(ra + ca) * 3 + ch]; tr = s32[(ra + cb) * 3 + ch];
        bl = s32[(rb + ca) * 3 + ch]; br = s32[(rb + cb) * 3 + ch];
      } else {
        tl = sane ? (float)s8[(ra + ca) * 3 + ch] : 0.f; tr = sane ? (float)s8[(ra + cb) * 3 + ch] : 0.f;
        bl = sane ? (float)s8[(rb + ca) * 3 + ch] : 0.f; br = sane ? (float)s8[(rb + cb) * 3 + ch] : 0.f;
      }
      tl = (v0 && u0) ? tl : 0.f; tr = (v0 && u1) ? tr : 0.f;
      bl = (v1 && u0) ? bl : 0.f; br = (v1 && u1) ? br : 0.f;
      const float top = tl + (tr - tl) * wx;
      const float bot = bl + (br - bl) * wx;
      d[ch] = top + (bot - top) * wy;
    }
  }
}

extern "C" int imm_align_warp_u8(const void* src, int src_f32, const int64_t* offsets, const int32_t* hw, int n_images,
                                 const int32_t* boxes, const float* geom, const float* coef, const float* basis_t, int m3, int batch,
                                 int image_size, int out_size, float* dst, int ld_dst, void* stream) {
  IMM_REQUIRE(src && geom && coef && dst, "align_warp_u8: null pointer");
  IMM_REQUIRE(src_f32 || (offsets && hw && boxes && n_images > 0), "align_warp_u8: the u8 source needs offsets, hw, boxes and n_images > 0");
  IMM_REQUIRE(batch > 0 && batch <= 65535 * AL_TB && m3 >= 3 && m3 <= AL_MAX_M3, "align_warp_u8: batch, 3 <= m3 <= %d", AL_MAX_M3);
  IMM_REQUIRE(m3 == 3 || basis_t, "align_warp_u8: m3 = %d needs the basis", m3);
  IMM_REQUIRE(image_size > 0 && image_size <= 8192 && out_size > 0 && out_size <= 8192 && ld_dst >= 3, "align_warp_u8: sizes (ld_dst >= 3)");
  const dim3 grid((out_size * out_size + 255) / 256, (batch + AL_TB - 1) / AL_TB);
  const size_t lds = (size_t)m3 * AL_TB * sizeof(float2);
  const AlignSrc in{src, offsets, hw, boxes, n_images};
  // 2 / So as the correctly rounded float quotient (exact for a power-of-two So); the device's '/' may be approximate
  const float q_step = (float)(2.0 / (double)out_size);
#define AL_LAUNCH(BASIS, F32)                                                                                                      \
  hipLaunchKernelGGL((align_warp_kernel<BASIS, F32>), grid, dim3(256), lds, (hipStream_t)stream, in, geom, coef, basis_t, m3, batch, \
                     image_size, out_size, q_step, dst, ld_dst)
  if (m3 > 3) { if (src_f32) AL_LAUNCH(true, true); else AL_LAUNCH(true, false); }
  else        { if (src_f32) AL_LAUNCH(false, true); else AL_LAUNCH(false, false); }
#undef AL_LAUNCH
  IMM_CHECK_LAUNCH("imm_align_warp_u8");
  return 0;
}
