// morph_common.h — what morph_u8_kernel (morph.hip) and seam_fit_kernel (seam.hip) share, so that imm_seam_fit takes its samples in the
// morph's own order of operations by running the morph's own text: a row's donor side, and the two samples with their mix.
#pragma once
#include "paste_common.h"

#define SEAM_MIN_B 16                        // ring samples of a row (imm_seam_fit, imm_morph_seam_u8)
#define SEAM_MAX_B 256

struct MorphRow {
  SplineRow s;
  const float *ca, *cb;       // coef_a, coef_b [M + 3][2]
  float tex;
  float by, bx, dhy, dhx;     // the donor box: corner and half sides
  int dimg;                   // the donor photo, -1: the row is not active
};

// the donor side of row j: its box as floats, and whether the row is ACTIVE
__device__ __forceinline__ void morph_donor(const int32_t* __restrict__ dboxes, int n_donor, int j, MorphRow& q) {
  const int di = dboxes[5 * j], dy0 = dboxes[5 * j + 1], dx0 = dboxes[5 * j + 2];
  // in 64 bits: the sides of a box row that holds anything
  const int64_t dh = (int64_t)dboxes[5 * j + 3] - dy0, dw = (int64_t)dboxes[5 * j + 4] - dx0;
  q.by = (float)dy0; q.bx = (float)dx0;
  q.dhy = 0.5f * (float)dh; q.dhx = 0.5f * (float)dw;
  q.dimg = (di >= 0 && di < n_donor && dh > 0 && dw > 0) ? di : -1;
}

// the donor's place of the frame point (qy, qx) displaced by DB
__device__ __forceinline__ void morph_donor_place(const MorphRow& q, float qy, float qx, const float (&DB)[2], float& by, float& bx) {
#pragma clang fp contract(off)
  by = q.by + ((qy + DB[0]) + 1.f) * q.dhy;
  bx = q.bx + ((qx + DB[1]) + 1.f) * q.dhx;
}

// the row's own photo sampled at (ay, ax), the donor photo at (by, bx) (g != nullptr: times its gain, plus its offset), mixed by tex
template <bool COLOUR>
__device__ __forceinline__ void morph_mix(const uint8_t* __restrict__ sp, int sh, int sw, const uint8_t* __restrict__ dp, int dh, int dw,
                                          float ay, float ax, float by, float bx, const float* g, float tex, float (&mix)[3]) {
#pragma clang fp contract(off)
  float ga[3], gb[3];
  paste_sample_photo(sp, sh, sw, ay, ax, ga);
  paste_sample_photo(dp, dh, dw, by, bx, gb);
  if constexpr (COLOUR) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float sc = gb[ch] * g[2 * ch];
      gb[ch] = sc + g[2 * ch + 1];
    }
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float e = gb[ch] - ga[ch];
    const float te = tex * e;
    mix[ch] = ga[ch] + te;
  }
}
