/* imm_align.h - C-ABI of the alignment entry points of libimm_hip.so (ABI 25; imm_amd/csrc/align.hip, imm_amd/alignment.py):
 * photos warped so that their landmarks land on a fixed template.  Included by imm_hip.h, whose conventions hold here: plain
 * pointers and sizes, an explicit hipStream_t as void*, int status (0 = ok) and imm_last_error(). */
#ifndef IMM_ALIGN_H
#define IMM_ALIGN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The backward map T_b (template frame -> the sample's S x S landmark frame) of the similarity, affine and thin-plate-spline models is
 * linear in the sample's landmarks: coef[b] = F . vec(mu[b]).  mu f32 [batch, K, 2] ((y, x) in [-1, 1]); ft f32 [2K][2 m3] = F
 * transposed (F f64 [2 m3, 2K] from LandmarkTemplate.fit_matrix, rounded once); coef f32 [batch, m3, 2] written ((y, x) per basis
 * function: U(|q - t_j|^2) for j < m3 - 3, then 1, q_y, q_x).  1 <= k <= 64, 3 <= m3 <= 67.  One workgroup per sample, an f32 fma
 * chain over i = 0 .. 2K - 1.  Every pointer is read at the launch only, so the call can be captured behind the pose head. */
int imm_align_coeffs(const float* mu, const float* ft, int batch, int k, int m3, float* coef, void* stream);
/* dst[b][i][j][0..2] (f32, pixel stride ld_dst >= 3, out_size x out_size pixels) = the photo of row b sampled bilinearly at
 *   q = (-1 + 2 i / out_size, -1 + 2 j / out_size);  v = sum_j basis_j(q) coef[b][j];  c = (v + 1) / 2 * image_size;
 *   s = (geom[b][0] + c_y geom[b][2], geom[b][1] + c_x geom[b][3])
 * with taps floor(s), floor(s) + 1 and zeros outside the photo (the conventions of the keypoint epilogue: a keypoint and an aligned
 * pixel name the same place).  src_f32 == 0: src is the packed u8 HWC buffer of imm_resize_crop_u8 (offsets, hw indexed by image,
 * n_images of them) and row b reads image boxes[5 b] (int32 [batch, 5] rows; only the image index is used, clamped to n_images).
 * src_f32 != 0: src is f32 [batch, image_size, image_size, 3] and row b reads its own image (offsets / hw / boxes ignored).
 * basis_t f32 [m3][out_size^2] is shared by the batch and read for j < m3 - 3 only (1, q_y, q_x come from registers); m3 == 3 takes
 * basis_t == NULL.  Tap indices are clamped before an address is formed; NaN or far-away coordinates read as outside.  With a
 * power-of-two image_size == out_size, an identity coef and geom (0, 0, 1, 1) the output equals the photo bit for bit. */
int imm_align_warp_u8(const void* src, int src_f32, const int64_t* offsets, const int32_t* hw, int n_images, const int32_t* boxes,
                      const float* geom, const float* coef, const float* basis_t, int m3, int batch, int image_size, int out_size,
                      float* dst, int ld_dst, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IMM_ALIGN_H */
