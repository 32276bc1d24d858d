// conv_dispatch.h — the convolution files' private interface (host only): every internal imm_* function that one .hip file
// defines and another calls is declared here, once, and both files include this header.
#pragma once
#include "common.h"

struct ConvArgs;   // conv_common.h

// ---- forward / data gradient, in imm_conv2d's dispatch order (conv_igemm.hip: conv_plan) -----------------------------------------
// Each family: does it take the descriptor, its imm_conv2d_variant code, its rows of batch-norm partial sums, its launch.
bool imm_halo2_applicable(const imm_conv_desc* d);                                 // conv_halo2.hip: filter in registers
int imm_halo2_variant(const imm_conv_desc* d);
int imm_halo2_grid(const imm_conv_desc* d);
void imm_conv_halo2_launch(int dtype, const imm_conv_desc* d, const ConvArgs& a, hipStream_t s);
bool imm_halo_applicable(const imm_conv_desc* d);                                  // conv_halo.hip: filter in LDS
int imm_halo_variant(const imm_conv_desc* d);
int imm_halo_grid(const imm_conv_desc* d);
void imm_conv_halo_launch(int dtype, const imm_conv_desc* d, const ConvArgs& a, hipStream_t s);
bool imm_halo_s2d_applicable(const imm_conv_desc* d);                              //   one-launch stride-2 data gradient
void imm_conv_halo_s2d_launch(int dtype, const imm_conv_desc* d, const ConvArgs& a, hipStream_t s);
bool imm_hdeep_applicable(const imm_conv_desc* d);                                 // conv_hdeep.hip: LDS halo, deep K
int imm_hdeep_variant(const imm_conv_desc* d);
int imm_hdeep_stats_blocks(const imm_conv_desc* d);
void imm_conv_hdeep_launch(int dtype, const imm_conv_desc* d, const ConvArgs& a, hipStream_t s);
bool imm_hdeep_s2d_applicable(const imm_conv_desc* d);
void imm_conv_hdeep_s2d_launch(int dtype, const imm_conv_desc* d, const ConvArgs& a, hipStream_t s);
bool imm_hdeep6_enabled();                                                         // conv_hdeep6.hip: hdeep's 16x16x128 tile
void imm_conv_hdeep6_launch(int dtype, const ConvArgs& a, int n_patches, int patches_x, int patches_y, int n_wg, bool persist, int cus,
                            hipStream_t s);
bool imm_s2f_applicable(const imm_conv_desc* d);                                   // conv_s2f.hip: stride-2 forward
int imm_s2f_variant(const imm_conv_desc* d);
int imm_s2f_stats_blocks(const imm_conv_desc* d);
void imm_conv_s2f_launch(int dtype, const imm_conv_desc* d, const ConvArgs& a, hipStream_t s);
void imm_conv64_launch(int dtype, ConvArgs& a, int bm, int bn, hipStream_t s);      // conv_igemm64.hip: im2col, BK = 64
bool imm_conv64_group_launch(int dtype, ConvArgs* args, int n, int bm, int bn, hipStream_t s);
int imm_conv_f32(const imm_conv_desc* d, const void* x, const void* wt, const float* bias, void* y, float* stats_partial,
                 const void* mask_ref, hipStream_t s);                             // conv_f32.hip: the f32 witness
int imm_conv_f32_wgrad(const imm_conv_desc* d, const void* x, const void* dy, int lddy, float* slab, int nsplit, hipStream_t s);

// ---- filter gradient (conv_wgrad.hip: wgm_classify) ---------------------------------------------------------------------------------
bool imm_wgrad_tr_applicable(const imm_conv_desc* d, int lddy);                    // conv_wgrad_tr.hip
int imm_wgrad_tr_variant(const imm_conv_desc* d);
void imm_wgrad_tr_launch(int dtype, const imm_conv_desc* d, const void* x, const void* dy, int lddy, float* slab, int nsplit,
                         hipStream_t s);
int imm_wgrad_tr_args_bytes();
int imm_wgrad_tr_fill(const imm_conv_desc* d, const void* x, const void* dy, int lddy, float* slab, int nsplit, void* out, int* steps);
void imm_wgrad_tr_launch_multi(int dtype, int bn, const void* tab_dev, const int* first_dev, int n, int blocks, hipStream_t s);
bool imm_wgrad_halo_applicable(const imm_conv_desc* d, int lddy);                  // conv_wgrad_halo.hip
int imm_wgrad_halo_variant(const imm_conv_desc* d, int lddy);
int imm_wgrad_halo_splits(const imm_conv_desc* d, int lddy);
int imm_wgrad_halo_blocks(const imm_conv_desc* d, int lddy, int* n_patches);
int imm_wgrad_halo_per_cu(int variant);
void imm_wgrad_halo_launch(int dtype, const imm_conv_desc* d, const void* x, const void* dy, int lddy, float* slab, int nsplit,
                           hipStream_t s, const float* nol_scale, const float* nol_shift, int nol_relu);
int imm_wgrad_halo_args_bytes();
int imm_wgrad_halo_fill(const imm_conv_desc* d, const void* x, const void* dy, int lddy, float* slab, int nsplit, void* out, int* steps,
                        const float* nol_scale, const float* nol_shift, int nol_relu);
void imm_wgrad_halo_launch_multi(int dtype, int variant, const void* tab_dev, const int* first_dev, int n, int blocks, hipStream_t s);
