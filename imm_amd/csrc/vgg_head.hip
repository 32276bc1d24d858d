// vgg_head.hip — the head of the frozen perceptual VGG16 in ONE launch: gray+normalise -> conv1_1 (1 -> 64) -> conv1_2 (64 -> 64).
//
// Reference: imm/models/selfsup/build_vgg16.py:22-26 (mean over RGB, /255, -114.451/255), imm/models/selfsup/vgg16.py:345-346
// (conv1_1, conv1_2: 3x3 SAME + bias + ReLU), input batch concat([gt, pred], 0) (imm/models/imm_model.py:126).
//
// Why: conv1_1's output is the largest tensor of the step (2B x 128^2 x 64 = 134 MB at batch 32) and lived for exactly one
// kernel boundary — vgg_conv1_1_fwd wrote it (35 us, HBM-bound), conv_halo2<64,64> read it back (77 us, of which 15 us are input
// traffic: profiles/r06_halo2_ablation.txt).  Here the persistent conv1_2 workgroup PRODUCES the 10x18-pixel conv1_1 halo of its
// next patch itself, on the matrix cores, straight into the LDS stage the 3x3 taps read:
//   * a pre-pass (vgg_gray_kernel, 4 MB, L2-resident afterwards) stores the normalised gray image as a PAIR of 16-bit values per
//     pixel, g = hi + lo (lo = the rounding residue of hi): with the filter split the same way, w = whi + wlo, one
//     v_mfma_f32_16x16x32 per 16 pixels x 16 channels computes whi.ghi + whi.glo + wlo.ghi over the 9 taps (27 of the 32 k slots)
//     — the f32 product to 2^-16 relative, i.e. the arithmetic of the VALU kernel it replaces up to the rounding of the last
//     bit, for 48 extra MFMAs per patch next to conv1_2's 576;
//   * the 12 x 24-word gray patch of patch it+3 is DMA'd into a 3-deep LDS ring (one buffer_load_dwordx4 ... lds per wave),
//     the halo of patch it+1 is produced during step it (two LDS halo stages), the 3x3 loop of patch it and the interleaved
//     epilogue of patch it-1 are conv_halo2's (filter taps in 144 VGPRs, halo rows read once for three vertical taps);
//   * conv1_1's activation is still stored where somebody reads it: the prediction half (the ReLU mask of conv1_2's data
//     gradient), 8x16 interior pixels per patch, from the producer's registers (`store_from` = first image stored).
// Every loop VMEM op is issued from inline asm with a fixed count per wave and step (1 DMA + 6 conv1_1 stores + 4 output stores;
// out-of-range buffer offsets turn the ones without work into no-ops), so one counted s_waitcnt vmcnt per step is exact.
#include "conv_common.h"
#include <stdlib.h>

#define VH_PH 8
#define VH_PW 16
#define VH_HW 18
#define VH_GROW 24                  // gray patch row: image columns x0-4 .. x0+19 (16-byte aligned pieces)
#define VH_GSTAGE_U4 256            // one gray stage: 4 waves x 1 KB (72 pieces of 16 B used)
#define VH_HSTAGE_U4 (192 * 8)      // one halo stage: 192 pixel slots x 128 B
#define VH_NG 3                     // gray ring depth = prefetch distance in steps
#define VH_VMEM_PER_STEP 11

struct VhArgs {
  const uint32_t* gray;             // [n_img][s][s] words: hi | lo << 16
  const float* w11; const float* b11;
  const uint16_t* wt12; const float* b12; int kpad12;
  uint16_t* a11; uint16_t* y12;
  int n_img, s, store_from;
  int n_patches, patches_x, patches_y, lg_px, lg_pi;
  uint32_t gray_bytes, act_bytes;
};

// Loop VMEM ops: lds_dma16 and store16 of gfx950.h (store16's trailing s_nop 1: a > 64-bit store reads its data registers after
// issue); halo chunk swizzle: swz8, as in conv_halo2.hip.

// normalised gray image as (hi, lo) pairs of the activation type (the VALU expression of vgg_conv1_1_fwd_kernel, bit for bit)
template <typename ET>
__global__ __launch_bounds__(256) void vgg_gray_kernel(const float* __restrict__ gt, const float* __restrict__ pred, int ldp, int batch,
                                                       int s, uint32_t* __restrict__ gray) {
  const int64_t npix = (int64_t)2 * batch * s * s;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < npix; p += (int64_t)gridDim.x * 256) {
    const int64_t per = (int64_t)batch * s * s;
    const float* src = p < per ? gt + p * 3 : pred + (p - per) * ldp;
    const float g = (src[0] + src[1] + src[2]) / 3.0f / 255.0f - 114.451f / 255.0f;
    const uint16_t hi = ET::from_f32(g);
    const uint16_t lo = ET::from_f32(g - ET::to_f32(hi));
    gray[p] = (uint32_t)hi | ((uint32_t)lo << 16);
  }
}

template <typename ET>
__global__ __launch_bounds__(256) void conv_halo2_vgg_head_kernel(const VhArgs ha) {
  constexpr int CI = 64, KS = 2, MT = 4, NT = 2, NR = MT + 2, KW = 3, KH = 3;
  constexpr int PIXB = CI * 2, ROWB = VH_HW * PIXB;
  constexpr int H_U4 = VH_HSTAGE_U4;
  // At the top of step `it` the gray patch of patch it+1 — requested first thing in step it-2 — must have landed.  vmcnt counts
  // loads and stores alike and the two kinds need not complete in order with each other (LLVM's waitcnt model treats mixed pending
  // VMEM reads and writes of gfx9 as out of order), so the wait is NOT "all but the 21 ops issued after it": it is conv_halo2's
  // rule — at most ONE WHOLE step of VMEM ops outstanding, i.e. everything issued two steps ago (the request among it) is done,
  // whatever the order inside a step.
  constexpr int WAITN = VH_VMEM_PER_STEP;
  extern __shared__ __attribute__((aligned(16))) uint4 smem[];   // [2][H_U4] halo stages | [VH_NG][VH_GSTAGE_U4] gray ring

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid >> 1, wn = wid & 1;
  const int frow = lane & 15, q = lane >> 4;
  const int S = ha.s;
  const u32x4_t gr = buffer_rsrc(ha.gray, ha.gray_bytes), yr = buffer_rsrc(ha.y12, ha.act_bytes), ar = buffer_rsrc(ha.a11, ha.act_bytes);
  const uint32_t lds_base = (uint32_t)(size_t)(lds_void_t*)smem;
  const int G = gridDim.x, per_img = ha.patches_x * ha.patches_y;
  // patch order: conv_halo2.hip (one contiguous band of patches per XCD, walked side by side by its workgroups)
  const bool xcd_mode = (G & 7) == 0;
  const int xq = ha.n_patches >> 3, xrem = ha.n_patches & 7, xid = blockIdx.x & 7;
  const int band0 = xid * xq + (xid < xrem ? xid : xrem), band_n = xq + (xid < xrem ? 1 : 0);
  auto seq_patch = [&](int seq) -> int {
    if (xcd_mode) {
      const int local = (int)(blockIdx.x >> 3) + seq * (G >> 3);
      return local < band_n ? band0 + local : -1;
    }
    const int pt = blockIdx.x + seq * G;
    return pt < ha.n_patches ? pt : -1;
  };
  struct Pd { int img, y0, x0; };
  const bool pow2 = ha.lg_px >= 0;
  auto decode = [&](int patch) -> Pd {
    Pd d;
    if (patch < 0) { d.img = 0; d.y0 = 0x4000; d.x0 = 0; return d; }
    int pr, py;
    if (pow2) { d.img = patch >> ha.lg_pi; pr = patch & (per_img - 1); py = pr >> ha.lg_px; d.x0 = (pr & (ha.patches_x - 1)) * VH_PW; }
    else { d.img = patch / per_img; pr = patch - d.img * per_img; py = pr / ha.patches_x; d.x0 = (pr - py * ha.patches_x) * VH_PW; }
    d.y0 = py * VH_PH;
    return d;
  };

  // ---- conv1_2 filter -> registers (conv_halo2.hip: MFMA row 4q'+r of tile j <-> channel 32 wn + 8q' + 4j + r) -------------------
  u32x4_t bw[KH * KW][KS][NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int n = wn * 32 + (frow >> 2) * 8 + j * 4 + (frow & 3);
    const uint16_t* wrow = ha.wt12 + (size_t)n * ha.kpad12 + q * 8;
#pragma unroll
    for (int tap = 0; tap < KH * KW; ++tap)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) bw[tap][ks][j] = *(const u32x4_t*)(wrow + tap * CI + ks * 32);
  }
  float bv[NT][4];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) bv[j][r] = ha.b12[wn * 32 + q * 8 + j * 4 + r];

  // ---- conv1_1 filter as the A operands of the producer: tile jj (16 channels), row rho = frow <-> channel 32 (jj >> 1) + 8 (rho >> 2)
  // + 4 (jj & 1) + (rho & 3), so that a lane (which holds D rows 4q .. 4q+3 of every tile) owns the 16-byte chunks q (tiles 0, 1) and
  // q + 4 (tiles 2, 3) of its pixel.  The B operand is the RAW gray words of the lane's taps — k slots (2i, 2i+1) of k group q = (ghi,
  // glo) of tap 4q + i (q = 2: tap 8 and zeros, q = 3: zeros): no shuffling, four ds_read_b32 per lane.  Two MFMAs share it:
  //   w1a: slots (2i, 2i+1) = (whi, whi) of that tap  -> whi.ghi + whi.glo
  //   w1b: slots (2i, 2i+1) = (wlo, 0)                -> wlo.ghi            (wlo.glo, 2^-16 relative, is dropped)
  // conv1_1's bias is "tap 9": (bhi, 0) / (blo, 0) against a constant (1.0, 0) in slot (q = 2, i = 1) of the B operand.
  // (in registers: read from an LDS image instead, every producer MFMA waited for its own ds_read — 108 vs 102 us)
  u32x4_t w1a[4], w1b[4];
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    const int n = (jj >> 1) * 32 + (frow >> 2) * 8 + (jj & 1) * 4 + (frow & 3);
    uint32_t ea[4], eb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int t = 4 * q + i;
      // tap 9 = the bias against the constant 1.0 the B operand carries in that slot: (bhi, 0) x (1, 0) + (blo, 0) x (1, 0)
      const float wv = t < 9 ? ha.w11[(t < 9 ? t : 0) * 64 + n] : t == 9 ? ha.b11[n] : 0.f;
      const uint16_t h = ET::from_f32(wv);
      const uint16_t l = ET::from_f32(wv - ET::to_f32(h));
      ea[i] = t == 9 ? (uint32_t)h : (uint32_t)h | ((uint32_t)h << 16);
      eb[i] = (uint32_t)l;
    }
    w1a[jj] = u32x4_t{ea[0], ea[1], ea[2], ea[3]};
    w1b[jj] = u32x4_t{eb[0], eb[1], eb[2], eb[3]};
  }
  const uint32_t one_word = (uint32_t)ET::from_f32(1.0f);     // (1.0, 0) as a (hi, lo) pair
  // compiler-visible global loads end here (conv_halo2.hip: keep the compiler's own vmcnt(0) out of the loop)
#pragma unroll
  for (int tap = 0; tap < KH * KW; ++tap)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int j = 0; j < NT; ++j) asm volatile("" : "+v"(bw[tap][ks][j]));
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) asm volatile("" : "+v"(bv[j][r]));
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) { asm volatile("" : "+v"(w1a[jj])); asm volatile("" : "+v"(w1b[jj])); }

  // ---- producer geometry: wave wid makes the 16-slot groups wid, wid + 4, wid + 8 of the 192 halo slots ------------------------------
  int p_hyx[3];             // (hy << 8) | hx, hy = 0x40 for the padding slots >= 180
  int p_gb[3], p_go[4];     // gray word of the lane's tap 4q + i inside a gray stage = p_gb[k] + p_go[i]; the dead slots (taps >= 9: zero
                            // filter) read the pixel's own word — any FINITE value does (words 0 .. 303 of a stage are written by every DMA)
  int p_hw[3];              // byte offset of chunk q inside a halo stage (chunk q + 4: ^ 64)
  int p_ar[3];              // byte offset of the pixel's chunk q in conv1_1's activation, relative to the patch origin
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int hp = (wid + 4 * k) * 16 + frow;
    const int hy = hp / VH_HW, hx = hp - hy * VH_HW;
    p_hyx[k] = ((hp < (VH_PH + 2) * VH_HW ? hy : 0x40) << 8) | hx;
    p_gb[k] = hy * VH_GROW + hx + 2;
    p_hw[k] = hp * PIXB + ((q ^ swz8(hx)) << 4);
    p_ar[k] = ((hy - 1) * S + (hx - 1)) * (CI * 2) + q * 16;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int t = 4 * q + i;
    p_go[i] = t < 9 ? (t / 3) * VH_GROW + t % 3 : 0;
  }
  // gray DMA piece of this lane: piece = 64 wid + lane of 72 (row = piece / 6 of 12, 16-byte column piece % 6 of 6)
  const int g_piece = wid * 64 + lane;
  const int g_row = g_piece / 6, g_col = g_piece - g_row * 6;
  auto gray_dma = [&](const Pd& d, int slot) {
    const int iy = d.y0 - 2 + g_row, ix = d.x0 - 4 + 4 * g_col;
    const bool ok = (g_piece < 72) & ((unsigned)iy < (unsigned)S) & ((unsigned)ix < (unsigned)S);
    uint32_t in_range = (uint32_t)((iy * S + ix) * 4);
    asm volatile("" : "+v"(in_range));
    const uint32_t vo = ok ? in_range : BUFFER_OOB;
    lds_dma16(gr, lds_base + (uint32_t)((2 * H_U4 + slot * VH_GSTAGE_U4) * 16 + wid * 1024), vo, (uint32_t)(d.img * S * S) * 4u);
  };
  // producer, group k, in three pieces that the row loop spreads over consecutive rows (each piece's inputs are then a row old: no
  // exposed latency, and the VALU part rides in the shadow of the 3x3 loop's MFMAs like the epilogue does):
  // (1) the lane's four gray words = the B operand (+ the constant 1.0 of the bias slot)
  auto gather = [&](int gslot, int k) -> uint4 {
    const uint32_t* Gs = (const uint32_t*)(smem + 2 * H_U4 + gslot * VH_GSTAGE_U4);
    const uint32_t g1 = Gs[p_gb[k] + p_go[1]];
    return make_uint4(Gs[p_gb[k] + p_go[0]], q == 2 ? one_word : g1, Gs[p_gb[k] + p_go[2]], Gs[p_gb[k] + p_go[3]]);
  };
  // (2) 16 pixels x 64 channels of conv1_1 (+ bias) on the matrix cores
  auto pmfma = [&](f32x4_t (&pa)[4], const uint4 gop) {
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) pa[jj] = ET::mfma(__builtin_bit_cast(uint4, w1a[jj]), gop, f32x4_t{0.f, 0.f, 0.f, 0.f});
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) pa[jj] = ET::mfma(__builtin_bit_cast(uint4, w1b[jj]), gop, pa[jj]);
  };
  // (3) ReLU, zero padding, 16-bit -> halo stage `stage` of patch d; interior pixels of images >= store_from to HBM
  auto ppost = [&](const Pd& d, int stage, int k, const f32x4_t (&pa)[4]) {
    char* Hs = (char*)(smem + stage * H_U4);
    const int hy = p_hyx[k] >> 8, hx = p_hyx[k] & 0xff;
    const int iy = d.y0 - 1 + hy, ix = d.x0 - 1 + hx;
    const bool valid = ((unsigned)iy < (unsigned)S) & ((unsigned)ix < (unsigned)S);     // (padding slots: hy = 0x40, never valid)
    const bool interior = valid & (d.img >= ha.store_from) & (hy >= 1) & (hy <= VH_PH) & (hx >= 1) & (hx <= VH_PW);
    // ReLU and the SAME zero padding of conv1_2's INPUT in one v_med3: median(x, 0, cap), cap = +inf inside the image, 0 outside
    const float cap = valid ? __builtin_huge_valf() : 0.f;
    uint32_t a_in = (uint32_t)((d.y0 * S + d.x0) * (CI * 2) + p_ar[k]);
    asm volatile("" : "+v"(a_in));
    const uint32_t a_vo = interior ? a_in : BUFFER_OOB;
    const uint32_t a_soff = (uint32_t)(d.img * S * S) * (uint32_t)(CI * 2);
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = __builtin_amdgcn_fmed3f(pa[2 * p + (e >> 2)][e & 3], 0.f, cap);
      const uint4 pk = pack8<ET>(v);
#ifdef VH_ABLATE      // diagnosis builds only (tools/ablate_build.sh): 2 = no conv1_1 stores, 4 = no halo writes either
      if (!(VH_ABLATE & 4)) *(uint4*)(Hs + (p_hw[k] ^ (p << 6))) = pk;
      else if (pk.x == 0x12345678u) *(uint4*)(Hs + (p_hw[k] ^ (p << 6))) = pk;
      if (!(VH_ABLATE & 6)) store16(ar, u32x4_t{pk.x, pk.y, pk.z, pk.w}, interior ? a_vo + (uint32_t)(p << 6) : BUFFER_OOB, a_soff);
#else
      *(uint4*)(Hs + (p_hw[k] ^ (p << 6))) = pk;
      store16(ar, u32x4_t{pk.x, pk.y, pk.z, pk.w}, interior ? a_vo + (uint32_t)(p << 6) : BUFFER_OOB, a_soff);
#endif
    }
  };

  // per-lane byte offset of the A fragments inside a halo stage (conv_halo2.hip)
  int lrel[KW];
#pragma unroll
  for (int kx = 0; kx < KW; ++kx) lrel[kx] = wm * MT * ROWB + (frow + kx) * PIXB + ((q ^ swz8(frow + kx)) << 4);
  const uint32_t ovoff = (uint32_t)((frow * 64 + wn * 32 + q * 8) * 2);

  // ---- prologue ------------------------------------------------------------------------------------------------------------------
  Pd dq[4];                                    // patches it .. it+3
#pragma unroll
  for (int s_ = 0; s_ < 4; ++s_) dq[s_] = decode(seq_patch(s_));
  gray_dma(dq[0], 0); gray_dma(dq[1], 1); gray_dma(dq[2], 2);
  wait_vmcnt<0>();
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int k = 0; k < 3; ++k) { f32x4_t pa0[4]; pmfma(pa0, gather(0, k)); ppost(dq[0], 0, k, pa0); }
  // the steady-state wait assumes two whole steps of VMEM ops behind the gray request it waits for: pad with no-op stores so that
  // the first steps' waits are never early (the three prologue DMAs are already complete)

  f32x4_t acc[2][MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[1][i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  int it = 0;
  int gs1 = 1;                                 // gray slot of patch it+1 = (it + 1) % 3
  uint32_t prev_voff = BUFFER_OOB, prev_soff = 0u;

  auto step = [&](auto phase, auto mma) {
    constexpr int PH = decltype(phase)::value;
    constexpr bool MMA = decltype(mma)::value;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(WAITN) : "memory");   // gray(it+1) landed; this wave's halo(it) writes done
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    const int hs = it & 1;
    const int gs0 = gs1 == 0 ? VH_NG - 1 : gs1 - 1;                           // it % 3: the slot gray(it+3) goes to
    uint4 gop = make_uint4(0, 0, 0, 0);        // the producer's B operand of the next group of patch it+1 (gray(it+1) was waited for above)
    f32x4_t paA[4], paB[4];
    if constexpr (MMA) {
      gray_dma(dq[3], gs0);
      gop = gather(gs1, 0);
    }
    const uint4* rowp[KW][KS];
#pragma unroll
    for (int kx = 0; kx < KW; ++kx)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        rowp[kx][ks] = (const uint4*)((const char*)smem + hs * (H_U4 * 16) + (lrel[kx] ^ (ks * 64)));
    uint4 fa[2][KW][KS];
    if constexpr (MMA) {
#pragma unroll
      for (int kx = 0; kx < KW; ++kx)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) fa[0][kx][ks] = rowp[kx][ks][0];
    }
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[PH][i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    __builtin_amdgcn_sched_barrier(0);

#pragma unroll
    for (int rr = 0; rr < NR; ++rr) {
      int n_mfma = 0;
      if constexpr (MMA) {
        if (rr + 1 < NR) {
#pragma unroll
          for (int kx = 0; kx < KW; ++kx)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) fa[(rr + 1) & 1][kx][ks] = rowp[kx][ks][(rr + 1) * (ROWB / 16)];
        }
#pragma unroll
        for (int kx = 0; kx < KW; ++kx)
#pragma unroll
          for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int ky = 0; ky < KH; ++ky) {
              const int i = rr - ky;
              if (i >= 0 && i < MT) {
#pragma unroll
                for (int j = 0; j < NT; ++j)
                  acc[PH][i][j] = ET::mfma(__builtin_bit_cast(uint4, bw[ky * KW + kx][ks][j]), fa[rr & 1][kx][ks], acc[PH][i][j]);
                n_mfma += NT;
              }
            }
      }
      // ---- epilogue of the previous patch, tile row rr - 1: bias, ReLU, one 16-byte store per lane -------------------------------
      if (rr >= 1 && rr <= MT) {
        const int i = rr - 1;
        float v[8];
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) v[j * 4 + r] = fmaxf(acc[PH ^ 1][i][j][r] + bv[j][r], 0.f);
        const uint4 o = pack8<ET>(v);
        store16(yr, u32x4_t{o.x, o.y, o.z, o.w}, prev_voff == BUFFER_OOB ? BUFFER_OOB : prev_voff + (uint32_t)((wm * MT + i) * S * 64 * 2), prev_soff);
      }
      // ---- the conv1_1 halo of patch it+1: three 16-slot groups per wave, software-pipelined over rows 0 .. 3 ---------------------
      if constexpr (MMA) {
        if (rr == 0) { pmfma(paA, gop); gop = gather(gs1, 1); n_mfma += 8; }
        if (rr == 1) { ppost(dq[1], hs ^ 1, 0, paA); pmfma(paB, gop); gop = gather(gs1, 2); n_mfma += 8; }
        if (rr == 2) { ppost(dq[1], hs ^ 1, 1, paB); pmfma(paA, gop); n_mfma += 8; }
        if (rr == 3) { ppost(dq[1], hs ^ 1, 2, paA); }
      }
      if constexpr (MMA) {
        __builtin_amdgcn_sched_group_barrier(SG_DSREAD, KW * KS, 0);
#pragma unroll
        for (int m = 0; m < 44; ++m) {
          if (m < n_mfma) {
            __builtin_amdgcn_sched_group_barrier(SG_MFMA, 1, 0);
            __builtin_amdgcn_sched_group_barrier(SG_VALU | SG_SALU, 3, 0);
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (MMA) {
      prev_voff = dq[0].y0 < 0x4000 ? (uint32_t)((dq[0].y0 * S + dq[0].x0) * 64 * 2) + ovoff : BUFFER_OOB;
      prev_soff = (uint32_t)(dq[0].img * S * S) * (uint32_t)(64 * 2);
      dq[0] = dq[1]; dq[1] = dq[2]; dq[2] = dq[3];
      dq[3] = decode(seq_patch(it + 4));
    }
    gs1 = gs1 + 1 == VH_NG ? 0 : gs1 + 1;
    ++it;
  };
  for (;;) {
    step(Int<0>(), Int<1>());
    if (dq[0].y0 >= 0x4000) { step(Int<1>(), Int<0>()); break; }
    step(Int<1>(), Int<1>());
    if (dq[0].y0 >= 0x4000) { step(Int<0>(), Int<0>()); break; }
  }
  wait_vmcnt<0>();     // no LDS-DMA may outlive the workgroup
}

// ---------------------------------------------------------------------------------------------------------------------------------
extern "C" int imm_vgg_head_supported(int batch, int s, int dtype) {
  static const bool off = imm_conv_disabled("vgg_head");
  if (off || (dtype != IMM_BF16 && dtype != IMM_F16)) return 0;
  if (batch <= 0 || s < 32 || s % VH_PW || s % VH_PH) return 0;
  return (int64_t)2 * batch * s * s * 128 < (1LL << 31) ? 1 : 0;
}

extern "C" int64_t imm_vgg_head_scratch_bytes(int batch, int s) { return (int64_t)2 * batch * s * s * (int64_t)sizeof(uint32_t); }

extern "C" int imm_vgg_head_fwd(const float* gt, const float* pred, int ldp, int batch, int s, const float* w9x64, const float* b64,
                                const void* wt12, int kpad12, const float* b12, void* a11, int store_from, void* y12, void* gray_scratch,
                                int dtype, void* stream) {
  IMM_REQUIRE(gt && pred && w9x64 && b64 && wt12 && b12 && a11 && y12 && gray_scratch, "vgg_head_fwd: null");
  IMM_REQUIRE(ldp >= 3 && kpad12 == 9 * 64, "vgg_head_fwd: ldp >= 3, conv1_2 filter packed [co][9 taps x 64 channels]");
  IMM_REQUIRE(imm_vgg_head_supported(batch, s, dtype), "vgg_head_fwd: shape / dtype not served (imm_vgg_head_supported)");
  IMM_REQUIRE(store_from >= 0 && store_from <= 2 * batch, "vgg_head_fwd: store_from in [0, 2 batch]");
  hipStream_t st = (hipStream_t)stream;
  const int64_t npix = (int64_t)2 * batch * s * s;
  const unsigned ggrid = (unsigned)((npix + 255) / 256 > 4096 ? 4096 : (npix + 255) / 256);
  IMM_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((vgg_gray_kernel<ET>), dim3(ggrid), dim3(256), 0, st, gt, pred, ldp, batch, s,
                                               (uint32_t*)gray_scratch));
  IMM_CHECK_LAUNCH("imm_vgg_head_fwd(gray)");
  VhArgs ha;
  ha.gray = (const uint32_t*)gray_scratch;
  ha.w11 = w9x64; ha.b11 = b64;
  ha.wt12 = (const uint16_t*)wt12; ha.b12 = b12; ha.kpad12 = kpad12;
  ha.a11 = (uint16_t*)a11; ha.y12 = (uint16_t*)y12;
  ha.n_img = 2 * batch; ha.s = s; ha.store_from = store_from;
  ha.patches_x = s / VH_PW; ha.patches_y = s / VH_PH;
  ha.n_patches = ha.n_img * ha.patches_x * ha.patches_y;
  const int per_img = ha.patches_x * ha.patches_y;
  ha.lg_px = ha.lg_pi = -1;
  if ((ha.patches_x & (ha.patches_x - 1)) == 0 && (per_img & (per_img - 1)) == 0) {
    ha.lg_px = __builtin_ctz(ha.patches_x); ha.lg_pi = __builtin_ctz(per_img);
  }
  ha.gray_bytes = (uint32_t)(npix * 4);
  ha.act_bytes = (uint32_t)(npix * 128);
  const size_t lds = (size_t)(2 * VH_HSTAGE_U4 + VH_NG * VH_GSTAGE_U4) * 16;
  const int cus = imm_device_cus();
  const int grid = ha.n_patches < cus ? ha.n_patches : cus;
  IMM_DISPATCH_DTYPE(dtype, imm_launch<conv_halo2_vgg_head_kernel<ET>>(dim3(grid), dim3(256), lds, st, ha));
  IMM_CHECK_LAUNCH("imm_vgg_head_fwd");
  return 0;
}
