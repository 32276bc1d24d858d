// gfx950.h — the ONE definition of the gfx950 buffer, LDS-DMA and DPP primitives the hand-written convolution kernels share
// (included by conv_common.h).  Everything here is a typedef, a constant or a __forceinline__ helper: moving a kernel onto it
// leaves its device assembly unchanged line for line (profiles/gfx950_header_asm_identity.txt).  The inline-asm statements are
// the ones tools/asm_hazard_audit.py checks (rules S, M and D): a wait state, a clobber or a descriptor bit changes HERE.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

typedef __attribute__((address_space(3))) void lds_void_t;               // (uint32_t)(size_t)(lds_void_t*)smem = LDS byte address
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;        // four SGPRs (descriptor) or four VGPRs (16 B of data)

// ---- buffer resource descriptor ---------------------------------------------------------------------------------------------
// Words 0-1 = 48-bit base address (stride 0 in the upper 16 bits of word 1), word 2 = extent in bytes, word 3 = the flags word
// cdna_hip_programming.md T8 gives for a raw buffer on this chip (`__builtin_amdgcn_make_buffer_rsrc(ptr, /*stride*/ 0, bytes,
// flags)`, which conv_igemm.hip and conv_wgrad.hip use as is): with it a buffer_* instruction adds its 32-bit per-lane offset and
// its scalar offset to the base as BYTES and range-checks the sum against word 2 in hardware.  The kernels rely on exactly that
// check: an out-of-range lane of a load or an LDS-DMA load delivers zeros, an out-of-range lane of a store is dropped.  Build
// the descriptor from wave-uniform values only (T20).
#define BUFFER_RSRC_FLAGS 0x00020000u
__device__ __forceinline__ u32x4_t buffer_rsrc(const void* base, uint32_t bytes) {
  const uint64_t a = (uint64_t)base;
  return u32x4_t{(uint32_t)a, (uint32_t)(a >> 32) & 0xffffu, bytes, BUFFER_RSRC_FLAGS};
}
// per-lane offset beyond every extent: the load returns zero, the store is dropped — how a kernel with a FIXED number of VMEM
// instructions per step (one counted s_waitcnt vmcnt is then exact) turns the ones without work into no-ops
#define BUFFER_OOB 0x80000000u

// One LDS-DMA instruction: 64 lanes x 16 B from buffer `rsrc` (+ per-lane voff + scalar soff; out-of-range lanes
// deliver zeros) to LDS bytes [lds_addr, lds_addr + 1024), lane-linear.  Inline asm on purpose: hipcc models the builtin form
// as an LDS write and drains vmcnt(0) in front of the next ds_read, which serialises the ring; an asm statement is
// invisible to that bookkeeping, so the kernel's own counted s_waitcnt is the only wait.  M0 (LDS base of the DMA) is
// written in the same statement that uses it (the compiler does not preserve M0 across statements); s_nop 0 is the wait state
// between the SALU write of M0 and the LDS-DMA load that reads it (audit rule M).
__device__ __forceinline__ void lds_dma16(u32x4_t rsrc, uint32_t lds_addr, uint32_t voff, uint32_t soff) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
               :: "s"(lds_addr), "v"(voff), "s"(rsrc), "s"(soff) : "memory");
}

// One 16-byte store per lane, from asm so that it counts as exactly one VMEM instruction of the kernel's own vmcnt schedule.
__device__ __forceinline__ void store16(u32x4_t rsrc, u32x4_t data, uint32_t voff, uint32_t soff) {
  // The trailing s_nop 1 is REQUIRED (round 5): a VMEM store of more than 64 bits reads its data registers over the cycles after
  // issue, and hipcc — which does not know what is inside an asm statement — pads no wait states behind it; without them its next
  // VALU instruction may overwrite v[data] before the store has read it (cdna_hip_programming.md §5.7 "Stores").  Seen as a
  // 0.3 % rate of corrupted 16-byte outputs of conv_halo2's ci = 64 instantiations (358 registers, the data registers are reused
  // at once) whenever a second process shared the GPU — the flaky two-rank test of rounds 3-5 (tools/det_graph.py reproduces it).
  asm volatile("buffer_store_dwordx4 %0, %1, %2, %3 offen\n\ts_nop 1" :: "v"(data), "v"(voff), "s"(rsrc), "s"(soff) : "memory");
}

// total over each row of 16 lanes, in every lane: x += row_ror(x, 8), 4, 2, 1 — the rotation rides on the add (one VALU
// instruction per step; s_nop 1 = the two wait states a DPP read needs after the VALU write of its source)
__device__ __forceinline__ float row_sum16(float x) {
  float y;
  asm volatile("s_nop 1\n\tv_add_f32_dpp %0, %1, %1 row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
               "s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_ror:4 row_mask:0xf bank_mask:0xf\n\t"
               "s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_ror:2 row_mask:0xf bank_mask:0xf\n\t"
               "s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_ror:1 row_mask:0xf bank_mask:0xf\n\ts_nop 1"
               : "=&v"(y) : "v"(x));
  return y;
}

// The kernels' OWN waits, from asm like the operations they wait for (hipcc counts neither): at most N VMEM operations of this
// wave outstanding (loads, LDS-DMA loads and stores alike; N = 0 drains them) / every LDS and scalar-memory operation done.
template <int N>
__device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
__device__ __forceinline__ void wait_lgkmcnt0() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// ---- compile-time helpers ---------------------------------------------------------------------------------------------------
// f(integral_constant<int, I>) for I = first .. N-1: the index decides fragment buffers, LDS immediates and which DMA pieces
// ride on a step
template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}
// compile-time int as a function argument (a generic lambda reads decltype(tag)::value)
template <int V> using Int = std::integral_constant<int, V>;

// __builtin_amdgcn_sched_group_barrier masks (LLVM AMDGPU SchedGroupMask)
#define SG_VALU 0x002
#define SG_SALU 0x004
#define SG_MFMA 0x008
#define SG_DSREAD 0x100

// ---- LDS chunk swizzles -----------------------------------------------------------------------------------------------------
// A pixel (or filter row) is C8 chunks of 16 B; chunk c of row x is stored at slot c ^ swz(x).  LDS-DMA writes lane-linear, so
// the permutation is applied on the source side of the DMA and again by the ds_read.  WHY each one is conflict-free for a
// kernel's read pattern is written at that kernel; swizzles that only one kernel uses stay there.
__device__ __forceinline__ int swz8(int x) { return ((x >> 1) & 3) << 1; }     // 128-byte rows (8 chunks)
__device__ __forceinline__ int swz4(int x) { return ((x >> 2) & 1) << 1; }     // 64-byte rows (4 chunks)
template <int C8>
__device__ __forceinline__ int halo_swz(int row) { return C8 == 8 ? swz8(row) : swz4(row); }
