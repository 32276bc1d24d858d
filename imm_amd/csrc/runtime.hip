// runtime.hip — error plumbing, device info and HIP-graph capture for libimm_hip.so.
// The graph entry points replace the role of TF's static-graph session.run
// (/root/reference/imm/train/cnn_train_multi.py:459): a whole training-step launch sequence is
// captured once on the caller's stream and replayed without host work.
#include "common.h"
#include <string.h>

thread_local char imm_err_buf[512] = "";

int imm_fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(imm_err_buf, sizeof(imm_err_buf), fmt, ap);
  va_end(ap);
  return code;
}

extern "C" int imm_abi_version(void) { return IMM_ABI_VERSION; }

bool imm_conv_disabled(const char* name) {
  const char* e = getenv("IMM_CONV_DISABLE");
  if (!e || !*e) return false;
  const size_t n = strlen(name);
  for (const char* p = e; *p;) {
    const char* q = strchr(p, ',');
    const size_t len = q ? (size_t)(q - p) : strlen(p);
    if (len == n && strncmp(p, name, n) == 0) return true;
    p += len + (q ? 1 : 0);
  }
  return false;
}
bool imm_hdeep_prof() {
  static const bool prof = getenv("IMM_HDEEP_PROF") != nullptr;
  return prof;
}
extern "C" const char* imm_last_error(void) { return imm_err_buf; }

int imm_device_cus() {
  static int cus = 0;
  if (cus == 0) {
    hipDeviceProp_t p; int dev = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&p, dev) == hipSuccess) cus = p.multiProcessorCount;
    else (void)hipGetLastError();       // no device (the CPU-only queries): not an error of the caller's next launch
    if (cus <= 0) cus = 256;
  }
  return cus;
}
bool imm_dyn_lds_opt_in(const void* kernel, size_t bytes) {
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) imm_fail(IMM_E_HIP, "hipFuncSetAttribute(dyn LDS %zu): %s", bytes, hipGetErrorString(e));
  return e == hipSuccess;
}

#ifndef IMM_SOURCE_DIGEST
#define IMM_SOURCE_DIGEST "unknown"
#endif
// the marker makes the digest readable from the file without loading it (imm_amd/build.py)
static const char imm_digest_marker[] = "IMM_SOURCE_DIGEST=" IMM_SOURCE_DIGEST;
extern "C" const char* imm_source_digest(void) { return imm_digest_marker + 18; }

__global__ void debug_stamp_kernel(uint64_t* slots, int index) { slots[index] = wall_clock64(); }

extern "C" int imm_debug_stamp(uint64_t* slots, int index, void* stream) {
  IMM_REQUIRE(slots && index >= 0, "debug_stamp: null / negative slot");
  hipLaunchKernelGGL(debug_stamp_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, slots, index);
  IMM_CHECK_LAUNCH("imm_debug_stamp");
  return 0;
}

extern "C" int imm_device_info(int32_t* out2) {
  IMM_REQUIRE(out2, "device_info: null");
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return imm_fail(IMM_E_HIP, "hipGetDevice: %s", hipGetErrorString(e));
  hipDeviceProp_t p;
  e = hipGetDeviceProperties(&p, dev);
  if (e != hipSuccess) return imm_fail(IMM_E_HIP, "hipGetDeviceProperties: %s", hipGetErrorString(e));
  out2[0] = p.multiProcessorCount;
  int arch = 0;
  const char* n = p.gcnArchName;  // "gfx950:sramecc+:xnack-"
  if (n[0] == 'g' && n[1] == 'f' && n[2] == 'x')
    for (const char* c = n + 3; *c && *c != ':'; ++c) {
      if (*c >= '0' && *c <= '9') arch = arch * 16 + (*c - '0');
      else if (*c >= 'a' && *c <= 'f') arch = arch * 16 + (*c - 'a' + 10);
    }
  out2[1] = arch;  // hex digits of the gfx name: gfx950 -> 0x950
  return 0;
}

extern "C" int imm_graph_begin(void* stream) {
  hipError_t e = hipStreamBeginCapture((hipStream_t)stream, hipStreamCaptureModeThreadLocal);
  if (e != hipSuccess) return imm_fail(IMM_E_HIP, "hipStreamBeginCapture: %s", hipGetErrorString(e));
  return 0;
}

extern "C" int imm_graph_end(void* stream, void** graph_exec_out) {
  IMM_REQUIRE(graph_exec_out, "graph_end: null out");
  hipGraph_t g = nullptr;
  hipError_t e = hipStreamEndCapture((hipStream_t)stream, &g);
  if (e != hipSuccess) return imm_fail(IMM_E_HIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
  hipGraphExec_t ge = nullptr;
  e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (e != hipSuccess) return imm_fail(IMM_E_HIP, "hipGraphInstantiate: %s", hipGetErrorString(e));
  *graph_exec_out = (void*)ge;
  return 0;
}

extern "C" int imm_graph_launch(void* graph_exec, void* stream) {
  IMM_REQUIRE(graph_exec, "graph_launch: null graph");
  hipError_t e = hipGraphLaunch((hipGraphExec_t)graph_exec, (hipStream_t)stream);
  if (e != hipSuccess) return imm_fail(IMM_E_HIP, "hipGraphLaunch: %s", hipGetErrorString(e));
  return 0;
}

extern "C" int imm_graph_destroy(void* graph_exec) {
  if (graph_exec) (void)hipGraphExecDestroy((hipGraphExec_t)graph_exec);
  return 0;
}

// ---- CRC-32C (Castagnoli), host-side: the checksum of TensorFlow's checkpoint bundles (tensor_bundle's per-tensor and
// per-block crc32c; imm_amd/utils/tf_checkpoint.py reads/writes the authors' `model.ckpt-N.{index,data-*}` files,
// reference: cnn_train_multi.py:404-439 tf.train.Saver).  Slicing-by-8 tables, reflected polynomial 0x82F63B78.
namespace {
struct Crc32cTables {
  uint32_t t[8][256];
  Crc32cTables() {
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0x82F63B78u & (0u - (c & 1u)));
      t[0][i] = c;
    }
    for (uint32_t i = 0; i < 256; ++i)
      for (int s = 1; s < 8; ++s) t[s][i] = (t[s - 1][i] >> 8) ^ t[0][t[s - 1][i] & 0xff];
  }
};
}  // namespace

// A copy done by a KERNEL (loads and stores go through the L2 like every other kernel's), for hand-overs between the host-bounced
// gradient exchange of the gloo test path and the step's kernels: src / dst may be device memory or pinned host memory (device
// accessible under HIP's unified addressing).  Round 5: after `hipMemcpyAsync` host -> device into the gradient buffer, a replayed
// optimizer graph read — on one rank in ~1 of 50 eight-rank runs sharing one GPU — the PREVIOUS (local, un-reduced) gradient of
// the tensor the backward pass had written last: lines still valid in an L2 that the copy engine's writes to memory do not update.
__global__ __launch_bounds__(256) void copy_f32_kernel(float* __restrict__ dst, const float* __restrict__ src, int64_t n, int vec) {
  if (vec) {
    const int64_t n4 = n >> 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256)
      ((float4*)dst)[i] = ((const float4*)src)[i];
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) dst[(n4 << 2) + threadIdx.x] = src[(n4 << 2) + threadIdx.x];
  } else {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) dst[i] = src[i];
  }
}

extern "C" int imm_copy_f32(float* dst, const float* src, int64_t n, void* stream) {
  IMM_REQUIRE(dst && src && n > 0 && ((uintptr_t)dst % 4 == 0) && ((uintptr_t)src % 4 == 0), "copy_f32: args");
  const int vec = ((uintptr_t)dst % 16 == 0) && ((uintptr_t)src % 16 == 0);        // (a bucket of the flat buffer may start anywhere)
  int64_t blocks = ((vec ? n / 4 : n) + 255) / 256;
  if (blocks < 1) blocks = 1;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(copy_f32_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, dst, src, n, vec);
  IMM_CHECK_LAUNCH("imm_copy_f32");
  return 0;
}

extern "C" int imm_crc32c(const void* data, uint64_t n, uint32_t* crc_inout) {
  IMM_REQUIRE(crc_inout && (data || n == 0), "crc32c: null pointer");
  static const Crc32cTables tab;
  const uint8_t* p = (const uint8_t*)data;
  uint32_t c = ~*crc_inout;
  while (n && ((uintptr_t)p & 7)) { c = (c >> 8) ^ tab.t[0][(c ^ *p++) & 0xff]; --n; }
  while (n >= 8) {
    uint64_t v = *(const uint64_t*)p;      // p is 8-byte aligned here
    v ^= c;
    c = tab.t[7][v & 0xff] ^ tab.t[6][(v >> 8) & 0xff] ^ tab.t[5][(v >> 16) & 0xff] ^ tab.t[4][(v >> 24) & 0xff] ^
        tab.t[3][(v >> 32) & 0xff] ^ tab.t[2][(v >> 40) & 0xff] ^ tab.t[1][(v >> 48) & 0xff] ^ tab.t[0][(v >> 56) & 0xff];
    p += 8; n -= 8;
  }
  while (n) { c = (c >> 8) ^ tab.t[0][(c ^ *p++) & 0xff]; --n; }
  *crc_inout = ~c;
  return 0;
}

// ---------------------------------------------------------------------------------------------
// workspace sizes (bytes) of the caller-allocated scratch buffers: thin twins of the row-count queries
// ---------------------------------------------------------------------------------------------
extern "C" int64_t imm_conv2d_workspace_bytes(const imm_conv_desc* d) {
  if (!d) return IMM_E_INVALID;
  if (!(d->flags & IMM_CONV_STATS)) return 0;
  const int rows = imm_conv_stats_blocks(d);
  return rows < 0 ? rows : (int64_t)rows * 2 * d->co * 4;
}
extern "C" int64_t imm_conv2d_group_workspace_bytes(const imm_conv_desc* descs, int n) {
  if (!descs || n < 1) return IMM_E_INVALID;
  if (!(descs[0].flags & IMM_CONV_STATS)) return 0;
  const int rows = imm_conv2d_group_stats_blocks(descs, n);
  return rows < 0 ? rows : (int64_t)rows * 2 * descs[0].co * 4;
}
extern "C" int64_t imm_conv2d_wgrad_workspace_bytes(const imm_conv_desc* d, int lddy, int nsplit) {
  if (!d) return IMM_E_INVALID;
  const int forced = imm_conv2d_wgrad_splits(d, lddy);
  if (forced < 0) return forced;
  const int ns = forced > 0 ? forced : (nsplit > 0 ? nsplit : 1);
  return (int64_t)ns * d->kpad * d->co * 4;
}
extern "C" int64_t imm_colsum_workspace_bytes(int64_t npix, int c) {
  const int rows = imm_colsum_blocks(npix, c);
  return rows < 0 ? rows : (int64_t)rows * c * 4;
}
extern "C" int64_t imm_bn_bwd_workspace_bytes(int64_t npix, int c) {
  const int rows = imm_bn_bwd_blocks(npix, c);
  return rows < 0 ? rows : (int64_t)rows * 2 * c * 4;
}
extern "C" int64_t imm_upsample2x_bwd_bn_workspace_bytes(int batch, int h, int w, int c) {
  const int rows = imm_upsample2x_bwd_bn_blocks(batch, h, w, c);
  return rows < 0 ? rows : (int64_t)rows * 2 * c * 4;
}
extern "C" int64_t imm_masked_sse_workspace_bytes(int nfeat) { return nfeat > 0 ? (int64_t)nfeat * IMM_SSE_BLOCKS * 4 : IMM_E_INVALID; }
