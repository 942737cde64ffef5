// Test-only C entry points (e2ekt_*) of libe2etts_kernels_test.so around the launch wrappers of csrc/fastformer.hip (the additive-attention
// pool with its workspace queries, and the scale / residual pass): a sixth source beside kernel_harness.hip, kernel_harness_act16.hip,
// forced_harness.hip, small_harness.hip and denoiser_harness.hip, linked into the same library, with a staleness marker of its own
// (e2ekt_fastformer_version).  Thin on purpose: flat arguments in, the wrapper's own `const char*` (nullptr = launched) out, on the stream given.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

#ifndef E2EKT_FF_SRC_HASH
#define E2EKT_FF_SRC_HASH "unknown"
#endif
#define KT_API extern "C" __attribute__((visibility("default")))

using namespace e2etts;

KT_API const char* e2ekt_fastformer_version() { return "E2EKT_FF_SRC_HASH=" E2EKT_FF_SRC_HASH; }

KT_API const char* e2ekt_ff_pool(const float* v, int v_ld, const float* scale, const float* wl, const float* bl, const int32_t* lens, float* out,
                                 float* ws, size_t ws_bytes, int B, int N, int H, int head_size, void* stream) {
  return launch_ff_pool(v, v_ld, scale, wl, bl, lens, out, ws, ws_bytes, B, N, H, head_size, (hipStream_t)stream);
}

KT_API const char* e2ekt_ff_scale(const float* q, int q_ld, const float* gk, const float* x, float* wv, float* qx, int B, int N, int H,
                                  void* stream) {
  return launch_ff_scale(q, q_ld, gk, x, wv, qx, B, N, H, (hipStream_t)stream);
}

KT_API size_t e2ekt_ff_pool_workspace_bytes(int B, int N, int H, int head_size) { return ff_pool_workspace_bytes(B, N, H, head_size); }

KT_API int e2ekt_ff_pool_splits(int B, int N, int H, int head_size) { return ff_pool_splits(B, N, H, head_size); }
