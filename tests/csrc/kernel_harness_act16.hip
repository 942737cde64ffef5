// Test-only C entry points (e2ekt_*) of libe2etts_kernels_test.so for the group launchers of conv_bf16.hip and for launch_conv_post_bf16: a
// second source beside kernel_harness.hip, linked into the same library, with a staleness marker of its own (e2ekt_act16_version), so that
// the marker of kernel_harness.hip keeps saying what that file says.  Thin on purpose, as kernel_harness.hip is: flat arguments in, the
// wrapper's own `const char*` (nullptr = launched) out, on the stream given.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

#ifndef E2EKT_A16_SRC_HASH
#define E2EKT_A16_SRC_HASH "unknown"
#endif
#define KT_API extern "C" __attribute__((visibility("default")))

using namespace e2etts;

// staleness marker of this file (build() compares it with the hash of the kernel sources + this file)
KT_API const char* e2ekt_act16_version() { return "E2EKT_A16_SRC_HASH=" E2EKT_A16_SRC_HASH; }

// n members of launch_conv_bf16_group: every field of BConvParams but rows_hint (the group's own) as an array of n -- B, T, Cin, Cout,
// in_bf16 and act16 too, so that a test can hand over a mixed group and see it refused
KT_API const char* e2ekt_conv_bf16_group(int n, const void* const* in, const int* in_bf16, const float* in_slope, const float* const* in_add0,
                                         const float* const* in_add1, const float* const* in_add2, const float* in_div, const void* const* wimg,
                                         const int* KWe, const int* tap_split, const float* const* bias, const float* act_slope,
                                         const float* const* res, const int* accumulate, const float* out_div, float* const* out, void* const* out_b,
                                         const float* outb_slope, const int* B, const int* T, const int* Cin, const int* Cout, const int* KW,
                                         const int* dil, const int* pad, const int* act16, void* stream) {
  BConvParams ps[BC_GROUP_MAX];
  if (n < 1 || n > BC_GROUP_MAX) return "e2ekt_conv_bf16_group: 1 .. 4 members";
  for (int i = 0; i < n; ++i) {
    BConvParams& p = ps[i];
    p.in = in[i]; p.in_bf16 = in_bf16[i]; p.in_slope = in_slope[i];
    p.in_add[0] = in_add0[i]; p.in_add[1] = in_add1[i]; p.in_add[2] = in_add2[i]; p.in_div = in_div[i];
    p.wimg = wimg[i]; p.KWe = KWe[i]; p.tap_split = tap_split[i]; p.bias = bias[i]; p.act_slope = act_slope[i]; p.res = res[i];
    p.accumulate = accumulate[i]; p.out_div = out_div[i]; p.out = out[i]; p.out_b = out_b[i]; p.outb_slope = outb_slope[i];
    p.B = B[i]; p.T = T[i]; p.Cin = Cin[i]; p.Cout = Cout[i]; p.KW = KW[i]; p.dil = dil[i]; p.pad = pad[i]; p.rows_hint = 0; p.act16 = act16[i];
  }
  return launch_conv_bf16_group(ps, n, (hipStream_t)stream);
}

// n members of launch_pair_bf16_group: dense tensors (x_bs = out_bs = T * C), no fragment weights, no act_rows; the rest as arrays of n
KT_API const char* e2ekt_pair_bf16_group(int n, const float* const* x, const float* const* b1, const float* const* b2, float* const* out, const int* B,
                                         const int* T, const int* C, const int* KW, const int* dil, const float* slope, const int* accumulate,
                                         const float* out_div, const int* mode, const void* const* bimg1, const void* const* bimg2, void* stream) {
  PairParams ps[BC_GROUP_MAX];
  if (n < 1 || n > BC_GROUP_MAX) return "e2ekt_pair_bf16_group: 1 .. 4 members";
  for (int i = 0; i < n; ++i) {
    PairParams& p = ps[i];
    p.x = x[i]; p.wfrag = nullptr; p.b1 = b1[i]; p.b2 = b2[i]; p.out = out[i]; p.act_rows = nullptr; p.act_rows_host = nullptr;
    p.B = B[i]; p.T = T[i]; p.C = C[i]; p.KW = KW[i]; p.dil = dil[i]; p.x_bs = (long long)T[i] * C[i]; p.out_bs = (long long)T[i] * C[i];
    p.slope = slope[i]; p.accumulate = accumulate[i]; p.out_div = out_div[i]; p.mode = mode[i]; p.bimg1 = bimg1[i]; p.bimg2 = bimg2[i];
  }
  return launch_pair_bf16_group(ps, n, (hipStream_t)stream);
}

KT_API const char* e2ekt_conv_post_bf16(const void* x, const float* w16, const float* bias16, float* wav, int16_t* pcm, int B, long long N, int C,
                                        int KW, void* stream, int fp16) {
  return launch_conv_post_bf16(x, w16, bias16, wav, pcm, B, N, C, KW, (hipStream_t)stream, fp16 != 0);
}
