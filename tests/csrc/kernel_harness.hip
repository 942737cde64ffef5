// Test-only C entry points (e2ekt_*) around the launch wrappers of e2e_tts_amd/csrc/kernels.h, so that a test can call
// one kernel at one shape and compare every output element with a float64 reference (tests/kernel_ref.py).  Thin on purpose: flat scalar
// and pointer arguments in, the wrapper's own `const char*` (nullptr = launched) out, on the stream given.  Linked with the library's
// non-engine objects into libe2etts_kernels_test.so; the product libraries do not contain it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

#ifndef E2EKT_SRC_HASH
#define E2EKT_SRC_HASH "unknown"
#endif
#define KT_API extern "C" __attribute__((visibility("default")))

using namespace e2etts;

// staleness marker of this library (build() compares it with the hash of the kernel sources + this file)
KT_API const char* e2ekt_version() { return "E2EKT_SRC_HASH=" E2EKT_SRC_HASH; }

// ---- convolutions on ConvParams
#define CONV_ARGS                                                                                                                       \
  const float *in, const float *w, const float *wfrag, const float *bias, const float *res, float *out, const int32_t *lens,           \
      const int32_t *act_rows, const int32_t *act_rows_host, int B, int T, int Cin, int Cout, int KW, int dil, int pad, long long in_bs, \
      long long out_bs, long long res_bs, int in_ld, int out_ld, int res_ld, int x3, int zero_tap_split, float in_slope, int act,       \
      float act_slope, int accumulate, float out_div
#define CONV_PASS                                                                                                                    \
  in, w, wfrag, bias, res, out, lens, act_rows, act_rows_host, B, T, Cin, Cout, KW, dil, pad, in_bs, out_bs, res_bs, in_ld, out_ld,   \
      res_ld, x3, zero_tap_split, in_slope, act, act_slope, accumulate, out_div

static ConvParams conv_params(CONV_ARGS) {
  ConvParams p;
  p.in = in; p.w = w; p.wfrag = wfrag; p.bias = bias; p.res = res; p.out = out;
  p.lens = lens; p.act_rows = act_rows; p.act_rows_host = act_rows_host;
  p.B = B; p.T = T; p.Cin = Cin; p.Cout = Cout; p.KW = KW; p.dil = dil; p.pad = pad;
  p.in_bs = in_bs; p.out_bs = out_bs; p.res_bs = res_bs; p.in_ld = in_ld; p.out_ld = out_ld; p.res_ld = res_ld;
  p.x3 = x3; p.zero_tap_split = zero_tap_split; p.in_slope = in_slope; p.act = act; p.act_slope = act_slope;
  p.accumulate = accumulate; p.out_div = out_div;
  return p;
}
KT_API const char* e2ekt_conv_gemm(CONV_ARGS, void* stream) { return launch_conv_gemm(conv_params(CONV_PASS), (hipStream_t)stream); }
KT_API const char* e2ekt_conv_ksplit(CONV_ARGS, void* stream) { return launch_conv_ksplit(conv_params(CONV_PASS), (hipStream_t)stream); }
KT_API const char* e2ekt_conv_rows(CONV_ARGS, void* stream) { return launch_conv_rows(conv_params(CONV_PASS), (hipStream_t)stream); }
KT_API const char* e2ekt_conv_gemm_class(CONV_ARGS) { return conv_gemm_class(conv_params(CONV_PASS)); }
KT_API int e2ekt_conv_ksplit_supported(CONV_ARGS) { return conv_ksplit_supported(conv_params(CONV_PASS)) ? 1 : 0; }
KT_API int e2ekt_conv_rows_supported(CONV_ARGS) { return conv_rows_supported(conv_params(CONV_PASS)) ? 1 : 0; }

// ---- conv_bf16 on BConvParams
#define BCONV_ARGS                                                                                                                        \
  const void *in, int in_bf16, float in_slope, const float *in_add0, const float *in_add1, const float *in_add2, float in_div,           \
      const void *wimg, int KWe, int tap_split, const float *bias, float act_slope, const float *res, int accumulate, float out_div,     \
      float *out, void *out_b, float outb_slope, int B, int T, int Cin, int Cout, int KW, int dil, int pad, int rows_hint, int act16
#define BCONV_PASS                                                                                                                      \
  in, in_bf16, in_slope, in_add0, in_add1, in_add2, in_div, wimg, KWe, tap_split, bias, act_slope, res, accumulate, out_div, out, out_b, \
      outb_slope, B, T, Cin, Cout, KW, dil, pad, rows_hint, act16

static BConvParams bconv_params(BCONV_ARGS) {
  BConvParams p;
  p.in = in; p.in_bf16 = in_bf16; p.in_slope = in_slope;
  p.in_add[0] = in_add0; p.in_add[1] = in_add1; p.in_add[2] = in_add2; p.in_div = in_div;
  p.wimg = wimg; p.KWe = KWe; p.tap_split = tap_split; p.bias = bias; p.act_slope = act_slope; p.res = res;
  p.accumulate = accumulate; p.out_div = out_div; p.out = out; p.out_b = out_b; p.outb_slope = outb_slope;
  p.B = B; p.T = T; p.Cin = Cin; p.Cout = Cout; p.KW = KW; p.dil = dil; p.pad = pad; p.rows_hint = rows_hint; p.act16 = act16;
  return p;
}
KT_API const char* e2ekt_conv_bf16(BCONV_ARGS, void* stream) { return launch_conv_bf16(bconv_params(BCONV_PASS), (hipStream_t)stream); }
KT_API int e2ekt_conv_bf16_supported(BCONV_ARGS) { return conv_bf16_supported(bconv_params(BCONV_PASS)) ? 1 : 0; }
KT_API const char* e2ekt_conv_bf16_class(BCONV_ARGS) { return conv_bf16_class(bconv_params(BCONV_PASS)); }

// ---- weight images
KT_API size_t e2ekt_x3_frag_bytes(int Cout, int KW, int Cin) { return x3_frag_bytes(Cout, KW, Cin); }
KT_API const char* e2ekt_x3_to_frag(const float* x3, float* frag, int Cout, int KW, int Cin, void* stream) {
  return launch_x3_to_frag(x3, frag, Cout, KW, Cin, (hipStream_t)stream);
}
KT_API const char* e2ekt_f32_to_frag(const float* w, float* frag, int Cout, int KW, int Cin, void* stream) {
  return launch_f32_to_frag(w, frag, Cout, KW, Cin, (hipStream_t)stream);
}
KT_API size_t e2ekt_bf16_image_bytes(int Cout, int KW, int Cin, int tap_split) { return bf16_image_bytes(Cout, KW, Cin, tap_split); }
KT_API const char* e2ekt_bf16_image(const float* x3, void* img, int Cout, int KW, int Cin, int tap_split, void* stream) {
  return launch_bf16_image(x3, img, Cout, KW, Cin, tap_split, (hipStream_t)stream);
}
KT_API const char* e2ekt_f16_image(const float* w, void* img, int Cout, int KW, int Cin, int tap_split, void* stream) {
  return launch_f16_image(w, img, Cout, KW, Cin, tap_split, (hipStream_t)stream);
}

// ---- attention, LayerNorm
KT_API const char* e2ekt_attention(const float* qkv, float* out, const int32_t* lens, int B, int N, int H, int n_head, int x3, void* stream,
                                   const int32_t* lens_host, float* ws, size_t ws_bytes) {
  return launch_attention(qkv, out, lens, B, N, H, n_head, x3, (hipStream_t)stream, lens_host, ws, ws_bytes);
}
KT_API size_t e2ekt_attention_workspace_bytes(int B, int N, int H, int n_head) { return attention_workspace_bytes(B, N, H, n_head); }
KT_API long long e2ekt_attention_par_max_grid() { return attention_par_max_grid(); }
KT_API const char* e2ekt_rel_attention(const float* qkv, const float* pos, int pos_rows, const float* u, const float* v, float* out, int B,
                                       int N, int H, int n_head, void* stream, const float* pos_x3) {
  return launch_rel_attention(qkv, pos, pos_rows, u, v, out, B, N, H, n_head, (hipStream_t)stream, pos_x3);
}
KT_API const char* e2ekt_layernorm(const float* x, float* y, const float* gamma, const float* beta, const int32_t* lens, int B, int N, int C,
                                   float eps, void* stream) {
  return launch_layernorm(x, y, gamma, beta, lens, B, N, C, eps, (hipStream_t)stream);
}

// ---- fused ResBlocks
KT_API int e2ekt_resblock_pair_supported(int C, int KW, int dil) { return resblock_pair_supported(C, KW, dil) ? 1 : 0; }
static PairParams pair_params(const float* x, const float* wfrag, const float* b1, const float* b2, float* out, const int32_t* act_rows,
                              const int32_t* act_rows_host, int B, int T, int C, int KW, int dil, long long x_bs, long long out_bs, float slope,
                              int accumulate, float out_div, int mode, const void* bimg1, const void* bimg2) {
  PairParams p;
  p.x = x; p.wfrag = wfrag; p.b1 = b1; p.b2 = b2; p.out = out; p.act_rows = act_rows; p.act_rows_host = act_rows_host;
  p.B = B; p.T = T; p.C = C; p.KW = KW; p.dil = dil; p.x_bs = x_bs; p.out_bs = out_bs; p.slope = slope;
  p.accumulate = accumulate; p.out_div = out_div; p.mode = mode; p.bimg1 = bimg1; p.bimg2 = bimg2;
  return p;
}
#define PAIR_ARGS                                                                                                                      \
  const float *x, const float *wfrag, const float *b1, const float *b2, float *out, const int32_t *act_rows,                            \
      const int32_t *act_rows_host, int B, int T, int C, int KW, int dil, long long x_bs, long long out_bs, float slope, int accumulate, \
      float out_div, int mode, const void *bimg1, const void *bimg2
#define PAIR_PASS x, wfrag, b1, b2, out, act_rows, act_rows_host, B, T, C, KW, dil, x_bs, out_bs, slope, accumulate, out_div, mode, bimg1, bimg2
KT_API const char* e2ekt_resblock_pair(PAIR_ARGS, void* stream) { return launch_resblock_pair(pair_params(PAIR_PASS), (hipStream_t)stream); }
KT_API const char* e2ekt_pair_bf16(PAIR_ARGS, void* stream) { return launch_pair_bf16(pair_params(PAIR_PASS), (hipStream_t)stream); }
KT_API int e2ekt_pair_bf16_supported(PAIR_ARGS) { return pair_bf16_supported(pair_params(PAIR_PASS)) ? 1 : 0; }

KT_API int e2ekt_resblock_chain_supported(int C, int KW, const int* dil, int n_dil) { return resblock_chain_supported(C, KW, dil, n_dil) ? 1 : 0; }
// b1 / b2: three pointers each; dil: three dilations
KT_API const char* e2ekt_resblock_chain(const float* x, const float* wfrag, const float* const* b1, const float* const* b2, float* out,
                                        const int32_t* act_rows, const int32_t* act_rows_host, int B, int T, int C, int KW, const int* dil,
                                        long long x_bs, long long out_bs, float slope, int accumulate, float out_div, int mode, void* stream) {
  ChainParams p;
  p.x = x; p.wfrag = wfrag; p.out = out; p.act_rows = act_rows; p.act_rows_host = act_rows_host;
  for (int m = 0; m < 3; ++m) { p.b1[m] = b1[m]; p.b2[m] = b2[m]; p.dil[m] = dil[m]; }
  p.B = B; p.T = T; p.C = C; p.KW = KW; p.x_bs = x_bs; p.out_bs = out_bs; p.slope = slope;
  p.accumulate = accumulate; p.out_div = out_div; p.mode = mode;
  return launch_resblock_chain(p, (hipStream_t)stream);
}

// n members; member i, pair m: bimg[(i * RB_MAX_PAIRS + m) * 2 + {0, 1}], b1 / b2 / dil[i * RB_MAX_PAIRS + m]; x / out / KW / accumulate /
// out_div per member, the rest shared
static void rb_params(RbParams* ps, int n, const float* const* x, float* const* out, const void* const* bimg, const float* const* b1,
                      const float* const* b2, const int* dil, const int* KW, const int* accumulate, const float* out_div, int n_pairs, int B, int T,
                      int C, long long x_bs, long long out_bs, float slope, int act16) {
  for (int i = 0; i < n; ++i) {
    RbParams& p = ps[i];
    p.x = x[i]; p.out = out[i];
    for (int m = 0; m < RB_MAX_PAIRS; ++m) {
      p.bimg[m][0] = bimg[(i * RB_MAX_PAIRS + m) * 2]; p.bimg[m][1] = bimg[(i * RB_MAX_PAIRS + m) * 2 + 1];
      p.b1[m] = b1[i * RB_MAX_PAIRS + m]; p.b2[m] = b2[i * RB_MAX_PAIRS + m]; p.dil[m] = dil[i * RB_MAX_PAIRS + m];
    }
    p.n_pairs = n_pairs; p.B = B; p.T = T; p.C = C; p.KW = KW[i]; p.x_bs = x_bs; p.out_bs = out_bs; p.slope = slope;
    p.accumulate = accumulate[i]; p.out_div = out_div[i]; p.act16 = act16;
  }
}
#define RB_ARGS                                                                                                                          \
  int n, const float *const *x, float *const *out, const void *const *bimg, const float *const *b1, const float *const *b2, const int *dil, \
      const int *KW, const int *accumulate, const float *out_div, int n_pairs, int B, int T, int C, long long x_bs, long long out_bs,     \
      float slope, int act16
#define RB_PASS n, x, out, bimg, b1, b2, dil, KW, accumulate, out_div, n_pairs, B, T, C, x_bs, out_bs, slope, act16
KT_API int e2ekt_rb_bf16_supported(RB_ARGS) {
  RbParams ps[BC_GROUP_MAX];
  if (n < 1 || n > BC_GROUP_MAX) return 0;
  rb_params(ps, RB_PASS);
  for (int i = 0; i < n; ++i)
    if (!rb_bf16_supported(ps[i])) return 0;
  return 1;
}
KT_API const char* e2ekt_rb_bf16_group(RB_ARGS, void* stream) {
  RbParams ps[BC_GROUP_MAX];
  if (n < 1 || n > BC_GROUP_MAX) return "e2ekt_rb_bf16_group: 1 .. 4 members";
  rb_params(ps, RB_PASS);
  return launch_rb_bf16_group(ps, n, (hipStream_t)stream);
}
KT_API int e2ekt_rb_bf16_stage_supported(RB_ARGS) {
  RbParams ps[BC_GROUP_MAX];
  if (n < 1 || n > BC_GROUP_MAX) return 0;
  rb_params(ps, RB_PASS);
  return rb_bf16_stage_supported(ps, n) ? 1 : 0;
}
KT_API const char* e2ekt_rb_bf16_stage(RB_ARGS, void* stream) {
  RbParams ps[BC_GROUP_MAX];
  if (n < 1 || n > BC_GROUP_MAX) return "e2ekt_rb_bf16_stage: 1 .. 4 members";
  rb_params(ps, RB_PASS);
  return launch_rb_bf16_stage(ps, n, (hipStream_t)stream);
}

// ---- small kernels
KT_API const char* e2ekt_conv_post(const float* x, const float* w, const float* bias, float* wav, int16_t* pcm, int B, long long N, int C, int KW,
                                   void* stream, const int32_t* act_rows, const int32_t* act_rows_host, const float* const* x_add, float x_div) {
  return launch_conv_post(x, w, bias, wav, pcm, B, N, C, KW, (hipStream_t)stream, act_rows, act_rows_host, x_add, x_div);
}
KT_API const char* e2ekt_dwconv_swish(const float* in, const float* w, const float* bias, float* out, int B, int N, int C, int k, void* stream) {
  return launch_dwconv_swish(in, w, bias, out, B, N, C, k, (hipStream_t)stream);
}
// *fused_out: 1 when the one-pass kernel ran, 0 when the two-kernel form did
KT_API const char* e2ekt_dwconv_glu_swish(const float* in, const float* w, const float* bias, float* out, float* scratch, int B, int N, int C,
                                          int k, void* stream, int* fused_out) {
  bool fused = false;
  const char* e = launch_dwconv_glu_swish(in, w, bias, out, scratch, B, N, C, k, (hipStream_t)stream, &fused);
  if (fused_out) *fused_out = fused ? 1 : 0;
  return e;
}
KT_API const char* e2ekt_glu(const float* in, float* out, long long rows, int C, void* stream) { return launch_glu(in, out, rows, C, (hipStream_t)stream); }
