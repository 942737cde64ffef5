// The engine's common ground (engine.h): workspace buffers, the profiling records, the one conv / linear launch every pass goes through,
// copies between the caller's memory and the engine's.
#include "engine.h"

namespace e2etts {
namespace eng {

int ensure(e2etts_engine* e, DevBuf& b, size_t bytes) {
  if (bytes <= b.cap) return E2ETTS_OK;
  HIPCHK(e, hipStreamSynchronize(e->stream));
  if (b.p) {
    HIPCHK(e, hipFree(b.p));
    e->dev_bytes -= b.cap;
    b.p = nullptr;
    b.cap = 0;
  }
  if (std::find(e->owned.begin(), e->owned.end(), &b) == e->owned.end()) e->owned.push_back(&b);
  size_t want = (bytes + 255) & ~size_t(255);
  if (hipMalloc(&b.p, want) != hipSuccess) {
    b.p = nullptr;
    return e->fail(E2ETTS_ENOMEM, "hipMalloc(%zu bytes) failed", want);
  }
  b.cap = want;
  e->dev_bytes += want;
  // ragged mode leaves rows nobody needs uncomputed: make sure what they hold is at least finite
  HIPCHK(e, hipMemsetAsync(b.p, 0, want, e->stream));
  return E2ETTS_OK;
}

int prof_class(e2etts_engine* e, const char* name) {
  for (size_t i = 0; i < e->prof_stats.size(); ++i)
    if (!strcmp(e->prof_stats[i].name, name)) return (int)i;
  e2etts_kernel_stat s{};
  snprintf(s.name, sizeof s.name, "%s", name);
  e->prof_stats.push_back(s);
  return (int)e->prof_stats.size() - 1;
}

hipEvent_t get_event(e2etts_engine* e) {
  if (!e->ev_pool.empty()) {
    hipEvent_t ev = e->ev_pool.back();
    e->ev_pool.pop_back();
    return ev;
  }
  hipEvent_t ev = nullptr;
  (void)hipEventCreate(&ev);
  return ev;
}

// The plain-bf16 mode's convolutions on conv_bf16.hip (bit-identical to conv_gemm's mode 2, so the choice is per launch): a padded
// batch, dense rows, an activation that is a slope.  (tuning().bconv: off keeps them on conv_gemm.)
bool bconv_params(const ConvParams& p, BConvParams& q) {
  if (!tuning().bconv || p.x3 != 2 || !p.bimg || p.act_rows || p.lens) return false;
  if (p.act != ACT_NONE && p.act != ACT_RELU && p.act != ACT_LRELU) return false;
  if (p.in_ld != p.Cin || p.out_ld != p.Cout || (p.res && p.res_ld != p.Cout)) return false;
  if (p.in_bs != (long long)p.T * p.Cin || p.out_bs != (long long)p.T * p.Cout || (p.res && p.res_bs != p.out_bs)) return false;
  if (p.bimg_tap_split != p.zero_tap_split) return false;
  q = BConvParams();
  q.in = p.in; q.in_bf16 = p.in_bf16; q.in_slope = p.in_slope; q.wimg = p.bimg; q.tap_split = p.bimg_tap_split;
  for (int k = 0; k < 3; ++k) q.in_add[k] = p.in_add[k];
  q.in_div = p.in_div;
  q.KWe = p.bimg_tap_split > 0 ? 2 : p.KW;
  q.bias = p.bias; q.act_slope = p.act == ACT_LRELU ? p.act_slope : (p.act == ACT_RELU ? 0.f : 1.f);
  q.res = p.res; q.accumulate = p.accumulate; q.out_div = p.out_div; q.out = p.out; q.out_b = p.out_b; q.outb_slope = p.outb_slope;
  q.B = p.B; q.T = p.T; q.Cin = p.Cin; q.Cout = p.Cout; q.KW = p.KW; q.dil = p.dil; q.pad = p.pad;
  return conv_bf16_supported(q);
}

// E2ETTS_PROFILE_FINE (set at all, in the product library too): one profile class per layer shape instead of per kernel configuration.
// It names profile classes and selects nothing.
bool profile_fine() {
  static const bool fine = getenv("E2ETTS_PROFILE_FINE") != nullptr;
  return fine;
}

// One conv / linear launch.  alg_scale < 1 when part of the packed weight is structural zeros
// (the polyphase upsampler) so that the recorded FLOPs stay the algorithmic ones.
// ksplit: a phoneme-level layer (encoder FFT blocks, predictors): served by conv_ksplit.hip at every batch size when its fp32 fragment
// image exists
int conv(e2etts_engine* e, ConvParams p, double alg_scale, bool ksplit) {
  if (p.in_ld == 0) p.in_ld = p.Cin;
  if (p.out_ld == 0) p.out_ld = p.Cout;
  if (p.res && p.res_ld == 0) p.res_ld = p.Cout;
  if (p.in_bs == 0) p.in_bs = (long long)p.T * p.in_ld;
  if (p.out_bs == 0) p.out_bs = (long long)p.T * p.out_ld;
  if (p.res && p.res_bs == 0) p.res_bs = (long long)p.T * p.res_ld;
  if (!p.wfrag) {  // fragment-order image of these weights (split-precision image or fp32 tensor: the map is keyed by pointer)
    auto it = e->frag_of.find(p.w);
    if (it != e->frag_of.end()) p.wfrag = it->second;
  }
  const bool fine = profile_fine();
  char fname[48];
  if (fine && e->prof_on)
    snprintf(fname, sizeof fname, "%s %d>%d k%d d%d r%lld%s%s", p.x3 ? "x3" : "f32", p.Cin, p.Cout, p.KW, p.dil,
             (long long)p.B * p.T, p.res ? "+r" : "", p.accumulate ? "+a" : "");
  {
    BConvParams q;
    if (bconv_params(p, q)) {
      ProfScope ps(e, fine && e->prof_on ? fname : conv_bf16_class(q), conv_gemm_flops(p) * alg_scale, conv_gemm_bytes(p));
      KCHK(e, launch_conv_bf16(q, e->stream));
      return E2ETTS_OK;
    }
    if (p.in_bf16 || p.out_b || p.in_add[0]) return e->fail(E2ETTS_EINVAL, "bf16 hand-over / joined input asked of a launch conv_bf16 does not serve");
  }
  // ... and only where the chain is long (K = KW x Cin >= 768: the FFN convolutions, the predictors): a q | k | v or fc projection
  // (K = 384) is a chain of 12 short links, and at B = 32 the split costs those more (three idle waves per epilogue) than it saves.
  // The choice is by layer shape, never by batch size, so every batch size sums every layer in the same order.
  if (ksplit && (long long)((p.Cin + 31) / 32) * p.KW >= 24 && conv_ksplit_supported(p)) {
    ProfScope ps(e, fine && e->prof_on ? fname : "conv_ksplit", conv_gemm_flops(p) * alg_scale, conv_gemm_bytes(p));
    KCHK(e, launch_conv_ksplit(p, e->stream));
    return E2ETTS_OK;
  }
  // few rows (small batches, the B = 1 latency path) on fragment-order weights: conv_rows -- conv_gemm's arithmetic, MFMA for MFMA, with
  // one wavefront per 32-row tile and no workgroup barrier (conv_ksplit.hip).  Same bits: tuning().rows changes speed only.
  // Taken where it measured ahead: convolutions (KW >= 3: a k = 1 Linear stages a slab per 6 MFMAs here, conv_gemm's multi-chunk items do
  // better) on grids of at most one 64 x 64 workgroup per CU -- B = 1: the decoder's k = 9 convolution 63 -> 40 us, the postnet's 52 -> 36;
  // at B = 4 conv_gemm's several workgroups per CU already hide what this kernel avoids.
  const long long wg64 = (long long)((p.T + 63) / 64) * p.B * ((p.Cout + 63) / 64);
  if (tuning().rows && p.KW >= 3 && wg64 <= 256 && tile_few_rows(p.B, p.T, p.Cout) && conv_rows_supported(p)) {
    ProfScope ps(e, fine && e->prof_on ? fname : (p.x3 ? "conv_x3_rows" : "conv_rows"), conv_gemm_flops(p) * alg_scale, conv_gemm_bytes(p));
    KCHK(e, launch_conv_rows(p, e->stream));
    return E2ETTS_OK;
  }
  ProfScope ps(e, fine && e->prof_on ? fname : conv_gemm_class(p), conv_gemm_flops(p) * alg_scale, conv_gemm_bytes(p));
  KCHK(e, launch_conv_gemm(p, e->stream));
  return E2ETTS_OK;
}

bool is_device_pointer(const void* p) {
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return attr.type == hipMemoryTypeDevice;
}

int copy_in(e2etts_engine* e, void* dst, const void* src, size_t bytes) {
  HIPCHK(e, hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, e->stream));
  return E2ETTS_OK;
}

int size_act(e2etts_engine* e, int B, bool dev, bool host) {
  const size_t n = (size_t)ActSlots{e->cfg.voc_stages}.count() * B;
  if (dev) RET(ensure(e, e->actbuf, n * 4));
  if (host) e->h_act.resize(n, 0);
  return E2ETTS_OK;
}

}  // namespace eng
}  // namespace e2etts
