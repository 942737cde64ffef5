// Engine + C ABI (include/e2etts.h): owns the weights, the workspace, one HIP stream, and sequences the
// kernels of kernels.h into the reference's inference path
//   UnsupervisedFastSpeech2.inference (reference U/model.py:155-194)  ->  HifiGan.forward (V/generator.py:37-53)
// exactly as TTS.inference drives them per batch (API/utils.py:130-148).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include <dlfcn.h>

#include "../../include/e2etts.h"
#include "host_logic.h"
#include "forced_entry.h"
#ifndef E2ETTS_ST_DEPTH
#define E2ETTS_ST_DEPTH 2   // chunks the streaming vocoder keeps in flight (tuning builds: 3)
#endif
#include "kernels.h"
#include "tuning.h"

using namespace e2etts;

namespace {

thread_local std::string g_create_error;

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
};

struct FFTLayer {
  const float *wqkv, *bqkv, *wo, *bo, *ln1g, *ln1b, *w1, *b1, *w2, *b2, *ln2g, *ln2b;
  const float *wqkv_x3 = nullptr, *wo_x3 = nullptr, *w1_x3 = nullptr, *w2_x3 = nullptr;  // optional split-precision images
};
// Conformer block (U/blocks/conformer.py:171-255), as packed by packer._pack_conformer
struct CfGemm {
  const float *w = nullptr, *b = nullptr, *wx3 = nullptr;
};
struct CfLayer {
  const float *ff_lng[2], *ff_lnb[2];
  CfGemm ff_a[2], ff_b[2];  // FeedForwardModule x 2: Linear(H -> F), Linear(F -> H) (half-step factor folded in)
  const float *att_lng, *att_lnb, *att_u, *att_v;
  CfGemm att_qkv, att_o;
  const float* pos[2];  // pos_proj(table) per head [n_head][rows][d_head]: stored / regenerated table
  const float* posx[2] = {nullptr, nullptr};  // the same as bf16 hi | lo rows (decoder, optional): the split-precision attention kernel's operand
  uint64_t pos_rows[2];
  const float *cv_lng, *cv_lnb, *dw_w, *dw_b;
  CfGemm pw1, pw2;
  const float *lng, *lnb;
};
// Fastformer layer (U/blocks/fastformer.py:144-175), as packed by packer._pack_fastformer
struct FfLayer {
  const float *att_lng, *att_lnb, *ffn_lng, *ffn_lnb;
  CfGemm qk, wt, w1, w2;  // query | key (H -> 2H), transform, FFN conv k -> GELU -> conv 1
};
struct FfSide {
  std::vector<FfLayer> layers;
  const float *wql = nullptr, *bql = nullptr, *wkl = nullptr, *bkl = nullptr;  // the logit layers, tied across the layers (:161-165); [H][heads]
  int head_size = 0;  // = n_head / dec_n_head of the config: the block runs hidden / n_head heads of that size (:190-191)
};
struct PredLayer {
  const float *w, *b, *g, *beta;
};
struct Predictor {
  std::vector<PredLayer> layers;
  const float *lin_w = nullptr, *lin_b = nullptr, *alpha = nullptr;
  int kernel = 0, chans = 0, odim = 0;
};
struct ConvW {
  const float *w = nullptr, *b = nullptr;
  const float* wx3 = nullptr;  // split-precision (bf16 hi | lo) image, when the blob carries one
};

struct ProfRec {
  hipEvent_t start, stop;
  int cls;
  double flops, bytes;
};

}  // namespace

struct e2etts_engine {
  e2etts_config cfg{};
  int device = 0;
  hipStream_t stream = nullptr;
  std::mutex mu;
  std::string err;
  size_t dev_bytes = 0;

  std::vector<DevBuf*> owned;  // every buffer ensure() has ever allocated (members of this struct); e2etts_destroy frees them

  // weights
  DevBuf blob;
  std::map<std::string, std::pair<const float*, uint64_t>> tensors;
  // split-precision image -> the same weights in MFMA-fragment order (built on the device at load time for the layers
  // the 128-column kernel serves: their waves read weight fragments straight from L2, no LDS tile, no barrier per tap)
  std::map<const float*, float*> frag_of;
  // split-precision image -> its hi halves in conv_bf16.hip's order (launch_bf16_image), for the vocoder's plain-bf16 mode; value: image
  // and the tap_split it was built with (polyphase upsamplers keep two taps per 32-column tile)
  std::map<const float*, std::pair<void*, int>> bimg_of;
  // precision "bf16_act" only: the images of the convolutions mode 2 does not stage from bimg_of (ResBlock2), and the bf16-rounded
  // copies (as fp32) of every vocoder bias and of conv_post's weights, keyed by the fp32 tensor; both built once at load
  std::map<const float*, std::pair<void*, int>> bimg_act;
  std::map<const float*, float*> r16_of;
  // precision "fp16_act" only, built at the FIRST selection of the mode (an engine that never selects it owns none of this): the fp16
  // images of every vocoder convolution, keyed by the fp32 weight tensor they are rounded from (launch_f16_image), and the fp16-rounded
  // copies (as fp32) of the biases and of conv_post's weights
  std::map<const float*, std::pair<void*, int>> himg_of;
  std::map<const float*, float*> r16h_of;
  size_t frag_bytes = 0;
  bool ac_loaded = false, voc_loaded = false;
  std::vector<FFTLayer> enc, dec;
  std::vector<CfLayer> cf_enc, cf_dec;  // cfg.block_type == 1
  FfSide ff_enc, ff_dec;                // cfg.block_type == 2
  Predictor dur, pitch, energy;
  const float *emb = nullptr, *enc_pos = nullptr, *dec_pos = nullptr, *pos_regen = nullptr, *spk_emb = nullptr;
  const float *var_pos = nullptr, *pitch_emb = nullptr, *energy_emb = nullptr, *energy_bins = nullptr, *pitch_bins = nullptr;
  uint64_t var_pos_rows = 0;
  ConvW mel_lin, voc_pre, voc_post;
  std::vector<ConvW> postnet, voc_up;
  std::vector<std::vector<ConvW>> rb_c1, rb_c2;  // [stage * n_kernels + j][dilation index]
  // fused ResBlock pairs (resblock_pair.hip): conv1's fragment-order image followed by conv2's, per [stage * n_kernels + j][m];
  // stage_fused[i]: every pair of stage i can run fused (channels 32 / 64 / 128)
  std::vector<std::vector<float*>> rb_pair_frag;
  std::vector<float*> rb_frag_base;  // the allocations rb_pair_frag points into (one per ResBlock)
  // the same for the exact-fp32 mode (launch_f32_to_frag order), built for the stages of <= 64 channels only: wider stages are bound by
  // the fp32 matrix pipe, where the fused kernel's (KW - 1) / BMI recompute costs more than its saved HBM traffic buys
  std::vector<std::vector<float*>> rb_pair_frag32;
  std::vector<char> stage_fused;
  int fuse_pairs = 2;  // e2etts_set_fused_resblocks: 0 off, 1 pairs, 2 pairs + whole k = 3 ResBlocks

  // workspace
  DevBuf ids, lens64, lens32, spk, xa, xb, xs, xp, tmp, qkv, att, hid, p1, p2, attws;
  DevBuf ffpool;  // Fastformer: pooled query | pooled key [2][B, H]
  DevBuf logd, durf, cum, mel64, mel32, posbuf, ppred, epred, pidx, eidx;
  DevBuf ctlbuf;  // [3][B * L] fp32: the d / p / e controls of the _ctl entry points (grows with B * L only)
  // e2etts_acoustic_forced: a host map's copy [B, T, L], the given mel lengths, the frame-resolved targets [3][B, T] awaiting their
  // per-phoneme means, the targets at the model's level [3][B, N] (f0 or pitch | uv | energy), the decoder's input (tap "dec_in")
  DevBuf fattn, fmel64, ftgf, ftg, decin;
  bool forced_last = false, forced_pitch = false, forced_energy = false;   // what the taps of the last acoustic pass can hand out
  int forced_T = 0;   // columns of its [B, T] targets
  DevBuf dx, dxb, mel, melpost, pn1, pn2;
  DevBuf melin;
  // Everything one vocoder pass works in besides the weights; vocoder_impl / vocoder_act16 are handed one and touch no other pass.  The
  // engine owns one for the one-shot calls and synthesize (`voc`: its stream is the engine's, its result the resident one), every
  // stream slot one, e2etts_denoiser_calibrate one.
  struct VocPass {
    hipStream_t stream = nullptr;   // the pass's compute stream: the engine is enqueuing on it (e->stream, see OnStream) while the pass runs
    DevBuf v0, v1, v2, v3;
    // small batches: the ResBlocks of a vocoder stage run side by side, ResBlock j > 0 on side stream j - 1 with buffers of its own
    // (stage sum, two ping-pong buffers); created on first use
    DevBuf vside[E2ETTS_MAX_RB_KERNELS - 1][3];
    hipStream_t side[E2ETTS_MAX_RB_KERNELS - 1] = {};
    hipEvent_t ev_fork = nullptr, ev_join[E2ETTS_MAX_RB_KERNELS - 1] = {};
    DevBuf wav, pcm;
    DevBuf istft_q, istft_ri, istft_sp;  // iSTFTNet tail: conv_post output, Re/Im per bin, exp / sin heads (tap "istft_spec_phase")
    int istft_B = 0;
    long long istft_F = 0;
    bool resident = false;   // a finished pass becomes the engine's resident result (have_wav, voc_B, voc_T): what fetches and taps read
  };
  VocPass voc;
  DevBuf tempo_in, tempo_out;  // e2etts_tempo
  int64_t* h_mel = nullptr;  // pinned
  int last_B = 0, last_L = 0, last_T = 0, voc_B = 0, voc_T = 0;
  bool have_acoustic = false, have_wav = false;
  int voc_precision = 0;  // 0: fp32 MFMA (default: the reference's arithmetic), 1: bf16x3 split-precision MFMA, 2: plain bf16, 3 / 4: bf16 / fp16
                          // activations (E2ETTS_PRECISION_*)
  // streaming vocoder (e2etts_vocoder_stream_*): trailing mel frames kept as context / not yet emitted
  DevBuf st_carry, st_win;
  int st_B = 0, st_carry_n = 0, st_halo = 0;
  long long st_emitted = 0;
  bool st_open = false, st_done = false;
  // denoised stream (e2etts_vocoder_stream_begin_denoised): every window carries st_delay more frames of context per side than the halo and
  // its waveform is denoised as a function of the window alone (denoise_stream_impl), so nothing of the denoiser is carried between chunks
  bool st_dn = false;
  float st_strength = 0.f;
  int st_delay = 0;
  long long st_abs0 = 0;   // absolute frame index of the carry's first frame
  // Two chunks may be in flight: _push enqueues and returns, _fetch takes the OLDEST unfetched chunk.  A chunk's pass depends on the mel
  // stream only (the carried context is mel frames), so the two passes are independent: each slot has a compute stream, a workspace and
  // output buffers of its own, and the kernels of chunk i + 1 fill the CUs that chunk i's launch tails and small launches leave idle.
  // Window assembly, uploads and downloads run on the engine's own stream, which carries no kernels while a stream is open (and is the
  // one e2etts_order_after orders behind the caller's work).  That makes three streams busy at a time: a process has FOUR hardware
  // queues by default (GPU_MAX_HW_QUEUES), the null stream holds one, and streams beyond that share a queue, i.e. run in turn --
  // measured: with a copy stream of its own the two passes landed on one queue and did not overlap at all.
  static constexpr int ST_DEPTH = E2ETTS_ST_DEPTH;
  struct StSlot {
    VocPass pass;   // (a stream of its own; the window's wav / PCM are pass.wav / pass.pcm)
    DevBuf win;
    DevBuf dn_pad, dn_spec, dn_ola, dn_lens, dn_wav, dn_pcm;   // a denoised stream: the slot's own denoiser workspace and denoised outputs
    void* pin = nullptr;
    size_t pin_cap = 0;
    hipEvent_t done = nullptr, win_ready = nullptr;
    int emit_n = 0, emit_off = 0, win_n = 0;
  } st_slot[ST_DEPTH];
  int st_head = 0, st_pending = 0;
  int ragged = 1;         // synthesize(): skip rows of shorter utterances that no valid output sample depends on
  bool rag_short = false; // the last acoustic pass had an utterance shorter than T (else ragged mode has nothing to skip)
  DevBuf actbuf;          // [5 + voc_stages][B] int32 row limits: decoder, mel_linear / postnet, vocoder stage 0 .. voc_stages, encoder (unused on the
                          // device: lens32 serves), variance predictors
  std::vector<int32_t> h_act;  // the same limits on the host, same layout (valid for the call that computed them): the launchers build
                               // their compact grids from them (kernels.h: RowMap)
  double rag_frac_dec = 1.0, rag_frac_post = 1.0, rag_frac_voc = 1.0;  // fraction of the padded rows those limits leave (profile FLOP counts)
  int dec_precision = 0;  // same choice for decoder + mel_linear + postnet (encoder / variance adaptor: always fp32)

  // vocoder-bias denoiser (e2etts_denoiser_*, e2etts_denoise; denoiser.hip).  The bases are not part of the weight blob: they and
  // the bias stay across e2etts_load_weights (a caller that loads another vocoder calibrates again).
  struct {
    int nfft = 0, hop = 0, nov = 0, cpad = 0;  // filter_length, hop, n_overlap, filter_length + 2 padded to a multiple of 32
    bool loaded = false, have_bias = false;
    float strength = 0.f;                      // e2etts_set_denoise: > 0 denoises e2etts_synthesize[_ctl]'s rows
  } dn;
  DevBuf dn_wf, dn_wi, dn_wf_frag, dn_wi_frag;  // forward basis, tap-major [Cout][KW * Cin], the inverse basis as one [hop][cpad] matrix per tap, and their fragment-order copies
  DevBuf dn_win, dn_bias;                       // squared window [filter_length] float64; bias spectrum [filter_length / 2 + 1]
  DevBuf dn_in, dn_lens, dn_pad, dn_spec, dn_ola, dn_out, dn_pcm;
  DevBuf dn_mel;    // calibration: the mel ...
  VocPass dn_pass;  // ... and the pass that turns it into audio, on the engine's stream: no resident result (wav, PCM, iSTFT tap) is touched
  std::vector<int32_t> dn_h;                    // host copy of dn_lens: [2 + n_overlap][B] = valid samples, frames, rows of the overlap-add per inverse launch

  // profiling
  bool prof_on = false;
  std::string prof_filter;  // non-empty: only launches of this class are bracketed by events (e2etts_profile_filter)
  std::vector<ProfRec> prof_recs;
  std::vector<hipEvent_t> ev_pool;
  std::vector<e2etts_kernel_stat> prof_stats;

  int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    err = buf;
    return code;
  }
};

namespace {

#define HIPCHK(e, expr)                                                                     \
  do {                                                                                      \
    hipError_t _s = (expr);                                                                 \
    if (_s != hipSuccess) return (e)->fail(E2ETTS_EHIP, "%s: %s", #expr, hipGetErrorString(_s)); \
  } while (0)

#define RET(expr)            \
  do {                       \
    int _r = (expr);         \
    if (_r != E2ETTS_OK) return _r; \
  } while (0)

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

template <typename T>
T* ptr(DevBuf& b) { return reinterpret_cast<T*>(b.p); }

using VocPass = e2etts_engine::VocPass;

// e->stream is the stream the engine is enqueuing on: conv(), ProfScope, ensure() and the denoiser helpers read it.  Work that goes
// elsewhere -- a stream slot's pass, a ResBlock on a side stream -- says so with one of these for as long as it lasts; besides
// e2etts_create and e2etts_destroy nothing else assigns e->stream.
struct OnStream {
  e2etts_engine* e;
  hipStream_t back;
  OnStream(e2etts_engine* e_, hipStream_t s) : e(e_), back(e_->stream) { e->stream = s; }
  ~OnStream() { e->stream = back; }
  OnStream(const OnStream&) = delete;
  OnStream& operator=(const OnStream&) = delete;
};

template <typename F>
void for_each_pass(e2etts_engine* e, F f) {
  f(e->voc);
  f(e->dn_pass);
  for (auto& sl : e->st_slot) f(sl.pass);
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

struct ProfScope {
  e2etts_engine* e;
  ProfRec rec{};
  bool on;
  ProfScope(e2etts_engine* e_, const char* name, double flops, double bytes) : e(e_), on(e_->prof_on) {
    if (on && !e->prof_filter.empty() && e->prof_filter != name) on = false;
    if (!on) return;
    rec.cls = prof_class(e, name);
    rec.flops = flops;
    rec.bytes = bytes;
    rec.start = get_event(e);
    rec.stop = get_event(e);
    (void)hipEventRecord(rec.start, e->stream);
  }
  ~ProfScope() {
    if (!on) return;
    (void)hipEventRecord(rec.stop, e->stream);
    e->prof_recs.push_back(rec);
  }
};

int prof_collect(e2etts_engine* e) {
  if (e->prof_recs.empty()) return E2ETTS_OK;
  HIPCHK(e, hipStreamSynchronize(e->stream));
  for (auto& r : e->prof_recs) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.start, r.stop) == hipSuccess) {
      auto& s = e->prof_stats[r.cls];
      s.launches += 1;
      s.ms += ms;
      s.flops += r.flops;
      s.bytes += r.bytes;
    }
    e->ev_pool.push_back(r.start);
    e->ev_pool.push_back(r.stop);
  }
  e->prof_recs.clear();
  return E2ETTS_OK;
}

#define KCHK(e, expr)                                              \
  do {                                                             \
    const char* _m = (expr);                                       \
    if (_m) return (e)->fail(E2ETTS_EINVAL, "%s", _m);             \
  } while (0)

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
int conv(e2etts_engine* e, ConvParams p, double alg_scale = 1.0, bool ksplit = false) {
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

void free_frags(e2etts_engine* e) {
  for (auto& kv : e->frag_of) {
    (void)hipFree(kv.second);
  }
  e->frag_of.clear();
  for (auto& kv : e->bimg_of) (void)hipFree(kv.second.first);
  e->bimg_of.clear();
  for (auto& kv : e->bimg_act) (void)hipFree(kv.second.first);
  e->bimg_act.clear();
  for (auto& kv : e->r16_of) (void)hipFree(kv.second);
  e->r16_of.clear();
  for (auto& kv : e->himg_of) (void)hipFree(kv.second.first);
  e->himg_of.clear();
  for (auto& kv : e->r16h_of) (void)hipFree(kv.second);
  e->r16h_of.clear();
  for (float* f : e->rb_frag_base)
    if (f) (void)hipFree(f);
  e->rb_frag_base.clear();
  e->rb_pair_frag.clear();
  e->rb_pair_frag32.clear();
  e->stage_fused.clear();
  e->dev_bytes -= e->frag_bytes;
  e->frag_bytes = 0;
}

int make_frag(e2etts_engine* e, const float* wx3, uint64_t cout, uint64_t kw, uint64_t cin) {
  if (!wx3 || cout <= 64 || e->frag_of.count(wx3)) return E2ETTS_OK;  // <= 64 columns: the LDS-tile kernels measured no gain
  float* f = nullptr;
  const size_t bytes = x3_frag_bytes((int)cout, (int)kw, (int)cin);
  HIPCHK(e, hipMalloc(&f, bytes));
  e->dev_bytes += bytes;
  e->frag_bytes += bytes;
  e->frag_of[wx3] = f;
  KCHK(e, launch_x3_to_frag(wx3, f, (int)cout, (int)kw, (int)cin, e->stream));
  return E2ETTS_OK;
}

// fp32 weights of a layer the 128-column kernels serve (Cout > 64) -> fp32 fragment order, for the exact-fp32 mode.
// phoneme_level: a layer conv_ksplit.hip serves -- that kernel has no other weight format, so its image is made whatever tuning().frag32 says.
int make_frag32(e2etts_engine* e, const float* w, uint64_t cout, uint64_t kw, uint64_t cin, bool narrow = false, bool phoneme_level = false) {
  if ((!tuning().frag32 && !phoneme_level) || !w || (cout <= 64 && !narrow && !phoneme_level) || e->frag_of.count(w)) return E2ETTS_OK;
  float* f = nullptr;
  const size_t bytes = x3_frag_bytes((int)cout, (int)kw, (int)cin);
  HIPCHK(e, hipMalloc(&f, bytes));
  e->dev_bytes += bytes;
  e->frag_bytes += bytes;
  e->frag_of[w] = f;
  KCHK(e, launch_f32_to_frag(w, f, (int)cout, (int)kw, (int)cin, e->stream));
  return E2ETTS_OK;
}

// hi halves of a vocoder convolution's split-precision image in conv_bf16.hip's order (plain-bf16 mode).  tap_split: see BConvParams.
int make_bimg(e2etts_engine* e, const float* wx3, uint64_t cout, uint64_t kw, uint64_t cin, int tap_split = 0,
              std::map<const float*, std::pair<void*, int>>* into = nullptr) {
  auto& dst = into ? *into : e->bimg_of;
  if (!wx3 || (cout % 32) || dst.count(wx3)) return E2ETTS_OK;
  if (tap_split > 0 && (kw != 3 || (tap_split % 32))) tap_split = 0;   // no polyphase image: the kernel multiplies the zeros
  void* img = nullptr;
  const size_t bytes = bf16_image_bytes((int)cout, (int)kw, (int)cin, tap_split);
  HIPCHK(e, hipMalloc(&img, bytes));
  e->dev_bytes += bytes;
  e->frag_bytes += bytes;
  dst[wx3] = {img, tap_split};
  KCHK(e, launch_bf16_image(wx3, img, (int)cout, (int)kw, (int)cin, tap_split, e->stream));
  return E2ETTS_OK;
}

// fp32 -> the nearest IEEE binary16 value (ties to even), as fp32: overflow (>= 65520) to infinity, subnormals (multiples of 2^-24) kept
static float round_to_f16(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  const uint32_t sign = u & 0x80000000u;
  uint32_t a = u & 0x7fffffffu;
  if (a >= 0x7f800000u) return f;   // infinity, NaN
  if (a < 0x38800000u) {            // below 2^-14: the quantum is 2^-24, which is fp32's in [0.5, 1)
    float af;
    memcpy(&af, &a, 4);
    volatile float t = af + 0.5f;
    af = t - 0.5f;
    memcpy(&a, &af, 4);
  } else {
    a = (a + 0xfffu + ((a >> 13) & 1u)) & ~0x1fffu;
    if (a >= 0x47800000u) a = 0x7f800000u;
  }
  a |= sign;
  memcpy(&f, &a, 4);
  return f;
}

// precision "bf16_act": a copy of n fp32 values rounded to bf16 (nearest-even), kept as fp32, made once at load
// (fp16 = true: rounded to fp16 into r16h_of, for precision "fp16_act", made at the first selection of that mode)
int make_r16(e2etts_engine* e, const float* src, size_t n, bool fp16 = false) {
  auto& dst = fp16 ? e->r16h_of : e->r16_of;
  if (!src || dst.count(src)) return E2ETTS_OK;
  std::vector<float> h(n);
  HIPCHK(e, hipMemcpyAsync(h.data(), src, n * 4, hipMemcpyDefault, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  for (float& f : h) {
    if (fp16) { f = round_to_f16(f); continue; }
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7f800000u) != 0x7f800000u) u = (u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u;
    memcpy(&f, &u, 4);
  }
  float* d = nullptr;
  HIPCHK(e, hipMalloc(&d, n * 4));
  e->dev_bytes += n * 4;
  e->frag_bytes += n * 4;
  dst[src] = d;
  HIPCHK(e, hipMemcpyAsync(d, h.data(), n * 4, hipMemcpyDefault, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return E2ETTS_OK;
}

// precision "fp16_act": a vocoder convolution's fp32 weights [cout][kw][cin] as the fp16 image in conv_bf16.hip's order
int make_himg(e2etts_engine* e, const float* w, uint64_t cout, uint64_t kw, uint64_t cin, int tap_split = 0) {
  if (!w || (cout % 32) || e->himg_of.count(w)) return E2ETTS_OK;
  if (tap_split > 0 && (kw != 3 || (tap_split % 32))) tap_split = 0;
  void* img = nullptr;
  const size_t bytes = bf16_image_bytes((int)cout, (int)kw, (int)cin, tap_split);
  HIPCHK(e, hipMalloc(&img, bytes));
  e->dev_bytes += bytes;
  e->frag_bytes += bytes;
  e->himg_of[w] = {img, tap_split};
  KCHK(e, launch_f16_image(w, img, (int)cout, (int)kw, (int)cin, tap_split, e->stream));
  return E2ETTS_OK;
}

int get_tensor(e2etts_engine* e, const std::string& name, uint64_t numel, const float** out) {
  auto it = e->tensors.find(name);
  if (it == e->tensors.end()) return e->fail(E2ETTS_EKEY, "weight blob has no tensor '%s'", name.c_str());
  if (numel && it->second.second != numel)
    return e->fail(E2ETTS_EINVAL, "tensor '%s' has %llu elements, expected %llu", name.c_str(),
                   (unsigned long long)it->second.second, (unsigned long long)numel);
  *out = it->second.first;
  return E2ETTS_OK;
}

int bind_fft(e2etts_engine* e, const char* side, int layers, std::vector<FFTLayer>& v) {
  const auto& c = e->cfg;
  const uint64_t H = c.hidden, F = c.ffn_dim;
  v.resize(layers);
  for (int l = 0; l < layers; ++l) {
    std::string p = std::string(side) + "." + std::to_string(l) + ".";
    FFTLayer& f = v[l];
    RET(get_tensor(e, p + "wqkv", 3 * H * H, &f.wqkv));
    RET(get_tensor(e, p + "bqkv", 3 * H, &f.bqkv));
    RET(get_tensor(e, p + "wo", H * H, &f.wo));
    RET(get_tensor(e, p + "bo", H, &f.bo));
    RET(get_tensor(e, p + "ln1.g", H, &f.ln1g));
    RET(get_tensor(e, p + "ln1.b", H, &f.ln1b));
    RET(get_tensor(e, p + "w1", F * c.ffn_k1 * H, &f.w1));
    RET(get_tensor(e, p + "b1", F, &f.b1));
    RET(get_tensor(e, p + "w2", H * F, &f.w2));
    RET(get_tensor(e, p + "b2", H, &f.b2));
    RET(get_tensor(e, p + "ln2.g", H, &f.ln2g));
    RET(get_tensor(e, p + "ln2.b", H, &f.ln2b));
    const bool ph = side[0] == 'e';  // the encoder runs over phonemes
    RET(make_frag32(e, f.wqkv, 3 * H, 1, H));
    RET(make_frag32(e, f.wo, H, 1, H));
    RET(make_frag32(e, f.w1, F, c.ffn_k1, H, false, ph));
    RET(make_frag32(e, f.w2, H, 1, F, false, ph));
    const uint64_t Hc = (H + 31) / 32 * 32, Fc = (F + 31) / 32 * 32;
    if (e->tensors.count(p + "wqkv.x3")) {
      RET(get_tensor(e, p + "wqkv.x3", 3 * H * Hc, &f.wqkv_x3));
      RET(get_tensor(e, p + "wo.x3", H * Hc, &f.wo_x3));
      RET(get_tensor(e, p + "w1.x3", F * c.ffn_k1 * Hc, &f.w1_x3));
      RET(get_tensor(e, p + "w2.x3", H * Fc, &f.w2_x3));
      RET(make_frag(e, f.wqkv_x3, 3 * H, 1, H));
      RET(make_frag(e, f.wo_x3, H, 1, H));
      RET(make_frag(e, f.w1_x3, F, c.ffn_k1, H));
      RET(make_frag(e, f.w2_x3, H, 1, F));
    }
  }
  return E2ETTS_OK;
}

int bind_cf_gemm(e2etts_engine* e, const std::string& name, const char* bias, uint64_t cout, uint64_t cin, CfGemm& g) {
  RET(get_tensor(e, name, cout * cin, &g.w));
  RET(make_frag32(e, g.w, cout, 1, cin));
  g.b = nullptr;
  if (bias) RET(get_tensor(e, bias, cout, &g.b));
  g.wx3 = nullptr;
  if (e->tensors.count(name + ".x3")) {
    RET(get_tensor(e, name + ".x3", cout * ((cin + 31) / 32 * 32), &g.wx3));
    RET(make_frag(e, g.wx3, cout, 1, cin));
  }
  return E2ETTS_OK;
}

int bind_conformer(e2etts_engine* e, const char* side, int layers, std::vector<CfLayer>& v, int n_head) {
  const auto& c = e->cfg;
  const uint64_t H = c.hidden, F = c.ffn_dim, nh = n_head;
  v.resize(layers);
  for (int l = 0; l < layers; ++l) {
    const std::string p = std::string(side) + "." + std::to_string(l) + ".";
    CfLayer& f = v[l];
    for (int i = 0; i < 2; ++i) {
      const std::string q = p + (i ? "ff2." : "ff1.");
      RET(get_tensor(e, q + "ln.g", H, &f.ff_lng[i]));
      RET(get_tensor(e, q + "ln.b", H, &f.ff_lnb[i]));
      RET(bind_cf_gemm(e, q + "w1", (q + "b1").c_str(), F, H, f.ff_a[i]));
      RET(bind_cf_gemm(e, q + "w2", (q + "b2").c_str(), H, F, f.ff_b[i]));
    }
    RET(get_tensor(e, p + "att.ln.g", H, &f.att_lng));
    RET(get_tensor(e, p + "att.ln.b", H, &f.att_lnb));
    RET(get_tensor(e, p + "att.u", H, &f.att_u));
    RET(get_tensor(e, p + "att.v", H, &f.att_v));
    RET(bind_cf_gemm(e, p + "att.wqkv", nullptr, 3 * H, H, f.att_qkv));  // LinearNorm default: no bias (U/blocks/utils.py:182)
    RET(bind_cf_gemm(e, p + "att.wo", nullptr, H, H, f.att_o));
    const uint64_t rows[2] = {(uint64_t)c.max_seq_len + 1, (uint64_t)c.pos_table_rows};
    const char* tag[2] = {"att.pos", "att.posr"};
    for (int i = 0; i < 2; ++i) {
      f.pos_rows[i] = rows[i];
      RET(get_tensor(e, p + tag[i], nh * rows[i] * (H / nh), &f.pos[i]));
      f.posx[i] = nullptr;
      if (e->tensors.count(p + tag[i] + ".x3")) RET(get_tensor(e, p + tag[i] + ".x3", nh * rows[i] * (H / nh), &f.posx[i]));
    }
    RET(get_tensor(e, p + "cv.ln.g", H, &f.cv_lng));
    RET(get_tensor(e, p + "cv.ln.b", H, &f.cv_lnb));
    RET(bind_cf_gemm(e, p + "cv.pw1.w", (p + "cv.pw1.b").c_str(), 2 * H, H, f.pw1));
    RET(get_tensor(e, p + "cv.dw.w", (uint64_t)c.ffn_k1 * H, &f.dw_w));
    RET(get_tensor(e, p + "cv.dw.b", H, &f.dw_b));
    RET(bind_cf_gemm(e, p + "cv.pw2.w", (p + "cv.pw2.b").c_str(), H, H, f.pw2));
    RET(get_tensor(e, p + "ln.g", H, &f.lng));
    RET(get_tensor(e, p + "ln.b", H, &f.lnb));
  }
  return E2ETTS_OK;
}

int bind_ff_gemm(e2etts_engine* e, const std::string& name, const std::string& bias, uint64_t cout, uint64_t kw, uint64_t cin, CfGemm& g) {
  RET(get_tensor(e, name, cout * kw * cin, &g.w));
  RET(make_frag32(e, g.w, cout, kw, cin));
  RET(get_tensor(e, bias, cout, &g.b));
  g.wx3 = nullptr;
  if (e->tensors.count(name + ".x3")) {
    RET(get_tensor(e, name + ".x3", cout * kw * ((cin + 31) / 32 * 32), &g.wx3));
    RET(make_frag(e, g.wx3, cout, kw, cin));
  }
  return E2ETTS_OK;
}

int bind_fastformer(e2etts_engine* e, const char* side, int layers, FfSide& v, int n_head) {
  const auto& c = e->cfg;
  const uint64_t H = c.hidden, F = c.ffn_dim, heads = H / n_head;
  v.head_size = n_head;
  v.layers.resize(layers);
  if (layers > 0) {
    const std::string p = std::string(side) + ".ff.";
    RET(get_tensor(e, p + "wql", H * heads, &v.wql));
    RET(get_tensor(e, p + "bql", heads, &v.bql));
    RET(get_tensor(e, p + "wkl", H * heads, &v.wkl));
    RET(get_tensor(e, p + "bkl", heads, &v.bkl));
  }
  for (int l = 0; l < layers; ++l) {
    const std::string p = std::string(side) + "." + std::to_string(l) + ".";
    FfLayer& f = v.layers[l];
    RET(get_tensor(e, p + "att.ln.g", H, &f.att_lng));
    RET(get_tensor(e, p + "att.ln.b", H, &f.att_lnb));
    RET(bind_ff_gemm(e, p + "att.wqk", p + "att.bqk", 2 * H, 1, H, f.qk));
    RET(bind_ff_gemm(e, p + "att.wt", p + "att.bt", H, 1, H, f.wt));
    RET(get_tensor(e, p + "ffn.ln.g", H, &f.ffn_lng));
    RET(get_tensor(e, p + "ffn.ln.b", H, &f.ffn_lnb));
    RET(bind_ff_gemm(e, p + "ffn.w1", p + "ffn.b1", F, c.ffn_k1, H, f.w1));
    RET(bind_ff_gemm(e, p + "ffn.w2", p + "ffn.b2", H, 1, F, f.w2));
  }
  return E2ETTS_OK;
}

int bind_pred(e2etts_engine* e, const char* name, int layers, int kernel, int chans, int odim, bool alpha, Predictor& pr) {
  const uint64_t H = e->cfg.hidden;
  pr.layers.resize(layers);
  pr.kernel = kernel;
  pr.chans = chans;
  pr.odim = odim;
  for (int i = 0; i < layers; ++i) {
    std::string p = std::string(name) + "." + std::to_string(i) + ".";
    const uint64_t cin = i == 0 ? H : (uint64_t)chans;
    RET(get_tensor(e, p + "w", (uint64_t)chans * kernel * cin, &pr.layers[i].w));
    RET(make_frag32(e, pr.layers[i].w, chans, kernel, cin, false, true));
    RET(get_tensor(e, p + "b", chans, &pr.layers[i].b));
    RET(get_tensor(e, p + "g", chans, &pr.layers[i].g));
    RET(get_tensor(e, p + "beta", chans, &pr.layers[i].beta));
  }
  RET(get_tensor(e, std::string(name) + ".lin.w", (uint64_t)odim * chans, &pr.lin_w));
  RET(get_tensor(e, std::string(name) + ".lin.b", odim, &pr.lin_b));
  if (alpha) RET(get_tensor(e, std::string(name) + ".alpha", 1, &pr.alpha));
  return E2ETTS_OK;
}

int bind_acoustic(e2etts_engine* e) {
  const auto& c = e->cfg;
  const uint64_t H = c.hidden;
  RET(get_tensor(e, "enc.emb", (uint64_t)(c.n_symbols + 1) * H, &e->emb));
  RET(get_tensor(e, "enc.pos", (uint64_t)(c.max_seq_len + 1) * H, &e->enc_pos));
  RET(get_tensor(e, "dec.pos", (uint64_t)(c.max_seq_len + 1) * H, &e->dec_pos));
  RET(get_tensor(e, "pos.regen", (uint64_t)c.pos_table_rows * H, &e->pos_regen));
  RET(get_tensor(e, "spk.emb", (uint64_t)c.n_speakers * H, &e->spk_emb));
  if (c.block_type == 1) {
    RET(bind_conformer(e, "enc", c.enc_layers, e->cf_enc, c.n_head));
    RET(bind_conformer(e, "dec", c.dec_layers, e->cf_dec, c.dec_n_head ? c.dec_n_head : c.n_head));
  } else if (c.block_type == 2) {
    RET(bind_fastformer(e, "enc", c.enc_layers, e->ff_enc, c.n_head));
    RET(bind_fastformer(e, "dec", c.dec_layers, e->ff_dec, c.dec_n_head ? c.dec_n_head : c.n_head));
  } else {
    RET(bind_fft(e, "enc", c.enc_layers, e->enc));
    RET(bind_fft(e, "dec", c.dec_layers, e->dec));
  }
  RET(bind_pred(e, "dur", c.dur_layers, c.dur_kernel, c.dur_chans, 1, false, e->dur));
  RET(bind_pred(e, "pitch", c.var_layers, c.var_kernel, c.var_chans, c.pitch_no_uv ? 1 : 2, true, e->pitch));
  RET(bind_pred(e, "energy", c.energy_layers ? c.energy_layers : c.var_layers, c.energy_kernel ? c.energy_kernel : c.var_kernel, c.var_chans, 1, true,
                e->energy));
  {
    auto it = e->tensors.find("var.pos");
    if (it == e->tensors.end()) return e->fail(E2ETTS_EKEY, "weight blob has no tensor 'var.pos'");
    if (it->second.second % H) return e->fail(E2ETTS_EINVAL, "var.pos size is not a multiple of hidden");
    e->var_pos = it->second.first;
    e->var_pos_rows = it->second.second / H;
  }
  RET(get_tensor(e, "pitch.emb", (uint64_t)(c.pitch_emb_rows ? c.pitch_emb_rows : c.n_bins) * H, &e->pitch_emb));
  e->pitch_bins = nullptr;
  if (c.pitch_no_uv) RET(get_tensor(e, "pitch.bins", (uint64_t)c.n_bins - 1, &e->pitch_bins));
  RET(get_tensor(e, "energy.emb", (uint64_t)c.n_bins * H, &e->energy_emb));
  RET(get_tensor(e, "energy.bins", (uint64_t)c.n_bins - 1, &e->energy_bins));
  RET(get_tensor(e, "mel.w", (uint64_t)c.n_mel * H, &e->mel_lin.w));
  RET(make_frag32(e, e->mel_lin.w, c.n_mel, 1, H));
  RET(get_tensor(e, "mel.b", c.n_mel, &e->mel_lin.b));
  e->mel_lin.wx3 = nullptr;
  if (e->tensors.count("mel.w.x3")) RET(get_tensor(e, "mel.w.x3", (uint64_t)c.n_mel * ((H + 31) / 32 * 32), &e->mel_lin.wx3));
  RET(make_frag(e, e->mel_lin.wx3, c.n_mel, 1, H));
  e->postnet.resize(c.postnet_layers);
  for (int i = 0; i < c.postnet_layers; ++i) {
    const uint64_t cin = i == 0 ? c.n_mel : c.postnet_dim, cout = i == c.postnet_layers - 1 ? c.n_mel : c.postnet_dim;
    std::string p = "post." + std::to_string(i) + ".";
    RET(get_tensor(e, p + "w", cout * c.postnet_kernel * cin, &e->postnet[i].w));
    RET(make_frag32(e, e->postnet[i].w, cout, c.postnet_kernel, cin));
    RET(get_tensor(e, p + "b", cout, &e->postnet[i].b));
    e->postnet[i].wx3 = nullptr;
    if (e->tensors.count(p + "w.x3")) RET(get_tensor(e, p + "w.x3", cout * c.postnet_kernel * ((cin + 31) / 32 * 32), &e->postnet[i].wx3));
    RET(make_frag(e, e->postnet[i].wx3, cout, c.postnet_kernel, cin));
  }
  return E2ETTS_OK;
}

// fp32 weight + bias (required) and the split-precision image (optional: older blobs do not carry it)
int bind_conv(e2etts_engine* e, const std::string& name, uint64_t cout, uint64_t kw, uint64_t cin, ConvW& w) {
  RET(get_tensor(e, name + ".w", cout * kw * cin, &w.w));
  RET(make_frag32(e, w.w, cout, kw, cin));
  RET(get_tensor(e, name + ".b", cout, &w.b));
  w.wx3 = nullptr;
  if (e->tensors.count(name + ".wx3")) RET(get_tensor(e, name + ".wx3", cout * kw * ((cin + 31) / 32) * 32, &w.wx3));
  RET(make_frag(e, w.wx3, cout, kw, cin));
  return E2ETTS_OK;
}

// Precision "fp16_act": the fp16 image of every vocoder convolution and the fp16-rounded biases / conv_post weights of the bound vocoder
// (HiFi-GAN tail).  Called at the first selection of the mode, and by bind_vocoder when new weights arrive under it; what exists is kept.
int make_fp16_act_params(e2etts_engine* e) {
  const auto& c = e->cfg;
  if (c.voc_istft_nfft) return E2ETTS_OK;
  uint64_t ch = c.voc_init_ch;
  RET(make_himg(e, e->voc_pre.w, ch, 7, c.n_mel));
  RET(make_r16(e, e->voc_pre.b, ch, true));
  for (int i = 0; i < c.voc_stages; ++i) {
    const uint64_t cin = ch, cout = ch / 2, s = c.voc_up_rate[i];
    RET(make_himg(e, e->voc_up[i].w, s * cout, 3, cin, (int)(s * cout / 2)));
    RET(make_r16(e, e->voc_up[i].b, s * cout, true));
    ch = cout;
    for (int j = 0; j < c.voc_n_kernels; ++j) {
      const int idx = i * c.voc_n_kernels + j;
      const uint64_t k = c.voc_rb_kernel[j];
      for (int m = 0; m < c.voc_n_dil; ++m) {
        RET(make_himg(e, e->rb_c1[idx][m].w, ch, k, ch));
        RET(make_r16(e, e->rb_c1[idx][m].b, ch, true));
        if (c.voc_resblock == 2) continue;
        RET(make_himg(e, e->rb_c2[idx][m].w, ch, k, ch));
        RET(make_r16(e, e->rb_c2[idx][m].b, ch, true));
      }
    }
  }
  RET(make_r16(e, e->voc_post.w, 7 * ch, true));
  RET(make_r16(e, e->voc_post.b, 1, true));
  HIPCHK(e, hipStreamSynchronize(e->stream));   // the stream slots' passes run on streams of their own
  return E2ETTS_OK;
}

int bind_vocoder(e2etts_engine* e) {
  const auto& c = e->cfg;
  const uint64_t C0 = c.voc_init_ch;
  RET(bind_conv(e, "voc.pre", C0, 7, c.n_mel, e->voc_pre));
  RET(make_bimg(e, e->voc_pre.wx3, C0, 7, c.n_mel));
  RET(make_r16(e, e->voc_pre.b, C0));
  e->voc_up.resize(c.voc_stages);
  e->rb_c1.assign((size_t)c.voc_stages * c.voc_n_kernels, {});
  e->rb_c2.assign((size_t)c.voc_stages * c.voc_n_kernels, {});
  e->rb_pair_frag.assign((size_t)c.voc_stages * c.voc_n_kernels, {});
  e->rb_pair_frag32.assign((size_t)c.voc_stages * c.voc_n_kernels, {});
  e->stage_fused.clear();
  uint64_t ch = C0;
  for (int i = 0; i < c.voc_stages; ++i) {
    const uint64_t cin = ch, cout = ch / 2, s = c.voc_up_rate[i];
    RET(bind_conv(e, "voc.up." + std::to_string(i), s * cout, 3, cin, e->voc_up[i]));
    // the last upsampler of HiFi-GAN V1 (64 columns), exact fp32: fragments for the zero-tap-skipping 256 x 32 tile (conv_gemm.hip)
    if (s * cout == 64) RET(make_frag32(e, e->voc_up[i].w, s * cout, 3, cin, true));
    RET(make_bimg(e, e->voc_up[i].wx3, s * cout, 3, cin, (int)(s * cout / 2)));
    RET(make_r16(e, e->voc_up[i].b, s * cout));
    ch = cout;
    for (int j = 0; j < c.voc_n_kernels; ++j) {
      const int idx = i * c.voc_n_kernels + j;
      const uint64_t k = c.voc_rb_kernel[j];
      e->rb_c1[idx].resize(c.voc_n_dil);
      e->rb_c2[idx].resize(c.voc_n_dil);
      for (int m = 0; m < c.voc_n_dil; ++m) {
        std::string q = "voc.rb." + std::to_string(idx) + ".";
        if (c.voc_resblock == 2) {  // ResBlock2: one convolution per dilation (V/layers.py:52-56)
          RET(bind_conv(e, q + "c." + std::to_string(m), ch, k, ch, e->rb_c1[idx][m]));
          RET(make_bimg(e, e->rb_c1[idx][m].wx3, ch, k, ch, 0, &e->bimg_act));
          RET(make_r16(e, e->rb_c1[idx][m].b, ch));
          continue;
        }
        RET(bind_conv(e, q + "c1." + std::to_string(m), ch, k, ch, e->rb_c1[idx][m]));
        RET(bind_conv(e, q + "c2." + std::to_string(m), ch, k, ch, e->rb_c2[idx][m]));
        RET(make_bimg(e, e->rb_c1[idx][m].wx3, ch, k, ch));
        RET(make_bimg(e, e->rb_c2[idx][m].wx3, ch, k, ch));
        RET(make_r16(e, e->rb_c1[idx][m].b, ch));
        RET(make_r16(e, e->rb_c2[idx][m].b, ch));
      }
    }
    // fused pairs: all of a stage or none (the two forms use the stage's scratch buffers differently)
    bool fusable = c.voc_resblock == 1;
    for (int j = 0; j < c.voc_n_kernels && fusable; ++j)
      for (int m = 0; m < c.voc_n_dil; ++m)
        fusable = fusable && resblock_pair_supported((int)ch, c.voc_rb_kernel[j], c.voc_rb_dil[j][m]) &&
                  e->rb_c1[i * c.voc_n_kernels + j][m].wx3 && e->rb_c2[i * c.voc_n_kernels + j][m].wx3;
    e->stage_fused.push_back(fusable ? 1 : 0);
    for (int j = 0; j < c.voc_n_kernels && fusable; ++j) {
      const int idx = i * c.voc_n_kernels + j;
      const int k = c.voc_rb_kernel[j];
      // ONE allocation per ResBlock: conv1 | conv2 of pair 0, pair 1, ... contiguous, so that the whole-ResBlock kernel
      // (resblock_chain.hip) walks all of them through one buffer descriptor; rb_pair_frag[idx][m] points at pair m
      const size_t one = x3_frag_bytes((int)ch, k, (int)ch);
      float* base = nullptr;
      HIPCHK(e, hipMalloc(&base, 2 * one * c.voc_n_dil));
      e->dev_bytes += 2 * one * c.voc_n_dil;
      e->frag_bytes += 2 * one * c.voc_n_dil;
      e->rb_frag_base.push_back(base);
      for (int m = 0; m < c.voc_n_dil; ++m) {
        float* f = base + (size_t)m * 2 * (one / 4);
        e->rb_pair_frag[idx].push_back(f);
        KCHK(e, launch_x3_to_frag(e->rb_c1[idx][m].wx3, f, (int)ch, k, (int)ch, e->stream));
        KCHK(e, launch_x3_to_frag(e->rb_c2[idx][m].wx3, f + one / 4, (int)ch, k, (int)ch, e->stream));
      }
      // at 128 / 256 channels the fp32 kernels are bound by the matrix pipe and the fused form recomputes (KW - 1) / 128 of its rows:
      // it pays up to kernel size 7 at 128 channels and not at 256 (same bits either way)
      if (ch <= 64 || (ch == 128 && k <= 7)) {  // fp32 images of the same pairs
        float* b32 = nullptr;
        HIPCHK(e, hipMalloc(&b32, 2 * one * c.voc_n_dil));
        e->dev_bytes += 2 * one * c.voc_n_dil;
        e->frag_bytes += 2 * one * c.voc_n_dil;
        e->rb_frag_base.push_back(b32);
        for (int m = 0; m < c.voc_n_dil; ++m) {
          float* f = b32 + (size_t)m * 2 * (one / 4);
          e->rb_pair_frag32[idx].push_back(f);
          KCHK(e, launch_f32_to_frag(e->rb_c1[idx][m].w, f, (int)ch, k, (int)ch, e->stream));
          KCHK(e, launch_f32_to_frag(e->rb_c2[idx][m].w, f + one / 4, (int)ch, k, (int)ch, e->stream));
        }
      }
    }
  }
  if (c.voc_istft_nfft) {  // conv_post to n_fft + 2 channels (padded to a multiple of 4 by the packer), V/generator.py:92
    const uint64_t pc = ((uint64_t)c.voc_istft_nfft + 2 + 3) / 4 * 4;
    RET(bind_conv(e, "voc.post", pc, 7, ch, e->voc_post));
  } else {
    RET(get_tensor(e, "voc.post.w", 7 * ch, &e->voc_post.w));
    RET(get_tensor(e, "voc.post.b", 1, &e->voc_post.b));
    RET(make_r16(e, e->voc_post.w, 7 * ch));
    RET(make_r16(e, e->voc_post.b, 1));
  }
  if (e->voc_precision == E2ETTS_PRECISION_FP16_ACT) RET(make_fp16_act_params(e));   // new weights under a mode selected earlier
  return E2ETTS_OK;
}

// 6 x FFTBlock (reference U/blocks/transformer.py:178-189), in place on x ([B, N, H]); lens32: device [B]
int fft_stack(e2etts_engine* e, const std::vector<FFTLayer>& layers, int n_head, float* x, float* xalt, const int32_t* lens, int B, int N, bool x3,
              const int32_t* act = nullptr, double act_frac = 1.0, bool ksplit = false, const int32_t* act_host = nullptr) {
  const auto& c = e->cfg;
  const int H = c.hidden, F = c.ffn_dim;
  float* qkv = ptr<float>(e->qkv);
  float* att = ptr<float>(e->att);
  float* tmp = ptr<float>(e->tmp);
  float* hid = ptr<float>(e->hid);
  for (const FFTLayer& f : layers) {
    ConvParams p;
    p.B = B; p.T = N; p.act_rows = act; p.act_rows_host = act_host; p.act_frac = act_frac;
    // q | k | v projections as one GEMM (U/blocks/transformer.py:220-222)
    const bool sx = x3 && f.wqkv_x3;
    p.in = x; p.w = sx ? f.wqkv_x3 : f.wqkv; p.x3 = sx; p.bias = f.bqkv; p.out = qkv; p.Cin = H; p.Cout = 3 * H;
    RET(conv(e, p, 1.0, ksplit));
    {
      const double fl = 4.0 * B * n_head * (double)N * N * (H / n_head);
      ProfScope ps(e, sx ? "attention_x3" : "attention", fl, 4.0 * 4.0 * B * N * H);
      float* aws = nullptr;   // workspace for the parallel key segments of small fp32 grids (attention.hip); 3.6 MB at B = 1, T = 768
      size_t aws_bytes = 0;
      if (!sx && !act_host && (long long)B * ((N + 63) / 64) * n_head <= attention_par_max_grid() && N > 32 * 8) {
        aws_bytes = attention_workspace_bytes(B, N, H, n_head);
        RET(ensure(e, e->attws, aws_bytes));
        aws = ptr<float>(e->attws);
      }
      KCHK(e, launch_attention(qkv, att, lens, B, N, H, n_head, sx ? 1 : 0, e->stream, act_host, aws, aws_bytes));
    }
    // fc + residual (:238-239), LayerNorm eps 1e-5, masked_fill (:182-183)
    p = ConvParams(); p.B = B; p.T = N; p.act_rows = act; p.act_rows_host = act_host; p.act_frac = act_frac;
    p.in = att; p.w = sx ? f.wo_x3 : f.wo; p.x3 = sx; p.bias = f.bo; p.res = x; p.out = tmp; p.Cin = H; p.Cout = H;
    RET(conv(e, p, 1.0, ksplit));
    {
      ProfScope ps(e, "layernorm", 0, 8.0 * B * N * H);
      KCHK(e, launch_layernorm(tmp, xalt, f.ln1g, f.ln1b, lens, B, N, H, 1e-5f, e->stream));
    }
    // conv k9 + ReLU, conv k1 + residual, LayerNorm, masked_fill (:289-297, :185-187)
    p = ConvParams(); p.B = B; p.T = N; p.act_rows = act; p.act_rows_host = act_host; p.act_frac = act_frac;
    p.in = xalt; p.w = sx ? f.w1_x3 : f.w1; p.x3 = sx; p.bias = f.b1; p.out = hid; p.Cin = H; p.Cout = F; p.KW = c.ffn_k1; p.pad = (c.ffn_k1 - 1) / 2;
    p.act = ACT_RELU;
    RET(conv(e, p, 1.0, ksplit));
    p = ConvParams(); p.B = B; p.T = N; p.act_rows = act; p.act_rows_host = act_host; p.act_frac = act_frac;
    p.in = hid; p.w = sx ? f.w2_x3 : f.w2; p.x3 = sx; p.bias = f.b2; p.res = xalt; p.out = tmp; p.Cin = F; p.Cout = H;
    RET(conv(e, p, 1.0, ksplit));
    {
      ProfScope ps(e, "layernorm", 0, 8.0 * B * N * H);
      KCHK(e, launch_layernorm(tmp, x, f.ln2g, f.ln2b, lens, B, N, H, 1e-5f, e->stream));
    }
  }
  return E2ETTS_OK;
}

// n x ConformerBlock (reference U/blocks/conformer.py:214-255), in place on x ([B, N, H]).  Every sub-module is a pre-norm residual
// unit; nothing inside a block is masked (nn.Sequential hands the attention module no mask, :252, and the depthwise convolution
// runs over the padded length), so all N rows are computed; only the block's final LayerNorm output is zeroed at rows >= lens[b].
int conformer_stack(e2etts_engine* e, const std::vector<CfLayer>& layers, int n_head, float* x, float* xalt, const int32_t* lens, int B, int N, bool x3) {
  const auto& c = e->cfg;
  const int H = c.hidden, F = c.ffn_dim, nh = n_head, dh = H / nh;
  float* qkv = ptr<float>(e->qkv);
  float* att = ptr<float>(e->att);
  float* tmp = ptr<float>(e->tmp);
  float* hid = ptr<float>(e->hid);
  float *cur = x, *oth = xalt;
  const int tsel = N > c.max_seq_len ? 1 : 0;  // eval-time regenerated table (:339-344)
  auto gemm = [&](const CfGemm& g, const float* in, float* out, int cin, int cout, const float* res, int act = ACT_NONE) -> int {
    ConvParams p;
    p.B = B; p.T = N; p.in = in; p.out = out; p.Cin = cin; p.Cout = cout; p.bias = g.b; p.res = res; p.act = act;
    const bool sx = x3 && g.wx3;
    p.w = sx ? g.wx3 : g.w; p.x3 = sx;
    return conv(e, p);
  };
  auto ln = [&](const float* in, float* out, const float* g, const float* b, const int32_t* mask) -> int {
    ProfScope ps(e, "layernorm", 0, 8.0 * B * N * H);
    KCHK(e, launch_layernorm(in, out, g, b, mask, B, N, H, 1e-5f, e->stream));
    return E2ETTS_OK;
  };
  for (const CfLayer& f : layers) {
    if ((uint64_t)N > f.pos_rows[tsel])
      return e->fail(E2ETTS_EINVAL, "sequence of %d rows exceeds the Conformer position table (%llu rows)", N, (unsigned long long)f.pos_rows[tsel]);
    for (int half = 0; half < 2; ++half) {
      if (half == 1) {
        // MultiHeadedSelfAttentionModule (:335-353) + RelativeMultiHeadAttention (:399-440)
        RET(ln(cur, tmp, f.att_lng, f.att_lnb, nullptr));
        RET(gemm(f.att_qkv, tmp, qkv, H, 3 * H, nullptr));
        {  // the shifted position scores are computed inside the kernel, from this layer's projected table (attention.hip)
          // FLOPs: content scores and P . V (4 N^2 d_h per head) + the position bands (2 x 32 x 64 x d_h per 32 x 32 tile = 4 N^2 d_h)
          const double fl = 8.0 * B * nh * (double)N * N * dh;
          ProfScope ps(e, "rel_attention", fl, 4.0 * B * (4.0 * N * H) + 4.0 * nh * N * dh);
          KCHK(e, launch_rel_attention(qkv, f.pos[tsel], (int)f.pos_rows[tsel], f.att_u, f.att_v, att, B, N, H, nh, e->stream,
                                       x3 ? f.posx[tsel] : nullptr));
        }
        RET(gemm(f.att_o, att, oth, H, H, cur));
        std::swap(cur, oth);
        // ConformerConvModule (:468-481): LayerNorm, pointwise 2H + GLU, depthwise k + BatchNorm + Swish, pointwise
        RET(ln(cur, tmp, f.cv_lng, f.cv_lnb, nullptr));
        RET(gemm(f.pw1, tmp, hid, H, 2 * H, nullptr));
        {  // GLU + depthwise k + BatchNorm + Swish in one pass (small_kernels.hip); `att` is scratch for shapes without a fused form
          ProfScope ps(e, "dwconv_glu_swish", 2.0 * B * N * (double)H * c.ffn_k1, 12.0 * B * N * H);
          KCHK(e, launch_dwconv_glu_swish(hid, f.dw_w, f.dw_b, tmp, att, B, N, H, c.ffn_k1, e->stream));
        }
        RET(gemm(f.pw2, tmp, oth, H, H, cur));
        std::swap(cur, oth);
      }
      // FeedForwardModule (:294-301): LayerNorm, Linear + Swish (GEMM epilogue), Linear; x + factor * ff(x) with the factor folded into the weights
      RET(ln(cur, tmp, f.ff_lng[half], f.ff_lnb[half], nullptr));
      RET(gemm(f.ff_a[half], tmp, hid, H, F, nullptr, ACT_SWISH));
      RET(gemm(f.ff_b[half], hid, oth, F, H, cur));
      std::swap(cur, oth);
    }
    RET(ln(cur, oth, f.lng, f.lnb, lens));  // final LayerNorm (:248) + masked_fill (:253-254)
    std::swap(cur, oth);
  }
  if (cur != x) HIPCHK(e, hipMemcpyAsync(x, cur, (size_t)B * N * H * 4, hipMemcpyDeviceToDevice, e->stream));
  return E2ETTS_OK;
}

// n x [PreNorm(FastAttention), PreNorm(PositionwiseFeedForward)] (reference U/blocks/fastformer.py:167-175), in place on x ([B, N, H]).
// Both sub-blocks are pre-norm residual units followed by masked_fill (:169-173); there is no LayerNorm after them.  Every one of the N
// rows is computed: the attention's mask is inverted (:223-225, see fastformer.hip), so the padded positions of a row carry practically
// all the pooling weight, and the FFN convolution reads LayerNorm(0) = beta in the padding.  Logits, softmax and pooling are fp32 in every
// precision mode; x3 moves the four GEMMs of a layer to the split-precision path (decoder only).
int fastformer_stack(e2etts_engine* e, const FfSide& side, float* x, float* xalt, const int32_t* lens, int B, int N, bool x3) {
  const auto& c = e->cfg;
  const int H = c.hidden, F = c.ffn_dim, hs = side.head_size, heads = H / hs;
  float* qk = ptr<float>(e->qkv);   // q | k, [B, N, 2H]
  float* att = ptr<float>(e->att);
  float* tmp = ptr<float>(e->tmp);
  float* hid = ptr<float>(e->hid);
  float *cur = x, *oth = xalt;
  const size_t ws_bytes = ff_pool_workspace_bytes(B, N, H, hs);
  RET(ensure(e, e->attws, ws_bytes));
  RET(ensure(e, e->ffpool, (size_t)2 * B * H * 4));
  float* ws = ptr<float>(e->attws);
  float* gq = ptr<float>(e->ffpool);
  float* gk = gq + (size_t)B * H;
  auto gemm = [&](const CfGemm& g, const float* in, float* out, int cin, int cout, int kw, const float* res, const int32_t* mask, int act) -> int {
    ConvParams p;
    p.B = B; p.T = N; p.in = in; p.out = out; p.Cin = cin; p.Cout = cout; p.KW = kw; p.pad = (kw - 1) / 2; p.bias = g.b; p.res = res; p.lens = mask;
    p.act = act;
    const bool sx = x3 && g.wx3;
    p.w = sx ? g.wx3 : g.w; p.x3 = sx;
    return conv(e, p);
  };
  auto ln = [&](const float* in, float* out, const float* g, const float* b) -> int {
    ProfScope ps(e, "layernorm", 0, 8.0 * B * N * H);
    KCHK(e, launch_layernorm(in, out, g, b, nullptr, B, N, H, 1e-5f, e->stream));
    return E2ETTS_OK;
  };
  // one pass over [B, N, H] (+ the logit weights per workgroup, from L2); 2 N H heads FLOP of logits + the pooling
  const double pool_fl = 2.0 * B * (double)N * H * heads + 4.0 * B * (double)N * H;
  const double pool_by = 4.0 * B * (double)N * H + 4.0 * H * heads;
  for (const FfLayer& f : side.layers) {
    RET(ln(cur, tmp, f.att_lng, f.att_lnb));                                     // PreNorm (:139-141)
    RET(gemm(f.qk, tmp, qk, H, 2 * H, 1, nullptr, nullptr, ACT_NONE));            // query | key (:229-230)
    {
      ProfScope ps(e, "ff_pool", pool_fl, pool_by);                              // pooled query (:232-243)
      KCHK(e, launch_ff_pool(qk, 2 * H, nullptr, side.wql, side.bql, lens, gq, ws, ws_bytes, B, N, H, hs, e->stream));
    }
    {
      ProfScope ps(e, "ff_pool", pool_fl, pool_by + 4.0 * B * H);                // pooled key over k * pooled query (:248-259)
      KCHK(e, launch_ff_pool(qk + H, 2 * H, gq, side.wkl, side.bkl, lens, gk, ws, ws_bytes, B, N, H, hs, e->stream));
    }
    {
      ProfScope ps(e, "ff_scale", 2.0 * B * (double)N * H, 16.0 * B * (double)N * H);
      KCHK(e, launch_ff_scale(qk, 2 * H, gk, cur, att, tmp, B, N, H, e->stream));  // pooled key * query (:262); q + x for the epilogue below
    }
    RET(gemm(f.wt, att, oth, H, H, 1, tmp, lens, ACT_NONE));                     // transform + bias + (q + x), masked_fill (:265, :169-170)
    std::swap(cur, oth);
    RET(ln(cur, tmp, f.ffn_lng, f.ffn_lnb));
    RET(gemm(f.w1, tmp, hid, H, F, c.ffn_k1, nullptr, nullptr, ACT_GELU));         // conv k -> GELU (erf form, :296)
    RET(gemm(f.w2, hid, oth, F, H, 1, cur, lens, ACT_NONE));                      // conv 1 + x, masked_fill (:172-173)
    std::swap(cur, oth);
  }
  if (cur != x) HIPCHK(e, hipMemcpyAsync(x, cur, (size_t)B * N * H * 4, hipMemcpyDeviceToDevice, e->stream));
  return E2ETTS_OK;
}

// conv -> ReLU -> channel LayerNorm(eps 1e-12) [-> x (1 - mask)] stack + small Linear
// (reference DurationPredictor U/layers.py:410-420, VariancePredictor :499-503)
int predictor(e2etts_engine* e, const Predictor& pr, const float* x, float* out, const int32_t* mask_lens, int B, int L,
              const int32_t* act = nullptr, const int32_t* act_host = nullptr, double act_frac = 1.0, bool frame_level = false) {
  const int H = e->cfg.hidden;
  float* a = ptr<float>(e->p1);  // conv output
  float* b = ptr<float>(e->p2);  // LayerNorm output = next layer's input
  const float* in = x;
  int cin = H;
  for (const PredLayer& l : pr.layers) {
    ConvParams p;
    p.B = B; p.T = L; p.in = in; p.w = l.w; p.bias = l.b; p.out = a; p.Cin = cin; p.Cout = pr.chans;
    p.act_rows = act; p.act_rows_host = act_host; p.act_frac = act_frac;
    p.KW = pr.kernel; p.pad = e->cfg.pred_pad_left ? pr.kernel - 1 : (pr.kernel - 1) / 2; p.act = ACT_RELU;  // ConstantPad1d, U/layers.py:400-402
    RET(conv(e, p, 1.0, !frame_level));  // phoneme-level layer: conv_ksplit.hip at every batch size; frame-level (B x T rows): conv_gemm at every batch size
    {
      ProfScope ps(e, "layernorm", 0, 8.0 * B * L * pr.chans);
      KCHK(e, launch_layernorm(a, b, l.g, l.beta, mask_lens, B, L, pr.chans, 1e-12f, e->stream));
    }
    in = b;
    cin = pr.chans;
  }
  {
    ProfScope ps(e, "misc", 0, 0);
    KCHK(e, launch_rowdot(in, pr.lin_w, pr.lin_b, out, mask_lens, B, L, pr.chans, pr.odim, e->stream));
  }
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

int copy_out(e2etts_engine* e, void* dst, const void* src, size_t bytes) {
  HIPCHK(e, hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, e->stream));
  return E2ETTS_OK;
}

__global__ void lens_to_i32_kernel(const int64_t* in, int32_t* out, int B, int L) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B) {
    long long v = in[i];
    out[i] = (int32_t)(v < 0 ? 0 : (v > L ? L : v));
  }
}

// The array controls of e2etts_acoustic_ctl / e2etts_synthesize_ctl: d, p, e (host or device memory; nullptr = the scalar) and their
// counts, already checked by check_controls.
struct CtlArgs {
  const float* v[3] = {nullptr, nullptr, nullptr};
  int n[3] = {0, 0, 0};
};

int check_controls(e2etts_engine* e, const CtlArgs& ctl, int B, int L) {
  static const char* names[3] = {"d_control", "p_control", "e_control"};
  for (int k = 0; k < 3; ++k)
    if (ctl.v[k] && ctl.n[k] != 1 && ctl.n[k] != B && (long long)ctl.n[k] != (long long)B * L)
      return e->fail(E2ETTS_EINVAL, "%s holds %d values: expected 1, B = %d or B * L = %lld", names[k], ctl.n[k], B, (long long)B * L);
  return E2ETTS_OK;
}

// What e2etts_acoustic_forced asked for, resolved against the model (forced_plan; the struct itself passed host_logic.h: forced_check).
struct ForcedPlan {
  const e2etts_forced* f = nullptr;
  bool soft = false;                 // attn_soft: the soft expansion, T and mel_lens as given
  bool has_p = false, has_e = false; // a pitch / an energy target
  bool p_avg = false, e_avg = false; // ... frame-resolved, for a phoneme_level feature: averaged over the durations
  int T = 0;
  const int64_t* mel_lens_host = nullptr;
};

// The variance adaptor's teacher-forced steps (U/layers.py:202-241 with attn_prior): the durations as given, their scan in
// launch_duration's output format, the targets brought to the model's level.  Called where the predicted pass calls launch_duration.
int forced_durations_and_targets(e2etts_engine* e, const ForcedPlan& fp, int B, int L, float d_control, const CtlRef& d_ctl) {
  const auto& c = e->cfg;
  const e2etts_forced& f = *fp.f;
  const size_t BL = (size_t)B * L, BT = (size_t)B * std::max(fp.T, 1);
  if (f.durations) RET(copy_in(e, e->durf.p, f.durations, BL * 4));
  else KCHK(e, launch_duration(ptr<float>(e->logd), d_control, ptr<float>(e->durf), ptr<int32_t>(e->cum), ptr<int64_t>(e->mel64),
                               ptr<int32_t>(e->mel32), B, L, e->stream, d_ctl));
  TeacherScanParams sp;
  sp.dur = ptr<float>(e->durf); sp.txt_lens = ptr<int32_t>(e->lens32); sp.cum = ptr<int32_t>(e->cum);
  sp.mel64 = ptr<int64_t>(e->mel64); sp.mel32 = ptr<int32_t>(e->mel32);
  sp.B = B; sp.L = L; sp.T = fp.T;
  if (fp.soft) {
    RET(ensure(e, e->fmel64, (size_t)B * 8));
    RET(copy_in(e, e->fmel64.p, f.mel_lens, (size_t)B * 8));
    sp.mel_given = ptr<int64_t>(e->fmel64);
  }
  // targets: slot 0 = f0 or pitch, 1 = uv, 2 = energy; each [B, N] at the model's level, N = L (phoneme_level) or T columns (frame_level)
  if (fp.has_p || fp.has_e) {
    const size_t n_lvl = std::max(BL, BT);
    RET(ensure(e, e->ftg, 3 * n_lvl * 4));
    if (fp.p_avg || fp.e_avg) RET(ensure(e, e->ftgf, 3 * BT * 4));
    const float* src[3] = {c.pitch_no_uv ? f.pitch : f.f0, c.pitch_no_uv ? nullptr : f.uv, f.energy};
    for (int k = 0; k < 3; ++k) {
      if (!src[k]) continue;
      const bool avg = k < 2 ? fp.p_avg : fp.e_avg;
      const bool frame = k < 2 ? c.pitch_frame != 0 : c.energy_frame != 0;
      float* lvl = ptr<float>(e->ftg) + k * n_lvl;
      if (avg) {
        float* fr = ptr<float>(e->ftgf) + k * BT;
        RET(copy_in(e, fr, src[k], BT * 4));
        sp.tg[sp.n_tg].src = fr; sp.tg[sp.n_tg].dst = lvl; sp.tg[sp.n_tg].uv = k == 1;
        ++sp.n_tg;
      } else {
        RET(copy_in(e, lvl, src[k], (frame ? BT : BL) * 4));
      }
    }
  }
  KCHK(e, launch_teacher_scan(sp, e->stream));
  return E2ETTS_OK;
}

// launch_variance_embed of one level ([B, N] rows of x) with the features of `feat` that have a target embedded from it
int forced_embed(e2etts_engine* e, const ForcedPlan& fp, float* x, int B, int L, int N, int tld, int feat, float p_control, float e_control,
                 int pitch_mode, const VarCtl& vc) {
  const auto& c = e->cfg;
  const size_t n_lvl = std::max((size_t)B * L, (size_t)B * std::max(fp.T, 1));
  TargetEmbedParams q;
  if ((feat & 1) && fp.has_p) { q.pitch_t = ptr<float>(e->ftg); if (!c.pitch_no_uv) q.uv_t = ptr<float>(e->ftg) + n_lvl; }
  if ((feat & 2) && fp.has_e) q.energy_t = ptr<float>(e->ftg) + 2 * n_lvl;
  if (!q.pitch_t && !q.energy_t) {   // nothing of this level has a target: the predicted pass's own launch
    KCHK(e, launch_variance_embed(x, ptr<float>(e->ppred), ptr<float>(e->epred), p_control, e_control, c.f0_mean, c.f0_std, e->energy_bins, c.n_bins,
                                  e->pitch_emb, e->energy_emb, ptr<int32_t>(e->pidx), ptr<int32_t>(e->eidx), B, N, c.hidden, e->stream, pitch_mode,
                                  e->pitch_bins, feat, vc));
    return E2ETTS_OK;
  }
  q.tld = tld; q.N = N; q.H = c.hidden;
  q.p_control = p_control; q.e_control = e_control; q.f0_mean = c.f0_mean; q.f0_std = c.f0_std;
  q.energy_bins = e->energy_bins; q.pitch_bins = e->pitch_bins; q.n_bins = c.n_bins; q.pitch_mode = pitch_mode; q.feat = feat;
  q.pitch_emb = e->pitch_emb; q.energy_emb = e->energy_emb; q.pitch_idx = ptr<int32_t>(e->pidx); q.energy_idx = ptr<int32_t>(e->eidx);
  q.ctl = vc;
  KCHK(e, launch_target_embed(x, ptr<float>(e->ppred), ptr<float>(e->epred), q, B, e->stream));
  return E2ETTS_OK;
}

int acoustic_impl(e2etts_engine* e, const int64_t* ids, const int64_t* lens, int B, int L, const int64_t* speaker,
                  int n_spk_ids, float d_control, float p_control, float e_control, bool ragged = false, const CtlArgs* ctl = nullptr,
                  const ForcedPlan* fp = nullptr) {
  const auto& c = e->cfg;
  if (!e->ac_loaded) return e->fail(E2ETTS_ESTATE, "acoustic weights not loaded");
  if (!ids || !lens || !speaker) return e->fail(E2ETTS_EINVAL, "ids / lens / speaker must not be NULL");
  if (B <= 0 || L <= 0) return e->fail(E2ETTS_EINVAL, "B and L must be positive (got B=%d L=%d)", B, L);
  if (n_spk_ids != 1 && n_spk_ids != B) return e->fail(E2ETTS_EINVAL, "speaker must hold 1 or B ids");
  if (L > c.max_seq_len && L > c.pos_table_rows)
    return e->fail(E2ETTS_EINVAL, "L=%d exceeds the shipped position table (%d rows)", L, c.pos_table_rows);
  if ((uint64_t)L + 1 > e->var_pos_rows)
    return e->fail(E2ETTS_EINVAL, "L=%d exceeds the variance-predictor position table (%llu rows)", L,
                   (unsigned long long)e->var_pos_rows);
  // host-side validation when the caller's buffers are host memory (KeyError / IndexError in the reference)
  if (!is_device_pointer(ids) && !is_device_pointer(lens)) {
    for (int b = 0; b < B; ++b)
      if (lens[b] < 1 || lens[b] > L) return e->fail(E2ETTS_EINVAL, "lens[%d]=%lld outside [1, %d]", b, (long long)lens[b], L);
    for (long long i = 0; i < (long long)B * L; ++i)
      if (ids[i] < 0 || ids[i] > c.n_symbols) return e->fail(E2ETTS_EINVAL, "symbol id %lld out of range", (long long)ids[i]);
  }
  if (!is_device_pointer(speaker))
    for (int i = 0; i < n_spk_ids; ++i)
      if (speaker[i] < 0 || speaker[i] >= c.n_speakers) return e->fail(E2ETTS_EINVAL, "speaker id %lld out of range", (long long)speaker[i]);

  const int H = c.hidden, F = c.ffn_dim;
  const size_t BL = (size_t)B * L;
  RET(ensure(e, e->ids, BL * 8));
  RET(ensure(e, e->lens64, (size_t)B * 8));
  RET(ensure(e, e->lens32, (size_t)B * 4));
  RET(ensure(e, e->spk, (size_t)B * 8));
  RET(ensure(e, e->xa, BL * H * 4));
  RET(ensure(e, e->xb, BL * H * 4));
  RET(ensure(e, e->xs, BL * H * 4));
  RET(ensure(e, e->xp, BL * H * 4));
  RET(ensure(e, e->tmp, BL * H * 4));
  RET(ensure(e, e->qkv, BL * 3 * H * 4));
  RET(ensure(e, e->att, BL * H * 4));
  RET(ensure(e, e->hid, BL * F * 4));
  const size_t pc = std::max(c.dur_chans, c.var_chans);
  RET(ensure(e, e->p1, BL * pc * 4));
  RET(ensure(e, e->p2, BL * pc * 4));
  RET(ensure(e, e->logd, BL * 4));
  RET(ensure(e, e->durf, BL * 4));
  RET(ensure(e, e->cum, BL * 4));
  RET(ensure(e, e->mel64, (size_t)B * 8));
  RET(ensure(e, e->mel32, (size_t)B * 4));
  RET(ensure(e, e->posbuf, BL * 4));
  RET(ensure(e, e->ppred, BL * 2 * 4));
  RET(ensure(e, e->epred, BL * 4));
  RET(ensure(e, e->pidx, BL * 4));
  RET(ensure(e, e->eidx, BL * 4));

  e->have_acoustic = false;
  e->forced_last = e->forced_pitch = e->forced_energy = false;
  RET(copy_in(e, e->ids.p, ids, BL * 8));
  RET(copy_in(e, e->lens64.p, lens, (size_t)B * 8));
  RET(copy_in(e, e->spk.p, speaker, (size_t)n_spk_ids * 8));
  // array controls: copied into the engine's control workspace, read there with the stride their count gives (kernels.h: CtlRef)
  CtlRef cref[3];
  if (ctl) {
    RET(ensure(e, e->ctlbuf, 3 * BL * 4));
    for (int k = 0; k < 3; ++k) {
      if (!ctl->v[k]) continue;
      float* dst = ptr<float>(e->ctlbuf) + k * BL;
      RET(copy_in(e, dst, ctl->v[k], (size_t)ctl->n[k] * 4));
      cref[k].p = dst;
      if ((size_t)ctl->n[k] == BL && ctl->n[k] != B) { cref[k].sb = L; cref[k].sl = 1; }   // per phoneme, [B, L] row-major
      else if (ctl->n[k] == B) { cref[k].sb = 1; cref[k].sl = 0; }                          // per utterance
      else { cref[k].sb = 0; cref[k].sl = 0; }                                              // one value for the batch
    }
  }
  hipLaunchKernelGGL(lens_to_i32_kernel, dim3((B + 63) / 64), dim3(64), 0, e->stream, ptr<int64_t>(e->lens64),
                     ptr<int32_t>(e->lens32), B, L);
  const int32_t* tl = ptr<int32_t>(e->lens32);

  // Encoder (U/blocks/transformer.py:58-86): embedding + position table, 6 x FFTBlock
  const float* pos = L > c.max_seq_len ? e->pos_regen : e->enc_pos;  // eval-time regeneration branch (:68-73)
  float* x = ptr<float>(e->xa);
  {
    ProfScope ps(e, "misc", 0, 0);
    KCHK(e, launch_embed(ptr<int64_t>(e->ids), e->emb, pos, x, B, L, H, c.n_symbols + 1, e->stream));
  }
  // Ragged mode at the phoneme level (synthesize, lengths in HOST memory -- the compact grids are built from them).  FFT blocks and
  // duration predictor: every consumer of a row >= len masks it (keys masked, LayerNorm kernels write zeros there), so their convolutions
  // compute rows < len only.  Pitch / energy predictors are unmasked stacks of n convolutions of kernel k: the rows < len that the bucket
  // kernel reads depend on rows < len + (n - 1)(k - 1)/2 of the layers before, so every layer computes that many (cap L).
  const int32_t *act_enc = nullptr, *act_enc_h = nullptr, *act_var = nullptr, *act_var_h = nullptr;
  double frac_enc = 1.0, frac_var = 1.0;
  bool enc_short = false;  // some utterance is shorter than the padded length (else every limit equals L: nothing to skip, and the
                           // launches keep their plain grids -- the B = 1 latency path pays no act_rows kernels)
  if (ragged && c.block_type == 0 && !is_device_pointer(lens))
    for (int b = 0; b < B; ++b) enc_short = enc_short || lens[b] < L;
  if (enc_short) {
    RET(ensure(e, e->actbuf, (size_t)(5 + c.voc_stages) * B * 4));
    e->h_act.resize((size_t)(5 + c.voc_stages) * B, 0);
    int32_t* he = e->h_act.data() + (size_t)(3 + c.voc_stages) * B;
    int32_t* hv = he + B;
    // (one limit for both variance predictors: the deeper reach of the two)
    const int add_var = std::max((c.var_layers - 1) * ((c.var_kernel - 1) / 2),
                                 ((c.energy_layers ? c.energy_layers : c.var_layers) - 1) * (((c.energy_kernel ? c.energy_kernel : c.var_kernel) - 1) / 2));
    double se = 0, sv = 0;
    for (int b = 0; b < B; ++b) {
      he[b] = (int32_t)std::min<long long>(std::max<long long>(lens[b], 0), L);   // lens_to_i32_kernel's clamp
      hv[b] = (int32_t)std::min<long long>((long long)he[b] + add_var, L);        // act_rows_kernel's arithmetic
      se += he[b];
      sv += hv[b];
    }
    int32_t* dv = ptr<int32_t>(e->actbuf) + (size_t)(4 + c.voc_stages) * B;
    KCHK(e, launch_act_rows(tl, dv, B, add_var, 1, L, e->stream));
    act_enc = tl; act_enc_h = he; act_var = dv; act_var_h = hv;
    frac_enc = se / ((double)B * L);
    frac_var = sv / ((double)B * L);
  }
  if (c.block_type == 1) RET(conformer_stack(e, e->cf_enc, c.n_head, x, ptr<float>(e->xb), tl, B, L, false));
  else if (c.block_type == 2) RET(fastformer_stack(e, e->ff_enc, x, ptr<float>(e->xb), tl, B, L, false));
  else RET(fft_stack(e, e->enc, c.n_head, x, ptr<float>(e->xb), tl, B, L, false, act_enc, frac_enc, true, act_enc_h));  // encoder: always exact fp32, K-split kernel

  // Variance adaptor, inference branch (U/layers.py:195-258)
  float* xs = ptr<float>(e->xs);
  {
    ProfScope ps(e, "misc", 0, 0);
    KCHK(e, launch_add_speaker(x, xs, e->spk_emb, ptr<int64_t>(e->spk), n_spk_ids, c.n_speakers, B, L, H, e->stream));
  }
  RET(predictor(e, e->dur, xs, ptr<float>(e->logd), tl, B, L, act_enc, act_enc_h, frac_enc));
  if (fp) {   // teacher-forced: given durations, targets (the predictors still run: their outputs are returned)
    ProfScope ps(e, "misc", 0, 0);
    RET(forced_durations_and_targets(e, *fp, B, L, d_control, cref[0]));
  } else {
    ProfScope ps(e, "misc", 0, 0);
    KCHK(e, launch_duration(ptr<float>(e->logd), d_control, ptr<float>(e->durf), ptr<int32_t>(e->cum),
                            ptr<int64_t>(e->mel64), ptr<int32_t>(e->mel32), B, L, e->stream, cref[0]));
  }
  const bool soft = fp && fp->soft;   // T and the mel lengths are the caller's: nothing to wait for
  hipEvent_t mel_ready = nullptr;
  if (!soft) {
    HIPCHK(e, hipMemcpyAsync(e->h_mel, e->mel64.p, (size_t)B * 8, hipMemcpyDeviceToHost, e->stream));
    mel_ready = get_event(e);
    HIPCHK(e, hipEventRecord(mel_ready, e->stream));
  }
  // pitch / energy predictors run while the mel lengths travel to the host
  float* xp = ptr<float>(e->xp);
  const bool p_frame = c.pitch_frame != 0, e_frame = c.energy_frame != 0;   // frame_level features wait for the length regulator (below)
  const int pitch_mode = c.pitch_no_uv ? 2 : (c.pitch_log2 ? 1 : 0);
  if (!p_frame) {
    {
      ProfScope ps(e, "misc", 0, 0);
      KCHK(e, launch_var_positions(xs, ptr<int32_t>(e->posbuf), e->var_pos, (int)e->var_pos_rows, e->pitch.alpha, xp, B, L, H, e->stream));
    }
    RET(predictor(e, e->pitch, xp, ptr<float>(e->ppred), nullptr, B, L, act_var, act_var_h, frac_var));
  }
  if (!e_frame) {
    {
      ProfScope ps(e, "misc", 0, 0);
      KCHK(e, launch_var_positions(xs, ptr<int32_t>(e->posbuf), e->var_pos, (int)e->var_pos_rows, e->energy.alpha, xp, B, L, H, e->stream,
                                   p_frame));  // the positions depend on xs alone: the pitch predictor's pass (if it ran) left them in posbuf
    }
    RET(predictor(e, e->energy, xp, ptr<float>(e->epred), nullptr, B, L, act_var, act_var_h, frac_var));
  }
  if (!p_frame || !e_frame) {
    ProfScope ps(e, "misc", 0, 0);
    VarCtl vc;   // (the features computed here read their controls by phoneme)
    vc.p = p_frame ? CtlRef() : cref[1];
    vc.e = e_frame ? CtlRef() : cref[2];
    vc.N = L;
    if (fp) {
      RET(forced_embed(e, *fp, xs, B, L, L, L, (p_frame ? 0 : 1) | (e_frame ? 0 : 2), p_control, e_control, pitch_mode, vc));
    } else {
      KCHK(e, launch_variance_embed(xs, ptr<float>(e->ppred), ptr<float>(e->epred), p_control, e_control, c.f0_mean, c.f0_std,
                                    e->energy_bins, c.n_bins, e->pitch_emb, e->energy_emb, ptr<int32_t>(e->pidx),
                                    ptr<int32_t>(e->eidx), B, L, H, e->stream, pitch_mode, e->pitch_bins, (p_frame ? 0 : 1) | (e_frame ? 0 : 2), vc));
    }
  }
  long long T = 0;
  if (soft) {
    // the mel lengths as the scan kernel clamps them; given in device memory, every utterance counts as T frames long on the host (the
    // launch grids stay padded; the kernels mask by the device copy)
    T = fp->T;
    for (int b = 0; b < B; ++b) e->h_mel[b] = fp->mel_lens_host ? std::min<long long>(std::max<long long>(fp->mel_lens_host[b], 0), T) : T;
  } else {
    // the one host synchronisation of the acoustic model: T = max(mel_lens) sizes everything downstream
    HIPCHK(e, hipEventSynchronize(mel_ready));
    e->ev_pool.push_back(mel_ready);
    for (int b = 0; b < B; ++b) T = std::max<long long>(T, e->h_mel[b]);
  }
  if (T <= 0)
    return e->fail(E2ETTS_EINVAL, fp && fp->f->durations ? "every given duration is zero (or was clamped to zero): nothing to synthesise"
                                                         : "every predicted duration is zero: nothing to synthesise");
  if (T > c.max_seq_len && T > c.pos_table_rows)
    return e->fail(E2ETTS_EINVAL, "T=%lld exceeds the shipped position table (%d rows)", T, c.pos_table_rows);
  if (T > (1 << 20)) return e->fail(E2ETTS_EINVAL, "T=%lld is unreasonably large", T);
  if (fp && !soft && ((fp->has_p && c.pitch_frame) || (fp->has_e && c.energy_frame)) && T > fp->T)
    return e->fail(E2ETTS_EINVAL, "the durations give T=%lld frames, the frame_level targets have %d columns", T, fp->T);
  const size_t BT = (size_t)B * T;
  RET(ensure(e, e->dx, BT * H * 4));
  RET(ensure(e, e->dxb, BT * H * 4));
  RET(ensure(e, e->tmp, BT * H * 4));
  RET(ensure(e, e->qkv, BT * 3 * H * 4));
  RET(ensure(e, e->att, BT * H * 4));
  RET(ensure(e, e->hid, BT * F * 4));
  RET(ensure(e, e->mel, BT * c.n_mel * 4));
  RET(ensure(e, e->melpost, BT * c.n_mel * 4));
  RET(ensure(e, e->pn1, BT * c.postnet_dim * 4));
  RET(ensure(e, e->pn2, BT * c.postnet_dim * 4));

  // Length regulator (U/layers.py:423-457) fused with the decoder's position add (U/blocks/transformer.py:138-153)
  const float* dpos = T > c.max_seq_len ? e->pos_regen : e->dec_pos;
  float* dx = ptr<float>(e->dx);
  const int32_t* ml = ptr<int32_t>(e->mel32);
  if (soft) {
    // soft expansion (U/layers.py:244-245) fused with the position add, exact fp32; ragged: rows < mel_len only (a frame_level feature's
    // predictors read every row: padded then)
    SoftExpandParams sx;
    sx.attn = fp->f->attn_soft;
    if (!is_device_pointer(sx.attn)) {
      RET(ensure(e, e->fattn, BT * L * 4));
      RET(copy_in(e, e->fattn.p, sx.attn, BT * L * 4));
      sx.attn = ptr<float>(e->fattn);
    }
    sx.x = xs; sx.txt_lens = tl; sx.pos = (p_frame || e_frame) ? nullptr : dpos; sx.out = dx;
    sx.B = B; sx.T = (int)T; sx.L = L; sx.H = H;
    bool any_short = false;
    for (int b = 0; b < B; ++b) any_short = any_short || e->h_mel[b] < T;
    if (ragged && any_short && !p_frame && !e_frame) {
      e->h_act.resize((size_t)(5 + c.voc_stages) * B, 0);
      for (int b = 0; b < B; ++b) e->h_act[b] = (int32_t)e->h_mel[b];
      sx.act_rows = ml; sx.act_rows_host = e->h_act.data();
    }
    ProfScope ps(e, "soft_expand", soft_expand_flops(sx), 4.0 * ((double)BT * L + (double)BL * H + (double)BT * H));
    KCHK(e, launch_soft_expand(sx, e->stream));
  } else {
    ProfScope ps(e, "misc", 0, 0);
    KCHK(e, launch_length_regulate(xs, ptr<int32_t>(e->cum), ml, (p_frame || e_frame) ? nullptr : dpos, dx, B, L, (int)T, H, e->stream));
  }
  if (p_frame || e_frame) {
    // frame_level pitch / energy (U/layers.py:249-257): both predictors read the length regulator's output, their embeddings are added
    // to it -- on every row, padded ones included, as the reference does; the decoder masks those -- and the decoder's positions follow
    if (T + 1 > (long long)e->var_pos_rows)
      return e->fail(E2ETTS_EINVAL, "T=%lld exceeds the variance predictors' position table (%lld rows)", T, (long long)e->var_pos_rows);
    const size_t pcw = (size_t)std::max(c.dur_chans, c.var_chans);
    RET(ensure(e, e->p1, BT * pcw * 4));
    RET(ensure(e, e->p2, BT * pcw * 4));
    RET(ensure(e, e->posbuf, BT * 4));
    if (p_frame) { RET(ensure(e, e->ppred, BT * 2 * 4)); RET(ensure(e, e->pidx, BT * 4)); }
    if (e_frame) { RET(ensure(e, e->epred, BT * 4)); RET(ensure(e, e->eidx, BT * 4)); }
    float* xpf = ptr<float>(e->dxb);   // [B, T, H]: free until the decoder starts
    if (p_frame) {
      {
        ProfScope ps(e, "misc", 0, 0);
        KCHK(e, launch_var_positions(dx, ptr<int32_t>(e->posbuf), e->var_pos, (int)e->var_pos_rows, e->pitch.alpha, xpf, B, (int)T, H, e->stream));
      }
      RET(predictor(e, e->pitch, xpf, ptr<float>(e->ppred), nullptr, B, (int)T, nullptr, nullptr, 1.0, true));
    }
    if (e_frame) {
      {
        ProfScope ps(e, "misc", 0, 0);
        KCHK(e, launch_var_positions(dx, ptr<int32_t>(e->posbuf), e->var_pos, (int)e->var_pos_rows, e->energy.alpha, xpf, B, (int)T, H, e->stream,
                                     !p_frame));
      }
      RET(predictor(e, e->energy, xpf, ptr<float>(e->epred), nullptr, B, (int)T, nullptr, nullptr, 1.0, true));
    }
    ProfScope ps(e, "misc", 0, 0);
    VarCtl vc;   // frame level: a per-phoneme control is expanded along the rounded durations (include/e2etts.h: e2etts_acoustic_ctl)
    vc.p = p_frame ? cref[1] : CtlRef();
    vc.e = e_frame ? cref[2] : CtlRef();
    vc.N = (int)T;
    vc.cum = ptr<int32_t>(e->cum);
    vc.Lp = L;
    if (fp) {
      RET(forced_embed(e, *fp, dx, B, L, (int)T, fp->T, (p_frame ? 1 : 0) | (e_frame ? 2 : 0), p_control, e_control, pitch_mode, vc));
    } else {
      KCHK(e, launch_variance_embed(dx, ptr<float>(e->ppred), ptr<float>(e->epred), p_control, e_control, c.f0_mean, c.f0_std,
                                    e->energy_bins, c.n_bins, e->pitch_emb, e->energy_emb, ptr<int32_t>(e->pidx),
                                    ptr<int32_t>(e->eidx), B, (int)T, H, e->stream, pitch_mode, e->pitch_bins, (p_frame ? 1 : 0) | (e_frame ? 2 : 0), vc));
    }
    KCHK(e, launch_add_positions(dx, dpos, B, (int)T, H, e->stream));
  }
  if (fp) {   // tap "dec_in": the decoder works in place on dx
    RET(ensure(e, e->decin, BT * H * 4));
    HIPCHK(e, hipMemcpyAsync(e->decin.p, dx, BT * H * 4, hipMemcpyDeviceToDevice, e->stream));
  }
  // Ragged mode (synthesize only).  Decoder: every consumer of a row >= mel_len masks it (keys are masked, the LayerNorm
  // kernels write zeros there), so its convolutions compute rows < mel_len only and valid rows stay bit-identical.
  // mel_linear / postnet are unmasked and the vocoder reads `halo` frames past the end, so they compute rows
  // < mel_len + halo + 2 * postnet_layers; rows beyond hold stale finite values that no valid sample depends on.
  const int32_t *act_dec = nullptr, *act_post = nullptr, *act_dec_h = nullptr, *act_post_h = nullptr;
  // (equal lengths -- B = 1, a fixed-length batch --: every limit would equal T; nothing is skipped and no act_rows kernel is launched)
  e->rag_short = false;
  for (int b = 0; b < B; ++b) e->rag_short = e->rag_short || e->h_mel[b] < T;
  if (ragged && e->rag_short) {
    RET(ensure(e, e->actbuf, (size_t)(5 + c.voc_stages) * B * 4));
    int32_t* ab = ptr<int32_t>(e->actbuf);
    const int halo = vocoder_halo_frames(c);
    KCHK(e, launch_act_rows(ml, ab, B, 0, 1, T, e->stream));
    KCHK(e, launch_act_rows(ml, ab + B, B, halo + 2 * c.postnet_layers * ((c.postnet_kernel - 1) / 2), 1, T, e->stream));
    act_dec = ab;
    act_post = ab + B;
    double sd = 0, sp = 0, sv = 0;  // the same limits on the host (mel lengths are in e->h_mel since the sync above)
    const long long add_post = halo + 2 * c.postnet_layers * ((c.postnet_kernel - 1) / 2);
    e->h_act.resize((size_t)(5 + c.voc_stages) * B, 0);
    for (int b = 0; b < B; ++b) {
      const long long m32 = std::min<long long>(e->h_mel[b], 0x7fffffffLL);  // what duration_kernel wrote to mel32 (act_rows_kernel's input)
      e->h_act[b] = (int32_t)std::min<long long>(m32, T);
      e->h_act[(size_t)B + b] = (int32_t)std::min<long long>(m32 + add_post, T);
      sd += (double)std::min<long long>(e->h_mel[b], T);
      sp += (double)std::min<long long>(e->h_mel[b] + add_post, T);
      sv += (double)std::min<long long>(e->h_mel[b] + halo, T);
    }
    act_dec_h = e->h_act.data();
    act_post_h = e->h_act.data() + B;
    e->rag_frac_dec = sd / ((double)B * T);
    e->rag_frac_post = sp / ((double)B * T);
    e->rag_frac_voc = sv / ((double)B * T);
  }
  // (a Conformer decoder computes every row: its attention is unmasked and its depthwise convolution crosses into the padding; so does a
  // Fastformer decoder: its inverted mask puts the pooling weight ON the padding)
  const int dec_heads = c.dec_n_head ? c.dec_n_head : c.n_head;
  if (c.block_type == 1) RET(conformer_stack(e, e->cf_dec, dec_heads, dx, ptr<float>(e->dxb), ml, B, (int)T, e->dec_precision == 1));
  else if (c.block_type == 2) RET(fastformer_stack(e, e->ff_dec, dx, ptr<float>(e->dxb), ml, B, (int)T, e->dec_precision == 1));
  else RET(fft_stack(e, e->dec, dec_heads, dx, ptr<float>(e->dxb), ml, B, (int)T, e->dec_precision == 1, act_dec, act_dec ? e->rag_frac_dec : 1.0, false, act_dec_h));
  // mel_linear (U/model.py:186)
  ConvParams p;
  auto setw = [&](ConvParams& q, const ConvW& w) {
    q.bias = w.b;
    if (e->dec_precision == 1 && w.wx3) { q.w = w.wx3; q.x3 = 1; }
    else { q.w = w.w; q.x3 = 0; }
  };
  p.B = B; p.T = (int)T; p.act_rows = act_post; p.act_rows_host = act_post_h; p.act_frac = act_post ? e->rag_frac_post : 1.0; p.in = dx; setw(p, e->mel_lin); p.out = ptr<float>(e->mel); p.Cin = H; p.Cout = c.n_mel;
  RET(conv(e, p));
  // Postnet (U/layers.py:556-563; BatchNorm folded at pack time) + residual (U/model.py:188); unmasked
  const float* pin = ptr<float>(e->mel);
  int cin = c.n_mel;
  float* bufs[2] = {ptr<float>(e->pn1), ptr<float>(e->pn2)};
  for (int i = 0; i < c.postnet_layers; ++i) {
    const bool last = i == c.postnet_layers - 1;
    p = ConvParams();
    p.B = B; p.T = (int)T; p.act_rows = act_post; p.act_rows_host = act_post_h; p.act_frac = act_post ? e->rag_frac_post : 1.0; p.in = pin; setw(p, e->postnet[i]); p.Cin = cin;
    p.Cout = last ? c.n_mel : c.postnet_dim; p.KW = c.postnet_kernel; p.pad = (c.postnet_kernel - 1) / 2;
    if (last) { p.out = ptr<float>(e->melpost); p.res = ptr<float>(e->mel); }
    else { p.out = bufs[i & 1]; p.act = ACT_TANH; }
    RET(conv(e, p));
    pin = p.out;
    cin = p.Cout;
  }
  e->last_B = B; e->last_L = L; e->last_T = (int)T;
  e->have_acoustic = true;
  if (fp) { e->forced_last = true; e->forced_pitch = fp->has_p; e->forced_energy = fp->has_e; e->forced_T = fp->T; }
  return E2ETTS_OK;
}

// ---- the ResBlock launches of the two vocoder walks (vocoder_impl, vocoder_act16): one set of builders

// How a walk reads a convolution's weights.  kind 0, vocoder_impl: fp32 biases, the fragment-order pair images and -- in plain bf16 --
// the conv_bf16.hip images of bimg_of; kind 1 / 2, vocoder_act16: bf16 / fp16 elements, i.e. the images of bimg_of | bimg_act / himg_of and
// the parameters rounded to that type (r16_of / r16h_of).
struct VocWeights {
  const e2etts_engine* e;
  int kind;
  const float* param(const float* p) const {   // a bias (conv_post's weights) as the walk's arithmetic takes it
    if (!kind) return p;
    const auto& tab = kind == 2 ? e->r16h_of : e->r16_of;
    auto it = tab.find(p);
    return it == tab.end() ? nullptr : it->second;
  }
  const void* image(const ConvW& w, int* split = nullptr) const {   // null: the walk has no such image
    if (kind == 2) {
      auto ih = e->himg_of.find(w.w);
      if (ih == e->himg_of.end()) return nullptr;
      if (split) *split = ih->second.second;
      return ih->second.first;
    }
    if (!w.wx3 || (!kind && e->voc_precision != E2ETTS_PRECISION_BF16)) return nullptr;
    auto it = e->bimg_of.find(w.wx3);
    if (it == e->bimg_of.end()) {
      if (!kind) return nullptr;
      it = e->bimg_act.find(w.wx3);
      if (it == e->bimg_act.end()) return nullptr;
    }
    if (split) *split = it->second.second;
    return it->second.first;
  }
  const float* pair_frag(size_t idx, size_t m) const {   // resblock_pair.hip's image of pair m (null where bind_vocoder built none)
    if (kind) return nullptr;
    const auto& tab = e->voc_precision == E2ETTS_PRECISION_FP32 ? e->rb_pair_frag32 : e->rb_pair_frag;
    return idx < tab.size() && m < tab[idx].size() ? tab[idx][m] : nullptr;
  }
  int pair_mode() const { return kind ? kind + 2 : e->voc_precision; }   // PairParams::mode
  const char* cls() const { return kind == 2 ? "fp16_act" : (kind ? "bf16_act" : "bf16"); }   // in the profile classes of the conv_bf16.hip launches
  double elt() const { return kind ? 0.5 : 1.0; }   // activation bytes per element over fp32's: scales the *_bytes() figures
};

struct RbStage {   // the ResBlocks of vocoder stage `stage`: B x n rows of co channels
  int stage, B, co;
  long long n;
};

// The {stage sum, ping, pong} buffers of ResBlock j within a pass: the main ones, or those a ResBlock beside ResBlock 0 has for itself
struct RbBufs {
  float *S, *T1, *CUR;
};
RbBufs rb_bufs(VocPass& P, int j) {
  if (j == 0) return {ptr<float>(P.v0), ptr<float>(P.v2), ptr<float>(P.v3)};
  return {ptr<float>(P.vside[j - 1][0]), ptr<float>(P.vside[j - 1][1]), ptr<float>(P.vside[j - 1][2])};
}

// dispatch order inside a grouped launch: largest kernel size first
void rb_order(const e2etts_config& c, int* order) {
  for (int j = 0; j < c.voc_n_kernels; ++j) order[j] = j;
  std::sort(order, order + c.voc_n_kernels, [&](int a, int b) { return c.voc_rb_kernel[a] > c.voc_rb_kernel[b]; });
}

// How ResBlock j closes (V/generator.py:44-48): on one stream the last pair of ResBlock j > 0 adds to the sum the ResBlocks before it left in S
// and the last ResBlock divides by num_kernels; side by side every ResBlock writes a sum of its own and the join does both.
struct Closing {
  int accumulate;
  float out_div;
};
Closing closing(int j, bool last_pair, int nk, bool side_by_side) {
  const bool acc = last_pair && !side_by_side && j > 0;
  return {acc ? 1 : 0, acc && j == nk - 1 ? (float)nk : 1.0f};
}

// Pair m of ResBlock j (V/layers.py:35-39) as one fused launch; the caller adds x, out, the row limits and the closing
PairParams pair_params(const VocWeights& w, const RbStage& g, int j, int m) {
  const auto& c = w.e->cfg;
  const size_t idx = (size_t)g.stage * c.voc_n_kernels + j;
  const ConvW &c1 = w.e->rb_c1[idx][m], &c2 = w.e->rb_c2[idx][m];
  PairParams q;
  q.wfrag = w.pair_frag(idx, m); q.b1 = w.param(c1.b); q.b2 = w.param(c2.b); q.bimg1 = w.image(c1); q.bimg2 = w.image(c2);
  q.B = g.B; q.T = (int)g.n; q.C = g.co; q.KW = c.voc_rb_kernel[j]; q.dil = c.voc_rb_dil[j][m];
  q.x_bs = q.out_bs = g.n * g.co; q.slope = 0.1f; q.mode = w.pair_mode();
  return q;
}

// The same pair as two conv_bf16 launches with a 16-bit hand-over: a: mid = bf16(lrelu(c1(lrelu(x)) + b1)), conv2's operand as it is;
// z: out = c2(mid) + b2 + x.  The caller adds the closing.
void handover_params(const VocWeights& w, const RbStage& g, int j, int m, const void* x, void* mid, void* out, BConvParams& a, BConvParams& z) {
  const auto& c = w.e->cfg;
  const size_t idx = (size_t)g.stage * c.voc_n_kernels + j;
  const int k = c.voc_rb_kernel[j], d = c.voc_rb_dil[j][m];
  a = BConvParams();
  a.in = x; a.in_bf16 = w.kind ? 1 : 0; a.in_slope = 0.1f; a.wimg = w.image(w.e->rb_c1[idx][m]); a.KWe = a.KW = k; a.dil = d; a.pad = (k * d - d) / 2;
  a.bias = w.param(w.e->rb_c1[idx][m].b); a.act_slope = 0.1f; a.out_b = mid; a.act16 = w.kind; a.B = g.B; a.T = (int)g.n; a.Cin = a.Cout = g.co;
  z = BConvParams();
  z.in = mid; z.in_bf16 = 1; z.wimg = w.image(w.e->rb_c2[idx][m]); z.KWe = z.KW = k; z.dil = 1; z.pad = (k - 1) / 2;
  z.bias = w.param(w.e->rb_c2[idx][m].b); z.res = reinterpret_cast<const float*>(x); z.act16 = w.kind; z.B = g.B; z.T = (int)g.n; z.Cin = z.Cout = g.co;
  if (w.kind) z.out_b = out;
  else z.out = reinterpret_cast<float*>(out);
}

// The whole ResBlock1 j as one launch (conv_bf16.hip: rb_bf16), x -> out; false: not served (plain bf16 and the 16-bit-activation modes only)
bool rb_params(const VocWeights& w, const RbStage& g, int j, const float* x, float* out, RbParams& r) {
  const auto& c = w.e->cfg;
  if ((!w.kind && w.e->voc_precision != E2ETTS_PRECISION_BF16) || c.voc_resblock != 1 || c.voc_n_dil > RB_MAX_PAIRS) return false;
  const size_t idx = (size_t)g.stage * c.voc_n_kernels + j;
  r = RbParams();
  r.x = x; r.out = out; r.n_pairs = c.voc_n_dil; r.B = g.B; r.T = (int)g.n; r.C = g.co; r.KW = c.voc_rb_kernel[j];
  r.x_bs = r.out_bs = g.n * g.co; r.slope = 0.1f; r.act16 = w.kind;
  for (int m = 0; m < c.voc_n_dil; ++m) {
    r.bimg[m][0] = w.image(w.e->rb_c1[idx][m]); r.bimg[m][1] = w.image(w.e->rb_c2[idx][m]);
    if (!r.bimg[m][0] || !r.bimg[m][1]) return false;
    r.b1[m] = w.param(w.e->rb_c1[idx][m].b); r.b2[m] = w.param(w.e->rb_c2[idx][m].b); r.dil[m] = c.voc_rb_dil[j][m];
  }
  return rb_bf16_supported(r);
}

// Every ResBlock of the stage on x and their sum / num_kernels into out as ONE launch, where rb_bf16's stage form serves it (32 channels): x
// read once, the sum written once, nothing left to join.  rq [num_kernels]: the ResBlocks' parameters in j order -- the kernel adds their
// results as the join does, (S_0 + S_1) + S_2; all: each of them can run as a launch of its own (the caller's other rb_bf16 forms start
// from rq), fl: their FLOPs; done: the stage has been launched.
int whole_stage(e2etts_engine* e, const VocWeights& w, const RbStage& g, const float* x, float* out, RbParams* rq, bool& all, double& fl, bool& done) {
  const int nk = e->cfg.voc_n_kernels;
  all = true; fl = 0; done = false;
  for (int j = 0; j < nk && all; ++j) {
    all = rb_params(w, g, j, x, out, rq[j]);
    if (all) fl += rb_bf16_flops(rq[j]);
  }
  if (!all || !rb_bf16_stage_supported(rq, nk)) return E2ETTS_OK;
  char nm[48];
  snprintf(nm, sizeof nm, "rb_%s_stage_%d", w.cls(), g.co);
  ProfScope ps(e, nm, fl, 4.0 * w.elt() * 2.0 * g.B * (double)g.n * g.co);
  KCHK(e, launch_rb_bf16_stage(rq, nk, e->stream));
  done = true;
  return E2ETTS_OK;
}

int whole_stage(e2etts_engine* e, const VocWeights& w, const RbStage& g, const float* x, float* out, bool& done) {   // for a caller with no other rb_bf16 form
  RbParams rq[E2ETTS_MAX_RB_KERNELS];
  bool all;
  double fl;
  return whole_stage(e, w, g, x, out, rq, all, fl, done);
}

// Every ResBlock of the stage in one launch, each into the sum buffer of its own (rb_bufs); the sums are joined downstream.  rq, fl: of whole_stage
int rb_group(e2etts_engine* e, const VocWeights& w, const RbStage& g, VocPass& P, const RbParams* rq, double fl) {
  const int nk = e->cfg.voc_n_kernels;
  RbParams gq[E2ETTS_MAX_RB_KERNELS];
  int order[E2ETTS_MAX_RB_KERNELS];
  rb_order(e->cfg, order);
  double by = 0;
  for (int t = 0; t < nk; ++t) {
    gq[t] = rq[order[t]];
    gq[t].out = rb_bufs(P, order[t]).S;
    by += rb_bf16_bytes(gq[t]) * w.elt();
  }
  char nm[48];
  snprintf(nm, sizeof nm, "rb_%s_group_%d", w.cls(), g.co);
  ProfScope ps(e, nm, fl, by);
  KCHK(e, launch_rb_bf16_group(gq, nk, e->stream));
  return E2ETTS_OK;
}

// One ResBlock as a launch of its own, closing as cl says
int rb_single(e2etts_engine* e, const VocWeights& w, const RbStage& g, RbParams& r, Closing cl) {
  r.accumulate = cl.accumulate; r.out_div = cl.out_div;
  char nm[48];
  snprintf(nm, sizeof nm, "rb_%s_%d", w.cls(), g.co);
  ProfScope ps(e, nm, rb_bf16_flops(r), rb_bf16_bytes(r) * w.elt());
  KCHK(e, launch_rb_bf16(r, e->stream));
  return E2ETTS_OK;
}

// Pair m of EVERY ResBlock of the stage in one launch, ResBlock j in its own buffers: cur[j], its running x, moves on to what the pair
// wrote (the sum buffer after the last pair; x and out must differ, so the running x ping-pongs CUR / T1)
int pair_group(e2etts_engine* e, const VocWeights& w, const RbStage& g, VocPass& P, int m, const int* order, const float** cur) {
  const int nk = e->cfg.voc_n_kernels;
  PairParams qs[E2ETTS_MAX_RB_KERNELS];
  double fl = 0, by = 0;
  for (int t = 0; t < nk; ++t) {
    const int j = order[t];
    const RbBufs b = rb_bufs(P, j);
    PairParams& q = qs[t];
    q = pair_params(w, g, j, m);
    q.x = cur[j];
    q.out = m == e->cfg.voc_n_dil - 1 ? b.S : (cur[j] == b.CUR ? b.T1 : b.CUR);
    fl += resblock_pair_flops(q); by += resblock_pair_bytes(q) * w.elt();
  }
  char nm[48];
  snprintf(nm, sizeof nm, "pair_%s_group_%d", w.cls(), g.co);
  ProfScope ps(e, nm, fl, by);
  KCHK(e, launch_pair_bf16_group(qs, nk, e->stream));
  for (int t = 0; t < nk; ++t) cur[order[t]] = qs[t].out;
  return E2ETTS_OK;
}

// HifiGan.forward in precision "bf16_act" (E2ETTS_PRECISION_BF16_ACT; the reference module after .bfloat16(), V/generator.py:37-53,
// V/layers.py:33-40 / 59-64): every activation in HBM is bf16 [B, n, C], every step rounded as include/e2etts.h lists.  On the pass's
// stream: conv_pre and the upsamplers on conv_bf16 (bf16 in / out), the ResBlocks as the fusion level asks -- 2: whole ResBlocks
// (rb_bf16, the 32-channel stage as ONE launch with its sum), 1: fused pairs (pair_bf16), 0: two conv_bf16 launches per pair; the stage sum
// in the ResBlocks' epilogues (S = bf16(S + rb_j), then bf16(S / num_kernels)) or, at small windows, in the next upsampler's staging (see
// small_window below) -- and conv_post_bf16.  Every level gives the same bits.  The
// padded batch is computed in full (no ragged row limits).  Everything the call needs is checked before the first launch.
// Precision "fp16_act" (E2ETTS_PRECISION_FP16_ACT, the module after .half()) is the same walk with element kind 2: fp16 tensors, the fp16
// images and fp16-rounded parameters of make_fp16_act_params, the fp16 MFMA; profile classes *_fp16_act*.
int vocoder_act16(e2etts_engine* e, VocPass& P, const float* mel_btc, int B, int T) {
  const auto& c = e->cfg;
  const int kind = e->voc_precision == E2ETTS_PRECISION_FP16_ACT ? 2 : 1;
  const VocWeights W{e, kind};
  const char* tag = kind == 2 ? "fp16" : "bf16";
  const char* conv_nm = kind == 2 ? "conv_fp16_act" : "conv_bf16_act";
  const int nk = c.voc_n_kernels, nd = c.voc_n_dil;
  long long len = T, ch = c.voc_init_ch, maxv = len * ch;
  for (int i = 0; i < c.voc_stages; ++i) {
    len *= c.voc_up_rate[i];
    ch /= 2;
    maxv = std::max(maxv, len * ch);
  }
  if (len != (long long)T * c.hop_length) return e->fail(E2ETTS_EINVAL, "upsample product != hop_length");
  if (len > 0x7fffffffLL / 2) return e->fail(E2ETTS_EINVAL, "utterance too long");
  // ---- parameters, and every launch's geometry, before anything is launched
  auto conv_q = [&](const ConvW& w, const void* in, int in_bf16, float in_slope, void* out, int Tn, int Cin, int Cout, int KW, int dil,
                    int pad, BConvParams& q) -> bool {
    q = BConvParams();
    int split = 0;
    q.wimg = W.image(w, &split);
    q.in = in; q.in_bf16 = in_bf16; q.in_slope = in_slope; q.tap_split = split; q.KWe = split > 0 ? 2 : KW;
    q.bias = W.param(w.b); q.out_b = out; q.act16 = kind;
    q.B = B; q.T = Tn; q.Cin = Cin; q.Cout = Cout; q.KW = KW; q.dil = dil; q.pad = pad;
    return q.wimg && q.bias && conv_bf16_supported(q);
  };
  {
    BConvParams q;
    bool ok = conv_q(e->voc_pre, mel_btc, 0, 1.0f, nullptr, T, c.n_mel, c.voc_init_ch, 7, 1, 3, q);
    long long n = T, cc = c.voc_init_ch;
    for (int i = 0; i < c.voc_stages && ok; ++i) {
      const int s = c.voc_up_rate[i], co = (int)cc / 2;
      ok = conv_q(e->voc_up[i], nullptr, 1, 0.1f, nullptr, (int)n, (int)cc, s * co, 3, 1, 1, q);
      n *= s;
      cc = co;
      for (int j = 0; j < nk && ok; ++j)
        for (int m = 0; m < nd && ok; ++m) {
          const int idx = i * nk + j, k = c.voc_rb_kernel[j], d = c.voc_rb_dil[j][m];
          ok = conv_q(e->rb_c1[idx][m], nullptr, 1, 0.1f, nullptr, (int)n, co, co, k, d, (k * d - d) / 2, q);
          if (ok && c.voc_resblock == 1) ok = conv_q(e->rb_c2[idx][m], nullptr, 1, 1.0f, nullptr, (int)n, co, co, k, 1, (k - 1) / 2, q);
        }
    }
    if (!ok || !W.param(e->voc_post.w) || !W.param(e->voc_post.b) || ch > 128 || (ch % 4))
      return e->fail(E2ETTS_EINVAL, "precision %s_act: this vocoder (weights without %s images, or a geometry conv_bf16 does not serve at T = %d) has no %s-activation route", tag, tag, T, tag);
  }
  const size_t vb = (size_t)B * maxv * 2;
  RET(ensure(e, P.v0, vb));
  RET(ensure(e, P.v1, vb));
  RET(ensure(e, P.v2, vb));
  RET(ensure(e, P.v3, vb));
  RET(ensure(e, P.wav, (size_t)B * len * 4));
  RET(ensure(e, P.pcm, (size_t)B * len * 2));
  if (P.resident) e->have_wav = false;
  auto run_conv = [&](const char* nm, const BConvParams& q, double fl) -> int {
    ProfScope ps(e, nm, fl, 2.0 * ((double)q.B * q.T * (q.Cin + q.Cout * (q.res ? 2 : 1) + (q.accumulate ? q.Cout : 0))) + 2.0 * q.KWe * q.Cin * q.Cout);
    KCHK(e, launch_conv_bf16(q, e->stream));
    return E2ETTS_OK;
  };
  // Small windows (the streaming chunks): the ResBlocks of a stage as grouped launches (launch_rb_bf16_group / launch_pair_bf16_group), each
  // into buffers of its own, their sum formed by the next upsampler while it stages its input -- the same roundings in the same order
  // as the accumulating epilogues (bf16(bf16(S_0 + S_1) + S_2), then / num_kernels), so the same bits
  const bool small_window = nk > 1 && nk <= E2ETTS_MAX_RB_KERNELS && nk <= BC_GROUP_MAX && (long long)B * T <= 2048 && e->fuse_pairs >= 1;
  if (small_window)
    for (int j = 0; j + 1 < nk; ++j)
      for (int k = 0; k < 3; ++k) RET(ensure(e, P.vside[j][k], vb));
  // (16-bit elements behind the float pointers of the parameter structs)
  float* const XU = ptr<float>(P.v1);
  const RbBufs mb = rb_bufs(P, 0);
  float *const S = mb.S, *const T1 = mb.T1, *const CUR = mb.CUR;
  const float* pend_add[3] = {nullptr, nullptr, nullptr};
  float pend_div = 1.0f;
  auto join_downstream = [&] {   // the next upsampler sums the ResBlocks' buffers while it stages its input
    for (int j = 1; j < nk; ++j) pend_add[j - 1] = rb_bufs(P, j).S;
    pend_div = (float)nk;
  };
  BConvParams q;
  conv_q(e->voc_pre, mel_btc, 0, 1.0f, S, T, c.n_mel, c.voc_init_ch, 7, 1, 3, q);   // bf16(conv_pre(bf16(mel)) + b)
  RET(run_conv(conv_nm, q, 2.0 * B * (double)T * c.voc_init_ch * 7 * c.n_mel));
  long long n = T;
  ch = c.voc_init_ch;
  for (int i = 0; i < c.voc_stages; ++i) {
    const int s = c.voc_up_rate[i], co = (int)ch / 2;
    // bf16(ConvTranspose1d(bf16(lrelu_0.1(x))) + b) as the polyphase 3-tap convolution (row q of [n, s co] = rows q s .. q s + s - 1)
    conv_q(e->voc_up[i], S, 1, 0.1f, XU, (int)n, (int)ch, s * co, 3, 1, 1, q);
    for (int k = 0; k < 3; ++k) q.in_add[k] = pend_add[k];   // the previous stage's sum, formed while staging
    q.in_div = pend_div;
    pend_add[0] = pend_add[1] = pend_add[2] = nullptr; pend_div = 1.0f;
    RET(run_conv(conv_nm, q, 2.0 * B * (double)n * s * co * 2 * ch));
    n *= s;
    ch = co;
    const RbStage g{i, B, co, n};
    const bool group_ok = small_window && i + 1 < c.voc_stages;
    bool stage_done = false;
    if (e->fuse_pairs >= 2 && nk <= BC_GROUP_MAX) {   // whole ResBlocks
      RbParams rq[E2ETTS_MAX_RB_KERNELS];
      bool all = false;
      double fl = 0;
      RET(whole_stage(e, W, g, XU, S, rq, all, fl, stage_done));
      if (!stage_done && all) {
        if (group_ok) {   // every ResBlock in one launch, largest kernel first; joined downstream
          RET(rb_group(e, W, g, P, rq, fl));
          join_downstream();
        } else {
          for (int j = 0; j < nk; ++j) RET(rb_single(e, W, g, rq[j], closing(j, true, nk, false)));
        }
        stage_done = true;
      }
    }
    if (!stage_done && group_ok && c.voc_resblock == 1) {   // pair m of every ResBlock in one launch
      bool ok = true;
      for (int j = 0; j < nk && ok; ++j)   // every member of every launch servable: decided before anything is launched
        for (int m = 0; m < nd && ok; ++m) ok = pair_bf16_supported(pair_params(W, g, j, m));
      if (ok) {
        const float* curj[E2ETTS_MAX_RB_KERNELS];
        int order[E2ETTS_MAX_RB_KERNELS];
        for (int j = 0; j < nk; ++j) curj[j] = XU;
        rb_order(c, order);
        for (int m = 0; m < nd; ++m) RET(pair_group(e, W, g, P, m, order, curj));
        join_downstream();
        stage_done = true;
      }
    }
    for (int j = 0; j < nk && !stage_done; ++j) {
      const int idx = i * nk + j, k = c.voc_rb_kernel[j];
      const float* cur = XU;
      for (int m = 0; m < nd; ++m) {
        const int d = c.voc_rb_dil[j][m];
        const bool last = m == nd - 1;
        const Closing cl = closing(j, last, nk, false);
        if (c.voc_resblock == 2) {   // x = bf16(bf16(c(bf16(lrelu(x))) + b) + x); never in place (neighbouring rows are still read)
          float* out = last ? S : (cur == CUR ? T1 : CUR);
          conv_q(e->rb_c1[idx][m], cur, 1, 0.1f, out, (int)n, co, co, k, d, (k * d - d) / 2, q);
          q.res = cur; q.accumulate = cl.accumulate; q.out_div = cl.out_div;
          RET(run_conv(conv_nm, q, 2.0 * B * (double)n * co * k * co));
          cur = out;
          continue;
        }
        PairParams pq;
        if (e->fuse_pairs >= 1) {
          pq = pair_params(W, g, j, m);
          pq.x = cur; pq.out = last ? S : (cur == CUR ? T1 : CUR);
          pq.accumulate = cl.accumulate; pq.out_div = cl.out_div;
        }
        if (e->fuse_pairs >= 1 && pair_bf16_supported(pq)) {
          char nm[48];
          snprintf(nm, sizeof nm, "pair_%s_%d", W.cls(), co);
          ProfScope ps(e, nm, resblock_pair_flops(pq), resblock_pair_bytes(pq) * W.elt());
          KCHK(e, launch_pair_bf16(pq, e->stream));
          cur = pq.out;
          continue;
        }
        // two launches: xt = bf16(lrelu(bf16(c1 + b1))) handed over in bf16, then x = bf16(bf16(c2(xt) + b2) + x) (conv2 may write over x:
        // its slab reads xt, and each output row reads only its own residual row -- but never over the stage input XU)
        float* mid = cur == T1 ? CUR : T1;
        float* out = last ? S : (cur == XU ? (mid == T1 ? CUR : T1) : const_cast<float*>(cur));
        BConvParams q2;
        handover_params(W, g, j, m, cur, mid, out, q, q2);
        q2.accumulate = cl.accumulate; q2.out_div = cl.out_div;
        RET(run_conv(conv_nm, q, 2.0 * B * (double)n * co * k * co));
        RET(run_conv(conv_nm, q2, 2.0 * B * (double)n * co * k * co));
        cur = out;
      }
    }
  }
  {
    ProfScope ps(e, kind == 2 ? "conv_post_fp16_act" : "conv_post_bf16", 2.0 * B * (double)n * 7 * ch, (double)B * n * (ch * 2.0 + 6.0));
    KCHK(e, launch_conv_post_bf16(S, W.param(e->voc_post.w), W.param(e->voc_post.b), ptr<float>(P.wav), ptr<int16_t>(P.pcm), B, n, (int)ch, 7, e->stream, kind == 2));
  }
  if (P.resident) {
    e->voc_B = B; e->voc_T = T;
    e->have_wav = true;
  }
  return E2ETTS_OK;
}

// HifiGan.forward (V/generator.py:37-53) on channels-last mel [B, T, n_mel] already in HBM, in the working set P; the engine is enqueuing
// on P.stream (e->stream == P.stream: a slot's pass runs inside an OnStream)
int vocoder_impl(e2etts_engine* e, VocPass& P, const float* mel_btc, int B, int T, const int32_t* ragged_lens = nullptr,
                 const int64_t* ragged_lens_host = nullptr) {
  const auto& c = e->cfg;
  if (!e->voc_loaded) return e->fail(E2ETTS_ESTATE, "vocoder weights not loaded");
  if (B <= 0 || T <= 0) return e->fail(E2ETTS_EINVAL, "B and T must be positive");
  if (e->voc_precision == E2ETTS_PRECISION_BF16_ACT || e->voc_precision == E2ETTS_PRECISION_FP16_ACT) return vocoder_act16(e, P, mel_btc, B, T);   // (ragged limits unused)
  // largest activation of any stage, in floats per utterance
  long long len = T, ch = c.voc_init_ch;
  long long maxv = len * ch;
  for (int i = 0; i < c.voc_stages; ++i) {
    len *= c.voc_up_rate[i];
    ch /= 2;
    maxv = std::max(maxv, len * ch);
  }
  if (ch < 4 || (ch % 4)) return e->fail(E2ETTS_EINVAL, "final vocoder width %lld must be a positive multiple of 4", ch);
  const bool istft = c.voc_istft_nfft != 0;
  const long long nsamp = istft ? len * c.voc_istft_hop : len;
  if (nsamp != (long long)T * c.hop_length) return e->fail(E2ETTS_EINVAL, "upsample product != hop_length");
  if (istft) maxv += ch;  // the reflection-padded frame (the tail itself is always computed in full: it is 18 channels wide)
  const size_t vb = (size_t)B * maxv * 4;
  RET(ensure(e, P.v0, vb));
  RET(ensure(e, P.v1, vb));
  RET(ensure(e, P.v2, vb));
  RET(ensure(e, P.v3, vb));
  RET(ensure(e, P.wav, (size_t)B * nsamp * 4));
  RET(ensure(e, P.pcm, (size_t)B * nsamp * 2));
  if (P.resident) e->have_wav = false;
  float* const XU = ptr<float>(P.v1);
  const RbBufs mb = rb_bufs(P, 0);
  float *const S = mb.S, *const T1 = mb.T1, *const CUR = mb.CUR;
  const Tuning& tune = tuning();
  const VocWeights W{e, 0};

  // weight selection: split-precision image when requested and present, else fp32
  auto setw = [&](ConvParams& q, const ConvW& w) {
    q.bias = w.b;
    if (e->voc_precision != E2ETTS_PRECISION_FP32 && w.wx3) { q.w = w.wx3; q.x3 = e->voc_precision; }
    else { q.w = w.w; q.x3 = 0; }
    // plain bf16: the same weights in conv_bf16.hip's order (the router in conv() decides)
    if (const void* im = W.image(w, &q.bimg_tap_split)) q.bimg = im;
  };
  // Ragged mode: the layers of stage i compute rows < mel_len * rate_i + halo_i only (host_logic.h: vocoder_stage_halo_rows -- the
  // reach of what is still to come, in that stage's rows: 12 frames after conv_pre, 76 / 109 / 94 / 63 rows in the four stages of
  // HiFi-GAN V1).  What lies beyond is stale but finite and out of the reach of every valid sample.
  const int32_t* act_stage[E2ETTS_MAX_STAGES + 1] = {nullptr};
  const int32_t* act_stage_h[E2ETTS_MAX_STAGES + 1] = {nullptr};  // the same limits in host memory (compact grids), when the caller has the lengths there
  double vfs[E2ETTS_MAX_STAGES + 1];  // fraction of the padded rows the limits of stage i leave (profile FLOP counts, tile choice without host lengths)
  for (int i = 0; i <= E2ETTS_MAX_STAGES; ++i) vfs[i] = ragged_lens ? e->rag_frac_voc : 1.0;
  if (ragged_lens) {
    RET(ensure(e, e->actbuf, (size_t)(5 + c.voc_stages) * B * 4));
    int32_t* ab = ptr<int32_t>(e->actbuf) + 2 * B;
    long long halo[E2ETTS_MAX_STAGES + 1];
    vocoder_stage_halo_rows(c, halo);
    if (ragged_lens_host) e->h_act.resize((size_t)(5 + c.voc_stages) * B, 0);
    long long rate = 1;
    for (int i = 0; i <= c.voc_stages; ++i) {
      KCHK(e, launch_act_rows(ragged_lens, ab + (size_t)i * B, B, 0, (int)rate, (long long)T * rate, e->stream, halo[i]));
      act_stage[i] = ab + (size_t)i * B;
      if (ragged_lens_host) {  // act_rows_kernel's arithmetic on the host copy of its input
        int32_t* h = e->h_act.data() + (size_t)(2 + i) * B;
        double sum = 0;
        for (int b = 0; b < B; ++b) {
          const long long m32 = std::min<long long>(ragged_lens_host[b], 0x7fffffffLL);
          h[b] = (int32_t)std::min<long long>(m32 * rate + halo[i], (long long)T * rate);
          sum += (double)std::max(h[b], 0);
        }
        act_stage_h[i] = h;
        vfs[i] = sum / ((double)B * T * rate);
      }
      if (i < c.voc_stages) rate *= c.voc_up_rate[i];
    }
  }
  // Small batches (the B = 1 latency path): the ResBlocks of a stage are independent until their sum (V/generator.py:44-48), and one
  // ResBlock's launches -- 384 tiles on 256 CUs at B = 1, chains of 40-70 us kernels -- leave CUs idle at every tail.  They run side by
  // side: ResBlock 0 on the pass's stream into S, ResBlock j > 0 on a side stream into a sum buffer of its own, joined by
  // S = (S + S_j) [/ num_kernels] in the accumulating epilogue's order -- same operations, same bits.  Off while the full class profile is taken
  // and above tuning().voc_conc_frames frames (default 2 048; 4 096 in exact fp32), where every launch fills the chip.
  // (measured per batch size and mode: bf16x3 gains up to B = 2 at T = 768 and loses 1-2 % from B = 4, exact fp32 still gains 2 % at
  // B = 4 and loses from B = 8; a per-stage limit on the tile count instead showed nothing beyond noise)
  const long long conc_frames = tune.voc_conc_frames >= 0 ? tune.voc_conc_frames : (e->voc_precision == E2ETTS_PRECISION_FP32 ? 4096 : 2048);
  const int nk = c.voc_n_kernels, nd = c.voc_n_dil;
  // (a profile of ALL classes wants one kernel at a time; a profile filtered to one class -- bench.py's timed region -- records its
  // events on whichever stream the launch goes to and is fine)
  const bool full_profile = e->prof_on && e->prof_filter.empty();
  // Plain bf16 at such sizes goes one step further (conv_bf16.hip: launch_*_group): pair m of ALL ResBlocks of the stage is ONE launch on
  // the pass's stream -- a third of the launches, no fork / join events, and a grid the three kernel sizes fill together (one ResBlock's
  // pair is 1.15 rounds of workgroups at a 542-frame window, the k = 11 stream the critical path of every stage, and the host needed
  // longer to enqueue three streams' launches than the GPU to run them).  Each ResBlock keeps its own buffers as on the side streams,
  // and the join below is the same: same bits.  (tuning().voc_group: off keeps the streams.)
  const bool small_window = nk > 1 && nk <= E2ETTS_MAX_RB_KERNELS && nk <= BC_GROUP_MAX && (long long)B * T <= conc_frames;
  const bool group_mode = tune.voc_group && small_window && e->voc_precision == E2ETTS_PRECISION_BF16 && !ragged_lens && c.voc_resblock == 1 && e->fuse_pairs;
  // A pass in a stream slot (e2etts_vocoder_stream_push) overlaps with the other slot's pass instead: side streams of its own would only
  // crowd the process's four hardware queues; the calibration pass has none either.
  const bool conc = (!full_profile || group_mode) && nk > 1 && nk <= E2ETTS_MAX_RB_KERNELS && (long long)B * T <= conc_frames &&
                    (P.resident || group_mode);
  if (conc)
    for (int j = 0; j + 1 < nk; ++j)
      for (int k = 0; k < 3; ++k) RET(ensure(e, P.vside[j][k], vb));
  // the pass's side streams and events, made when a stage first forks: a pass whose stages all run grouped never owns any
  auto side_streams = [&]() -> int {
    for (int j = 0; j + 1 < nk; ++j) {
      if (!P.side[j]) HIPCHK(e, hipStreamCreateWithFlags(&P.side[j], hipStreamNonBlocking));
      if (!P.ev_join[j]) HIPCHK(e, hipEventCreateWithFlags(&P.ev_join[j], hipEventDisableTiming));
    }
    if (!P.ev_fork) HIPCHK(e, hipEventCreateWithFlags(&P.ev_fork, hipEventDisableTiming));
    return E2ETTS_OK;
  };
  // A failure between a stage's fork and its join must not leave ResBlocks queued on the side streams: the next call could overwrite
  // XU or vside[*] -- or ensure() free them -- under work still in flight.  Whatever path leaves this function while
  // `armed`, the side streams are drained first.
  struct SideDrain {
    VocPass& P; int n; bool armed;
    ~SideDrain() {
      if (!armed) return;
      for (int j = 0; j < n; ++j)
        if (P.side[j]) (void)hipStreamSynchronize(P.side[j]);
    }
  } drain{P, conc ? nk - 1 : 0, false};
  ConvParams p;
  p.B = B; p.T = T; p.act_rows = act_stage[0]; p.act_rows_host = act_stage_h[0]; p.act_frac = vfs[0]; p.in = mel_btc; setw(p, e->voc_pre); p.out = S; p.Cin = c.n_mel; p.Cout = c.voc_init_ch;
  p.KW = 7; p.pad = 3;
  RET(conv(e, p));
  long long n = T;
  ch = c.voc_init_ch;
  // stage i's upsampler on n_in rows of ch_in channels (input S)
  auto make_up = [&](int i, long long n_in, long long ch_in, ConvParams& q) {
    const int s = c.voc_up_rate[i];
    const int co = (int)ch_in / 2;
    q = ConvParams();
    q.B = B; q.T = (int)n_in; q.act_rows = act_stage[i]; q.act_rows_host = act_stage_h[i]; q.act_frac = vfs[i]; q.in = S; setw(q, e->voc_up[i]); q.out = XU; q.Cin = (int)ch_in; q.Cout = s * co;
    q.KW = 3; q.pad = 1; q.in_slope = 0.1f;
    q.zero_tap_split = s * co / 2;  // phases < s/2 never use tap 2, the others never tap 0 (packer.polyphase_upsampler)
  };
  // a join that the NEXT layer performs while staging its input (grouped stages, below): S = (((S + pend_add[0]) + ...) / pend_div
  const float* pend_add[3] = {nullptr, nullptr, nullptr};
  float pend_div = 1.0f;
  for (int i = 0; i < c.voc_stages; ++i) {
    const int s = c.voc_up_rate[i];
    const int co = (int)ch / 2;
    // leaky_relu(0.1) -> ConvTranspose1d(k = 2s, stride s, pad s/2)  (V/generator.py:40-41) as a 3-tap convolution
    // with s * co output channels: row q of the [n, s*co] result IS rows q*s .. q*s+s-1 of the [n*s, co] signal.
    make_up(i, n, ch, p);
    for (int k = 0; k < 3; ++k) p.in_add[k] = pend_add[k];   // the previous stage's join, folded into this layer's input (see below)
    p.in_div = pend_div;
    pend_add[0] = pend_add[1] = pend_add[2] = nullptr; pend_div = 1.0f;
    RET(conv(e, p, 2.0 / 3.0));
    n *= s;
    ch = co;
    if (n > 0x7fffffffLL / 2) return e->fail(E2ETTS_EINVAL, "utterance too long");
    const RbStage g{i, B, co, n};
    // ---- grouped launches (see group_mode above): pair m of every ResBlock in one launch; at 256 channels, where a pair runs as two
    // convolutions with a bf16 hand-over, conv1 of every ResBlock and then conv2 of every ResBlock
    bool grouped_stage = false;
    bool joined_in_kernel = false;   // the stage's launch already wrote (S_0 + S_1 + ...) / n to S
    if (group_mode) {
      int order[E2ETTS_MAX_RB_KERNELS];
      rb_order(c, order);
      bool as_pairs = co <= 128;
      // fused pairs at 256 channels too where conv_bf16.hip has them (eight-wavefront workgroups).  Asked of pair (0, 0) as it is: should its
      // dilation be out of pair_bf16's reach, the hand-over form is probed below and fails on the same halo limit -- the stage is not grouped
      if (co == 256) as_pairs = pair_bf16_supported(pair_params(W, g, 0, 0));
      // 32 / 64 channels: the WHOLE ResBlock of every kernel size in one launch (these stages' tensors, 35 MB per 542-frame window at 48 kHz,
      // stream through the Infinity Cache: pair by pair each is read twice and written once per pair) ... and, where one workgroup can
      // hold it (32 channels), ALL the ResBlocks of the stage and their sum
      if (e->fuse_pairs >= 2) {
        RbParams rq[E2ETTS_MAX_RB_KERNELS];
        bool all = false;
        double fl = 0;
        RET(whole_stage(e, W, g, XU, S, rq, all, fl, joined_in_kernel));
        if (!joined_in_kernel && all) RET(rb_group(e, W, g, P, rq, fl));
        grouped_stage = joined_in_kernel || all;
      }
      // every member of every launch must be servable: decided before anything is launched
      bool ok = !grouped_stage;
      for (int j = 0; j < nk && ok; ++j)
        for (int m = 0; m < nd && ok; ++m) {
          if (as_pairs) {
            ok = pair_bf16_supported(pair_params(W, g, j, m));
          } else {
            const RbBufs b = rb_bufs(P, j);
            BConvParams a, z;
            handover_params(W, g, j, m, XU, b.T1, b.S, a, z);
            ok = a.wimg && z.wimg && conv_bf16_supported(a);
          }
        }
      if (ok) {
        grouped_stage = true;
        const float* curj[E2ETTS_MAX_RB_KERNELS];
        for (int j = 0; j < nk; ++j) curj[j] = XU;
        for (int m = 0; m < nd; ++m) {
          if (as_pairs) {
            RET(pair_group(e, W, g, P, m, order, curj));
            continue;
          }
          BConvParams q1[E2ETTS_MAX_RB_KERNELS], q2[E2ETTS_MAX_RB_KERNELS];
          double fl = 0, by = 0;
          for (int t = 0; t < nk; ++t) {
            const int j = order[t], k = c.voc_rb_kernel[j];
            const RbBufs b = rb_bufs(P, j);
            handover_params(W, g, j, m, curj[j], b.T1, m == nd - 1 ? b.S : b.CUR, q1[t], q2[t]);
            fl += 2.0 * B * (double)n * co * k * co; by += 4.0 * ((double)B * n * co * 2.0 + (double)co * k * co);
          }
          char nm[48];
          snprintf(nm, sizeof nm, "conv_bf16_group_%d", co);
          {
            ProfScope ps(e, nm, fl, by);
            KCHK(e, launch_conv_bf16_group(q1, nk, e->stream));
          }
          {
            ProfScope ps(e, nm, fl, by * 1.5);
            KCHK(e, launch_conv_bf16_group(q2, nk, e->stream));
          }
          for (int t = 0; t < nk; ++t) curj[order[t]] = q2[t].out;
        }
      }
    }
    if (conc && !grouped_stage) {  // fork: the side streams may start once the upsampler's output (and everything before it) is complete
      RET(side_streams());
      HIPCHK(e, hipEventRecord(P.ev_fork, P.stream));
      drain.armed = true;
      for (int j = 0; j + 1 < nk; ++j) HIPCHK(e, hipStreamWaitEvent(P.side[j], P.ev_fork, 0));
    }
    // Side by side, the ResBlocks are ENQUEUED last one first: at small windows (a 542-frame streaming window's 256-channel stage: six
    // launches of ~15 us per ResBlock) the host needs longer to enqueue a ResBlock's launches than the GPU to run them, so the stream
    // enqueued last starts late by the others' enqueue time -- and the last ResBlock has the largest kernel size, the stage's critical
    // path.  Which stream a ResBlock runs on, and every result bit, are unchanged.
    // Large grids, plain bf16, padded batch: the stage form of rb_bf16 (every ResBlock of the stage and their sum per workgroup: x read once,
    // the sum written once) where it exists (32 channels) -- there these stages run on the HBM roofline as pair launches.
    bool whole_stage_done = false;
    if (!grouped_stage && !conc && e->fuse_pairs >= 2 && !act_stage[i + 1] && nk <= BC_GROUP_MAX)
      RET(whole_stage(e, W, g, XU, S, whole_stage_done));
    for (int jj = 0; jj < nk && !grouped_stage && !whole_stage_done; ++jj) {
      const int j = conc ? nk - 1 - jj : jj;
      const int idx = i * nk + j;
      const int k = c.voc_rb_kernel[j];
      // this ResBlock's stream and buffers (shadowing the stage-wide names)
      const bool aside = conc && j > 0;
      const RbBufs rb = rb_bufs(P, aside ? j : 0);
      float *const S = rb.S, *const T1 = rb.T1, *const CUR = rb.CUR;
      OnStream on(e, aside ? P.side[j - 1] : P.stream);   // whatever path leaves this iteration, the engine is back on the pass's stream
      const float* cur = XU;
      const bool f32 = e->voc_precision == E2ETTS_PRECISION_FP32;
      bool fused = e->fuse_pairs && e->stage_fused[i] && (!f32 || !e->rb_pair_frag32[idx].empty());
      // 256 channels: the fused pair runs ONE 512-thread workgroup per CU on tiles of ~118-126 rows; with fewer tiles than CUs (small
      // batches: 52 tiles at B = 1, T = 768) the two-launch form on 64 x 64 tiles fills the chip better (B = 1: 5.99 vs 6.45 ms per
      // utterance).  Both forms give the same bits, so the choice is invisible in the output.
      if (fused && co == 256 && (long long)B * (n / 128) < 256) fused = false;
      // (no whole ResBlock per launch, rb_bf16, here: at large grids the pair / chain kernels, two or three workgroups per CU, are ahead
      // of that one-workgroup-per-CU kernel: measured 7.9 against 8.4 ms for the 60 s utterance in one call)
      // the whole ResBlock in one launch (resblock_chain.hip) where it exists: kernel size 3 at 32 / 64 channels
      const bool chained = fused && !f32 && e->fuse_pairs >= 2 && resblock_chain_supported(co, k, c.voc_rb_dil[j], nd);
      if (chained) {
        const Closing cl = closing(j, true, nk, conc);
        ChainParams q;
        q.x = XU; q.wfrag = e->rb_pair_frag[idx][0]; q.out = S;
        for (int m = 0; m < 3; ++m) { q.b1[m] = e->rb_c1[idx][m].b; q.b2[m] = e->rb_c2[idx][m].b; q.dil[m] = c.voc_rb_dil[j][m]; }
        q.act_rows = act_stage[i + 1]; q.act_rows_host = act_stage_h[i + 1]; q.act_frac = vfs[i + 1];
        q.B = B; q.T = (int)n; q.C = co; q.KW = k;
        q.x_bs = q.out_bs = (long long)n * co;
        q.slope = 0.1f; q.mode = e->voc_precision;
        q.accumulate = cl.accumulate; q.out_div = cl.out_div;
        char nm[48];
        snprintf(nm, sizeof nm, "resblock_chain_%d", co);
        ProfScope ps(e, nm, resblock_chain_flops(q), resblock_chain_bytes(q));
        KCHK(e, launch_resblock_chain(q, e->stream));
      }
      for (int m = 0; m < nd && fused && !chained; ++m) {
        // the whole pair in one launch (resblock_pair.hip); x and out must differ, so the running x ping-pongs CUR / T1
        const Closing cl = closing(j, m == nd - 1, nk, conc);
        PairParams q = pair_params(W, g, j, m);   // (plain bf16: with its conv_bf16.hip images, so that pair_bf16 may serve it -- same bits)
        q.x = cur; q.out = m == nd - 1 ? S : (cur == CUR ? T1 : CUR);
        q.act_rows = act_stage[i + 1]; q.act_rows_host = act_stage_h[i + 1]; q.act_frac = vfs[i + 1];
        q.accumulate = cl.accumulate; q.out_div = cl.out_div;
        // (at large grids the two kernel families are level pair by pair; the whole 60 s utterance in one call: 7.69 ms with pair_bf16
        // everywhere against 7.91 with resblock_pair.hip there, same box -- same bits)
        const bool bpair = pair_bf16_supported(q);
        char nm[48];
        if (profile_fine()) snprintf(nm, sizeof nm, "pair %d k%d d%d r%lld%s", co, k, q.dil, (long long)B * n, q.accumulate ? "+a" : "");
        else if (bpair) snprintf(nm, sizeof nm, "pair_bf16_%d", co);
        else snprintf(nm, sizeof nm, f32 ? "resblock_pair_f32_%d" : "resblock_pair_%d", co);
        ProfScope ps(e, nm, resblock_pair_flops(q), resblock_pair_bytes(q));
        KCHK(e, bpair ? launch_pair_bf16(q, e->stream) : launch_resblock_pair(q, e->stream));
        cur = q.out;
      }
      for (int m = 0; m < nd && c.voc_resblock == 2; ++m) {
        // ResBlock2 (V/layers.py:59-63): x = c(lrelu(x)) + x per dilation; the last one adds into the stage sum
        const bool last = m == nd - 1;
        const Closing cl = closing(j, last, nk, conc);
        p = ConvParams();
        p.B = B; p.T = (int)n; p.act_rows = act_stage[i + 1]; p.act_rows_host = act_stage_h[i + 1]; p.act_frac = vfs[i + 1]; p.in = cur; setw(p, e->rb_c1[idx][m]); p.res = cur; p.Cin = co; p.Cout = co;
        p.KW = k; p.dil = c.voc_rb_dil[j][m]; p.pad = (k * p.dil - p.dil) / 2; p.in_slope = 0.1f;
        p.out = last ? S : (cur == CUR ? T1 : CUR);  // never in place: other workgroups still read the rows around this tile
        p.accumulate = cl.accumulate; p.out_div = cl.out_div;
        RET(conv(e, p));
        cur = p.out;
      }
      for (int m = 0; m < nd && !fused && c.voc_resblock == 1; ++m) {
        const int d = c.voc_rb_dil[j][m];
        // xt = c1(lrelu(x)); the lrelu that feeds c2 is applied here, in c1's epilogue (V/layers.py:35-38)
        p = ConvParams();
        p.B = B; p.T = (int)n; p.act_rows = act_stage[i + 1]; p.act_rows_host = act_stage_h[i + 1]; p.act_frac = vfs[i + 1]; p.in = cur; setw(p, e->rb_c1[idx][m]); p.out = T1; p.Cin = co; p.Cout = co;
        p.KW = k; p.dil = d; p.pad = (k * d - d) / 2; p.in_slope = 0.1f; p.act = ACT_LRELU; p.act_slope = 0.1f;
        // plain bf16 on conv_bf16.hip: xt is only ever read as conv2's bf16 operand, so conv1 writes THAT (2 bytes per element, rounded
        // once, here) and conv2 copies it into its slab -- the values conv2's staging would have formed from an fp32 xt
        bool handover = false;
        {
          ConvParams p2 = ConvParams();
          p2.B = B; p2.T = (int)n; p2.in = T1; setw(p2, e->rb_c2[idx][m]); p2.res = cur; p2.out = CUR; p2.Cin = co; p2.Cout = co; p2.KW = k; p2.pad = (k - 1) / 2;
          p2.in_ld = p2.out_ld = p2.res_ld = co; p2.in_bs = p2.out_bs = p2.res_bs = (long long)n * co;
          ConvParams p1 = p; p1.in_ld = p1.out_ld = co; p1.in_bs = p1.out_bs = (long long)n * co;
          BConvParams q1, q2;
          handover = !p.act_rows && bconv_params(p1, q1) && bconv_params(p2, q2);
        }
        if (handover) { p.out = nullptr; p.out_b = T1; p.outb_slope = 1.0f; }
        RET(conv(e, p));
        // x = c2(xt) + x (:38-39); the last pair adds into the stage sum, and the last ResBlock divides by num_kernels
        // (V/generator.py:44-48)
        const bool last = m == nd - 1;
        const Closing cl = closing(j, last, nk, conc);
        p = ConvParams();
        p.B = B; p.T = (int)n; p.act_rows = act_stage[i + 1]; p.act_rows_host = act_stage_h[i + 1]; p.act_frac = vfs[i + 1]; p.in = T1; setw(p, e->rb_c2[idx][m]); p.res = cur; p.Cin = co; p.Cout = co;
        p.in_bf16 = handover ? 1 : 0;
        p.KW = k; p.dil = 1; p.pad = (k - 1) / 2;
        p.out = last ? S : CUR;
        p.accumulate = cl.accumulate; p.out_div = cl.out_div;
        RET(conv(e, p));
        cur = CUR;
      }
      if (aside) HIPCHK(e, hipEventRecord(P.ev_join[j - 1], e->stream));
    }
    // A grouped stage leaves its join to the layer that reads the sum -- the next upsampler (conv_bf16.hip stages (S_0 + S_1 + S_2) / 3 from
    // the three tensors) or conv_post -- where that layer can take it: accum_div's additions and division in its order (same bits), without
    // its launch and its pass over four tensors (142 MB at the 32- and 64-channel stages of a 542-frame window at 48 kHz).
    bool deferred = false;
    if (joined_in_kernel) deferred = true;   // nothing left to join
    if (conc && grouped_stage && !joined_in_kernel && tune.voc_defer_join && nk <= 4) {
      bool can = false;
      if (i + 1 < c.voc_stages) {
        ConvParams q;
        make_up(i + 1, n, ch, q);
        q.in_ld = q.Cin; q.out_ld = q.Cout; q.in_bs = (long long)q.T * q.Cin; q.out_bs = (long long)q.T * q.Cout;
        q.in_add[0] = rb_bufs(P, 1).S;
        BConvParams bq;
        can = bconv_params(q, bq);
      } else {
        can = !istft;
      }
      if (can) {
        for (int j = 1; j < nk; ++j) pend_add[j - 1] = rb_bufs(P, j).S;
        pend_div = (float)nk;
        deferred = true;
      }
    }
    if (conc && !deferred) {  // join: S = ((S_0 + S_1) + S_2 ...) / num_kernels, the accumulating epilogues' order
      for (int j = 1; j < nk && !grouped_stage; ++j) HIPCHK(e, hipStreamWaitEvent(P.stream, P.ev_join[j - 1], 0));
      for (int j = 1; j < nk; j += 2) {  // two side sums per pass: (S + S_j) + S_j+1, the same additions in the same order
        const bool two = j + 1 < nk;
        const bool closes = (two ? j + 1 : j) == nk - 1;
        KCHK(e, launch_accum_div(S, rb_bufs(P, j).S, (long long)B * n * co, closes ? (float)nk : 1.0f, P.stream, two ? rb_bufs(P, j + 1).S : nullptr));
      }
      drain.armed = false;  // every side stream's work is now ordered before the pass's next launch
    }
  }
  if (istft) {
    // x = leaky_relu(x) [slope 0.01]; ReflectionPad1d((1, 0)); conv_post; spec = exp(..), phase = sin(..) (V/generator.py:107-111);
    // wav = istft(spec * exp(j phase), n_fft, hop, window = hann) (src/tools/stft.py:138-148)
    const long long F = n + 1;
    const int pc = (c.voc_istft_nfft + 2 + 3) / 4 * 4, bins = c.voc_istft_nfft / 2 + 1;
    RET(ensure(e, P.istft_q, (size_t)B * F * pc * 4));
    RET(ensure(e, P.istft_ri, (size_t)B * F * bins * 8));
    RET(ensure(e, P.istft_sp, (size_t)B * F * bins * 2 * 4));
    {
      ProfScope ps(e, "misc", 0, 0);
      KCHK(e, launch_reflect_lrelu(S, XU, B, n, (int)ch, 0.01f, e->stream));
    }
    p = ConvParams();
    p.B = B; p.T = (int)F; p.in = XU; setw(p, e->voc_post); p.out = ptr<float>(P.istft_q); p.Cin = (int)ch; p.Cout = pc; p.KW = 7; p.pad = 3;
    RET(conv(e, p));
    {
      ProfScope ps(e, "istft", 0, (double)B * F * pc * 4.0 + (double)B * nsamp * 6.0);
      KCHK(e, launch_istft(ptr<float>(P.istft_q), pc, ptr<float>(P.istft_sp), ptr<float>(P.istft_ri), ptr<float>(P.wav),
                           ptr<int16_t>(P.pcm), B, F, c.voc_istft_nfft, c.voc_istft_hop, e->stream));
    }
    P.istft_B = B;
    P.istft_F = F;
  } else {
    ProfScope ps(e, "conv_post", 2.0 * B * (double)n * 7 * ch, (double)B * n * (ch * 4.0 + 6.0));
    KCHK(e, launch_conv_post(S, e->voc_post.w, e->voc_post.b, ptr<float>(P.wav), ptr<int16_t>(P.pcm), B, n, (int)ch, 7, e->stream,
                             act_stage[c.voc_stages], act_stage_h[c.voc_stages], pend_add[0] ? pend_add : nullptr, pend_div));
  }
  if (P.resident) {
    e->voc_B = B; e->voc_T = T;
    e->have_wav = true;
  }
  return E2ETTS_OK;
}

// ---- vocoder-bias denoiser (reference V/denoiser.py; kernels and the convolution view: denoiser.hip)

// The per-utterance table of one pass: nv[b] valid samples (checked by the caller: 0 <= nv[b] <= n, multiples of hop) -> e->dn_h / dn_lens
// [2 + n_overlap][B] = samples, frames F_b = nv / hop + 1, then for s = 0 .. n_overlap - 1 the rows F_b + n_overlap - 1 - s of the overlap-add that
// the inverse launch shifted by s rows computes; all 0 for a row too short to reflect.
// *F_max: the largest frame count; *ragged: the counts differ.  Returns a status.
int denoise_table(e2etts_engine* e, const long long* nv, int B, int* F_max, bool* ragged) {
  const auto& d = e->dn;
  const size_t nt = (size_t)(2 + d.nov) * B;
  e->dn_h.assign(nt, 0);
  int fmax = 0, fmin = 0x7fffffff;
  for (int b = 0; b < B; ++b) {
    const int F = nv[b] > d.nfft / 2 ? (int)(nv[b] / d.hop) + 1 : 0;
    e->dn_h[b] = (int32_t)nv[b];
    e->dn_h[(size_t)B + b] = F;
    for (int s = 0; s < d.nov; ++s) e->dn_h[(size_t)(2 + s) * B + b] = F ? F + d.nov - 1 - s : 0;
    fmax = std::max(fmax, F);
    fmin = std::min(fmin, F);
  }
  RET(ensure(e, e->dn_lens, nt * 4));
  HIPCHK(e, hipMemcpyAsync(e->dn_lens.p, e->dn_h.data(), nt * 4, hipMemcpyHostToDevice, e->stream));
  *F_max = fmax;
  *ragged = fmin != fmax;
  return E2ETTS_OK;
}

// The forward transform of the padded rows pad [B, R, hop] into spec [B, R, cpad].  h_tab: the table of denoise_table on the host; d_tab: the
// same on the device when the rows differ in length, else null.
int denoise_fwd_conv(e2etts_engine* e, const float* pad, float* spec, const int32_t* h_tab, const int32_t* d_tab, int B, int R) {
  const auto& d = e->dn;
  ConvParams p;
  p.B = B; p.T = R; p.in = pad; p.w = ptr<float>(e->dn_wf); p.wfrag = ptr<float>(e->dn_wf_frag); p.out = spec;
  p.Cin = d.hop; p.Cout = d.cpad; p.KW = d.nov; p.pad = 0; p.x3 = 0;
  p.in_ld = p.Cin; p.out_ld = p.Cout; p.in_bs = (long long)R * p.in_ld; p.out_bs = (long long)R * p.out_ld;
  double rows = 0;
  for (int b = 0; b < B; ++b) rows += h_tab[(size_t)B + b];
  p.act_frac = rows / ((double)B * R);   // (the rows F_max .. R - 1 of the longest utterances are computed and then zeroed)
  if (d_tab) { p.act_rows = d_tab + B; p.act_rows_host = h_tab + B; }
  char name[48];
  snprintf(name, sizeof name, "dn_fwd %s", conv_gemm_class(p));
  ProfScope ps(e, name, conv_gemm_flops(p), conv_gemm_bytes(p));
  KCHK(e, launch_conv_gemm(p, e->stream));
  return E2ETTS_OK;
}

// reflect-pad + forward transform of in [B] rows (stride in_bs) into e->dn_spec [B, R, cpad], R = F_max + n_overlap - 1; the table is in place
int denoise_forward(e2etts_engine* e, const float* in, long long in_bs, int B, int F_max, bool ragged) {
  const auto& d = e->dn;
  const int R = F_max + d.nov - 1;
  const int32_t* lens = ptr<int32_t>(e->dn_lens);
  RET(ensure(e, e->dn_pad, (size_t)B * R * d.hop * 4));
  RET(ensure(e, e->dn_spec, (size_t)B * R * d.cpad * 4));
  {
    ProfScope ps(e, "denoise_pad", 0, (double)B * R * d.hop * 8.0);
    KCHK(e, launch_stft_pad(in, in_bs, lens, ptr<float>(e->dn_pad), B, R, d.nfft, d.hop, e->stream));
  }
  return denoise_fwd_conv(e, ptr<float>(e->dn_pad), ptr<float>(e->dn_spec), e->dn_h.data(), ragged ? lens : nullptr, B, R);
}

// The transposed convolution of spec [B, R, cpad] into the overlap-add ola [B, R, hop]; h_tab / d_tab as for denoise_fwd_conv.
// ONE LAUNCH PER TAP: out[q] = sum_s spec[q - s] . W_s, s = 0 first, the others accumulated onto it through an output pointer moved down s
// rows (no row is read out of range).  As one KW = n_overlap convolution every output would be a single fp32 chain of n_overlap x 1 056 terms
// of the size of the spectrum's peaks that cancel to a sample: measured 3.6 x the reference's own fp32 error, and past the bar on audio with
// a constant offset.  Chains a quarter as long, summed in a fixed order, halve that; the price is the spectrum read once per tap instead of
// once.
int denoise_inv_convs(e2etts_engine* e, const float* spec, float* ola, const int32_t* h_tab, const int32_t* d_tab, int B, int R) {
  const auto& d = e->dn;
  const size_t wmat = (size_t)d.hop * d.cpad, wfrag = x3_frag_bytes(d.hop, 1, d.cpad) / 4;
  for (int s = 0; s < d.nov; ++s) {
    if (R - s <= 0) break;
    ConvParams p;
    p.B = B; p.T = R - s; p.in = spec; p.w = ptr<float>(e->dn_wi) + s * wmat; p.wfrag = ptr<float>(e->dn_wi_frag) + s * wfrag;
    p.out = ola + (size_t)s * d.hop;
    p.Cin = d.cpad; p.Cout = d.hop; p.KW = 1; p.pad = 0; p.x3 = 0; p.accumulate = s > 0;
    p.in_ld = p.Cin; p.out_ld = p.Cout; p.in_bs = (long long)R * p.in_ld; p.out_bs = (long long)R * p.out_ld;
    double rows = 0;
    for (int b = 0; b < B; ++b) rows += h_tab[(size_t)(2 + s) * B + b];
    p.act_frac = rows / ((double)B * p.T);
    if (d_tab) { p.act_rows = d_tab + (size_t)(2 + s) * B; p.act_rows_host = h_tab + (size_t)(2 + s) * B; }
    char name[48];
    snprintf(name, sizeof name, "dn_inv %s", conv_gemm_class(p));
    ProfScope ps(e, name, conv_gemm_flops(p), conv_gemm_bytes(p));
    KCHK(e, launch_conv_gemm(p, e->stream));
  }
  return E2ETTS_OK;
}

// in: device rows [B] of stride in_bs; wav / pcm: device [B, n] (either may be null).  Always the exact-fp32 convolution.
int denoise_impl(e2etts_engine* e, const float* in, long long in_bs, const long long* nv, int B, long long n, float strength, float* wav, int16_t* pcm) {
  const auto& d = e->dn;
  int F_max = 0;
  bool ragged = false;
  RET(denoise_table(e, nv, B, &F_max, &ragged));
  const int32_t* lens = ptr<int32_t>(e->dn_lens);
  const int R = F_max + d.nov - 1;
  RET(ensure(e, e->dn_ola, (size_t)B * R * d.hop * 4));
  if (F_max > 0) {
    RET(denoise_forward(e, in, in_bs, B, F_max, ragged));
    {
      ProfScope ps(e, "denoise_sub", 0, (double)B * R * d.cpad * 8.0);
      KCHK(e, launch_spectral_subtract(ptr<float>(e->dn_spec), ptr<float>(e->dn_bias), lens + B, B, R, d.cpad, d.nfft, d.nov, strength, e->stream));
    }
    RET(denoise_inv_convs(e, ptr<float>(e->dn_spec), ptr<float>(e->dn_ola), e->dn_h.data(), ragged ? lens : nullptr, B, R));   // (one launch per tap)
  }
  ProfScope ps(e, "denoise_ola", 0, (double)B * n * (4.0 + (wav ? 4.0 : 0.0) + (pcm ? 2.0 : 0.0)));
  KCHK(e, launch_ola_norm(ptr<float>(e->dn_ola), in, in_bs, lens, lens + B, ptr<double>(e->dn_win), wav, pcm, B, n, R, d.nfft, d.hop, e->stream));
  return E2ETTS_OK;
}

int denoise_ready(e2etts_engine* e) {
  if (!e->dn.loaded) return e->fail(E2ETTS_ESTATE, "no denoiser bases loaded (e2etts_denoiser_load)");
  if (!e->dn.have_bias) return e->fail(E2ETTS_ESTATE, "no denoiser bias spectrum (e2etts_denoiser_set_bias / e2etts_denoiser_calibrate)");
  return E2ETTS_OK;
}

// The denoiser as a function of one window of a stream, on the engine's CURRENT stream (the slot's, swapped in) and in the slot's own
// workspace.  seg: L vocoder samples per row (stride seg_bs) that start at absolute sample S0 of the stream; the window's left edge is the
// stream's start iff S0 == 0, its right edge the stream's end iff right_real.  Writes the denoised samples seg[e0 .. e0 + n_out) of every row
// to sl.dn_wav / sl.dn_pcm [B, n_out].  The caller keeps filter_length - hop samples of context between a context edge and the emitted range:
// the frames a context edge lacks (zero frames here, as past a real end) spoil only those.  Every spectrum element and every tap of the
// inverse is the same k-ordered fp32 chain as in denoise_impl on the whole signal, on the same absolute frame grid: same bits.
int denoise_stream_impl(e2etts_engine* e, e2etts_engine::StSlot& sl, const float* seg, long long seg_bs, int B, long long L, long long S0, bool right_real,
                        long long e0, long long n_out, float strength) {
  const auto& d = e->dn;
  const int half = d.nfft / 2;
  const bool left_real = S0 == 0;
  RET(ensure(e, sl.dn_wav, (size_t)B * n_out * 4));
  RET(ensure(e, sl.dn_pcm, (size_t)B * n_out * 2));
  const double* win = ptr<double>(e->dn_win);
  if (left_real && right_real && L <= half) {   // the whole stream cannot be reflected: copied through, as e2etts_denoise does with such a row
    ProfScope ps(e, "denoise_ola", 0, (double)B * n_out * 10.0);
    KCHK(e, launch_ola_norm_stream(nullptr, 0, 0, seg + e0, seg_bs, win, ptr<float>(sl.dn_wav), ptr<int16_t>(sl.dn_pcm), B, n_out, S0 + e0 + half, 1, d.nfft,
                                   d.hop, true, e->stream));
    return E2ETTS_OK;
  }
  const long long lead = left_real ? half : 0, padded = L + lead + (right_real ? half : 0);
  const int R = (int)(padded / d.hop), G = R - d.nov + 1;   // padded rows = spectrum rows = overlap-add rows; whole frames in the window
  if (G <= 0 || e0 < 0 || e0 + n_out > L) return e->fail(E2ETTS_EINVAL, "denoised stream: window of %lld samples too short", L);
  if ((long long)R > ((1LL << 31) - 1) / ((long long)d.cpad * 4))
    return e->fail(E2ETTS_EINVAL, "denoised stream: the window's spectrum (%d rows of %d floats) must stay below 2 GiB: push smaller chunks", R, d.cpad);
  RET(ensure(e, sl.dn_pad, (size_t)B * R * d.hop * 4));
  RET(ensure(e, sl.dn_spec, (size_t)B * R * d.cpad * 4));
  RET(ensure(e, sl.dn_ola, (size_t)B * R * d.hop * 4));
  RET(ensure(e, sl.dn_lens, (size_t)B * 4));
  std::vector<int32_t> tab((size_t)(2 + d.nov) * B);   // denoise_table's layout, every row alike (read by the host only)
  for (int b = 0; b < B; ++b) {
    tab[b] = (int32_t)L;
    tab[(size_t)B + b] = G;
    for (int s = 0; s < d.nov; ++s) tab[(size_t)(2 + s) * B + b] = R - s;
  }
  {
    ProfScope ps(e, "denoise_pad", 0, (double)B * R * d.hop * 8.0);
    KCHK(e, launch_fill_i32(ptr<int32_t>(sl.dn_lens), B, G, e->stream));
    KCHK(e, launch_stft_pad_stream(seg, seg_bs, ptr<float>(sl.dn_pad), B, L, R, d.nfft, d.hop, left_real, right_real, e->stream));
  }
  RET(denoise_fwd_conv(e, ptr<float>(sl.dn_pad), ptr<float>(sl.dn_spec), tab.data(), nullptr, B, R));
  {
    ProfScope ps(e, "denoise_sub", 0, (double)B * R * d.cpad * 8.0);
    KCHK(e, launch_spectral_subtract(ptr<float>(sl.dn_spec), ptr<float>(e->dn_bias), ptr<int32_t>(sl.dn_lens), B, R, d.cpad, d.nfft, d.nov, strength, e->stream));
  }
  RET(denoise_inv_convs(e, ptr<float>(sl.dn_spec), ptr<float>(sl.dn_ola), tab.data(), nullptr, B, R));
  ProfScope ps(e, "denoise_ola", 0, (double)B * n_out * 14.0);
  KCHK(e, launch_ola_norm_stream(ptr<float>(sl.dn_ola), (long long)R * d.hop, e0 + lead, seg + e0, seg_bs, win, ptr<float>(sl.dn_wav), ptr<int16_t>(sl.dn_pcm), B,
                                 n_out, S0 + e0 + half, right_real ? (S0 + L) / d.hop + 1 : LLONG_MAX, d.nfft, d.hop, false, e->stream));
  return E2ETTS_OK;
}

bool denoised_stream_busy(const e2etts_engine* e) { return e->st_open && e->st_dn && (!e->st_done || e->st_pending > 0); }

}  // namespace

extern "C" {

// E2ETTS_SRC_HASH: sha256 (first 16 hex digits) of csrc/* + include/e2etts.h, passed by __graft_entry__.build(); the marker string
// "E2ETTS_SRC_HASH=" lets build() read it from the file without loading the library, so a stale shipped .so is rebuilt, not reused.
#ifndef E2ETTS_SRC_HASH
#define E2ETTS_SRC_HASH "unknown"
#endif
const char* e2etts_version(void) { return "e2etts-hip 0.4 (gfx950; fp32 MFMA + bf16x3 split-precision MFMA) E2ETTS_SRC_HASH=" E2ETTS_SRC_HASH; }

// The struct layout is part of the ABI: a change of its size must come with a new E2ETTS_ABI_VERSION (and a new row in the sizes
// e2etts_create accepts), never silently.
static_assert(sizeof(e2etts_config) == 320, "e2etts_config changed size: bump E2ETTS_ABI_VERSION and review e2etts_create's size check");
static_assert(offsetof(e2etts_config, struct_size) == 0, "struct_size must stay the first field");
int e2etts_abi_version(void) { return E2ETTS_ABI_VERSION; }
size_t e2etts_config_size(void) { return sizeof(e2etts_config); }

const char* e2etts_last_error(const e2etts_engine* engine) { return engine ? engine->err.c_str() : g_create_error.c_str(); }

int e2etts_create(int device_id, const e2etts_config* cfg, e2etts_engine** out) {
  if (!cfg || !out) { g_create_error = "cfg / out must not be NULL"; return E2ETTS_EINVAL; }
  *out = nullptr;
  // Nothing of *cfg is read before its size is known to be this header's: a host compiled against another revision of the struct
  // would otherwise be read out of bounds (or have its fields mistaken for others).
  if (cfg->struct_size != (uint32_t)sizeof(e2etts_config)) {
    char m[192];
    snprintf(m, sizeof m, "e2etts_config.struct_size = %u is not a size this library knows (sizeof(e2etts_config) = %zu, ABI version %d): "
             "the caller was built against another revision of e2etts.h", (unsigned)cfg->struct_size, sizeof(e2etts_config), E2ETTS_ABI_VERSION);
    g_create_error = m;
    return E2ETTS_EINVAL;
  }
  const e2etts_config& c = *cfg;
  auto bad = [&](const char* m) { g_create_error = m; return E2ETTS_EINVAL; };
  if (const char* m = config_check(c)) return bad(m);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    g_create_error = "no HIP device visible: the e2etts engine has no CPU fallback";
    return E2ETTS_EHIP;
  }
  if (device_id < 0 || device_id >= ndev) return bad("device_id out of range");
  if (hipSetDevice(device_id) != hipSuccess) { g_create_error = "hipSetDevice failed"; return E2ETTS_EHIP; }
  e2etts_engine* e = new e2etts_engine();
  e->cfg = c;
  e->device = device_id;
  if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess ||
      hipHostMalloc((void**)&e->h_mel, 4096 * sizeof(int64_t)) != hipSuccess) {
    g_create_error = "stream / pinned buffer creation failed";
    delete e;
    return E2ETTS_EHIP;
  }
  e->voc.stream = e->dn_pass.stream = e->stream;
  e->voc.resident = true;
  *out = e;
  return E2ETTS_OK;
}

void e2etts_destroy(e2etts_engine* e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  (void)hipStreamSynchronize(e->stream);
  for (auto& sl : e->st_slot)
    if (sl.pass.stream) (void)hipStreamSynchronize(sl.pass.stream);
  for (DevBuf* b : e->owned)  // registered by ensure(): no hand-kept list to fall behind when a buffer is added
    if (b->p) (void)hipFree(b->p);
  for (auto& r : e->prof_recs) { (void)hipEventDestroy(r.start); (void)hipEventDestroy(r.stop); }
  for (auto ev : e->ev_pool) (void)hipEventDestroy(ev);
  free_frags(e);
  if (e->h_mel) (void)hipHostFree(e->h_mel);
  for (auto& sl : e->st_slot) {
    if (sl.pin) (void)hipHostFree(sl.pin);
    if (sl.done) (void)hipEventDestroy(sl.done);
    if (sl.win_ready) (void)hipEventDestroy(sl.win_ready);
    if (sl.pass.stream) (void)hipStreamDestroy(sl.pass.stream);
  }
  for_each_pass(e, [](VocPass& P) {   // (their buffers are in e->owned)
    for (auto& st : P.side)
      if (st) (void)hipStreamDestroy(st);
    if (P.ev_fork) (void)hipEventDestroy(P.ev_fork);
    for (auto& ev : P.ev_join)
      if (ev) (void)hipEventDestroy(ev);
  });
  if (e->stream) (void)hipStreamDestroy(e->stream);
  delete e;
}

// Binds the blob resident in e->blob (nbytes bytes, copy possibly still in flight on the engine's stream): header and directory are
// read back from HBM, validated by host_logic.h, and the tensors located.
static int bind_resident_blob(e2etts_engine* e, size_t nbytes) {
  BlobHeader h;
  HIPCHK(e, hipMemcpyAsync(&h, e->blob.p, sizeof h, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  if (const char* m = blob_check_header(h, nbytes)) return e->fail(E2ETTS_EINVAL, "%s", m);
  std::vector<BlobEntry> dir(h.n_entries);
  if (h.n_entries)
    HIPCHK(e, hipMemcpy(dir.data(), (const char*)e->blob.p + sizeof h, (size_t)h.n_entries * sizeof(BlobEntry), hipMemcpyDeviceToHost));
  std::vector<BlobTensor> ts;
  std::string bad;
  if (const char* m = blob_check_directory(h, dir.data(), nbytes, ts, bad)) return e->fail(E2ETTS_EINVAL, "tensor '%s': %s", bad.c_str(), m);
  e->tensors.clear();
  free_frags(e);
  for (const BlobTensor& t : ts) e->tensors[t.name] = {reinterpret_cast<const float*>((const char*)e->blob.p + t.offset), t.numel};
  // a blob may carry the acoustic model, the vocoder, or both (the reference loads them from two checkpoints)
  const bool has_ac = e->tensors.count("enc.emb") != 0, has_voc = e->tensors.count("voc.pre.w") != 0;
  if (!has_ac && !has_voc) return e->fail(E2ETTS_EKEY, "blob holds neither acoustic ('enc.emb') nor vocoder ('voc.pre.w') tensors");
  if (has_ac) RET(bind_acoustic(e));
  if (has_voc) RET(bind_vocoder(e));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  e->ac_loaded = has_ac;
  e->voc_loaded = has_voc;
  return E2ETTS_OK;
}

// New weights replace the tensors the stream slots' kernels read: whatever they still have in flight finishes first, and an open stream
// is closed (its chunks were computed with the old weights; the next _push says so).
static int drain_stream_slots(e2etts_engine* e) {
  for (auto& sl : e->st_slot)
    if (sl.pass.stream) HIPCHK(e, hipStreamSynchronize(sl.pass.stream));
  e->st_open = false;
  e->st_pending = 0;
  return E2ETTS_OK;
}

int e2etts_load_weights(e2etts_engine* e, const void* blob, size_t nbytes) {
  if (!e) return E2ETTS_EINVAL;
  std::lock_guard<std::mutex> lk(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  if (!blob || nbytes < sizeof(BlobHeader)) return e->fail(E2ETTS_EINVAL, "weight blob too small");
  BlobHeader h;
  HIPCHK(e, hipMemcpy(&h, blob, sizeof h, hipMemcpyDefault));
  if (const char* m = blob_check_header(h, nbytes)) return e->fail(E2ETTS_EINVAL, "%s", m);  // before anything resident is touched
  RET(drain_stream_slots(e));
  e->ac_loaded = e->voc_loaded = false;
  RET(ensure(e, e->blob, nbytes));
  HIPCHK(e, hipMemcpyAsync(e->blob.p, blob, nbytes, hipMemcpyDefault, e->stream));
  return bind_resident_blob(e, nbytes);
}

// RCCL entry points, resolved at the first call: from the process image when the host already links or has loaded RCCL (the
// communicator handed in must come from THAT copy), else from librccl.so.1 (or the file named by E2ETTS_RCCL_LIB).
extern "C++" {
namespace {
typedef int (*nccl_bcast_fn)(const void*, void*, size_t, int /*ncclDataType_t*/, int, void* /*ncclComm_t*/, hipStream_t);
typedef int (*nccl_rank_fn)(void*, int*);
typedef const char* (*nccl_errstr_fn)(int);
struct RcclApi {
  nccl_bcast_fn bcast = nullptr;
  nccl_rank_fn user_rank = nullptr;
  nccl_errstr_fn errstr = nullptr;
  std::string err;
};
RcclApi& rccl_api() {
  static RcclApi api = [] {
    RcclApi a;
    void* h = RTLD_DEFAULT;
    if (!dlsym(h, "ncclBroadcast")) {
      const char* path = getenv("E2ETTS_RCCL_LIB");
      h = dlopen(path ? path : "librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
      if (!h) {
        const char* why = dlerror();
        a.err = std::string("RCCL not loadable: ") + (why ? why : "?");
        return a;
      }
    }
    a.bcast = (nccl_bcast_fn)dlsym(h, "ncclBroadcast");
    a.user_rank = (nccl_rank_fn)dlsym(h, "ncclCommUserRank");
    a.errstr = (nccl_errstr_fn)dlsym(h, "ncclGetErrorString");
    if (!a.bcast || !a.user_rank) a.err = "RCCL library lacks ncclBroadcast / ncclCommUserRank";
    return a;
  }();
  return api;
}
}  // namespace
}  // extern "C++"

int e2etts_load_weights_bcast(e2etts_engine* e, const void* blob_or_null, size_t nbytes, void* rccl_comm, int root) {
  if (!e) return E2ETTS_EINVAL;
  std::lock_guard<std::mutex> lk(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  if (!rccl_comm) return e->fail(E2ETTS_EINVAL, "rccl_comm must not be NULL");
  if (nbytes < sizeof(BlobHeader)) return e->fail(E2ETTS_EINVAL, "weight blob too small");
  RcclApi& api = rccl_api();
  if (!api.err.empty()) return e->fail(E2ETTS_ESTATE, "%s", api.err.c_str());
  int rank = -1;
  int rc = api.user_rank(rccl_comm, &rank);
  if (rc != 0) return e->fail(E2ETTS_EHIP, "ncclCommUserRank: %s", api.errstr ? api.errstr(rc) : "error");
  if (rank == root && !blob_or_null) return e->fail(E2ETTS_EINVAL, "the root rank must supply the blob");
  RET(drain_stream_slots(e));
  e->ac_loaded = e->voc_loaded = false;
  RET(ensure(e, e->blob, nbytes));
  if (rank == root) HIPCHK(e, hipMemcpyAsync(e->blob.p, blob_or_null, nbytes, hipMemcpyDefault, e->stream));
  rc = api.bcast(e->blob.p, e->blob.p, nbytes, 1 /* ncclUint8 */, root, rccl_comm, e->stream);  // in place, on the engine's stream
  if (rc != 0) return e->fail(E2ETTS_EHIP, "ncclBroadcast: %s", api.errstr ? api.errstr(rc) : "error");
  return bind_resident_blob(e, nbytes);
}

int e2etts_order_after(e2etts_engine* e, void* caller_stream) {
  if (!e) return E2ETTS_EINVAL;
  std::lock_guard<std::mutex> lk(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  hipEvent_t ev = get_event(e);
  if (!ev) return e->fail(E2ETTS_EHIP, "hipEventCreate failed");
  HIPCHK(e, hipEventRecord(ev, (hipStream_t)caller_stream));
  HIPCHK(e, hipStreamWaitEvent(e->stream, ev, 0));  // the wait refers to the record above even if the event is re-recorded later
  e->ev_pool.push_back(ev);
  return E2ETTS_OK;
}

static int acoustic_entry(e2etts_engine* e, const int64_t* ids, const int64_t* lens, int B, int L, const int64_t* speaker,
                          int n_spk_ids, float d_control, float p_control, float e_control, const CtlArgs* ctl, float* dur_out,
                          int64_t* mel_lens_out, int* T_out, int32_t* pitch_idx_out, int32_t* energy_idx_out, float* log_dur_out,
                          float* pitch_pred_out, float* energy_pred_out, const e2etts_forced* forced = nullptr) {
  if (!e) return E2ETTS_EINVAL;
  std::lock_guard<std::mutex> lk(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  if (B > 4096) return e->fail(E2ETTS_EINVAL, "B > 4096");
  if (ctl) RET(check_controls(e, *ctl, B, L));
  ForcedPlan fp;
  if (forced) {
    // the struct is validated before anything is enqueued (host_logic.h: forced_check); its size field first, nothing else before it
    uint32_t fsize = 0;
    memcpy(&fsize, forced, sizeof fsize);
    e2etts_forced f;
    memset(&f, 0, sizeof f);
    if (fsize == sizeof f) f = *forced;
    ForcedShape sh;
    sh.B = B; sh.L = L; sh.pitch_no_uv = e->cfg.pitch_no_uv; sh.pitch_frame = e->cfg.pitch_frame; sh.energy_frame = e->cfg.energy_frame;
    sh.max_seq_len = e->cfg.max_seq_len; sh.pos_table_rows = e->cfg.pos_table_rows; sh.var_pos_rows = e->var_pos_rows;
    const float* dur_h = f.durations && !is_device_pointer(f.durations) ? f.durations : nullptr;
    const int64_t* ml_h = f.mel_lens && !is_device_pointer(f.mel_lens) ? f.mel_lens : nullptr;
    const int64_t* len_h = lens && !is_device_pointer(lens) ? lens : nullptr;
    const std::string bad = forced_check(fsize, f, sh, dur_h, ml_h, len_h);
    if (!bad.empty()) return e->fail(E2ETTS_EINVAL, "%s", bad.c_str());
    if (!forced_is_null(f)) {   // (every member NULL: the predicted pass, e2etts_acoustic_ctl bit for bit)
      fp.f = forced;
      fp.soft = f.attn_soft != nullptr;
      fp.has_p = f.f0 || f.pitch;
      fp.has_e = f.energy != nullptr;
      fp.p_avg = fp.has_p && f.pitch_frames && !e->cfg.pitch_frame;
      fp.e_avg = fp.has_e && f.energy_frames && !e->cfg.energy_frame;
      fp.T = f.T;
      fp.mel_lens_host = ml_h;
    }
  }
  // the forced pass serves generate_mel, which keeps valid frames only: it follows e2etts_set_ragged like e2etts_synthesize
  RET(acoustic_impl(e, ids, lens, B, L, speaker, n_spk_ids, d_control, p_control, e_control, fp.f ? e->ragged != 0 : false, ctl, fp.f ? &fp : nullptr));
  const size_t BL = (size_t)B * L;
  if (dur_out) RET(copy_out(e, dur_out, e->durf.p, BL * 4));
  if (mel_lens_out) RET(copy_out(e, mel_lens_out, e->mel64.p, (size_t)B * 8));
  if ((e->cfg.pitch_frame && (pitch_idx_out || pitch_pred_out)) || (e->cfg.energy_frame && (energy_idx_out || energy_pred_out)))
    return e->fail(E2ETTS_EINVAL, "a frame_level feature's index / prediction has T columns: pass NULL here and read it with e2etts_fetch_tap[_i32]");
  if (pitch_idx_out) RET(copy_out(e, pitch_idx_out, e->pidx.p, BL * 4));
  if (energy_idx_out) RET(copy_out(e, energy_idx_out, e->eidx.p, BL * 4));
  if (log_dur_out) RET(copy_out(e, log_dur_out, e->logd.p, BL * 4));
  if (pitch_pred_out) RET(copy_out(e, pitch_pred_out, e->ppred.p, BL * (e->cfg.pitch_no_uv ? 4 : 8)));
  if (energy_pred_out) RET(copy_out(e, energy_pred_out, e->epred.p, BL * 4));
  if (T_out) *T_out = e->last_T;
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return E2ETTS_OK;
}

int e2etts_acoustic(e2etts_engine* e, const int64_t* ids, const int64_t* lens, int B, int L, const int64_t* speaker,
                    int n_spk_ids, float d_control, float p_control, float e_control, float* dur_out, int64_t* mel_lens_out,
                    int* T_out, int32_t* pitch_idx_out, int32_t* energy_idx_out, float* log_dur_out, float* pitch_pred_out,
                    float* energy_pred_out) {
  return acoustic_entry(e, ids, lens, B, L, speaker, n_spk_ids, d_control, p_control, e_control, nullptr, dur_out, mel_lens_out, T_out,
                        pitch_idx_out, energy_idx_out, log_dur_out, pitch_pred_out, energy_pred_out);
}

int e2etts_acoustic_ctl(e2etts_engine* e, const int64_t* ids, const int64_t* lens, int B, int L, const int64_t* speaker,
                        int n_spk_ids, const float* d_control, int n_d, const float* p_control, int n_p, const float* e_control,
                        int n_e, float* dur_out, int64_t* mel_lens_out, int* T_out, int32_t* pitch_idx_out, int32_t* energy_idx_out,
                        float* log_dur_out, float* pitch_pred_out, float* energy_pred_out) {
  CtlArgs ctl;
  ctl.v[0] = d_control; ctl.v[1] = p_control; ctl.v[2] = e_control;
  ctl.n[0] = n_d; ctl.n[1] = n_p; ctl.n[2] = n_e;
  return acoustic_entry(e, ids, lens, B, L, speaker, n_spk_ids, 1.0f, 1.0f, 1.0f, &ctl, dur_out, mel_lens_out, T_out, pitch_idx_out,
                        energy_idx_out, log_dur_out, pitch_pred_out, energy_pred_out);
}

}  // extern "C"
// The teacher-forced pass (include/e2etts_forced.h).  NOT an entry point of this library -- its ABI is frozen --: a C++ symbol that stays
// inside whatever library the engine object is linked into; csrc/forced/forced.hip exports it from libe2etts_forced.so, which links this
// object and therefore works on the same e2etts_engine layout as the library that created the handle (forced_entry.h).
namespace e2etts {
const char* engine_version() { return e2etts_version(); }
int acoustic_forced_entry(e2etts_engine* e, const int64_t* ids, const int64_t* lens, int B, int L, const int64_t* speaker, int n_spk_ids,
                          const float* d_control, int n_d, const float* p_control, int n_p, const float* e_control, int n_e,
                          const e2etts_forced* forced, float* dur_out, int64_t* mel_lens_out, int* T_out, int32_t* pitch_idx_out,
                          int32_t* energy_idx_out, float* log_dur_out, float* pitch_pred_out, float* energy_pred_out) {
  CtlArgs ctl;
  ctl.v[0] = d_control; ctl.v[1] = p_control; ctl.v[2] = e_control;
  ctl.n[0] = n_d; ctl.n[1] = n_p; ctl.n[2] = n_e;
  return acoustic_entry(e, ids, lens, B, L, speaker, n_spk_ids, 1.0f, 1.0f, 1.0f, &ctl, dur_out, mel_lens_out, T_out, pitch_idx_out,
                        energy_idx_out, log_dur_out, pitch_pred_out, energy_pred_out, forced);
}
}  // namespace e2etts
extern "C" {

int e2etts_fetch_mel(e2etts_engine* e, float* mel, float* mel_post) {
  if (!e) return E2ETTS_EINVAL;
  std::lock_guard<std::mutex> lk(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  if (!e->have_acoustic) return e->fail(E2ETTS_ESTATE, "no acoustic result resident");
  const size_t n = (size_t)e->last_B * e->last_T * e->cfg.n_mel * 4;
  if (mel) RET(copy_out(e, mel, e->mel.p, n));
  if (mel_post) RET(copy_out(e, mel_post, e->melpost.p, n));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return E2ETTS_OK;
}

int e2etts_fetch_tap(e2etts_engine* e, const char* which, float* out, size_t n_floats) {
  if (!e || !which || !out) return E2ETTS_EINVAL;
  std::lock_guard<std::mutex> lk(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  const void* src = nullptr;
  size_t n = 0;
  if (!strcmp(which, "istft_spec_phase")) {
    if (!e->cfg.voc_istft_nfft || !e->have_wav) return e->fail(E2ETTS_ESTATE, "no iSTFT vocoder result resident");
    n = (size_t)e->voc.istft_B * e->voc.istft_F * (e->cfg.voc_istft_nfft + 2);
    if (n_floats != n) return e->fail(E2ETTS_EINVAL, "tap '%s' holds %zu floats, caller asked for %zu", which, n, n_floats);
    RET(copy_out(e, out, e->voc.istft_sp.p, n * 4));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return E2ETTS_OK;
  }
  if (!e->have_acoustic) return e->fail(E2ETTS_ESTATE, "no acoustic result resident");
  const size_t np = (size_t)e->last_B * (e->cfg.pitch_frame ? e->last_T : e->last_L), ne = (size_t)e->last_B * (e->cfg.energy_frame ? e->last_T : e->last_L);
  if (!strcmp(which, "pitch_pred")) { src = e->ppred.p; n = np * (e->cfg.pitch_no_uv ? 1 : 2); }
  else if (!strcmp(which, "energy_pred")) { src = e->epred.p; n = ne; }
  else if (!strcmp(which, "enc_out")) { src = e->xa.p;  /* the encoder's output stays in its own buffer: nothing later in the pass writes it */ n = (size_t)e->last_B * e->last_L * e->cfg.hidden; }
  else if (!strcmp(which, "dec_out")) { src = e->dx.p; n = (size_t)e->last_B * e->last_T * e->cfg.hidden; }
  else if (!strcmp(which, "dec_in") || !strcmp(which, "pitch_target") || !strcmp(which, "energy_target")) {
    // taps of e2etts_acoustic_forced: the targets at the model's level as embedded (kept as separate f0 | uv | energy planes of
    // max(B L, B T_given) floats with rows of L or T_given columns), the decoder's input
    const bool is_p = which[0] == 'p', is_e = which[0] == 'e';
    if (!e->forced_last || (is_p && !e->forced_pitch) || (is_e && !e->forced_energy))
      return e->fail(E2ETTS_ESTATE, "tap '%s': the last acoustic pass was not an e2etts_acoustic_forced call that had it", which);
    if (!is_p && !is_e) { src = e->decin.p; n = (size_t)e->last_B * e->last_T * e->cfg.hidden; }
    else {
      const bool frame = is_p ? e->cfg.pitch_frame != 0 : e->cfg.energy_frame != 0;
      const size_t N = frame ? e->last_T : e->last_L, ld = frame ? (size_t)e->forced_T : (size_t)e->last_L, rows = e->last_B;
      const int planes = is_p && !e->cfg.pitch_no_uv ? 2 : 1;
      n = rows * N * planes;
      if (n_floats != n) return e->fail(E2ETTS_EINVAL, "tap '%s' holds %zu floats, caller asked for %zu", which, n, n_floats);
      const size_t n_lvl = std::max((size_t)e->last_B * e->last_L, (size_t)e->last_B * std::max(e->forced_T, 1));
      for (int k = 0; k < planes; ++k) {   // plane k -> column k of [B, N, planes]: one strided copy per row of N values
        const float* pl = ptr<float>(e->ftg) + (is_e ? 2 : k) * n_lvl;
        for (size_t b = 0; b < rows; ++b)
          HIPCHK(e, hipMemcpy2DAsync(out + b * N * planes + k, (size_t)planes * 4, pl + b * ld, 4, 4, N, hipMemcpyDefault, e->stream));
      }
      HIPCHK(e, hipStreamSynchronize(e->stream));
      return E2ETTS_OK;
    }
  }
  else return e->fail(E2ETTS_EKEY, "unknown tap '%s'", which);
  if (n_floats != n) return e->fail(E2ETTS_EINVAL, "tap '%s' holds %zu floats, caller asked for %zu", which, n, n_floats);
  RET(copy_out(e, out, src, n * 4));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return E2ETTS_OK;
}

int e2etts_fetch_tap_i32(e2etts_engine* e, const char* which, int32_t* out, size_t n_values) {
  if (!e || !which || !out) return E2ETTS_EINVAL;
  std::lock_guard<std::mutex> lk(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  if (!e->have_acoustic) return e->fail(E2ETTS_ESTATE, "no acoustic result resident");
  const void* src = nullptr;
  size_t n = 0;
  if (!strcmp(which, "pitch_idx")) { src = e->pidx.p; n = (size_t)e->last_B * (e->cfg.pitch_frame ? e->last_T : e->last_L); }
  else if (!strcmp(which, "energy_idx")) { src = e->eidx.p; n = (size_t)e->last_B * (e->cfg.energy_frame ? e->last_T : e->last_L); }
  else return e->fail(E2ETTS_EKEY, "unknown tap '%s'", which);
  if (n_values != n) return e->fail(E2ETTS_EINVAL, "tap '%s' holds %zu values, caller asked for %zu", which, n, n_values);
  RET(copy_out(e, out, src, n * 4));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return E2ETTS_OK;
}

static int vocoder_entry(e2etts_engine* e, const float* mel, bool channels_first, int B, int T, float* wav_out, int16_t* pcm_out) {
  if (!e) return E2ETTS_EINVAL;
  std::lock_guard<std::mutex> lk(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  const float* src = nullptr;
  if (!mel) {
    if (!e->have_acoustic) return e->fail(E2ETTS_ESTATE, "mel == NULL but no acoustic result is resident");
    if (B != e->last_B || T != e->last_T) return e->fail(E2ETTS_EINVAL, "resident mel is [%d, %d, n_mel], caller said [%d, %d]", e->last_B, e->last_T, B, T);
    src = ptr<float>(e->melpost);
  } else {
    if (B <= 0 || T <= 0) return e->fail(E2ETTS_EINVAL, "B and T must be positive");
    const size_t n = (size_t)B * T * e->cfg.n_mel * 4;
    RET(ensure(e, e->melin, 2 * n));
    float* stage = ptr<float>(e->melin);
    float* btc = stage + (size_t)B * T * e->cfg.n_mel;
    if (channels_first) {
      RET(copy_in(e, stage, mel, n));
      KCHK(e, launch_transpose_bct_btc(stage, btc, B, e->cfg.n_mel, T, e->stream));
    } else {
      RET(copy_in(e, btc, mel, n));
    }
    src = btc;
  }
  RET(vocoder_impl(e, e->voc, src, B, T));
  const size_t ns = (size_t)B * T * e->cfg.hop_length;
  if (wav_out) RET(copy_out(e, wav_out, e->voc.wav.p, ns * 4));
  if (pcm_out) RET(copy_out(e, pcm_out, e->voc.pcm.p, ns * 2));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return E2ETTS_OK;
}

int e2etts_vocoder(e2etts_engine* e, const float* mel_bct, int B, int T, float* wav_out, int16_t* pcm_out) {
  return vocoder_entry(e, mel_bct, true, B, T, wav_out, pcm_out);
}

int e2etts_vocoder_btc(e2etts_engine* e, const float* mel_btc, int B, int T, float* wav_out, int16_t* pcm_out) {
  return vocoder_entry(e, mel_btc, false, B, T, wav_out, pcm_out);
}

static int synthesize_entry(e2etts_engine* e, const int64_t* ids, const int64_t* lens, int B, int L, const int64_t* speaker,
                            int n_spk_ids, float d_control, float p_control, float e_control, const CtlArgs* ctl, int16_t* pcm_out,
                            size_t pcm_capacity, int64_t* mel_lens_out, int* T_out) {
  if (!e) return E2ETTS_EINVAL;
  std::lock_guard<std::mutex> lk(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  if (B > 4096) return e->fail(E2ETTS_EINVAL, "B > 4096");
  if (ctl) RET(check_controls(e, *ctl, B, L));
  const bool denoise = e->dn.strength > 0.f;   // e2etts_set_denoise
  if (denoise) {
    RET(denoise_ready(e));
    if (e->cfg.hop_length % e->dn.hop)
      return e->fail(E2ETTS_EINVAL, "denoiser hop %d does not divide the vocoder's hop_length %d", e->dn.hop, e->cfg.hop_length);
  }
  bool ragged = e->ragged != 0;
  RET(acoustic_impl(e, ids, lens, B, L, speaker, n_spk_ids, d_control, p_control, e_control, ragged, ctl));
  ragged = ragged && e->rag_short;
  if (T_out) *T_out = e->last_T;
  RET(vocoder_impl(e, e->voc, ptr<float>(e->melpost), B, e->last_T, ragged ? ptr<int32_t>(e->mel32) : nullptr, ragged ? e->h_mel : nullptr));
  if (denoise) {  // each row's valid samples, before the int16 conversion: the resident PCM becomes the denoised one, the resident wav stays
    const long long n = (long long)e->last_T * e->cfg.hop_length;
    std::vector<long long> nv(B);
    for (int b = 0; b < B; ++b) nv[b] = std::min<long long>(std::max<long long>(e->h_mel[b], 0), e->last_T) * e->cfg.hop_length;
    RET(denoise_impl(e, ptr<float>(e->voc.wav), n, nv.data(), B, n, e->dn.strength, nullptr, ptr<int16_t>(e->voc.pcm)));
  }
  if (mel_lens_out) RET(copy_out(e, mel_lens_out, e->mel64.p, (size_t)B * 8));
  const size_t ns = (size_t)B * e->last_T * e->cfg.hop_length;
  if (pcm_out) {
    if (pcm_capacity < ns) {
      HIPCHK(e, hipStreamSynchronize(e->stream));
      return e->fail(E2ETTS_EINVAL, "pcm buffer holds %zu samples, result has %zu (fetch it with e2etts_fetch_pcm)", pcm_capacity, ns);
    }
    RET(copy_out(e, pcm_out, e->voc.pcm.p, ns * 2));
  }
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return E2ETTS_OK;
}

int e2etts_synthesize(e2etts_engine* e, const int64_t* ids, const int64_t* lens, int B, int L, const int64_t* speaker, int n_spk_ids,
                      float d_control, float p_control, float e_control, int16_t* pcm_out, size_t pcm_capacity,
                      int64_t* mel_lens_out, int* T_out) {
  return synthesize_entry(e, ids, lens, B, L, speaker, n_spk_ids, d_control, p_control, e_control, nullptr, pcm_out, pcm_capacity,
                          mel_lens_out, T_out);
}

int e2etts_synthesize_ctl(e2etts_engine* e, const int64_t* ids, const int64_t* lens, int B, int L, const int64_t* speaker,
                          int n_spk_ids, const float* d_control, int n_d, const float* p_control, int n_p, const float* e_control,
                          int n_e, int16_t* pcm_out, size_t pcm_capacity, int64_t* mel_lens_out, int* T_out) {
  CtlArgs ctl;
  ctl.v[0] = d_control; ctl.v[1] = p_control; ctl.v[2] = e_control;
  ctl.n[0] = n_d; ctl.n[1] = n_p; ctl.n[2] = n_e;
  return synthesize_entry(e, ids, lens, B, L, speaker, n_spk_ids, 1.0f, 1.0f, 1.0f, &ctl, pcm_out, pcm_capacity, mel_lens_out, T_out);
}

int e2etts_fetch_pcm(e2etts_engine* e, int16_t* pcm_out, size_t capacity) {
  if (!e || !pcm_out) return E2ETTS_EINVAL;
  std::lock_guard<std::mutex> lk(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  if (!e->have_wav) return e->fail(E2ETTS_ESTATE, "no vocoder result resident");
  const size_t ns = (size_t)e->voc_B * e->voc_T * e->cfg.hop_length;
  if (capacity < ns) return e->fail(E2ETTS_EINVAL, "buffer holds %zu samples, result has %zu", capacity, ns);
  RET(copy_out(e, pcm_out, e->voc.pcm.p, ns * 2));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return E2ETTS_OK;
}

int e2etts_fetch_wav(e2etts_engine* e, float* wav_out, size_t capacity) {
  if (!e || !wav_out) return E2ETTS_EINVAL;
  std::lock_guard<std::mutex> lk(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  if (!e->have_wav) return e->fail(E2ETTS_ESTATE, "no vocoder result resident");
  const size_t ns = (size_t)e->voc_B * e->voc_T * e->cfg.hop_length;
  if (capacity < ns) return e->fail(E2ETTS_EINVAL, "buffer holds %zu samples, result has %zu", capacity, ns);
  RET(copy_out(e, wav_out, e->voc.wav.p, ns * 4));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return E2ETTS_OK;
}

// denoise_strength < 0: a plain stream; else a denoised one, *delay_out = its extra frames of context per side
static int stream_begin(e2etts_engine* e, int B, float denoise_strength, int* delay_out) {
  if (!e) return E2ETTS_EINVAL;
  std::lock_guard<std::mutex> lk(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  if (!e->voc_loaded) return e->fail(E2ETTS_ESTATE, "vocoder weights not loaded");
  if (B <= 0 || B > 4096) return e->fail(E2ETTS_EINVAL, "B out of range");
  const bool dn = denoise_strength >= 0.f;
  int delay = 0;
  if (dn) {   // refused before anything of an open stream is touched
    RET(denoise_ready(e));
    if (e->cfg.hop_length % e->dn.hop)
      return e->fail(E2ETTS_EINVAL, "denoiser hop %d does not divide the vocoder's hop_length %d", e->dn.hop, e->cfg.hop_length);
    if (e->cfg.voc_istft_nfft != 0)
      return e->fail(E2ETTS_EINVAL, "a denoised stream does not serve the iSTFT tail (its tap buffers are engine-wide: two chunks in flight would share them)");
    delay = (e->dn.nfft - e->dn.hop + e->cfg.hop_length - 1) / e->cfg.hop_length;
  }
  for (auto& sl : e->st_slot) {
    if (!sl.done) HIPCHK(e, hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    if (!sl.win_ready) HIPCHK(e, hipEventCreateWithFlags(&sl.win_ready, hipEventDisableTiming));
    if (!sl.pass.stream) HIPCHK(e, hipStreamCreateWithFlags(&sl.pass.stream, hipStreamNonBlocking));
    // chunks of an abandoned stream may still be in flight: nothing of theirs is delivered
    HIPCHK(e, hipStreamSynchronize(sl.pass.stream));
  }
  HIPCHK(e, hipStreamSynchronize(e->stream));
  e->st_head = 0;
  e->st_pending = 0;
  e->st_B = B;
  e->st_carry_n = 0;
  e->st_emitted = 0;
  e->st_halo = vocoder_halo_frames(e->cfg);
  e->st_dn = dn;
  e->st_strength = dn ? denoise_strength : 0.f;
  e->st_delay = delay;
  e->st_abs0 = 0;
  e->st_open = true;
  e->st_done = false;
  if (delay_out) *delay_out = delay;
  return e->st_halo;
}

int e2etts_vocoder_stream_begin(e2etts_engine* e, int B) { return stream_begin(e, B, -1.f, nullptr); }

int e2etts_vocoder_stream_begin_denoised(e2etts_engine* e, int B, float strength, int* delay_frames_out) {
  if (!e) return E2ETTS_EINVAL;
  if (!(strength >= 0.f)) {
    std::lock_guard<std::mutex> lk(e->mu);
    return e->fail(E2ETTS_EINVAL, "strength must be >= 0");
  }
  return stream_begin(e, B, strength, delay_frames_out);
}

// Whether a caller's pointer is ordinary (pageable) host memory: such a chunk is copied into the slot's pinned buffer before _push
// returns, so the caller may reuse it at once; device memory and memory the caller pinned is read by the copy engine later.
static bool st_pageable_host(const void* p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return true;
  }
  return a.type == hipMemoryTypeUnregistered;
}

int e2etts_vocoder_stream_push(e2etts_engine* e, const float* mel_btc, int n, int last, int* n_frames_out) {
  if (!e) return E2ETTS_EINVAL;
  std::lock_guard<std::mutex> lk(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  if (!e->st_open || e->st_done) return e->fail(E2ETTS_ESTATE, "no open vocoder stream");
  if (n < 0 || (n > 0 && !mel_btc)) return e->fail(E2ETTS_EINVAL, "bad chunk");
  if (e->st_pending >= e2etts_engine::ST_DEPTH) return e->fail(E2ETTS_ESTATE, "%d chunks await e2etts_vocoder_stream_fetch", e2etts_engine::ST_DEPTH);
  // a denoised stream keeps st_delay frames more on each side: what the denoiser's frames reach beyond a sample (denoise_stream_impl)
  const int B = e->st_B, H = e->st_halo + e->st_delay, M = e->cfg.n_mel;
  const int total = e->st_carry_n + n;
  if (n_frames_out) *n_frames_out = 0;
  auto& sl = e->st_slot[(e->st_head + e->st_pending) % e2etts_engine::ST_DEPTH];   // free: whatever used it last has been fetched, hence has finished
  hipStream_t const cp = e->stream;   // assembly and copies: see the note at st_slot
  // window = [carry | new]; carry = up to H already-emitted frames (left context) followed by the frames not yet emitted
  const int left_ctx = (int)std::min<long long>(H, std::min<long long>(e->st_emitted, e->st_carry_n));
  const int emit_end = last ? total : total - H;   // frames before emit_end have their full right context in the window
  RET(ensure(e, sl.win, (size_t)B * std::max(total, 1) * M * 4));
  const size_t row_new = (size_t)n * M * 4, row_carry = (size_t)e->st_carry_n * M * 4, row_win = (size_t)total * M * 4;
  const void* src = mel_btc;
  if (n && st_pageable_host(mel_btc)) {   // taken now, so that the caller may reuse the chunk; sent up by the copy engine
    const size_t bytes = (size_t)B * row_new;
    if (sl.pin_cap < bytes) {
      if (sl.pin) HIPCHK(e, hipHostFree(sl.pin));
      sl.pin = nullptr;
      sl.pin_cap = 0;
      HIPCHK(e, hipHostMalloc(&sl.pin, bytes + bytes / 4, hipHostMallocDefault));
      sl.pin_cap = bytes + bytes / 4;
    }
    memcpy(sl.pin, mel_btc, bytes);
    src = sl.pin;
  }
  if (e->st_carry_n)
    HIPCHK(e, hipMemcpy2DAsync(sl.win.p, row_win, e->st_carry.p, row_carry, row_carry, B, hipMemcpyDeviceToDevice, cp));
  if (n)
    HIPCHK(e, hipMemcpy2DAsync((char*)sl.win.p + row_carry, row_win, src, row_new, row_new, B, hipMemcpyDefault, cp));
  int n_emit = emit_end - left_ctx;
  if (n_emit < 0) n_emit = 0;
  // next carry: H frames of emitted context + everything not yet emitted (it depends on the window alone, not on the pass)
  const int keep_from = std::max(0, (n_emit > 0 ? emit_end : left_ctx) - H);
  const int keep_n = last ? 0 : total - keep_from;
  if (keep_n > 0) {
    RET(ensure(e, e->st_carry, (size_t)B * keep_n * M * 4));
    HIPCHK(e, hipMemcpy2DAsync(e->st_carry.p, (size_t)keep_n * M * 4, (char*)sl.win.p + (size_t)keep_from * M * 4, row_win,
                               (size_t)keep_n * M * 4, B, hipMemcpyDeviceToDevice, cp));
  }
  e->st_carry_n = keep_n;
  const long long win_abs0 = e->st_abs0;
  e->st_abs0 += keep_from;
  if (last) e->st_done = true;
  if (n_emit > 0) {
    HIPCHK(e, hipEventRecord(sl.win_ready, cp));
    hipStream_t const cs = sl.pass.stream;
    HIPCHK(e, hipStreamWaitEvent(cs, sl.win_ready, 0));
    int rc;
    {
      OnStream in_slot(e, cs);   // the pass and the denoiser's launches behind it
      rc = vocoder_impl(e, sl.pass, ptr<float>(sl.win), B, total);
      if (rc == E2ETTS_OK && e->st_dn) {
        // the window's samples from st_delay frames before the emitted range to st_delay frames after it (or to the stream's ends): all of
        // them have the vocoder's full halo in the window, i.e. are the one-shot vocoder's samples
        const long long hl = e->cfg.hop_length;
        const int d_lo = std::max(0, left_ctx - e->st_delay), d_hi = std::min(total, emit_end + e->st_delay);
        rc = denoise_stream_impl(e, sl, ptr<float>(sl.pass.wav) + (size_t)d_lo * hl, (long long)total * hl, B, (long long)(d_hi - d_lo) * hl,
                                 (win_abs0 + d_lo) * hl, last && d_hi == total, (long long)(left_ctx - d_lo) * hl, (long long)n_emit * hl, e->st_strength);
      }
    }
    if (rc != E2ETTS_OK) {   // the carried context has moved on already: this stream cannot be continued
      e->st_open = false;
      (void)hipStreamSynchronize(cs);
      return rc;
    }
    HIPCHK(e, hipEventRecord(sl.done, cs));
    if (e->prof_on) HIPCHK(e, hipStreamSynchronize(cs));   // the profile's events are read after a wait on the engine's stream alone
    sl.win_n = total;
    sl.emit_off = left_ctx;
    sl.emit_n = n_emit;
    e->st_emitted += n_emit;
    ++e->st_pending;
  } else {
    HIPCHK(e, hipStreamSynchronize(cp));   // nothing to fetch: this call is the only place its errors can surface
  }
  if (n_frames_out) *n_frames_out = n_emit;
  return E2ETTS_OK;
}

int e2etts_vocoder_stream_fetch(e2etts_engine* e, float* wav_out, int16_t* pcm_out, size_t capacity) {
  if (!e) return E2ETTS_EINVAL;
  std::lock_guard<std::mutex> lk(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  if (!e->st_open || e->st_pending <= 0) return e->fail(E2ETTS_ESTATE, "no pushed chunk awaits a fetch (the last push emitted nothing?)");
  auto& sl = e->st_slot[e->st_head];
  const size_t hop = e->cfg.hop_length, ns = (size_t)sl.emit_n * hop;
  if (capacity < (size_t)e->st_B * ns) return e->fail(E2ETTS_EINVAL, "buffer holds %zu samples, chunk has %zu", capacity, (size_t)e->st_B * ns);
  // a denoised stream's slot holds the emitted samples alone, [B, ns] compact
  const size_t src_row = e->st_dn ? ns : (size_t)sl.win_n * hop, off = e->st_dn ? 0 : (size_t)sl.emit_off * hop;
  DevBuf &src_wav = e->st_dn ? sl.dn_wav : sl.pass.wav, &src_pcm = e->st_dn ? sl.dn_pcm : sl.pass.pcm;
  HIPCHK(e, hipStreamWaitEvent(e->stream, sl.done, 0));
  if (wav_out)
    HIPCHK(e, hipMemcpy2DAsync(wav_out, ns * 4, ptr<float>(src_wav) + off, src_row * 4, ns * 4, e->st_B, hipMemcpyDefault, e->stream));
  if (pcm_out)
    HIPCHK(e, hipMemcpy2DAsync(pcm_out, ns * 2, ptr<int16_t>(src_pcm) + off, src_row * 2, ns * 2, e->st_B, hipMemcpyDefault, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  e->st_head = (e->st_head + 1) % e2etts_engine::ST_DEPTH;
  --e->st_pending;
  return E2ETTS_OK;
}

int e2etts_tempo(e2etts_engine* e, const int16_t* pcm_in, size_t n_in, double speed, int sample_rate, int16_t* pcm_out, size_t capacity,
                 size_t* n_out) {
  if (!e) return E2ETTS_EINVAL;
  std::lock_guard<std::mutex> lk(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  if (!pcm_in || !n_out) return e->fail(E2ETTS_EINVAL, "pcm_in / n_out must not be NULL");
  if (!(speed >= 0.25 && speed <= 4.0)) return e->fail(E2ETTS_EINVAL, "speed must lie in [0.25, 4]");
  if (sample_rate < 4000 || sample_rate > 96000) return e->fail(E2ETTS_EINVAL, "sample_rate must lie in [4000, 96000]");
  if (n_in == 0 || n_in > (size_t)1 << 30) return e->fail(E2ETTS_EINVAL, "n_in out of range");
  // the geometry of e2e_tts_amd/api.py: time_stretch_wsola: 40 ms frames (even), 50 % overlap, +-10 ms search
  const int n = std::max((int)(sample_rate * 40.0 / 1000.0) / 2 * 2, 64);
  const int hop_out = n / 2, delta = std::max((int)(sample_rate * 10.0 / 1000.0), 1);
  const double sp = speed;
  const int n_frames = std::max((int)std::ceil(((double)n_in / sp) / hop_out), 1);
  const long long want = std::llrint((double)n_in / sp);   // Python round(): half to even
  const long long avail = (long long)n_frames * hop_out + hop_out;   // what the frames cover; want <= n_frames * hop_out + 1 by the choice of n_frames
  const long long nout = std::min(want, avail);
  *n_out = (size_t)nout;
  if (!pcm_out) return E2ETTS_OK;  // size query
  if (capacity < (size_t)nout) return e->fail(E2ETTS_EINVAL, "output holds %zu samples, result has %lld", capacity, nout);
  RET(ensure(e, e->tempo_in, n_in * 2));
  RET(ensure(e, e->tempo_out, (size_t)std::max<long long>(nout, 1) * 2));
  RET(copy_in(e, e->tempo_in.p, pcm_in, n_in * 2));
  if (speed == 1.0) {
    RET(copy_out(e, pcm_out, e->tempo_in.p, n_in * 2));
  } else {
    KCHK(e, launch_wsola(ptr<int16_t>(e->tempo_in), (long long)n_in, ptr<int16_t>(e->tempo_out), nout, sp, n, delta, n_frames, e->stream));
    RET(copy_out(e, pcm_out, e->tempo_out.p, (size_t)nout * 2));
  }
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return E2ETTS_OK;
}

int e2etts_denoiser_load(e2etts_engine* e, const float* fwd_basis, const float* inv_basis, const float* win_sq_or_null, int filter_length, int hop) {
  if (!e) return E2ETTS_EINVAL;
  std::lock_guard<std::mutex> lk(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  if (!fwd_basis || !inv_basis) return e->fail(E2ETTS_EINVAL, "fwd_basis / inv_basis must not be NULL");
  if (denoised_stream_busy(e)) return e->fail(E2ETTS_ESTATE, "a denoised vocoder stream is open: its chunks in flight read the bases and the bias");
  int nov = 0;
  if (const char* m = denoiser_geometry_check(filter_length, hop, &nov))
    return e->fail(E2ETTS_EINVAL, "%s (filter_length %d, hop %d)", m, filter_length, hop);
  const int N = filter_length, C2 = N + 2, cpad = (C2 + 31) / 32 * 32;
  // the reference's buffers ([filter_length + 2, filter_length], STFT.forward_basis / inverse_basis squeezed) -> conv_gemm's tap-major
  // [Cout][KW * Cin]: forward Cout = cpad (rows beyond filter_length + 2 zero), tap j = columns j * hop ..: the basis rows as they are;
  // inverse: one [hop][cpad] matrix per tap s (a plain Linear each, see denoise_impl), the basis columns s * hop ..
  std::vector<float> hb((size_t)C2 * N), wf((size_t)cpad * N, 0.f), wi((size_t)hop * nov * cpad, 0.f);
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipMemcpy(hb.data(), fwd_basis, hb.size() * 4, hipMemcpyDefault));
  std::copy(hb.begin(), hb.end(), wf.begin());
  HIPCHK(e, hipMemcpy(hb.data(), inv_basis, hb.size() * 4, hipMemcpyDefault));
  for (int r = 0; r < hop; ++r)
    for (int j = 0; j < nov; ++j)
      for (int c = 0; c < C2; ++c) wi[((size_t)j * hop + r) * cpad + c] = hb[(size_t)c * N + (size_t)j * hop + r];
  std::vector<double> win(N);
  if (win_sq_or_null) {
    std::vector<float> w32(N);
    HIPCHK(e, hipMemcpy(w32.data(), win_sq_or_null, (size_t)N * 4, hipMemcpyDefault));
    for (int k = 0; k < N; ++k) win[k] = (double)w32[k];
  } else {  // periodic Hann (scipy.signal.get_window('hann', N, fftbins=True)), squared, in float64
    for (int k = 0; k < N; ++k) {
      const double w = 0.5 - 0.5 * std::cos(2.0 * M_PI * (double)k / (double)N);
      win[k] = w * w;
    }
  }
  e->dn.loaded = false;
  e->dn.have_bias = false;   // a bias belongs to the geometry it was taken with
  RET(ensure(e, e->dn_wf, wf.size() * 4));
  RET(ensure(e, e->dn_wi, wi.size() * 4));
  RET(ensure(e, e->dn_wf_frag, x3_frag_bytes(cpad, nov, hop)));
  RET(ensure(e, e->dn_wi_frag, (size_t)nov * x3_frag_bytes(hop, 1, cpad)));
  RET(ensure(e, e->dn_win, (size_t)N * 8));
  RET(ensure(e, e->dn_bias, (size_t)(N / 2 + 1) * 4));
  HIPCHK(e, hipMemcpyAsync(e->dn_wf.p, wf.data(), wf.size() * 4, hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipMemcpyAsync(e->dn_wi.p, wi.data(), wi.size() * 4, hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipMemcpyAsync(e->dn_win.p, win.data(), (size_t)N * 8, hipMemcpyHostToDevice, e->stream));
  KCHK(e, launch_f32_to_frag(ptr<float>(e->dn_wf), ptr<float>(e->dn_wf_frag), cpad, nov, hop, e->stream));
  for (int j = 0; j < nov; ++j)
    KCHK(e, launch_f32_to_frag(ptr<float>(e->dn_wi) + (size_t)j * hop * cpad, ptr<float>(e->dn_wi_frag) + (size_t)j * (x3_frag_bytes(hop, 1, cpad) / 4), hop, 1,
                               cpad, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));   // the host images above are read until here
  e->dn.nfft = N; e->dn.hop = hop; e->dn.nov = nov; e->dn.cpad = cpad;
  e->dn.loaded = true;
  return E2ETTS_OK;
}

int e2etts_denoiser_set_bias(e2etts_engine* e, const float* bias, int n_bins) {
  if (!e) return E2ETTS_EINVAL;
  std::lock_guard<std::mutex> lk(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  if (denoised_stream_busy(e)) return e->fail(E2ETTS_ESTATE, "a denoised vocoder stream is open: its chunks in flight read the bases and the bias");
  if (!e->dn.loaded) return e->fail(E2ETTS_ESTATE, "no denoiser bases loaded (e2etts_denoiser_load)");
  if (!bias || n_bins != e->dn.nfft / 2 + 1)
    return e->fail(E2ETTS_EINVAL, "bias must hold filter_length / 2 + 1 = %d bins (caller said %d)", e->dn.nfft / 2 + 1, n_bins);
  RET(copy_in(e, e->dn_bias.p, bias, (size_t)n_bins * 4));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  e->dn.have_bias = true;
  return E2ETTS_OK;
}

int e2etts_denoiser_calibrate(e2etts_engine* e, const float* mel_btc_or_null, int T, float* bias_out_or_null) {
  if (!e) return E2ETTS_EINVAL;
  std::lock_guard<std::mutex> lk(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  if (denoised_stream_busy(e)) return e->fail(E2ETTS_ESTATE, "a denoised vocoder stream is open: its chunks in flight read the bases and the bias");
  if (!e->dn.loaded) return e->fail(E2ETTS_ESTATE, "no denoiser bases loaded (e2etts_denoiser_load)");
  if (!e->voc_loaded) return e->fail(E2ETTS_ESTATE, "vocoder weights not loaded");
  if (T <= 0) return e->fail(E2ETTS_EINVAL, "T must be positive");
  const long long ns = (long long)T * e->cfg.hop_length;
  if (ns % e->dn.hop || ns <= e->dn.nfft / 2)
    return e->fail(E2ETTS_EINVAL, "%d frames give %lld samples: need a multiple of the denoiser hop %d above filter_length / 2 = %d", T, ns, e->dn.hop,
                   e->dn.nfft / 2);
  const size_t nm = (size_t)T * e->cfg.n_mel * 4;
  RET(ensure(e, e->dn_mel, nm));
  if (mel_btc_or_null) RET(copy_in(e, e->dn_mel.p, mel_btc_or_null, nm));
  else HIPCHK(e, hipMemsetAsync(e->dn_mel.p, 0, nm, e->stream));
  // the pass works in buffers of its own, so every resident result (the wav and PCM of the last call, the "istft_spec_phase" tap) is what it was
  RET(vocoder_impl(e, e->dn_pass, ptr<float>(e->dn_mel), 1, T));
  const long long nv = ns;
  int F_max = 0;
  bool ragged = false;
  RET(denoise_table(e, &nv, 1, &F_max, &ragged));
  RET(denoise_forward(e, ptr<float>(e->dn_pass.wav), ns, 1, F_max, false));
  KCHK(e, launch_bias_frame(ptr<float>(e->dn_spec), ptr<float>(e->dn_bias), e->dn.nfft, e->stream));   // magnitudes of frame 0 (V/denoiser.py:179)
  if (bias_out_or_null) RET(copy_out(e, bias_out_or_null, e->dn_bias.p, (size_t)(e->dn.nfft / 2 + 1) * 4));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  e->dn.have_bias = true;
  return E2ETTS_OK;
}

int e2etts_denoise(e2etts_engine* e, const float* wav_in_or_null, const int64_t* n_valid_or_null, int B, int64_t n, float strength, float* wav_out,
                   int16_t* pcm_out) {
  if (!e) return E2ETTS_EINVAL;
  std::lock_guard<std::mutex> lk(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  RET(denoise_ready(e));
  if (B <= 0 || B > 65535 || n <= 0) return e->fail(E2ETTS_EINVAL, "B must lie in [1, 65535] and n be positive (B %d, n %lld)", B, (long long)n);
  {  // one utterance's spectrum, [n / hop + n_overlap rows][cpad] fp32, is addressed with 32-bit byte offsets by the convolutions
    const long long rows = (long long)(n / e->dn.hop) + e->dn.nov, limit = ((1LL << 31) - 1) / ((long long)e->dn.cpad * 4);
    if (rows > limit)
      return e->fail(E2ETTS_EINVAL, "n = %lld samples per row is too long: its spectrum (%lld rows of %d floats) must stay below 2 GiB, i.e. n <= %lld",
                     (long long)n, rows, e->dn.cpad, (limit - e->dn.nov) * e->dn.hop);
  }
  if (!wav_out && !pcm_out) return e->fail(E2ETTS_EINVAL, "wav_out and pcm_out are both NULL");
  if (!(strength >= 0.f)) return e->fail(E2ETTS_EINVAL, "strength must be >= 0");
  if (!wav_in_or_null) {
    if (!e->have_wav) return e->fail(E2ETTS_ESTATE, "wav_in == NULL but no vocoder result is resident");
    if (B != e->voc_B || n != (long long)e->voc_T * e->cfg.hop_length)
      return e->fail(E2ETTS_EINVAL, "resident wav is [%d, %lld], caller said [%d, %lld]", e->voc_B, (long long)e->voc_T * e->cfg.hop_length, B, (long long)n);
  }
  std::vector<long long> nv((size_t)B, n);
  if (n_valid_or_null) {
    std::vector<int64_t> h(B);
    HIPCHK(e, hipMemcpyAsync(h.data(), n_valid_or_null, (size_t)B * 8, hipMemcpyDefault, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    for (int b = 0; b < B; ++b) nv[b] = h[b];
  }
  for (int b = 0; b < B; ++b)
    if (nv[b] < 0 || nv[b] > n || nv[b] % e->dn.hop)
      return e->fail(E2ETTS_EINVAL, "row %d: %lld valid samples must lie in [0, %lld] and be a multiple of the denoiser hop %d", b, nv[b], (long long)n, e->dn.hop);
  const size_t ns = (size_t)B * (size_t)n;
  const float* in = ptr<float>(e->voc.wav);
  if (wav_in_or_null) {
    RET(ensure(e, e->dn_in, ns * 4));
    RET(copy_in(e, e->dn_in.p, wav_in_or_null, ns * 4));
    in = ptr<float>(e->dn_in);
  }
  if (wav_out) RET(ensure(e, e->dn_out, ns * 4));
  if (pcm_out) RET(ensure(e, e->dn_pcm, ns * 2));
  RET(denoise_impl(e, in, n, nv.data(), B, n, strength, wav_out ? ptr<float>(e->dn_out) : nullptr, pcm_out ? ptr<int16_t>(e->dn_pcm) : nullptr));
  if (wav_out) RET(copy_out(e, wav_out, e->dn_out.p, ns * 4));
  if (pcm_out) RET(copy_out(e, pcm_out, e->dn_pcm.p, ns * 2));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return E2ETTS_OK;
}

int e2etts_set_denoise(e2etts_engine* e, float strength) {
  if (!e) return E2ETTS_EINVAL;
  std::lock_guard<std::mutex> lk(e->mu);
  if (!(strength >= 0.f)) return e->fail(E2ETTS_EINVAL, "strength must be >= 0");
  if (strength > 0.f) RET(denoise_ready(e));
  e->dn.strength = strength;
  return E2ETTS_OK;
}

int e2etts_set_precision(e2etts_engine* e, int vocoder_precision, int decoder_precision) {
  if (!e) return E2ETTS_EINVAL;
  std::lock_guard<std::mutex> lk(e->mu);
  if (vocoder_precision != E2ETTS_PRECISION_FP32 && vocoder_precision != E2ETTS_PRECISION_BF16X3 &&
      vocoder_precision != E2ETTS_PRECISION_BF16 && vocoder_precision != E2ETTS_PRECISION_BF16_ACT && vocoder_precision != E2ETTS_PRECISION_FP16_ACT)
    return e->fail(E2ETTS_EINVAL, "unknown vocoder precision %d", vocoder_precision);
  if (decoder_precision != E2ETTS_PRECISION_FP32 && decoder_precision != E2ETTS_PRECISION_BF16X3)
    return e->fail(E2ETTS_EINVAL, "decoder precision must be fp32 or bf16x3 (got %d; bf16, bf16_act and fp16_act are vocoder-only)", decoder_precision);
  if (vocoder_precision == E2ETTS_PRECISION_BF16_ACT || vocoder_precision == E2ETTS_PRECISION_FP16_ACT) {   // the geometries they serve, decided here rather than in the middle of a call
    const auto& c = e->cfg;
    const char* mode = vocoder_precision == E2ETTS_PRECISION_FP16_ACT ? "fp16_act" : "bf16_act";
    const char* el = vocoder_precision == E2ETTS_PRECISION_FP16_ACT ? "fp16" : "bf16";
    if (c.voc_istft_nfft) return e->fail(E2ETTS_EINVAL, "precision %s serves the HiFi-GAN tail only, not the iSTFT tail", mode);
    long long ch = c.voc_init_ch;
    bool ok = ch >= 32 && ch % 32 == 0 && c.n_mel >= 8 && c.n_mel % 8 == 0 && (c.voc_resblock == 1 || c.voc_resblock == 2);
    for (int i = 0; i < c.voc_stages && ok; ++i) {
      ch /= 2;
      ok = ch >= 32 && ch % 32 == 0;
    }
    for (int j = 0; j < c.voc_n_kernels && ok; ++j)
      for (int m = 0; m < c.voc_n_dil && ok; ++m) ok = c.voc_rb_dil[j][m] * (c.voc_rb_kernel[j] - 1) <= 64;
    if (!ok || ch > 128)
      return e->fail(E2ETTS_EINVAL, "precision %s needs every vocoder width a multiple of 32 (>= 32; final <= 128) and ResBlock reaches <= 64 rows: "
                                    "init width %d over %d stages has no %s-I/O route", mode, c.voc_init_ch, c.voc_stages, el);
    // the fp16 images and parameters, at the first selection (the previous mode stays selected if this fails)
    if (vocoder_precision == E2ETTS_PRECISION_FP16_ACT && e->voc_loaded) {
      HIPCHK(e, hipSetDevice(e->device));
      RET(make_fp16_act_params(e));
    }
  }
  e->voc_precision = vocoder_precision;
  e->dec_precision = decoder_precision;
  return E2ETTS_OK;
}

int e2etts_set_ragged(e2etts_engine* e, int enable) {
  if (!e) return E2ETTS_EINVAL;
  std::lock_guard<std::mutex> lk(e->mu);
  e->ragged = enable != 0;
  return E2ETTS_OK;
}

#ifdef E2ETTS_TEST_HOOKS
int e2etts_debug_poison_workspace(e2etts_engine* e) {
  if (!e) return E2ETTS_EINVAL;
  std::lock_guard<std::mutex> lk(e->mu);
  // what the workspaces held is gone: taps, fetches and vocoder(NULL) must say so instead of handing out the pattern
  e->have_acoustic = false;
  e->have_wav = false;
  auto poison = [&](DevBuf& b) -> int {
    if (b.p) HIPCHK(e, hipMemsetAsync(b.p, 0x4B, b.cap, e->stream));
    return E2ETTS_OK;
  };
  auto poison_work = [&](VocPass& P) -> int {   // a pass's activations
    for (DevBuf* b : {&P.v0, &P.v1, &P.v2, &P.v3}) RET(poison(*b));
    for (auto& row : P.vside)
      for (DevBuf& b : row) RET(poison(b));
    return E2ETTS_OK;
  };
  auto poison_out = [&](VocPass& P) -> int {   // its outputs and the iSTFT tail's taps
    for (DevBuf* b : {&P.wav, &P.pcm, &P.istft_q, &P.istft_ri, &P.istft_sp}) RET(poison(*b));
    return E2ETTS_OK;
  };
  for (DevBuf* b : {&e->xa, &e->xb, &e->xs, &e->xp, &e->tmp, &e->qkv, &e->att, &e->hid, &e->p1, &e->p2, &e->attws, &e->ffpool, &e->dx, &e->dxb, &e->mel,
                    &e->melpost, &e->pn1, &e->pn2, &e->melin, &e->fattn, &e->ftgf, &e->ftg, &e->decin})
    RET(poison(*b));
  RET(poison_work(e->voc));
  RET(poison_out(e->voc));
  // the stream slots' workspaces too (their outputs and windows only when nothing awaits a fetch)
  for (auto& sl : e->st_slot) {
    if (sl.pass.stream) HIPCHK(e, hipStreamSynchronize(sl.pass.stream));
    RET(poison_work(sl.pass));
    if (e->st_pending == 0) {
      RET(poison_out(sl.pass));
      RET(poison(sl.win));
    }
  }
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return E2ETTS_OK;
}
#endif  // E2ETTS_TEST_HOOKS

int e2etts_set_fused_resblocks(e2etts_engine* e, int level) {
  if (!e) return E2ETTS_EINVAL;
  std::lock_guard<std::mutex> lk(e->mu);
  if (level < 0 || level > 2) return e->fail(E2ETTS_EINVAL, "fusion level must be 0 (off), 1 (pairs) or 2 (pairs + whole k = 3 ResBlocks)");
  e->fuse_pairs = level;
  return E2ETTS_OK;
}

int e2etts_profile_filter(e2etts_engine* e, const char* kernel_class) {
  if (!e) return E2ETTS_EINVAL;
  std::lock_guard<std::mutex> lk(e->mu);
  e->prof_filter = kernel_class ? kernel_class : "";
  return E2ETTS_OK;
}

int e2etts_profile_enable(e2etts_engine* e, int enable) {
  if (!e) return E2ETTS_EINVAL;
  std::lock_guard<std::mutex> lk(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  RET(prof_collect(e));
  e->prof_stats.clear();
  e->prof_on = enable != 0;
  return E2ETTS_OK;
}

int e2etts_profile_read(e2etts_engine* e, e2etts_kernel_stat* out, int cap) {
  if (!e) return E2ETTS_EINVAL;
  std::lock_guard<std::mutex> lk(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  RET(prof_collect(e));
  const int n = (int)e->prof_stats.size();
  for (int i = 0; i < n && i < cap && out; ++i) out[i] = e->prof_stats[i];
  return n;
}

size_t e2etts_device_bytes(const e2etts_engine* e) { return e ? e->dev_bytes : 0; }

void* e2etts_stream(e2etts_engine* e) { return e ? (void*)e->stream : nullptr; }

int e2etts_sync(e2etts_engine* e) {
  if (!e) return E2ETTS_EINVAL;
  std::lock_guard<std::mutex> lk(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  for (auto& sl : e->st_slot)
    if (sl.pass.stream) HIPCHK(e, hipStreamSynchronize(sl.pass.stream));
  return E2ETTS_OK;
}

}  // extern "C"
