// The engine's internal header: struct e2etts_engine, the weight and workspace structs that type its members, and what the engine's sources
// (engine*.hip) need of each other.  Seen by those sources only: never by a kernel source, a companion or a test harness.
//
// The once-compiled engine_*.hip objects are linked into the product and the test-hooks libraries alike.  That rests on one rule:
// E2ETTS_TEST_HOOKS adds functions and never a member of e2etts_engine.  engine.hip alone sees E2ETTS_TEST_HOOKS and E2ETTS_SRC_HASH.
#pragma once
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

#include "../../include/e2etts.h"
#include "host_logic.h"
// (a build that overrides this must pass the flag to EVERY engine source: it sizes a member array of e2etts_engine)
#ifndef E2ETTS_ST_DEPTH
#define E2ETTS_ST_DEPTH 2   // chunks the streaming vocoder keeps in flight (tuning builds: 3)
#endif
#include "kernels.h"
#include "tuning.h"

namespace e2etts {
namespace eng {

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

}  // namespace eng
}  // namespace e2etts

using namespace e2etts;
using namespace e2etts::eng;

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

#define KCHK(e, expr)                                              \
  do {                                                             \
    const char* _m = (expr);                                       \
    if (_m) return (e)->fail(E2ETTS_EINVAL, "%s", _m);             \
  } while (0)

namespace e2etts {
namespace eng {

template <typename T>
T* ptr(DevBuf& b) { return reinterpret_cast<T*>(b.p); }

using VocPass = e2etts_engine::VocPass;

// ---- what crosses a file boundary (everything else is file-local in the source that uses it)
// engine_core.hip
int ensure(e2etts_engine* e, DevBuf& b, size_t bytes);
int prof_class(e2etts_engine* e, const char* name);
hipEvent_t get_event(e2etts_engine* e);
bool bconv_params(const ConvParams& p, BConvParams& q);
bool profile_fine();
int conv(e2etts_engine* e, ConvParams p, double alg_scale = 1.0, bool ksplit = false);
bool is_device_pointer(const void* p);
int copy_in(e2etts_engine* e, void* dst, const void* src, size_t bytes);

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

// ---- the ragged row-limit table: e->actbuf on the device, e->h_act on the host, one row of B int32 limits per slot
struct ActSlots {
  int stages;   // cfg.voc_stages
  int dec() const { return 0; }
  int post() const { return 1; }            // mel_linear / postnet
  int voc(int i) const { return 2 + i; }    // vocoder stage i = 0 .. stages (0: conv_pre's output)
  int enc() const { return 3 + stages; }    // (the host copy only: lens32 serves on the device)
  int var() const { return 4 + stages; }    // variance predictors
  int count() const { return 5 + stages; }
};
inline int32_t* act_dev(e2etts_engine* e, int slot, int B) { return ptr<int32_t>(e->actbuf) + (size_t)slot * B; }
inline int32_t* act_host(e2etts_engine* e, int slot, int B) { return e->h_act.data() + (size_t)slot * B; }
// sizes the table for a batch of B: the device copy, the host copy or both (engine_core.hip)
int size_act(e2etts_engine* e, int B, bool dev, bool host);
// the limits of one slot as a launch helper takes them
struct RowLimits {
  const int32_t* dev = nullptr;
  const int32_t* host = nullptr;   // (null: the lengths are not in host memory; the grids stay padded)
  double frac = 1.0;               // fraction of the padded rows the limits leave (profile FLOP counts)
};

// engine_weights.hip
void free_frags(e2etts_engine* e);
int bind_acoustic(e2etts_engine* e);
int bind_vocoder(e2etts_engine* e);
int make_fp16_act_params(e2etts_engine* e);

// engine_acoustic.hip
// The array controls of e2etts_acoustic_ctl / e2etts_synthesize_ctl: d, p, e (host or device memory; nullptr = the scalar) and their
// counts, already checked by check_controls.
struct CtlArgs {
  const float* v[3] = {nullptr, nullptr, nullptr};
  int n[3] = {0, 0, 0};
};
int check_controls(e2etts_engine* e, const CtlArgs& ctl, int B, int L);
// What e2etts_acoustic_forced asked for, resolved against the model (forced_plan; the struct itself passed host_logic.h: forced_check).
struct ForcedPlan {
  const e2etts_forced* f = nullptr;
  bool soft = false;                 // attn_soft: the soft expansion, T and mel_lens as given
  bool has_p = false, has_e = false; // a pitch / an energy target
  bool p_avg = false, e_avg = false; // ... frame-resolved, for a phoneme_level feature: averaged over the durations
  int T = 0;
  const int64_t* mel_lens_host = nullptr;
};
int acoustic_impl(e2etts_engine* e, const int64_t* ids, const int64_t* lens, int B, int L, const int64_t* speaker,
                  int n_spk_ids, float d_control, float p_control, float e_control, bool ragged = false, const CtlArgs* ctl = nullptr,
                  const ForcedPlan* fp = nullptr);

// engine_vocoder.hip
int vocoder_impl(e2etts_engine* e, VocPass& P, const float* mel_btc, int B, int T, const int32_t* ragged_lens = nullptr,
                 const int64_t* ragged_lens_host = nullptr);

// engine_denoise.hip
int denoise_table(e2etts_engine* e, const long long* nv, int B, int* F_max, bool* ragged);
int denoise_forward(e2etts_engine* e, const float* in, long long in_bs, int B, int F_max, bool ragged);
int denoise_impl(e2etts_engine* e, const float* in, long long in_bs, const long long* nv, int B, long long n, float strength, float* wav, int16_t* pcm);
int denoise_stream_impl(e2etts_engine* e, e2etts_engine::StSlot& sl, const float* seg, long long seg_bs, int B, long long L, long long S0, bool right_real,
                        long long e0, long long n_out, float strength);

}  // namespace eng
}  // namespace e2etts

