// The vocoder passes: HifiGan.forward (reference V/generator.py:37-53) in fp32 / split precision / plain bf16 (vocoder_impl) and with 16-bit
// activations (vocoder_act16), on one set of ResBlock builders.
#include "engine.h"

namespace e2etts {
namespace eng {
namespace {

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

}  // namespace

// HifiGan.forward (V/generator.py:37-53) on channels-last mel [B, T, n_mel] already in HBM, in the working set P; the engine is enqueuing
// on P.stream (e->stream == P.stream: a slot's pass runs inside an OnStream)
int vocoder_impl(e2etts_engine* e, VocPass& P, const float* mel_btc, int B, int T, const int32_t* ragged_lens,
                 const int64_t* ragged_lens_host) {
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
    RET(size_act(e, B, true, ragged_lens_host != nullptr));
    const ActSlots slot{c.voc_stages};
    long long halo[E2ETTS_MAX_STAGES + 1];
    vocoder_stage_halo_rows(c, halo);
    long long rate = 1;
    for (int i = 0; i <= c.voc_stages; ++i) {
      int32_t* ab = act_dev(e, slot.voc(i), B);
      KCHK(e, launch_act_rows(ragged_lens, ab, B, 0, (int)rate, (long long)T * rate, e->stream, halo[i]));
      act_stage[i] = ab;
      if (ragged_lens_host) {  // the same limits from the host copy of the kernel's input
        int32_t* h = act_host(e, slot.voc(i), B);
        vfs[i] = host_row_limits(h, ragged_lens_host, B, 0, (int)rate, (long long)T * rate, halo[i]) / ((double)B * T * rate);
        act_stage_h[i] = h;
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

}  // namespace eng
}  // namespace e2etts
