// The acoustic pass: UnsupervisedFastSpeech2.inference (reference U/model.py:155-194) from phoneme ids to the post-net mel, predicted or
// teacher-forced.
#include "engine.h"

namespace e2etts {
namespace eng {

// 6 x FFTBlock (reference U/blocks/transformer.py:178-189), in place on x ([B, N, H]); lens32: device [B]
static int fft_stack(e2etts_engine* e, const std::vector<FFTLayer>& layers, int n_head, float* x, float* xalt, const int32_t* lens, int B, int N, bool x3,
                     const RowLimits& act = RowLimits(), bool ksplit = false) {
  const auto& c = e->cfg;
  const int H = c.hidden, F = c.ffn_dim;
  float* qkv = ptr<float>(e->qkv);
  float* att = ptr<float>(e->att);
  float* tmp = ptr<float>(e->tmp);
  float* hid = ptr<float>(e->hid);
  for (const FFTLayer& f : layers) {
    ConvParams p;
    p.B = B; p.T = N; p.act_rows = act.dev; p.act_rows_host = act.host; p.act_frac = act.frac;
    // q | k | v projections as one GEMM (U/blocks/transformer.py:220-222)
    const bool sx = x3 && f.wqkv_x3;
    p.in = x; p.w = sx ? f.wqkv_x3 : f.wqkv; p.x3 = sx; p.bias = f.bqkv; p.out = qkv; p.Cin = H; p.Cout = 3 * H;
    RET(conv(e, p, 1.0, ksplit));
    {
      const double fl = 4.0 * B * n_head * (double)N * N * (H / n_head);
      ProfScope ps(e, sx ? "attention_x3" : "attention", fl, 4.0 * 4.0 * B * N * H);
      float* aws = nullptr;   // workspace for the parallel key segments of small fp32 grids (attention.hip); 3.6 MB at B = 1, T = 768
      size_t aws_bytes = 0;
      if (!sx && !act.host && (long long)B * ((N + 63) / 64) * n_head <= attention_par_max_grid() && N > 32 * 8) {
        aws_bytes = attention_workspace_bytes(B, N, H, n_head);
        RET(ensure(e, e->attws, aws_bytes));
        aws = ptr<float>(e->attws);
      }
      KCHK(e, launch_attention(qkv, att, lens, B, N, H, n_head, sx ? 1 : 0, e->stream, act.host, aws, aws_bytes));
    }
    // fc + residual (:238-239), LayerNorm eps 1e-5, masked_fill (:182-183)
    p = ConvParams(); p.B = B; p.T = N; p.act_rows = act.dev; p.act_rows_host = act.host; p.act_frac = act.frac;
    p.in = att; p.w = sx ? f.wo_x3 : f.wo; p.x3 = sx; p.bias = f.bo; p.res = x; p.out = tmp; p.Cin = H; p.Cout = H;
    RET(conv(e, p, 1.0, ksplit));
    {
      ProfScope ps(e, "layernorm", 0, 8.0 * B * N * H);
      KCHK(e, launch_layernorm(tmp, xalt, f.ln1g, f.ln1b, lens, B, N, H, 1e-5f, e->stream));
    }
    // conv k9 + ReLU, conv k1 + residual, LayerNorm, masked_fill (:289-297, :185-187)
    p = ConvParams(); p.B = B; p.T = N; p.act_rows = act.dev; p.act_rows_host = act.host; p.act_frac = act.frac;
    p.in = xalt; p.w = sx ? f.w1_x3 : f.w1; p.x3 = sx; p.bias = f.b1; p.out = hid; p.Cin = H; p.Cout = F; p.KW = c.ffn_k1; p.pad = (c.ffn_k1 - 1) / 2;
    p.act = ACT_RELU;
    RET(conv(e, p, 1.0, ksplit));
    p = ConvParams(); p.B = B; p.T = N; p.act_rows = act.dev; p.act_rows_host = act.host; p.act_frac = act.frac;
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
static int conformer_stack(e2etts_engine* e, const std::vector<CfLayer>& layers, int n_head, float* x, float* xalt, const int32_t* lens, int B, int N, bool x3) {
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
static int fastformer_stack(e2etts_engine* e, const FfSide& side, float* x, float* xalt, const int32_t* lens, int B, int N, bool x3) {
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
static int predictor(e2etts_engine* e, const Predictor& pr, const float* x, float* out, const int32_t* mask_lens, int B, int L,
                     const RowLimits& act = RowLimits(), bool frame_level = false) {
  const int H = e->cfg.hidden;
  float* a = ptr<float>(e->p1);  // conv output
  float* b = ptr<float>(e->p2);  // LayerNorm output = next layer's input
  const float* in = x;
  int cin = H;
  for (const PredLayer& l : pr.layers) {
    ConvParams p;
    p.B = B; p.T = L; p.in = in; p.w = l.w; p.bias = l.b; p.out = a; p.Cin = cin; p.Cout = pr.chans;
    p.act_rows = act.dev; p.act_rows_host = act.host; p.act_frac = act.frac;
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

namespace {
__global__ void lens_to_i32_kernel(const int64_t* in, int32_t* out, int B, int L) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B) {
    long long v = in[i];
    out[i] = (int32_t)(v < 0 ? 0 : (v > L ? L : v));
  }
}
}  // namespace

int check_controls(e2etts_engine* e, const CtlArgs& ctl, int B, int L) {
  static const char* names[3] = {"d_control", "p_control", "e_control"};
  for (int k = 0; k < 3; ++k)
    if (ctl.v[k] && ctl.n[k] != 1 && ctl.n[k] != B && (long long)ctl.n[k] != (long long)B * L)
      return e->fail(E2ETTS_EINVAL, "%s holds %d values: expected 1, B = %d or B * L = %lld", names[k], ctl.n[k], B, (long long)B * L);
  return E2ETTS_OK;
}

// The variance adaptor's teacher-forced steps (U/layers.py:202-241 with attn_prior): the durations as given, their scan in
// launch_duration's output format, the targets brought to the model's level.  Called where the predicted pass calls launch_duration.
static int forced_durations_and_targets(e2etts_engine* e, const ForcedPlan& fp, int B, int L, float d_control, const CtlRef& d_ctl) {
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
static int forced_embed(e2etts_engine* e, const ForcedPlan& fp, float* x, int B, int L, int N, int tld, int feat, float p_control, float e_control,
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
                  int n_spk_ids, float d_control, float p_control, float e_control, bool ragged, const CtlArgs* ctl,
                  const ForcedPlan* fp) {
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
  const ActSlots slot{c.voc_stages};
  RowLimits act_enc, act_var;
  bool enc_short = false;  // some utterance is shorter than the padded length (else every limit equals L: nothing to skip, and the
                           // launches keep their plain grids -- the B = 1 latency path pays no act_rows kernels)
  if (ragged && c.block_type == 0 && !is_device_pointer(lens))
    for (int b = 0; b < B; ++b) enc_short = enc_short || lens[b] < L;
  if (enc_short) {
    RET(size_act(e, B, true, true));
    int32_t* he = act_host(e, slot.enc(), B);
    int32_t* hv = act_host(e, slot.var(), B);
    // (one limit for both variance predictors: the deeper reach of the two)
    const int add_var = std::max((c.var_layers - 1) * ((c.var_kernel - 1) / 2),
                                 ((c.energy_layers ? c.energy_layers : c.var_layers) - 1) * (((c.energy_kernel ? c.energy_kernel : c.var_kernel) - 1) / 2));
    double se = 0;
    for (int b = 0; b < B; ++b) {
      he[b] = (int32_t)std::min<long long>(std::max<long long>(lens[b], 0), L);   // lens_to_i32_kernel's clamp
      se += he[b];
    }
    const double sv = host_row_limits(hv, he, B, add_var, 1, L, 0);
    int32_t* dv = act_dev(e, slot.var(), B);
    KCHK(e, launch_act_rows(tl, dv, B, add_var, 1, L, e->stream));
    act_enc = RowLimits{tl, he, se / ((double)B * L)};
    act_var = RowLimits{dv, hv, sv / ((double)B * L)};
  }
  if (c.block_type == 1) RET(conformer_stack(e, e->cf_enc, c.n_head, x, ptr<float>(e->xb), tl, B, L, false));
  else if (c.block_type == 2) RET(fastformer_stack(e, e->ff_enc, x, ptr<float>(e->xb), tl, B, L, false));
  else RET(fft_stack(e, e->enc, c.n_head, x, ptr<float>(e->xb), tl, B, L, false, act_enc, true));  // encoder: always exact fp32, K-split kernel

  // Variance adaptor, inference branch (U/layers.py:195-258)
  float* xs = ptr<float>(e->xs);
  {
    ProfScope ps(e, "misc", 0, 0);
    KCHK(e, launch_add_speaker(x, xs, e->spk_emb, ptr<int64_t>(e->spk), n_spk_ids, c.n_speakers, B, L, H, e->stream));
  }
  RET(predictor(e, e->dur, xs, ptr<float>(e->logd), tl, B, L, act_enc));
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
    RET(predictor(e, e->pitch, xp, ptr<float>(e->ppred), nullptr, B, L, act_var));
  }
  if (!e_frame) {
    {
      ProfScope ps(e, "misc", 0, 0);
      KCHK(e, launch_var_positions(xs, ptr<int32_t>(e->posbuf), e->var_pos, (int)e->var_pos_rows, e->energy.alpha, xp, B, L, H, e->stream,
                                   p_frame));  // the positions depend on xs alone: the pitch predictor's pass (if it ran) left them in posbuf
    }
    RET(predictor(e, e->energy, xp, ptr<float>(e->epred), nullptr, B, L, act_var));
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
      RET(size_act(e, B, false, true));
      int32_t* hd = act_host(e, slot.dec(), B);
      for (int b = 0; b < B; ++b) hd[b] = (int32_t)e->h_mel[b];
      sx.act_rows = ml; sx.act_rows_host = hd;
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
      RET(predictor(e, e->pitch, xpf, ptr<float>(e->ppred), nullptr, B, (int)T, RowLimits(), true));
    }
    if (e_frame) {
      {
        ProfScope ps(e, "misc", 0, 0);
        KCHK(e, launch_var_positions(dx, ptr<int32_t>(e->posbuf), e->var_pos, (int)e->var_pos_rows, e->energy.alpha, xpf, B, (int)T, H, e->stream,
                                     !p_frame));
      }
      RET(predictor(e, e->energy, xpf, ptr<float>(e->epred), nullptr, B, (int)T, RowLimits(), true));
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
    RET(size_act(e, B, true, true));
    int32_t *ad = act_dev(e, slot.dec(), B), *ap = act_dev(e, slot.post(), B);
    int32_t *hd = act_host(e, slot.dec(), B), *hp = act_host(e, slot.post(), B);
    const int halo = vocoder_halo_frames(c);
    const int add_post = halo + 2 * c.postnet_layers * ((c.postnet_kernel - 1) / 2);
    KCHK(e, launch_act_rows(ml, ad, B, 0, 1, T, e->stream));
    KCHK(e, launch_act_rows(ml, ap, B, add_post, 1, T, e->stream));
    act_dec = ad;
    act_post = ap;
    // the same limits on the host (mel lengths are in e->h_mel since the sync above; duration_kernel wrote them to mel32 clamped to int32)
    e->rag_frac_dec = host_row_limits(hd, e->h_mel, B, 0, 1, T, 0) / ((double)B * T);
    e->rag_frac_post = host_row_limits(hp, e->h_mel, B, add_post, 1, T, 0) / ((double)B * T);
    e->rag_frac_voc = host_row_limits(nullptr, e->h_mel, B, halo, 1, T, 0) / ((double)B * T);
    act_dec_h = hd;
    act_post_h = hp;
  }
  // (a Conformer decoder computes every row: its attention is unmasked and its depthwise convolution crosses into the padding; so does a
  // Fastformer decoder: its inverted mask puts the pooling weight ON the padding)
  const int dec_heads = c.dec_n_head ? c.dec_n_head : c.n_head;
  if (c.block_type == 1) RET(conformer_stack(e, e->cf_dec, dec_heads, dx, ptr<float>(e->dxb), ml, B, (int)T, e->dec_precision == 1));
  else if (c.block_type == 2) RET(fastformer_stack(e, e->ff_dec, dx, ptr<float>(e->dxb), ml, B, (int)T, e->dec_precision == 1));
  else RET(fft_stack(e, e->dec, dec_heads, dx, ptr<float>(e->dxb), ml, B, (int)T, e->dec_precision == 1, RowLimits{act_dec, act_dec_h, act_dec ? e->rag_frac_dec : 1.0}));
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

}  // namespace eng
}  // namespace e2etts
