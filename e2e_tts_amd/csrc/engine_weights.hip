// Weight binding: the blob's tensors onto the engine's layer structs, and the images built from them at load time (fragment-order,
// bf16, fp16) that the kernels read instead.
#include "engine.h"

namespace e2etts {
namespace eng {

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

static int make_frag(e2etts_engine* e, const float* wx3, uint64_t cout, uint64_t kw, uint64_t cin) {
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
static int make_frag32(e2etts_engine* e, const float* w, uint64_t cout, uint64_t kw, uint64_t cin, bool narrow = false, bool phoneme_level = false) {
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
static int make_bimg(e2etts_engine* e, const float* wx3, uint64_t cout, uint64_t kw, uint64_t cin, int tap_split = 0,
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
static int make_r16(e2etts_engine* e, const float* src, size_t n, bool fp16 = false) {
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
static int make_himg(e2etts_engine* e, const float* w, uint64_t cout, uint64_t kw, uint64_t cin, int tap_split = 0) {
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

static int get_tensor(e2etts_engine* e, const std::string& name, uint64_t numel, const float** out) {
  auto it = e->tensors.find(name);
  if (it == e->tensors.end()) return e->fail(E2ETTS_EKEY, "weight blob has no tensor '%s'", name.c_str());
  if (numel && it->second.second != numel)
    return e->fail(E2ETTS_EINVAL, "tensor '%s' has %llu elements, expected %llu", name.c_str(),
                   (unsigned long long)it->second.second, (unsigned long long)numel);
  *out = it->second.first;
  return E2ETTS_OK;
}

static int bind_fft(e2etts_engine* e, const char* side, int layers, std::vector<FFTLayer>& v) {
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

static int bind_cf_gemm(e2etts_engine* e, const std::string& name, const char* bias, uint64_t cout, uint64_t cin, CfGemm& g) {
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

static int bind_conformer(e2etts_engine* e, const char* side, int layers, std::vector<CfLayer>& v, int n_head) {
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

static int bind_ff_gemm(e2etts_engine* e, const std::string& name, const std::string& bias, uint64_t cout, uint64_t kw, uint64_t cin, CfGemm& g) {
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

static int bind_fastformer(e2etts_engine* e, const char* side, int layers, FfSide& v, int n_head) {
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

static int bind_pred(e2etts_engine* e, const char* name, int layers, int kernel, int chans, int odim, bool alpha, Predictor& pr) {
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
static int bind_conv(e2etts_engine* e, const std::string& name, uint64_t cout, uint64_t kw, uint64_t cin, ConvW& w) {
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

}  // namespace eng
}  // namespace e2etts
