#include "engine.h"

namespace e2etts {
namespace eng {

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
static int denoise_fwd_conv(e2etts_engine* e, const float* pad, float* spec, const int32_t* h_tab, const int32_t* d_tab, int B, int R) {
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
static int denoise_inv_convs(e2etts_engine* e, const float* spec, float* ola, const int32_t* h_tab, const int32_t* d_tab, int B, int R) {
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

}  // namespace eng
}  // namespace e2etts
