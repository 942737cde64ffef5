// Host-side logic of the engine that touches no HIP API: weight-blob header / directory validation, engine-config validation,
// the vocoder's receptive field, the ragged row limits, and the tile choice of conv_gemm.  Kept free of <hip/...> so that
// tests/csrc/host_logic_test.cc can build it with gcc -fsanitize=address,undefined and feed it truncated / corrupt blobs
// (tests/test_host_sanitizer.py); the engine's sources (engine.h), conv_gemm.hip and small_kernels.hip include the same header, so what the
// sanitizer run exercises is the code the library ships.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/e2etts.h"
#include "../../include/e2etts_forced.h"

namespace e2etts {

// Blob layout (e2e_tts_amd/packer.py: build_blob), little endian: 32-byte header, n_entries x 80-byte directory entries, then the
// fp32 tensors, each at a 256-byte aligned offset.
struct BlobHeader {
  char magic[8];
  uint32_t version;
  uint32_t n_entries;
  uint64_t data_offset;
  uint64_t total_bytes;
};
struct BlobEntry {
  char name[64];
  uint64_t offset;
  uint64_t numel;
};
static_assert(sizeof(BlobHeader) == 32 && sizeof(BlobEntry) == 80, "blob layout is fixed by packer.py");

struct BlobTensor {
  std::string name;
  uint64_t offset = 0, numel = 0;
};

// nullptr when the header is plausible for a blob of `nbytes` bytes, else a static message
inline const char* blob_check_header(const BlobHeader& h, size_t nbytes) {
  if (nbytes < sizeof(BlobHeader)) return "weight blob too small";
  if (memcmp(h.magic, "E2ETTSW1", 8) != 0 || h.version != 1) return "not an e2etts weight blob (bad magic / version)";
  if (h.total_bytes != (uint64_t)nbytes) return "blob size differs from the header's total";
  if (h.n_entries > 100000) return "corrupt blob directory (entry count)";
  const uint64_t dir_end = sizeof(BlobHeader) + (uint64_t)h.n_entries * sizeof(BlobEntry);
  if (dir_end > h.data_offset || h.data_offset > (uint64_t)nbytes || (h.data_offset & 255)) return "corrupt blob directory (data offset)";
  return nullptr;
}

// Validates the n_entries directory records (`dir` holds exactly h.n_entries of them) against the blob size and appends them to `out`.
// Every arithmetic step is overflow-checked: numel comes from the file.
inline const char* blob_check_directory(const BlobHeader& h, const BlobEntry* dir, size_t nbytes, std::vector<BlobTensor>& out, std::string& bad_name) {
  out.clear();
  out.reserve(h.n_entries);
  for (uint32_t i = 0; i < h.n_entries; ++i) {
    BlobEntry en = dir[i];
    en.name[sizeof en.name - 1] = 0;
    bad_name = en.name;
    if ((en.offset & 255) || en.offset < h.data_offset || en.offset > (uint64_t)nbytes) return "tensor lies outside the blob";
    if (en.numel > ((uint64_t)nbytes - en.offset) / 4) return "tensor lies outside the blob";
    BlobTensor t;
    t.name = en.name;
    t.offset = en.offset;
    t.numel = en.numel;
    out.push_back(t);
  }
  bad_name.clear();
  return nullptr;
}

// e2etts_create's argument validation (nullptr = valid)
inline const char* config_check(const e2etts_config& c) {
  // ranges first: every later expression (2 * rate, 4 << stages, hidden / n_head ...) then stays far inside int32
  auto in = [](int v, int lo, int hi) { return v >= lo && v <= hi; };
  const int BIG = 1 << 20;
  if (!in(c.hidden, 4, BIG) || !in(c.n_head, 1, BIG) || c.hidden % 4 || c.hidden % c.n_head) return "hidden must be a positive multiple of 4 and of n_head";
  if (!in(c.n_symbols, 1, BIG) || !in(c.n_speakers, 1, BIG)) return "n_symbols and n_speakers must be positive";
  if (!in(c.enc_layers, 0, 64) || !in(c.dec_layers, 0, 64)) return "layer counts out of range";
  if (!in(c.n_mel, 4, BIG) || c.n_mel % 4) return "n_mel must be a positive multiple of 4";
  if (!in(c.ffn_dim, 4, BIG) || !in(c.dur_chans, 4, BIG) || !in(c.var_chans, 4, BIG) || !in(c.postnet_dim, 4, BIG)) return "channel counts must be positive";
  if (c.ffn_dim % 4 || c.dur_chans % 4 || c.var_chans % 4 || c.postnet_dim % 4) return "channel counts must be multiples of 4";
  if (c.ffn_k2 != 1 || !in(c.ffn_k1, 1, 255) || !(c.ffn_k1 & 1)) return "FFN kernels must be (odd, 1)";
  if (!in(c.dur_layers, 1, 16) || !in(c.var_layers, 1, 16) || !in(c.dur_kernel, 1, 255) || !in(c.var_kernel, 1, 255) || !(c.dur_kernel & 1) || !(c.var_kernel & 1))
    return "predictor layer counts / kernels out of range";
  if ((c.energy_layers != 0 && !in(c.energy_layers, 1, 16)) || (c.energy_kernel != 0 && (!in(c.energy_kernel, 1, 255) || !(c.energy_kernel & 1))))
    return "energy predictor layer count / kernel out of range";
  if (!in(c.postnet_layers, 1, 16) || !in(c.postnet_kernel, 1, 255) || !(c.postnet_kernel & 1)) return "postnet layers / kernel out of range";
  if (!in(c.voc_stages, 1, E2ETTS_MAX_STAGES) || !in(c.voc_n_kernels, 1, E2ETTS_MAX_RB_KERNELS) || !in(c.voc_n_dil, 1, E2ETTS_MAX_DILATIONS))
    return "vocoder stage / kernel / dilation counts out of range";
  for (int i = 0; i < c.voc_stages; ++i)
    if (!in(c.voc_up_rate[i], 2, 1024) || c.voc_up_kernel[i] != 2 * c.voc_up_rate[i] || (c.voc_up_rate[i] & 1)) return "upsample kernel must be 2 x rate, rate even";
  for (int j = 0; j < c.voc_n_kernels; ++j) {
    if (!in(c.voc_rb_kernel[j], 1, 255) || !(c.voc_rb_kernel[j] & 1)) return "ResBlock kernel sizes must be odd";
    for (int m = 0; m < c.voc_n_dil; ++m)
      if (!in(c.voc_rb_dil[j][m], 1, 1024)) return "ResBlock dilations must be positive";
  }
  if (!in(c.voc_init_ch, 4, BIG) || (c.voc_init_ch >> c.voc_stages) < 4 || (c.voc_init_ch % (4 << c.voc_stages))) return "upsample_initial_channel too small for the stage count";
  if (c.voc_resblock != 1 && c.voc_resblock != 2) return "voc_resblock must be 1 or 2";
  if (c.voc_resblock == 2 && c.voc_n_dil != 2) return "ResBlock2 has exactly two dilated convolutions (voc_n_dil == 2)";
  if (c.voc_istft_nfft != 0) {
    const int n = c.voc_istft_nfft;
    if (n < 4 || n > 256 || (n & (n - 1)) || !in(c.voc_istft_hop, 1, 256) || n % c.voc_istft_hop) return "iSTFT: n_fft must be a power of two in [4, 256] and a multiple of the hop";
  }
  if (c.block_type != 0 && c.block_type != 1 && c.block_type != 2) return "block_type must be 0 (FFT block), 1 (Conformer block) or 2 (Fastformer block)";
  if (c.dec_n_head != 0 && (!in(c.dec_n_head, 1, BIG) || c.hidden % c.dec_n_head)) return "hidden must be a multiple of dec_n_head";
  if (c.block_type == 1) {
    const int dh = c.hidden / c.n_head, dhd = c.hidden / (c.dec_n_head ? c.dec_n_head : c.n_head);
    for (int d : {dh, dhd})
      if (d != 8 && d != 16 && d != 32 && d != 48 && d != 64 && d != 96) return "Conformer head dim must be one of 8, 16, 32, 48, 64, 96";
    if (c.ffn_dim < 2 * c.hidden) return "Conformer ffn_expansion_factor must be at least 2";
  }
  if (c.block_type == 2) {
    // U/blocks/fastformer.py:190-191: hidden / n_head heads of size n_head; fastformer.hip keeps one head's running sums in registers
    if (c.hidden > 1024) return "Fastformer: hidden must be at most 1024";
    for (int hs : {c.n_head, c.dec_n_head ? c.dec_n_head : c.n_head}) {
      if (c.hidden % hs) return "Fastformer: hidden must be a multiple of n_head and dec_n_head";
      if (hs != 1 && hs != 2 && hs != 4 && hs != 8) return "Fastformer: n_head / dec_n_head (the head SIZE of this block) must be 1, 2, 4 or 8";
      if (c.hidden / hs > 512) return "Fastformer: at most 512 heads (hidden / n_head)";
    }
  }
  if (c.n_bins != 256) return "n_bins must be 256";
  if (c.pitch_emb_rows != 0 && !in(c.pitch_emb_rows, c.n_bins, BIG)) return "pitch_emb_rows must cover n_bins";
  if ((c.pitch_no_uv != 0 && c.pitch_no_uv != 1) || (c.pitch_log2 != 0 && c.pitch_log2 != 1) || (c.pred_pad_left != 0 && c.pred_pad_left != 1) ||
      (c.pitch_frame != 0 && c.pitch_frame != 1) || (c.energy_frame != 0 && c.energy_frame != 1))
    return "pitch_no_uv / pitch_log2 / pred_pad_left / pitch_frame / energy_frame must be 0 or 1";
  if (!in(c.max_seq_len, 1, BIG) || !in(c.pos_table_rows, c.max_seq_len + 1, 1 << 24)) return "pos_table_rows must cover max_seq_len + 1";
  if (!in(c.hop_length, 1, BIG) || !in(c.sample_rate, 1, 1 << 24)) return "hop_length and sample_rate must be positive";
  return nullptr;
}

// Rows past the last valid one (mel_len * rate_i) that the layers of vocoder stage i have to compute so that every valid sample sees
// exactly the inputs the padded computation gives it: out[i], i = 0 .. voc_stages (i = 0: conv_pre's output, rate 1; i >= 1: the
// upsampler output and the ResBlocks of stage i, rate = product of the first i upsampling factors).  Conservative bound from the
// layer geometry, back to front: the tail reads `tail` rows of the trunk's output past a sample (conv_post: 3; iSTFTNet: conv_post 3
// frames + the reflection pad's shift of 1 + the inverse STFT's overlap -- a sample is the sum of n_fft / hop frames, n_fft / (2 hop) to
// either side); every layer of a stage computes the rows its output needs plus the widest ResBlock's reach
// sum_m ((k-1)/2 d_m + (k-1)/2) (one limit per stage covers the intermediate layers too); an upsampler reads +-2 input positions.
inline void vocoder_stage_halo_rows(const e2etts_config& c, long long out[E2ETTS_MAX_STAGES + 1]) {
  long long need = c.voc_istft_nfft ? 4 + (c.voc_istft_nfft + 2 * c.voc_istft_hop - 1) / (2 * c.voc_istft_hop) : 3;
  for (int i = c.voc_stages; i >= 1; --i) {
    long long worst = 0;
    for (int j = 0; j < c.voc_n_kernels; ++j) {
      long long sum = 0;
      for (int m = 0; m < c.voc_n_dil; ++m) sum += (long long)(c.voc_rb_kernel[j] - 1) / 2 * (c.voc_rb_dil[j][m] + 1);
      worst = sum > worst ? sum : worst;
    }
    out[i] = need + worst;
    const long long r = c.voc_up_rate[i - 1];
    need = (out[i] + r - 1) / r + 2;
  }
  out[0] = need;
}

// Frames of mel context one output frame depends on, each side: conv_pre's output limit plus its own 3 frames.
inline int vocoder_halo_frames(const e2etts_config& c) {
  long long h[E2ETTS_MAX_STAGES + 1];
  vocoder_stage_halo_rows(c, h);
  return (int)std::min<long long>(h[0] + 3, 1 << 24);
}

// conv_gemm tile choice for Cout > 64 (rows = T per utterance).  few: so few tiles (small batches, the B = 1 latency path, the encoder)
// that 128 x 128 tiles would leave CUs idle -> 64 x 64.  half (fragment path only): a 128 x 128 grid whose last round of workgroups
// (2 per CU = 512 at a time) is mostly empty runs as 64 x 128 tiles: twice the workgroups at half the work.
inline long long tiles_128(int B, int T, int Cout) {  // 128 x 128 tiles of the launch, saturating (the callers only compare with ~512)
  const long long t = ((long long)T + 127) / 128 * (((long long)Cout + 127) / 128);
  return t > (1LL << 40) / (B > 0 ? B : 1) ? (1LL << 40) : t * B;
}
// Under one round of 128 x 128 tiles but >= 6144 rows (the first vocoder stage at B = 1 .. 2, 6144 x 256: 96 tiles): 64 x 64 tiles are
// 384 workgroups whose waves each fetch their own weight fragments for ONE 32 x 32 MFMA tile -- that launch waits on L2 bandwidth
// (540 MB of fragments in 55 us) -- so those run as 64 x 128 too: 192 workgroups, two MFMA row tiles per fragment (B = 1 step: 9.46 ->
// 9.05 ms fp32, 5.21 -> 5.11 ms bf16x3; B = 4: -4 %).  With fewer rows (the decoder at B <= 4, the encoder) 64 x 64 stayed ahead.
// The predicates on counts (t128 = 128 x 128 tiles of the launch, rows = output rows of the launch): a ragged batch passes the tiles and
// rows that really run (conv_gemm.hip counts them from ConvParams::act_rows_host), a padded one those of B x T.
inline bool tile_many_rows_n(long long rows) { return rows >= 6144; }
inline bool tile_few_rows_n(long long t128, long long rows, int Cout) { return Cout > 64 && t128 < 2 * 256 && !tile_many_rows_n(rows); }
inline bool tile_half_rows_n(long long t128, long long rows, int Cout) {
  if (Cout <= 64 || tile_few_rows_n(t128, rows, Cout)) return false;
  if (t128 < 2 * 256) return true;  // under one round, many rows
  const long long slots = 2 * 256;
  const long long r128 = (t128 + slots - 1) / slots, r64 = (2 * t128 + slots - 1) / slots;
  return 0.5 * 1.06 * (double)r64 < (double)r128;
}
inline bool tile_many_rows(int B, int T) { return tile_many_rows_n((long long)B * T); }
inline bool tile_few_rows(int B, int T, int Cout) { return tile_few_rows_n(tiles_128(B, T, Cout), (long long)B * T, Cout); }
inline bool tile_half_rows(int B, int T, int Cout) { return tile_half_rows_n(tiles_128(B, T, Cout), (long long)B * T, Cout); }

// 128 x 128 tiles and rows of a ragged launch: utterance b computes min(rows[b], T) rows (rows = ConvParams::act_rows_host)
inline void ragged_counts(const int32_t* rows, int B, int T, int Cout, long long* t128, long long* nrows) {
  long long t = 0, r = 0;
  for (int b = 0; b < B; ++b) {
    const long long v = rows[b] < 0 ? 0 : (rows[b] > T ? T : rows[b]);
    t += (v + 127) / 128;
    r += v;
  }
  *t128 = t * (((long long)Cout + 127) / 128);
  *nrows = r;
}

// ---- ragged-batch row limits: the rows of utterance b that a layer computes, min(cap, (len + add) * mul + add_rows).  Written once:
// act_rows_kernel (small_kernels.hip) computes the device copy with it, host_row_limits the host copy that the compact grids
// (kernels.h: RowMap) are built from -- the two must agree row for row.
#ifdef __HIPCC__
#define E2ETTS_HOST_DEVICE __host__ __device__
#else
#define E2ETTS_HOST_DEVICE
#endif
E2ETTS_HOST_DEVICE inline long long row_limit(long long len, int add, int mul, long long cap, long long add_rows) {
  const long long v = (len + add) * mul + add_rows;
  return v < cap ? v : cap;
}
// out[0 .. B) (may be null): the limits the kernel writes for these lengths, which it reads as int32 (a length beyond INT32_MAX reached it
// as INT32_MAX).  Returns the sum over b of the limit of len[b] as given, a negative one counting as no rows (profile FLOP fractions).
template <typename Len>
inline double host_row_limits(int32_t* out, const Len* len, int B, int add, int mul, long long cap, long long add_rows) {
  double sum = 0;
  for (int b = 0; b < B; ++b) {
    const long long l = (long long)len[b], l32 = l < 0x7fffffffLL ? l : 0x7fffffffLL;
    if (out) out[b] = (int32_t)row_limit(l32, add, mul, cap, add_rows);
    const long long v = row_limit(l, add, mul, cap, add_rows);
    sum += (double)(v > 0 ? v : 0);
  }
  return sum;
}

// ---- e2etts_acoustic_forced (include/e2etts_forced.h): what the struct asks for, checked before anything is enqueued.
// Every member NULL: the call is e2etts_acoustic_ctl (the engine routes it there and reads nothing else of the struct).
inline bool forced_is_null(const e2etts_forced& f) {
  return !f.durations && !f.attn_soft && !f.mel_lens && !f.f0 && !f.uv && !f.pitch && !f.energy;
}
// What of the engine's state the checks depend on.
struct ForcedShape {
  int B = 0, L = 0;
  int pitch_no_uv = 0, pitch_frame = 0, energy_frame = 0;   // e2etts_config
  int max_seq_len = 0, pos_table_rows = 0;
  unsigned long long var_pos_rows = 0;   // rows of the variance predictors' position table
};
// "" when the struct is served, else the message (it names the offending value).  `struct_size` is what the caller wrote into the
// struct's first field (read before anything else; nothing of `f` is trusted when it is not this header's).  dur_host / mel_lens_host /
// lens_host: the same arrays when they lie in HOST memory, else nullptr (device arrays are clamped by the kernels that read them).
inline std::string forced_check(uint32_t struct_size, const e2etts_forced& f, const ForcedShape& s, const float* dur_host,
                                const int64_t* mel_lens_host, const int64_t* lens_host) {
  char m[256];
  auto msg = [&](const char* fmt, auto... a) { snprintf(m, sizeof m, fmt, a...); return std::string(m); };
  if (struct_size != sizeof(e2etts_forced))
    return msg("e2etts_forced.struct_size = %u, this library knows %zu: the caller was built against another revision of e2etts_forced.h",
               (unsigned)struct_size, sizeof(e2etts_forced));
  if (s.B <= 0 || s.L <= 0) return msg("B and L must be positive (got B=%d L=%d)", s.B, s.L);
  if (f.pitch_frames != 0 && f.pitch_frames != 1) return msg("pitch_frames = %d: expected 0 or 1", (int)f.pitch_frames);
  if (f.energy_frames != 0 && f.energy_frames != 1) return msg("energy_frames = %d: expected 0 or 1", (int)f.energy_frames);
  if (f.T < 0) return msg("T = %d is negative", (int)f.T);
  if (f.T > (1 << 20)) return msg("T=%lld is unreasonably large", (long long)f.T);
  // target kinds
  if (s.pitch_no_uv && (f.f0 || f.uv)) return msg("an f0 / uv target was given, but the model has pitch_no_uv = %d: pass `pitch`", s.pitch_no_uv);
  if (!s.pitch_no_uv && f.pitch) return msg("a `pitch` target was given, but the model has pitch_no_uv = %d (use_uv): pass f0 and uv", s.pitch_no_uv);
  if ((f.f0 != nullptr) != (f.uv != nullptr)) return msg("f0 and uv come together: %s is NULL", f.f0 ? "uv" : "f0");
  const bool has_p = f.f0 || f.pitch, has_e = f.energy != nullptr;
  // a [B, T] target: frame-resolved, or at the level of a frame_level feature
  const bool p_bt = has_p && (f.pitch_frames || s.pitch_frame), e_bt = has_e && (f.energy_frames || s.energy_frame);
  const bool p_avg = has_p && f.pitch_frames && !s.pitch_frame, e_avg = has_e && f.energy_frames && !s.energy_frame;
  if ((p_avg || e_avg) && !f.durations)
    return msg("a frame-resolved %s target of a phoneme_level feature is averaged over `durations`, which is NULL", p_avg ? "pitch" : "energy");
  if ((p_bt || e_bt) && f.T <= 0) return msg("a [B, T] %s target needs T, which is %d", p_bt ? "pitch" : "energy", (int)f.T);
  // soft expansion
  if (f.attn_soft) {
    if (f.T <= 0) return msg("attn_soft needs T, which is %d", (int)f.T);
    if (!f.mel_lens) return msg("attn_soft [B = %d, T = %d, L = %d] needs mel_lens, which is NULL", s.B, (int)f.T, s.L);
    if (f.T > s.max_seq_len && f.T > s.pos_table_rows)
      return msg("T=%lld exceeds the shipped position table (%d rows)", (long long)f.T, s.pos_table_rows);
    if ((s.pitch_frame || s.energy_frame) && (unsigned long long)f.T + 1 > s.var_pos_rows)
      return msg("T=%lld exceeds the variance predictors' position table (%lld rows)", (long long)f.T, (long long)s.var_pos_rows);
    if (mel_lens_host)
      for (int b = 0; b < s.B; ++b)
        if (mel_lens_host[b] < 1 || mel_lens_host[b] > f.T)
          return msg("mel_lens[%d]=%lld outside [1, %d]", b, (long long)mel_lens_host[b], (int)f.T);
  } else if (f.mel_lens) {
    return msg("mel_lens was given without attn_soft (T = %d): the length regulator takes its lengths from the durations", (int)f.T);
  }
  if (f.durations && dur_host) {
    for (int b = 0; b < s.B; ++b) {
      double sum = 0;
      const long long len = lens_host ? (lens_host[b] < 0 ? 0 : (lens_host[b] > s.L ? s.L : lens_host[b])) : s.L;
      for (int l = 0; l < s.L; ++l) {
        const float d = dur_host[(size_t)b * s.L + l];
        if (!(d == d) || std::isinf(d)) return msg("durations[%d, %d] = %g is not finite", b, l, (double)d);
        if (d < 0.f) return msg("durations[%d, %d] = %g is negative", b, l, (double)d);
        if (d != std::floor(d)) return msg("durations[%d, %d] = %g is not an integer", b, l, (double)d);
        if (d > 1048576.f) return msg("durations[%d, %d] = %g exceeds 2^20 frames", b, l, (double)d);
        if (l < len) sum += d;
      }
      if ((p_avg || e_avg) && sum > (double)f.T)
        return msg("durations of utterance %d sum to %.0f frames, the frame-resolved targets have T = %d", b, sum, (int)f.T);
    }
  }
  return std::string();
}

}  // namespace e2etts
