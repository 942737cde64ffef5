// libe2etts_mel.so: the reference's TorchSTFT.mel_spectrogram (e2e_tts/src/tools/stft.py:46-89) behind the C ABI of include/e2etts_mel.h.
// A companion of libe2etts_hip.so that shares its kernel objects (the exact-fp32 convolution launch_conv_gemm is the transform, as it
// is the denoiser's forward STFT) and none of its entry points.
//
// Three launches per call:
//   pad        mel_pad_kernel: per row (n_fft - hop) / 2 reflected samples, the row's own samples (int16 PCM / 32768 when asked), the
//              reflection at the row's OWN end, zeros; written as rows [B, R, hop], R = T + n_overlap - 1;
//   transform  one exact-fp32 launch_conv_gemm, Cin = hop, KW = n_overlap, pad = 0, Cout = Cpad (re[0 .. bins) | im[0 .. bins) | zero
//              columns up to a multiple of 32): frame f is rows f .. f + n_overlap - 1.  The convolution has one length for input and
//              output, so the spectrum is [B, R, Cpad]; its last n_overlap - 1 rows per utterance are frames that do not exist and are
//              never read;
//   tail       mel_tail_kernel: a tile of frames per workgroup; re | im -> magnitudes in LDS once, the energy reduced in a fixed order, the
//              banded mel projection, the clamp and the log (the floor log(clip) itself computed on the host in float64).  The spectrum is read exactly once, magnitudes never reach HBM.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../../include/e2etts_mel.h"
#ifdef E2EMEL_TEST_HOOKS
#define E2E_COMPANION_TEST_HOOKS
#endif
#include "../companion/handle.h"
#include "../kernels.h"

#ifndef E2EMEL_SRC_HASH
#define E2EMEL_SRC_HASH "unknown"
#endif

using namespace e2etts;
using namespace e2etts::companion;

static_assert(E2EMEL_OK == E_OK && E2EMEL_EINVAL == E_INVAL && E2EMEL_EHIP == E_HIP && E2EMEL_ESTATE == E_STATE && E2EMEL_ENOMEM == E_NOMEM,
              "include/e2etts_mel.h and csrc/companion/handle.h disagree on the error codes");

namespace {

constexpr int TAIL_THREADS = 256;
constexpr int TAIL_MAX_FRAMES = 16;
constexpr size_t TAIL_LDS_MAX = 64 * 1024;   // what a kernel gets without opting in

// One thread per 4 consecutive positions of the padded signal of row blockIdx.y (hop % 32 == 0: rows and float4s line up).  Position p holds
// sample s = p - half of the row, reflected about 0 and about nb - 1 (F.pad(mode = 'reflect'): the edge sample is not repeated); positions
// past nb + 2 * half are zeros.  The host has checked half < nb <= n <= stride, so every s read lies in [0, nb).
template <typename TIn>
__global__ void __launch_bounds__(256) mel_pad_kernel(const TIn* __restrict__ audio, long long stride, const int32_t* __restrict__ n_valid,
                                                      float* __restrict__ out, int R, int hop, int half) {
  const int b = blockIdx.y;
  const long long total4 = (long long)R * hop / 4;
  const long long i4 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i4 >= total4) return;
  const long long nb = n_valid[b];
  const long long padded = nb + 2LL * half;
  const TIn* w = audio + (long long)b * stride;
  float t[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long long p = i4 * 4 + k;
    long long s = p - half;
    if (s < 0) s = -s;
    else if (s >= nb) s = 2 * (nb - 1) - s;
    float v = 0.f;
    if (p < padded) {
      if (sizeof(TIn) == 2) v = (float)w[s] * (1.0f / 32768.0f);   // exact: a power of two
      else v = (float)w[s];
    }
    t[k] = v;
  }
  *reinterpret_cast<float4*>(out + ((long long)b * R * hop + i4 * 4)) = make_float4(t[0], t[1], t[2], t[3]);
}

// One workgroup = FT frames (a power of two <= 16) of row blockIdx.y, 4 wavefronts.
//
// Phase 1: wavefront w takes frames w, w + 4, ...; its lanes stride the bins, so lane l reads re / im of bins l, l + 64, ... (coalesced),
// writes mag[f][k] and squares it into its own partial of the energy (ascending k); the 64 partials are summed by a butterfly whose shape
// does not depend on the grid or the batch: the energy of a frame is the same bits wherever the frame lies.
// Phase 2: lane l of a wavefront holds frame f = l mod FT and mel row r = l / FT of the 64 / FT rows the wavefront takes at a time.  The
// wavefront walks the UNION of its rows' bands in ascending k; a lane adds w[m][k] * mag[f][k] only while k lies in its own row's band, so
// each mel value is the sum over its band alone, in ascending bin order.
//
// LDS row stride = bins, which is odd (n_fft / 2 is even for every geometry served).  Phase 1 writes 64 consecutive dwords per instruction:
// conflict-free at any stride.  Phase 2 reads mag[f][k] with one k per wavefront: lanes of the same frame read the same address (a
// broadcast), lanes of different frames are f * bins dwords apart, and with bins odd f * bins mod 32 is distinct for all f < 32 -- the up
// to 16 distinct addresses of a 32-lane group fall into distinct banks.  Any even stride would fold frames onto each other's banks.
__global__ void __launch_bounds__(TAIL_THREADS) mel_tail_kernel(const float* __restrict__ spec, const float* __restrict__ basis,
                                                                const int2* __restrict__ band, const int32_t* __restrict__ lens,
                                                                float* __restrict__ mel, float* __restrict__ energy, int T, int R, int Cpad, int bins,
                                                                int n_mel, int FT, float clip, float log_clip) {
  extern __shared__ __attribute__((aligned(16))) float mel_smag[];   // [FT][bins]
  const int b = blockIdx.y, t0 = blockIdx.x * FT, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int len = lens[b];
  const int in_tile = min(FT, T - t0);            // frames of this tile that exist in the output
  const int nf = max(0, min(in_tile, len - t0));  // of those, the frames of the recording
  // frames >= mel_lens[b]: zeros in both outputs, nothing computed
  for (int e = tid; e < (in_tile - nf) * n_mel; e += TAIL_THREADS) mel[((size_t)b * T + t0 + nf) * n_mel + e] = 0.f;
  for (int f = nf + tid; f < in_tile; f += TAIL_THREADS) energy[(size_t)b * T + t0 + f] = 0.f;
  if (nf == 0) return;   // uniform over the workgroup
  for (int f = wave; f < nf; f += 4) {
    const float* row = spec + ((size_t)b * R + t0 + f) * Cpad;
    float e = 0.f;
    for (int k = lane; k < bins; k += 64) {
      const float re = row[k], im = row[bins + k];
      // sqrt((re^2 + im^2) + 1e-9), every product and sum rounded on its own as torch's pow(2).sum(-1) + 1e-9 rounds them
      const float mg = sqrtf(__fadd_rn(__fadd_rn(mul_rn(re, re), mul_rn(im, im)), 1e-9f));
      mel_smag[f * bins + k] = mg;
      e = fmaf(mg, mg, e);
    }
    for (int o = 32; o >= 1; o >>= 1) e += __shfl_xor(e, o, 64);
    if (lane == 0) energy[(size_t)b * T + t0 + f] = sqrtf(e);
  }
  __syncthreads();
  const int f = lane & (FT - 1), r = lane / FT, rows = 64 / FT;
  const int fr = min(f, nf - 1);   // lanes of frames past nf read a row that was written and store nothing
  for (int m0 = wave * rows; m0 < n_mel; m0 += 4 * rows) {   // uniform over the wavefront
    const int m = m0 + r;
    const bool live = m < n_mel && f < nf;
    int first = 0x7fffffff, last = -1;
    if (live) {
      const int2 bd = band[m];
      if (bd.y >= bd.x) {   // (an all-zero row keeps the empty band and does not widen the union)
        first = bd.x;
        last = bd.y;
      }
    }
    int kmin = first, kmax = last;
    for (int o = 32; o >= 1; o >>= 1) {
      kmin = min(kmin, __shfl_xor(kmin, o, 64));
      kmax = max(kmax, __shfl_xor(kmax, o, 64));
    }
    const float* wrow = basis + (size_t)min(m, n_mel - 1) * bins;
    const float* mrow = mel_smag + fr * bins;
    float acc = 0.f;
    // A wavefront whose rows are all empty (an all-zero basis, a group of masked channels) has kmin = INT_MAX > kmax = -1 and walks
    // nothing; inside the guard 0 <= kmin <= kmax < bins, so neither k nor kmax - 3 can overflow.
    if (kmin <= kmax) {
      int k = kmin;
      for (; k <= kmax - 3; k += 4) {      // four bins' loads in flight per pass; the additions stay in ascending order
        float w[4], v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          w[u] = wrow[k + u];
          v[u] = mrow[k + u];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (k + u >= first && k + u <= last) acc = fmaf(w[u], v[u], acc);
      }
      for (; k <= kmax; ++k) {
        const float w = wrow[k], v = mrow[k];
        if (k >= first && k <= last) acc = fmaf(w, v, acc);
      }
    }
    // log(max(acc, clip)): a clamped element gets the host's correctly rounded log(clip) (logf is good to an ulp, and the floor is the
    // value of every silent frame); a NaN fails the comparison and stays a NaN, as under torch.clamp(min)
    if (live) mel[((size_t)b * T + t0 + f) * n_mel + m] = acc <= clip ? log_clip : logf(acc);
  }
}

thread_local std::string g_create_error;

}  // namespace

struct e2emel_handle : Handle {
  int n_fft = 0, hop = 0, nov = 0, n_mel = 0, bins = 0, cpad = 0, tile = 0;
  float clip = 1e-5f, log_clip = 0.f;            // log_clip = log(clip) in float64, rounded once
  bool loaded = false;
  Buf wf{this, Buf::WEIGHTS}, wf_frag{this, Buf::WEIGHTS}, basis{this, Buf::WEIGHTS}, band{this, Buf::WEIGHTS};   // the bases
  Buf in{this}, pad{this}, spec{this}, mel{this}, energy{this}, lens{this};   // workspaces; mel / energy are the resident outputs
  std::vector<int32_t> host_lens;                // int32 image of the frame counts: outlives the asynchronous copy of a call
  std::vector<int64_t> host_lens64;
  std::vector<int32_t> host_band;                // [n_mel][first, last] as recorded by e2emel_load
  int rB = 0;                                    // batch of the resident outputs (0: nothing resident)
};

namespace {

// the images of e2emel_load into fresh buffers nb = {wf, wf_frag, basis, band}; returns after the stream has drained
int stage_bases(e2emel_handle* h, Buf* nb, const std::vector<float>& wf, const std::vector<float>& mb, const std::vector<int32_t>& band) {
  HIPCHK(h, hipStreamSynchronize(h->stream));
  RET(reserve(h, nb[0], wf.size() * 4));
  RET(reserve(h, nb[1], x3_frag_bytes(h->cpad, h->nov, h->hop)));
  RET(reserve(h, nb[2], mb.size() * 4));
  RET(reserve(h, nb[3], band.size() * 4));
  HIPCHK(h, hipMemcpyAsync(nb[0].p, wf.data(), wf.size() * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(nb[2].p, mb.data(), mb.size() * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(nb[3].p, band.data(), band.size() * 4, hipMemcpyHostToDevice, h->stream));
  KCHK(h, launch_f32_to_frag((const float*)nb[0].p, (float*)nb[1].p, h->cpad, h->nov, h->hop, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));   // the host images are read until here
  return E2EMEL_OK;
}

// the geometry limits, those of denoiser_geometry_check restated on the host side of this library so that e2emel_create gives its own message
const char* geometry_check(int n_fft, int hop, int n_mel, int* nov_out) {
  if (const char* m = denoiser_geometry_check(n_fft, hop, nov_out)) return m;
  if (n_mel < 4 || n_mel % 4 || n_mel > E2EMEL_MAX_MEL) return "n_mel must be a positive multiple of 4, at most E2EMEL_MAX_MEL";
  return nullptr;
}

int tile_frames(int bins) {
  int ft = TAIL_MAX_FRAMES;
  while (ft > 1 && (size_t)ft * bins * 4 > TAIL_LDS_MAX) ft >>= 1;
  return ft;
}

// the tail over the spectrum in h->spec ([B, T + n_overlap - 1, cpad]) into h->mel / h->energy, frames [B] on the device: the one place
// mel_tail_kernel is launched from (e2emel_forward, and e2emel_debug_tail of the test build)
int launch_tail(e2emel_handle* h, const int32_t* d_frames, int B, int T) {
  const int FT = h->tile, R = T + h->nov - 1;
  hipLaunchKernelGGL(mel_tail_kernel, dim3((T + FT - 1) / FT, B), dim3(TAIL_THREADS), (size_t)FT * h->bins * 4, h->stream, (const float*)h->spec.p,
                     (const float*)h->basis.p, (const int2*)h->band.p, d_frames, (float*)h->mel.p, (float*)h->energy.p, T, R, h->cpad, h->bins,
                     h->n_mel, FT, h->clip, h->log_clip);
  HIPCHK(h, hipGetLastError());
  return E2EMEL_OK;
}

}  // namespace

extern "C" {

const char* e2emel_version(void) { return "e2etts-mel 1 E2EMEL_SRC_HASH=" E2EMEL_SRC_HASH; }
int e2emel_abi_version(void) { return E2EMEL_ABI_VERSION; }

const char* e2emel_last_error(const e2emel_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int e2emel_create(int device_id, int n_fft, int hop, int n_mel, e2emel_handle** out) {
  if (!out) {
    g_create_error = "e2emel_create: out is NULL";
    return E2EMEL_EINVAL;
  }
  *out = nullptr;
  int nov = 0;
  const char* m = device_id < 0 ? "device_id must not be negative" : geometry_check(n_fft, hop, n_mel, &nov);
  if (m) {
    g_create_error = std::string("e2emel_create: ") + m + " (n_fft " + std::to_string(n_fft) + ", hop " + std::to_string(hop) + ", n_mel " +
                     std::to_string(n_mel) + "); served: n_fft = hop * n_overlap, n_overlap in {2, 4, 8}, hop % 32 == 0, hop <= 1024, n_mel % 4 == 0";
    return E2EMEL_EINVAL;
  }
  e2emel_handle* h = new (std::nothrow) e2emel_handle();
  if (!h) {
    g_create_error = "out of host memory";
    return E2EMEL_ENOMEM;
  }
  h->device = device_id;
  h->n_fft = n_fft; h->hop = hop; h->nov = nov; h->n_mel = n_mel;
  h->bins = n_fft / 2 + 1;
  h->cpad = (2 * h->bins + 31) / 32 * 32;
  h->tile = tile_frames(h->bins);   // hop <= 1024, n_overlap <= 8: bins <= 4097, one row is 16 KiB: always fits
  *out = h;
  return E2EMEL_OK;
}

void e2emel_destroy(e2emel_handle* h) { companion::destroy(h); }

int e2emel_load(e2emel_handle* h, const float* dft_basis, const float* mel_basis, float clip_val) {
  if (!h) return E2EMEL_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  if (!dft_basis || !mel_basis) return h->fail(E2EMEL_EINVAL, "dft_basis and mel_basis must not be NULL");
  if (!(clip_val > 0.f) || !std::isfinite(clip_val)) return h->fail(E2EMEL_EINVAL, "clip_val must be a positive finite number (its logarithm is the floor of the mel)");
  const int N = h->n_fft, bins = h->bins, cpad = h->cpad, M = h->n_mel;
  // the DFT basis -> conv_gemm's tap-major [Cout][KW * Cin] with Cout = cpad (rows beyond 2 * bins zero) and tap j = columns j * hop ..:
  // the basis rows as they are
  std::vector<float> hb, mb, wf((size_t)cpad * N, 0.f);
  RET(fetch_host(h, dft_basis, (size_t)2 * bins * N, hb));
  RET(fetch_host(h, mel_basis, (size_t)M * bins, mb));
  std::copy(hb.begin(), hb.end(), wf.begin());
  // [first, last] non-zero bin of every mel row (an all-zero row: the empty band [0, -1])
  std::vector<int32_t> band((size_t)2 * M);
  for (int m = 0; m < M; ++m) {
    int first = 0, last = -1;
    for (int k = 0; k < bins; ++k)
      if (mb[(size_t)m * bins + k] != 0.f) {
        if (last < 0) first = k;
        last = k;
      }
    band[2 * m] = first;
    band[2 * m + 1] = last;
  }
  RET(open_device(h));
  // staged in buffers of their own and swapped in only when everything has arrived: a failure leaves the bases loaded before in place
  Buf nb[4];   // wf, wf_frag, basis, band: free-standing until they replace the members below
  const int rc = stage_bases(h, nb, wf, mb, band);
  if (rc != E2EMEL_OK) {
    for (Buf& b : nb) release(h, b);
    return rc;
  }
  const auto swap_in = [h](Buf& member, const Buf& fresh) {
    release(h, member);   // the stream is drained: nothing reads the old bases
    member = fresh;
  };
  swap_in(h->wf, nb[0]); swap_in(h->wf_frag, nb[1]); swap_in(h->basis, nb[2]); swap_in(h->band, nb[3]);
  h->rB = 0;
  h->host_band = band;
  h->clip = clip_val;
  h->log_clip = (float)std::log((double)clip_val);
  h->loaded = true;
  return E2EMEL_OK;
}

void* e2emel_stream(e2emel_handle* h) { return companion::stream(h); }
int e2emel_order_after(e2emel_handle* h, void* caller_stream) { return companion::order_after(h, caller_stream); }
int e2emel_sync(e2emel_handle* h) { return companion::sync(h); }
size_t e2emel_device_bytes(const e2emel_handle* h) { return companion::device_bytes(h); }

int e2emel_forward(e2emel_handle* h, const void* audio, int dtype, long long audio_stride, const int64_t* n_valid, int B, long long n, float* mel_out,
                   float* energy_out, int64_t* mel_lens_out, int* T_out) {
  if (!h) return E2EMEL_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  // ---- validation: nothing is enqueued before the last check
  if (!audio) return h->fail(E2EMEL_EINVAL, "audio must not be NULL");
  if (dtype != E2EMEL_F32 && dtype != E2EMEL_I16) return h->fail(E2EMEL_EINVAL, "dtype must be E2EMEL_F32 or E2EMEL_I16 (got " + std::to_string(dtype) + ")");
  if (B < 1 || B > E2EMEL_MAX_B) return h->fail(E2EMEL_EINVAL, "B must lie in [1, " + std::to_string(E2EMEL_MAX_B) + "] (got " + std::to_string(B) + ")");
  if (n < 1 || audio_stride < n)
    return h->fail(E2EMEL_EINVAL, "need n >= 1 and audio_stride >= n (got n " + std::to_string(n) + ", audio_stride " + std::to_string(audio_stride) + ")");
  const int hop = h->hop, nov = h->nov, half = (h->n_fft - hop) / 2;
  // 32-bit offsets inside one utterance of the convolution (its input rows of hop floats, its output rows of cpad floats)
  const long long T_cap = (1LL << 29) / (h->cpad > hop ? h->cpad : hop) - nov;
  if (n / hop > T_cap) return h->fail(E2EMEL_EINVAL, "n too large: one row's spectrum must stay below 2 GiB (at most " + std::to_string(T_cap) + " frames)");
  const size_t esz = dtype == E2EMEL_I16 ? 2 : 4;
  if ((uintptr_t)audio % esz) return h->fail(E2EMEL_EINVAL, "audio is not aligned to its element size");
  std::vector<int64_t> nv((size_t)B, (int64_t)n);
  if (n_valid) RET(fetch_host(h, n_valid, (size_t)B, nv));
  int T = 0;
  for (int b = 0; b < B; ++b) {
    const long long v = nv[b];
    if (v > n || v <= half || v < hop)
      return h->fail(E2EMEL_EINVAL, "n_valid[" + std::to_string(b) + "] = " + std::to_string(v) + ": need (n_fft - hop) / 2 = " + std::to_string(half) +
                                        " < n_valid <= n = " + std::to_string(n) + " (a shorter row cannot be reflected) and n_valid >= hop = " +
                                        std::to_string(hop) + " (one frame)");
    T = std::max(T, (int)(v / hop));
  }
  if (!h->loaded) return h->fail(E2EMEL_ESTATE, "e2emel_forward before e2emel_load");
  // ---- enqueue
  RET(begin_call(h));
  h->rB = 0;
  const int R = T + nov - 1, M = h->n_mel;
  bool ragged = false;
  h->host_lens.resize(B);
  h->host_lens64.resize(B);
  for (int b = 0; b < B; ++b) {
    h->host_lens64[b] = nv[b] / hop;
    h->host_lens[b] = (int32_t)(nv[b] / hop);
    ragged = ragged || h->host_lens[b] != T;
  }
  // device tables: [B] frames (int32) | [B] samples (int32)
  std::vector<int32_t>& hl = h->host_lens;
  hl.resize((size_t)2 * B);
  for (int b = 0; b < B; ++b) hl[(size_t)B + b] = (int32_t)nv[b];   // n <= T_cap * hop < 2^29
  RET(reserve(h, h->lens, hl.size() * 4));
  RET(reserve(h, h->pad, (size_t)B * R * hop * 4));
  RET(reserve(h, h->spec, (size_t)B * R * h->cpad * 4));
  RET(reserve(h, h->mel, (size_t)B * T * M * 4));
  RET(reserve(h, h->energy, (size_t)B * T * 4));
  hipStream_t s = h->stream;
  HIPCHK(h, hipMemcpyAsync(h->lens.p, hl.data(), hl.size() * 4, hipMemcpyHostToDevice, s));
  const void* dev_audio = audio;
  long long stride = audio_stride;
  if (!is_device_pointer(audio)) {   // host samples: only the n samples of each row travel
    RET(reserve(h, h->in, (size_t)B * n * esz));
    HIPCHK(h, hipMemcpy2DAsync(h->in.p, (size_t)n * esz, audio, (size_t)audio_stride * esz, (size_t)n * esz, B, hipMemcpyHostToDevice, s));
    dev_audio = h->in.p;
    stride = n;
  }
  const int32_t* d_frames = (const int32_t*)h->lens.p;
  const int32_t* d_samples = d_frames + B;
  if (h->profile) HIPCHK(h, hipEventRecord(h->ev[0], s));
  {
    const long long total4 = (long long)R * hop / 4;
    const dim3 grid((unsigned)((total4 + 255) / 256), B);
    if (dtype == E2EMEL_I16)
      hipLaunchKernelGGL(mel_pad_kernel<int16_t>, grid, dim3(256), 0, s, (const int16_t*)dev_audio, stride, d_samples, (float*)h->pad.p, R, hop, half);
    else
      hipLaunchKernelGGL(mel_pad_kernel<float>, grid, dim3(256), 0, s, (const float*)dev_audio, stride, d_samples, (float*)h->pad.p, R, hop, half);
    HIPCHK(h, hipGetLastError());
  }
  if (h->profile) HIPCHK(h, hipEventRecord(h->ev[1], s));
  {
    ConvParams p;
    p.B = B; p.T = R; p.in = (const float*)h->pad.p; p.w = (const float*)h->wf.p; p.wfrag = (const float*)h->wf_frag.p; p.out = (float*)h->spec.p;
    p.Cin = hop; p.Cout = h->cpad; p.KW = nov; p.pad = 0; p.x3 = 0;   // exact fp32
    p.in_ld = p.Cin; p.out_ld = p.Cout; p.in_bs = (long long)R * p.in_ld; p.out_bs = (long long)R * p.out_ld;
    if (ragged) { p.act_rows = d_frames; p.act_rows_host = hl.data(); }   // rows past a recording's frames are not computed (nor read below)
    KCHK(h, launch_conv_gemm(p, s));
  }
  if (h->profile) HIPCHK(h, hipEventRecord(h->ev[2], s));
  RET(launch_tail(h, d_frames, B, T));
  if (h->profile) HIPCHK(h, hipEventRecord(h->ev[3], s));
  RET(copy_out(h, mel_out, h->mel.p, (size_t)B * T * M * 4));
  RET(copy_out(h, energy_out, h->energy.p, (size_t)B * T * 4));
  if (mel_lens_out) {
    if (is_device_pointer(mel_lens_out)) HIPCHK(h, hipMemcpyAsync(mel_lens_out, h->host_lens64.data(), (size_t)B * 8, hipMemcpyHostToDevice, s));
    else memcpy(mel_lens_out, h->host_lens64.data(), (size_t)B * 8);
  }
  const Phase phases[3] = {{0, 1}, {1, 2}, {2, 3}};   // pad, transform, tail
  RET(finish(h, phases));
  h->rB = B;
  if (T_out) *T_out = T;
  return E2EMEL_OK;
}

const float* e2emel_mel_dev(e2emel_handle* h) {
  if (!h) return nullptr;
  std::lock_guard<std::mutex> lk(h->mu);
  return h->rB ? (const float*)h->mel.p : nullptr;
}

const float* e2emel_energy_dev(e2emel_handle* h) {
  if (!h) return nullptr;
  std::lock_guard<std::mutex> lk(h->mu);
  return h->rB ? (const float*)h->energy.p : nullptr;
}

int e2emel_tile_frames(const e2emel_handle* h) { return h ? h->tile : 0; }

int e2emel_profile_enable(e2emel_handle* h, int on) { return companion::profile_enable(h, on); }
int e2emel_profile_read(e2emel_handle* h, double ms_out[3]) { return companion::profile_read(h, ms_out); }

#ifdef E2EMEL_TEST_HOOKS
int e2emel_debug_poison_workspace(e2emel_handle* h) {
  if (!h) return E2EMEL_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  RET(poison_workspaces(h));
  h->rB = 0;
  return E2EMEL_OK;
}

int e2emel_debug_force_dense(e2emel_handle* h, int on) {
  if (!h) return E2EMEL_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  if (!h->loaded) return h->fail(E2EMEL_ESTATE, "e2emel_debug_force_dense before e2emel_load");
  HIPCHK(h, hipSetDevice(h->device));
  std::vector<int32_t> band = h->host_band;
  if (on)
    for (int m = 0; m < h->n_mel; ++m) {
      band[2 * m] = 0;
      band[2 * m + 1] = h->bins - 1;
    }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(h->band.p, band.data(), band.size() * 4, hipMemcpyHostToDevice));
  return E2EMEL_OK;
}

int e2emel_debug_tail(e2emel_handle* h, const float* spec, const int32_t* frames, int B, int T, float* mel_out, float* energy_out) {
  if (!h) return E2EMEL_EINVAL;
  std::lock_guard<std::mutex> lk(h->mu);
  if (!spec || !frames) return h->fail(E2EMEL_EINVAL, "spec and frames must not be NULL");
  if (B < 1 || B > E2EMEL_MAX_B || T < 1 || T > (1 << 20)) return h->fail(E2EMEL_EINVAL, "e2emel_debug_tail: B or T out of range");
  std::vector<int32_t> fr;
  RET(fetch_host(h, frames, (size_t)B, fr));
  for (int b = 0; b < B; ++b)
    if (fr[b] < 0 || fr[b] > T) return h->fail(E2EMEL_EINVAL, "e2emel_debug_tail: frames[b] must lie in [0, T]");
  if (!h->loaded) return h->fail(E2EMEL_ESTATE, "e2emel_debug_tail before e2emel_load");
  RET(begin_call(h));
  h->rB = 0;
  const size_t R = (size_t)T + h->nov - 1, M = h->n_mel;
  h->host_lens = fr;   // outlives the asynchronous copy
  RET(reserve(h, h->lens, (size_t)B * 4));
  RET(reserve(h, h->spec, (size_t)B * R * h->cpad * 4));
  RET(reserve(h, h->mel, (size_t)B * T * M * 4));
  RET(reserve(h, h->energy, (size_t)B * T * 4));
  HIPCHK(h, hipMemcpyAsync(h->lens.p, h->host_lens.data(), (size_t)B * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->spec.p, spec, (size_t)B * R * h->cpad * 4, hipMemcpyDefault, h->stream));
  RET(launch_tail(h, (const int32_t*)h->lens.p, B, T));
  RET(copy_out(h, mel_out, h->mel.p, (size_t)B * T * M * 4));
  RET(copy_out(h, energy_out, h->energy.p, (size_t)B * T * 4));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->unfinished = false;
  h->rB = B;
  return E2EMEL_OK;
}
#endif

}  // extern "C"
