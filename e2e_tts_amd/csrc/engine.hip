// Engine + C ABI (include/e2etts.h): owns the weights, the workspace, one HIP stream, and sequences the
// kernels of kernels.h into the reference's inference path
//   UnsupervisedFastSpeech2.inference (reference U/model.py:155-194)  ->  HifiGan.forward (V/generator.py:37-53)
// exactly as TTS.inference drives them per batch (API/utils.py:130-148).
// This file: the C ABI and what only it uses.  The passes it sequences live in engine_{core,weights,acoustic,vocoder,denoise}.hip, behind
// engine.h.
#include <dlfcn.h>

#include "engine.h"
#include "forced_entry.h"

namespace {

thread_local std::string g_create_error;

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

int copy_out(e2etts_engine* e, void* dst, const void* src, size_t bytes) {
  HIPCHK(e, hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, e->stream));
  return E2ETTS_OK;
}

int denoise_ready(e2etts_engine* e) {
  if (!e->dn.loaded) return e->fail(E2ETTS_ESTATE, "no denoiser bases loaded (e2etts_denoiser_load)");
  if (!e->dn.have_bias) return e->fail(E2ETTS_ESTATE, "no denoiser bias spectrum (e2etts_denoiser_set_bias / e2etts_denoiser_calibrate)");
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
