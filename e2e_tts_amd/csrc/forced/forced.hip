// libe2etts_forced.so: the entry points of include/e2etts_forced.h.  The pass itself lives in engine_acoustic.hip (acoustic_impl's forced plan) and
// teacher.hip; this file only gives it exported names, because the main library's set of exports is frozen.  Linked with the engine
// objects and every kernel object of the main library.
#include "../forced_entry.h"

#ifndef E2EFORCED_SRC_HASH
#define E2EFORCED_SRC_HASH "unknown"
#endif

extern "C" {

const char* e2etts_forced_version(void) { return "e2etts-forced 1 E2EFORCED_SRC_HASH=" E2EFORCED_SRC_HASH; }
int e2etts_forced_abi_version(void) { return E2ETTS_FORCED_ABI_VERSION; }
const char* e2etts_forced_engine_version(void) { return e2etts::engine_version(); }

int e2etts_acoustic_forced(e2etts_engine* engine, const int64_t* ids, const int64_t* lens, int B, int L, const int64_t* speaker, int n_spk_ids,
                           const float* d_control, int n_d, const float* p_control, int n_p, const float* e_control, int n_e,
                           const e2etts_forced* forced, float* dur_out, int64_t* mel_lens_out, int* T_out, int32_t* pitch_idx_out,
                           int32_t* energy_idx_out, float* log_dur_out, float* pitch_pred_out, float* energy_pred_out) {
  return e2etts::acoustic_forced_entry(engine, ids, lens, B, L, speaker, n_spk_ids, d_control, n_d, p_control, n_p, e_control, n_e, forced, dur_out,
                                       mel_lens_out, T_out, pitch_idx_out, energy_idx_out, log_dur_out, pitch_pred_out, energy_pred_out);
}

}  // extern "C"
