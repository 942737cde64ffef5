// What engine.hip hands to csrc/forced/forced.hip, the source of the companion library libe2etts_forced.so (include/e2etts_forced.h): the
// teacher-forced pass as a C++ function with hidden visibility.  The main library links it too and exports nothing of it.
#pragma once
#include <stdint.h>

#include "../../include/e2etts_forced.h"

namespace e2etts {
const char* engine_version();   // e2etts_version() of this engine object
int acoustic_forced_entry(e2etts_engine* e, const int64_t* ids, const int64_t* lens, int B, int L, const int64_t* speaker, int n_spk_ids,
                          const float* d_control, int n_d, const float* p_control, int n_p, const float* e_control, int n_e,
                          const e2etts_forced* forced, float* dur_out, int64_t* mel_lens_out, int* T_out, int32_t* pitch_idx_out,
                          int32_t* energy_idx_out, float* log_dur_out, float* pitch_pred_out, float* energy_pred_out);
}  // namespace e2etts
