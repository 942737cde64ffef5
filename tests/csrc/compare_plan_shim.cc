// e2e_tts_amd/csrc/compare/plan.h behind a C ABI, for tests/compare_ref.py: the float64 restatement takes the band predicate and the
// back-pointer index from the one place they live in, by building this file with g++ into a shared library.
#include "../../e2e_tts_amd/csrc/compare/plan.h"

namespace pl = e2ecmp_plan;

extern "C" {

// out [Ta, Tb]: 1 where the cell is allowed
void e2ecmp_shim_band_mask(long long Ta, long long Tb, long long band, unsigned char* out) {
  for (long long i = 0; i < Ta; ++i)
    for (long long j = 0; j < Tb; ++j) out[i * Tb + j] = pl::band_allows(i, j, Ta, Tb, band) ? 1 : 0;
}

int e2ecmp_shim_swapped(long long Ta, long long Tb) { return pl::swapped(Ta, Tb) ? 1 : 0; }
long long e2ecmp_shim_bp_words(long long Ta, long long Tb) { return pl::bp_words(Ta, Tb); }
int e2ecmp_shim_max_t(void) { return pl::MAX_T; }
}
