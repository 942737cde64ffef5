// Stand-alone program around the HIP-free checks of e2etts_acoustic_forced (e2e_tts_amd/csrc/host_logic.h: forced_check, forced_is_null),
// built with g++ -fsanitize=address,undefined by tests/test_forced_host.py and run as a program of its own.  engine.hip includes the same
// header, so this is the code the library ships.  Usage: forced_logic_test <case> -- prints "OK" or "ERR <message>" for one named case;
// "list" prints the case names.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../e2e_tts_amd/csrc/host_logic.h"

using namespace e2etts;

namespace {

struct Case {
  e2etts_forced f;
  ForcedShape s;
  uint32_t size;
  std::vector<float> dur;
  std::vector<int64_t> mel_lens, lens;
  bool dur_host = true, mel_host = true;
};

// B = 2, L = 4, T = 10 on a tiny model (max_seq_len 60, 4096 position rows): a valid soft call with every target frame-resolved
Case base() {
  Case c;
  memset(&c.f, 0, sizeof c.f);
  c.size = sizeof(e2etts_forced);
  c.f.struct_size = c.size;
  c.s.B = 2; c.s.L = 4; c.s.max_seq_len = 60; c.s.pos_table_rows = 4096; c.s.var_pos_rows = 4097;
  c.dur = {3, 2, 4, 1, 5, 5, 0, 0};
  c.mel_lens = {10, 10};
  c.lens = {4, 2};
  static float dummy[2 * 10 * 4];
  c.f.T = 10;
  c.f.attn_soft = dummy;
  c.f.f0 = dummy; c.f.uv = dummy; c.f.energy = dummy;
  c.f.pitch_frames = c.f.energy_frames = 1;
  return c;
}

std::string run(Case& c) {
  c.f.durations = c.f.durations ? c.dur.data() : nullptr;
  c.f.mel_lens = c.f.mel_lens ? c.mel_lens.data() : nullptr;
  return forced_check(c.size, c.f, c.s, c.f.durations && c.dur_host ? c.dur.data() : nullptr, c.f.mel_lens && c.mel_host ? c.mel_lens.data() : nullptr,
                      c.lens.data());
}

const char* NAMES[] = {"valid", "valid_hard", "valid_device_arrays", "null", "size", "size_zero", "nouv_with_f0", "uv_with_pitch", "f0_without_uv",
                       "frames_without_durations", "attn_without_T", "attn_without_mel_lens", "mel_lens_without_attn", "mel_len_zero", "mel_len_past_T",
                       "T_past_position_table", "T_past_var_table", "T_huge", "T_negative", "dur_negative", "dur_fraction", "dur_nan", "dur_inf", "dur_sum_past_T",
                       "dur_padding_ignored_in_sum", "flag_bad", "bt_target_without_T"};

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string name = argv[1];
  if (name == "list") {
    for (const char* n : NAMES) printf("%s\n", n);
    return 0;
  }
  Case c = base();
  static float one;
  static int64_t one64;
  c.f.durations = &one;     // "given": run() points them at the case's arrays
  c.f.mel_lens = &one64;
  if (name == "valid") {
  } else if (name == "valid_hard") { c.f.attn_soft = nullptr; c.f.mel_lens = nullptr;
  } else if (name == "valid_device_arrays") { c.dur_host = c.mel_host = false; c.dur = {-1, 0.5f, std::numeric_limits<float>::quiet_NaN(), 1, 1, 1, 1, 1}; c.mel_lens = {0, 99};
  } else if (name == "null") {
    memset(&c.f, 0, sizeof c.f);
    c.f.struct_size = c.size; c.f.T = 7; c.f.pitch_frames = 1;   // scalars do not make a struct non-null
    printf("%s\n", forced_is_null(c.f) && run(c).empty() ? "OK null" : "ERR not null");
    Case d = base();
    printf("%s\n", !forced_is_null(d.f) ? "OK non-null" : "ERR null");
    return 0;
  } else if (name == "size") { c.size = sizeof(e2etts_forced) + 8;
  } else if (name == "size_zero") { c.size = 0;
  } else if (name == "nouv_with_f0") { c.s.pitch_no_uv = 1;
  } else if (name == "uv_with_pitch") { c.f.pitch = c.f.f0; c.f.f0 = c.f.uv = nullptr;
  } else if (name == "f0_without_uv") { c.f.uv = nullptr;
  } else if (name == "frames_without_durations") { c.f.durations = nullptr;
  } else if (name == "attn_without_T") { c.f.T = 0; c.f.f0 = c.f.uv = c.f.energy = nullptr;
  } else if (name == "attn_without_mel_lens") { c.f.mel_lens = nullptr;
  } else if (name == "mel_lens_without_attn") { c.f.attn_soft = nullptr;
  } else if (name == "mel_len_zero") { c.mel_lens = {10, 0};
  } else if (name == "mel_len_past_T") { c.mel_lens = {11, 10};
  } else if (name == "T_past_position_table") { c.f.T = 4097; c.mel_lens = {4097, 4097};
  } else if (name == "T_past_var_table") { c.s.pitch_frame = 1; c.s.var_pos_rows = 10;
  } else if (name == "T_huge") { c.f.T = (1 << 20) + 1; c.s.pos_table_rows = 1 << 30;
  } else if (name == "T_negative") { c.f.T = -3;
  } else if (name == "dur_negative") { c.dur[2] = -1.f;
  } else if (name == "dur_fraction") { c.dur[5] = 2.5f;
  } else if (name == "dur_nan") { c.dur[0] = std::numeric_limits<float>::quiet_NaN();
  } else if (name == "dur_inf") { c.dur[7] = std::numeric_limits<float>::infinity();
  } else if (name == "dur_sum_past_T") { c.dur[3] = 2.f;
  } else if (name == "dur_padding_ignored_in_sum") { c.dur[6] = 9.f;   // row 1 has 2 phonemes: slot 2 is padding
  } else if (name == "flag_bad") { c.f.energy_frames = 2;
  } else if (name == "bt_target_without_T") { c.f.attn_soft = nullptr; c.f.mel_lens = nullptr; c.f.T = 0;
  } else {
    fprintf(stderr, "unknown case %s\n", name.c_str());
    return 2;
  }
  const std::string m = run(c);
  printf("%s\n", m.empty() ? "OK" : ("ERR " + m).c_str());
  return 0;
}
