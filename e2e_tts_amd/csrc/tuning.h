// The tuning switches: every one selects between paths that give the same bits, so a test can run a child process on the other path and
// compare.  Only the test build (-DE2ETTS_TEST_HOOKS) reads them from the environment; the product library runs on the defaults below
// whatever its environment holds.  Names and meanings: the table in tuning.hip.
#pragma once

namespace e2etts {

struct Tuning {
  int wg_per_cu = 24;
  bool frag64 = true;
  bool frag32 = true;
  bool rows = true;
  long long att_split_max = -1;
  bool att_par = true;
  bool dwglu = true;
  long long voc_conc_frames = -1;
  bool bconv = true;
  bool bpair = true;
  bool brb = true;
  bool voc_group = true;
  bool voc_defer_join = true;
};

const Tuning& tuning();

}  // namespace e2etts
