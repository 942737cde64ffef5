// tuning(): the one reader of the tuning switches (tuning.h).  Compiled twice, like engine.hip: the product object returns the defaults
// and names no variable; the test build (-DE2ETTS_TEST_HOOKS) fills the table from the environment, once.  Every switch selects a path
// that gives the same bits as the default one, and a test runs a child process with it set.
#include "tuning.h"
#ifdef E2ETTS_TEST_HOOKS
#include <stdlib.h>
#endif

namespace e2etts {

const Tuning& tuning() {
  static const Tuning table = [] {
    Tuning t;
#ifdef E2ETTS_TEST_HOOKS
    auto num = [](const char* name, long long unset) { const char* v = getenv(name); return v ? atoll(v) : unset; };   // NAME=n
    auto on = [&](const char* name) { return num(name, 1) != 0; };                                                      // NAME=0: off
    // conv_gemm.hip
    t.wg_per_cu = (int)num("E2ETTS_WG_PER_CU", t.wg_per_cu);   // =n: row groups per CU that conv_gemm sizes its persistent workgroups for
    t.frag64 = on("E2ETTS_FRAG64");                            // =0: the 64 x 64 few-rows tile on the LDS weight tile, not on fragments
    // engine_weights.hip, engine_core.hip, engine_vocoder.hip
    t.frag32 = getenv("E2ETTS_NO_FRAG32") == nullptr;          // set at all: fp32 weights through the LDS tile (A/B against the fragments)
    t.rows = on("E2ETTS_ROWS");                                // =0: few-rows convolutions on conv_gemm's 64 x 64 tile instead of conv_rows
    t.bconv = on("E2ETTS_BCONV");                              // =0: plain-bf16 convolutions stay on conv_gemm's mode 2
    t.voc_conc_frames = num("E2ETTS_VOC_CONC_FRAMES", -1);     // =n: most frames per call whose ResBlocks run side by side (unset: 2 048; 4 096 in fp32)
    t.voc_group = on("E2ETTS_VOC_GROUP");                      // =0: side streams where plain bf16 groups a stage's ResBlocks into one launch
    t.voc_defer_join = on("E2ETTS_VOC_DEFER_JOIN");            // =0: a grouped stage's join as a launch of its own
    // attention.hip
    t.att_split_max = num("E2ETTS_ATT_SPLIT_MAX", -1);         // =n: largest grid (64-query workgroups) on the split kernels (0: never)
    t.att_par = on("E2ETTS_ATT_PAR");                          // =0: fp32 attention never computes its key segments in parallel workgroups
    // small_kernels.hip
    t.dwglu = on("E2ETTS_DWGLU");                              // =0: the Conformer's GLU and depthwise convolution as two kernels
    // conv_bf16.hip
    t.bpair = on("E2ETTS_BPAIR");                              // =0: no pair_bf16: ResBlock pairs stay on resblock_pair.hip
    t.brb = on("E2ETTS_BRB");                                  // =0: no rb_bf16: whole ResBlocks and stages stay pair launches
#endif
    return t;
  }();
  return table;
}

}  // namespace e2etts
