// Which attention kernel a launch runs: decided here and nowhere else.  attention_launch() (attention.hip) asks attention_plan() once per launch and
// dispatches on the answer; the host-only entry gill_attention_plan (tests/test_attention_inst_host.py) asks the same function.  No kernel and no HIP call
// behind this header.
#pragma once
#include "ops.h"
#include <stdlib.h>

// GILL_ATT_DMA=0: the register-staged kernel everywhere (A/B switch).  Read once per process; attention_plan() itself takes the value.
inline bool attention_env_dma() {
  static const bool on = [] { const char* e = getenv("GILL_ATT_DMA"); return !(e && e[0] == '0'); }();
  return on;
}

enum { ATT_FAMILY_REG = 0, ATT_FAMILY_DMA = 1 };   // attention_kernel<DP, NTHR> (register-staged) | attention_dma_kernel<DP, NTHR> (LDS-DMA)

// All int: a row of gill_attention_plan.
struct AttnPlan {
  int family;      // ATT_FAMILY_*
  int dp;          // template argument DP: 48 | 64 | 80 | 128 | 160 (0: unsupported padded head dim, nothing is launched)
  int nthr;        // template argument NTHR: 256 | 512 threads per workgroup = 128 | 256 queries
  int grid;        // workgroups: (XCD, pair slot, query tile), see the kernels' map
};

inline AttnPlan attention_plan(const AttnArgs& a, bool att_dma) {
  AttnPlan p = {ATT_FAMILY_REG, 0, 0, 0};
  if (a.dp != 48 && a.dp != 64 && a.dp != 80 && a.dp != 128 && a.dp != 160) return p;
  p.dp = a.dp;
  // 256 queries per workgroup when that still gives every CU a workgroup (measured: level 1, 256 workgroups, is 2 % faster
  // this way; level 2, 64 workgroups, 15-22 % faster with 128-query workgroups); shorter query ranges (UNet levels 1-2, OPT, the
  // mapper) get 128-query workgroups instead of leaving most CUs idle (each workgroup stages the whole K/V itself,
  // which is L2-resident at those sizes).  (128-thread workgroups would stage 10+ chunks per thread: spills)
  const int64_t bh = (int64_t)a.H * a.B;
  const bool big = cdiv(a.nq, 256) * bh >= 256;
  p.nthr = big ? 512 : 256;
  // the LDS-DMA kernel: d = 40 in 48, non-causal, whole query tiles, whole 64-key tiles in the allocation
  const bool dma = att_dma && a.dp == 48 && a.d == 40 && !a.causal && a.nq % (p.nthr / 2) == 0 && a.nkv_pad % 64 == 0 && a.dpv >= 64 && a.nkv >= 1;
  p.family = dma ? ATT_FAMILY_DMA : ATT_FAMILY_REG;
  p.grid = 8 * cdiv(a.H * a.B, 8) * (dma ? a.nq / (p.nthr / 2) : cdiv(a.nq, p.nthr / 2));
  return p;
}
