// The host-side plan of one gemm_launch(): which gemm_kernel instantiation runs, on which grid, with which GemmDev integers, and what follows it.
// gemm_plan.hip works it out ONCE per launch from the arguments and an explicit environment; gemm.hip's launcher, the engines' queries
// (gemm_row_planes() ...) and the host-only entry gill_gemm_plan (tests/test_gemm_plan_host.py) read it.  No kernel and no HIP call behind this header.
#pragma once
#include "ops.h"

#define GEMM_BK 64        // K elements per K step (gemm.hip's BK)
#define GEMM_ZERO_PAGE_STEPS 127

// What a plan depends on besides the arguments.  gemm_env_default() (gemm.hip) reads the process-wide getters: GILL_GEMM_PP, GILL_GEMM_COOP (both
// read once) and the CU count of the first device a GEMM ran on.
struct GemmEnv {
  int pp;        // GILL_GEMM_PP != 0: ping-pong tiles for the convolutions, the short-K plain GEMMs and the QKV GEMMs
  int coop;      // GILL_GEMM_COOP (gemm_coop_mode())
  int cus;       // compute units: the co-residency bound of the in-kernel finish
};
GemmEnv gemm_env_default();

// All int, in the order gill_gemm_plan writes them after the return code (include/gill_amd.h).
struct GemmPlan {
  int k_nwv, k_bn, k_conv, k_epi, k_stages, k_kt, k_mi;      // gemm_kernel<NWV, BN, CONV, EPI, STAGES, KT, MI>
  int grid_x, grid_y, grid_z;                                // tiles_m * groups_n, splitk, ncls
  // GemmDev, the non-pointer fields (nwv / mi are what the KERNEL BODY reads for its tile -> workgroup map, not always the template pair: the
  // eight-wave 128 x 128 GEGLU / QKV kernel runs under nwv = 4, mi = 4)
  int ksteps, ksteps_per_split, tiles_m, tiles_n, npw, groups_n, nwv, mi, kt, n_major, xb_m, xb_n;
  int M, rows_per_batch;                                     // the kernel's row space (UPS4: one parity class)
  int tile_rows, ncls, splitk;                               // rows of an M tile; parity classes in blockIdx.z; the effective split (>= 1)
  int coop;                                                  // GroupNorm finish inside this launch (EPI 6)
  int reduce, reduce_M;                                      // the split-K reducer launch follows, over reduce_M output rows (the OUTPUT tensor's)
  int row_planes, gn_slab_rows, coop_counters;               // gemm_row_planes() / gemm_gn_slab_rows() / gemm_coop_counters()
};
#define GEMM_PLAN_INTS 33
static_assert(sizeof(GemmPlan) == GEMM_PLAN_INTS * sizeof(int), "GemmPlan is a row of ints");

// The tile choice and everything derived from it, for any arguments (pure, cannot fail; an empty problem gives the zero plan).
void gemm_plan_fill(const GemmArgs& a, const GemmEnv& env, GemmPlan* p);
// gemm_launch()'s argument checks, then the plan.  A refused launch (non-zero return, gill_last_error) has no plan.
int gemm_plan(const GemmArgs& a, const GemmEnv& env, GemmPlan* p);

// What gemm_launch() ran: the plans of this thread's GEMM_PLAN_LOG_CAP most recent successful dispatches and the launches since the record was last
// read (gemm.hip; host only, one struct copy per launch).  gemm_plan_log_take() writes the most recent min(cap, GEMM_PLAN_LOG_CAP, launched) plans,
// oldest first, returns how many it wrote, sets *launched and clears the record.  For tests (gill_gemm_plan_log): an operator entry picks split
// factors, blocked weights and per-sample operands itself, so only the launcher knows which instantiation an operator call executed.
#define GEMM_PLAN_LOG_CAP 32
int gemm_plan_log_take(GemmPlan* out, int cap, int* launched);

// the engines' pre-launch choices under an explicit environment (ops.h declares the process-wide forms)
int gemm_pick_splitk_env(const GemmEnv& env, int M, int N, int K, int act, bool plain, bool generic);
int gemm_pick_splitk_blk64_env(const GemmEnv& env, int M, int N, int K);
bool gemm_conv_pingpong_env(const GemmEnv& env, int rows_multiple_of, int Cout);
bool conv_k_chunked_env(const GemmEnv& env, int HW, int Cin, int Cout);
