// The plan of one gemm_launch() (gemm_plan.h): every host-side decision about a GEMM / convolution launch — tile width, tile rows, waves, ring depth,
// epilogue, N tiles per workgroup, XCD map, in-kernel finish, reducer — made here, once, from the arguments and an explicit GemmEnv.
// Host code only: no kernel, no HIP call.  Each rule is written in ONE function; the measurement comments are the record of why a rule exists and
// stay with it.  tests/test_gemm_plan_host.py pins every decision against a recording of the launcher this file replaced (profiles/gemm_plan_isa.md).
#include "gemm_plan.h"
#include "gemm_dev.h"

#define BK GEMM_BK
#define BM_HOST 128       // rows of the 4-wave tile, for the host-side split-K heuristic; the kernel's BM is 32 * NWV

// ---- the rules that several decisions share -----------------------------------------------------------------------------------------------------

// The 160 / 128 width rule.  Measured on MI355X (profiles/r01_sweep_gemm_tiles.md): the 128x160 tile (5 N sub-tiles per wave: more MFMAs per LDS
// byte) beats 128x128 by 15-40 % on every UNet width, all of which are multiples of 160
static inline int width_160_or_128(int N) { return (N % 160 == 0) ? 160 : 128; }

// The 64-row-tile rule: plain GEMMs whose 128-row tiling leaves CUs without a tile (fewer than 300 tiles, more than one 64-row tile of rows).
// `tiles_n` is the caller's count of N tiles, and the callers do NOT all count at the same width — see plan_tile_width() and plan_waves().
// (measured: < 300 +0.3 %, < 520 -3 % end to end; re-measured with the 3-deep ring of the four-wave 64-row tile: < 300 493.8 ms, < 400 495.6,
// < 520 496.3, < 700 496.5)
static inline bool few_tiles_64row(int M, int tiles_n) { return (int64_t)cdiv(M, 128) * tiles_n < 300 && M > 64; }

// The 128 / 256 ping-pong row rule (160-wide eight-wave tiles; N % 160 == 0, M % 128 == 0).  Where the 256-row tiling x split-K gives at most 128
// workgroups (UNet levels 1-3 at the 8-sample batch), run 128 x 160 ping-pong tiles (eight waves of 32 x 80); gemm_pick_splitk() then aims at 256
// workgroups of those, i.e. half the split factor: half the fp32 partials (none at level 1) (loop 561.1 -> 558.0 ms).  Rows that 256 does not
// divide (plain GEMMs only: the convolutions' rows are multiples of 256, gemm_conv_pingpong()) take the 128-row tile as well.
static inline int pingpong_tile_rows(int M, int N, int sk, int ncls) {
  return ((int64_t)cdiv(M, 256) * ncls * (N / 160) * sk <= 128 || M % 256 != 0) ? 128 : 256;
}

// The "one balanced round" window: from K = 640 up, `wg` ping-pong workgroups that are ONE full round, one per CU — with ten K steps a second,
// partial round costs more than the tile gains.  (Round 6: proj_in / attn1.to_out of level 1 at the CFG batch 8, 8192 x 640 x 640: 256 ping-pong
// workgroups instead of 320 four-wave 128 x 128 tiles of which 64 CUs get two; 17.4 -> 14.3 us stand-alone, tools/pp_shortk_probe.py.  Fewer tiles
// than CUs (2048 x 1280 x 1280: 16.4 -> 18.3 us) and K = 320 (level 0: +-0) stay on the general tiles.)
static inline bool one_balanced_round(const GemmEnv& env, int K, int64_t wg) { return env.pp != 0 && K >= 640 && wg >= 200 && wg <= 256; }

// Long-K plain GEMMs whose width tiles by 160 (the feed-forward output GEMMs of UNet levels 1-3: K = 5 C) run on the convolutions'
// ping-pong kernel too: their 64 x 160 / 128 x 160 four-wave tiles fetch 22 / 14 KiB per MFLOP through a 64 B/clk L2 port, the 8-wave
// tiles 14 / 10 (round 4 A/B: 57 -> 43 us at level 1, loop -0.5 %)
// ... and the short-K ones of one_balanced_round(), counted in the tiles pingpong_tile_rows() gives them unsplit.
// GILL_GEMM_PP = 0 (A/B switch, read once): no ping-pong tiles for the convolutions, the short-K plain GEMMs and the QKV GEMMs (the long-K plain
// GEMMs keep them)
static bool plain_pingpong(const GemmEnv& env, int M, int N, int K) {
  if (N % 160 != 0 || M % 128 != 0 || K % 64 != 0) return false;
  if (K >= 2560) return true;
  return one_balanced_round(env, K, (int64_t)(M / pingpong_tile_rows(M, N, 1, 1)) * (N / 160));
}
// ... and the launch's other conditions (the width rule and the wave rule used to test different things): the 8-wave plain kernel has
// the lean bf16 row-major epilogue only
// (per-sample weights — GemmArgs::wb_rows, the cross-attention values GEMM — where samples are whole 256-row tiles: round 6, loop 441.8 -> 440.0 ms)
static bool plain_pingpong_args(const GemmEnv& env, const GemmArgs& a) {
  return !a.conv && plain_pingpong(env, a.M, a.N, a.K) && a.act == ACT_NONE && a.out_mode == OUT_BF16 && !a.resid_f32 && a.wb_rows % 256 == 0 && !a.ln_stats;
}

// QKV GEMMs (head-major scatter epilogue, folded LayerNorm) on the 256 x 160 ping-pong tiles where those give a balanced round of one workgroup per CU
// (round 6): the workgroups fill >= 75 % of their last round of 256, and 128-row tiles would not fill theirs better.  Level 2 at the CFG batch 8
// (2048 x 3840 x 1280: 192 workgroups) 52.5 -> 38.5 us per launch, loop -0.9 %.  Returns the wave M sub-tile count (4) or 0.
// (Measured with it and not kept: the 128-row tiles where THEY are the balanced choice — level 1, 8192 x 1920 x 640, 768 workgroups = three rounds:
// 46.9 -> 42.7 us per launch, and the loop gains nothing because the card then clocks 15 MHz lower, three boxes, profiles/r06_skeleton_ab.log.
// Round 4 had these GEMMs on 128-wide ping-pong tiles at every level and lost 0.6-1 %: K = 320 at level 0 and the 1.5-round grids were in it.)
static int qkv_pingpong_mi(const GemmEnv& env, const GemmArgs& a) {
  if (!env.pp || a.conv || a.out_mode != OUT_QKV || a.N % 160 != 0 || a.M % 256 != 0 || a.K % 64 != 0 || a.K < 640 || a.splitk > 1 || a.wb_rows || a.w_blk64) return 0;
  auto fill = [](int64_t wg) { return (double)wg / (double)(((wg + 255) / 256) * 256); };
  const double f128 = fill((int64_t)(a.M / 128) * (a.N / 160)), f256 = fill((int64_t)(a.M / 256) * (a.N / 160));
  // ONE round only: several rounds of these tiles (level 1 at UNet batch 16: 768 workgroups) make the kernel faster and the card clock lower, like the
  // 128-row form at batch 8 — loop 764.6 ms without, 767.3 ms with, 15-35 MHz apart (profiles/r06_skeleton_ab.log, session r06_s33)
  if ((int64_t)(a.M / 256) * (a.N / 160) > 256) return 0;
  return (f256 >= 0.75 && f256 >= f128) ? 4 : 0;
}

// 3x3 convolutions whose row count is a multiple of 256 and whose width tiles by 160 run on the 256 x 160 ping-pong kernel
// (GILL_GEMM_PP = 0: two co-resident 128 x 160 workgroups instead, the round-1 structure)
// (round 4: 256 x 128 ping-pong tiles for the widths 160 does not divide — the VAE decoder's 128 / 256 / 512-channel convolutions: 484.8 /
// 403.2 / 303.9 us against 464.8 / 406.1 / 301.0 us on the four-wave 128 x 128 tiles, VAE decode 12.74 vs 12.69 ms.  Not kept.)
bool gemm_conv_pingpong_env(const GemmEnv& env, int rows_multiple_of, int Cout) {
  return env.pp != 0 && rows_multiple_of % 256 == 0 && Cout % 160 == 0;
}
bool gemm_conv_pingpong(int rows_multiple_of, int Cout) { return gemm_conv_pingpong_env(gemm_env_default(), rows_multiple_of, Cout); }

bool conv_k_chunked_env(const GemmEnv& env, int HW, int Cin, int Cout) {
  return HW >= 4096 && (int64_t)HW * Cin * 2 > (int64_t)4 << 20 && !gemm_conv_pingpong_env(env, HW, Cout);
}
bool conv_k_chunked(int HW, int Cin, int Cout) { return conv_k_chunked_env(gemm_env_default(), HW, Cin, Cout); }

bool gemm_fused_gn_ok(int N, int cg) {
  if (cg < 1 || N % cg != 0 || N / cg > 64) return false;
  const int bn = width_160_or_128(N);
  // in-kernel epilogue: bins must not straddle N tiles; split-K reducer: nor its 64- or 80-column blocks
  return bn % cg == 0 && (64 % cg == 0 || (80 % cg == 0 && N % 80 == 0));
}

// ---- the split factor, chosen by the engines BEFORE the launch (the plan depends on it) ------------------------------------------------------------

// STREAM64.  Weight-streaming GEMMs (a few hundred rows against 33-134 MB matrices: OPT-6.7b at <= 8 prompts) ran at 2.2-3 TB/s of weights on
// the general tiles, whatever the ring depth (profiles/r05_opt_stream64.md: 128 x 64 tiles with a 6-deep ring streamed no faster than 64 x 128
// tiles with a 3-deep one): a K step fetched 64-128 weight ROWS of 128 B each at a stride of 2 K bytes, i.e. one DRAM page activation per 128 B.
// STREAM64 changes the layout, not only the tile: the matrix is stored at load time as [N / 64][K / 64][64][64] (gemm_stream64_weights() says
// which matrices; convert_to_bf16_blk64_launch() writes them), so the 128 x 64 tile's weight stage is one contiguous 8 KiB run, a workgroup's
// whole K walk one contiguous K * 128 B stream, fetched with the non-temporal policy (MI355X_MICROARCH "nt-weights") into a 6-deep ring
// (144 KiB, one workgroup of eight waves per CU, 40 KiB of weights + 80 KiB of L2-resident activations in flight per CU).  All rows of a <= 128-row problem
// sit in the one M tile (every weight is read once); more rows = more M tiles next to each other on one XCD (n_major), sharing the L2.
// No split for >= 160 workgroups; narrower matrices split K to ~256 workgroups.  (The A/B switch of round 5 is gone: row-major weights on the general
// tiles measured 5.95-6.08 ms for the OPT stage against 4.31 ms, profiles/r05_opt_stream64.md.)
bool gemm_stream64_weights(int N, int K) {
  return N % 64 == 0 && K % 64 == 0 && K >= 1024 && (int64_t)N * K >= ((int64_t)4 << 20);
}
int gemm_pick_splitk_blk64_env(const GemmEnv& env, int M, int N, int K) {
  if (M > GEMM_STREAM64_MAX_ROWS) return gemm_pick_splitk_env(env, M, N, K, ACT_NONE, false, false);     // (runs on the general tiles: plan_general())
  const int tiles = cdiv(M, 128) * (N / 64), ksteps = K / BK;
  if (tiles >= 160) return 1;
  int s = (256 + tiles / 2) / tiles;
  while (s > 1 && ksteps / s < 8) --s;
  if (s > 16) s = 16;
  // no empty trailing split (ksteps = 129, s = 16 -> 9 steps per split, split 15 would start past the end and write a zero plane)
  return cdiv(ksteps, cdiv(ksteps, s));
}
int gemm_pick_splitk_blk64(int M, int N, int K) { return gemm_pick_splitk_blk64_env(gemm_env_default(), M, N, K); }

int gemm_pick_splitk_env(const GemmEnv& env, int M, int N, int K, int act, bool plain, bool generic) {
  if (act == ACT_GEGLU) return 1;
  const int bn = width_160_or_128(N);
  const int tiles = cdiv(M, BM_HOST) * cdiv(N, bn);
  const int ksteps = K / BK;
  if (tiles >= 384 || ksteps < 8) return 1;
  {   // convs (and plain GEMMs) the plan puts on 128 x 160 ping-pong tiles: one workgroup per CU, 256 slots
    if (!generic && (plain ? plain_pingpong(env, M, N, K) : gemm_conv_pingpong_env(env, M, N)) && tiles <= 256 && M % 128 == 0) {
      int s = (256 + tiles / 2) / tiles;
      const int min_steps = (M <= 256 || tiles < 64) ? 4 : 24;
      if (s > ksteps / min_steps) s = ksteps / min_steps;
      if (s > 16) s = 16;
      return s < 1 ? 1 : s;
    }
  }
  // (round 5, first session: an M-dependent rule for skinny weight-streaming GEMMs lived here.  The OPT matrices now take gemm_pick_splitk_blk64();
  // for everything else it made the split factor — the fp32 summation order — depend on the batch, and the tiny UNet's batch-invariance check went
  // from bit-identical to 2.4e-2 after 11 recurrent calls.  Removed.)
  // plain GEMMs with 150..299 128-row tiles run on 64-row tiles instead (few_tiles_64row: >= 300 workgroups, no partials):
  // measured 8192 x 640 x 3200 unsplit 49.1 us, two-way split + reducer 54.6 us
  if (plain && !generic && tiles >= 150 && few_tiles_64row(M, cdiv(N, bn))) return 1;
  int s = (512 + tiles / 2) / tiles;   // aim for ~2 workgroups per CU (512 resident slots)
  // each split pays an fp32 partial write + a reduce pass: keep >= 24 K steps per split (measured: K = 1280 GEMMs lose
  // from any split, K >= 5120 convs win up to 4-8 ways), except for skinny weight-streaming GEMMs (OPT, M <= 256)
  // where filling every CU with HBM requests matters more than the tiny partials
  const int min_steps = (M <= 256 || tiles < 64) ? 4 : 24;
  if (s > ksteps / min_steps) s = ksteps / min_steps;
  if (s > 16) s = 16;
  if (s < 1) s = 1;
  return s;
}
int gemm_pick_splitk(int M, int N, int K, int act, bool plain, bool generic) { return gemm_pick_splitk_env(gemm_env_default(), M, N, K, act, plain, generic); }

// ---- the plan ------------------------------------------------------------------------------------------------------------------------------------

// Tile width.  Tried and removed (numbers in profiles/r02_big_tile.md, profiles/r01_sweep_gemm_tiles.md): a 256 x 256 8-wave tile for
// the wide plain GEMMs (GEGLU 94 -> 100 us, QKV 46.6 -> 48.3 us: those kernels are bound by their epilogues), a 4-deep ring of
// 32-wide K stages (+7 % on the loop), a 3-deep ring on the 4-wave tiles.
static int plan_tile_width(const GemmArgs& a, int qkv_mi, bool plain_pp) {
  if (a.act == ACT_GEGLU) return 128;
  int bn = width_160_or_128(a.N);
  // ... except for the head-major scatter epilogue (QKV / to_q), whose columns fall into 48..160-wide heads: 128-wide tiles
  // measured 579.3 -> 576.3 ms on the loop
  if (!a.conv && a.out_mode == OUT_QKV && a.N % 128 == 0 && !qkv_mi) bn = 128;
  // ... and except on the 64-row tile (plain GEMMs with few tiles): 64 x 128 needs 48 KiB of LDS, i.e. three
  // workgroups (six waves) per CU instead of two (four) — loop 587.3 -> 584.7 ms
  // (this rule counts 128 x 160 tiles when it hands these GEMMs BN = 128, plan_waves() then counts 128 x 128 tiles: an 8192 x 640 GEMM
  // — 256 vs 320 — therefore lands on the 4-wave 128 x 128 tile, not the 64-row one; measured better that way: 567.8 vs 575.5 ms.  Deliberate.)
  if (!a.conv && a.splitk <= 1 && a.N % 128 == 0 && !a.gn_stats && few_tiles_64row(a.M, cdiv(a.N, 160)) && a.out_mode != OUT_SOFTMAX80 && !plain_pp) bn = 128;
  return bn;
}

// Waves per workgroup and 16-row M sub-tiles per wave, as the kernel body reads them (GemmDev::nwv / mi): tile rows = (nwv / 2) * mi * 16.
static void plan_waves(const GemmArgs& a, const GemmEnv& env, int bn, int sk, int Mk, int ncls, int tiles_n, int qkv_mi, bool plain_pp, int* nwv_out, int* mi_out) {
  // 64-row tiles for plain GEMMs whose 128-row tiling leaves CUs without a tile (counted at THIS launch's width: see plan_tile_width())
  int nwv = 4, mi = 4;
  if (!a.conv && sk == 1 && few_tiles_64row(a.M, tiles_n)) nwv = 2;
  if (a.wb_rows % 128 != 0 && !a.conv && sk == 1) nwv = 2;      // per-sample weights on samples of 64 rows (GemmArgs::wb_rows): 64-row tiles
  // the 64-row tile on FOUR waves (2 x 2, wave tile 32 x 64) where its width is 128: same LDS, twice the waves per CU —
  // loop 580.4 -> 576.3 ms, 2048 x 1280 x 1280 19.8 -> 17.3 us
  if (nwv == 2 && bn == 128 && a.act != ACT_GEGLU && !a.gn_stats) { nwv = 4; mi = 2; }
  // ... and where it is 160 (the feed-forward output GEMMs of levels 1-3 with their fused GroupNorm partials: bins of 20 / 40 channels
  // need the 160-wide tile): loop 492.4 -> 489.4 ms against the two-wave tile.
  if (nwv == 2 && bn == 160 && a.act == ACT_NONE && a.out_mode == OUT_BF16) { nwv = 4; mi = 2; }
  if (a.out_mode == OUT_SOFTMAX80) { nwv = 4; mi = 2; }      // (see plan_kernel)
  // ... or, where 128-row ping-pong tiles are exactly one balanced round (level 1 at the CFG batch 8: 8192 x 640 x 640 = 256 workgroups instead of 512
  // four-wave ones), those (round 6, like the plain GEMMs of that shape)
  if (bn == 160 && a.out_mode == OUT_SOFTMAX80 && sk == 1 && a.M % 128 == 0 && a.wb_rows % 128 == 0 && one_balanced_round(env, a.K, (int64_t)(a.M / 128) * tiles_n)) {
    nwv = 8; mi = 2;
  }
  // (round 4: the 64-row four-wave tile with its 3-deep ring — 96 instead of 64 KB in flight per CU — on ALL GEGLU / QKV / 128-wide plain
  // GEMMs, not only the few-tile ones: loop 460.4 -> 469.4 / 464.8 / 460.7 ms.  Not kept.)
  // 3x3 convolutions: 256 x 160 tile with the ping-pong main loop, one workgroup per CU (GILL_GEMM_PP = 0 keeps the two
  // co-resident 128 x 160 workgroups); 128 x 160 where pingpong_tile_rows() says so
  if (bn == 160 && a.conv && gemm_conv_pingpong_env(env, Mk, a.N)) { nwv = 8; mi = pingpong_tile_rows(Mk, a.N, sk, ncls) / 64; }
  if (bn == 160 && plain_pp) { nwv = 8; mi = pingpong_tile_rows(Mk, a.N, sk, 1) / 64; }
  if (bn == 160 && qkv_mi) { nwv = 8; mi = qkv_mi; }
  // (round 4: the short-K GEGLU / QKV GEMMs on 256 x 128 / 128 x 128 ping-pong tiles, one N tile per workgroup: loop 464.0 -> 478.0 / 480.4 ms
  // (GEGLU), 467.0 / 468.8 ms (QKV) — ten K steps do not amortise a prologue and an epilogue that no second workgroup covers.  Not kept.)
  *nwv_out = nwv; *mi_out = mi;
}

// XCD BLOCK MAP.  Model of the fabric traffic of one launch under a map that gives every XCD an xm x xn block of the (M tile, N group) grid (all
// K splits of a tile sit on its XCD: blockIdx.y does not move the XCD when gridDim.x % 8 == 0):
//   activations: the block's rows x the channels a K walk reads, once if they fit next to the streaming weights in the 4 MiB L2 (budget 2 MiB),
//                else once per re-read (a tap-major 3x3 convolution re-reads its input rows 9 times, a plain GEMM once per N tile a workgroup walks);
//   weights:     the block's N columns x K, once (the block's M tiles walk K in step and share the stream).
// Picks the block with the least modelled traffic; the two range maps (n_major / m-major) are candidates like any other, and the block map is only
// used where it beats the range map in force by 15 % (profiles/r06_xcd_block_map.md: level-2 convolutions 417 -> ... MB per dispatch).
static void xcd_block_pick(const GemmArgs& a, GemmPlan& d, int bm_rows, int bn_cols, int ncls) {
  d.xb_m = d.xb_n = 0;
  const int nwg = d.tiles_m * d.groups_n;
  // (the ping-pong tiles only — the 3x3 convolutions and the long-K plain GEMMs of levels 1-3, one workgroup per CU: the launches whose fetch
  // profiles/r05_fetch_by_kernel.md flagged; the model is not trusted on the multi-N-tile walks of the GEGLU / QKV kernels)
  if (ncls != 1 || nwg % 8 != 0 || nwg < 16 || a.wb_rows || d.nwv != 8 || bn_cols != 160) return;
  const double l2_budget = 2.0 * 1024 * 1024;
  const int taps = a.conv ? 9 : 1;
  const double row_bytes = 2.0 * (a.conv ? (double)(a.Cin + a.KX) * (a.stride == 2 ? 4 : 1) : (double)a.K);     // input bytes behind one output row
  const double col_bytes = 2.0 * (double)a.K * bn_cols * d.npw;                                                   // weight bytes of one N group
  auto cost = [&](double xm, double xn) {
    const double A = xm * bm_rows * row_bytes, W = xn * col_bytes;
    // (a plain GEMM's N groups of one M tile run side by side on the XCD and share the activation stream; only a workgroup's own walk over npw N
    // tiles comes back to the same rows later)
    const double rereads = (A <= l2_budget) ? 1.0 : (a.conv ? (a.k_chunked ? 1.0 : (double)taps) : (double)d.npw);
    return A * rereads + W;
  };
  double best = 1e30; int bxm = 0, bxn = 0;
  for (int blocks_m = 1; blocks_m <= 8; blocks_m *= 2) {
    const int blocks_n = 8 / blocks_m;
    if (d.tiles_m % blocks_m != 0 || d.groups_n % blocks_n != 0) continue;
    const int xm = d.tiles_m / blocks_m, xn = d.groups_n / blocks_n;
    const double c = cost(xm, xn);
    if (c < best) { best = c; bxm = xm; bxn = xn; }
  }
  if (bxm == 0) return;
  // the range map in force: n_major = (all of M, 1/8 of N) per XCD, else (1/8 of M, all of N) — priced with the same model
  const double cur = d.n_major ? cost(d.tiles_m, d.groups_n / 8.0) : cost(d.tiles_m / 8.0, d.groups_n);
  if (best <= 0.85 * cur) { d.xb_m = bxm; d.xb_n = bxn; }
}

// ---- COOP (GemmArgs::coop_ctr): which launches may finish in-kernel.  `p` holds the tile of this launch.
// GILL_GEMM_COOP = 0: every finish as its own launch (GroupNorm-apply), the round-5 dataflow (A/B and the on / off parity test);
// anything else (default 1): the GroupNorm finish in the 3x3 convolutions' epilogue (EPI 6).  Split-K GEMMs always finish in the reducer launch
// (the in-kernel form measured slower: profiles/r06_coop_finish.md).
static bool plan_coop(const GemmArgs& a, const GemmEnv& env, const GemmPlan& p) {
  if (!a.coop_ctr || env.coop == 0 || a.splitk > 1) return false;
  // the ping-pong convolution tiles only (upsample forms: parity classes in blockIdx.z / a 9-tap gather — their finish stays a launch)
  if (!a.conv || a.ups || p.nwv != 8 || p.k_bn != 160) return false;
  const int bm = p.tile_rows;
  const int rpb = a.rows_per_batch;
  if (rpb <= 0 || a.M % bm != 0 || a.M % rpb != 0) return false;
  // co-residency: the waiting workgroups must all be on the chip — one per CU (the ping-pong tiles take a CU's whole LDS), so the grid may not
  // exceed the CU count (MI355X: 256; a device with fewer falls back to the launches)
  if ((int64_t)(a.M / bm) * (a.N / 160) > env.cus) return false;
  if (a.out_mode != OUT_BF16 || a.act != ACT_NONE || a.resid_f32 || a.row_stats || a.ln_stats || a.alpha != 1.f || a.wb_rows || a.partials_only || a.w_blk64)
    return false;
  // GroupNorm finish in the convolution's epilogue: whole M tiles per sample, <= 64 slab partials per bin (the apply kernel's own limit),
  // <= 32 bins per N tile, groups made of whole bins inside one N tile
  if ((!a.fn_Y && !a.fn_ss) || !a.fn_gamma || !a.fn_beta) return false;
  if (!a.gn_stats || a.gn_cg <= 0 || 160 % a.gn_cg != 0 || 160 / a.gn_cg > 32 || a.gn_cg * a.gn_groups != a.N) return false;
  if (a.fn_cg <= 0 || a.fn_cg % a.gn_cg != 0 || 160 % a.fn_cg != 0) return false;
  if (rpb % bm != 0 || rpb % GN_SLAB_ROWS != 0 || rpb / GN_SLAB_ROWS > 64) return false;
  return true;
}

// The gemm_kernel instantiation: template waves / sub-tiles (which differ from GemmDev's pair on one kernel) and the depth of the LDS ring.
static void plan_kernel(const GemmArgs& a, GemmPlan& p) {
  p.k_conv = !a.conv ? 0 : (a.ups == 2 ? 3 : (a.ups ? 2 : 1));
  if (p.coop) p.k_epi = 6;
  else if (p.splitk > 1) p.k_epi = 2;
  else if (a.conv) p.k_epi = 0;
  else if (a.act == ACT_GEGLU) p.k_epi = 1;
  else if (a.out_mode == OUT_SOFTMAX80) p.k_epi = 5;
  else if (a.out_mode == OUT_QKV) p.k_epi = 3;
  else p.k_epi = (a.act == ACT_NONE && a.out_mode == OUT_BF16 && !a.resid_f32) ? 4 : 0;
  p.k_kt = BK;
  p.k_nwv = p.nwv; p.k_mi = p.mi; p.k_stages = 2;
  if (p.nwv == 8) {
    p.k_stages = 3;       // the ping-pong tiles, 256 x 160 (mi 4) or 128 x 160 (mi 2): one workgroup per CU
  } else if (p.nwv == 4 && p.mi == 2 && p.k_epi == 5) {
    // 64 x 160 tile on four waves of 32 x 80.  Measured on the three UNet shapes of the 8-sample batch back to back (tools/xalg_bench.py, 20
    // launches each, operands warm): two waves of 64 x 80 1177 us, this with a 2-deep ring 1003-1013 us, 3-deep 1212 us, 3-deep only on
    // the <= 256-workgroup grids 1051 us.  In the UNet forward the per-sample weights are cold (13 MB per layer, read once per call) and
    // a workgroup's K walk is a chain of HBM round trips: there the 3-deep ring on the one-workgroup-per-CU grids (levels 2-3) wins,
    // loop 446.7 -> 444.1 ms (4-deep: 444.7).
    p.k_stages = (p.grid_x * p.grid_y <= 256) ? 3 : 2;
  } else if (p.nwv == 4 && p.mi == 2 && p.k_bn == 128) {
    // 64-row tile on four waves, 3-deep ring (72 KB: two workgroups per CU).  These grids are 1-2 workgroups per CU, so the ring depth IS
    // the number of K stages in flight on a CU, and a K step of these short-K GEMMs is one L2 round trip: 2-deep 487.3 ms, 3-deep
    // 483.4 ms, 4-deep (one workgroup per CU) 496.1 ms on the loop.
    p.k_stages = 3;
  } else if (p.nwv == 4 && p.mi == 2) {
    // 64 x 160 (2-deep ring: 56 KB, two workgroups per CU; 3-deep = 84 KB = one per CU measured slower: 495.7 vs 489.4 ms)
    p.k_stages = 2;
  } else if (p.nwv == 4 && p.k_conv == 0 && p.k_bn == 128 && (p.k_epi == 1 || p.k_epi == 3)) {
    // round 5: the 128 x 128 tile of the GEGLU / QKV GEMMs on eight waves of 32 x 64 (two workgroups = 16 waves per CU, 116 registers) instead of four of
    // 64 x 64: half the LDS-DMA pieces, fragment reads and MFMAs per wave and step, twice the waves to overlap them.  Loop 447.4 -> 445.8 ms (A/B x3,
    // profiles/r05_linears.md); level-1 GEGLU 82.1 -> 79.7 us stand-alone.  The body still maps workgroups to tiles with nwv = 4, mi = 4.
    // (the same for the UNet's plain 128-row GEMMs — the lean row-major epilogue, EPI 4 — measured slower: loop 451.3 -> 456.0 ms, profiles/r05_linears.md)
    p.k_nwv = 8; p.k_mi = 2;
  }
  // (nwv == 2: the 64-row two-wave tile, 2-deep ring; nwv == 4, mi == 4: the 128-row four-wave tile, 2-deep ring, two workgroups per CU)
}

// STREAM64: w_blk64 weights up to GEMM_STREAM64_MAX_ROWS rows on the 128 x 64 streaming tile, 6-deep ring = 144 KiB, one workgroup per CU
// (gemm_stream64_weights() above has the story).
static void plan_stream64(const GemmArgs& a, GemmPlan& p) {
  p.k_bn = 64;
  p.tiles_n = a.N / 64; p.tiles_m = cdiv(a.M, 128); p.npw = 1; p.groups_n = p.tiles_n; p.n_major = 1; p.xb_m = p.xb_n = 0;
  // (round 5: every workgroup starting its K walk (t * 5 | 13 | 29) % steps into its slice, against HBM-channel camping of 256 lockstep streams
  // whose bases are K * 128 B apart: OPT stage 5.18 -> 5.24 ms, profiles/r05_opt_stream64.md.  Not that; removed.)
  // eight waves of 32 x 32 (three LDS-DMA pieces per wave and stage) rather than four of 64 x 32 (six): OPT stage 5.03 -> 4.70 ms — a wave issues its
  // pieces, fragment reads and MFMAs one after the other, and with one workgroup per CU only more waves overlap them
  p.nwv = 8; p.mi = 2; p.tile_rows = 128;
  p.grid_x = p.tiles_n * p.tiles_m;
  p.k_nwv = 8; p.k_conv = 0; p.k_stages = 6; p.k_kt = BK; p.k_mi = 2;
  p.k_epi = p.splitk > 1 ? 2 : (a.out_mode == OUT_QKV ? 3 : 0);
}

static void plan_general(const GemmArgs& a, const GemmEnv& env, int bn, int qkv_mi, bool plain_pp, GemmPlan& p) {
  const int sk = p.splitk;
  // UPS4 (a.ups == 2): the kernel's rows are the SOURCE pixels of one parity class, blockIdx.z the class
  const int ncls = p.ncls = (a.conv && a.ups == 2) ? 4 : 1;
  const int Mk = p.M = a.M / ncls;
  p.rows_per_batch = a.rows_per_batch / ncls;
  p.k_bn = bn;
  p.tiles_n = cdiv(a.N, bn);
  plan_waves(a, env, bn, sk, Mk, ncls, p.tiles_n, qkv_mi, plain_pp, &p.nwv, &p.mi);
  p.tile_rows = (p.nwv / 2) * p.mi * 16;
  p.tiles_m = cdiv(Mk, p.tile_rows);
  // Short-K GEMMs with many N tiles (GEGLU, QKV: K = 320..1280, 6..80 N tiles) spend most of a tile's life in the first-load
  // latency and the epilogue.  Let one workgroup walk `npw` N tiles back to back instead: the ring is staged across tile
  // boundaries, so the loads of tile t+1 fly during the epilogue of tile t.  Keep ~2 workgroups per CU.
  p.npw = 1;
  if (!a.conv && sk == 1 && p.nwv != 8 && !a.gn_stats && p.tiles_n >= 2) {
    int groups = cdiv(512, p.tiles_m);   // ~2 workgroups per CU
    if (groups < 1) groups = 1;
    if (groups > p.tiles_n) groups = p.tiles_n;
    p.npw = cdiv(p.tiles_n, groups);
  }
  p.groups_n = cdiv(p.tiles_n, p.npw);
  {
    const int64_t wel = (int64_t)a.N * a.K;
    const int64_t ael = (int64_t)a.M * (a.conv ? a.Cin + a.KX : a.K);
    p.n_major = (wel > ael && p.groups_n >= 8) ? 1 : 0;
  }
  xcd_block_pick(a, p, p.tile_rows, bn, ncls);
  p.grid_x = p.tiles_m * p.groups_n;
  // COOP: the finish inside this launch (EPI 6: GroupNorm in the conv epilogue) — no second launch
  p.coop = plan_coop(a, env, p) ? 1 : 0;
  plan_kernel(a, p);
}


// Fills *out and returns the width the GENERAL tiles give these arguments (gemm_plan()'s checks read it also where the streaming tile runs).
static int plan_fill(const GemmArgs& a, const GemmEnv& env, GemmPlan* out) {
  GemmPlan p = {};
  *out = p;
  if (a.M <= 0 || a.N <= 0 || a.K <= 0) return 0;
  const int sk = p.splitk = a.splitk > 1 ? a.splitk : 1;
  const int qkv_mi = qkv_pingpong_mi(env, a);
  const bool plain_pp = plain_pingpong_args(env, a);
  const int bn = plan_tile_width(a, qkv_mi, plain_pp);
  p.M = a.M; p.rows_per_batch = a.rows_per_batch; p.ncls = 1;
  p.kt = BK;
  p.ksteps = a.K / BK;
  p.ksteps_per_split = cdiv(p.ksteps, sk);
  p.grid_y = sk;
  // (GEGLU never takes the streaming tile.  More than GEMM_STREAM64_MAX_ROWS rows: the general tiles read the blocked layout — the 128 x 64 tile
  // is CU-bound per M tile: profiles/r05_opt_stream64.md)
  if (a.w_blk64 && a.act != ACT_GEGLU && a.M <= GEMM_STREAM64_MAX_ROWS) plan_stream64(a, p);
  else plan_general(a, env, bn, qkv_mi, plain_pp, p);
  p.grid_z = p.ncls;
  // the reducer sees the OUTPUT tensor, whatever the conv kernel's row space is
  p.reduce = (sk > 1 && !a.partials_only) ? 1 : 0;
  p.reduce_M = p.reduce ? a.M : 0;
  // planes of row_stats and rows per GroupNorm-statistics slab: the epilogue's (two wave columns per N tile of the general width — also what the
  // streaming launches, which write no statistics, have always reported; 64-row slabs) or the reducer's blocks
  p.row_planes = a.splitk > 1 ? cdiv(a.N, reduce_width(a)) : 2 * cdiv(a.N, bn);
  if (a.splitk > 1 && a.fn_Y) p.gn_slab_rows = a.rows_per_batch;      // the fused reducer files one partial per (sample, bin)
  else p.gn_slab_rows = a.splitk > 1 ? reduce_rows(a) : GN_SLAB_ROWS;
  p.coop_counters = cdiv(a.M, 128) * cdiv(a.N, 160);     // (an upper bound: one per 128-row tile)
  *out = p;
  return bn;
}
void gemm_plan_fill(const GemmArgs& a, const GemmEnv& env, GemmPlan* p) { (void)plan_fill(a, env, p); }

int gemm_row_planes(const GemmArgs& a) { GemmPlan p; gemm_plan_fill(a, gemm_env_default(), &p); return p.row_planes; }
int gemm_gn_slab_rows(const GemmArgs& a) { GemmPlan p; gemm_plan_fill(a, gemm_env_default(), &p); return p.gn_slab_rows; }
int gemm_coop_counters(const GemmArgs& a) { GemmPlan p; gemm_plan_fill(a, gemm_env_default(), &p); return p.coop_counters; }
bool gemm_coop_ok(const GemmArgs& a) { GemmPlan p; gemm_plan_fill(a, gemm_env_default(), &p); return p.coop != 0; }

int gemm_plan(const GemmArgs& a, const GemmEnv& env, GemmPlan* out) {
  // (the checks read two decisions — the general tile width and the in-kernel finish — so the tile is worked out first; none of it survives a refusal)
  GemmPlan p;
  const int width = plan_fill(a, env, &p);
  *out = GemmPlan{};
  GILL_REQUIRE(a.M > 0 && a.N > 0 && a.K > 0, "empty GEMM");
  GILL_REQUIRE((int64_t)a.M * (a.lda > a.N ? a.lda : a.N) < (int64_t)1 << 31, "GEMM operand too large for 32-bit offsets");
  GILL_REQUIRE((int64_t)a.M * (a.ldc > a.ldr ? a.ldc : a.ldr) < (int64_t)1 << 31, "GEMM output / residual too large for 32-bit offsets");
  GILL_REQUIRE(a.K % BK == 0, "K must be a multiple of 64");
  GILL_REQUIRE(a.N % 4 == 0, "N must be a multiple of 4");
  GILL_REQUIRE(a.A != nullptr && a.W != nullptr, "null operand");
  if (a.conv) {
    if (a.ups == 2) {
      GILL_REQUIRE(a.Cin % BK == 0 && a.K == 4 * a.Cin && a.KX == 0, "upsample conv (4-tap form): Cin must be a multiple of 64 and K == 4*Cin");
      GILL_REQUIRE(!a.k_chunked && !a.resid && !a.rowvec && a.M % 4 == 0 && a.OH == 2 * a.IH && a.OW == 2 * a.IW,
                   "upsample conv (4-tap form): tap-major weights, no residual / row vector, output = 2x the source grid");
      GILL_REQUIRE(!a.gn_stats || a.rows_per_batch % 256 == 0, "upsample conv (4-tap form): fused GroupNorm statistics need whole 64-row slabs per class");
    } else {
      GILL_REQUIRE(a.Cin % BK == 0 && a.K == 9 * a.Cin + a.KX, "conv: Cin must be a multiple of 64 and K == 9*Cin + KX");
    }
    if (a.KX) {
      GILL_REQUIRE(a.stride == 1 && !a.ups && a.X1 != nullptr, "conv: the fused 1x1 segment needs stride 1, no upsample");
      GILL_REQUIRE(a.KX % BK == 0 && a.KX1 % BK == 0 && a.KX1 <= a.KX && (a.KX1 == a.KX || a.X2 != nullptr),
                   "conv: fused 1x1 segment channel counts must be multiples of 64");
    }
    GILL_REQUIRE(a.K1 % BK == 0 && a.K1 <= a.Cin, "conv: source split must be a multiple of 64");
    GILL_REQUIRE(a.Cin / BK <= GEMM_ZERO_PAGE_STEPS, "conv: Cin too large for the zero page");
    GILL_REQUIRE(a.K1 == a.Cin || a.A2 != nullptr, "conv: second source missing");
    GILL_REQUIRE(!(a.ups && a.stride != 1), "conv: upsample needs stride 1");
    if (a.pad_shift) {
      GILL_REQUIRE(a.pad_shift == 1 && a.stride == 2 && !a.ups && a.KX == 0, "conv: pad_shift is 0 or 1 and needs stride 2, no upsample, no fused 1x1 segment");
      GILL_REQUIRE(a.IH % 2 == 0 && a.IW % 2 == 0 && a.OH == a.IH / 2 && a.OW == a.IW / 2, "conv: pad_shift needs even IH and IW and an output of half the size");
    }
    GILL_REQUIRE(a.out_mode == OUT_BF16 && a.act == ACT_NONE && !a.resid_f32 && !a.row_stats,
                 "conv: bf16 row-major epilogue without activation / fp32 residual / row statistics only");
    GILL_REQUIRE((int64_t)(a.M / (a.OH * a.OW)) * a.IH * a.IW * a.Cin < (int64_t)1 << 31, "conv input too large for 32-bit offsets");
  } else {
    GILL_REQUIRE(a.K1 % BK == 0 && a.K1 <= a.K, "K split must be a multiple of 64");
    GILL_REQUIRE(a.K1 == a.K || a.A2 != nullptr, "second A source missing");
  }
  if (a.gn_stats) {
    GILL_REQUIRE(a.out_mode != OUT_QKV && a.act != ACT_GEGLU, "fused GroupNorm statistics need the row-major epilogue");
    GILL_REQUIRE(a.rows_per_batch % 64 == 0 && a.gn_groups > 0 && a.gn_groups <= 64 && a.gn_cg * a.gn_groups == a.N,
                 "fused GroupNorm statistics: rows per sample must be a multiple of 64 and bins must tile N");
    GILL_REQUIRE(gemm_fused_gn_ok(a.N, a.gn_cg) && width % a.gn_cg == 0,
                 "fused GroupNorm statistics: bins must not straddle output tiles");
  }
  if (a.row_stats)
    GILL_REQUIRE(a.out_mode == OUT_BF16 && a.act != ACT_GEGLU, "row statistics need the bf16 row-major epilogue");
  if (a.ln_stats) {
    GILL_REQUIRE(a.ln_planes >= 1 && a.ln_planes <= LN_MAX_PLANES, "folded LayerNorm: 1 <= ln_planes <= 20");
    GILL_REQUIRE(a.ln_colsum != nullptr && !a.conv && a.K1 == a.K, "folded LayerNorm: column sums missing / single-source plain GEMM only");
    GILL_REQUIRE(a.act == ACT_GEGLU || a.out_mode == OUT_QKV || a.out_mode == OUT_SOFTMAX80, "folded LayerNorm is implemented in the GEGLU, QKV and softmax epilogues");
    GILL_REQUIRE(a.alpha == 1.f, "folded LayerNorm: alpha must be 1");
  }
  GILL_REQUIRE((a.fn_Y == nullptr && a.fn_ss == nullptr) || p.coop || (a.fn_ss == nullptr && a.splitk > 1 && gemm_fused_norm_ok(a)),
               "fused GroupNorm output: split-K GEMMs of a supported geometry, or an in-kernel finish (gemm_coop_ok), only");
  GILL_REQUIRE(a.C != nullptr || a.fn_Y != nullptr || a.out_mode == OUT_QKV, "no output tensor");
  if (a.splitk > 1) {
    GILL_REQUIRE(a.ws != nullptr, "split-K workspace missing");
    GILL_REQUIRE(a.act != ACT_GEGLU, "split-K cannot be combined with GEGLU");
  }
  if (a.act == ACT_GEGLU) {
    GILL_REQUIRE(a.N % 128 == 0 && a.out_mode == OUT_BF16, "GEGLU needs N % 128 == 0 and bf16 row-major output");
  } else {
    if (a.out_mode == OUT_SOFTMAX80)
      GILL_REQUIRE(a.N % 160 == 0 && a.splitk <= 1 && a.ln_stats && a.ln_colsum && a.bias && !a.conv && !a.gn_stats && !a.row_stats && a.C,
                   "softmax epilogue: N % 160 == 0, no split-K, folded-LayerNorm operands and a bias vector required");
    if (a.out_mode == OUT_QKV) GILL_REQUIRE(a.dp % 8 == 0 && a.heads > 0 && a.ntok > 0, "bad QKV scatter geometry (padded head dim must be a multiple of 8)");
    if (a.w_blk64)
      GILL_REQUIRE(!a.conv && a.N % 64 == 0 && a.K1 == a.K && !a.gn_stats && !a.row_stats && !a.ln_stats && !a.wb_rows && !a.fn_Y &&
                       a.act != ACT_GEGLU && a.out_mode != OUT_SOFTMAX80,
                   "64 x 64-blocked weights (STREAM64): plain GEMMs with the row-major, QKV or split-K epilogue only");
  }
  if (p.k_bn != 64) {      // what the general tiles ask of the arguments
    GILL_REQUIRE(a.wb_rows == 0 || (a.wb_rows % p.tile_rows == 0 && !a.conv), "per-sample weights: tiles must not straddle samples");
    if (p.nwv == 8) GILL_REQUIRE(p.npw == 1, "internal: the ping-pong kernel walks one N tile per workgroup");
    GILL_REQUIRE(p.coop || p.splitk > 1 || (a.fn_Y == nullptr && a.fn_ss == nullptr), "fused GroupNorm output without a split-K reducer or an in-kernel finish");
  }
  *out = p;
  return 0;
}
