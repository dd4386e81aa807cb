// bf16 MFMA GEMM / implicit-GEMM 3x3 convolution for gfx950 (CDNA4).
//
//   C[M,N] = epilogue(alpha * A[M,K] . W[N,K]^T)
//
// Tile: 128 x BN x 64 per 256-thread workgroup (4 waves as 2x2, each wave 64 x BN/2 via
// v_mfma_f32_16x16x32_bf16), two workgroups per CU; the 3x3 convolutions run on a 256 x 160 tile of 8 waves, one workgroup
// per CU, 3-deep ring, with a ping-pong main loop (see "PING-PONG" in the kernel).  Both operands are K-contiguous, so both LDS tiles are
// [rows][64 bf16] = 128 B rows filled by direct-to-LDS DMA (global_load_lds_dwordx4: one
// wave instruction = 1 KiB = 8 tile rows) into a 2-deep ring: the DMA of K step i+1 flies while
// step i is multiplied.  The DMA destination is lane-linear, so the bank-conflict swizzle
// (16-B slot ^= row&7) is applied on the per-lane SOURCE address and again on the ds_read_b128
// address (conflict-free for the 16-lane read groups).
// The MFMA is issued "swapped" (W fragment as the A operand) so every lane ends up with 4
// consecutive N columns of one M row: bias/residual/activation run on float4s and the
// store is 8 B of bf16 per lane.
//
// The conv path computes the im2col row pointers on the fly: NHWC activations make each
// 64-wide K step a contiguous 128-B run inside one (tap, pixel); per K step the tap offset is a
// wave-uniform scalar added to a per-row centre offset, padding taps read a zero page.
//
// Workgroup -> tile mapping is XCD-aware: the dispatcher places workgroup b on XCD b % 8, so ids are
// remapped (bijectively) to give every XCD a contiguous range of tiles — the N tiles of one M range
// and the 3x3 halo rows of neighbouring M ranges then hit the same 4 MiB L2.
#include "gemm_dev.h"
#include "gemm_plan.h"
#include <stdlib.h>

#define BK GEMM_BK
#define GEMM_THREADS 256

// zeros read by padding taps; a row's pointer advances 128 B per K step within a (tap, source) segment, so the page
// covers the longest segment (ZERO_PAGE_STEPS K steps) plus one 128-B row
#define ZERO_PAGE_STEPS GEMM_ZERO_PAGE_STEPS
__device__ __attribute__((aligned(256))) uint32_t g_zero_page_storage[(ZERO_PAGE_STEPS + 1) * 32];

const bf16_t* gill_zero_page() {
  static const bf16_t* p = nullptr;
  if (!p) {
    void* d = nullptr;
    if (hipGetSymbolAddress(&d, HIP_SYMBOL(g_zero_page_storage)) == hipSuccess) {
      (void)hipMemset(d, 0, sizeof(g_zero_page_storage));
      p = (const bf16_t*)d;
    }
  }
  return p;
}

struct GemmDev {
  GemmArgs a;
  const bf16_t* zero;
  int ksteps;        // K / 64
  int ksteps_per_split;
  int tiles_n;
  int npw;           // N tiles one workgroup walks back to back (plain GEMM, no split-K): the LDS ring keeps flowing
  int groups_n;      // cdiv(tiles_n, npw)
  int nwv;           // waves per workgroup: 4 (128-row tile) or 2 (64-row tile)
  int mi;            // 16-row M sub-tiles per wave: 4, or 2 (nwv = 4: the 64-row tile on four waves)
  int kt;            // K elements per ring stage: 64 (2-deep ring) or 32 (4-deep ring, 128-row tiles only)
  int n_major;       // 1: consecutive tile ids walk M first (an XCD's contiguous id range = a range of N tiles over every M tile)
  int tiles_m;
  int xb_m, xb_n;    // > 0: XCD BLOCK MAP — XCD x owns an xb_m x xb_n block of the (M tile, N group) grid (see xcd_block_pick()); 0: the range map above
};

// ---- COOP: hand-offs between the co-resident workgroups of ONE launch (cdna_hip_programming.md Guideline 16, recipe R1; prices in
// MI355X_MICROARCH.md "publish-large").  Payload (the GroupNorm partials) goes out WRITE-THROUGH (sc1: nothing left dirty, no release fence), every storing
// wave drains its own stores (s_waitcnt vmcnt(0)), the workgroup meets at a barrier, ONE lane arrives on the group's counter (agent-scope atomic)
// and polls it relaxed with s_sleep; readers then read the few words with sc1 loads.
// Counters are zeroed once per forward (unet.hip), every slot is used by exactly one launch: the target is the group size.
// The spin is bounded: a workgroup that gives up poisons its outputs with NaN (every test and bench.py check finiteness) instead of hanging the GPU.
__device__ __forceinline__ void st_wt_f32(float* p, float v) {
  __hip_atomic_store(reinterpret_cast<unsigned*>(p), __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float ld_wt_f32(const float* p) {
  return __uint_as_float(__hip_atomic_load(reinterpret_cast<const unsigned*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
#define COOP_SPIN_LIMIT (1u << 18)
// give-ups since the last gemm_coop_check(): a waiter that ran out of patience (the GPU is being shared with another process or stream that ALSO
// runs waiting workgroups — the co-residency contract of GemmArgs::coop_ctr is broken) counts itself here before it poisons its outputs
__device__ unsigned g_coop_giveups;
__device__ __forceinline__ void coop_note_giveup() { __hip_atomic_fetch_add(&g_coop_giveups, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void coop_arrive(unsigned* ctr) { __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ bool coop_wait(unsigned* ctr, unsigned target) {
  for (unsigned spins = 0;; ++spins) {
    if (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= target) return true;
    if (spins > COOP_SPIN_LIMIT) { coop_note_giveup(); return false; }
    __builtin_amdgcn_s_sleep(2);
  }
}

// CONV: 0 plain GEMM, 1 conv3x3, 2 conv3x3 with fused nearest-2x upsample (9 taps gathered from the source grid),
//       3 nearest-2x upsample + conv3x3 as FOUR 2x2-tap convolutions of the source grid, one per output parity (see "UPS4")
// EPI : 0 row-major (bf16 / fp32) epilogue, 1 GEGLU, 2 raw fp32 split-K partials, 3 QKV head-major scatter,
//       4 = 0 without activation / fp32 output / fp32 residual (the UNet's plain GEMMs: half the epilogue's code and branches)
//       5 folded-LayerNorm scores + softmax over each wave's 80 columns (OUT_SOFTMAX80; BN = 160)
//       6 = 0 on the ping-pong conv tiles + the consuming GroupNorm finished in-kernel (COOP, splitk == 1: see GemmArgs::coop_ctr)
// STAGES: depth of the LDS ring.  2: two workgroups per CU hide each other's DMA waits.  3: one workgroup per CU,
//         the DMA of K steps i+1 AND i+2 is in flight while step i is multiplied (counted s_waitcnt vmcnt(N), raw
//         s_barrier) — for grids of ~one workgroup per CU where co-residency cannot do the hiding.
// NWV: waves per workgroup.  4 -> 128-row tile (waves 2 x 2).  2 -> 64-row tile (waves 1 x 2) for problems with so few
// 128-row tiles that half the CUs would idle (UNet level 2-3 projections: M = 2048 / 512).
// 8 -> 256-row tile (waves 4 x 2, one workgroup per CU).  BN = 160, STAGES = 3: the convolutions' ping-pong kernel.
// BN: 128 | 160 (general and ping-pong tiles), 64 (STREAM64).  (A 256 x 256 eight-wave tile for the wide plain GEMMs — half the bytes per FLOP of the
// 128 x 160 tile, whose 36.8 KiB per 2.6 MFLOP is 89 % of the 64 B/clk a CU can pull from L2 at the MFMA peak — measured slower and is gone with
// its switch: profiles/r02_big_tile.md.)
// KT: K elements per ring stage.  Every instantiation has KT = 64 and the plan never asks for another (GemmPlan::k_kt, GemmDev::kt).  The
// parameter is what is left of a 4-deep ring of 32-wide stages in the SAME 73.7 KiB of LDS — loads issued three stages ahead and waited for with
// counted s_waitcnt vmcnt(N), at the price of a barrier per 32-wide stage; that price measured higher than the gain (+7 % on the loop) and the
// switch that selected it is gone.  It stays a parameter because removing it renames and re-lays-out every kernel.
// MI: 16-row M sub-tiles per wave (4 | 2).  MI = 2 with NWV = 4 is a 64-row tile on FOUR waves (2 x 2, wave tile 32 x BN/2) for the
// small plain GEMMs: the same 48 KiB of LDS as the 2-wave 64 x 128 tile (three workgroups per CU), twice the waves per CU.
// (The timing-only ablation guards of round 4 — PP_ABL: no fragment reads / no LDS-DMA / no MFMAs / no bookkeeping / no epilogue / no barriers —
// are gone from this file; their table is profiles/r04_pingpong_ablations.md, the bare loops live on in tools/ubench/gemm_loop.hip and gemm_ws.hip.)
// The kernel body is a device function of the workgroup's coordinates; gemm_kernel below passes blockIdx / gridDim.  (Reading them in the body itself
// is the same program and a different instruction schedule in all 63 instantiations — profiles/gemm_prune_isa.md — so the wrapper stays.)
struct GemmTileCtx {
  int bx, by, bz, gdx;
};
template <int NWV, int BN, int CONV, int EPI, int STAGES, int KT, int MI>
__device__ __forceinline__ void gemm_tile(const GemmDev& d, const GemmTileCtx cx) {
  constexpr int BM = (NWV / 2) * MI * 16;
  static_assert(MI == 4 || (MI == 2 && NWV == 4 && CONV == 0 && (STAGES == 2 || STAGES == 3) && KT == 64) ||
                    (MI == 2 && NWV == 8 && BN == 160 && STAGES == 3 && KT == 64) || (MI == 2 && NWV == 8 && BN == 64 && STAGES == 6 && CONV == 0 && KT == 64) ||
                    (MI == 2 && NWV == 8 && BN == 128 && STAGES == 2 && CONV == 0 && KT == 64),
                "MI = 2: the 4-wave 64-row plain tile, the 128 x 160 ping-pong tile (8 waves of 32 x 80), or the 128 x 64 streaming tile on 8 waves of 32 x 32");
  constexpr int NT = BN / 32;  // 16-wide N sub-tiles per wave (wave covers BN/2 columns)
  constexpr bool PP = (NWV == 8 && BN == 160 && STAGES == 3 && KT == 64);   // ping-pong main loop (see there)
  // STREAM64 (host side: gemm_stream64_weights()): W is stored as [N / 64][K / 64][64 rows][64 k] — a K step's 64 x 64 weight tile is ONE
  // contiguous 8 KiB run (whole DRAM pages) instead of 64 rows of 128 B at a stride of K — and is streamed with the non-temporal policy
  constexpr bool WBLK = (BN == 64 && STAGES == 6 && CONV == 0);
  static_assert(KT == 64 || KT == 32, "stage depth");
  constexpr int LPR = KT / 8;          // lanes (16-B chunks) per tile row
  constexpr int RPI = 64 / LPR;        // tile rows one 1-KiB LDS-DMA wave-instruction covers (8 | 16)
  constexpr int KK = KT / 32;          // 32-wide MFMA k steps per stage
  // XOR swizzle of the 16-B chunk index by the row: conflict-free ds_read_b128 of 16 consecutive rows
  // (KT = 64: rows are 128 B, chunk ^= row & 7; KT = 32: rows are 64 B, chunk ^= (row >> 2) & 3)
#define SWZ(row) (KT == 64 ? ((row) & 7) : (((row) >> 2) & 3))
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  bf16_t* smem = reinterpret_cast<bf16_t*>(smem_raw);
  // layout: [buf][A tile BM*KT | B tile BN*KT]
  constexpr int A_ELEMS = BM * KT;
  constexpr int B_ELEMS = BN * KT;
  constexpr int BUF_ELEMS = A_ELEMS + B_ELEMS;

  const GemmArgs& p = d.a;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  // XCD-aware (bijective) remap of the workgroup id
  int tile;
  {
    const int nwg = cx.gdx, bid = cx.bx;
    const int q = nwg >> 3, r = nwg & 7;
    const int xcd = bid & 7, idx = bid >> 3;
    tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  // weight-heavy problems (N*K > the activation matrix: UNet levels 2-3, the LM) give each XCD a range of N tiles, so every
  // weight is fetched into one L2 only; activation-heavy ones a range of M tiles (N tiles and 3x3 halo rows share the L2)
  int gn = d.n_major ? tile / d.tiles_m : tile % d.groups_n;
  int tm = d.n_major ? tile % d.tiles_m : tile / d.groups_n;
  if (d.xb_m > 0) {
    // XCD block map (round 6): the 8 XCDs tile the (M tile, N group) grid with xb_m x xb_n blocks, so that an XCD's L2 holds xb_m tiles' worth of
    // activations (read once, re-used by the 3x3 taps and by the block's N groups) and 1 / (groups_n / xb_n) of the weights — the two range maps
    // above are its extreme cases (all of M x 1/8 of N: every L2 pulls the whole activation tensor per tap; 1/8 of M x all of N: every L2 pulls
    // every weight).  gridDim.x == tiles_m * groups_n == 8 * xb_m * xb_n (xcd_block_pick()).
    const int bid = cx.bx, xcd = bid & 7, idx = bid >> 3;
    const int blocks_m = d.tiles_m / d.xb_m;
    const int bmi = xcd % blocks_m, bni = xcd / blocks_m;
    tm = bmi * d.xb_m + idx % d.xb_m;
    gn = bni * d.xb_n + idx / d.xb_m;
  }
  const int m0 = tm * BM;
  const int tn_first = gn * d.npw;
  // (convolutions and split-K partials: one N tile per workgroup — gemm_plan.hip plan_general() — known at compile time, so that the K walk's
  // state is dead by the epilogue instead of being carried around it for a next tile that never comes)
  const int ntl = (CONV != 0 || EPI == 2) ? 1 : ((d.tiles_n - tn_first < d.npw) ? d.tiles_n - tn_first : d.npw);   // N tiles of this workgroup
  int n0 = tn_first * BN;
  const int z = cx.by;
  const int kt_beg = z * d.ksteps_per_split;
  int kt_end = kt_beg + d.ksteps_per_split;
  if (kt_end > d.ksteps) kt_end = d.ksteps;
  const int nsteps = kt_end - kt_beg;
  // UPS4 (CONV = 3).  conv3x3(nearest_2x(x)) reads, for the output pixel (2y + py, 2x + px), only the 2 x 2 source pixels
  // (y + py - 1 + a, x + px - 1 + b), a, b in {0, 1}: the 9 taps fall onto them in groups whose weights can be summed once at load
  // (conv_weight_relayout_ups4_launch: W4[class][n][a*2+b][c]; a summed group is always in or out of the image as a whole).  So the
  // layer is four stride-1 2x2-tap convolutions of the SOURCE grid — K = 4 Cin instead of 9 Cin, the same linear map with 2.25x
  // fewer multiply-adds.  blockIdx.z = parity class; p.M = source pixels (rows of one class); output row of source row m:
  // (b * OH + 2y + py) * OW + 2x + px.
  const int cls = (CONV == 3) ? cx.bz : 0;
  const int ups_py = cls >> 1, ups_px = cls & 1;

  // ---- per-lane staging geometry: instruction i of wave w fills tile rows (i*NWV+w)*RPI .. +RPI
  const int srow = lane / LPR;                            // row within the instruction's row group
  const int schunk = (lane % LPR) ^ SWZ(srow);            // logical 16-B chunk this lane fetches (source-side swizzle;
                                                          // group bases are multiples of RPI, so SWZ(row) == SWZ(srow))

  // A rows (4 per lane): element offset of the row start (plain) / of the centre input pixel (conv) in each source,
  // plus conv flag bits {1: dy=-1 in range, 2: dy=+1, 4: dx=-1, 8: dx=+1, 16: oy odd, 32: ox odd}
  constexpr int AI = BM / (RPI * NWV);                    // A instructions per wave per stage (4 | 2)
  int a_off1[AI], a_off2[AI], a_fl[AI], a_pc[AI];
#pragma unroll
  for (int i = 0; i < AI; ++i) {
    int row = (i * NWV + w) * RPI + srow;
    int m = m0 + row;
    if (m > p.M - 1) m = p.M - 1;
    a_fl[i] = 0; a_pc[i] = 0;
    if constexpr (CONV == 0) {
      a_off1[i] = m * p.lda + schunk * 8;
      a_off2[i] = m * p.lda2 + schunk * 8;
    } else {
      const int ohw = p.OH * p.OW;
      const int b = m / ohw;
      const int r = m - b * ohw;
      const int oy = r / p.OW;
      const int ox = r - oy * p.OW;
      int fl = 0, pc;
      if constexpr (CONV == 3) {      // rows are SOURCE pixels: a stride-1 walk of the source grid
        const int shw = p.IH * p.IW;
        const int sb = m / shw;
        const int sr = m - sb * shw;
        const int sy = sr / p.IW, sx = sr - sy * p.IW;
        pc = m;
        fl |= (sy - 1 >= 0) ? 1 : 0; fl |= (sy + 1 < p.IH) ? 2 : 0;
        fl |= (sx - 1 >= 0) ? 4 : 0; fl |= (sx + 1 < p.IW) ? 8 : 0;
      } else if constexpr (CONV == 2) {
        pc = (b * p.IH + (oy >> 1)) * p.IW + (ox >> 1);
        fl |= (oy - 1 >= 0) ? 1 : 0; fl |= (oy + 1 < p.OH) ? 2 : 0;
        fl |= (ox - 1 >= 0) ? 4 : 0; fl |= (ox + 1 < p.OW) ? 8 : 0;
        fl |= (oy & 1) << 4; fl |= (ox & 1) << 5;
      } else {
        const int cy = oy * p.stride + p.pad_shift, cx = ox * p.stride + p.pad_shift;     // (pad_shift: GemmArgs — the centre moves, the flags follow)
        pc = (b * p.IH + cy) * p.IW + cx;
        fl |= (cy - 1 >= 0) ? 1 : 0; fl |= (cy + 1 < p.IH) ? 2 : 0;
        fl |= (cx - 1 >= 0) ? 4 : 0; fl |= (cx + 1 < p.IW) ? 8 : 0;
      }
      a_fl[i] = fl;
      a_pc[i] = m;          // output pixel == input pixel of the fused 1x1 shortcut segment (stride 1 only)
      a_off1[i] = pc * p.K1 + schunk * 8;
      a_off2[i] = pc * (p.Cin - p.K1) + schunk * 8;
    }
  }
  // W rows: groups of RPI rows dealt to the waves round robin; a wave's last instruction may have no group (KT = 32, BN = 160:
  // 10 groups over 4 waves)
  constexpr int WG = BN / RPI;                  // row groups of the W tile
  constexpr int WI = (WG + NWV - 1) / NWV;      // W instructions per wave per stage (the last one predicated)
  static_assert(BN % RPI == 0, "whole row groups");
  const bool w_last_ok = ((WI - 1) * NWV + w) < WG;       // wave-uniform
  const int lw = AI + (w_last_ok ? WI : WI - 1);           // LDS-DMA instructions this wave issues per stage
  const bf16_t* w_ptr[WI];
  int n_issue = n0;        // first column of the N tile being staged
  // WIDE EPILOGUE STORES.  The MFMA (W fragment as the A operand) leaves a lane with 4 consecutive output columns of one row per
  // 16-wide sub-tile j; stored as they are, a wave instruction writes 16 rows x 32 B.  Which weight row sits in which LDS tile row
  // is free (the DMA source address is per lane), so tile row (j, x) of a wave's half is loaded with column c(j, x) such that the
  // sub-tiles j, j + 1 of a lane hold 8 CONSECUTIVE columns: c = (j >> 1) * 32 + (x >> 2) * 8 + (j & 1) * 4 + (x & 3) — one 16-B
  // store per lane, 64 contiguous bytes per row per instruction, half the store instructions (a last unpaired sub-tile, NT odd,
  // keeps c = j * 16 + x).  GEGLU (EPI 1; weight rows come in [16 value | 16 gate] blocks of 16 outputs): value and gate
  // sub-tiles of two pairs are laid out so that the lane's two products are 8 consecutive OUTPUT columns.
  auto tile_col = [&](int R) -> int {    // LDS tile row R -> column of the tile whose weight row it holds
    const int half = R / (BN / 2), q = R - half * (BN / 2);
    const int j = q >> 4, x = q & 15;
    int c;
    if constexpr (EPI == 1) {
      static_assert(EPI != 1 || NT % 4 == 0, "GEGLU: whole value/gate quads per wave");
      const int o = (x >> 2) * 8 + ((j >> 1) & 1) * 4 + (x & 3);          // output column within the quad's 32
      c = (j >> 2) * 64 + (o >> 4) * 32 + (o & 15) + (j & 1) * 16;       // physical: [16 value | 16 gate] per 16 outputs
    } else {
      c = ((j | 1) < NT) ? (j >> 1) * 32 + (x >> 2) * 8 + (j & 1) * 4 + (x & 3) : q;
    }
    return half * (BN / 2) + c;
  };
  // 64 x 64-blocked weights on the GENERAL tiles too (plain GEMMs, GemmArgs::w_blk64 with more rows than the STREAM64 tile is for — ADVICE r05): the
  // tile's weight rows come out of N / 64 blocks, a K step ahead is the next 8 KiB block of each
  const bool wblk = WBLK || (CONV == 0 && p.w_blk64 != 0);
  const int w_step = wblk ? 4096 : KT;
  const bf16_t* Wb = p.W + (p.wb_rows ? (size_t)(m0 / p.wb_rows) * (size_t)p.wb_stride : (size_t)0);     // per-sample weights (GemmArgs::wb_rows)
  auto w_setup = [&]() {
#pragma unroll
    for (int i = 0; i < WI; ++i) {
      int row = tile_col((i * NWV + w) * RPI + srow);
      int n = n_issue + row;
      if (n > p.N - 1) n = p.N - 1;
      if (wblk) w_ptr[i] = Wb + ((size_t)(n >> 6) * d.ksteps + kt_beg) * 4096 + (n & 63) * 64 + schunk * 8;     // (N % 64 == 0: n is never clamped across a block)
      else w_ptr[i] = Wb + ((size_t)cls * p.N + n) * p.K + schunk * 8 + kt_beg * KT;
    }
  };
  w_setup();
  const bf16_t* zero_lane = d.zero + schunk * 8;

  // ---- K-step addressing is incremental: K is walked in (tap, source) segments inside which every row pointer just
  // advances by 64 elements; seg_setup() (wave-uniform control flow, once per segment) recomputes the 4 A row pointers
  const bf16_t* a_ptr[AI];
  int seg_left = 0;
  auto seg_setup = [&](int k0) {
    if constexpr (CONV == 0) {
      const bool first = (k0 < p.K1);
      const bf16_t* src = first ? p.A : p.A2;
      const int kk = first ? k0 : k0 - p.K1;
#pragma unroll
      for (int i = 0; i < AI; ++i) a_ptr[i] = src + (first ? a_off1[i] : a_off2[i]) + kk;
      seg_left = ((first ? p.K1 : p.K) - k0) / KT;
    } else {
      if (CONV == 1 && k0 >= 9 * p.Cin) {
        // fused 1x1 "conv_shortcut" segment: K continues over the channels of the raw block input X1 (++ X2) at the
        // centre pixel; the weight rows carry [conv taps | shortcut] back to back
        const int ke = k0 - 9 * p.Cin;
        const bool fx = (ke < p.KX1);
        const bf16_t* xs = fx ? p.X1 : p.X2;
        const int cx = fx ? p.KX1 : (p.KX - p.KX1);
        const int kc = (fx ? ke : ke - p.KX1) + schunk * 8;
#pragma unroll
        for (int i = 0; i < AI; ++i) a_ptr[i] = xs + (size_t)a_pc[i] * cx + kc;
        seg_left = ((fx ? p.KX1 : p.KX) - ke) / KT;
      } else {
        // all wave-uniform: chunk, tap, source tensor, channel offset, tap displacement.  K order: 64-channel chunks, the 9
        // taps inside a chunk (see conv_weight_relayout_chunked_launch): one (chunk, tap) per K step
        int tap, c0;
        if (p.k_chunked) {
          const int chunk = k0 / (9 * BK);
          const int r = k0 - chunk * (9 * BK);
          tap = r / BK;
          c0 = chunk * BK + (r - tap * BK);
        } else {
          tap = k0 / p.Cin;
          c0 = k0 - tap * p.Cin;
        }
        const int ty = tap / 3;
        int dy = ty - 1, dx = tap - ty * 3 - 1;
        if constexpr (CONV == 3) { dy = ups_py - 1 + (tap >> 1); dx = ups_px - 1 + (tap & 1); }    // tap = a * 2 + b of the 2 x 2 window
        const int need = (dy < 0 ? 1 : (dy > 0 ? 2 : 0)) | (dx < 0 ? 4 : (dx > 0 ? 8 : 0));
        const bool first = (c0 < p.K1);
        const bf16_t* src = first ? p.A : p.A2;
        const int cs = first ? p.K1 : (p.Cin - p.K1);
        const int cc = first ? c0 : c0 - p.K1;
        const int delta = (dy * p.IW + dx) * cs + cc;   // used when CONV == 1
#pragma unroll
        for (int i = 0; i < AI; ++i) {
          int off = (first ? a_off1[i] : a_off2[i]);
          if constexpr (CONV == 2) {
            const int ddy = (dy + ((a_fl[i] >> 4) & 1)) >> 1, ddx = (dx + ((a_fl[i] >> 5) & 1)) >> 1;
            off += (ddy * p.IW + ddx) * cs + cc;
          } else {
            off += delta;
          }
          const bool ok = (a_fl[i] & need) == need;
          a_ptr[i] = ok ? src + off : zero_lane;
        }
        seg_left = p.k_chunked ? 1 : ((first ? p.K1 : p.Cin) - c0) / KT;
      }
    }
  };
  int k_issue = kt_beg * KT;     // K coordinate of the next step to stage
  int steps_in_tile = 0;
  // One stage = prepare (pointer set-up when the K walk enters a new N tile / (tap, source) segment) + dma (the LDS-DMA
  // instructions) + post (advance the walk).  The ping-pong loop runs the three in different phases.
  auto issue_prepare = [&]() {
    if (steps_in_tile == nsteps) {   // next N tile of this workgroup: same A rows from the top, next BN weight rows
      steps_in_tile = 0;
      k_issue = kt_beg * KT;
      seg_left = 0;
      n_issue += BN;
      w_setup();
    }
    if (seg_left == 0) seg_setup(k_issue);
  };
  auto issue_dma = [&](int buf) {
    bf16_t* As = smem + buf * BUF_ELEMS;
    bf16_t* Bs = As + A_ELEMS;
#pragma unroll
    for (int i = 0; i < AI; ++i) {
      bf16_t* l = As + (i * NWV + w) * RPI * KT;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)a_ptr[i],
                                       (__attribute__((address_space(3))) void*)l, 16, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < WI; ++i) {
      if (i == WI - 1 && !w_last_ok) break;
      bf16_t* l = Bs + (i * NWV + w) * RPI * KT;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)w_ptr[i],
                                       (__attribute__((address_space(3))) void*)l, 16, 0, WBLK ? 2 : 0);     // (aux 2 = nt)
    }
  };
  auto issue_post = [&]() {
    ++steps_in_tile;
    --seg_left;
#pragma unroll
    for (int i = 0; i < AI; ++i) a_ptr[i] += KT;
#pragma unroll
    for (int i = 0; i < WI; ++i) w_ptr[i] += WBLK ? 4096 : (CONV == 0 ? w_step : KT);
    k_issue += KT;
  };
  auto issue = [&](int buf) {
    issue_prepare();
    issue_dma(buf);
    issue_post();
  };

  f32x4 acc[MI][NT];

  const int wm = w >> 1, wn = w & 1;
  const int frow = lane & 15;       // fragment row within a 16-row sub-tile
  const int fkc = lane >> 4;        // 16-B k chunk within the 32-wide MFMA k step

  static_assert(STAGES >= 2 && STAGES <= 6, "ring depth");
  const int total_steps = ntl * nsteps;
#pragma unroll
  for (int s = 0; s < STAGES - 1; ++s)
    if (s < total_steps) issue(s);
  // folded LayerNorm (GEGLU / QKV epilogues): the row factors are loaded here, under the first tile's DMA latency
  float ln_rr[4] = {1.f, 1.f, 1.f, 1.f}, ln_rm[4] = {0.f, 0.f, 0.f, 0.f};   // (first MI entries used)
  if constexpr (EPI == 1 || EPI == 3 || EPI == 5) {
    if (p.ln_stats) {
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const int m = m0 + wm * (MI * 16) + i * 16 + frow;
        if (m < p.M) ln_row_factors(p, m, ln_rr[i], ln_rm[i]);
      }
    }
  }
  int buf = 0, buf_issue = STAGES - 1;
  int flat = 0;          // K steps consumed over all N tiles of this workgroup
  // GEGLU / QKV GEMMs walk several N tiles per workgroup with a 2-deep ring: see DEFER in the main loop
  constexpr bool DEFER = (CONV == 0 && STAGES == 2 && !PP && (EPI == 1 || EPI == 3));
  int deferred_buf = -1;
  for (int t = 0; t < ntl; ++t, n0 += BN) {
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  if constexpr (PP) {
    // ---- PING-PONG main loop (256 x 160 tile, 8 waves 4 x 2, one workgroup per CU, 3-deep ring).  Waves w and w + 4 share a
    // SIMD and sit in different groups; the groups run half a K step apart, so in every phase ONE wave of each SIMD issues its
    // step's 40 MFMAs while the other does its step's memory work (18 ds_read_b128 fragment loads, then its 6-7 LDS-DMA pieces of
    // stage k + 2 with their address bookkeeping).  Phase p (one s_barrier each):  group A  MEM(k) at p = 2k, MMA(k) at 2k + 1;
    // group B  MEM(k) at 2k + 1, MMA(k) at 2k + 2.  Invariant: before the barrier into phase 2k every wave has waited for its own
    // pieces of stage k (in-order vmcnt: at most the pieces of stage k + 1 stay in flight).  Stage k's buffer is last read in
    // phase 2k + 1 and refilled (as stage k + 3) from phase 2k + 2 on.  Bare loop 1352 vs 1058 TFLOP/s for two co-resident
    // 128 x 160 workgroups (tools/ubench/gemm_loop.hip).
    const int grp = w >> 2;
    int issued = total_steps < STAGES - 1 ? total_steps : STAGES - 1;     // stages this wave has issued so far
    bf16x8 af[KK][MI];
    bf16x8 bfr[KK][NT];
    // own pieces of stage k have landed.  With a 3-deep ring at most ONE younger stage is in flight at that point, so the count is 0 or
    // this wave's pieces per stage (AI + WI, or one fewer on the waves whose last W piece has no row group): immediates behind a
    // two-way test — wait_vm()'s general switch is a chain of ~13 compare-and-branch pairs, twice per K step, at the END of group A's MMA phase
    auto landed = [&](int k) {
      if (k >= nsteps) return;
      if (issued - 1 - k <= 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      else if (w_last_ok) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(AI + WI) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(AI + WI - 1) : "memory");
    };
    auto mem = [&](int k) {
      const int sb = k % STAGES;
      const bf16_t* As = smem + sb * BUF_ELEMS;
      const bf16_t* Bs = As + A_ELEMS;
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
#pragma unroll
        for (int i = 0; i < MI; ++i) {
          const int row = wm * (MI * 16) + i * 16 + frow;
          af[kk][i] = *reinterpret_cast<const bf16x8*>(As + row * KT + (((kk * 4 + fkc) ^ SWZ(row)) * 8));
        }
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const int row = wn * (BN / 2) + j * 16 + frow;
          bfr[kk][j] = *reinterpret_cast<const bf16x8*>(Bs + row * KT + (((kk * 4 + fkc) ^ SWZ(row)) * 8));
        }
      }
      // (the pointers of this stage were prepared during the previous MMA phase: only the DMA instructions here)
      // (round 4: only the A rows' pieces here and the W rows' at the tail of the wave's MMA phase, behind its 40 MFMAs — to shorten the
      // memory phase, the longer of the two by the cycle model: loop 477.7 -> 492.6 ms, A/B of two builds.  Not kept.)
      // (the pieces BEFORE the fragment reads instead of behind them: loop 448.6 -> 449.7 ms.  Not kept.)
      if (k + STAGES - 1 < nsteps) { issue_dma((k + STAGES - 1) % STAGES); ++issued; }
    };
    auto mma = [&](int k) {
      // the K walk's pointer advance is straight-line code: it goes out BETWEEN the MFMAs (one scalar / vector instruction per MFMA: the
      // matrix pipe paces the MFMAs at 16 cycles each, an in-order wave that issues them back to back and the bookkeeping behind them
      // pays for the bookkeeping in full at the tail of the phase).  (Past the last issued stage the advanced pointers are never used.)
      issue_post();
#pragma unroll
      for (int kk = 0; kk < KK; ++kk)
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int j = 0; j < NT; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[kk][j], af[kk][i], acc[i][j], 0, 0, 0);
#pragma unroll
      for (int q = 0; q < KK * MI * NT; ++q) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x006, 1, 0);
      }
      // ... the next segment's set-up (branches) behind them
      if (k + STAGES < nsteps) issue_prepare();
    };
    if (STAGES - 1 < nsteps) issue_prepare();
    landed(0);
    __builtin_amdgcn_s_barrier();
    if (grp == 0) {
      for (int k = 0; k < nsteps; ++k) {
        mem(k);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        mma(k);
        landed(k + 1);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
      }
      __builtin_amdgcn_s_barrier();
    } else {
      __builtin_amdgcn_s_barrier();
      for (int k = 0; k < nsteps; ++k) {
        mem(k);
        landed(k + 1);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        mma(k);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
      }
    }
  } else
  for (int it = 0; it < nsteps; ++it, ++flat) {
    // wait for stage `flat` only: the up to STAGES - 2 younger stages (lw instructions each) stay in flight
    if constexpr (STAGES == 2) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else if constexpr (STAGES == 3) {
      // at most one younger stage in flight: 0 or this wave's pieces per stage, as immediates (see the ping-pong loop's landed())
      if (total_steps - 1 - flat <= 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      else if (w_last_ok) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(AI + WI) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(AI + WI - 1) : "memory");
    } else {
      // deeper rings (STREAM64: 6): in the steady state STAGES - 2 younger stages are in flight — this wave's pieces per stage times that, as an
      // immediate behind a two-way test; the last STAGES - 2 steps of the walk just wait for everything (wait_vm()'s run-time switch compiles to a
      // chain of ~15 compare-and-branch pairs per K step: an EMPTY step of this loop cost 0.34 us with it, profiles/r05_opt_stream64.md)
      if (total_steps - 1 - flat < STAGES - 2) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      else if (w_last_ok) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((STAGES - 2) * (AI + WI)) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" ::"n"((STAGES - 2) * (AI + WI - 1)) : "memory");
    }
    __builtin_amdgcn_s_barrier();
    const bf16_t* As = smem + buf * BUF_ELEMS;
    const bf16_t* Bs = As + A_ELEMS;
    buf = (buf + 1 == STAGES) ? 0 : buf + 1;
    // Fragment reads are software-pipelined by hand: the reads of k step kk+1 are ISSUED before the MFMAs of k step kk (two
    // fragment sets live), and sched_barriers pin that order.  Left alone, the compiler recycles one 4-register A fragment
    // for the second k step (read -> s_waitcnt lgkmcnt(0) -> 5 MFMAs, three times over): every one of those waits exposes a
    // full LDS round trip.
    bf16x8 af[KK][MI];
    bf16x8 bfr[KK][NT];
    auto frag_load = [&](int kk) {
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const int row = wm * (MI * 16) + i * 16 + frow;
        const int slot = (kk * 4 + fkc) ^ SWZ(row);
        af[kk][i] = *reinterpret_cast<const bf16x8*>(As + row * KT + slot * 8);
      }
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int row = wn * (BN / 2) + j * 16 + frow;
        const int slot = (kk * 4 + fkc) ^ SWZ(row);
        bfr[kk][j] = *reinterpret_cast<const bf16x8*>(Bs + row * KT + slot * 8);
      }
    };
    frag_load(0);
    // stage the next tile while the first fragments are in flight from LDS (its ~30 instructions cover that latency)
    // (round 4: the stage's 8-9 LDS-DMA pieces issued one at a time BETWEEN this step's MFMAs, fenced, instead of in a bunch here — the
    // microarchitecture notes price a piece at ~60 cycles among bare MFMAs against 100-185 behind fragment reads: loop 447.5 -> 469.1 ms,
    // A/B of two builds in one session.  Not kept.)
    // (DEFER: the first stage of the NEXT N tile is issued from this tile's epilogue instead, after the epilogue's own parameter
    // loads — vmcnt returns in order, so loads issued behind a 1-KiB-per-lane-group DMA stage wait for the whole stage to land, and
    // the compiler fences the epilogue's first load with vmcnt(0) anyway: 1-1.5 us per tile with nothing to do)
    if (flat + STAGES - 1 < total_steps) {
      if (DEFER && it == nsteps - 1) deferred_buf = buf_issue;
      else issue(buf_issue);
    }
    buf_issue = (buf_issue + 1 == STAGES) ? 0 : buf_issue + 1;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      if (kk + 1 < KK) {
        __builtin_amdgcn_sched_barrier(0);
        frag_load(kk + 1);
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[kk][j], af[kk][i], acc[i][j], 0, 0, 0);
    }
  }

  // ---- epilogue.  acc[i][j][r]: m = m0 + wm*(MI*16) + i*16 + (lane&15); column: see tile_col() — sub-tiles (2g, 2g+1) of a lane
  // hold the 8 consecutive columns nbase + g*32 + fkc*8 .. +7 (registers r of sub-tile 2g, then of 2g+1); an unpaired last
  // sub-tile (NT odd) holds nbase + j*16 + fkc*4 .. +3
  const int mrow = m0 + wm * (MI * 16) + frow;
  const int nbase = n0 + wn * (BN / 2);
  constexpr int NG = (NT + 1) / 2;      // column groups per lane
  // UPS4: output row of source row m (divisions once per row, here only)
  auto out_row = [&](int m) -> int {
    if constexpr (CONV == 3) {
      const int shw = p.IH * p.IW;
      const int sb = m / shw;
      const int sr = m - sb * shw;
      const int sy = sr / p.IW, sx = sr - sy * p.IW;
      return (sb * p.OH + 2 * sy + ups_py) * p.OW + 2 * sx + ups_px;
    } else {
      return m;
    }
  };
  if constexpr (EPI == 2) {
    float* ws = p.ws + (size_t)z * (CONV == 3 ? 4 : 1) * p.M * p.N;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      if (mrow + i * 16 >= p.M) continue;
      const int m = out_row(mrow + i * 16);
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const bool pair = (2 * g + 1 < NT);
        const int j1 = pair ? 2 * g + 1 : 2 * g;
        const int n = nbase + (pair ? g * 32 + fkc * 8 : (2 * g) * 16 + fkc * 4);
        if (n >= p.N) continue;
        float* dst = ws + (size_t)m * p.N + n;
        *reinterpret_cast<float4*>(dst) = make_float4(acc[i][2 * g][0], acc[i][2 * g][1], acc[i][2 * g][2], acc[i][2 * g][3]);
        if (pair && n + 4 < p.N)
          *reinterpret_cast<float4*>(dst + 4) = make_float4(acc[i][j1][0], acc[i][j1][1], acc[i][j1][2], acc[i][j1][3]);
      }
    }
  } else if constexpr (EPI == 1) {
    // weight rows are interleaved in 16-row blocks (even block = value rows, odd block = gate rows of 16 outputs); tile_col() deals
    // a quad of sub-tiles (value, gate, value, gate) so that the lane's 2 x 4 products are 8 consecutive output columns
    const float* rr = ln_rr; const float* rm = ln_rm;
#pragma unroll
    for (int qd = 0; qd < NT / 4; ++qd) {
      const int ol = fkc * 8;                                          // output column within the quad's 32 (first of 8)
      const int pv = nbase + qd * 64 + (ol >> 4) * 32 + (ol & 15);     // physical column of the first value row (4 consecutive; +4: second pair)
      if (nbase + qd * 64 >= p.N) continue;            // (N % 128 == 0: a quad's 64 physical columns are all inside or all outside)
      const int no = (nbase + qd * 64) / 2 + ol;                       // logical output column (8 consecutive)
      float4 bv[2], bg[2], sv[2], sg[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        bv[h] = p.bias ? *reinterpret_cast<const float4*>(p.bias + pv + 4 * h) : make_float4(0, 0, 0, 0);
        bg[h] = p.bias ? *reinterpret_cast<const float4*>(p.bias + pv + 16 + 4 * h) : make_float4(0, 0, 0, 0);
        sv[h] = p.ln_stats ? *reinterpret_cast<const float4*>(p.ln_colsum + pv + 4 * h) : make_float4(0, 0, 0, 0);
        sg[h] = p.ln_stats ? *reinterpret_cast<const float4*>(p.ln_colsum + pv + 16 + 4 * h) : make_float4(0, 0, 0, 0);
      }
      // (no branch between these loads and their uses, one explicit wait the compiler's counter tracking sees, stores predicated:
      // see the row-major epilogue)
      __builtin_amdgcn_s_waitcnt(0x0F70);     // vmcnt(0)
      if (DEFER && qd == NT / 4 - 1 && deferred_buf >= 0) { issue(deferred_buf); deferred_buf = -1; }
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const int m = mrow + i * 16;
        float o[8];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const f32x4 av = acc[i][qd * 4 + 2 * h], ag = acc[i][qd * 4 + 2 * h + 1];
          o[4 * h + 0] = (av[0] * rr[i] - rm[i] * sv[h].x + bv[h].x) * gelu_erf(ag[0] * rr[i] - rm[i] * sg[h].x + bg[h].x);
          o[4 * h + 1] = (av[1] * rr[i] - rm[i] * sv[h].y + bv[h].y) * gelu_erf(ag[1] * rr[i] - rm[i] * sg[h].y + bg[h].y);
          o[4 * h + 2] = (av[2] * rr[i] - rm[i] * sv[h].z + bv[h].z) * gelu_erf(ag[2] * rr[i] - rm[i] * sg[h].z + bg[h].z);
          o[4 * h + 3] = (av[3] * rr[i] - rm[i] * sv[h].w + bv[h].w) * gelu_erf(ag[3] * rr[i] - rm[i] * sg[h].w + bg[h].w);
        }
        uint4 ov; ov.x = pack_bf2(o[0], o[1]); ov.y = pack_bf2(o[2], o[3]); ov.z = pack_bf2(o[4], o[5]); ov.w = pack_bf2(o[6], o[7]);
        if (m < p.M) *reinterpret_cast<uint4*>((bf16_t*)p.C + (size_t)m * p.ldc + no) = ov;
      }
    }
  } else if constexpr (EPI == 5) {
    // scores of one (sample, head) per wave half: the wave's 80 columns ARE the head's keys (77 + 3 pads whose bias is -1e30), so the
    // softmax of a row is a reduction over the lane's 20 values and the 4 lanes (fkc) that share the row.  exp2 domain (scale * log2(e)
    // is folded into the per-sample weights).  P is stored row-major: the A operand of the second GEMM.
    static_assert(EPI != 5 || BN == 160, "softmax epilogue: one 80-column head per wave half");
    const size_t vb = p.wb_rows ? (size_t)(m0 / p.wb_rows) * (size_t)p.vb_stride : (size_t)0;
    const float* bias = p.bias + vb;
    const float* csum = p.ln_colsum + vb;
    float4 bzs[NG][2], css[NG][2];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const bool pair = (2 * g + 1 < NT);
      const int n = nbase + (pair ? g * 32 + fkc * 8 : (2 * g) * 16 + fkc * 4);
      bzs[g][0] = *reinterpret_cast<const float4*>(bias + n);
      css[g][0] = *reinterpret_cast<const float4*>(csum + n);
      bzs[g][1] = pair ? *reinterpret_cast<const float4*>(bias + n + 4) : make_float4(0, 0, 0, 0);
      css[g][1] = pair ? *reinterpret_cast<const float4*>(csum + n + 4) : make_float4(0, 0, 0, 0);
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);     // vmcnt(0): see the row-major epilogue
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int m = mrow + i * 16;
      const float rr = ln_rr[i], rm = ln_rm[i];
      float v[NG][8];
      float mx = -INFINITY;
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const bool pair = (2 * g + 1 < NT);
        const f32x4 a0 = acc[i][2 * g], a1 = acc[i][pair ? 2 * g + 1 : 2 * g];
        v[g][0] = a0[0] * rr - rm * css[g][0].x + bzs[g][0].x; v[g][1] = a0[1] * rr - rm * css[g][0].y + bzs[g][0].y;
        v[g][2] = a0[2] * rr - rm * css[g][0].z + bzs[g][0].z; v[g][3] = a0[3] * rr - rm * css[g][0].w + bzs[g][0].w;
        v[g][4] = pair ? a1[0] * rr - rm * css[g][1].x + bzs[g][1].x : -INFINITY; v[g][5] = pair ? a1[1] * rr - rm * css[g][1].y + bzs[g][1].y : -INFINITY;
        v[g][6] = pair ? a1[2] * rr - rm * css[g][1].z + bzs[g][1].z : -INFINITY; v[g][7] = pair ? a1[3] * rr - rm * css[g][1].w + bzs[g][1].w : -INFINITY;
#pragma unroll
        for (int e = 0; e < 8; ++e) mx = fmaxf(mx, v[g][e]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      float sum = 0.f;
#pragma unroll
      for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int e = 0; e < 8; ++e) { v[g][e] = __builtin_amdgcn_exp2f(v[g][e] - mx); sum += v[g][e]; }
      sum += __shfl_xor(sum, 16, 64);
      sum += __shfl_xor(sum, 32, 64);
      const float inv = 1.f / sum;
      if (m < p.M) {
        bf16_t* crow = (bf16_t*)p.C + (size_t)m * p.ldc;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
          const bool pair = (2 * g + 1 < NT);
          const int n = nbase + (pair ? g * 32 + fkc * 8 : (2 * g) * 16 + fkc * 4);
          uint4 o; o.x = pack_bf2(v[g][0] * inv, v[g][1] * inv); o.y = pack_bf2(v[g][2] * inv, v[g][3] * inv);
          o.z = pack_bf2(v[g][4] * inv, v[g][5] * inv); o.w = pack_bf2(v[g][6] * inv, v[g][7] * inv);
          if (pair) *reinterpret_cast<uint4*>(crow + n) = o;
          else *reinterpret_cast<uint2*>(crow + n) = make_uint2(o.x, o.y);
        }
      }
    }
  } else if constexpr (EPI == 3) {
    // head-major scatter; all divisions hoisted: per-row (b, t) once, per-column-group (segment, head, dd) once (dp % 8 == 0: the 8
    // columns of a group lie in one head of one segment)
    int rq[MI], rk[MI], rv[MI]; bool mok[MI];
    float rr[MI], rm[MI];
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int m = mrow + i * 16;
      mok[i] = m < p.M;
      rr[i] = p.ln_stats ? ln_rr[i] : p.alpha; rm[i] = ln_rm[i];
      const int b = m / p.ntok, t = m - b * p.ntok;
      rq[i] = (b * p.heads * p.ntok_pad_q + t) * p.dp;
      rk[i] = (b * p.heads * p.ntok_pad_kv + t + p.kv_tok_offset) * p.dp;
      rv[i] = b * p.heads * p.dpv * p.ntok_pad_kv + t + p.kv_tok_offset;
    }
    const int hd = p.heads * p.dp;
    // epilogue parameters of every column group first (then the deferred stage of the next N tile: see DEFER)
    float4 bzs[NG][2], css[NG][2];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const bool pair = (2 * g + 1 < NT);
      const int n = nbase + (pair ? g * 32 + fkc * 8 : (2 * g) * 16 + fkc * 4);
      const bool hi = pair && (n + 4 < p.N);
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const bool ok = (n < p.N) && ((e == 0) || hi);
        bzs[g][e] = (p.bias && ok) ? *reinterpret_cast<const float4*>(p.bias + n + 4 * e) : make_float4(0, 0, 0, 0);
        css[g][e] = (p.ln_stats && ok) ? *reinterpret_cast<const float4*>(p.ln_colsum + n + 4 * e) : make_float4(0, 0, 0, 0);
      }
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);     // vmcnt(0): see the row-major epilogue
    if (DEFER && deferred_buf >= 0) { issue(deferred_buf); deferred_buf = -1; }
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const bool pair = (2 * g + 1 < NT);
      const int j1 = pair ? 2 * g + 1 : 2 * g;
      const int n = nbase + (pair ? g * 32 + fkc * 8 : (2 * g) * 16 + fkc * 4);
      if (n >= p.N) continue;
      const bool hi = pair && (n + 4 < p.N);
      const int segl = n / hd;
      const int within = n - segl * hd;
      const int h = within / p.dp, dd = within - h * p.dp;
      const int seg = p.seg_base + segl;
      const float4* bz = bzs[g]; const float4* cs = css[g];
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        if (!mok[i]) continue;
        float v[8];
        const f32x4 a0 = acc[i][2 * g], a1 = acc[i][j1];
        v[0] = a0[0] * rr[i] - rm[i] * cs[0].x + bz[0].x; v[1] = a0[1] * rr[i] - rm[i] * cs[0].y + bz[0].y;
        v[2] = a0[2] * rr[i] - rm[i] * cs[0].z + bz[0].z; v[3] = a0[3] * rr[i] - rm[i] * cs[0].w + bz[0].w;
        v[4] = a1[0] * rr[i] - rm[i] * cs[1].x + bz[1].x; v[5] = a1[1] * rr[i] - rm[i] * cs[1].y + bz[1].y;
        v[6] = a1[2] * rr[i] - rm[i] * cs[1].z + bz[1].z; v[7] = a1[3] * rr[i] - rm[i] * cs[1].w + bz[1].w;
        if (seg == 0) {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] *= p.qscale;   // softmax scale * log2(e) folded into Q
        }
        if (seg <= 1) {
          bf16_t* dst = (seg == 0) ? p.Cq + (size_t)rq[i] + (size_t)h * p.ntok_pad_q * p.dp + dd
                                   : p.Ck + (size_t)rk[i] + (size_t)h * p.ntok_pad_kv * p.dp + dd;
          if (hi) {
            uint4 o; o.x = pack_bf2(v[0], v[1]); o.y = pack_bf2(v[2], v[3]); o.z = pack_bf2(v[4], v[5]); o.w = pack_bf2(v[6], v[7]);
            *reinterpret_cast<uint4*>(dst) = o;
          } else {
            uint2 o; o.x = pack_bf2(v[0], v[1]); o.y = pack_bf2(v[2], v[3]);
            *reinterpret_cast<uint2*>(dst) = o;
          }
        } else {
          bf16_t* base = p.Cvt + (size_t)rv[i] + (size_t)(h * p.dpv + dd) * p.ntok_pad_kv;
          const int ne = hi ? 8 : 4;
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (e < ne) base[(size_t)e * p.ntok_pad_kv] = f2bf(v[e]);
          // spare row dp of Vt := 1.0: the attention kernel reads the softmax row sum off the PV MFMAs
          if (dd + ne == p.dp && p.dpv > p.dp) base[(size_t)ne * p.ntok_pad_kv] = (bf16_t)0x3F80;
        }
      }
    }
  } else {
    // row-major epilogue; per-row offsets (incl. the batch index of the row vector) hoisted out of the column loop
    // (32-bit element offsets: gemm_launch() checks M * max(ldc, ldr) < 2^31)
    // The epilogue is written WITHOUT branches between its loads and their uses: all of a column group's loads (bias, row vector,
    // residual, for every row) are issued back to back from addresses clamped into the tensors, then everything is computed, and only
    // the stores are predicated.  With a `continue` per row the compiler has to re-fence every row's block with s_waitcnt vmcnt(0) —
    // and on gfx9 that counter also holds the stores, so every row waited for the previous row's store round trip: 12 serialised
    // round trips made the 256 x 160 conv tile's epilogue 4.1 us (tools/conv_ksweep.py with stamps), 3.4 us per GEGLU tile.
    int crow[MI], rrow[MI]; bool mok[MI];
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int m = mrow + i * 16;
      mok[i] = m < p.M;
      const int mc = mok[i] ? m : p.M - 1;
      crow[i] = out_row(mc) * p.ldc;
      rrow[i] = mc * p.ldr;
    }
    // fused GroupNorm statistics of the OUTPUT tensor (consumed by the next GroupNorm: saves its whole stats pass).
    // The 64 rows of a wave belong to one slab of one sample (rows_per_batch % 64 == 0).  Fixed-order reduction: 4 rows in the
    // lane, 16 row lanes by xor-shuffles, one LDS cell per (row half, column) written once (the tile ring is dead by now),
    // then one thread per (row half, bin, moment) adds the bin's gn_cg columns and stores the partial: no atomics anywhere.
    float2* red = reinterpret_cast<float2*>(smem);   // [NWV / 2 wave rows][BN] {sum, sum of squares}: one 8-byte LDS write per column at
                                                     // base + immediate offset (separate moment planes cost one address register per column)
    float2* red_lane = red + wm * BN + wn * (BN / 2);
    if (p.gn_stats) __syncthreads();                 // every wave is done reading the ring
    float rws[4] = {0.f, 0.f, 0.f, 0.f}, rwq[4] = {0.f, 0.f, 0.f, 0.f};   // row sums for a following (folded) LayerNorm
    constexpr bool F32_PATHS = (CONV == 0 && EPI != 4);     // fp32 residual / fp32 output / activation: plain GEMMs on EPI 0 only
    // phase A: the loads.  Column vector cv = bias (+ the row vector, a per-sample bias — ResnetBlock2D's time embedding — which is the
    // same for all rows of the wave when they lie in one sample: the case in the engines); a wave that straddles samples, and the
    // fp32 residual (32 B per lane and row), take the slow path: loads inside the row loop.
    // The bf16-only kernels (convs, EPI 4) issue the loads of all NG column groups up front (at most 24 + 48 registers next to the
    // 80 accumulators) and wait once: one round trip per tile, and no load ever queues behind a store.  The generic EPI 0 kernel, which
    // also carries the fp32 / activation paths, goes group by group (loads, wait, compute, store: NG round trips).
    constexpr bool ALL_UPFRONT = !F32_PATHS;
    constexpr int NSLOT = ALL_UPFRONT ? NG : 1;
    const int wrow0 = m0 + wm * (MI * 16);
    const int wrow1 = (wrow0 + MI * 16 - 1 < p.M) ? wrow0 + MI * 16 - 1 : p.M - 1;
    const bool rv_pre = p.rowvec && wrow0 < p.M && (wrow0 / p.rows_per_batch == wrow1 / p.rows_per_batch);   // wave-uniform
    const bool rv_slow = p.rowvec && !rv_pre;
    const bool rf_slow = F32_PATHS && p.resid && p.resid_f32;
    const bool rb_pre = p.resid && !rf_slow;
    const float* colvec = rv_pre ? p.rowvec + (wrow0 / p.rows_per_batch) * p.rowvec_bstride : p.bias;    // first (or only) column vector
    const float* colvec2 = rv_pre ? p.bias : nullptr;                                                      // bias on top of a row vector
    float4 cv[NSLOT][2];
    uint2 rb[NSLOT][MI][2];
    auto load_group = [&](int g, int sl) {
      const bool pair = (2 * g + 1 < NT);
      const int n = nbase + (pair ? g * 32 + fkc * 8 : (2 * g) * 16 + fkc * 4);
      const bool hi = pair && (n + 4 < p.N);
      const int nl = (n < p.N) ? n : 0;      // columns the loads use: always inside the row (lanes beyond N are never stored)
      const int nh = hi ? n + 4 : nl;
      cv[sl][0] = cv[sl][1] = make_float4(0, 0, 0, 0);
      if (colvec) {
        cv[sl][0] = *reinterpret_cast<const float4*>(colvec + nl);
        cv[sl][1] = *reinterpret_cast<const float4*>(colvec + nh);
      }
      if (colvec2) {
        const float4 t0 = *reinterpret_cast<const float4*>(colvec2 + nl);
        const float4 t1 = *reinterpret_cast<const float4*>(colvec2 + nh);
        cv[sl][0].x += t0.x; cv[sl][0].y += t0.y; cv[sl][0].z += t0.z; cv[sl][0].w += t0.w;
        cv[sl][1].x += t1.x; cv[sl][1].y += t1.y; cv[sl][1].z += t1.z; cv[sl][1].w += t1.w;
      }
    };
    auto load_group_resid = [&](int g, int sl) {
      const bool pair = (2 * g + 1 < NT);
      const int n = nbase + (pair ? g * 32 + fkc * 8 : (2 * g) * 16 + fkc * 4);
      const bool hi = pair && (n + 4 < p.N);
      const int nl = (n < p.N) ? n : 0;
      const int nh = hi ? n + 4 : nl;
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        rb[sl][i][0] = *reinterpret_cast<const uint2*>((const bf16_t*)p.resid + rrow[i] + nl);
        rb[sl][i][1] = *reinterpret_cast<const uint2*>((const bf16_t*)p.resid + rrow[i] + nh);
      }
    };
    if constexpr (ALL_UPFRONT) {
#pragma unroll
      for (int g = 0; g < NG; ++g) load_group(g, g);
      if (rb_pre) {
#pragma unroll
        for (int g = 0; g < NG; ++g) load_group_resid(g, g);
      }
      // phase B: an explicit s_waitcnt, which the compiler's own counter tracking sees — nothing is pending behind it, so the
      // predicated stores below (branches, i.e. control-flow joins) cannot draw conservative vmcnt(0) fences
      __builtin_amdgcn_s_waitcnt(0x0F70);     // vmcnt(0)
    }
    // phase C: compute and store
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const int sl = ALL_UPFRONT ? g : 0;
      const int rs = sl;
      if constexpr (!ALL_UPFRONT) {
        load_group(g, 0);
        if (rb_pre) load_group_resid(g, 0);
        __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
      }
      const bool pair = (2 * g + 1 < NT);
      const int j1 = pair ? 2 * g + 1 : 2 * g;
      const int cl = pair ? g * 32 + fkc * 8 : (2 * g) * 16 + fkc * 4;    // first column of the group within the wave's half
      const int n = nbase + cl;
      const bool nok = n < p.N;
      const bool hi = pair && (n + 4 < p.N);
      float gs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, gq[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const f32x4 a0 = acc[i][2 * g], a1 = acc[i][j1];
        float v[8] = {a0[0] * p.alpha + cv[sl][0].x, a0[1] * p.alpha + cv[sl][0].y, a0[2] * p.alpha + cv[sl][0].z, a0[3] * p.alpha + cv[sl][0].w,
                      a1[0] * p.alpha + cv[sl][1].x, a1[1] * p.alpha + cv[sl][1].y, a1[2] * p.alpha + cv[sl][1].z, a1[3] * p.alpha + cv[sl][1].w};
        // (slow paths: guarded by wave-uniform flags ONLY and loading from clamped columns, so that they compile to scalar branches —
        // under a lane predicate a never-taken load still executes its s_waitcnt vmcnt(0), which queues behind the previous row's store)
        if (rv_slow) {
          const int vr = (min(mrow + i * 16, p.M - 1) / p.rows_per_batch) * p.rowvec_bstride;
          const int nl = nok ? n : 0, nh = hi ? n + 4 : nl;
          const float4 b0 = *reinterpret_cast<const float4*>(p.rowvec + vr + nl);
          const float4 b1 = *reinterpret_cast<const float4*>(p.rowvec + vr + nh);
          v[0] += b0.x; v[1] += b0.y; v[2] += b0.z; v[3] += b0.w;
          v[4] += b1.x; v[5] += b1.y; v[6] += b1.z; v[7] += b1.w;
        }
        if (rb_pre) {
          v[0] += bf2f((bf16_t)(rb[rs][i][0].x & 0xffff)); v[1] += bf2f((bf16_t)(rb[rs][i][0].x >> 16));
          v[2] += bf2f((bf16_t)(rb[rs][i][0].y & 0xffff)); v[3] += bf2f((bf16_t)(rb[rs][i][0].y >> 16));
          v[4] += bf2f((bf16_t)(rb[rs][i][1].x & 0xffff)); v[5] += bf2f((bf16_t)(rb[rs][i][1].x >> 16));
          v[6] += bf2f((bf16_t)(rb[rs][i][1].y & 0xffff)); v[7] += bf2f((bf16_t)(rb[rs][i][1].y >> 16));
        }
        if (F32_PATHS && rf_slow) {
          const int nl = nok ? n : 0, nh = hi ? n + 4 : nl;
          const float4 r0 = *reinterpret_cast<const float4*>((const float*)p.resid + rrow[i] + nl);
          const float4 r1 = *reinterpret_cast<const float4*>((const float*)p.resid + rrow[i] + nh);
          v[0] += r0.x; v[1] += r0.y; v[2] += r0.z; v[3] += r0.w;
          v[4] += r1.x; v[5] += r1.y; v[6] += r1.z; v[7] += r1.w;
        }
        // (convolutions: no activation, bf16 output, no LayerNorm row sums — gemm_launch() checks — so their kernels carry none of it)
        if (F32_PATHS && p.act != ACT_NONE) {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = apply_act(v[e], p.act);
        }
        const bool st = mok[i] && nok;
        float vs[8];      // what the GroupNorm partials add up: the values as stored (rounded, where the output is bf16)
#pragma unroll
        for (int e = 0; e < 8; ++e) vs[e] = v[e];
        if (F32_PATHS && p.out_mode == OUT_F32) {
          if (st) *reinterpret_cast<float4*>((float*)p.C + crow[i] + n) = make_float4(v[0], v[1], v[2], v[3]);
          if (st && hi) *reinterpret_cast<float4*>((float*)p.C + crow[i] + n + 4) = make_float4(v[4], v[5], v[6], v[7]);
        } else {
          uint4 o; o.x = pack_bf2(v[0], v[1]); o.y = pack_bf2(v[2], v[3]); o.z = pack_bf2(v[4], v[5]); o.w = pack_bf2(v[6], v[7]);
          vs[0] = __uint_as_float(o.x << 16); vs[1] = __uint_as_float(o.x & 0xffff0000u); vs[2] = __uint_as_float(o.y << 16); vs[3] = __uint_as_float(o.y & 0xffff0000u);
          vs[4] = __uint_as_float(o.z << 16); vs[5] = __uint_as_float(o.z & 0xffff0000u); vs[6] = __uint_as_float(o.w << 16); vs[7] = __uint_as_float(o.w & 0xffff0000u);
          const bool stc = st && EPI != 6;     // (COOP: the raw tensor — where somebody else reads it — is stored AFTER the arrival, see below)
          if (stc && hi) *reinterpret_cast<uint4*>((bf16_t*)p.C + crow[i] + n) = o;
          else if (stc) *reinterpret_cast<uint2*>((bf16_t*)p.C + crow[i] + n) = make_uint2(o.x, o.y);
          if constexpr (EPI == 6) {      // the finished values stay in the accumulators until the group's statistics are complete
            acc[i][2 * g] = (f32x4){v[0], v[1], v[2], v[3]};
            if (pair) acc[i][j1] = (f32x4){v[4], v[5], v[6], v[7]};
          }
          if (CONV == 0 && p.row_stats) {   // statistics of what the consumer will read: the rounded values (columns beyond N: none)
            const float r0 = __uint_as_float(o.x << 16), r1 = __uint_as_float(o.x & 0xffff0000u);
            const float r2 = __uint_as_float(o.y << 16), r3 = __uint_as_float(o.y & 0xffff0000u);
            const float r4 = __uint_as_float(o.z << 16), r5 = __uint_as_float(o.z & 0xffff0000u);
            const float r6 = __uint_as_float(o.w << 16), r7 = __uint_as_float(o.w & 0xffff0000u);
            const float slo = (r0 + r1) + (r2 + r3), qlo = (r0 * r0 + r1 * r1) + (r2 * r2 + r3 * r3);
            const float shi = (r4 + r5) + (r6 + r7), qhi = (r4 * r4 + r5 * r5) + (r6 * r6 + r7 * r7);
            rws[i] += nok ? slo : 0.f;
            rwq[i] += nok ? qlo : 0.f;
            rws[i] += hi ? shi : 0.f;      // (two separate additions, low half first: the order the sums have always been formed in)
            rwq[i] += hi ? qhi : 0.f;
          }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {       // (rows beyond M hold the clamped row's values: they must not reach the statistics)
          const float ve = mok[i] ? vs[e] : 0.f;
          gs[e] += ve; gq[e] += ve * ve;
        }
      }
      if (p.gn_stats) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          if (e >= 4 && !pair) break;
          const float a = row16_sum(gs[e]), q = row16_sum(gq[e]);     // over the 16 row lanes (DPP: no LDS traffic)
          if (frow == 0) red_lane[cl + e] = make_float2(a, q);
        }
      }
    }
    if (CONV == 0 && p.row_stats) {
      // a row's BN/2 columns of this wave sit in the 4 lanes {frow, frow+16, frow+32, frow+48}; plane = (N tile, wave column)
      float* plane = p.row_stats + (size_t)((n0 / BN) * 2 + wn) * p.M * 2;
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        rws[i] += __shfl_xor(rws[i], 16, 64); rwq[i] += __shfl_xor(rwq[i], 16, 64);
        rws[i] += __shfl_xor(rws[i], 32, 64); rwq[i] += __shfl_xor(rwq[i], 32, 64);
        if (fkc == 0 && mok[i]) *reinterpret_cast<float2*>(plane + (size_t)(mrow + i * 16) * 2) = make_float2(rws[i], rwq[i]);
      }
    }
    if (p.gn_stats) {
      __syncthreads();
      constexpr int HALVES = BM / 64;
      const int bins_tile = BN / p.gn_cg;            // gemm_fused_gn_ok(): BN % gn_cg == 0
      if (tid < 2 * HALVES * bins_tile) {
        const int which = tid & 1, half = (tid >> 1) % HALVES, lb = (tid >> 1) / HALVES;
        const int mfirst = m0 + half * 64;
        const int bin = n0 / p.gn_cg + lb;
        if (mfirst < p.M && bin < p.gn_groups) {
          // a 64-row slab holds 64 / (MI * 16) wave rows (1, or 2 on the MI = 2 tiles): added in wave-row order, then column order
          constexpr int GPS = 64 / (MI * 16);
          float a = 0.f;
#pragma unroll
          for (int g = 0; g < GPS; ++g) {
            const float* src = reinterpret_cast<const float*>(red + (half * GPS + g) * BN + lb * p.gn_cg) + which;
            for (int c = 0; c < p.gn_cg; ++c) a += src[2 * c];
          }
          // (UPS4: rows_per_batch = SOURCE pixels per sample; a slab = 64 source rows of one class — any fixed partition of a
          // sample's output pixels into 64-row slabs serves the consumer, which only adds the slabs up in index order)
          const int b = mfirst / p.rows_per_batch;
          const int slab = (mfirst - b * p.rows_per_batch) / GN_SLAB_ROWS + (CONV == 3 ? cls * (p.rows_per_batch / GN_SLAB_ROWS) : 0);
          const int nslab = (CONV == 3 ? 4 : 1) * (p.rows_per_batch / GN_SLAB_ROWS);
          float* dst = p.gn_stats + (((size_t)b * nslab + slab) * p.gn_groups + bin) * 2 + which;
          if constexpr (EPI == 6) st_wt_f32(dst, a);       // COOP: the other workgroups of the group read it inside this launch
          else *dst = a;
        }
      }
    }
    if constexpr (EPI == 6) {
      // ---- COOP GroupNorm finish (GemmArgs::coop_ctr, splitk == 1).  The rows_per_batch / BM workgroups that hold the M tiles of one (sample, N tile)
      // have each published their per-slab partials above; once all have arrived every one of them totals the sample's partials for its BN columns
      // EXACTLY as groupnorm_apply_kernel does (16-partial segments on a fixed tree, segments in order, bins in order: bit-identical statistics),
      // folds gamma / beta into per-column scale | shift and normalises the ROUNDED values it still holds in its accumulators — what the
      // stand-alone pass would have read back from HBM.
      static_assert(EPI != 6 || (PP && CONV == 1), "COOP GroupNorm finish: the ping-pong convolution tiles");
      // Order (round 6, second pass): nothing but the few partial stores is in flight at the drain — the raw tensor's 40-80 KiB of stores per
      // workgroup go out AFTER the arrival and land while the group fills up, and gamma / beta are in registers before the wait.
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      float* cs = reinterpret_cast<float*>(smem_raw + 16384);    // scratch behind `red`: seg [32 bins][2][4] | tot [32][2] | scale [BN] | shift [BN] | flag
      float* c_seg = cs; float* c_tot = cs + 256; float* c_sc = cs + 320; float* c_sh = cs + 320 + BN; unsigned* okf = reinterpret_cast<unsigned*>(cs + 320 + 2 * BN);
      const int bsmp = m0 / p.rows_per_batch;
      unsigned* gctr = p.coop_ctr + (size_t)bsmp * d.tiles_n + n0 / BN;
      if (tid == 0) coop_arrive(gctr);
      const bool colt = tid < BN && n0 + tid < p.N;
      const float gam_c = colt ? p.fn_gamma[n0 + tid] : 0.f, bet_c = colt ? p.fn_beta[n0 + tid] : 0.f;
      if (p.C) {
#pragma unroll
        for (int g = 0; g < NG; ++g) {
          const bool pair = (2 * g + 1 < NT);
          const int j1 = pair ? 2 * g + 1 : 2 * g;
          const int n = nbase + (pair ? g * 32 + fkc * 8 : (2 * g) * 16 + fkc * 4);
          const bool nok = n < p.N;
          const bool hi = pair && (n + 4 < p.N);
#pragma unroll
          for (int i = 0; i < MI; ++i) {
            const f32x4 a0 = acc[i][2 * g], a1 = acc[i][j1];
            uint4 o; o.x = pack_bf2(a0[0], a0[1]); o.y = pack_bf2(a0[2], a0[3]); o.z = pack_bf2(a1[0], a1[1]); o.w = pack_bf2(a1[2], a1[3]);
            if (mok[i] && nok && hi) *reinterpret_cast<uint4*>((bf16_t*)p.C + crow[i] + n) = o;
            else if (mok[i] && nok) *reinterpret_cast<uint2*>((bf16_t*)p.C + crow[i] + n) = make_uint2(o.x, o.y);
          }
        }
      }
      if (tid == 0) {
        const bool ok = coop_wait(gctr, (unsigned)(p.rows_per_batch / BM));
        *okf = ok ? 1u : 0u;
      }
      __syncthreads();
      const bool ok = *okf != 0u;
      const int bins_tile = BN / p.gn_cg;                       // <= 32 (gemm_coop_ok)
      const int ns = p.rows_per_batch / GN_SLAB_ROWS;           // <= 64 partials per (sample, bin)
      if (tid < bins_tile * 8) {
        const int seg = tid & 3, which = (tid >> 2) & 1, lb = tid >> 3;
        const float* src = p.gn_stats + (((size_t)bsmp * ns + seg * 16) * p.gn_groups + n0 / p.gn_cg + lb) * 2 + which;
        const size_t step = (size_t)p.gn_groups * 2;
        float pv[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) pv[i] = (seg * 16 + i < ns) ? ld_wt_f32(src + (size_t)i * step) : 0.f;      // sc1 loads: the producers stored sc1
        c_seg[(lb * 2 + which) * 4 + seg] = (((pv[0] + pv[1]) + (pv[2] + pv[3])) + ((pv[4] + pv[5]) + (pv[6] + pv[7]))) +
                                            (((pv[8] + pv[9]) + (pv[10] + pv[11])) + ((pv[12] + pv[13]) + (pv[14] + pv[15])));
      }
      __syncthreads();
      if (tid < bins_tile * 2) { const float* g4 = c_seg + tid * 4; c_tot[tid] = (g4[0] + g4[1]) + (g4[2] + g4[3]); }
      __syncthreads();
      if (tid < BN && n0 + tid < p.N) {
        const int gl = tid / p.fn_cg, r1 = p.fn_cg / p.gn_cg;
        float a = 0.f, q = 0.f;
        for (int bin = gl * r1; bin < (gl + 1) * r1; ++bin) { a += c_tot[bin * 2]; q += c_tot[bin * 2 + 1]; }
        const float inv_n = 1.f / ((float)p.fn_cg * (float)p.rows_per_batch);
        const float sm = a * inv_n;         // E[x]
        const float sq = q * inv_n;         // E[x^2]
        const float var = fmaxf(sq - sm * sm, 0.f);
        const float rstd = rsqrtf(var + p.fn_eps);
        float sc = rstd * gam_c;
        if (!ok) sc = __builtin_nanf("");
        const float sh = bet_c - sm * sc;
        c_sc[tid] = sc; c_sh[tid] = sh;
        if (p.fn_ss && m0 == bsmp * p.rows_per_batch) {        // the scale | shift table, once per (sample, N tile): [B][2][N]
          p.fn_ss[((size_t)bsmp * 2 + 0) * p.N + n0 + tid] = sc;
          p.fn_ss[((size_t)bsmp * 2 + 1) * p.N + n0 + tid] = sh;
        }
      }
      __syncthreads();
      if (p.fn_Y) {
#pragma unroll
        for (int g = 0; g < NG; ++g) {
          const bool pair = (2 * g + 1 < NT);
          const int j1 = pair ? 2 * g + 1 : 2 * g;
          const int cl = pair ? g * 32 + fkc * 8 : (2 * g) * 16 + fkc * 4;
          const int n = nbase + cl;
          const bool nok = n < p.N;
          const bool hi = pair && (n + 4 < p.N);
          const float* scp = c_sc + wn * (BN / 2) + cl; const float* shp = c_sh + wn * (BN / 2) + cl;
          const float4 s0 = *reinterpret_cast<const float4*>(scp), h0 = *reinterpret_cast<const float4*>(shp);
          const float4 s1 = pair ? *reinterpret_cast<const float4*>(scp + 4) : s0, h1 = pair ? *reinterpret_cast<const float4*>(shp + 4) : h0;
#pragma unroll
          for (int i = 0; i < MI; ++i) {
            const f32x4 a0 = acc[i][2 * g], a1 = acc[i][j1];
            float o[8];
            o[0] = fmaf(bf2f(f2bf(a0[0])), s0.x, h0.x); o[1] = fmaf(bf2f(f2bf(a0[1])), s0.y, h0.y);
            o[2] = fmaf(bf2f(f2bf(a0[2])), s0.z, h0.z); o[3] = fmaf(bf2f(f2bf(a0[3])), s0.w, h0.w);
            o[4] = fmaf(bf2f(f2bf(a1[0])), s1.x, h1.x); o[5] = fmaf(bf2f(f2bf(a1[1])), s1.y, h1.y);
            o[6] = fmaf(bf2f(f2bf(a1[2])), s1.z, h1.z); o[7] = fmaf(bf2f(f2bf(a1[3])), s1.w, h1.w);
            if (p.fn_silu) {
#pragma unroll
              for (int e = 0; e < 8; ++e) o[e] = silu_f(o[e]);
            }
            uint4 ov; ov.x = pack_bf2(o[0], o[1]); ov.y = pack_bf2(o[2], o[3]); ov.z = pack_bf2(o[4], o[5]); ov.w = pack_bf2(o[6], o[7]);
            bf16_t* yrow = p.fn_Y + (size_t)(mrow + i * 16) * p.N + n;
            if (mok[i] && nok && hi) *reinterpret_cast<uint4*>(yrow) = ov;
            else if (mok[i] && nok) *reinterpret_cast<uint2*>(yrow) = make_uint2(ov.x, ov.y);
          }
        }
      }
    }
  }
  }   // N tiles of this workgroup
#undef SWZ
}
template <int NWV, int BN, int CONV, int EPI, int STAGES, int KT, int MI>
__global__ __launch_bounds__(NWV * 64, NWV == 8 ? ((BN == 128 && STAGES == 2) ? 2 : 1) : (MI == 2 ? 3 : 2)) void gemm_kernel(const GemmDev d) {
  kernarg_warm<sizeof(GemmDev)>();
  GemmTileCtx cx;
  cx.bx = blockIdx.x; cx.by = blockIdx.y; cx.bz = blockIdx.z; cx.gdx = gridDim.x;
  gemm_tile<NWV, BN, CONV, EPI, STAGES, KT, MI>(d, cx);
}

// ---- host half: the launcher.  Every decision about a launch is made in gemm_plan.hip (gemm_plan.h); this file supplies the process-wide environment,
// fills GemmDev from the plan and maps the plan's template tuple to its instantiation.

// GILL_GEMM_PP = 0 (A/B switch, read once): no ping-pong tiles for the convolutions, the short-K plain GEMMs and the QKV GEMMs (the long-K plain GEMMs keep them)
static bool gemm_pp_switch() {
  static const int pp_env = [] { const char* v = getenv("GILL_GEMM_PP"); return v ? atoi(v) : 1; }();
  return pp_env != 0;
}
static int device_cus() {
  static const int n = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    return v;
  }();
  return n;
}
// GILL_GEMM_COOP = 0: every finish as its own launch (GroupNorm-apply), the round-5 dataflow (A/B and the on / off parity test);
// anything else (default 1): the GroupNorm finish in the 3x3 convolutions' epilogue (EPI 6) — gemm_plan.hip plan_coop()
int gemm_coop_mode() {
  static const int mode = [] { const char* e = getenv("GILL_GEMM_COOP"); return e ? atoi(e) : 1; }();
  return mode;
}
GemmEnv gemm_env_default() {
  GemmEnv e;
  e.pp = gemm_pp_switch() ? 1 : 0; e.coop = gemm_coop_mode(); e.cus = device_cus();
  return e;
}
// Reads and clears the give-up count of the in-kernel finishes (a small synchronous copy: call it where the host waits anyway).  Non-zero means
// outputs of an earlier launch were NaN-poisoned because waiting workgroups were not co-resident: this process shared the GPU with another stream
// or process that ALSO ran waiting workgroups (two of them can starve each other for CUs).  The contract is exclusive use of the device by ONE
// handle's stream while it runs, or GILL_GEMM_COOP=0.
int gemm_coop_giveups(unsigned* count) {
  unsigned n = 0;
  *count = 0;
  if (gemm_coop_mode() == 0) return 0;
  GILL_CHECK_HIP(hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_coop_giveups), sizeof(n)));
  if (n) {
    const unsigned zero = 0;
    GILL_CHECK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_coop_giveups), &zero, sizeof(zero)));
  }
  *count = n;
  return 0;
}

template <int NWV, int BN, int CONV, int EPI, int STAGES, int KT, int MI>
static int gemm_launch_inst(const GemmDev& d, dim3 grid, hipStream_t s) {
  static bool attr_set = false;
  constexpr int smem = STAGES * ((NWV / 2) * MI * 16 * KT + BN * KT) * (int)sizeof(bf16_t);
  if (!attr_set) {
    GILL_CHECK_HIP(hipFuncSetAttribute((const void*)gemm_kernel<NWV, BN, CONV, EPI, STAGES, KT, MI>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, smem));
    attr_set = true;
  }
  hipLaunchKernelGGL((gemm_kernel<NWV, BN, CONV, EPI, STAGES, KT, MI>), grid, dim3(NWV * 64), smem, s, d);
  GILL_CHECK_HIP(hipGetLastError());
  return 0;
}

// The gemm_kernel instantiations that exist: (NWV, BN, CONV, EPI, STAGES, KT, MI).  A plan names one of them or the launch is refused.
#define GEMM_KERNELS(X) \
  /* STREAM64: 128 x 64, 6-deep ring */ \
  X(8, 64, 0, 0, 6, 64, 2) X(8, 64, 0, 2, 6, 64, 2) X(8, 64, 0, 3, 6, 64, 2) \
  /* plain, 128 wide: 64-row two-wave, 128-row four-wave, 64-row four-wave (3-deep), 128-row eight-wave (GEGLU / QKV) */ \
  X(2, 128, 0, 0, 2, 64, 4) X(4, 128, 0, 0, 2, 64, 4) X(4, 128, 0, 0, 3, 64, 2) \
  X(2, 128, 0, 1, 2, 64, 4) X(4, 128, 0, 1, 2, 64, 4) X(8, 128, 0, 1, 2, 64, 2) \
  X(4, 128, 0, 2, 2, 64, 4) \
  X(2, 128, 0, 3, 2, 64, 4) X(4, 128, 0, 3, 2, 64, 4) X(4, 128, 0, 3, 3, 64, 2) X(8, 128, 0, 3, 2, 64, 2) \
  X(2, 128, 0, 4, 2, 64, 4) X(4, 128, 0, 4, 2, 64, 4) X(4, 128, 0, 4, 3, 64, 2) \
  /* convolutions, 128 wide */ \
  X(4, 128, 1, 0, 2, 64, 4) X(4, 128, 1, 2, 2, 64, 4) X(4, 128, 2, 0, 2, 64, 4) X(4, 128, 2, 2, 2, 64, 4) X(4, 128, 3, 0, 2, 64, 4) X(4, 128, 3, 2, 2, 64, 4) \
  /* plain, 160 wide: the same tiles + the ping-pong ones (eight waves, 3-deep: 128 / 256 rows) */ \
  X(2, 160, 0, 0, 2, 64, 4) X(4, 160, 0, 0, 2, 64, 2) X(4, 160, 0, 0, 2, 64, 4) \
  X(4, 160, 0, 2, 2, 64, 4) X(8, 160, 0, 2, 3, 64, 2) X(8, 160, 0, 2, 3, 64, 4) \
  X(2, 160, 0, 3, 2, 64, 4) X(4, 160, 0, 3, 2, 64, 4) X(8, 160, 0, 3, 3, 64, 2) X(8, 160, 0, 3, 3, 64, 4) \
  X(2, 160, 0, 4, 2, 64, 4) X(4, 160, 0, 4, 2, 64, 2) X(4, 160, 0, 4, 2, 64, 4) X(8, 160, 0, 4, 3, 64, 2) X(8, 160, 0, 4, 3, 64, 4) \
  X(2, 160, 0, 5, 2, 64, 4) X(4, 160, 0, 5, 2, 64, 2) X(4, 160, 0, 5, 2, 64, 4) X(4, 160, 0, 5, 3, 64, 2) X(8, 160, 0, 5, 3, 64, 2) \
  /* convolutions, 160 wide: four-wave and ping-pong, + the in-kernel GroupNorm finish (EPI 6) */ \
  X(4, 160, 1, 0, 2, 64, 4) X(8, 160, 1, 0, 3, 64, 2) X(8, 160, 1, 0, 3, 64, 4) X(4, 160, 1, 2, 2, 64, 4) X(8, 160, 1, 2, 3, 64, 2) X(8, 160, 1, 2, 3, 64, 4) \
  X(8, 160, 1, 6, 3, 64, 2) X(8, 160, 1, 6, 3, 64, 4) \
  X(4, 160, 2, 0, 2, 64, 4) X(8, 160, 2, 0, 3, 64, 2) X(8, 160, 2, 0, 3, 64, 4) X(4, 160, 2, 2, 2, 64, 4) X(8, 160, 2, 2, 3, 64, 2) X(8, 160, 2, 2, 3, 64, 4) \
  X(4, 160, 3, 0, 2, 64, 4) X(8, 160, 3, 0, 3, 64, 2) X(8, 160, 3, 0, 3, 64, 4) X(4, 160, 3, 2, 2, 64, 4) X(8, 160, 3, 2, 3, 64, 2) X(8, 160, 3, 2, 3, 64, 4)

static int gemm_dispatch(const GemmPlan& p, const GemmDev& d, dim3 grid, hipStream_t s) {
#define GEMM_KERNEL_CASE(NWV, BN, CONV, EPI, STAGES, KT, MI)                                                                                    \
  if (p.k_nwv == NWV && p.k_bn == BN && p.k_conv == CONV && p.k_epi == EPI && p.k_stages == STAGES && p.k_kt == KT && p.k_mi == MI)             \
    return gemm_launch_inst<NWV, BN, CONV, EPI, STAGES, KT, MI>(d, grid, s);
  GEMM_KERNELS(GEMM_KERNEL_CASE)
#undef GEMM_KERNEL_CASE
  GILL_REQUIRE(false, "internal: no kernel for this plan");
  return -2;
}

// the record behind gemm_plan_log_take() (gemm_plan.h): a ring of the most recent dispatched plans, per thread
static thread_local GemmPlan g_plan_log[GEMM_PLAN_LOG_CAP];
static thread_local unsigned g_plan_log_launched = 0;

int gemm_launch(const GemmArgs& a, hipStream_t s) {
  GemmPlan p;
  GILL_TRY(gemm_plan(a, gemm_env_default(), &p));
  GemmDev d;
  d.a = a;
  d.zero = gill_zero_page();
  GILL_REQUIRE(d.zero != nullptr, "zero page unavailable");
  d.a.splitk = p.splitk;
  const GemmArgs red = d.a;       // what the split-K reducer sees: the output tensor, whatever the conv kernel's row space is
  d.a.M = p.M;
  d.a.rows_per_batch = p.rows_per_batch;
  d.ksteps = p.ksteps; d.ksteps_per_split = p.ksteps_per_split;
  d.tiles_n = p.tiles_n; d.npw = p.npw; d.groups_n = p.groups_n;
  d.nwv = p.nwv; d.mi = p.mi; d.kt = p.kt;
  d.n_major = p.n_major; d.tiles_m = p.tiles_m; d.xb_m = p.xb_m; d.xb_n = p.xb_n;
  GILL_TRY(gemm_dispatch(p, d, dim3(p.grid_x, p.grid_y, p.grid_z), s));
  g_plan_log[g_plan_log_launched++ % GEMM_PLAN_LOG_CAP] = p;
  if (p.reduce) return gemm_splitk_reduce_launch(red, s);
  return 0;
}

int gemm_plan_log_take(GemmPlan* out, int cap, int* launched) {
  const unsigned total = g_plan_log_launched;
  unsigned n = total < GEMM_PLAN_LOG_CAP ? total : GEMM_PLAN_LOG_CAP;
  if (cap < 0) cap = 0;
  if (n > (unsigned)cap) n = (unsigned)cap;
  for (unsigned i = 0; i < n; ++i) out[i] = g_plan_log[(total - n + i) % GEMM_PLAN_LOG_CAP];
  *launched = (int)total;
  g_plan_log_launched = 0;
  return (int)n;
}
