// Retrieval on the device (include/gill_amd.h "Retrieval"): a resident bf16 index in an MFMA-blocked layout, one fused score + top-k pass over
// it for up to 16 queries, and the merge of the per-wave candidate lists.  Stands for gill/models.py:671-696 (ret_emb -> emb_matrix @ ret_emb.T
// -> seen penalty -> topk) and :895-900 (unit rows scaled by exp(logit_scale)).
//
// LAYOUT.  dim is zero-padded to KS = ceil(dim / 32) k-steps.  Rows are stored in 16-row tiles; a tile is KS consecutive 1 KiB blocks, block s
// holding the 16 x 32 slice k = 32 s .. 32 s + 31 as the 64 lanes' 16-byte A fragments of v_mfma_f32_16x16x32_bf16, in lane order: lane l has
// row (l & 15), k = 32 s + 8 (l >> 4) + j, j = 0..7.  Every load of the search is therefore one contiguous 1 KiB wave load that goes straight
// into the matrix instruction: no LDS staging, no shuffle, every matrix byte read once per pass.
//
// SEARCH.  2048 waves at most per launch (8 per CU on a 256-CU part), each over one contiguous slab of tiles.  The queries (bf16, B operand, column = query)
// stay in registers.  Each wave keeps, per query, a list of its k best in LDS, unsorted, with its worst entry marked; a lane compares its four
// accumulators with its query's worst kept score first, and only a wave in which some lane passes takes the insertion path: rows in ascending
// order, the 16 queries in parallel, one lane per list — the worst entry is replaced and the new worst found by k independent reads.  The
// lists are sorted once, by rank, as they leave (score desc, index asc).  Rows arrive in ascending order and a tie goes to the lower index, so the filter is a
// strict >.  The seen penalty only lowers a score: it is looked up on the insertion path, after the filter on the raw score.  The lists go to the
// handle's workspace; a second launch (one workgroup per query) merges them: the k lists with the best heads, then the k best of their entries.
// Nothing waits on another workgroup and nothing is atomic: the result does not depend on the grid.
//
// PREFIX.  A wave's slab is short (1328 rows of a 2.7 M-row index), so a list that starts empty keeps inserting: k ln(n / k) with a small n, in
// every one of 2048 waves.  From 1024 tiles on, the first 1 / 64 of the tiles is therefore searched and merged first (two small launches), and the
// k-th score of that prefix is the floor every list of the main pass starts its filter from.  The floor is exact, not a heuristic: k rows of
// the prefix score at least that much (penalties included) and all of them have lower indices than any row of the main pass, so a later row
// must beat it strictly.  Every matrix byte is still read once: the main pass starts behind the prefix and the last merge takes the lists of both.
#include "../../include/gill_amd.h"
#include "common.h"
#include <limits.h>
#include <math.h>
#include <new>

#define RET_MAX_LISTS 2048      // per-wave lists of one launch (the prefix and the main pass have that many each at most)
#define RET_MIN_TILES 4         // a wave's slab is at least this many tiles (while there are tiles); 2 in the prefix
#define RET_PREFIX_MIN 1024     // tiles from which the prefix pass runs
#define RET_PREFIX_DIV 64       // ... over ntiles / 64 tiles
#define RET_KMAX 32
#define RET_EMAX 64
#define RET_EMPTY INT_MAX       // index of an empty list slot (rows are < 2^31 - 1)

struct gill_ret_index {
  int dim = 0, KS = 0;
  int64_t capacity = 0, size = 0;
  uint4* mat = nullptr;         // [tiles][KS][64] 16-byte fragments
  uint4* qfrag = nullptr;       // [KS][64]: the B operand of one chunk of 16 queries
  float* ws_s = nullptr;        // [16][lists][k]
  int* ws_i = nullptr;
  float* floor_s = nullptr;     // [16][k]: the prefix pass's own top k
  int64_t* floor_i = nullptr;
};

// lists [0, wa) scan tiles [0, pa) (the prefix; none below RET_PREFIX_MIN tiles), lists [wa, wa + wb) tiles [pa, ntiles)
struct RetGeometry {
  int64_t ntiles, pa, tpl_a, tpl_b;
  int wa, wb;
};

static void ret_split(int64_t tiles, int min_tiles, int* nlists, int64_t* tiles_per_list) {
  int64_t w = cdiv64(tiles, min_tiles);
  if (w < 1) w = 1;
  if (w > RET_MAX_LISTS) w = RET_MAX_LISTS;
  w = cdiv64(w, 4) * 4;
  const int64_t tpl = cdiv64(tiles, w);
  *nlists = (int)w;
  *tiles_per_list = tpl < 1 ? 1 : tpl;
}

static RetGeometry ret_geometry(int64_t size) {
  RetGeometry g;
  g.ntiles = cdiv64(size, 16);
  g.pa = g.ntiles >= RET_PREFIX_MIN ? g.ntiles / RET_PREFIX_DIV : 0;
  g.wa = 0; g.tpl_a = 1;
  if (g.pa > 0) ret_split(g.pa, 2, &g.wa, &g.tpl_a);
  ret_split(g.ntiles - g.pa, RET_MIN_TILES, &g.wb, &g.tpl_b);
  return g;
}

// ---------------------------------------------------------------------------------------------------------------- add / rows
__device__ __forceinline__ void ret_load8(const void* rows, int dtype, size_t off, float* x) {
  if (dtype == GILL_DTYPE_F32) {
    const float4 a = *(const float4*)((const float*)rows + off), b = *(const float4*)((const float*)rows + off + 4);
    x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
  } else {
    const uint4 v = *(const uint4*)((const uint16_t*)rows + off);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (dtype == GILL_DTYPE_BF16) {
        x[2 * i] = bf2f((bf16_t)(w[i] & 0xffffu)); x[2 * i + 1] = bf2f((bf16_t)(w[i] >> 16));
      } else {
        x[2 * i] = (float)__builtin_bit_cast(_Float16, (uint16_t)(w[i] & 0xffffu));
        x[2 * i + 1] = (float)__builtin_bit_cast(_Float16, (uint16_t)(w[i] >> 16));
      }
    }
  }
}

// one wave per row; a lane holds the 8-column groups lane and lane + 64 (dim <= 1024)
__global__ __launch_bounds__(256) void ret_add_kernel(const void* rows, int dtype, int64_t n, int dim, int KS, int64_t first, int normalize,
                                                      float scale, uint4* mat) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const int groups = dim >> 3;
  float x[2][8];
  float ss = 0.f;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int grp = lane + 64 * h;
    if (grp < groups) {
      ret_load8(rows, dtype, (size_t)i * dim + 8 * grp, x[h]);
#pragma unroll
      for (int j = 0; j < 8; ++j) ss = fmaf(x[h][j], x[h][j], ss);
    }
  }
  float f = 1.f;
  if (normalize) {
    ss = wave_sum(ss);
    f = ss > 0.f ? scale / sqrtf(ss) : 0.f;      // a zero row stays zero
  }
  const int64_t r = first + i;
  const size_t tile = (size_t)(r >> 4);
  const int rr = (int)(r & 15);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int grp = lane + 64 * h;
    if (grp < groups) {
      uint4 o;
      if (normalize) {
        o.x = pack_bf2(x[h][0] * f, x[h][1] * f); o.y = pack_bf2(x[h][2] * f, x[h][3] * f);
        o.z = pack_bf2(x[h][4] * f, x[h][5] * f); o.w = pack_bf2(x[h][6] * f, x[h][7] * f);
      } else {
        o.x = pack_bf2(x[h][0], x[h][1]); o.y = pack_bf2(x[h][2], x[h][3]);
        o.z = pack_bf2(x[h][4], x[h][5]); o.w = pack_bf2(x[h][6], x[h][7]);
      }
      mat[(tile * KS + (grp >> 2)) * 64 + (grp & 3) * 16 + rr] = o;
    }
  }
}

__global__ __launch_bounds__(256) void ret_rows_kernel(const uint4* mat, int64_t first, int64_t n, int dim, int KS, uint4* out) {
  const int groups = dim >> 3;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n * groups) return;
  const int64_t i = t / groups;
  const int grp = (int)(t - i * groups);
  const int64_t r = first + i;
  out[t] = mat[((size_t)(r >> 4) * KS + (grp >> 2)) * 64 + (grp & 3) * 16 + (int)(r & 15)];
}

// ---------------------------------------------------------------------------------------------------------------- queries -> B operand
// One wave per query slot c of the chunk: bf16(q / ||q||_2) (or bf16(q)) into the fragment order lane = 16 (group & 3) + c of k-step group >> 2;
// slots >= Q and columns >= dim are zero.  A zero query stays zero.
__global__ __launch_bounds__(64) void ret_query_kernel(const float* queries, int Q, int dim, int KS, int normalize, uint4* qfrag) {
  const int c = blockIdx.x, lane = threadIdx.x;
  const int groups = dim >> 3;
  float x[2][8];
  float ss = 0.f;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int grp = lane + 64 * h;
#pragma unroll
    for (int j = 0; j < 8; ++j) x[h][j] = 0.f;
    if (c < Q && grp < groups) {
      ret_load8(queries, GILL_DTYPE_F32, (size_t)c * dim + 8 * grp, x[h]);
#pragma unroll
      for (int j = 0; j < 8; ++j) ss = fmaf(x[h][j], x[h][j], ss);
    }
  }
  if (normalize) {
    ss = wave_sum(ss);
    const float nrm = sqrtf(ss);
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int j = 0; j < 8; ++j) x[h][j] = ss > 0.f ? x[h][j] / nrm : 0.f;
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int grp = lane + 64 * h;
    if (grp < 4 * KS) {
      uint4 o;
      o.x = pack_bf2(x[h][0], x[h][1]); o.y = pack_bf2(x[h][2], x[h][3]);
      o.z = pack_bf2(x[h][4], x[h][5]); o.w = pack_bf2(x[h][6], x[h][7]);
      qfrag[(grp >> 2) * 64 + (grp & 3) * 16 + c] = o;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- search
struct RetSearchArgs {
  const uint4* mat;
  const uint4* qfrag;
  const int64_t* exclude;   // (Q, E) of this chunk, or null
  const float* floor_s;     // [16][k]: list q of the prefix pass, or null
  float* ws_s;              // [16][nlists][k]
  int* ws_i;
  int64_t size, tile_begin, tile_end, tiles_per_list;   // this launch: list j scans tiles tile_begin + [j, j + 1) * tiles_per_list, up to tile_end
  int KS, Q, k, E, nlists, list_base;                   // its lists are list_base + j of the workspace's nlists
  float penalty;
};

#define RET_LD 33   // list stride in LDS words (odd: the 16 lists' slot j fall in 16 banks); word 32 of a list: its worst entry's score | slot

__device__ __forceinline__ void ret_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The insertion path of one tile (rare after warm-up).  acc: this lane's four scores (query lane & 15, rows 4 (lane >> 4) + reg), masked.
__device__ __forceinline__ float ret_insert_tile(const int* lex, int E, float penalty, int Q, int k, float floor, float* ls, int* li,
                                                 f32x4 acc, int64_t row0, float thr) {
  const int lane = threadIdx.x & 63, q = lane & 15, g = lane >> 4;
#pragma unroll 1
  for (int gg = 0; gg < 4; ++gg) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const float raw = acc[reg];
      const bool c = (g == gg) && raw > thr;
      if (__ballot(c) == 0) continue;
      if (c) {
        const int row = (int)(row0 + 4 * gg + reg);
        float v = raw;
        bool seen = false;
        for (int e = 0; e < E; ++e) seen = seen || (lex[q * E + e] == row);
        if (seen) v -= penalty;
        if (v > thr) {                     // every entry has a lower index: an equal score keeps its place
          const int wp = li[q * RET_LD + RET_KMAX];       // replace the worst entry, then find the new worst: k independent reads
          ls[q * RET_LD + wp] = v;
          li[q * RET_LD + wp] = row;
          float wsc = INFINITY;
          int wix = -1, wpos = 0;
          for (int j0 = 0; j0 < k; j0 += 4) {       // four entries per trip, loaded together (the last one again past k: harmless)
            float sv[4];
            int iv[4], jv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              jv[u] = j0 + u < k ? j0 + u : k - 1;
              sv[u] = ls[q * RET_LD + jv[u]];
              iv[u] = li[q * RET_LD + jv[u]];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const bool w = sv[u] < wsc || (sv[u] == wsc && iv[u] > wix);
              wsc = w ? sv[u] : wsc; wix = w ? iv[u] : wix; wpos = w ? jv[u] : wpos;
            }
          }
          ls[q * RET_LD + RET_KMAX] = wsc;
          li[q * RET_LD + RET_KMAX] = wpos;
        }
      }
      ret_wave_sync();
      if (q < Q) thr = fmaxf(floor, ls[q * RET_LD + RET_KMAX]);
    }
  }
  return thr;
}

template <int KSMAX, bool EXACT>
__global__ __launch_bounds__(256) void ret_search_kernel(const RetSearchArgs a) {
  __shared__ float l_s[4][16 * RET_LD];
  __shared__ int l_i[4][16 * RET_LD];
  __shared__ int l_ex[16 * RET_EMAX];         // the chunk's seen rows (-1: none), shared by the four waves
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int q = lane & 15, g = lane >> 4;
  const int list = blockIdx.x * 4 + wv;
  const int KS = EXACT ? KSMAX : a.KS;
  constexpr bool PREFETCH = KSMAX <= 8;       // two tiles in flight per wave; from 16 k-steps on one tile is 16 KiB already
  constexpr int GROUP = KSMAX < 16 ? KSMAX : 16;
  float* ls = l_s[wv];       // (plain accesses: every hand-over between lanes goes through ret_wave_sync's fences)
  int* li = l_i[wv];
  for (int j = g; j < RET_KMAX; j += 4) { ls[q * RET_LD + j] = -INFINITY; li[q * RET_LD + j] = RET_EMPTY; }
  if (g == 0) { ls[q * RET_LD + RET_KMAX] = -INFINITY; li[q * RET_LD + RET_KMAX] = 0; }
  for (int i = threadIdx.x; i < a.Q * a.E; i += 256) {
    const int64_t r = a.exclude[i];
    l_ex[i] = (r >= 0 && r < a.size) ? (int)r : -1;
  }
  __syncthreads();

  bf16x8 b[KSMAX];
#pragma unroll
  for (int s = 0; s < KSMAX; ++s) {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (EXACT || s < KS) v = a.qfrag[s * 64 + lane];
    b[s] = __builtin_bit_cast(bf16x8, v);
  }
  // the prefix's k-th score: k rows of lower index score at least this, so only a strictly larger score is a candidate
  const float floor = (a.floor_s && q < a.Q) ? a.floor_s[q * a.k + a.k - 1] : -INFINITY;
  float thr = q < a.Q ? floor : INFINITY;       // unused query columns never pass the filter

  int64_t t0 = a.tile_begin + (int64_t)list * a.tiles_per_list;
  int64_t t1 = t0 + a.tiles_per_list;
  if (t1 > a.tile_end) t1 = a.tile_end;
  if (t0 > t1) t0 = t1;
  const uint4* p = a.mat + ((size_t)t0 * KS) * 64 + lane;
  const size_t tile_stride = (size_t)KS * 64;

  if constexpr (PREFETCH) {
    uint4 cur[KSMAX], nxt[KSMAX];
#pragma unroll
    for (int s = 0; s < KSMAX; ++s) cur[s] = nxt[s] = make_uint4(0, 0, 0, 0);
    if (t0 < t1) {
#pragma unroll
      for (int s = 0; s < KSMAX; ++s) if (EXACT || s < KS) cur[s] = p[s * 64];
    }
    for (int64_t t = t0; t < t1; ++t) {
      p += tile_stride;
      if (t + 1 < t1) {
#pragma unroll
        for (int s = 0; s < KSMAX; ++s) if (EXACT || s < KS) nxt[s] = p[s * 64];
      }
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < KSMAX; ++s)
        if (EXACT || s < KS) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, cur[s]), b[s], acc, 0, 0, 0);
      const int64_t row0 = t * 16;
      if (row0 + 16 > a.size) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) if (row0 + 4 * g + reg >= a.size) acc[reg] = -INFINITY;
      }
      const bool hit = acc[0] > thr || acc[1] > thr || acc[2] > thr || acc[3] > thr;
      if (__ballot(hit) != 0) thr = ret_insert_tile(l_ex, a.E, a.penalty, a.Q, a.k, floor, ls, li, acc, row0, thr);
#pragma unroll
      for (int s = 0; s < KSMAX; ++s) cur[s] = nxt[s];
    }
  } else {
    for (int64_t t = t0; t < t1; ++t) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s0 = 0; s0 < KSMAX; s0 += GROUP) {
        uint4 cur[GROUP];
#pragma unroll
        for (int s = 0; s < GROUP; ++s) if (EXACT || s0 + s < KS) cur[s] = p[(s0 + s) * 64];
#pragma unroll
        for (int s = 0; s < GROUP; ++s)
          if (EXACT || s0 + s < KS) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, cur[s]), b[s0 + s], acc, 0, 0, 0);
      }
      p += tile_stride;
      const int64_t row0 = t * 16;
      if (row0 + 16 > a.size) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) if (row0 + 4 * g + reg >= a.size) acc[reg] = -INFINITY;
      }
      const bool hit = acc[0] > thr || acc[1] > thr || acc[2] > thr || acc[3] > thr;
      if (__ballot(hit) != 0) thr = ret_insert_tile(l_ex, a.E, a.penalty, a.Q, a.k, floor, ls, li, acc, row0, thr);
    }
  }

  // the lists leave sorted: an entry goes to the slot of its rank (equal empty entries: by slot)
  ret_wave_sync();
  for (int j = g; j < a.k; j += 4) {
    const float s = ls[q * RET_LD + j];
    const int i = li[q * RET_LD + j];
    int rank = 0;
#pragma unroll 4
    for (int jj = 0; jj < a.k; ++jj) {
      const float s2 = ls[q * RET_LD + jj];
      const int i2 = li[q * RET_LD + jj];
      rank += (s2 > s || (s2 == s && (i2 < i || (i2 == i && jj < j)))) ? 1 : 0;
    }
    const size_t o = ((size_t)q * a.nlists + a.list_base + list) * a.k + rank;
    a.ws_s[o] = s;
    a.ws_i[o] = i;
  }
}

// ---------------------------------------------------------------------------------------------------------------- merge
__device__ __forceinline__ bool ret_better(float s1, int i1, float s2, int i2) { return s1 > s2 || (s1 == s2 && i1 < i2); }

// Block-wide argmax by (score descending, index ascending) of one candidate per thread; every thread returns the winner.  The 16 lanes of a
// DPP row on the VALU (as row16_sum), the 16 rows of the block through LDS.  Two barriers.
template <int CTRL>
__device__ __forceinline__ void ret_dpp_best(float& s, int& i) {
  const float s2 = dpp_row_mov<CTRL>(s);
  const int i2 = __builtin_amdgcn_update_dpp(0, i, CTRL, 0xf, 0xf, true);
  if (ret_better(s2, i2, s, i)) { s = s2; i = i2; }
}
__device__ __forceinline__ void ret_block_best(float& ws, int& wi, float* r_s, int* r_i) {
  ret_dpp_best<0xB1>(ws, wi);      // quad_perm [1,0,3,2]
  ret_dpp_best<0x4E>(ws, wi);      // quad_perm [2,3,0,1]
  ret_dpp_best<0x141>(ws, wi);     // row_half_mirror
  ret_dpp_best<0x140>(ws, wi);     // row_mirror: every lane of the row holds the row's best
  if ((threadIdx.x & 15) == 0) { r_s[threadIdx.x >> 4] = ws; r_i[threadIdx.x >> 4] = wi; }
  __syncthreads();
  ws = r_s[0]; wi = r_i[0];
#pragma unroll
  for (int w = 1; w < 16; ++w) if (ret_better(r_s[w], r_i[w], ws, wi)) { ws = r_s[w]; wi = r_i[w]; }
  __syncthreads();
}

// One workgroup per query, over the first `count` of the workspace's nlists lists.  Every list is sorted, so a row of the top k sits in one of
// the k lists with the best heads: k heads beat every entry of any other list.  Phase 1 picks those lists, k rounds of a block-wide argmax over
// the heads, which stay in registers (thread t owns lists t, t + 256, ...: at most 16).  Phase 2 loads their k x k entries, at most four per
// thread, and picks the k best the same way.  No memory access inside either loop but the result store.  Row indices are unique over the lists,
// so the winning index names its owner; exhausted lists offer (-inf, RET_EMPTY): such a winner is written as index -1.
__global__ __launch_bounds__(256) void ret_merge_kernel(const float* ws_s, const int* ws_i, int nlists, int count, int k, float* scores_out,
                                                        int64_t* idx_out) {
  __shared__ float r_s[16];
  __shared__ int r_i[16];
  __shared__ int sel[RET_KMAX];
  __shared__ float o_s[RET_KMAX];     // the results, stored once at the end: a global store in front of every barrier would be waited for
  __shared__ int o_i[RET_KMAX];
  const int qq = blockIdx.x, t = threadIdx.x;
  const float* S = ws_s + (size_t)qq * nlists * k;
  const int* I = ws_i + (size_t)qq * nlists * k;
  constexpr int OWN = 2 * RET_MAX_LISTS / 256;
  float hs[OWN];
  int hi[OWN];
#pragma unroll
  for (int m = 0; m < OWN; ++m) {
    const int L = t + 256 * m;
    hs[m] = -INFINITY; hi[m] = RET_EMPTY;
    if (L < count) { hs[m] = S[(size_t)L * k]; hi[m] = I[(size_t)L * k]; }
  }
  for (int r = 0; r < k; ++r) {
    float bs = -INFINITY;
    int bi = RET_EMPTY;
#pragma unroll
    for (int m = 0; m < OWN; ++m) if (ret_better(hs[m], hi[m], bs, bi)) { bs = hs[m]; bi = hi[m]; }
    float ws = bs;
    int wi = bi;
    ret_block_best(ws, wi, r_s, r_i);
    if (wi == RET_EMPTY) {
      if (t == 0) sel[r] = -1;
    } else if (wi == bi) {
#pragma unroll
      for (int m = 0; m < OWN; ++m)
        if (hi[m] == wi) { sel[r] = t + 256 * m; hs[m] = -INFINITY; hi[m] = RET_EMPTY; }
    }
  }
  __syncthreads();
  float cs[4];
  int ci[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int e = t + 256 * u;
    cs[u] = -INFINITY; ci[u] = RET_EMPTY;
    if (e < k * k) {
      const int L = sel[e / k];
      if (L >= 0) { cs[u] = S[(size_t)L * k + e % k]; ci[u] = I[(size_t)L * k + e % k]; }
    }
  }
  for (int r = 0; r < k; ++r) {
    float bs = -INFINITY;
    int bi = RET_EMPTY;
#pragma unroll
    for (int u = 0; u < 4; ++u) if (ret_better(cs[u], ci[u], bs, bi)) { bs = cs[u]; bi = ci[u]; }
    float ws = bs;
    int wi = bi;
    ret_block_best(ws, wi, r_s, r_i);
    if (t == 0) { o_s[r] = ws; o_i[r] = wi; }
    if (wi != RET_EMPTY && wi == bi) {
#pragma unroll
      for (int u = 0; u < 4; ++u) if (ci[u] == wi) { cs[u] = -INFINITY; ci[u] = RET_EMPTY; }
    }
  }
  __syncthreads();
  if (t < k) {
    scores_out[(size_t)qq * k + t] = o_i[t] == RET_EMPTY ? -INFINITY : o_s[t];
    idx_out[(size_t)qq * k + t] = o_i[t] == RET_EMPTY ? (int64_t)-1 : (int64_t)o_i[t];
  }
}

// ---------------------------------------------------------------------------------------------------------------- host
static int ret_storage(gill_ret_index* h, hipStream_t s) {
  if (h->mat) return 0;
  const size_t tiles = (size_t)cdiv64(h->capacity, 16);
  const size_t bytes = tiles * h->KS * 64 * sizeof(uint4);
  GILL_CHECK_HIP(hipMalloc((void**)&h->mat, bytes ? bytes : 16));
  GILL_CHECK_HIP(hipMemsetAsync(h->mat, 0, bytes, s));      // the column padding and the rows past size read as zero
  const RetGeometry g = ret_geometry(h->capacity);      // (the list count never falls as the index grows)
  const size_t nlists = (size_t)g.wa + g.wb;
  GILL_CHECK_HIP(hipMalloc((void**)&h->ws_s, sizeof(float) * 16 * nlists * RET_KMAX));
  GILL_CHECK_HIP(hipMalloc((void**)&h->ws_i, sizeof(int) * 16 * nlists * RET_KMAX));
  GILL_CHECK_HIP(hipMalloc((void**)&h->floor_s, sizeof(float) * 16 * RET_KMAX));
  GILL_CHECK_HIP(hipMalloc((void**)&h->floor_i, sizeof(int64_t) * 16 * RET_KMAX));
  GILL_CHECK_HIP(hipMalloc((void**)&h->qfrag, sizeof(uint4) * h->KS * 64));
  return 0;
}

extern "C" int gill_ret_index_create(gill_ret_index** out, int dim, int64_t capacity) {
  GILL_REQUIRE(out != nullptr, "ret_index_create: out is null");
  *out = nullptr;
  GILL_REQUIRE(dim >= 8 && dim % 8 == 0 && dim <= 1024, "ret_index_create: dim must be a multiple of 8, at most 1024");
  GILL_REQUIRE(capacity >= 1 && capacity < 2147483647LL, "ret_index_create: 1 <= capacity < 2^31 - 1");
  gill_ret_index* h = new (std::nothrow) gill_ret_index();
  GILL_REQUIRE(h != nullptr, "ret_index_create: out of host memory");
  h->dim = dim; h->KS = cdiv(dim, 32); h->capacity = capacity;
  *out = h;       // the device memory is allocated by the first add / search
  return 0;
}

extern "C" void gill_ret_index_destroy(gill_ret_index* h) {
  if (!h) return;
  if (h->mat) (void)hipFree(h->mat);
  if (h->ws_s) (void)hipFree(h->ws_s);
  if (h->ws_i) (void)hipFree(h->ws_i);
  if (h->qfrag) (void)hipFree(h->qfrag);
  if (h->floor_s) (void)hipFree(h->floor_s);
  if (h->floor_i) (void)hipFree(h->floor_i);
  delete h;
}

extern "C" int64_t gill_ret_index_size(const gill_ret_index* h) { return h ? h->size : -1; }

extern "C" int gill_ret_index_slabs(const gill_ret_index* h, int64_t* first_row, int* nlists, int64_t* rows_per_list) {
  GILL_REQUIRE(h != nullptr, "ret_index_slabs: null handle");
  const RetGeometry g = ret_geometry(h->size);
  if (first_row) *first_row = 16 * g.pa;
  if (nlists) *nlists = g.wb;
  if (rows_per_list) *rows_per_list = 16 * g.tpl_b;
  return 0;
}

extern "C" int gill_ret_index_add(gill_ret_index* h, const void* rows, int dtype, int64_t n, int normalize, float scale, void* stream) {
  GILL_REQUIRE(h != nullptr, "ret_index_add: null handle");
  GILL_REQUIRE(n >= 0, "ret_index_add: n < 0");
  GILL_REQUIRE(dtype == GILL_DTYPE_BF16 || dtype == GILL_DTYPE_F32 || dtype == GILL_DTYPE_F16, "ret_index_add: dtype is GILL_DTYPE_BF16, _F32 or _F16");
  GILL_REQUIRE(n <= h->capacity - h->size, "ret_index_add: more rows than the capacity leaves");
  if (n == 0) return 0;
  GILL_REQUIRE(rows != nullptr && ((uintptr_t)rows & 15) == 0, "ret_index_add: rows must be a 16-byte aligned device pointer");
  hipStream_t s = (hipStream_t)stream;
  GILL_TRY(ret_storage(h, s));
  ret_add_kernel<<<dim3((unsigned)cdiv64(n, 4)), dim3(256), 0, s>>>(rows, dtype, n, h->dim, h->KS, h->size, normalize ? 1 : 0, scale, h->mat);
  GILL_CHECK_HIP(hipGetLastError());
  h->size += n;
  return 0;
}

extern "C" int gill_ret_index_rows(gill_ret_index* h, int64_t first, int64_t n, void* out_bf16, void* stream) {
  GILL_REQUIRE(h != nullptr, "ret_index_rows: null handle");
  GILL_REQUIRE(first >= 0 && n >= 0 && first <= h->size && n <= h->size - first, "ret_index_rows: [first, first + n) must lie inside the index");
  if (n == 0) return 0;
  GILL_REQUIRE(out_bf16 != nullptr && ((uintptr_t)out_bf16 & 15) == 0, "ret_index_rows: out must be a 16-byte aligned device pointer");
  hipStream_t s = (hipStream_t)stream;
  const int64_t work = n * (h->dim >> 3);
  ret_rows_kernel<<<dim3((unsigned)cdiv64(work, 256)), dim3(256), 0, s>>>(h->mat, first, n, h->dim, h->KS, (uint4*)out_bf16);
  GILL_CHECK_HIP(hipGetLastError());
  return 0;
}

template <int KSMAX>
static void ret_search_launch_ks(const RetSearchArgs& a, int lists, hipStream_t s) {
  const dim3 grid(lists / 4), block(256);
  if (a.KS == KSMAX) ret_search_kernel<KSMAX, true><<<grid, block, 0, s>>>(a);
  else ret_search_kernel<KSMAX, false><<<grid, block, 0, s>>>(a);
}

static void ret_search_launch(const RetSearchArgs& a, int lists, hipStream_t s) {
  if (a.KS <= 1) ret_search_launch_ks<1>(a, lists, s);
  else if (a.KS <= 2) ret_search_launch_ks<2>(a, lists, s);
  else if (a.KS <= 4) ret_search_launch_ks<4>(a, lists, s);
  else if (a.KS <= 8) ret_search_launch_ks<8>(a, lists, s);
  else if (a.KS <= 16) ret_search_launch_ks<16>(a, lists, s);
  else ret_search_launch_ks<32>(a, lists, s);
}

extern "C" int gill_ret_index_search(gill_ret_index* h, const float* queries, int Q, int normalize, int k, const int64_t* exclude, int E,
                                     float penalty, float* scores_out, int64_t* idx_out, void* stream) {
  GILL_REQUIRE(h != nullptr, "ret_index_search: null handle");
  GILL_REQUIRE(Q >= 1, "ret_index_search: Q < 1");
  GILL_REQUIRE(k >= 1 && k <= RET_KMAX, "ret_index_search: 1 <= k <= 32");
  GILL_REQUIRE(E >= 0 && E <= RET_EMAX, "ret_index_search: 0 <= E <= 64");
  GILL_REQUIRE(queries != nullptr && ((uintptr_t)queries & 15) == 0, "ret_index_search: queries must be a 16-byte aligned device pointer");
  GILL_REQUIRE(scores_out != nullptr && idx_out != nullptr, "ret_index_search: outputs are null");
  hipStream_t s = (hipStream_t)stream;
  GILL_TRY(ret_storage(h, s));
  RetSearchArgs a;
  a.mat = h->mat; a.qfrag = h->qfrag; a.ws_s = h->ws_s; a.ws_i = h->ws_i;
  const RetGeometry g = ret_geometry(h->size);
  a.size = h->size; a.nlists = g.wa + g.wb;
  a.KS = h->KS; a.k = k; a.penalty = penalty;
  for (int q0 = 0; q0 < Q; q0 += 16) {       // one pass over the matrix per 16 queries
    const int Qc = Q - q0 < 16 ? Q - q0 : 16;
    a.Q = Qc;
    a.exclude = (exclude && E > 0) ? exclude + (size_t)q0 * E : nullptr;
    a.E = a.exclude ? E : 0;
    ret_query_kernel<<<dim3(16), dim3(64), 0, s>>>(queries + (size_t)q0 * h->dim, Qc, h->dim, h->KS, normalize ? 1 : 0, h->qfrag);
    a.floor_s = nullptr;
    if (g.pa > 0) {        // the prefix: its own lists, merged at once into the floor of the main pass
      a.tile_begin = 0; a.tile_end = g.pa; a.tiles_per_list = g.tpl_a; a.list_base = 0;
      ret_search_launch(a, g.wa, s);
      ret_merge_kernel<<<dim3(Qc), dim3(256), 0, s>>>(h->ws_s, h->ws_i, a.nlists, g.wa, k, h->floor_s, h->floor_i);
      a.floor_s = h->floor_s;
    }
    a.tile_begin = g.pa; a.tile_end = g.ntiles; a.tiles_per_list = g.tpl_b; a.list_base = g.wa;
    ret_search_launch(a, g.wb, s);
    ret_merge_kernel<<<dim3(Qc), dim3(256), 0, s>>>(h->ws_s, h->ws_i, a.nlists, a.nlists, k, scores_out + (size_t)q0 * k,
                                                    idx_out + (size_t)q0 * k);
    GILL_CHECK_HIP(hipGetLastError());
  }
  return 0;
}
