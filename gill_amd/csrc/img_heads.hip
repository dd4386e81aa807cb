// The image-block heads (include/gill_amd.h "Image-block heads"): what generate_for_images_and_texts does with the first [IMG] hidden state of a
// block (gill/models.py:671-676, :698-704) for n blocks in one launch, and the CLIP rerank score of the generated images (:733-751).
//
// HEADS.  One workgroup of 16 waves per block; nothing is shared between workgroups, so a block's outputs are a function of its own row and
// the weights alone: the same bits at any n, at any position of row_idx and on any run.  The gathered fp32 row is rounded to bf16 into LDS once
// (16 bytes per lane and trip).  The E + C output columns go to the waves in groups of four, round-robin; a lane walks K in 8-element groups
// lane, lane + 64, ... with one 16-byte weight load per column and group (four columns in flight), accumulates in fp32 in ascending k and the
// wave folds the 64 partials with the xor butterfly 32, 16, .. 1.  That order depends on D only.  The sums land in LDS with their bias; after
// one barrier every wave derives the squared norm from them in the same fixed order (lanes stride E, the same butterfly) and the workgroup's threads
// store y / ||y||; thread 0 does the softmax and the argmax of the at most four decision logits.  A workgroup reads (E + C) D 2 bytes of weights:
// every one after the first from L2.
//
// RERANK.  One wave per generated image: dot(v, r), |v|^2, |r|^2 with lanes striding E, the butterfly, dot / (|v| |r|); a zero row gives 0.
#include "../../include/gill_amd.h"
#include "common.h"
#include "ops.h"
#include <math.h>

#define IH_MAX_D 8192
#define IH_MAX_E 1024
#define IH_MAX_C 4
#define IH_COLS 4           // columns a wave has in flight
#define IH_WAVES 16         // waves of a workgroup: a block is one workgroup, so its waves are all the memory parallelism it has

struct ImgHeadsArgs {
  const float* hidden;
  const int* row_idx;
  const bf16_t* Wr;
  const float* br;
  const bf16_t* Wd;
  const float* bd;
  float* ret_emb;
  float* probs;
  int* choice;
  int64_t rows;
  int D, E, C;              // E = 0: no retrieval head, C = 0: no decision head
};

__device__ __forceinline__ float ih_dot8(const uint4 w, const uint4 x, float acc) {
  const uint32_t ww[4] = {w.x, w.y, w.z, w.w}, xx[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    acc = fmaf(bf2f((bf16_t)(ww[i] & 0xffffu)), bf2f((bf16_t)(xx[i] & 0xffffu)), acc);
    acc = fmaf(bf2f((bf16_t)(ww[i] >> 16)), bf2f((bf16_t)(xx[i] >> 16)), acc);
  }
  return acc;
}

__global__ __launch_bounds__(64 * IH_WAVES) void img_heads_kernel(const ImgHeadsArgs a) {
  __shared__ uint4 xs[IH_MAX_D / 8];               // the row as bf16
  __shared__ float ys[IH_MAX_E + IH_MAX_C];        // y (E), then z (C)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int groups = a.D >> 3;
  int64_t r = a.row_idx[blockIdx.x];
  r = r < 0 ? 0 : (r >= a.rows ? a.rows - 1 : r);
  const float* src = a.hidden + (size_t)r * a.D;
  for (int g = threadIdx.x; g < groups; g += 64 * IH_WAVES) {
    const float4 lo = *(const float4*)(src + 8 * g), hi = *(const float4*)(src + 8 * g + 4);
    uint4 o;
    o.x = pack_bf2(lo.x, lo.y); o.y = pack_bf2(lo.z, lo.w); o.z = pack_bf2(hi.x, hi.y); o.w = pack_bf2(hi.z, hi.w);
    xs[g] = o;
  }
  __syncthreads();

  const int ncols = a.E + a.C;
  for (int c0 = IH_COLS * wv; c0 < ncols; c0 += IH_COLS * IH_WAVES) {
    const bf16_t* w[IH_COLS];
    float acc[IH_COLS];
#pragma unroll
    for (int u = 0; u < IH_COLS; ++u) {
      const int c = c0 + u < ncols ? c0 + u : ncols - 1;      // past the end: the last column again, not stored
      w[u] = c < a.E ? a.Wr + (size_t)c * a.D : a.Wd + (size_t)(c - a.E) * a.D;
      acc[u] = 0.f;
    }
    for (int g = lane; g < groups; g += 64) {
      const uint4 x = xs[g];
      uint4 wq[IH_COLS];
#pragma unroll
      for (int u = 0; u < IH_COLS; ++u) wq[u] = *(const uint4*)(w[u] + 8 * g);
#pragma unroll
      for (int u = 0; u < IH_COLS; ++u) acc[u] = ih_dot8(wq[u], x, acc[u]);
    }
#pragma unroll
    for (int u = 0; u < IH_COLS; ++u) {
      const float s = wave_sum(acc[u]);
      const int c = c0 + u;
      if (lane == 0 && c < ncols) ys[c] = s + (c < a.E ? a.br[c] : a.bd[c - a.E]);
    }
  }
  __syncthreads();

  if (a.E > 0) {
    float ss = 0.f;
    for (int c = lane; c < a.E; c += 64) ss = fmaf(ys[c], ys[c], ss);
    ss = wave_sum(ss);
    const float nrm = sqrtf(ss);
    float* out = a.ret_emb + (size_t)blockIdx.x * a.E;
    for (int c = threadIdx.x; c < a.E; c += 64 * IH_WAVES) out[c] = ss > 0.f ? ys[c] / nrm : 0.f;      // a zero y stays zero
  }
  if (a.C > 0 && threadIdx.x == 0) {
    const float* z = ys + a.E;
    float m = z[0];
    int best = 0;
    for (int c = 1; c < a.C; ++c) if (z[c] > m) { m = z[c]; best = c; }      // a tie goes to the lower index
    float e[IH_MAX_C], sum = 0.f;
    for (int c = 0; c < a.C; ++c) { e[c] = expf(z[c] - m); sum += e[c]; }
    for (int c = 0; c < a.C; ++c) a.probs[(size_t)blockIdx.x * a.C + c] = e[c] / sum;
    a.choice[blockIdx.x] = best;
  }
}

__global__ __launch_bounds__(64) void img_rerank_kernel(const float* visual, const float* ret_emb, int g, int E, float* scores) {
  const int lane = threadIdx.x;
  const float* v = visual + (size_t)blockIdx.x * E;
  const float* r = ret_emb + (size_t)(blockIdx.x / g) * E;
  float dot = 0.f, vv = 0.f, rr = 0.f;
  for (int c = lane; c < E; c += 64) {
    const float x = v[c], y = r[c];
    dot = fmaf(x, y, dot); vv = fmaf(x, x, vv); rr = fmaf(y, y, rr);
  }
  dot = wave_sum(dot); vv = wave_sum(vv); rr = wave_sum(rr);
  if (lane == 0) scores[blockIdx.x] = (vv > 0.f && rr > 0.f) ? dot / (sqrtf(vv) * sqrtf(rr)) : 0.f;
}

int img_heads_launch(const float* hidden, int64_t rows, int D, const int* row_idx, int n, const bf16_t* Wr, const float* br, int E, const bf16_t* Wd,
                     const float* bd, int C, float* ret_emb, float* probs, int* choice, hipStream_t s) {
  const bool ret = Wr != nullptr || br != nullptr, dec = Wd != nullptr || bd != nullptr;
  GILL_REQUIRE(n >= 0 && rows >= 1, "img_block_heads: n >= 0 and rows >= 1");
  GILL_REQUIRE(D >= 8 && D % 8 == 0 && D <= IH_MAX_D, "img_block_heads: D must be a multiple of 8, at most 8192");
  GILL_REQUIRE(ret || dec, "img_block_heads: both weight pairs are NULL");
  GILL_REQUIRE(!ret || (Wr != nullptr && br != nullptr), "img_block_heads: Wr and br come as a pair");
  GILL_REQUIRE(!dec || (Wd != nullptr && bd != nullptr), "img_block_heads: Wd and bd come as a pair");
  GILL_REQUIRE(!ret || (E >= 1 && E <= IH_MAX_E), "img_block_heads: 1 <= E <= 1024");
  GILL_REQUIRE(!dec || (C >= 1 && C <= IH_MAX_C), "img_block_heads: 1 <= C <= 4");
  GILL_REQUIRE(hidden != nullptr && ((uintptr_t)hidden & 15) == 0, "img_block_heads: hidden must be a 16-byte aligned device pointer");
  GILL_REQUIRE(((uintptr_t)Wr & 15) == 0 && ((uintptr_t)Wd & 15) == 0, "img_block_heads: the weights must be 16-byte aligned");
  GILL_REQUIRE(((uintptr_t)br & 3) == 0 && ((uintptr_t)bd & 3) == 0 && ((uintptr_t)row_idx & 3) == 0, "img_block_heads: misaligned pointer");
  GILL_REQUIRE(((uintptr_t)ret_emb & 3) == 0 && ((uintptr_t)probs & 3) == 0 && ((uintptr_t)choice & 3) == 0, "img_block_heads: misaligned output");
  GILL_REQUIRE(!ret || ret_emb != nullptr, "img_block_heads: ret_emb is NULL");
  GILL_REQUIRE(!dec || (probs != nullptr && choice != nullptr), "img_block_heads: probs / choice are NULL");
  if (n == 0) return 0;
  GILL_REQUIRE(row_idx != nullptr, "img_block_heads: row_idx is NULL");
  ImgHeadsArgs a;
  a.hidden = hidden; a.row_idx = row_idx; a.Wr = Wr; a.br = br; a.Wd = Wd; a.bd = bd;
  a.ret_emb = ret_emb; a.probs = probs; a.choice = choice;
  a.rows = rows; a.D = D; a.E = ret ? E : 0; a.C = dec ? C : 0;
  img_heads_kernel<<<dim3((unsigned)n), dim3(64 * IH_WAVES), 0, s>>>(a);
  GILL_CHECK_HIP(hipGetLastError());
  return 0;
}

int img_rerank_launch(const float* visual, const float* ret_emb, int n, int g, int E, float* scores, hipStream_t s) {
  GILL_REQUIRE(n >= 0 && g >= 1 && E >= 1, "img_rerank_scores: n >= 0, g >= 1, E >= 1");
  GILL_REQUIRE((int64_t)n * g < 2147483647LL, "img_rerank_scores: n * g must stay below 2^31 - 1");
  if (n == 0) return 0;
  GILL_REQUIRE(visual != nullptr && ret_emb != nullptr && scores != nullptr, "img_rerank_scores: null pointer");
  GILL_REQUIRE(((uintptr_t)visual & 3) == 0 && ((uintptr_t)ret_emb & 3) == 0 && ((uintptr_t)scores & 3) == 0, "img_rerank_scores: misaligned pointer");
  img_rerank_kernel<<<dim3((unsigned)(n * g)), dim3(64), 0, s>>>(visual, ret_emb, g, E, scores);
  GILL_CHECK_HIP(hipGetLastError());
  return 0;
}
