// On-device decision of the generate loop (gill/models.py:471-520): the [IMG] logit rule, the greedy pick with the [IMG]
// forcing and the next step's input embeddings, the temperature + top-p filter of the sampled path, and the seeded draw that
// replaces torch.multinomial (decode_sample_kernel).
//
// Every kernel is one workgroup per row of the (B, vocab) fp32 logits; workgroups never wait for each other and no value is
// summed through atomics, so each output is a fixed function of its row: bit-repeatable.
#include "ops.h"
#include "philox.h"

namespace {

constexpr int kPickThreads = 1024;
constexpr int kFilterThreads = 1024;
constexpr int kFilterPerThread = 64;    // the row lives in registers: vocab <= 1024 * 64

// The reference's surgery on one row, in its order (:476-489), by one thread: ids may repeat or overlap, and a later
// assignment reads what an earlier one wrote, exactly as the sequence of torch index assignments does.
__device__ void apply_rule_row(float* __restrict__ row, const DecodeRuleDev& r) {
  for (int j = 1; j < r.n_ret; ++j) row[r.ret[j]] = r.filter_value;
  for (int j = 1; j < r.n_gen; ++j) row[r.gen[j]] = r.filter_value;
  if (!r.special) return;
  if (r.suppress) {
    for (int j = 0; j < r.n_ret; ++j) row[r.ret[j]] = r.filter_value;
    for (int j = 0; j < r.n_gen; ++j) row[r.gen[j]] = r.filter_value;
    return;
  }
  if (r.do_ret_scale) row[r.ret[0]] = fabsf(row[r.ret[0]]) * r.ret_scale;
  if (r.do_gen_scale) row[r.gen[0]] = fabsf(row[r.gen[0]]) * r.gen_scale;
}

// torch.argmax order: NaN above every number (the first NaN wins), then larger value, then smaller index.  A total order,
// so the reduction tree does not change the winner.
__device__ __forceinline__ bool argmax_better(float va, int ia, float vb, int ib) {
  const bool na = va != va, nb = vb != vb;
  if (na || nb) return na && nb ? ia < ib : na;
  return va == vb ? ia < ib : va > vb;
}

// The best (value, index) of the workgroup under argmax_better, valid in thread 0 only: waves by shuffles, then thread 0 over the
// 16 wave results in wv / wi (one barrier).
__device__ __forceinline__ void block_argmax(float& bv, int& bi, float* wv, int* wi) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (argmax_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  if ((tid & 63) == 0) { wv[tid >> 6] = bv; wi[tid >> 6] = bi; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kPickThreads / 64; ++w)
      if (argmax_better(wv[w], wi[w], bv, bi)) { bv = wv[w]; bi = wi[w]; }
  }
}

// What follows the pick `bi` (thread 0's), by the whole workgroup: the [IMG] forcing (:518-520), the ids into tokens, their count
// into *n_out and their input_embeddings rows into next_embeds.
__device__ __forceinline__ void emit_pick(int bi, int row, const DecodeRuleDev& r, const bf16_t* __restrict__ table, int D,
                                          int64_t* __restrict__ tokens, int ld, int col, int32_t* __restrict__ n_out, int force,
                                          bf16_t* __restrict__ next_embeds, int64_t* emit, int* n_emit) {
  const int tid = threadIdx.x;
  if (tid == 0) {
    int n = 1;
    emit[0] = bi;
    if (force && bi == r.ret0_raw) {       // :518-520 (force is set by the host for B == 1 only)
      if (r.ret_eq_gen) {
        n = r.n_ret;
        for (int j = 0; j < n; ++j) emit[j] = r.ret_raw[j];
      } else {
        n = -1;                            // the reference's AssertionError: the host raises it when it reads the count
      }
    }
    *n_emit = n;
    for (int j = 0; j < n; ++j) tokens[(size_t)row * ld + col + j] = emit[j];
    if (row == 0) *n_out = n;
  }
  __syncthreads();
  // input_embeddings(next_token): the bf16 rows copied as embed_rows_bf16_kernel copies them (same clamp of the id)
  const int n = *n_emit;
  for (int j = 0; j < n; ++j) {
    int64_t id = emit[j];
    if (id < 0) id = 0;
    if (id >= r.vocab) id = r.vocab - 1;
    const uint32_t* e = reinterpret_cast<const uint32_t*>(table + (size_t)id * D);
    uint32_t* o = reinterpret_cast<uint32_t*>(next_embeds + (size_t)(row + j) * D);
    for (int c = tid; c < D / 2; c += kPickThreads) o[c] = e[c];
  }
}

template <bool PICK>
__global__ __launch_bounds__(kPickThreads) void decode_rule_pick_kernel(float* __restrict__ logits, int V, DecodeRuleDev r,
                                                                        const bf16_t* __restrict__ table, int D,
                                                                        int64_t* __restrict__ tokens, int ld, int col,
                                                                        int32_t* __restrict__ n_out, int force,
                                                                        bf16_t* __restrict__ next_embeds) {
  const int row = blockIdx.x, tid = threadIdx.x;
  float* x = logits + (size_t)row * V;
  if (tid == 0) apply_rule_row(x, r);
  if (!PICK) return;
  __syncthreads();    // workgroup-scope release / acquire: the rule's stores are visible to every wave below

  float bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int c = tid; c < V; c += kPickThreads) {
    const float v = x[c];
    if (argmax_better(v, c, bv, bi)) { bv = v; bi = c; }
  }
  __shared__ float wv[kPickThreads / 64];
  __shared__ int wi[kPickThreads / 64];
  __shared__ int64_t emit[kDecodeMaxIds];
  __shared__ int n_emit;
  block_argmax(bv, bi, wv, wi);
  emit_pick(bi, row, r, table, D, tokens, ld, col, n_out, force, next_embeds, emit, &n_emit);
}

// Fixed-order sum over the workgroup, result in every thread.  `red` is double-buffered by the caller's parity so that one
// barrier per call suffices.
__device__ __forceinline__ float block_sum_fixed(float v, float* red, int& parity) {
  v = wave_sum(v);
  float* buf = red + parity * (kFilterThreads / 64);
  parity ^= 1;
  if ((threadIdx.x & 63) == 0) buf[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int w = 0; w < kFilterThreads / 64; ++w) s += buf[w];
  return s;
}

__device__ __forceinline__ float block_max(float v, float* red, int& parity) {
  v = wave_max(v);
  float* buf = red + parity * (kFilterThreads / 64);
  parity ^= 1;
  if ((threadIdx.x & 63) == 0) buf[threadIdx.x >> 6] = v;
  __syncthreads();
  float m = buf[0];
#pragma unroll
  for (int w = 1; w < kFilterThreads / 64; ++w) m = fmaxf(m, buf[w]);
  return m;
}

template <bool RECIP>
__device__ __forceinline__ float divide(float x, float t, float inv_t) { return RECIP ? x * inv_t : __fdiv_rn(x, t); }

// The softmax numerators of a row and its top-p threshold, shared by the filter and the draw so that both keep the same set.
// In: e[i] = y of column tid + i * kFilterThreads (-inf past the row's end).  Out: e[i] = exp(y - max), 0 where y = -inf; mx = the
// row's maximum (fmaxf: NaNs ignored); returns K, the kept tokens being those with bits(e) >= K (0 without top-p: every token).
// The token at sorted position j stays iff j == 0 or the probability mass before it is <= top_p (:503-512).  The mass before a
// token is the sum of e over the tokens with a larger e, over Z = sum(e); as a function of a threshold k on the bits of e
// (non-negative floats: the bits are ordered like the values) that mass never grows with k, so K is the smallest k whose mass is
// <= top_p, found by bisection.  Each candidate's mass is a fixed-order sum over the row held in registers.  Tokens whose e round
// to one fp32 value are kept or dropped together.  The loop is a bisection on integers: it ends after 30 rounds whatever the
// row holds (NaN sums compare false).
__device__ __forceinline__ uint32_t softmax_keep_threshold(float (&e)[kFilterPerThread], float& mx, int do_top_p, float top_p,
                                                           float* red, int& parity) {
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < kFilterPerThread; ++i) m = fmaxf(m, e[i]);
  mx = block_max(m, red, parity);
  float z = 0.f;
#pragma unroll
  for (int i = 0; i < kFilterPerThread; ++i) {
    e[i] = e[i] == -INFINITY ? 0.f : __expf(e[i] - mx);
    z += e[i];
  }
  if (!do_top_p) return 0;
  z = block_sum_fixed(z, red, parity);
  const float bound = top_p * z;
  // smallest k in [0, bits(1.0)] with mass(e > k) <= top_p; mass(e > bits(1.0)) = 0
  uint32_t lo = 0, hi = __float_as_uint(1.0f);
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kFilterPerThread; ++i) s += __float_as_uint(e[i]) > mid ? e[i] : 0.f;
    s = block_sum_fixed(s, red, parity);
    if (s <= bound) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// out = in / t, then filter_value on every token the reference's sort / softmax / cumsum rule drops (:503-512).
template <bool RECIP>
__global__ __launch_bounds__(kFilterThreads) void decode_filter_kernel(const float* __restrict__ in, float* __restrict__ out, int V,
                                                                       float t, float inv_t, int do_top_p, float top_p,
                                                                       float filter_value) {
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* x = in + (size_t)row * V;
  float* y = out + (size_t)row * V;
  if (!do_top_p) {
    for (int c = tid; c < V; c += kFilterThreads) y[c] = divide<RECIP>(x[c], t, inv_t);
    return;
  }
  __shared__ float red[2 * (kFilterThreads / 64)];
  int parity = 0;
  float e[kFilterPerThread];
#pragma unroll
  for (int i = 0; i < kFilterPerThread; ++i) {
    const int c = tid + i * kFilterThreads;
    float v = -INFINITY;
    if (c < V) {
      v = divide<RECIP>(x[c], t, inv_t);
      y[c] = v;                   // kept tokens keep this value; the last pass overwrites the dropped ones
    }
    e[i] = v;
  }
  float mx;
  const uint32_t lo = softmax_keep_threshold(e, mx, 1, top_p, red, parity);
  // the dropped tokens, from the values this thread stored above (e recomputed bit for bit; a rolled loop, so the compiler does
  // not keep 64 addresses alive across the bisection)
  for (int c = tid; c < V; c += kFilterThreads) {
    const float v = y[c];
    const float ev = v == -INFINITY ? 0.f : __expf(v - mx);
    if (__float_as_uint(ev) < lo) y[c] = filter_value;
  }
}

// The seeded draw (the contract is in include/gill_amd.h at gill_opt_sample_token): rule, y = x / t, the filter's kept set, then
// the exponential race: key_c = exp(y_c - max) / -log(u_c) with u_c a Philox uniform keyed by (seed, row, draw, c), and the token
// is the argmax of the keys over the kept columns (P(c wins) = e_c / sum e: the construction torch.multinomial uses for one
// sample).  Every key is a fixed function of its own column and argmax_better is a total order, so the winner does not depend on
// the reduction tree, on the batch, or on the order workgroups run in.  Rows without a finite maximum (a NaN, a +inf, or all
// -inf) draw nothing: they take torch.argmax's pick on y.  The logits keep the post-rule, pre-temperature values.
__global__ __launch_bounds__(kFilterThreads) void decode_sample_kernel(float* __restrict__ logits, int V, DecodeRuleDev r, float t,
                                                                       int do_top_p, float top_p, uint64_t seed, uint32_t row0,
                                                                       uint32_t draw, const bf16_t* __restrict__ table, int D,
                                                                       int64_t* __restrict__ tokens, int ld, int col,
                                                                       int32_t* __restrict__ n_out, int force,
                                                                       bf16_t* __restrict__ next_embeds) {
  static_assert(kFilterThreads == kPickThreads, "block_argmax / emit_pick stride by kPickThreads");
  const int row = blockIdx.x, tid = threadIdx.x;
  float* x = logits + (size_t)row * V;
  if (tid == 0) apply_rule_row(x, r);
  __syncthreads();    // workgroup-scope release / acquire: the rule's stores are visible to every wave below

  __shared__ float red[2 * (kFilterThreads / 64)];
  __shared__ float wv[kPickThreads / 64];
  __shared__ int wi[kPickThreads / 64];
  __shared__ int64_t emit[kDecodeMaxIds];
  __shared__ int n_emit;
  int parity = 0;
  float e[kFilterPerThread];
#pragma unroll
  for (int i = 0; i < kFilterPerThread; ++i) {
    const int c = tid + i * kFilterThreads;
    e[i] = c < V ? divide<false>(x[c], t, 0.f) : -INFINITY;
  }
  float mx;
  const uint32_t lo = softmax_keep_threshold(e, mx, do_top_p, top_p, red, parity);
  // fmaxf drops NaNs, so the maximum alone does not show them; exp(NaN - mx) is a NaN (tested here rather than on y in the load
  // loop, where the flag costs the registers that make the row spill)
  int has_nan = 0;
#pragma unroll
  for (int i = 0; i < kFilterPerThread; ++i) has_nan |= e[i] != e[i];
  const int no_draw = __syncthreads_or(has_nan) || !(fabsf(mx) < INFINITY);    // uniform over the workgroup

  float bv = -INFINITY;
  int bi = 0x7fffffff;
  if (no_draw) {
    for (int c = tid; c < V; c += kFilterThreads) {
      const float v = divide<false>(x[c], t, 0.f);
      if (argmax_better(v, c, bv, bi)) { bv = v; bi = c; }
    }
  } else {
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), prow = row0 + (uint32_t)row;
    // e recomputed bit for bit from the row, as the filter's last pass does: a rolled loop, so the 64 registers of the bisection are
    // dead here and the ten Philox rounds are in the instruction stream once.  Each key depends on its own column only, so the
    // columns may go to the threads in any order: a thread takes the four columns of one Philox block, one call for four words.
#pragma unroll 1
    for (int q = tid; 4 * q < V; q += kFilterThreads) {
      float ev[4];
      bool kept = false;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = 4 * q + j;
        ev[j] = -1.f;                    // below every threshold: a column past the row's end (V % 4 != 0) or a dropped one
        if (c < V) {
          const float v = divide<false>(x[c], t, 0.f);
          const float e1 = v == -INFINITY ? 0.f : __expf(v - mx);
          if (__float_as_uint(e1) >= lo) { ev[j] = e1; kept = true; }
        }
      }
      if (!kept) continue;               // under top-p most blocks hold no kept column: no Philox call for them
      const Philox4 p = philox4x32_10((uint32_t)q, prow, draw, 0u, k0, k1);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (ev[j] >= 0.f) {
          const float key = __fdiv_rn(ev[j], -logf(philox_uniform(p.w[j])));
          if (argmax_better(key, 4 * q + j, bv, bi)) { bv = key; bi = 4 * q + j; }
        }
      }
    }
  }
  block_argmax(bv, bi, wv, wi);
  emit_pick(bi, row, r, table, D, tokens, ld, col, n_out, force, next_embeds, emit, &n_emit);
}

// ---- ragged decision: every row its own step count, length and [IMG] forcing state (the layout of `st` is in include/gill_amd.h) ----

// The draw of decode_sample_kernel on one row, as a device function for the ragged kernel (decode_sample_kernel keeps its own copy so that its
// code stays what it was): rule already applied; on return (bv, bi) is this thread's best key, to be joined by block_argmax.
__device__ __forceinline__ void draw_row(const float* __restrict__ x, int V, float t, int do_top_p, float top_p, uint64_t seed, uint32_t prow,
                                         uint32_t draw, float* red, float& bv, int& bi) {
  const int tid = threadIdx.x;
  int parity = 0;
  float e[kFilterPerThread];
#pragma unroll
  for (int i = 0; i < kFilterPerThread; ++i) {
    const int c = tid + i * kFilterThreads;
    e[i] = c < V ? divide<false>(x[c], t, 0.f) : -INFINITY;
  }
  float mx;
  const uint32_t lo = softmax_keep_threshold(e, mx, do_top_p, top_p, red, parity);
  int has_nan = 0;
#pragma unroll
  for (int i = 0; i < kFilterPerThread; ++i) has_nan |= e[i] != e[i];
  const int no_draw = __syncthreads_or(has_nan) || !(fabsf(mx) < INFINITY);    // uniform over the workgroup
  bv = -INFINITY;
  bi = 0x7fffffff;
  if (no_draw) {
    for (int c = tid; c < V; c += kFilterThreads) {
      const float v = divide<false>(x[c], t, 0.f);
      if (argmax_better(v, c, bv, bi)) { bv = v; bi = c; }
    }
    return;
  }
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll 1
  for (int q = tid; 4 * q < V; q += kFilterThreads) {
    float ev[4];
    bool kept = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = 4 * q + j;
      ev[j] = -1.f;
      if (c < V) {
        const float v = divide<false>(x[c], t, 0.f);
        const float e1 = v == -INFINITY ? 0.f : __expf(v - mx);
        if (__float_as_uint(e1) >= lo) { ev[j] = e1; kept = true; }
      }
    }
    if (!kept) continue;
    const Philox4 p = philox4x32_10((uint32_t)q, prow, draw, 0u, k0, k1);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (ev[j] >= 0.f) {
        const float key = __fdiv_rn(ev[j], -logf(philox_uniform(p.w[j])));
        if (argmax_better(key, 4 * q + j, bv, bi)) { bv = key; bi = 4 * q + j; }
      }
    }
  }
}

// One workgroup per row, one launch per iteration of the ragged loop.  A row in a forced [IMG] block emits the block's next id and touches no
// logit; a finished row (step >= max_steps, no block pending) changes nothing; every other row takes a decision: the rule with suppress =
// (its own step < min_word_tokens), the argmax or the seeded draw keyed (seed, row_id, draw = step), then step + 1.  A pick of ret[0] with
// n_ret > 1 opens a forced block (or, with ret != gen, sets the row's error flag: the reference's assert).  An emitting row appends its id to
// tokens[row][n_tok++], copies the id's embedding row to next_embeds[row] and advances len.  The active-row count goes down by one (an integer
// atomic: exact in any order) when a row emits its last id.  Rows never read each other's state: a row's tokens do not depend on the batch.
template <bool SAMPLE>
__global__ __launch_bounds__(kPickThreads) void decode_ragged_kernel(float* __restrict__ logits, int V, DecodeRuleDev r, DecodeRuleDev rs, int min_word_tokens,
                                                                     int max_steps, float t, int do_top_p, float top_p, uint64_t seed,
                                                                     int32_t* __restrict__ st, int B, int32_t* __restrict__ clamp_flags,
                                                                     const bf16_t* __restrict__ table, int D, int64_t* __restrict__ tokens,
                                                                     int ld, bf16_t* __restrict__ next_embeds) {
  static_assert(kFilterThreads == kPickThreads, "block_argmax strides by kPickThreads");
  const int row = blockIdx.x, tid = threadIdx.x;
  __shared__ float red[2 * (kFilterThreads / 64)];
  __shared__ float wv[kPickThreads / 64];
  __shared__ int wi[kPickThreads / 64];
  __shared__ int64_t emit_id;
  const int step = st[DEC_STEP * B + row], forced = st[DEC_FORCED * B + row];
  __syncthreads();      // every thread holds the row's state before thread 0 rewrites it
  if (tid == 0 && clamp_flags && clamp_flags[row]) {      // a length clamp of the step's attention: reported through the row's flags
    st[DEC_FLAGS * B + row] |= DEC_FLAG_CLAMP;
    clamp_flags[row] = 0;
  }
  if (forced == 0 && step >= max_steps) return;           // finished (uniform over the workgroup)
  int bi = 0;
  if (forced == 0) {
    float* x = logits + (size_t)row * V;
    if (tid == 0) {       // r with suppress = 0, rs with suppress = 1: the row's own step chooses
      if (step < min_word_tokens) apply_rule_row(x, rs);
      else apply_rule_row(x, r);
    }
    __syncthreads();
    float bv = -INFINITY;
    bi = 0x7fffffff;
    if (SAMPLE) {
      draw_row(x, V, t, do_top_p, top_p, seed, (uint32_t)st[DEC_ROW_ID * B + row], (uint32_t)step, red, bv, bi);
    } else {
      for (int c = tid; c < V; c += kPickThreads) {
        const float v = x[c];
        if (argmax_better(v, c, bv, bi)) { bv = v; bi = c; }
      }
    }
    block_argmax(bv, bi, wv, wi);
  }
  if (tid == 0) {
    int64_t id;
    int nforced = 0, nstep = step, flags = 0;
    if (forced > 0) {
      id = r.ret_raw[forced];
      nforced = forced + 1 < r.n_ret ? forced + 1 : 0;
    } else {
      id = bi;
      nstep = step + 1;
      if (bi == r.ret0_raw && r.n_ret > 1) {
        if (r.ret_eq_gen) { id = r.ret_raw[0]; nforced = 1; }
        else flags |= DEC_FLAG_ASSERT;
      }
    }
    const int nt = st[DEC_NTOK * B + row];
    if (nt < ld) tokens[(size_t)row * ld + nt] = id;
    else flags |= DEC_FLAG_FULL;
    st[DEC_NTOK * B + row] = nt + 1;
    st[DEC_LEN * B + row] += 1;
    st[DEC_STEP * B + row] = nstep;
    st[DEC_FORCED * B + row] = nforced;
    if (flags) st[DEC_FLAGS * B + row] |= flags;
    if (nforced == 0 && nstep >= max_steps) atomicSub(&st[DEC_FIELDS * B], 1);
    emit_id = id;
  }
  __syncthreads();
  int64_t id = emit_id;
  if (id < 0) id = 0;
  if (id >= r.vocab) id = r.vocab - 1;
  const uint32_t* e = reinterpret_cast<const uint32_t*>(table + (size_t)id * D);
  uint32_t* o = reinterpret_cast<uint32_t*>(next_embeds + (size_t)row * D);
  for (int c = tid; c < D / 2; c += kPickThreads) o[c] = e[c];
}

}  // namespace

int decode_ragged_launch(float* logits, int B, int V, const DecodeRuleDev& r_in, int min_word_tokens, int max_steps, const DecodeSampler* sm,
                         int32_t* state, int32_t* clamp_flags, const bf16_t* table, int D, int64_t* tokens, int ld, bf16_t* next_embeds,
                         hipStream_t s) {
  GILL_REQUIRE(B >= 1 && V >= 1 && D % 2 == 0 && ld >= 1 && max_steps >= 0, "ragged decode: bad shape");
  GILL_REQUIRE(logits && state && tokens && next_embeds && table, "ragged decode: null argument");
  DecodeRuleDev r = r_in, rs = r_in;
  r.suppress = 0;
  rs.suppress = 1;
  if (sm) {
    GILL_TRY(decode_sample_check(B, V, r, *sm, D, kDecodeMaxIds + 1, 0));
    hipLaunchKernelGGL(decode_ragged_kernel<true>, dim3(B), dim3(kPickThreads), 0, s, logits, V, r, rs, min_word_tokens, max_steps,
                       (float)sm->temperature, (int)(sm->top_p < 1.0), (float)sm->top_p, sm->seed, state, B, clamp_flags, table, D, tokens, ld,
                       next_embeds);
  } else {
    hipLaunchKernelGGL(decode_ragged_kernel<false>, dim3(B), dim3(kPickThreads), 0, s, logits, V, r, rs, min_word_tokens, max_steps, 1.f, 0, 1.f,
                       (uint64_t)0, state, B, clamp_flags, table, D, tokens, ld, next_embeds);
  }
  GILL_CHECK_HIP(hipGetLastError());
  return 0;
}

int decode_rule_pick_launch(float* logits, int B, int V, const DecodeRuleDev& r, const bf16_t* table, int D, int64_t* tokens,
                            int ld, int col, int32_t* n_out, bf16_t* next_embeds, hipStream_t s) {
  GILL_REQUIRE(B >= 1 && V >= 1 && D % 2 == 0, "decode pick: bad shape");
  GILL_REQUIRE(tokens && n_out && next_embeds && table, "decode pick: null argument");
  const int force = B == 1;
  GILL_REQUIRE(col >= 0 && col + (force ? (r.n_ret > 1 ? r.n_ret : 1) : 1) <= ld, "decode pick: token buffer too short");
  hipLaunchKernelGGL(decode_rule_pick_kernel<true>, dim3(B), dim3(kPickThreads), 0, s, logits, V, r, table, D, tokens, ld, col,
                     n_out, force, next_embeds);
  GILL_CHECK_HIP(hipGetLastError());
  return 0;
}

int decode_sample_check(int B, int V, const DecodeRuleDev& r, const DecodeSampler& sm, int D, int ld, int col) {
  GILL_REQUIRE(B >= 1 && V >= 1 && D % 2 == 0, "decode sample: bad shape");
  GILL_REQUIRE(V <= kFilterThreads * kFilterPerThread, "decode sample: needs vocab <= 65536");
  GILL_REQUIRE(sm.temperature > 0 && (float)sm.temperature > 0 && (float)sm.temperature < INFINITY,
               "decode sample: temperature must be a positive fp32 number");     // false for a NaN too
  GILL_REQUIRE(sm.top_p > 0 && sm.top_p <= 1.0, "decode sample: top_p must be in (0, 1]");
  GILL_REQUIRE(sm.draw >= 0 && sm.row0 >= 0, "decode sample: draw and row0 must be >= 0");
  GILL_REQUIRE(col >= 0 && col + (B == 1 ? (r.n_ret > 1 ? r.n_ret : 1) : 1) <= ld, "decode sample: token buffer too short");
  return 0;
}

int decode_sample_launch(float* logits, int B, int V, const DecodeRuleDev& r, const DecodeSampler& sm, const bf16_t* table, int D,
                         int64_t* tokens, int ld, int col, int32_t* n_out, bf16_t* next_embeds, hipStream_t s) {
  GILL_REQUIRE(logits && tokens && n_out && next_embeds && table, "decode sample: null argument");
  GILL_TRY(decode_sample_check(B, V, r, sm, D, ld, col));
  const int force = B == 1;
  hipLaunchKernelGGL(decode_sample_kernel, dim3(B), dim3(kFilterThreads), 0, s, logits, V, r, (float)sm.temperature,
                     (int)(sm.top_p < 1.0), (float)sm.top_p, sm.seed, (uint32_t)sm.row0, (uint32_t)sm.draw, table, D, tokens, ld, col,
                     n_out, force, next_embeds);
  GILL_CHECK_HIP(hipGetLastError());
  return 0;
}

int decode_rule_launch(float* logits, int B, int V, const DecodeRuleDev& r, hipStream_t s) {
  GILL_REQUIRE(B >= 1 && V >= 1, "decode rule: bad shape");
  hipLaunchKernelGGL(decode_rule_pick_kernel<false>, dim3(B), dim3(64), 0, s, logits, V, r, nullptr, 0, nullptr, 0, 0, nullptr, 0,
                     nullptr);
  GILL_CHECK_HIP(hipGetLastError());
  return 0;
}

int decode_filter_launch(const float* in, float* out, int B, int V, double temperature, int reciprocal, double top_p,
                         double filter_value, hipStream_t s) {
  GILL_REQUIRE(B >= 1 && V >= 1 && in && out, "decode filter: bad argument");
  GILL_REQUIRE(temperature != 0, "decode filter: temperature must not be 0");
  const int do_top_p = top_p < 1.0;
  GILL_REQUIRE(!do_top_p || top_p > 0, "decode filter: top_p must be > 0");
  GILL_REQUIRE(!do_top_p || V <= kFilterThreads * kFilterPerThread, "decode filter: top-p needs vocab <= 65536");
  GILL_REQUIRE(in != out, "decode filter: out of place only");
  const float t = (float)temperature;
  const float inv_t = 1.0f / t;    // torch's rule for a device tensor divided by a host scalar: a * (1 / b), both in fp32
  if (reciprocal)
    hipLaunchKernelGGL(decode_filter_kernel<true>, dim3(B), dim3(kFilterThreads), 0, s, in, out, V, t, inv_t, do_top_p, (float)top_p,
                       (float)filter_value);
  else
    hipLaunchKernelGGL(decode_filter_kernel<false>, dim3(B), dim3(kFilterThreads), 0, s, in, out, V, t, inv_t, do_top_p, (float)top_p,
                       (float)filter_value);
  GILL_CHECK_HIP(hipGetLastError());
  return 0;
}
