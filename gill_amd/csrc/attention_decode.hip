// Decode attention with append for gfx950: one new token per sequence, every sequence at its own cache length (AttnDecodeArgs in ops.h).
//
// The step is a read of the (b, h) pair's K and V^T up to its length and nothing else: ~2 flops per byte, memory-bound, so there is no MFMA and no LDS
// staging here.  One workgroup of four waves per (b, h):
//   1. scores.  K rows are dp contiguous bf16; LPK lanes share a key, each taking 16-byte chunks of the row straight into VGPRs (q is held scaled, in
//      fp32, in the same lanes), the four waves take interleaved blocks of 64 / LPK keys, UNROLL blocks in flight.  The new key comes from the input
//      row, never from the slot it is stored to.  Scores go to LDS (log2 domain).
//   2. softmax over the n + 1 scores in LDS: maximum, exp2, sum.
//   3. P V.  V^T rows are keys-contiguous: a lane takes 8 keys of a row with one 16-byte load, the wave covers 512 keys per pass, each wave owns
//      dp / 4 rows of the head.  The new value comes from the input row.
//   4. the appended K row, V^T column (and the ones-row entry the flash kernel expects where dpv > dp) are stored; O as bf16, token-major.
// Keys beyond the length are excluded by SELECTION: their scores are never formed, and the tail of the last 8-key chunk of V^T is selected out of
// the sum term by term, so whatever finite or non-finite bits a slot holds cannot reach the output.  Every 16-byte load lies inside the pitch
// (pitch % 32 == 0, chunk starts below the clamped length).
// Fixed function: every reduction has a fixed order (a lane's own terms in index order, xor trees over lanes, the four waves in index order), there
// are no atomics, and nothing depends on B, on another row's length or on the order workgroups run in: the same (b, h) data gives the same bits.
#include "attention_decode_dev.h"

namespace {

using namespace attn_dec;

// the four steps above are attn_dec::decode_token (attention_decode_dev.h), which gill_attention_append's kernel runs once per new token
template <int DP, int LPK>
__global__ __launch_bounds__(kDecThreads) void attention_decode_kernel(const AttnDecodeArgs p) {
  extern __shared__ __attribute__((aligned(16))) float dec_sc[];     // [pitch + 8]: scores, then probabilities
  __shared__ float red[2 * kDecWaves];
  __shared__ float ob[DP];

  const int tid = threadIdx.x;
  const int b = blockIdx.x / p.H, h = blockIdx.x - b * p.H;
  int n = p.lens[b];
  const bool clamped = n < 0 || n > p.pitch - 1;
  n = n < 0 ? 0 : (n > p.pitch - 1 ? p.pitch - 1 : n);
  if (clamped && p.flags && h == 0 && tid == 0) p.flags[b] = 1;

  const size_t in = (size_t)b * p.ld + h * DP;
  decode_token<DP, LPK>(p.q + in, p.k + in, p.v + in, p.K + (size_t)(b * p.H + h) * p.pitch * DP, p.Vt + (size_t)(b * p.H + h) * p.dpv * p.pitch,
                        p.O + (size_t)b * p.ldo + h * DP, n, p.pitch, p.dpv, p.qscale, dec_sc, red, ob);
}

template <int DP, int LPK>
int launch_dp(const AttnDecodeArgs& a, hipStream_t s) {
  const size_t smem = sizeof(float) * (size_t)(a.pitch + 8);
  hipLaunchKernelGGL((attention_decode_kernel<DP, LPK>), dim3(a.B * a.H), dim3(kDecThreads), smem, s, a);
  GILL_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace

int attention_decode_launch(const AttnDecodeArgs& a, hipStream_t s) {
  GILL_REQUIRE(a.q && a.k && a.v && a.K && a.Vt && a.lens && a.O, "decode attention: null argument");
  GILL_REQUIRE(a.B > 0 && a.H > 0, "decode attention: empty batch");
  GILL_REQUIRE(a.pitch >= 32 && a.pitch % 32 == 0 && a.pitch <= 8192, "decode attention: cache pitch must be a multiple of 32, at most 8192");
  GILL_REQUIRE(a.dpv == round_up(a.dp, 32), "decode attention: dpv must be dp rounded up to 32");
  GILL_REQUIRE(a.ld % 8 == 0 && a.ld >= a.H * a.dp && a.ldo % 2 == 0 && a.ldo >= a.H * a.dp, "decode attention: row strides");
  GILL_REQUIRE(((uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v | (uintptr_t)a.K | (uintptr_t)a.Vt) % 16 == 0 && (uintptr_t)a.O % 4 == 0,
               "decode attention: operands must be 16-byte aligned");
  switch (a.dp) {
    case 64:  return launch_dp<64, 8>(a, s);
    case 80:  return launch_dp<80, 2>(a, s);
    case 128: return launch_dp<128, 8>(a, s);
    default:
      gill_set_error("decode attention: unsupported head dim (supported: 64, 80, 128)");
      return -2;
  }
}
