// Decode attention with a multi-token append for gfx950 (AttnAppendArgs in ops.h): row b brings nq consecutive new tokens at its own cache
// length n = lens[b]; token i attends to the cache slots 0 .. n - 1 and to the tokens 0 .. i of its own block, and its key / value go to slot n + i.
//
// One workgroup of four waves per (b, h, token), each running the single-token kernel's body (attn_dec::decode_token) for its token with the
// length n + i.  The keys and values of the block's earlier tokens 0 .. i - 1 are the bf16 values of their input rows, which is also what their
// slots will hold: the body (its BLOCK mode) takes them from the input rows at the places where the single-token kernel reads the slots, so the
// same values enter the same sums in the same order.  A row's output and cache are therefore, to the bit, those of nq successive single-token
// launches, at any B and any grouping of the tokens into blocks; nq == 1 is the single-token kernel.  Nothing orders the tokens of a block:
// a workgroup reads cache slots below n only (plus, inside 16-byte V^T chunks that straddle n, bytes it replaces or selects out), which no
// workgroup of the launch writes, and stores slot n + i alone.  No barrier between tokens, no fence, no flag; the step stays a memory-bound
// read with no MFMA and no LDS staging of the cache, and its latency is that of one token.
#include "attention_decode_dev.h"

namespace {

using namespace attn_dec;

template <int DP, int LPK>
__global__ __launch_bounds__(kDecThreads) void attention_append_kernel(const AttnAppendArgs p) {
  extern __shared__ __attribute__((aligned(16))) float dec_sc[];     // [pitch + 8]: scores, then probabilities
  __shared__ float red[2 * kDecWaves];
  __shared__ float ob[DP];
  __shared__ __attribute__((aligned(16))) bf16_t vblk[kBlockMax * DP];

  const int tid = threadIdx.x;
  const int bh = blockIdx.x / p.nq, i = blockIdx.x - bh * p.nq;
  const int b = bh / p.H, h = bh - b * p.H;
  int n = p.lens[b];
  const int top = p.pitch - p.nq;       // >= 0: checked by the launcher
  const bool clamped = n < 0 || n > top;
  n = n < 0 ? 0 : (n > top ? top : n);
  if (clamped && p.flags && h == 0 && i == 0 && tid == 0) p.flags[b] = 1;

  const size_t row0 = (size_t)b * p.nq, in0 = row0 * p.ld + h * DP, in = in0 + (size_t)i * p.ld;
  decode_token<DP, LPK, true>(p.q + in, p.k + in, p.v + in, p.K + (size_t)bh * p.pitch * DP, p.Vt + (size_t)bh * p.dpv * p.pitch,
                              p.O + (row0 + i) * p.ldo + h * DP, n + i, p.pitch, p.dpv, p.qscale, dec_sc, red, ob, n, p.k + in0, p.v + in0, p.ld, vblk);
}

template <int DP, int LPK>
int launch_dp(const AttnAppendArgs& a, hipStream_t s) {
  const size_t smem = sizeof(float) * (size_t)(a.pitch + 8);
  hipLaunchKernelGGL((attention_append_kernel<DP, LPK>), dim3(a.B * a.H * a.nq), dim3(kDecThreads), smem, s, a);
  GILL_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace

int attention_append_launch(const AttnAppendArgs& a, hipStream_t s) {
  GILL_REQUIRE(a.q && a.k && a.v && a.K && a.Vt && a.lens && a.O, "append attention: null argument");
  GILL_REQUIRE(a.B > 0 && a.H > 0, "append attention: empty batch");
  GILL_REQUIRE(a.nq >= 1 && a.nq <= kBlockMax, "append attention: 1 .. 16 new tokens per row");
  GILL_REQUIRE(a.pitch >= 32 && a.pitch % 32 == 0 && a.pitch <= 8192, "append attention: cache pitch must be a multiple of 32, at most 8192");
  GILL_REQUIRE(a.dpv == round_up(a.dp, 32), "append attention: dpv must be dp rounded up to 32");
  GILL_REQUIRE(a.ld % 8 == 0 && a.ld >= a.H * a.dp && a.ldo % 2 == 0 && a.ldo >= a.H * a.dp, "append attention: row strides");
  GILL_REQUIRE(((uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v | (uintptr_t)a.K | (uintptr_t)a.Vt) % 16 == 0 && (uintptr_t)a.O % 4 == 0,
               "append attention: operands must be 16-byte aligned");
  switch (a.dp) {
    case 64:  return launch_dp<64, 8>(a, s);
    case 80:  return launch_dp<80, 2>(a, s);
    case 128: return launch_dp<128, 8>(a, s);
    default:
      gill_set_error("append attention: unsupported head dim (supported: 64, 80, 128)");
      return -2;
  }
}
