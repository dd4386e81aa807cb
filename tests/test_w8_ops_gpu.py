"""The w8 format's kernels on the MI355X (csrc/linear_w8.hip) through ops.w8_quant / w8_dequant / linear_w8.

Quantiser and dequantiser: bit-equal to the host reference (tests/w8_util.py).  Linear: against fp64 on the same operands under
w8_util.element_bar: 10 x the CPU-measured accumulation distance (tools/w8_tolerance.py -> profiles/w8_decode.md) times the magnitude
sum_k |a||w| + |bias| + |resid|, plus half a bf16 ulp of the result for bf16 outputs.  tests/test_w8_host.py shows on the CPU that each
way of breaking the kernel misses that bar by more than 10^4 x.

Shapes of the linear tests (w8_util.OP_CASES), smallest at which each path occurs:
  (64, 64)          one workgroup, one K step: waves 1 .. 3 contribute zeros
  (192, 320)        three workgroups of four column groups; K = 5 x 64: no multiple of the 4-step unroll; forced splitk 2 (2 + 3 steps)
                    and 3 (1 + 2 + 2: the step count is not divisible by 3)
  (768, 3072)       the launcher's own rule: 4 slices
  (4096, 4096)      one OPT-6.7b matrix (out_proj), the launcher's own rule: 4 slices, 256 workgroups
  (128, 4160)       65 K steps unsplit: a second activation stage"""
import pytest
import torch

import kv_cache_util as U
import w8_util as W
from gill_amd import ops

pytestmark = pytest.mark.gpu

_CASE = {}


def _case(N, K, cuda):
  """Operands of one matrix shape (all MAX_ROWS activation rows), host quantisation, device copies and the fp64 pieces, built once."""
  if (N, K) not in _CASE:
    o = W.operands(N, K, W.MAX_ROWS, seed=100 + N + K)
    q, s = W.quantise(o["w"])
    o["qv"], o["s"] = q.float(), s
    o["w8_dev"], o["s_dev"] = W.kernel_order(q).to(cuda), s.to(cuda)
    o["A_dev"] = o["A"].to(cuda, torch.bfloat16)
    o["acc64"] = o["A"].double() @ (o["qv"].double() * s.double()[:, None]).T
    o["mag64"] = o["A"].double().abs() @ (o["qv"].double().abs() * s.double()[:, None]).T
    _CASE[(N, K)] = o
  return _CASE[(N, K)]


def _ref(o, M, bias, resid, act):
  y, mag = o["acc64"][:M].clone(), o["mag64"][:M].clone()
  if bias:
    y, mag = y + o["bias"].double()[None], mag + o["bias"].double().abs()[None]
  if act == "relu":
    y = torch.relu(y)
  if resid:
    y, mag = y + o["resid"][:M].double(), mag + o["resid"][:M].double().abs()
  return y, mag


def test_w8_max_rows():
  assert ops.w8_max_rows() == W.MAX_ROWS >= 16


@pytest.mark.parametrize("N,K", [(64, 64), (192, 320), (768, 3072)])
def test_quantiser_and_dequantiser_match_the_host_bit_for_bit(cuda, N, K):
  w = torch.randn((N, K), generator=torch.Generator().manual_seed(N + K)) * 0.03 * torch.pow(2.0, (torch.arange(N) % 7 - 3).float())[:, None]
  w[1] = 0                                     # an all-zero row
  w[2, 3] = 100 * w[2].abs().max()             # an outlier
  w[3] = 448.0 * 2.0 ** -12                    # max / 448 a power of two exactly: f = 0.875
  w = U.bf(w)
  q, s = W.quantise(w)
  w8, sc, ok = ops.w8_quant(w.to(cuda, torch.bfloat16))
  assert ok
  assert torch.equal(sc.cpu(), s), "scales differ from the host reference"
  assert torch.equal(w8.cpu(), W.kernel_order(q)), "bytes differ from the host reference"
  want = W.dequantise(q, s)
  dq, ok = ops.w8_dequant(w8, sc, N, K)
  assert ok and torch.equal(dq.float().cpu(), want), "row-major dequantiser"
  dqb, ok = ops.w8_dequant(w8, sc, N, K, blk64=True)
  assert ok and torch.equal(dqb.float().cpu(), W.blk64(want)), "64 x 64-blocked dequantiser"


@pytest.mark.parametrize("M", sorted(set(W.OP_ROWS)))
@pytest.mark.parametrize("N,K,sk", W.OP_CASES)
def test_linear_epilogues_vs_fp64(cuda, N, K, sk, M):
  """bias -> bf16; bias + ReLU -> bf16; bias + fp32 residual in place -> fp32; partials + opt_reduce_ln_launch: stream row and LayerNorm row."""
  o = _case(N, K, cuda)
  a = o["A_dev"][:M].contiguous()
  dev = lambda t: t.to(cuda)   # noqa: E731
  worst = 0.0
  for act in ("none", "relu"):
    got, ok = ops.linear_w8(a, o["w8_dev"], o["s_dev"], bias=dev(o["bias"]), act=act, splitk=sk)
    ref, mag = _ref(o, M, True, False, act)
    assert ok and got.dtype == torch.bfloat16
    worst = max(worst, W.figure(f"{N}x{K} sk={sk} M={M} bias {act} -> bf16", got.float().cpu(), ref, W.element_bar(ref, mag, True)))
  got, ok = ops.linear_w8(a, o["w8_dev"], o["s_dev"], bias=dev(o["bias"]), resid=dev(o["resid"][:M].contiguous()), splitk=sk)
  ref, mag = _ref(o, M, True, True, "none")
  assert ok and got.dtype == torch.float32
  worst = max(worst, W.figure(f"{N}x{K} sk={sk} M={M} bias + resid -> fp32", got.cpu(), ref, W.element_bar(ref, mag, False)))
  h, nb, ok = ops.linear_w8(a, o["w8_dev"], o["s_dev"], bias=dev(o["bias"]), resid=dev(o["resid"][:M].contiguous()), splitk=sk,
                            ln=(dev(o["gamma"]), dev(o["beta"])))
  assert ok
  worst = max(worst, W.figure(f"{N}x{K} sk={sk} M={M} reduce+LN stream row", h.cpu(), ref, W.element_bar(ref, mag, False)))
  # the LayerNorm row: fp64 LayerNorm of the fp64 stream row; the reducer's own fp32 arithmetic on a row of N values and the stream
  # row's distance, both through the normalisation (1 / std), then half a bf16 ulp
  mean, var = ref.mean(1, keepdim=True), ref.var(1, unbiased=False, keepdim=True)
  rstd = 1.0 / torch.sqrt(var + 1e-5)
  ln = (ref - mean) * rstd * o["gamma"].double()[None] + o["beta"].double()[None]
  ln_bar = (W.W8_BAR * mag.amax(1, keepdim=True) + 16 * 2.0 ** -24 * ref.abs().amax(1, keepdim=True)) * rstd * o["gamma"].double().abs()[None] \
    + 2.0 ** -22 * ln.abs() + W.half_ulp_bf16(ln)
  worst = max(worst, W.figure(f"{N}x{K} sk={sk} M={M} reduce+LN LayerNorm row", nb.float().cpu(), ln, ln_bar))
  assert worst <= 1.0, worst


@pytest.mark.parametrize("N,K,sk", [(192, 320, 1), (192, 320, 3), (768, 3072, 0)])
def test_batch_invariance(cuda, N, K, sk):
  """Row r of an M = 16 call, the other rows random, is bit-identical to the M = 1 call on that row: unsplit and split shapes."""
  o = _case(N, K, cuda)
  bias = o["bias"].to(cuda)
  full, ok = ops.linear_w8(o["A_dev"], o["w8_dev"], o["s_dev"], bias=bias, out_f32=True, splitk=sk)
  assert ok
  for r in (0, 7, 15):
    one, ok = ops.linear_w8(o["A_dev"][r:r + 1].contiguous(), o["w8_dev"], o["s_dev"], bias=bias, out_f32=True, splitk=sk)
    assert ok and torch.equal(one[0], full[r]), f"row {r}: {(one[0] - full[r]).abs().max().item():.3e}"


@pytest.mark.parametrize("N,K,sk,M", [(192, 320, 1, 3), (192, 320, 2, 5), (64, 64, 1, 1)])
def test_rows_beyond_m_are_not_written(cuda, N, K, sk, M):
  o = _case(N, K, cuda)
  for f32 in (False, True):
    got, ok = ops.linear_w8(o["A_dev"][:M].contiguous(), o["w8_dev"], o["s_dev"], bias=o["bias"].to(cuda), out_f32=f32, splitk=sk, out_rows=16,
                            canary=-77.0)
    assert ok and bool((got[M:] == -77.0).all()) and bool((got[:M] != -77.0).any())


@pytest.mark.parametrize("N,K", [(192, 320), (4096, 4096)])
def test_agrees_with_the_bf16_gemm_on_the_dequantised_matrix(cuda, N, K):
  """ops.gemm(A, dequantised W) and ops.linear_w8 within the sum of their two bars.  Both are bf16 operands with fp32 accumulation in some
  order and a bf16 result, so each gets element_bar: the accumulation bar on the fp32 sum plus half a bf16 ulp.  (192, 320): the GEMM's
  general tile; (4096, 4096): its STREAM64 tile on the blocked copy, split-K."""
  o = _case(N, K, cuda)
  M = 16
  wdq = W.dequantise(o["qv"].to(torch.float8_e4m3fn), o["s"]).to(cuda, torch.bfloat16)
  a = ops.gemm(o["A_dev"], wdq, bias=o["bias"].to(cuda))
  b, ok = ops.linear_w8(o["A_dev"], o["w8_dev"], o["s_dev"], bias=o["bias"].to(cuda))
  assert ok
  ref, mag = _ref(o, M, True, False, "none")
  bar = 2 * W.element_bar(ref, mag, True)
  f = W.figure(f"{N}x{K} gemm vs linear_w8", a.float().cpu(), b.float().cpu().double(), bar)
  assert f <= 1.0, f


def test_bad_arguments_are_errors_and_launch_nothing(cuda):
  from gill_amd import _native as Nn
  o = _case(192, 320, cuda)
  a17 = torch.zeros((W.MAX_ROWS + 1, 320), device=cuda, dtype=torch.bfloat16)
  with pytest.raises(Nn.GillNativeError):
    ops.linear_w8(a17, o["w8_dev"], o["s_dev"])
  a = torch.zeros((2, 96), device=cuda, dtype=torch.bfloat16)            # K = 96: no multiple of 64
  w8 = torch.zeros(192 * 96, device=cuda, dtype=torch.uint8)
  with pytest.raises(Nn.GillNativeError):
    ops.linear_w8(a, w8, o["s_dev"], out_rows=2, canary=-5.0)
  with pytest.raises(Nn.GillNativeError):
    ops.w8_quant(torch.zeros((64, 96), device=cuda, dtype=torch.bfloat16))
  torch.cuda.synchronize()
