"""Proof, on the CPU, that the bars of test_ln_gemm_gpu.py can fail — and that a correct kernel can meet them.

ln_gemm_util.consumer_emulation restates the folded-LayerNorm consumer of csrc/gemm.hip in torch (fp32 plane sums added in plane order,
bf16(W * g) weights, rstd * acc - mean * rstd * colsum + beta W^T + b, bf16 output) and can be broken in the ways the real path could be.
On the operands the GPU tests use (ln_gemm_util.case_operands), against the same fp32 reference (ln_linear_ref):

  0. the unbroken emulation stays within half of the 1e-2 bar, per row and over the whole tensor, for q / k / v^T (measured 0.40 .. 0.48 of
     the bar), and within 0.65 of it for GEGLU (measured 0.60 at C = 640, 0.50 at C = 1280: see the test);
  1. every statistics defect (a dropped plane, statistics shifted by one row, the last row taking its neighbour's statistics, column sums of
     W instead of g * W, beta W^T missing from the folded bias, the ln_rows wrap ignored) and every scatter defect (q scale applied to the K
     segment, V^T written untransposed or one token off) exceeds the bar;
  2. a producer that took its statistics from the unrounded accumulator instead of the bf16 values it stored, or left one plane's columns out,
     misses the planes' bar (rtol 2e-4, atol 2e-3 against sums of the stored tensor) — a defect no consumer output can show.

Each test prints its margin."""
import pytest
import torch

import ln_gemm_util as U

M = 200                                                         # the ragged row count of the GPU cases
GEOMS = [(320, 8, 40), (640, 8, 80), (1280, 8, 160), (640, 10, 64)]         # (C, heads, d) of the GPU QKV cases


def _qkv_case(C, heads, d, ntok=100, P=10, dup_half=False, ln_rows=0):
  t, g, beta, W, b = U.case_operands(M, C, 3 * C, dup_half)
  sums = U.row_sums(t)[:ln_rows or M]
  return (t, g, beta, W, b), U.split_planes(sums, P, seed=C + P), U.qkv_layout(U.ln_linear_ref(t, g, beta, W, b), M // ntok, ntok, heads, d)


def _worst(tag, got_list, ref_list):
  """max over the operands of the per-row figure and of the whole-tensor figure."""
  from test_ops_gpu import _report
  w = 0.0
  for name, got, ref in zip(("q", "k", "v^T"), U.qkv_token_major(*got_list), U.qkv_token_major(*ref_list)):
    w = max(w, U.rows_figure(f"{tag} {name}", got, ref), _report(f"{tag} {name}", got, ref))
  return w


@pytest.mark.parametrize("C,heads,d", GEOMS)
def test_emulation_meets_half_the_bar_qkv(C, heads, d):
  ops, planes, ref = _qkv_case(C, heads, d)
  emu = [U.bf(x) for x in U.qkv_layout(U.consumer_emulation(ops[0], planes, *ops[1:]), M // 100, 100, heads, d)]
  w = _worst(f"emulation C={C} d={d}", emu, ref)
  print(f"[C={C} heads={heads}] emulation: {w:.3e} = {w / U.BAR:.2f} of the bar")
  assert w <= U.BAR / 2


@pytest.mark.parametrize("C", [640, 1280])
def test_emulation_meets_the_bar_geglu(C):
  """GEGLU multiplies two projections, so the bf16(W * g) rounding enters twice: the bf16 rounding of the output costs up to 2^-8 = 3.9e-3 of
  the row's maximum as it does for q / k / v^T, and each factor adds what the linear cases show on top of that (4.7e-3 - 3.9e-3 = 0.8e-3
  measured there, 1.3e-3 allowed): 3.9e-3 + 2 x 1.3e-3 = 6.5e-3, i.e. 0.65 of the bar rather than the half the linear outputs keep.
  Measured: 6.02e-3 (C = 640), 4.97e-3 (C = 1280)."""
  from test_ops_gpu import _report
  t, g, beta, W, b = U.case_operands(M, C, 8 * C)
  planes = U.split_planes(U.row_sums(t), 20, seed=C)
  ref = U.geglu(U.ln_linear_ref(t, g, beta, W, b))
  emu = U.bf(U.geglu(U.consumer_emulation(t, planes, g, beta, W, b)))
  w = max(U.rows_figure(f"emulation GEGLU C={C}", emu, ref), _report(f"emulation GEGLU C={C}", emu, ref))
  print(f"[GEGLU C={C}] emulation: {w:.3e} = {w / U.BAR:.2f} of the bar")
  assert w <= 0.65 * U.BAR


@pytest.mark.parametrize("defect", U.STAT_DEFECTS)
@pytest.mark.parametrize("C,heads,d", GEOMS)
def test_statistics_defect_exceeds_the_bar(C, heads, d, defect):
  P = 20 if C == 1280 else 10
  ops, planes, ref = _qkv_case(C, heads, d, P=P)
  bad = [U.bf(x) for x in U.qkv_layout(U.consumer_emulation(ops[0], planes, *ops[1:], defect=defect), M // 100, 100, heads, d)]
  w = _worst(f"{defect} C={C}", bad, ref)
  print(f"[C={C} heads={heads}] {defect}: {w / U.BAR:.1f}x the bar")
  assert not w < U.BAR
  if C >= 640:      # ... and in the GEGLU output
    t, g, beta, W, b = U.case_operands(M, C, 8 * C)
    pl = U.split_planes(U.row_sums(t), P, seed=C)
    wg = U.rows_figure(f"{defect} GEGLU C={C}", U.bf(U.geglu(U.consumer_emulation(t, pl, g, beta, W, b, defect=defect))),
                       U.geglu(U.ln_linear_ref(t, g, beta, W, b)))
    print(f"[GEGLU C={C}] {defect}: {wg / U.BAR:.1f}x the bar")
    assert not wg < U.BAR


@pytest.mark.parametrize("P", [1, 4])
@pytest.mark.parametrize("C,heads,d", GEOMS)
def test_ignored_ln_rows_wrap_exceeds_the_bar(C, heads, d, P):
  ops, planes, ref = _qkv_case(C, heads, d, P=P, dup_half=True, ln_rows=M // 2)
  good = [U.bf(x) for x in U.qkv_layout(U.consumer_emulation(ops[0], planes, *ops[1:], ln_rows=M // 2), M // 100, 100, heads, d)]
  assert _worst(f"wrap C={C} P={P}", good, ref) <= U.BAR / 2
  bad = [U.bf(x) for x in U.qkv_layout(U.consumer_emulation(ops[0], planes, *ops[1:], ln_rows=M // 2, defect="ln_rows_wrap_ignored"),
                                       M // 100, 100, heads, d)]
  w = _worst(f"wrap ignored C={C} P={P}", bad, ref)
  print(f"[C={C} heads={heads} P={P}] ln_rows wrap ignored: {w / U.BAR:.1f}x the bar")
  assert not w < U.BAR


@pytest.mark.parametrize("defect", U.LAYOUT_DEFECTS)
@pytest.mark.parametrize("C,heads,d", GEOMS)
def test_scatter_defect_exceeds_the_bar(C, heads, d, defect):
  ops, planes, ref = _qkv_case(C, heads, d)
  y = U.consumer_emulation(ops[0], planes, *ops[1:])
  bad = [U.bf(x) for x in U.qkv_layout(y, M // 100, 100, heads, d, defect=defect)]
  w = _worst(f"{defect} C={C}", bad, ref)
  print(f"[C={C} heads={heads}] {defect}: {w / U.BAR:.1f}x the bar")
  assert not w < U.BAR


@pytest.mark.parametrize("M,N", [(200, 320), (128, 640), (200, 1280)])
def test_producer_plane_defects_miss_the_plane_bar(M, N):
  """Row sums of the fp32 result against row sums of its bf16 rounding (what the kernel stores and the consumer reads): the rounding errors of a
  row (~2^-9 of each value, random sign) add up to far more than atol + rtol |sum| in the `sum` moment, so statistics of the unrounded accumulator
  fail the bar the GPU test applies; so does a plane's worth of columns (N / 20 of them) left out."""
  ref = U.producer_operands(M, N, N)[4]
  want = U.row_sums(U.bf(ref))
  ok = lambda got: torch.allclose(got, want, rtol=U.PLANE_RTOL, atol=U.PLANE_ATOL)      # noqa: E731
  assert ok(U.row_sums(U.bf(ref).double()).float())            # (the bar itself is reachable: fp64 sums of the stored values, rounded to fp32)
  unrounded = U.row_sums(ref)
  excess = ((unrounded - want).abs() / (U.PLANE_ATOL + U.PLANE_RTOL * want.abs())).max().item()
  print(f"[{M}x{N}] statistics of the unrounded accumulator: {excess:.1f}x the planes' bar")
  assert not ok(unrounded) and excess >= 3
  assert not ok(U.row_sums(U.bf(ref)[:, N // 20:]))
