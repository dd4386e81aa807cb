"""Operator-level net under the folded-LayerNorm chain of UNet levels 1-3 (csrc/unet.hip xf(): norm1 / norm2 / norm3 never run as kernels).

  producer  ops.linear_rowstats  the GEMM that writes the residual stream and files {sum, sum of squares} of every stored row into
                                 GemmArgs::row_stats planes: the row-major epilogue of gemm_kernel (one plane per (N tile, wave column)) when
                                 unsplit, gemm_splitk_reduce_kernel (one plane per 64-column block) under split-K;
  consumer  ops.ln_gemm_geglu /  the GEMM that reads the planes back through ln_row_factors() and applies rstd * acc - mean * rstd * colsum +
            ops.ln_gemm_qkv      bias in the GEGLU epilogue (EPI 1), the head-major scatter epilogue (EPI 3), or the split-K reducer (store4()).

Every case is compared with a plain fp32 statement of the same operation on the same bf16-rounded operands (ln_gemm_util.ln_linear_ref), at
the project's existing bars: 6e-3 for the residual stream, rtol 2e-4 / atol 2e-3 for the planes against sums of the tensor the kernel
stored, 1e-2 per row and over the whole tensor for q / k / v^T and GEGLU.  test_ln_gemm_host.py shows on the CPU that these operands leave
a correct kernel half of the 1e-2 bar (0.65 of it for GEGLU) and that every defect it lists exceeds it.

Measured on an MI355X (worst case of each kind): residual stream 3.5e-3 of 6e-3; q / k / v^T 5.2e-3 per row (M = 4096, the ping-pong tile), 4.3e-3 over
the whole tensor; GEGLU 5.4e-3 per row (the chain at C = 640, both producers), 3.9e-3 over the whole tensor; plane sums within 1.2e-2 of sums of squares
of 6e4 (2e-7 relative).  No case needed a fix in gemm.hip.

Which kernel a case lands on follows gemm_plan.hip's plan_tile_width() / plan_waves() / plan_kernel() (kernel = gemm_kernel<waves, BN, conv, EPI,
ring depth, KT, MI>, rows per tile = waves / 2 * MI * 16); each case says so next to its parameters."""
import functools

import pytest
import torch

import ln_gemm_util as U
from test_ops_gpu import _bf, _report, _rnd

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------ producer
def _plane_sum(planes):
  tot = torch.zeros(planes.shape[1:])
  for p in planes.float().cpu():        # plane order, as the consumers add them
    tot = tot + p
  return tot


def _check_producer(cuda, M, N, K, sk, want_planes, a2=False, inplace=False):
  from gill_amd import ops
  a, w, bias, resid, ref = U.producer_operands(M, N, K)
  K1 = 4 * N if a2 else K
  t, planes, (t_guard, p_guard) = ops.linear_rowstats(_bf(a[:, :K1]).contiguous().to(cuda), _bf(w).to(cuda), bias.to(cuda), _bf(resid).to(cuda),
                                                      a2=_bf(a[:, K1:]).contiguous().to(cuda) if a2 else None, splitk=sk, inplace=inplace)
  tag = f"linear_rowstats {M}x{N}x{K} sk{sk}{' a2' if a2 else ''}{' in place' if inplace else ''}"
  print(f"[{tag}] planes {planes.shape[0]} (expected {want_planes})")
  rel = _report(tag, t, ref)
  got, want = _plane_sum(planes), U.row_sums(t.float().cpu())
  print(f"[{tag}] plane sums: max abs diff {float((got - want).abs().max()):.3e}, max |want| {float(want.abs().max()):.3e}")
  assert planes.shape[0] == want_planes and want_planes <= 20
  # NaN-prefilled by the wrapper: every (plane, row < M) and every element of t was written, nothing beyond row M or the last plane was
  assert torch.isfinite(t.float()).all() and torch.isfinite(planes).all()
  assert torch.isnan(t_guard.float()).all() and torch.isnan(p_guard).all()
  assert rel < U.T_BAR
  assert torch.allclose(got, want, rtol=U.PLANE_RTOL, atol=U.PLANE_ATOL), float((got - want).abs().max())


@pytest.mark.parametrize("M,N,want_planes", [
  (64, 320, 4), (64, 640, 8), (64, 1280, 16),        # one 128-row tile, half of it beyond M: gemm_kernel<4, 160, 0, 4, 2> (M <= 64 keeps the 160-wide tile)
  (128, 320, 4), (200, 320, 4), (512, 320, 4),       # 64-row tiles, 320 % 128 != 0: gemm_kernel<4, 160, 0, 4, 2, 64, 2>, 2 N tiles x 2 wave columns
  (128, 640, 10), (200, 640, 10), (512, 640, 10),    # few tiles, N % 128 == 0: plan_tile_width() = 128, gemm_kernel<4, 128, 0, 4, 3, 64, 2>, 5 N tiles
  (128, 1280, 20), (200, 1280, 20), (512, 1280, 20),       # the same kernel, 10 N tiles: LN_MAX_PLANES
  (3900, 1280, 20),                                  # 31 x 10 = 310 tiles of 128 x 128, the last M tile ragged: the 128-row four-wave tile gemm_kernel<4, 128, 0, 4, 2>
  (4096, 1280, 16),                                  # 32 x 8 = 256 ping-pong workgroups, one round: gemm_plain_pingpong(), gemm_kernel<8, 160, 0, 4, 3, 64, 2>
])
def test_linear_rowstats_unsplit(cuda, M, N, want_planes):
  """proj_in / attn1.to_out / attn2.to_out of a level-1..3 block (K = N), split-K 1: the planes come from the row-major epilogue EPI 4 of gemm_kernel, one
  per (N tile, wave column); M = 200 and M = 64 leave tile rows beyond M that must not be written (t and the planes are followed by NaN guards)."""
  _check_producer(cuda, M, N, N, 1, want_planes)


@pytest.mark.parametrize("M,N,sk,want_planes", [
  (128, 320, 2, 5), (200, 640, 3, 10), (64, 1280, 2, 20), (512, 1280, 2, 20),      # gemm_splitk_reduce_kernel<64, 1>: 16-row blocks (fewer than 1024 blocks of 64)
  (4096, 1280, 2, 20),                               # 20 x 64 = 1280 blocks: gemm_splitk_reduce_kernel<64, 4>, 64-row blocks (partials from the ping-pong tiles)
  (128, 640, 0, 10), (128, 1280, 0, 20),             # auto: gemm_pick_splitk() splits these 2 and 5 ways (4 / 8 tiles, >= 4 K steps per split): the reducer again
  (512, 320, 0, 4),                                  # auto: 5 K steps < 8, unsplit: the epilogue's 4 planes
])
def test_linear_rowstats_splitk(cuda, M, N, sk, want_planes):
  """The same GEMMs under split-K (forced, or the engine's heuristic): partials from gemm_kernel<4, BN, 0, 2, 2>, then gemm_splitk_reduce_kernel sums the
  slices, stores t and files one plane per 64-column block (blockIdx.x) from the bf16-rounded values; M = 200 is ragged in its 16-row blocks."""
  _check_producer(cuda, M, N, N, sk, want_planes)


@pytest.mark.parametrize("M,N,want_planes", [
  (128, 640, 8),       # K = 3200 >= 2560, M % 128 == 0: gemm_plain_pingpong(), the 8-wave ping-pong kernel gemm_kernel<8, 160, 0, 4, 3, 64, 2> (128 x 160 tiles)
  (200, 320, 4),       # M % 128 != 0: no ping-pong, gemm_kernel<4, 160, 0, 4, 2, 64, 2> walking two A sources
])
def test_linear_rowstats_two_sources(cuda, M, N, want_planes):
  """The fused feed-forward output GEMM of levels 1-3: A = [h (M, 4N) | t (M, N)] as two K-concatenated sources (GemmArgs::A2, K1 = 4N, K = 5N) + bias +
  the outer residual, with row statistics (the engine files GroupNorm partials here; the K-concatenation itself has no other operator test)."""
  _check_producer(cuda, M, N, 5 * N, 1, want_planes, a2=True)


@pytest.mark.parametrize("M,N,sk,want_planes", [
  (128, 640, 1, 10),       # epilogue: the residual rows are loaded before the first store of the tile (gemm_kernel<4, 128, 0, 4, 3, 64, 2>)
  (200, 1280, 2, 20),      # reducer: store4() reads the residual quad it is about to overwrite (gemm_splitk_reduce_kernel<64, 1>)
])
def test_linear_rowstats_residual_in_place(cuda, M, N, sk, want_planes):
  """resid aliased to the output, as attn1.to_out / attn2.to_out run in the engine (t += o W^T + b): same values, same planes."""
  _check_producer(cuda, M, N, N, sk, want_planes, inplace=True)


# ------------------------------------------------------------------------------------------------ consumer
@functools.lru_cache(maxsize=None)
def _consumer_ref(M, C, N, dup_half=False):
  return U.ln_linear_ref(*U.case_operands(M, C, N, dup_half))


def _planes_for(t, P, ln_rows, cuda):
  return U.split_planes(U.row_sums(t)[:ln_rows or t.shape[0]], P, seed=t.shape[1] + P).to(cuda)


def _assert_qkv(tag, outs, y_ref, B, ntok, heads, d):
  """q / k / v^T of ops.ln_gemm_qkv against the scatter of y_ref: what test_lnproj_proj_in_qkv_vs_torch asserts, per row as well."""
  from gill_amd import ops
  q, k, vt = outs
  nseg = 1 if k is None else 3
  dp = ops.padded_head_dim(d)
  dpv = (dp + 31) // 32 * 32
  got = [q[:, :, :ntok, :d].float().cpu()] + ([] if nseg == 1 else [k[:, :, :ntok, :d].float().cpu(), vt[:, :, :d, :ntok].float().cpu()])
  pad3 = lambda xs: xs + [None] * (3 - len(xs))      # noqa: E731
  figs = []      # (every figure is printed before anything is asserted)
  for name, g, r in zip(("q", "k", "v^T"), U.qkv_token_major(*pad3(got)), U.qkv_token_major(*pad3(U.qkv_layout(y_ref, B, ntok, heads, d)))):
    figs.append((name, U.rows_figure(f"{tag} {name}", g, r), _report(f"{tag} {name}", g, r)))
  # NaN-prefilled by the wrapper: all dp columns of every token < ntok, rows 0 .. dp (+ the spare row) of V^T were written
  for x in ([q] if nseg == 1 else [q, k]):
    assert torch.isfinite(x[:, :, :ntok].float()).all()
    if dp > d:
      assert float(x[:, :, :ntok, d:].float().abs().max()) == 0
  if nseg == 3:
    assert torch.isfinite(vt[:, :, :dp + (1 if dpv > dp else 0), :ntok].float()).all()
    if dp > d:
      assert float(vt[:, :, d:dp, :ntok].float().abs().max()) == 0
    if dpv > dp:
      assert torch.all(vt[:, :, dp, :ntok].float() == 1.0)
  for name, per_row, whole in figs:
    assert per_row < U.BAR and whole < U.BAR, (tag, name, per_row, whole)


def _run_qkv(cuda, C, heads, d, nseg, B, ntok, P, splitk=1, ln_rows=0):
  from gill_amd import ops
  M = B * ntok
  t, g, beta, W, b = U.case_operands(M, C, nseg * C, bool(ln_rows))
  outs = ops.ln_gemm_qkv(_bf(t).to(cuda), _planes_for(t, P, ln_rows, cuda), g.to(cuda), beta.to(cuda), _bf(W).to(cuda), b.to(cuda), heads, ntok,
                         ln_rows=ln_rows, splitk=splitk)
  _assert_qkv(f"ln_gemm qkv C={C} h={heads} nseg={nseg} M={M} ntok={ntok} P={P} sk={splitk} ln_rows={ln_rows}", outs,
              _consumer_ref(M, C, nseg * C, bool(ln_rows)), B, ntok, heads, d)


@pytest.mark.parametrize("ntok", [64, 100])
@pytest.mark.parametrize("nseg", [3, 1])
@pytest.mark.parametrize("C,heads,d,P", [(320, 8, 40, 4), (640, 8, 80, 10), (1280, 8, 160, 20), (640, 10, 64, 1)])
def test_ln_gemm_qkv(cuda, C, heads, d, P, nseg, ntok):
  """norm1 -> attn1.to_q / to_k / to_v (nseg 3) and norm2 -> attn2.to_q (nseg 1) as xf() launches them, B = 2: M = 128, or M = 200 with ntok = 100 padded to
  128 token rows and tiles that straddle the two samples.  N = nseg * heads * dp is a multiple of 128 in every geometry, so plan_tile_width() = 128 and the few
  tiles run gemm_kernel<4, 128, 0, 3, 3, 64, 2> (64-row four-wave tile, scatter epilogue EPI 3).  Padded head dims: 40 -> 48 and 80 -> 80 with a spare V^T row
  (dpv 64 / 96), 160 and 64 without (dpv == dp).  Planes: 4, 10 (the predicated tail of the 4-at-a-time reader), 20 (LN_MAX_PLANES) and 1."""
  _run_qkv(cuda, C, heads, d, nseg, 2, ntok, P)


def test_ln_gemm_qkv_one_128_row_tile(cuda):
  """M = 64: plan_waves() keeps nwv = 4, mi = 4 and plan_kernel() puts the scatter epilogue on the eight-wave 128 x 128 tile
  gemm_kernel<8, 128, 0, 3, 2, 64, 2>; rows 64 .. 127 of the tile are beyond M."""
  _run_qkv(cuda, 640, 8, 80, 3, 1, 64, 10)


def test_ln_gemm_qkv_pingpong_256_row_tile(cuda):
  """M = 4096, C = 640, N = 1920: gemm_qkv_pingpong_mi() = 4 (16 x 12 = 192 workgroups of 256 x 160: 75 % of a round, no worse than 128-row tiles), so
  plan_tile_width() stays 160 and the scatter epilogue runs on the ping-pong kernel gemm_kernel<8, 160, 0, 3, 3> — level 1 at UNet batch 4."""
  _run_qkv(cuda, 640, 8, 80, 3, 4, 1024, 8)


@pytest.mark.parametrize("C,heads,d,nseg,B,ntok,P,sk", [
  (640, 8, 80, 3, 2, 64, 10, 2),       # M = 128
  (1280, 8, 160, 1, 1, 64, 20, 2),     # M = 64
  (320, 8, 40, 3, 2, 100, 4, 2),       # M = 200: ragged in the reducer's 16-row blocks, K = 320 split 3 + 2 steps, pad columns and the spare row from store4()
  (1280, 8, 160, 3, 2, 64, 16, 0),     # auto: gemm_pick_splitk() = 5 (24 tiles, 20 K steps)
])
def test_ln_gemm_qkv_splitk(cuda, C, heads, d, nseg, B, ntok, P, sk):
  """Split-K: gemm_kernel<4, 128, 0, 2, 2> writes fp32 partials and gemm_splitk_reduce_kernel<64, 1> applies the folded LayerNorm (its ln_stats branch:
  ln_row_factors() per row, the column sums per quad) and scatters through store4()'s OUT_QKV branch."""
  _run_qkv(cuda, C, heads, d, nseg, B, ntok, P, splitk=sk)


@pytest.mark.parametrize("P", [1, 4, 10, 20])
def test_ln_gemm_qkv_plane_counts(cuda, P):
  """One shape (C = 640, M = 200, nseg 3), the true row sums split over 1, 4, 10 and 20 planes with random positive weights: ln_row_factors() adds them
  four at a time, P = 10 ends in a predicated pair, P = 1 in a predicated triple."""
  _run_qkv(cuda, 640, 8, 80, 3, 2, 100, P)


@pytest.mark.parametrize("C,heads,d,nseg,P,sk", [(640, 8, 80, 1, 4, 1), (1280, 8, 160, 1, 20, 1), (640, 8, 80, 3, 10, 2)])
def test_ln_gemm_qkv_ln_rows_wrap(cuda, C, heads, d, nseg, P, sk):
  """ln_rows = M / 2: the second half of t repeats the first and the planes cover only M / 2 rows (the shared classifier-free-guidance prefix: attn2.to_q
  after out1 ran on half the batch) — rows m >= ln_rows must read the sums of row m - ln_rows, in the scatter epilogue and in the split-K reducer."""
  _run_qkv(cuda, C, heads, d, nseg, 2, 64, P, splitk=sk, ln_rows=64)


def _run_geglu(cuda, M, C, P, ln_rows=0):
  from gill_amd import ops
  t, g, beta, W, b = U.case_operands(M, C, 8 * C, bool(ln_rows))
  out = ops.ln_gemm_geglu(_bf(t).to(cuda), _planes_for(t, P, ln_rows, cuda), g.to(cuda), beta.to(cuda), _bf(W).to(cuda), b.to(cuda), ln_rows=ln_rows)
  ref = U.geglu(_consumer_ref(M, C, 8 * C, bool(ln_rows)))
  tag = f"ln_gemm geglu M={M} C={C} P={P} ln_rows={ln_rows}"
  per_row, whole = U.rows_figure(tag, out, ref), _report(tag, out, ref)
  assert torch.isfinite(out.float()).all()          # (NaN-prefilled: every tile was written)
  assert per_row < U.BAR and whole < U.BAR, (tag, per_row, whole)


@pytest.mark.parametrize("M,C,P,ln_rows", [
  (128, 640, 10, 0), (200, 640, 4, 0), (128, 1280, 20, 0), (200, 1280, 10, 0),      # few tiles: the 64-row two-wave tile gemm_kernel<2, 128, 0, 1, 2>
  (64, 1280, 16, 0),                   # one 128-row tile: gemm_kernel<8, 128, 0, 1, 2, 64, 2>, rows 64 .. 127 beyond M
  (200, 1280, 10, 100),                # ln_rows = M / 2 in the GEGLU epilogue
  (4096, 640, 8, 0),                   # 32 x 40 tiles of 128 x 128: gemm_kernel<8, 128, 0, 1, 2, 64, 2> walking 3 N tiles per workgroup (npw) with the deferred stage
])
def test_ln_gemm_geglu(cuda, M, C, P, ln_rows):
  """norm3 -> ff.net.0 (GEGLU, inner = 4 C) as xf() launches it: value / gate rows interleaved as gill_op_geglu does, the folded LayerNorm applied to both
  halves in the GEGLU epilogue (EPI 1)."""
  _run_geglu(cuda, M, C, P, ln_rows)


def test_ln_gemm_refusals(cuda):
  """What the launcher does not implement it must refuse, not compute wrongly: GEGLU under split-K, more planes than LN_MAX_PLANES."""
  from gill_amd import ops
  from gill_amd._native import GillNativeError
  M, C = 128, 640
  t, g, beta, W, b = U.case_operands(M, C, 8 * C)
  dev = lambda P: (_bf(t).to(cuda), _planes_for(t, P, 0, cuda), g.to(cuda), beta.to(cuda), _bf(W).to(cuda), b.to(cuda))      # noqa: E731
  with pytest.raises(GillNativeError, match="split-K cannot be combined with GEGLU"):
    ops.ln_gemm_geglu(*dev(4), splitk=2)
  with pytest.raises(GillNativeError, match="ln_planes"):
    ops.ln_gemm_geglu(*dev(21))


# ------------------------------------------------------------------------------------------------ producer -> consumer
def _chain(cuda, C, sk):
  """x (200, C) -> t = x W1^T + b1 with its planes (ops.linear_rowstats) -> q / k / v^T and GEGLU of LN(t) from those planes."""
  from gill_amd import ops
  M, heads = 200, 8
  a, w1, b1, _, _ = U.producer_operands(M, C, C)
  t, planes, _ = ops.linear_rowstats(_bf(a).to(cuda), _bf(w1).to(cuda), b1.to(cuda), splitk=sk)
  _, g, beta, W, b = U.case_operands(M, C, 3 * C)
  _, g3, beta3, W3, b3 = U.case_operands(M, C, 8 * C)
  qkv = ops.ln_gemm_qkv(t, planes, g.to(cuda), beta.to(cuda), _bf(W).to(cuda), b.to(cuda), heads, 100)
  ff = ops.ln_gemm_geglu(t, planes, g3.to(cuda), beta3.to(cuda), _bf(W3).to(cuda), b3.to(cuda))
  return (a @ w1.T + b1, (g, beta, W, b), (g3, beta3, W3, b3)), (t, planes, qkv, ff)


@pytest.mark.parametrize("C,sk,want_planes", [(640, 1, 10), (640, 2, 10), (1280, 1, 20), (1280, 3, 20)])
def test_chain_producer_planes_into_consumer(cuda, C, sk, want_planes):
  """The producer's real planes (epilogue: sk 1; reducer: sk 2 / 3) fed straight into both consumers, M = 200: t against fp32 at 6e-3, q / k / v^T and GEGLU
  against fp32 LayerNorm + Linear of the t the producer STORED at 1e-2 — the only place a plane layout the two sides disagree on would show."""
  (t_ref, qkv_ops, ff_ops), (t, planes, qkv, ff) = _chain(cuda, C, sk)
  assert planes.shape[0] == want_planes
  assert _report(f"chain C={C} sk={sk} t", t, t_ref) < U.T_BAR
  ts = t.float().cpu()
  _assert_qkv(f"chain C={C} sk={sk}", qkv, U.ln_linear_ref(ts, *qkv_ops), 2, 100, 8, C // 8)
  ref = U.geglu(U.ln_linear_ref(ts, *ff_ops))
  per_row, whole = U.rows_figure(f"chain C={C} sk={sk} geglu", ff, ref), _report(f"chain C={C} sk={sk} geglu", ff, ref)
  assert torch.isfinite(ff.float()).all() and per_row < U.BAR and whole < U.BAR


@pytest.mark.parametrize("C,sk", [(640, 1), (1280, 3)])
def test_chain_is_bit_reproducible(cuda, C, sk):
  """ops.h promises fixed-order sums (each partial written once, added in index order, no atomics): two runs of one chain are bit-identical — the
  residual stream, the planes, q / k / v^T with their pads, GEGLU."""
  _, (t1, p1, qkv1, ff1) = _chain(cuda, C, sk)
  _, (t2, p2, qkv2, ff2) = _chain(cuda, C, sk)
  bits = lambda x: x.contiguous().view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32)      # noqa: E731  (NaN-prefilled pads compare equal)
  for name, x, y in [("t", t1, t2), ("planes", p1, p2), ("geglu", ff1, ff2)] + [(n, x, y) for n, x, y in zip(("q", "k", "v^T"), qkv1, qkv2)]:
    assert torch.equal(bits(x), bits(y)), name
