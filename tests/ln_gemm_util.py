"""Shared by test_ln_gemm_gpu.py and test_ln_gemm_host.py (not a test module): the folded-LayerNorm consumer of csrc/gemm.hip.

  * `ln_operands`: the operands both files use.  Rows of T differ from each other (per-row scale in [0.5, 3], per-row mean offset in
    [-1, 1]), so a row that reads another row's statistics cannot pass; gain 1 + 0.2 N(0,1), LayerNorm bias 0.1 N(0,1), weights
    0.06 N(0,1), everything the kernels read as bf16 rounded to bf16;
  * `ln_linear_ref`: the reference, a plain fp32 F.layer_norm(T) @ W.T + b on those operands;
  * `row_sums` / `split_planes`: the true {sum, sum of squares} of every row of T and a split of them over P planes with random positive
    weights (what a producer with P column ranges would have filed, up to the split itself);
  * `consumer_emulation`: a torch restatement of what the kernels compute (gemm.hip ln_row_factors() + the GEGLU / QKV epilogues: fp32
    plane sums, bf16(W * g) weights, rstd * acc - mean * rstd * colsum + (beta W^T + b)), with a `defect=` switch that breaks it in one of
    the ways the real path could be broken;
  * `geglu` / `qkv_layout` / `qkv_token_major`: GEGLU, the head-major q / k / v^T scatter (with its layout defects) and its inverse.

BAR is the project's q / k / v^T and GEGLU bar (test_ops_gpu.py: test_lnproj_*, test_geglu): max abs error over the row's (the tensor's)
max |ref|, per row (kv_cache_util.report_rows) and over the whole tensor (test_ops_gpu._report)."""
import functools

import torch
import torch.nn.functional as F

from kv_cache_util import bf, report_rows

BAR = 1e-2
T_BAR = 6e-3                 # the residual stream against fp32: test_lnproj_*'s bar
PLANE_RTOL, PLANE_ATOL = 2e-4, 2e-3          # the planes against sums of the stored tensor: test_ffn_fused_vs_torch's bar for its partial sums
EPS = 1e-5
LOG2E = 1.4426950408889634

STAT_DEFECTS = ("dropped_plane", "stats_shifted_one_row", "last_row_takes_neighbour", "unfolded_colsum", "missing_beta_w")
LAYOUT_DEFECTS = ("qscale_on_k", "vt_untransposed", "vt_one_token_off")


def _rnd(shape, seed, scale=1.0):
  g = torch.Generator().manual_seed(seed)
  return torch.randn(shape, generator=g) * scale


def _uniform(shape, seed, lo, hi):
  g = torch.Generator().manual_seed(seed)
  return lo + (hi - lo) * torch.rand(shape, generator=g)


def distinct_rows(M, C, seed):
  """(M, C) fp32: N(0,1) rows times a per-row scale in [0.5, 3] plus a per-row offset in [-1, 1]."""
  return _rnd((M, C), seed) * _uniform((M, 1), seed + 1, 0.5, 3.0) + _uniform((M, 1), seed + 2, -1.0, 1.0)


@functools.lru_cache(maxsize=None)
def ln_operands(M, C, N, seed, dup_half=False):
  """(t (M,C), g (C), beta (C), W (N,C), b (N)) fp32 tensors; t and W hold bf16 values.  dup_half: the second half of t repeats the first
  (a classifier-free-guidance pair before its first cross-attention)."""
  t = bf(distinct_rows(M // 2 if dup_half else M, C, seed))
  if dup_half:
    t = torch.cat([t, t], 0)
  return (t, 1.0 + 0.2 * _rnd((C,), seed + 3), 0.1 * _rnd((C,), seed + 4), bf(_rnd((N, C), seed + 5, 0.06)), 0.1 * _rnd((N,), seed + 6))


def ln_linear_ref(t, g, beta, W, b):
  return F.layer_norm(t.float(), (t.shape[-1],), g, beta, EPS) @ W.float().T + (0 if b is None else b)


def row_sums(t):
  t = t.float()
  return torch.stack([t.sum(-1), (t * t).sum(-1)], -1)           # (rows, 2)


def split_planes(sums, P, seed):
  """(P, rows, 2) fp32 that add up to sums (rows, 2): random positive weights per (plane, row, moment)."""
  w = _uniform((P,) + tuple(sums.shape), seed, 0.2, 1.0)
  return (sums[None] * (w / w.sum(0, keepdim=True))).float().contiguous()


def consumer_emulation(t, planes, g, beta, W, b, ln_rows=0, defect=None):
  """fp32 (M, N): what a folded-LayerNorm GEMM leaves in front of its GEGLU / scatter epilogue.  defect: one of STAT_DEFECTS or
  "ln_rows_wrap_ignored"."""
  t, W = t.float(), W.float()
  M, C = t.shape
  R = ln_rows or M
  P = planes.shape[0]
  assert planes.shape == (P, R, 2)
  if defect == "dropped_plane":
    planes = planes[:-1]
  st = torch.zeros(R, 2)
  for p in planes.float():                  # plane order
    st = st + p
  idx = torch.arange(M)
  if defect == "ln_rows_wrap_ignored" and R < M:
    # row m >= R read at (plane * R + m): that is row m - R of the NEXT plane, and past the buffer's end for the last plane (taken as zeros)
    st = torch.cat([st, st - planes[0].float()], 0)[:M]
  else:
    st = st[torch.where(idx >= R, idx - R, idx)]
  if defect == "stats_shifted_one_row":
    st = torch.roll(st, 1, 0)
  if defect == "last_row_takes_neighbour":
    st = st.clone()
    st[-1] = st[-2]
  mean = st[:, 0] / C
  var = (st[:, 1] / C - mean * mean).clamp_min(0)
  rstd = torch.rsqrt(var + EPS)
  Wf = bf(W * g)                                              # ln_fold_rows_kernel: one rounding of the product
  colsum = (W if defect == "unfolded_colsum" else Wf).sum(-1)
  bias = torch.zeros(W.shape[0]) if b is None else b.clone()
  if defect != "missing_beta_w":
    bias = bias + W @ beta
  return rstd[:, None] * (t @ Wf.T) - (mean * rstd)[:, None] * colsum + bias


def geglu(y):
  h = y.shape[-1] // 2
  return y[:, :h] * F.gelu(y[:, h:])


def qscale(d):
  return LOG2E / d ** 0.5


def qkv_layout(y, B, ntok, heads, d, defect=None):
  """y (B * ntok, nseg * heads * d) -> [q (B,h,ntok,d) * qscale, k (B,h,ntok,d), vt (B,h,d,ntok)] (the first nseg of them), as the scatter
  epilogue lays them out (pads left out).  defect: one of LAYOUT_DEFECTS."""
  C = heads * d
  heads_of = lambda v: v.reshape(B, ntok, heads, d).permute(0, 2, 1, 3)      # noqa: E731
  out = [heads_of(y[:, :C]) * qscale(d)]
  if y.shape[1] == 3 * C:
    k, v = heads_of(y[:, C:2 * C]), heads_of(y[:, 2 * C:])
    if defect == "qscale_on_k":
      k = k * qscale(d)
    vt = v.transpose(2, 3)
    if defect == "vt_untransposed":                           # the (tok, d) block stored as it is where a (d, tok) block belongs
      vt = v.contiguous().reshape(B, heads, d, ntok)
    if defect == "vt_one_token_off":                          # every token one column late; column 0 keeps what was there (zeros)
      vt = torch.cat([torch.zeros_like(vt[..., :1]), vt[..., :-1]], -1)
    out += [k, vt]
  return out


def qkv_token_major(q, k, vt):
  """The inverse of qkv_layout on its unpadded outputs: [(B * ntok, heads * d)] per operand (q still scaled), for per-row figures."""
  back = lambda v: v.permute(0, 2, 1, 3).reshape(v.shape[0] * v.shape[2], -1)      # noqa: E731
  return [back(q)] + ([] if k is None else [back(k), back(vt.transpose(2, 3))])


def rows_figure(name, got, ref):
  """kv_cache_util.report_rows on a (rows, columns) pair."""
  return report_rows(name, got.float().cpu()[None], ref.float().cpu()[None])


def case_operands(M, C, N, dup_half=False):
  """ln_operands with the seed both test files use for this shape."""
  return ln_operands(M, C, N, 500 + M + C + N, dup_half)


@functools.lru_cache(maxsize=None)
def producer_operands(M, N, K):
  """The producer cases' operands: a (M,K) with rows that differ (distinct_rows), w (N,K) 0.06 N(0,1), bias, residual, and the fp32 result."""
  seed = 300 + M + N + K
  a, w = bf(distinct_rows(M, K, seed)), bf(_rnd((N, K), seed + 3, 0.06))
  bias, resid = 0.2 * _rnd((N,), seed + 4), bf(_rnd((M, N), seed + 5))
  return a, w, bias, resid, a @ w.T + bias + resid
