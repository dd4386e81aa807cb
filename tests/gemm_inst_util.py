"""Shared by test_gemm_inst_host.py, test_gemm_inst_gpu.py and tools/gemm_inst_tolerance.py (not a test module): ONE OPERATOR CALL PER
REACHABLE gemm_kernel INSTANTIATION, at the edges of its own tile.

  * `CASES`: for each of the 56 instantiations the planner can reach (tests/test_gemm_plan_host.py) the smallest `ops` call that lands on it,
    plus edge variants (ragged M / N, uneven split-K, N-tile walks, the tile -> workgroup maps, the convolution and epilogue features).  A case
    names the wrapper (`op`), its arguments, the instantiation of its main launch, how many GEMM launches the call makes and the plan
    properties it claims (`tile_rows`, `npw`, `n_major`, `xb_m`, ragged M / N, uneven split ...).
  * `descriptor(case)`: the gill_gemm_plan descriptor of the case's main launch, built the way the operator entry (csrc/capi.hip,
    csrc/unet_ops.hip) builds its GemmArgs — split factors, blocked weights and K order from gill_gemm_query.  The host test plans it under
    (PP 1, COOP 1, 256 CUs); the GPU test does not trust it and reads what the launcher ran from ops.gemm_plan_log().
  * `bar()` / `judge_*`: how results are judged.  The reference is fp64 on the CPU from the same bf16-rounded operands.
      exact pass   small-integer operands (A in [-2, 3], W in [-3, 2], bias in [-8, 8], residual in [-64, 64], alpha = 1): every partial sum
                   is an integer below 2^24 (|sum| <= 9 K + 72 for K <= 11520), exact in fp32 in any order, so the output must be the bf16
                   (fp32) rounding of the fp64 result, bit for bit;
      random pass  |got - ref| <= u |ref| + (K + 4) 2^-24 S per element, S = |alpha| |A| |W|^T + |bias| + |resid| in fp64, u = 2^-8 for bf16
                   and 2^-24 for fp32 output: round-to-nearest bf16 has unit roundoff 2^-8, bf16 x bf16 products are exact in fp32, K fp32
                   additions in any order err by at most (K - 1) 2^-24 sum |terms|, the epilogue adds a few more.  A bound: no margin;
      activations  that bar on the pre-activation times the activation's Lipschitz constant (ReLU 1, SiLU 1.1, GELU 1.13) plus
                   c_act |pre| for the kernel's transcendental approximation, c_act from tests/golden/gemm_inst_tolerance.json (measured on
                   the fp32-output path against fp64 by tools/gemm_inst_tolerance.py, times 4);
      GEGLU, QKV, softmax-80, GroupNorm finish, fused statistics: the bars and references of the standing operator tests, unchanged.
"""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

import gemm_plan_util as U
from gill_amd import ops

MAC_CAP = 8e9                     # multiply-adds (M N K) of a case's main launch
PLAN_ENV = (1, 1, 256)            # (GILL_GEMM_PP, GILL_GEMM_COOP, CUs) the table is chosen under: the defaults on an MI355X
R = U.R
TOLERANCE_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_inst_tolerance.json")
LIPSCHITZ = {"none": 1.0, "relu": 1.0, "silu": 1.1, "gelu": 1.13}      # sup |act'|: SiLU 1.0998, GELU (erf) 1.1290
ACT_CODE = {"none": U.ACT_NONE, "relu": U.ACT_RELU, "gelu": U.ACT_GELU, "silu": U.ACT_SILU}
ACT_FP64 = {"none": lambda v: v, "relu": F.relu, "silu": F.silu, "gelu": F.gelu}
# c_act cannot be below the fp32 arithmetic of the activation itself: exp2, add, reciprocal, multiply = four roundings of 2^-24
ACT_TERM_FLOOR = 4 * 2.0 ** -24
ACT_TERM_MARGIN = 4.0


class Case:
  def __init__(self, id, op, inst, launches=1, claims=None, over_cap=None, **kw):
    self.id, self.op, self.inst, self.launches, self.claims, self.over_cap, self.kw = id, op, tuple(inst), launches, dict(claims or {}), over_cap, kw

  def __repr__(self):
    return self.id


def _gemm(id, inst, M, N, K, claims=None, **kw):
  return Case(id, "gemm", inst, claims=claims, M=M, N=N, K=K, **kw)


def _conv(id, inst, B, H, C1, Cout, claims=None, **kw):
  return Case(id, "conv", inst, claims=claims, B=B, H=H, C1=C1, Cout=Cout, **kw)


def _cases():
  c = []
  # ---- STREAM64 (128 x 64, blocked weights): N K >= 4 Mi, K >= 1024, up to 256 rows
  c += [_gemm("stream64", (8, 64, 0, 0, 6, 64, 2), 8, 4096, 1024, bias=True, splitk=1),
        _gemm("stream64-ragged-m-relu-f32", (8, 64, 0, 0, 6, 64, 2), 100, 4096, 1024, bias=True, act="relu", out_f32=True, splitk=1, claims=dict(ragged_m=1)),
        _gemm("stream64-two-m-tiles-resid", (8, 64, 0, 0, 6, 64, 2), 200, 4096, 1024, bias=True, resid="bf16", splitk=1, claims=dict(ragged_m=1, tiles_m=2)),
        _gemm("stream64-split", (8, 64, 0, 2, 6, 64, 2), 64, 1024, 4096, bias=True, splitk=4),
        _gemm("stream64-split-uneven", (8, 64, 0, 2, 6, 64, 2), 100, 1024, 4096 + 64, bias=True, resid="bf16", splitk=3, claims=dict(uneven_split=1, ragged_m=1)),
        Case("stream64-qkv", "qkv", (8, 64, 0, 3, 6, 64, 2), C=1280, heads=8, d=160, nseg=3, B=1, ntok=77, ln=False, claims=dict(ragged_m=1))]
  # ---- plain GEMMs on the 128-wide tiles
  c += [_gemm("p128-2w-act-stats", (2, 128, 0, 0, 2, 64, 4), 128, 512, 512, bias=True, act="silu", gn=dict(bin=16, rpb=64), claims=dict(tile_rows=64)),
        _gemm("p128-2w-stats", (2, 128, 0, 4, 2, 64, 4), 128, 512, 64, bias=True, resid="bf16", gn=dict(bin=16, rpb=64), claims=dict(tile_rows=64)),
        _gemm("p128-4w128-relu", (4, 128, 0, 0, 2, 64, 4), 64, 128, 64, bias=True, act="relu", splitk=1, claims=dict(tile_rows=128)),
        _gemm("p128-4w128-gelu-ragged-m-n", (4, 128, 0, 0, 2, 64, 4), 50, 132, 192, bias=True, resid="bf16", act="gelu", alpha=0.5, splitk=1,
              claims=dict(tile_rows=128, ragged_m=1, ragged_n=1)),
        _gemm("p128-4w128-silu-f32-two-m-tiles", (4, 128, 0, 0, 2, 64, 4), 200, 128 * 150, 64, bias=True, act="silu", out_f32=True, splitk=1,
              claims=dict(tile_rows=128, ragged_m=1, tiles_m=2)),
        _gemm("p128-4w128-f32", (4, 128, 0, 0, 2, 64, 4), 64, 256, 128, bias=True, out_f32=True, alpha=0.5, splitk=1, claims=dict(tile_rows=128)),
        _gemm("p128-4w64-silu", (4, 128, 0, 0, 3, 64, 2), 128, 256, 256, bias=True, act="silu", splitk=1, claims=dict(tile_rows=64)),
        _gemm("p128-4w64-relu-ragged-m-n", (4, 128, 0, 0, 3, 64, 2), 100, 644, 128, bias=True, act="relu", resid="bf16", splitk=1,
              claims=dict(tile_rows=64, ragged_m=1, ragged_n=1, tiles_m=2)),
        _gemm("p128-4w64-gelu-f32", (4, 128, 0, 0, 3, 64, 2), 200, 256, 128, bias=True, act="gelu", out_f32=True, splitk=1, claims=dict(tile_rows=64, ragged_m=1)),
        _gemm("p128-split", (4, 128, 0, 2, 2, 64, 4), 130, 384, 1024, bias=True, splitk=4, claims=dict(ragged_m=1, tiles_m=2)),
        _gemm("p128-split-uneven-ragged-n-f32", (4, 128, 0, 2, 2, 64, 4), 50, 132, 448, bias=True, resid="bf16", out_f32=True, splitk=3,
              claims=dict(uneven_split=1, ragged_m=1, ragged_n=1)),
        _gemm("p128-4w128", (4, 128, 0, 4, 2, 64, 4), 64, 128, 64, bias=True, splitk=1, claims=dict(tile_rows=128)),
        _gemm("p128-4w128-ragged-m-n-resid", (4, 128, 0, 4, 2, 64, 4), 50, 132, 192, bias=True, resid="bf16", splitk=1, claims=dict(ragged_m=1, ragged_n=1)),
        _gemm("p128-4w64", (4, 128, 0, 4, 3, 64, 2), 128, 128, 64, bias=True, splitk=1, claims=dict(tile_rows=64)),
        _gemm("p128-4w64-ragged-m-n-walk", (4, 128, 0, 4, 3, 64, 2), 100, 644, 192, bias=True, resid="bf16", splitk=1,
              claims=dict(tile_rows=64, ragged_m=1, ragged_n=1, tiles_m=2))]
  # ---- GEGLU (EPI 1)
  c += [Case("geglu-2w", "geglu", (2, 128, 0, 1, 2, 64, 4), M=128, inner=1280, K=320, claims=dict(tile_rows=64)),
        Case("geglu-2w-ragged-m-ln", "geglu", (2, 128, 0, 1, 2, 64, 4), M=200, inner=2560, K=640, ln=True, P=4, claims=dict(tile_rows=64, ragged_m=1)),
        Case("geglu-8w", "geglu", (8, 128, 0, 1, 2, 64, 2), M=64, inner=128, K=64, claims=dict(tile_rows=128)),
        Case("geglu-8w-walk-even", "geglu", (8, 128, 0, 1, 2, 64, 2), M=4096, inner=1280, K=64, claims=dict(tile_rows=128, npw=2, walk_even=1)),
        Case("geglu-8w-walk-ragged", "geglu", (8, 128, 0, 1, 2, 64, 2), M=8192, inner=1280, K=320, claims=dict(tile_rows=128, npw=3, walk_ragged=1))]
  # ---- QKV scatter (EPI 3)
  c += [Case("qkv-4w64", "qkv", (4, 128, 0, 3, 3, 64, 2), C=640, heads=8, d=80, nseg=3, B=2, ntok=64, ln=True, P=10, claims=dict(tile_rows=64)),
        Case("qkv-4w64-ragged-m", "qkv", (4, 128, 0, 3, 3, 64, 2), C=320, heads=8, d=40, nseg=3, B=2, ntok=100, ln=True, P=4, claims=dict(tile_rows=64, ragged_m=1)),
        Case("qkv-8w128", "qkv", (8, 128, 0, 3, 2, 64, 2), C=640, heads=8, d=80, nseg=3, B=1, ntok=64, ln=True, P=10, claims=dict(tile_rows=128, ragged_m=1)),
        Case("qkv-2w-160", "qkv", (2, 160, 0, 3, 2, 64, 4), C=320, heads=4, d=80, nseg=1, B=2, ntok=64, ln=True, P=4, claims=dict(tile_rows=64)),
        Case("qkv-2w-160-ragged-m", "qkv", (2, 160, 0, 3, 2, 64, 4), C=320, heads=4, d=80, nseg=1, B=2, ntok=100, ln=True, P=4, claims=dict(tile_rows=64, ragged_m=1)),
        Case("qkv-4w-160", "qkv", (4, 160, 0, 3, 2, 64, 4), C=320, heads=4, d=80, nseg=1, B=1, ntok=64, ln=True, P=4, claims=dict(tile_rows=128, ragged_m=1)),
        Case("qkv-pingpong-256", "qkv", (8, 160, 0, 3, 3, 64, 4), C=640, heads=8, d=80, nseg=3, B=4, ntok=1024, ln=True, P=8, claims=dict(tile_rows=256))]
  # ---- plain GEMMs on the 160-wide tiles
  c += [_gemm("p160-2w-silu", (2, 160, 0, 0, 2, 64, 4), 128, 320, 320, bias=True, act="silu", splitk=1, claims=dict(tile_rows=64)),
        _gemm("p160-2w-gelu-f32-ragged-m", (2, 160, 0, 0, 2, 64, 4), 100, 320, 128, bias=True, act="gelu", out_f32=True, resid="bf16", alpha=0.5, splitk=1,
              claims=dict(tile_rows=64, ragged_m=1, tiles_m=2)),
        _gemm("p160-4w64-resid-f32", (4, 160, 0, 0, 2, 64, 2), 128, 320, 320, bias=True, resid="f32", splitk=1, claims=dict(tile_rows=64)),
        _gemm("p160-4w64-resid-f32-ragged-m", (4, 160, 0, 0, 2, 64, 2), 100, 960, 128, bias=True, resid="f32", splitk=1, claims=dict(tile_rows=64, ragged_m=1, tiles_m=2)),
        _gemm("p160-4w128-silu", (4, 160, 0, 0, 2, 64, 4), 16, 1280, 320, bias=True, act="silu", splitk=1, claims=dict(tile_rows=128, ragged_m=1, n_major=1)),
        _gemm("p160-4w128-relu-f32", (4, 160, 0, 0, 2, 64, 4), 64, 320, 128, bias=True, act="relu", out_f32=True, splitk=1, claims=dict(tile_rows=128)),
        _gemm("p160-split", (4, 160, 0, 2, 2, 64, 4), 64, 320, 576, bias=True, splitk=2, claims=dict(uneven_split=1)),
        _gemm("p160-split-ragged-m", (4, 160, 0, 2, 2, 64, 4), 200, 320, 448, bias=True, resid="bf16", splitk=3, claims=dict(uneven_split=1, ragged_m=1, tiles_m=2)),
        _gemm("p160-4w64", (4, 160, 0, 4, 2, 64, 2), 128, 320, 64, bias=True, splitk=1, claims=dict(tile_rows=64)),
        _gemm("p160-4w64-ragged-m-resid", (4, 160, 0, 4, 2, 64, 2), 100, 960, 192, bias=True, resid="bf16", splitk=1, claims=dict(tile_rows=64, ragged_m=1, tiles_m=2)),
        _gemm("p160-4w128", (4, 160, 0, 4, 2, 64, 4), 64, 320, 64, bias=True, splitk=1, claims=dict(tile_rows=128)),
        _gemm("p160-4w128-ragged-m-resid", (4, 160, 0, 4, 2, 64, 4), 50, 640, 192, bias=True, resid="bf16", splitk=1, claims=dict(tile_rows=128, ragged_m=1)),
        _gemm("p160-pp128-split", (8, 160, 0, 2, 3, 64, 2), 128, 320, 2560, bias=True, splitk=2, claims=dict(tile_rows=128)),
        _gemm("p160-pp128-split-uneven", (8, 160, 0, 2, 3, 64, 2), 256, 320, 2624, bias=True, resid="bf16", splitk=3, claims=dict(tile_rows=128, uneven_split=1)),
        _gemm("p160-pp256-split-n-major", (8, 160, 0, 2, 3, 64, 4), 256, 1920, 2560, bias=True, splitk=16, row_major=True, claims=dict(tile_rows=256, n_major=1)),
        _gemm("p160-pp128", (8, 160, 0, 4, 3, 64, 2), 128, 320, 2560, bias=True, splitk=1, claims=dict(tile_rows=128)),
        _gemm("p160-pp128-resid-two-m-tiles", (8, 160, 0, 4, 3, 64, 2), 256, 640, 2560, bias=True, resid="bf16", splitk=1, claims=dict(tile_rows=128, tiles_m=2)),
        _gemm("p160-pp256-balanced-round", (8, 160, 0, 4, 3, 64, 4), 6400, 1280, 640, bias=True, resid="bf16", splitk=1, claims=dict(tile_rows=256))]
  # ---- softmax-80 (EPI 5): the cross-attention score GEMM, between the GEMM that folds the per-sample operands (xalg_operands_launch) and the
  # values GEMM on them: three launches
  c += [Case("softmax-4w-2deep", "xattn", (4, 160, 0, 5, 2, 64, 2), launches=3, B=130, HW=64, C=320, heads=4, ctx_len=77, E=768, claims=dict(tile_rows=64)),
        Case("softmax-4w-3deep", "xattn", (4, 160, 0, 5, 3, 64, 2), launches=3, B=2, HW=64, C=640, heads=8, ctx_len=5, E=768, claims=dict(tile_rows=64)),
        Case("softmax-pp128-balanced-round", "xattn", (8, 160, 0, 5, 3, 64, 2), launches=3, B=50, HW=128, C=640, heads=8, ctx_len=80, E=768, claims=dict(tile_rows=128))]
  # ---- 3x3 convolutions, 128 wide (four waves)
  c += [_conv("c128", (4, 128, 1, 0, 2, 64, 4), 1, 8, 64, 128, splitk=1, bias=True),
        _conv("c128-ragged-m-x2-rowvec-resid", (4, 128, 1, 0, 2, 64, 4), 3, 10, 64, 128, C2=64, splitk=1, bias=True, rowvec=True, resid=True,
              claims=dict(ragged_m=1, tiles_m=3)),
        _conv("c128-stride2-pad-shift", (4, 128, 1, 0, 2, 64, 4), 2, 12, 64, 128, stride=2, pad_shift=1, splitk=1, bias=True, claims=dict(ragged_m=1)),
        _conv("c128-stride2", (4, 128, 1, 0, 2, 64, 4), 2, 12, 64, 128, stride=2, splitk=1, bias=True, claims=dict(ragged_m=1)),
        Case("c128-shortcut", "conv_sc", (4, 128, 1, 0, 2, 64, 4), B=2, H=10, C1=64, CS1=64, CS2=64, Cout=128, splitk=1, claims=dict(ragged_m=1, tiles_m=2)),
        _conv("c128-split-uneven", (4, 128, 1, 2, 2, 64, 4), 1, 10, 64, 128, splitk=2, bias=True, resid=True, claims=dict(uneven_split=1, ragged_m=1)),
        _conv("c128-ups9", (4, 128, 2, 0, 2, 64, 4), 1, 4, 64, 128, ups=True, splitk=1, bias=True, rowvec=True),
        _conv("c128-ups9-split-ragged-m", (4, 128, 2, 2, 2, 64, 4), 1, 5, 64, 128, ups=True, splitk=2, bias=True, resid=True, claims=dict(uneven_split=1, ragged_m=1)),
        _conv("c128-ups4", (4, 128, 3, 0, 2, 64, 4), 1, 4, 64, 128, ups=True, splitk=1, bias=True, claims=dict(ragged_m=1)),
        _conv("c128-ups4-two-m-tiles-x2", (4, 128, 3, 0, 2, 64, 4), 2, 10, 64, 128, C2=64, ups=True, splitk=1, bias=True, claims=dict(ragged_m=1, tiles_m=2)),
        _conv("c128-ups4-split", (4, 128, 3, 2, 2, 64, 4), 1, 6, 128, 128, ups=True, splitk=3, bias=True, claims=dict(uneven_split=1, ragged_m=1))]
  # ---- 3x3 convolutions, 160 wide: four waves where the rows are no multiple of 256
  c += [_conv("c160-4w", (4, 160, 1, 0, 2, 64, 4), 1, 8, 64, 320, splitk=1, bias=True, claims=dict(ragged_m=1)),
        _conv("c160-4w-ragged-m-x2-rowvec-resid", (4, 160, 1, 0, 2, 64, 4), 3, 10, 64, 160, C2=64, splitk=1, bias=True, rowvec=True, resid=True,
              claims=dict(ragged_m=1, tiles_m=3)),
        _conv("c160-4w-stride2-pad-shift", (4, 160, 1, 0, 2, 64, 4), 2, 12, 64, 160, stride=2, pad_shift=1, splitk=1, bias=True, claims=dict(ragged_m=1)),
        Case("c160-4w-shortcut", "conv_sc", (4, 160, 1, 0, 2, 64, 4), B=2, H=10, C1=64, CS1=64, CS2=0, Cout=160, splitk=1, claims=dict(ragged_m=1, tiles_m=2)),
        _conv("c160-4w-split-uneven", (4, 160, 1, 2, 2, 64, 4), 1, 10, 64, 320, splitk=2, bias=True, rowvec=True, claims=dict(uneven_split=1, ragged_m=1)),
        _conv("c160-4w-ups9", (4, 160, 2, 0, 2, 64, 4), 1, 4, 64, 320, ups=True, splitk=1, bias=True, rowvec=True, claims=dict(ragged_m=1)),
        _conv("c160-4w-ups9-split", (4, 160, 2, 2, 2, 64, 4), 1, 4, 64, 320, ups=True, splitk=2, bias=True, resid=True, claims=dict(uneven_split=1, ragged_m=1)),
        _conv("c160-4w-ups4", (4, 160, 3, 0, 2, 64, 4), 1, 4, 64, 320, ups=True, splitk=1, bias=True, claims=dict(ragged_m=1)),
        _conv("c160-4w-ups4-split", (4, 160, 3, 2, 2, 64, 4), 2, 10, 128, 160, ups=True, splitk=3, bias=True, claims=dict(uneven_split=1, ragged_m=1, tiles_m=2))]
  # ---- ... the ping-pong tiles (rows a multiple of 256): 128 rows, 256 rows where (M / 256) (N / 160) splitk > 128
  c += [_conv("c160-pp128", (8, 160, 1, 0, 3, 64, 2), 1, 16, 64, 320, splitk=1, bias=True, claims=dict(tile_rows=128, n_major=0, xb_m=0)),
        _conv("c160-pp128-x2-rowvec-resid", (8, 160, 1, 0, 3, 64, 2), 2, 16, 64, 160, C2=64, splitk=1, bias=True, rowvec=True, resid=True, claims=dict(tile_rows=128)),
        _conv("c160-pp128-stride2-pad-shift", (8, 160, 1, 0, 3, 64, 2), 1, 32, 64, 160, stride=2, pad_shift=1, splitk=1, bias=True, claims=dict(tile_rows=128)),
        _conv("c160-pp128-stride2", (8, 160, 1, 0, 3, 64, 2), 1, 32, 64, 160, stride=2, splitk=1, bias=True, claims=dict(tile_rows=128)),
        _conv("c160-pp128-xcd-block-map", (8, 160, 1, 0, 3, 64, 2), 4, 16, 64, 320, splitk=1, bias=True, claims=dict(tile_rows=128, xb_m_on=1)),
        _conv("c160-pp128-n-major", (8, 160, 1, 0, 3, 64, 2), 1, 16, 64, 1280, splitk=1, bias=True, claims=dict(tile_rows=128, n_major=1)),
        Case("c160-pp128-shortcut-two-sources", "conv_sc", (8, 160, 1, 0, 3, 64, 2), B=1, H=16, C1=64, CS1=64, CS2=64, Cout=160, splitk=1, claims=dict(tile_rows=128)),
        _conv("c160-pp256", (8, 160, 1, 0, 3, 64, 4), 65, 16, 64, 320, splitk=1, bias=True, rowvec=True, claims=dict(tile_rows=256)),
        _conv("c160-pp128-split", (8, 160, 1, 2, 3, 64, 2), 1, 16, 64, 320, splitk=2, bias=True, resid=True, claims=dict(tile_rows=128, uneven_split=1)),
        _conv("c160-pp256-split", (8, 160, 1, 2, 3, 64, 4), 4, 16, 64, 1280, splitk=5, bias=True, rowvec=True, claims=dict(tile_rows=256, uneven_split=1)),
        Case("c160-pp128-gn-finish", "conv_gn", (8, 160, 1, 6, 3, 64, 2), B=1, H=16, Cin=64, Cout=320, silu=True, raw=True, rowvec=True, claims=dict(tile_rows=128)),
        Case("c160-pp128-gn-finish-resid-table", "conv_gn", (8, 160, 1, 6, 3, 64, 2), B=2, H=16, Cin=64, Cout=640, silu=False, raw=True, resid=True, table=True,
             claims=dict(tile_rows=128)),
        Case("c160-pp256-gn-finish", "conv_gn", (8, 160, 1, 6, 3, 64, 4), B=65, H=16, Cin=64, Cout=320, silu=True, raw=False, rowvec=True, claims=dict(tile_rows=256)),
        _conv("c160-pp128-ups9", (8, 160, 2, 0, 3, 64, 2), 1, 8, 64, 320, ups=True, splitk=1, bias=True, rowvec=True, claims=dict(tile_rows=128)),
        _conv("c160-pp256-ups9", (8, 160, 2, 0, 3, 64, 4), 65, 8, 64, 320, ups=True, splitk=1, bias=True, resid=True, claims=dict(tile_rows=256)),
        _conv("c160-pp128-ups9-split", (8, 160, 2, 2, 3, 64, 2), 1, 8, 64, 320, ups=True, splitk=2, bias=True, rowvec=True, claims=dict(tile_rows=128, uneven_split=1)),
        _conv("c160-pp256-ups9-split", (8, 160, 2, 2, 3, 64, 4), 4, 8, 64, 1280, ups=True, splitk=5, bias=True, resid=True, claims=dict(tile_rows=256, uneven_split=1)),
        _conv("c160-pp128-ups4", (8, 160, 3, 0, 3, 64, 2), 1, 16, 64, 320, ups=True, splitk=1, bias=True, claims=dict(tile_rows=128)),
        _conv("c160-pp128-ups4-x2", (8, 160, 3, 0, 3, 64, 2), 2, 16, 64, 160, C2=64, ups=True, splitk=1, bias=True, claims=dict(tile_rows=128)),
        _conv("c160-pp256-ups4", (8, 160, 3, 0, 3, 64, 4), 33, 16, 64, 160, ups=True, splitk=1, bias=True, claims=dict(tile_rows=256)),
        _conv("c160-pp128-ups4-split", (8, 160, 3, 2, 3, 64, 2), 1, 16, 128, 320, ups=True, splitk=3, bias=True, claims=dict(tile_rows=128, uneven_split=1)),
        _conv("c160-pp256-ups4-split", (8, 160, 3, 2, 3, 64, 4), 4, 16, 64, 1280, ups=True, splitk=2, bias=True, claims=dict(tile_rows=256))]
  return c


CASES = _cases()
assert len({k.id for k in CASES}) == len(CASES)


# ---------------------------------------------------------------------------------------------------------------- descriptors
def _q(what, *a):
  return int(ops.gemm_query([[what] + list(a) + [0] * (6 - len(a))], *PLAN_ENV)[0])


def _pick(M, N, K, act=0, plain=False):
  return _q(U.Q_PICK, M, N, K, act, int(plain), 0)


def conv_geometry(kw):
  """(Cin, OH, M, ups_form, K) of a "conv" case as op_conv3x3 (csrc/capi.hip) works them out; ups_form 2 = the four-tap parity form."""
  Cin = kw["C1"] + kw.get("C2", 0)
  H, stride = kw["H"], kw.get("stride", 1)
  ups = bool(kw.get("ups"))
  ups4 = ups and stride == 1 and not kw.get("rowvec") and not kw.get("resid")
  OH = 2 * H if ups else (H // 2 if kw.get("pad_shift") else (H - 1) // stride + 1)
  return Cin, OH, kw["B"] * OH * OH, (2 if ups4 else int(ups)), (4 if ups4 else 9) * Cin


def descriptor(case):
  """The gill_gemm_plan descriptor (54 ints) of the case's main launch."""
  kw, op = case.kw, case.op
  if op == "gemm":
    M, N, K = kw["M"], kw["N"], kw["K"]
    act = ACT_CODE[kw.get("act", "none")]
    d = dict(bias=int(bool(kw.get("bias"))), resid=int(bool(kw.get("resid"))), resid_f32=int(kw.get("resid") == "f32"), act=act,
             out_mode=U.OUT_F32 if kw.get("out_f32") else U.OUT_BF16, alpha_is_one=int(kw.get("alpha", 1.0) == 1.0))
    if "gn" in kw:      # gill_op_gemm_gn_stats
      g = kw["gn"]
      return U.plain(M, N, K, gn_stats=1, gn_groups=N // g["bin"], gn_cg=g["bin"], rows_per_batch=g["rpb"], splitk=kw.get("splitk", 1), **d)
    blk = int(not kw.get("row_major") and _q(U.Q_STREAM64_WEIGHTS, N, K))
    sk = kw.get("splitk", 0)
    if sk <= 0:
      sk = _q(U.Q_PICK_BLK64, M, N, K) if blk else _pick(M, N, K, act)
    return U.plain(M, N, K, w_blk64=blk, splitk=sk, **d)
  if op == "geglu":
    ln = dict(ln_stats=1, ln_colsum=1, ln_planes=kw["P"]) if kw.get("ln") else {}
    return U.plain(kw["M"], 2 * kw["inner"], kw["K"], act=U.ACT_GEGLU, bias=1, ldc=kw["inner"], **ln)
  if op == "qkv":
    C, heads, d, nseg, ntok = kw["C"], kw["heads"], kw["d"], kw["nseg"], kw["ntok"]
    dp = ops.padded_head_dim(d)
    N, M = nseg * heads * dp, kw["B"] * ntok
    ln = dict(ln_stats=1, ln_colsum=1, ln_planes=kw["P"]) if kw.get("ln") else {}
    blk = int(not kw.get("ln") and _q(U.Q_STREAM64_WEIGHTS, N, C))
    return U.case(M=M, N=N, K=C, out_mode=U.OUT_QKV, heads=heads, dp=dp, ntok=ntok, C=0, bias=1, w_blk64=blk, splitk=kw.get("splitk", 1), **ln)
  if op == "xattn":      # the score GEMM (xf_xalg_args, csrc/xf_args.h)
    M = kw["B"] * kw["HW"]
    return U.plain(M, 80 * kw["heads"], kw["C"], out_mode=U.OUT_SOFTMAX80, wb_rows=kw["HW"], ln_stats=1, ln_colsum=1, ln_planes=1, bias=1)
  if op == "conv":
    Cin, OH, M, upsf, K = conv_geometry(kw)
    H, stride, Cout = kw["H"], kw.get("stride", 1), kw["Cout"]
    chunked = 0 if upsf == 2 else _q(U.Q_CONV_K_CHUNKED, H * H, Cin, Cout)
    sk = kw.get("splitk", 0)
    if sk <= 0:
      sk = _pick(M, Cout, K)
    return U.case(M=M, N=Cout, K=K, conv=1, IH=H, IW=H, OH=OH, OW=OH, Cin=Cin, K1=kw["C1"], A2=int(kw.get("C2", 0) > 0), stride=stride, ups=upsf,
                  pad_shift=int(kw.get("pad_shift", 0)), k_chunked=chunked, rows_per_batch=OH * OH, bias=int(bool(kw.get("bias"))),
                  rowvec=int(bool(kw.get("rowvec"))), resid=int(bool(kw.get("resid"))), splitk=sk)
  if op == "conv_sc":
    H, C1, CS1, CS2, Cout = kw["H"], kw["C1"], kw["CS1"], kw.get("CS2", 0), kw["Cout"]
    M, K = kw["B"] * H * H, 9 * C1 + CS1 + CS2
    sk = kw.get("splitk", 0)
    if sk <= 0:
      sk = _pick(M, Cout, K)
    return U.case(M=M, N=Cout, K=K, conv=1, IH=H, IW=H, OH=H, OW=H, Cin=C1, K1=C1, KX=CS1 + CS2, KX1=CS1, X1=1, X2=int(CS2 > 0),
                  k_chunked=_q(U.Q_CONV_K_CHUNKED, H * H, C1, Cout), rows_per_batch=H * H, bias=1, splitk=sk)
  if op == "conv_gn":      # gill_op_conv3x3_gn, splitk 1, coop: bins as the engine picks them (C / 64 channels, else one group)
    H, Cin, Cout = kw["H"], kw["Cin"], kw["Cout"]
    sbin = Cout // 64 if (Cout % 64 == 0 and Cout // 64 >= 2) else Cout // 32
    return U.case(M=kw["B"] * H * H, N=Cout, K=9 * Cin, conv=1, IH=H, IW=H, OH=H, OW=H, Cin=Cin, K1=Cin, rows_per_batch=H * H, bias=1,
                  rowvec=int(bool(kw.get("rowvec"))), resid=int(bool(kw.get("resid"))), C=int(bool(kw.get("raw"))), fn_Y=1, fn_ss=int(bool(kw.get("table"))),
                  fn_gamma=1, fn_beta=1, fn_cg=Cout // 32, gn_stats=1, gn_groups=Cout // sbin, gn_cg=sbin, coop_ctr=1)
  raise ValueError(op)


def plan_row(case):
  return ops.gemm_plan(np.asarray([descriptor(case)], dtype=np.int32), *PLAN_ENV)[0]


def macs(case):
  d = dict(zip(U.CASE_FIELDS, descriptor(case)))
  return float(d["M"]) * d["N"] * d["K"]


def inst_of(row):
  return tuple(int(v) for v in row[R["k_nwv"]:R["k_mi"] + 1])


def check_claims(case, row):
  """The plan properties the case claims, on a plan row (the planner's on the host, the launcher's own on the GPU)."""
  c, g = case.claims, lambda n: int(row[R[n]])      # noqa: E731
  d = dict(zip(U.CASE_FIELDS, descriptor(case)))
  for name in ("tile_rows", "npw", "n_major", "xb_m", "tiles_m"):
    if name in c:
      assert g(name) == c[name], (case.id, name, g(name), c[name])
  if c.get("xb_m_on"):
    assert g("xb_m") > 0 and g("xb_n") > 0, (case.id, "XCD block map off")
  if c.get("ragged_m"):
    assert g("M") % g("tile_rows") != 0, (case.id, "M divides the tile rows")
  if c.get("ragged_n"):
    assert d["N"] % g("k_bn") != 0 and d["N"] % 4 == 0, (case.id, "N divides the tile width")
  if c.get("uneven_split"):
    assert g("splitk") > 1 and g("ksteps") % g("splitk") != 0 and g("reduce") == 1, (case.id, "even split")
    assert g("ksteps_per_split") * (g("splitk") - 1) < g("ksteps"), (case.id, "an empty trailing slice")
  if c.get("walk_even"):
    assert g("npw") > 1 and g("tiles_n") % g("npw") == 0, case.id
  if c.get("walk_ragged"):
    assert g("npw") > 1 and g("tiles_n") % g("npw") != 0, case.id


# ---------------------------------------------------------------------------------------------------------------- the bar
def bf(x):
  return x.to(torch.bfloat16).float()


def _gen(seed):
  return torch.Generator().manual_seed(seed)


def _randn(shape, seed, scale=1.0, mean=0.0):
  return torch.randn(shape, generator=_gen(seed)) * scale + mean


def _ints(shape, seed, lo, hi):
  return torch.randint(lo, hi + 1, shape, generator=_gen(seed)).float()


def unit_roundoff(out_f32):
  return 2.0 ** -24 if out_f32 else 2.0 ** -8


def bar(ref, S, K, out_f32=False):
  """Per-element bound of a linear epilogue (module docstring): fp64 tensors."""
  return unit_roundoff(out_f32) * ref.abs() + (K + 4) * 2.0 ** -24 * S


def act_terms():
  """{act: c_act} from tests/golden/gemm_inst_tolerance.json: max(4 x measured, the fp32 floor); ReLU is exact."""
  with open(TOLERANCE_JSON) as f:
    t = json.load(f)
  return {"none": 0.0, "relu": 0.0, "silu": float(t["silu"]["term"]), "gelu": float(t["gelu"]["term"])}


def act_term_from_measured(measured):
  return max(ACT_TERM_MARGIN * measured, ACT_TERM_FLOOR)


def act_bar(pre, S, K, act, out_f32, c_act):
  """(c): the linear bar on the pre-activation times the Lipschitz constant, plus c_act |pre|."""
  return LIPSCHITZ[act] * bar(pre, S, K, out_f32) + c_act * pre.abs()


def worst(got, ref, allowed):
  """(max of |got - ref| / allowed, elements over the bar, index of the worst) — NaN counts as over."""
  err = (got.double() - ref).abs()
  ratio = err / allowed.clamp_min(1e-300)
  ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))
  ratio = torch.where((err == 0) & torch.isfinite(err), torch.zeros_like(ratio), ratio)
  return float(ratio.max()), int((ratio > 1).sum()), int(ratio.argmax())


def round_out(ref, out_f32):
  """The output format's round-to-nearest-even of an fp64 tensor (through fp32, which the exact pass's integers survive)."""
  return ref.float() if out_f32 else ref.float().to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------------------------- operands and references
def gemm_operands(kw, exact, seed=0):
  """a (M,K), w (N,K) holding bf16 values, bias, resid (bf16 values unless fp32), alpha.  exact: the small-integer operands; else asymmetric
  random ones (non-zero means, different scales for A and W)."""
  M, N, K = kw["M"], kw["N"], kw["K"]
  s = 1000 + seed + M + 3 * N + 7 * K
  if exact:
    a, w = _ints((M, K), s, -2, 3), _ints((N, K), s + 1, -3, 2)
    bias = _ints((N,), s + 2, -8, 8) if kw.get("bias") else None
    resid = _ints((M, N), s + 3, -64, 64) if kw.get("resid") else None
    return a, w, bias, resid, 1.0
  a, w = bf(_randn((M, K), s, 1.0, 0.25)), bf(_randn((N, K), s + 1, 0.05, 0.01))
  bias = _randn((N,), s + 2, 1.0, 0.3) if kw.get("bias") else None
  resid = None
  if kw.get("resid"):
    resid = _randn((M, N), s + 3, 1.0, -0.2)
    resid = resid if kw["resid"] == "f32" else bf(resid)
  return a, w, bias, resid, float(kw.get("alpha", 1.0))


def gemm_ref(a, w, bias, resid, alpha):
  """(pre-activation fp64, S fp64)."""
  ref = alpha * (a.double() @ w.double().T)
  S = abs(alpha) * (a.double().abs() @ w.double().abs().T)
  if bias is not None:
    ref, S = ref + bias.double(), S + bias.double().abs()
  if resid is not None:
    ref, S = ref + resid.double(), S + resid.double().abs()
  return ref, S


def conv_operands(kw, exact, seed=0):
  """x1, x2 (NHWC, bf16 values), w (OIHW fp32 holding bf16 values), bias, rowvec, resid; for "conv_sc" also xs1, xs2, wsc.  Random weights sit on
  the grid k / 64, |k| <= 8 with a non-zero mean: the four-tap upsample form stores SUMS of up to four taps in bf16, which are then exact too, so
  the 9-tap reference below holds for both forms."""
  B, H, C1, C2, Cout = kw["B"], kw["H"], kw["C1"], kw.get("C2", 0), kw["Cout"]
  s = 2000 + seed + 5 * B + 11 * H + C1 + 3 * Cout
  _, OH, _, _, _ = conv_geometry(kw) if "CS1" not in kw else (0, H, 0, 0, 0)
  CS1, CS2 = kw.get("CS1", 0), kw.get("CS2", 0)
  o = {}
  if exact:
    act = lambda shape, k: _ints(shape, s + k, -2, 3)      # noqa: E731
    o["w"] = _ints((Cout, C1 + C2, 3, 3), s + 2, -3, 2)
    o["wsc"] = _ints((Cout, CS1 + CS2), s + 8, -3, 2) if CS1 else None
    o["bias"] = _ints((Cout,), s + 3, -8, 8) if kw.get("bias", "CS1" in kw) else None
    o["rowvec"] = _ints((B, Cout), s + 4, -8, 8) if kw.get("rowvec") else None
    o["resid"] = _ints((B, OH, OH, Cout), s + 5, -64, 64) if kw.get("resid") else None
  else:
    act = lambda shape, k: bf(_randn(shape, s + k, 1.0, 0.25))      # noqa: E731
    o["w"] = _ints((Cout, C1 + C2, 3, 3), s + 2, -8, 6) / 64.0
    o["wsc"] = _ints((Cout, CS1 + CS2), s + 8, -8, 6) / 64.0 if CS1 else None
    o["bias"] = _randn((Cout,), s + 3, 1.0, 0.3) if kw.get("bias", "CS1" in kw) else None
    o["rowvec"] = _randn((B, Cout), s + 4, 0.5, 0.2) if kw.get("rowvec") else None
    o["resid"] = bf(_randn((B, OH, OH, Cout), s + 5, 1.0, -0.2)) if kw.get("resid") else None
  o["x1"] = act((B, H, H, C1), 0)
  o["x2"] = act((B, H, H, C2), 1) if C2 else None
  o["xs1"] = act((B, H, H, CS1), 6) if CS1 else None
  o["xs2"] = act((B, H, H, CS2), 7) if CS2 else None
  return o


def conv_ref(kw, o):
  """(ref, S) fp64 NHWC of conv3x3(x1 ++ x2) [+ conv1x1(xs1 ++ xs2)] + bias + rowvec + resid."""
  def run(x, w, bias, rowvec, resid, xs, wsc):
    x = x.permute(0, 3, 1, 2)
    if kw.get("ups"):
      x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    if kw.get("pad_shift"):
      y = F.conv2d(F.pad(x, (0, 1, 0, 1)), w, None, stride=2, padding=0)
    else:
      y = F.conv2d(x, w, None, stride=kw.get("stride", 1), padding=1)
    y = y.permute(0, 2, 3, 1)
    if xs is not None:
      y = y + xs @ wsc.T
    if bias is not None:
      y = y + bias
    if rowvec is not None:
      y = y + rowvec[:, None, None, :]
    if resid is not None:
      y = y + resid
    return y
  dd = lambda t: None if t is None else t.double()      # noqa: E731
  cat = lambda p, q: None if p is None else (dd(p) if q is None else torch.cat([dd(p), dd(q)], -1))      # noqa: E731
  x, xs = cat(o["x1"], o["x2"]), cat(o["xs1"], o["xs2"])
  ab = lambda t: None if t is None else t.abs()      # noqa: E731
  args = (x, dd(o["w"]), dd(o["bias"]), dd(o["rowvec"]), dd(o["resid"]), xs, dd(o["wsc"]))
  return run(*args), run(*[ab(t) for t in args])


# ---------------------------------------------------------------------------------------------------------------- running a case on the GPU
def _dev(t, dev, dtype=None):
  if t is None:
    return None
  return (t if dtype is None else t.to(dtype)).to(dev)


def _launch_linear(case, o, dev):
  """One guarded (or NaN-prefilled) call of a "gemm" / "conv" / "conv_sc" case on operands `o`: (output on the CPU, guard_ok, extras)."""
  kw = case.kw
  b16 = torch.bfloat16
  if case.op == "gemm":
    a, w, bias, resid, alpha = o
    rdt = None if kw.get("resid") == "f32" else b16
    if "gn" in kw:
      y, stats, slab_rows, nslab = ops.gemm_gn_stats(_dev(a, dev, b16), _dev(w, dev, b16), kw["gn"]["bin"], kw["gn"]["rpb"], _dev(bias, dev), _dev(resid, dev, b16),
                                                     splitk=kw.get("splitk", 1), act=kw.get("act", "none"))
      return y.cpu(), True, (stats.cpu(), slab_rows, nslab)
    y, ok = ops.gemm(_dev(a, dev, b16), _dev(w, dev, b16), _dev(bias, dev), _dev(resid, dev, rdt), alpha=alpha, act=kw.get("act", "none"),
                     out_f32=bool(kw.get("out_f32")), splitk=kw.get("splitk", 0), row_major=bool(kw.get("row_major")), guarded=True)
    return y.cpu(), ok, None
  x1, x2 = _dev(o["x1"], dev, b16), _dev(o["x2"], dev, b16)
  if case.op == "conv":
    y, ok = ops.conv3x3(x1, _dev(o["w"], dev), _dev(o["bias"], dev), x2=x2, rowvec=_dev(o["rowvec"], dev), resid=_dev(o["resid"], dev, b16),
                        stride=kw.get("stride", 1), upsample=bool(kw.get("ups")), splitk=kw.get("splitk", 0), pad_shift=kw.get("pad_shift"), guarded=True)
  else:
    y, ok = ops.conv3x3_shortcut(x1, _dev(o["w"], dev), _dev(o["xs1"], dev, b16), _dev(o["wsc"], dev), _dev(o["bias"], dev), x2=x2,
                                 xs2=_dev(o["xs2"], dev, b16), splitk=kw.get("splitk", 0), guarded=True)
  return y.cpu(), ok, None


def _linear_ref(case, exact):
  if case.op == "gemm":
    o = gemm_operands(case.kw, exact)
    return o, gemm_ref(*o)
  o = conv_operands(case.kw, exact)
  return o, conv_ref(case.kw, o)


def take_log(case, seen):
  """Reads the launcher's record of the call just made: launch count, the expected instantiation among the plans, the claimed properties."""
  rows, launched = ops.gemm_plan_log()
  insts = [inst_of(r) for r in rows]
  seen.update(insts)
  assert launched == case.launches, (case.id, "launches", launched, case.launches, insts)
  assert case.inst in insts, (case.id, "ran", insts, "expected", case.inst)
  check_claims(case, rows[insts.index(case.inst)])
  return insts


def run_linear(case, dev, terms, seen):
  """"gemm" (with or without activation / fused statistics), "conv", "conv_sc": random pass with the plan assertions, exact pass where the
  epilogue is linear (ReLU included: exact on integers), and a second run that must give the same bits."""
  kw = case.kw
  act, out_f32 = kw.get("act", "none"), bool(kw.get("out_f32"))
  K = dict(zip(U.CASE_FIELDS, descriptor(case)))["K"]
  o, (pre, S) = _linear_ref(case, False)
  ops.gemm_plan_log()
  got, ok, extra = _launch_linear(case, o, dev)
  take_log(case, seen)
  assert ok, (case.id, "guard words behind the output were overwritten")
  assert not torch.isnan(got.float()).any(), (case.id, "unwritten output", int(torch.isnan(got.float()).sum()))
  ref = ACT_FP64[act](pre)
  allowed = act_bar(pre, S, K, act, out_f32, terms[act])
  ratio, over, at = worst(got.reshape(ref.shape), ref, allowed)
  print(f"[{case.id}] random pass: worst |err| / bar {ratio:.3f}, {over} of {ref.numel()} over (worst at flat index {at})")
  if extra is not None:      # fused GroupNorm statistics: the standing bar of tests/gn_stats_util.py on the sums of the STORED tensor
    import gn_stats_util as GN
    stats, slab_rows, nslab = extra
    B, nb = kw["M"] // kw["gn"]["rpb"], kw["N"] // kw["gn"]["bin"]
    st = stats[:B * nslab * nb * 2].view(B, nslab, nb, 2)
    sref, denom = GN.partials_ref(got.float().view(B, kw["gn"]["rpb"], kw["N"]), slab_rows, kw["gn"]["bin"])
    fig = GN.partials_figure(case.id, st, sref, denom)
    assert fig < GN.STAT_BAR, (case.id, "statistics", fig)
  assert over == 0, (case.id, "random pass", ratio, over)
  if act in ("none", "relu"):
    oe, (pre_e, _) = _linear_ref(case, True)
    got_e, ok_e, _ = _launch_linear(case, oe, dev)
    want = round_out(ACT_FP64[act](pre_e), out_f32).reshape(got_e.shape)
    nbad = int((got_e != want).sum())
    print(f"[{case.id}] exact pass: {nbad} of {want.numel()} elements differ from the rounded fp64 result")
    assert ok_e and torch.equal(got_e, want), (case.id, "exact pass", nbad)
  again, ok2, _ = _launch_linear(case, o, dev)
  assert ok2 and torch.equal(again.view(torch.int16 if again.dtype == torch.bfloat16 else torch.int32), got.view(torch.int16 if got.dtype == torch.bfloat16 else torch.int32)), \
      (case.id, "a second run gave other bits")
  return ratio


def _std_figures(tag, got, ref, bar_):
  """The standing operator tests' pair of figures (per row and over the tensor: ln_gemm_util.rows_figure, test_ops_gpu._report) under `bar_`."""
  import ln_gemm_util as LU
  from test_ops_gpu import _report
  per_row, whole = LU.rows_figure(tag, got, ref), _report(tag, got, ref)
  assert per_row < bar_ and whole < bar_, (tag, per_row, whole)


def run_geglu(case, dev, terms, seen):
  import ln_gemm_util as LU
  kw = case.kw
  M, inner, K = kw["M"], kw["inner"], kw["K"]
  b16 = torch.bfloat16
  if kw.get("ln"):
    t, g, beta, W, b = LU.case_operands(M, K, 2 * inner)
    planes = LU.split_planes(LU.row_sums(t), kw["P"], seed=K + kw["P"]).to(dev)
    call = lambda: (ops.ln_gemm_geglu(_dev(t, dev, b16), planes, g.to(dev), beta.to(dev), _dev(W, dev, b16), b.to(dev)), True)      # noqa: E731
    ref = LU.geglu(LU.ln_linear_ref(t, g, beta, W, b))
  else:
    a, w, bias, _, _ = gemm_operands(dict(M=M, N=2 * inner, K=K, bias=True), False)
    call = lambda: ops.geglu(_dev(a, dev, b16), _dev(w, dev, b16), bias.to(dev), guarded=True)      # noqa: E731
    ref = LU.geglu(gemm_ref(a, w, bias, None, 1.0)[0]).float()
  ops.gemm_plan_log()
  out, ok = call()
  take_log(case, seen)
  assert ok and torch.isfinite(out.float()).all(), (case.id, "guard / unwritten output")
  _std_figures(case.id, out, ref, LU.BAR)
  again, _ = call()
  assert torch.equal(out, again), (case.id, "a second run gave other bits")


def run_qkv(case, dev, terms, seen):
  import ln_gemm_util as LU
  from test_ln_gemm_gpu import _assert_qkv
  kw = case.kw
  C, heads, d, nseg, B, ntok = kw["C"], kw["heads"], kw["d"], kw["nseg"], kw["B"], kw["ntok"]
  M, b16 = B * ntok, torch.bfloat16
  if kw.get("ln"):
    t, g, beta, W, b = LU.case_operands(M, C, nseg * C)
    planes = LU.split_planes(LU.row_sums(t), kw["P"], seed=C + kw["P"]).to(dev)
    call = lambda: ops.ln_gemm_qkv(_dev(t, dev, b16), planes, g.to(dev), beta.to(dev), _dev(W, dev, b16), b.to(dev), heads, ntok)      # noqa: E731
    y_ref = LU.ln_linear_ref(t, g, beta, W, b)
  else:
    t, W, b, _, _ = gemm_operands(dict(M=M, N=nseg * C, K=C, bias=True), False)
    call = lambda: ops.ln_gemm_qkv(_dev(t, dev, b16), None, None, None, _dev(W, dev, b16), b.to(dev), heads, ntok)      # noqa: E731
    y_ref = gemm_ref(t, W, b, None, 1.0)[0].float()
  ops.gemm_plan_log()
  outs = call()
  take_log(case, seen)
  _assert_qkv(case.id, outs, y_ref, B, ntok, heads, d)
  for x, y in zip(outs, call()):
    assert x is None or torch.equal(x.view(torch.int16), y.view(torch.int16)), (case.id, "a second run gave other bits")      # (pad rows stay NaN: compare bits)
  if not kw.get("ln") and nseg == 3:      # the k and v segments are linear epilogues: exact on the integer operands
    te, We, be, _, _ = gemm_operands(dict(M=M, N=nseg * C, K=C, bias=True), True)
    _, k, vt = ops.ln_gemm_qkv(_dev(te, dev, b16), None, None, None, _dev(We, dev, b16), be.to(dev), heads, ntok)
    _, k_ref, vt_ref = LU.qkv_layout(gemm_ref(te, We, be, None, 1.0)[0], B, ntok, heads, d)
    assert torch.equal(k[:, :, :ntok, :d].cpu(), k_ref.float().to(b16)) and torch.equal(vt[:, :, :d, :ntok].cpu(), vt_ref.float().to(b16)), (case.id, "exact pass k / v^T")


def run_xattn(case, dev, terms, seen):
  """test_cross_attention_folded_vs_torch's operands, reference and bars at this case's shape (context width 768 as there: the bar on the attention
  term is relative to that term, and a narrow context makes it small against the bf16 rounding of the residual stream it is added to)."""
  from test_ops_gpu import _bf, _report, _rnd
  kw = case.kw
  B, HW, C, nh, ctx_len, E = kw["B"], kw["HW"], kw["C"], kw["heads"], kw["ctx_len"], kw["E"]
  d, M = C // nh, B * HW
  t = _bf(_rnd((M, C), 90, 1.5) + 0.3)
  ln_g, ln_b = 1.0 + 0.2 * _rnd((C,), 91), 0.1 * _rnd((C,), 92)
  wq, wk, wv = _bf(_rnd((C, C), 93, 0.05)), _bf(_rnd((C, E), 94, 0.05)), _bf(_rnd((C, E), 95, 0.05))
  wo, bo = _bf(_rnd((C, C), 96, 0.05)), 0.2 * _rnd((C,), 97)
  ctx = _bf(_rnd((B, ctx_len, E), 98))
  q = F.layer_norm(t.float(), (C,), ln_g, ln_b, 1e-5) @ wq.float().T
  k, v = ctx.float() @ wk.float().T, ctx.float() @ wv.float().T
  hq = q.view(B, HW, nh, d).permute(0, 2, 1, 3)
  hk, hv = (x.view(B, ctx_len, nh, d).permute(0, 2, 1, 3) for x in (k, v))
  p_ref = torch.softmax(hq @ hk.transpose(2, 3) / d ** 0.5, dim=-1)
  out_ref = t.float() + (p_ref @ hv).permute(0, 2, 1, 3).reshape(M, C) @ wo.float().T + bo
  call = lambda: ops.cross_attention_folded(*[x.to(dev) for x in (t, ln_g, ln_b, wq, wk, wv, wo, bo, ctx)], nh, B, HW)      # noqa: E731
  ops.gemm_plan_log()
  out, P = call()
  take_log(case, seen)
  assert torch.isfinite(out.float()).all() and torch.isfinite(P.float()).all(), (case.id, "unwritten output")
  Pv = P.float().cpu().view(B, HW, nh, 80).permute(0, 2, 1, 3)
  assert ctx_len == 80 or float(Pv[..., ctx_len:].abs().max()) == 0
  assert float((Pv.sum(-1) - 1).abs().max()) < 2e-2
  assert _report(f"{case.id} softmax weights", Pv[..., :ctx_len], p_ref) < 2e-2
  assert _report(f"{case.id} attention term", out.float().cpu() - t.float(), out_ref - t.float()) < 2e-2
  assert _report(f"{case.id} out", out, out_ref) < 6e-3
  out2, P2 = call()
  assert torch.equal(out, out2) and torch.equal(P, P2), (case.id, "a second run gave other bits")


def run_conv_gn(case, dev, terms, seen):
  """test_conv3x3_groupnorm_finished_in_the_epilogue's operands, reference and bar at this case's shape."""
  from test_ops_gpu import _bf, _report, _rnd
  kw = case.kw
  B, H, Cin, Cout, silu = kw["B"], kw["H"], kw["Cin"], kw["Cout"], bool(kw.get("silu"))
  x = _bf(_rnd((B, H, H, Cin), 290))
  w = _rnd((Cout, Cin, 3, 3), 291, (9 * Cin) ** -0.5)
  b = 0.1 * _rnd((Cout,), 292)
  r = _bf(_rnd((B, H, H, Cout), 293)) if kw.get("resid") else None
  rv = 0.3 * _rnd((B, Cout), 296) if kw.get("rowvec") else None
  gamma, beta = 1.0 + 0.2 * _rnd((Cout,), 294), 0.1 * _rnd((Cout,), 295)
  eps = 1e-5 if silu else 1e-6
  ref_raw = F.conv2d(x.float().permute(0, 3, 1, 2), _bf(w).float(), b, padding=1)
  if rv is not None:
    ref_raw = ref_raw + rv.view(B, Cout, 1, 1)
  if r is not None:
    ref_raw = ref_raw + r.float().permute(0, 3, 1, 2)
  ref = F.group_norm(_bf(ref_raw).float(), 32, gamma, beta, eps)
  if silu:
    ref = F.silu(ref)
  d = lambda t: None if t is None else t.to(dev)      # noqa: E731
  call = lambda: ops.conv3x3_gn(d(x), d(w), d(b), d(gamma), d(beta), 32, eps, silu, d(r), 1, bool(kw.get("raw")), coop=True, rowvec=d(rv),      # noqa: E731
                                want_table=bool(kw.get("table")))
  ops.gemm_plan_log()
  res = call()
  take_log(case, seen)
  y_raw, y_norm = res[0], res[1]
  assert torch.isfinite(y_norm.float()).all(), (case.id, "unwritten output")
  assert _report(f"{case.id} normalised", y_norm.permute(0, 3, 1, 2), ref) < 1.5e-2
  if kw.get("raw"):
    assert torch.isfinite(y_raw.float()).all() and _report(f"{case.id} raw", y_raw.permute(0, 3, 1, 2), ref_raw) < 1.5e-2
  if kw.get("table"):
    tb = res[2]
    assert torch.isfinite(tb).all()
    from_table = y_raw.float() * tb[:, 0].view(B, 1, 1, Cout) + tb[:, 1].view(B, 1, 1, Cout)
    assert _report(f"{case.id} raw * scale + shift", (F.silu(from_table) if silu else from_table).permute(0, 3, 1, 2), ref) < 1.5e-2
  again = call()
  assert torch.equal(y_norm, again[1]) and (y_raw is None or torch.equal(y_raw, again[0])), (case.id, "a second run gave other bits")
  from gill_amd import _native as N
  assert N.lib().gill_coop_timeouts() == 0


RUNNERS = {"gemm": run_linear, "conv": run_linear, "conv_sc": run_linear, "geglu": run_geglu, "qkv": run_qkv, "xattn": run_xattn, "conv_gn": run_conv_gn}


def run_case(case, dev, terms, seen):
  return RUNNERS[case.op](case, dev, terms, seen)
