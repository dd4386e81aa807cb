"""The case table of tests/gemm_inst_util.py and its bar, on the CPU (no GPU is touched):

  1. every case's descriptor lands on the instantiation it names under (PP 1, COOP 1, 256 CUs), and shows the properties it claims (ragged M / N,
     uneven split with a reducer, N-tile walk, n_major, XCD block map, tile rows);
  2. the table's instantiations are exactly the reachable ones of test_gemm_plan_host.py (63 less UNREACHABLE);
  3. every case is under the multiply-add cap or says why not;
  4. the bar holds for the reference side alone and defects miss it: a CPU emulation of the kernel's arithmetic (bf16-valued operands, fp32
     accumulation in 64-wide K steps, forwards and backwards, one bf16 rounding) stays under the bar on every element at K = 64 / 2560 / 5120,
     and each of six defects puts elements over it in the place it touches.  By how much each misses is printed."""
import functools

import pytest
import torch

import gemm_inst_util as G
from test_gemm_plan_host import N_INSTANTIATIONS, UNREACHABLE


@pytest.mark.parametrize("case", G.CASES, ids=[c.id for c in G.CASES])
def test_case_lands_on_its_instantiation(case):
  row = G.plan_row(case)
  assert row[G.R["rc"]] == 0, (case.id, "the launcher would refuse this call")
  assert G.inst_of(row) == case.inst
  G.check_claims(case, row)
  assert case.launches >= 1


def test_table_covers_every_reachable_instantiation():
  table = {c.inst for c in G.CASES}
  assert not (table & UNREACHABLE)
  assert len(table) == N_INSTANTIATIONS - len(UNREACHABLE), sorted(table)


def test_edge_variants_are_present():
  """Each kind of edge the table promises exists on the tiles that admit it."""
  def insts(pred):
    return {c.inst for c in G.CASES if pred(c)}
  # (the two-wave 64 x 128 tile with a row-major epilogue runs only with fused GroupNorm statistics, whose samples are whole 64-row slabs: never ragged)
  four_two_wave = {i for i in {c.inst for c in G.CASES} if i[0] in (2, 4) and i[2] == 0 and i[3] in (0, 1, 3, 4) and i[:4] not in ((2, 128, 0, 0), (2, 128, 0, 4))}
  assert four_two_wave <= insts(lambda c: c.claims.get("ragged_m")), sorted(four_two_wave - insts(lambda c: c.claims.get("ragged_m")))
  assert {i for i in insts(lambda c: c.claims.get("ragged_m")) if i[1] == 64}, "STREAM64 with ragged M"
  assert insts(lambda c: c.claims.get("tiles_m") == 2 and c.claims.get("ragged_m"))
  assert {i[:5] for i in insts(lambda c: c.claims.get("ragged_n"))} >= {(4, 128, 0, 0, 2), (4, 128, 0, 0, 3), (4, 128, 0, 2, 2), (4, 128, 0, 4, 2), (4, 128, 0, 4, 3)}
  assert {i[1] for i in insts(lambda c: c.claims.get("uneven_split"))} == {64, 128, 160}
  assert insts(lambda c: c.claims.get("walk_even")) and insts(lambda c: c.claims.get("walk_ragged"))
  pp = lambda c: c.inst[0] == 8 and c.inst[1] == 160      # noqa: E731
  assert insts(lambda c: pp(c) and c.claims.get("n_major") == 1) and insts(lambda c: pp(c) and c.claims.get("n_major") == 0 and c.claims.get("xb_m") == 0)
  assert insts(lambda c: pp(c) and c.claims.get("xb_m_on"))
  for feature in ("C2", "stride", "pad_shift", "rowvec", "resid"):      # each on a four-wave and on a ping-pong convolution tile
    got = {c.inst[0] for c in G.CASES if c.op == "conv" and c.kw.get(feature)}
    assert got >= {4, 8}, feature
  assert {c.inst[0] for c in G.CASES if c.op == "conv_sc"} >= {4, 8}
  for act in ("relu", "silu", "gelu"):      # on the 64-row and the 128-row EPI 0 tiles
    rows = {c.claims.get("tile_rows") for c in G.CASES if c.op == "gemm" and c.kw.get("act") == act and c.inst[3] == 0}
    assert rows >= {64, 128}, act
  assert any(c.kw.get("out_f32") for c in G.CASES) and any(c.kw.get("alpha", 1.0) != 1.0 for c in G.CASES)


def test_cases_are_under_the_multiply_add_cap():
  for c in G.CASES:
    assert G.macs(c) <= G.MAC_CAP or c.over_cap, (c.id, G.macs(c))


# ---------------------------------------------------------------------------------------------------------------- the bar against defects
M_, N_ = 256, 320
TILE = (slice(64, 128), slice(160, 320))      # a 64 x 160 tile of the output


def _emulate(a, w, order):
  """fp32 accumulation of 64-wide K steps in `order` (each step's 64 products summed in fp32 by the matmul)."""
  acc = torch.zeros(a.shape[0], w.shape[0])
  for s in order:
    acc = acc + a[:, 64 * s:64 * s + 64] @ w[:, 64 * s:64 * s + 64].T
  return acc


def _truncate_bf16(x):
  return (x.float().view(torch.int32) & -65536).view(torch.float32)


@functools.lru_cache(maxsize=None)
def _bar_case(K):
  a, w, bias, _, _ = G.gemm_operands(dict(M=M_, N=N_, K=K, bias=True), False)
  ref, S = G.gemm_ref(a, w, bias, None, 1.0)
  steps = list(range(K // 64))
  return K, a, w, bias, ref, G.bar(ref, S, K), _emulate(a, w, steps), _emulate(a, w, steps[::-1])


@pytest.fixture(scope="module", params=[64, 2560, 5120])
def bar_case(request):
  return _bar_case(request.param)


def test_emulation_stays_under_the_bar(bar_case):
  K, a, w, bias, ref, allowed, fwd, bwd = bar_case
  for name, acc in (("forwards", fwd), ("backwards", bwd)):
    ratio, over, _ = G.worst(G.bf(acc + bias), ref, allowed)
    print(f"K = {K} {name}: worst |err| / bar = {ratio:.3f}")
    assert over == 0 and ratio <= 1.0


def test_exact_pass_operands_are_exact_in_any_order():
  a, w, bias, resid, _ = G.gemm_operands(dict(M=M_, N=N_, K=5120, bias=True, resid="bf16"), True)
  ref, S = G.gemm_ref(a, w, bias, resid, 1.0)
  assert float(S.max()) < 2 ** 24
  steps = list(range(5120 // 64))
  for order in (steps, steps[::-1]):
    assert torch.equal((_emulate(a, w, order) + bias + resid).to(torch.bfloat16), G.round_out(ref, False))


DEFECTS = ("skipped_k_step", "bias_dropped_on_last_quad", "two_rows_swapped", "quad_transposed", "stale_tile")


@pytest.mark.parametrize("defect", DEFECTS)
def test_defects_miss_the_bar(bar_case, defect):
  _defect_misses(bar_case, defect)


def test_truncation_misses_the_bar_at_k64():
  """Truncation instead of round-to-nearest, on the K = 64 case (with a long K the accumulation term of the bar reaches a bf16 ulp of the small elements)."""
  _defect_misses(_bar_case(64), "truncation")


def _defect_misses(bar_case, defect):
  K, a, w, bias, ref, allowed, fwd, _ = bar_case
  out = fwd + bias
  touched = torch.zeros(M_, N_, dtype=torch.bool)
  if defect == "skipped_k_step":
    s = (K // 64) // 2
    out[TILE] -= a[TILE[0], 64 * s:64 * s + 64] @ w[TILE[1], 64 * s:64 * s + 64].T
    touched[TILE] = True
  elif defect == "bias_dropped_on_last_quad":
    out[:, -4:] -= bias[-4:]
    touched[:, -4:] = True
  elif defect == "two_rows_swapped":
    out[[70, 71]] = out[[71, 70]]
    touched[70:72] = True
  elif defect == "quad_transposed":
    out[64:68, 160:164] = out[64:68, 160:164].T.clone()
    touched[64:68, 160:164] = True
    touched[64:68, 160:164].fill_diagonal_(False)
  elif defect == "stale_tile":      # the tile still holds another launch's answer
    a2 = G.gemm_operands(dict(M=M_, N=N_, K=K, bias=True), False, seed=1)[0]
    out[TILE] = (_emulate(a2, w, range(K // 64)) + bias)[TILE]
    touched[TILE] = True
  got = _truncate_bf16(out) if defect == "truncation" else G.bf(out)
  if defect == "truncation":
    touched[:] = True
  ratio = ((got.double() - ref).abs() / allowed)[touched]
  over = int((ratio > 1).sum())
  print(f"K = {K} {defect}: {over} of {ratio.numel()} touched elements over the bar; |err| / bar median {float(ratio.median()):.1f}, max {float(ratio.max()):.1f}")
  clean = ((G.bf(fwd + bias).double() - ref).abs() / allowed)[~touched]
  assert clean.numel() == 0 or float(clean.max()) <= 1.0
  assert over > 0
  if defect in ("bias_dropped_on_last_quad", "stale_tile"):
    assert over >= 0.95 * ratio.numel(), "nearly every touched element misses"
  if defect == "skipped_k_step":
    assert float(ratio.median()) > 1.0


def test_plan_log_entry_refuses_bad_arguments():
  """gill_gemm_plan_log on the host: an empty record after a read, errors (not crashes) for a missing output or a negative capacity."""
  import ctypes
  import numpy as np
  from gill_amd import _native as N, ops
  ops.gemm_plan_log()      # (whatever this process launched before)
  rows, launched = ops.gemm_plan_log()
  assert launched == 0 and rows.shape == (0, 34)
  lib, n = N.lib(), ctypes.c_int(-1)
  buf = np.zeros((4, 34), dtype=np.int32)
  assert lib.gill_gemm_plan_log(None, 4, ctypes.byref(n)) != 0 and b"gemm_plan_log" in lib.gill_last_error()
  assert lib.gill_gemm_plan_log(buf.ctypes.data, -1, ctypes.byref(n)) != 0
  assert lib.gill_gemm_plan_log(buf.ctypes.data, 4, None) != 0
  assert lib.gill_gemm_plan_log(None, 0, ctypes.byref(n)) == 0 and n.value == 0 and not buf.any()
