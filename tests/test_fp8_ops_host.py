"""CPU companion of test_fp8_ops_gpu.py (fp8_util.py holds the references, bars, cases, emulations and defects).  Two things are shown for every
case the GPU file runs: the honest fp32 emulation of each kernel passes every bar and cap, and each listed defect, on each case it applies to,
misses the bar it is aimed at by 3x or more (the factor is printed).  The layout restatements are cross-checked against F.conv2d and a plain
matmul, rne_code against torch's own e4m3 cast, and gelu_erf's formula against fp64 erf."""
import math

import pytest
import torch
import torch.nn.functional as F

import fp8_util as U

MISS = 3.0


def _report(kind, defect, case, factor):
  print(f"[{kind}] defect {defect} on {case}: misses its bar by {factor:.3g}x")
  assert factor >= MISS, (kind, defect, case, factor)


# ------------------------------------------------------------------------------------------------ the tools themselves
def test_e4m3_table_and_rne_code():
  assert U.E4M3[0x7e].item() == 448.0 and U.E4M3[0x01].item() == 2.0 ** -9 and U.E4M3[0x08].item() == 2.0 ** -6
  assert torch.isnan(U.E4M3[0x7f]) and torch.isnan(U.E4M3[0xff])
  v = torch.cat([U._rnd((20000,), 1, 100.0), U._rnd((20000,), 2, 0.01), torch.tensor([0.0, -0.0, 448.0, -448.0, 464.0, 1e9, -1e9])]).double()
  mine = U.rne_code(v)
  theirs = v.clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
  assert torch.equal(mine, theirs)
  # ties go to the even code, in the normals and in the subnormals; every code maps to itself
  mid = (U._POS[:-1] + U._POS[1:]) / 2
  even = torch.arange(0x7e)
  even = even + even % 2
  assert torch.equal(U.rne_code(mid).long(), even)
  assert torch.equal(U.rne_code(U.E4M3[:0x7f]), torch.arange(0x7f, dtype=torch.uint8))
  assert U.rne_code(torch.tensor([float("nan")], dtype=torch.float64)).item() == 0x7f
  # code_ok: the neighbour only inside the allowance
  x = torch.tensor([1.0625 * (1 + 2.0 ** -17), 1.0625 * (1 + 2.0 ** -15)], dtype=torch.float64)       # just above the midpoint of 1.0 and 1.125
  ok, neigh = U.code_ok(torch.tensor([0x38, 0x38], dtype=torch.uint8), x, U.D_NORM)
  assert ok.tolist() == [True, False] and neigh.tolist() == [True, False]
  assert U.code_ok(torch.tensor([0x38], dtype=torch.uint8), x[:1], 0.0)[0].tolist() == [False]


def test_layout_restatements_against_conv2d_and_matmul():
  for cin, cout in ((64, 8), (192, 5), (320, 12)):
    g = U._gen(cin)
    x = torch.randint(-3, 4, (2, 5, 7, cin), generator=g).double()
    w = torch.randint(-3, 4, (cout, cin, 3, 3), generator=g).double()
    hpt, kpad = cin // 64, U.conv_kpad(cin)
    assert kpad % 128 == 0 and 0 <= kpad - 9 * cin < 128
    rows = torch.full((cout, kpad), 7.0, dtype=torch.float64)            # the kernel's comment, element by element
    for k in range(kpad):
      q, cc = k >> 6, k & 63
      tap = q // hpt
      rows[:, k] = w[:, (q - tap * hpt) * 64 + cc, tap // 3, tap % 3] if q < 9 * hpt else 0.0
    back, pad = U.conv_w8_to_oihw(rows, cin)
    assert torch.equal(back, w) and bool((pad == 0).all()) and torch.equal(U.conv_oihw_to_rows(w), rows)
    want = F.conv2d(x.permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1).reshape(-1, cout)
    assert torch.equal(U.conv_a_matrix(x, cin) @ rows.T, want)
    if hpt > 1:
      assert not torch.equal(U.conv_a_matrix(x, cin, "chunk_major") @ rows.T, want)
  inner, K = 48, 16
  g = U._gen(5)
  W = torch.randint(-3, 4, (2 * inner, K), generator=g).double()
  x = torch.randint(-3, 4, (9, K), generator=g).double()
  phys = U.geglu_interleave(W[:inner], W[inner:])
  for o in range(inner):                                                   # csrc/engine_util.h geglu_row_permutation, row by row
    assert torch.equal(phys[(o // 16) * 32 + o % 16], W[o]) and torch.equal(phys[(o // 16) * 32 + 16 + o % 16], W[inner + o])
  v, gt = U.geglu_split((x @ phys.T).T)
  h, gate = (x @ W.T).chunk(2, -1)
  assert torch.equal(v.T, h) and torch.equal(gt.T, gate)
  st = torch.arange(2 * 3 * 2, dtype=torch.float32).reshape(2, 3, 2)
  tot = U.row_stat_sums(st, 5, 3)
  assert tot.shape == (5, 2) and torch.equal(tot[3], tot[0]) and tot[1, 0].item() == st[0, 1, 0].item() + st[1, 1, 0].item()
  buf = torch.arange(2 * 4 * 3 * 2 + 5, dtype=torch.float32)
  view, rest = U.gn_stats_view(buf, 2, 256, 3)
  assert view[1, 2, 1, 0].item() == ((1 * 4 + 2) * 3 + 1) * 2 and rest.numel() == 5


def test_gelu_erf_formula_against_fp64_erf():
  """What fp8_util's GEGLU bar takes from this: relative 2^-20 holds for x >= 0 only; everywhere |error| <= 2^-20 max(|gelu|, |x| / 2)."""
  x = torch.linspace(-12.0, 12.0, 480001, dtype=torch.float64).float()
  err = (U.gelu_erf32(x).double() - U.gelu64(x.double())).abs()
  ref = U.gelu64(x.double()).abs()
  pos = x > 0
  rel_pos = (err[pos] / ref[pos]).max().item()
  neg = (x < -1) & (ref > 1e-30)
  rel_neg = (err[neg] / ref[neg]).max().item()
  half = (err / (x.double().abs() / 2).clamp_min(1e-30))[x != 0].max().item()
  print(f"gelu_erf vs fp64: x > 0 relative 2^{math.log2(rel_pos):.2f}; x < -1 relative up to {rel_neg:.3g}; |err| / (|x| / 2) 2^{math.log2(half):.2f}")
  assert rel_pos < 2.0 ** -20 and half < 2.0 ** -20 and rel_neg > 0.05
  assert bool((err <= 2.0 ** -20 * torch.maximum(ref, x.double().abs() / 2)).all())


# ------------------------------------------------------------------------------------------------ convolution
@pytest.mark.parametrize("name", list(U.CONV_CASES))
def test_conv_emulation_passes_and_defects_fail(name):
  x8, w8, cs = U.host_conv_bytes(name)
  fig = U.conv_figures(name, x8, w8, cs, U.emulate_conv(name, x8, w8, cs))
  print(f"[conv emulation {name}] " + ", ".join(f"{k} {v:.3f}" for k, v in fig.items()))
  assert all(v <= 1.0 for v in fig.values()), fig
  for d in U.CONV_DEFECTS + U.STATS_DEFECTS:
    if U.conv_defect_applies(d, name):
      bad = U.conv_figures(name, x8, w8, cs, U.emulate_conv(name, x8, w8, cs, d))
      _report("conv", d, name, bad["stats" if d in U.STATS_DEFECTS else "y"])


def test_conv_dropped_weight_element_is_seen():
  """One weight byte zeroed (the smallest defect a convolution can have) on the smallest case."""
  name = "b3_8x8_64_128_rv_res_bin4"
  x8, w8, cs = U.host_conv_bytes(name)
  w8d = w8.clone()
  row = 40
  k = int(U.decode(w8[row]).abs().argmax())
  w8d[row, k] = 0
  _report("conv", "one_weight_element_dropped", name, U.conv_figures(name, x8, w8, cs, U.emulate_conv(name, x8, w8d, cs))["y"])


# ------------------------------------------------------------------------------------------------ quantisers
def _rounding_defects(kind, case, v64, delta, emulate):
  for mode in U.ROUNDING_DEFECTS:
    if U.rounding_defect_applies(mode, v64):
      _report(kind, mode, case, U.bytes_figure(f"{kind} {case} {mode}", emulate(mode), v64, delta))


def test_quant_fp8_emulation_and_defects():
  x = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
  v64 = x.double() * U.CONV_ACT
  assert U.bytes_figure("quant_fp8 all bf16 patterns", U.rne_code((x.float() * U.CONV_ACT).double()), v64, U.D_EXACT) == 0.0
  _rounding_defects("quant_fp8", "all bf16 patterns", v64, U.D_EXACT, lambda mode: U.rne_code((x.float() * U.CONV_ACT).double(), mode))
  _report("quant_fp8", "scale_16_for_8", "all bf16 patterns", U.bytes_figure("quant_fp8 x16", U.rne_code(x.double() * 16.0), v64, U.D_EXACT))


@pytest.mark.parametrize("cout,cin", U.CONV_W_CASES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_conv_weight_quantiser_emulation_and_defects(cout, cin, dtype):
  rows = U.conv_oihw_to_rows(U.conv_weights(cout, cin, 77 + cout).to(dtype).float())
  w8, cs = U.emulate_weight_quant(rows, U.CONV_ACT)
  fig, ulps = U.weight_quant_check(f"conv weights {cout}x{cin} {dtype}", w8, cs, rows, U.CONV_ACT)
  assert fig <= 1.0 and ulps <= 2.0 and bool((w8[:, 9 * cin:] == 0).all()) and bool((w8[1] == 0).all()) and cs[1].item() == 1.0 / U.CONV_ACT
  assert w8[2, 9 * cin - 1].item() == 0x7e        # the row whose maximum is the last tap of the last channel: the last byte before the padding
  v64 = rows.double() / (cs.double() * U.CONV_ACT)[:, None]
  _rounding_defects("conv weights", f"{cout}x{cin} {dtype}", v64, U.D_WEIGHT, lambda mode: U.emulate_weight_quant(rows, U.CONV_ACT, mode)[0])
  # colscale without the activation scale folded in, and a tap-major / chunk-major mix-up of the rows
  assert U.weight_quant_check("colscale without act", w8, cs * U.CONV_ACT, rows, U.CONV_ACT)[1] >= 2.0 * MISS
  if cin > 64:
    mixed = w8[:, :9 * cin].reshape(cout, 9, cin // 64, 64).permute(0, 2, 1, 3).reshape(cout, 9 * cin)
    _report("conv weights", "chunk_major_rows", f"{cout}x{cin}", U.bytes_figure("mixed", mixed, v64[:, :9 * cin], U.D_WEIGHT))


@pytest.mark.parametrize("n,k", U.LIN_W_CASES)
def test_linear_weight_quantiser_emulation_and_defects(n, k):
  w = U.linear_weights(n, k, 31 + n)
  w8, cs = U.emulate_weight_quant(w, U.LIN_ACT)
  fig, ulps = U.weight_quant_check(f"linear weights {n}x{k}", w8, cs, w, U.LIN_ACT)
  assert fig <= 1.0 and ulps <= 2.0 and bool((w8[1] == 0).all()) and cs[1].item() == 1.0 / U.LIN_ACT
  v64 = w.double() / (cs.double() * U.LIN_ACT)[:, None]
  _rounding_defects("linear weights", f"{n}x{k}", v64, U.D_WEIGHT, lambda mode: U.emulate_weight_quant(w, U.LIN_ACT, mode)[0])
  assert U.weight_quant_check("colscale with scale 8 for 16", w8, cs * 2.0, w, U.LIN_ACT)[1] >= 2.0 * MISS


@pytest.mark.parametrize("name", list(U.GN_CASES))
def test_groupnorm_quantiser_emulation_and_defects(name):
  B, H, W, C1, C2, silu, form = U.GN_CASES[name]
  v64 = U.gn_reference(name)
  sat, sub = (v64.abs() > 448).double().mean().item(), ((v64.abs() < 2.0 ** -6) & (v64.abs() >= 2.0 ** -10)).double().mean().item()
  print(f"[groupnorm -> e4m3 {name}] saturated {sat:.2e}, subnormal {sub:.2e} of the tensor")
  assert sat > 0 and sub > (1e-2 if silu else 0)
  assert U.bytes_figure(f"groupnorm -> e4m3 {name}", U.gn_emulated_bytes(name), v64, U.D_NORM) <= 1.0
  _rounding_defects("groupnorm -> e4m3", name, v64, U.D_NORM, lambda mode: U.gn_emulated_bytes(name, mode=mode))
  if silu:
    _report("groupnorm -> e4m3", "silu_dropped", name, U.bytes_figure("silu dropped", U.gn_emulated_bytes(name, "silu_dropped"), v64, U.D_NORM))
  if C2:
    _report("groupnorm -> e4m3", "split_one_vector_off", name,
            U.bytes_figure("split off", U.gn_emulated_bytes(name, "split_one_vector_off"), v64, U.D_NORM))


@pytest.mark.parametrize("name", list(U.LN_CASES))
def test_layernorm_quantiser_emulation_and_defects(name):
  M, C, planes, ln_rows = U.LN_CASES[name]
  t, stats = U.ln_case(name)
  v64 = U.ln_q_ref(t, stats, ln_rows, U.LN_EPS, U.LIN_ACT)
  got = U.emulate_ln_q(t, stats, ln_rows, U.LN_EPS, U.LIN_ACT)
  assert U.bytes_figure(f"layernorm -> e4m3 {name}", got, v64, U.D_NORM) <= 1.0
  assert bool(((got & 0x7f) != 0x7f).all())
  if C == 1280:
    assert bool((got[0] & 0x7f == 0).all()) and got[1, 77].item() == 0x7e and got[2, C - 1].item() == 0xfe and v64[1, 77].item() > 448
  _rounding_defects("layernorm -> e4m3", name, v64, U.D_NORM, lambda mode: U.emulate_ln_q(t, stats, ln_rows, U.LN_EPS, U.LIN_ACT, mode=mode))
  for d in U.LN_DEFECTS:
    if U.ln_defect_applies(d, name):
      _report("layernorm -> e4m3", d, name, U.bytes_figure(d, U.emulate_ln_q(t, stats, ln_rows, U.LN_EPS, U.LIN_ACT, defect=d), v64, U.D_NORM))


# ------------------------------------------------------------------------------------------------ GEGLU
def _geglu_bytes(M, K, N):
  t, stats, w, bias = U.geglu_case(M, K, N)
  w8, cs = U.emulate_weight_quant(w, U.LIN_ACT)
  return U.emulate_ln_q(t, stats, 0, U.LN_EPS, U.LIN_ACT), w8, cs, bias


@pytest.mark.parametrize("M,K,N", U.GEGLU_CASES)
def test_geglu_emulation_passes_and_defects_fail(M, K, N):
  x8, w8, cs, bias = _geglu_bytes(M, K, N)
  ref, bar = U.geglu_ref(x8, w8, cs, bias)
  out, guard = U.emulate_geglu(x8, w8, cs, bias)
  assert U.ratio_figure(f"geglu emulation {M}x{K}x{N}", out, ref, bar) <= 1.0 and bool((guard == 0).all())
  for d in U.GEGLU_DEFECTS:
    if U.geglu_defect_applies(d, M, K, N):
      out, guard = U.emulate_geglu(x8, w8, cs, bias, d)
      f = float("inf") if bool((guard != 0).any()) else U.ratio_figure(f"geglu {d}", out, ref, bar)
      _report("geglu", d, f"{M}x{K}x{N}", f)
