"""The fp8 (e4m3) path of the UNet one launcher at a time, on quantised operands (gill_amd.ops quant_fp8, conv_weight_quant_fp8, conv3x3_fp8_q,
groupnorm_fp8, groupnorm_from_stats(out8_scale=), linear_weight_quant_fp8, ln_quant_fp8, geglu_fp8_q).  The quantisers' bytes are read back
and checked as bytes; the matrix kernels are held to fp64 arithmetic on those same bytes.  References, bars, cases and their derivations:
fp8_util.py; test_fp8_ops_host.py shows on the CPU which defects each check below catches.  Measured figures: profiles/fp8_ops.md."""
import pytest
import torch

import fp8_util as U
import gn_stats_util as G

pytestmark = pytest.mark.gpu


def _dev(t, cuda, bf16=False):
  if t is None:
    return None
  return (t.bfloat16() if bf16 else t).to(cuda)


@pytest.mark.parametrize("n", [65536, 8 * (256 + 37)])      # every bf16 bit pattern (256 blocks of 256 threads x 8); a partial last block
def test_quant_fp8_bytes_equal(cuda, n):
  """Both NaN signs, +-inf -> +-448, subnormals, every tie: 8 x is exact in fp32, so no allowance — the bytes are equal."""
  from gill_amd import ops
  x = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
  x = x[torch.randperm(65536, generator=U._gen(3))][:n].contiguous()
  y, ok = ops.quant_fp8(x.to(cuda), U.CONV_ACT)
  assert ok, "guard bytes behind the output were overwritten"
  assert U.bytes_figure(f"quant_fp8 n {n}", y.cpu(), x.double() * U.CONV_ACT, U.D_EXACT) == 0.0


@pytest.mark.parametrize("cout,cin", U.CONV_W_CASES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_conv_weight_quantiser(cuda, cout, cin, dtype):
  from gill_amd import ops
  w = U.conv_weights(cout, cin, 77 + cout).to(dtype)
  w8, cs, ok = ops.conv_weight_quant_fp8(w.to(cuda), U.CONV_ACT)
  assert ok and tuple(w8.shape) == (cout, U.conv_kpad(cin))
  w8, cs = w8.cpu(), cs.cpu()
  fig, ulps = U.weight_quant_check(f"conv weights {cout}x{cin} {dtype}", w8, cs, U.conv_oihw_to_rows(w.float()), U.CONV_ACT)
  assert fig <= 1.0 and ulps <= 2.0
  assert bool((w8[:, 9 * cin:] == 0).all()), "padding bytes must be exactly zero"
  assert bool((w8[1] == 0).all()) and cs[1].item() == 1.0 / U.CONV_ACT, "the all-zero row: scale 1"
  assert w8[2, 9 * cin - 1].item() == 0x7e, "the row's maximum (last tap of the last channel) is the last byte before the padding, at 448"


def _run_conv(name, cuda, x8, w8, cs, partials=False):
  from gill_amd import ops
  c = U.conv_case(name)
  return ops.conv3x3_fp8_q(x8, w8, cs, bias=_dev(c["bias"], cuda), rowvec=_dev(c["rowvec"], cuda), resid=_dev(c["resid"], cuda, True),
                           splitk=c["splitk"], stats_bin=c["bin"], partials=partials)


@pytest.mark.parametrize("name", list(U.CONV_CASES))
def test_conv3x3_fp8_on_device_quantised_bytes(cuda, name):
  """The convolution fed from the two device quantisers: output per element, GroupNorm partials per (sample, slab, bin) against the unrounded
  fp64 sums, split-K partials per slice against the accumulation term alone; NaN pre-fill intact where no tile files, guards intact, a
  second run bit-equal.  The accumulation term is NOT the derived fp32 bound any more: the partials measured 1.040, 1.352 and 4.938 times
  that bound on the three split cases (profiles/fp8_ops.md "Split-K partials": the scaled MFMA's internal accumulation, a finding about the
  instruction), so its product part carries fp8_util.ACC_FACTOR = 2 x 4.938 — the measurement against fp64 times 2, no more."""
  from gill_amd import ops
  c = U.conv_case(name)
  x8, ok_x = ops.quant_fp8(_dev(c["x"], cuda, True), U.CONV_ACT)
  w8, cs, ok_w = ops.conv_weight_quant_fp8(c["w"].to(cuda), U.CONV_ACT)
  assert ok_x and ok_w
  out = _run_conv(name, cuda, x8, w8, cs)
  assert out[-1], "guard words behind an output were overwritten"
  got = {"y": out[0].float().cpu()}
  if c["bin"]:
    nb = c["Cout"] // c["bin"]
    st, rest = U.gn_stats_view(out[1].cpu(), c["B"], c["H"] * c["W"], nb)
    assert bool(torch.isnan(rest).all()), "the kernel wrote beyond its B * nslab * bins partials"
    got["stats"] = st
  if c["splitk"] > 1:
    ws, ok = _run_conv(name, cuda, x8, w8, cs, partials=True)
    assert ok
    got["partials"] = ws.cpu()
  fig = U.conv_figures(name, x8, w8, cs, got)
  print(f"[conv3x3_fp8_q {name}] " + ", ".join(f"{k} {v:.3f}" for k, v in fig.items()) + " of the bar")
  assert all(v <= 1.0 for v in fig.values()), fig
  again = _run_conv(name, cuda, x8, w8, cs)
  assert torch.equal(again[0], out[0]) and (not c["bin"] or torch.equal(again[1].nan_to_num(7.0), out[1].nan_to_num(7.0))), "two runs differ"


def test_conv3x3_fp8_refuses_bins_the_tile_cannot_file(cuda):
  """192 output channels run on the 128-wide tile: bins of 6 channels (GroupNorm's own 32 groups) do not divide it — an error, not a result."""
  from gill_amd import _native as N, ops
  c = U.conv_case("b1_8x8_192_192_bin4")
  x8, _ = ops.quant_fp8(_dev(c["x"], cuda, True), U.CONV_ACT)
  w8, cs, _ = ops.conv_weight_quant_fp8(c["w"].to(cuda), U.CONV_ACT)
  with pytest.raises(N.GillNativeError):
    ops.conv3x3_fp8_q(x8, w8, cs, stats_bin=6)


@pytest.mark.parametrize("name", list(U.GN_CASES))
def test_groupnorm_to_e4m3(cuda, name):
  """GroupNorm (+ SiLU) writing fp8(8 y): stand-alone (statistics pass of its own; one and two sources) and from producer partials (one
  and two statistics blocks), against fp64 GroupNorm of the bf16 input.  Saturated and subnormal outputs are in every case (host file)."""
  from gill_amd import ops
  B, H, W, C1, C2, silu, form = U.GN_CASES[name]
  x1, x2, st1, st2, gamma, beta = U.gn_case(name)
  def run():      # noqa: E306
    if form == "tensor":
      return ops.groupnorm_fp8(_dev(x1, cuda, True), gamma.to(cuda), beta.to(cuda), G.GROUPS, silu, U.CONV_ACT, x2=_dev(x2, cuda, True), eps=U.GN_EPS)
    r = ops.groupnorm_from_stats(_dev(x1, cuda, True), st1.to(cuda), form[0], gamma.to(cuda), beta.to(cuda), G.GROUPS, U.GN_EPS, silu,
                                 x2=_dev(x2, cuda, True), stats2=_dev(st2, cuda), bin2=form[2], out8_scale=U.CONV_ACT)
    return r[0], r[4]
  y, ok = run()
  assert ok and y.dtype == torch.uint8
  assert U.bytes_figure(f"groupnorm -> e4m3 {name}", y.cpu(), U.gn_reference(name), U.D_NORM) <= 1.0
  assert torch.equal(run()[0], y), "two runs differ"


@pytest.mark.parametrize("name", list(U.LN_CASES))
def test_ln_quant_fp8(cuda, name):
  """planes 1, 2 and 5, ln_rows, the variance guard (a constant row whose sums give a negative variance) and the +-448 clamp (one-hot rows
  at C = 1280), against the fp64 value of the stated formula from the same plane sums."""
  from gill_amd import ops
  M, C, planes, ln_rows = U.LN_CASES[name]
  t, stats = U.ln_case(name)
  y, ok = ops.ln_quant_fp8(_dev(t, cuda, True), stats.to(cuda), ln_rows, U.LN_EPS, U.LIN_ACT)
  assert ok
  y = y.cpu()
  assert bool(((y & 0x7f) != 0x7f).all()), "NaN out for finite input"
  assert U.bytes_figure(f"layernorm -> e4m3 {name}", y, U.ln_q_ref(t, stats, ln_rows, U.LN_EPS, U.LIN_ACT), U.D_NORM) <= 1.0
  if C == 1280:
    assert bool((y[0] & 0x7f == 0).all()) and y[1, 77].item() == 0x7e and y[2, C - 1].item() == 0xfe


@pytest.mark.parametrize("n,k", U.LIN_W_CASES)
def test_linear_weight_quantiser(cuda, n, k):
  from gill_amd import ops
  w = U.linear_weights(n, k, 31 + n)
  w8, cs, ok = ops.linear_weight_quant_fp8(_dev(w, cuda, True), U.LIN_ACT)
  assert ok
  fig, ulps = U.weight_quant_check(f"linear weights {n}x{k}", w8.cpu(), cs.cpu(), w, U.LIN_ACT)
  assert fig <= 1.0 and ulps <= 2.0
  assert bool((w8[1].cpu() == 0).all()) and cs[1].item() == 1.0 / U.LIN_ACT


@pytest.mark.parametrize("M,K,N", U.GEGLU_CASES)
def test_geglu_fp8_on_device_quantised_bytes(cuda, M, K, N):
  """M = 1, a single K step, N not a multiple of the 128-wide tile (the masked pv >= N quads), more than one tile each way."""
  from gill_amd import ops
  t, stats, w, bias = U.geglu_case(M, K, N)
  x8, ok_x = ops.ln_quant_fp8(_dev(t, cuda, True), stats.to(cuda), 0, U.LN_EPS, U.LIN_ACT)
  w8, cs, ok_w = ops.linear_weight_quant_fp8(_dev(w, cuda, True), U.LIN_ACT)
  out, ok = ops.geglu_fp8_q(x8, w8, cs, bias.to(cuda))
  assert ok_x and ok_w and ok, "guard words behind an output were overwritten"
  ref, bar = U.geglu_ref(x8.cpu(), w8.cpu(), cs, bias)
  assert U.ratio_figure(f"geglu_fp8_q {M}x{K}x{N}", out.float().cpu(), ref, bar) <= 1.0
  assert torch.equal(ops.geglu_fp8_q(x8, w8, cs, bias.to(cuda))[0], out), "two runs differ"


def test_geglu_fp8_natural_entry_equals_the_quantised_chain(cuda):
  """geglu_fp8 (natural operands: the loader's interleave and LayerNorm fold inside) against ln_quant_fp8 + linear_weight_quant_fp8 +
  geglu_fp8_q with the fold and the interleave done here: bit-equal, which ties the loader's recipe to fp8_util's restated row order.  The
  operands sit on dyadic grids (fp8_util.geglu_natural_case), so every fp32 sum on either side is exact whatever its order."""
  from gill_amd import ops
  t, gamma, beta, w, b = U.geglu_natural_case()
  inner = w.shape[0] // 2
  want = ops.geglu_fp8(_dev(t, cuda, True), gamma.to(cuda), beta.to(cuda), _dev(w, cuda, True), b.to(cuda))
  wp, bp = U.geglu_interleave(w[:inner], w[inner:]), U.geglu_interleave(b[:inner], b[inner:])
  folded = (wp * gamma).bfloat16()                         # ln_fold_rows: bf16(w * gamma)
  bias = bp + (wp.double() @ beta.double()).float()        # + beta . w^T on the un-folded rows (exact)
  stats = torch.stack([t.double().sum(1), (t.double() ** 2).sum(1)], -1).float()[None].contiguous()
  x8, _ = ops.ln_quant_fp8(_dev(t, cuda, True), stats.to(cuda), 0, 1e-5, U.LIN_ACT)
  w8, cs, _ = ops.linear_weight_quant_fp8(folded.to(cuda), U.LIN_ACT)
  got, ok = ops.geglu_fp8_q(x8, w8, cs, bias.to(cuda))
  assert ok and torch.equal(got, want)
