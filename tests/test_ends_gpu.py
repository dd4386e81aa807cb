"""The kernels at the ends of the engines against the fp64 restatements of tests/ends_util.py: conv_out (both kernels and every compile-time
variant, with the path the launcher took asserted), conv_in (im2col + the K = 64 GEMM, and the counters the im2col launch clears), the timestep
embedding, the transformer block's split-K reducer + LayerNorm (every vector count, slice loop and ragged width), the fused against the unfused
linear, and the lm_head GEMV.

Exact inputs must come out bit for bit; rounding inputs inside bars derived in the util (measured terms: tools/ends_tolerance.py,
profiles/ends.md).  Every output is NaN-prefilled and followed by guard words that must survive; tests/test_ends_host.py shows what the checks catch."""
import pytest
import torch

import ends_util as U

pytestmark = pytest.mark.gpu


def _nhwc_bf16(x, cuda):
  return x.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).to(cuda)


# ---------------------------------------------------------------------------------------------------------------- conv_out
@pytest.mark.parametrize("shape", list(U.CONV_OUT_SHAPES), ids=str)
def test_conv_out_exact_inputs_give_the_fp64_bits_on_the_expected_path(cuda, shape):
  from gill_amd import ops
  B, H, W, Cin, Cout = shape
  want_path = U.CONV_OUT_SHAPES[shape]
  x, w, b = U.conv_out_inputs(shape, True)
  want = U.conv_out_exact(x, w, b)[0]
  xd = _nhwc_bf16(x, cuda)
  for dtype in (torch.float32, torch.float16, torch.bfloat16):      # every loader dtype holds these integers
    y, path, guard = ops.conv_out(xd, w.to(dtype).to(cuda), b.float().to(cuda))
    assert path == want_path, (shape, path)
    assert guard and torch.equal(y.cpu().double(), want), (shape, dtype)
  y0, _, guard = ops.conv_out(xd, w.float().to(cuda), None)
  assert guard and torch.equal(y0.cpu().double(), U.conv_out_exact(x, w, None)[0])
  if want_path != 0:      # the one-wave-per-pixel kernel on the same input (it holds Cout <= 8 only)
    if Cout <= 8:
      yg, pg, guard = ops.conv_out(xd, w.float().to(cuda), b.float().to(cuda), force_general=True)
      assert pg == 0 and guard and torch.equal(yg, y)
    else:
      from gill_amd import _native as N
      with pytest.raises(N.GillNativeError, match="Cout <= 8"):
        ops.conv_out(xd, w.float().to(cuda), b.float().to(cuda), force_general=True)


@pytest.mark.parametrize("shape", list(U.CONV_OUT_SHAPES), ids=str)
def test_conv_out_rounding_inputs_stay_inside_the_fp32_summation_bar(cuda, shape):
  from gill_amd import ops
  B, H, W, Cin, Cout = shape
  x, w, b = U.conv_out_inputs(shape, False)
  xd, wd = _nhwc_bf16(x, cuda), w.float().to(cuda)
  forced = (False, True) if (U.CONV_OUT_SHAPES[shape] != 0 and Cout <= 8) else (False,)
  for bias in (b, None):
    want, mag = U.conv_out_exact(x, w, bias)
    for force in forced:
      y, path, guard = ops.conv_out(xd, wd, None if bias is None else bias.float().to(cuda), force_general=force)
      assert guard and path == (0 if force else U.CONV_OUT_SHAPES[shape])
      ok, ratio = U.check_conv_out(y.cpu(), want, mag, Cin)
      print(f"[ends conv_out {shape}] path {path} bias {bias is not None}: worst |got - exact| / bar = {ratio:.3e}")
      assert ok, (shape, path, ratio)


def test_conv_out_refuses_more_than_8_channels_off_the_matrix_path(cuda):
  from gill_amd import _native as N, ops
  B, H, W, Cin, Cout = U.CONV_OUT_REFUSED
  x = torch.zeros((B, H, W, Cin), device=cuda, dtype=torch.bfloat16)
  with pytest.raises(N.GillNativeError, match="Cout <= 8"):
    ops.conv_out(x, torch.zeros((Cout, Cin, 3, 3), device=cuda))


# ---------------------------------------------------------------------------------------------------------------- conv_in
@pytest.mark.parametrize("shape", U.CONV_IN_SHAPES, ids=str)
def test_conv_in_matches_fp64(cuda, shape):
  from gill_amd import ops
  x, w, b = U.conv_in_inputs(shape, True)
  want = U.conv_in_exact(x, w, b)[0]
  for dtype in (torch.float32, torch.float16, torch.bfloat16):
    y, guard = ops.conv_in(x.float().to(cuda), w.to(dtype).to(cuda), b.float().to(cuda))
    assert guard and torch.equal(y.cpu().double(), want), (shape, dtype)
  y0, guard = ops.conv_in(x.float().to(cuda), w.float().to(cuda), None)
  assert guard and torch.equal(y0.cpu().double(), U.conv_in_exact(x, w, None)[0])
  x, w, b = U.conv_in_inputs(shape, False)
  want, mag = U.conv_in_exact(x, w, b)
  y, guard = ops.conv_in(x.float().to(cuda), w.float().to(cuda), b.float().to(cuda))
  ok, ratio = U.check_conv_in(y.cpu(), want, mag)
  print(f"[ends conv_in {shape}] worst |got - exact| / (bf16 ulp + slack) = {ratio:.3e}")
  assert guard and ok, (shape, ratio)


def test_conv_in_clears_exactly_the_counters_it_is_given(cuda):
  """The UNet forward's first kernel also resets the COOP arrival counters.  The smallest shape's grid is one or two workgroups, so the zeroing
  loop must stride to reach 600 words."""
  from gill_amd import ops
  shape = U.CONV_IN_SHAPES[0]
  x, w, b = U.conv_in_inputs(shape, False)
  xd, wd, bd = x.float().to(cuda), w.float().to(cuda), b.float().to(cuda)
  y_plain, guard = ops.conv_in(xd, wd, bd)
  assert guard
  ctr = torch.full((1000,), -1, device=cuda, dtype=torch.int32)      # 0xFFFFFFFF
  y, guard = ops.conv_in(xd, wd, bd, counters=ctr, nzero=600)
  assert guard and bool((ctr[:600] == 0).all()) and bool((ctr[600:] == -1).all())
  assert torch.equal(y.view(torch.int16), y_plain.view(torch.int16))
  ctr.fill_(-1)
  y, guard = ops.conv_in(xd, wd, bd, counters=ctr, nzero=0)
  assert guard and bool((ctr == -1).all()) and torch.equal(y.view(torch.int16), y_plain.view(torch.int16))


def test_conv_in_refuses_more_than_64_taps(cuda):
  from gill_amd import _native as N, ops
  B, Cin, H, W, Cout = U.CONV_IN_REFUSED
  with pytest.raises(N.GillNativeError, match="64-wide K step"):
    ops.conv_in(torch.zeros((B, Cin, H, W), device=cuda), torch.zeros((Cout, Cin, 3, 3), device=cuda))


# ---------------------------------------------------------------------------------------------------------------- timestep embedding
@pytest.mark.parametrize("dim", U.TIMESTEP_DIMS)
def test_timestep_embedding_matches_fp64(cuda, dim):
  from gill_amd import ops
  for t in U.timestep_sets():
    got, guard = ops.timestep_embed(t.to(cuda), dim)
    want = U.timestep_ref(t, dim)
    ok, ratio = U.check_timestep(got.cpu(), want, dim)
    print(f"[ends timestep dim {dim} n {t.numel()}] worst |got - exact| / (2^-8 |exact| + E) = {ratio:.3e}, "
          f"worst |got - exact| = {(got.cpu().double() - want).abs().max().item():.3e}")
    assert guard and ok, (dim, t.numel(), ratio)
  t = torch.tensor(U.TIMESTEP_FIXED[:2])      # t = 0: the first half is cosines (1), the second sines (0); t = 1, channel 0: cos(1) | sin(1)
  got = ops.timestep_embed(t.to(cuda), dim)[0].cpu().float()
  half = dim // 2
  assert bool((got[0, :half] == 1).all()) and bool((got[0, half:] == 0).all())
  assert abs(got[1, 0].item() - 0.5403) < 4e-3 and abs(got[1, half].item() - 0.8415) < 4e-3


def test_timestep_embedding_refuses_an_odd_width(cuda):
  from gill_amd import _native as N, ops
  with pytest.raises(N.GillNativeError, match="even"):
    ops.timestep_embed(torch.zeros(4, device=cuda), 3)


# ---------------------------------------------------------------------------------------------------------------- reduce + LayerNorm
@pytest.mark.parametrize("D", U.REDUCE_D)
def test_reduce_ln_stream_bits_and_normalised_rows(cuda, D):
  """Every (sk, M, row kind, eps) at this width.  Stream row: bit for bit the fp32 sum in slice order, then bias, then residual — additions only, so
  there is nothing the compiler may contract; the two NaN slices behind slice sk - 1 must never be read into it.  Normalised row: one bf16 ulp of
  the fp64 LayerNorm of that row plus the measured A; a constant row gives beta."""
  from gill_amd import ops
  worst = {k: 0.0 for k in U.REDUCE_KINDS}
  for kind in U.REDUCE_KINDS:
    A = U.REDUCE_A[(D, kind)]
    for sk in U.REDUCE_SK:
      for M in U.REDUCE_M:
        ws, bias, resid, gamma, beta = U.reduce_case(D, sk, M, kind)
        want_h = U.reduce_sum_f32(ws, sk, bias, resid)
        dev = [t.to(cuda) for t in (ws, bias, resid, gamma, beta)]
        for eps in U.REDUCE_EPS:
          h, nb, guard = ops.reduce_ln(dev[0], sk, dev[1], dev[2], dev[3], dev[4], eps)
          assert guard, (D, kind, sk, M)
          assert torch.equal(h.cpu().view(torch.int32), want_h.view(torch.int32)), (D, kind, sk, M)
          ok, ratio = U.check_layernorm(nb.cpu(), want_h, gamma, beta, eps, A)
          worst[kind] = max(worst[kind], ratio)
          assert ok, (D, kind, sk, M, eps, ratio)
          if kind == "const":
            assert bool(((nb.cpu().double() - beta.double()).abs() <= U.bf16_ulp(beta.double())).all()), (D, sk, M, eps)
  print(f"[ends reduce_ln D {D}] worst |nb - fp64| / (bf16 ulp + A) per row kind: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))


def test_reduce_ln_honours_eps(cuda):
  from gill_amd import ops
  ws, bias, resid, gamma, beta = U.reduce_case(768, 2, 3, "normal")
  dev = [t.to(cuda) for t in (ws, bias, resid, gamma, beta)]
  a = ops.reduce_ln(dev[0], 2, *dev[1:], eps=U.REDUCE_EPS[0])[1]
  b = ops.reduce_ln(dev[0], 2, *dev[1:], eps=U.REDUCE_EPS[1])[1]
  assert not torch.equal(a, b)
  h = U.reduce_sum_f32(ws, 2, bias, resid)
  assert not U.check_layernorm(a.cpu(), h, gamma, beta, U.REDUCE_EPS[1], U.REDUCE_A[(768, "normal")])[0]


@pytest.mark.parametrize("D", U.REDUCE_REFUSED)
def test_reduce_ln_refuses_widths_off_the_vector_or_past_8192(cuda, D):
  from gill_amd import _native as N, ops
  z = lambda *s: torch.zeros(s, device=cuda)   # noqa: E731
  with pytest.raises(N.GillNativeError, match="multiple of 4, at most 8192"):
    ops.reduce_ln(z(2, 1, D), 2, z(D), z(1, D), z(D), z(D))


# ---------------------------------------------------------------------------------------------------------------- fused against unfused linear
@pytest.mark.parametrize("case", U.LINEAR_CASES, ids=str)
def test_fused_reducer_gives_the_bits_of_the_gemm_reducer(cuda, case):
  """tfm.hip's claim: opt_reduce_ln_kernel adds in the order of gemm_reduce.hip's reducer epilogue (slices in split order, bias, fp32 residual), so the
  stream is the same bit for bit whichever way TfmRun::linear runs; the two LayerNorms (one fused, one layernorm_kernel) agree to a bf16 ulp."""
  from gill_amd import ops
  M, N, K, sk = case
  a, w, bias, h, gamma, beta = U.linear_case(*case)
  dev = [a.to(torch.bfloat16).to(cuda), w.to(torch.bfloat16).to(cuda)] + [t.to(cuda) for t in (bias, h, gamma, beta)]
  hf, nf, gf = ops.linear_reduce_ln(*dev, splitk=sk, fuse=True)
  hu, nu, gu = ops.linear_reduce_ln(*dev, splitk=sk, fuse=False)
  assert gf and gu
  assert torch.equal(hf.view(torch.int32), hu.view(torch.int32)), case
  # the stream itself: any fp32 order of K products in sk slices, the slices, bias and residual
  want, mag = U.linear_ref(a, w, bias, h)
  hr = ((hf.cpu().double() - want).abs() / (2.0 * (K + sk + 2) * 2.0 ** -24 * mag)).max().item()
  assert hr <= 1.0, (case, hr)
  d = (nf.cpu().double() - nu.cpu().double()).abs()
  ulp = torch.maximum(U.bf16_ulp(nf.cpu().double()), U.bf16_ulp(nu.cpu().double()))
  assert bool((d <= ulp).all()), (case, (d / ulp).max().item())
  for name, hh, nb in (("fused", hf, nf), ("unfused", hu, nu)):
    ok, ratio = U.check_layernorm(nb.cpu(), hh.cpu(), gamma, beta, 1e-5, U.LINEAR_A[case])
    print(f"[ends linear {case}] {name}: worst |nb - fp64| / (bf16 ulp + A) = {ratio:.3e}; stream |h - fp64| / bar = {hr:.3e}; "
          f"elements where the two nb differ: {int((d > 0).sum())}")
    assert ok, (case, name, ratio)


# ---------------------------------------------------------------------------------------------------------------- GEMV
@pytest.mark.parametrize("shape", U.SKINNY_SHAPES, ids=str)
def test_skinny_gemm_exact_inputs_give_the_fp64_bits(cuda, shape):
  from gill_amd import ops
  x, w = U.skinny_inputs(*shape)
  out, guard = ops.skinny_gemm(x.to(torch.bfloat16).to(cuda), w.to(torch.bfloat16).to(cuda))
  assert guard and torch.equal(out.cpu().double(), x @ w.T), shape


@pytest.mark.parametrize("shape", U.SKINNY_REFUSED, ids=str)
def test_skinny_gemm_refuses_more_than_8_rows_and_a_ragged_k(cuda, shape):
  from gill_amd import _native as N, ops
  M, Nn, K = shape
  with pytest.raises(N.GillNativeError, match="M <= 8, K % 8 == 0"):
    ops.skinny_gemm(torch.zeros((M, K), device=cuda, dtype=torch.bfloat16), torch.zeros((Nn, K), device=cuda, dtype=torch.bfloat16))
