"""CPU checks of the end-kernel tests' own yardstick (tests/ends_util.py): the fp64 restatements agree with F.conv2d and the oracle, the exact
inputs really are exact in fp32, a plain fp32 emulation of every kernel stays inside every bar of tests/test_ends_gpu.py, and every seeded
mistake — a dropped tap or channel octet, H and W swapped, the first sample's batch stride, truncated pixels, [sin | cos], the c / (half - 1)
exponent, a reducer one slice short or long, variance over D - 1, eps dropped, gamma / beta of the ragged last vector misread — breaks its check."""
import pytest
import torch
import torch.nn.functional as F

import ends_util as U

CONV_OUT = list(U.CONV_OUT_SHAPES)


@pytest.fixture(scope="module")
def conv_out_rigs():
  rigs = {}
  for shape in CONV_OUT:
    for exact in (True, False):
      x, w, b = U.conv_out_inputs(shape, exact)
      rigs[(shape, exact)] = (x, w, b, *U.conv_out_exact(x, w, b))
  return rigs


@pytest.fixture(scope="module")
def conv_in_rigs():
  rigs = {}
  for shape in U.CONV_IN_SHAPES:
    for exact in (True, False):
      x, w, b = U.conv_in_inputs(shape, exact)
      rigs[(shape, exact)] = (x, w, b, *U.conv_in_exact(x, w, b))
  return rigs


# ---------------------------------------------------------------------------------------------------------------- restatements
def test_conv_restatement_is_conv2d_in_fp64():
  for shape in ((2, 5, 12, 64, 4), (1, 3, 3, 8, 8), (1, 1, 1, 8, 1)):
    x, w, b = U.conv_out_inputs(shape, False)
    y, mag = U.conv3x3_ref(x, w, b)
    assert torch.allclose(y, F.conv2d(x, w, b, padding=1), rtol=0, atol=1e-12)
    assert torch.allclose(mag, F.conv2d(x.abs(), w.abs(), b.abs(), padding=1), rtol=0, atol=1e-12)
    assert torch.allclose(U.conv3x3_ref(x, w, None)[0], F.conv2d(x, w, None, padding=1), rtol=0, atol=1e-12)


def test_timestep_restatement_is_the_oracle_within_half_of_e():
  from oracle import unet_ref
  for dim in U.TIMESTEP_DIMS:
    for t in U.timestep_sets():
      want = U.timestep_ref(t, dim)
      assert want.shape == (t.numel(), dim)
      d = (unet_ref.timestep_embedding(t, dim).double() - want).abs().max().item()
      assert d <= 0.5 * U.TIMESTEP_E[dim], (dim, d)
  # of the size of its rough bound |angle| 2^-22
  assert 0.1 * 1000 * 2.0 ** -22 < U.TIMESTEP_E[320] < 1000 * 2.0 ** -22
  fixed, spread = U.timestep_sets()
  assert spread.numel() == U.TIMESTEP_N and (spread != spread.round()).any() and 0 <= spread.min() and spread.max() < 1000
  for dim in (64, 320):
    assert (U.TIMESTEP_N * dim // 2) % 256 != 0      # a tail block


# ---------------------------------------------------------------------------------------------------------------- exact inputs
def test_exact_conv_out_inputs_are_exact(conv_out_rigs):
  for shape in CONV_OUT:
    x, w, b, want, mag = conv_out_rigs[(shape, True)]
    for t in (x, w):
      assert torch.equal(U.bf16_round(t), t)
    assert mag.max().item() < 2 ** 24
    assert torch.equal(F.conv2d(x.float(), w.float(), b.float(), padding=1).double(), want), shape
    assert want.abs().max() > 0


def test_exact_conv_in_inputs_are_exact(conv_in_rigs):
  for shape in U.CONV_IN_SHAPES:
    x, w, b, want, mag = conv_in_rigs[(shape, True)]
    assert want.abs().max().item() < 256 and torch.equal(U.bf16_round(want), want)
    assert torch.equal(F.conv2d(x.float(), w.float(), b.float(), padding=1).permute(0, 2, 3, 1).double(), want), shape


def test_exact_skinny_inputs_are_exact():
  for shape in U.SKINNY_SHAPES:
    x, w = U.skinny_inputs(*shape)
    assert torch.equal(U.bf16_round(x), x) and torch.equal(U.bf16_round(w), w)
    assert (x.abs() @ w.abs().T).max().item() < 2 ** 24
    assert torch.equal((x.float() @ w.float().T).double(), x @ w.T)


# ---------------------------------------------------------------------------------------------------------------- the reference alone passes
def test_fp32_conv_out_stays_inside_the_bar(conv_out_rigs):
  for shape in CONV_OUT:
    x, w, b, want, mag = conv_out_rigs[(shape, False)]
    got = F.conv2d(U.bf16_round(x).float(), U.bf16_round(w).float(), b.float(), padding=1)
    ok, ratio = U.check_conv_out(got, want, mag, shape[3])
    assert ok and ratio <= 0.5, (shape, ratio)
    nb = U.conv_out_exact(x, w, None)
    assert U.check_conv_out(F.conv2d(U.bf16_round(x).float(), U.bf16_round(w).float(), None, padding=1), *nb, shape[3])[0]


def test_fp32_conv_in_stays_inside_the_bar(conv_in_rigs):
  for shape in U.CONV_IN_SHAPES:
    x, w, b, want, mag = conv_in_rigs[(shape, False)]
    got = F.conv2d(U.bf16_round(x).float(), U.bf16_round(w).float(), b.float(), padding=1).permute(0, 2, 3, 1).to(torch.bfloat16)
    ok, ratio = U.check_conv_in(got, want, mag)
    assert ok, (shape, ratio)


def test_fp32_timestep_embedding_stays_inside_the_bar():
  from oracle import unet_ref
  for dim in U.TIMESTEP_DIMS:
    for t in U.timestep_sets():
      ok, ratio = U.check_timestep(unet_ref.timestep_embedding(t, dim).to(torch.bfloat16), U.timestep_ref(t, dim), dim)
      assert ok, (dim, ratio)


@pytest.mark.parametrize("D", U.REDUCE_D)
def test_fp32_layernorm_stays_inside_the_bar_on_every_case(D):
  for kind in U.REDUCE_KINDS:
    A = U.REDUCE_A[(D, kind)]
    for sk in U.REDUCE_SK:
      for M in U.REDUCE_M:
        ws, bias, resid, gamma, beta = U.reduce_case(D, sk, M, kind)
        assert bool(torch.isnan(ws[sk:]).all()) and bool(torch.isfinite(ws[:sk]).all())
        h = U.reduce_sum_f32(ws, sk, bias, resid)
        assert h.dtype == torch.float32 and bool(torch.isfinite(h).all())
        if kind == "const":
          assert bool((h == 0.75).all())
        if kind == "outlier":
          assert (h.abs().max(-1).values > 900).all()
        if kind == "offset":
          assert (h.mean(-1) > 99).all()
        for eps in U.REDUCE_EPS:
          assert U.layernorm_f32_distance(h, gamma, beta, eps) <= A      # (the table holds four times the figure measured where it was made)
          nb = U.layernorm_ref(h, gamma, beta, eps, torch.float32).to(torch.bfloat16)
          ok, ratio = U.check_layernorm(nb, h, gamma, beta, eps, A)
          assert ok, (D, kind, sk, M, eps, ratio)
          if kind == "const":      # beta, to one bf16 ulp
            assert bool(((nb.double() - beta.double()).abs() <= U.bf16_ulp(beta.double())).all())


def test_fp32_linear_rows_stay_inside_the_bar():
  for case in U.LINEAR_CASES:
    a, w, bias, h, gamma, beta = U.linear_case(*case)
    assert torch.equal(U.bf16_round(a), a) and torch.equal(U.bf16_round(w), w)
    hn = U.linear_ref(a, w, bias, h)[0].float()
    nb = U.layernorm_ref(hn, gamma, beta, 1e-5, torch.float32).to(torch.bfloat16)
    assert U.check_layernorm(nb, hn, gamma, beta, 1e-5, U.LINEAR_A[case])[0]


# ---------------------------------------------------------------------------------------------------------------- seeded mistakes
def _conv_mutant_applies(mutant, B, C, H, W):
  # (the last tap of a one-row or one-column image lies in the padding)
  return {"last_tap": H > 1 and W > 1, "last_octet": C > 8, "hw_swapped": H != W and H > 1, "batch0": B > 1}[mutant]


@pytest.mark.parametrize("mutant", U.CONV_MUTANTS)
def test_conv_out_mistakes_break_both_checks(conv_out_rigs, mutant):
  hit = 0
  for shape in CONV_OUT:
    B, H, W, Cin, Cout = shape
    if not _conv_mutant_applies(mutant, B, Cin, H, W):
      continue
    hit += 1
    x, w, b, want, mag = conv_out_rigs[(shape, True)]
    assert not torch.equal(U.conv_out_exact(x, w, b, mutant)[0], want), (mutant, shape)
    x, w, b, want, mag = conv_out_rigs[(shape, False)]
    ok, ratio = U.check_conv_out(U.conv_out_exact(x, w, b, mutant)[0].float(), want, mag, Cin)
    assert not ok and ratio > 10, (mutant, shape, ratio)
  assert hit >= 3, (mutant, hit)     # (H != W with more than one row: four of the shapes; B > 1: five)


@pytest.mark.parametrize("mutant", ("last_tap", "hw_swapped", "batch0"))
def test_conv_in_mistakes_break_both_checks(conv_in_rigs, mutant):
  hit = 0
  for shape in U.CONV_IN_SHAPES:
    B, Cin, H, W, Cout = shape
    if not _conv_mutant_applies(mutant, B, Cin, H, W):
      continue
    hit += 1
    x, w, b, want, mag = conv_in_rigs[(shape, True)]
    assert not torch.equal(U.conv_in_exact(x, w, b, mutant)[0], want), (mutant, shape)
    x, w, b, want, mag = conv_in_rigs[(shape, False)]
    ok, ratio = U.check_conv_in(U.conv_in_exact(x, w, b, mutant)[0].to(torch.bfloat16), want, mag)
    assert not ok and ratio > 10, (mutant, shape, ratio)
  assert hit >= 2, (mutant, hit)


def test_truncated_pixels_break_the_conv_in_bar(conv_in_rigs):
  """im2col that drops the low 16 bits of the fp32 pixels instead of rounding them: the rest of the chain (fp32 accumulation, one RNE rounding of the
  output) left as it is.  The exact inputs cannot see it (integers survive truncation); the rounding inputs do, at every shape."""
  for shape in U.CONV_IN_SHAPES:
    x, w, b, want, mag = conv_in_rigs[(shape, False)]
    assert not torch.equal(U.bf16_trunc(x), U.bf16_round(x))
    got = F.conv2d(U.bf16_trunc(x).float(), U.bf16_round(w).float(), b.float(), padding=1).permute(0, 2, 3, 1).to(torch.bfloat16)
    ok, ratio = U.check_conv_in(got, want, mag)
    assert not ok, (shape, ratio)
    x, w, b, want, mag = conv_in_rigs[(shape, True)]
    assert torch.equal(U.conv_in_exact(x, w, b, pixel_round=U.bf16_trunc)[0], want)


@pytest.mark.parametrize("mutant", U.TIMESTEP_MUTANTS)
def test_timestep_mistakes_break_the_bar(mutant):
  for dim in U.TIMESTEP_DIMS:
    for t in U.timestep_sets():
      got = U.timestep_ref(t, dim, mutant).to(torch.bfloat16)
      ok, ratio = U.check_timestep(got, U.timestep_ref(t, dim), dim)
      assert not ok and not ratio <= 10, (mutant, dim, ratio)


@pytest.mark.parametrize("mutant", U.REDUCE_MUTANTS)
def test_a_reducer_one_slice_off_changes_the_stream_bits(mutant):
  for D in (4, 1028):
    for sk in U.REDUCE_SK:
      for kind in U.REDUCE_KINDS:
        ws, bias, resid, gamma, beta = U.reduce_case(D, sk, 3, kind)
        assert not torch.equal(U.reduce_sum_f32(ws, sk, bias, resid, mutant), U.reduce_sum_f32(ws, sk, bias, resid)), (mutant, D, sk, kind)


def _ln_mutant_caught(D, kind, eps, mutant, sk=3, M=3):
  ws, bias, resid, gamma, beta = U.reduce_case(D, sk, M, kind)
  h = U.reduce_sum_f32(ws, sk, bias, resid)
  nb = U.layernorm_ref(h, gamma, beta, eps, torch.float32, mutant).to(torch.bfloat16)
  return not U.check_layernorm(nb, h, gamma, beta, eps, U.REDUCE_A[(D, kind)])[0]


def test_layernorm_mistakes_break_the_bar():
  # variance over D - 1 moves every value by 1 / (2 D) of itself: above one bf16 ulp only at the small widths, which is why they are in the list
  for D in (4, 64):
    assert _ln_mutant_caught(D, "normal", 1e-5, "var_d_minus_1")
  # eps dropped: the second eps value (0.25 against a variance of about 1) shows it on every varied row, a constant row (0 * inf) at any eps
  for D in U.REDUCE_D:
    assert _ln_mutant_caught(D, "normal", 0.25, "no_eps")
    assert _ln_mutant_caught(D, "const", 1e-5, "no_eps")
  # gamma / beta of the ragged last vector
  for D in (1020, 1028, 4100):
    for kind in U.REDUCE_KINDS:
      assert _ln_mutant_caught(D, kind, 1e-5, "ragged_offset")
