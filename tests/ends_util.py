"""fp64 restatements, inputs and bars for the kernels at the ends of the engines — conv_out, conv_in (im2col + the K = 64 GEMM), the timestep
embedding, the transformer block's split-K reducer + LayerNorm and the lm_head GEMV — for tests/test_ends_host.py, tests/test_ends_gpu.py and
tools/ends_tolerance.py.  Written from the operations' definitions (3x3 / pad 1 convolution, diffusers Timesteps, LayerNorm), not from the kernels;
CPU, torch only.

Two kinds of input.  EXACT inputs are small integers, exact in bf16, drawn so that every product and every partial sum is exact in fp32: the
kernel must then equal the fp64 result bit for bit whatever its summation order, and one dropped tap or mis-indexed row shows.  ROUNDING inputs
are random normal floats; their bars are derived next to each check below.

TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import math

import torch

# ---------------------------------------------------------------------------------------------------------------- shapes
# conv_out (B, H, W, Cin, Cout) -> the path conv_out_launch must take: 0 one wave per pixel, 1 MFMA with the run-time K loop, 2 | 4 | 10 MFMA with
# that compile-time KS = Cin / 32
CONV_OUT_SHAPES = {
  (2, 5, 16, 320, 4): 10,     # H != W, 10 groups of 16 pixels: not a multiple of the 4 waves of a workgroup
  (2, 3, 32, 320, 4): 10,     # two groups per image row
  (1, 4, 16, 128, 3): 4,
  (2, 16, 16, 64, 4): 2,
  (1, 3, 16, 32, 4): 1,
  (2, 2, 16, 96, 16): 1,      # every weight row of the 16 x 16 tile in use
  (1, 2, 16, 448, 8): 1,      # 64 512 B of weights: just under the 64 KiB of LDS the launcher allows
  (1, 1, 16, 64, 9): 2,       # a single image row, Cout past 8; Cin = 64 is a compile-time width, so the dispatch gives KS = 2
  (2, 5, 12, 64, 4): 0,       # W % 16 != 0, 120 pixels
  (1, 3, 16, 40, 4): 0,       # Cin % 32 != 0
  (1, 2, 16, 512, 8): 0,      # 73 728 B of weights: the SD VAE encoder's conv_out
  (1, 1, 1, 8, 1): 0,
  (1, 3, 3, 8, 8): 0,
}
CONV_OUT_REFUSED = (1, 2, 12, 64, 9)      # general path with Cout > 8
# conv_in (B, Cin, H, W, Cout)
CONV_IN_SHAPES = ((2, 4, 3, 5, 64), (1, 3, 4, 4, 128), (1, 7, 2, 6, 320), (2, 4, 8, 8, 320))
CONV_IN_REFUSED = (1, 8, 2, 2, 64)        # 72 > 64
TIMESTEP_DIMS = (2, 64, 320)
TIMESTEP_FIXED = (0.0, 1.0, 0.5, 250.25, 998.5, 999.0)
TIMESTEP_N = 300
REDUCE_D = (4, 64, 768, 1020, 1024, 1028, 2560, 4096, 4100, 5120, 8192)
REDUCE_SK = (1, 2, 3, 4, 5, 8, 16)
REDUCE_M = (1, 3)
REDUCE_KINDS = ("normal", "outlier", "offset", "const")
REDUCE_EPS = (1e-5, 0.25)
REDUCE_REFUSED = (6, 8196)
LINEAR_CASES = ((5, 1280, 512, 2), (3, 768, 3072, 4), (2, 5120, 1024, 5))      # (M, N, K, splitk)
SKINNY_SHAPES = ((1, 7, 8), (8, 4, 520), (3, 10, 768), (5, 64, 4096))          # (M, N, K)
SKINNY_REFUSED = ((9, 4, 8), (1, 4, 12))


def bf16_round(t: torch.Tensor) -> torch.Tensor:
  """round to nearest even onto the bf16 grid, in t's dtype"""
  return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def bf16_trunc(t: torch.Tensor) -> torch.Tensor:
  """the seeded mistake: drop the low 16 bits of the fp32 value instead of rounding"""
  bits = t.to(torch.float32).contiguous().view(torch.int32) & -65536
  return bits.view(torch.float32).to(t.dtype)


def bf16_ulp(v: torch.Tensor) -> torch.Tensor:
  """spacing of the bf16 grid at |v| (fp64; normal range)"""
  return torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -120))) - 7)


def _gen(*key):
  return torch.Generator().manual_seed(int(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31)))


def _ints(g, shape, lo, hi):
  return torch.randint(lo, hi + 1, shape, generator=g).double()


# ---------------------------------------------------------------------------------------------------------------- 3x3 / pad 1 convolution
CONV_MUTANTS = ("last_tap", "last_octet", "hw_swapped", "batch0")


def conv3x3_ref(x: torch.Tensor, w: torch.Tensor, bias, mutate: str = None):
  """x (B,C,H,W) fp64, w (O,C,3,3) fp64, bias (O) or None -> (y (B,O,H,W), mag (B,O,H,W) = sum |x . w| over the taps + |bias|).  `mutate`: one seeded
  mistake (CONV_MUTANTS) for the host test."""
  B, C, H, W = x.shape
  O = w.shape[0]
  if mutate == "batch0":          # the batch stride of the input taken from the first sample
    x = x[:1].expand(B, C, H, W)
  if mutate == "hw_swapped":      # pixel p decoded as (p / H, p % H): the image read as W rows of H
    return tuple(t.reshape(B, O, H, W) for t in conv3x3_ref(x.reshape(B, C, W, H), w, bias))
  xp = torch.zeros((B, C, H + 2, W + 2), dtype=x.dtype)
  xp[:, :, 1:H + 1, 1:W + 1] = x
  y = torch.zeros((B, O, H, W), dtype=x.dtype)
  mag = torch.zeros_like(y)
  for ky in range(3):
    for kx in range(3):
      if mutate == "last_tap" and ky == 2 and kx == 2:
        continue
      c_end = C - 8 if (mutate == "last_octet" and C > 8) else C
      win = xp[:, :c_end, ky:ky + H, kx:kx + W]
      wt = w[:, :c_end, ky, kx]
      y += torch.einsum("bchw,oc->bohw", win, wt)
      mag += torch.einsum("bchw,oc->bohw", win.abs(), wt.abs())
  if bias is not None:
    y = y + bias.reshape(1, O, 1, 1)
    mag = mag + bias.abs().reshape(1, O, 1, 1)
  return y, mag


def conv_out_inputs(shape, exact: bool):
  """(x (B,Cin,H,W), w (Cout,Cin,3,3), bias (Cout)) fp64.  exact: integers x in [-8, 8], w in [-4, 4], bias in [-64, 64] — every sum below
  9 * 512 * 32 + 64 < 2^24.  Otherwise x ~ N(0,1) rounded to bf16 (the kernel's input type), w ~ N(0, 1 / (9 Cin)) and bias ~ N(0, 0.5^2) NOT
  rounded: the loader rounds w, the reference rounds it the same way (conv_out_exact)."""
  B, H, W, Cin, Cout = shape
  g = _gen(*shape, int(exact))
  if exact:
    return _ints(g, (B, Cin, H, W), -8, 8), _ints(g, (Cout, Cin, 3, 3), -4, 4), _ints(g, (Cout,), -64, 64)
  r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
  return bf16_round(r(B, Cin, H, W)), (r(Cout, Cin, 3, 3) / math.sqrt(9 * Cin)).float().double(), (0.5 * r(Cout)).float().double()


def conv_out_exact(x, w, bias, mutate=None):
  """fp64 result and magnitude from the bf16-rounded x and w (bias stays fp32)"""
  return conv3x3_ref(bf16_round(x), bf16_round(w), bias, mutate)


def conv_out_bar(mag: torch.Tensor, Cin: int) -> torch.Tensor:
  """Per element.  bf16 x bf16 products are exact in fp32, so a sum of 9 Cin products and a bias in ANY fp32 order is off by at most
  (9 Cin + 1) 2^-24 (sum |x w| + |bias|) to first order; the factor 2 is for the matrix unit, whose internal order and rounding are not documented."""
  return 2.0 * (9 * Cin + 1) * 2.0 ** -24 * mag


def check_conv_out(got: torch.Tensor, want: torch.Tensor, mag: torch.Tensor, Cin: int):
  """(passes, worst |got - want| / bar) for fp32 `got`"""
  if not bool(torch.isfinite(got).all()):
    return False, math.inf
  ratio = ((got.double() - want).abs() / conv_out_bar(mag, Cin).clamp_min(1e-300)).max().item()
  return ratio <= 1.0, ratio


def conv_in_inputs(shape, exact: bool):
  """(x (B,Cin,H,W), w (Cout,Cin,3,3), bias (Cout)) fp64.  exact: integers x in [-2, 2], w in {-1, 0, 1}, bias in [-8, 8]: |y| <= 9 * 7 * 2 + 8
  < 256 is exact in the bf16 output.  Otherwise fp32 normal pixels (NOT bf16-representable: the im2col kernel rounds them), w ~ N(0, 1 / (9 Cin)),
  bias ~ N(0, 0.5^2)."""
  B, Cin, H, W, Cout = shape
  g = _gen(*shape, int(exact), 17)
  if exact:
    return _ints(g, (B, Cin, H, W), -2, 2), _ints(g, (Cout, Cin, 3, 3), -1, 1), _ints(g, (Cout,), -8, 8)
  r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
  return r(B, Cin, H, W).float().double(), (r(Cout, Cin, 3, 3) / math.sqrt(9 * Cin)).float().double(), (0.5 * r(Cout)).float().double()


def conv_in_exact(x, w, bias, mutate=None, pixel_round=bf16_round):
  """fp64 NHWC result (B,H,W,Cout) and magnitude from x^ = RNE-bf16(x) and w^ = RNE-bf16(w); pixel_round = bf16_trunc is the seeded mistake"""
  y, mag = conv3x3_ref(pixel_round(x), bf16_round(w), bias, mutate)
  return y.permute(0, 2, 3, 1).contiguous(), mag.permute(0, 2, 3, 1).contiguous()


def check_conv_in(got: torch.Tensor, want: torch.Tensor, mag: torch.Tensor):
  """bf16 `got` within one bf16 ulp of the exact value plus 2 * 64 * 2^-24 (sum |x^ w^| + |bias|): the K = 64 fp32 accumulation (any order, the
  matrix unit's factor 2) moves the value before the one rounding to bf16, which then costs at most half an ulp of where the value landed."""
  if not bool(torch.isfinite(got).all()):
    return False, math.inf
  bar = bf16_ulp(want) + 2.0 * 64 * 2.0 ** -24 * mag
  ratio = ((got.double() - want).abs() / bar).max().item()
  return ratio <= 1.0, ratio


# ---------------------------------------------------------------------------------------------------------------- timestep embedding
TIMESTEP_MUTANTS = ("sin_cos", "half_minus_1")


def timestep_sets():
  """the two calls of the test, fp32: the fixed timesteps (n = 6), and TIMESTEP_N fractional ones spread over [0, 1000) — n * dim / 2 is then no
  multiple of the 256 threads of a block for dim 64 and 320 (and one partial block for dim 2)"""
  g = _gen(1000, TIMESTEP_N)
  spread = (torch.arange(TIMESTEP_N, dtype=torch.float64) + torch.rand(TIMESTEP_N, generator=g, dtype=torch.float64)) * (1000.0 / TIMESTEP_N)
  return torch.tensor(TIMESTEP_FIXED, dtype=torch.float32), spread.float()


def timestep_ref(t: torch.Tensor, dim: int, mutate: str = None) -> torch.Tensor:
  """diffusers Timesteps(dim, flip_sin_to_cos=True, downscale_freq_shift=0) in fp64: [cos(t f_c) | sin(t f_c)], f_c = 10000^(-c / half)"""
  half = dim // 2
  c = torch.arange(half, dtype=torch.float64)
  f = torch.exp(-math.log(10000.0) * c / (half - 1 if mutate == "half_minus_1" else half))
  a = t.double()[:, None] * f[None, :]
  parts = [torch.sin(a), torch.cos(a)] if mutate == "sin_cos" else [torch.cos(a), torch.sin(a)]
  return torch.cat(parts, dim=-1)


def check_timestep(got: torch.Tensor, want: torch.Tensor, dim: int):
  """|got - want| <= 2^-8 |want| + E[dim]: one bf16 ulp of the value, and E for the fp32 angle t * f (see TIMESTEP_E)"""
  if not bool(torch.isfinite(got).all()):
    return False, math.inf
  ratio = ((got.double() - want).abs() / (2.0 ** -8 * want.abs() + TIMESTEP_E[dim])).max().item()
  return ratio <= 1.0, ratio


# ---------------------------------------------------------------------------------------------------------------- reduce + LayerNorm
def reduce_case(D: int, sk: int, M: int, kind: str):
  """fp32 operands of one reducer call whose new stream rows are of `kind`: ws (sk + 2, M, D) with two NaN slices behind the sk real ones, bias
  (D), resid (M, D), gamma, beta (D).  normal: N(0,1); outlier: one channel 10^3 times the rest; offset: N(100, 1) (mean >> spread); const: every
  operand a multiple of 1/64 and resid chosen so that the fp32 sum is EXACTLY 0.75 in every channel."""
  g = _gen(D, sk, M, REDUCE_KINDS.index(kind), 5)
  r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
  q, bias = r(sk, M, D) / math.sqrt(sk), 0.3 * r(D)
  if kind == "const":
    q, bias = torch.round(q * 64) / 64, torch.round(bias * 64) / 64
    target = torch.full((M, D), 0.75, dtype=torch.float64)
  else:
    target = r(M, D)
    if kind == "outlier":
      target[:, (3 * D) // 4] = 1000.0 * torch.sign(target[:, (3 * D) // 4] + 1e-9)
    if kind == "offset":
      target = target + 100.0
  resid = (target - q.sum(0) - bias).float()
  ws = torch.full((sk + 2, M, D), float("nan"), dtype=torch.float32)
  ws[:sk] = q.float()
  gamma, beta = (1.0 + 0.2 * r(D)).float(), (0.2 * r(D)).float()
  return ws, bias.float(), resid, gamma, beta


REDUCE_MUTANTS = ("sk_minus_1", "sk_plus_1")


def reduce_sum_f32(ws, sk, bias, resid, mutate=None):
  """the kernel's stated order in fp32 on the CPU: ((((q0 + q1) + q2) + ...) + bias) + resid.  Additions only — nothing to contract — so the device
  must give these bits for any input."""
  n = sk + {"sk_minus_1": -1, "sk_plus_1": 1}.get(mutate, 0)
  a = ws[0].clone() if n >= 1 else torch.zeros_like(ws[0])
  for z in range(1, n):
    a = a + ws[z]
  return (a + bias[None, :]) + resid


LN_MUTANTS = ("var_d_minus_1", "no_eps", "ragged_offset")


def layernorm_ref(h, gamma, beta, eps, dtype=torch.float64, mutate=None):
  """two-pass LayerNorm of the rows of h in `dtype` (fp64: the reference; fp32: the plain CPU emulation whose distance from fp64 sizes the bar)"""
  x, g, b = h.to(dtype), gamma.to(dtype), beta.to(dtype)
  D = x.shape[-1]
  mean = x.sum(-1, keepdim=True) / D
  d = x - mean
  var = (d * d).sum(-1, keepdim=True) / (D - 1 if mutate == "var_d_minus_1" else D)
  if mutate == "ragged_offset" and D % 1024 != 0:      # gamma / beta of the ragged last vector read from the vector before it
    g, b = g.clone(), b.clone()
    g[-4:], b[-4:] = g[-8:-4].clone(), b[-8:-4].clone()
  return d * torch.rsqrt(var + (0.0 if mutate == "no_eps" else eps)) * g + b


def check_layernorm(nb: torch.Tensor, h: torch.Tensor, gamma, beta, eps, A: float):
  """bf16 `nb` within one bf16 ulp of the fp64 LayerNorm of the SAME fp32 rows h, plus the absolute term A of the case (REDUCE_A / LINEAR_A)"""
  if not bool(torch.isfinite(nb.float()).all()):
    return False, math.inf
  want = layernorm_ref(h, gamma, beta, eps)
  ratio = ((nb.double() - want).abs() / (bf16_ulp(want) + A).clamp_min(1e-300)).max().item()
  return ratio <= 1.0, ratio


def layernorm_f32_distance(h, gamma, beta, eps) -> float:
  """max |fp32 two-pass LayerNorm - fp64 LayerNorm| over the rows of h: what tools/ends_tolerance.py measures; A is four times it"""
  return (layernorm_ref(h, gamma, beta, eps, torch.float32).double() - layernorm_ref(h, gamma, beta, eps)).abs().max().item()


def linear_case(M, N, K, sk):
  """a (M,K), w (N,K) bf16-representable fp32, bias (N), h (M,N), gamma, beta (N) fp32"""
  g = _gen(M, N, K, sk, 3)
  r = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
  return bf16_round(r(M, K)), bf16_round(r(N, K) / math.sqrt(K)), 0.3 * r(N), r(M, N), 1.0 + 0.2 * r(N), 0.2 * r(N)


def linear_ref(a, w, bias, h):
  """fp64 new stream and magnitude sum |a w| + |bias| + |h|"""
  return a.double() @ w.double().T + bias.double() + h.double(), a.double().abs() @ w.double().abs().T + bias.double().abs() + h.double().abs()


# ---------------------------------------------------------------------------------------------------------------- GEMV
def skinny_inputs(M, N, K):
  """integers x (M,K) in [-8, 8], w (N,K) in [-4, 4]: sums below 4096 * 32 < 2^24"""
  g = _gen(M, N, K, 11)
  return _ints(g, (M, K), -8, 8), _ints(g, (N, K), -4, 4)


# ---------------------------------------------------------------------------------------------------------------- measured terms
# tools/ends_tolerance.py (CPU, the inputs above), figures rounded UP to four digits; profiles/ends.md.
# REDUCE_A[(D, kind)]: 4 x the largest layernorm_f32_distance over sk in REDUCE_SK, M in REDUCE_M, eps in REDUCE_EPS on the rows reduce_sum_f32
# gives — the margin of 4 is for the device's different reduction tree and rsqrtf.  (const rows: the fp32 emulation is exact — every deviation is 0 —
# so a constant row must come out as beta within the bf16 ulp alone.)
# LINEAR_A[(M, N, K, sk)]: the same on the rows fp32(linear_ref), eps 1e-5.
# TIMESTEP_E[dim]: 2 x the largest |oracle.unet_ref.timestep_embedding (fp32) - timestep_ref (fp64)| over both timestep_sets() x all channels; of the
# size of its rough bound |angle| 2^-22 = 1000 * 2^-22 = 2.4e-4 (the fp32 product t * f and the fp32 f each move the angle by up to |angle| 2^-24,
# expf by another ulp or two).
REDUCE_A = {
  (4, "normal"): 1.089e-06, (4, "outlier"): 9.987e-07, (4, "offset"): 8.675e-05, (4, "const"): 0.000e+00,
  (64, "normal"): 2.610e-06, (64, "outlier"): 5.880e-06, (64, "offset"): 7.808e-05, (64, "const"): 0.000e+00,
  (768, "normal"): 2.595e-06, (768, "outlier"): 2.062e-05, (768, "offset"): 1.007e-04, (768, "const"): 0.000e+00,
  (1020, "normal"): 4.036e-06, (1020, "outlier"): 2.309e-05, (1020, "offset"): 7.801e-05, (1020, "const"): 0.000e+00,
  (1024, "normal"): 2.425e-06, (1024, "outlier"): 2.438e-05, (1024, "offset"): 6.544e-05, (1024, "const"): 0.000e+00,
  (1028, "normal"): 3.351e-06, (1028, "outlier"): 1.829e-05, (1028, "offset"): 1.046e-04, (1028, "const"): 0.000e+00,
  (2560, "normal"): 3.343e-06, (2560, "outlier"): 3.533e-05, (2560, "offset"): 8.114e-05, (2560, "const"): 0.000e+00,
  (4096, "normal"): 3.068e-06, (4096, "outlier"): 4.362e-05, (4096, "offset"): 5.701e-05, (4096, "const"): 0.000e+00,
  (4100, "normal"): 3.172e-06, (4100, "outlier"): 3.264e-05, (4100, "offset"): 9.105e-05, (4100, "const"): 0.000e+00,
  (5120, "normal"): 3.416e-06, (5120, "outlier"): 4.157e-05, (5120, "offset"): 5.954e-05, (5120, "const"): 0.000e+00,
  (8192, "normal"): 3.190e-06, (8192, "outlier"): 7.266e-05, (8192, "offset"): 1.105e-04, (8192, "const"): 0.000e+00,
}
LINEAR_A = {(5, 1280, 512, 2): 2.223e-06, (3, 768, 3072, 4): 2.080e-06, (2, 5120, 1024, 5): 2.461e-06}
TIMESTEP_E = {2: 6.798e-08, 64: 6.698e-05, 320: 1.107e-04}
