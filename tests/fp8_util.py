"""Shared by test_fp8_ops_gpu.py and test_fp8_ops_host.py (not a test module): the fp8 (OCP e4m3) path of the UNet one launcher at a time —
csrc/conv_fp8.hip, csrc/linear_fp8.hip and the e4m3 output branch of groupnorm_apply_kernel (csrc/norm.hip) — through the gill_amd.ops entries
that take and return QUANTISED operands (quant_fp8, conv_weight_quant_fp8, conv3x3_fp8_q, groupnorm_fp8, groupnorm_from_stats(out8_scale=),
linear_weight_quant_fp8, ln_quant_fp8, geglu_fp8_q).  Nothing here emulates a quantiser in order to compare a matrix kernel with it: the
quantisers' bytes are read back and checked AS BYTES, and the matrix kernels are held to fp64 arithmetic on those same bytes.

Bytes.  `E4M3` is the 256-entry decode table.  `code_ok(byte, v64, delta)`: the byte must be the saturating round-to-nearest-even code of
clamp(v64, +-448) (`rne_code`, written out on the table: no cast of torch's is trusted); the neighbouring code is also accepted, but only
where v64 lies within RELATIVE delta of the midpoint between the two, and the share of bytes that use this allowance may not exceed
NEIGHBOUR_CAP = 0.2 % of a tensor (`bytes_figure`).  A NaN in gives a NaN code (0x7f / 0xff); a zero result may carry either sign.
  delta = 0 for quant_fp8: 8 x is exact in fp32, the bytes are equal.
  delta = 2^-21 for the weight quantisers, whose reference value is w / (colscale * act_scale) with the DEVICE's colscale: the kernel
    multiplies by fl(1 / sc) instead (two fp32 roundings, 2^-23).  colscale itself: within 2 ulp of amax / 448 / act_scale.
  delta = 2^-16 for the GroupNorm and LayerNorm quantisers (fp32 statistics, fmaf, rsqrtf, the fast SiLU): far above fp32 error, and 2^-12 of
    an e4m3 step.

Matrix kernels.  `conv_ref` / `geglu_ref` work in fp64 from the bytes (every product exact) and also return the magnitude sums
pm = sum |a| |w| colscale and mag = pm + |bias| + |rowvec| + |resid|.  Per element
    |got - ref| <= 2^-8 |ref| + (K + 4) 2^-24 mag                                                                         (`elem_bar`)
the first term one bf16 rounding, the second the first-order worst case of an fp32 sum of K exact products plus the epilogue's adds in ANY
order (each addition and the colscale multiply contributes at most 2^-24 of the running magnitude).  `acc_bar` states the second term a
little tighter — (K + 1) 2^-24 pm for the products and the multiply, 3 2^-24 mag for the three adds — and, since the device's fp32 partials
showed that the matrix instruction's own accumulation is NOT an fp32 chain, carries the measured factor on the products' part (`ACC_FACTOR`,
see there).  The fp32 split-K partials carry the accumulation term alone, slice by slice.
  GEGLU: out = V gelu(G) with V, G each as above (errors eV, eG); |gelu'| <= 1.13, so
    |got - ref| <= 2^-8 |ref| + eV |gelu(G)| + 1.13 |V| eG + 1.13 eV eG + 2^-20 |V| max(|gelu(G)|, |G| / 2)                   (`geglu_ref`)
  The last term is gelu_erf's own error.  The plan was "relative 2^-20"; test_fp8_ops_host.py checks the kernel's formula
  (Abramowitz-Stegun 7.1.26, fp32) against fp64 erf on [-12, 12] and finds: for x >= 0 the relative error is at most 2^-20.8, for x < 0 it is
  NOT relatively bounded (the form's absolute erf error 1.5e-7 against 1 + erf -> 0: it reaches 100 % below x = -5), but |error| <= 2^-20.7 |x| / 2
  everywhere.  Hence 2^-20 relative to max(|gelu(x)|, |x| / 2) — for x >= 0, where gelu(x) >= x / 2, exactly the relative 2^-20 asked for.

Fused GroupNorm statistics of the convolution (`stats_check`): the partials against fp64 sums of the UNROUNDED fp64 reference values per
(sample, 64-row slab, bin) (gn_stats_util.partials_ref's unrounded= hook), with e_i = acc_bar of the element, the value's own fp32 error:
    |d sum|   <= sum e_i + 64 cg 2^-24 sum |v_i|
    |d sumsq| <= sum (2 |v_i| e_i + e_i^2) + (64 cg + 2) 2^-24 sum v_i^2
(the sum of n = 64 cg terms in any order: n 2^-24 of the magnitude sum; the square itself two more roundings).  Sums of the bf16-ROUNDED
values miss the exact sums by a random walk of the roundings, which this worst-case bar would swallow; so every statistics case carries one
bin (`RB_BIN`) whose values all round the same way — bias 200.3 under weight rows scaled by 2^-10, no residual: every element loses 0.3 to
its rounding — and there the rounded sums miss the bar by 30x.

Defects (`*_DEFECTS`) are applied to the CPU emulations here, never to the library; test_fp8_ops_host.py shows that the honest fp32
emulation passes every bar and cap on every GPU case and that each defect misses the bar it is aimed at by 3x or more."""
import functools
import math

import torch
import torch.nn.functional as F

import gn_stats_util as G

E4M3 = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).double()
_POS = E4M3[:0x7f].clone()                  # codes 0x00 .. 0x7e: 0 .. 448, increasing
NEIGHBOUR_CAP = 2e-3
D_EXACT, D_WEIGHT, D_NORM = 0.0, 2.0 ** -21, 2.0 ** -16
CONV_ACT, LIN_ACT = 8.0, 16.0               # csrc/ops.h F8_ACT_SCALE, F8_LIN_ACT_SCALE
U24 = 2.0 ** -24
RB_BIN = 1                                  # the bin of every statistics case whose values all round the same way (module docstring)


def bf(x):
  return x.bfloat16().float()


def _gen(seed):
  return torch.Generator().manual_seed(seed)


def _rnd(shape, seed, scale=1.0):
  return torch.randn(shape, generator=_gen(seed)) * scale


def decode(b):
  return E4M3[b.long()]


# ------------------------------------------------------------------------------------------------ bytes
def _bracket(m):
  """m >= 0 fp64 (finite, <= 448) -> (lo code, hi code, midpoint): the two positive codes around m."""
  lo = (torch.searchsorted(_POS, m, right=True) - 1).clamp(0, 0x7e)
  hi = (lo + 1).clamp(max=0x7e)
  return lo, hi, (_POS[lo] + _POS[hi]) / 2


def rne_code(v, mode="rne"):
  """fp64 -> uint8: saturating round-to-nearest-even e4m3 code of v, NaN -> 0x7f | sign.  mode (the quantiser defects): "trunc" rounds
  towards zero, "nosat" gives NaN beyond +-448, "flush" gives zero below the smallest normal 2^-6."""
  nan = torch.isnan(v)
  sign = torch.signbit(v)
  m = torch.where(nan, torch.zeros_like(v), v.abs())
  over = m > 448.0
  m = m.clamp(max=448.0)
  lo, hi, mid = _bracket(m)
  up = (m > mid) | ((m == mid) & (lo % 2 == 1))
  if mode == "trunc":
    up = torch.zeros_like(up)
  code = torch.where(up, hi, lo)
  if mode == "flush":
    code = torch.where(m < 2.0 ** -6, torch.zeros_like(code), code)
  if mode == "nosat":
    code = torch.where(over, torch.full_like(code, 0x7f), code)
  code = torch.where(nan, torch.full_like(code, 0x7f), code)
  return (code + 128 * sign.long()).to(torch.uint8)


def code_ok(byte, v64, delta):
  """(ok, used_neighbour) boolean tensors (module docstring)."""
  byte = byte.long().cpu()
  v64 = v64.double()
  nan = torch.isnan(v64)
  mag_b, sign_b = byte & 0x7f, byte >> 7
  m = torch.where(nan, torch.zeros_like(v64), v64.abs()).clamp(max=448.0)
  lo, hi, mid = _bracket(m)
  want = rne_code(v64).long() & 0x7f
  other = torch.where(want == lo, hi, lo)
  near = (m - mid).abs() <= delta * mid
  sign_ok = (sign_b == torch.signbit(v64).long()) | (mag_b == 0)
  exact = (mag_b == want) & sign_ok
  neigh = (mag_b == other) & near & sign_ok & (mag_b != want)
  ok = torch.where(nan, mag_b == 0x7f, exact | neigh)
  return ok, neigh & ~nan


def bytes_figure(name, byte, v64, delta):
  """The quantisers' figure: inf if any byte is not acceptable, else the neighbour-allowance share over NEIGHBOUR_CAP (pass: <= 1)."""
  ok, neigh = code_ok(byte, v64, delta)
  bad = int((~ok).sum())
  share = neigh.double().mean().item()
  msg = f"[{name}] {byte.numel()} bytes: {bad} unacceptable, neighbour allowance used by {int(neigh.sum())} ({share:.2e} of the tensor, cap {NEIGHBOUR_CAP:.0e})"
  if bad:
    w = int((~ok).flatten().nonzero()[0])
    msg += f"; first at {w}: byte 0x{int(byte.flatten()[w]):02x} for value {v64.flatten()[w].item():.9g}"
  print(msg)
  return float("inf") if bad else share / NEIGHBOUR_CAP


# ------------------------------------------------------------------------------------------------ layouts, restated from csrc/ops.h
def conv_kpad(cin):
  """bytes per fp8 weight row: 9 * cin / 64 halves of 64, two halves per 128-byte K step, rounded up to whole steps."""
  return (9 * (cin // 64) + 1) // 2 * 128


def conv_w8_to_oihw(w8, cin):
  """w8 (Cout, Kpad) in the kernel's K order (half q = tap * cin / 64 + chunk, then the chunk's 64 channels) -> (codes (Cout, cin, 3, 3), the
  padding bytes (Cout, Kpad - 9 cin))."""
  cout, hpt = w8.shape[0], cin // 64
  assert w8.shape[1] == conv_kpad(cin)
  body = w8[:, :9 * cin].reshape(cout, 9, hpt, 64)                  # [o][tap][chunk][channel in chunk]
  return body.permute(0, 2, 3, 1).reshape(cout, cin, 3, 3), w8[:, 9 * cin:]


def conv_a_matrix(x, cin, order="tap_major"):
  """The implicit GEMM's A operand: x (B, H, W, cin) -> (B H W, Kpad), column (tap * hpt + chunk) * 64 + cc = the pixel displaced by tap
  (dy, dx) = (tap // 3 - 1, tap % 3 - 1), zero outside the map and in the padding half.  order="chunk_major": the mix-up defect."""
  B, H, W, _ = x.shape
  hpt = cin // 64
  xp = F.pad(x, (0, 0, 1, 1, 1, 1))
  taps = torch.stack([xp[:, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)], 3)       # (B, H, W, 9, cin)
  taps = taps.reshape(B * H * W, 9, hpt, 64)
  if order == "chunk_major":
    taps = taps.permute(0, 2, 1, 3)
  a = torch.zeros((B * H * W, conv_kpad(cin)), dtype=x.dtype)
  a[:, :9 * cin] = taps.reshape(B * H * W, 9 * cin)
  return a


def geglu_split(t):
  """t (N, ...) in the PHYSICAL row order -> (value (N / 2, ...), gate (N / 2, ...)): rows 32 j .. 32 j + 15 are the value rows of outputs
  16 j .. 16 j + 15, rows 32 j + 16 .. 32 j + 31 their gate rows."""
  n = t.shape[0]
  v = t.reshape((n // 32, 2, 16) + tuple(t.shape[1:]))
  return v[:, 0].reshape((n // 2,) + tuple(t.shape[1:])), v[:, 1].reshape((n // 2,) + tuple(t.shape[1:]))


def geglu_interleave(value, gate):
  """The inverse of geglu_split: diffusers' [value rows | gate rows] halves -> the physical order."""
  inner = value.shape[0]
  rest = tuple(value.shape[1:])
  return torch.stack([value.reshape((inner // 16, 16) + rest), gate.reshape((inner // 16, 16) + rest)], 1).reshape((2 * inner,) + rest)


def gn_stats_view(buf, B, rows, nb):
  """The raw gn_stats block -> ((B, rows / 64, nb, 2) filed as [(b * nslab + slab) * nb + bin][2], the floats behind it)."""
  nslab = rows // 64
  used = B * nslab * nb * 2
  return buf[:used].reshape(B, nslab, nb, 2), buf[used:]


def row_stat_sums(stats, M, ln_rows):
  """stats (planes, R, 2), R = ln_rows or M (GemmArgs::row_stats: [(plane * R + row)][2]) -> fp64 (M, 2): the planes added up; rows
  m >= ln_rows take the sums of row m - ln_rows."""
  tot = stats.double().sum(0)
  if ln_rows:
    tot = torch.cat([tot, tot[:M - ln_rows]], 0)
  return tot


# ------------------------------------------------------------------------------------------------ references from bytes, bars
def _nchw(t):
  return t.permute(0, 3, 1, 2)


def conv_ref(x8, w8_oihw, colscale, bias=None, rowvec=None, resid=None):
  """fp64 (ref, mag), both (B, H, W, Cout), and the accumulator part (acc colscale, its magnitude) for the split-K partials."""
  x, w = decode(x8), decode(w8_oihw)
  cs = colscale.double().cpu()
  acc = F.conv2d(_nchw(x), w, padding=1).permute(0, 2, 3, 1)
  amag = F.conv2d(_nchw(x.abs()), w.abs(), padding=1).permute(0, 2, 3, 1)
  ref, mag = acc * cs, amag * cs.abs()
  pa, pm = ref.clone(), mag.clone()
  if bias is not None:
    ref, mag = ref + bias.double(), mag + bias.double().abs()
  if rowvec is not None:
    ref, mag = ref + rowvec.double()[:, None, None, :], mag + rowvec.double().abs()[:, None, None, :]
  if resid is not None:
    ref, mag = ref + resid.double(), mag + resid.double().abs()
  return ref, mag, pa, pm


# The scaled MFMA's own accumulation: the fp32 split-K partials of conv3x3_fp8_kernel (no bf16 rounding, no epilogue) miss the first-order fp32 bound
# (K_slice + 4) 2^-24 pm on the device — worst |partial - fp64| / bound per case: 1.040 (3 slices of 3 K steps), 1.352 (4 slices), 4.938 (16 slices: the
# worst element sits in the one-step slice), profiles/fp8_ops.md "Split-K partials".  The deviation does not grow with K (it is largest on the SHORTEST
# slice): v_mfma_scale_f32_16x16x128_f8f6f4 does not add its 128 products as an fp32 chain.  By the rule set for these tests, the accumulation term takes the
# measured worst ratio times 2 as its factor, nothing more.
ACC_MEASURED = 4.938          # profiles/fp8_ops.md, "Split-K partials", row b1_8x8_320_128_sk16
ACC_FACTOR = 2.0 * ACC_MEASURED


def acc_bar(K, pm, mag=None):
  """The accumulation term: ACC_FACTOR (K + 1) 2^-24 pm for the K products and the colscale multiply (pm = sum |a| |w| colscale), plus
  3 2^-24 mag for the epilogue's three adds (mag = pm + |bias| + |rowvec| + |resid|).  With ACC_FACTOR = 1 this is the derived fp32 bound, never
  above the (K + 4) 2^-24 mag of the module docstring."""
  return ACC_FACTOR * (K + 1) * U24 * pm + (0.0 if mag is None else 3 * U24 * mag)


def elem_bar(K, ref, pm, mag):
  return 2.0 ** -8 * ref.abs() + acc_bar(K, pm, mag)


def gelu64(x):
  return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def geglu_ref(x8, w8, colscale, bias=None):
  """fp64 (ref (M, N / 2), bar (M, N / 2)) from the bytes; w8 / colscale / bias (N) in the physical order."""
  x, w = decode(x8), decode(w8)
  cs = colscale.double().cpu()
  b = torch.zeros_like(cs) if bias is None else bias.double().cpu()
  K = x.shape[1]
  pm = x.abs() @ w.abs().T * cs.abs()
  proj, e = x @ w.T * cs + b, acc_bar(K, pm, pm + b.abs())
  (V, Gt), (eV, eG) = geglu_split(proj.T), geglu_split(e.T)
  V, Gt, eV, eG = V.T, Gt.T, eV.T, eG.T
  g = gelu64(Gt)
  ref = V * g
  bar = 2.0 ** -8 * ref.abs() + eV * g.abs() + 1.13 * V.abs() * eG + 1.13 * eV * eG + 2.0 ** -20 * V.abs() * torch.maximum(g.abs(), Gt.abs() / 2)
  return ref, bar


def ratio_figure(name, got, ref, bar):
  """max |got - ref| / bar (pass: <= 1); a NaN or an unwritten element counts as inf."""
  r = (got.double().cpu() - ref).abs() / bar.clamp_min(1e-300)
  r = torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))
  w = int(r.argmax())
  print(f"[{name}] worst element {w} of {r.numel()}: |err| = {r.flatten()[w].item():.3f} x its bar (ref {ref.flatten()[w].item():.5g})")
  return r.max().item()


def _blocks(t, bin):
  """(B, H, W, C) -> (B, rows / 64, 64, C / bin, bin)"""
  B, C = t.shape[0], t.shape[-1]
  t = t.reshape(B, -1, C)
  return t.reshape(B, t.shape[1] // 64, 64, C // bin, bin)


def stats_check(name, part, ref, pm, mag, K, bin):
  """part (B, nslab, nb, 2) fp32 against the fp64 sums of the unrounded reference (module docstring).  Returns max |error| / bar."""
  sref, _ = G.partials_ref(ref, 64, bin, defect="sums_of_unrounded_values", unrounded=ref)
  v, e = _blocks(ref, bin), _blocks(acc_bar(K, pm, mag), bin)
  n = 64 * bin
  bar_s = e.sum((2, 4)) + n * U24 * v.abs().sum((2, 4))
  bar_q = (2 * v.abs() * e + e * e).sum((2, 4)) + (n + 2) * U24 * (v * v).sum((2, 4))
  return ratio_figure(name + " partials", part, sref, torch.stack([bar_s, bar_q], -1))


# ------------------------------------------------------------------------------------------------ quantiser references (fp64) and emulations (fp32)
def weight_quant_check(name, w8_rows, colscale, w_rows, act):
  """w8_rows / w_rows (N, K) in the same element order, colscale (N) from the device (or the emulation).  Returns (bytes figure, the worst
  colscale error in ulps of amax / 448 / act, bar 2)."""
  w = w_rows.double().cpu()
  cs = colscale.double().cpu()
  fig = bytes_figure(name, w8_rows.cpu(), w / (cs * act)[:, None], D_WEIGHT)
  amax = w.abs().amax(1)
  want = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax)) / act
  ulp = 2.0 ** (torch.floor(torch.log2(want)) - 23)
  ulps = ((cs - want).abs() / ulp).max().item()
  print(f"[{name}] colscale: worst {ulps:.2f} ulp (bar 2)")
  return fig, ulps


def emulate_weight_quant(w_rows, act, mode="rne"):
  """fp32 restatement of the two weight quantisers: (bytes (N, K), colscale (N))."""
  w = w_rows.float()
  amax = w.abs().amax(1)
  sc = torch.where(amax > 0, amax / torch.tensor(448.0), torch.ones_like(amax))
  inv = torch.tensor(1.0) / sc
  return rne_code((w * inv[:, None]).double(), mode), sc / torch.tensor(act)


def groupnorm_q_ref(x, groups, gamma, beta, eps, silu, scale):
  """fp64 scale * [silu](GroupNorm(x)) of the bf16 tensor x (B, HW, C)."""
  return scale * G.groupnorm_ref(x, groups, gamma, beta, eps, silu)


def emulate_groupnorm_q(x1, x2, table, silu, scale, defect=None, mode="rne"):
  """fp32 restatement of groupnorm_apply_kernel's e4m3 branch behind its scale | shift table (B, 2, C) (gn_stats_util.emulate_apply): fmaf,
  SiLU, scale, clamp, convert.  defect: "silu_dropped", "split_one_vector_off" (the last 8 channels of x1 read x2's first 8 instead)."""
  x = x1 if x2 is None else torch.cat([x1, x2], -1)
  if defect == "split_one_vector_off":
    x = x.clone()
    x[..., x1.shape[-1] - 8:x1.shape[-1]] = x2[..., :8]
  y = (x.double() * table[:, 0].double()[:, None] + table[:, 1].double()[:, None]).float()
  if silu and defect != "silu_dropped":
    y = y * (torch.tensor(1.0) / (1.0 + torch.exp(-y)))
  return rne_code((y * torch.tensor(scale)).double(), mode)


def ln_q_ref(t, stats, ln_rows, eps, scale):
  """fp64 scale * (t - mean) * rsqrt(max(var, 0) + eps), mean / var of row m from the plane sums (csrc/linear_fp8.hip's stated formula)."""
  M, C = t.shape
  tot = row_stat_sums(stats, M, ln_rows)
  mean = tot[:, 0] / C
  var = (tot[:, 1] / C - mean * mean).clamp_min(0.0)
  return scale * (t.double() - mean[:, None]) * torch.rsqrt(var + eps)[:, None]


def emulate_ln_q(t, stats, ln_rows, eps, scale, defect=None, mode="rne"):
  """fp32 restatement of ln_quant_fp8_kernel.  defect: "scale_8", "planes_beyond_first_ignored", "ln_rows_ignored" (row m reads entry m of
  every plane as if the planes held M rows; reads past the block give zeros), "negative_variance_not_clamped"."""
  M, C = t.shape
  P, R, _ = stats.shape
  st = stats.float()
  if defect == "planes_beyond_first_ignored":
    st, P = st[:1], 1
  rows = torch.arange(M)
  ms = torch.where(rows >= R, rows - R, rows)
  sx, sq = torch.zeros(M), torch.zeros(M)
  for pl in range(P):
    if defect == "ln_rows_ignored":
      flat = torch.cat([st.reshape(-1, 2), torch.zeros(M, 2)], 0)
      v = flat[pl * R + rows]
    else:
      v = st[pl, ms]
    sx, sq = sx + v[:, 0], sq + v[:, 1]
  invc = torch.tensor(1.0) / torch.tensor(float(C))
  mean = sx * invc
  var = sq * invc - mean * mean
  if defect != "negative_variance_not_clamped":
    var = var.clamp_min(0.0)
  rs = torch.rsqrt(var + torch.tensor(eps)) * torch.tensor(8.0 if defect == "scale_8" else scale)
  off = -mean * rs
  o = (t.double() * rs.double()[:, None] + off.double()[:, None]).float()          # fmaf: one rounding
  return rne_code(o.double(), mode)


def gelu_erf32(x):
  """fp32 restatement of csrc/common.h gelu_erf (Abramowitz-Stegun 7.1.26; exp and reciprocal exact to fp32 here)."""
  x = x.float()
  one = torch.tensor(1.0)
  z = x * torch.tensor(0.70710678118654752)
  a = z.abs()
  t = one / (torch.tensor(0.3275911) * a + one)
  p = torch.tensor(1.061405429) * t + torch.tensor(-1.453152027)
  for c in (1.421413741, -0.284496736, 0.254829592):
    p = p * t + torch.tensor(c)
  r = one - p * t * torch.exp(-a * a)
  return torch.tensor(0.5) * x * (one + torch.copysign(r, z))


# ------------------------------------------------------------------------------------------------ the convolution's cases, emulation and defects
# name -> (B, H, W, Cin, Cout, splitk, stats bin, operands: b = bias, v = rowvec, r = resid)
CONV_CASES = {
  "b3_8x8_64_128_rv_res_bin4": (3, 8, 8, 64, 128, 1, 4, "bvr"),       # odd halves, every step two taps, tiles straddle samples, last half tile past M
  "b2_16x16_128_160_bin5": (2, 16, 16, 128, 160, 1, 5, "bvr"),        # the 160-wide tile, four slabs per sample
  # 27 halves, second N tile half masked.  Bins of 4, not the group's 6: N = 192 runs on the 128-wide tile, whose width a bin must divide —
  # conv3x3_fp8_launch refuses bin 6 here (test_fp8_ops_gpu.py checks that it does)
  "b1_8x8_192_192_bin4": (1, 8, 8, 192, 192, 1, 4, "bvr"),
  "b3_12x20_192_64_plain": (3, 12, 20, 192, 64, 1, 0, ""),            # W not a power of two, ragged M, N below the tile; no optional operand at all
  "b2_8x8_320_320_bin10": (2, 8, 8, 320, 320, 1, 10, "bvr"),
  "b2_8x8_128_160_sk3": (2, 8, 8, 128, 160, 3, 0, "bvr"),             # 9 K steps in 3 slices
  "b2_8x8_128_160_sk4": (2, 8, 8, 128, 160, 4, 0, "b"),               # ... in 4 slices of 3: the last one empty
  "b1_8x8_320_128_sk16": (1, 8, 8, 320, 128, 16, 0, "bvr"),           # 23 K steps in slices of 2: slice 11 short, 12 .. 15 empty
}
CONV_DEFECTS = ("border_reads_wrapped_neighbour", "padding_half_not_zero", "tap_chunk_mixup", "colscale_four_columns_off",
                "bias_four_columns_off", "rowvec_four_columns_off", "rowvec_of_tiles_first_sample", "residual_left_out_rows_64_up")
STATS_DEFECTS = ("sums_of_rounded_values", "slab_shifted_one", "bin_shifted_one", "second_half_filed_under_first_sample")


def conv_weights(cout, cin, seed, bin=0):
  """fp32 OIHW: N(0, std) rows with output sigma ~ 1; row 1 all zero, row 2 with its maximum at the last tap of the last channel; with a
  statistics bin, the rows of bin RB_BIN scaled by 2^-10."""
  w = _rnd((cout, cin, 3, 3), seed, (9 * cin * 0.6) ** -0.5)
  w[1] = 0.0
  w[2, cin - 1, 2, 2] = 4.0 * w[2].abs().max()
  if bin:
    w[RB_BIN * bin:(RB_BIN + 1) * bin] *= 2.0 ** -10
  return w


@functools.lru_cache(maxsize=None)
def conv_case(name):
  """dict: x (B,H,W,Cin) bf16-valued natural activations (SiLU of a normal with an offset per (sample, 16-row block)), w fp32 OIHW, bias,
  rowvec, resid (None where the case has none), and the geometry."""
  B, H, W, Cin, Cout, sk, bin, opts = CONV_CASES[name]
  seed = 1300 + sum(ord(c) for c in name)
  HW = H * W
  x = bf(F.silu(_rnd((B, HW, Cin), seed, 1.5) + G._block_offsets(B, HW, 1, Cin, seed + 1, -1.0, 1.0))).reshape(B, H, W, Cin)
  d = dict(B=B, H=H, W=W, Cin=Cin, Cout=Cout, splitk=sk, bin=bin, K=9 * Cin, x=x, w=conv_weights(Cout, Cin, seed + 2, bin), bias=None, rowvec=None,
           resid=None)
  cb = bin if bin else 4
  nb = Cout // cb
  rb = slice(RB_BIN * bin, (RB_BIN + 1) * bin) if bin else slice(0, 0)
  if "b" in opts:
    d["bias"] = G._block_offsets(1, 1, nb, cb, seed + 3, -2.0, 2.0)[0, 0] + _rnd((Cout,), seed + 4, 0.1)
    d["bias"][rb] = 200.3
  if "v" in opts:
    d["rowvec"] = G._block_offsets(B, 1, nb, cb, seed + 5, -1.5, 1.5)[:, 0] + _rnd((B, Cout), seed + 6, 0.05)
    d["rowvec"][:, rb] = 0.0625 * (1.0 + torch.arange(B, dtype=torch.float32))[:, None]
  if "r" in opts:
    r = bf(_rnd((B, HW, Cout), seed + 7, 0.5) + G._block_offsets(B, HW, nb, cb, seed + 8, -2.0, 2.0))
    r[..., rb] = 0.0
    d["resid"] = r.reshape(B, H, W, Cout)
  return d


def conv_defect_applies(defect, name):
  B, H, W, Cin, Cout, sk, bin, opts = CONV_CASES[name]
  straddle = B > 1 and (H * W) % 128 != 0
  return {"border_reads_wrapped_neighbour": True, "padding_half_not_zero": (9 * Cin // 64) % 2 == 1, "tap_chunk_mixup": Cin == 192,
          "colscale_four_columns_off": True, "bias_four_columns_off": "b" in opts, "rowvec_four_columns_off": "v" in opts,
          "rowvec_of_tiles_first_sample": "v" in opts and straddle, "residual_left_out_rows_64_up": "r" in opts and B * H * W > 64,
          "sums_of_rounded_values": bin > 0, "slab_shifted_one": bin > 0 and B * H * W > 64, "bin_shifted_one": bin > 0,
          "second_half_filed_under_first_sample": bin > 0 and straddle}[defect]


def emulate_conv(name, x8, w8, colscale, defect=None):
  """fp32 restatement of conv3x3_fp8_kernel (+ the split-K reducer) on bytes x8 (B,H,W,Cin), w8 (Cout,Kpad): the implicit GEMM over the
  kernel's own K order with fp32 accumulation, the epilogue's adds in fp32, a bf16 store.  Returns dict(y bf16-valued (B,H,W,Cout), v the
  fp32 values before the rounding, partials (splitk, M, Cout) for split cases, stats (B, nslab, nb, 2) for statistics cases)."""
  c = conv_case(name)
  B, H, W, Cin, Cout, sk, bin = c["B"], c["H"], c["W"], c["Cin"], c["Cout"], c["splitk"], c["bin"]
  M, hpt = B * H * W, Cin // 64
  a = conv_a_matrix(decode(x8).float(), Cin, "chunk_major" if defect == "tap_chunk_mixup" else "tap_major")
  wm = decode(w8).float().clone()
  if defect == "border_reads_wrapped_neighbour":
    m = W * (H // 2)                                  # a pixel at x = 0: tap (0, -1) = tap 3, chunk 0 reads pixel m - 1 instead of zeros
    a[m, 3 * hpt * 64:3 * hpt * 64 + 64] = decode(x8).float().reshape(M, Cin)[m - 1, :64]
  if defect == "padding_half_not_zero":
    a[:, 9 * Cin:] = a[:, 4 * hpt * 64:4 * hpt * 64 + 64]       # the centre tap's first chunk
    wm[:, 9 * Cin:] = wm[:, 9 * Cin - 64:9 * Cin]
  cs = colscale.float().cpu()
  if defect == "colscale_four_columns_off":
    cs = torch.roll(cs, -4)
  out = {}
  if sk > 1:
    steps = conv_kpad(Cin) // 128
    per = -(-steps // sk)
    parts = torch.zeros(sk, M, Cout)
    for z in range(sk):
      k0, k1 = min(z * per, steps) * 128, min((z + 1) * per, steps) * 128
      if k1 > k0:
        parts[z] = (a[:, k0:k1] @ wm[:, k0:k1].T) * cs
    out["partials"] = parts
    v = torch.zeros(M, Cout)
    for z in range(sk):
      v = v + parts[z]
  else:
    v = (a @ wm.T) * cs
  rows = torch.arange(M)
  if c["bias"] is not None:
    v = v + (torch.roll(c["bias"], -4) if defect == "bias_four_columns_off" else c["bias"])
  if c["rowvec"] is not None:
    rv = torch.roll(c["rowvec"], -4, 1) if defect == "rowvec_four_columns_off" else c["rowvec"]
    b = (rows // 128 * 128 if defect == "rowvec_of_tiles_first_sample" else rows) // (H * W)
    v = v + rv[b]
  if c["resid"] is not None:
    r = c["resid"].reshape(M, Cout).clone()
    if defect == "residual_left_out_rows_64_up":
      r[rows % 128 >= 64] = 0.0
    v = v + r
  out["v"], out["y"] = v.reshape(B, H, W, Cout), bf(v).reshape(B, H, W, Cout)
  if bin:
    src = out["y"] if defect == "sums_of_rounded_values" else out["v"]
    st = G.emulate_partials(src.reshape(B, H * W, Cout), 64, bin)
    if defect == "slab_shifted_one":
      st = torch.roll(st.flatten(0, 1), 1, 0).reshape(st.shape)
    if defect == "bin_shifted_one":
      st = torch.roll(st, 1, 2)
    if defect == "second_half_filed_under_first_sample":      # 64-row maps: a tile's second half is the next sample; its partials land on the first's
      flat = st.flatten(0, 1).clone()
      for i in range(1, flat.shape[0], 2):
        flat[i - 1] = flat[i]
        flat[i] = float("nan")
      st = flat.reshape(st.shape)
    out["stats"] = st
  return out


# ------------------------------------------------------------------------------------------------ weight quantiser cases
CONV_W_CASES = [(8, 64), (5, 192), (160, 320)]
LIN_W_CASES = [(32, 128), (96, 384), (4, 2)]           # K = 2: one thread of the block's 256 converts, the other 255 only take part in the maximum


@functools.lru_cache(maxsize=None)
def linear_weights(n, k, seed):
  """bf16-valued (N, K) rows of differing scale; row 1 all zero."""
  w = _rnd((n, k), seed, k ** -0.5) * (0.25 + 4.0 * torch.rand((n, 1), generator=_gen(seed + 1)))
  w[1] = 0.0
  return bf(w)


# ------------------------------------------------------------------------------------------------ GroupNorm -> e4m3 cases
# name -> (B, H, W, C1, C2, silu, form): form "tensor" (statistics pass of its own) or (bin1, ns1, bin2, ns2) host-made partials
GN_CASES = {
  "c64_g32": (2, 8, 8, 64, 0, False, "tensor"),
  "c128+64_silu": (2, 6, 10, 128, 64, True, "tensor"),
  "partials_320_one_block_silu": (2, 8, 8, 320, 0, True, (5, 4, 0, 0)),
  "partials_640+320_two_blocks_silu": (2, 8, 8, 640, 320, True, (10, 16, 5, 4)),
}
GN_EPS = 1e-5


@functools.lru_cache(maxsize=None)
def gn_case(name):
  """(x1, x2, st1, st2, gamma, beta): bf16-valued activations with a scale per (sample, channel pair) and an offset per (sample, 16-row
  block, channel pair), every 16th pixel an outlier 8 sigma out (a group of two channels over 64 pixels then normalises to ~ +-7, times a
  gain of 20 and the scale 8: saturated); gains in {0.25, 1, 3, 20} and shifts in {-9, -3, 0, 2} by channel, so that under SiLU whole
  channels sit at -13 .. -6 (8 silu there: e4m3 subnormals)."""
  B, H, W, C1, C2, silu, form = GN_CASES[name]
  seed = 1700 + sum(ord(c) for c in name)
  HW, C = H * W, C1 + C2
  x = G.consumer_acts(B, HW, C, 2, seed).clone()
  x[:, ::16] += 8.0 * torch.sign(_rnd((B, (HW + 15) // 16, C), seed + 1))
  x = bf(x)
  gamma = torch.tensor([0.25, 1.0, 3.0, 20.0])[torch.randint(0, 4, (C,), generator=_gen(seed + 2))] * (1.0 + 0.1 * _rnd((C,), seed + 3))
  beta = torch.tensor([-9.0, -3.0, 0.0, 2.0])[torch.randint(0, 4, (C,), generator=_gen(seed + 4))] + 0.1 * _rnd((C,), seed + 5)
  x1, x2 = x[..., :C1].contiguous(), (x[..., C1:].contiguous() if C2 else None)
  st1 = st2 = None
  if form != "tensor":
    bin1, ns1, bin2, ns2 = form
    st1 = G.host_partials(G.bin_totals(x1, bin1), ns1, seed + 6)
    if C2:
      st2 = G.host_partials(G.bin_totals(x2, bin2), ns2, seed + 7)
  return x1, x2, st1, st2, gamma, beta


def gn_emulated_bytes(name, defect=None, mode="rne"):
  """The fp32 emulation's bytes of a GN case (the stand-alone form's statistics: one fp32 partial per (sample, group) over the whole map of
  the concatenated tensor)."""
  B, H, W, C1, C2, silu, form = GN_CASES[name]
  x1, x2, st1, st2, gamma, beta = gn_case(name)
  if form == "tensor":
    x = x1 if x2 is None else torch.cat([x1, x2], -1)
    cg = (C1 + C2) // G.GROUPS
    _, table = G.emulate_apply(x, G.emulate_partials(x, H * W, cg), cg, gamma, beta, G.GROUPS, GN_EPS, silu)
  else:
    _, table = G.emulate_apply(x1, st1, form[0], gamma, beta, G.GROUPS, GN_EPS, silu, x2=x2, st2=st2, bin2=form[2])
  return emulate_groupnorm_q(x1, x2, table, silu, CONV_ACT, defect, mode)


def gn_reference(name):
  B, H, W, C1, C2, silu, form = GN_CASES[name]
  x1, x2, _, _, gamma, beta = gn_case(name)
  x = x1 if x2 is None else torch.cat([x1, x2], -1)
  return groupnorm_q_ref(x, G.GROUPS, gamma, beta, GN_EPS, silu, CONV_ACT)


# ------------------------------------------------------------------------------------------------ LayerNorm -> e4m3 cases
# name -> (M, C, planes, ln_rows)
LN_CASES = {
  "m5_c128_p1": (5, 128, 1, 0),
  "m37_c320_p2": (37, 320, 2, 0),
  "m4_c1280_p5_const_onehot": (4, 1280, 5, 0),
  "m6_c128_p2_lnrows3": (6, 128, 2, 3),
}
LN_EPS = 1e-5


@functools.lru_cache(maxsize=None)
def ln_case(name):
  """(t (M, C) bf16-valued, stats (planes, R, 2) fp32).  The rows' fp64 sums are split into uneven shares and rounded to fp32 once.  C = 1280:
  row 0 constant 128 (a power of two and plane sums that add up exactly: the fp32 mean is exactly 128 and -mean * rstd has no rounding, so the
  row's output is exactly zero) with its sum of squares 8 ulp LOW (a producer's fp32 error: the variance comes out at -0.012), row 1 one-hot +3 (35.8
  sigma: saturates at +448), row 2 one-hot -3.  ln_rows: the second half of the rows are the first half reversed (the same sums)."""
  M, C, planes, ln_rows = LN_CASES[name]
  seed = 1900 + sum(ord(c) for c in name)
  R = ln_rows if ln_rows else M
  t = bf(_rnd((R, C), seed, 1.7) + 0.3 + 0.5 * _rnd((R, 1), seed + 1))
  if C == 1280:
    t[0] = 128.0
    t[1] = 0.0; t[1, 77] = 3.0
    t[2] = 0.0; t[2, C - 1] = -3.0
  tot = torch.stack([t.double().sum(1), (t.double() ** 2).sum(1)], -1)             # (R, 2)
  w = (0.2 + torch.rand((planes, R, 2), generator=_gen(seed + 2))).double()
  stats = (tot[None] * (w / w.sum(0, keepdim=True))).float()
  if C == 1280:      # row 0: shares in multiples of 4, so that the planes add up exactly in fp32: to 163 840 (mean exactly 128) and to 1280 * 2^14 - 16
    tot[0, 1] -= 16.0
    stats[:-1, 0] = torch.floor(stats[:-1, 0] / 4) * 4
    stats[-1, 0] = (tot[0] - stats[:-1, 0].double().sum(0)).float()
  stats = stats.contiguous()
  if ln_rows:
    t = torch.cat([t, t.flip(-1)[:M - R]], 0)
  return t.contiguous(), stats


LN_DEFECTS = ("scale_8", "planes_beyond_first_ignored", "ln_rows_ignored", "negative_variance_not_clamped")
ROUNDING_DEFECTS = ("trunc", "nosat", "flush")


def ln_defect_applies(defect, name):
  M, C, planes, ln_rows = LN_CASES[name]
  return {"scale_8": True, "planes_beyond_first_ignored": planes > 1, "ln_rows_ignored": ln_rows > 0,
          "negative_variance_not_clamped": C == 1280}[defect]


def rounding_defect_applies(mode, v64):
  """does the tensor hold a value the rounding defect gets wrong?"""
  v = v64[torch.isfinite(v64)].abs()
  if mode == "nosat":
    return bool((v > 448.0 * (1 + 2.0 ** -20)).any())
  if mode == "flush":
    return bool(((v >= 2.0 ** -10 * 1.01) & (v < 2.0 ** -6 * 0.99)).any())
  return True


# ------------------------------------------------------------------------------------------------ GEGLU cases, emulation and defects
GEGLU_CASES = [(1, 128, 32), (129, 128, 96), (200, 384, 160), (256, 640, 256)]          # (M, K, N physical)
GEGLU_DEFECTS = ("gate_scale_from_value_column", "value_and_gate_swapped", "last_n_tile_not_masked", "one_k_step_reads_a_second")


@functools.lru_cache(maxsize=None)
def geglu_case(M, K, N):
  """(t (M, K) bf16-valued, its one-plane row sums (1, M, 2) fp32, w (N, K) bf16-valued rows in the PHYSICAL order, bias (N))."""
  seed = 2100 + M + 3 * K + 7 * N
  t = bf(_rnd((M, K), seed, 1.7) + 0.3)
  stats = torch.stack([t.double().sum(1), (t.double() ** 2).sum(1)], -1).float()[None].contiguous()
  w = linear_weights(N, K, seed + 1).clone()
  w[1] = bf(_rnd((K,), seed + 2, K ** -0.5))        # (no zero row here: a zero value row would hide its gate)
  return t, stats, w, _rnd((N,), seed + 3, 0.3)


def geglu_defect_applies(defect, M, K, N):
  return {"gate_scale_from_value_column": True, "value_and_gate_swapped": True, "last_n_tile_not_masked": N % 128 != 0,
          "one_k_step_reads_a_second": K == 128}[defect]


def emulate_geglu(x8, w8, colscale, bias, defect=None, guard=256):
  """fp32 restatement of geglu_fp8_kernel on bytes.  Returns (out (M, N / 2) bf16-valued, the `guard` floats behind it: zeros unless the
  emulated kernel wrote there)."""
  x, w = decode(x8).float(), decode(w8).float()
  M, K = x.shape
  N = w.shape[0]
  inner = N // 2
  cs, b = colscale.float().cpu(), bias.float().cpu()
  acc = x @ w.T
  if defect == "one_k_step_reads_a_second":       # the pointers step 128 bytes on: the next row of each operand (clamped at the last row)
    xn = torch.cat([x[1:], x[-1:]], 0)
    wn = torch.cat([w[1:], w[-1:]], 0)
    acc = acc + xn @ wn.T
  (av, ag), (sv, sg), (bv, bg) = (tuple(u.T for u in geglu_split(acc.T))), geglu_split(cs), geglu_split(b)
  if defect == "gate_scale_from_value_column":
    sg = sv
  V, Gt = av * sv + bv, ag * sg + bg
  if defect == "value_and_gate_swapped":
    V, Gt = Gt, V
  out = bf(V * gelu_erf32(Gt))
  buf = torch.zeros(M * inner + guard)
  buf[:M * inner] = out.flatten()
  if defect == "last_n_tile_not_masked":          # the columns of the tile beyond N are stored too: row m's spill lands at the head of row m + 1 ...
    spill = ((N + 127) // 128 * 128 - N) // 2
    buf[M * inner:M * inner + spill] = 1.0        # ... and the last row's behind the tensor
  return buf[:M * inner].reshape(M, inner), buf[M * inner:]


def geglu_natural_case():
  """Operands on dyadic grids, so that every fp32 sum the loader's recipe and the row-sum kernel form is exact in any order: t in eighths,
  beta in quarters, w (diffusers order [value rows | gate rows]) in 2^-8, b in 2^-10; gamma is free (it only multiplies elementwise)."""
  M, C, inner = 129, 128, 48
  g = _gen(2300)
  t = torch.randint(-32, 33, (M, C), generator=g).float() / 8
  w = torch.randint(-100, 101, (2 * inner, C), generator=g).float() / 256
  b = torch.randint(-300, 301, (2 * inner,), generator=g).float() / 1024
  beta = torch.randint(-4, 5, (C,), generator=g).float() / 4
  gamma = 1.0 + 0.2 * _rnd((C,), 2301)
  return t, gamma, beta, w, b


# ------------------------------------------------------------------------------------------------ shared by the two test files
def conv_oihw_to_rows(w_oihw):
  """(Cout, Cin, 3, 3) values -> (Cout, Kpad) in the kernel's K order, zeros in the padding: the inverse of conv_w8_to_oihw."""
  cout, cin = w_oihw.shape[:2]
  rows = torch.zeros((cout, conv_kpad(cin)), dtype=w_oihw.dtype)
  rows[:, :9 * cin] = w_oihw.reshape(cout, cin // 64, 64, 9).permute(0, 3, 1, 2).reshape(cout, 9 * cin)
  return rows


def host_conv_bytes(name):
  """The case's operands quantised by the fp32 emulations: (x8 (B,H,W,Cin), w8 (Cout,Kpad), colscale (Cout))."""
  c = conv_case(name)
  w8, cs = emulate_weight_quant(conv_oihw_to_rows(c["w"]), CONV_ACT)
  return rne_code(c["x"].double() * CONV_ACT), w8, cs


def conv_figures(name, x8, w8, colscale, got):
  """got: dict(y (B,H,W,Cout)[, stats (B,nslab,nb,2)][, partials (splitk,M,Cout)]) from the device or from emulate_conv -> dict of figures
  (each passes at <= 1): "y" the per-element bar, "stats" the statistics' bar, "partials" every slice's fp32 partial against the
  accumulation term alone (acc_bar of the slice's K range and magnitude sum)."""
  c = conv_case(name)
  codes, _ = conv_w8_to_oihw(w8.cpu(), c["Cin"])
  ref, mag, pa, pm = conv_ref(x8.cpu(), codes, colscale, c["bias"], c["rowvec"], c["resid"])
  fig = {"y": ratio_figure(name, got["y"], ref, elem_bar(c["K"], ref, pm, mag))}
  if "stats" in got:
    fig["stats"] = stats_check(name, got["stats"], ref, pm, mag, c["K"], c["bin"])
  if "partials" in got:      # every slice against its own K range of the implicit GEMM (slices beyond the K steps: exactly zero, bar 0)
    p = got["partials"].double().cpu()
    a64, w64 = conv_a_matrix(decode(x8.cpu()), c["Cin"]), decode(w8.cpu())
    csd = colscale.double().cpu()
    steps = conv_kpad(c["Cin"]) // 128
    per = -(-steps // c["splitk"])
    pref, pbar = torch.zeros_like(p), torch.zeros_like(p)
    for z in range(c["splitk"]):
      k0, k1 = min(z * per, steps) * 128, min((z + 1) * per, steps) * 128
      if k1 > k0:
        pref[z] = a64[:, k0:k1] @ w64[:, k0:k1].T * csd
        pbar[z] = acc_bar(k1 - k0, a64[:, k0:k1].abs() @ w64[:, k0:k1].abs().T * csd)
    fig["partials"] = ratio_figure(name + " split-K partials", p, pref, pbar)
  return fig
