"""Shared by test_w8_host.py, test_w8_ops_gpu.py, test_w8_decode_gpu.py, test_w8_generate_gpu.py and tools/w8_tolerance.py (not a
test module): the weight-only fp8 decoder format ("w8", include/gill_amd.h gill_opt_create_ex) on the host.

  * `quantise` / `dequantise`: the reference quantiser, torch on the CPU with torch.float8_e4m3fn for the rounding; `kernel_order`: the
    bytes in the storage order of csrc/linear_w8.hip; `w8_state_dict`: a state dict with the four matrices of every decoder layer
    replaced by their dequantised values (the quantised model IS that bf16 model);
  * `emulate_linear`: an fp32 emulation of linear_w8_kernel's sum (bf16 operands, fp32 accumulation, K visited in the kernel's permuted
    and split order: 32-wide MFMA chunks, four waves taking the 64-wide K steps in turn, waves then slices added in order), with a
    `defect=` switch; `reference_linear`: fp64 on the same operands; `magnitude`: sum_k |a| |w| + |bias| + |resid|, the unit of the bar;
  * the bars.  W8_ACC_DIST is the largest |emulation - fp64| / magnitude over OP_CASES, measured on the CPU by
    `python tools/w8_tolerance.py --write` (-> profiles/w8_decode.md); the operator bar is 10 x that (the project's precedent:
    tools/decode_sample_tolerance.py, tools/lm_loss_tolerance.py) times the magnitude, plus half a bf16 ulp of the result for bf16 outputs."""
import torch

import kv_cache_util as U

MAX_ROWS = 16                      # W8_MAX_ROWS of csrc/ops.h (gill_w8_max_rows() on the GPU tests)
W8_ACC_DIST = 6.1e-08              # tools/w8_tolerance.py: largest |fp32 emulation - fp64| / magnitude over OP_CASES
W8_BAR = 10 * W8_ACC_DIST

DEFECTS = ("scale_of_next_row", "scale_dropped", "k_pair_swapped", "relu_before_bias", "partial_dropped", "padding_rows_nan")

# (N, K, splitk) of the operator test; splitk 0 = the launcher's rule (pick_splitk)
#   (64, 64, 1)      one column group per wave and one K step: waves 1 .. 3 have no step at all
#   (192, 320, 1)    three workgroups, four column groups per wave; K = 5 x 64 is no multiple of the loop's unroll (4 steps) nor of the 4 waves
#   (192, 320, 2/3)  forced split: 5 K steps over 2 (2 + 3) and 3 (1 + 2 + 2) slices
#   (768, 3072, 0)   the launcher's own rule on OPT-125m's fc2: 4 slices of 12 steps
#   (4096, 4096, 0)  one OPT-6.7b matrix (out_proj): 4 slices of 16 steps, 256 workgroups
#   (128, 4160, 1)   65 K steps unsplit: a second activation stage (2048 columns each) of one step
OP_CASES = ((64, 64, 1), (192, 320, 1), (192, 320, 2), (192, 320, 3), (768, 3072, 0), (4096, 4096, 0), (128, 4160, 1))
OP_ROWS = (1, 3, 16, MAX_ROWS)


def pick_splitk(N, K):
  """w8_pick_splitk of csrc/linear_w8.hip."""
  tiles, nkb = N // 64, K // 64
  return max(1, min(-(-256 // tiles), nkb // 8, 4))


# ------------------------------------------------------------------------------------------------ the format
def quantise(w):
  """w (N, K) fp32 holding bf16 values -> (q (N, K) torch.float8_e4m3fn, s (N) fp32 = 2^e).  e = ceil(log2(max|w| / 448)) from the
  maximum's mantissa and exponent (max = f 2^p, f in [0.5, 1): e = p - 9 for f <= 448 / 512, else p - 8), kept >= -100; a zero row: s = 1."""
  w = w.float()
  amax = w.abs().amax(1)
  f, p = torch.frexp(amax)
  e = torch.where(f <= 0.875, p - 9, p - 8).clamp_min(-100)
  e = torch.where((amax > 0) & torch.isfinite(amax), e, torch.zeros_like(e))
  s = torch.ldexp(torch.ones_like(amax), e)
  return (w / s[:, None]).to(torch.float8_e4m3fn), s


def dequantise(q, s):
  return q.float() * s[:, None]


def kernel_order(q):
  """q (N, K) float8 -> uint8 (N * K) in linear_w8.hip's order [N / 16][K / 64][(k % 64) / 16][n % 16][k % 16]."""
  N, K = q.shape
  b = q.view(torch.uint8).view(N // 16, 16, K // 64, 4, 16)
  return b.permute(0, 2, 3, 1, 4).contiguous().view(-1)


def blk64(w):
  """(N, K) -> the 64 x 64-blocked order [N / 64][K / 64][64][64], flat."""
  N, K = w.shape
  return w.view(N // 64, 64, K // 64, 64).permute(0, 2, 1, 3).contiguous().view(-1)


W8_MATRICES = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj", "fc1", "fc2")


def w8_state_dict(sd, cfg):
  """sd with the four matrices ([q|k|v] stacked: a row's scale is its own) of every decoder layer replaced by w8 * s; everything else as it is."""
  out = dict(sd)
  for i in range(cfg.num_layers):
    for n in W8_MATRICES:
      k = f"model.decoder.layers.{i}.{n}.weight"
      out[k] = dequantise(*quantise(U.bf(sd[k].float()))).to(sd[k].dtype)
  return out


# ------------------------------------------------------------------------------------------------ the linear
def operands(N, K, M, seed):
  """A (M, K) bf16-valued N(0, 1); w (N, K) bf16-valued N(0, 0.02) with row n scaled by 2^(n % 5 - 2) (neighbouring rows have different
  scales), bias (N) ~ 0.5 N(0, 1), resid (M, N) N(0, 1), LayerNorm gamma / beta."""
  g = torch.Generator().manual_seed(seed)
  r = lambda *sh: torch.randn(sh, generator=g)   # noqa: E731
  A = U.bf(r(MAX_ROWS, K))[:M].clone()          # row m is the same for every M
  w = U.bf(r(N, K) * 0.02 * torch.pow(2.0, (torch.arange(N) % 5 - 2).float())[:, None])
  return dict(A=A, w=w, bias=0.5 * r(N), resid=r(MAX_ROWS, N)[:M].clone(), gamma=1.0 + 0.1 * r(N), beta=0.1 * r(N))


def k_schedule(K, sk):
  """[slice][wave] -> the 64-wide K steps in the order the wave visits them (stages of 32 steps, wave w: s0 + w, s0 + w + 4, ...)."""
  nkb = K // 64
  out = []
  for z in range(sk):
    kb0, kb1 = z * nkb // sk, (z + 1) * nkb // sk
    waves = [[] for _ in range(4)]
    for s0 in range(kb0, kb1, 32):
      for w in range(4):
        waves[w] += list(range(s0 + w, min(s0 + 32, kb1), 4))
    out.append(waves)
  return out


def emulate_linear(A, qv, s, bias=None, resid=None, act="none", sk=1, out_bf16=False, defect=None):
  """The kernel's arithmetic in fp32 on the 16-row tile -> (16, N) (rows M .. 15: what the accumulators of the padding rows hold; the
  kernel does not store them).  A (M, K) bf16-valued, qv (N, K) the e4m3 values as fp32, s (N)."""
  assert defect is None or defect in DEFECTS
  M, K = A.shape
  N = qv.shape[0]
  nkb = K // 64
  Ap = torch.zeros(16, K)
  Ap[:M] = A
  if defect == "padding_rows_nan":
    Ap[M:] = float("nan")
  Wv = qv.float().view(N, nkb, 4, 2, 8)
  if defect == "k_pair_swapped":          # positions 0 and 1 of every 32-block of the weights
    Wv = Wv.clone()
    Wv[:, :, 0, :, 0], Wv[:, :, 0, :, 1] = Wv[:, :, 0, :, 1].clone(), Wv[:, :, 0, :, 0].clone()
  # one MFMA: k = 64 kb + 16 q + 8 j + 0 .. 7 over q = 0 .. 3
  P = torch.einsum("mbqjk,nbqjk->bjmn", Ap.view(16, nkb, 4, 2, 8), Wv)
  sc = s.float()
  if defect == "scale_of_next_row":
    sc = sc.roll(-1)
  parts = []
  for waves in k_schedule(K, sk):
    tot = None
    for steps in waves:
      acc = torch.zeros(16, N)
      for kb in steps:
        acc = acc + P[kb, 0]
        acc = acc + P[kb, 1]
      tot = acc if tot is None else tot + acc
    parts.append(tot if defect == "scale_dropped" else tot * sc[None])
  if defect == "partial_dropped":
    assert sk > 1
    parts = parts[:-1]
  y = parts[0]
  for p in parts[1:]:
    y = y + p
  b = torch.zeros(N) if bias is None else bias.float()
  if defect == "relu_before_bias":
    assert act == "relu"
    y = torch.relu(y) + b[None]
  else:
    y = y + b[None]
    if act == "relu":
      y = torch.relu(y)
  if resid is not None:
    y[:M] = y[:M] + resid.float()
  return U.bf(y) if out_bf16 else y


def reference_linear(A, qv, s, bias=None, resid=None, act="none"):
  """fp64 on the same operands -> (M, N)."""
  y = A.double() @ (qv.double() * s.double()[:, None]).T
  if bias is not None:
    y = y + bias.double()[None]
  if act == "relu":
    y = torch.relu(y)
  if resid is not None:
    y = y + resid.double()
  return y


def magnitude(A, qv, s, bias=None, resid=None):
  m = A.double().abs() @ (qv.double().abs() * s.double()[:, None]).T
  if bias is not None:
    m = m + bias.double().abs()[None]
  if resid is not None:
    m = m + resid.double().abs()
  return m


def half_ulp_bf16(x):
  """Half a bf16 ulp at |x| (fp64 in, fp64 out): 2^(e - 9) for |x| = f 2^e, f in [0.5, 1)."""
  _, e = torch.frexp(x.abs().clamp_min(2.0 ** -120))
  return torch.ldexp(torch.ones_like(x), e - 9)


def element_bar(ref, mag, out_bf16, factor=W8_BAR):
  return factor * mag + (half_ulp_bf16(ref) if out_bf16 else 0.0)


def figure(name, got, ref, bar):
  """max |got - ref| / bar over the elements (inf for a non-finite result); prints it."""
  err = (got.double() - ref).abs() / bar
  err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
  f = err.max().item()
  print(f"[{name}] worst |got - fp64| / bar = {f:.3f}  (max abs err {(got.double() - ref).abs().nan_to_num(float('inf')).max().item():.3e})")
  return f


def acc_distance(N, K, M, sk, seed):
  """|fp32 emulation - fp64| / magnitude, its maximum over the elements, bias + fp32 residual epilogue, fp32 out."""
  o = operands(N, K, M, seed)
  q, s = quantise(o["w"])
  qv = q.float()
  y = emulate_linear(o["A"], qv, s, o["bias"], o["resid"], sk=sk or pick_splitk(N, K))[:M]
  ref = reference_linear(o["A"], qv, s, o["bias"], o["resid"])
  return ((y.double() - ref).abs() / magnitude(o["A"], qv, s, o["bias"], o["resid"])).max().item()
