"""fp64 restatement of the VAE mid block's single-head attention behind its GroupNorm (csrc/vae.hip vae_attention_chain), its inputs, its
metrics and its bars, for tests/test_vae_attention_host.py, tests/test_vae_attention_gpu.py and tools/vae_attention_tolerance.py.  Written from
the structure (diffusers AutoencoderKL mid_block.attentions.0), not from the engine; CPU, torch only.

    q = (n Wq^T + bq) / sqrt(C)    k = n Wk^T + bk    v = n Wv^T + bv
    S = q k^T    P = softmax(S)    O = P v    out = O Wo^T + bo [+ resid]

`attn_exact` rounds nothing.  `attn_storage` rounds exactly the tensors the engine STORES as bf16 — q (after scaling), k, v, S, P, O, out — and
nothing else; its distance from `attn_exact` (STORAGE below, measured by the tool) is what bf16 storage alone costs, and the GPU bars are twice it.

TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import math

import torch

STORED = ("q", "k", "v", "S", "P", "O", "out")

# (B, HW, C) of the GPU chain test and the gains (to_q multiplier = score standard deviation) it runs each at
SHAPES = ((2, 64, 64), (3, 256, 128), (2, 576, 512), (2, 1024, 512))
GAINS = (1, 4)
# (rows, n) of the softmax kernel's own test: rows off the 4 rows per block, n around the 512-element per-wave stride
SOFTMAX_SHAPES = ((4, 8), (5, 64), (3, 504), (4, 512), (7, 520), (8, 576), (2, 4096))
BLOCK_CASE = (3, 256, 128, 4)      # the whole-block case (GroupNorm + chain against oracle/vae_ref._attn): B, HW, C, gain


def case_seed(B, HW, C, gain):
  return 1000 * gain + HW + C + B


def bf16_round(t: torch.Tensor) -> torch.Tensor:
  return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def attn_inputs(B: int, HW: int, C: int, gain: float, seed: int):
  """bf16-representable fp64 operands: n (B,HW,C) ~ normal with a per-channel scale and a per-sample offset (samples differ in more than noise),
  wq / wk / wv / wo (C,C) ~ N(0, 1/C) with to_q multiplied by `gain` (score standard deviation ~ gain), bq / bk / bv / bo (C) ~ N(0, 0.3^2) —
  large enough that a dropped bias shows — and a residual (B,HW,C) ~ N(0,1)."""
  g = torch.Generator().manual_seed(seed)
  r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
  scale = 0.6 + 0.8 * torch.rand(C, generator=g, dtype=torch.float64)
  scale = scale / scale.pow(2).mean().sqrt()
  d = {"n": r(B, HW, C) * scale + 0.3 * r(B, 1, C)}
  for name in ("wq", "wk", "wv", "wo"):
    d[name] = r(C, C) / math.sqrt(C)
  d["wq"] = d["wq"] * gain
  for name in ("bq", "bk", "bv", "bo"):
    d[name] = 0.3 * r(C)
  d["resid"] = r(B, HW, C)
  return {k: bf16_round(v) for k, v in d.items()}


def attn_chain(inp, with_resid: bool, store=(), mutate: str = None):
  """The chain in fp64; tensors named in `store` (of STORED) are rounded to bf16 where the engine stores them.  `mutate`: one seeded mistake
  (MUTANTS) for the host test.  Returns (out (B,HW,C), P (B,HW,HW))."""
  rnd = lambda name, t: bf16_round(t) if name in store else t   # noqa: E731
  n = inp["n"]
  B, HW, C = n.shape
  scale = 1.0 / math.sqrt(C)
  if mutate == "scale_log2e":
    scale *= math.log2(math.e)
  if mutate == "scale_ln2":
    scale *= math.log(2.0)
  zero = torch.zeros(C, dtype=n.dtype)
  q = rnd("q", (n @ inp["wq"].T + (zero if mutate == "no_q_bias" else inp["bq"])) * scale)
  k = rnd("k", n @ inp["wk"].T + inp["bk"])
  v = rnd("v", n @ inp["wv"].T + (zero if mutate == "no_v_bias" else inp["bv"]))
  if mutate in ("kv_sample0", "k_sample0"):
    k = k[:1].expand(B, HW, C)
  if mutate in ("kv_sample0", "v_sample0"):
    v = v[:1].expand(B, HW, C)
  if mutate == "v_shift1":
    v = torch.roll(v, 1, dims=1)
  S = rnd("S", q @ k.transpose(1, 2))
  if mutate == "last64":
    S = S.clone(); S[:, :, HW - 64:] = -math.inf
  if mutate == "last8":
    S = S.clone(); S[:, :, HW - 8:] = -math.inf
  if mutate == "uniform":
    S = torch.zeros_like(S)
  P = rnd("P", torch.softmax(S, dim=-1))
  if mutate == "p_last_image":
    P = P[B - 1:].expand(B, HW, HW)
  O = rnd("O", P @ v)
  out = O @ inp["wo"].T + (zero if mutate == "no_out_bias" else inp["bo"])
  if with_resid:
    out = out + {None: 1.0, "resid_dropped": 0.0, "resid_twice": 2.0}.get(mutate, 1.0) * inp["resid"]
  return rnd("out", out), P


# Seeded mistakes of the host test.  ("to_k bias dropped" is not one: bk adds q_i . bk to every score of row i, which no softmax can see.)
MUTANTS = ("kv_sample0", "k_sample0", "v_sample0", "p_last_image", "scale_log2e", "scale_ln2", "last64", "last8", "uniform", "v_shift1",
           "no_q_bias", "no_v_bias", "no_out_bias", "resid_dropped", "resid_twice")


def attn_exact(inp, with_resid: bool):
  return attn_chain(inp, with_resid)


def attn_storage(inp, with_resid: bool):
  return attn_chain(inp, with_resid, store=STORED)


def distances(got: torch.Tensor, ref: torch.Tensor):
  """(worst-sample rel-L2, worst-row rel-L2) of got against ref, both (B, rows, cols).  The row figure is what sees a mistake confined to a few
  rows or a few keys."""
  d = got.double() - ref.double()
  ref = ref.double()
  sample = (d.flatten(1).norm(dim=1) / ref.flatten(1).norm(dim=1)).max().item()
  row = (d.norm(dim=2) / ref.norm(dim=2)).max().item()
  return sample, row


METRICS = ("out", "out_resid", "P")

# tools/vae_attention_tolerance.py (CPU, the inputs above): distances(attn_storage, attn_exact) as (sample, row) per metric, rounded UP to four
# digits (profiles/vae_attention.md).  The GPU bars are TWICE these figures: the factor covers the MFMA accumulation and split-K order and __expf.
STORAGE = {
  (2, 64, 64, 1): {"out": (3.011e-03, 4.446e-03), "out_resid": (2.095e-03, 2.683e-03), "P": (4.205e-03, 8.577e-03)},
  (2, 64, 64, 4): {"out": (6.284e-03, 1.902e-02), "out_resid": (4.377e-03, 1.319e-02), "P": (8.486e-03, 2.942e-02)},
  (3, 256, 128, 1): {"out": (2.577e-03, 5.469e-03), "out_resid": (1.910e-03, 3.468e-03), "P": (5.587e-03, 1.388e-02)},
  (3, 256, 128, 4): {"out": (8.448e-03, 2.981e-02), "out_resid": (5.736e-03, 1.760e-02), "P": (1.180e-02, 4.040e-02)},
  (2, 576, 512, 1): {"out": (2.273e-03, 3.580e-03), "out_resid": (1.815e-03, 2.209e-03), "P": (4.978e-03, 1.358e-02)},
  (2, 576, 512, 4): {"out": (9.208e-03, 3.539e-02), "out_resid": (5.873e-03, 2.168e-02), "P": (1.220e-02, 5.413e-02)},
  (2, 1024, 512, 1): {"out": (2.287e-03, 3.775e-03), "out_resid": (1.798e-03, 2.261e-03), "P": (5.128e-03, 1.490e-02)},
  (2, 1024, 512, 4): {"out": (9.677e-03, 4.668e-02), "out_resid": (5.949e-03, 2.683e-02), "P": (1.287e-02, 5.766e-02)},
}

# the whole-block case: GroupNorm (fp64, output rounded to bf16) + attn_storage against the fp64 block, (sample, row) of the output
BLOCK_STORAGE = (4.919e-03, 1.615e-02)


def bars(key):
  return {m: (2 * s, 2 * r) for m, (s, r) in STORAGE[key].items()}


def check_chain(key, out, out_resid, P, exact):
  """The GPU test's check, shared with the host test.  `exact`: {"out", "out_resid", "P"} from attn_exact.  Returns a list of
  (name, measured, bar) — the caller asserts measured <= bar for every entry."""
  res = []
  b = bars(key)
  for m, got in (("out", out), ("out_resid", out_resid), ("P", P)):
    s, r = distances(got, exact[m])
    if not bool(torch.isfinite(got).all()):      # (the GPU test asserts finiteness; NaN compares false with everything)
      s = r = math.inf
    res.append((m + ".sample", s, b[m][0]))
    res.append((m + ".row", r, b[m][1]))
  res.append(("P.rowsum", (P.double().sum(-1) - 1).abs().max().item(), 2.0 ** -8))
  return res


def exact_of(inp):
  o, P = attn_exact(inp, False)
  return {"out": o, "out_resid": attn_exact(inp, True)[0], "P": P}


# ---- the whole block: GroupNorm(32, eps 1e-6) + chain + residual = x, against oracle/vae_ref._attn
def block_inputs(B, HW, C, gain, seed):
  """x (B,HW,C) bf16-representable with per-channel scale and mean (so the GroupNorm matters), gamma / beta, and attn_inputs' weights."""
  inp = attn_inputs(B, HW, C, gain, seed)
  g = torch.Generator().manual_seed(seed + 7)
  r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
  x = bf16_round(inp["n"] * (1.0 + 0.5 * torch.rand(C, generator=g, dtype=torch.float64)) + 0.5 * r(C))
  return x, bf16_round(1.0 + 0.2 * r(C)), bf16_round(0.2 * r(C)), inp


def block_state_dict(gamma, beta, inp, p="a"):
  sd = {p + ".group_norm.weight": gamma, p + ".group_norm.bias": beta}
  for lin, w, b in (("to_q", "wq", "bq"), ("to_k", "wk", "bk"), ("to_v", "wv", "bv"), ("to_out.0", "wo", "bo")):
    sd[f"{p}.{lin}.weight"], sd[f"{p}.{lin}.bias"] = inp[w], inp[b]
  return sd


def softmax_cases(rows: int, n: int, seed: int):
  """Two (rows, n) bf16 softmax inputs for any rows >= 2: normal x 1 with row 0 all-equal, and normal x 30 with row 0 all -3e4 (uniform result) and
  the last row a single entry 80 above the rest (exactly one 1 and zeros)."""
  g = torch.Generator().manual_seed(seed)
  a = torch.randn(rows, n, generator=g)
  b = 30.0 * torch.randn(rows, n, generator=g)
  a[0] = 1.25
  b[0] = -3e4
  b[rows - 1] = -7.0
  b[rows - 1, (5 * n) // 8] = 73.0
  return [a.to(torch.bfloat16), b.to(torch.bfloat16)]


def check_softmax(got: torch.Tensor, s: torch.Tensor):
  """got, s (rows, n) bf16: the fp64 softmax of the same bf16 values, one bf16 ulp (|got - want| <= 2^-7 want) for want >= 2^-120, got <= 2^-119 below,
  row sums within 2^-8 of 1.  Returns a list of failure strings (empty: passes)."""
  want = torch.softmax(s.double(), dim=-1)
  g = got.double()
  bad = []
  if not bool(torch.isfinite(g).all()):
    return ["non-finite output"]
  big = want >= 2.0 ** -120
  err = ((g - want).abs() / want.clamp_min(2.0 ** -130))[big]
  if err.numel() and err.max().item() > 2.0 ** -7:
    bad.append(f"relative error {err.max().item():.3e} > 2^-7")
  if (~big).any() and g[~big].max().item() > 2.0 ** -119:
    bad.append(f"underflow region holds {g[~big].max().item():.3e}")
  rs = (g.sum(-1) - 1).abs().max().item()
  if rs > 2.0 ** -8:
    bad.append(f"row sum off by {rs:.3e}")
  return bad
