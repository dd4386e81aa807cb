"""Shared by test_kv8_host.py, test_attention_kv8_gpu.py, test_kv8_engine_gpu.py and tools/kv8_tolerance.py (not a test module): the e4m3 KV
cache ("kv8", include/gill_amd.h, csrc/attention_kv8_dev.h) on the host.

  * `quantise_rows` / `dequantise_rows`: the row quantiser, w8_util.quantise per (token, head) row of d elements (the input is rounded to bf16
    first, as the device's projection output is); exponents as int8;
  * `attend`: cached attention on a quantised cache, the arithmetic the two kernels share stated once: the key scale multiplies the finished
    score, the value scale goes into the probability, every key and value, the query token's own included, enters as code x 2^e.  dtype
    float64 with no rounding is THE REFERENCE (it equals plain attention on the dequantised operands); float32 with `rnd_p` (the extend kernel
    rounds P to bf16 for its MFMAs, the decode kernel does not) is the emulation; `defect=` breaks it in one of the ways DEFECTS lists;
  * `kv8_forward`: the OPT engine with that attention, one causal pass per sequence.  The quantised-cache model is an exact function of the token
    sequence (every key and value is rounded before any query uses it), so the ragged prefill, the extend pass of a session and the single
    steps are all this one function; `n_ext` says which positions went through the extend kernel (P rounded) for the emulation;
  * `greedy_ref`: the reference's own greedy run of one row; `prompt_ids`, the bars and seeds of tests/golden/kv8_tolerance.json
    (tools/kv8_tolerance.py --write measures and chooses them on the CPU)."""
import functools
import json
import os

import torch
import torch.nn.functional as F

import kv_cache_util as U
import ragged_decode_util as R
import w8_util as W
from gill_amd import synth

DEFECTS = ("scale_of_neighbour",          # slot j is scaled by the exponent of slot j - 1 (keys and values)
           "scale_dropped",               # codes are used as values: every scale is 1
           "v_scale_on_k",                # the key's score takes the VALUE's exponent of its slot
           "own_token_unquantised",       # the query token's own key and value enter as the bf16 rows, not as their codes
           "exponent_unsigned",           # the int8 exponent is read as uint8: a negative e becomes e + 256
           "stale_exponent_visible")      # the query token's own key and value take the exponent its slot held before the store

TOLERANCE_FILE = "kv8_tolerance.json"     # under tests/golden
LENGTHS = R.RUNS["b3"][0]                 # the ragged batch of the engine test: (30, 23, 9)
N_DEC = 6                                 # free greedy decisions per row (min_word_tokens = N_DEC: the [IMG] ids stay filtered)
SEED = 46
MARGIN = 4.0                              # bar = MARGIN x the emulation's worst distance from the fp64 run: the margin of the w8 tests


# ------------------------------------------------------------------------------------------------ the format
def quantise_rows(x):
  """x (..., d) -> (codes (..., d) torch.float8_e4m3fn, e (...) int8) of bf16(x), a row's scale being 2^e."""
  d = x.shape[-1]
  q, s = W.quantise(U.bf(x.float()).reshape(-1, d))
  e = torch.frexp(s)[1] - 1
  return q.view(x.shape), e.to(torch.int8).view(x.shape[:-1])


def pow2(e, dtype=torch.float32):
  return torch.ldexp(torch.ones(e.shape, dtype=dtype), e.to(torch.int32))


def dequantise_rows(q, e, dtype=torch.float32):
  return q.to(dtype) * pow2(e, dtype)[..., None]


def code_bytes(q):
  """float8 codes -> uint8 with the sign bit of a zero code cleared (+0 and -0 are one value)."""
  b = q.view(torch.uint8).clone()
  b[b == 0x80] = 0
  return b


# ------------------------------------------------------------------------------------------------ attention on a quantised cache
def attend(q, kq, ke, vq, ve, dtype=torch.float32, defect=None, rnd_p=None, n_ext=0, k_raw=None, v_raw=None, stale_e=0):
  """q (H, nq, d), already scaled by d^-0.5, the last nq tokens of a sequence of nkv; kq / vq (H, nkv, d) the code VALUES, ke / ve (H, nkv)
  integer exponents.  Query i sees the keys 0 .. nkv - nq + i.  rnd_p / n_ext: the first n_ext queries round P (behind the row sum, as the
  extend kernel does).  k_raw / v_raw (H, nkv, d): the rows before quantisation (own_token_unquantised); stale_e: what the queries' own slots
  held as exponent before the store (stale_exponent_visible).  -> (H, nq, d) in dtype."""
  assert defect is None or defect in DEFECTS
  H, nq, d = q.shape
  nkv = kq.shape[1]
  past = nkv - nq
  ke, ve = ke.to(torch.int32), ve.to(torch.int32)
  if defect == "exponent_unsigned":
    ke, ve = ke % 256, ve % 256
  if defect == "scale_of_neighbour":
    ke, ve = ke.roll(1, 1), ve.roll(1, 1)
  if defect == "scale_dropped":
    ke, ve = torch.zeros_like(ke), torch.zeros_like(ve)
  ks = pow2(ve if defect == "v_scale_on_k" else ke, dtype)       # (H, nkv)
  vs = pow2(ve, dtype)
  qd, kc, vc = q.to(dtype), kq.to(dtype), vq.to(dtype)
  s = (qd @ kc.transpose(1, 2)) * ks[:, None, :]                 # the scale multiplies the finished score
  vsq = vs[:, None, :].expand(H, nq, nkv).clone()                # the value scale as query i applies it to key j
  own = torch.arange(nq) + past
  ii = torch.arange(nq)
  vown = None
  if defect == "own_token_unquantised":
    s[:, ii, own] = (qd * k_raw[:, past:].to(dtype)).sum(-1)
    vown = v_raw[:, past:].to(dtype) - vc[:, past:] * vs[:, past:, None]     # what the own term gains over its dequantised row
  if defect == "stale_exponent_visible":
    st = pow2(torch.as_tensor(stale_e, dtype=torch.int32).expand(H, nq), dtype)
    s[:, ii, own] = (qd * kc[:, past:]).sum(-1) * st
    vsq[:, ii, own] = st
  vis = torch.arange(nkv)[None, :] <= own[:, None]
  s = s.masked_fill(~vis[None], float("-inf"))
  e = torch.exp(s - s.amax(-1, keepdim=True))
  l = e.sum(-1, keepdim=True)
  p = e
  if rnd_p is not None and n_ext > 0:
    p = torch.cat([rnd_p(e[:, :n_ext]), e[:, n_ext:]], 1)
  o = (p * vsq) @ vc
  if vown is not None:
    o = o + p[:, ii, own][..., None] * vown
  return o / l


# ------------------------------------------------------------------------------------------------ the engine
def kv8_forward(sd, cfg, embeds, rnd=None, dtype=torch.float32, defect=None, n_ext=0):
  """The OPT decoder with an e4m3 KV cache on embeds (B, T, D), every row its own sequence from position 0 -> hidden_states[-1] (B, T, D) in
  dtype.  rnd: rounding of every GEMM operand and of the extend rows' P (the bf16-storage emulation; None: none).  Keys and values are rounded
  to bf16 and quantised either way: that IS the model."""
  ident = lambda t: t   # noqa: E731
  rnd = rnd or ident
  B, T, D = embeds.shape
  H = cfg.num_heads
  hd = D // H
  pre = "model.decoder."
  w = lambda n: sd[n].to(dtype)   # noqa: E731
  h = embeds.to(dtype) + w(pre + "embed_positions.weight")[2 + torch.arange(T)][None]
  heads = lambda t: t.view(B, T, H, hd).transpose(1, 2)     # noqa: E731
  for i in range(cfg.num_layers):
    p = f"{pre}layers.{i}."
    lin = lambda x, n: F.linear(rnd(x), w(p + n + ".weight"), w(p + n + ".bias"))   # noqa: E731
    y = F.layer_norm(h, (D,), w(p + "self_attn_layer_norm.weight"), w(p + "self_attn_layer_norm.bias"), 1e-5)
    q = heads(rnd(lin(y, "self_attn.q_proj"))) * hd ** -0.5          # the kernels scale the rounded q (the score) in fp32
    k_raw, v_raw = heads(U.bf(lin(y, "self_attn.k_proj").float())), heads(U.bf(lin(y, "self_attn.v_proj").float()))
    kq, ke = quantise_rows(k_raw)
    vq, ve = quantise_rows(v_raw)
    a = torch.stack([attend(q[b], kq[b].float(), ke[b], vq[b].float(), ve[b], dtype, defect, rnd if rnd is not ident else None, n_ext,
                            k_raw[b], v_raw[b]) for b in range(B)])
    h = h + lin(a.transpose(1, 2).reshape(B, T, D), "self_attn.out_proj")
    y = F.layer_norm(h, (D,), w(p + "final_layer_norm.weight"), w(p + "final_layer_norm.bias"), 1e-5)
    h = h + lin(F.relu(lin(y, "fc1")), "fc2")
  return F.layer_norm(h, (D,), w(pre + "final_layer_norm.weight"), w(pre + "final_layer_norm.bias"), 1e-5)


def logits_of(sd, hidden):
  """lm_head (tied to the embeddings unless the state dict has one) on hidden rows (n, D) -> (n, vocab) in hidden's dtype."""
  wt = sd["lm_head.weight"] if "lm_head.weight" in sd else sd["model.decoder.embed_tokens.weight"]
  return hidden @ wt.to(hidden.dtype).T


def row_rel(got, ref):
  """The hidden-state figure: the largest per-row |got - ref|_2 / |ref|_2 over rows (..., D); non-finite -> inf."""
  got, ref = got.double(), ref.double()
  r = (got - ref).norm(dim=-1) / ref.norm(dim=-1).clamp_min(1e-30)
  r = torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))
  return r.max().item() if r.numel() else 0.0


def greedy_ref(sd, cfg, row_ids, n_dec=N_DEC, emulate=True):
  """The fp64 quantised-cache model's own greedy run of one row for n_dec decisions with the [IMG] ids filtered.  -> dict(tokens, margins
  (top-2, in logits), ids (the whole sequence), hidden (len(ids), D) fp64 of the final sequence, logits [n_dec] fp64 after the filter, and with
  `emulate` hid_dist / logit_dist: the bf16-storage fp32 emulation's largest row_rel / |logit| distance from it over the decision rows)."""
  ids = [int(v) for v in row_ids]
  n0 = len(ids)
  table = sd["model.decoder.embed_tokens.weight"].float()
  toks, margins, all_logits, hid_dist, logit_dist = [], [], [], 0.0, 0.0
  for _ in range(n_dec):
    x = F.embedding(torch.tensor(ids)[None], table)
    h = kv8_forward(sd, cfg, x, dtype=torch.float64)[0]
    lg = logits_of(sd, h[-1:])[0]
    if emulate:      # the prompt through the extend kernel, the tokens behind it through single steps
      he = kv8_forward(sd, cfg, x, rnd=U.bf, n_ext=n0)[0]
      hid_dist = max(hid_dist, row_rel(he[n0 - 1:], h[n0 - 1:]))
      logit_dist = max(logit_dist, (logits_of(sd, U.bf(he[-1:]))[0].double() - lg).abs().max().item())
    lg[synth.IMG_TOKEN_IDS] = float("-inf")
    top = lg.topk(2)
    toks.append(int(top.indices[0]))
    margins.append(float(top.values[0] - top.values[1]))
    all_logits.append(lg)
    ids.append(toks[-1])
  x = F.embedding(torch.tensor(ids)[None], table)
  hidden = kv8_forward(sd, cfg, x, dtype=torch.float64)[0]
  return dict(tokens=toks, margins=margins, ids=ids, hidden=hidden, logits=all_logits, hid_dist=hid_dist, logit_dist=logit_dist)


def model(weights="bf16"):
  """(cfg, sd) of the OPT-125m rig (ragged_decode_util.gen_model); weights 'fp8': its w8 model (w8_util.w8_state_dict)."""
  cfg, sd = R.gen_model()
  return cfg, (W.w8_state_dict(sd, cfg) if weights == "fp8" else sd)


def prompt_row(b, seed, lengths=LENGTHS):
  """Row b of the engine test's ragged batch at its own seed: lengths[b] ids."""
  return synth.synthetic_prompt_ids(len(lengths), max(lengths), seed=seed)[b, :lengths[b]].clone()


def prompt_ids(seeds, lengths=LENGTHS, pad=1):
  """(ids (B, max(lengths)) right-padded, lengths) of the engine test's ragged batch; seeds: one per row (the golden file's)."""
  ids = torch.full((len(lengths), max(lengths)), pad, dtype=torch.int64)
  for b, n in enumerate(lengths):
    ids[b, :n] = prompt_row(b, seeds[b], lengths)
  return ids, list(lengths)


@functools.lru_cache(maxsize=None)
def batch_reference(weights, seeds):
  """greedy_ref (no emulation) of every row of prompt_ids(seeds) (a tuple) on model(weights); computed once, read-only."""
  cfg, sd = model(weights)
  ids, lens = prompt_ids(seeds)
  return [greedy_ref(sd, cfg, ids[b, :n], emulate=False) for b, n in enumerate(lens)]


def golden():
  path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", TOLERANCE_FILE)
  with open(path) as f:
    return json.load(f)


# ------------------------------------------------------------------------------------------------ operator level
def attn_operands(H, nq, nkv, d, seed):
  """kv_cache_util.decode_attn_inputs for one sequence, with token j's key row scaled by 2^(j % 3 - 1) and its value row by 2^(j % 5 - 2):
  neighbouring slots have different exponents, keys and values of a slot too.  -> q (nq, H*d), k, v (nkv, H*d), bf16-valued."""
  q, k, v = U.decode_attn_inputs(1, H, nq, nkv, d, seed=seed)
  j = torch.arange(nkv)
  k = k[0] * torch.pow(2.0, (j % 3 - 1).float())[:, None]
  v = v[0] * torch.pow(2.0, (j % 5 - 2).float())[:, None]
  return q[0], U.bf(k), U.bf(v)


def tie_operands(H, d, seed):
  """The inputs at which `own_token_unquantised` shows (on peaked random operands the e4m3 rounding of one row moves the output by less than
  the accuracy bar): two keys, the cached one and the new token's own, from the SAME bf16 row, so their codes are equal and the quantised model
  gives both a probability of exactly 1/2; q = 8 sign(row - dequantised row), so a raw own key would gain 8 sum |rounding error| / sqrt(d) on
  its score; the values are r and -r / 2 (the honest output is r / 4).  -> q (1, H*d), k, v (2, H*d), the new token last."""
  g = torch.Generator().manual_seed(seed)
  kr = U.bf(torch.randn(H, d, generator=g))
  delta = kr - dequantise_rows(*quantise_rows(kr))
  q = torch.where(delta >= 0, 8.0, -8.0).reshape(1, H * d)
  vr = U.bf(torch.randn(H, d, generator=g)).reshape(1, H * d)
  return q, kr.reshape(1, H * d).repeat(2, 1), torch.cat([-0.5 * vr, vr])


EDGE_ROWS = ("zero", "exact_448", "one_step_above", "subnormal_rest", "one_element_2e20")


def edge_row(kind, d, g):
  """A quantiser edge row of d bf16 values.  exact_448: the maximum is 448 * 2^-8 = 1.75 exactly (e = -8, the code 448); one_step_above: the
  next bf16 number, 1.7578125 (e = -7); subnormal_rest: beside a maximum of 1.75 every other element lies below the smallest normal code
  (2^-6 * 2^-8) and off the subnormal grid (multiples of 2^-9 * 2^-8), so it is rounded among the subnormal codes; one_element_2e20: one
  element 2^20 times the rest (the rest round to zero codes)."""
  r = torch.randn(d, generator=g)
  if kind == "zero":
    return torch.zeros(d)
  if kind in ("exact_448", "one_step_above"):
    x = U.bf(r.clamp(-3, 3) * 0.3)
    x[int(torch.randint(d, (1,), generator=g))] = 1.75 if kind == "exact_448" else 1.7578125
    return x
  if kind == "subnormal_rest":
    x = U.bf((torch.rand(d, generator=g) * 7.2 + 0.3) * torch.sign(r) * 2.0 ** -17)
    x[int(torch.randint(d, (1,), generator=g))] = -1.75
    return x
  x = U.bf(r * 2.0 ** -20)
  i = int(torch.randint(d, (1,), generator=g))
  x[i] = U.bf(x[i] * 2.0 ** 20 + torch.sign(r[i]) * 0.5)
  return x


def plant_edge_rows(k, v, H, d, first, seed):
  """Edge rows into the head slices of the tokens first .. of k / v (n, H*d), in place: token first + t gets EDGE_ROWS[(t + h) % 5] in head
  h < 2 of k for even t and of v for odd t (the other heads keep the peaked operands the accuracy figure is about)."""
  g = torch.Generator().manual_seed(seed)
  for t in range(k.shape[0] - first):
    for h in range(min(2, H)):
      (k if t % 2 == 0 else v)[first + t, h * d:(h + 1) * d] = edge_row(EDGE_ROWS[(t + h) % len(EDGE_ROWS)], d, g)


def quantise_heads(x, H, d):
  """x (n, H*d) -> codes (H, n, d) float8, e (H, n) int8."""
  return quantise_rows(x.view(-1, H, d).transpose(0, 1).contiguous())


def attention_ref(q, kq, ke, vq, ve, H, d):
  """THE REFERENCE of the operator tests: fp64 attention on the dequantised operands.  q (nq, H*d) unscaled; -> (nq, H*d) float32."""
  nq = q.shape[0]
  qh = q.view(nq, H, d).transpose(0, 1).double() * d ** -0.5
  o = attend(qh, kq.float(), ke, vq.float(), ve, torch.float64)
  return o.transpose(0, 1).reshape(nq, H * d).float()
