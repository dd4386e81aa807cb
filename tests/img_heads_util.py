"""Shared by test_img_heads_host.py, test_img_heads_gpu.py and tools/img_heads_tolerance.py (not a test module): the image-block heads
(gill_op_img_block_heads) and the rerank score (gill_op_img_rerank_scores) restated in numpy.

  * `op_inputs` / `rerank_inputs`: the operator tests' inputs per case, seeded;
  * `heads_ref`: THE REFERENCE: fp64 on the operands the kernel multiplies (the gathered row rounded to bf16, the bf16 weights);
  * `heads_emulate`: the kernel's arithmetic in fp32 (fp32 accumulation, norm, softmax) with K in a permuted, strictly sequential order: another
    legitimate summation order of the same sum.  Its distance from fp64 is what an fp32 accumulation costs at these shapes; the operator bars
    are 10 x the largest distances (tools/img_heads_tolerance.py --write -> tests/golden/img_heads_tolerance.json), the convention of
    tools/w8_tolerance.py;
  * `rerank_ref` / `rerank_emulate`: the same pair for the cosine of the rerank."""
import json
import os

import numpy as np
import torch

# (D, E, C, n): 17 blocks are past a 16-block tile; D = 4096 is the OPT-6.7b width; (1024, 64, 3) has three decisions and a short E
OP_CASES = ((768, 256, 2, 1), (768, 256, 2, 3), (768, 256, 2, 17), (4096, 256, 2, 2), (1024, 64, 3, 5))
# (n, g, E)
RERANK_CASES = ((1, 1, 256), (3, 2, 256), (5, 4, 64))
EXTRA_ROWS = 9          # hidden has more rows than are used
TOLERANCE_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "img_heads_tolerance.json")


def bf(a):
  """fp32 array -> the nearest bf16 values (round to nearest even), as fp32."""
  return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().float().numpy()


def case_seed(ci):
  return 300 + ci


def op_inputs(D, E, C, n, seed):
  """-> dict(hidden (rows, D) fp32, row_idx (n,) int32 scattered with a repeated row from n = 3 on, Wr (E, D) / Wd (C, D) fp32 holding bf16
  values, br (E), bd (C) fp32)."""
  rng = np.random.default_rng(seed)
  rows = n + EXTRA_ROWS
  hidden = rng.standard_normal((rows, D)).astype(np.float32)
  row_idx = np.array([(5 * i + 3) % rows for i in range(n)], dtype=np.int32)
  if n >= 3:
    row_idx[-1] = row_idx[0]
  Wr = bf(rng.standard_normal((E, D)).astype(np.float32) * np.float32(D ** -0.5))
  br = (rng.standard_normal(E) * 0.1).astype(np.float32)
  Wd = bf(rng.standard_normal((C, D)).astype(np.float32) * np.float32(0.05))
  bd = (rng.standard_normal(C) * 0.1).astype(np.float32)
  return dict(hidden=hidden, row_idx=row_idx, Wr=Wr, br=br, Wd=Wd, bd=bd)


def gather(hidden, row_idx):
  """The rows the kernel reads: indices clamped into [0, rows), values rounded to bf16."""
  r = np.clip(row_idx.astype(np.int64), 0, hidden.shape[0] - 1)
  return bf(hidden[r])


def _softmax(z):
  e = np.exp(z - z.max(axis=-1, keepdims=True))
  return e / e.sum(axis=-1, keepdims=True)


def heads_ref(inp, ret=True, decision=True):
  """fp64 on the same operands -> (ret_emb (n, E), probs (n, C), choice (n,), z (n, C)); None for an absent head."""
  x = gather(inp["hidden"], inp["row_idx"]).astype(np.float64)
  emb = probs = choice = z = None
  if ret:
    y = x @ inp["Wr"].astype(np.float64).T + inp["br"].astype(np.float64)
    nrm = np.sqrt((y * y).sum(axis=-1, keepdims=True))
    emb = np.where(nrm > 0, y / np.where(nrm > 0, nrm, 1.0), 0.0)
  if decision:
    z = x @ inp["Wd"].astype(np.float64).T + inp["bd"].astype(np.float64)
    probs = _softmax(z)
    choice = z.argmax(axis=-1).astype(np.int32)        # numpy's argmax returns the first of equal maxima: the lower index
  return emb, probs, choice, z


def _acc32(x, W, perm):
  """sum_k x[:, k] W[:, k] in fp32, one k at a time in the order perm (products of bf16 values are exact in fp32)."""
  acc = np.zeros((x.shape[0], W.shape[0]), dtype=np.float32)
  for k in perm:
    acc += x[:, k, None] * W[None, :, k]
  return acc


def heads_emulate(inp, seed):
  """The operator in fp32 with K in a permuted sequential order -> (ret_emb, probs), fp32."""
  x = gather(inp["hidden"], inp["row_idx"])
  perm = np.random.default_rng(seed + 7919).permutation(x.shape[1])
  y = _acc32(x, inp["Wr"], perm) + inp["br"]
  ss = np.zeros(y.shape[0], dtype=np.float32)
  for c in np.random.default_rng(seed + 104729).permutation(y.shape[1]):
    ss += y[:, c] * y[:, c]
  nrm = np.sqrt(ss).astype(np.float32)
  emb = np.where(ss[:, None] > 0, y / np.where(nrm > 0, nrm, np.float32(1))[:, None], np.float32(0)).astype(np.float32)
  z = _acc32(x, inp["Wd"], perm) + inp["bd"]
  # exp rounded to fp32 from the fp64 function: numpy's own fp32 exp differs by an ulp between CPUs, which a recorded distance must not see
  e = np.exp((z - z.max(axis=-1, keepdims=True)).astype(np.float32).astype(np.float64)).astype(np.float32)
  probs = (e / e.sum(axis=-1, keepdims=True, dtype=np.float32)).astype(np.float32)
  return emb, probs


def heads_distances(D, E, C, n, seed):
  """(largest element distance of ret_emb, largest probability distance of probs) between the fp32 emulation and fp64."""
  inp = op_inputs(D, E, C, n, seed)
  emb, probs, _, _ = heads_ref(inp)
  e32, p32 = heads_emulate(inp, seed)
  return float(np.abs(e32 - emb).max()), float(np.abs(p32 - probs).max())


def decision_margin(inp):
  """The smallest fp64 gap between the two largest decision logits over the blocks."""
  z = np.sort(heads_ref(inp)[3], axis=-1)
  return float((z[:, -1] - z[:, -2]).min())


def rerank_inputs(n, g, E, seed):
  """-> (visual (n g, E) fp32 un-normalised, ret_emb (n, E) fp32 unit rows)."""
  rng = np.random.default_rng(seed)
  visual = (rng.standard_normal((n * g, E)) * 3.0).astype(np.float32)
  r = rng.standard_normal((n, E))
  ret_emb = (r / np.linalg.norm(r, axis=-1, keepdims=True)).astype(np.float32)
  return visual, ret_emb


def rerank_ref(visual, ret_emb):
  """fp64 cosine -> (n, g); a zero row gives 0."""
  n = ret_emb.shape[0]
  g = visual.shape[0] // n
  v, r = visual.astype(np.float64).reshape(n, g, -1), ret_emb.astype(np.float64)[:, None, :]
  den = np.sqrt((v * v).sum(-1)) * np.sqrt((r * r).sum(-1))
  return np.where(den > 0, (v * r).sum(-1) / np.where(den > 0, den, 1.0), 0.0)


def rerank_emulate(visual, ret_emb, seed):
  n = ret_emb.shape[0]
  g = visual.shape[0] // n
  v, r = visual.reshape(n, g, -1), np.broadcast_to(ret_emb[:, None, :], (n, g, ret_emb.shape[1]))
  dot, vv, rr = (np.zeros((n, g), dtype=np.float32) for _ in range(3))
  for c in np.random.default_rng(seed + 7919).permutation(v.shape[-1]):
    dot += v[..., c] * r[..., c]
    vv += v[..., c] * v[..., c]
    rr += r[..., c] * r[..., c]
  return (dot / (np.sqrt(vv).astype(np.float32) * np.sqrt(rr).astype(np.float32))).astype(np.float32)


def rerank_distance(n, g, E, seed):
  visual, ret_emb = rerank_inputs(n, g, E, seed)
  return float(np.abs(rerank_emulate(visual, ret_emb, seed) - rerank_ref(visual, ret_emb)).max())


def measure():
  """The largest distances over the operator tests' shapes -> dict(ret_emb, probs, rerank)."""
  d_emb = d_p = d_r = 0.0
  for ci, (D, E, C, n) in enumerate(OP_CASES):
    a, b = heads_distances(D, E, C, n, case_seed(ci))
    d_emb, d_p = max(d_emb, a), max(d_p, b)
  for ci, (n, g, E) in enumerate(RERANK_CASES):
    d_r = max(d_r, rerank_distance(n, g, E, case_seed(ci)))
  return dict(ret_emb=d_emb, probs=d_p, rerank=d_r)


def load_bars():
  """The recorded bars: 10 x the measured distances -> dict(ret_emb, probs, rerank)."""
  with open(TOLERANCE_FILE) as f:
    return {k: float(v) for k, v in json.load(f)["bars"].items()}
