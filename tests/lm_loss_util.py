"""Shared by test_lm_loss_host.py, test_lm_loss_gpu.py and tools/lm_loss_tolerance.py (not a test module).

  * `build_inputs`: bf16-valued operands of the fused LM-head loss operator whose true ranks cover 0, 1-4, 5-50 and the thousands, with a fixed
    share of ignored rows and targets on the kernel's edges (column 0, column V - 1, first / last column of a slab and of a column tile);
  * `reference`: the operator restated in fp64 (logits, lse, tgt, rank, summary), with a `defect=` switch that breaks it in one of the ways the
    kernel could be broken (DEFECTS);
  * `fp32_permuted`: the same in fp32 with the K chunks accumulated in a permuted order and the slabs merged like the kernel merges them: a CPU
    emulation of the kernel's arithmetic, not the kernel;
  * `operator_ratio` / `assert_operator`: the one check both test files apply (bars below, rank window, top-1 / top-5, summary);
  * the reference's forward restated for the engine tests: its label loops as plain loops, oracle.opt_ref for the LM, F.cross_entropy for the loss;
  * the bars.  profiles/lm_loss.md (written by tools/lm_loss_tolerance.py) holds the distances they rest on and the reasoning for the margins.
"""
import math

import torch
import torch.nn.functional as F

DEFECTS = ("tail_columns_counted", "merge_without_rescale", "target_off_by_one", "ignore_index_scored", "self_counted", "last_slab_dropped")

# ---- bars (profiles/lm_loss.md) ----------------------------------------------------------------------------------------------------
# term (a): a logit is a K-term bf16 dot product accumulated in fp32.  The permuted-order fp32 emulation sits at most 2.3e-6 from fp64 on
# these inputs (D = 4096; 2.0e-6 at D = 768); the bar is 8x that, rounded up: x2 for an adder that truncates (1 ulp per add where the
# emulation has 1/2), x2 for the 32-term sums inside one matrix instruction, whose order the emulation does not model, x2 because the
# emulation's maximum is over one draw.  (The fp32-output GEMMs of this library, on the same instruction, were recorded at 3e-7 .. 7e-7 of the
# largest output at K = 4096, profiles/r06_gpu_tests_with_stats.log: 8e-6 on logits of at most 11.5.)  lse is 1-Lipschitz in the logits (sup
# norm), so it inherits the logit bar, plus 4e-6 for the fast exponential (v_exp_f32 on (v - m) log2 e: the argument's rounding at
# |v - m| <= 16 is 1.4e-6 relative on a term, the instruction itself 1 ulp), the fp32 sums and logf.
LOGIT_BAR = 2e-5
TGT_BAR = LOGIT_BAR
LSE_BAR = LOGIT_BAR + 4e-6
# summary[0] is a mean of lse - tgt: no more than their two bars, plus the fp32 mean itself (1e-6 relative on a loss of ~10)
MEAN_BAR = LSE_BAR + TGT_BAR + 1e-5
# term (b): the engine against the fp32 oracle.  A bf16-operand emulation of the 2-layer OPT pass (every GEMM operand rounded, the final
# hidden rows rounded before the head) moves a token's loss by at most 2.9e-2 and the batch loss by 1.8e-3 (B = 1 and 3, T = 24, losses of
# ~13.5); the bars are 4x those: the emulation is to stay within half a bar (the discipline of test_kv_cache_host.py), and the engine also
# accumulates in another order and forms its LayerNorm statistics from fused partial sums.
TOKEN_LOSS_BAR = 1.2e-1
LOSS_BAR = 7e-3
LAST_LOGIT_BAR = 1.8e-1       # a whole logits row (last_output_logit): the emulation's largest logit distance is 4.3e-2; 4x, as above

IGNORE_EVERY = 4          # rows r with r % 4 == 3 are ignored: a fixed quarter
ALPHAS = (8.0, 4.3, 3.7, 1.0, 8.0, 4.0, 3.2, 0.0)      # graded over the rows: target logit ~ alpha + N(0, 1) among V logits ~ N(0, 1)


def bf(x):
  return x.bfloat16().float()


def edge_columns(V, geom):
  """Columns on which the kernel's partition has an edge: 0, V - 1, the first / last column of a slab and of a column tile."""
  _, col_tile, _, cps = geom
  cols = [0, V - 1, cps - 1, cps, 2 * cps - 1, 2 * cps, col_tile - 1, col_tile, (V - 1) // cps * cps, (V - 1) // col_tile * col_tile]
  out = []
  for c in cols:
    if 0 <= c < V and c not in out:
      out.append(c)
  return out


def build_inputs(M, V, D, seed, geom):
  """x (M, D), w (V, D) bf16-valued fp32, target (M) int64.  Row r: x = noise + alpha_r W[target_r]; rows r % 4 == 3 are ignored; the first
  valid rows take their targets from edge_columns, the others are drawn."""
  g = torch.Generator().manual_seed(seed)
  w = bf(torch.randn((V, D), generator=g) / math.sqrt(D))
  target = torch.randint(0, V, (M,), generator=g)
  edges = edge_columns(V, geom)
  valid_rows = [r for r in range(M) if r % IGNORE_EVERY != IGNORE_EVERY - 1]
  for i, r in enumerate(valid_rows[:len(edges)]):
    target[r] = edges[i]
  alpha = torch.tensor([ALPHAS[(r // 2) % len(ALPHAS)] for r in range(M)])
  x = bf(torch.randn((M, D), generator=g) + alpha[:, None] * w[target])
  target = target.clone()
  for r in range(M):
    if r % IGNORE_EVERY == IGNORE_EVERY - 1:
      target[r] = -100
  return x, w, target


def _rank(logits, tcol):
  """#{c != t : L[c] > L[t] or (L[c] == L[t] and c < t)} per row."""
  lt = logits.gather(1, tcol[:, None])
  idx = torch.arange(logits.shape[1])[None, :]
  return ((logits > lt) | ((logits == lt) & (idx < tcol[:, None]))).sum(1)


def _summary(lse, tgt, rank):
  valid = rank >= 0
  n = int(valid.sum())
  mean = float((lse - tgt)[valid].sum() / n) if n else float("nan")
  return [mean, float(n), float((valid & (rank < 1)).sum()), float((valid & (rank < 5)).sum())]


def reference(x, w, target, geom, defect=None):
  """fp64.  Returns dict(logits (M,V), lse, tgt (fp64), rank (int64), summary [4])."""
  assert defect is None or defect in DEFECTS
  M, V = x.shape[0], w.shape[0]
  _, col_tile, _, cps = geom
  L = x.double() @ w.double().T
  tg = target.clone()
  if defect == "target_off_by_one":
    tg = torch.roll(target, 1)
  valid = tg != -100
  if defect == "ignore_index_scored":
    valid = torch.ones_like(valid)
  tcol = tg.clamp(0, V - 1)
  Ls = L
  if defect == "tail_columns_counted":
    pad = (V + col_tile - 1) // col_tile * col_tile - V
    Ls = torch.cat([L, torch.zeros((M, pad), dtype=L.dtype)], 1)
  if defect == "last_slab_dropped" and V > cps:
    Ls = L[:, :(V - 1) // cps * cps]
  if defect == "merge_without_rescale":
    parts = Ls.split(cps, dim=1)
    ms = torch.stack([p.amax(1) for p in parts], 1)
    ss = torch.stack([torch.exp(p - p.amax(1, keepdim=True)).sum(1) for p in parts], 1)
    lse = ms.amax(1) + torch.log(ss.sum(1))
  else:
    lse = torch.logsumexp(Ls, 1)
  tgt = L.gather(1, tcol[:, None])[:, 0]
  lt = tgt[:, None]
  idx = torch.arange(Ls.shape[1])[None, :]
  before = (Ls > lt) | ((Ls == lt) & (idx < tcol[:, None]))
  if defect == "self_counted":
    before = before | (idx == tcol[:, None])
  else:
    before = before & (idx != tcol[:, None])
  rank = before.sum(1)
  lse = torch.where(valid, lse, torch.zeros_like(lse))
  tgt = torch.where(valid, tgt, torch.zeros_like(tgt))
  rank = torch.where(valid, rank, torch.full_like(rank, -1))
  return dict(logits=L, lse=lse, tgt=tgt, rank=rank, summary=_summary(lse, tgt, rank))


def fp32_permuted(x, w, target, geom, seed=0):
  """The kernel's arithmetic emulated on the CPU: fp32 accumulation over 32-wide K chunks taken in a permuted order, per-slab (max, sum of
  exp) merged in ascending order in fp32.  Same dict as reference() (fp32 values)."""
  M, D = x.shape
  V = w.shape[0]
  _, _, _, cps = geom
  perm = torch.randperm(D // 32, generator=torch.Generator().manual_seed(seed)).tolist()
  L = torch.zeros((M, V), dtype=torch.float32)
  for c in perm:
    L = L + x[:, 32 * c:32 * c + 32].float() @ w[:, 32 * c:32 * c + 32].float().T
  valid = target != -100
  tcol = target.clamp(0, V - 1)
  parts = L.split(cps, dim=1)
  ms = torch.stack([p.amax(1) for p in parts], 1)
  ss = torch.stack([torch.exp(p - p.amax(1, keepdim=True)).sum(1) for p in parts], 1)
  m = ms.amax(1)
  s = torch.zeros_like(m)
  for k in range(ms.shape[1]):
    s = s + ss[:, k] * torch.exp(ms[:, k] - m)
  lse = m + torch.log(s)
  tgt = L.gather(1, tcol[:, None])[:, 0]
  rank = _rank(L, tcol)
  lse = torch.where(valid, lse, torch.zeros_like(lse))
  tgt = torch.where(valid, tgt, torch.zeros_like(tgt))
  rank = torch.where(valid, rank, torch.full_like(rank, -1))
  return dict(logits=L, lse=lse, tgt=tgt, rank=rank, summary=_summary(lse.double(), tgt.double(), rank))


def rank_window(ref, target, tau=LOGIT_BAR):
  """(lo, hi) per row from the fp64 logits: #{c : L[c] > L[t] + 2 tau} <= rank <= #{c != t : L[c] >= L[t] - 2 tau}; (-1, -1) where ignored."""
  L = ref["logits"]
  V = L.shape[1]
  valid = target != -100
  tcol = target.clamp(0, V - 1)
  lt = L.gather(1, tcol[:, None])
  idx = torch.arange(V)[None, :]
  lo = (L > lt + 2 * tau).sum(1)
  hi = ((L >= lt - 2 * tau) & (idx != tcol[:, None])).sum(1)
  neg = torch.full_like(lo, -1)
  return torch.where(valid, lo, neg), torch.where(valid, hi, neg)


def ambiguous_rows(ref, target, tau=LOGIT_BAR):
  """Rows whose top-1 / top-5 verdict the window leaves open: lo < k <= hi for k in {1, 5}."""
  lo, hi = rank_window(ref, target, tau)
  bad = torch.zeros_like(lo, dtype=torch.bool)
  for k in (1, 5):
    bad |= (lo < k) & (k <= hi)
  return bad.nonzero()[:, 0].tolist()


def operator_ratio(tag, got, ref, target):
  """How far `got` (dict of lse, tgt, rank, summary: the kernel's outputs, or a stand-in) is from `ref` = reference(...), as a ratio to the bars:
  <= 1 passes.  A discrete failure (rank outside its window, a top-1 / top-5 verdict or a summary count that differs, an ignored row not -1) is
  an infinite ratio.  Prints every figure."""
  valid = target != -100
  lse, tgt, rank = (torch.as_tensor(got[k]).cpu() for k in ("lse", "tgt", "rank"))
  summ = [float(v) for v in torch.as_tensor(got["summary"]).cpu().tolist()]
  e_lse = float((lse.double() - ref["lse"]).abs().max())
  e_tgt = float((tgt.double() - ref["tgt"]).abs().max())
  lo, hi = rank_window(ref, target)
  rank = rank.long()
  n_out = int(((rank < lo) | (rank > hi)).sum())
  n_top = sum(int((((rank < k) & valid) != ((ref["rank"] < k) & valid)).sum()) for k in (1, 5))
  want = ref["summary"]
  counts_ok = summ[1:] == want[1:]
  if math.isnan(want[0]):
    e_mean = 0.0 if math.isnan(summ[0]) else float("inf")
  else:
    e_mean = abs(summ[0] - want[0]) if math.isfinite(summ[0]) else float("inf")
  ratio = max(e_lse / LSE_BAR, e_tgt / TGT_BAR, e_mean / MEAN_BAR)
  if not math.isfinite(ratio) or n_out or n_top or not counts_ok:
    ratio = float("inf")
  print(f"[{tag}] |lse - ref| {e_lse:.3e} (bar {LSE_BAR:.1e})  |tgt - ref| {e_tgt:.3e} (bar {TGT_BAR:.1e})  |mean - ref| {e_mean:.3e} (bar {MEAN_BAR:.1e})  "
        f"ranks outside window {n_out}  top-1/5 verdicts off {n_top}  summary {summ} want {want}  -> ratio {ratio:.3g}")
  return ratio


def assert_operator(tag, got, ref, target):
  ratio = operator_ratio(tag, got, ref, target)
  assert ratio <= 1.0, f"{tag}: misses the operator bars by {ratio:.3g}x"
  return ratio


# ---- the reference's forward, restated for the engine tests --------------------------------------------------------------------------
def label_loops(labels, mode, n_front, pad_id, ret_ids, gen_ids):
  """full_labels the way the reference builds them, row by row and token by token: n_front columns of -100 in front, then in captioning
  mode everything from the first pad / retrieval / generation token on becomes -100; in the other two modes everything from the first pad
  on, and then everything from the first pad or non-leading retrieval / generation token on."""
  rows = []
  for row in labels.tolist():
    full = [-100] * n_front + list(row)
    if mode == "captioning":
      stops = [pad_id] + list(ret_ids) + list(gen_ids)
      for k, tok in enumerate(full):
        if tok in stops:
          for j in range(k, len(full)):
            full[j] = -100
          break
    else:
      for k, tok in enumerate(full):
        if tok == pad_id:
          for j in range(k, len(full)):
            full[j] = -100
          break
      later = list(ret_ids[1:]) + list(gen_ids[1:])
      for k, tok in enumerate(full):
        if tok == pad_id or tok in later:
          for j in range(k, len(full)):
            full[j] = -100
          break
    rows.append(full)
  return torch.tensor(rows, dtype=torch.int64)


def lm_scores(sd, num_layers, num_heads, inputs_embeds, full_labels, hidden_fn=None):
  """The LM call of the reference on the fp32 oracle: hidden_states[-1], logits, HF's shifted mean cross-entropy, and per token the loss and
  the rank of the label.  hidden_fn replaces oracle.opt_ref.opt_hidden_states (the bf16 emulation of the tolerance tool)."""
  from oracle import opt_ref
  hidden = (hidden_fn or (lambda e: opt_ref.opt_hidden_states(sd, num_layers, num_heads, e)))(inputs_embeds)
  logits = opt_ref.opt_logits(sd, hidden)
  B, T, V = logits.shape
  shift_logits, shift_labels = logits[:, :-1].reshape(-1, V), full_labels[:, 1:].reshape(-1)
  loss = F.cross_entropy(shift_logits, shift_labels, ignore_index=-100)
  token_loss = F.cross_entropy(shift_logits, shift_labels, ignore_index=-100, reduction="none").reshape(B, T - 1)
  valid = shift_labels != -100
  rank = _rank(shift_logits.double(), shift_labels.clamp(0, V - 1))
  rank = torch.where(valid, rank, torch.full_like(rank, -1)).reshape(B, T - 1)
  return dict(hidden=hidden, logits=logits, loss=loss, token_loss=token_loss, token_rank=rank)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def operator_shapes(geom_of):
  """(M, V, D) of the operator tests.  geom_of(M, V, D) -> (row_tile, col_tile, n_slabs, cols_per_slab) is gill_lm_loss_geometry: the shapes
  aim at the kernel's real edges — one row, a ragged tile, one row past a tile; a vocabulary inside one column tile, one column past three
  tiles, three columns past two slabs — at a short and a long K, then the real slab partition of GILL's vocabulary and a long-K case."""
  row_tile, col_tile, _, cps = geom_of(1, 50274, 768)
  shapes = [(M, V, D) for D in (128, 768) for V in (50, 3 * col_tile + 1, 2 * cps + 3) for M in (1, 17, row_tile + 1)]
  return shapes + [(40, 50274, 768), (33, 2050, 4096)]


OP_SEED = 5      # every shape's inputs are free of threshold-ambiguous rows at this seed (asserted on the CPU before a test touches the GPU)


def lm_head(cfg, seed):
  """An untied head with logits of a trained LM's range (std ~2): synth's embedding table (std 0.5: logits of std ~14, losses above 100) would
  put every token loss where one column carries the whole softmax."""
  from gill_amd import synth
  return bf(synth.normal("lm_head.weight", (cfg.vocab_size, cfg.hidden_size), seed, 2.0 / math.sqrt(cfg.hidden_size)))


def engine_case(B, T=24, seed=81):
  """opt-125m geometry with 2 layers and GILL's vocabulary; B padded sequences of T positions: a prompt, the 8 [IMG] tokens, then 3 b pads in
  row b; an untied lm_head (lm_head()).  Returns (cfg, sd (bf16-valued), ids (B,T), full_labels (B,T) of the generation regime, last_idx (B,))."""
  from gill_amd import synth
  cfg = synth.OptConfig(vocab_size=50274, hidden_size=768, num_layers=2, num_heads=12, ffn_dim=3072)
  sd = {k: bf(v) for k, v in synth.opt_state_dict(cfg, seed=seed).items()}
  sd["lm_head.weight"] = lm_head(cfg, seed)
  tok = synth.HashTokenizer()
  prompt = synth.synthetic_prompt_ids(B, T - 8, seed=seed)[:, :T - 8]
  rows, last = [], []
  for b in range(B):
    n = T - 8 - 3 * b
    rows.append(prompt[b, :n].tolist() + list(synth.IMG_TOKEN_IDS) + [tok.pad_token_id] * (3 * b))
    last.append(n + 8 - 1)
  ids = torch.tensor(rows, dtype=torch.int64)
  full = label_loops(ids, "generation", 0, tok.pad_token_id, synth.IMG_TOKEN_IDS, synth.IMG_TOKEN_IDS)
  return cfg, sd, ids, full, torch.tensor(last)
