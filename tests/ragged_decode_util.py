"""Shared by test_ragged_decode_host.py and test_ragged_decode_gpu.py (not a test module): the ragged decode run in fp32.

A ragged run is B sequences of different lengths in one batch: a right-padded prefill of Tmax positions (pad positions hold a real token
and write keys / values at slots >= len[b], as the engine's prefill does), then S teacher-forced steps of one token per row, row b's
token of step s at position len[b] + s (gill_opt_decode_step with the lengths advanced by hand).

  * `ragged_inputs`: the teacher-forced rows, one sequence per row (kv_cache_util.token_embeds), the padded prompt block and the steps;
  * `oracle_rows`: THE REFERENCE: every row as its own sequence through oracle.opt_ref.opt_hidden_states; -> the prompt rows per row and
    the step rows (B, S, D);
  * `ragged_ref`: an fp32 restatement of the ragged run on kv_cache_util.cached_forward_ref (the prefill is that function's call on the
    padded block; the steps replay its layer arithmetic at per-row lengths), with a `defect=` switch that breaks it in the ways this path
    could be broken (DEFECTS), and `rnd=` for the bf16-operand emulation;
  * `compare_ragged` / `check_ragged`: kv_cache_util's per-call statistics and bars, one "call" per step over all rows and one per row's
    prompt."""
import torch
import torch.nn.functional as F

import kv_cache_util as U
from oracle import opt_ref

DEFECTS = ("length_of_row_zero",        # every row uses len[0]: slot, visible range and position
           "pad_key_visible",           # the prefill's pad slots len[b] + s + 1 .. Tmax - 1 are attended
           "newest_key_hidden",         # the step's own key is not attended
           "position_of_longest_row",   # every row takes the position of the longest row
           "append_one_early",          # the step's key / value land at slot len - 1, slot len is read as it was left
           "neighbour_head")            # head h reads the cache of head h + 1

# (lengths, steps): B = 3 with rows crossing the 32-slot edge at different steps and row 0 the 64-slot edge; B = 9 spread over 5 .. 31
RUNS = {"b3": ((30, 23, 9), 40), "b9": ((5, 31, 12, 26, 8, 19, 29, 15, 22), 40)}


_RIG = {}


def gill125_rig(cuda):
  """The GILL model of test_decode_sample_gpu.py (OPT-125m geometry, synthetic weights), built once for the ragged GPU test modules."""
  if "g" not in _RIG:
    from test_decode_sample_gpu import _gill_opt125m
    _RIG["g"] = _gill_opt125m(cuda)
  return _RIG["g"]


def ragged_inputs(sd, cfg, lengths, steps, seed):
  """-> seqs (B, max(lengths) + steps, D): row b's own sequence in its first lengths[b] + steps rows; prompt (B, Tmax, D): rows
  :lengths[b] of it, the pad positions filled with OTHER tokens (real, finite embeddings: what a pad id embeds to);
  step_x (B, steps, D): row b's tokens lengths[b] .. lengths[b] + steps - 1."""
  table = sd["model.decoder.embed_tokens.weight"]
  return tuple(F.embedding(t, table) for t in ragged_ids(cfg, lengths, steps, seed))


def ragged_ids(cfg, lengths, steps, seed):
  """The token ids behind ragged_inputs (kv_cache_util.token_embeds' ids): seq_ids, prompt_ids, step_ids."""
  from gill_amd import synth
  B, Tmax = len(lengths), max(lengths)
  ids = lambda T, sd_: synth.synthetic_prompt_ids(16, T, seed=sd_, vocab_lo=3, vocab_hi=cfg.vocab_size - 1)[:B, :T]   # noqa: E731
  seqs = ids(Tmax + steps, seed)
  prompt = ids(Tmax, seed + 500).clone()      # pad positions: other tokens than the row's continuation
  for b, n in enumerate(lengths):
    prompt[b, :n] = seqs[b, :n]
  step = torch.stack([seqs[b, n:n + steps] for b, n in enumerate(lengths)])
  return seqs, prompt, step


def oracle_rows(sd, cfg, seqs, lengths, steps):
  """Every row alone through the oracle -> ([prompt rows (lengths[b], D)], step rows (B, steps, D))."""
  pro, st = [], []
  for b, n in enumerate(lengths):
    h = opt_ref.opt_hidden_states(sd, cfg.num_layers, cfg.num_heads, seqs[b:b + 1, :n + steps])[0]
    pro.append(h[:n])
    st.append(h[n:n + steps])
  return pro, torch.stack(st)


def ragged_ref(sd, cfg, prompt, lengths, step_x, defect=None, rnd=None, cache=None):
  """The ragged run -> (prefill hidden (B, Tmax, D), step hidden (B, S, D), cache).  cache: kv_cache_util.new_cache() (or what an
  earlier sequence left in it), at least max(lengths) + S + 1 slots."""
  assert defect is None or defect in DEFECTS
  rnd = rnd or (lambda t: t)
  B, Tmax, D = prompt.shape
  S, H = step_x.shape[1], cfg.num_heads
  hd = D // H
  cache = cache if cache is not None else U.new_cache(cfg, B, max(lengths) + S + 1)
  (pre_h,), cache = U.cached_forward_ref(sd, cfg, prompt, (Tmax,), cache=cache, rnd=rnd)
  pre = "model.decoder."
  postab = sd[pre + "embed_positions.weight"].float()
  cap = cache[0][0].shape[2]
  outs = []
  for s in range(S):
    lens = [n + s for n in lengths]
    if defect == "length_of_row_zero":
      lens = [lens[0]] * B
    plen = [max(lens)] * B if defect == "position_of_longest_row" else lens
    h = step_x[:, s].float() + postab[2 + torch.tensor(plen)]
    for i in range(cfg.num_layers):
      p = f"{pre}layers.{i}."
      lin = lambda x, n: F.linear(rnd(x), sd[p + n + ".weight"].float(), sd[p + n + ".bias"].float())   # noqa: E731
      y = F.layer_norm(h, (D,), sd[p + "self_attn_layer_norm.weight"].float(), sd[p + "self_attn_layer_norm.bias"].float(), 1e-5)
      q = rnd(lin(y, "self_attn.q_proj")).view(B, H, hd) * hd ** -0.5      # the kernel scales the rounded q in fp32
      k, v = rnd(lin(y, "self_attn.k_proj")).view(B, H, hd), rnd(lin(y, "self_attn.v_proj")).view(B, H, hd)
      kc, vc = cache[i]
      a = torch.empty(B, H, hd)
      for b, n in enumerate(lens):
        slot = n - 1 if (defect == "append_one_early" and n > 0) else n
        kc[b, :, slot], vc[b, :, slot] = k[b], v[b]
        if defect == "append_one_early":
          kk, vv = kc[b, :, :n + 1], vc[b, :, :n + 1]            # slot n as it was left (a pad key, or zeros)
        else:
          kk, vv = torch.cat([kc[b, :, :n], k[b][:, None]], 1), torch.cat([vc[b, :, :n], v[b][:, None]], 1)   # the new key from the registers
        if defect == "pad_key_visible" and n + 1 < min(Tmax, cap):
          kk, vv = torch.cat([kk, kc[b, :, n + 1:Tmax]], 1), torch.cat([vv, vc[b, :, n + 1:Tmax]], 1)
        if defect == "newest_key_hidden" and n > 0:
          kk, vv = kk[:, :n], vv[:, :n]
        if defect == "neighbour_head":
          kk, vv = kk.roll(-1, 0), vv.roll(-1, 0)
        sc = (q[b][:, None] @ kk.transpose(1, 2))[:, 0]           # (H, keys)
        e = torch.exp(sc - sc.amax(-1, keepdim=True))
        a[b] = (e[:, None] @ vv)[:, 0] / e.sum(-1, keepdim=True)   # fp32 probabilities: the decode kernel does not round P
      h = h + lin(a.reshape(B, D), "self_attn.out_proj")
      y = F.layer_norm(h, (D,), sd[p + "final_layer_norm.weight"].float(), sd[p + "final_layer_norm.bias"].float(), 1e-5)
      h = h + lin(F.relu(lin(y, "fc1")), "fc2")
    outs.append(F.layer_norm(h, (D,), sd[pre + "final_layer_norm.weight"].float(), sd[pre + "final_layer_norm.bias"].float(), 1e-5))
  return pre_h, torch.stack(outs, 1), cache


def compare_ragged(tag, pre_h, step_h, oracle_prompt, oracle_steps, lengths):
  """kv_cache_util.compare_calls statistics: one call per row's prompt rows (only the first lengths[b] rows of the prefill mean
  anything), then one call per step over all rows.  -> [(rel, cos, min row cos)], prompts first."""
  stats = []
  for b, n in enumerate(lengths):
    stats += U.compare_calls(f"{tag} prompt of row {b}", [pre_h[b:b + 1, :n]], oracle_prompt[b][None], [(0, n)])
  S = oracle_steps.shape[1]
  stats += U.compare_calls(f"{tag} step", [step_h[:, s:s + 1] for s in range(S)], oracle_steps, [(s, 1) for s in range(S)])
  return stats


def check_ragged(tag, pre_h, step_h, oracle_prompt, oracle_steps, lengths, rel_bar=U.REL_BAR, cos_bar=U.COS_BAR):
  stats = compare_ragged(tag, pre_h, step_h, oracle_prompt, oracle_steps, lengths)
  U.assert_calls(stats, rel_bar, cos_bar)
  return stats


# ------------------------------------------------------------------------------------------------ the end-to-end case of test_generate_batch_gpu.py
# Greedy, B = 6 at ragged lengths on the rig of test_decode_sample_gpu.py (OPT-125m geometry, synth.opt_state_dict seed 5), min_word_tokens = 3
# and gen_scale_factor = 1e5: three free decisions per row, then [IMG0] is certain.  Free-running tokens of two arithmetic paths (the ragged
# batch, the one-sequence loop) can part at a near tie; the bar m for "near" is 10 x the largest logit distance between the bf16-operand
# emulation and the fp32 oracle on these very prompts (tools/ragged_decode_tolerance.py --write -> tests/golden/ragged_decode_tolerance.json),
# and GEN_SEED is chosen (by that tool) so that the ORACLE's own greedy run has no decision with a top-2 margin under m.
GEN_LENGTHS = (9, 6, 12, 5, 11, 8)
GEN_SEED = 46
GEN_MWT = 3
GEN_TOLERANCE_FILE = "ragged_decode_tolerance.json"       # under tests/golden


def gen_model():
  from gill_amd import synth
  cfg = synth.OptConfig(vocab_size=50274, hidden_size=768, num_layers=12, num_heads=12, ffn_dim=3072)
  return cfg, {k: U.bf(v) for k, v in synth.opt_state_dict(cfg, seed=5).items()}


def gen_prompt_ids(seed=GEN_SEED, pad=1):
  """(ids (6, 12) right-padded with `pad`, lengths)."""
  from gill_amd import synth
  T = max(GEN_LENGTHS)
  ids = synth.synthetic_prompt_ids(len(GEN_LENGTHS), T, seed=seed)[:, :T].clone()
  for b, n in enumerate(GEN_LENGTHS):
    ids[b, n:] = pad
  return ids, list(GEN_LENGTHS)


def load_gen_tolerance():
  import json
  import os
  with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GEN_TOLERANCE_FILE)) as f:
    return float(json.load(f)["m"])


def oracle_greedy(sd, cfg, row_ids, n_dec=GEN_MWT):
  """The fp32 oracle's own greedy run of one row for n_dec decisions, all under min_word_tokens (the [IMG] ids filtered).  -> (tokens,
  top-2 margins, the sequence's ids, the bf16-emulation's largest logit distance from the oracle over the decision rows)."""
  from gill_amd import synth
  ids = [int(v) for v in row_ids]
  toks, margins, dist = [], [], 0.0
  table = sd["model.decoder.embed_tokens.weight"].float()
  for _ in range(n_dec):
    x = F.embedding(torch.tensor(ids)[None], table)
    h = opt_ref.opt_hidden_states(sd, cfg.num_layers, cfg.num_heads, x)[0, -1]
    logits = opt_ref.opt_logits(sd, h[None])[0]
    (he,), _ = U.cached_forward_ref(sd, cfg, x, (len(ids),), rnd=U.bf)
    dist = max(dist, (opt_ref.opt_logits(sd, U.bf(he[0, -1])[None])[0] - logits).abs().max().item())
    logits[synth.IMG_TOKEN_IDS] = float("-inf")
    top = logits.topk(2)
    toks.append(int(top.indices[0]))
    margins.append(float(top.values[0] - top.values[1]))
    ids.append(toks[-1])
  return toks, margins, ids, dist
