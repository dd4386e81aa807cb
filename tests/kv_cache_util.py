"""Shared by test_kv_cache_gpu.py, test_kv_cache_host.py and the decode-offset attention tests of test_ops_gpu.py (not a test module).

  * the two OPT geometries, the call schedules and the teacher-forced inputs of the KV-cache tests;
  * `cached_forward_ref`: an fp32 restatement of what gill_opt_forward_cached computes call by call (keys / values appended to a
    cache at `past`, the new rows attending to cache[:past + T_new] under the offset causal mask, positions 2 + past + t), with a
    `defect=` switch that breaks it in one of the ways the real path could be broken;
  * `compare_calls` / `assert_calls`: the per-call comparison with the fp32 oracle both test files use (the stat helper and the bars
    of test_opt_6_7b_geometry_img_hidden_vs_oracle, plus the minimum per-row cosine);
  * the operator-level twins: inputs, per-row error and defects for ops.attention(causal=True) at nq < nkv.

Weights.  With synth's plain weights OPT attention is nearly uniform (logit std ~ 1), so one key more or less among 60 moves a
hidden row by a fraction of the bars and a broken cache passes.  `peaked_opt_state_dict` therefore scales q_proj by QK_GAIN (a
peaked softmax: logit std ~ QK_GAIN) and mixes SELF_MIX of q_proj into k_proj (a token's own key, the newest one of its step,
carries real weight, as it does in a trained LM).  test_kv_cache_host.py checks on the CPU that with these weights every defect
misses a bar by 3x or more (measured: 49x .. 500x) while a bf16 emulation of the kernel arithmetic stays within half of each bar
(measured: 0.18 of a bar at 12 layers); the hidden rows keep an rms of ~1."""
import math

import torch
import torch.nn.functional as F

from gill_amd import synth

DEFECTS = ("newest_key_hidden", "causal_off_by_one", "positions_not_advanced", "stale_key_visible", "batch_row_zero",
           "v_written_one_early")
ATTN_DEFECTS = tuple(d for d in DEFECTS if d != "positions_not_advanced")     # the position table is not attention's business

REL_BAR, COS_BAR = 3e-2, 0.999        # test_opt_6_7b_geometry_img_hidden_vs_oracle
CACHED_VS_FULL_REL_BAR = 2e-2         # test_generate_kv_cache_matches_full_reforward

QK_GAIN, SELF_MIX = 2.0, 0.1

GEOMETRIES = {
  # OPT-6.7b geometry (BASELINE configs[1]): D = 4096, 32 heads x 128, FFN 16384.  prefill 30, single tokens to 33, one 8-token
  # [IMG] block (-> 41), single tokens across the 64-key tile edge to 66
  "opt67": dict(cfg=synth.OptConfig(vocab_size=512, hidden_size=4096, num_layers=2, num_heads=32, ffn_dim=16384, max_positions=512),
                seed=71, schedule=(30, 1, 1, 1, 8) + (1,) * 25, batches=(1, 4)),
  # OPT-125m at full depth: 12 layers, 12 heads x 64.  204 tokens of context: nq = 1 walks four 64-key tiles; two 8-token blocks,
  # the second one straddling the 128-key edge (126 -> 134)
  "opt125": dict(cfg=synth.OptConfig(vocab_size=512, hidden_size=768, num_layers=12, num_heads=12, ffn_dim=3072, max_positions=512),
                 seed=72, schedule=(30,) + (1,) * 20 + (8,) + (1,) * 68 + (8,) + (1,) * 70, batches=(2, 9)),
}


def bf(x):
  return x.bfloat16().float()


def peaked_opt_state_dict(cfg, seed):
  """synth.opt_state_dict with a peaked, self-favouring attention (module docstring); bf16-rounded."""
  sd = synth.opt_state_dict(cfg, seed=seed)
  for i in range(cfg.num_layers):
    p = f"model.decoder.layers.{i}.self_attn."
    wq, bq = sd[p + "q_proj.weight"], sd[p + "q_proj.bias"]
    sd[p + "k_proj.weight"] = sd[p + "k_proj.weight"] + SELF_MIX * wq
    sd[p + "q_proj.weight"], sd[p + "q_proj.bias"] = wq * QK_GAIN, bq * QK_GAIN
  return {k: bf(v) for k, v in sd.items()}


def token_embeds(sd, cfg, B, T, seed):
  """Teacher-forced inputs: fixed synthetic ids (B, T) -> their embedding rows (exact in bf16, the table is bf16-rounded).  The rows
  of a smaller batch are the first rows of a larger one with the same seed."""
  ids = synth.synthetic_prompt_ids(16, T, seed=seed, vocab_lo=3, vocab_hi=cfg.vocab_size - 1)[:B, :T]
  return F.embedding(ids, sd["model.decoder.embed_tokens.weight"])


def calls_of(schedule, start=0):
  """[(past_len, T_new)] of a schedule of T_new values."""
  out, past = [], start
  for tn in schedule:
    out.append((past, tn))
    past += tn
  return out


# ------------------------------------------------------------------------------------------------ the cached algorithm, in fp32
def new_cache(cfg, max_batch, cap):
  hd = cfg.hidden_size // cfg.num_heads
  return [(torch.zeros(max_batch, cfg.num_heads, cap, hd), torch.zeros(max_batch, cfg.num_heads, cap, hd)) for _ in range(cfg.num_layers)]


def _attend_call(q, kc, vc, B, past, tn, defect, rnd):
  """q (B,H,tn,d) pre-scaled; kc / vc the layer's whole cache (maxB,H,cap,d), already holding this call's rows."""
  nkv, cap = past + tn, kc.shape[2]
  nvis = min(nkv + 1, cap) if defect == "stale_key_visible" else nkv
  k, v = kc[:B, :, :nvis], vc[:B, :, :nvis]
  if defect == "batch_row_zero":
    k, v = k[:1].expand(B, -1, -1, -1), v[:1].expand(B, -1, -1, -1)
  kv = torch.arange(nvis)[None, :]
  qidx = torch.arange(tn)[:, None] + past
  off = 1 if (defect == "causal_off_by_one" and tn > 1) else 0
  vis = (kv <= qidx + off) & (kv < nkv)
  if defect == "newest_key_hidden":
    vis = vis & (kv < nkv - 1)
  if defect == "stale_key_visible":
    vis = vis | (kv == nkv)
  s = (q @ k.transpose(-1, -2)).masked_fill(~vis, float("-inf"))
  e = torch.exp(s - s.amax(-1, keepdim=True))
  return (rnd(e) @ v) / e.sum(-1, keepdim=True)           # the kernel rounds the unnormalised P for the PV MFMAs


def cached_forward_ref(sd, cfg, embeds, schedule, defect=None, cache=None, rnd=None):
  """Replays the calls of `schedule` (past_len restarts at 0) on embeds (B, sum(schedule), D) and returns ([per-call hidden rows
  (B, T_new, D)], cache).  `cache` (new_cache(), or the one an earlier sequence left behind: its rows stay where they are, as in a
  re-used handle) is written at [past, past + T_new) and read at [0, past + T_new) by every call, per layer.  Everything but
  attention is row-wise, so inside a layer the linear parts run once over all rows and the calls are replayed for the attention;
  the values are those of a call-by-call run.  rnd: rounding applied to every GEMM operand (bf16 emulation), default none.
  defect: one of DEFECTS."""
  assert defect is None or defect in DEFECTS
  rnd = rnd or (lambda t: t)
  B, T, D = embeds.shape
  H = cfg.num_heads
  hd = D // H
  calls = calls_of(schedule)
  assert T == sum(schedule)
  cache = cache if cache is not None else new_cache(cfg, B, T + 1)
  pre = "model.decoder."
  postab = sd[pre + "embed_positions.weight"].float()
  tpos = torch.cat([torch.arange(tn) + (0 if defect == "positions_not_advanced" else past) for past, tn in calls])
  h = embeds.float() + postab[2 + tpos][None]
  heads = lambda t: t.view(B, T, H, hd).transpose(1, 2)     # noqa: E731
  for i in range(cfg.num_layers):
    p = f"{pre}layers.{i}."
    lin = lambda x, n: F.linear(rnd(x), sd[p + n + ".weight"].float(), sd[p + n + ".bias"].float())   # noqa: E731
    y = F.layer_norm(h, (D,), sd[p + "self_attn_layer_norm.weight"].float(), sd[p + "self_attn_layer_norm.bias"].float(), 1e-5)
    q = heads(rnd(lin(y, "self_attn.q_proj") * hd ** -0.5))
    k, v = heads(rnd(lin(y, "self_attn.k_proj"))), heads(rnd(lin(y, "self_attn.v_proj")))
    kc, vc = cache[i]
    a = torch.empty(B, H, T, hd)
    row = 0
    for past, tn in calls:
      kc[:B, :, past:past + tn] = k[:, :, row:row + tn]
      vpast = past - 1 if (defect == "v_written_one_early" and tn == 8 and past > 0) else past
      vc[:B, :, vpast:vpast + tn] = v[:, :, row:row + tn]
      a[:, :, row:row + tn] = _attend_call(q[:, :, row:row + tn], kc, vc, B, past, tn, defect, rnd)
      row += tn
    h = h + lin(a.transpose(1, 2).reshape(B, T, D), "self_attn.out_proj")
    y = F.layer_norm(h, (D,), sd[p + "final_layer_norm.weight"].float(), sd[p + "final_layer_norm.bias"].float(), 1e-5)
    h = h + lin(F.relu(lin(y, "fc1")), "fc2")
  h = F.layer_norm(h, (D,), sd[pre + "final_layer_norm.weight"].float(), sd[pre + "final_layer_norm.bias"].float(), 1e-5)
  return list(h.split(list(schedule), dim=1)), cache


# ------------------------------------------------------------------------------------------------ the engine-level comparison
def compare_calls(tag, outs, ref, calls):
  """outs[c] (B, T_new, D) of call c = (past, T_new) against ref[:, past : past + T_new] (one full causal pass of the oracle).  One
  line and one (rel, cos, min per-row cos) per call."""
  from test_stages_gpu import _stats
  res = []
  for c, ((past, tn), got) in enumerate(zip(calls, outs)):
    got, want = got.float().cpu(), ref[:, past:past + tn].float()
    assert got.shape == want.shape, (got.shape, want.shape)
    _, rel, cos = _stats(f"{tag} call {c} past={past} T_new={tn}", got, want)
    rows = F.cosine_similarity(got, want, dim=-1)
    b, t = divmod(int(rows.argmin()), tn)
    mrc = rows.min().item()
    if not math.isfinite(rel + cos + mrc):
      rel, cos, mrc = float("inf"), -1.0, -1.0
    print(f"[{tag} call {c}] min row cos={mrc:.6f} (batch row {b}, position {past + t})")
    res.append((rel, cos, mrc))
  return res


def worst_ratio(stats, rel_bar=REL_BAR, cos_bar=COS_BAR):
  """How far the worst call is from the bars: max over calls of rel / bar and (1 - cos) / (1 - bar), whole call and worst row.
  <= 1 passes; a bar "missed by a factor of 3" is a ratio >= 3."""
  return max(max(rel / rel_bar, (1 - cos) / (1 - cos_bar), (1 - mrc) / (1 - cos_bar)) for rel, cos, mrc in stats)


def assert_calls(stats, rel_bar=REL_BAR, cos_bar=COS_BAR):
  for c, (rel, cos, mrc) in enumerate(stats):
    assert rel < rel_bar and cos > cos_bar and mrc > cos_bar, f"call {c}: rel_l2 {rel:.3e} cos {cos:.6f} min row cos {mrc:.6f}"


def check_calls(tag, outs, ref, calls, rel_bar=REL_BAR, cos_bar=COS_BAR):
  """The engine-level check: compare, print, assert; returns the per-call statistics."""
  stats = compare_calls(tag, outs, ref, calls)
  assert_calls(stats, rel_bar, cos_bar)
  return stats


# ------------------------------------------------------------------------------------------------ operator level
ATTN_BAR = 2e-2     # test_attention

# (B, H, nq, nkv, d): ops.attention(causal=True) as a decode step sees it, nq new rows against nkv = past + nq keys
DECODE_SHAPES = (
  [(1, 32, 1, n, 128) for n in (1, 32, 33, 64, 65, 128, 129, 257)] +         # B H = 32: whole rounds of the 8-XCD map
  [(3, 12, 1, n, 64) for n in (1, 32, 33, 64, 65, 128, 129, 257)] +          # B H = 36: a ragged last round
  [(2, 32, 8, n, 128) for n in (64, 65, 71, 72)] +                           # a forced [IMG] block ending before / on / after a tile edge
  [(1, 12, 8, n, 64) for n in (64, 65, 71, 72)] +                            # B H = 12
  [(1, 32, 33, 97, 128), (3, 12, 33, 64, 64),                                # two waves
   (1, 32, 130, 300, 128), (2, 12, 130, 300, 64), (1, 12, 130, 130 + 64, 64)])  # two query tiles with different key-tile bounds


def decode_attn_inputs(B, H, nq, nkv, d, seed):
  """bf16-valued q (B,nq,H*d), k / v (B,nkv,H*d).  Scores have a std of ~3 (a peaked softmax), and every key of the step also leans
  towards its own query and the one before it, so the diagonal key carries real weight in its row and the first masked key
  would, if it were seen."""
  g = torch.Generator().manual_seed(seed)
  q, k, v = (torch.randn((B, n, H, d), generator=g) for n in (nq, nkv, nkv))
  coff = nkv - nq
  lean = 6.0 / math.sqrt(d)                    # + ~6 on the score (q . q ~ d, times d ** -0.5)
  k[:, coff:] += lean * q / 3.0
  k[:, coff + 1:] += lean * q[:, :-1] / 3.0
  q = q * 3.0
  return tuple(bf(t.reshape(B, -1, H * d)) for t in (q, k, v))


def report_rows(name, got, ref):
  """test_ops_gpu._report's figure (max abs error over max |ref|), per query row; prints the worst row and returns its figure."""
  got, ref = got.float().cpu(), ref.float().cpu()
  err = (got - ref).abs().amax(dim=(0, 2))
  rel = err / ref.abs().amax(dim=(0, 2)).clamp_min(1e-6)
  rel = torch.where(torch.isfinite(rel), rel, torch.full_like(rel, float("inf")))
  w = int(rel.argmax())
  print(f"[{name}] worst query row {w} of {rel.numel()}: max_abs={err[w].item():.4e} rel_to_row_max={rel[w].item():.4e}")
  return rel[w].item()


def attn_defect_applies(defect, B, nq, nkv):
  return {"newest_key_hidden": nkv > 1, "causal_off_by_one": nq > 1, "stale_key_visible": True, "batch_row_zero": B > 1,
          "v_written_one_early": nq == 8 and nkv > nq}[defect]


def defective_attn_ref(attn_ref, q, k, v, H, scale, defect, seed=0):
  """What ops.attention(causal=True) would return with `defect`, stated through test_ops_gpu._attn_ref on altered operands."""
  B, nq, _ = q.shape
  nkv = k.shape[1]
  if defect == "newest_key_hidden":       # the last row loses key nkv - 1; no other row sees that key anyway
    head = attn_ref(q[:, :-1], k[:, :-1], v[:, :-1], H, scale, True) if nq > 1 else q[:, :0].float()
    return torch.cat([head, attn_ref(q[:, -1:], k[:, :-1], v[:, :-1], H, scale, False)], 1)
  if defect == "causal_off_by_one":       # row i sees key i + coff + 1 as well: the mask of nq - 1 rows against the same keys
    return torch.cat([attn_ref(q[:, :-1], k, v, H, scale, True), attn_ref(q[:, -1:], k, v, H, scale, False)], 1)
  if defect == "stale_key_visible":       # one more key that every row sees: put in front, the offset mask moves with it.  The stale
    g = torch.Generator().manual_seed(1000 + seed)    # row is what an earlier sequence left: here a key the last query leans towards
    sk = bf(q[:, -1:].float() / 3.0 * (2.0 / math.sqrt(q.shape[2] // H)))     # (+ ~6 on the last row's score, like its own key)
    sv = bf(torch.randn(v[:, :1].shape, generator=g))
    return attn_ref(q, torch.cat([sk, k.float()], 1), torch.cat([sv, v.float()], 1), H, scale, True)
  if defect == "batch_row_zero":
    return attn_ref(q, k[:1].expand(B, -1, -1), v[:1].expand(B, -1, -1), H, scale, True)
  if defect == "v_written_one_early":     # the step's V rows land one slot early; slot nkv - 1 keeps what was there (zeros)
    past = nkv - nq
    v2 = v.clone()
    v2[:, past - 1:nkv - 1] = v[:, past:]
    v2[:, nkv - 1] = 0
    return attn_ref(q, k, v2, H, scale, True)
  raise ValueError(defect)
