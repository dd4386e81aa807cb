"""gill_opt_prefill_ids + gill_opt_decode_step -- the engine under GILLModel.generate_batch -- against the fp32 oracle, on the MI355X.

Driven through the C ABI on handles of chosen capacity, teacher-forced: fixed synthetic token ids, no argmax anywhere.  A run is a
right-padded prefill of rows of different lengths and then single-token steps with the per-row lengths advanced by hand on the device
array, so the rows cross the 32- and 64-slot edges at different iterations.  The reference is every row as ITS OWN sequence through
oracle.opt_ref.opt_hidden_states; the statistics and bars are kv_cache_util's (rel_l2 < 3e-2, cos > 0.999, minimum per-row cosine >
0.999), one call per row's prompt and one per step over all rows (ragged_decode_util.check_ragged).
tests/test_ragged_decode_host.py shows on the CPU that with these weights and lengths each of six ways of breaking the ragged path misses
these bars by 75x or more, while bf16 kernel arithmetic stays within 0.2 of them."""
import ctypes as C
import os

import pytest
import torch

import kv_cache_util as U
import ragged_decode_util as R

pytestmark = pytest.mark.gpu
GEOM = "opt125"
SLOW = pytest.mark.skipif(os.environ.get("GILL_SKIP_SLOW") == "1", reason="slow CPU oracle")


class _Handle:
  def __init__(self, sd, cfg, max_batch, max_seq, dev):
    from gill_amd import _native as N
    self.N, self.cfg, self.dev = N, cfg, dev
    c = N.gill_opt_config(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, num_layers=cfg.num_layers, num_heads=cfg.num_heads,
                          ffn_dim=cfg.ffn_dim, max_positions=cfg.max_positions, max_batch=max_batch, max_seq=max_seq)
    arr, keep = N.make_tensor_table(sd, dev)
    self.h = C.c_void_p()
    with torch.cuda.device(dev):
      N.check(N.lib().gill_opt_create(C.byref(self.h), C.byref(c), arr, len(keep)))
    del keep

  def prefill_ids(self, ids):
    N = self.N
    idt = ids.to(self.dev, torch.int64).contiguous()
    B, T = idt.shape
    out = torch.empty((B, T, self.cfg.hidden_size), device=self.dev, dtype=torch.float32)
    with torch.cuda.device(self.dev):
      N.check(N.lib().gill_opt_prefill_ids(self.h, N.ptr(idt), B, T, None, 0, N.ptr(out), N.current_stream()))
    return out.cpu()

  def step(self, x, lens, len_bound=None):
    """x (B, D) host fp32 (bf16-exact), lens: this step's per-row positions -> (B, D) host."""
    N = self.N
    xb = x.to(self.dev, torch.bfloat16).contiguous()
    ld = torch.tensor(lens, dtype=torch.int32, device=self.dev)
    out = torch.empty(xb.shape, device=self.dev, dtype=torch.float32)
    with torch.cuda.device(self.dev):
      N.check(N.lib().gill_opt_decode_step(self.h, N.ptr(xb), N.ptr(ld), xb.shape[0], max(lens) + 1 if len_bound is None else len_bound,
                                           N.ptr(out), N.current_stream()))
    return out.cpu()

  def ragged(self, prompt_ids, lengths, step_x):
    pre = self.prefill_ids(prompt_ids)
    outs = [self.step(step_x[:, s], [n + s for n in lengths]) for s in range(step_x.shape[1])]
    return pre, torch.stack(outs, 1)

  def cached(self, x, past):
    N = self.N
    xb = x.to(self.dev, torch.bfloat16).contiguous()
    out = torch.empty(xb.shape, device=self.dev, dtype=torch.float32)
    with torch.cuda.device(self.dev):
      N.check(N.lib().gill_opt_forward_cached(self.h, N.ptr(xb), xb.shape[0], xb.shape[1], past, N.ptr(out), N.current_stream()))
    return out.cpu()

  def close(self):
    if self.h:
      self.N.lib().gill_opt_destroy(self.h)
      self.h = None


_W = {}


def _weights(geom=GEOM):
  g = U.GEOMETRIES[geom]
  if geom not in _W:
    _W[geom] = U.peaked_opt_state_dict(g["cfg"], g["seed"])
  return g["cfg"], _W[geom], g["seed"]


def _inputs(cfg, sd, lengths, steps, seed):
  seqs, _, step_x = R.ragged_inputs(sd, cfg, lengths, steps, seed)
  _, prompt_ids, _ = R.ragged_ids(cfg, lengths, steps, seed)
  return seqs, prompt_ids, step_x


@pytest.mark.parametrize("geom,name", [("opt125", "b3"), ("opt125", "b9"), pytest.param("opt67", "b3", marks=SLOW)])
def test_ragged_schedule_vs_oracle(cuda, geom, name):
  """B = 3 with lengths (30, 23, 9) and B = 9 with lengths over 5 .. 31: prefill, then 40 steps; every row against its own sequence.
  (opt67: the OPT-6.7b geometry at 2 layers, heads of 128.)"""
  cfg, sd, seed = _weights(geom)
  lengths, steps = R.RUNS[name]
  seqs, prompt_ids, step_x = _inputs(cfg, sd, lengths, steps, seed + 10)
  h = _Handle(sd, cfg, max(len(lengths), 8), max(lengths) + steps + 5, cuda)
  try:
    pre, st = h.ragged(prompt_ids, lengths, step_x)
  finally:
    h.close()
  opro, ost = R.oracle_rows(sd, cfg, seqs, lengths, steps)
  R.check_ragged(f"{geom} {name} ragged vs oracle", pre, st, opro, ost, lengths)


def test_equal_lengths_agree_with_the_uniform_path(cuda):
  """Equal lengths: the same schedule through gill_opt_forward_cached, per step at the cached-vs-re-forward bar (rel < 2e-2)."""
  cfg, sd, seed = _weights()
  lengths, steps = (20, 20, 20), 40
  seqs, prompt_ids, step_x = _inputs(cfg, sd, lengths, steps, seed + 11)
  h = _Handle(sd, cfg, 8, 64, cuda)
  try:
    pre, st = h.ragged(prompt_ids, lengths, step_x)
    uni = [h.cached(seqs[:, :20], 0)] + [h.cached(seqs[:, 20 + s:21 + s], 20 + s) for s in range(steps)]
  finally:
    h.close()
  calls = [(0, 20)] + [(20 + s, 1) for s in range(steps)]
  U.check_calls("ragged vs gill_opt_forward_cached", [pre] + [st[:, s:s + 1] for s in range(steps)], torch.cat(uni, 1), calls,
                rel_bar=U.CACHED_VS_FULL_REL_BAR)


def test_handle_reuse_stale_rows_have_no_influence(cuda):
  """A 100-token B = 4 uniform sequence, then on the same handle a ragged B = 2 run: its rows sit under the first sequence's keys (beyond
  each length, inside the same tiles, and in batch rows 2, 3).  Bit-identical to the same run on a fresh handle of equal capacity,
  and it meets the oracle."""
  cfg, sd, seed = _weights()
  first = (60,) + (1,) * 40
  x1 = U.token_embeds(sd, cfg, 4, sum(first), seed + 12)
  lengths, steps = (27, 11), 40
  seqs, prompt_ids, step_x = _inputs(cfg, sd, lengths, steps, seed + 13)
  used, fresh = _Handle(sd, cfg, 8, 128, cuda), None
  try:
    for past, tn in U.calls_of(first):
      used.cached(x1[:, past:past + tn], past)
    pre, st = used.ragged(prompt_ids, lengths, step_x)
    fresh = _Handle(sd, cfg, 8, 128, cuda)
    pre_f, st_f = fresh.ragged(prompt_ids, lengths, step_x)
  finally:
    used.close()
    if fresh is not None:
      fresh.close()
  opro, ost = R.oracle_rows(sd, cfg, seqs, lengths, steps)
  R.check_ragged("ragged run on the re-used handle", pre, st, opro, ost, lengths)
  assert torch.equal(st, st_f), f"re-used handle differs from a fresh one by {(st - st_f).abs().max().item():.3e}"
  for b, n in enumerate(lengths):
    assert torch.equal(pre[b, :n], pre_f[b, :n])


@pytest.mark.parametrize("max_seq", [64, 75])
def test_capacity_edges(cuda, max_seq):
  """A row filling the cache to exactly max_seq (its last token at slot max_seq - 1; max_seq = 75: cache pitch 96 > max_seq) passes and
  meets the oracle; len_bound = max_seq + 1 is refused by the argument check, before any launch."""
  from gill_amd import _native as N
  cfg, sd, seed = _weights()
  steps = 12
  lengths = (max_seq - steps, 7, max_seq - steps - 3)
  seqs, prompt_ids, step_x = _inputs(cfg, sd, lengths, steps, seed + 14)
  h = _Handle(sd, cfg, 8, max_seq, cuda)
  try:
    pre, st = h.ragged(prompt_ids, lengths, step_x)
    with pytest.raises(N.GillNativeError):
      h.step(step_x[:, 0], [n + steps for n in lengths])            # max(lens) + 1 == max_seq + 1
    with pytest.raises(N.GillNativeError):
      h.step(step_x[:, 0], [3, 3, 3], len_bound=max_seq + 1)
  finally:
    h.close()
  opro, ost = R.oracle_rows(sd, cfg, seqs, lengths, steps)
  R.check_ragged(f"max_seq={max_seq}", pre, st, opro, ost, lengths)


def test_device_length_beyond_the_cache_is_clamped_and_reported(cuda):
  """The host's len_bound passes, but the device array holds a length past the cache: the step clamps it (no access outside the cache),
  the other rows keep their bits, and the next ragged decision reports the clamp in the row's flags."""
  from gill_amd import _native as N
  cfg, sd, seed = _weights()
  lengths, steps = (12, 9, 7), 2
  seqs, prompt_ids, step_x = _inputs(cfg, sd, lengths, steps, seed + 15)
  h = _Handle(sd, cfg, 8, 64, cuda)
  try:
    h.prefill_ids(prompt_ids)
    good = h.step(step_x[:, 0], list(lengths))
    h.prefill_ids(prompt_ids)
    bad = h.step(step_x[:, 0], [4000, lengths[1], lengths[2]], len_bound=13)
    assert torch.isfinite(bad).all() and torch.equal(bad[1:], good[1:])
    B, V = 3, cfg.vocab_size
    st = torch.zeros(6 * B + 1, dtype=torch.int32, device=cuda)
    logits = torch.zeros((B, V), device=cuda)
    tokens = torch.full((B, 4), -1, device=cuda, dtype=torch.int64)
    nxt = torch.zeros((B, cfg.hidden_size), device=cuda, dtype=torch.bfloat16)
    rule = N.gill_decode_rule()
    rule.filter_value = float("-inf")
    rule.ret_scale = rule.gen_scale = 1.0
    N.check(N.lib().gill_opt_pick_token_ragged(h.h, N.ptr(logits), B, C.byref(rule), 4, None, N.ptr(st), N.ptr(tokens), 4, N.ptr(nxt),
                                               N.current_stream()))
    torch.cuda.synchronize()
    assert st[5 * B:6 * B].cpu().tolist() == [2, 0, 0]
    N.check(N.lib().gill_opt_pick_token_ragged(h.h, N.ptr(logits), B, C.byref(rule), 4, None, N.ptr(st), N.ptr(tokens), 4, N.ptr(nxt),
                                               N.current_stream()))
    torch.cuda.synchronize()
    assert st[5 * B:6 * B].cpu().tolist() == [2, 0, 0] and st[3 * B:4 * B].cpu().tolist() == [2, 2, 2]
  finally:
    h.close()
