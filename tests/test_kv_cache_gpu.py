"""gill_opt_forward_cached -- the path every GILLModel.generate() step takes -- against the fp32 oracle, on the MI355X.

Driven through the C ABI directly (ctypes -> libgill_amd.so) on handles of chosen capacity, with teacher-forced embeddings: fixed
synthetic token ids, no argmax anywhere, so a near-tie can neither hide nor fake a difference.  Every call's output rows are compared
with the rows at the same positions of ONE full causal pass of oracle.opt_ref.opt_hidden_states on the same bf16-rounded weights.
Statistics are per call (kv_cache_util.check_calls): the stat helper and the bars of test_opt_6_7b_geometry_img_hidden_vs_oracle
(rel_l2 < 3e-2, cos > 0.999) plus the minimum per-row cosine over the call's new rows (> 0.999).  The first failing call, its batch
row and position are in the printed lines.

The weights (kv_cache_util.peaked_opt_state_dict) make the softmax peaked; tests/test_kv_cache_host.py shows on the CPU that with
them each of six ways of breaking the cache misses these bars by 49x or more, while bf16 kernel arithmetic stays within 0.2 of them."""
import ctypes as C
import os

import pytest
import torch

import kv_cache_util as U
from oracle import opt_ref

pytestmark = pytest.mark.gpu
SLOW = pytest.mark.skipif(os.environ.get("GILL_SKIP_SLOW") == "1", reason="slow CPU oracle")
GEOMS = [pytest.param("opt67", marks=SLOW), "opt125"]


class _Handle:
  """One gill_opt handle of a given capacity."""

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

  def cached(self, x, past):
    """x (B, T_new, D) host fp32 (bf16-exact) -> hidden rows (B, T_new, D) fp32, host."""
    N = self.N
    xb = x.to(self.dev, torch.bfloat16).contiguous()
    out = torch.empty(xb.shape, device=self.dev, dtype=torch.float32)
    with torch.cuda.device(self.dev):
      N.check(N.lib().gill_opt_forward_cached(self.h, N.ptr(xb), xb.shape[0], xb.shape[1], past, N.ptr(out), N.current_stream()))
    return out.cpu()

  def full(self, x):
    N = self.N
    xb = x.to(self.dev, torch.bfloat16).contiguous()
    out = torch.empty(xb.shape, device=self.dev, dtype=torch.float32)
    with torch.cuda.device(self.dev):
      N.check(N.lib().gill_opt_forward(self.h, N.ptr(xb), xb.shape[0], xb.shape[1], N.ptr(out), N.current_stream()))
    return out.cpu()

  def run(self, x, schedule):
    return [self.cached(x[:, past:past + tn], past) for past, tn in U.calls_of(schedule)]

  def close(self):
    if self.h:
      self.N.lib().gill_opt_destroy(self.h)
      self.h = None


_WEIGHTS = {}


def _weights(name):
  if name not in _WEIGHTS:
    g = U.GEOMETRIES[name]
    _WEIGHTS[name] = U.peaked_opt_state_dict(g["cfg"], g["seed"])
  return _WEIGHTS[name]


def _oracle(sd, cfg, x):
  return opt_ref.opt_hidden_states(sd, cfg.num_layers, cfg.num_heads, x)


@pytest.mark.parametrize("name", GEOMS)
def test_cached_decode_schedule_vs_oracle(cuda, name):
  """The geometry's whole schedule at both batch sizes (opt67: B = 1, 4; prefill 30, single tokens to 33, an 8-token block, single
  tokens across the 64-key tile edge to 66.  opt125, 12 layers: B = 2, 9; 204 tokens, nq = 1 walking four key tiles, two 8-token
  blocks), each call against the oracle; then gill_opt_forward over the whole sequence against the cached rows, per call, at the bars
  of the cached-vs-re-forward test (rel < 2e-2, cos > 0.999)."""
  g = U.GEOMETRIES[name]
  cfg, schedule, sd = g["cfg"], g["schedule"], _weights(name)
  T, calls = sum(schedule), U.calls_of(schedule)
  for B in g["batches"]:
    x = U.token_embeds(sd, cfg, B, T, g["seed"])
    h = _Handle(sd, cfg, max(B, 8), T + 30, cuda)
    try:
      outs = h.run(x, schedule)
      whole = h.full(x)
    finally:
      h.close()
    U.check_calls(f"{name} B={B} cached vs oracle", outs, _oracle(sd, cfg, x), calls)
    U.check_calls(f"{name} B={B} cached vs gill_opt_forward", outs, whole, calls, rel_bar=U.CACHED_VS_FULL_REL_BAR)


@pytest.mark.parametrize("name", GEOMS)
def test_split_prefill_vs_oracle(cuda, name):
  """The same 30 tokens as one call and as 17 + 13 (T_new = 13 at past = 17): each against the oracle.  (Not bit-equal to each other:
  split-K factors depend on M.)"""
  g = U.GEOMETRIES[name]
  cfg, sd = g["cfg"], _weights(name)
  B = g["batches"][-1]
  x = U.token_embeds(sd, cfg, B, 30, g["seed"] + 1)
  ref = _oracle(sd, cfg, x)
  h = _Handle(sd, cfg, max(B, 8), 64, cuda)
  try:
    one = h.run(x, (30,))
    two = h.run(x, (17, 13))
  finally:
    h.close()
  U.check_calls(f"{name} B={B} prefill 30", one, ref, U.calls_of((30,)))
  U.check_calls(f"{name} B={B} prefill 17 + 13", two, ref, U.calls_of((17, 13)))


@pytest.mark.parametrize("name", GEOMS)
def test_handle_reuse_stale_rows_have_no_influence(cuda, name):
  """A long sequence (B = 4, 100 tokens), then on the same handle past_len = 0 with other tokens, a shorter prompt (20) and B = 2,
  run for several steps to 45 tokens: the cache still holds the first sequence's keys beyond nkv, inside the same 64-key tile and in
  batch rows 2, 3.  The second sequence's outputs must be bit-identical to the same schedule on a fresh handle of the same capacity,
  and meet the oracle."""
  g = U.GEOMETRIES[name]
  cfg, sd = g["cfg"], _weights(name)
  first, second = (60,) + (1,) * 40, (20, 1, 1, 1, 8) + (1,) * 14
  x1 = U.token_embeds(sd, cfg, 4, sum(first), g["seed"] + 2)
  x2 = U.token_embeds(sd, cfg, 2, sum(second), g["seed"] + 3)
  used, fresh = _Handle(sd, cfg, 8, 128, cuda), None
  try:
    outs1 = used.run(x1, first)
    outs2 = used.run(x2, second)
    fresh = _Handle(sd, cfg, 8, 128, cuda)
    outs2_fresh = fresh.run(x2, second)
  finally:
    used.close()
    if fresh is not None:
      fresh.close()
  U.check_calls(f"{name} first sequence", outs1, _oracle(sd, cfg, x1), U.calls_of(first))
  U.check_calls(f"{name} second sequence on the re-used handle", outs2, _oracle(sd, cfg, x2), U.calls_of(second))
  for c, (a, b) in enumerate(zip(outs2, outs2_fresh)):
    assert torch.equal(a, b), f"call {c} {U.calls_of(second)[c]}: re-used handle differs from a fresh one by {(a - b).abs().max().item():.3e}"


@pytest.mark.parametrize("name,max_seq", [("opt125", 96), ("opt125", 80), pytest.param("opt67", 96, marks=SLOW), pytest.param("opt67", 75, marks=SLOW)])
def test_capacity_edges(cuda, name, max_seq):
  """max_seq = 96 (cache pitch tcap % 64 == 32: the last key tile's V loads are clamped) and a max_seq in 65 .. 95 that is not a
  multiple of 32 (pitch 96 > max_seq), filled to exactly past_len + T_new == max_seq by an 8-token block and a last single token;
  every call against the oracle.  One token more is refused by the argument check, before any launch."""
  from gill_amd import _native as N
  g = U.GEOMETRIES[name]
  cfg, sd = g["cfg"], _weights(name)
  B = 3
  schedule = (30,) + (1,) * (max_seq - 39) + (8, 1)
  assert sum(schedule) == max_seq
  x = U.token_embeds(sd, cfg, B, max_seq + 1, g["seed"] + 4)
  h = _Handle(sd, cfg, 8, max_seq, cuda)
  try:
    outs = h.run(x[:, :max_seq], schedule)
    with pytest.raises(N.GillNativeError):
      h.cached(x[:, max_seq:], max_seq)
    with pytest.raises(N.GillNativeError):
      h.cached(x[:, max_seq - 7:], max_seq - 7)
  finally:
    h.close()
  U.check_calls(f"{name} max_seq={max_seq}", outs, _oracle(sd, cfg, x[:, :max_seq]), U.calls_of(schedule))
