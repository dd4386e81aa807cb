"""gill_opt_extend (the layers over packed new tokens at per-row cache lengths) on the MI355X, on the OPT-125m synthetic rig
(ragged_decode_util.gill125_rig).

Four rows at history lengths 37, 0, 70 and 12 bring 33, 20, 17 and 0 new tokens.  The histories are put into the handle's cache by one
right-padded cached forward at past_len = 0 (so every row's slots beyond its length hold what the pad positions wrote), then one packed extend
runs.  Reference per row: that row ALONE through gill_opt_forward_cached, its history at past_len = 0 and then its new tokens as one call of
T_new rows at past_len = the history length (the flash kernel under a host-side past_len).  Bars: kv_cache_util.CACHED_VS_FULL_REL_BAR = 2e-2 on
the relative L2 error, with kv_cache_util's cosine bars (whole call and worst row).

  * every new token's hidden row (the packed output) meets the bars, fed as ids and fed as embeddings (the two inputs give the same bits);
  * hidden_last holds each row's last new row, bit for bit; the row without new tokens keeps what hidden_last held;
  * the row without new tokens keeps its cache: a decode step of that row after the extend gives the bits it gives without the extend (the
    step reads the row's whole cache below its length), and the extended rows' next decode step meets the bars against the row alone;
  * host bounds are checked before anything is enqueued."""
import pytest
import torch

import kv_cache_util as U
import ragged_decode_util as R
from gill_amd import _native as N
from gill_amd import synth

pytestmark = pytest.mark.gpu

HIST = (37, 0, 70, 12)
NEW = (33, 20, 17, 0)
CAP = 128


@pytest.fixture(scope="module")
def model(cuda):
  return R.gill125_rig(cuda).model


def _ids(cuda):
  T = max(h + n for h, n in zip(HIST, NEW)) + 1
  return synth.synthetic_prompt_ids(len(HIST), T, seed=83)[:, :T].to(cuda)      # one further token per row for the decode step


def _prefill(m, ids, cuda):
  """All histories into the cache rows 0 .. 3, right-padded with the rows' own continuation (stale keys / values beyond each length)."""
  m._opt_native(len(HIST), CAP)
  m._lm_forward_hidden_cached(m.input_embeddings(ids[:, :max(HIST)]), 0)


def _decode_step(m, ids, lens, cuda):
  B = len(lens)
  emb = torch.stack([m.input_embeddings(ids[b:b + 1, n:n + 1])[0, 0] for b, n in enumerate(lens)]).to(torch.bfloat16).contiguous()
  out = torch.empty((B, 1, 768), device=cuda, dtype=torch.float32)
  N.check(N.lib().gill_opt_decode_step(m._opt_handle, N.ptr(emb), N.ptr(torch.tensor(lens, dtype=torch.int32, device=cuda)), B, max(lens) + 1,
                                       N.ptr(out), N.current_stream()))
  torch.cuda.synchronize()
  return out[:, 0].clone()


def test_packed_extend_matches_every_row_alone(cuda, model):
  m = model
  ids = _ids(cuda)
  B, D = len(HIST), 768
  # the reference: every row alone, the flash kernel at a host-side past_len; then one decode step at the row's new length
  ref, ref_step = [], []
  for b, (h, n) in enumerate(zip(HIST, NEW)):
    m._opt_native(B, CAP)
    if h:
      m._lm_forward_hidden_cached(m.input_embeddings(ids[b:b + 1, :h]), 0)
    ref.append(m._lm_forward_hidden_cached(m.input_embeddings(ids[b:b + 1, h:h + n]), h)[0].clone() if n else None)
    if h + n:
      ref_step.append(m._lm_forward_hidden_cached(m.input_embeddings(ids[b:b + 1, h + n:h + n + 1]), h + n)[0, 0].clone())
    else:
      ref_step.append(None)
  # the idle row's decode step without any extend
  _prefill(m, ids, cuda)
  idle = _decode_step(m, ids, list(HIST), cuda)[3]

  cu = torch.tensor([0] + torch.tensor(NEW).cumsum(0).tolist(), dtype=torch.int32, device=cuda)
  lens = torch.tensor(HIST, dtype=torch.int32, device=cuda)
  packed = torch.cat([ids[b, h:h + n] for b, (h, n) in enumerate(zip(HIST, NEW))]).contiguous()
  total, bound = sum(NEW), max(h + n for h, n in zip(HIST, NEW))
  outs = []
  for mode in ("ids", "embeds"):
    _prefill(m, ids, cuda)
    last = torch.full((B, 1, D), 5.0, device=cuda, dtype=torch.float32)
    allh = torch.empty((total, D), device=cuda, dtype=torch.float32)
    kw = dict(ids=packed) if mode == "ids" else dict(embeds=m.input_embeddings(packed[None])[0].to(torch.bfloat16).contiguous())
    m._lm_extend(cu, lens, B, total, max(NEW), bound, last, hidden_all=allh, **kw)
    torch.cuda.synchronize()
    outs.append((last.clone(), allh.clone()))
  assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "ids and embeddings inputs give different bits"
  last, allh = outs[0]
  rows = allh.split(list(NEW))
  for b, (h, n) in enumerate(zip(HIST, NEW)):
    if n == 0:
      assert bool((last[b] == 5.0).all()), "hidden_last of a row without new tokens was written"
      continue
    U.check_calls(f"opt_extend row {b} (history {h}, {n} new)", [rows[b][None]], ref[b][None].cpu(), [(0, n)],
                  rel_bar=U.CACHED_VS_FULL_REL_BAR)
    assert torch.equal(last[b, 0], rows[b][-1]), f"row {b}: hidden_last is not the row's last new row"
  # the decode step that follows: the idle row bit for bit, the extended rows against the row alone
  after = _decode_step(m, ids, [h + n for h, n in zip(HIST, NEW)], cuda)
  assert torch.equal(after[3], idle), "a row without new tokens did not keep its cache"
  for b in range(3):
    U.check_calls(f"opt_extend row {b}: decode step on the extended cache", [after[b][None, None]], ref_step[b][None, None].cpu(), [(0, 1)],
                  rel_bar=U.CACHED_VS_FULL_REL_BAR)


def test_extend_checks_host_bounds_before_anything_is_enqueued(cuda, model):
  m = model
  m._opt_native(len(HIST), CAP)
  cb, ct = m._opt_cap
  B = 2
  cu = torch.tensor([0, 3, 5], dtype=torch.int32, device=cuda)
  lens = torch.tensor([4, 0], dtype=torch.int32, device=cuda)
  ids = torch.full((5,), 7, dtype=torch.int64, device=cuda)
  last = torch.full((B, 1, 768), 5.0, device=cuda, dtype=torch.float32)
  def call(**over):
    a = dict(h=m._opt_handle, ids=ids.data_ptr(), emb=None, extra=None, n_extra=0, cu=cu.data_ptr(), lens=lens.data_ptr(), B=B, total=5,
             max_new=3, bound=7, last=last.data_ptr(), allh=None, stream=N.current_stream())
    a.update(over)
    return N.lib().gill_opt_extend(a["h"], a["ids"], a["emb"], a["extra"], a["n_extra"], a["cu"], a["lens"], a["B"], a["total"], a["max_new"],
                                   a["bound"], a["last"], a["allh"], a["stream"])

  assert call(bound=ct + 1) != 0, "len_bound beyond max_seq accepted"
  assert call(bound=2) != 0, "len_bound below max_new accepted"
  assert call(max_new=0) != 0, "max_new = 0 accepted"
  assert call(B=cb + 1) != 0, "B beyond the workspace accepted"
  assert call(total=cb * ct + 1) != 0, "total_new beyond the workspace accepted"
  assert call(ids=None) != 0, "neither ids nor embeddings accepted"
  assert call(n_extra=2) != 0, "n_extra without a table accepted"
  torch.cuda.synchronize()
  assert bool((last == 5.0).all()), "a refused call wrote something"
  with pytest.raises(N.GillNativeError, match="KV cache"):
    m._lm_extend(cu, lens, B, 5, 3, ct + 1, last, ids=ids)
  assert call() == 0
  torch.cuda.synchronize()
  assert not bool((last == 5.0).any())
