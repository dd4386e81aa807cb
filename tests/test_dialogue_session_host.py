"""The host side of dialogue sessions, on the CPU: the bookkeeping functions of gill_amd/dialogue.py (packing and cu_new, the pending token,
rollback, reset, epoch invalidation, <bos> on a dialogue's first string only), the new C symbols and their ctypes signatures, and the proof that
the prompts of test_dialogue_session_gpu.py need no excusal by themselves: the fp32 oracle's own greedy run of the test's sessions
(dialogue_session_util.oracle_session) has no decision with a top-2 margin under the recorded near-tie bar m, and m is 10 x the bf16-operand
emulation's logit distance from the oracle measured on those very histories (tools/dialogue_session_tolerance.py)."""
import ctypes as C
import inspect

import pytest
import torch

import dialogue_session_util as S
from gill_amd import dialogue as Dg
from gill_amd import synth


def test_pack_feed_packs_rows_and_builds_cu_new():
  packed, cu, max_new = Dg.pack_feed([[5, 6, 7], [], [9], [-1, -2, 11]], [0, 0, 0, 4])
  assert packed == [5, 6, 7, 9, -5, -6, 11]            # row 3's visual rows start at row 4 of the call's table
  assert cu == [0, 3, 3, 4, 7] and max_new == 3
  assert Dg.pack_feed([[], []], [0, 0]) == ([], [0, 0, 0], 0)
  assert Dg.pack_feed([], []) == ([], [0], 0)


def test_row_book_keeps_the_newest_token_pending():
  bk = Dg.RowBook()
  bk.append([2, 10, 11])
  assert bk.feed() == [2, 10, 11] and not bk.ready
  bk.fed()
  assert bk.cached == 3 and bk.feed() == [] and bk.ready
  bk.generated([20, 21, 22])
  # the cache is valid on [0, len - 1): the newest token's key / value may not have been stored
  assert bk.ids == [2, 10, 11, 20, 21, 22] and bk.cached == 5 and bk.turn_start == 3 and not bk.ready
  bk.append([30, 31])
  assert bk.feed() == [22, 30, 31]                       # [pending token | new tokens]
  bk.fed()
  assert bk.cached == 8
  bk.generated([])                                       # max_len = 0: nothing emitted, nothing pending
  assert bk.cached == 8 and bk.ids[-1] == 31


def test_row_book_reindexes_visual_rows_per_turn():
  bk = Dg.RowBook()
  bk.append([-1, -2, 2, 7], n_new_extra=2)
  bk.fed()
  bk.generated([40])
  bk.append([-1, -2, -3, 8], n_new_extra=3)              # the second turn's images: rows 2 .. 4 of the row's own table
  assert bk.ids == [-1, -2, 2, 7, 40, -3, -4, -5, 8] and bk.n_extra == 5
  with pytest.raises(ValueError):
    bk.append([-2], n_new_extra=1)


def test_rollback_only_lowers_the_length_and_the_history():
  bk = Dg.RowBook()
  bk.append([2, 10])
  bk.fed()
  bk.generated([20, 21, 22, 23])
  assert bk.cached == 5
  bk.rollback(2)
  assert bk.ids == [2, 10, 20, 21] and bk.cached == 3 and bk.feed() == [21] and not bk.ready      # the newest kept token is pending again
  bk.append([30])
  assert bk.feed() == [21, 30]
  bk.fed()
  bk.generated([40, 41])
  with pytest.raises(ValueError):
    bk.rollback(3)
  bk.rollback(0)                                         # the whole reply gone: the turn's last prompt token is pending
  assert bk.ids == [2, 10, 20, 21, 30] and bk.cached == 4 and bk.feed() == [30]
  # a rollback never raises the cached length
  bk2 = Dg.RowBook()
  bk2.append([2, 3, 4])
  bk2.fed()
  bk2.generated([9])
  bk2.rollback(1)
  assert bk2.cached == 3 and bk2.feed() == [9]


def test_reset_empties_a_row():
  bk = Dg.RowBook()
  bk.append([-1, 2, 10], n_new_extra=1)
  bk.fed()
  bk.generated([20])
  bk.reset()
  assert bk.ids == [] and bk.cached == 0 and bk.n_extra == 0 and bk.turn_start == 0 and not bk.ready and bk.feed() == []


def test_a_stale_epoch_raises():
  Dg.check_epoch(3, 3)
  with pytest.raises(Dg.StaleSessionError, match="stale"):
    Dg.check_epoch(3, 4)


def test_every_cache_writing_entry_bumps_the_epoch():
  """generate, generate_batch, _lm_forward_hidden_cached, _opt_native growth, quantize_lm and refresh_native each carry the counter; the
  session's own entries (_lm_extend, the shared loop) do not."""
  from gill_amd.models import GILLModel
  for name in ("generate", "generate_batch", "_lm_forward_hidden_cached", "_opt_native", "quantize_lm", "refresh_native"):
    assert "_cache_epoch += 1" in inspect.getsource(getattr(GILLModel, name)), name
  for name in ("_lm_extend", "_ragged_decode_loop", "_ragged_results"):
    assert "_cache_epoch" not in inspect.getsource(getattr(GILLModel, name)), name


class _StubModel:
  """What DialogueSession touches of a GILLModel, on the CPU: the extend call is recorded instead of run."""

  def __init__(self):
    self.opt_cfg = synth.OptConfig(vocab_size=512, hidden_size=64, num_layers=1, num_heads=1, ffn_dim=64, max_positions=256)
    self.logit_scale = torch.zeros(())
    self._cache_epoch = 0
    self._opt_cap = (0, 0)
    self.calls = []

  def _opt_native(self, B, T):
    if B > self._opt_cap[0] or T > self._opt_cap[1]:
      self._cache_epoch += 1
      self._opt_cap = (max(B, self._opt_cap[0]), max(T, self._opt_cap[1]))
    return object()

  def _lm_extend(self, cu_new, lens_dev, B, total_new, max_new, len_bound, hidden_last, ids=None, embeds=None, extra_rows=None,
                 hidden_all=None):
    self.calls.append(dict(cu=cu_new.tolist(), lens=lens_dev.tolist(), B=B, total=total_new, max_new=max_new, bound=len_bound,
                           ids=ids.tolist(), extra=None if extra_rows is None else extra_rows.float()))


def test_session_extend_packs_pending_and_new_tokens_at_the_cached_lengths():
  m = _StubModel()
  s = Dg.DialogueSession(m, 3, 64)
  vis = torch.arange(2 * 64, dtype=torch.float32).reshape(2, 64).bfloat16()
  s.extend([0, 2], ids=[[2, 10, 11], [-1, -2, 2, 12]], extra_rows=[None, vis])
  c = m.calls[-1]
  assert c["cu"] == [0, 3, 3, 7] and c["lens"] == [0, 0, 0] and c["ids"] == [2, 10, 11, -1, -2, 2, 12]
  assert (c["B"], c["total"], c["max_new"], c["bound"]) == (3, 7, 4, 4) and torch.equal(c["extra"], vis.float())
  # what a decode loop leaves: the newest token pending
  s.books[0].generated([20, 21])
  s.books[2].generated([30])
  s.extend([0], ids=[[40]])
  c = m.calls[-1]
  assert c["cu"] == [0, 2, 2, 2] and c["lens"] == [4, 0, 4] and c["ids"] == [21, 40] and c["bound"] == 6 and c["extra"] is None
  # history: re-indexed for a from-scratch call
  ids, extra = s.history(2)
  assert ids.tolist() == [-1, -2, 2, 12, 30] and torch.equal(extra, vis)
  # a second image turn in row 2: the call's table holds the row's rows, the new ids count on from them
  vis2 = torch.ones((1, 64)).bfloat16()
  s.extend([2, 1], ids=[[-1, 13], [2, 5]], extra_rows=[vis2, None])
  c = m.calls[-1]
  assert c["cu"] == [0, 0, 2, 5] and c["lens"] == [6, 0, 4] and c["ids"] == [2, 5, 30, -3, 13]
  assert torch.equal(c["extra"], torch.cat([vis, vis2]).float())
  # rollback and reset are host-only
  n_calls = len(m.calls)
  s.books[2].generated([50, 51, 52])
  s.rollback(2, 1)
  s.reset([1])
  assert len(m.calls) == n_calls and s.history(2)[0].tolist()[-1] == 50 and s.history(1)[0].numel() == 0 and s.history(1)[1] is None
  with pytest.raises(RuntimeError, match="extend"):
    s.generate([1])                                       # an emptied row has nothing to decode from
  with pytest.raises(ValueError, match="capacity"):
    s.extend([1], ids=[[2] * 64])
  with pytest.raises(ValueError):
    s.extend([1, 1], ids=[[2], [3]])
  # a second session over the same handle takes the cache over
  s_old = Dg.DialogueSession(m, 2, 32)
  s = Dg.DialogueSession(m, 3, 64)
  with pytest.raises(Dg.StaleSessionError):
    s_old.extend([0], ids=[[2, 3]])
  s.extend([0], ids=[[2, 3]])
  # another entry wrote the cache: the session refuses to go on
  m._cache_epoch += 1
  for call in (lambda: s.extend([0], ids=[[7]]), lambda: s.generate([0]), lambda: s.rollback(0, 0), lambda: s.reset([0])):
    with pytest.raises(Dg.StaleSessionError):
      call()


def test_bos_goes_on_a_dialogues_first_string_only():
  tok = synth.HashTokenizer()
  is_image = lambda p: isinstance(p, torch.Tensor)      # noqa: E731
  img = torch.zeros((4, 4, 3), dtype=torch.uint8)
  ids, images, done = Dg.segment_turn(tok, [img, "a photo of", img, "a kite"], 4, False, False, is_image)
  words = tok("a photo of", add_special_tokens=False).input_ids
  assert ids[:4] == [-1, -2, -3, -4] and ids[4] == tok.bos_token_id and ids[5:8] == words
  assert ids[8:12] == [-5, -6, -7, -8] and tok.bos_token_id not in ids[12:] and len(images) == 2 and done
  # a later turn: no <bos>, unless always_add_bos
  ids2, _, done2 = Dg.segment_turn(tok, ["and now a dog"], 4, done, False, is_image)
  assert tok.bos_token_id not in ids2 and done2
  ids3, _, _ = Dg.segment_turn(tok, ["and now", "a dog"], 4, done, True, is_image)
  assert ids3.count(tok.bos_token_id) == 2
  # a first turn without a string leaves <bos> to the first string of a later turn
  ids4, _, done4 = Dg.segment_turn(tok, [img], 4, False, False, is_image)
  assert ids4 == [-1, -2, -3, -4] and not done4
  ids5, _, done5 = Dg.segment_turn(tok, ["what is this"], 4, done4, False, is_image)
  assert ids5[0] == tok.bos_token_id and done5
  with pytest.raises(ValueError):
    Dg.segment_turn(tok, [3.5], 4, False, False, is_image)
  with pytest.raises(ValueError):
    Dg.segment_turn(tok, [], 4, False, False, is_image)


def test_new_symbols_load_with_their_signatures():
  from gill_amd import _native as N
  lib = N.lib()
  vp, i = C.c_void_p, C.c_int
  want = {
    "gill_attention_extend": [vp, vp, vp, i, vp, vp, vp, vp, vp, i, i, i, i, i, i, vp, vp],
    "gill_opt_extend": [vp, vp, vp, vp, i, vp, vp, i, i, i, i, vp, vp, vp],
  }
  for name, args in want.items():
    fn = getattr(lib, name)
    assert fn.restype is C.c_int and list(fn.argtypes) == args, name
  # argument errors come back as codes with a message, without a GPU
  assert lib.gill_attention_extend(None, None, None, 0, None, None, None, None, None, 1, 1, 1, 12, 64, 96, None, None) != 0
  assert b"extend attention" in lib.gill_last_error()
  assert lib.gill_opt_extend(None, None, None, None, 0, None, None, 1, 1, 1, 1, None, None, None) != 0


def test_session_plans_walk_the_recorded_histories():
  """The plans themselves: a row idle in turn 2, a rolled-back row, a row reset and restarted; <bos> only where a dialogue starts."""
  seeds = S.load_seeds()
  for name, plan in S.PLANS.items():
    seen = []
    hist = S.walk(plan, seeds[name], lambda turn, row, h: seen.append((turn, row, h)) or [7, 8, 9] + synth.IMG_TOKEN_IDS * 2)
    for turn, row, h in seen:
      assert h[0] == 2 and h.count(2) == 1, (name, turn, row)
      assert len(h) + S.MAX_LEN * 8 <= S.CAPACITY - 1
  three = S.PLANS["three"]
  assert three[1] == ("rollback", 2, 2) and 1 not in three[2][1] and three[3] == ("reset", 3) and 3 in three[4][1]


def test_oracle_greedy_run_of_the_sessions_has_no_near_tie():
  m = S.load_tolerance()
  memo = {}
  runs = [r for name in S.PLANS for r in S.oracle_session(name, memo=memo)]
  dist, margin = max(r[5] for r in runs), min(min(r[4]) for r in runs)
  print(f"[dialogue sessions] {len(runs)} decoding rows, bf16 emulation vs oracle logit distance {dist:.3e}, m = {m:.3e}; smallest oracle top-2 "
        f"margin {margin:.3e}")
  assert abs(m - 10 * dist) <= 1e-3 * m
  assert margin >= m
