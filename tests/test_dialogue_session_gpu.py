"""Dialogue sessions end to end on the MI355X: GILLModel.open_session (rows whose KV caches are kept across turns, fed through gill_opt_extend)
and GILL.open_dialogues on top of it.

The sessions are the plans of dialogue_session_util (B = 4, greedy, min_word_tokens = 3, gen_scale_factor = 1e5, max_len = 5: three free tokens,
then two forced [IMG] blocks; n_tokens = 19, n_hidden = 11): a two-turn session with every row in both turns, and a three-turn one with a row idle
in turn 2, a row rolled back to two of its tokens and a row reset and restarted.  Every decoding row of every turn is compared with a from-scratch
generate_batch on what session.history(row) held when it decoded (the references run after the session has ended: generate_batch takes the cache
over, which the last check of each session uses to see a stale session raise).

Tokens follow the excusal rule of test_generate_batch_gpu.py: a disagreement is excused only at a free decision and only when the one-sequence
reference run's own logits put the two tokens within m; the row then leaves that turn's comparison, and excused decisions are capped at 5 % of all
decisions.  m is 10 x the bf16-operand emulation's logit distance from the fp32 oracle on these sessions' histories
(tools/dialogue_session_tolerance.py -> tests/golden/dialogue_session_tolerance.json); test_dialogue_session_host.py asserts on the CPU that the
oracle's own run of them has no decision with a top-2 margin under m.  The hidden rows (all 11, and the [IMG] block's 8) must be within REL_BAR."""
import pytest
import torch

import dialogue_session_util as S
import kv_cache_util as U
import ragged_decode_util as R
from gill_amd.dialogue import StaleSessionError
from test_decode_sample_gpu import IMG
from test_generate_batch_gpu import _rel, rig   # noqa: F401  (rig: the module fixture of the batch-API test)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gill125(cuda):
  return R.gill125_rig(cuda)


def _run_plan(m, name, cuda):
  """The session of PLANS[name] -> (session, [(turn, row, the ids the row decoded from, its tokens, n_hidden, its hidden rows)])."""
  seeds = S.load_seeds()[name]
  s = m.open_session(S.B, S.CAPACITY)
  records, turn = [], 0
  for op in S.PLANS[name]:
    if op[0] == "rollback":
      s.rollback(op[1], op[2])
    elif op[0] == "reset":
      s.reset([op[1]])
    else:
      rows = sorted(op[1])
      s.extend(rows, ids=[S.new_ids(turn, r, op[1][r], first=s.history(r)[0].numel() == 0, seed=seeds[(turn, r)]) for r in rows])
      before = [s.history(r)[0] for r in range(S.B)]
      tokens, n_tok, hidden, n_hid = s.generate(rows, max_len=S.MAX_LEN, **S.GEN_KW)
      assert tokens.shape == (S.B, 40) and hidden.shape == (S.B, 40, 768)
      for r in range(S.B):
        if r in rows:
          assert int(n_tok[r]) == S.N_TOK and int(n_hid[r]) == S.N_HID, (name, turn, r, n_tok.tolist(), n_hid.tolist())
          records.append((turn, r, before[r], tokens[r, :S.N_TOK].tolist(), int(n_hid[r]), hidden[r, :S.N_HID].clone()))
          assert s.history(r)[0].tolist() == before[r].tolist() + tokens[r, :S.N_TOK].tolist()
        else:     # idle: no decision, no token, the history as it was
          assert int(n_tok[r]) == 0 and int(n_hid[r]) == 0 and bool((tokens[r] == -1).all())
          assert s.history(r)[0].tolist() == before[r].tolist()
      turn += 1
  return s, records


def _check_against_from_scratch(m, name, records, cuda):
  tol = S.load_tolerance()
  excused = 0
  for turn in sorted({rec[0] for rec in records}):
    recs = [rec for rec in records if rec[0] == turn]
    lens = [int(rec[2].numel()) for rec in recs]
    ids = torch.full((len(recs), max(lens)), 1, dtype=torch.int64)
    for k, rec in enumerate(recs):
      ids[k, :lens[k]] = rec[2]
    tokens, n_tok, hidden, n_hid = m.generate_batch(ids=ids.to(cuda), lengths=lens, max_len=S.MAX_LEN, **S.GEN_KW)
    for k, (_, row, prompt, got, got_nh, got_h) in enumerate(recs):
      want = tokens[k, :int(n_tok[k])].tolist()
      assert want[3:11] == IMG and want[11:19] == IMG and int(n_tok[k]) == S.N_TOK and int(n_hid[k]) == got_nh == S.N_HID
      if got != want:
        col = next(j for j in range(S.N_TOK) if got[j] != want[j])
        assert col < 3, (name, turn, row, got, want)                # only a free decision can differ
        _, _, logits = m.generate(m.input_embeddings(prompt[None].to(cuda)), S.MAX_LEN, **S.GEN_KW)
        margin = abs(float(logits[col][0, got[col]] - logits[col][0, want[col]]))
        print(f"[dialogue session {name}] turn {turn} row {row} decision {col}: session picked {got[col]}, from scratch {want[col]}; the "
              f"reference's logits are {margin:.3e} apart (m = {tol:.3e})")
        assert margin <= tol, (name, turn, row, col, got[col], want[col], margin)
        excused += 1
        continue
      rel, rel_img = _rel(got_h, hidden[k, :S.N_HID]), _rel(got_h[3:11], hidden[k, 3:11])
      print(f"[dialogue session {name}] turn {turn} row {row} (history {lens[k]}): hidden rows rel_l2 {rel:.3e}, [IMG] block {rel_img:.3e}")
      assert rel < U.REL_BAR and rel_img < U.REL_BAR
  assert excused * 20 <= len(records) * S.MAX_LEN, excused


@pytest.mark.parametrize("name", ["two", "three"])
def test_greedy_session_equals_from_scratch_generate_batch(cuda, gill125, name):
  m = gill125.model
  s, records = _run_plan(m, name, cuda)
  assert len(records) == sum(len(op[1]) for op in S.PLANS[name] if op[0] == "turn")
  _check_against_from_scratch(m, name, records, cuda)
  # generate_batch has taken the cache over: the session must refuse, not read a cache that is no longer its own
  with pytest.raises(StaleSessionError):
    s.extend([0], ids=[[7, 8]])
  with pytest.raises(StaleSessionError):
    s.generate([0])


def test_a_seeded_row_draws_the_same_tokens_in_the_session_as_alone(cuda, gill125):
  m = gill125.model
  seeds = S.load_seeds()["two"]
  prompts = [S.new_ids(0, r, n, first=True, seed=seeds[(0, r)]) for r, n in sorted(S.PLANS["two"][0][1].items())]
  more = [S.new_ids(1, r, n, first=False, seed=seeds[(1, r)]) for r, n in sorted(S.PLANS["two"][1][1].items())]
  kw = dict(max_len=4, temperature=4.0, top_p=0.9, seed=7)
  cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state()

  def run(rows):
    s = m.open_session(S.B, S.CAPACITY)
    out = []
    for turn_ids in (prompts, more):
      s.extend(rows, ids=[turn_ids[r] for r in rows])
      tokens, n_tok, _, _ = s.generate(rows, **kw)
      out.append({r: tokens[r, :int(n_tok[r])].tolist() for r in rows})
    return out

  full = run([0, 1, 2, 3])
  assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(), dev_state)
  assert len({tuple(v) for v in full[0].values()}) > 1
  for r in (0, 2):
    alone = run([r])
    assert alone[0][r] == full[0][r] and alone[1][r] == full[1][r], r


def test_session_argument_errors(cuda, gill125):
  m = gill125.model
  with pytest.raises(ValueError, match="position table"):
    m.open_session(2, m.opt_cfg.max_positions + 1)
  s = m.open_session(2, 64)
  with pytest.raises(RuntimeError, match="extend"):
    s.generate([0])
  s.extend([0], ids=[[2, 5, 6]])
  with pytest.raises(ValueError, match="capacity"):
    s.generate([0], max_len=8)                            # 3 + 8 * 8 > 64
  with pytest.raises(ValueError, match="seed"):
    s.generate([0], max_len=2, temperature=1.0)
  with pytest.raises(NotImplementedError):
    s.extend([1], embeddings=torch.zeros(1, 3, 768))
  with pytest.raises(ValueError):
    s.extend([1], ids=[[-1, 5]])                          # a visual row without a table
  # an idle row near the session's capacity does not count against the rows that decode (its length stands while theirs grow)
  s.extend([1], ids=[[2] + list(range(100, 161))])        # 62 of the 63 tokens a row may hold
  tokens, n_tok, _, _ = s.generate([0], max_len=5, **S.GEN_KW)      # 3 + 40 <= 64
  assert n_tok.tolist() == [S.N_TOK, 0]


def test_open_dialogues_equals_the_batch_method_on_the_concatenated_prompts(rig):   # noqa: F811
  """Two dialogues, two turns, an image in turn 1 of dialogue 0; dialogue 1 is idle in turn 2.  Turn 1 decodes with min_word_tokens = 0 (two
  certain [IMG] blocks), so its reply is exactly the string '[IMG0]..[IMG7]' twice and the concatenated prompt list of turn 2 can state it:
  [image, text, reply, the new strings], <bos> on the first string only."""
  g = rig.m
  m = g.model
  gen_prefix = "".join(f"[IMG{i}]" for i in range(8))
  first = [[rig.img, rig.text], ["a photo of", "a small red kite"]]
  second = [["and next to it", "two brown dogs on a beach"], None]
  kw1 = dict(num_words=2, min_word_tokens=0, gen_scale_factor=1e5)
  kw2 = dict(num_words=5, min_word_tokens=3, gen_scale_factor=1e5)
  d = g.open_dialogues(2, capacity=256)
  got1 = d.say(first, **kw1)
  hist1 = d.history(0)[0].tolist()
  got2 = d.say(second, **kw2)
  assert got2[1] is None and len(got1) == len(got2) == 2
  # the history is token ids and visual rows: the image's 4 slots, <bos> + text, the reply's 16 ids; then turn 2 without a <bos>
  assert hist1[:4] == [-1, -2, -3, -4] and hist1[4] == 2 and hist1[-16:] == IMG * 2 and hist1.count(2) == 1
  ids2, extra2 = d.history(0)
  assert ids2.tolist()[:len(hist1)] == hist1 and ids2.tolist().count(2) == 1 and extra2.shape == (4, 768)
  want1 = g.generate_for_images_and_texts_batch(first, **kw1)
  want2 = g.generate_for_images_and_texts_batch([first[0] + [gen_prefix * 2] + second[0]], **kw2)
  with pytest.raises(StaleSessionError):
    d.say(second, **kw2)
  for tag, got, want in (("turn 1 dialogue 0", got1[0], want1[0]), ("turn 1 dialogue 1", got1[1], want1[1]), ("turn 2 dialogue 0", got2[0], want2[0])):
    assert len(got) == len(want) == 2
    assert got[0] == want[0] and got[0].endswith("[IMG7]"), (tag, got[0], want[0])
    assert got[1]["decision"] == want[1]["decision"] == ["gen", [0, 1]] and got[1]["ret"] == []
    a, w = got[1]["gen"][0], want[1]["gen"][0]
    assert a.shape == w.shape == (1, 77, 768)
    rel = _rel(a, w)
    print(f"[open_dialogues] {tag}: caption {got[0]!r}; gen embedding rel_l2 {rel:.3e}")
    assert rel < U.REL_BAR
  # reset passes through: the dialogue starts again, with its <bos>
  d2 = g.open_dialogues(2, capacity=256)
  d2.say([["a photo of"], None], **kw1)
  d2.reset([0])
  assert d2.history(0)[0].numel() == 0
  d2.say([["a small red kite"], None], **kw1)
  assert d2.history(0)[0].tolist()[0] == 2
