"""The e4m3 KV cache end to end on the MI355X, on the OPT-125m rig of ragged_decode_util: GILLModel.quantize_kv('fp8') under generate_batch and
a dialogue session, the cache's size, and the entries that refuse it.

The reference is the quantised-cache model on the CPU in fp64 (kv8_util.kv8_forward / greedy_ref): every key and value rounded to its e4m3 row
before any query uses it, a function of the token sequence alone.  Bars (tests/golden/kv8_tolerance.json, measured on the CPU by
tools/kv8_tolerance.py on these very inputs; profiles/kv8.md):

  hid_bar  4 x the worst per-row rel-L2 distance between the bf16-storage fp32 emulation and that fp64 run.  A one-ulp bf16 difference in a K or
           V element can flip an e4m3 code, so two honest runs differ by more than their accumulation order; the emulation measures by how much.
  m_logit  4 x the worst logit distance of the same two runs: the near-tie bar.  A greedy decision at which the device parts from the reference
           is excused only if the REFERENCE's own margin between the two tokens is within m_logit; the row then leaves the comparison; at most
           one decision in ten may be excused.  The prompt seeds are chosen (same tool, same file; tests/test_kv8_host.py asserts it) so that
           the reference alone has no decision inside m_logit."""
import contextlib

import pytest
import torch

import dialogue_session_util as S
import kv8_util as K
import ragged_decode_util as R
from gill_amd.dialogue import StaleSessionError
from test_decode_sample_gpu import IMG

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _kv8(cuda, weights="bf16"):
  """The shared rig with an e4m3 cache (and the given weight format); handed back as it was."""
  g = R.gill125_rig(cuda)
  m = g.model
  try:
    m.quantize_kv("fp8")
    m.quantize_lm(weights)
    yield g
  finally:
    m.quantize_lm("bf16")
    if hasattr(m, "quantize_kv"):
      m.quantize_kv("bf16")


def _lib():
  from gill_amd import _native as N
  return N.lib()


def _excusal(tag, weights, prompt, got, want, col, m_logit):
  """The reference's own margin between the two tokens at the decision where two runs part (prompt + the tokens they share)."""
  cfg, sd = K.model(weights)
  lg = K.greedy_ref(sd, cfg, list(prompt) + list(want[:col]), n_dec=1, emulate=False)["logits"][0]
  margin = abs(float(lg[got[col]] - lg[want[col]]))
  print(f"[{tag}] decision {col}: {got[col]} against {want[col]}; the reference's logits are {margin:.3e} apart (m_logit {m_logit:.3e})")
  assert margin <= m_logit, (tag, col, got[col], want[col], margin)


@pytest.mark.parametrize("weights", ["bf16", "fp8"])
def test_ragged_batch_on_the_e4m3_cache_follows_the_quantised_reference(cuda, weights):
  gold = K.golden()
  seeds = tuple(gold["seeds"])
  ids, lens = K.prompt_ids(seeds)
  kw = dict(max_len=K.N_DEC, min_word_tokens=K.N_DEC)
  with _kv8(cuda, weights) as g:
    m = g.model
    tokens, n_tok, hidden, n_hid = m.generate_batch(ids=ids.to(cuda), lengths=lens, **kw)
    assert _lib().gill_opt_kv_format(m._opt_handle) == 1 and _lib().gill_opt_weight_mode(m._opt_handle) == (1 if weights == "fp8" else 0)
    # the same prompts handed over as embeddings: the same packed prefill, the same bits
    t2, n2, h2, _ = m.generate_batch(embeddings=m.input_embeddings(ids.to(cuda)), lengths=lens, **kw)
    assert torch.equal(t2, tokens) and torch.equal(n2, n_tok) and torch.equal(h2, hidden)
  assert n_tok.tolist() == [K.N_DEC] * len(lens) and n_hid.tolist() == [K.N_DEC - 1] * len(lens)
  ref = K.batch_reference(weights, seeds)
  excused, worst = 0, 0.0
  for b, n in enumerate(lens):
    got, want = tokens[b, :K.N_DEC].tolist(), ref[b]["tokens"]
    col = next((j for j in range(K.N_DEC) if got[j] != want[j]), K.N_DEC)
    if col < K.N_DEC:
      _excusal(f"kv8 batch {weights} row {b}", weights, ids[b, :n].tolist(), got, want, col, gold["m_logit"])
      excused += 1
    # hidden[b, j] belongs to generated token j's position n + j: comparable while the two runs share their tokens
    rows = min(col, K.N_DEC - 1)
    rel = K.row_rel(hidden[b, :rows].cpu(), ref[b]["hidden"][n:n + rows])
    worst = max(worst, rel)
    print(f"[kv8 batch {weights}] row {b} (length {n}): {rows} hidden rows, worst rel_l2 {rel:.3e} (hid_bar {gold['hid_bar']:.3e}); tokens {got}")
    assert rel < gold["hid_bar"], (b, rel)
  assert excused * 10 <= len(lens) * K.N_DEC, excused


def _run_plan(s, seeds):
  """The session of the golden plan -> [(turn, row, the ids the row decoded from, its tokens, its hidden rows)]."""
  records, turn = [], 0
  for op in S.PLANS[K.golden()["plan"]]:
    if op[0] == "rollback":
      s.rollback(op[1], op[2])
    elif op[0] == "reset":
      s.reset([op[1]])
    else:
      rows = sorted(op[1])
      s.extend(rows, ids=[S.new_ids(turn, r, op[1][r], first=s.history(r)[0].numel() == 0, seed=seeds[(turn, r)]) for r in rows])
      before = [s.history(r)[0] for r in range(S.B)]
      tokens, n_tok, hidden, n_hid = s.generate(rows, max_len=S.MAX_LEN, **S.GEN_KW)
      for r in rows:
        assert int(n_tok[r]) == S.N_TOK and int(n_hid[r]) == S.N_HID, (turn, r, n_tok.tolist(), n_hid.tolist())
        records.append((turn, r, before[r], tokens[r, :S.N_TOK].tolist(), hidden[r, :S.N_HID].clone()))
      turn += 1
  return records


def test_session_on_the_e4m3_cache_equals_from_scratch_and_survives_a_rollback(cuda):
  gold = K.golden()
  seeds = {tuple(int(v) for v in k.split(",")): int(v) for k, v in gold["session_seeds"].items()}
  excused = decisions = 0
  with _kv8(cuda) as g:
    m = g.model
    s = m.open_session(S.B, S.CAPACITY)
    records = _run_plan(s, seeds)
    assert len(records) == sum(len(op[1]) for op in S.PLANS[gold["plan"]] if op[0] == "turn")
    # rollback to the row's prompt, extend without new tokens (the pending token alone), decode again: the last turn's tokens
    for row in (0, 2):
      _, _, prompt, want, want_h = [rec for rec in records if rec[1] == row][-1]
      s.rollback(row, 0)
      assert s.history(row)[0].tolist() == prompt.tolist()
      s.extend([row], ids=[[]])
      tokens, n_tok, hidden, _ = s.generate([row], max_len=S.MAX_LEN, **S.GEN_KW)
      got = tokens[row, :int(n_tok[row])].tolist()
      decisions += S.MAX_LEN
      if got != want:
        col = next(j for j in range(S.N_TOK) if got[j] != want[j])
        assert col < 3, (row, got, want)
        _excusal(f"kv8 session rollback row {row}", "bf16", prompt.tolist(), got, want, col, gold["m_logit"])
        excused += 1
        continue
      rel = K.row_rel(hidden[row, :S.N_HID].cpu(), want_h.cpu())
      print(f"[kv8 session] rollback + extend of row {row}: the turn's {S.N_TOK} tokens again, hidden rows rel_l2 {rel:.3e}")
      assert rel < gold["hid_bar"]
    # every decoding row of every turn against a from-scratch generate_batch on what its history held (this takes the cache over)
    for turn in sorted({rec[0] for rec in records}):
      recs = [rec for rec in records if rec[0] == turn]
      lens = [int(rec[2].numel()) for rec in recs]
      ids = torch.full((len(recs), max(lens)), 1, dtype=torch.int64)
      for k, rec in enumerate(recs):
        ids[k, :lens[k]] = rec[2]
      tokens, n_tok, hidden, n_hid = m.generate_batch(ids=ids.to(cuda), lengths=lens, max_len=S.MAX_LEN, **S.GEN_KW)
      for k, (_, row, prompt, got, got_h) in enumerate(recs):
        want = tokens[k, :int(n_tok[k])].tolist()
        decisions += S.MAX_LEN
        assert want[3:11] == IMG and want[11:19] == IMG and int(n_tok[k]) == S.N_TOK and int(n_hid[k]) == S.N_HID
        if got != want:
          col = next(j for j in range(S.N_TOK) if got[j] != want[j])
          assert col < 3, (turn, row, got, want)                # only a free decision can differ
          _excusal(f"kv8 session turn {turn} row {row}", "bf16", prompt.tolist(), got, want, col, gold["m_logit"])
          excused += 1
          continue
        rel = K.row_rel(got_h.cpu(), hidden[k, :S.N_HID].cpu())
        print(f"[kv8 session] turn {turn} row {row} (history {lens[k]}): hidden rows rel_l2 {rel:.3e} (hid_bar {gold['hid_bar']:.3e})")
        assert rel < gold["hid_bar"]
    with pytest.raises(StaleSessionError):
      s.generate([0])
  assert excused * 10 <= decisions, (excused, decisions)


def test_cache_bytes_of_both_formats(cuda):
  lib = _lib()
  ids, lens = K.prompt_ids(tuple(K.golden()["seeds"]))
  kw = dict(ids=ids.to(cuda), lengths=lens, max_len=1)
  with _kv8(cuda) as g:
    m = g.model
    c = m.opt_cfg
    dp = c.hidden_size // c.num_heads
    dpv = (dp + 31) // 32 * 32
    h = m._opt_native(len(lens), 64)
    assert lib.gill_opt_kv_bytes(h) == 0, "no cache before the first cached entry"
    m.generate_batch(**kw)
    cb, ct = m._opt_cap
    slots = c.num_layers * cb * c.num_heads * ((ct + 31) // 32 * 32)
    assert lib.gill_opt_kv_format(m._opt_handle) == 1 and lib.gill_opt_kv_bytes(m._opt_handle) == slots * (dp + dpv + 2)
    m.quantize_kv("bf16")
    m.generate_batch(**kw)
    cb, ct = m._opt_cap
    slots = c.num_layers * cb * c.num_heads * ((ct + 31) // 32 * 32)
    assert lib.gill_opt_kv_format(m._opt_handle) == 0 and lib.gill_opt_kv_bytes(m._opt_handle) == slots * 2 * (dp + dpv)


def test_entries_that_refuse_the_e4m3_cache(cuda):
  from gill_amd import _native as N
  lib = _lib()
  ids, lens = K.prompt_ids(tuple(K.golden()["seeds"]))
  with _kv8(cuda) as g:
    m = g.model
    emb = m.input_embeddings(ids[:1, :lens[0]].to(cuda))
    with pytest.raises(ValueError, match="generate_batch"):
      m.generate(emb, 2)
    with pytest.raises(ValueError, match="generate_batch"):
      m._lm_forward_hidden_cached(emb, 0)
    with pytest.raises(ValueError, match="generate_batch"):
      g.generate_for_images_and_texts(["a photo of"], num_words=2)
    with pytest.raises(ValueError, match="quantize_kv"):
      m.quantize_kv("int4")
    out, _, _ = m.generate(emb, 1, min_word_tokens=1, use_kv_cache=False)          # no cache: untouched
    assert out.shape == (1, 1)
    # the C ABI: the format is refused once the cache exists; the flash entries name the format
    m.generate_batch(ids=ids.to(cuda), lengths=lens, max_len=1)
    h = m._opt_handle
    assert lib.gill_opt_kv_bytes(h) > 0
    assert lib.gill_opt_set_kv_format(h, 0) != 0 and b"allocated" in lib.gill_last_error()
    assert lib.gill_opt_set_kv_format(h, 1) == 0 and lib.gill_opt_set_kv_format(h, 2) != 0
    x = emb.to(torch.bfloat16).contiguous()
    full = torch.zeros((1, lens[0], m.opt_cfg.hidden_size), device=cuda, dtype=torch.float32)
    assert lib.gill_opt_forward_cached(h, N.ptr(x), 1, lens[0], 0, N.ptr(full), N.current_stream()) != 0
    assert b"e4m3" in lib.gill_last_error()
    idt = ids[:1].to(cuda).contiguous()
    assert lib.gill_opt_prefill_ids(h, N.ptr(idt), 1, ids.shape[1], None, 0, N.ptr(full), N.current_stream()) != 0
    assert b"e4m3" in lib.gill_last_error()
    torch.cuda.synchronize()
    assert bool((full == 0).all()), "a refused entry wrote something"
    # a change of the format drops the handle: an open session goes stale
    s = m.open_session(2, 64)
    s.extend([0], ids=[[2, 5, 6]])
    m.quantize_kv("bf16")
    with pytest.raises(StaleSessionError):
      s.generate([0])
    m.quantize_kv("fp8")
    with pytest.raises(StaleSessionError):
      s.extend([0], ids=[[7]])
