"""The ragged decision (gill_opt_pick_token_ragged: every row its own step count, length and [IMG] forcing state) on crafted logits,
exactly: no model forward, no tolerance.  The state is the int32 block of include/gill_amd.h ("ragged decode state"): len, step,
forced, n_tok, row_id, flags per row, then the count of active rows."""
import ctypes as C

import pytest
import torch

import decode_sample_util as U
from gill_amd import _native as N
from gill_amd import synth
from test_decode_sample_gpu import IMG, NEG_INF, OTHER, V, _draw, _rule, _sampler

pytestmark = pytest.mark.gpu
LEN, STEP, FORCED, NTOK, ROW_ID, FLAGS = range(6)
LD = 24


@pytest.fixture(scope="module")
def gill125(cuda):
  import ragged_decode_util as R
  return R.gill125_rig(cuda)


class _Machine:
  """B rows of ragged decode state on the device, stepped by gill_opt_pick_token_ragged."""

  def __init__(self, m, B, lens, steps=None, row_ids=None, active=None):
    self.m, self.B = m, B
    self.h = m._opt_native(8, 64)
    self.dev = torch.device("cuda:0")
    st = torch.zeros(6 * B + 1, dtype=torch.int32)
    st[LEN * B:(LEN + 1) * B] = torch.tensor(lens)
    if steps is not None:
      st[STEP * B:(STEP + 1) * B] = torch.tensor(steps)
    st[ROW_ID * B:(ROW_ID + 1) * B] = torch.tensor(row_ids if row_ids is not None else list(range(B)))
    st[6 * B] = B if active is None else active
    self.st = st.to(self.dev)
    self.tokens = torch.full((B, LD), -7, device=self.dev, dtype=torch.int64)
    self.nxt = torch.full((B, m.opt_cfg.hidden_size), 9.0, device=self.dev, dtype=torch.bfloat16)

  def call(self, x, rule_args, max_steps, sampler=None):
    """One decision on logits x (B, V) (host); -> the logits after the call (host)."""
    got = x.to(self.dev).contiguous()
    N.check(N.lib().gill_opt_pick_token_ragged(self.h, N.ptr(got), self.B, C.byref(_rule(*rule_args)), max_steps,
                                               C.byref(sampler) if sampler is not None else None, N.ptr(self.st), N.ptr(self.tokens), LD,
                                               N.ptr(self.nxt), N.current_stream()))
    torch.cuda.synchronize()
    return got.cpu()

  def field(self, f):
    return self.st[f * self.B:(f + 1) * self.B].cpu().tolist()

  @property
  def active(self):
    return int(self.st[6 * self.B])

  def toks(self, b):
    return self.tokens[b, :self.field(NTOK)[b]].cpu().tolist()


def _peaked(B, peaks, seed, runner_up=None):
  """(B, V) small noise with row b's maximum at peaks[b] (and, optionally, a second place at runner_up[b])."""
  g = torch.Generator().manual_seed(seed)
  x = torch.randn((B, V), generator=g)
  for b, c in enumerate(peaks):
    if runner_up is not None:
      x[b, runner_up[b]] = 20.0
    x[b, c] = 30.0
  return x


RULE = (IMG, IMG, 0, 0, 1.0, 1.0, NEG_INF)


def test_forced_block_takes_eight_calls_of_its_row_only(cuda, gill125):
  m = gill125.model
  B = 3
  mc = _Machine(m, B, lens=[10, 20, 30])
  want = [[], [], []]
  for it in range(2):                                   # decisions 0 and 1: plain tokens
    mc.call(_peaked(B, [100 + it, 200 + it, 300 + it], it), RULE, 16)
    for b in range(B):
      want[b].append(100 * (b + 1) + it)
  x = _peaked(B, [102, IMG[0], 302], 2)                   # decision 2: row 1 picks [IMG0]
  mc.call(x, RULE, 16)
  want[0].append(102); want[1].append(IMG[0]); want[2].append(302)
  assert mc.field(STEP) == [3, 3, 3] and mc.field(FORCED) == [0, 1, 0]
  for j in range(1, 8):                                 # the next seven calls: [IMG1..7] whatever the logits hold
    x = _peaked(B, [400 + j, 500 + j, 600 + j], 10 + j)
    after = mc.call(x, RULE, 16)
    assert torch.equal(after[1], x[1]), "a forcing row's logits must not be touched"
    want[0].append(400 + j); want[1].append(IMG[j]); want[2].append(600 + j)
    assert mc.field(STEP) == [3 + j, 3, 3 + j], "the forcing row's step stands still, the others decide"
    assert mc.field(FORCED) == [0, (j + 1) % 8, 0]
  assert mc.field(NTOK) == [10, 10, 10] and mc.field(LEN) == [20, 30, 40] and mc.field(FLAGS) == [0, 0, 0]
  mc.call(_peaked(B, [700, 701, 702], 30), RULE, 16)     # row 1 decides again
  want[0].append(700); want[1].append(701); want[2].append(702)
  assert mc.field(STEP) == [11, 4, 11]
  for b in range(B):
    assert mc.toks(b) == want[b]
  assert (mc.tokens[:, 11:] == -7).all() and mc.active == B
  # the embeddings of the last ids
  assert torch.equal(mc.nxt, m.input_embeddings(torch.tensor([700, 701, 702], device=cuda)).bfloat16())


def test_min_word_tokens_acts_on_each_rows_own_step(cuda, gill125):
  m = gill125.model
  mc = _Machine(m, 2, lens=[5, 6])
  both = lambda seed: _peaked(2, [IMG[0], IMG[0]], seed, runner_up=[900, 901])       # noqa: E731: [IMG0] on top in both rows
  rule2 = (IMG, IMG, 0, 2, 1.0, 1.0, NEG_INF)
  for it in range(2):                                   # steps 0, 1 < 2: [IMG] suppressed, the runner-up is picked
    mc.call(both(it), rule2, 32)
  assert mc.toks(0) == [900, 900] and mc.toks(1) == [901, 901]
  mc.call(_peaked(2, [IMG[0], 777], 3), rule2, 32)      # step 2: row 0 opens a block, row 1 goes on
  for j in range(1, 8):
    mc.call(_peaked(2, [50, 800 + j], 4 + j), rule2, 32)
  assert mc.field(STEP) == [3, 10] and mc.field(FORCED) == [0, 0] and mc.toks(0)[2:] == IMG
  # ten calls in, min_word_tokens = 6: row 0 (3 decisions) is still under it, row 1 (10) is not
  rule6 = (IMG, IMG, 0, 6, 1.0, 1.0, NEG_INF)
  after = mc.call(both(20), rule6, 32)
  assert mc.toks(0)[-1] == 900 and mc.toks(1)[-1] == IMG[0]
  assert mc.field(FORCED) == [0, 1] and mc.field(STEP) == [4, 11]
  assert after[0, IMG[0]] == NEG_INF and after[1, IMG[0]] == 30.0 and (after[:, IMG[1:]] == NEG_INF).all()


def test_finished_rows_emit_nothing_and_keep_their_length(cuda, gill125):
  m = gill125.model
  mc = _Machine(m, 2, lens=[4, 17], steps=[0, 2], active=1)       # row 1 has taken its 2 decisions
  for it in range(3):
    x = _peaked(2, [60 + it, 70 + it], it)
    after = mc.call(x, RULE, 2)
    assert torch.equal(after[1], x[1])
    assert mc.active == (1 if it == 0 else 0)
  assert mc.field(NTOK) == [2, 0] and mc.field(LEN) == [6, 17] and mc.field(STEP) == [2, 2]
  assert mc.toks(0) == [60, 61] and (mc.tokens[1] == -7).all()
  assert (mc.nxt[1].float() == 9.0).all(), "a finished row's next_embeds row must stay what it was"
  # a block opened by the last decision is still emitted to its end, and the row leaves the count after its last id
  mc = _Machine(m, 1, lens=[3])
  mc.call(_peaked(1, [IMG[0]], 5), RULE, 1)
  assert mc.active == 1
  for j in range(1, 8):
    mc.call(_peaked(1, [33], 6), RULE, 1)
    assert mc.active == (1 if j < 7 else 0)
  mc.call(_peaked(1, [33], 7), RULE, 1)
  assert mc.toks(0) == IMG and mc.field(LEN) == [11] and mc.field(STEP) == [1]


def test_img0_with_ret_not_gen_sets_the_error_flag(cuda, gill125):
  m = gill125.model
  mc = _Machine(m, 2, lens=[4, 4])
  mc.call(_peaked(2, [IMG[0], 55], 1), (IMG, OTHER, 0, 0, 1.0, 1.0, NEG_INF), 8)
  assert mc.field(FLAGS) == [1, 0] and mc.field(FORCED) == [0, 0]
  # through the model: ret != gen and a scale that makes [IMG0] certain
  ids = synth.synthetic_prompt_ids(2, 9, seed=13)[:, :9].to(cuda)
  saved = m.gen_token_idx
  try:
    m.gen_token_idx = list(OTHER)
    with pytest.raises(AssertionError):
      m.generate_batch(ids=ids, lengths=[9, 6], max_len=2, ret_scale_factor=1e5)
  finally:
    m.gen_token_idx = saved


def test_greedy_and_seeded_picks_equal_the_one_sequence_entries(cuda, gill125):
  """Row b of the ragged call == gill_opt_pick_token / gill_opt_draw_token at B = 1 on that row, with row0 = the row's id and draw =
  the row's decision count; tokens, post-rule logits and embedding rows bit for bit."""
  m = gill125.model
  h = m._opt_native(8, 64)
  x = U.operator_logits()[:5].clone()
  x[3, IMG[0]] = 80.0                                   # one row picks [IMG0]
  steps, rows = [0, 3, 5, 1, 2], [4, 9, 2, 0, 7]
  for mwt, rs in [(0, 1.0), (4, 3.5)]:
    rule_args = (IMG, IMG, 0, mwt, rs, 1.0, NEG_INF)
    for sampler in (None, (0.7, 1.0), (1.3, 0.9)):
      mc = _Machine(m, 5, lens=[7] * 5, steps=steps, row_ids=rows)
      sm = _sampler(77, 0, 0, *sampler) if sampler else None
      after = mc.call(x, rule_args, 32, sm)
      got = [mc.toks(b)[0] for b in range(5)]
      for b in range(5):
        one_rule = (IMG, IMG, steps[b], mwt, rs, 1.0, NEG_INF)
        if sampler:
          d = _draw(m, h, x[b:b + 1], one_rule, _sampler(77, steps[b], rows[b], *sampler), ld=12, col=0, rows=8)
          tok, logits, nxt = d.tok[0], d.logits.cpu(), d.nxt[0, 0]
        else:
          gl = x[b:b + 1].to(cuda).contiguous()
          tk = torch.full((1, 12), -7, device=cuda, dtype=torch.int64)
          n_out = torch.zeros(1, device=cuda, dtype=torch.int32)
          nx = torch.zeros((1, 8, m.opt_cfg.hidden_size), device=cuda, dtype=torch.bfloat16)
          N.check(N.lib().gill_opt_pick_token(h, N.ptr(gl), 1, C.byref(_rule(*one_rule)), N.ptr(tk), 12, 0, N.ptr(n_out), N.ptr(nx),
                                              N.current_stream()))
          torch.cuda.synchronize()
          tok, logits, nxt = int(tk[0, 0]), gl.cpu(), nx[0, 0]
        assert got[b] == tok, (mwt, sampler, b, got[b], tok)
        assert torch.equal(after[b].view(torch.int32), logits[0].view(torch.int32))
        assert torch.equal(mc.nxt[b], nxt)
      assert (got[3] == IMG[0]) == (steps[3] >= mwt)
      # next_embeds rows are gill_opt_embed's
      emb = torch.empty_like(mc.nxt)
      idt = torch.tensor(got, device=cuda, dtype=torch.int64)
      N.check(N.lib().gill_opt_embed(h, N.ptr(idt), 5, N.ptr(emb), N.current_stream()))
      torch.cuda.synchronize()
      assert torch.equal(mc.nxt, emb)
