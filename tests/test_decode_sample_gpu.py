"""The seeded draw on the device (gill_opt_draw_token / gill_opt_sample_token, GILLModel.generate(seed=...)) against the numpy
restatement of tests/decode_sample_util.py: the token is the fp64 argmax of the race keys except at near ties (bar measured by
tools/decode_sample_tolerance.py), the kept set is gill_opt_filter_logits', and the result is repeatable, batch-invariant and
keyed by (seed, row, draw).  V = 50274 is no multiple of 4 or 1024: the last Philox block and the last register column are partial."""
import ctypes as C
import itertools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import decode_sample_util as U
from gill_amd import _native as N
from gill_amd import synth

pytestmark = pytest.mark.gpu
V = U.OP_V
IMG = synth.IMG_TOKEN_IDS
OTHER = [50262, 50263, 50264, 50265, 50267, 120, 121, 122]   # a gen list that overlaps IMG in one id (not [IMG0])
NEG_INF = float("-inf")


def _bfw(sd):
  return {k: v.bfloat16().float() for k, v in sd.items()}


def _gill_opt125m(cuda):
  from gill_amd.models import GILL
  tok = synth.HashTokenizer()
  ocfg = synth.OptConfig(vocab_size=50274, hidden_size=768, num_layers=12, num_heads=12, ffn_dim=3072)
  args = SimpleNamespace(freeze_lm=True, freeze_vm=True, opt_version="facebook/opt-125m", visual_encoder="openai/clip-vit-base-patch16",
                         n_visual_tokens=4, ret_emb_dim=256, gen_emb_dim=768, text_emb_layers=[-1], text_fc_mode="gill_mapper",
                         ret_text_fc_mode="linear", num_tokens=8, num_clip_tokens=77, retrieval_token_idx=synth.IMG_TOKEN_IDS,
                         gen_token_idx=synth.IMG_TOKEN_IDS, opt_state_dict=_bfw(synth.opt_state_dict(ocfg, seed=5)))
  g = GILL(tok, args, load_sd=False)
  g.model.gen_text_hidden_fcs[0].load_state_dict(_bfw(synth.mapper_state_dict(synth.MapperConfig(in_dim=768), seed=7)), strict=True)
  g = g.eval()
  g = g.bfloat16()
  g = g.cuda()
  return g


@pytest.fixture(scope="module")
def gill125(cuda):
  return _gill_opt125m(cuda)


@pytest.fixture(scope="module")
def tol():
  return U.load_tolerance()


@pytest.fixture(scope="module")
def op_logits():
  """the operator test's 64 rows, computed once and never modified (every user clones or uploads a copy)"""
  return U.operator_logits()


def _rule(ret, gen, step, mwt, rs, gs, fv):
  r = N.gill_decode_rule()
  r.n_ret, r.n_gen = len(ret), len(gen)
  for j, v in enumerate(ret):
    r.ret_ids[j] = v
  for j, v in enumerate(gen):
    r.gen_ids[j] = v
  r.step, r.min_word_tokens, r.ret_eq_gen = step, mwt, int(ret == gen)
  r.ret_scale, r.gen_scale, r.filter_value = rs, gs, fv
  return r


NO_RULE = ([], [], 0, 0, 1.0, 1.0, NEG_INF)          # no ids: the rule changes nothing


def _sampler(seed, draw, row0, t, p):
  s = N.gill_decode_sampler()
  s.seed, s.draw, s.row0, s.temperature, s.top_p = seed, draw, row0, t, p
  return s


def _host_rule(logits, ret, gen, i, min_word_tokens, ret_scale_factor, gen_scale_factor, filter_value):
  """models.py:476-489 as the host decision runs it (CPU tensor, in place)."""
  logits[:, ret[1:]] = filter_value
  logits[:, gen[1:]] = filter_value
  if (ret or gen) and ret[0] != -1 and gen[0] != -1:
    if i < min_word_tokens:
      logits[:, ret] = filter_value
      logits[:, gen] = filter_value
    else:
      if ret_scale_factor > 1:
        logits[:, ret[0]] = logits[:, ret[0]].abs() * ret_scale_factor
      if gen_scale_factor > 1:
        logits[:, gen[0]] = logits[:, gen[0]].abs() * gen_scale_factor
  return logits


def _same_bits(a, b):
  """bit-equal where not NaN, NaN at the same places"""
  a, b = a.cpu(), b.cpu()
  na, nb = torch.isnan(a), torch.isnan(b)
  return torch.equal(na, nb) and torch.equal(a[~na].view(torch.int32), b[~nb].view(torch.int32))


class _Drawn(SimpleNamespace):
  pass


def _draw(m, h, x, rule_args, sampler, ld=4, col=1, rows=1):
  """gill_opt_draw_token on a device copy of x (B, V): tokens column `col` (host list), the whole token buffer, *n_out, the
  embedding rows and the logits after the call."""
  cuda = torch.device("cuda:0")
  D = m.opt_cfg.hidden_size
  B = x.shape[0]
  got = x.to(cuda).contiguous()
  tokens = torch.full((B, ld), -7, device=cuda, dtype=torch.int64)
  n_out = torch.zeros(1, device=cuda, dtype=torch.int32)
  nxt = torch.zeros((B, rows, D), device=cuda, dtype=torch.bfloat16)
  N.check(N.lib().gill_opt_draw_token(h, N.ptr(got), B, C.byref(_rule(*rule_args)), C.byref(sampler), N.ptr(tokens), ld, col,
                                      N.ptr(n_out), N.ptr(nxt), N.current_stream()))
  torch.cuda.synchronize()
  return _Drawn(tok=tokens[:, col].cpu().tolist(), tokens=tokens.cpu(), n=int(n_out[0]), nxt=nxt, logits=got)


def _kept(h, xd, t, p):
  """the kept set of gill_opt_filter_logits(reciprocal = 0) on the device logits xd; None at top_p == 1 (every token)"""
  if p >= 1.0:
    return None
  out = torch.empty_like(xd)
  N.check(N.lib().gill_opt_filter_logits(h, N.ptr(xd), N.ptr(out), xd.shape[0], t, p, NEG_INF, 0, N.current_stream()))
  return (out != NEG_INF).cpu().numpy()


def test_operator_matches_restatement(cuda, gill125, tol, op_logits):
  m = gill125.model
  h = m._opt_native(8, 64)
  rule_args = (IMG, IMG, 0, 1, 1.0, 1.0, NEG_INF)            # step 0 < min_word_tokens: the eight [IMG] columns are -inf
  post = _host_rule(op_logits.clone(), *rule_args)
  postd = post.to(cuda)
  near = total = 0
  for t, p in itertools.product(U.OP_TEMPERATURES, U.OP_TOP_PS):
    keep = _kept(h, postd, t, p)
    y = U.divide(post.numpy(), t)
    for draw in U.OP_DRAWS:
      d = _draw(m, h, op_logits, rule_args, _sampler(U.OP_SEED, draw, 0, t, p))
      assert d.n == 1 and _same_bits(d.logits, post)           # the logits keep the post-rule, pre-temperature values
      tok = np.array(d.tok)
      assert ((tok >= 0) & (tok < V)).all()
      assert np.isfinite(y[np.arange(64), tok]).all()
      if keep is not None:
        assert keep[np.arange(64), tok].all(), (t, p, draw)    # the two kernels share the kept set
      verdicts = U.judge_rows(tok, y, U.OP_SEED, 0, draw, keep, tol)
      assert "wrong" not in verdicts, (t, p, draw, [b for b, v in enumerate(verdicts) if v == "wrong"])
      near += verdicts.count("near")
      total += len(verdicts)
      assert torch.equal(d.nxt[:, 0], m.input_embeddings(torch.tensor(d.tok, device=cuda)).bfloat16())
  print(f"seeded draw: {near} of {total} draws excused as near ties (tol {tol:.3e})")
  assert total == 64 * 2 * 3 * 4
  assert near * 20 <= total


def test_top_p_of_one_token_is_argmax(cuda, gill125, op_logits):
  m = gill125.model
  h = m._opt_native(8, 64)
  for t in (0.7, 1.3):
    d = _draw(m, h, op_logits, NO_RULE, _sampler(3, 0, 0, t, 1e-6))
    assert d.tok == torch.argmax(op_logits, dim=-1).tolist()


def test_low_temperature_does_not_overflow(cuda, gill125, tol):
  m = gill125.model
  h = m._opt_native(8, 64)
  g = torch.Generator().manual_seed(21)
  x = torch.randn((8, V), generator=g) * 10
  x[0, 17], x[1, 50273], x[2, 3] = 87.0, 87.0, -87.0
  x[3, 1000], x[3, 2000] = 86.9, 87.0                       # two columns 0.1 apart: exp(-2) of the mass at T = 0.05
  assert float(x.max()) >= 87 and float(x.min()) <= -87
  assert torch.isinf((x / 0.05).exp()).any()                 # what the torch path hands to multinomial
  y = U.divide(x.numpy(), 0.05)
  seen = set()
  for draw in range(4):
    d = _draw(m, h, x, NO_RULE, _sampler(11, draw, 0, 0.05, 1.0))
    assert all(0 <= t < V for t in d.tok)
    assert "wrong" not in U.judge_rows(d.tok, y, 11, 0, draw, None, tol)
    assert d.tok[0] == 17 and d.tok[1] == 50273
    seen.add(d.tok[3])
  assert seen <= {1000, 2000}


def test_repeatable_and_keyed_by_seed_and_draw(cuda, gill125, op_logits):
  m = gill125.model
  h = m._opt_native(8, 64)
  rule_args = (IMG, IMG, 0, 0, 1.0, 1.0, NEG_INF)
  a = _draw(m, h, op_logits, rule_args, _sampler(77, 2, 0, 1.3, 0.9))
  b = _draw(m, h, op_logits, rule_args, _sampler(77, 2, 0, 1.3, 0.9))
  assert a.tok == b.tok and _same_bits(a.logits, b.logits) and torch.equal(a.nxt, b.nxt)
  for other in [_sampler(78, 2, 0, 1.3, 0.9), _sampler(77 + 2 ** 32, 2, 0, 1.3, 0.9), _sampler(77, 3, 0, 1.3, 0.9),
                _sampler(77, 2, 1, 1.3, 0.9)]:
    assert _draw(m, h, op_logits, rule_args, other).tok != a.tok


def test_batch_invariant(cuda, gill125, op_logits):
  m = gill125.model
  h = m._opt_native(8, 64)
  for t, p in [(0.7, 1.0), (1.3, 0.9)]:
    big = _draw(m, h, op_logits[:12], NO_RULE, _sampler(5, 1, 0, t, p))
    small = _draw(m, h, op_logits[5:9], NO_RULE, _sampler(5, 1, 5, t, p))
    assert big.tok[5:9] == small.tok
    one = _draw(m, h, op_logits[7:8], NO_RULE, _sampler(5, 1, 7, t, p), ld=12, rows=8)      # B == 1: the forcing kernel path
    assert one.tok == big.tok[7:8]


def _planted_logits(seed):
  g = torch.Generator().manual_seed(seed)
  x = torch.randn((6, V), generator=g) * 3
  x[1, 777] = x[1, 40000] = 50.0                  # two columns share the maximum
  x[1, IMG[0]] = 50.0
  x[2, 1234] = float("nan")
  x[2, 99] = float("nan")                         # the first NaN wins
  x[2, 5] = 1e30
  x[3, :] = NEG_INF                               # all -inf: index 0
  x[4, ::7] = 3e38                                # huge values: x / 0.7 and |x| * scale overflow to inf
  x[4, IMG[0]] = -3e38
  x[5, IMG[0]] = 10.0                             # the max on [IMG0]
  x[5, OTHER[0]] = -9.0
  return x


def test_rule_nonfinite_rows_and_embeddings(cuda, gill125, tol):
  m = gill125.model
  h = m._opt_native(8, 64)
  x0 = _planted_logits(1)
  n, row3 = 0, set()
  for (step, mwt), (rs, gs), fv, eq in [((0, 0), (1.0, 1.0), NEG_INF, True), ((3, 5), (3.5, 2.0), -123.5, True),
                                        ((5, 5), (3.5, 2.0), NEG_INF, False), ((5, 5), (1.0, 1e5), -123.5, True)]:
    ret, gen = IMG, (IMG if eq else OTHER)
    rule_args = (ret, gen, step, mwt, rs, gs, fv)
    post = _host_rule(x0.clone(), *rule_args)
    t, p, seed = 0.7, (1.0 if n % 2 == 0 else 0.9), 40 + n
    y = U.divide(post.numpy(), t)
    no_draw = [b for b in range(6) if np.isnan(y[b]).any() or not np.isfinite(y[b].max())]
    assert 2 in no_draw and 4 in no_draw, (rule_args, no_draw)      # the NaN row and the 3e38 row (x / 0.7 = inf)
    row3.add(3 in no_draw)       # all -inf, unless the rule plants finite filter values (then it draws) or |-inf| * scale = inf
    keep = None
    if p < 1.0:                                   # the filter kernel's set on the rows that draw (the others never read it)
      keep = np.ones((6, V), dtype=bool)
      rows = [b for b in range(6) if b not in no_draw]
      keep[rows] = _kept(h, post[rows].to(cuda), t, p)
    d = _draw(m, h, x0, rule_args, _sampler(seed, step, 0, t, p))
    assert _same_bits(d.logits, post), rule_args
    verdicts = U.judge_rows(d.tok, y, seed, 0, step, keep, tol)
    assert "wrong" not in verdicts, (rule_args, verdicts)
    for b in no_draw:                              # no finite maximum: torch.argmax's pick on y, no draw
      assert d.tok[b] == U.argmax_rule(y[b]) == int(torch.argmax(torch.from_numpy(y[b])))
    assert d.n == 1 and (d.tokens[:, 0] == -7).all() and (d.tokens[:, 2:] == -7).all()
    assert torch.equal(d.nxt[:, 0], m.input_embeddings(torch.tensor(d.tok, device=cuda)).bfloat16())
    # B == 1, each row alone under its own row id: the same token, and the forcing where the pick is [IMG0]
    for b in range(6):
      d1 = _draw(m, h, x0[b:b + 1], rule_args, _sampler(seed, step, b, t, p), ld=12, col=2, rows=8)
      assert _same_bits(d1.logits, post[b:b + 1])
      assert d1.tok[0] == d.tok[b] or d.tok[b] == ret[0], (rule_args, b)
      if d.tok[b] == ret[0]:
        assert d1.n == (8 if eq else -1)
        if eq:
          assert d1.tokens[0, 2:10].tolist() == IMG and (d1.tokens[0, :2] == -7).all() and (d1.tokens[0, 10:] == -7).all()
          assert torch.equal(d1.nxt, m.input_embeddings(torch.tensor(IMG, device=cuda)[None]).bfloat16())
      else:
        assert d1.n == 1 and (d1.tokens[0, :2] == -7).all() and (d1.tokens[0, 3:] == -7).all()
        assert torch.equal(d1.nxt[0, 0], m.input_embeddings(torch.tensor(d.tok[b:b + 1], device=cuda)).bfloat16()[0])
    n += 1
  assert n == 4 and row3 == {True, False}


def test_img_forcing_is_certain_under_a_large_scale(cuda, gill125):
  m = gill125.model
  h = m._opt_native(8, 64)
  g = torch.Generator().manual_seed(8)
  x = torch.randn((1, V), generator=g)
  x[0, IMG[0]] = -1.0                                        # |x| * 1e5 = 1e5: every other key underflows to 0
  for draw in range(3):
    d = _draw(m, h, x, (IMG, IMG, 0, 0, 1.0, 1e5, NEG_INF), _sampler(1, draw, 0, 1.3, 0.95), ld=12, col=3, rows=8)
    assert d.n == 8
    assert d.tokens[0, 3:11].tolist() == IMG and (d.tokens[0, :3] == -7).all() and d.tokens[0, 11] == -7
    assert torch.equal(d.nxt, m.input_embeddings(torch.tensor(IMG, device=cuda)[None]).bfloat16())
  d = _draw(m, h, x, (IMG, OTHER, 0, 0, 1e5, 1.0, NEG_INF), _sampler(1, 0, 0, 1.3, 0.95), ld=12, col=0, rows=8)
  assert d.n == -1                                           # [IMG0] with ret != gen: the reference's AssertionError


def test_bad_arguments_return_errors(cuda, gill125):
  m = gill125.model
  h = m._opt_native(8, 64)
  lib = N.lib()
  D = m.opt_cfg.hidden_size
  x = torch.zeros((1, V), device=cuda)
  tokens = torch.zeros((1, 12), device=cuda, dtype=torch.int64)
  n_out = torch.zeros(1, device=cuda, dtype=torch.int32)
  nxt = torch.zeros((1, 8, D), device=cuda, dtype=torch.bfloat16)
  hidden = torch.zeros((1, 2, D), device=cuda)
  rule = _rule(IMG, IMG, 0, 0, 1.0, 1.0, NEG_INF)
  s = N.current_stream()

  def draw(sm, logits=x, tok=tokens, ld=12, col=0, n=n_out, e=nxt, r=rule):
    return lib.gill_opt_draw_token(h, N.ptr(logits), 1, None if r is None else C.byref(r), None if sm is None else C.byref(sm),
                                   N.ptr(tok), ld, col, N.ptr(n), N.ptr(e), s)

  def sample(sm, hid=hidden, logits=x, tok=tokens, ld=12, col=0):
    return lib.gill_opt_sample_token(h, N.ptr(hid), 1, 2, C.byref(rule), None if sm is None else C.byref(sm), N.ptr(logits),
                                     N.ptr(tok), ld, col, N.ptr(n_out), N.ptr(nxt), s)

  good = _sampler(1, 0, 0, 0.7, 0.9)
  assert draw(good) == 0 and sample(good) == 0
  for bad in [_sampler(1, 0, 0, 0.0, 0.9), _sampler(1, 0, 0, -1.0, 0.9), _sampler(1, 0, 0, float("nan"), 0.9),
              _sampler(1, 0, 0, 0.7, 0.0), _sampler(1, 0, 0, 0.7, -0.5), _sampler(1, 0, 0, 0.7, 1.5),
              _sampler(1, -1, 0, 0.7, 0.9), _sampler(1, 0, -1, 0.7, 0.9), None]:
    assert draw(bad) != 0 and lib.gill_last_error()
    assert sample(bad) != 0 and lib.gill_last_error()
  assert draw(good, logits=None) != 0 and draw(good, tok=None) != 0 and draw(good, n=None) != 0 and draw(good, e=None) != 0
  assert draw(good, r=None) != 0
  assert sample(good, hid=None) != 0 and sample(good, logits=None) != 0 and sample(good, tok=None) != 0
  assert draw(good, col=5) != 0 and sample(good, col=5) != 0          # B == 1: the buffer must hold the whole forced block
  assert draw(good, col=-1) != 0
  assert draw(good, col=4) == 0
  torch.cuda.synchronize()
  # a vocabulary the row-in-registers kernel cannot hold
  ocfg = synth.OptConfig(vocab_size=65600, hidden_size=128, num_layers=2, num_heads=2, ffn_dim=256, max_positions=128)
  cfg = N.gill_opt_config(vocab_size=ocfg.vocab_size, hidden_size=ocfg.hidden_size, num_layers=ocfg.num_layers, num_heads=ocfg.num_heads,
                          ffn_dim=ocfg.ffn_dim, max_positions=ocfg.max_positions, max_batch=8, max_seq=64)
  arr, keep = N.make_tensor_table(_bfw(synth.opt_state_dict(ocfg, seed=1)), cuda)
  wide = C.c_void_p()
  N.check(lib.gill_opt_create(C.byref(wide), C.byref(cfg), arr, len(keep)))
  try:
    xw = torch.zeros((1, 65600), device=cuda)
    nw = torch.zeros((1, 8, 128), device=cuda, dtype=torch.bfloat16)
    none = _rule([], [], 0, 0, 1.0, 1.0, NEG_INF)
    for p in (1.0, 0.9):
      sm = _sampler(1, 0, 0, 0.7, p)
      assert lib.gill_opt_draw_token(wide, N.ptr(xw), 1, C.byref(none), C.byref(sm), N.ptr(tokens), 12, 0, N.ptr(n_out), N.ptr(nw), s) != 0
      assert b"65536" in lib.gill_last_error()
  finally:
    torch.cuda.synchronize()
    lib.gill_opt_destroy(wide)


def _generate_seeded(m, *a, **k):
  cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state()
  res = m.generate(*a, **k)
  assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(), dev_state)
  return res


@pytest.mark.parametrize("use_kv_cache", [True, False])
@pytest.mark.parametrize("p", [0.9, 1.0])
def test_generate_seeded(cuda, gill125, tol, p, use_kv_cache):
  m = gill125.model
  ids = synth.synthetic_prompt_ids(2, 9, seed=13)[:, :9].to(cuda)
  emb = m.input_embeddings(ids)
  h = None
  near = total = 0
  for e, waits in [(emb, 0), (emb[:1], 6)]:
    B = e.shape[0]
    kw = dict(temperature=4.0, top_p=p, use_kv_cache=use_kv_cache)
    out, embs, logits = _generate_seeded(m, e, 6, seed=7, **kw)
    assert m._decode_host_waits == waits
    out2, embs2, logits2 = _generate_seeded(m, e, 6, seed=7, **kw)
    assert torch.equal(out, out2) and out.dtype == torch.int64 and out.is_cuda and out.shape[0] == B and out.shape[1] >= 6
    assert len(embs) == len(logits) == 6 and all(torch.equal(a, b) for a, b in zip(logits, logits2))
    assert all(torch.equal(a, b) for a, b in zip(embs, embs2))
    for l in logits:
      assert l.shape == (B, V) and l.dtype == torch.float32
      assert l.device.type == ("cpu" if p == 1.0 else "cuda")      # :471-472
    if p == 1.0:            # (at top_p 0.9 this model keeps one token in most steps: nothing left for a seed to decide)
      out3, _, _ = _generate_seeded(m, e, 6, seed=8, **kw)
      assert not torch.equal(out, out3)
    # step 0 sees the same prompt as the unseeded path: the same output_logits, bit for bit
    _, _, l0 = m.generate(e, 1, **kw)
    assert l0[0].device == logits[0].device and torch.equal(l0[0], logits[0])
    # every step's token is the draw of that step's output_logits
    h = m._opt_native(B, 64)
    outh, col = out.cpu(), 0
    for i, l in enumerate(logits):
      keep = _kept(h, l.to(cuda), 4.0, p)
      tok = outh[:, col].tolist()
      verdicts = U.judge_rows(tok, U.divide(l.cpu().numpy(), 4.0), 7, 0, i, keep, tol)
      assert "wrong" not in verdicts, (B, i, tok, verdicts)
      near += verdicts.count("near")
      total += B
      if B == 1 and tok[0] == IMG[0]:
        assert outh[0, col:col + 8].tolist() == IMG
        col += 8
      else:
        col += 1
    assert col == out.shape[1]
  assert near * 20 <= total


def test_generate_seeded_rows_do_not_depend_on_the_batch(cuda, gill125):
  """B = 12 (the lm_head beyond 8 rows): every row draws what it draws in a batch of 2 — a row's stream is keyed by its own
  (seed, row, step) and its own logits; min_word_tokens keeps [IMG] out so that B == 1's forcing never applies."""
  m = gill125.model
  ids = synth.synthetic_prompt_ids(12, 9, seed=17)[:, :9].to(cuda)
  emb = m.input_embeddings(ids)
  out, embs, logits = m.generate(emb, 4, temperature=4.0, top_p=0.9, seed=7, min_word_tokens=4)
  assert m._decode_host_waits == 0
  assert out.shape == (12, 4) and len(embs) == 4 and logits[-1].shape == (12, V) and logits[-1].is_cuda
  assert ((out >= 0) & (out < V)).all()
  out2, _, l2 = m.generate(emb[:2], 4, temperature=4.0, top_p=0.9, seed=7, min_word_tokens=4)
  assert torch.equal(l2[0], logits[0][:2])                   # a row's logits do not depend on B (gill_opt_last_logits)
  assert out2[:, 0].tolist() == out[:2, 0].tolist()


def test_seed_arguments(cuda, gill125):
  m = gill125.model
  ids = synth.synthetic_prompt_ids(2, 9, seed=13)[:, :9].to(cuda)
  emb = m.input_embeddings(ids)
  # temperature 0 with a seed is plain greedy
  og, _, lg = m.generate(emb, 3, min_word_tokens=3)
  os_, _, ls = m.generate(emb, 3, min_word_tokens=3, seed=5)
  assert torch.equal(og, os_) and all(torch.equal(a, b) for a, b in zip(lg, ls))
  with pytest.raises(ValueError):
    m.generate(emb, 2, temperature=0.0, top_p=0.9, seed=5)
  with pytest.raises(AssertionError, match="top_p should be above 0"):
    m.generate(emb, 2, temperature=1.0, top_p=0.0, seed=5)
  with pytest.raises(ValueError):
    m.generate(emb, 2, temperature=1.0, seed=-1)
  m.decode_on_device = False
  try:
    with pytest.raises(ValueError, match="decode_on_device"):
      m.generate(emb, 2, temperature=1.0, seed=5)
  finally:
    m.decode_on_device = True
  # the forced [IMG0] with ret != gen raises the reference's AssertionError through the count readback
  saved = m.gen_token_idx
  try:
    m.gen_token_idx = list(OTHER)
    with pytest.raises(AssertionError):
      m.generate(emb[:1], 2, temperature=1.0, top_p=0.9, ret_scale_factor=1e5, seed=5)
  finally:
    m.gen_token_idx = saved
  # a temperature the torch draw cannot take (exp overflows) is fine here
  out, _, _ = m.generate(emb, 3, temperature=0.05, top_p=0.95, seed=5)
  assert out.shape == (2, 3) and ((out >= 0) & (out < V)).all()


def test_public_api_hands_the_seed_through(cuda, gill125):
  text = "a synthetic prompt of five words"
  kw = dict(num_words=4, temperature=4.0, top_p=0.9, seed=3)
  cpu_state = torch.get_rng_state()
  a = gill125.generate_for_images_and_texts([text], **kw)
  b = gill125.generate_for_images_and_texts([text], **kw)
  assert isinstance(a[0], str) and a[0] == b[0] and len(a) == len(b)
  c = gill125.generate_for_images_and_texts([text], num_words=4, temperature=4.0, top_p=0.9, seed=4)
  d = gill125.generate_for_images_and_texts([text], num_words=4, temperature=4.0, top_p=0.9, seed=5)
  assert len({a[0], c[0], d[0]}) > 1                          # the seed reaches the draw
  assert torch.equal(torch.get_rng_state(), cpu_state)
