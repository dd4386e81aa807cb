"""The fused LM-head loss on the GPU: the operator (gill_op_lm_head_loss) against its fp64 restatement, the scoring pass of the OPT engine
(gill_opt_forward_loss) against gill_opt_img_hidden_ex / gill_opt_last_logits (bits) and the fp32 oracle (bars), and the three modes of
GILLModel.forward against the reference's forward restated on the oracle.  Inputs, restatements and bars: tests/lm_loss_util.py;
test_lm_loss_host.py shows on the CPU that these checks can fail."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import lm_loss_util as U
from gill_amd import synth

pytestmark = pytest.mark.gpu


def _shapes():
  from gill_amd import ops
  return U.operator_shapes(ops.lm_loss_geometry)


_CASES = {}


def _case(shape):
  from gill_amd import ops
  if shape not in _CASES:
    M, V, D = shape
    geom = ops.lm_loss_geometry(M, V, D)
    x, w, t = U.build_inputs(M, V, D, U.OP_SEED, geom)
    ref = U.reference(x, w, t, geom)
    assert U.ambiguous_rows(ref, t) == [], "a row of the inputs is threshold-ambiguous: pick another seed"      # before the GPU is touched
    _CASES[shape] = SimpleNamespace(geom=geom, x=x, w=w, t=t, ref=ref)
  return _CASES[shape]


def _run(c, cuda, rows=None):
  from gill_amd import ops
  x, t = (c.x, c.t) if rows is None else (c.x[:rows], c.t[:rows])
  lse, tgt, rank, summary = ops.lm_head_loss(x.to(cuda, torch.bfloat16), c.w.to(cuda, torch.bfloat16), t.to(cuda))
  return dict(lse=lse.cpu(), tgt=tgt.cpu(), rank=rank.cpu(), summary=summary.cpu())


@pytest.mark.parametrize("shape", _shapes(), ids=lambda s: "x".join(map(str, s)))
def test_operator_vs_fp64(cuda, shape):
  c = _case(shape)
  got = _run(c, cuda)
  U.assert_operator(f"lm_head_loss {shape}", got, c.ref, c.t)
  ignored = c.t == -100
  assert (got["rank"][ignored] == -1).all() and (got["lse"][ignored] == 0).all() and (got["tgt"][ignored] == 0).all()
  assert (got["rank"][~ignored] >= 0).all()
  # the loss of a row is never negative beyond rounding: tgt is one of the logits lse sums over
  slack = float((got["tgt"] - got["lse"]).max())
  print(f"[{shape}] max (tgt - lse) {slack:.3e}")
  assert slack <= 4e-6
  again = _run(c, cuda)
  for k in got:
    assert torch.equal(got[k], again[k]), f"two calls differ in {k}"


@pytest.mark.parametrize("shape,rows", [((129, 385, 768), 17), ((40, 50274, 768), 9), ((33, 2050, 4096), 1)], ids=["129of385", "40of50274", "33of2050"])
def test_first_rows_of_a_larger_batch_keep_their_bits(cuda, shape, rows):
  c = _case(shape)
  full, part = _run(c, cuda), _run(c, cuda, rows=rows)
  for k in ("lse", "tgt", "rank"):
    assert torch.equal(full[k][:rows], part[k]), f"{k} of the first {rows} rows depends on the batch"


def test_all_rows_ignored_and_bad_targets(cuda):
  from gill_amd import ops
  c = _case((17, 50, 128))
  x, w = c.x.to(cuda, torch.bfloat16), c.w.to(cuda, torch.bfloat16)
  lse, tgt, rank, summary = ops.lm_head_loss(x, w, torch.full((17,), -100, device=cuda))
  assert (rank == -1).all() and (lse == 0).all() and (tgt == 0).all()
  s = summary.cpu().tolist()
  assert s[0] != s[0] and s[1:] == [0.0, 0.0, 0.0], s      # torch's mean over no target: NaN
  for bad in (50, -1, -101):
    t = c.t.clone()
    t[0] = bad
    with pytest.raises(ValueError):
      ops.lm_head_loss(x, w, t.to(cuda))
  # unchecked, the library clamps into [0, V): row 0 is then scored against column V - 1
  t = c.t.clone()
  t[0] = 50
  got = ops.lm_head_loss(x, w, t.to(cuda), check=False)
  t[0] = 49
  want = ops.lm_head_loss(x, w, t.to(cuda))
  assert all(torch.equal(a, b) for a, b in zip(got, want))


# ---------------------------------------------------------------------------------------------------------------- engine
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

  def close(self):
    if self.h:
      self.N.lib().gill_opt_destroy(self.h)
      self.h = None


@pytest.fixture(scope="module")
def engine(cuda):
  cfg, sd, _, _, _ = U.engine_case(1)
  h = _Handle(sd, cfg, 4, 32, cuda)
  yield SimpleNamespace(h=h, cfg=cfg, sd=sd)
  h.close()


@pytest.mark.parametrize("B", [1, 3])
def test_engine_forward_loss(cuda, engine, B):
  N = engine.h.N
  cfg, sd = engine.cfg, engine.sd
  _, _, ids, full, last = U.engine_case(B)
  T, D, V = ids.shape[1], cfg.hidden_size, cfg.vocab_size
  emb = F.embedding(ids, sd["model.decoder.embed_tokens.weight"])
  extra = None
  if B == 3:      # two visual rows in place of two prompt tokens of row 1 (negative ids, as the interleaved prompts pass them)
    extra = U.bf(synth.normal("lm_loss_extra", (2, D), 7, 0.5))
    ids = ids.clone()
    ids[1, 2], ids[1, 3] = -2, -1
    emb = emb.clone()
    emb[1, 2], emb[1, 3] = extra[1], extra[0]
  ref = U.lm_scores(sd, cfg.num_layers, cfg.num_heads, emb, full)

  dev = cuda
  ids_d, full_d = ids.to(dev), full.to(dev)
  extra_d = extra.to(dev, torch.bfloat16) if extra is not None else None
  n_extra = 0 if extra is None else extra.shape[0]
  arr = (C.c_int32 * B)(*[int(v) for v in last.tolist()])
  new = lambda *s, dt=torch.float32: torch.empty(s, device=dev, dtype=dt)      # noqa: E731
  raw, embo = new(B, 8, D, dt=torch.bfloat16), new(B, 8, D, dt=torch.bfloat16)
  raw0, emb0 = new(B, 8, D, dt=torch.bfloat16), new(B, 8, D, dt=torch.bfloat16)
  tl, tr, summ = new(B, T - 1), new(B, T - 1, dt=torch.int32), new(4)
  ll, hid = new(B, V), new(B, T, D)
  with torch.cuda.device(dev):
    N.check(N.lib().gill_opt_img_hidden_ex(engine.h.h, N.ptr(ids_d), arr, B, T, 8, N.ptr(extra_d), n_extra, N.ptr(raw0), N.ptr(emb0), N.current_stream()))
    N.check(N.lib().gill_opt_forward_loss(engine.h.h, N.ptr(ids_d), arr, B, T, 8, N.ptr(extra_d), n_extra, N.ptr(full_d), N.ptr(raw), N.ptr(embo),
                                          N.ptr(tl), N.ptr(tr), N.ptr(summ), N.ptr(ll), N.ptr(hid), N.current_stream()))
    rows = torch.stack([hid[b, int(last[b]) - 1] for b in range(B)])[:, None, :].contiguous()      # (B, 1, D): each its own last position
    ll0 = new(B, V)
    N.check(N.lib().gill_opt_last_logits(engine.h.h, N.ptr(rows), B, 1, N.ptr(ll0), N.current_stream()))
  assert torch.equal(raw, raw0) and torch.equal(embo, emb0), "raw / emb differ from gill_opt_img_hidden_ex"
  assert torch.equal(ll, ll0), "last_logit_out differs from gill_opt_last_logits on that row"

  valid = full[:, 1:] != -100
  tl, tr, summ = tl.cpu(), tr.cpu(), summ.cpu().tolist()
  d_loss = abs(summ[0] - float(ref["loss"]))
  d_tok = float((tl - ref["token_loss"]).abs().max())
  d_hid = float((hid.cpu() - ref["hidden"]).norm() / ref["hidden"].norm())
  want_rank = ref["token_rank"]
  agree = [float((((tr < k) & valid) == ((want_rank < k) & valid)).float().mean()) for k in (1, 5)]
  print(f"[forward_loss B={B}] loss {summ[0]:.5f} oracle {float(ref['loss']):.5f} |d| {d_loss:.2e} (bar {U.LOSS_BAR:.1e})  max |token_loss d| {d_tok:.2e} "
        f"(bar {U.TOKEN_LOSS_BAR:.1e})  hidden rel-L2 {d_hid:.2e}  top-1 / top-5 verdicts agreeing {agree}")
  assert summ[1] == float(valid.sum())
  assert (tr[~valid] == -1).all() and (tl[~valid] == 0).all() and (tr[valid] >= 0).all()
  assert d_loss <= U.LOSS_BAR and d_tok <= U.TOKEN_LOSS_BAR
  # the summary is the mean / the counts of what the per-token outputs say
  assert abs(summ[0] - float(tl[valid].double().mean())) <= 1e-5
  assert summ[2] == float(((tr < 1) & valid).sum()) and summ[3] == float(((tr < 5) & valid).sum())
  d_ll = float((ll.cpu() - torch.stack([ref["logits"][b, int(last[b]) - 1] for b in range(B)])).abs().max())
  print(f"[forward_loss B={B}] max |last_logit d| {d_ll:.2e} (bar {U.LAST_LOGIT_BAR:.1e})")
  assert d_ll <= U.LAST_LOGIT_BAR


# ---------------------------------------------------------------------------------------------------------------- GILLModel.forward
PREFIX = "a picture of"


@pytest.fixture(scope="module")
def rig(cuda):
  from gill_amd.models import GILLModel
  cfg, sd, ids, _, last = U.engine_case(2)
  ccfg = synth.ClipConfig.tiny()
  tok = synth.HashTokenizer()
  csd = {k: U.bf(v) for k, v in synth.clip_state_dict(ccfg, seed=5).items()}
  args = SimpleNamespace(freeze_lm=True, freeze_vm=True, opt_version="facebook/opt-125m", visual_encoder="openai/clip-tiny",
                         n_visual_tokens=4, ret_emb_dim=256, gen_emb_dim=768, text_emb_layers=[-1], text_fc_mode="gill_mapper",
                         ret_text_fc_mode="linear", num_tokens=8, num_clip_tokens=77, retrieval_token_idx=synth.IMG_TOKEN_IDS,
                         gen_token_idx=synth.IMG_TOKEN_IDS, opt_state_dict=sd, clip_state_dict=csd, clip_config=ccfg)
  torch.manual_seed(11)
  m = GILLModel(tok, args)
  proj = {}
  synth._linear(proj, "visual_embeddings", 4 * 768, ccfg.hidden_size, 5)
  synth._linear(proj, "visual_fc", 256, ccfg.hidden_size, 5)
  with torch.no_grad():
    for name in ("visual_embeddings", "visual_fc"):
      getattr(m, name).weight.copy_(U.bf(proj[name + ".weight"]))
      getattr(m, name).bias.copy_(U.bf(proj[name + ".bias"]))
  m.eval()
  m = m.bfloat16().cuda()
  px = synth.normal("lm_loss_pixels", (2, 3, ccfg.image_size, ccfg.image_size), 3)
  return SimpleNamespace(m=m, cfg=cfg, sd=sd, tok=tok, ids=ids, caption_len=last + 1, px=px.to(cuda), cuda=cuda)


def _restate(rig, mode, prefix, visual_embs):
  """The reference's forward on the oracle: inputs_embeds = [visual rows (captioning) | prefix | labels], its label loops, its LM call."""
  table = rig.sd["model.decoder.embed_tokens.weight"]
  B = rig.ids.shape[0]
  front = []
  if mode == "captioning":
    front.append(visual_embs.float().cpu())
  if prefix is not None:
    pid = rig.tok(prefix, add_special_tokens=False, return_tensors="pt").input_ids
    front.append(F.embedding(pid, table).repeat(B, 1, 1))
  n_front = sum(f.shape[1] for f in front)
  emb = torch.cat(front + [F.embedding(rig.ids, table)], 1)
  full = U.label_loops(rig.ids, mode, n_front, rig.tok.pad_token_id, synth.IMG_TOKEN_IDS, synth.IMG_TOKEN_IDS)
  return full, n_front, U.lm_scores(rig.sd, rig.cfg.num_layers, rig.cfg.num_heads, emb, full)


@pytest.mark.parametrize("prefix", [None, PREFIX], ids=["no prefix", "prefix"])
@pytest.mark.parametrize("mode", ["captioning", "retrieval", "generation"])
def test_forward_modes_vs_restatement(rig, mode, prefix):
  from gill_amd import utils
  m = rig.m
  with torch.no_grad():
    out = m(rig.px, rig.ids.to(rig.cuda), rig.caption_len.to(rig.cuda), mode=mode, input_prefix=prefix, lm_loss=True, return_logits=True)
  output, full_labels, last_embedding, last_output_logit, visual_embs, visual_embs_norm, input_embs_norm, llm_hidden = out
  caption_embs = m.get_visual_embs(rig.px, "captioning") if mode == "captioning" else None
  full, n_front, ref = _restate(rig, mode, prefix, caption_embs)
  assert torch.equal(full_labels.cpu(), full), "full_labels differ from the reference's loops"
  valid = full[:, 1:] != -100
  d_loss = abs(float(output.loss) - float(ref["loss"]))
  d_tok = float((output.token_loss.cpu() - ref["token_loss"]).abs().max())
  print(f"[forward {mode} prefix={prefix!r}] loss {float(output.loss):.5f} restated {float(ref['loss']):.5f} |d| {d_loss:.2e} (bar {U.LOSS_BAR:.1e})  "
        f"max |token_loss d| {d_tok:.2e} (bar {U.TOKEN_LOSS_BAR:.1e})  n_tokens {float(output.n_tokens):.0f}")
  assert output.loss.dim() == 0 and output.loss.dtype == torch.float32 and output.loss.is_cuda
  assert float(output.n_tokens) == float(valid.sum()) and output.hidden_states is None
  assert d_loss <= U.LOSS_BAR and d_tok <= U.TOKEN_LOSS_BAR
  assert float(input_embs_norm) > 0 and float(visual_embs_norm) >= 0
  # return_logits: the (B, T, V) tensor reproduces the loss and the accuracies through torch
  B, T, V = output.logits.shape
  assert (B, T) == tuple(full.shape) and output.logits.dtype == torch.float32
  ce = F.cross_entropy(output.logits[:, :-1].reshape(-1, V), full_labels[:, 1:].reshape(-1), ignore_index=-100)
  d_ce = abs(float(ce) - float(output.loss))
  acc_l = utils.accuracy(output.logits[:, :-1], full_labels[:, 1:], -100, topk=(1, 5))
  acc_r = utils.accuracy_from_ranks(output.token_rank, topk=(1, 5))
  one = 100.0 / float(valid.sum())
  print(f"  logits route: |loss d| {d_ce:.2e}  top-1 / top-5 {float(acc_l[0]):.2f} / {float(acc_l[1]):.2f} %, from ranks {float(acc_r[0]):.2f} / {float(acc_r[1]):.2f} %")
  # the same bf16 operands, fp32 accumulation in two orders: two mean bars; a verdict can flip only on a tie within the logit bar (at most one token)
  assert d_ce <= 2 * U.MEAN_BAR
  assert all(abs(float(a) - float(b)) <= one + 1e-4 for a, b in zip(acc_l, acc_r))
  if mode == "captioning":
    assert last_embedding is None and last_output_logit is None and llm_hidden == []
    return
  want_ll = torch.stack([ref["logits"][b, int(rig.caption_len[b]) - 1 + n_front - 1] for b in range(B)])
  d_ll = float((last_output_logit.cpu() - want_ll).abs().max())
  print(f"  max |last_output_logit d| {d_ll:.2e} (bar {U.LAST_LOGIT_BAR:.1e})")
  assert last_output_logit.shape == (B, V) and d_ll <= U.LAST_LOGIT_BAR
  assert llm_hidden[0].shape == (B, 8, rig.cfg.hidden_size)
  if mode == "retrieval":
    scale = float(m.logit_scale.float().exp())
    n_t = last_embedding.float().norm(dim=-1).cpu()
    n_v = visual_embs.float().norm(dim=-1).cpu()
    print(f"  |last_embedding| {n_t.tolist()}  |visual_embs| {n_v.tolist()}  exp(logit_scale) {scale:.4f}")
    assert last_embedding.shape == (B, 256) and visual_embs.shape == (B, 256)
    # bf16 rows: a unit norm to 2^-8 relative per element, i.e. well inside 1e-2 on the norm
    assert (n_t - 1).abs().max() <= 1e-2 and (n_v / scale - 1).abs().max() <= 1e-2
  else:
    assert last_embedding.shape == (B, 77, 768)


def test_forward_generation_default_is_the_hidden_rows_pass(rig):
  m = rig.m
  ids, cl = rig.ids.to(rig.cuda), rig.caption_len.to(rig.cuda)
  with torch.no_grad():
    output, full_labels, last_embedding, last_output_logit, visual_embs, visual_embs_norm, input_embs_norm, llm_hidden = m(
      rig.px, ids, cl, mode="generation")
    raw, emb = m.img_hidden_states(ids, cl - 1)
    want = m.gen_text_hidden_fcs[0](raw.to(m.logit_scale.dtype), emb.to(m.logit_scale.dtype))
  assert output.loss is None and output.logits is None and output.hidden_states is None
  assert last_output_logit is None and input_embs_norm is None
  assert torch.equal(llm_hidden[0], raw.to(m.logit_scale.dtype)) and torch.equal(last_embedding, want)
  assert visual_embs.shape == (2, 1, 768) and float(visual_embs_norm) == 0.0
  assert torch.equal(full_labels.cpu(), U.label_loops(rig.ids, "generation", 0, rig.tok.pad_token_id, synth.IMG_TOKEN_IDS, synth.IMG_TOKEN_IDS))
  # scoring leaves the rows what they were
  with torch.no_grad():
    scored = m(rig.px, ids, cl, mode="generation", lm_loss=True)
  assert scored[0].loss is not None and scored[0].logits is None
  assert torch.equal(scored[7][0], llm_hidden[0]) and torch.equal(scored[2], last_embedding)


def test_forward_refuses_what_is_not_built(rig):
  ids, cl = rig.ids.to(rig.cuda), rig.caption_len.to(rig.cuda)
  for mode in ("captioning", "retrieval", "generation"):
    with pytest.raises(NotImplementedError):
      rig.m(rig.px, ids, cl, mode=mode, concat_captions=True)
  with pytest.raises(ValueError):
    rig.m(rig.px, ids, cl, mode="training")
