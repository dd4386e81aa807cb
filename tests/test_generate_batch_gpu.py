"""GILLModel.generate_batch and GILL.generate_for_images_and_texts_batch end to end on the MI355X: one dialogue per row of a ragged batch
with the tokens the one-sequence loop emits for that row alone.

Free-running tokens of two arithmetic paths (the ragged batch; generate() at batch 1) can part at a near tie.  A disagreement is excused
only if the batch-1 run's own output_logits at that decision put the two tokens within m, the row then leaves the comparison, and excused
decisions are capped at 5 % of all decisions (the cap of test_decode_sample_gpu.py).  m is 10 x the logit distance between the
bf16-operand emulation and the fp32 oracle on these prompts (tools/ragged_decode_tolerance.py, tests/golden/ragged_decode_tolerance.json);
tests/test_ragged_decode_host.py asserts on the CPU that the oracle's own greedy run on them has no decision with a top-2 margin under m."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

import kv_cache_util as U
import ragged_decode_util as R
from gill_amd import synth
from test_decode_sample_gpu import IMG

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LONG = "a long text-only prompt about two brown dogs running along a beach at sunset with a red ball and a kite"


@pytest.fixture(scope="module")
def gill125(cuda):
  return R.gill125_rig(cuda)


def _rel(a, b):
  a, b = a.float().cpu(), b.float().cpu()
  return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def test_greedy_ragged_batch_equals_the_one_sequence_loop(cuda, gill125):
  """B = 6 at lengths (9, 6, 12, 5, 11, 8), min_word_tokens = 3, gen_scale_factor = 1e5, 5 decisions: three free tokens, then [IMG0] is
  certain at decisions 3 and 4 (two forced blocks; the second one ends the row, so n_hidden = 11 covers the first block)."""
  m = gill125.model
  tol = R.load_gen_tolerance()
  ids, lens = R.gen_prompt_ids()
  kw = dict(min_word_tokens=R.GEN_MWT, gen_scale_factor=1e5)
  tokens, n_tok, hidden, n_hid = m.generate_batch(ids=ids.to(cuda), lengths=lens, max_len=5, **kw)
  waits = m._decode_host_waits
  assert tokens.shape == (6, 40) and tokens.dtype == torch.int64 and hidden.shape == (6, 40, 768) and hidden.dtype == torch.float32
  assert n_tok.tolist() == [19] * 6 and n_hid.tolist() == [11] * 6
  assert waits <= 19 + 1, waits                     # one read per iteration, one iteration late: at most one surplus iteration
  assert (tokens[:, 19:] == -1).all()
  # the same prompts handed over as embeddings: the same prefill arithmetic, the same bits
  t2, n2, h2, nh2 = m.generate_batch(embeddings=m.input_embeddings(ids.to(cuda)), lengths=lens, max_len=5, **kw)
  assert torch.equal(t2, tokens) and torch.equal(n2, n_tok) and torch.equal(nh2, n_hid) and torch.equal(h2[:, :11], hidden[:, :11])
  excused = 0
  for b, n in enumerate(lens):
    emb = m.input_embeddings(ids[b:b + 1, :n].to(cuda))
    out, embs, logits = m.generate(emb, 5, **kw)
    got, want = tokens[b, :19].tolist(), out[0].tolist()
    assert want[3:11] == IMG and want[11:19] == IMG
    if got != want:
      col = next(j for j in range(19) if got[j] != want[j])
      assert col < 3, (b, got, want)                # only a free decision can differ
      margin = abs(float(logits[col][0, got[col]] - logits[col][0, want[col]]))
      print(f"[generate_batch] row {b} decision {col}: batch picked {got[col]}, alone {want[col]}; their logits are {margin:.3e} apart (m = {tol:.3e})")
      assert margin <= tol, (b, col, got[col], want[col], margin)
      excused += 1
      continue
    rel = _rel(hidden[b, :11], embs[-1][0, n:n + 11])
    rel_img = _rel(hidden[b, 3:11], embs[-1][0, n + 3:n + 11])
    print(f"[generate_batch] row {b} (length {n}): hidden rows rel_l2 {rel:.3e}, [IMG] block {rel_img:.3e}")
    assert rel < U.REL_BAR and rel_img < U.REL_BAR
  assert excused * 20 <= 6 * 5, excused


def test_seeded_rows_do_not_depend_on_the_batch(cuda, gill125):
  m = gill125.model
  ids, lens = R.gen_prompt_ids()
  kw = dict(max_len=4, temperature=4.0, top_p=0.9, seed=7)
  cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state()
  tokens, n_tok, _, _ = m.generate_batch(ids=ids.to(cuda), lengths=lens, **kw)
  again, n_again, _, _ = m.generate_batch(ids=ids.to(cuda), lengths=lens, **kw)
  assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(), dev_state)
  assert torch.equal(tokens, again) and torch.equal(n_tok, n_again)
  other, _, _, _ = m.generate_batch(ids=ids.to(cuda), lengths=lens, **dict(kw, top_p=1.0))
  other2, _, _, _ = m.generate_batch(ids=ids.to(cuda), lengths=lens, **dict(kw, top_p=1.0, seed=8))
  assert not torch.equal(other, other2)
  for r, n in enumerate(lens):
    t1, n1, _, _ = m.generate_batch(ids=ids[r:r + 1, :n].to(cuda), lengths=[n], row_ids=[r], **kw)
    assert int(n1[0]) == int(n_tok[r])
    assert t1[0, :int(n1[0])].tolist() == tokens[r, :int(n_tok[r])].tolist(), r


def test_argument_errors(cuda, gill125):
  m = gill125.model
  ids, lens = R.gen_prompt_ids()
  ids = ids.to(cuda)
  with pytest.raises(ValueError, match="position table"):
    m.generate_batch(ids=ids, lengths=lens, max_len=300)                # 12 + 300 * 8 > 2048
  with pytest.raises(ValueError, match="seed"):
    m.generate_batch(ids=ids, lengths=lens, max_len=2, temperature=1.0)
  with pytest.raises(ValueError, match="lengths"):
    m.generate_batch(ids=ids, lengths=lens[:-1], max_len=2)
  with pytest.raises(ValueError, match="lengths"):
    m.generate_batch(ids=ids, lengths=[13] + lens[1:], max_len=2)
  with pytest.raises(ValueError):
    m.generate_batch(ids=ids, embeddings=m.input_embeddings(ids), lengths=lens, max_len=2)
  with pytest.raises(ValueError, match="top_p"):
    m.generate_batch(ids=ids, lengths=lens, max_len=2, top_p=0.5)


def _bfw(sd):
  return {k: v.bfloat16().float() for k, v in sd.items()}


@pytest.fixture(scope="module")
def rig(cuda):
  """The rig of tests/test_interleaved_prompts_gpu.py (tiny CLIP at 32 px, OPT-125m shapes, the seeds of golden/gill_visual_tiny.npz)
  without a retrieval matrix: the generation branch."""
  from gill_amd.models import GILL
  g = np.load(os.path.join(GOLD, "gill_visual_tiny.npz"))
  ccfg = synth.ClipConfig.tiny()
  ocfg = synth.OptConfig(vocab_size=50274, hidden_size=768, num_layers=12, num_heads=12, ffn_dim=3072)
  args = SimpleNamespace(freeze_lm=True, freeze_vm=True, opt_version="facebook/opt-125m", visual_encoder="openai/clip-tiny",
                         n_visual_tokens=4, ret_emb_dim=256, gen_emb_dim=768, text_emb_layers=[-1], text_fc_mode="gill_mapper",
                         ret_text_fc_mode="linear", num_tokens=8, num_clip_tokens=77, retrieval_token_idx=synth.IMG_TOKEN_IDS,
                         gen_token_idx=synth.IMG_TOKEN_IDS, opt_state_dict=_bfw(synth.opt_state_dict(ocfg, seed=int(g["opt_seed"]))),
                         clip_state_dict=_bfw(synth.clip_state_dict(ccfg, seed=int(g["clip_seed"]))), clip_config=ccfg)
  m = GILL(synth.HashTokenizer(), args, load_sd=False)
  proj = {}
  synth._linear(proj, "visual_embeddings", 4 * 768, ccfg.hidden_size, int(g["clip_seed"]))
  with torch.no_grad():
    m.model.visual_embeddings.weight.copy_(proj["visual_embeddings.weight"].bfloat16().float())
    m.model.visual_embeddings.bias.copy_(proj["visual_embeddings.bias"].bfloat16().float())
  m.model.gen_text_hidden_fcs[0].load_state_dict(_bfw(synth.mapper_state_dict(synth.MapperConfig(in_dim=768), seed=int(g["mapper_seed"]))),
                                                 strict=True)
  m = m.eval().bfloat16().cuda()
  return SimpleNamespace(m=m, img=Image.fromarray(g["image"]), text=str(g["text"]))


def test_batch_api_equals_the_one_sequence_method(rig):
  """Three prompt lists, one with an image, load_sd=False: captions equal, the 'gen' embeddings within REL_BAR."""
  m = rig.m
  lists = [[rig.img, rig.text], [LONG], ["a photo of", "a small red kite"]]
  kw = dict(num_words=5, min_word_tokens=3, gen_scale_factor=1e5)
  got = m.generate_for_images_and_texts_batch(lists, **kw)
  assert len(got) == 3
  for b, pl in enumerate(lists):
    want = m.generate_for_images_and_texts(pl, **kw)
    assert len(got[b]) == len(want) == 2
    assert got[b][0] == want[0] and got[b][0].endswith("[IMG7]"), (b, got[b][0], want[0])
    assert got[b][1]["decision"] == want[1]["decision"] == ["gen", [0, 1]] and got[b][1]["ret"] == []
    a, w = got[b][1]["gen"][0], want[1]["gen"][0]
    assert a.shape == w.shape == (1, 77, 768)
    rel = _rel(a, w)
    print(f"[generate_for_images_and_texts_batch] prompt list {b}: caption {got[b][0]!r}; gen embedding rel_l2 {rel:.3e}")
    assert rel < U.REL_BAR
  # scope: with retrieval embeddings attached the batch entry refuses and names the one-sequence method
  m.emb_matrix = torch.zeros((4, 256), device="cuda")
  try:
    with pytest.raises(NotImplementedError, match="generate_for_images_and_texts"):
      m.generate_for_images_and_texts_batch(lists, **kw)
  finally:
    m.emb_matrix = None
  with pytest.raises(NotImplementedError):
    m.generate_for_images_and_texts_batch(lists, num_words=0)
  with pytest.raises(ValueError):
    m.generate_for_images_and_texts_batch([[3.5]], num_words=2)
