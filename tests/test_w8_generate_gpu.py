"""GILLModel.quantize_lm('fp8') end to end on the MI355X: greedy generate_batch on the weight-only fp8 decoder against a second,
unquantised model whose lm weights are w8_util.w8_state_dict of the same weights (the quantised model IS that bf16 model).

The rig is ragged_decode_util.gill125_rig; the prompts are gen_prompt_ids at the seed of tests/golden/w8_generate_tolerance.json.  The
standing golden (ragged_decode_tolerance.json, seed 46) does not carry over: on the dequantised weights the oracle's greedy run at that
seed has a decision with a top-2 margin of 1.97, under its m = 2.76.  tools/w8_tolerance.py --write therefore repeats
tools/ragged_decode_tolerance.py's method on the dequantised weights (m = 10 x the logit distance between the bf16-operand emulation and the
fp32 oracle; first seed whose oracle decisions all clear m) and tests/test_w8_host.py re-checks the claim on the CPU.  A disagreement is
excused only by the near-tie rule of test_generate_batch_gpu.py: the reference run's own logits at that decision put the two tokens within
m, the row then leaves the comparison, and excused decisions are capped at 5 % of all decisions."""
import json
import os
from types import SimpleNamespace

import pytest
import torch

import kv_cache_util as U
import ragged_decode_util as R
import w8_util as W
from gill_amd import synth
from test_decode_sample_gpu import IMG, _bfw

pytestmark = pytest.mark.gpu
KW = dict(min_word_tokens=R.GEN_MWT, gen_scale_factor=1e5)


def _golden():
  with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "w8_generate_tolerance.json")) as f:
    return json.load(f)


@pytest.fixture(scope="module")
def gill125(cuda):
  g = R.gill125_rig(cuda)
  yield g
  g.model.quantize_lm(None)          # the rig is shared with other modules


@pytest.fixture(scope="module")
def reference(cuda):
  """An unquantised model on w8_state_dict of the rig's lm weights."""
  from gill_amd.models import GILL
  ocfg = synth.OptConfig(vocab_size=50274, hidden_size=768, num_layers=12, num_heads=12, ffn_dim=3072)
  sdq = W.w8_state_dict(_bfw(synth.opt_state_dict(ocfg, seed=5)), ocfg)
  args = SimpleNamespace(freeze_lm=True, freeze_vm=True, opt_version="facebook/opt-125m", visual_encoder="openai/clip-vit-base-patch16",
                         n_visual_tokens=4, ret_emb_dim=256, gen_emb_dim=768, text_emb_layers=[-1], text_fc_mode="gill_mapper",
                         ret_text_fc_mode="linear", num_tokens=8, num_clip_tokens=77, retrieval_token_idx=synth.IMG_TOKEN_IDS,
                         gen_token_idx=synth.IMG_TOKEN_IDS, opt_state_dict=sdq)
  return GILL(synth.HashTokenizer(), args, load_sd=False).eval().bfloat16().cuda()


def test_quantize_lm_switch(cuda, gill125):
  from gill_amd import _native as N
  m = gill125.model
  rec = _golden()
  ids, lens = R.gen_prompt_ids(rec["seed"])
  m.quantize_lm(None)
  t0, n0, h0, nh0 = m.generate_batch(ids=ids.to(cuda), lengths=lens, max_len=5, **KW)
  assert N.lib().gill_opt_weight_mode(m._opt_handle) == 0
  with pytest.raises(ValueError):
    m.quantize_lm("int4")
  assert m.opt_weights == "bf16"
  assert m.quantize_lm("fp8") is m and m.opt_weights == "fp8" and m._opt_handle is None
  t8, n8, h8, nh8 = m.generate_batch(ids=ids.to(cuda), lengths=lens, max_len=5, **KW)
  assert N.lib().gill_opt_weight_mode(m._opt_handle) == 1 and N.lib().gill_opt_decode_uses_w8(m._opt_handle, len(lens)) == 1
  m._opt_native(32, 128)              # a handle rebuilt for capacity keeps its mode
  assert N.lib().gill_opt_weight_mode(m._opt_handle) == 1
  m.quantize_lm("bf16")
  assert m._opt_handle is None
  t1, n1, h1, nh1 = m.generate_batch(ids=ids.to(cuda), lengths=lens, max_len=5, **KW)
  assert torch.equal(t1, t0) and torch.equal(n1, n0) and torch.equal(nh1, nh0) and torch.equal(h1, h0), "bf16 outputs are not restored bit for bit"
  rel = ((h8[:, :3] - h0[:, :3]).norm() / h0[:, :3].norm()).item()
  print(f"fp8 vs bf16 decoder: hidden rows of the free decisions rel_l2 {rel:.3e}")
  assert rel > 0, "the quantised decoder returned the bf16 decoder's bits"


def test_greedy_generate_batch_on_the_quantised_decoder(cuda, gill125, reference):
  m, ref = gill125.model, reference.model
  rec = _golden()
  tol = float(rec["m"])
  ids, lens = R.gen_prompt_ids(rec["seed"])
  m.quantize_lm("fp8")
  tokens, n_tok, hidden, n_hid = m.generate_batch(ids=ids.to(cuda), lengths=lens, max_len=5, **KW)
  assert n_tok.tolist() == [19] * 6 and n_hid.tolist() == [11] * 6
  excused = 0
  for b, n in enumerate(lens):
    emb = ref.input_embeddings(ids[b:b + 1, :n].to(cuda))
    out, embs, logits = ref.generate(emb, 5, **KW)
    got, want = tokens[b, :19].tolist(), out[0].tolist()
    assert want[3:11] == IMG and want[11:19] == IMG
    if got != want:
      col = next(j for j in range(19) if got[j] != want[j])
      assert col < 3, (b, got, want)
      margin = abs(float(logits[col][0, got[col]] - logits[col][0, want[col]]))
      print(f"[w8 generate_batch] row {b} decision {col}: fp8 picked {got[col]}, reference {want[col]}; their logits are {margin:.3e} apart (m = {tol:.3e})")
      assert margin <= tol, (b, col, got[col], want[col], margin)
      excused += 1
      continue
    a, w = hidden[b, :11].float().cpu(), embs[-1][0, n:n + 11].float().cpu()
    rel = ((a - w).norm() / w.norm()).item()
    print(f"[w8 generate_batch] row {b} (length {n}): hidden rows rel_l2 {rel:.3e}")
    assert rel < U.REL_BAR
  assert excused * 20 <= 6 * 5, excused
