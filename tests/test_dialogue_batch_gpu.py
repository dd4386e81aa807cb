"""GILL.generate_for_images_and_texts_batch(all_branches=True) on the MI355X: retrieval, the decision MLP and the CLIP rerank for a ragged
batch of dialogues, against the reference's golden values for the golden row and against generate_for_images_and_texts on every row alone.
The rig is that of test_stages_gpu.test_retrieval_branch_vs_reference_golden (tests/dialogue_batch_util.py).  tests/test_img_heads_host.py
asserts on the CPU that the oracle's 3rd and 4th retrieval picks on these prompts are more than 2 x 3e-3 apart, so picks are compared exactly."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import dialogue_batch_util as DB
import kv_cache_util as U
from gill_amd import synth

pytestmark = pytest.mark.gpu
KW = dict(num_words=2, gen_scale_factor=1e5)


@pytest.fixture(scope="module")
def rig(cuda, tmp_path_factory):
  r = DB.build_rig(cuda, tmp_path_factory.mktemp("dialogue_images"))
  r.lists = DB.prompt_lists(r.g)
  r.alone = {}          # (index attached, keyword arguments) -> the one-sequence method's outputs per prompt list, computed once
  return r


def _with_index(rig, attach):
  m = rig.m
  if attach and m.ret_index is None:
    m.build_retrieval_index()
  if not attach:
    m.ret_index = None
  return m


def _alone(rig, attach, lists, **kw):
  key = (attach, tuple(map(tuple, lists)), tuple(sorted(kw.items())))
  if key not in rig.alone:
    m = _with_index(rig, attach)
    rig.alone[key] = [m.generate_for_images_and_texts(pl, **kw) for pl in lists]
  return rig.alone[key]


def _reds(rets):
  return [int(np.asarray(r[0])[0, 0, 0]) for r in rets]


def _rel(a, b):
  a, b = a.float().cpu(), b.float().cpu()
  return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _same_blocks(tag, got, want):
  """One prompt list's outputs of the batch entry against the one-sequence method's."""
  assert len(got) == len(want), (tag, got, want)
  for i, (a, w) in enumerate(zip(got, want)):
    if isinstance(w, str):
      assert a == w, (tag, i, a, w)
      continue
    assert _reds(a["ret"]) == _reds(w["ret"]) and all(r[1] == "ret" and r[0].size == (224, 224) for r in a["ret"]), (tag, i)
    d = np.abs(np.array([r[2] for r in a["ret"]]) - np.array([r[2] for r in w["ret"]])).max()
    assert a["decision"][0] == w["decision"][0] and len(a["decision"]) == len(w["decision"]) == 2
    dp = np.abs(np.array(a["decision"][1]) - np.array(w["decision"][1]).reshape(-1)).max()
    rel = _rel(a["gen"][0], w["gen"][0])
    print(f"[dialogue batch] {tag} item {i}: picks {_reds(a['ret'])}, score distance {d:.3e}, decision {a['decision'][0]} (probability distance "
          f"{dp:.3e}), gen embedding rel_l2 {rel:.3e}")
    assert d < DB.SCORE_BAR and dp < DB.PROB_BAR
    assert a["gen"][0].shape == w["gen"][0].shape == (1, 77, 768) and rel < U.REL_BAR


@pytest.mark.parametrize("attach", [True, False], ids=["index", "no_index"])
def test_all_branches_against_golden_and_the_one_sequence_method(rig, cuda, attach):
  m, g = _with_index(rig, attach), rig.g
  got = m.generate_for_images_and_texts_batch(rig.lists, all_branches=True, **KW)
  assert len(got) == 3 and all(len(o) == 2 for o in got)
  # the golden row: the reference's own picks and scores, the decision against plain fp32 math on the row's hidden state
  out = got[0][1]
  scores = np.array([r[2] for r in out["ret"]])
  print("[dialogue batch] golden picks", _reds(out["ret"]), "scores", scores.tolist(), "reference", g["ret_red"].tolist(), g["ret_scores"].tolist())
  assert _reds(out["ret"]) == g["ret_red"].tolist()
  assert np.abs(scores - g["ret_scores"]).max() < DB.SCORE_BAR
  prompt = m.model.tokenizer(str(g["text"]), add_special_tokens=True, return_tensors="pt").input_ids.to(cuda)
  _, embs, _ = m.model.generate(m.model.input_embeddings(prompt), 2, gen_scale_factor=1e5)
  h0 = embs[-1][:, prompt.shape[1], :].float().cpu()
  lin = rig.dec[1]
  logits = h0 @ lin.weight.float().cpu().T + lin.bias.float().cpu()
  exp = logits.softmax(-1)[0].tolist()
  print("[dialogue batch] golden decision", out["decision"], "expected", exp)
  assert out["decision"][0] == {0: "gen", 1: "ret"}[int(logits.argmax())]
  assert np.abs(np.array(out["decision"][1]) - np.array(exp)).max() < DB.PROB_BAR
  # every row against the one-sequence method on it alone
  for b, want in enumerate(_alone(rig, attach, rig.lists, **KW)):
    _same_blocks(f"prompt list {b}", got[b], want)


def test_a_row_without_an_img_block_returns_its_caption(rig):
  """gen_scale_factor is one value for the whole call, so under 1.0 no row of the batch forces a block: this covers the caption-only rows
  of a call in which no block exists at all (the heads are then never launched), not caption-only rows beside rows with blocks."""
  m = _with_index(rig, False)
  lists = [[DB.LONG], list(DB.PARTS)]
  got = m.generate_for_images_and_texts_batch(lists, num_words=2, gen_scale_factor=1.0, all_branches=True)
  for b, o in enumerate(got):
    print(f"[dialogue batch] free-running row {b}: {o}")
    assert len(o) == 1 and isinstance(o[0], str) and "[IMG" not in o[0]


@pytest.mark.parametrize("attach", [True, False], ids=["index", "no_index"])
def test_two_rounds_exclude_the_first_round_picks(rig, attach):
  """num_words = 3 under gen_scale_factor = 1e5 is three forced [IMG] blocks per row, two of them with hidden states: with
  max_num_rets = 2 every row has two blocks, and round 1 searches with round 0's picks excluded (no crafted hits are needed)."""
  m = _with_index(rig, attach)
  lists = [[DB.LONG], [str(rig.g["text"])]]
  kw = dict(num_words=3, gen_scale_factor=1e5, max_num_rets=2)
  got = m.generate_for_images_and_texts_batch(lists, all_branches=True, **kw)
  first, second = got[0][1], got[0][3]
  assert len(got[0]) == 4 and len(first["ret"]) == 3 and len(second["ret"]) == 3
  assert not set(_reds(first["ret"])) & set(_reds(second["ret"]))
  assert all(r[2] > -500 for r in second["ret"])          # nothing carrying the seen penalty was picked: 21 other images remain
  for b, want in enumerate(_alone(rig, attach, lists, **kw)):      # (test_img_heads_host.py holds the oracle's gaps of both rows, both rounds)
    assert len(got[b]) == 4 and not set(_reds(got[b][1]["ret"])) & set(_reds(got[b][3]["ret"]))
    _same_blocks(f"two rounds, row {b}", got[b], want)


def test_skip_gen_on_ret(rig):
  m = _with_index(rig, True)
  base = m.generate_for_images_and_texts_batch(rig.lists, all_branches=True, **KW)
  d = sorted(float(np.log(o[1]["decision"][1][1] / o[1]["decision"][1][0])) for o in base)      # z1 - z0 per row
  bias = m.decision_model[1].bias
  keep = bias.detach().clone()
  try:
    with torch.no_grad():
      bias[1] -= 0.5 * (d[0] + d[1])        # between the two lowest rows: one row decides 'gen', two decide 'ret'
    full = m.generate_for_images_and_texts_batch(rig.lists, all_branches=True, **KW)
    skip = m.generate_for_images_and_texts_batch(rig.lists, all_branches=True, skip_gen_on_ret=True, **KW)
  finally:
    with torch.no_grad():
      bias.copy_(keep)
  labels = [o[1]["decision"][0] for o in full]
  print("[dialogue batch] decisions with the moved bias:", labels, "logit differences before", d)
  assert sorted(set(labels)) == ["gen", "ret"]
  for f, s in zip(full, skip):
    assert s[0] == f[0] and s[1]["decision"] == f[1]["decision"] and _reds(s[1]["ret"]) == _reds(f[1]["ret"])
    if f[1]["decision"][0] == "ret":
      assert s[1]["gen"] == [] and len(f[1]["gen"]) == 1
    else:
      assert _rel(s[1]["gen"][0], f[1]["gen"][0]) < U.REL_BAR


def test_default_still_refuses(rig):
  m = _with_index(rig, False)
  with pytest.raises(NotImplementedError, match="generate_for_images_and_texts"):
    m.generate_for_images_and_texts_batch(rig.lists, **KW)
  with pytest.raises(TypeError):
    m.generate_for_images_and_texts_batch(rig.lists, every_branch=True, **KW)


def _bfw(sd):
  return {k: v.bfloat16().float() for k, v in sd.items()}


def test_all_branches_with_sd_vae_and_clip_rerank(cuda, tmp_path):
  """The rig of test_stages_gpu.test_public_api_all_branches_with_sd (tiny SD + VAE + tiny CLIP), two prompt lists, two images per block:
  3 'ret' and 2 'gen' entries per block, 'gen' sorted by descending score, and each best score equal to the cosine recomputed through the
  one-sequence method's host preprocessing.  Images are not compared across the two entries: they draw latents in different batch shapes."""
  from PIL import Image
  from gill_amd import utils
  from gill_amd.models import GILL
  from gill_amd.sd import GillSDPipeline
  ucfg = synth.UNetConfig(block_out_channels=(64, 128, 256, 256), num_heads=4, cross_attention_dim=768, sample_size=16)
  uncond = synth.uncond_context(ucfg.ctx_len, ucfg.cross_attention_dim, seed=3).bfloat16().float()
  vcfg = synth.VAEConfig.tiny(16)
  pipe = GillSDPipeline(_bfw(synth.unet_state_dict(ucfg, seed=3)), ucfg, uncond, cuda, max_batch=8,
                        vae_state=_bfw(synth.vae_decoder_state_dict(vcfg, seed=5)), vae_cfg=vcfg)
  ccfg = synth.ClipConfig.tiny()
  tok = synth.HashTokenizer()
  args = SimpleNamespace(freeze_lm=True, freeze_vm=True, opt_version="facebook/opt-125m", visual_encoder="openai/clip-tiny",
                         n_visual_tokens=4, ret_emb_dim=256, gen_emb_dim=768, text_emb_layers=[-1], text_fc_mode="gill_mapper",
                         ret_text_fc_mode="linear", num_tokens=8, num_clip_tokens=77, retrieval_token_idx=synth.IMG_TOKEN_IDS,
                         gen_token_idx=synth.IMG_TOKEN_IDS, opt_state_dict=_bfw(synth.opt_state_dict(DB.opt_cfg(), seed=5)),
                         clip_state_dict=_bfw(synth.clip_state_dict(ccfg, seed=13)), clip_config=ccfg)
  paths = []
  for k in range(8):
    p = str(tmp_path / f"{k}.png")
    Image.fromarray(np.full((12, 12, 3), 20 * k, dtype=np.uint8)).save(p)
    paths.append(p)
  emb_matrix = synth.normal("api_emb_matrix", (8, 256), 2)
  emb_matrix = emb_matrix / emb_matrix.norm(dim=-1, keepdim=True)
  m = GILL(tok, args, path_array=paths, emb_matrix=emb_matrix, load_sd=True, sd_pipe=pipe, num_gen_images=2)
  m.model.gen_text_hidden_fcs[0].load_state_dict(_bfw(synth.mapper_state_dict(synth.MapperConfig(in_dim=768), seed=7)), strict=True)
  m = m.eval().bfloat16().cuda()
  m.emb_matrix = emb_matrix.to(cuda)
  texts = ["two birds on a wire", "a small red fox jumps over the lazy dog"]
  got = m.generate_for_images_and_texts_batch([[t] for t in texts], num_inference_steps=4, all_branches=True,
                                              generator=torch.Generator("cpu").manual_seed(5), **KW)
  assert len(got) == 2
  for text, o in zip(texts, got):
    out = o[1]
    assert len(out["ret"]) == 3 and len(out["gen"]) == 2 and out["decision"] is None
    (im0, s0), (im1, s1) = out["gen"]
    assert im0.size == (128, 128) and im1.size == (128, 128) and np.isfinite([s0, s1]).all() and s0 >= s1
    # the rerank score of the best image, recomputed: cos(visual_fc(CLIP(image)), ret_text_hidden_fcs(raw_emb)[0])
    prompt = tok(text, add_special_tokens=True, return_tensors="pt").input_ids.to(cuda)
    _, embs, _ = m.model.generate(m.model.input_embeddings(prompt), 2, gen_scale_factor=1e5)
    raw = embs[-1][:, prompt.shape[1]:prompt.shape[1] + 8, :]
    r = m.model.ret_text_hidden_fcs[0](raw, None)[:, 0, :].float()
    r = r / r.norm(dim=-1, keepdim=True)
    px = utils.get_pixel_values_for_model(m.model.feature_extractor, im0.resize((224, 224)).convert("RGB"))[None].to(cuda)
    v = m.model.get_visual_embs(px, mode="retrieval").float().reshape(1, -1)
    v = v / v.norm(dim=-1, keepdim=True)
    print(f"[dialogue batch rerank] {text!r}: scores {s0} {s1}, recomputed best {float((v * r).sum())}")
    assert abs(float((v * r).sum()) - s0) < 2e-2
