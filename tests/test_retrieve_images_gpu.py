"""GILL.retrieve_images and the index path of generate_for_images_and_texts on the small GILL of
tests/test_stages_gpu.py::test_retrieval_branch_vs_reference_golden (opt-125m shapes, the same seeds, the same 24-row matrix), against the
reference's own picks and scores (tests/golden/gill_visual_tiny.npz, F7) and the fp64 restatement of tests/retrieval_util.py."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import retrieval_util as U
from gill_amd import synth

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _bfw(sd):
  return {k: v.bfloat16().float() for k, v in sd.items()}


@pytest.fixture(scope="module")
def rig(cuda, tmp_path_factory):
  from PIL import Image
  from gill_amd.models import GILL
  g = np.load(os.path.join(GOLD, "gill_visual_tiny.npz"))
  tmp = tmp_path_factory.mktemp("ret_images")
  tok = synth.HashTokenizer()
  ocfg = synth.OptConfig(vocab_size=50274, hidden_size=768, num_layers=12, num_heads=12, ffn_dim=3072)
  args = SimpleNamespace(freeze_lm=True, freeze_vm=True, opt_version="facebook/opt-125m", visual_encoder="openai/clip-vit-base-patch16",
                         n_visual_tokens=4, ret_emb_dim=256, gen_emb_dim=768, text_emb_layers=[-1], text_fc_mode="gill_mapper",
                         ret_text_fc_mode="linear", num_tokens=8, num_clip_tokens=77, retrieval_token_idx=synth.IMG_TOKEN_IDS,
                         gen_token_idx=synth.IMG_TOKEN_IDS, opt_state_dict=_bfw(synth.opt_state_dict(ocfg, seed=int(g["opt_seed"]))))
  n_img = int(g["n_img"])
  paths = []
  for k in range(n_img):
    arr = np.full((20, 20, 3), (7 * k) % 256, dtype=np.uint8)
    arr[:, :, 1] = (13 * k + 5) % 256
    p = str(tmp / f"{k}.png")
    Image.fromarray(arr).save(p)
    paths.append(p)
  emb_matrix = synth.normal("cc3m_emb_matrix", (n_img, 256), int(g["clip_seed"]))
  emb_matrix = emb_matrix / emb_matrix.norm(dim=-1, keepdim=True)
  m = GILL(tok, args, path_array=paths, emb_matrix=emb_matrix, load_sd=False)
  rproj = {}
  synth._linear(rproj, "ret_text_hidden_fcs.0.model", 256, 768, int(g["clip_seed"]))
  with torch.no_grad():
    m.model.ret_text_hidden_fcs[0].model.weight.copy_(rproj["ret_text_hidden_fcs.0.model.weight"].bfloat16().float())
    m.model.ret_text_hidden_fcs[0].model.bias.copy_(rproj["ret_text_hidden_fcs.0.model.bias"].bfloat16().float())
  m.model.gen_text_hidden_fcs[0].load_state_dict(_bfw(synth.mapper_state_dict(synth.MapperConfig(in_dim=768), seed=int(g["mapper_seed"]))),
                                                 strict=True)
  m = m.eval().bfloat16().cuda()
  m.emb_matrix = emb_matrix.to(cuda)
  assert m.ret_index is None
  return SimpleNamespace(m=m, g=g, text=str(g["text"]), other="a photo of two dogs on a beach", paths=paths, n_img=n_img)


def test_retrieve_images_matches_the_reference_golden(rig):
  m, g = rig.m, rig.g
  m.ret_index = None
  with pytest.raises(RuntimeError, match="build_retrieval_index"):
    m.retrieve_images([rig.text])
  ix = m.build_retrieval_index()
  try:
    assert ix is m.ret_index and len(ix) == rig.n_img and ix.dim == 256
    assert torch.equal(ix.rows(0, rig.n_img).cpu(), m.emb_matrix.cpu().to(torch.bfloat16))     # as it stands: no renormalisation
    out = m.retrieve_images([rig.text, rig.other, rig.text], k=3, return_embeddings=True)
    assert out.indices.shape == (3, 3) and out.indices.dtype == torch.int64 and out.scores.shape == (3, 3) and out.scores.dtype == torch.float32
    want = [(r // 7) for r in g["ret_red"].tolist()]          # red = 7 k mod 256, k < 24
    assert want == [5, 18, 7]
    idx, scores = out.indices.cpu(), out.scores.cpu()
    print("[retrieve_images] idx", idx.tolist(), "scores", scores.tolist(), "reference", g["ret_scores"].tolist())
    for b in (0, 2):
      assert idx[b].tolist() == want
      assert np.abs(scores[b].numpy() - g["ret_scores"]).max() < 3e-3
    assert torch.equal(idx[0], idx[2])
    assert out.paths == [[rig.paths[i] for i in row] for row in idx.tolist()]
    # the search half against the restatement fed the embeddings that were searched
    emb = out.embeddings.cpu()
    assert emb.shape == (3, 256) and emb.dtype == torch.float32
    S, mag = U.penalised_scores(ix.rows(0, rig.n_img).cpu().double(), U.normalized_queries(emb))
    ok, why = U.accept(scores, idx, S, U.bound(mag, 256, True))
    assert ok, why
    # k past the index, exclusions per prompt, an id tensor as input
    big = m.retrieve_images([rig.text], k=32)
    assert big.indices[0, :rig.n_img].sort().values.tolist() == list(range(rig.n_img)) and bool((big.indices[0, rig.n_img:] == -1).all())
    assert len(big.paths[0]) == rig.n_img
    ex = m.retrieve_images([rig.text, rig.text], k=3, exclude=[[5, 18], []])
    assert ex.indices[1].tolist() == want and ex.indices[0, 0].item() == 7 and 5 not in ex.indices[0].tolist()
    ids = m.model.tokenizer(rig.text, add_special_tokens=True, return_tensors="pt").input_ids
    ids = torch.cat([ids, torch.full((1, 3), m.model.tokenizer.pad_token_id, dtype=torch.int64)], 1)
    by_ids = m.retrieve_images(ids, k=3)
    assert by_ids.indices[0].tolist() == want and (by_ids.scores[0].cpu() - scores[0]).abs().max().item() < 3e-3
  finally:
    m.ret_index = None


def test_one_rank_group_equals_no_group(rig, tmp_path):
  import torch.distributed as dist
  m = rig.m
  m.build_retrieval_index()
  try:
    alone = m.retrieve_images([rig.text, rig.other], k=3, distributed=False, return_embeddings=True)
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
    try:
      group = m.retrieve_images([rig.text, rig.other], k=3, distributed=True, return_embeddings=True)
    finally:
      dist.destroy_process_group()
    assert torch.equal(alone.indices, group.indices) and torch.equal(alone.scores, group.scores)
    assert torch.equal(alone.embeddings, group.embeddings) and alone.paths == group.paths
  finally:
    m.ret_index = None


def _golden_asserts(rig, ret):
  g = rig.g
  rets = ret[1]["ret"]
  reds = [int(np.asarray(r[0])[0, 0, 0]) for r in rets]
  scores = np.array([r[2] for r in rets])
  print("[retrieval via index] picks", reds, "scores", scores.tolist(), "reference", g["ret_red"].tolist(), g["ret_scores"].tolist())
  assert reds == g["ret_red"].tolist() and all(r[1] == "ret" and r[0].size == (224, 224) for r in rets)
  assert np.abs(scores - g["ret_scores"]).max() < 3e-3
  assert ret[1]["gen"][0].shape == (1, 77, 768)


def test_generate_for_images_and_texts_through_the_index(rig, monkeypatch):
  from gill_amd.models import GILL
  m = rig.m
  calls = []
  legacy = GILL._scores

  def counting(matrix, query):
    calls.append(tuple(matrix.shape))
    return legacy(matrix, query)

  # without an index: the legacy path, called as before
  m.ret_index = None
  monkeypatch.setattr(GILL, "_scores", staticmethod(counting))
  ret = m.generate_for_images_and_texts([rig.text], num_words=2, gen_scale_factor=1e5)
  assert calls == [(rig.n_img, 256)]
  _golden_asserts(rig, ret)

  # with one: _scores must not see the matrix
  def refusing(matrix, query):
    if tuple(matrix.shape) == (rig.n_img, 256):
      raise AssertionError("the (N, D) matrix went through _scores although an index is attached")
    return legacy(matrix, query)

  monkeypatch.setattr(GILL, "_scores", staticmethod(refusing))
  m.build_retrieval_index()
  try:
    ret2 = m.generate_for_images_and_texts([rig.text], num_words=2, gen_scale_factor=1e5)
    _golden_asserts(rig, ret2)
    assert [r[2] for r in ret2[1]["ret"]] == pytest.approx([r[2] for r in ret[1]["ret"]], abs=3e-3)
  finally:
    m.ret_index = None
