"""Host half of the interleaved image + text prompts of GILL.generate_images / retrieve_images: how a prompt list becomes the id matrix with
negative slots (gill/models.py:600-631: <bos> on the first string only, n_visual_tokens rows per image), how a rank's shard renumbers them,
and the argument errors, all before anything touches a device."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

from gill_amd import synth
from gill_amd.models import GILL


def _tiny_gill(with_clip=True):
  tok = synth.HashTokenizer()
  ocfg = synth.OptConfig(vocab_size=len(tok), hidden_size=128, num_layers=2, num_heads=2, ffn_dim=256, max_positions=128)
  extra = {}
  if with_clip:
    ccfg = synth.ClipConfig.tiny()
    extra = dict(clip_state_dict=synth.clip_state_dict(ccfg, seed=2), clip_config=ccfg)
  args = SimpleNamespace(freeze_lm=True, freeze_vm=True, opt_version="facebook/opt-tiny-synth",
                         visual_encoder="openai/clip-tiny" if with_clip else "openai/clip-vit-base-patch16",
                         n_visual_tokens=4, ret_emb_dim=256, gen_emb_dim=768, text_emb_layers=[-1], text_fc_mode="gill_mapper",
                         ret_text_fc_mode="linear", num_tokens=8, num_clip_tokens=77, retrieval_token_idx=synth.IMG_TOKEN_IDS,
                         gen_token_idx=synth.IMG_TOKEN_IDS, opt_state_dict=synth.opt_state_dict(ocfg, seed=1), **extra)
  return GILL(tok, args, load_sd=False)


@pytest.fixture(scope="module")
def gill():
  return _tiny_gill()


def _img(v=0):
  return Image.fromarray(np.full((9, 7, 3), v, dtype=np.uint8))


def _tok(g, s, bos):
  return g.model.tokenizer(s, add_special_tokens=bos, return_tensors="pt").input_ids[0].tolist()


def test_text_only_batches_are_prompt_ids_own(gill):
  prompts = ["a photo of a cat", "two dogs on a beach at sunset"]
  ids, lens, images = gill._interleaved_ids(prompts)
  want_ids, want_lens = gill._prompt_ids(prompts)
  assert images is None and torch.equal(ids, want_ids) and torch.equal(lens, want_lens)
  t = torch.tensor([[2, 11, 12, 1, 1]])
  ids, lens, images = gill._interleaved_ids(t)
  assert images is None and torch.equal(ids, t) and lens.tolist() == [3]
  assert gill._shard_prompts(ids, lens, None, 0, 1)[2] == {}


def test_segmentation_bos_and_negative_slots(gill):
  a, b, c = _img(1), np.zeros((5, 6, 3), dtype=np.uint8), torch.zeros((4, 4, 3), dtype=torch.uint8)
  prompts = [[a, "first caption", b, "second one"], "plain text", (c,), ["only text here"]]
  ids, lens, images = gill._interleaved_ids(prompts)
  pad = gill.model.tokenizer.pad_token_id
  row0 = [-1, -2, -3, -4] + _tok(gill, "first caption", True) + [-5, -6, -7, -8] + _tok(gill, "second one", False)
  row1 = _tok(gill, "plain text", True)
  row2 = [-9, -10, -11, -12]                                   # images only: no <bos>, as the reference would build it
  row3 = _tok(gill, "only text here", True)
  assert row0[4] == gill.model.tokenizer.bos_token_id and row1[0] == row0[4] and gill.model.tokenizer.bos_token_id not in row0[5:]
  for r, want in enumerate((row0, row1, row2, row3)):
    assert lens[r].item() == len(want) and ids[r, :len(want)].tolist() == want and bool((ids[r, len(want):] == pad).all())
  assert [len(x) for x in images] == [2, 0, 1, 0] and images[0][0] is a and images[0][1] is b and images[2][0] is c
  # always_add_bos mirrors the reference's keyword: every string segment carries <bos>
  ids2, lens2, _ = gill._interleaved_ids(prompts[:1], always_add_bos=True)
  assert ids2[0, :lens2[0]].tolist() == [-1, -2, -3, -4] + _tok(gill, "first caption", True) + [-5, -6, -7, -8] + _tok(gill, "second one", True)


def test_a_shard_embeds_only_its_own_images_and_renumbers(gill, monkeypatch):
  imgs = [_img(i) for i in range(4)]
  prompts = [[imgs[0], "a"], "b", [imgs[1], imgs[2], "c"], [imgs[3]]]
  ids, lens, images = gill._interleaved_ids(prompts)
  seen = []

  def rows(mine):
    seen.append(list(mine))
    return torch.zeros((4 * len(mine), 128), dtype=torch.bfloat16)

  monkeypatch.setattr(gill, "_visual_rows", rows)
  sid, slen, kw = gill._shard_prompts(ids, lens, images, 2, 4)
  assert seen == [[imgs[1], imgs[2], imgs[3]]] and kw["extra_rows"].shape == (12, 128)
  assert sid[0, :8].tolist() == [-1, -2, -3, -4, -5, -6, -7, -8] and sid[1, :4].tolist() == [-9, -10, -11, -12]
  assert torch.equal(sid >= 0, ids[2:4] >= 0) and torch.equal(sid[sid >= 0], ids[2:4][ids[2:4] >= 0]) and torch.equal(slen, lens[2:4])
  sid, _, kw = gill._shard_prompts(ids, lens, images, 1, 2)       # a shard without images: the plain call, nothing embedded
  assert kw == {} and len(seen) == 1 and torch.equal(sid, ids[1:2])
  sid, _, kw = gill._shard_prompts(ids, lens, images, 4, 4)       # an empty shard
  assert kw == {} and sid.shape[0] == 0


def test_argument_errors_come_before_any_device_work(gill):
  with pytest.raises(ValueError, match="Input prompts should be either PIL.Image.Image or str types, got <class 'int'> instead."):
    gill.generate_images([[3]])
  with pytest.raises(ValueError, match="PIL.Image.Image or str types"):
    gill.generate_images([["text", torch.zeros((2, 5), dtype=torch.int64)]])       # an id tensor is a prompt of its own, not a segment
  with pytest.raises(ValueError, match="PIL.Image.Image or str types"):
    gill.generate_images([["text", np.zeros((4, 4, 3), dtype=np.float32)]])
  with pytest.raises(ValueError):
    gill.generate_images([["a"], 3])
  with pytest.raises(ValueError):
    gill.generate_images([[]])
  no_clip = _tiny_gill(with_clip=False)
  with pytest.raises(NotImplementedError, match="CLIP vision weights"):
    no_clip.generate_images([[_img(), "a caption"]])
  ids, _, images = no_clip._interleaved_ids([["just text"], "more"])            # lists without images need no tower
  assert [len(x) for x in images] == [0, 0] and bool((ids >= 0).all())
  # img_hidden_states refuses ids below -n_extra on its host copy (the library can only clamp them)
  with pytest.raises(ValueError, match="extra row 4 of 4"):
    gill.model.img_hidden_states(torch.tensor([[2, -5, 7]]), torch.tensor([2]), extra_rows=torch.zeros((4, 128), dtype=torch.bfloat16))
  with pytest.raises(ValueError, match="bfloat16"):
    gill.model.img_hidden_states(torch.tensor([[2, -1, 7]]), torch.tensor([2]), extra_rows=torch.zeros((4, 128)))
