"""Interleaved image + text prompts through the batched entries (GILL.generate_images / retrieve_images) and the id-driven OPT pass with visual
rows (gill_opt_img_hidden_ex), on the rig of tests/test_stages_gpu.py::test_image_prompt_vs_reference_golden: tiny CLIP at 32 px, opt-125m
shapes, the seeds of tests/golden/gill_visual_tiny.npz — which holds the reference's own gen_emb for [image, text] — plus the retrieval head,
the 24-row matrix and the local PNGs of tests/test_retrieve_images_gpu.py."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

from gill_amd import synth

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LONG = "a long text-only prompt about two brown dogs running along a beach at sunset with a red ball and a kite"


def _bfw(sd):
  return {k: v.bfloat16().float() for k, v in sd.items()}


def _mse(name, got, ref):
  got, ref = got.float().cpu(), torch.as_tensor(ref).float().cpu()
  mse = ((got - ref) ** 2).mean().item()
  print(f"[{name}] mse={mse:.3e} max_abs={(got - ref).abs().max().item():.3e} ref_rms={ref.pow(2).mean().sqrt().item():.3f}")
  return mse


@pytest.fixture(scope="module")
def rig(cuda, tmp_path_factory):
  from gill_amd.models import GILL
  g = np.load(os.path.join(GOLD, "gill_visual_tiny.npz"))
  tmp = tmp_path_factory.mktemp("interleaved_ret_images")
  ccfg = synth.ClipConfig.tiny()
  tok = synth.HashTokenizer()
  ocfg = synth.OptConfig(vocab_size=50274, hidden_size=768, num_layers=12, num_heads=12, ffn_dim=3072)
  args = SimpleNamespace(freeze_lm=True, freeze_vm=True, opt_version="facebook/opt-125m", visual_encoder="openai/clip-tiny",
                         n_visual_tokens=4, ret_emb_dim=256, gen_emb_dim=768, text_emb_layers=[-1], text_fc_mode="gill_mapper",
                         ret_text_fc_mode="linear", num_tokens=8, num_clip_tokens=77, retrieval_token_idx=synth.IMG_TOKEN_IDS,
                         gen_token_idx=synth.IMG_TOKEN_IDS, opt_state_dict=_bfw(synth.opt_state_dict(ocfg, seed=int(g["opt_seed"]))),
                         clip_state_dict=_bfw(synth.clip_state_dict(ccfg, seed=int(g["clip_seed"]))), clip_config=ccfg)
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
  proj = {}
  synth._linear(proj, "visual_embeddings", 4 * 768, ccfg.hidden_size, int(g["clip_seed"]))
  synth._linear(proj, "ret_text_hidden_fcs.0.model", 256, 768, int(g["clip_seed"]))
  with torch.no_grad():
    m.model.visual_embeddings.weight.copy_(proj["visual_embeddings.weight"].bfloat16().float())
    m.model.visual_embeddings.bias.copy_(proj["visual_embeddings.bias"].bfloat16().float())
    m.model.ret_text_hidden_fcs[0].model.weight.copy_(proj["ret_text_hidden_fcs.0.model.weight"].bfloat16().float())
    m.model.ret_text_hidden_fcs[0].model.bias.copy_(proj["ret_text_hidden_fcs.0.model.bias"].bfloat16().float())
  m.model.gen_text_hidden_fcs[0].load_state_dict(_bfw(synth.mapper_state_dict(synth.MapperConfig(in_dim=768), seed=int(g["mapper_seed"]))),
                                                 strict=True)
  m = m.eval().bfloat16().cuda()
  m.emb_matrix = emb_matrix.to(cuda)
  return SimpleNamespace(m=m, g=g, img=Image.fromarray(g["image"]), text=str(g["text"]), paths=paths, n_img=n_img, cuda=cuda)


def test_image_and_text_prompt_vs_reference_golden(rig):
  """generate_images([[image, text]]) against the reference's own gen_emb; bar: SD-embedding MSE < 1e-4, the project's stage-2 bar."""
  out = rig.m.generate_images([[rig.img, rig.text]])
  assert out.shape == (1, 77, 768)
  assert _mse("generate_images([[image, text]]) vs reference gen_emb", out, rig.g["gen_emb"]) < 1e-4
  # the same image as an array and as a device tensor: the same pixels, the same embedding
  a = rig.g["image"]
  assert torch.equal(rig.m.generate_images([[a, rig.text]]), out)
  assert torch.equal(rig.m.generate_images([(torch.from_numpy(a).to(rig.cuda), rig.text)]), out)


def test_ragged_batch_of_interleaved_and_text_prompts(rig):
  out = rig.m.generate_images([[rig.img, rig.text], LONG, (rig.img, rig.text)])
  assert out.shape == (3, 77, 768)
  for b in (0, 2):
    assert _mse(f"ragged batch row {b} vs reference gen_emb", out[b:b + 1], rig.g["gen_emb"]) < 1e-4
  alone = rig.m.generate_images([LONG])
  assert _mse("ragged batch row 1 vs the text-only call", out[1:2], alone) < 1e-4


def _ids16(seed):
  """(2,16) ids: 8 prompt positions with 4 negative slots at different columns per row, then the 8 [IMG] ids."""
  ids = synth.synthetic_prompt_ids(2, 8, seed=seed)[:, :8]
  ids = torch.cat([ids, torch.tensor([synth.IMG_TOKEN_IDS, synth.IMG_TOKEN_IDS], dtype=torch.int64)], dim=1)
  cols = (1, 4)
  ids[0, cols[0]:cols[0] + 4] = torch.tensor([-1, -2, -3, -4])
  ids[1, cols[1]:cols[1] + 4] = torch.tensor([-8, -7, -6, -5])       # its own rows, and not in table order
  return ids, cols


def test_img_hidden_ex_without_extras_is_img_hidden(rig):
  mm = rig.m.model
  ids = synth.synthetic_prompt_ids(2, 8, seed=41)
  assert ids.shape == (2, 16)
  last = torch.tensor([15, 15])
  raw0, emb0 = mm.img_hidden_states(ids.to(rig.cuda), last)
  raw1, emb1 = mm.img_hidden_states(ids.to(rig.cuda), last, extra_rows=torch.empty((0, 768), device=rig.cuda, dtype=torch.bfloat16))
  assert torch.equal(raw0, raw1) and torch.equal(emb0, emb1)


def test_img_hidden_ex_with_extras_vs_embeds_forward(rig):
  """raw against bf16 of gill_opt_forward's hidden rows at the same positions, fed the same embeddings assembled with gill_opt_embed +
  torch.cat.  Same B and T give the same launches up to the final LayerNorm, whose output is rounded to bf16 once here and through fp32 there:
  at most one flipped bf16 rounding, |a - b| <= 2^-7 |b| + 1e-5 elementwise (derived, not measured)."""
  mm = rig.m.model
  ids, cols = _ids16(seed=43)
  extra = (synth.normal("interleaved_extra_rows", (8, 768), 9) * 0.5).to(rig.cuda, torch.bfloat16)
  last = torch.tensor([15, 15])
  raw, emb = mm.img_hidden_states(ids.to(rig.cuda), last, extra_rows=extra)
  assert raw.shape == emb.shape == (2, 8, 768) and raw.dtype == emb.dtype == torch.bfloat16
  tok = mm.input_embeddings(ids.clamp(min=0).to(rig.cuda)).to(torch.bfloat16)            # gill_opt_embed
  x = torch.stack([torch.cat([tok[0, :cols[0]], extra[0:4], tok[0, cols[0] + 4:]], dim=0),
                   torch.cat([tok[1, :cols[1]], extra[[7, 6, 5, 4]], tok[1, cols[1] + 4:]], dim=0)], dim=0)
  hidden = mm._lm_forward_hidden(x)                                                       # gill_opt_forward, (2,16,768) fp32
  want = hidden[:, 8:16].to(torch.bfloat16).float()
  got = raw.float()
  err = (got - want).abs()
  bar = want.abs() * 2.0 ** -7 + 1e-5
  print(f"[img_hidden_ex with extras] max |a-b| {err.max().item():.3e}, worst ratio to the bar {(err / bar).max().item():.3f}, "
        f"rows differing {(err > 0).any(dim=-1).sum().item()} of 16")
  assert bool((err <= bar).all())
  assert torch.equal(emb, tok[:, 8:16])
  # the extra rows did go in: the same ids with another table give other hidden states
  raw2, _ = mm.img_hidden_states(ids.to(rig.cuda), last, extra_rows=torch.zeros_like(extra))
  assert not torch.equal(raw2, raw)
  # the emb_out gather takes extra rows as well: a window that ends inside the slots of row 0
  _, emb3 = mm.img_hidden_states(ids.to(rig.cuda), torch.tensor([8, 15]), extra_rows=extra)
  assert torch.equal(emb3[0], x[0, 1:9]) and torch.equal(emb3[1], tok[1, 8:16])


def test_ids_below_the_table_are_refused(rig):
  ids, _ = _ids16(seed=43)
  extra = torch.zeros((7, 768), device=rig.cuda, dtype=torch.bfloat16)                     # row 1 asks for the 8th row
  with pytest.raises(ValueError, match="extra row 7 of 7"):
    rig.m.model.img_hidden_states(ids.to(rig.cuda), torch.tensor([15, 15]), extra_rows=extra)


def test_retrieve_images_with_an_image_prompt(rig):
  """retrieve_images([[image, text]], k=3) against the 'ret' branch of the one-sequence path on the same prompt, through the same index."""
  m = rig.m
  m.build_retrieval_index()
  try:
    ret = m.generate_for_images_and_texts([rig.img, rig.text], num_words=2, gen_scale_factor=1e5)
    rets = ret[1]["ret"]
    want_idx = [int(np.asarray(r[0])[0, 0, 0]) // 7 for r in rets]              # red = 7 k mod 256, k < 24
    want_scores = np.array([r[2] for r in rets])
    out = m.retrieve_images([[rig.img, rig.text]], k=4)
    idx, scores = out.indices[0].cpu().tolist(), out.scores[0].cpu().numpy()
    gap = float(scores[2] - scores[3])
    print(f"[retrieve_images image prompt] idx {idx} scores {scores.tolist()} one-sequence idx {want_idx} scores {want_scores.tolist()} "
          f"gap 3rd-4th {gap:.4e}")
    assert len(want_idx) == 3
    top = m.retrieve_images([[rig.img, rig.text]], k=3)
    assert top.indices.shape == (1, 3) and top.indices[0].cpu().tolist() == idx[:3]
    if gap < 6e-3:
      assert set(idx[:3]) == set(want_idx)
      assert np.abs(np.sort(scores[:3]) - np.sort(want_scores)).max() < 3e-3
    else:
      assert idx[:3] == want_idx
      assert np.abs(scores[:3] - want_scores).max() < 3e-3
    assert top.paths == [[rig.paths[i] for i in idx[:3]]]
  finally:
    m.ret_index = None


def test_errors_and_image_only_prompts(rig):
  from gill_amd.models import GILL
  m = rig.m
  with pytest.raises(ValueError, match="Input prompts should be either PIL.Image.Image or str types"):
    m.generate_images([[3]])
  tok = synth.HashTokenizer()
  ocfg = synth.OptConfig(vocab_size=len(tok), hidden_size=128, num_layers=2, num_heads=2, ffn_dim=256, max_positions=128)
  args = SimpleNamespace(freeze_lm=True, freeze_vm=True, opt_version="facebook/opt-tiny-synth", visual_encoder="openai/clip-vit-base-patch16",
                         n_visual_tokens=4, ret_emb_dim=256, gen_emb_dim=768, text_emb_layers=[-1], text_fc_mode="gill_mapper",
                         ret_text_fc_mode="linear", num_tokens=8, num_clip_tokens=77, retrieval_token_idx=synth.IMG_TOKEN_IDS,
                         gen_token_idx=synth.IMG_TOKEN_IDS, opt_state_dict=synth.opt_state_dict(ocfg, seed=1))
  blind = GILL(tok, args, load_sd=False).eval().bfloat16().cuda()
  with pytest.raises(NotImplementedError, match="CLIP vision weights"):
    blind.generate_images([[rig.img, rig.text]])
  # images only: no <bos> (the reference adds it to the first string, and there is none); 4 visual rows + the 8 [IMG] ids
  ids, lens, images = m._interleaved_ids([[rig.img]])
  assert ids.tolist() == [[-1, -2, -3, -4]] and lens.tolist() == [4] and len(images[0]) == 1
  out = m.generate_images([[rig.img], [rig.img, rig.img]])
  assert out.shape == (2, 77, 768) and bool(torch.isfinite(out.float()).all())
  assert not torch.equal(out[0], out[1])
