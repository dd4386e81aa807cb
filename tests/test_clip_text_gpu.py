"""The CLIP text tower (gill_clip_text_forward: csrc/cliptext.hip) and the text-prompt path of GillSDPipeline on the MI355X.

Reference: transformers.CLIPTextModel(CLIPTextConfig(...)).eval() in fp32 on the CPU (the pipeline's actual dependency,
gill/custom_sd.py:305-309), holding the same bf16-rounded synthetic weights as the native tower, so the comparison measures the
arithmetic.  Bar for the parity tests: the project's bar for the 24-layer vision tower on the same arithmetic
(tests/test_stages_gpu.py:375), relative L2 < 3e-2 and cosine > 0.999.  Everything about determinism, causality and the pipeline is
checked bit for bit."""
import dataclasses
import json
import os

import pytest
import torch
import transformers  # noqa: F401  (plain import: a skip would hide the only parity evidence)

from gill_amd import synth

from clip_text_util import StubTokenizer, bfw, hf_last_hidden_state, hf_text_model, prompt_like_ids, stats

pytestmark = pytest.mark.gpu


def _encoder(cuda, cfg, seed, max_batch=4):
  from gill_amd.clip_text import GillClipTextEncoder
  sd = bfw(synth.clip_text_state_dict(cfg, seed=seed))
  return GillClipTextEncoder(sd, cfg, cuda, max_batch=max_batch), sd


@pytest.fixture(scope="module")
def tiny(cuda):
  cfg = synth.ClipTextConfig.tiny()
  enc, sd = _encoder(cuda, cfg, seed=11, max_batch=4)
  return enc, hf_text_model(cfg, sd), cfg


def _check_parity(name, enc, ref_model, ids):
  f32, b16 = enc(ids, both=True)
  torch.cuda.synchronize()
  ref = hf_last_hidden_state(ref_model, ids)
  assert f32.shape == ref.shape and f32.dtype == torch.float32 and b16.dtype == torch.bfloat16
  assert torch.isfinite(f32).all()
  _, rel, cos = stats(f"{name} fp32", f32, ref)
  _, rel16, cos16 = stats(f"{name} bf16", b16, ref)
  assert rel < 3e-2 and cos > 0.999
  assert rel16 < 3e-2 and cos16 > 0.999
  # the bf16 output is the round-to-nearest-even of the fp32 output of the same pass: they can never disagree
  assert torch.equal(b16, f32.bfloat16())
  return rel, cos


# ------------------------------------------------------------------------------------------------ 1. operator parity, tiny tower
@pytest.mark.parametrize("T", [1, 31, 32, 33, 64, 77])
def test_clip_text_tiny_vs_transformers(cuda, tiny, T):
  enc, ref_model, cfg = tiny
  ids = prompt_like_ids(cfg.vocab_size, 3, T, eos_positions=(T // 3, T - 1, 2 * T // 3), seed=T)
  _check_parity(f"clip text tiny T={T}", enc, ref_model, ids)


def test_clip_text_tiny_exact_gelu_vs_transformers(cuda):
  cfg = dataclasses.replace(synth.ClipTextConfig.tiny(), hidden_act="gelu")
  enc, sd = _encoder(cuda, cfg, seed=12, max_batch=3)
  ids = prompt_like_ids(cfg.vocab_size, 3, 77, eos_positions=(5, 40, 76), seed=2)
  _check_parity("clip text tiny gelu", enc, hf_text_model(cfg, sd), ids)


# ------------------------------------------------------------------------------------------------ 2. operator parity, real geometries
@pytest.mark.parametrize("name", ["sd15", "sd21"])
def test_clip_text_real_geometry_vs_transformers(cuda, name):
  """SD-1.5's tower (12 layers, D 768, QuickGELU) and SD-2.1's (23 layers, D 1024, exact GELU), vocab 49408, B = 4, T = 77, ids = BOS,
  random words, EOS at 1 / 10 / 40 / 76, EOS padding.
  Measured on the MI355X: see DESIGN.md section "CLIP text tower"."""
  cfg = getattr(synth.ClipTextConfig, name)()
  enc, sd = _encoder(cuda, cfg, seed=13, max_batch=4)
  ids = prompt_like_ids(cfg.vocab_size, 4, 77, eos_positions=(1, 10, 40, 76), seed=7)
  assert ids[0, 1] == cfg.vocab_size - 1 and ids[3, 76] == cfg.vocab_size - 1 and ids[3, 75] != cfg.vocab_size - 1
  _check_parity(f"clip text {name}", enc, hf_text_model(cfg, sd), ids)


# ------------------------------------------------------------------------------------------------ 3. causality is exact
@pytest.mark.parametrize("j", [1, 32, 76])
def test_clip_text_causality_is_exact(cuda, tiny, j):
  enc, _, cfg = tiny
  ids = prompt_like_ids(cfg.vocab_size, 3, 77, eos_positions=(76,), seed=5)
  a = enc(ids)
  ids2 = ids.clone()
  ids2[:, j] = (ids2[:, j] + 17) % (cfg.vocab_size - 2)
  assert (ids2[:, j] != ids[:, j]).all()
  b = enc(ids2)
  torch.cuda.synchronize()
  assert torch.equal(a[:, :j], b[:, :j]), "a later token changed an earlier row: masked keys must contribute exactly zero"
  for r in range(3):
    assert not torch.equal(a[r, j], b[r, j])


# ------------------------------------------------------------------------------------------------ 4. determinism, graph capture
def test_clip_text_deterministic_and_capturable(cuda, tiny):
  enc, _, cfg = tiny
  ids = enc.validate_ids(prompt_like_ids(cfg.vocab_size, 3, 77, eos_positions=(9, 30, 76), seed=8)).to(cuda)
  shape = (3, 77, cfg.hidden_size)
  a32, a16 = torch.empty(shape, device=cuda), torch.empty(shape, device=cuda, dtype=torch.bfloat16)
  b32, b16 = torch.empty(shape, device=cuda), torch.empty(shape, device=cuda, dtype=torch.bfloat16)
  enc.forward_device(ids, a16, a32)
  enc.forward_device(ids, b16, b32)
  torch.cuda.synchronize()
  assert torch.equal(a32, b32) and torch.equal(a16, b16)
  # no host synchronisation inside: the forward records into a graph on a side stream (one stream, linear) and replays to the same bits
  side = torch.cuda.Stream(device=cuda)
  g32, g16 = torch.zeros(shape, device=cuda), torch.zeros(shape, device=cuda, dtype=torch.bfloat16)
  torch.cuda.synchronize()
  with torch.cuda.stream(side):
    enc.forward_device(ids, g16, g32)          # the side stream's first use happens outside the capture
  side.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph, stream=side):
    enc.forward_device(ids, g16, g32)
  g32.zero_(), g16.zero_()
  torch.cuda.synchronize()
  graph.replay()
  torch.cuda.synchronize()
  assert torch.equal(g32, a32) and torch.equal(g16, a16)
  g32.zero_()
  graph.replay()
  torch.cuda.synchronize()
  assert torch.equal(g32, a32)


def test_clip_text_out_of_range_is_an_error(cuda, tiny):
  from gill_amd import _native as N
  enc, _, cfg = tiny
  out = torch.empty((5, 77, cfg.hidden_size), device=cuda)
  ids = torch.zeros((5, 77), dtype=torch.int32, device=cuda)
  with pytest.raises(N.GillNativeError, match="max_batch"):
    enc.forward_device(ids, None, out)                         # B = 5 > max_batch = 4
  with pytest.raises(N.GillNativeError, match="max_positions"):
    enc.forward_device(torch.zeros((1, 78), dtype=torch.int32, device=cuda), None, out)
  with pytest.raises(N.GillNativeError, match="no output"):
    enc.forward_device(ids[:1], None, None)
  with pytest.raises(ValueError, match="out of range"):
    enc(torch.full((1, 77), cfg.vocab_size, dtype=torch.int64))
  with pytest.raises(ValueError, match="out of range"):
    enc(torch.full((1, 77), -1, dtype=torch.int64))
  sd = bfw(synth.clip_text_state_dict(cfg, seed=11))
  del sd["text_model.encoder.layers.1.mlp.fc2.bias"]
  from gill_amd.clip_text import GillClipTextEncoder
  with pytest.raises(N.GillNativeError, match="missing weight tensor: text_model.encoder.layers.1.mlp.fc2.bias"):
    GillClipTextEncoder(sd, cfg, cuda, max_batch=1)
  # unknown extra keys are ignored, as the published files carry text_model.embeddings.position_ids
  sd = bfw(synth.clip_text_state_dict(cfg, seed=11))
  sd["text_model.embeddings.position_ids"] = torch.arange(77)[None]
  enc2 = GillClipTextEncoder(sd, cfg, cuda, max_batch=4)
  ids = prompt_like_ids(cfg.vocab_size, 2, 77, eos_positions=(9,), seed=1)
  assert torch.equal(enc2(ids), enc(ids))


# ------------------------------------------------------------------------------------------------ 5. pipeline
def _pipe(cuda, with_text=True, max_batch=4, text_max_batch=None):
  from gill_amd.sd import GillSDPipeline
  ucfg = synth.UNetConfig.tiny(16)
  tcfg = synth.ClipTextConfig.tiny()
  usd = bfw(synth.unet_state_dict(ucfg, seed=31))
  uncond = synth.uncond_context(ucfg.ctx_len, ucfg.cross_attention_dim, seed=31)
  if not with_text:
    return GillSDPipeline(usd, ucfg, uncond, cuda, max_batch=max_batch)
  return GillSDPipeline(usd, ucfg, uncond, cuda, max_batch=max_batch, text_state=bfw(synth.clip_text_state_dict(tcfg, seed=32)),
                        text_cfg=tcfg, tokenizer=StubTokenizer(tcfg.vocab_size), text_max_batch=text_max_batch)


@pytest.fixture(scope="module")
def pipe(cuda):
  return _pipe(cuda)


def _ids(pipe, texts):
  return pipe.tokenizer(texts, padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids


A, B_, C_, D_ = "a red bicycle leaning on a wall", "two dogs", "blurry low quality", "text watermark"


def test_pipeline_return_prompts_only(cuda, pipe):
  out = pipe(prompt=[A, B_], return_prompts_only=True)
  want = pipe.encode_prompt_ids(_ids(pipe, [A, B_]))
  assert out.dtype == torch.float32 and out.is_cuda and out.shape == (2, 77, 128)       # the prompts alone: no negative half
  assert torch.equal(out, want)
  assert out.detach().cpu().numpy().dtype.name == "float32"                            # what preprocess_sd_embeddings.py:71 does
  out2 = pipe(prompt=[A, B_], return_prompts_only=True, num_images_per_prompt=2)
  assert out2.shape == (4, 77, 128)
  assert torch.equal(out2[0], want[0]) and torch.equal(out2[1], want[0]) and torch.equal(out2[2], want[1]) and torch.equal(out2[3], want[1])
  one = pipe(A, return_prompts_only=True)                                              # positional str, as the reference's callers pass it
  assert one.shape == (1, 77, 128)
  assert not torch.equal(want[0], want[1])


def test_pipeline_prompt_equals_prompt_embeds(cuda, pipe):
  x = synth.initial_latents(2, 4, 16, seed=77)
  kw = dict(latents=x, output_type="latent", num_inference_steps=3)
  got = pipe(prompt=[A, B_], negative_prompt=[C_, D_], **kw).images
  pe, ne = pipe.encode_prompt_ids(_ids(pipe, [A, B_])), pipe.encode_prompt_ids(_ids(pipe, [C_, D_]))
  want = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, **kw).images
  torch.cuda.synchronize()
  assert torch.isfinite(got).all() and torch.equal(got, want)
  # the prompts matter (the comparison above is not between two constants)
  other = pipe(prompt=[B_, A], negative_prompt=[C_, D_], **kw).images
  assert not torch.equal(other, got)
  # negative_prompt=None means "" for every prompt (custom_sd.py:321-322)
  got0 = pipe(prompt=[A, B_], **kw).images
  want0 = pipe(prompt_embeds=pe, negative_prompt_embeds=pipe.encode_prompt_ids(_ids(pipe, [""])), **kw).images
  torch.cuda.synchronize()
  assert torch.equal(got0, want0) and not torch.equal(got0, got)
  # one str prompt with one str negative prompt
  g1 = pipe(prompt=A, negative_prompt=C_, latents=x[:1], output_type="latent", num_inference_steps=3).images
  w1 = pipe(prompt_embeds=pipe.encode_prompt_ids(_ids(pipe, [A])), negative_prompt_embeds=pipe.encode_prompt_ids(_ids(pipe, [C_])),
            latents=x[:1], output_type="latent", num_inference_steps=3).images
  assert torch.equal(g1, w1)


def test_pipeline_truncate_side(cuda, pipe, monkeypatch):
  seen = []
  real = pipe.encode_prompt_ids
  monkeypatch.setattr(pipe, "encode_prompt_ids", lambda ids, dtype=torch.float32: (seen.append(ids.clone()), real(ids, dtype))[1])
  words = list(range(1, 101))
  long_prompt = " ".join(f"w{i}" for i in words)
  assert pipe.truncate_side == "right"
  head = pipe(prompt=long_prompt, return_prompts_only=True)
  assert seen[-1][0, 1:76].tolist() == words[:75] and seen[-1][0, 0] == 998 and seen[-1][0, 76] == 999
  monkeypatch.setattr(pipe, "truncate_side", "left")
  tail = pipe(prompt=long_prompt, return_prompts_only=True)
  # custom_sd.py:272-274: the last 77 ids in front of the closing token are decoded and tokenised again (with truncation)
  assert seen[-1][0, 1:76].tolist() == words[-77:][:75] and seen[-1][0, 0] == 998 and seen[-1][0, 76] == 999
  assert not torch.equal(head, tail)


def test_pipeline_prompt_errors(cuda, pipe):
  e = torch.zeros(1, 77, 128)
  with pytest.raises(ValueError, match="Cannot forward both `prompt`"):
    pipe(prompt=A, prompt_embeds=e)
  with pytest.raises(ValueError, match="Cannot forward both `negative_prompt`"):
    pipe(prompt=A, negative_prompt=C_, negative_prompt_embeds=e)
  with pytest.raises(TypeError, match="should be the same type"):
    pipe(prompt=[A], negative_prompt=C_)
  with pytest.raises(ValueError, match="has batch size 1, but `prompt`"):
    pipe(prompt=[A, B_], negative_prompt=[C_])
  with pytest.raises(ValueError, match="Provide either `prompt` or `prompt_embeds`"):
    pipe()
  bare = _pipe(cuda, with_text=False)
  with pytest.raises(ValueError, match="text prompts need the CLIP text encoder"):
    pipe_out = bare(prompt="a red bicycle")
  assert bare.text_encoder is None
  from gill_amd.sd import GillSDPipeline
  ucfg = synth.UNetConfig.tiny(16)
  with pytest.raises(ValueError, match="use_attention_mask"):
    GillSDPipeline(bfw(synth.unet_state_dict(ucfg, seed=31)), ucfg, synth.uncond_context(77, 128, seed=31), cuda, max_batch=2,
                   text_state={}, text_cfg=dataclasses.replace(synth.ClipTextConfig.tiny(), use_attention_mask=True),
                   tokenizer=StubTokenizer())


def test_pipeline_chunks_prompts_beyond_max_batch(cuda, pipe):
  assert pipe.text_encoder.max_batch == 4
  texts = [f"w{i} w{i + 1} w{2 * i + 3}" + " w7" * (i % 5) for i in range(1, 11)]       # 10 prompts: chunks of 4, 4, 2
  ids = _ids(pipe, texts)
  out = pipe(prompt=texts, return_prompts_only=True)
  assert out.shape == (10, 77, 128)
  for i in range(0, 10, 4):
    assert torch.equal(out[i:i + 4], pipe.encode_prompt_ids(ids[i:i + 4]))
  b16 = pipe.encode_prompt_ids(ids, dtype=torch.bfloat16)
  assert b16.dtype == torch.bfloat16 and torch.equal(b16, out.bfloat16())


# ------------------------------------------------------------------------------------------------ 6. from_pretrained
def test_from_pretrained_encodes_the_empty_prompt_natively(cuda, tmp_path, monkeypatch):
  from safetensors.torch import save_file
  from gill_amd.sd import GillSDPipeline
  ucfg, tcfg = synth.UNetConfig.tiny(16), synth.ClipTextConfig.tiny()
  root = str(tmp_path)
  os.makedirs(os.path.join(root, "unet")), os.makedirs(os.path.join(root, "text_encoder"))
  with open(os.path.join(root, "unet", "config.json"), "w") as f:
    json.dump(dict(in_channels=4, out_channels=4, block_out_channels=list(ucfg.block_out_channels), layers_per_block=2,
                   cross_attention_dim=ucfg.cross_attention_dim, attention_head_dim=ucfg.num_heads, norm_num_groups=32, sample_size=16), f)
  save_file({k: v.contiguous() for k, v in bfw(synth.unet_state_dict(ucfg, seed=41)).items()},
            os.path.join(root, "unet", "diffusion_pytorch_model.safetensors"))
  with open(os.path.join(root, "text_encoder", "config.json"), "w") as f:
    json.dump(dict(vocab_size=tcfg.vocab_size, hidden_size=tcfg.hidden_size, num_hidden_layers=tcfg.num_layers,
                   num_attention_heads=tcfg.num_heads, intermediate_size=tcfg.intermediate_size, max_position_embeddings=77,
                   hidden_act="quick_gelu", layer_norm_eps=1e-5), f)
  tsd = bfw(synth.clip_text_state_dict(tcfg, seed=42))
  tsd["text_model.embeddings.position_ids"] = torch.arange(77)[None]                    # as in the published files
  save_file({k: v.contiguous() for k, v in tsd.items()}, os.path.join(root, "text_encoder", "model.safetensors"))

  def _no(*a, **k):
    raise AssertionError("transformers' model classes must not be instantiated when the native tower can load the weights")
  monkeypatch.setattr(transformers.CLIPTextModel, "from_pretrained", _no)
  tok = StubTokenizer(tcfg.vocab_size)
  pipe = GillSDPipeline.from_pretrained(root, device=cuda, max_batch=2, tokenizer=tok)
  assert pipe.text_encoder is not None and pipe.tokenizer is tok
  want = pipe.encode_prompt_ids(_ids(pipe, [""]), dtype=torch.bfloat16)
  assert pipe.uncond_embeds.dtype == torch.bfloat16 and pipe.uncond_embeds.shape == (1, 77, 128)
  assert torch.equal(pipe.uncond_embeds, want) and pipe.uncond_embeds.float().abs().max() > 0
  # ... which agrees with the host computation it replaces to rounding
  ref = hf_last_hidden_state(hf_text_model(tcfg, bfw(synth.clip_text_state_dict(tcfg, seed=42))), _ids(pipe, [""]))
  _, rel, cos = stats("from_pretrained uncond_embeds", pipe.uncond_embeds, ref)
  assert rel < 3e-2 and cos > 0.999
  # and the pipeline runs from text end to end
  lat = pipe(prompt="w3 w4", latents=synth.initial_latents(1, 4, 16, seed=5), num_inference_steps=2).images
  assert lat.shape == (1, 4, 16, 16) and torch.isfinite(lat).all()
  # weights without any tokenizer: a clear error, not a silent host fallback
  with pytest.raises(ValueError, match="tokenizer"):
    GillSDPipeline.from_pretrained(root, device=cuda, max_batch=2)
