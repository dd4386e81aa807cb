"""Host-side checks of the text-prompt path (no GPU): the synthetic text-tower weights carry the names and shapes of the pipeline's
actual dependency (transformers.CLIPTextModel), and GillSDPipeline's prompt handling follows _encode_prompt
(gill/custom_sd.py:258-373) — checked with a stub tokenizer and the encoder call replaced by a recorder."""
import pytest
import torch
import transformers  # noqa: F401  (plain import: a skip would hide the only parity evidence)

from gill_amd import synth
from gill_amd.sd import GillSDPipeline

from clip_text_util import StubTokenizer, hf_config, hf_last_hidden_state, hf_text_model, map_names


# ------------------------------------------------------------------------------------------------ 7. names and shapes
@pytest.mark.parametrize("name", ["tiny", "sd15", "sd21"])
def test_clip_text_state_dict_loads_strict_into_transformers(name):
  from transformers import CLIPTextModel
  cfg = getattr(synth.ClipTextConfig, name)()
  sd = synth.clip_text_state_dict(cfg, seed=3)
  assert all(k.startswith("text_model.") for k in sd), "published checkpoint names carry the text_model. prefix"
  with torch.device("meta"):          # names and shapes only: no second copy of a 340 M parameter tower
    m = CLIPTextModel(hf_config(cfg))
  want = {k: tuple(v.shape) for k, v in m.state_dict().items() if not k.endswith("position_ids")}
  got = {k: tuple(v.shape) for k, v in map_names(m, sd).items()}
  assert got == want
  m.load_state_dict(map_names(m, sd), strict=True, assign=True)
  assert cfg.hidden_size // cfg.num_heads == 64


def test_clip_text_geometries():
  a, b, t = synth.ClipTextConfig.sd15(), synth.ClipTextConfig.sd21(), synth.ClipTextConfig.tiny()
  assert (a.vocab_size, a.hidden_size, a.num_layers, a.num_heads, a.intermediate_size, a.max_positions, a.hidden_act) == \
         (49408, 768, 12, 12, 3072, 77, "quick_gelu")
  assert (b.vocab_size, b.hidden_size, b.num_layers, b.num_heads, b.intermediate_size, b.max_positions, b.hidden_act) == \
         (49408, 1024, 23, 16, 4096, 77, "gelu")
  assert (t.vocab_size, t.hidden_size, t.num_layers, t.num_heads, t.intermediate_size, t.max_positions) == (1000, 128, 2, 2, 256, 77)
  # deterministic: same seed, same tensors
  s1, s2 = synth.clip_text_state_dict(t, seed=5), synth.clip_text_state_dict(t, seed=5)
  assert all(torch.equal(s1[k], s2[k]) for k in s1)


def test_reference_tower_is_causal_without_a_mask():
  """What the GPU tests rely on: CLIPTextModel called with input_ids alone masks causally, so row t depends on ids[:t + 1] only."""
  cfg = synth.ClipTextConfig.tiny()
  m = hf_text_model(cfg, synth.clip_text_state_dict(cfg, seed=1))
  ids = torch.randint(0, cfg.vocab_size, (2, 20), generator=torch.Generator().manual_seed(0))
  a = hf_last_hidden_state(m, ids)
  ids2 = ids.clone()
  ids2[:, 7] = (ids2[:, 7] + 1) % cfg.vocab_size
  b = hf_last_hidden_state(m, ids2)
  assert torch.allclose(a[:, :7], b[:, :7], atol=1e-6) and not torch.allclose(a[:, 7], b[:, 7], atol=1e-3)


# ------------------------------------------------------------------------------------------------ 8. prompt handling
class _Recorder:
  """Stands in for GillSDPipeline.encode_prompt_ids: records the ids, returns a (B,77,D) float32 tensor that names its row."""

  def __init__(self, D=8):
    self.D, self.calls = D, []

  def __call__(self, ids, dtype=torch.float32):
    self.calls.append(ids.clone())
    return ids[:, :, None].to(dtype).expand(-1, -1, self.D).contiguous()


def _host_pipe(with_text=True):
  pipe = GillSDPipeline.__new__(GillSDPipeline)     # no GPU: only the prompt handling in front of the encoder is exercised
  pipe.truncate_side = "right"
  pipe.tokenizer = StubTokenizer() if with_text else None
  pipe.text_encoder = object() if with_text else None
  pipe.encode_prompt_ids = _Recorder()
  return pipe


def _long_prompt(n=100):
  return " ".join(f"w{i + 1}" for i in range(n))


def test_prompt_ids_tokenizer_arguments_and_rows():
  pipe = _host_pipe()
  out = pipe(prompt=["w5 w6", "w7"], return_prompts_only=True)
  (ids,) = pipe.encode_prompt_ids.calls
  assert ids.shape == (2, 77) and ids.dtype == torch.int64
  assert ids[0, :4].tolist() == [998, 5, 6, 999] and ids[1, :3].tolist() == [998, 7, 999] and (ids[:, 4:] == 999).all()
  call = pipe.tokenizer.calls[-1]
  assert call["padding"] == "max_length" and call["max_length"] == 77 and call["truncation"] is True
  assert out.dtype == torch.float32 and out.shape == (2, 77, 8)          # no negative half
  # a str is one prompt
  out1 = pipe(prompt="w5 w6", return_prompts_only=True)
  assert out1.shape == (1, 77, 8) and torch.equal(pipe.encode_prompt_ids.calls[-1][0], ids[0])
  # num_images_per_prompt repeats per prompt (custom_sd.py:313-316): a a b b
  out2 = pipe(prompt=["w5 w6", "w7"], return_prompts_only=True, num_images_per_prompt=2)
  assert out2.shape == (4, 77, 8)
  assert torch.equal(out2[0], out[0]) and torch.equal(out2[1], out[0]) and torch.equal(out2[2], out[1]) and torch.equal(out2[3], out[1])
  # return_prompts_only never encodes a negative prompt (custom_sd.py:589-591)
  n = len(pipe.encode_prompt_ids.calls)
  pipe(prompt=["w5"], negative_prompt=["w9"], return_prompts_only=True)
  assert len(pipe.encode_prompt_ids.calls) == n + 1


def test_truncate_side_right_keeps_the_head_left_keeps_the_tail():
  words = list(range(1, 101))
  pipe = _host_pipe()
  pipe(prompt=_long_prompt(100), return_prompts_only=True)
  ids = pipe.encode_prompt_ids.calls[-1]
  assert ids.shape == (1, 77) and ids[0, 0] == 998 and ids[0, -1] == 999
  assert ids[0, 1:76].tolist() == words[:75]
  pipe.truncate_side = "left"
  pipe(prompt=_long_prompt(100), return_prompts_only=True)
  ids = pipe.encode_prompt_ids.calls[-1]
  # custom_sd.py:272-274 decodes untruncated_ids[:, -1 - 77:-1] (the last 77 ids in front of the closing token) and tokenises that
  # text again with truncation, which frames it with BOS / EOS and so keeps its first 75 words
  tail = words[-77:]
  assert ids.shape == (1, 77) and ids[0, 0] == 998 and ids[0, -1] == 999
  assert ids[0, 1:76].tolist() == tail[:75]
  assert ids[0, 1] == 24 and 1 not in ids[0].tolist()
  # a prompt that fits is untouched by either side
  pipe(prompt="w5 w6", return_prompts_only=True)
  assert pipe.encode_prompt_ids.calls[-1][0, :4].tolist() == [998, 5, 6, 999]
  pipe.truncate_side = "middle"
  with pytest.raises(ValueError):
    pipe(prompt="w5", return_prompts_only=True)


def test_prompt_error_cases():
  pipe = _host_pipe()
  e = torch.zeros(1, 77, 8)
  with pytest.raises(ValueError, match="Cannot forward both `prompt`"):
    pipe(prompt="w5", prompt_embeds=e)
  with pytest.raises(ValueError, match="Cannot forward both `negative_prompt`"):
    pipe(prompt="w5", negative_prompt="w6", negative_prompt_embeds=e)
  with pytest.raises(ValueError, match="Provide either `prompt` or `prompt_embeds`"):
    pipe()
  with pytest.raises(ValueError, match="has to be of type `str` or `list`"):
    pipe(prompt=("w5",))
  with pytest.raises(TypeError, match="should be the same type"):          # custom_sd.py:323-327
    pipe(prompt=["w5"], negative_prompt="w6")
  with pytest.raises(TypeError, match="should be the same type"):
    pipe(prompt="w5", negative_prompt=["w6"])
  with pytest.raises(ValueError, match="has batch size 1, but `prompt`"):   # custom_sd.py:330-335
    pipe(prompt=["w5", "w6"], negative_prompt=["w7"])
  # without guidance the negative prompt is not looked at (do_classifier_free_guidance, custom_sd.py:319), so neither are its errors
  out = pipe(prompt=["w5"], negative_prompt="w6", return_prompts_only=True, guidance_scale=1.0)
  assert out.shape == (1, 77, 8)
  assert pipe.encode_prompt_ids.calls and all(c.shape[1] == 77 for c in pipe.encode_prompt_ids.calls)


def test_pipeline_without_text_weights_keeps_its_error():
  pipe = _host_pipe(with_text=False)
  with pytest.raises(ValueError, match="text prompts need the CLIP text encoder"):
    pipe(prompt="a red bicycle")
  with pytest.raises(ValueError, match="text prompts need the CLIP text encoder"):
    pipe(prompt=["a red bicycle"], return_prompts_only=True)
  assert pipe.encode_prompt_ids.calls == []


def test_encoder_refuses_attention_mask_configs_and_unknown_activations():
  from gill_amd.clip_text import GillClipTextEncoder
  import dataclasses
  cfg = dataclasses.replace(synth.ClipTextConfig.tiny(), use_attention_mask=True)
  with pytest.raises(ValueError, match="use_attention_mask"):
    GillClipTextEncoder({}, cfg, "cuda")
  with pytest.raises(ValueError, match="hidden_act"):
    GillClipTextEncoder({}, dataclasses.replace(synth.ClipTextConfig.tiny(), hidden_act="relu"), "cuda")


def test_native_create_reports_errors():
  """Out of range is an error code with a message, not a fault (host-only: create fails before it touches the device)."""
  import ctypes as C
  from gill_amd import _native as N
  lib = N.lib()
  h = C.c_void_p()
  assert lib.gill_clip_text_create(C.byref(h), None, None, 0) != 0 and lib.gill_last_error()
  arr = (N.gill_tensor * 1)()
  bad = N.gill_clip_text_config(vocab_size=1000, hidden_size=384, num_layers=1, num_heads=4, intermediate_size=256, max_positions=77,
                                hidden_act=0, max_batch=1)      # head dim 96: not an attention width
  assert lib.gill_clip_text_create(C.byref(h), C.byref(bad), arr, 0) != 0
  assert b"head dim" in lib.gill_last_error()
  bad = N.gill_clip_text_config(vocab_size=1000, hidden_size=128, num_layers=1, num_heads=2, intermediate_size=256, max_positions=77,
                                hidden_act=7, max_batch=1)
  assert lib.gill_clip_text_create(C.byref(h), C.byref(bad), arr, 0) != 0
  assert b"hidden_act" in lib.gill_last_error()
  assert lib.gill_clip_text_forward(None, None, 1, 1, None, None, None) != 0
