"""Shared by test_clip_text_host.py and test_clip_text_gpu.py (not a test module): the reference for the CLIP text tower, built from
the pipeline's actual dependency (transformers.CLIPTextModel, fp32 on the CPU), and a stub tokenizer with the Hugging Face call
signature _encode_prompt uses (gill/custom_sd.py:266-284, :340-346)."""
import re
import zlib
from types import SimpleNamespace

import torch


def hf_config(cfg):
  from transformers import CLIPTextConfig
  return CLIPTextConfig(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
                        num_hidden_layers=cfg.num_layers, num_attention_heads=cfg.num_heads,
                        max_position_embeddings=cfg.max_positions, hidden_act=cfg.hidden_act, layer_norm_eps=1e-5,
                        bos_token_id=cfg.vocab_size - 2, eos_token_id=cfg.vocab_size - 1, pad_token_id=cfg.vocab_size - 1)


def map_names(model, sd):
  """Checkpoint-file names (`text_model.` prefix) -> the names this transformers version's CLIPTextModel.state_dict() uses (5.x
  dropped the prefix; 4.x has it)."""
  if any(k.startswith("text_model.") for k in model.state_dict()):
    return dict(sd)
  return {k[len("text_model."):]: v for k, v in sd.items()}


def hf_text_model(cfg, sd):
  """CLIPTextModel(CLIPTextConfig(...)).eval() in fp32 holding `sd` (strict)."""
  from transformers import CLIPTextModel
  m = CLIPTextModel(hf_config(cfg)).eval().float()
  m.load_state_dict(map_names(m, sd), strict=True)
  return m


def hf_last_hidden_state(model, ids):
  with torch.no_grad():
    return model(ids.long())[0].float()


def bfw(sd):
  return {k: v.bfloat16().float() for k, v in sd.items()}


def stats(name, got, ref):
  """Same statistic as tests/test_stages_gpu.py:_stats."""
  got, ref = got.float().cpu(), ref.float().cpu()
  mse = ((got - ref) ** 2).mean().item()
  rel = ((got - ref).norm() / ref.norm().clamp_min(1e-12)).item()
  cos = torch.nn.functional.cosine_similarity(got.flatten(), ref.flatten(), dim=0).item()
  print(f"[{name}] mse={mse:.3e} rel_l2={rel:.3e} cos={cos:.6f} max_abs={(got - ref).abs().max().item():.3e} "
        f"ref_rms={ref.pow(2).mean().sqrt().item():.3f}")
  return mse, rel, cos


def prompt_like_ids(vocab, B, T, eos_positions, seed):
  """(B,T) int64 the way the CLIP tokenizer pads: BOS, random words, EOS at eos_positions[b] (clipped to T - 1), EOS after it."""
  g = torch.Generator().manual_seed(seed)
  bos, eos = vocab - 2, vocab - 1
  ids = torch.randint(0, vocab - 2, (B, T), generator=g, dtype=torch.int64)
  ids[:, 0] = bos
  for b in range(B):
    e = min(int(eos_positions[b % len(eos_positions)]), T - 1)
    if e >= 1:
      ids[b, e:] = eos
  return ids


class StubTokenizer:
  """Whitespace words -> ids: 'w<n>' is id n (so batch_decode round-trips), anything else hashes into [0, vocab - 2).  BOS = vocab - 2,
  EOS = pad = vocab - 1, as CLIPTokenizer frames and pads its rows.  Records every call."""
  model_max_length = 77

  def __init__(self, vocab=1000):
    self.vocab = vocab
    self.bos_token_id, self.eos_token_id = vocab - 2, vocab - 1
    self.calls = []

  def _word(self, w):
    m = re.fullmatch(r"w(\d+)", w)
    if m and int(m.group(1)) < self.vocab - 2:
      return int(m.group(1))
    return zlib.crc32(w.encode()) % (self.vocab - 2)

  def __call__(self, text, padding=False, max_length=None, truncation=False, return_tensors=None):
    texts = [text] if isinstance(text, str) else list(text)
    self.calls.append(dict(text=text, padding=padding, max_length=max_length, truncation=truncation))
    rows = []
    for t in texts:
      ids = [self.bos_token_id] + [self._word(w) for w in t.split()] + [self.eos_token_id]
      if truncation and max_length is not None and len(ids) > max_length:
        ids = ids[:max_length - 1] + [self.eos_token_id]
      rows.append(ids)
    width = max_length if padding == "max_length" else max(len(r) for r in rows)
    rows = [r + [self.eos_token_id] * (width - len(r)) for r in rows]
    assert return_tensors == "pt"
    return SimpleNamespace(input_ids=torch.tensor(rows, dtype=torch.int64))

  def batch_decode(self, ids):
    out = []
    for row in ids:
      out.append(" ".join(f"w{int(t)}" for t in row if int(t) < self.vocab - 2))
    return out
