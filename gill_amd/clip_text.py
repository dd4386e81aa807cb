"""The CLIP text tower of the Stable Diffusion pipeline (`self.text_encoder`, gill/custom_sd.py:305-309) on libgill_amd.

`GillClipTextEncoder(ids)` is `transformers.CLIPTextModel(...)(input_ids)[0]`: last_hidden_state after final_layer_norm, causal
attention, no attention mask (gill_clip_text_forward: csrc/cliptext.hip).  Tokenisation is not part of it: ids come from a CPU
tokenizer object.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Union

import torch

from . import _native as N
from .synth import ClipTextConfig

_ACTS = {"quick_gelu": 0, "gelu": 1}


class GillClipTextEncoder:
  def __init__(self, state: Dict[str, torch.Tensor], cfg: ClipTextConfig, device: Union[str, torch.device] = "cuda",
               max_batch: int = 16):
    """`state`: the text_encoder state dict under the names of the published files (`text_model.` prefix; a bare
    `CLIPTextModel.state_dict()` of recent transformers lacks the prefix and must be mapped by the caller)."""
    if getattr(cfg, "use_attention_mask", False):
      raise ValueError("text-encoder configs with use_attention_mask=true are not supported (neither SD-1.5 nor SD-2.1 sets it): "
                       "the native tower runs without a padding mask, as custom_sd.py:300-303 does for them")
    if cfg.hidden_act not in _ACTS:
      raise ValueError(f"unsupported CLIP text hidden_act {cfg.hidden_act!r} (supported: {sorted(_ACTS)})")
    self.cfg = cfg
    self.device = torch.device(device if str(device) != "cuda" else "cuda:0")
    if self.device.type != "cuda":
      raise N.GillNativeError("GillClipTextEncoder runs only on an MI355X through libgill_amd")
    self.max_batch = int(max_batch)
    c = N.gill_clip_text_config(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, num_layers=cfg.num_layers,
                                num_heads=cfg.num_heads, intermediate_size=cfg.intermediate_size, max_positions=cfg.max_positions,
                                hidden_act=_ACTS[cfg.hidden_act], max_batch=self.max_batch)
    arr, keep = N.make_tensor_table(state, self.device)
    h = C.c_void_p()
    with torch.cuda.device(self.device):
      N.check(N.lib().gill_clip_text_create(C.byref(h), C.byref(c), arr, len(keep)))
    del keep
    self._h = h

  def __del__(self):
    try:
      if getattr(self, "_h", None):
        N.lib().gill_clip_text_destroy(self._h)
        self._h = None
    except Exception:
      pass

  def forward_device(self, ids_i32: torch.Tensor, out_bf16: Optional[torch.Tensor] = None,
                     out_f32: Optional[torch.Tensor] = None) -> None:
    """The raw call: ids (B,T) int32 already on the device and already validated, outputs (B,T,D) preallocated.  Enqueues on the
    current stream and returns; nothing synchronises, so it may run inside a graph capture."""
    assert ids_i32.dtype == torch.int32 and ids_i32.dim() == 2
    B, T = ids_i32.shape
    with torch.cuda.device(self.device):
      N.check(N.lib().gill_clip_text_forward(self._h, N.ptr(ids_i32), B, T, N.ptr(out_bf16), N.ptr(out_f32), N.current_stream()))

  def validate_ids(self, ids: torch.Tensor) -> torch.Tensor:
    """Host-side check of tokenizer output (the kernel indexes the embedding table with these): (B,T) int32 CPU tensor."""
    ids = torch.as_tensor(ids).detach().cpu()
    if ids.dim() != 2 or ids.dtype.is_floating_point or ids.dtype == torch.bool:
      raise ValueError(f"input ids must be an integer tensor of shape (batch, tokens), got {tuple(ids.shape)} {ids.dtype}")
    B, T = ids.shape
    if B < 1 or not 1 <= T <= self.cfg.max_positions:
      raise ValueError(f"input ids of shape {(B, T)}: need at least one row and 1..{self.cfg.max_positions} tokens per row")
    lo, hi = int(ids.min()), int(ids.max())
    if lo < 0 or hi >= self.cfg.vocab_size:
      raise ValueError(f"token id out of range: [{lo}, {hi}] for a vocabulary of {self.cfg.vocab_size}")
    return ids.to(torch.int32).contiguous()

  @torch.no_grad()
  def __call__(self, ids: torch.Tensor, dtype: torch.dtype = torch.float32, both: bool = False):
    """ids (B,T) integer tensor (any B: chunks of max_batch rows) -> (B,T,D) device tensor of `dtype` (float32 | bfloat16), or
    with both=True the pair (float32, bfloat16) of the same pass."""
    if dtype not in (torch.float32, torch.bfloat16):
      raise ValueError("dtype must be torch.float32 or torch.bfloat16")
    ids = self.validate_ids(ids).to(self.device)
    B, T = ids.shape
    shape = (B, T, self.cfg.hidden_size)
    f32 = torch.empty(shape, device=self.device, dtype=torch.float32) if (both or dtype == torch.float32) else None
    b16 = torch.empty(shape, device=self.device, dtype=torch.bfloat16) if (both or dtype == torch.bfloat16) else None
    for i in range(0, B, self.max_batch):
      j = min(B, i + self.max_batch)
      self.forward_device(ids[i:j], None if b16 is None else b16[i:j], None if f32 is None else f32[i:j])
    return (f32, b16) if both else (f32 if dtype == torch.float32 else b16)

  def flops(self, B: int, T: int) -> int:
    """FLOPs (2 per multiply-add) one forward needs: the four projections, the two MLP GEMMs and the causal half of the two
    attention products."""
    D, F, L = self.cfg.hidden_size, self.cfg.intermediate_size, self.cfg.num_layers
    return clip_text_flops(D, F, L, B, T)


def clip_text_flops(D: int, F: int, L: int, B: int, T: int) -> int:
  per_tok = 2 * (4 * D * D + 2 * D * F)
  attn = 2 * 2 * (T * (T + 1) // 2) * D
  return L * (B * T * per_tok + B * attn)
