"""Mirror of the reference's public surface gill/models.py — GILLArgs, GILLModel, GILL, load_gill — for the
image-generation hot path, with every FLOP in libgill_amd (hand-written HIP for MI355X).

Reference map (file:line in /root/reference/gill/models.py):
  GILLArgs                                   :21-36
  GILLModel.__init__ / get_visual_embs       :40-126 / :129-152
  GILLModel.forward (three modes)            :164-441  (label loops :202-227 / :277-298, :358-362; rows :374-387, :416-435)
  GILLModel.generate                         :443-532
  GILL.__init__ / __call__                   :536-561 / :563-580
  GILL.generate_for_images_and_texts         :582-762  ('gen' branch: :600-662, :706-731, :754-762)
  load_gill                                  :810-902
New here (NOT in the reference): GILL.generate_images — the batched entry whose
per-prompt semantics are the 'gen' branch of generate_for_images_and_texts([p], num_words=2, gen_scale_factor=1e5).

Also built: image prompts through the native CLIP vision tower (get_visual_embs), KV-cached decoding in
generate(), the retrieval / decision / CLIP-rerank branches of generate_for_images_and_texts, load_gill with the cc3m*.npy
retrieval embeddings; the captioning / retrieval / generation scoring modes of GILLModel.forward as gill/validate.py:66-120 calls
them (loss, token accuracy and the retrieval features, through the fused LM-head loss kernel: DESIGN.md section 7).  Out of scope
(raise NotImplementedError): concat_captions, an augmentation of main.py's training step; gradients.
"""
from __future__ import annotations

import ctypes as C
import glob
import json
import os
from collections import namedtuple
from types import SimpleNamespace
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor

from . import _native as N
from . import layers, utils
from .synth import ClipConfig, OptConfig


class GILLArgs:
  freeze_lm: bool = True
  freeze_vm: bool = True
  opt_version: str = 'facebook/opt-6.7b'
  visual_encoder: str = 'openai/clip-vit-large-patch14'
  n_visual_tokens: int = 1
  task: str = 'captioning'
  ret_emb_dim: Optional[int] = 256
  gen_emb_dim: Optional[int] = 256
  text_emb_layers: List[int] = [-1]
  gen_token_idx: List[int] = [0]
  retrieval_token_idx: List[int] = [0]
  text_fc_mode: str = 'gill_mapper'
  ret_text_fc_mode: str = 'linear'
  num_tokens: int = 8
  num_clip_tokens: int = 77


_OPT_SHAPES = {  # hidden, layers, heads, ffn  (public OPT configs; 350m is post-LN + project_in/out: unsupported)
  'opt-125m': (768, 12, 12, 3072), 'opt-1.3b': (2048, 24, 32, 8192), 'opt-2.7b': (2560, 32, 32, 10240),
  'opt-6.7b': (4096, 32, 32, 16384), 'opt-13b': (5120, 40, 40, 20480),
}
_OPT_WEIGHT_MODES = {'bf16': 0, 'fp8': 1}      # GILL_OPT_BF16, GILL_OPT_W8 (include/gill_amd.h)
_KV_CACHE_FORMATS = {'bf16': 0, 'fp8': 1}      # GILL_KV_BF16, GILL_KV_E4M3
_CLIP_HIDDEN = {'clip-vit-large-patch14': 1024, 'clip-vit-base-patch16': 768, 'clip-vit-base-patch32': 768}


class _ParamTree(nn.Module):
  """Parameter container whose state_dict() keys reproduce a given set of dotted names (so a module tree of
  transformers' OPTForCausalLM can be held — and checkpoint-loaded — without running any of its code)."""

  def __init__(self, state: Dict[str, Tensor]):
    super().__init__()
    for name, t in state.items():
      mod = self
      parts = name.split('.')
      for p in parts[:-1]:
        if p not in mod._modules:
          mod.add_module(p, _ParamTree({}))
        mod = mod._modules[p]
      mod.register_parameter(parts[-1], nn.Parameter(t, requires_grad=False))


class _NativeEmbedding(nn.Module):
  """`input_embeddings`: shares the OPT token-embedding parameter; lookup runs in libgill_amd (gill_opt_embed)."""

  def __init__(self, owner: "GILLModel", weight: nn.Parameter):
    super().__init__()
    self.weight = weight
    self._owner = [owner]   # list: keep the back-reference out of nn.Module's child registry
    self.embedding_dim = weight.shape[1]
    self.num_embeddings = weight.shape[0]

  def forward(self, ids: Tensor) -> Tensor:
    owner = self._owner[0]
    h = owner._opt_native(1, 1)
    ids = ids.to(self.weight.device, torch.int64).contiguous()
    out = torch.empty(tuple(ids.shape) + (self.embedding_dim,), device=self.weight.device, dtype=torch.bfloat16)
    with torch.cuda.device(self.weight.device):
      N.check(N.lib().gill_opt_embed(h, N.ptr(ids), ids.numel(), N.ptr(out), N.current_stream()))
    return out.to(self.weight.dtype)


class GILLModel(nn.Module):
  def __init__(self, tokenizer, args: GILLArgs = GILLArgs()):
    super().__init__()
    self.tokenizer = tokenizer
    self.feature_extractor = utils.get_feature_extractor_for_model(args.visual_encoder, train=False)   # models.py:48
    self.image_token = self.tokenizer.cls_token_id
    assert args.text_emb_layers != set(args.text_emb_layers), 'text_emb_layers not unique'
    self.args = args
    self.num_tokens = args.num_tokens
    self.num_clip_tokens = args.num_clip_tokens

    opt_version = args.opt_version
    visual_encoder = args.visual_encoder
    n_visual_tokens = args.n_visual_tokens
    print(f"Using {opt_version} for the language model.")
    print(f"Using {visual_encoder} for the visual model with {n_visual_tokens} visual tokens.")

    if 'facebook/opt' not in opt_version:
      raise NotImplementedError
    self.opt_version = opt_version
    self.opt_cfg, lm_state = self._load_opt(opt_version, len(tokenizer), getattr(args, 'opt_state_dict', None))
    self.lm = _ParamTree(lm_state)
    self.lm.config = SimpleNamespace(word_embed_proj_dim=self.opt_cfg.hidden_size, hidden_size=self.opt_cfg.hidden_size,
                                     num_hidden_layers=self.opt_cfg.num_layers)
    print("Freezing the LM.")   # the LM is always frozen here: this package is inference-only

    self.retrieval_token_idx = args.retrieval_token_idx
    self.gen_token_idx = args.gen_token_idx
    self.input_embeddings = _NativeEmbedding(self, self.lm.model.decoder.embed_tokens.weight)

    self.visual_model_name = visual_encoder
    # frozen CLIP vision tower (models.py:78-96): a parameter container; its forward runs in libgill_amd (gill_clip_*).
    # Weights: args.clip_state_dict (synthetic / pre-loaded), a local Hugging Face directory, or absent — then text prompts
    # work as always and image prompts raise.
    self.clip_cfg, clip_state = self._load_clip(visual_encoder, getattr(args, 'clip_state_dict', None),
                                                getattr(args, 'clip_config', None))
    self.visual_model = _ParamTree(clip_state) if clip_state is not None else None
    hidden_size = self.clip_cfg.hidden_size if self.clip_cfg is not None else self._clip_hidden(visual_encoder)
    if self.clip_cfg is not None and self.clip_cfg.image_size != self.feature_extractor.size:
      self.feature_extractor = utils.ClipImageProcessor(self.clip_cfg.image_size, self.clip_cfg.image_size)
    self._clip_handle = None

    embedding_dim = self.input_embeddings.embedding_dim * self.args.n_visual_tokens
    self.ret_text_hidden_fcs = nn.ModuleList([])
    self.gen_text_hidden_fcs = nn.ModuleList([])
    for layer_idx in self.args.text_emb_layers:
      if (layer_idx == -1 or layer_idx == self.lm.config.num_hidden_layers) and ('bert' not in opt_version):
        in_dim = self.lm.config.word_embed_proj_dim
      elif layer_idx < self.lm.config.num_hidden_layers:
        raise NotImplementedError('only text_emb_layers=[-1] (the shipped configuration) is supported')
      else:
        raise ValueError(f'Embedding of layer {layer_idx} was requested but model only has {self.lm.config.num_hidden_layers} layers.')
      self.ret_text_hidden_fcs.append(
        layers.TextFcLayer(in_dim, self.args.ret_emb_dim, num_input_tokens=self.args.num_tokens,
                           num_output_tokens=1, mode=self.args.ret_text_fc_mode))
      self.gen_text_hidden_fcs.append(
        layers.TextFcLayer(in_dim, self.args.gen_emb_dim, num_input_tokens=self.args.num_tokens,
                           num_output_tokens=self.args.num_clip_tokens, mode=self.args.text_fc_mode))

    # parameters of the out-of-scope branches are kept so reference checkpoints load with matching keys
    self.visual_embeddings = nn.Linear(hidden_size, embedding_dim)
    self.visual_fc = nn.Linear(hidden_size, self.args.ret_emb_dim)
    self.logit_scale = nn.Parameter(torch.ones([]) * np.log(1 / 0.07))
    self._opt_handle = None
    self._opt_cap = (0, 0)
    self._cache_epoch = 0         # bumped by every entry that writes or rebuilds the handle's KV cache: open sessions go stale (dialogue.py)
    self.opt_weights = 'bf16'     # quantize_lm(): 'fp8' = the weight-only fp8 decoder (gill_opt_create_ex, GILL_OPT_W8)
    self.kv_cache = 'bf16'        # quantize_kv(): 'fp8' = the e4m3 KV cache (gill_opt_set_kv_format, GILL_KV_E4M3)
    # native handles snapshot the weights: a state-dict load into this module (or, recursively, into a parent) drops them
    self.register_load_state_dict_post_hook(lambda module, incompatible_keys: module.refresh_native())

  # ---- weights -------------------------------------------------------------------------------
  @staticmethod
  def _clip_hidden(name: str) -> int:
    for k, v in _CLIP_HIDDEN.items():
      if k in name:
        return v
    raise NotImplementedError(f'unknown visual encoder {name}')

  @staticmethod
  def _load_opt(opt_version: str, vocab: int, state: Optional[Dict[str, Tensor]]):
    """Returns (OptConfig, OPTForCausalLM-named state dict with embeddings resized to `vocab` (models.py:73))."""
    if state is not None:   # caller-supplied weights (synthetic weights for tests / benchmarks)
      D = state['model.decoder.embed_tokens.weight'].shape[1]
      n_layers = 1 + max(int(k.split('.')[3]) for k in state if k.startswith('model.decoder.layers.'))
      F = state['model.decoder.layers.0.fc1.weight'].shape[0]
      shape = [v for k, v in _OPT_SHAPES.items() if k in opt_version]
      heads = shape[0][2] if shape and shape[0][0] == D else max(1, D // 64)
      heads = getattr(state, 'num_heads', heads)
      cfg = OptConfig(vocab_size=vocab, hidden_size=D, num_layers=n_layers, num_heads=heads, ffn_dim=F,
                      max_positions=state['model.decoder.embed_positions.weight'].shape[0] - 2)
      sd = dict(state)
    else:                   # the reference's way: transformers is the weight loader (never the executor)
      from transformers import OPTForCausalLM
      hf = OPTForCausalLM.from_pretrained(opt_version)
      c = hf.config
      if not c.do_layer_norm_before or c.word_embed_proj_dim != c.hidden_size:
        raise NotImplementedError('post-LN / projected OPT variants (opt-350m) are not supported')
      cfg = OptConfig(vocab_size=vocab, hidden_size=c.hidden_size, num_layers=c.num_hidden_layers,
                      num_heads=c.num_attention_heads, ffn_dim=c.ffn_dim, max_positions=c.max_position_embeddings)
      sd = {k: v for k, v in hf.state_dict().items() if k != 'lm_head.weight'}   # tied to embed_tokens
    emb = sd['model.decoder.embed_tokens.weight']
    if emb.shape[0] != vocab:   # resize_token_embeddings(len(tokenizer)): new rows ~ N(0, 0.02) like HF's _init_weights
      new = torch.empty((vocab, emb.shape[1]), dtype=emb.dtype).normal_(0.0, 0.02)
      n = min(vocab, emb.shape[0])
      new[:n] = emb[:n]
      sd['model.decoder.embed_tokens.weight'] = new
    return cfg, sd

  @staticmethod
  def _load_clip(name: str, state: Optional[Dict[str, Tensor]], cfg: Optional[ClipConfig]):
    """(ClipConfig, CLIPVisionModel-named state dict) or (None, None) when no vision weights are available offline."""
    if state is not None:
      if cfg is None:
        D = state['vision_model.embeddings.class_embedding'].shape[0]
        P = state['vision_model.embeddings.patch_embedding.weight'].shape[-1]
        ntok = state['vision_model.embeddings.position_embedding.weight'].shape[0]
        n_layers = 1 + max(int(k.split('.')[3]) for k in state if k.startswith('vision_model.encoder.layers.'))
        F = state['vision_model.encoder.layers.0.mlp.fc1.weight'].shape[0]
        cfg = ClipConfig(image_size=int(round((ntok - 1) ** 0.5)) * P, patch_size=P, hidden_size=D, num_layers=n_layers,
                         num_heads=max(1, D // 64), intermediate_size=F)
      return cfg, dict(state)
    if os.path.isdir(name) and os.path.exists(os.path.join(name, 'config.json')):   # local HF directory
      from transformers import CLIPVisionModel
      hf = CLIPVisionModel.from_pretrained(name)
      c = hf.config
      sd = {(k if k.startswith('vision_model.') else 'vision_model.' + k): v for k, v in hf.state_dict().items()}
      return ClipConfig(image_size=c.image_size, patch_size=c.patch_size, hidden_size=c.hidden_size,
                        num_layers=c.num_hidden_layers, num_heads=c.num_attention_heads,
                        intermediate_size=c.intermediate_size), sd
    return None, None

  def _require_vision(self):
    if self.visual_model is None:
      raise NotImplementedError('image prompts need the CLIP vision weights (args.clip_state_dict or a local '
                                'openai/clip-vit-* directory): none were available when this model was built')

  def _clip_native(self, B: int):
    dev = self.logit_scale.device
    if dev.type != 'cuda':
      raise N.GillNativeError('GILLModel runs only on an MI355X through libgill_amd; call .cuda() first.')
    self._require_vision()
    if self._clip_handle is not None and B <= self._clip_cap:
      return self._clip_handle
    if self._clip_handle is not None:
      N.lib().gill_clip_destroy(self._clip_handle)
      self._clip_handle = None
    c = self.clip_cfg
    cap = max(B, 4)
    cfg = N.gill_clip_config(image_size=c.image_size, patch_size=c.patch_size, hidden_size=c.hidden_size,
                             num_layers=c.num_layers, num_heads=c.num_heads, intermediate_size=c.intermediate_size,
                             max_batch=cap)
    arr, keep = N.make_tensor_table(self.visual_model.state_dict(), dev)
    h = C.c_void_p()
    with torch.cuda.device(dev):
      N.check(N.lib().gill_clip_create(C.byref(h), C.byref(cfg), arr, len(keep)))
    del keep
    self._clip_handle, self._clip_cap = h, cap
    return h

  def _apply(self, fn, *a, **k):
    self.release_native()
    return super()._apply(fn, *a, **k)

  def release_native(self):
    if getattr(self, '_opt_handle', None):
      N.lib().gill_opt_destroy(self._opt_handle)
    self._opt_handle = None
    self._opt_cap = (0, 0)
    if getattr(self, '_clip_handle', None):
      N.lib().gill_clip_destroy(self._clip_handle)
    self._clip_handle = None

  def refresh_native(self):
    """Call after mutating weights in place once a forward has already run (handles snapshot the weights)."""
    self._cache_epoch += 1
    self.release_native()
    for fcs in (self.gen_text_hidden_fcs, getattr(self, 'ret_text_hidden_fcs', [])):
      for fc in fcs:
        if hasattr(fc, 'release_native'):
          fc.release_native()

  def __del__(self):
    try:
      self.release_native()
    except Exception:
      pass

  def _opt_native(self, B: int, T: int):
    dev = self.logit_scale.device
    if dev.type != 'cuda':
      raise N.GillNativeError('GILLModel runs only on an MI355X through libgill_amd; call .cuda() first '
                              '(there is no CPU implementation in this package).')
    cb, ct = self._opt_cap
    if self._opt_handle is not None and B <= cb and T <= ct:
      return self._opt_handle
    self._cache_epoch += 1
    self.release_native()
    cb, ct = max(cb, B, 8), max(ct, T, 64)
    c = self.opt_cfg
    cfg = N.gill_opt_config(vocab_size=c.vocab_size, hidden_size=c.hidden_size, num_layers=c.num_layers,
                            num_heads=c.num_heads, ffn_dim=c.ffn_dim, max_positions=c.max_positions, max_batch=cb, max_seq=ct)
    arr, keep = N.make_tensor_table(self.lm.state_dict(), dev)
    h = C.c_void_p()
    with torch.cuda.device(dev):
      N.check(N.lib().gill_opt_create_ex(C.byref(h), C.byref(cfg), arr, len(keep), _OPT_WEIGHT_MODES[self.opt_weights]))
    del keep
    if self.kv_cache != 'bf16' and N.lib().gill_opt_set_kv_format(h, _KV_CACHE_FORMATS[self.kv_cache]) != 0:
      msg = N.lib().gill_last_error()
      N.lib().gill_opt_destroy(h)
      raise N.GillNativeError(msg.decode() if msg else 'gill_opt_set_kv_format failed')
    self._opt_handle, self._opt_cap = h, (cb, ct)
    return h

  def quantize_lm(self, mode: Optional[str] = 'fp8'):
    """Weight format of the OPT decoder's native handle.  'fp8': weight-only fp8 (OCP e4m3, one power-of-two scale per output row) for the
    four matrices of every decoder layer.  The decode steps then read half the weight bytes: the ragged step of generate_batch /
    generate_for_images_and_texts_batch at up to 16 rows, and every KV-cached step of generate() (greedy, seeded draw and host-decision
    paths, and with it generate_for_images_and_texts) that carries at most 16 rows in all, batch x new tokens: single tokens at batch <= 16
    and the 8-token [IMG] block at batch 1.  Every other pass (the prefill, a step of more than 16 rows, generate(use_kv_cache=False), the
    training-style forwards, the retrieval and likelihood scores) runs the dequantised weights on the bf16 kernels: the same model, no
    speed-up.  The handle holds both copies: about 1.5 x the decoder weights of a bf16 handle.  None or 'bf16': back to bf16.  The handle is
    rebuilt at the next call."""
    mode = 'bf16' if mode is None else mode
    if mode not in _OPT_WEIGHT_MODES:
      raise ValueError(f"quantize_lm: mode must be one of {sorted(_OPT_WEIGHT_MODES)} or None, got {mode!r}")
    if mode != self.opt_weights:
      self._cache_epoch += 1
      self.opt_weights = mode
      if self._opt_handle is not None:
        N.lib().gill_opt_destroy(self._opt_handle)
      self._opt_handle, self._opt_cap = None, (0, 0)
    return self

  def quantize_kv(self, mode: Optional[str] = 'fp8'):
    """Format of the KV cache in the OPT decoder's native handle.  'fp8': every key row and value row of a (token, head) is stored as OCP
    e4m3 bytes with one power-of-two scale (csrc/attention_kv8_dev.h), about half the cache bytes; every key and value, a token's own
    included, is e4m3-rounded before any query uses it, so the tokens can differ from those of the bf16 cache, and they are the same however
    the sequence was fed.  The entries that honour it are the ragged ones: generate_batch (its prefill then runs through the packed extend
    pass at lengths 0), generate_for_images_and_texts_batch, open_session / open_dialogues; with either weight format.  generate() with
    use_kv_cache, the cached forward and generate_for_images_and_texts raise a ValueError (their flash kernel writes and reads a bf16 cache):
    a batch of one row through the batch entries is the equivalent.  Entries that use no cache are untouched.  None or 'bf16': back to bf16.
    A change drops the handle (rebuilt at the next call) and makes open sessions stale."""
    mode = 'bf16' if mode is None else mode
    if mode not in _KV_CACHE_FORMATS:
      raise ValueError(f"quantize_kv: mode must be one of {sorted(_KV_CACHE_FORMATS)} or None, got {mode!r}")
    if mode != self.kv_cache:
      self._cache_epoch += 1
      self.kv_cache = mode
      if self._opt_handle is not None:
        N.lib().gill_opt_destroy(self._opt_handle)
      self._opt_handle, self._opt_cap = None, (0, 0)
    return self

  def _require_bf16_kv(self, what: str):
    if self.kv_cache != 'bf16':
      raise ValueError(f"{what} runs on a bf16 KV cache only and this model's is {self.kv_cache!r} (quantize_kv): use generate_batch / "
                       f"generate_for_images_and_texts_batch / open_session (a batch of one row is the equivalent), or quantize_kv('bf16').")

  # ---- reference API -------------------------------------------------------------------------
  def get_visual_embs(self, pixel_values: torch.FloatTensor, mode: str = 'captioning'):
    if mode not in ['captioning', 'retrieval', 'generation']:
      raise ValueError(f"mode should be one of ['captioning', 'retrieval', 'generation'], got {mode} instead.")
    if mode == 'generation':   # models.py:147-148: the image is ignored
      return torch.zeros((pixel_values.shape[0], 1, 768), device=pixel_values.device)
    # models.py:137-146: pooler_output of the frozen tower -> visual_embeddings / visual_fc -> (B, n_visual_tokens | 1, D)
    from . import ops
    px = pixel_values.to(self.logit_scale.device, torch.float32).contiguous()
    B = px.shape[0]
    h = self._clip_native(B)
    pooled = torch.empty((B, self.clip_cfg.hidden_size), device=px.device, dtype=torch.float32)
    with torch.cuda.device(px.device):
      N.check(N.lib().gill_clip_forward(h, N.ptr(px), B, N.ptr(pooled), N.current_stream()))
    fc = self.visual_embeddings if mode == 'captioning' else self.visual_fc
    out = ops.gemm(pooled.to(torch.bfloat16), fc.weight, bias=fc.bias, out_f32=True)
    n_tok = self.args.n_visual_tokens if mode == 'captioning' else 1
    return out.reshape(B, n_tok, -1).to(self.logit_scale.dtype)

  def train(self, mode=True):
    super(GILLModel, self).train(mode=mode)   # reference quirk kept: returns None (models.py:155-161)

  def _lm_forward_hidden(self, inputs_embeds: Tensor) -> Tensor:
    """self.lm(inputs_embeds=..., output_hidden_states=True).hidden_states[-1]  (models.py:363-365 / :465)."""
    B, T, D = inputs_embeds.shape
    h = self._opt_native(B, T)
    x = inputs_embeds.to(torch.bfloat16).contiguous()
    out = torch.empty((B, T, D), device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
      N.check(N.lib().gill_opt_forward(h, N.ptr(x), B, T, N.ptr(out), N.current_stream()))
    return out

  def _lm_forward_hidden_cached(self, new_embeds: Tensor, past_len: int) -> Tensor:
    """hidden_states[-1] rows of the tokens past_len .. past_len+T_new-1, computed against the handle's KV cache
    (gill_opt_forward_cached).  past_len == 0 starts a new sequence."""
    B, Tn, D = new_embeds.shape
    self._require_bf16_kv('the cached forward')
    self._cache_epoch += 1
    cb, ct = self._opt_cap
    if past_len > 0 and (self._opt_handle is None or B > cb or past_len + Tn > ct):
      # growing would rebuild the handle and lose the keys / values cached so far
      raise N.GillNativeError(f'KV cache of the OPT handle holds {ct} tokens x {cb} sequences; step needs {past_len + Tn} x {B}. '
                              f'generate() sizes it up front (max_positions = {self.opt_cfg.max_positions}).')
    h = self._opt_native(B, past_len + Tn)
    x = new_embeds.to(torch.bfloat16).contiguous()
    out = torch.empty((B, Tn, D), device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
      N.check(N.lib().gill_opt_forward_cached(h, N.ptr(x), B, Tn, past_len, N.ptr(out), N.current_stream()))
    return out

  def img_hidden_states(self, labels: Tensor, last_embedding_idx: Tensor, extra_rows: Optional[Tensor] = None):
    """Fast path of forward(mode='generation'): (B,T) ids, (B,) idx -> (raw (B,8,D), embs (B,8,D)) bf16.  extra_rows (n,D) bf16: the
    embedding rows of image prompts (models.py:606-613, 625); an id < 0 selects row -(id + 1) of them (gill_opt_img_hidden_ex)."""
    B, T = labels.shape
    dev = self.logit_scale.device
    D = self.opt_cfg.hidden_size
    n_extra = 0
    if extra_rows is not None:
      if extra_rows.dim() != 2 or extra_rows.shape[1] != D or extra_rows.dtype != torch.bfloat16:
        raise ValueError(f'extra_rows must be (n, {D}) bfloat16, got {tuple(extra_rows.shape)} {extra_rows.dtype}')
      extra_rows = extra_rows.to(dev).contiguous()
      n_extra = extra_rows.shape[0]
      lowest = int(labels.min()) if labels.numel() else 0
      if lowest < -n_extra:      # the library clamps what it cannot check (the ids live on the device): refuse here
        raise ValueError(f'id {lowest} selects extra row {-(lowest + 1)} of {n_extra}')
    h = self._opt_native(B, T)
    ids = labels.to(dev, torch.int64).contiguous()
    li = [int(v) for v in last_embedding_idx.reshape(-1).tolist()]
    arr = (C.c_int32 * B)(*li)
    raw = torch.empty((B, self.num_tokens, D), device=dev, dtype=torch.bfloat16)
    emb = torch.empty((B, self.num_tokens, D), device=dev, dtype=torch.bfloat16)
    with torch.cuda.device(dev):
      if extra_rows is None:
        N.check(N.lib().gill_opt_img_hidden(h, N.ptr(ids), arr, B, T, self.num_tokens, N.ptr(raw), N.ptr(emb), N.current_stream()))
      else:
        N.check(N.lib().gill_opt_img_hidden_ex(h, N.ptr(ids), arr, B, T, self.num_tokens, N.ptr(extra_rows) if n_extra else None, n_extra,
                                               N.ptr(raw), N.ptr(emb), N.current_stream()))
    return raw, emb

  def _full_labels(self, labels: Tensor, mode: str, n_front: int) -> Tensor:
    """full_labels of the reference's label loops, vectorised: n_front columns of -100 (visual rows and / or prefix), then `labels` with
    everything from the first stop token on set to -100.  The two regimes stop at different tokens and are kept apart:
      captioning (models.py:202-227): pad, or ANY retrieval / generation token id;
      retrieval / generation (:277-298, :358-362): pad, or a retrieval / generation token id other than the first of its list."""
    front = torch.full((labels.shape[0], n_front), -100, dtype=torch.int64, device=labels.device)
    full = torch.cat([front, labels.to(torch.int64)], dim=1)
    if mode == 'captioning':
      stops = [self.tokenizer.pad_token_id] + list(self.retrieval_token_idx) + list(self.gen_token_idx)
    else:
      stops = [self.tokenizer.pad_token_id] + list(self.retrieval_token_idx[1:]) + list(self.gen_token_idx[1:])
    stop = torch.zeros_like(full, dtype=torch.bool)
    for tok in stops:
      stop |= (full == tok)
    return torch.where(stop.cumsum(dim=1) > 0, torch.full_like(full, -100), full)

  def _lm_head_weight(self) -> Tensor:
    sd = self.lm.state_dict()
    return sd['lm_head.weight'] if 'lm_head.weight' in sd else sd['model.decoder.embed_tokens.weight']

  def lm_forward_loss(self, ids: Tensor, full_labels: Tensor, last_embedding_idx: Optional[Tensor] = None,
                      extra_rows: Optional[Tensor] = None, want_rows: bool = False, want_last_logit: bool = False,
                      want_hidden: bool = False):
    """One scoring pass of the LM (gill_opt_forward_loss): ids (B,T) with negative ids naming rows of extra_rows (n,D) bf16, full_labels
    (B,T) with -100 ignored; row (b,t) is scored against full_labels[b,t+1] by the fused LM-head loss kernel: no (B,T,vocab) tensor.
    Returns a namespace: token_loss / token_rank (B,T-1), summary (4) = [mean loss, n_valid, #top-1, #top-5], and on request raw / emb
    (B,num_tokens,D) bf16 (the rows img_hidden_states returns), last_logit (B,vocab) fp32 (logits row last_embedding_idx - 1),
    hidden (B,T,D) fp32."""
    B, T = ids.shape
    dev = self.logit_scale.device
    D, V = self.opt_cfg.hidden_size, self.opt_cfg.vocab_size
    if T < 2:
      raise ValueError('scoring needs at least two positions (the labels are shifted by one)')
    n_extra = 0
    if extra_rows is not None:
      extra_rows = extra_rows.to(dev, torch.bfloat16).contiguous()
      n_extra = extra_rows.shape[0]
      assert extra_rows.dim() == 2 and extra_rows.shape[1] == D, extra_rows.shape
    ids = ids.to(dev, torch.int64).contiguous()
    full_labels = full_labels.to(dev, torch.int64).contiguous()
    # the library clamps what it cannot check (ids and labels live on the device): refuse here, with one host read
    lo, hi = int(ids.min()), int(ids.max())
    if lo < -n_extra or hi >= V:
      raise ValueError(f'ids span [{lo}, {hi}]: outside the vocabulary of {V} and the {n_extra} extra rows')
    bad = (full_labels != -100) & ((full_labels < 0) | (full_labels >= V))
    if bool(bad.any()):
      raise ValueError(f'label {int(full_labels[bad][0])} is neither -100 nor a token of [0, {V})')
    h = self._opt_native(B, T)
    arr = None
    if want_rows or want_last_logit:
      arr = (C.c_int32 * B)(*[int(v) for v in last_embedding_idx.reshape(-1).tolist()])
    out = SimpleNamespace(raw=None, emb=None, last_logit=None, hidden=None)
    if want_rows:
      out.raw = torch.empty((B, self.num_tokens, D), device=dev, dtype=torch.bfloat16)
      out.emb = torch.empty((B, self.num_tokens, D), device=dev, dtype=torch.bfloat16)
    if want_last_logit:
      out.last_logit = torch.empty((B, V), device=dev, dtype=torch.float32)
    if want_hidden:
      out.hidden = torch.empty((B, T, D), device=dev, dtype=torch.float32)
    out.token_loss = torch.empty((B, T - 1), device=dev, dtype=torch.float32)
    out.token_rank = torch.empty((B, T - 1), device=dev, dtype=torch.int32)
    out.summary = torch.empty((4,), device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
      N.check(N.lib().gill_opt_forward_loss(h, N.ptr(ids), arr, B, T, self.num_tokens, N.ptr(extra_rows) if n_extra else None, n_extra,
                                            N.ptr(full_labels), N.ptr(out.raw), N.ptr(out.emb), N.ptr(out.token_loss), N.ptr(out.token_rank),
                                            N.ptr(out.summary), N.ptr(out.last_logit), N.ptr(out.hidden), N.current_stream()))
    return out

  def forward(self, pixel_values: torch.FloatTensor, labels: Optional[torch.LongTensor] = None,
              caption_len: Optional[torch.LongTensor] = None, mode: str = 'captioning', concat_captions: bool = False,
              input_prefix: Optional[str] = None, lm_loss: Optional[bool] = None, return_logits: bool = False):
    """The reference's forward (models.py:164-441) in its three modes.  lm_loss (default: True for captioning / retrieval, False for
    generation) scores the sequence: output.loss is HF's mean shifted cross-entropy over the valid tokens of the batch, a 0-d fp32 device
    tensor, with output.token_loss / output.token_rank (B, T-1) and output.n_tokens beside it, all from the fused LM-head loss kernel;
    output.logits stays None unless return_logits, which materialises (B, T, vocab) fp32 through ops.gemm.  mode='generation' with the
    defaults runs the hidden-rows-only pass and leaves loss / logits / last_output_logit / input_embs_norm None, as it always has."""
    if concat_captions:
      raise NotImplementedError("concat_captions is an augmentation of the reference's training step (main.py); not built")
    if mode not in ('captioning', 'retrieval', 'generation'):
      raise ValueError(f"mode should be one of ['captioning', 'retrieval', 'generation'], got {mode} instead.")
    if lm_loss is None:
      lm_loss = mode != 'generation'
    if mode != 'generation' and not lm_loss:
      raise ValueError(f"mode={mode!r} exists to score the sequence: lm_loss=False is only meaningful for mode='generation'")
    score = lm_loss or return_logits
    visual_embs = self.get_visual_embs(pixel_values, mode)
    batch_size, vis_seq_len = visual_embs.shape[0], visual_embs.shape[1]
    assert labels.shape[0] == batch_size, (visual_embs.shape, labels.shape)
    visual_embs_norm = ((visual_embs ** 2).sum(dim=-1) ** 0.5).mean()
    dev = self.logit_scale.device
    labels = labels.to(dev)
    last_embedding_idx = caption_len.to(dev) - 1 if caption_len is not None else None   # models.py:183

    # the id matrix of inputs_embeds: [visual rows (captioning) | prefix | labels]; a visual row is the id -(row + 1) of extra_rows
    front = []
    extra_rows = None
    if mode == 'captioning':
      n_vis = batch_size * vis_seq_len
      front.append(-(torch.arange(n_vis, device=dev, dtype=torch.int64).reshape(batch_size, vis_seq_len) + 1))
      extra_rows = visual_embs.reshape(n_vis, -1).to(torch.bfloat16)
    if input_prefix is not None:
      prompt_ids = self.tokenizer(input_prefix, add_special_tokens=False, return_tensors="pt").input_ids.to(dev)   # models.py:186
      front.append(prompt_ids.to(torch.int64).reshape(1, -1).repeat(batch_size, 1))
    n_front = sum(f.shape[1] for f in front)
    ids = torch.cat(front + [labels.to(torch.int64)], dim=1) if front else labels
    if last_embedding_idx is not None:
      last_embedding_idx = last_embedding_idx + n_front          # models.py:200, :209, :283
    full_labels = self._full_labels(labels, mode, n_front)

    dt = self.logit_scale.dtype
    input_embs_norm = None
    if score:
      input_embs = self.input_embeddings(labels)                 # models.py:180-181
      input_embs_norm = ((input_embs ** 2).sum(dim=-1) ** 0.5).mean()

    last_embedding = None
    last_output_logit = None
    llm_hidden_states = []
    want_rows = mode in ('retrieval', 'generation')
    if not score:
      raw, emb = self.img_hidden_states(ids, last_embedding_idx)      # models.py:363-365, 384-385
      output = SimpleNamespace(loss=None, logits=None, hidden_states=None)       # LM loss/logits were not asked for
    else:
      r = self.lm_forward_loss(ids, full_labels, last_embedding_idx, extra_rows, want_rows=want_rows, want_last_logit=want_rows,
                               want_hidden=return_logits)
      raw, emb, last_output_logit = r.raw, r.emb, r.last_logit
      logits = None
      if return_logits:
        from . import ops
        B, T, D = r.hidden.shape
        head = self._lm_head_weight().to(dev, torch.bfloat16)
        V = head.shape[0]
        if V % 4:      # ops.gemm takes N % 4 == 0 (GILL's 50274 is not): zero rows behind the head, cut off again
          head = torch.cat([head, head.new_zeros((4 - V % 4, D))], dim=0)
        logits = ops.gemm(r.hidden.reshape(B * T, D).to(torch.bfloat16), head, out_f32=True).reshape(B, T, -1)[..., :V]
      output = SimpleNamespace(loss=r.summary[0], logits=logits, hidden_states=None, token_loss=r.token_loss, token_rank=r.token_rank,
                               n_tokens=r.summary[1], summary=r.summary)
    if want_rows:
      text_hidden_fcs = self.ret_text_hidden_fcs if mode == 'retrieval' else self.gen_text_hidden_fcs
      llm_hidden_states = [raw.to(dt)]
      hidden = [fc(raw.to(dt), emb.to(dt)) for fc in text_hidden_fcs]            # models.py:387
      last_embedding = torch.stack(hidden, dim=-1).sum(dim=-1)                   # models.py:418
      if mode == 'retrieval':                                                    # models.py:425-435
        assert visual_embs.shape[1] == 1, visual_embs.shape
        assert last_embedding.shape[1] == 1, last_embedding.shape
        visual_embs = visual_embs[:, 0, :]
        visual_embs = visual_embs / visual_embs.norm(dim=1, keepdim=True)
        last_embedding = last_embedding[:, 0, :]
        last_embedding = last_embedding / last_embedding.norm(dim=1, keepdim=True)
        visual_embs = self.logit_scale.exp() * visual_embs
    return output, full_labels, last_embedding, last_output_logit, visual_embs, visual_embs_norm, input_embs_norm, llm_hidden_states

  # The decision of the generate loop (:471-520) runs on the device: the [IMG] logit rule, the greedy pick, the [IMG] forcing and
  # the next step's embeddings (gill_opt_next_token), and the rule, the temperature and the top-p filter of the sampled path
  # (gill_opt_decode_logits / gill_opt_filter_logits); with generate(seed=...) the sampled path's draw runs there too
  # (gill_opt_sample_token).  False runs the reference's host decision instead (A/B and test arm).
  decode_on_device = True
  _decode_host_waits = 0      # instrumentation: host waits inside the loop of the last generate() call

  def _decode_rule(self, step: int, min_word_tokens: int, ret_scale_factor: float, gen_scale_factor: float,
                   filter_value: float):
    """gill_decode_rule of loop step `step` (the arguments of :476-489)."""
    ret, gen = list(self.retrieval_token_idx), list(self.gen_token_idx)
    if len(ret) > 16 or len(gen) > 16:
      raise NotImplementedError('the on-device decode rule takes at most 16 retrieval / generation token ids')
    r = N.gill_decode_rule()
    r.n_ret, r.n_gen = len(ret), len(gen)
    for j, v in enumerate(ret):
      r.ret_ids[j] = int(v)
    for j, v in enumerate(gen):
      r.gen_ids[j] = int(v)
    r.step, r.min_word_tokens, r.ret_eq_gen = int(step), int(min_word_tokens), int(ret == gen)
    r.ret_scale, r.gen_scale, r.filter_value = float(ret_scale_factor), float(gen_scale_factor), float(filter_value)
    return r

  def generate(self, embeddings=torch.FloatTensor, max_len: int = 32, temperature: float = 0.0, top_p: float = 1.0,
               min_word_tokens: int = 0, ret_scale_factor: float = 1.0, gen_scale_factor: float = 1.0,
               filter_value: float = -float('Inf'), use_kv_cache: bool = True, seed: Optional[int] = None):
    """Greedy / top-p decoding, same loop and outputs as the reference (models.py:443-532).  The reference re-runs the
    whole sequence through the LM at every step; with use_kv_cache (default) only the tokens appended since the last
    step go through the layers, against keys/values cached in the native handle — causal attention makes the hidden
    states of earlier positions independent of later tokens, so the outputs are the same up to rounding.
    After quantize_lm('fp8') the cached steps behind the prefill run on the e4m3 weight bytes wherever batch x new tokens <= 16
    (gill_opt_cached_uses_w8); the prefill and use_kv_cache=False stay on the bf16 kernels.
    With decode_on_device (default) the logit rule and the pick run in libgill_amd: greedy decoding at batch > 1 never
    waits for the device inside the loop, at batch 1 it reads one 4-byte count per step (the [IMG] forcing decides how
    many tokens the next forward takes).  Outputs: out (N,T) token ids, output_embeddings list of hidden_states[-1],
    output_logits list (N, vocab) — CPU tensors when top_p == 1 (:471-472), device tensors otherwise.
    seed (an integer; None, the default, is the reference's torch.multinomial draw from torch's generator): with a temperature
    above 0 the draw runs in libgill_amd too (gill_opt_sample_token: an exponential race on Philox uniforms keyed by (seed, row,
    step), over exp(logit / temperature - max) and the top-p filter's kept set).  It is repeatable bit for bit, a row's tokens do
    not depend on the other rows of the batch, no temperature overflows, torch's generators are not touched, and the loop waits
    for the device as the greedy one does: never at batch > 1, one 4-byte count per step at batch 1."""
    if use_kv_cache:
      self._require_bf16_kv('generate() with use_kv_cache')
    self._decode_host_waits = 0
    self._cache_epoch += 1
    if seed is not None:
      if not self.decode_on_device:
        raise ValueError('seed needs decode_on_device: the seeded draw runs in libgill_amd only.')
      seed = int(seed)
      if not 0 <= seed < 2 ** 64:
        raise ValueError(f'seed should be in [0, 2**64), got {seed} instead.')
    if self.decode_on_device and temperature == 0.0 and top_p == 1.0:
      return self._generate_device(embeddings, max_len, min_word_tokens, ret_scale_factor, gen_scale_factor, filter_value,
                                   use_kv_cache)
    if seed is not None and temperature != 0.0:
      if top_p < 1.0:
        assert top_p > 0, f'top_p should be above 0, got {top_p} instead.'
      return self._generate_device(embeddings, max_len, min_word_tokens, ret_scale_factor, gen_scale_factor, filter_value,
                                   use_kv_cache, sample=(float(temperature), float(top_p), seed))
    with torch.no_grad():
      out = None
      output_embeddings = []
      output_logits = []
      dev = embeddings.device
      vocab = self.opt_cfg.vocab_size
      hidden = None
      if use_kv_cache:
        self._size_kv_cache(embeddings, max_len)
      for i in range(max_len):
        if use_kv_cache:
          past = 0 if hidden is None else hidden.shape[1]
          new_hidden = self._lm_forward_hidden_cached(embeddings[:, past:], past)
          hidden = new_hidden if hidden is None else torch.cat([hidden, new_hidden], dim=1)
        else:
          hidden = self._lm_forward_hidden(embeddings)                         # :465
        for idx in self.args.text_emb_layers:
          output_embeddings.append(hidden.to(embeddings.dtype))                # :467-468
        B, T, D = hidden.shape
        logits = torch.empty((B, vocab), device=dev, dtype=torch.float32)
        if self.decode_on_device:
          # :470-512 in libgill_amd: lm_head + rule (in place: what output_logits holds), then division + top-p out of place;
          # the draw stays torch.multinomial on the device the reference's tensor is on
          rule = self._decode_rule(i, min_word_tokens, ret_scale_factor, gen_scale_factor, filter_value)
          with torch.cuda.device(dev):
            N.check(N.lib().gill_opt_decode_logits(self._opt_handle, N.ptr(hidden), B, T, C.byref(rule), N.ptr(logits),
                                                   N.current_stream()))
          if temperature == 0.0:
            raise ValueError('top_p cannot be set if temperature is 0 (greedy decoding).')
          if top_p < 1.0:
            assert top_p > 0, f'top_p should be above 0, got {top_p} instead.'
          probs_in = torch.empty_like(logits)
          with torch.cuda.device(dev):
            N.check(N.lib().gill_opt_filter_logits(self._opt_handle, N.ptr(logits), N.ptr(probs_in), B, float(temperature),
                                                   float(top_p), float(filter_value), int(top_p != 1.0), N.current_stream()))
          if top_p == 1.0:
            logits, probs_in = logits.cpu(), probs_in.cpu()                    # :471-472: the host tensors of the reference
            self._decode_host_waits += 1
          output_logits.append(logits)
          next_token = torch.multinomial(probs_in.exp(), 1)
        else:
          with torch.cuda.device(dev):
            N.check(N.lib().gill_opt_last_logits(self._opt_handle, N.ptr(hidden), B, T, N.ptr(logits), N.current_stream()))
          if top_p == 1.0:
            logits = logits.cpu()                                              # :471-472
            self._decode_host_waits += 1
          output_logits.append(logits)
          logits[:, self.retrieval_token_idx[1:]] = filter_value               # :476-477
          logits[:, self.gen_token_idx[1:]] = filter_value
          if (self.retrieval_token_idx or self.gen_token_idx) and self.retrieval_token_idx[0] != -1 and self.gen_token_idx[0] != -1:
            if i < min_word_tokens:
              logits[:, self.retrieval_token_idx] = filter_value
              logits[:, self.gen_token_idx] = filter_value
            else:
              if ret_scale_factor > 1:
                logits[:, self.retrieval_token_idx[0]] = logits[:, self.retrieval_token_idx[0]].abs() * ret_scale_factor
              if gen_scale_factor > 1:
                logits[:, self.gen_token_idx[0]] = logits[:, self.gen_token_idx[0]].abs() * gen_scale_factor
          if temperature == 0.0:
            if top_p != 1.0:
              raise ValueError('top_p cannot be set if temperature is 0 (greedy decoding).')
            next_token = torch.argmax(logits, keepdim=True, dim=-1)
          else:
            logits = logits / temperature
            if top_p < 1.0:
              assert top_p > 0, f'top_p should be above 0, got {top_p} instead.'
              sorted_logits, sorted_indices = torch.sort(logits, descending=True)
              cumulative_probs = torch.cumsum(torch.softmax(sorted_logits, dim=-1), dim=-1)
              remove = cumulative_probs > top_p
              remove[..., 1:] = remove[..., :-1].clone()
              remove[..., 0] = 0
              for j in range(sorted_indices.shape[0]):
                logits[j, sorted_indices[j, remove[j, :]]] = filter_value
            next_token = torch.multinomial(logits.exp(), 1)
        # Force generation of the remaining [IMG] tokens if [IMG0] is generated (batch 1 only, :518-520).
        if next_token.shape[0] == 1:
          if next_token.is_cuda:
            self._decode_host_waits += 1
          forced = next_token.item() == self.retrieval_token_idx[0]
        else:
          forced = False
        if forced:
          assert self.retrieval_token_idx == self.gen_token_idx, (self.retrieval_token_idx, self.gen_token_idx)
          next_token = torch.tensor(self.retrieval_token_idx)[None, :].long().to(dev)
        else:
          next_token = next_token.long().to(dev)
        out = next_token if out is None else torch.cat([out, next_token], dim=-1)
        next_embedding = self.input_embeddings(next_token)
        embeddings = torch.cat([embeddings, next_embedding.to(embeddings.dtype)], dim=1)
    return out, output_embeddings, output_logits

  def _size_kv_cache(self, embeddings: Tensor, max_len: int):
    # the cache lives in the handle: size it for the longest sequence this call can produce — every one of the max_len
    # steps may emit [IMG0] and so append all len(retrieval_token_idx) forced tokens (:518-520) — capped at the LM's
    # position table.  The handle is never rebuilt mid-sequence (_lm_forward_hidden_cached raises instead).
    grow = max(1, len(self.retrieval_token_idx))
    self._opt_native(embeddings.shape[0], min(embeddings.shape[1] + max_len * grow, self.opt_cfg.max_positions))

  def _generate_device(self, embeddings: Tensor, max_len: int, min_word_tokens: int, ret_scale_factor: float,
                       gen_scale_factor: float, filter_value: float, use_kv_cache: bool,
                       sample: Optional[Tuple[float, float, int]] = None):
    """generate() with the decision in libgill_amd: the greedy pick (gill_opt_next_token), or with sample = (temperature, top_p,
    seed) the seeded draw (gill_opt_sample_token; draw = the step, row0 = 0).  The picked ids go to a device token buffer, their
    embeddings to the next step's input; the post-rule logits go to pinned host memory by asynchronous copies, and the one
    synchronisation is at the end — except at top_p < 1, where the reference keeps them on the device (:471-472).  At batch 1
    the count of emitted ids (1, or the 8 forced [IMG] ids) is read back each step: the next forward's length depends on it."""
    with torch.no_grad():
      output_embeddings = []
      output_logits = []
      dev = embeddings.device
      vocab = self.opt_cfg.vocab_size
      B0, _, D = embeddings.shape
      grow = max(1, len(self.retrieval_token_idx)) if B0 == 1 else 1      # ids one step can emit (:518-520: batch 1 only)
      tokens = torch.empty((B0, max(1, max_len * grow)), device=dev, dtype=torch.int64)
      nxt = torch.empty((B0, grow, D), device=dev, dtype=torch.bfloat16)
      n_dev = torch.empty(1, device=dev, dtype=torch.int32)
      n_host = torch.empty(1, dtype=torch.int32, pin_memory=True)
      logits_to_host = sample is None or sample[1] == 1.0
      host_logits = torch.empty((max_len, B0, vocab), dtype=torch.float32, pin_memory=True) \
        if max_len > 0 and logits_to_host else None
      if sample is not None:
        sampler = N.gill_decode_sampler()
        # top_p above 1 filters nothing, as in the reference (:502 tests top_p < 1.0 only)
        sampler.temperature, sampler.top_p, sampler.seed, sampler.row0 = sample[0], min(sample[1], 1.0), sample[2], 0
      ev = torch.cuda.Event()
      col = 0
      hidden = None
      new_embeds = None
      if use_kv_cache:
        self._size_kv_cache(embeddings, max_len)
      for i in range(max_len):
        if use_kv_cache:
          past = 0 if hidden is None else hidden.shape[1]
          new_hidden = self._lm_forward_hidden_cached(embeddings if hidden is None else new_embeds, past)
          hidden = new_hidden if hidden is None else torch.cat([hidden, new_hidden], dim=1)
        else:
          hidden = self._lm_forward_hidden(embeddings)                         # :465
        for idx in self.args.text_emb_layers:
          output_embeddings.append(hidden.to(embeddings.dtype))                # :467-468
        B, T, _ = hidden.shape
        logits = torch.empty((B, vocab), device=dev, dtype=torch.float32)
        rule = self._decode_rule(i, min_word_tokens, ret_scale_factor, gen_scale_factor, filter_value)
        with torch.cuda.device(dev):
          if sample is None:
            N.check(N.lib().gill_opt_next_token(self._opt_handle, N.ptr(hidden), B, T, C.byref(rule), N.ptr(logits), N.ptr(tokens),
                                                tokens.shape[1], col, N.ptr(n_dev), N.ptr(nxt), N.current_stream()))
          else:
            sampler.draw = i
            N.check(N.lib().gill_opt_sample_token(self._opt_handle, N.ptr(hidden), B, T, C.byref(rule), C.byref(sampler),
                                                  N.ptr(logits), N.ptr(tokens), tokens.shape[1], col, N.ptr(n_dev), N.ptr(nxt),
                                                  N.current_stream()))
          if logits_to_host:
            host_logits[i].copy_(logits, non_blocking=True)                    # :471-472, the post-rule values (:476-489)
            output_logits.append(host_logits[i])
          else:
            output_logits.append(logits)
          if B == 1:
            n_host.copy_(n_dev, non_blocking=True)
            ev.record()
            ev.synchronize()
            self._decode_host_waits += 1
            n = int(n_host[0])
            if n < 0:
              raise AssertionError((self.retrieval_token_idx, self.gen_token_idx))   # :519
          else:
            n = 1
        col += n
        new_embeds = nxt[:, :n].to(embeddings.dtype)
        if not use_kv_cache:
          embeddings = torch.cat([embeddings, new_embeds], dim=1)
      if max_len > 0 and logits_to_host:
        torch.cuda.current_stream(dev).synchronize()                           # the pinned logits are complete
    out = tokens[:, :col].clone() if max_len > 0 else None
    return out, output_embeddings, output_logits

  def _ragged_decode_loop(self, h, B: int, st: Tensor, hid: Tensor, steps: Tensor, nxt: Tensor, logits: Tensor, tokens: Tensor, rule,
                          sampler, max_len: int, L: int, len0: int, len_floor: int = 0) -> None:
    """The ragged loop generate_batch and a dialogue session share: per iteration one decode step over all B rows (from the second
    iteration on) and one decision; the count of active rows of iteration i is read after iteration i + 1 has been enqueued.  hid (B, D):
    the hidden rows the first decision reads; len0: the host's bound on the deciding rows' lengths at the first decode step (it grows by one
    per iteration); len_floor: the bound of rows that take no decision (a session's idle rows: their lengths stand)."""
    dev = st.device
    lib = N.lib()
    count = torch.zeros(2, dtype=torch.int32, pin_memory=True)
    evs = [torch.cuda.Event(), torch.cuda.Event()]
    with torch.cuda.device(dev):
      for it in range(L):
        if it > 0:
          N.check(lib.gill_opt_decode_step(h, N.ptr(nxt), N.ptr(st), B, max(len0 + it, len_floor), N.ptr(steps[it - 1]), N.current_stream()))
          hid = steps[it - 1]
        N.check(lib.gill_opt_next_token_ragged(h, N.ptr(hid), B, C.byref(rule), max_len, C.byref(sampler) if sampler is not None else None,
                                               N.ptr(logits), N.ptr(st), N.ptr(tokens), tokens.shape[1], N.ptr(nxt), N.current_stream()))
        count[it & 1:(it & 1) + 1].copy_(st[6 * B:], non_blocking=True)
        evs[it & 1].record()
        if it > 0:                    # one iteration late: the device already has iteration `it` to run
          evs[(it - 1) & 1].synchronize()
          self._decode_host_waits += 1
          if int(count[(it - 1) & 1]) == 0:
            break

  def _branch_decode_loop(self, h, S: int, G: int, groups: Tensor, st: Tensor, hid: Tensor, steps: Tensor, nxt: Tensor, logits: Tensor,
                          tokens: Tensor, rule, sampler, max_len: int, L: int, len0: int) -> None:
    """_ragged_decode_loop over S branches of cached dialogues (DialogueSession.sample): the decode step is gill_opt_decode_step_branch (the
    branches' groups: groups = [gstart (G + 1) | gparent (G) | gplen (G)] int32 on the device), the decision gill_opt_next_token_branch; the
    same one-iteration-late read of the active count.  hid (S, D): every branch's copy of its dialogue's hidden_last."""
    dev = st.device
    lib = N.lib()
    count = torch.zeros(2, dtype=torch.int32, pin_memory=True)
    evs = [torch.cuda.Event(), torch.cuda.Event()]
    gstart, gparent, gplen = groups, groups[G + 1:], groups[2 * G + 1:]
    with torch.cuda.device(dev):
      for it in range(L):
        if it > 0:
          N.check(lib.gill_opt_decode_step_branch(h, N.ptr(nxt), N.ptr(st), gstart.data_ptr(), gparent.data_ptr(), gplen.data_ptr(), S, G,
                                                  len0 + it, N.ptr(steps[it - 1]), N.current_stream()))
          hid = steps[it - 1]
        N.check(lib.gill_opt_next_token_branch(h, N.ptr(hid), S, C.byref(rule), max_len, C.byref(sampler) if sampler is not None else None,
                                               N.ptr(logits), N.ptr(st), N.ptr(tokens), tokens.shape[1], N.ptr(nxt), N.current_stream()))
        count[it & 1:(it & 1) + 1].copy_(st[6 * S:], non_blocking=True)
        evs[it & 1].record()
        if it > 0:
          evs[(it - 1) & 1].synchronize()
          self._decode_host_waits += 1
          if int(count[(it - 1) & 1]) == 0:
            break

  def _ragged_results(self, B: int, st: Tensor, tokens: Tensor, steps: Tensor, L: int, n_ret: int):
    """The state a ragged loop left -> (n_tokens (B,), n_hidden (B,) on the host, hidden (B, L, D)); raises on the rows' error flags."""
    D = steps.shape[2]
    state = st.cpu()
    flags = state[5 * B:6 * B]
    if bool((flags & 1).any()):
      raise AssertionError((self.retrieval_token_idx, self.gen_token_idx))   # :519
    if bool((flags & 6).any()):
      raise N.GillNativeError(f'ragged decode: a row outgrew the cache or the token buffer (flags {flags.tolist()})')
    n_tokens = state[3 * B:4 * B].to(torch.int64)
    toks = tokens.cpu()
    n_hidden = torch.zeros(B, dtype=torch.int64)
    for b in range(B):
      nt = int(n_tokens[b])
      last = 1
      if n_ret > 1 and nt >= n_ret and int(toks[b, nt - n_ret]) == int(self.retrieval_token_idx[0]):
        last = n_ret            # the row's last decision opened an [IMG] block, which ends the row
      n_hidden[b] = max(nt - last, 0)
    hidden = steps.transpose(0, 1)[:, :L].contiguous() if L > 0 else steps.new_zeros((B, 0, D))
    return n_tokens, n_hidden, hidden

  def _lm_extend(self, cu_new: Tensor, lens_dev: Tensor, B: int, total_new: int, max_new: int, len_bound: int, hidden_last: Tensor,
                 ids: Optional[Tensor] = None, embeds: Optional[Tensor] = None, extra_rows: Optional[Tensor] = None,
                 hidden_all: Optional[Tensor] = None) -> None:
    """gill_opt_extend on the handle as it stands (never grown here: that would drop the cache): packed new tokens, ids (total_new) int64 or
    embeds (total_new, D) bf16, row cu_new[b] + i at position lens_dev[b] + i of sequence b; -> hidden_last (B, 1, D) fp32 in place, and
    hidden_all (total_new, D) fp32 when given."""
    cb, ct = self._opt_cap
    if self._opt_handle is None or B > cb or len_bound > ct:
      raise N.GillNativeError(f'KV cache of the OPT handle holds {ct} tokens x {cb} sequences; extend needs {len_bound} x {B}.')
    n_extra = 0 if extra_rows is None else int(extra_rows.shape[0])
    with torch.cuda.device(cu_new.device):
      N.check(N.lib().gill_opt_extend(self._opt_handle, N.ptr(ids), N.ptr(embeds), N.ptr(extra_rows) if n_extra else None, n_extra,
                                      N.ptr(cu_new), N.ptr(lens_dev), B, total_new, max_new, len_bound, N.ptr(hidden_last),
                                      N.ptr(hidden_all), N.current_stream()))

  def _lm_score_candidates(self, pack, extra_rows: Optional[Tensor] = None, token_rank: Optional[Tensor] = None,
                           hidden_all: Optional[Tensor] = None, flags: Optional[Tensor] = None) -> Tensor:
    """gill_opt_score_candidates on the handle as it stands (never grown here: that would drop the cache) for one dialogue.CandidatePack.
    -> one fp32 device tensor [token_logprob (total_new) | score_sum (C) | score_mean (C) | n_scored (C, int32 bits)]: the caller's single
    device-to-host copy.  Reads the cache, writes nothing of the handle's state: the cache epoch stands."""
    dev = self.logit_scale.device
    if self._opt_handle is None:
      raise N.GillNativeError('the OPT handle has no KV cache to score against: open a session and extend it first.')
    T, Cn = pack.total_new, pack.n_candidates
    i32 = torch.tensor(pack.cu + pack.parent + pack.plen, dtype=torch.int32).to(dev)
    i64 = torch.tensor(pack.ids + pack.targets, dtype=torch.int64).to(dev)
    out = torch.zeros(T + 3 * Cn, dtype=torch.float32, device=dev)
    n_extra = 0 if extra_rows is None else int(extra_rows.shape[0])
    with torch.cuda.device(dev):
      N.check(N.lib().gill_opt_score_candidates(self._opt_handle, i64.data_ptr(), None, N.ptr(extra_rows) if n_extra else None, n_extra,
                                                i32.data_ptr(), i32[Cn + 1:].data_ptr(), i32[2 * Cn + 1:].data_ptr(), i64[T:].data_ptr(), Cn, T,
                                                max(pack.max_new, 1), max(pack.len_bound, 1), out.data_ptr(), N.ptr(token_rank),
                                                out[T:].data_ptr(), out[T + 2 * Cn:].data_ptr(), out[T + Cn:].data_ptr(), N.ptr(hidden_all),
                                                N.ptr(flags), N.current_stream()))
    return out

  def open_session(self, B: int, capacity: int):
    """A dialogue session over the handle's KV cache: B rows of up to `capacity` tokens whose caches are kept across turns
    (dialogue.DialogueSession).  Any other entry that writes or rebuilds the cache makes the session stale."""
    from .dialogue import DialogueSession
    return DialogueSession(self, B, capacity)

  def generate_batch(self, embeddings: Optional[Tensor] = None, lengths=None, ids: Optional[Tensor] = None,
                     extra_rows: Optional[Tensor] = None, max_len: int = 32, temperature: float = 0.0, top_p: float = 1.0,
                     min_word_tokens: int = 0, ret_scale_factor: float = 1.0, gen_scale_factor: float = 1.0,
                     filter_value: float = -float('Inf'), seed: Optional[int] = None, row_ids=None):
    """Ragged batched decoding: one dialogue per row, every row at its own length, with the tokens the one-sequence generate()
    emits for that row alone.  The prompts are right-padded: embeddings (B, Tmax, D), or ids (B, Tmax) int64 (an id < 0 selects
    row -(id + 1) of extra_rows (n, D) bf16, the visual embeddings of image prompts), with lengths (B,) the real lengths.
    One prefill, then per iteration one decode step over all rows (gill_opt_decode_step: every row against its own cache length)
    and one decision (gill_opt_next_token_ragged: every row its own step count and [IMG] forcing state, so an [IMG] block takes
    len(retrieval_token_idx) iterations of its row while the other rows go on deciding).  max_len counts decisions per row, as in
    generate().  temperature > 0 needs seed: the draw is the seeded one of generate(seed=), keyed (seed, row_ids[b], the row's
    decision count), so a row draws the same tokens alone (row_ids=[its id]) as inside any batch; row_ids defaults to 0 .. B - 1.
    The loop never makes the device wait: it reads the count of active rows of iteration i after it has enqueued iteration i + 1
    (at most one surplus iteration); _decode_host_waits counts those reads.
    Returns tokens (B, L) int64 padded with -1, n_tokens (B,), hidden (B, L, D) fp32 and n_hidden (B,): hidden[b, j] is
    hidden_states[-1] at generated token j's position for j < n_hidden[b] = n_tokens[b] minus what the row's last decision emitted
    — the rows generated_embeddings[-1][:, T0:] holds in the one-sequence call."""
    self._decode_host_waits = 0
    self._cache_epoch += 1
    if (embeddings is None) == (ids is None):
      raise ValueError('generate_batch takes embeddings (B, Tmax, D) or ids (B, Tmax), one of the two.')
    src = embeddings if embeddings is not None else ids
    B, Tmax = int(src.shape[0]), int(src.shape[1])
    if lengths is None:
      raise ValueError('generate_batch needs lengths (B,): the real length of every right-padded row.')
    lens = [int(v) for v in torch.as_tensor(lengths).reshape(-1).tolist()]
    if len(lens) != B:
      raise ValueError(f'lengths has {len(lens)} entries for a batch of {B}.')
    if min(lens) < 1 or max(lens) > Tmax:
      raise ValueError(f'lengths should be in [1, {Tmax}], got {lens}.')
    if temperature == 0.0 and top_p != 1.0:
      raise ValueError('top_p cannot be set if temperature is 0 (greedy decoding).')
    if temperature != 0.0:
      if seed is None:
        raise ValueError('generate_batch draws on the device only: temperature > 0 needs seed.')
      seed = int(seed)
      if not 0 <= seed < 2 ** 64:
        raise ValueError(f'seed should be in [0, 2**64), got {seed} instead.')
      assert top_p > 0, f'top_p should be above 0, got {top_p} instead.'
    max_len = int(max_len)
    n_ret = max(1, len(self.retrieval_token_idx))
    L = max_len * n_ret
    if max(lens) + L > self.opt_cfg.max_positions:
      raise ValueError(f'max(lengths) + max_len * {n_ret} = {max(lens) + L} exceeds the position table ({self.opt_cfg.max_positions}).')
    rows = list(range(B)) if row_ids is None else [int(v) for v in torch.as_tensor(row_ids).reshape(-1).tolist()]
    if len(rows) != B or min(rows) < 0:
      raise ValueError(f'row_ids should be {B} integers >= 0.')
    dev = self.logit_scale.device
    D, vocab = self.opt_cfg.hidden_size, self.opt_cfg.vocab_size
    with torch.no_grad():
      h = self._opt_native(B, max(Tmax, max(lens) + L))       # sized once: the handle is not rebuilt inside the loop
      lib = N.lib()
      st = torch.zeros(6 * B + 1, dtype=torch.int32)
      st[0:B] = torch.tensor(lens, dtype=torch.int32) - 1
      st[4 * B:5 * B] = torch.tensor(rows, dtype=torch.int32)
      st[6 * B] = B if max_len > 0 else 0
      st = st.to(dev)
      tokens = torch.full((B, max(L, 1)), -1, device=dev, dtype=torch.int64)
      kv8 = self.kv_cache != 'bf16'
      full = None if kv8 else torch.empty((B, Tmax, D), device=dev, dtype=torch.float32)
      # an e4m3 cache: the prompts packed, without their pad positions, through the extend pass at lengths 0 (a session's first turn)
      keep = (torch.arange(Tmax)[None, :] < torch.tensor(lens)[:, None]).reshape(-1).to(dev) if kv8 else None
      last = torch.zeros((B, 1, D), device=dev, dtype=torch.float32) if kv8 else None
      cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device=dev) if kv8 else None
      zero_lens = torch.zeros(B, dtype=torch.int32, device=dev) if kv8 else None
      with torch.cuda.device(dev):
        if ids is not None:
          idt = ids.to(dev, torch.int64).contiguous()
          n_extra = 0
          if extra_rows is not None:
            if extra_rows.dim() != 2 or extra_rows.shape[1] != D or extra_rows.dtype != torch.bfloat16:
              raise ValueError(f'extra_rows must be (n, {D}) bfloat16, got {tuple(extra_rows.shape)} {extra_rows.dtype}')
            extra_rows = extra_rows.to(dev).contiguous()
            n_extra = extra_rows.shape[0]
          lowest = int(idt.min())
          if lowest < -n_extra:
            raise ValueError(f'id {lowest} selects extra row {-(lowest + 1)} of {n_extra}')
          if kv8:
            self._lm_extend(cu, zero_lens, B, sum(lens), max(lens), max(lens), last, ids=idt.reshape(-1)[keep].contiguous(),
                            extra_rows=extra_rows if n_extra else None)
          else:
            N.check(lib.gill_opt_prefill_ids(h, N.ptr(idt), B, Tmax, N.ptr(extra_rows) if n_extra else None, n_extra, N.ptr(full),
                                             N.current_stream()))
        else:
          x = embeddings.to(dev, torch.bfloat16).contiguous()
          if kv8:
            self._lm_extend(cu, zero_lens, B, sum(lens), max(lens), max(lens), last, embeds=x.reshape(B * Tmax, D)[keep].contiguous())
          else:
            N.check(lib.gill_opt_forward_cached(h, N.ptr(x), B, Tmax, 0, N.ptr(full), N.current_stream()))
      if kv8:
        hid = last[:, 0].contiguous()
      else:
        lens_dev = torch.tensor(lens, device=dev, dtype=torch.int64)
        hid = full[torch.arange(B, device=dev), lens_dev - 1].contiguous()       # the rows len[b] - 1
      steps = torch.zeros((max(L, 1), B, D), device=dev, dtype=torch.float32)
      nxt = torch.zeros((B, D), device=dev, dtype=torch.bfloat16)
      logits = torch.empty((B, vocab), device=dev, dtype=torch.float32)
      rule = self._decode_rule(0, min_word_tokens, ret_scale_factor, gen_scale_factor, filter_value)
      sampler = None
      if temperature != 0.0:
        sampler = N.gill_decode_sampler()
        sampler.temperature, sampler.top_p, sampler.seed = float(temperature), min(float(top_p), 1.0), seed
      self._ragged_decode_loop(h, B, st, hid, steps, nxt, logits, tokens, rule, sampler, max_len, L, max(lens))
      n_tokens, n_hidden, hidden = self._ragged_results(B, st, tokens, steps, L, n_ret)
    return tokens[:, :L], n_tokens.to(dev), hidden, n_hidden.to(dev)

class _TopScores:
  """The scores of the rows a fused search returned, indexed by row like the reference's full score vector (scores[img_idx].item())."""

  def __init__(self, idx: Tensor, scores: Tensor):
    self._by_row = {int(i): s for i, s in zip(idx.tolist(), scores)}

  def __getitem__(self, row) -> Tensor:
    return self._by_row[int(row)]


class GILL(nn.Module):
  def __init__(self, tokenizer, model_args: Optional[GILLArgs] = None, path_array: Optional[List[str]] = None,
               emb_matrix: Optional[torch.tensor] = None, load_sd: bool = False, num_gen_images: int = 1,
               decision_model_path: Optional[str] = None, sd_pipe=None):
    super().__init__()
    self.model = GILLModel(tokenizer, model_args)
    self.path_array = path_array
    self.emb_matrix = emb_matrix
    self.ret_index = None            # device-resident retrieval index (build_retrieval_index); opt-in, not a reference attribute
    self.load_sd = load_sd
    self.num_gen_images = num_gen_images
    self.idx2dec = {0: 'gen', 1: 'ret', 2: 'same'}
    self.decision_model = None
    if load_sd:
      if sd_pipe is not None:          # synthetic / pre-built pipeline (tests, benchmarks)
        self.sd_pipe = sd_pipe
      else:                            # models.py:550-551
        from .sd import GillSDPipeline
        model_id = os.environ.get("GILL_SD_DIR", "runwayml/stable-diffusion-v1-5")
        self.sd_pipe = GillSDPipeline.from_pretrained(model_id).to("cuda")
    if decision_model_path is not None:
      # decision MLP of the gen-vs-ret choice (models.py:553-561); applied in generate_for_images_and_texts (:671-682)
      print('Loading decision model...')
      self.decision_model = nn.Sequential(*[nn.Dropout(0.5), nn.Linear(4096, 2)])
      mlp_checkpoint = torch.load(decision_model_path, map_location='cpu')
      self.decision_model.load_state_dict(mlp_checkpoint['state_dict'], strict=True)
      self.decision_model.eval()

  def __call__(self, images: Tensor, tgt_tokens: Optional[Tensor] = None, caption_len: Optional[Tensor] = None,
               generate: bool = False, num_words: int = 32, temperature: float = 1.0, top_p: float = 1.0,
               ret_scale_factor: float = 1.0, gen_scale_factor: float = 1.0, min_word_tokens: int = 0,
               mode: str = 'captioning', concat_captions: bool = False, input_prefix: Optional[str] = None) -> Tensor:
    if generate:
      return self.model.generate(images, num_words, temperature=temperature, top_p=top_p, min_word_tokens=min_word_tokens,
                                 ret_scale_factor=ret_scale_factor, gen_scale_factor=gen_scale_factor)
    return self.model(pixel_values=images, labels=tgt_tokens, caption_len=caption_len, mode=mode,
                      concat_captions=concat_captions, input_prefix=input_prefix)

  def generate_for_images_and_texts(self, prompts: List, num_words: int = 0, min_word_tokens: int = 0,
                                    ret_scale_factor: float = 1.0, gen_scale_factor: float = 1.0, top_p: float = 1.0,
                                    temperature: float = 0.0, max_num_rets: int = 1, generator=None,
                                    always_add_bos: bool = False, guidance_scale: float = 7.5, num_inference_steps: int = 50,
                                    seed: Optional[int] = None):
    """Encode prompts into embeddings, and generates text and image outputs accordingly (models.py:582-762).  seed: the seeded
    on-device draw of GILLModel.generate for the text (temperature > 0); None draws as the reference does."""
    input_embs = []
    input_ids = []
    add_bos = True
    dev = self.model.logit_scale.device
    # argument errors of the reference (models.py:624, :629) are raised before any device work
    for p in prompts:
      if type(p) != str and not type(p).__module__.startswith('PIL'):
        raise ValueError(f'Input prompts should be either PIL.Image.Image or str types, got {type(p)} instead.')
    if num_words == 0:
      raise NotImplementedError('Generation not implemented for num_words=0.')
    self.model._require_bf16_kv('generate_for_images_and_texts')
    with torch.no_grad():
      for p in prompts:
        if type(p) == str:
          text_ids = self.model.tokenizer(p, add_special_tokens=add_bos, return_tensors="pt").input_ids.to(dev)
          if not always_add_bos:
            add_bos = False
          input_embs.append(self.model.input_embeddings(text_ids))
          input_ids.append(text_ids)
        elif type(p).__module__.startswith('PIL'):
          # Encode as image (models.py:606-613)
          pixel_values = utils.get_pixel_values_for_model(self.model.feature_extractor, p)
          pixel_values = pixel_values.to(device=dev, dtype=self.model.logit_scale.dtype)[None, ...]
          visual_embs = self.model.get_visual_embs(pixel_values, mode='captioning')   # (1, n_visual_tokens, D)
          input_embs.append(visual_embs.to(input_embs[0].dtype) if input_embs else visual_embs)
        else:
          raise ValueError(f'Input prompts should be either PIL.Image.Image or str types, got {type(p)} instead.')
      input_embs = torch.cat(input_embs, dim=1)
      input_ids = torch.cat(input_ids, dim=1)

      if num_words == 0:
        raise NotImplementedError('Generation not implemented for num_words=0.')
      elif num_words > 0:
        generated_ids, generated_embeddings, _ = self.model.generate(
          input_embs, num_words, min_word_tokens=min_word_tokens, temperature=temperature, top_p=top_p,
          ret_scale_factor=ret_scale_factor, gen_scale_factor=gen_scale_factor, seed=seed)
        embeddings = generated_embeddings[-1][:, input_embs.shape[1]:]
        newline_token_id = self.model.tokenizer('\n', add_special_tokens=False).input_ids[0]
        trunc_idx = 0
        for j in range(generated_ids.shape[1]):
          if generated_ids[0, j] == newline_token_id:
            trunc_idx = j
            break
        if trunc_idx > 0:
          generated_ids = generated_ids[:, :trunc_idx]
          embeddings = embeddings[:, :trunc_idx]
      else:
        raise ValueError

      return_outputs = []
      all_ret_idx = [i for i, x in enumerate(generated_ids[0, :] == self.model.retrieval_token_idx[0]) if x][:max_num_rets]
      seen_image_idx = []  # Avoid showing the same image multiple times.
      last_ret_idx = 0
      if len(all_ret_idx) == 0:
        caption = self.model.tokenizer.batch_decode(generated_ids, skip_special_tokens=True)[0]
        return_outputs.append(utils.truncate_caption(caption))
      else:
        for ret_idx in all_ret_idx:
          assert generated_ids[0, ret_idx:ret_idx + self.model.num_tokens].cpu().detach().numpy().tolist() == self.model.retrieval_token_idx, (generated_ids[0, ret_idx:ret_idx + self.model.num_tokens], self.model.retrieval_token_idx)
          raw_emb = embeddings[:, ret_idx:ret_idx + self.model.num_tokens, :]  # (1, 8, 4096)
          assert len(self.model.args.text_emb_layers) == 1
          image_outputs = {'gen': [], 'ret': [], 'decision': None}
          if self.emb_matrix is not None:
            # Produce retrieval embedding (models.py:671-676); the Linear and the score GEMV run in libgill_amd
            from . import ops
            from PIL import UnidentifiedImageError
            ret_emb = self.model.ret_text_hidden_fcs[0](raw_emb, None)[:, 0, :]  # (1, 256)
            ret_emb = ret_emb / ret_emb.norm(dim=-1, keepdim=True)
            ret_emb = ret_emb.type(self.emb_matrix.dtype)  # (1, 256)
            if self.ret_index is not None:
              # the same three steps as one fused pass over the resident index: a seen image competes, and is reported, with its -1000
              top_scores, top_idx = self.ret_index.search(ret_emb.float(), 3, normalize=False, penalty=1000.0,
                                                          exclude=[[int(i) for i in seen_image_idx]] if seen_image_idx else None)
              top_image_idx = top_idx[0][top_idx[0] >= 0]
              scores = _TopScores(top_image_idx, top_scores[0])
            else:
              scores = self._scores(self.emb_matrix, ret_emb)                         # emb_matrix @ ret_emb.T, (N, 1)
              for seen_idx in seen_image_idx:   # Downweight seen images.
                scores[seen_idx, :] -= 1000
              _, top_image_idx = scores.squeeze().topk(3)
            for img_idx in top_image_idx:     # Find the first image that does not error out.
              try:
                seen_image_idx.append(img_idx)
                img = utils.get_image_from_url(self.path_array[img_idx])
                image_outputs['ret'].append((img, 'ret', scores[img_idx].item()))
                if len(image_outputs) == max_num_rets:
                  break
              except (UnidentifiedImageError, ConnectionError, OSError):
                pass
            if self.decision_model is not None:   # Make decision with MLP (models.py:698-704)
              decision_emb = raw_emb[:, 0, :]  # (1, 4096)
              lin = self.decision_model[1]
              assert decision_emb.shape[1] == lin.in_features, decision_emb.shape
              w4 = torch.zeros((4, lin.in_features), device=decision_emb.device, dtype=torch.bfloat16)
              w4[:lin.out_features] = lin.weight.to(decision_emb.device, torch.bfloat16)
              b4 = torch.zeros((4,), device=decision_emb.device)
              b4[:lin.out_features] = lin.bias.to(decision_emb.device).float()
              decision_logits = ops.gemm(decision_emb, w4, bias=b4, out_f32=True)[:, :lin.out_features]
              probs = decision_logits.softmax(dim=-1).cpu().float().numpy().tolist()
              image_outputs['decision'] = [self.idx2dec[decision_logits.argmax().item()]] + probs
          else:
            # If no embedding matrix is provided, generate instead.
            image_outputs['decision'] = ['gen', [0, 1]]

          gen_prefix = ''.join([f'[IMG{i}]' for i in range(self.model.args.num_tokens)])
          gen_prefx_ids = self.model.tokenizer(gen_prefix, add_special_tokens=False, return_tensors="pt").input_ids.to(dev)
          gen_prefix_embs = self.model.input_embeddings(gen_prefx_ids)  # (1, T, D)
          gen_emb = self.model.gen_text_hidden_fcs[0](raw_emb, gen_prefix_embs)  # (1, 77, 768)
          if gen_emb.shape[1] != 77:
            print(f"Padding {gen_emb.shape} with zeros")
            bs = gen_emb.shape[0]
            clip_emb = 768
            gen_emb = gen_emb.reshape(bs, -1, clip_emb)
            seq_len = gen_emb.shape[1]
            gen_emb = torch.cat([gen_emb, torch.zeros((bs, 77 - seq_len, clip_emb), device=gen_emb.device, dtype=gen_emb.dtype)], dim=1)
            print('Padded to', gen_emb.shape)
          gen_emb = gen_emb.repeat(self.num_gen_images, 1, 1)  # (self.num_gen_images, 77, 768)

          if self.load_sd:
            gen_max_bs = 8
            gen_images = []
            for i in range(0, self.num_gen_images, gen_max_bs):
              gen_images.extend(
                self.sd_pipe(prompt_embeds=gen_emb[i:i + gen_max_bs], generator=generator, guidance_scale=guidance_scale,
                             num_inference_steps=num_inference_steps,
                             output_type="pil" if getattr(self.sd_pipe, "_vae", None) else "latent").images)
            # PIL images when the pipeline holds VAE weights (reference behaviour), else the final latents (4,64,64)
            if self.emb_matrix is not None and getattr(self.sd_pipe, "_vae", None):
              # CLIP rerank of the generated images against the retrieval embedding (models.py:733-751)
              all_gen_pixels = []
              for img in gen_images:
                pixel_values = utils.get_pixel_values_for_model(self.model.feature_extractor, img.resize((224, 224)).convert('RGB'))
                all_gen_pixels.append(pixel_values.to(device=dev, dtype=self.model.logit_scale.dtype))
              all_gen_pixels = torch.stack(all_gen_pixels, dim=0)
              gen_visual_embs = self.model.get_visual_embs(all_gen_pixels, mode='retrieval')  # (n, 1, D)
              gen_visual_embs = gen_visual_embs / gen_visual_embs.norm(dim=-1, keepdim=True)
              gen_visual_embs = gen_visual_embs.type(self.emb_matrix.dtype)
              gen_rank_scores = self._scores(gen_visual_embs.reshape(len(gen_images), -1), ret_emb).squeeze()
              sorted_score_idx = torch.argsort(-gen_rank_scores)
              if self.num_gen_images > 1:   # Rank images by retrieval score.
                image_outputs['gen'] = [(gen_images[idx], gen_rank_scores[idx].item()) for idx in sorted_score_idx]
              else:
                image_outputs['gen'] = [(gen_images[0], gen_rank_scores.item())]
            else:
              image_outputs['gen'] = [(gen_images[0], 0)]
          else:
            image_outputs['gen'] = [gen_emb]

          caption = self.model.tokenizer.batch_decode(generated_ids[:, last_ret_idx:ret_idx], skip_special_tokens=True)[0]
          last_ret_idx = ret_idx + 1
          return_outputs.append(utils.truncate_caption(caption) + f' {gen_prefix}')
          return_outputs.append(image_outputs)
    return return_outputs

  @torch.no_grad()
  def generate_for_images_and_texts_batch(self, prompt_lists: List, num_words: int = 32, min_word_tokens: int = 0,
                                          ret_scale_factor: float = 1.0, gen_scale_factor: float = 1.0, top_p: float = 1.0,
                                          temperature: float = 0.0, max_num_rets: int = 1, generator=None,
                                          always_add_bos: bool = False, guidance_scale: float = 7.5, num_inference_steps: int = 50,
                                          seed: Optional[int] = None, all_branches: bool = False, skip_gen_on_ret: bool = False):
    """generate_for_images_and_texts for several dialogues at once: prompt_lists[b] is one prompt list (PIL images and strings); returns,
    per prompt list, the list the one-sequence method returns for it.  The prompts are segmented as the batched entries segment them
    (_interleaved_ids, _visual_rows), decoded as ONE ragged batch (GILLModel.generate_batch: every row at its own length, an [IMG]
    block forced per row), then per row the reference's newline truncation, the [IMG] blocks up to max_num_rets and the captions; the
    raw_emb blocks of ALL rows go through gen_text_hidden_fcs[0] in one call and, with load_sd, through the SD pipeline in chunks of 8.
    Scope by default (all_branches=False): the 'gen' branch only.  With a retrieval embedding matrix or a decision model attached this
    raises NotImplementedError: retrieval, the decision MLP and the CLIP rerank then stay with generate_for_images_and_texts, one
    sequence at a time.  all_branches=True runs every branch of that method for the batch (_batch_branches): one img_block_heads launch
    turns the first [IMG] hidden row of every block of every row into retrieval embeddings and decisions, retrieval runs in rounds
    (round j: the j-th block of every row, one search per round), and with a VAE and a retrieval matrix the generated images of all
    blocks are reranked together on the device.  skip_gen_on_ret=True (a stated divergence: the reference always computes both lists;
    ignored without a decision model) leaves blocks decided 'ret' out of the mapper, SD and rerank calls: their 'gen' is [].
    all_branches=True needs ret_text_fc_mode 'linear' (the mode of every shipped checkpoint; the heads kernel is that Linear): any other
    mode raises NotImplementedError, where the one-sequence method takes any mode.
    Nothing is sharded over ranks.  temperature > 0 needs seed (row b draws with row id b)."""
    if not all_branches and (self.emb_matrix is not None or self.decision_model is not None):
      raise NotImplementedError('generate_for_images_and_texts_batch covers the generation branch only by default: with retrieval '
                                'embeddings or a decision model attached, pass all_branches=True or call generate_for_images_and_texts '
                                'per prompt list.')
    prompts = [[p] if isinstance(p, str) else list(p) for p in prompt_lists]
    for pl in prompts:
      for p in pl:
        if type(p) != str and not self._is_image(p):
          raise ValueError(f'Input prompts should be either PIL.Image.Image or str types, got {type(p)} instead.')
    if num_words == 0:
      raise NotImplementedError('Generation not implemented for num_words=0.')
    if num_words < 0:
      raise ValueError
    m = self.model
    dev = m.logit_scale.device
    ids, lens, images = self._interleaved_ids(prompts, always_add_bos)
    flat = [im for row in images for im in row]
    extra = self._visual_rows(flat) if flat else None
    tokens, n_tok, hidden, n_hid = m.generate_batch(ids=ids, lengths=lens, extra_rows=extra, max_len=num_words, temperature=temperature,
                                                    top_p=top_p, min_word_tokens=min_word_tokens, ret_scale_factor=ret_scale_factor,
                                                    gen_scale_factor=gen_scale_factor, seed=seed)
    return self._batch_outputs(list(range(len(prompts))), tokens, n_tok, hidden, n_hid, max_num_rets, generator, guidance_scale,
                               num_inference_steps, all_branches, skip_gen_on_ret)[0]

  def open_dialogues(self, n: int, capacity: Optional[int] = None):
    """n multi-turn dialogues whose KV caches are kept across turns (dialogue.GillDialogues): .say(turns, ...) sends each dialogue's new
    turn only and returns what generate_for_images_and_texts_batch returns per prompt list.  capacity: tokens per dialogue (default: the LM's
    position table)."""
    from .dialogue import GillDialogues
    return GillDialogues(self, n, capacity)

  def rank_candidates(self, prompts: List, candidates: List[str], reduce: str = 'mean'):
    """Ranks candidate reply strings as continuations of one interleaved image / text prompt list (NEW, not a reference function).  The
    one-shot form of GillDialogues.rank: opens a one-row session sized for the context, runs the prompt through it once (images through
    _visual_rows, segmented as generate_for_images_and_texts segments a prompt) and scores every candidate against that cached context
    (gill_opt_score_candidates); the context is not re-run per candidate.  Returns dict(scores, order, best) as GillDialogues.rank.
    Stated divergence from get_log_likelihood_scores: that method averages over every text position of the whole prompt, history included;
    this one scores the candidate's own tokens only (reduce='sum' ranks equal-length candidates as the old method does; otherwise the
    normalisation differs).  Like any session opening it takes over the handle's KV cache: an open session goes stale."""
    from .dialogue import rank_order, segment_turn
    m = self.model
    if any(type(c) != str for c in candidates):
      raise NotImplementedError('rank_candidates takes candidate strings: images inside a candidate are not scored')
    nv = m.args.n_visual_tokens
    ids, images, done = segment_turn(m.tokenizer, [prompts] if isinstance(prompts, str) else list(prompts), nv, False, False, self._is_image)
    extra = None
    if images:
      m._require_vision()
      extra = self._visual_rows(images)
    cand_ids = [[int(v) for v in m.tokenizer(c, add_special_tokens=not done, return_tensors="pt").input_ids[0].tolist()] for c in candidates]
    s = m.open_session(1, len(ids) + 1)
    s.extend([0], ids=[ids], extra_rows=[extra])
    return rank_order(s.score([0], [cand_ids], reduce=reduce)[0])

  def _batch_outputs(self, rows, tokens: Tensor, n_tok: Tensor, hidden: Tensor, n_hid: Tensor, max_num_rets: int, generator,
                     guidance_scale: float, num_inference_steps: int, all_branches: bool, skip_gen_on_ret: bool):
    """What generate_for_images_and_texts_batch and GillDialogues.say do with a ragged decode's results (tokens (B, L), n_tokens, hidden
    (B, L, D), n_hidden as generate_batch returns them) for the rows `rows` of the batch: per row the reference's newline truncation, the
    [IMG] blocks up to max_num_rets and the captions; the raw_emb blocks of all rows through gen_text_hidden_fcs[0] in one call and, with
    load_sd, through the SD pipeline in chunks of 8; with all_branches the retrieval, decision and rerank branches (_batch_branches).
    -> (per row of `rows` the list the one-sequence method returns, per row the index its ids were truncated at, 0: not truncated)."""
    m = self.model
    dev = m.logit_scale.device
    n_tok, n_hid = n_tok.tolist(), n_hid.tolist()
    newline_token_id = m.tokenizer('\n', add_special_tokens=False).input_ids[0]
    gen_prefix = ''.join([f'[IMG{i}]' for i in range(m.args.num_tokens)])
    outputs, blocks, truncs = [], [], []          # blocks: (the image_outputs dict to fill, raw_emb (1, 8, D))
    where = []                        # per block: (prompt list b, the flat row of its first [IMG] hidden state in `hidden`)
    for b in rows:
      generated_ids = tokens[b:b + 1, :n_tok[b]]
      embeddings = hidden[b:b + 1, :n_hid[b]].to(m.logit_scale.dtype)
      trunc_idx = 0
      for j, t in enumerate(generated_ids[0].tolist()):
        if t == newline_token_id:
          trunc_idx = j
          break
      truncs.append(trunc_idx)
      if trunc_idx > 0:
        generated_ids = generated_ids[:, :trunc_idx]
        embeddings = embeddings[:, :trunc_idx]
      row_out = []
      all_ret_idx = [i for i, x in enumerate(generated_ids[0, :] == m.retrieval_token_idx[0]) if x][:max_num_rets]
      last_ret_idx = 0
      if len(all_ret_idx) == 0:
        row_out.append(utils.truncate_caption(m.tokenizer.batch_decode(generated_ids, skip_special_tokens=True)[0]))
      for ret_idx in all_ret_idx:
        assert generated_ids[0, ret_idx:ret_idx + m.num_tokens].tolist() == m.retrieval_token_idx, \
          (generated_ids[0, ret_idx:ret_idx + m.num_tokens], m.retrieval_token_idx)
        assert len(m.args.text_emb_layers) == 1
        image_outputs = {'gen': [], 'ret': [], 'decision': ['gen', [0, 1]]}
        blocks.append((image_outputs, embeddings[:, ret_idx:ret_idx + m.num_tokens, :]))
        where.append((b, b * hidden.shape[1] + ret_idx))
        caption = m.tokenizer.batch_decode(generated_ids[:, last_ret_idx:ret_idx], skip_special_tokens=True)[0]
        last_ret_idx = ret_idx + 1
        row_out.append(utils.truncate_caption(caption) + f' {gen_prefix}')
        row_out.append(image_outputs)
      outputs.append(row_out)
    ret_emb = None
    if all_branches and blocks:
      ret_emb = self._batch_branches(blocks, where, hidden, max_num_rets)
      if skip_gen_on_ret and self.emb_matrix is not None and self.decision_model is not None:
        keep = [k for k, (image_outputs, _) in enumerate(blocks) if image_outputs['decision'][0] != 'ret']
        blocks = [blocks[k] for k in keep]
        ret_emb = ret_emb[torch.tensor(keep, dtype=torch.int64, device=dev)] if keep else None
    if blocks:
      gen_prefx_ids = m.tokenizer(gen_prefix, add_special_tokens=False, return_tensors="pt").input_ids.to(dev)
      gen_prefix_embs = m.input_embeddings(gen_prefx_ids)                                  # (1, T, D)
      raw = torch.cat([r for _, r in blocks], dim=0)                                       # (n, 8, D): every row's blocks at once
      gen_emb = m.gen_text_hidden_fcs[0](raw, gen_prefix_embs)                             # (n, 77, 768)
      if gen_emb.shape[1] != 77:
        gen_emb = gen_emb.reshape(gen_emb.shape[0], -1, 768)
        gen_emb = torch.cat([gen_emb, torch.zeros((gen_emb.shape[0], 77 - gen_emb.shape[1], 768), device=dev, dtype=gen_emb.dtype)], dim=1)
      gen_emb = gen_emb.repeat_interleave(self.num_gen_images, dim=0)                      # block k: rows k * num_gen_images ..
      if self.load_sd:
        gen_images, gen_u8 = [], []
        for i in range(0, gen_emb.shape[0], 8):
          res = self.sd_pipe(prompt_embeds=gen_emb[i:i + 8], generator=generator, guidance_scale=guidance_scale,
                             num_inference_steps=num_inference_steps,
                             output_type="pil" if getattr(self.sd_pipe, "_vae", None) else "latent")
          gen_images.extend(res.images)
          gen_u8.append(getattr(res, 'images_u8', None))
        if ret_emb is not None and getattr(self.sd_pipe, "_vae", None):
          self._batch_rerank(blocks, gen_images, gen_u8, ret_emb)
        else:
          for k, (image_outputs, _) in enumerate(blocks):
            image_outputs['gen'] = [(gen_images[k * self.num_gen_images], 0)]
      else:
        for k, (image_outputs, _) in enumerate(blocks):
          image_outputs['gen'] = [gen_emb[k * self.num_gen_images:(k + 1) * self.num_gen_images]]
    return outputs, truncs

  def _batch_branches(self, blocks, where, hidden: Tensor, max_num_rets: int) -> Optional[Tensor]:
    """The retrieval and decision branches of generate_for_images_and_texts (models.py:671-704) for every [IMG] block of a batch.
    blocks: (image_outputs, raw_emb) per block, filled in place; where: (prompt list, flat row of `hidden`) per block; hidden: what
    generate_batch returned.  One ops.img_block_heads launch for all blocks, one search (or one _scores GEMM + topk) and one copy to
    the host per round of retrieval, one copy for all decisions.  Returns ret_emb (n, E) fp32 in block order, None without emb_matrix."""
    if self.emb_matrix is None:       # no embedding matrix: generate instead; every block keeps ['gen', [0, 1]] (models.py:706)
      return None
    from . import ops
    from PIL import UnidentifiedImageError
    m = self.model
    dev = m.logit_scale.device
    fc = m.ret_text_hidden_fcs[0]
    if getattr(fc, 'mode', None) != 'linear':
      raise NotImplementedError(f'generate_for_images_and_texts_batch(all_branches=True) needs ret_text_fc_mode "linear", got {fc.mode!r}')
    decision = None
    if self.decision_model is not None:
      lin = self.decision_model[1]
      assert hidden.shape[-1] == lin.in_features, hidden.shape
      decision = (lin.weight.to(dev, torch.bfloat16), lin.bias.to(dev).float())
    row_idx = torch.tensor([r for _, r in where], dtype=torch.int32).to(dev)          # the one upload of the block rows
    ret_emb, probs, choice = ops.img_block_heads(hidden, row_idx, ret=(fc.model.weight.to(torch.bfloat16), fc.model.bias.float()),
                                                 decision=decision)
    # retrieval in rounds: round j holds the j-th block of every prompt list, in block order
    rounds, nth = [], {}
    for k, (b, _) in enumerate(where):
      j = nth.get(b, 0)
      nth[b] = j + 1
      if j == len(rounds):
        rounds.append([])
      rounds[j].append(k)
    seen = {b: [] for b, _ in where}      # per prompt list: avoid showing the same image multiple times
    for ks in rounds:
      q = ret_emb if len(ks) == len(blocks) else ret_emb[torch.tensor(ks, dtype=torch.int64).to(dev)]
      q = q.type(self.emb_matrix.dtype)
      seen_lists = [[int(i) for i in seen[where[k][0]]] for k in ks]
      if self.ret_index is not None:
        top_scores, top_idx = self.ret_index.search(q.float(), 3, normalize=False, penalty=1000.0,
                                                    exclude=seen_lists if any(seen_lists) else None)
      else:
        scores = self._scores(self.emb_matrix, q)                                       # emb_matrix @ q.T, (N, Q)
        for c, lst in enumerate(seen_lists):
          for seen_idx in lst:      # Downweight seen images.
            scores[seen_idx, c] -= 1000
        top_scores, top_idx = scores.t().float().topk(3, dim=1)
      top_scores, top_idx = top_scores.cpu(), top_idx.cpu()                             # the round's one wait for the device
      for c, k in enumerate(ks):
        image_outputs, seen_image_idx = blocks[k][0], seen[where[k][0]]
        for img_idx, score in zip(top_idx[c].tolist(), top_scores[c].tolist()):     # Find the first image that does not error out.
          if img_idx < 0:           # the index holds fewer than 3 rows
            continue
          try:
            seen_image_idx.append(img_idx)
            img = utils.get_image_from_url(self.path_array[img_idx])
            image_outputs['ret'].append((img, 'ret', score))
            if len(image_outputs) == max_num_rets:
              break
          except (UnidentifiedImageError, ConnectionError, OSError):
            pass
    if decision is not None:          # Make decision with MLP (models.py:698-704): one copy for all blocks
      probs, choice = probs.cpu().tolist(), choice.cpu().tolist()
      for k, (image_outputs, _) in enumerate(blocks):
        image_outputs['decision'] = [self.idx2dec[choice[k]]] + [probs[k]]
    else:
      for image_outputs, _ in blocks:
        image_outputs['decision'] = None
    return ret_emb

  def _batch_rerank(self, blocks, gen_images, gen_u8, ret_emb: Tensor) -> None:
    """The CLIP rerank of the generated images (models.py:733-751) for all blocks at once: block k owns gen_images[k g : (k + 1) g].
    The pixels stay on the device where the pipeline handed them back (PipelineOutput.images_u8; otherwise the PIL bytes go up in one
    copy): ops.clip_preprocess, the CLIP tower in chunks, ops.img_rerank_scores, one copy of the (n, g) scores to the host."""
    from . import ops
    m = self.model
    dev = m.logit_scale.device
    g = self.num_gen_images
    if all(u is not None for u in gen_u8):
      images = torch.cat(gen_u8, dim=0)
    else:
      images = torch.from_numpy(np.stack([np.asarray(img.convert('RGB')) for img in gen_images])).to(dev)
    # img.resize((224, 224)), then the feature extractor (models.py:737): one pass when the extractor's own size is 224, as in every
    # shipped checkpoint; otherwise the 224 x 224 uint8 pixels of the first pass go through a second one at the extractor's size
    size = int(m.feature_extractor.size)
    if size == 224:
      px = ops.clip_preprocess(images, 224, dev)
    else:
      px = ops.clip_preprocess(ops.clip_preprocess(images, 224, dev, return_u8=True)[1], size, dev)
    chunk = self._clip_chunk_size(px.shape[0])
    visual = torch.cat([m.get_visual_embs(px[i:i + chunk], mode='retrieval') for i in range(0, px.shape[0], chunk)], dim=0)
    scores = ops.img_rerank_scores(visual.reshape(px.shape[0], -1).float(), ret_emb).cpu()
    for k, (image_outputs, _) in enumerate(blocks):
      if g > 1:   # Rank images by retrieval score.
        order = torch.argsort(-scores[k])
        image_outputs['gen'] = [(gen_images[k * g + int(i)], scores[k, int(i)].item()) for i in order]
      else:
        image_outputs['gen'] = [(gen_images[k * g], scores[k, 0].item())]

  @torch.no_grad()
  def get_log_likelihood_scores(self, prompts: List) -> float:
    """Log likelihood of an interleaved image / text prompt: minus the LM's mean next-token cross-entropy over the TEXT positions
    (image positions carry the label -100 and are skipped, the <bos> tag is added once) — models.py:764-807, whose
    `self.model.lm(inputs_embeds=..., labels=...)` is the OPT forward plus the tied lm_head and HF's shifted CrossEntropyLoss.
    Here: hidden_states[-1] from gill_opt_forward, the lm_head rows of the T - 1 predicting positions through
    gill_opt_last_logits (8 positions per call), and the log-softmax / mean on the (T - 1, vocab) fp32 host tensor."""
    dev = self.model.logit_scale.device
    embs, ids, first_text = [], [], True
    for p in prompts:
      if type(p) == str:
        t = self.model.tokenizer(p, add_special_tokens=True, return_tensors="pt").input_ids.to(dev)
        if not first_text:
          t = t[:, 1:]          # <bos> only once
        first_text = False
        embs.append(self.model.input_embeddings(t))
        ids.append(t)
      elif type(p).__module__.startswith('PIL'):
        px = utils.get_pixel_values_for_model(self.model.feature_extractor, p)
        px = px.to(device=dev, dtype=self.model.logit_scale.dtype)[None, ...]
        v = self.model.get_visual_embs(px, mode='captioning')
        embs.append(v)
        ids.append(torch.full(v.shape[:2], -100, dtype=torch.int64, device=dev))
      else:
        raise ValueError(f'Input prompts should be either PIL.Image.Image or str types, got {type(p)} instead.')
    dt = next(e.dtype for e in embs)
    x = torch.cat([e.to(dt) for e in embs], dim=1)
    labels = torch.cat(ids, dim=1)[0, 1:].cpu()                  # position t predicts token t + 1
    hidden = self.model._lm_forward_hidden(x)                      # (1, T, D) fp32, post final LayerNorm
    T, D = hidden.shape[1], hidden.shape[2]
    if T < 2 or bool((labels == -100).all()):
      return float('nan')                                          # HF's mean over zero targets
    vocab = self.model.opt_cfg.vocab_size
    rows = hidden[0, :T - 1].contiguous()
    logits = torch.empty((T - 1, vocab), device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
      for r0 in range(0, T - 1, 8):
        nb = min(8, T - 1 - r0)
        # (nb, 1, D): every row is the "last position" of its own one-token sequence
        N.check(N.lib().gill_opt_last_logits(self.model._opt_handle, N.ptr(rows[r0:r0 + nb]), nb, 1, N.ptr(logits[r0:r0 + nb]),
                                             N.current_stream()))
    loss = F.cross_entropy(logits.cpu(), labels, ignore_index=-100)
    return -loss.item()

  @staticmethod
  def _scores(matrix: Tensor, query: Tensor) -> Tensor:
    """matrix (N, D) @ query (Q, D).T -> (N, Q) in matrix's dtype, through the native GEMM (the queries are padded to a multiple of
    the 4 output columns the kernel's epilogue writes at a time; Q = 1 in the one-sequence method)."""
    from . import ops
    dev = query.device
    Nq, D = matrix.shape
    Dp = (D + 63) // 64 * 64
    Q = query.numel() // D
    a = torch.zeros((Nq, Dp), device=dev, dtype=torch.bfloat16)
    a[:, :D] = matrix.to(dev)
    q4 = torch.zeros(((Q + 3) // 4 * 4, Dp), device=dev, dtype=torch.bfloat16)
    q4[:Q, :D] = query.reshape(Q, D).to(torch.bfloat16)
    return ops.gemm(a, q4, out_f32=True)[:, :Q].to(matrix.dtype)

  # ---- NEW, build-defined retrieval entries (not reference functions) -------------------------------------
  def build_retrieval_index(self, raw=None, scale: Optional[float] = None):
    """Put the retrieval matrix on the device as a GillRetrievalIndex (gill_amd/retrieval.py) and set self.ret_index.  raw (N, ret_emb_dim): the
    rows as precomputed (the cc3m*.npy embeddings), normalised on the device to scale * row / ||row|| (gill/models.py:895-900; scale defaults to
    exp(logit_scale)).  raw None: the rows of self.emb_matrix as they stand, no renormalisation.  With an index attached,
    generate_for_images_and_texts ranks through it and retrieve_images becomes available; self.emb_matrix is not touched."""
    from .retrieval import GillRetrievalIndex
    dev = self.model.logit_scale.device
    if raw is None:
      if self.emb_matrix is None:
        raise ValueError('build_retrieval_index: no raw rows given and the model has no emb_matrix')
      self.ret_index = GillRetrievalIndex.from_embeddings(torch.as_tensor(self.emb_matrix), normalize=False, device=dev)
    else:
      if scale is None:
        scale = float(self.model.logit_scale.detach().float().exp().item())
      self.ret_index = GillRetrievalIndex.from_embeddings(raw, scale=float(scale), normalize=True, device=dev)
    return self.ret_index

  @torch.no_grad()
  def retrieve_images(self, prompts, k: int = 3, exclude=None, distributed: bool = True, return_embeddings: bool = False,
                      always_add_bos: bool = False):
    """Batched prompts -> retrieved images.  `prompts` is what generate_images takes: strings, lists mixing strings and images, or a (B,T) id
    tensor.  Per prompt this equals the 'ret' branch of generate_for_images_and_texts([p], num_words=2, gen_scale_factor=1e5): the 8 [IMG] ids are appended, one OPT pass yields
    their hidden states (models.py:384), ret_text_hidden_fcs[0] maps the first of them to the retrieval embedding (models.py:671-674, [:, 0, :]),
    and one fused search of the resident index normalises it, scores every row and keeps the top k (models.py:675-691).  exclude: per prompt
    the rows to downweight by 1000 (a list of lists or a (B, E) tensor, -1 = empty).  Returns a namespace with indices (B, k) int64 (-1 past
    the index's size), scores (B, k) fp32 and paths (a list of B lists from path_array; None without one) — nothing is fetched or opened —
    and, with return_embeddings, embeddings (B, ret_emb_dim) fp32 as handed to the search (before normalisation).  With torch.distributed
    initialised the prompts are sharded contiguously over ranks, the index is replicated like the weights, and the two result tensors are
    all-gathered; a rank with an empty shard still enters the collectives."""
    from . import parallel
    if self.ret_index is None:
      raise RuntimeError('retrieve_images needs a retrieval index: call build_retrieval_index() (or load_gill(..., ret_index=True)) first')
    dev = self.model.logit_scale.device
    if (isinstance(prompts, torch.Tensor) and prompts.numel() == 0) or (not isinstance(prompts, torch.Tensor) and len(prompts) == 0):
      raise ValueError('retrieve_images: empty prompt batch')
    ids, lens, images = self._interleaved_ids(prompts, always_add_bos)
    B_total = ids.shape[0]
    if exclude is not None:
      exclude = self.ret_index._exclude(exclude, B_total)
    lo, hi = parallel.shard_range(B_total, distributed)
    ids, lens, extra = self._shard_prompts(ids, lens, images, lo, hi)
    B = ids.shape[0]
    img = torch.tensor(self.model.retrieval_token_idx, dtype=torch.int64)
    nt = self.model.num_tokens
    T = int(lens.max().item()) + nt if B > 0 else nt
    pad = self.model.tokenizer.pad_token_id
    full = torch.full((B, T), pad if pad is not None else 1, dtype=torch.int64)
    for b in range(B):
      n = int(lens[b])
      full[b, :n] = ids[b, :n]
      full[b, n:n + nt] = img
    last_idx = lens + nt - 1
    scores = torch.zeros((0, k), device=dev, dtype=torch.float32)
    indices = torch.zeros((0, k), device=dev, dtype=torch.int64)
    embs = torch.zeros((0, self.ret_index.dim), device=dev, dtype=torch.float32)
    if B > 0:
      raw, _ = self.model.img_hidden_states(full.to(dev), last_idx, **extra)
      embs = self.model.ret_text_hidden_fcs[0](raw, None)[:, 0, :].float().contiguous()     # (B, ret_emb_dim)
      scores, indices = self.ret_index.search(embs, k, normalize=True, penalty=1000.0,
                                              exclude=None if exclude is None else exclude[lo:hi])
    scores = parallel.gather_rows(scores, B_total, distributed)
    indices = parallel.gather_rows(indices, B_total, distributed)
    paths = None
    if self.path_array is not None:
      paths = [[self.path_array[i] for i in row if i >= 0] for row in indices.cpu().tolist()]
    out = SimpleNamespace(indices=indices, scores=scores, paths=paths)
    if return_embeddings:
      out.embeddings = parallel.gather_rows(embs, B_total, distributed)
    return out

  # ---- NEW, build-defined batched entry (not a reference function) ---------------------------------------
  @torch.no_grad()
  def generate_images(self, prompts, num_inference_steps: int = 50, guidance_scale: float = 7.5,
                      latents: Optional[Tensor] = None, seed: int = 1337, return_latents: bool = True,
                      return_embeddings: bool = False, distributed: bool = True, decode: bool = False, scheduler=None,
                      always_add_bos: bool = False):
    """Batched prompts -> image latents.  scheduler: the sampler of this call (GillSDPipeline.__call__), None = the pipeline's own; a stochastic
    one draws its step noise from a CPU generator seeded with `seed` and the chunk's first prompt index.  `prompts` is a list of strings (tokenized here) or an int64 tensor
    (B,T) of prompt token ids WITHOUT the [IMG] tokens (right-padded with pad_token_id).  A prompt may also be a list or tuple mixing strings and
    images (PIL, (H,W,3) uint8 arrays or tensors), as generate_for_images_and_texts takes it (models.py:600-631): each image becomes the
    n_visual_tokens rows of get_visual_embs(mode='captioning'), computed for this rank's shard only — preprocessing (ops.clip_preprocess), CLIP
    tower and visual_embeddings all on the device — and <bos> goes on the first string only unless always_add_bos.  Per prompt this equals the
    'gen' branch of generate_for_images_and_texts([p], num_words=2, gen_scale_factor=1e5): the 8 [IMG] ids are
    appended, one OPT pass yields their hidden states (models.py:384), the GILLMapper maps them to the (77,768)
    SD conditioning (models.py:387/710) and the SD-1.5 UNet runs the CFG/PLMS loop (custom_sd.py:607-651).
    With torch.distributed initialised (one process per GPU, RCCL) the prompts are sharded contiguously over
    ranks and the final latents are all-gathered (the only collective of the path).  decode=True additionally runs
    the VAE decoder (custom_sd.py:385-392) on THIS rank's shard and returns (latents_all, images_local) with
    images_local (B_local,512,512,3) uint8 on the device; decoded pixels are never exchanged between ranks."""
    from . import parallel
    dev = self.model.logit_scale.device
    if (isinstance(prompts, torch.Tensor) and prompts.numel() == 0) or (not isinstance(prompts, torch.Tensor) and len(prompts) == 0):
      raise ValueError('generate_images: empty prompt batch')
    ids, lens, images = self._interleaved_ids(prompts, always_add_bos)
    B_total = ids.shape[0]
    lo, hi = parallel.shard_range(B_total, distributed)
    ids, lens, extra = self._shard_prompts(ids, lens, images, lo, hi)
    B = ids.shape[0]
    img = torch.tensor(self.model.gen_token_idx, dtype=torch.int64)
    k = self.model.num_tokens
    T = int(lens.max().item()) + k if B > 0 else k
    pad = self.model.tokenizer.pad_token_id
    full = torch.full((B, T), pad if pad is not None else 1, dtype=torch.int64)
    for b in range(B):
      n = int(lens[b])
      full[b, :n] = ids[b, :n]
      full[b, n:n + k] = img
    last_idx = lens + k - 1
    # a rank whose shard is empty (fewer prompts than ranks) still enters the collectives below with (0, ...) tensors
    embs = torch.zeros((0, self.model.args.num_clip_tokens, self.model.args.gen_emb_dim), device=dev,
                       dtype=self.model.logit_scale.dtype)
    local = None
    if self.load_sd:
      local = torch.zeros((0, self.sd_pipe.cfg.out_channels, self.sd_pipe.cfg.sample_size, self.sd_pipe.cfg.sample_size),
                          device=dev, dtype=torch.float32)
    if B > 0:
      raw, emb = self.model.img_hidden_states(full.to(dev), last_idx, **extra)
      embs = self.model.gen_text_hidden_fcs[0](raw, emb)          # (B,77,768)
      if self.load_sd:
        lat0 = None
        if latents is not None:
          lat0 = latents[lo:hi]
        else:
          from .synth import initial_latents
          lat0 = initial_latents(B_total, self.sd_pipe.cfg.out_channels, self.sd_pipe.cfg.sample_size, seed)[lo:hi]
        outs = []
        for i in range(0, B, 8):                                    # gen_max_bs = 8 (models.py:726)
          outs.append(self.sd_pipe(prompt_embeds=embs[i:i + 8], latents=lat0[i:i + 8], guidance_scale=guidance_scale,
                                   num_inference_steps=num_inference_steps, output_type="latent", scheduler=scheduler,
                                   generator=torch.Generator().manual_seed(seed + 1 + lo + i)).images)
        local = torch.cat(outs, 0)
    images = None
    if decode:
      if not self.load_sd:
        raise ValueError('decode=True needs load_sd=True')
      images = self.sd_pipe.decode_latents(local, as_uint8=True) if B > 0 else \
          torch.zeros((0, 8 * self.sd_pipe.cfg.sample_size, 8 * self.sd_pipe.cfg.sample_size, 3), device=dev, dtype=torch.uint8)
    if not self.load_sd:
      return parallel.gather_rows(embs, B_total, distributed)
    out = parallel.gather_rows(local, B_total, distributed)
    if decode:
      return out, images
    if return_embeddings:
      return out, parallel.gather_rows(embs.float(), B_total, distributed)
    return out

  def _prompt_ids(self, prompts):
    if isinstance(prompts, torch.Tensor):
      ids = prompts.to('cpu', torch.int64)
      pad = self.model.tokenizer.pad_token_id
      # length = row length minus the TRAILING run of pad ids (a global count of non-pad ids miscounts when pad == eos/bos,
      # which load_gill sets for tokenizers without a pad token)
      if pad is None:
        lens = torch.full((ids.shape[0],), ids.shape[1])
      else:
        not_pad = (ids != pad)
        last = torch.where(not_pad.any(dim=1), ids.shape[1] - 1 - torch.argmax(not_pad.flip(1).to(torch.int64), dim=1),
                           torch.full((ids.shape[0],), -1))
        lens = last + 1
      return ids, lens.to(torch.int64)
    rows = [self.model.tokenizer(p, add_special_tokens=True, return_tensors="pt").input_ids[0] for p in prompts]
    lens = torch.tensor([len(r) for r in rows], dtype=torch.int64)
    T = int(lens.max())
    pad = self.model.tokenizer.pad_token_id
    ids = torch.full((len(rows), T), pad if pad is not None else 1, dtype=torch.int64)
    for i, r in enumerate(rows):
      ids[i, :len(r)] = r
    return ids, lens

  # ---- interleaved image + text prompts of the batched entries ------------------------------------------
  @staticmethod
  def _is_image(p) -> bool:
    if type(p).__module__.startswith('PIL'):
      return True
    return isinstance(p, (np.ndarray, torch.Tensor)) and p.dtype in (np.uint8, torch.uint8) and p.ndim == 3

  def _interleaved_ids(self, prompts, always_add_bos: bool = False):
    """_prompt_ids for prompts that may hold images: (ids, lens, images).  A list / tuple prompt is segmented as generate_for_images_and_texts
    does it (models.py:600-631): strings are tokenised, <bos> on the first one only (always_add_bos: on every one), and image number j of the
    batch takes n_visual_tokens slots with the ids -(j * n_visual_tokens + t + 1): rows of the table img_hidden_states takes as extra_rows.
    images: per prompt the list of its images, None when no prompt is a list (then ids and lens are _prompt_ids' own)."""
    if isinstance(prompts, torch.Tensor) or not any(isinstance(p, (list, tuple)) for p in prompts):
      ids, lens = self._prompt_ids(prompts)
      return ids, lens, None
    tok = self.model.tokenizer
    nv = self.model.args.n_visual_tokens
    rows, images, n_img = [], [], 0
    for p in prompts:
      if not isinstance(p, (str, list, tuple)):
        raise ValueError(f'A prompt should be a str or a list of PIL.Image.Image and str, got {type(p)} instead.')
      add_bos = True
      parts, imgs = [], []
      for seg in ([p] if isinstance(p, str) else p):
        if type(seg) == str:
          parts.append(tok(seg, add_special_tokens=add_bos, return_tensors="pt").input_ids[0].to(torch.int64))
          if not always_add_bos:
            add_bos = False
        elif self._is_image(seg):
          parts.append(-(n_img * nv + torch.arange(nv, dtype=torch.int64) + 1))
          imgs.append(seg)
          n_img += 1
        else:
          raise ValueError(f'Input prompts should be either PIL.Image.Image or str types, got {type(seg)} instead.')
      if not parts:
        raise ValueError('Input prompts should be either PIL.Image.Image or str types, got an empty prompt instead.')
      rows.append(torch.cat(parts))
      images.append(imgs)
    if n_img:
      self.model._require_vision()
    lens = torch.tensor([len(r) for r in rows], dtype=torch.int64)
    pad = tok.pad_token_id
    ids = torch.full((len(rows), int(lens.max())), pad if pad is not None else 1, dtype=torch.int64)
    for i, r in enumerate(rows):
      ids[i, :len(r)] = r
    return ids, lens, images

  clip_chunk = 16     # images per CLIP forward of _visual_rows when the tower's handle has to grow

  def _clip_chunk_size(self, n: int) -> int:
    """Images per CLIP forward for n images: the tower handle's capacity when it has one, else at most clip_chunk."""
    m = self.model
    return max(m._clip_cap if m._clip_handle is not None else 0, min(n, self.clip_chunk))

  def _visual_rows(self, images) -> Tensor:
    """The images of a shard -> (len(images) * n_visual_tokens, D) bf16: ops.clip_preprocess, then get_visual_embs(mode='captioning') in chunks
    of the CLIP handle's capacity, cast as generate_for_images_and_texts casts them on their way into the LM."""
    from . import ops
    m = self.model
    dev = m.logit_scale.device
    px = ops.clip_preprocess(images, m.feature_extractor.size, dev)
    chunk = self._clip_chunk_size(len(images))
    rows = [m.get_visual_embs(px[i:i + chunk], mode='captioning').to(torch.bfloat16) for i in range(0, len(images), chunk)]
    return torch.cat(rows, dim=0).reshape(-1, m.opt_cfg.hidden_size)

  def _shard_prompts(self, ids: Tensor, lens: Tensor, images, lo: int, hi: int):
    """The rows lo .. hi - 1 of _interleaved_ids' result for this rank: (ids, lens, keyword arguments of img_hidden_states).  Only the shard's own
    images are preprocessed and embedded; its negative ids are renumbered from the shard's first image."""
    ids, lens = ids[lo:hi], lens[lo:hi]
    if images is None:
      return ids, lens, {}
    mine = [im for row in images[lo:hi] for im in row]
    if not mine:
      return ids, lens, {}
    first = sum(len(row) for row in images[:lo]) * self.model.args.n_visual_tokens
    ids = torch.where(ids < 0, ids + first, ids)
    return ids, lens, {'extra_rows': self._visual_rows(mine)}


def load_gill(model_dir: str, load_ret_embs: bool = True, decision_model_fn: str = 'decision_model.pth.tar', ret_index: bool = False,
              opt_weights: str = 'bf16', kv_cache: str = 'bf16') -> GILL:
  """reference: gill/models.py:810-902.  Same files, same errors, same tokenizer surgery, same checkpoint format.
  opt_weights (not a reference argument): 'fp8' = GILLModel.quantize_lm('fp8'), the weight-only fp8 decoder.
  kv_cache (not a reference argument): 'fp8' = GILLModel.quantize_kv('fp8'), the e4m3 KV cache of the batch and session entries.
  ret_index (not a reference argument): also build model.ret_index from the raw cc3m rows with the device normalise (GILL.build_retrieval_index);
  emb_matrix is set as without it."""
  model_args_path = os.path.join(model_dir, 'model_args.json')
  model_ckpt_path = os.path.join(model_dir, 'pretrained_ckpt.pth.tar')
  embs_paths = [s for s in glob.glob(os.path.join(model_dir, 'cc3m*.npy'))]
  if not os.path.exists(model_args_path):
    raise ValueError(f'model_args.json does not exist in {model_dir}.')
  if not os.path.exists(model_ckpt_path):
    raise ValueError(f'pretrained_ckpt.pth.tar does not exist in {model_dir}.')
  path_array, emb_matrix = None, None
  if load_ret_embs and embs_paths:
    # models.py:826-838: every cc3m*.npy is a pickle {'paths': [...], 'embeddings': [...]} precomputed with
    # get_visual_embs(image, mode='retrieval'); rows of all files are concatenated in glob order
    path_array, emb_matrix = _read_retrieval_embeddings(embs_paths)
  else:
    if not embs_paths:
      print(f'cc3m.npy files do not exist in {model_dir}.')
    print('Running the model without retrieval.')
  with open(model_args_path, 'r') as f:
    model_kwargs = json.load(f)

  from transformers import AutoTokenizer
  tokenizer = AutoTokenizer.from_pretrained(model_kwargs['opt_version'], use_fast=False)
  if tokenizer.pad_token is None:
    tokenizer.pad_token_id = tokenizer.eos_token_id
  tokenizer.add_special_tokens({"cls_token": "<|image|>"})
  model_kwargs['retrieval_token_idx'] = []
  for i in range(model_kwargs['num_tokens']):
    print(f'Adding [IMG{i}] token to vocabulary.')
    tokenizer.add_tokens(f'[IMG{i}]')
    ret_token_idx = tokenizer(f'[IMG{i}]', add_special_tokens=False).input_ids
    assert len(ret_token_idx) == 1, ret_token_idx
    model_kwargs['retrieval_token_idx'].append(ret_token_idx[0])
  model_kwargs['gen_token_idx'] = model_kwargs['retrieval_token_idx']
  args = namedtuple('args', model_kwargs)(**model_kwargs)

  decision_model_path = os.path.join(model_dir, decision_model_fn) if decision_model_fn is not None else None
  model = GILL(tokenizer, args, path_array=path_array, emb_matrix=emb_matrix, load_sd=True, num_gen_images=1,
               decision_model_path=decision_model_path)
  model = model.eval()
  model = model.bfloat16()
  model = model.cuda()

  checkpoint = torch.load(model_ckpt_path, map_location='cpu')
  state_dict = {}
  for k, v in checkpoint['state_dict'].items():
    state_dict[k.replace('module.', '')] = v
  img_token_embeddings = state_dict['model.input_embeddings.weight'].cpu().detach()
  del state_dict['model.input_embeddings.weight']
  model.load_state_dict(state_dict, strict=False)
  with torch.no_grad():
    if 'share_ret_gen' in model_kwargs:
      assert model_kwargs['share_ret_gen'], 'Model loading only supports share_ret_gen=True for now.'
    model.model.input_embeddings.weight[-model_kwargs['num_tokens']:, :].copy_(img_token_embeddings)
  model.model.refresh_native()   # native handles snapshot the weights: rebuild after the in-place copy
  model.model.quantize_lm(opt_weights)
  model.model.quantize_kv(kv_cache)
  if emb_matrix is not None:     # models.py:895-900: unit rows scaled by exp(logit_scale), in the model's dtype, on its device
    scale = model.model.logit_scale.exp()
    m = torch.as_tensor(emb_matrix).to(device=scale.device, dtype=scale.dtype)
    model.emb_matrix = scale * (m / m.norm(dim=1, keepdim=True))
    if ret_index:
      model.build_retrieval_index(emb_matrix)
  return model


def _read_retrieval_embeddings(paths: List[str]):
  """cc3m*.npy files (pickles despite the suffix) -> (list of image paths / urls, float array (N, ret_emb_dim))."""
  import pickle
  names: List[str] = []
  rows = []
  for p in paths:
    with open(p, 'rb') as f:
      blob = pickle.load(f)
    names.extend(blob['paths'])
    rows.extend(blob['embeddings'])
  mat = np.stack(rows, axis=0)
  assert len(names) == mat.shape[0], (len(names), mat.shape)   # one embedding per path (models.py:841)
  return names, mat
