"""Shared by test_img_heads_host.py and test_dialogue_batch_gpu.py (not a test module): the rig of
test_stages_gpu.test_retrieval_branch_vs_reference_golden (OPT-125m shapes, the seeds of golden/gill_visual_tiny.npz, a local path_array, the
decision model, load_sd=False) built once per variant, the engine test's prompt lists, and the fp32 oracle's view of them on the CPU: the
hidden state of every [IMG] block's first token (oracle/opt_ref.py) -> retrieval embedding -> scores against the embedding matrix."""
import os
from types import SimpleNamespace

import numpy as np
import torch

from gill_amd import synth

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# chosen on the CPU (test_img_heads_host.py): the oracle's 3rd and 4th retrieval picks are more than 2 x SCORE_BAR apart on each, LONG in two rounds
LONG = "a bowl of ripe cherries on a wooden table next to a folded newspaper and a cup of black coffee"
PARTS = ["show me", "a mountain lake in winter with snow on the pines"]
SCORE_BAR = 3e-3        # test_retrieval_branch_vs_reference_golden's bar on the 'ret' scores
PROB_BAR = 2e-2         # ... and on the decision probabilities


def golden():
  return np.load(os.path.join(GOLD, "gill_visual_tiny.npz"))


def prompt_lists(g):
  """Three prompt lists of different lengths; the first is the golden row."""
  return [[str(g["text"])], [LONG], list(PARTS)]


def _bfw(sd):
  return {k: v.bfloat16().float() for k, v in sd.items()}


def opt_cfg():
  return synth.OptConfig(vocab_size=50274, hidden_size=768, num_layers=12, num_heads=12, ffn_dim=3072)


def list_ids(pl):
  """The ids generate_for_images_and_texts feeds the LM for a list of strings: <bos> on the first string only."""
  tok = synth.HashTokenizer()
  ids = []
  for i, p in enumerate(pl):
    ids += tok(p, add_special_tokens=(i == 0)).input_ids
  return ids


def emb_matrix(g):
  e = synth.normal("cc3m_emb_matrix", (int(g["n_img"]), 256), int(g["clip_seed"]))
  return e / e.norm(dim=-1, keepdim=True)


def ret_proj(g):
  w = {}
  synth._linear(w, "ret_text_hidden_fcs.0.model", 256, 768, int(g["clip_seed"]))
  return w["ret_text_hidden_fcs.0.model.weight"].bfloat16().float(), w["ret_text_hidden_fcs.0.model.bias"].bfloat16().float()


def decision_linear(bias=None):
  """The decision MLP of the golden test (Dropout, Linear(768, 2)); bias: another (2,) bias, to move the outcome."""
  dec = torch.nn.Sequential(torch.nn.Dropout(0.5), torch.nn.Linear(768, 2))
  with torch.no_grad():
    dec[1].weight.copy_(synth.normal("decision.w", (2, 768), 3, 0.05).bfloat16().float())
    dec[1].bias.copy_(synth.normal("decision.b", (2,), 3, 0.1) if bias is None else torch.as_tensor(bias, dtype=torch.float32))
  return dec.eval()


def save_images(tmp_path, n_img):
  from PIL import Image
  paths = []
  for k in range(n_img):
    arr = np.full((20, 20, 3), (7 * k) % 256, dtype=np.uint8)
    arr[:, :, 1] = (13 * k + 5) % 256
    p = str(tmp_path / f"{k}.png")
    Image.fromarray(arr).save(p)
    paths.append(p)
  return paths


def build_rig(cuda, tmp_path):
  """-> namespace(m, g, dec): the GILL model of the golden retrieval test on the device, emb_matrix and decision model attached, no index."""
  from gill_amd.models import GILL
  g = golden()
  args = SimpleNamespace(freeze_lm=True, freeze_vm=True, opt_version="facebook/opt-125m", visual_encoder="openai/clip-vit-base-patch16",
                         n_visual_tokens=4, ret_emb_dim=256, gen_emb_dim=768, text_emb_layers=[-1], text_fc_mode="gill_mapper",
                         ret_text_fc_mode="linear", num_tokens=8, num_clip_tokens=77, retrieval_token_idx=synth.IMG_TOKEN_IDS,
                         gen_token_idx=synth.IMG_TOKEN_IDS, opt_state_dict=_bfw(synth.opt_state_dict(opt_cfg(), seed=int(g["opt_seed"]))))
  em = emb_matrix(g)
  m = GILL(synth.HashTokenizer(), args, path_array=save_images(tmp_path, int(g["n_img"])), emb_matrix=em, load_sd=False)
  w, b = ret_proj(g)
  with torch.no_grad():
    m.model.ret_text_hidden_fcs[0].model.weight.copy_(w)
    m.model.ret_text_hidden_fcs[0].model.bias.copy_(b)
  m.model.gen_text_hidden_fcs[0].load_state_dict(_bfw(synth.mapper_state_dict(synth.MapperConfig(in_dim=768), seed=int(g["mapper_seed"]))),
                                                 strict=True)
  dec = decision_linear()
  m.decision_model = dec
  m = m.eval().bfloat16().cuda()
  m.emb_matrix = em.to(cuda)
  return SimpleNamespace(m=m, g=g, dec=dec)


# ------------------------------------------------------------------------------------------------ the oracle's view, on the CPU
def oracle_block_hidden(g, ids, n_blocks):
  """hidden_states[-1] of the fp32 oracle at the first [IMG] token of each of n_blocks forced blocks behind the prompt ids -> (n_blocks, 768)."""
  from oracle import opt_ref
  cfg = opt_cfg()
  sd = _bfw(synth.opt_state_dict(cfg, seed=int(g["opt_seed"])))
  seq = torch.tensor([list(ids) + list(synth.IMG_TOKEN_IDS) * n_blocks], dtype=torch.int64)
  h = opt_ref.opt_hidden_states(sd, cfg.num_layers, cfg.num_heads, opt_ref.opt_embed(sd, seq))[0]
  return torch.stack([h[len(ids) + 8 * j] for j in range(n_blocks)])


def oracle_ret_scores(g, hidden_rows):
  """(n, 768) hidden rows -> (n, n_img) cosine scores of their retrieval embeddings against the embedding matrix, fp32 math."""
  w, b = ret_proj(g)
  y = hidden_rows.float() @ w.T + b
  y = y / y.norm(dim=-1, keepdim=True)
  return y @ emb_matrix(g).T


def third_fourth_gaps(g, pl, n_blocks=1):
  """Per block of the prompt list, in rounds: the oracle's gap between its 3rd and 4th pick, the earlier blocks' picks excluded (-1000)."""
  scores = oracle_ret_scores(g, oracle_block_hidden(g, list_ids(pl), n_blocks))
  gaps, seen = [], []
  for j in range(n_blocks):
    s = scores[j].clone()
    s[seen] -= 1000
    top = s.topk(4)
    gaps.append(float(top.values[2] - top.values[3]))
    seen += top.indices[:3].tolist()
  return gaps
