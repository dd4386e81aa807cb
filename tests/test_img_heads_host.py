"""CPU side of the image-block heads (gill_op_img_block_heads / gill_op_img_rerank_scores) and of the batched dialogue entry's tests:
the recorded operator bars are what tools/img_heads_tolerance.py measures; the inputs of the GPU tests are clear of near ties, so those tests
need no near-tie excuse; and Pillow's resize + the feature extractor equal the host restatement of ops.clip_preprocess, which is what lets
the batched rerank preprocess on the device."""
import numpy as np
import pytest
import torch

import clip_preprocess_util as P
import dialogue_batch_util as DB
import img_heads_util as H


def test_recorded_bars_are_ten_times_the_measured_distances():
  bars, d = H.load_bars(), H.measure()
  print("[img_heads bars]", bars, "measured", d)
  for k in ("ret_emb", "probs", "rerank"):
    assert d[k] > 0
    assert bars[k] == pytest.approx(10.0 * d[k], rel=1e-3), k          # (the fp64 side runs through the CPU's BLAS)
  # an fp32 accumulation of K <= 4096 products, nothing coarser: far under a bf16 ulp of a unit vector's element
  assert bars["ret_emb"] < 2 ** -9 and bars["probs"] < 2 ** -9 and bars["rerank"] < 2 ** -9


def test_restatement_agrees_with_torch():
  """heads_ref against torch's own fp64 linear / normalize / softmax."""
  D, E, C, n = H.OP_CASES[4]
  inp = H.op_inputs(D, E, C, n, H.case_seed(4))
  emb, probs, choice, _ = H.heads_ref(inp)
  x = torch.from_numpy(inp["hidden"][inp["row_idx"]]).bfloat16().double()
  y = torch.nn.functional.linear(x, torch.from_numpy(inp["Wr"]).double(), torch.from_numpy(inp["br"]).double())
  z = torch.nn.functional.linear(x, torch.from_numpy(inp["Wd"]).double(), torch.from_numpy(inp["bd"]).double())
  assert np.abs(torch.nn.functional.normalize(y, dim=-1).numpy() - emb).max() < 1e-12
  assert np.abs(z.softmax(-1).numpy() - probs).max() < 1e-12 and z.argmax(-1).tolist() == choice.tolist()
  assert inp["row_idx"][-1] == inp["row_idx"][0] and len(set(inp["row_idx"].tolist())) == n - 1      # scattered, one repeat
  # clamped indices, a zero row
  inp["row_idx"][1], inp["row_idx"][2] = -5, inp["hidden"].shape[0] + 3
  g = H.gather(inp["hidden"], inp["row_idx"])
  assert np.array_equal(g[1], H.bf(inp["hidden"][0])) and np.array_equal(g[2], H.bf(inp["hidden"][-1]))
  inp["hidden"][0] = 0
  inp["br"][:] = 0
  assert not H.heads_ref(inp)[0][1].any()
  v, r = H.rerank_inputs(3, 2, 256, 1)
  want = torch.nn.functional.cosine_similarity(torch.from_numpy(v).double().reshape(3, 2, -1), torch.from_numpy(r).double()[:, None], dim=-1)
  assert np.abs(want.numpy() - H.rerank_ref(v, r)).max() < 1e-12
  v[1] = 0
  assert H.rerank_ref(v, r)[0, 1] == 0


def test_operator_inputs_have_no_near_tie_decision():
  bars = H.load_bars()
  for ci, (D, E, C, n) in enumerate(H.OP_CASES):
    margin = H.decision_margin(H.op_inputs(D, E, C, n, H.case_seed(ci)))
    print(f"[img_heads margin] D={D} E={E} C={C} n={n}: {margin:.3e} (bar {bars['probs']:.3e})")
    assert margin > bars["probs"]


def test_engine_prompts_have_no_near_tie_pick():
  """The oracle's retrieval scores on the prompts of test_dialogue_batch_gpu.py: the 3rd and the 4th pick are more than 2 x 3e-3 apart, in
  both rounds of the two prompts the two-round test uses, so two arithmetic paths within 3e-3 of the oracle choose the same three images."""
  g = DB.golden()
  for pl in DB.prompt_lists(g):
    gaps = DB.third_fourth_gaps(g, pl, 1 if pl == DB.PARTS else 2)      # the two-round test runs the golden text and LONG
    print(f"[dialogue gaps] {pl}: {gaps}")
    assert min(gaps) > 2 * DB.SCORE_BAR, (pl, gaps)
  # the golden row: the oracle's picks are the reference's
  s = DB.oracle_ret_scores(g, DB.oracle_block_hidden(g, DB.list_ids([str(g["text"])]), 1))[0]
  assert np.abs(s.topk(3).values.numpy() - g["ret_scores"]).max() < DB.SCORE_BAR


@pytest.mark.parametrize("side,kind", [(128, "noise"), (512, "smooth"), (16, "noise")])
def test_pillow_resize_then_extractor_is_the_preprocess_restatement(side, kind):
  """generate_for_images_and_texts reranks img.resize((224, 224)) through the feature extractor; the batched entry runs ops.clip_preprocess
  at 224 (and once more at the extractor's size when that is not 224).  Equal at the uint8 stage and after normalisation, square inputs."""
  from PIL import Image
  from gill_amd.utils import ClipImageProcessor
  a = (P.noise_image if kind == "noise" else P.smooth_image)(side, side, side)
  r = Image.fromarray(a).resize((224, 224)).convert("RGB")
  u224 = P.crop_u8(a, 224)
  assert np.array_equal(np.asarray(r), u224)
  assert np.array_equal(ClipImageProcessor(224, 224)(r).pixel_values[0].numpy(), P.normalise(u224))
  assert np.array_equal(ClipImageProcessor(32, 32)(r).pixel_values[0].numpy(), P.normalise(P.crop_u8(u224, 32)))
