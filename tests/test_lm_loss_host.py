"""CPU half of the LM-head loss tests: the C surface exists, the geometry answers without a GPU, and the checks of test_lm_loss_gpu.py can fail.

  0. include/gill_amd.h declares gill_op_lm_head_loss, gill_lm_loss_geometry and gill_opt_forward_loss, and the built library exports them;
  1. gill_lm_loss_geometry answers on the host and its slabs cover [0, V) exactly once;
  2. the test inputs cover the rank ranges and hold no threshold-ambiguous row;
  3. every defect of lm_loss_util.DEFECTS, standing in for the kernel, misses the operator bars by 3x or more on the test inputs, while an fp32
     emulation of the kernel's arithmetic (permuted K order, slab-wise merge) stays within half of them: the discipline of test_kv_cache_host.py;
  4. the vectorised full_labels of GILLModel (both regimes) equal the reference's loops;
  5. utils.accuracy_from_ranks equals utils.accuracy on materialised logits."""
import os
import re
from types import SimpleNamespace

import pytest
import torch

import lm_loss_util as U
from gill_amd import _native as N
from gill_amd import ops, synth, utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gill_op_lm_head_loss", "gill_lm_loss_geometry", "gill_opt_forward_loss")
SHAPES = U.operator_shapes(ops.lm_loss_geometry)

_CASES = {}


def _case(shape):
  if shape not in _CASES:
    M, V, D = shape
    geom = ops.lm_loss_geometry(M, V, D)
    x, w, t = U.build_inputs(M, V, D, U.OP_SEED, geom)
    _CASES[shape] = SimpleNamespace(geom=geom, x=x, w=w, t=t, ref=U.reference(x, w, t, geom))
  return _CASES[shape]


def test_header_declares_and_library_exports_the_new_functions():
  header = open(os.path.join(ROOT, "include", "gill_amd.h")).read()
  lib = N.lib()
  for name in NEW:
    assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} is not declared in include/gill_amd.h"
    assert name in N.SYMBOLS and hasattr(lib, name), f"{name} is not exported by libgill_amd"


@pytest.mark.parametrize("V", [1, 50, 512, 513, 1027, 50272, 50274, 262144])
def test_geometry_covers_the_vocabulary_once(V):
  row_tile, col_tile, n_slabs, cps = ops.lm_loss_geometry(40, V, 768)
  assert row_tile > 0 and col_tile > 0 and cps % col_tile == 0 and n_slabs >= 1
  slabs = [(k * cps, min(V, (k + 1) * cps)) for k in range(n_slabs)]
  assert slabs[0][0] == 0 and slabs[-1][1] == V
  assert all(a < b for a, b in slabs), "an empty slab"
  assert all(slabs[k][1] == slabs[k + 1][0] for k in range(n_slabs - 1))
  # the partition is a function of V alone: a batch whose first rows are a smaller batch is split the same way
  assert ops.lm_loss_geometry(1, V, 128) == ops.lm_loss_geometry(8192, V, 4096)
  with pytest.raises(N.GillNativeError):
    ops.lm_loss_geometry(40, V, 100)      # D % 32


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_inputs_are_unambiguous_and_cover_the_edges(shape):
  c = _case(shape)
  M, V, D = shape
  assert U.ambiguous_rows(c.ref, c.t) == []
  valid = c.t != -100
  assert int((~valid).sum()) == M // U.IGNORE_EVERY
  want = U.edge_columns(V, c.geom)[:int(valid.sum())]
  assert c.t[valid][:len(want)].tolist() == want
  if M >= 17 and V > 1000:
    r = c.ref["rank"][valid]
    hist = [int((r == 0).sum()), int(((r >= 1) & (r < 5)).sum()), int(((r >= 5) & (r <= 50)).sum()), int((r > 50).sum())]
    print(f"[{shape}] true ranks 0 / 1-4 / 5-50 / >50: {hist}")
    assert all(h > 0 for h in hist)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fp32_emulation_stays_within_half_of_the_bars(shape):
  c = _case(shape)
  emu = U.fp32_permuted(c.x, c.w, c.t, c.geom, seed=3)
  assert U.operator_ratio(f"fp32 permuted {shape}", emu, c.ref, c.t) <= 0.5


def _applies(defect, shape, geom):
  M, V, _ = shape
  return {"tail_columns_counted": V % geom[1] != 0, "merge_without_rescale": geom[2] > 1, "last_slab_dropped": geom[2] > 1,
          "target_off_by_one": M > 1, "ignore_index_scored": M >= U.IGNORE_EVERY, "self_counted": True}[defect]


@pytest.mark.parametrize("defect", U.DEFECTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_defect_misses_the_operator_bars(shape, defect):
  c = _case(shape)
  if not _applies(defect, shape, c.geom):
    return      # nothing to break at this shape (one slab, one row, no ignored row)
  bad = U.reference(c.x, c.w, c.t, c.geom, defect=defect)
  ratio = U.operator_ratio(f"{defect} {shape}", bad, c.ref, c.t)
  with pytest.raises(AssertionError):
    U.assert_operator(f"{defect} {shape}", bad, c.ref, c.t)
  assert ratio >= 3.0


# ---------------------------------------------------------------------------------------------------------------- full_labels
PAD, IMG = synth.HashTokenizer.pad_token_id, synth.IMG_TOKEN_IDS
LABEL_CASES = {
  "pad in the middle": [[2, 10, 11, 12, PAD, PAD, 13, PAD], [2, 20, PAD, 21, 22, 23, 24, 25]],
  "no pad": [[2, 10, 11, 12, 13, 14, 15, 16], [2, 20, 21, 22, 23, 24, 25, 26]],
  "[IMG1] before any pad": [[2, 10, IMG[0], IMG[1], IMG[2], 11, PAD, PAD], [2, IMG[1], 20, 21, PAD, 22, 23, 24]],
  "[IMG0] only, then pad": [[2, 10, 11, IMG[0], 12, PAD, PAD, PAD], [2, 20, 21, 22, 23, IMG[0], PAD, PAD]],
}


@pytest.mark.parametrize("mode", ["captioning", "retrieval", "generation"])
@pytest.mark.parametrize("n_front", [0, 4], ids=["no prefix", "prefix"])
@pytest.mark.parametrize("case", list(LABEL_CASES))
def test_vectorised_full_labels_equal_the_loops(case, n_front, mode):
  from gill_amd.models import GILLModel
  stub = SimpleNamespace(tokenizer=SimpleNamespace(pad_token_id=PAD), retrieval_token_idx=list(IMG), gen_token_idx=list(IMG))
  labels = torch.tensor(LABEL_CASES[case], dtype=torch.int64)
  got = GILLModel._full_labels(stub, labels, mode, n_front)
  want = U.label_loops(labels, mode, n_front, PAD, IMG, IMG)
  assert got.dtype == torch.int64 and torch.equal(got, want), (got, want)
  assert torch.equal(labels, torch.tensor(LABEL_CASES[case])), "the caller's labels were written to"
  if mode == "captioning":      # the regimes differ where [IMG0] is: captioning stops at it, the others keep it
    assert (got == IMG[0]).sum() == 0
  elif case == "[IMG0] only, then pad":
    assert (got == IMG[0]).sum() == 2


def test_label_regimes_with_distinct_retrieval_and_generation_tokens():
  from gill_amd.models import GILLModel
  ret, gen = [50266, 50267], [50270, 50271]
  stub = SimpleNamespace(tokenizer=SimpleNamespace(pad_token_id=PAD), retrieval_token_idx=ret, gen_token_idx=gen)
  labels = torch.tensor([[2, 5, gen[0], ret[0], 6, gen[1], 7, PAD], [2, ret[1], 5, 6, 7, 8, 9, 10]])
  for mode in ("captioning", "retrieval"):
    assert torch.equal(GILLModel._full_labels(stub, labels, mode, 3), U.label_loops(labels, mode, 3, PAD, ret, gen))


# ---------------------------------------------------------------------------------------------------------------- accuracy
def test_accuracy_from_ranks_equals_accuracy_on_logits():
  c = _case((129, 385, 128))
  B, T = 4, 33
  V = c.w.shape[0]
  logits = c.ref["logits"][:128].float().reshape(B, 32, V)
  logits = torch.cat([logits, torch.zeros(B, 1, V)], 1)                       # (B, T, V): the last position predicts nothing
  labels = torch.cat([torch.full((B, 1), -100), c.t[:128].reshape(B, 32)], 1)  # (B, T): position t is scored against labels[t + 1]
  want = utils.accuracy(logits[:, :-1], labels[:, 1:], -100, topk=(1, 5))
  rank = U._rank(logits[:, :-1].reshape(-1, V).double(), labels[:, 1:].reshape(-1).clamp(0, V - 1))
  rank = torch.where(labels[:, 1:].reshape(-1) != -100, rank, torch.full_like(rank, -1)).reshape(B, T - 1).int()
  got = utils.accuracy_from_ranks(rank, topk=(1, 5))
  print(f"top-1 {float(want[0]):.3f} %, top-5 {float(want[1]):.3f} %")
  assert 0.0 < float(want[0]) < float(want[1]) < 100.0
  for g, w_ in zip(got, want):
    assert g.shape == w_.shape == (1,) and torch.allclose(g, w_, rtol=0, atol=1e-4)
  # the same numbers by hand
  valid = labels[:, 1:] != -100
  top5 = logits[:, :-1].topk(5, -1).indices
  hand = [(top5[..., :k] == labels[:, 1:, None]).any(-1)[valid].float().mean() * 100 for k in (1, 5)]
  assert abs(float(hand[0]) - float(want[0])) < 1e-4 and abs(float(hand[1]) - float(want[1])) < 1e-4
