"""GILLModel.generate() on the weight-only fp8 decoder (quantize_lm('fp8')) end to end on the MI355X: its KV-cached steps run on the e4m3
bytes (gill_opt_cached_uses_w8), the 8-token forced [IMG] block at batch 1 included.

Rig and reference exactly as in test_w8_generate_gpu.py: ragged_decode_util.gill125_rig quantised, and a second, unquantised model whose lm
weights are w8_util.w8_state_dict of the same weights (the quantised model IS that bf16 model).  Prompts are gen_prompt_ids at the seed of
tests/golden/w8_generate_tolerance.json, one generate() call per prompt at B = 1, max_len = 5: three free decisions (min_word_tokens), then
two forced [IMG] blocks; the forwards are the prefill, three single-token steps and one 8-token step.

  tokens        equal to the reference model's generate();
  hidden rows   output_embeddings[-1] at the 11 generated positions within kv_cache_util.REL_BAR of the reference's;
  near ties     a disagreement is excused only when the reference run's own logits put the two tokens within the golden m; the row then
                leaves the comparison; excused decisions are capped at 5 % of all decisions (at most 1 of 30; on these prompts the oracle's
                decisions all clear m: tests/test_w8_host.py::test_generate_margin_claim_holds_on_the_dequantised_weights);
  round trip    quantize_lm('bf16') afterwards restores generate()'s bits;
  host waits    _decode_host_waits is what the bf16 run had (one read per step at B = 1)."""
import pytest
import torch

import kv_cache_util as U
import ragged_decode_util as R
from test_decode_sample_gpu import IMG
from test_w8_generate_gpu import KW, _golden, reference   # noqa: F401  (reference: the module-scoped fixture)

pytestmark = pytest.mark.gpu
MAX_LEN = 5


@pytest.fixture(scope="module")
def gill125(cuda):
  g = R.gill125_rig(cuda)
  yield g
  g.model.quantize_lm(None)          # the rig is shared with other modules


def _generate(model, ids, n, cuda):
  emb = model.input_embeddings(ids[:, :n].to(cuda))
  out, embs, logits = model.generate(emb, MAX_LEN, **KW)
  torch.cuda.synchronize()
  return out, embs, logits, model._decode_host_waits


def test_generate_runs_its_cached_steps_on_the_quantised_decoder(cuda, gill125, reference):   # noqa: F811
  from gill_amd import _native as N
  m, ref = gill125.model, reference.model
  rec = _golden()
  tol = float(rec["m"])
  ids, lens = R.gen_prompt_ids(rec["seed"])
  m.quantize_lm(None)
  before = [_generate(m, ids[b:b + 1], n, cuda) for b, n in enumerate(lens)]
  m.quantize_lm("fp8")
  excused = 0
  for b, n in enumerate(lens):
    out8, embs8, _, waits8 = _generate(m, ids[b:b + 1], n, cuda)
    h = m._opt_handle
    assert N.lib().gill_opt_weight_mode(h) == 1
    assert N.lib().gill_opt_cached_uses_w8(h, 1, 1, n) == 1 and N.lib().gill_opt_cached_uses_w8(h, 1, 8, n + 3) == 1
    assert N.lib().gill_opt_cached_uses_w8(h, 1, n, 0) == 0
    assert waits8 == before[b][3], f"row {b}: {waits8} host waits on the fp8 decoder, {before[b][3]} on bf16"
    out, embs, logits, _ = _generate(ref, ids[b:b + 1], n, cuda)
    got, want = out8[0].tolist(), out[0].tolist()
    assert len(want) == 19 and want[3:11] == IMG and want[11:19] == IMG
    if got != want:
      col = next(j for j in range(min(len(got), 19)) if got[j] != want[j])
      assert col < 3, (b, got, want)
      margin = abs(float(logits[col][0, got[col]] - logits[col][0, want[col]]))
      print(f"[w8 generate] prompt {b} decision {col}: fp8 picked {got[col]}, reference {want[col]}; their logits are {margin:.3e} apart "
            f"(m = {tol:.3e})")
      assert margin <= tol, (b, col, got[col], want[col], margin)
      excused += 1
      continue
    a, w = embs8[-1][0, n:n + 11].float().cpu(), embs[-1][0, n:n + 11].float().cpu()
    assert a.shape == w.shape == (11, w.shape[-1])
    rel = ((a - w).norm() / w.norm()).item()
    differs = not torch.equal(embs8[-1][0, n:n + 11], before[b][1][-1][0, n:n + 11])
    print(f"[w8 generate] prompt {b} (length {n}): hidden rows of the generated positions rel_l2 {rel:.3e}; differ from the bf16 decoder's: {differs}")
    assert rel < U.REL_BAR
    assert differs, "the quantised decoder returned the bf16 decoder's bits"
  assert excused * 20 <= len(lens) * MAX_LEN, excused
  # mode round trip
  m.quantize_lm("bf16")
  for b, n in enumerate(lens):
    out, embs, logits, waits = _generate(m, ids[b:b + 1], n, cuda)
    out0, embs0, logits0, waits0 = before[b]
    assert torch.equal(out, out0) and waits == waits0
    assert len(embs) == len(embs0) and all(torch.equal(x, y) for x, y in zip(embs, embs0)), "bf16 hidden rows are not restored bit for bit"
    assert len(logits) == len(logits0) and all(torch.equal(x, y) for x, y in zip(logits, logits0)), "bf16 logits are not restored bit for bit"
