"""Stable Diffusion text embeddings of a caption file: the counterpart of the reference's scripts/preprocess_sd_embeddings.py, on the
native CLIP text tower (gill_clip_text_forward).  These are the regression targets the GILLMapper is trained on.

  python tools/sd_text_embeddings.py datasets/cc3m_val.tsv data/cc3m/validation/clip_embs --model-dir <stable-diffusion dir>
  python tools/sd_text_embeddings.py - /tmp/embs --synthetic 1280 --batch 128 [--no-save]

The caption file is tab separated with a header line: caption <tab> image id.  Ids that already have a file in the output directory
are skipped; every other caption gets `<id>.npy` holding its (77, D) float32 embedding, `pipe(batch, return_prompts_only=True)`.
--synthetic N needs no checkpoint: N made-up captions, hashed to CLIP-vocabulary ids, through synthetic weights of the SD-1.5 (or
--geometry sd21) tower.

Printed: a JSON line with the end-to-end rate (tokenising, forward, copy to the host, file writes) and, measured with HIP events
over repeated forwards of one uploaded batch, ms per forward, captions/s of the forward alone and its share of the MI355X's
2.5 PFLOP/s dense bf16 peak (FLOPs counted from the shapes: clip_text.clip_text_flops), with the GPU clock sampled over that loop.
"""
import argparse
import json
import os
import sys
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

PEAK_BF16_FLOPS = 2.5e15


class HashClipTokenizer:
  """Offline stand-in for CLIPTokenizer (no vocabulary files needed): whitespace words hash to ids below BOS; rows are framed and
  padded the way CLIPTokenizer does it for Stable Diffusion (BOS 49406, EOS = pad 49407)."""
  model_max_length = 77

  def __init__(self, vocab=49408):
    self.vocab, self.bos_token_id, self.eos_token_id = vocab, vocab - 2, vocab - 1

  def __call__(self, text, padding=False, max_length=None, truncation=False, return_tensors=None):
    from types import SimpleNamespace
    rows = []
    for t in ([text] if isinstance(text, str) else list(text)):
      ids = [self.bos_token_id] + [zlib.crc32(w.encode()) % (self.vocab - 2) for w in t.split()] + [self.eos_token_id]
      if truncation and max_length is not None and len(ids) > max_length:
        ids = ids[:max_length - 1] + [self.eos_token_id]
      rows.append(ids)
    width = max_length if padding == "max_length" else max(len(r) for r in rows)
    return SimpleNamespace(input_ids=torch.tensor([r + [self.eos_token_id] * (width - len(r)) for r in rows], dtype=torch.int64))

  def batch_decode(self, ids):
    return [" ".join(f"w{int(t)}" for t in row if int(t) < self.vocab - 2) for row in ids]


def synthetic_captions(n, seed=0):
  g = np.random.Generator(np.random.Philox(key=[seed, 77]))
  lens = g.integers(4, 40, size=n)
  return [" ".join(f"word{int(w)}" for w in g.integers(0, 30000, size=int(k))) for k in lens], [f"syn{i:07d}" for i in range(n)]


def read_captions(path, out_dir):
  existing = {f[:-4] for f in os.listdir(out_dir) if f.endswith(".npy")}
  captions, ids = [], []
  with open(path) as f:
    for line in f.readlines()[1:]:
      d = line.rstrip("\n").split("\t")
      if len(d) >= 2 and d[1] not in existing:
        captions.append(d[0])
        ids.append(d[1])
  return captions, ids


def build_pipe(a, dev):
  from gill_amd import synth
  from gill_amd.sd import GillSDPipeline
  if a.model_dir:
    return GillSDPipeline.from_pretrained(a.model_dir, device=dev, max_batch=2, text_max_batch=a.batch)
  if a.synthetic is None:
    raise SystemExit("give --model-dir (a local Stable Diffusion directory) or --synthetic N")
  tcfg = synth.ClipTextConfig.sd21() if a.geometry == "sd21" else synth.ClipTextConfig.sd15()
  # return_prompts_only never reaches the UNet: a reduced-width one keeps the pipeline object whole
  ucfg = synth.UNetConfig(block_out_channels=(64, 128, 256, 256), num_heads=4, cross_attention_dim=tcfg.hidden_size, sample_size=16)
  return GillSDPipeline(synth.unet_state_dict(ucfg, seed=0), ucfg, None, dev, max_batch=2,
                        text_state=synth.clip_text_state_dict(tcfg, seed=0), text_cfg=tcfg, tokenizer=HashClipTokenizer(tcfg.vocab_size),
                        text_max_batch=a.batch)


def time_forward(pipe, ids, dev, seconds, repeat):
  """HIP-event time of one forward of `ids` (already validated), averaged over enough back-to-back forwards to fill `seconds`;
  `repeat` such loops, all returned (the caller reports their median)."""
  import bench
  enc = pipe.text_encoder
  ids_dev = enc.validate_ids(ids).to(dev)
  out = torch.empty((ids.shape[0], ids.shape[1], enc.cfg.hidden_size), device=dev, dtype=torch.float32)
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

  def run(n):
    e0.record()
    for _ in range(n):
      enc.forward_device(ids_dev, None, out)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n

  run(5)                                   # warm-up: code objects, workspace, clocks
  iters = int(min(20000, max(20, seconds * 1e3 / max(run(10), 1e-3))))
  clocks = bench.ClockSampler(dev)
  clocks.start()
  runs = [run(iters) for _ in range(repeat)]
  return runs, iters, clocks.stop()


def main():
  ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument("captions", help="tab separated caption file with a header line ('-' with --synthetic)")
  ap.add_argument("out_dir")
  ap.add_argument("--batch", type=int, default=128)
  ap.add_argument("--model-dir", default=None, help="local Stable Diffusion directory (unet/, text_encoder/, tokenizer/)")
  ap.add_argument("--synthetic", type=int, default=None, metavar="N", help="N made-up captions through synthetic weights")
  ap.add_argument("--geometry", choices=("sd15", "sd21"), default="sd15", help="tower of --synthetic")
  ap.add_argument("--truncate-side", choices=("left", "right"), default="right")
  ap.add_argument("--no-save", action="store_true", help="measure only: write no files")
  ap.add_argument("--time-seconds", type=float, default=2.0, help="length of one HIP-event timing loop (0: skip it)")
  ap.add_argument("--repeat", type=int, default=3, help="timing loops; the median is reported")
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("sd_text_embeddings.py runs the native text tower: it needs the MI355X")
  import gill_amd
  gill_amd.configure_hip_runtime()
  dev = torch.device("cuda:0")
  os.makedirs(a.out_dir, exist_ok=True)
  if a.synthetic is not None:
    captions, image_ids = synthetic_captions(a.synthetic)
    existing = {f[:-4] for f in os.listdir(a.out_dir) if f.endswith(".npy")}
    keep = [i for i, k in enumerate(image_ids) if k not in existing]
    captions, image_ids = [captions[i] for i in keep], [image_ids[i] for i in keep]
  else:
    captions, image_ids = read_captions(a.captions, a.out_dir)
  pipe = build_pipe(a, dev)
  pipe.truncate_side = a.truncate_side
  if captions:
    pipe(captions[:a.batch], return_prompts_only=True)          # warm-up of the first batch's shapes
  torch.cuda.synchronize()
  t0 = time.time()
  for i in range(0, len(captions), a.batch):
    emb = pipe(captions[i:i + a.batch], return_prompts_only=True).detach().cpu().numpy()
    if not a.no_save:
      for j, k in enumerate(image_ids[i:i + a.batch]):
        np.save(os.path.join(a.out_dir, f"{k}.npy"), emb[j])
  dt = time.time() - t0
  enc = pipe.text_encoder
  rec = {"captions": len(captions), "batch": a.batch, "hidden_size": enc.cfg.hidden_size, "num_layers": enc.cfg.num_layers,
         "saved": not a.no_save, "end_to_end_s": dt, "captions_per_s_end_to_end": len(captions) / dt if captions and dt > 0 else None}
  if a.time_seconds > 0 and captions:
    ids = pipe._prompt_ids(captions[:a.batch])
    runs, iters, clocks = time_forward(pipe, ids, dev, a.time_seconds, max(1, a.repeat))
    ms = float(np.median(runs))
    flops = enc.flops(ids.shape[0], ids.shape[1])
    rec.update({"forward_rows": ids.shape[0] * ids.shape[1], "forward_ms": ms, "forward_ms_runs": runs, "forward_iters": iters,
                "captions_per_s_forward": ids.shape[0] / ms * 1e3, "forward_tflop": flops / 1e12,
                "achieved_tflops": flops / ms / 1e9, "share_of_bf16_peak": flops / (ms * 1e-3) / PEAK_BF16_FLOPS,
                "sclk_mhz_mean": clocks["sclk_mhz_mean"], "power_w_mean": clocks["power_w_mean"]})
    print(f"{ids.shape[0]} captions per forward: {ms:.3f} ms (HIP events, median of {len(runs)} loops of {iters} forwards), {rec['captions_per_s_forward']:.0f} captions/s, "
          f"{rec['achieved_tflops']:.1f} TFLOP/s = {100 * rec['share_of_bf16_peak']:.2f} % of the bf16 peak")
  print(json.dumps(rec))


if __name__ == "__main__":
  main()
