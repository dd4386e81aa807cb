"""What the CLIP image preprocessing costs on each side, and what the batched interleaved entry saves (report, no bar).

Part 1, 40 images (a VIST-shaped batch: 8 stories x 5 images) at 512x512 and at 640x480 (H x W = 480 x 640), uniform noise, size 224:
  device   ops.clip_preprocess on a packed uint8 buffer already on the device (HIP events; the two launches, the tap tables' build on the host and
           their upload), and, separately, the upload of the packed uint8 pixels (host clock around the copy and a synchronise);
  host     the utils.ClipImageProcessor loop over the same PIL images (host clock) and the upload of its fp32 pixel_values.
Part 2, 8 prompts of 5 images + 5 captions on a GILL with the ViT-L/14 tower and OPT-125m shapes (synthetic weights; the OPT size does not
  touch the preprocessing): generate_images(load_sd=False) on the batch beside 8 sequential generate_for_images_and_texts(num_words=2,
  gen_scale_factor=1e5) calls, host clock around work that ends in a synchronise, the two alternating.
Warm-up first, then `--runs` repeats of every figure: median, min and max are reported.  `--write` records the tables in `--out`
(default profiles/clip_preprocess.md).

    python tools/clip_preprocess_time.py [--write] [--runs 7] [--out profiles/clip_preprocess.md]
"""
import argparse
import os
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gill_amd  # noqa: E402
from gill_amd import ops, synth  # noqa: E402
from gill_amd.utils import ClipImageProcessor  # noqa: E402

N_IMAGES = 40
SIZE = 224
FRAMES = [(512, 512), (480, 640)]      # H x W


def _spread(xs):
  return f"{statistics.median(xs):.3f} ({min(xs):.3f} .. {max(xs):.3f})"


def _host_ms(fn, runs):
  out = []
  for _ in range(runs):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    out.append((time.perf_counter() - t) * 1e3)
  return out


def _event_ms(fn, runs):
  out = []
  for _ in range(runs):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    out.append(a.elapsed_time(b))
  return out


def preprocess_table(dev, runs):
  from PIL import Image
  rows = []
  proc = ClipImageProcessor(SIZE, SIZE)
  for H, W in FRAMES:
    rng = np.random.default_rng(H * 1000 + W)
    arrs = [rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8) for _ in range(N_IMAGES)]
    pils = [Image.fromarray(a) for a in arrs]
    packed_host = torch.from_numpy(np.stack(arrs))
    packed_dev = packed_host.to(dev)
    on_dev = lambda: ops.clip_preprocess(packed_dev, SIZE, dev)  # noqa: E731
    upload_u8 = lambda: packed_host.to(dev)  # noqa: E731
    whole = lambda: ops.clip_preprocess(arrs, SIZE, dev)  # noqa: E731    pack on the host + one upload + the device preprocess
    host_loop = lambda: torch.stack([proc(p, return_tensors="pt").pixel_values[0] for p in pils])  # noqa: E731
    px_host = host_loop()
    upload_f32 = lambda: px_host.to(dev)  # noqa: E731
    # the two sides agree before anything is timed
    got = on_dev().cpu()
    diff = (got - px_host).abs().max().item()
    assert diff <= 2e-6, diff
    for fn in (on_dev, upload_u8, whole, upload_f32, on_dev, whole):
      fn()
    t_dev = _event_ms(on_dev, runs)
    t_dev_wall = _host_ms(on_dev, runs)
    t_up8 = _host_ms(upload_u8, runs)
    t_whole = _host_ms(whole, runs)
    t_host = _host_ms(host_loop, max(3, runs // 2))
    t_up32 = _host_ms(upload_f32, runs)
    mb8, mb32 = packed_host.numel() / 1e6, px_host.numel() * 4 / 1e6
    rows.append(f"| {H} x {W} | {_spread(t_dev)} | {_spread(t_dev_wall)} | {mb8:.1f} | {_spread(t_up8)} | {_spread(t_whole)} | {_spread(t_host)} | "
                f"{mb32:.1f} | {_spread(t_up32)} | {statistics.median(t_host) + statistics.median(t_up32):.1f} | "
                f"{(statistics.median(t_host) + statistics.median(t_up32)) / statistics.median(t_whole):.1f} x |")
    print(rows[-1], f"(max |device - host| {diff:.2e})")
  return rows


def _vist_model(dev):
  from gill_amd.models import GILL
  bfw = lambda sd: {k: v.bfloat16().float() for k, v in sd.items()}  # noqa: E731
  tok = synth.HashTokenizer()
  ocfg = synth.OptConfig(vocab_size=50274, hidden_size=768, num_layers=12, num_heads=12, ffn_dim=3072)
  ccfg = synth.ClipConfig.vit_l14()
  args = SimpleNamespace(freeze_lm=True, freeze_vm=True, opt_version="facebook/opt-125m", visual_encoder="openai/clip-vit-large-patch14",
                         n_visual_tokens=4, ret_emb_dim=256, gen_emb_dim=768, text_emb_layers=[-1], text_fc_mode="gill_mapper",
                         ret_text_fc_mode="linear", num_tokens=8, num_clip_tokens=77, retrieval_token_idx=synth.IMG_TOKEN_IDS,
                         gen_token_idx=synth.IMG_TOKEN_IDS, opt_state_dict=bfw(synth.opt_state_dict(ocfg, seed=5)),
                         clip_state_dict=bfw(synth.clip_state_dict(ccfg, seed=6)), clip_config=ccfg)
  m = GILL(tok, args, load_sd=False)
  m.model.gen_text_hidden_fcs[0].load_state_dict(bfw(synth.mapper_state_dict(synth.MapperConfig(in_dim=768), seed=7)), strict=True)
  return m.eval().bfloat16().to(dev)


def vist_table(dev, runs):
  from PIL import Image
  m = _vist_model(dev)
  rows = []
  for H, W in FRAMES:
    rng = np.random.default_rng(H + W)
    stories = []
    for s in range(8):
      story = []
      for j in range(5):
        story.append(Image.fromarray(rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)))
        story.append(f"caption {j} of story {s}: a small brown dog runs along the beach")
      stories.append(story)
    batched = lambda: m.generate_images(stories)  # noqa: E731
    one_by_one = lambda: [m.generate_for_images_and_texts(s, num_words=2, gen_scale_factor=1e5) for s in stories]  # noqa: E731
    a = batched()
    b = torch.cat([r[1]["gen"][0] for r in one_by_one()], 0)
    mse = ((a.float() - b.float()) ** 2).mean().item()
    for fn in (batched, one_by_one, batched):
      fn()
    tb, to = [], []
    for _ in range(runs):                     # alternating
      tb += _host_ms(batched, 1)
      to += _host_ms(one_by_one, 1)
    rows.append(f"| {H} x {W} | {_spread(tb)} | {_spread(to)} | {statistics.median(to) / statistics.median(tb):.1f} x | {mse:.2e} |")
    print(rows[-1])
  return rows


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--write", action="store_true")
  ap.add_argument("--runs", type=int, default=7)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_preprocess.md"))
  args = ap.parse_args()
  if not torch.cuda.is_available():
    sys.exit("clip_preprocess_time needs the MI355X: a CPU run gives no time")
  gill_amd.configure_hip_runtime()
  torch.set_num_threads(synth.host_cores())
  dev = torch.device("cuda:0")
  pre = preprocess_table(dev, args.runs)
  vist = vist_table(dev, args.runs)
  if args.write:
    import PIL
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(
      "# CLIP image preprocessing: measured times (tools/clip_preprocess_time.py)\n\n"
      f"One MI355X, {synth.host_cores()} host cores, Pillow {PIL.__version__}.  {N_IMAGES} uniform-noise RGB images per frame size, resized to {SIZE} "
      f"and centre-cropped.  Every figure: median (min .. max) of {args.runs} runs after warm-up, in ms; the host loop {max(3, args.runs // 2)} runs.  "
      "The device output was compared with the host's before timing (max |difference| <= 2e-6).\n\n"
      "## Preprocessing 40 images\n\n"
      "- `device`: ops.clip_preprocess on a packed uint8 tensor already on the device, HIP events around the call: the host-side build of the "
      "tap tables, their upload, the two launches.  `device wall`: the same call by the host clock, to a synchronise.\n"
      "- `u8 upload`: the packed uint8 pixels host -> device (pageable memory), host clock to a synchronise.\n"
      "- `device path`: ops.clip_preprocess on the list of host arrays — packing, one upload, the device preprocess — host clock to a synchronise.\n"
      "- `host loop`: utils.ClipImageProcessor on each PIL image (Pillow resize, crop, numpy normalise), stacked; `fp32 upload`: its pixel_values "
      "host -> device.  `host path` = host loop + fp32 upload (medians).\n\n"
      "| frame H x W | device | device wall | u8 MB | u8 upload | device path | host loop | fp32 MB | fp32 upload | host path | host / device path |\n"
      "|---|---|---|---|---|---|---|---|---|---|---|\n" + "\n".join(pre) + "\n\n"
      "## 8 VIST-shaped prompts (5 images + 5 captions each)\n\n"
      "GILL with the ViT-L/14 tower and OPT-125m shapes, synthetic weights, load_sd=False (the output is the (8,77,768) SD conditioning).  "
      "`batched`: generate_images on the 8 prompts — one device preprocess of the 40 images, the tower in chunks, one OPT pass.  `one by one`: 8 "
      "generate_for_images_and_texts(num_words=2, gen_scale_factor=1e5) calls — per image a Pillow resize, an fp32 upload and a tower pass at batch 1, "
      "per prompt the two-step generate() loop.  Host clock around each side to a synchronise, the two alternating.  MSE: between the two sides' "
      "embeddings.\n\n"
      "| frame H x W | batched | one by one | one by one / batched | MSE |\n|---|---|---|---|---|\n" + "\n".join(vist) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
  main()
