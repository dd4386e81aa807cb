"""ops.clip_preprocess (gill_clip_preprocess) on the MI355X against gill_amd.utils.ClipImageProcessor, i.e. against Pillow's own BICUBIC resize:
the uint8 stage (resize + centre crop) must equal the PIL-derived crop exactly, the fp32 output within 2e-6 absolute — two fp32 roundings at
magnitude <= 4, allowing for a fused multiply-subtract in front of the division.  The PIL-derived crop is ClipImageProcessor's own steps up to
the cast (tests/test_clip_preprocess_host.py pins the numpy restatement of them to Pillow bit for bit)."""
import numpy as np
import pytest
import torch
from PIL import Image

import clip_preprocess_util as U
from gill_amd import ops
from gill_amd.utils import ClipImageProcessor

pytestmark = pytest.mark.gpu

# (H, W), size: landscape downscale with the crop window off zero; upscale; exact 2:1; extreme aspect (window far from the origin, one axis
# upscaled); portrait; landscape
FRAMES = [((48, 64), 32), ((20, 20), 32), ((64, 64), 32), ((17, 300), 32), ((600, 401), 224), ((333, 500), 224)]
F32_BAR = 2e-6


def _pil_crop(a, size):
  """The uint8 pixels ClipImageProcessor(size, size) normalises, by Pillow itself."""
  nh, nw = U.resized_shape(a.shape[0], a.shape[1], size)
  r = np.asarray(Image.fromarray(a).resize((nw, nh), resample=Image.BICUBIC), dtype=np.uint8)
  top, left = (nh - size) // 2, (nw - size) // 2
  return r[top:top + size, left:left + size]


def _check(name, a, size, px, u8):
  want_u8 = _pil_crop(a, size)
  want = ClipImageProcessor(size, size)(Image.fromarray(a), return_tensors="pt").pixel_values[0]
  got_u8, got = u8.cpu().numpy(), px.cpu()
  d_u8 = int(np.abs(got_u8.astype(np.int32) - want_u8.astype(np.int32)).max())
  d_f = (got - want).abs().max().item()
  print(f"[clip_preprocess {name}] {a.shape[0]}x{a.shape[1]} -> {size}: max |u8 diff| {d_u8}, max |fp32 diff| {d_f:.3e}")
  assert got_u8.shape == (size, size, 3) and got.shape == (3, size, size) and got.dtype == torch.float32
  assert np.array_equal(got_u8, want_u8)
  assert d_f <= F32_BAR


@pytest.mark.parametrize("hw,size", FRAMES, ids=[f"{h}x{w}_{s}" for (h, w), s in FRAMES])
def test_single_noise_image(cuda, hw, size):
  a = U.noise_image(hw[0], hw[1], seed=hw[0] * 1000 + hw[1])
  px, u8 = ops.clip_preprocess([Image.fromarray(a)], size, cuda, return_u8=True)
  assert px.shape == (1, 3, size, size) and u8.shape == (1, size, size, 3) and u8.dtype == torch.uint8 and px.is_cuda
  _check("noise", a, size, px[0], u8[0])
  assert torch.equal(ops.clip_preprocess([a], size, cuda), px)               # an array in, no uint8 stage out: the same fp32


@pytest.mark.parametrize("value", [0, 255])
def test_flat_images_land_on_the_clip_edges(cuda, value):
  a = np.full((20, 20, 3), value, dtype=np.uint8)
  px, u8 = ops.clip_preprocess([a], 32, cuda, return_u8=True)
  assert bool((u8 == value).all())
  _check(f"flat {value}", a, 32, px[0], u8[0])


def test_mixed_sizes_in_one_call(cuda):
  """All the 32-px frames and the two flat images in one packed buffer, as PIL images, arrays and tensors on the host and on the device."""
  frames = [U.noise_image(h, w, seed=h + w) for (h, w), s in FRAMES if s == 32]
  frames += [np.zeros((20, 20, 3), dtype=np.uint8), np.full((20, 20, 3), 255, dtype=np.uint8), U.smooth_image(41, 23, seed=3)]
  kinds = [Image.fromarray, lambda a: a, torch.from_numpy, lambda a: torch.from_numpy(a).to(cuda)]
  images = [kinds[i % 4](a) for i, a in enumerate(frames)]
  px, u8 = ops.clip_preprocess(images, 32, cuda, return_u8=True)
  assert px.shape == (len(frames), 3, 32, 32)
  for i, a in enumerate(frames):
    _check(f"mixed[{i}]", a, 32, px[i], u8[i])
  # the 224-px frames together: more than one block per image and different row counts per image
  big = [U.noise_image(h, w, seed=h + w) for (h, w), s in FRAMES if s == 224]
  px, u8 = ops.clip_preprocess(big, 224, cuda, return_u8=True)
  for i, a in enumerate(big):
    _check(f"mixed224[{i}]", a, 224, px[i], u8[i])


def test_device_batch_tensor(cuda):
  """A (B,H,W,3) uint8 device tensor, the form GillSDPipeline.decode_latents returns: no host copy of the pixels on the way in."""
  a = np.stack([U.noise_image(64, 64, seed=1), U.smooth_image(64, 64, seed=2)])
  t = torch.from_numpy(a).to(cuda)
  px, u8 = ops.clip_preprocess(t, 32, cuda, return_u8=True)
  assert px.shape == (2, 3, 32, 32)
  for i in range(2):
    _check(f"device[{i}]", a[i], 32, px[i], u8[i])


def test_bad_inputs_are_refused(cuda):
  with pytest.raises(ValueError):
    ops.clip_preprocess([np.zeros((4, 4, 3), dtype=np.float32)], 32, cuda)
  with pytest.raises(ValueError):
    ops.clip_preprocess([np.zeros((4, 4), dtype=np.uint8)], 32, cuda)
  with pytest.raises(ValueError):
    ops.clip_preprocess([], 32, cuda)
