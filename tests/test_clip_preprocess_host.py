"""CPU checks of the CLIP preprocessing: the numpy restatement (tests/clip_preprocess_util.py) is Pillow's BICUBIC resize and ClipImageProcessor's
pixel_values to the bit, and the tap tables the library builds on the host (gill_clip_resize_taps) are the restatement's, word for word."""
import ctypes as C

import numpy as np
import pytest
import torch
from PIL import Image

import clip_preprocess_util as U
from gill_amd.utils import ClipImageProcessor

# (H, W) -> (new_h, new_w): what ClipImageProcessor(32) / (224) asks of the resampler for these frames, and an upscale to the full 224
SHAPES = [((48, 64), (32, 42)), ((20, 20), (224, 224)), ((512, 512), (224, 224)), ((333, 500), (224, 336)), ((64, 64), (32, 32)),
          ((600, 401), (335, 224)), ((17, 300), (32, 564))]
IMAGES = {"noise": U.noise_image, "smooth": U.smooth_image}


@pytest.mark.parametrize("kind", sorted(IMAGES))
@pytest.mark.parametrize("src,dst", SHAPES, ids=[f"{s[0]}x{s[1]}" for s, _ in SHAPES])
def test_restatement_is_pillow_bicubic(src, dst, kind):
  a = IMAGES[kind](src[0], src[1], seed=src[0] * 1000 + src[1])
  want = np.asarray(Image.fromarray(a).resize((dst[1], dst[0]), resample=Image.BICUBIC))
  got = U.resize(a, dst[0], dst[1])
  assert got.shape == want.shape == (dst[0], dst[1], 3)
  assert np.array_equal(got, want), f"max |diff| {np.abs(got.astype(int) - want.astype(int)).max()}"


@pytest.mark.parametrize("kind", sorted(IMAGES))
@pytest.mark.parametrize("src,dst", SHAPES, ids=[f"{s[0]}x{s[1]}" for s, _ in SHAPES])
def test_restatement_is_the_image_processor(src, dst, kind):
  size = min(dst)
  assert U.resized_shape(src[0], src[1], size) == dst
  a = IMAGES[kind](src[0], src[1], seed=src[0] * 1000 + src[1] + 1)
  want = ClipImageProcessor(size, size)(Image.fromarray(a), return_tensors="pt").pixel_values[0]
  got = torch.from_numpy(U.normalise(U.crop_u8(a, size)))
  assert got.shape == want.shape == (3, size, size) and got.dtype == want.dtype == torch.float32
  assert torch.equal(got, want)


@pytest.mark.parametrize("n_in,n_out", [(64, 42), (20, 224), (500, 336), (300, 564), (4000, 224)])
def test_library_tap_tables_are_the_restatement(n_in, n_out):
  from gill_amd import _native as N
  lib = N.lib()
  ks = U.ksize(n_in, n_out)
  assert lib.gill_clip_resize_ksize(n_in, n_out) == ks
  i32p = C.POINTER(C.c_int32)
  # the whole axis, and a window off zero as the centre crop takes it
  for first, count in ((0, n_out), ((n_out - 32) // 2, 32)):
    xmin, n, k = U.taps(n_in, n_out, first, count)
    gx, gn = np.full(count, -1, dtype=np.int32), np.full(count, -1, dtype=np.int32)
    gk = np.full((count, ks + 2), -1, dtype=np.int32)                 # a stride above ksize: the padding is zero-filled too
    N.check(lib.gill_clip_resize_taps(n_in, n_out, first, count, gx.ctypes.data_as(i32p), gn.ctypes.data_as(i32p),
                                      gk.ctypes.data_as(i32p), ks + 2))
    assert np.array_equal(gx, xmin) and np.array_equal(gn, n)
    assert np.array_equal(gk[:, :ks], k) and not gk[:, ks:].any()
    assert int(n.max()) <= ks and int((xmin + n).max()) <= n_in and int(xmin.min()) >= 0
    assert np.abs(k.sum(axis=1) - (1 << U.PRECISION_BITS)).max() <= ks   # normalised weights: one in fixed point, up to a rounding per tap


def test_tap_table_arguments_are_checked():
  from gill_amd import _native as N
  lib = N.lib()
  i32p = C.POINTER(C.c_int32)
  buf = np.zeros(64, dtype=np.int32)
  p = buf.ctypes.data_as(i32p)
  assert lib.gill_clip_resize_ksize(0, 8) == 0 and lib.gill_clip_resize_ksize(8, 1 << 20) == 0
  assert lib.gill_clip_resize_taps(8, 8, 0, 1, p, p, p, 4) != 0              # k_stride below ksize (5)
  assert b"k_stride" in lib.gill_last_error()
  assert lib.gill_clip_resize_taps(8, 8, 8, 1, p, p, p, 5) != 0              # window past the axis
  assert lib.gill_clip_resize_taps(8, 8, 0, 1, None, p, p, 5) != 0
  assert lib.gill_clip_resize_taps(0, 8, 0, 1, p, p, p, 5) != 0
  # the preprocess entry point refuses what it does not build before it touches a device
  meta = (C.c_int64 * 3)(0, 4, 4)
  need = C.c_int64(0)
  N.check(lib.gill_clip_preprocess_workspace(meta, 1, 8, C.byref(need)))
  assert need.value > 0
  assert lib.gill_clip_preprocess(1, 48, meta, 1, 8, 16, 1, None, 8, need.value, None) != 0
  assert b"size == crop_size" in lib.gill_last_error()
  assert lib.gill_clip_preprocess(1, 47, meta, 1, 8, 8, 1, None, 8, need.value, None) != 0
  assert b"outside the packed buffer" in lib.gill_last_error()
  assert lib.gill_clip_preprocess(1, 48, meta, 1, 8, 8, 1, None, 8, need.value - 1, None) != 0
  assert b"workspace" in lib.gill_last_error()
