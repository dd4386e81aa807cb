"""The yardstick of the CLIP preprocessing tests: Pillow's 8-bit BICUBIC resize restated in numpy (tap tables in doubles, 22-bit fixed-point
coefficients, two integer passes with a uint8 intermediate), then the centre crop and the normalisation of gill_amd.utils.ClipImageProcessor.
tests/test_clip_preprocess_host.py pins it to Pillow itself; the library's tap tables and the device kernel are compared with it."""
import numpy as np

PRECISION_BITS = 22
MEAN = np.asarray((0.48145466, 0.4578275, 0.40821073), dtype=np.float32)
STD = np.asarray((0.26862954, 0.26130258, 0.27577711), dtype=np.float32)


def cubic(t):
  """Pillow's bicubic_filter (a = -0.5) on an array of doubles, operation for operation."""
  a = -0.5
  t = np.abs(np.asarray(t, dtype=np.float64))
  inner = ((a + 2.0) * t - (a + 3.0)) * t * t + 1
  outer = (((t - 5) * t + 8) * t - 4) * a
  return np.where(t < 1.0, inner, np.where(t < 2.0, outer, 0.0))


def ksize(n_in, n_out):
  scale = n_in / n_out
  return int(np.ceil(2.0 * max(scale, 1.0))) * 2 + 1


def taps(n_in, n_out, first=0, count=None):
  """(xmin (count,), n (count,), k (count, ksize) int32, zero past n) for the outputs first .. first + count - 1 of one axis n_in -> n_out."""
  count = n_out - first if count is None else count
  scale = n_in / n_out
  fs = max(scale, 1.0)
  support = 2.0 * fs
  ks = ksize(n_in, n_out)
  xx = np.arange(first, first + count, dtype=np.float64)
  center = (xx + 0.5) * scale
  xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)          # the cast truncates toward zero, as C's does
  xmax = np.minimum((center + support + 0.5).astype(np.int64), n_in)
  n = xmax - xmin
  w = np.zeros((count, ks), dtype=np.float64)
  ww = np.zeros(count, dtype=np.float64)
  for x in range(ks):                                                        # tap by tap: the sum runs in the resampler's order
    live = x < n
    wx = np.where(live, cubic((x + xmin - center + 0.5) / fs), 0.0)
    w[:, x] = wx
    ww = np.where(live, ww + wx, ww)
  w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
  one = float(1 << PRECISION_BITS)
  k = np.where(w < 0, np.trunc(-0.5 + w * one), np.trunc(0.5 + w * one)).astype(np.int32)
  k[np.arange(ks)[None, :] >= n[:, None]] = 0
  return xmin.astype(np.int32), n.astype(np.int32), k


def resample_axis0(a, n_out, first=0, count=None):
  """One pass along axis 0 of a uint8 array: out[i] = clip((2^21 + sum_x k[i, x] a[xmin[i] + x]) >> 22, 0, 255)."""
  xmin, n, k = taps(a.shape[0], n_out, first, count)
  out = np.empty((len(xmin),) + a.shape[1:], dtype=np.uint8)
  for i in range(len(xmin)):
    win = a[xmin[i]:xmin[i] + n[i]].astype(np.int64)
    acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(k[i, :n[i]].astype(np.int64), win, axes=(0, 0))
    out[i] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
  return out


def resize(a, new_h, new_w):
  """Image.fromarray(a).resize((new_w, new_h), Image.BICUBIC) for an (H, W, C) uint8 array: the horizontal pass first, then the vertical one
  on its uint8 result.  (Pillow skips a pass whose axis keeps its length; the taps of such a pass are the identity.)"""
  mid = resample_axis0(a.transpose(1, 0, 2), new_w).transpose(1, 0, 2)
  return resample_axis0(mid, new_h)


def resized_shape(h, w, size):
  """ClipImageProcessor's target: the shortest edge -> size, the long one int(size * long / short)."""
  short, long = (w, h) if w <= h else (h, w)
  new_short, new_long = size, int(size * long / short)
  return (new_long, new_short) if w <= h else (new_short, new_long)      # (new_h, new_w)


def crop_u8(a, size):
  """The (size, size, 3) uint8 pixels ClipImageProcessor(size, size) normalises: resize, then the centre crop."""
  nh, nw = resized_shape(a.shape[0], a.shape[1], size)
  r = resize(a, nh, nw)
  top, left = (nh - size) // 2, (nw - size) // 2
  return r[top:top + size, left:left + size]


def normalise(u8):
  """(size, size, 3) uint8 -> (3, size, size) float32, the arithmetic of ClipImageProcessor in float32."""
  x = u8.astype(np.float32) * np.float32(1.0 / 255.0)
  x = (x - MEAN) / STD
  return np.ascontiguousarray(x.transpose(2, 0, 1))


def noise_image(h, w, seed):
  return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def smooth_image(h, w, seed):
  y, x = np.mgrid[0:h, 0:w].astype(np.float64)
  ph = np.random.default_rng(seed).uniform(0, 6.28, size=3)
  chans = [127.5 + 127.5 * np.sin(x / max(w, 2) * (3.0 + c) + ph[c]) * np.cos(y / max(h, 2) * (2.0 + c)) for c in range(3)]
  return np.clip(np.stack(chans, axis=-1).round(), 0, 255).astype(np.uint8)
