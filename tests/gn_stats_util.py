"""Shared by test_gn_stats_gpu.py and test_gn_stats_host.py (not a test module): the fused GroupNorm statistics of csrc/gemm.hip (producers:
GemmArgs::gn_stats) and csrc/norm.hip (consumer: groupnorm_apply_launch), through gill_amd.ops.conv3x3_gn_stats / gemm_gn_stats /
groupnorm_from_stats.

  * inputs under which every partial matters.  `consumer_acts`: N(0,1) noise times a per-(sample, bin) scale in [0.5, 2] plus an offset in
    [-3, 3] that differs per (sample, 16-row block, bin) (ln_gemm_util.distinct_rows, one level down).  `producer_case`: the operands of a
    producer launch — activations with an offset per (sample, 16-row block) under weights with a positive mean 1 / K (the offset reaches
    the output), a bias that differs per bin, and where the form takes them a row vector per (sample, bin) and a residual with an offset per
    (sample, 16-row block, bin) — plus the fp32 reference of the output;
  * `partials_ref`: fp64 {sum, sum of squares} of a bf16 tensor per (sample, slab, bin) in the order the producers file them (the parity
    classes of the four-tap upsample form included), with the producer-side defects; `emulate_partials`: the same sums in fp32;
  * `bin_totals` / `host_partials`: the true per-bin totals of a tensor and an fp64 split of them into ns uneven positive shares, rounded
    to fp32 once.  Shares 16, 512 and the last one carry ~1/8 .. 1/5 of the total each, so that losing any one of them moves a group's
    rstd by 6 % or more — visible in the normalised tensor, not only in the table;
  * `groupnorm_ref` / `scale_shift_ref`: fp64 GroupNorm (+ SiLU) of the concatenated tensor and the scale | shift table;
  * `emulate_apply`: an fp32 restatement of the consumer (16-partial segments on the fixed tree, segments in order, bins in order,
    var = E[x^2] - E[x]^2, rsqrt, fma; more than 64 partials through groupnorm_total_kernel's slices first), with a `defect=` switch.

Bars.
  STAT_BAR: the fp32 partials against fp64 sums of the stored tensor, |d sum| / sum |v| and |d sumsq| / sum v^2 per partial
  (`partials_figure`), and the scale | shift table in the same unit (`table_figure`: an error eps of that kind in a group's sums moves
  var = E2 - mean^2 by at most 3 eps E2, hence rstd by 1.5 eps K rstd with K = E2 / (var + eps_gn), and shift = beta - mean scale by
  eps |scale| (E|x| + 1.5 K |mean|); the figure is the table's error over those two unit responses).  Measured on the CPU over every
  geometry of the two test files (test_gn_stats_host.py prints and asserts them): the fp32 emulations reach at most 4.6e-7 (producers'
  partials 4.6e-7, table 1.2e-7); the weakest defect is sums_of_unrounded_values at 3.4e-4 .. 1.7e-3, every other defect is at 7e-2 or
  more (table: dropped_partial_16 7.1e-2; partials: slab_shifted_one 0.46).  STAT_BAR = 1e-5: the emulation within 0.05 of it, the
  weakest defect 34x above it.
  Y_BAR: the normalised bf16 tensor against fp64, max |error| over max |ref| per (sample, group) (`group_figure`): the project's
  1.5e-2 (test_groupnorm).  Emulation at most 3.8e-3 (the bf16 rounding of the output); the weakest consumer defect in a two-block
  geometry (no table there) is dropped_partial_16 at 0.10, 6.7x the bar."""
import functools
import math

import torch
import torch.nn.functional as F

STAT_BAR = 1e-5
Y_BAR = 1.5e-2
TENSOR_BAR = 1.5e-2          # the producers' output against the fp32 conv / GEMM reference: test_conv3x3's bar
GROUPS = 32

CONSUMER_DEFECTS = ("dropped_last_partial", "dropped_partial_16", "partials_of_other_sample", "bin_off_by_one", "block2_offset_ignored",
                    "straddling_group_takes_block1_only", "totals_stop_at_512", "block2_totals_at_block1_offset")
PRODUCER_DEFECTS = ("slab_shifted_one", "bin_shifted_one", "sums_of_unrounded_values", "residual_left_out")

# consumer geometries: (C1, bin1, C2, bin2); one block: C2 == 0
ONE_BLOCK_NSLAB = (1, 15, 16, 17, 33, 63, 64, 65, 128, 513)
ONE_BLOCK = [(320, 5, 2, 64, ns) for ns in ONE_BLOCK_NSLAB] + [(128, 4, 2, 100, 4)]       # (C, bin, B, HW, nslab)
TWO_BLOCK = [(640, 10, 320, 5), (1280, 20, 640, 10), (1280, 20, 1280, 20), (320, 5, 320, 5), (640, 5, 320, 5)]
TWO_BLOCK_NSLAB = [(16, 4), (4, 1), (65, 4), (4, 65)]
TWO_BLOCK_HW = (64, 256)


def bf(x):
  return x.bfloat16().float()


def _gen(seed):
  return torch.Generator().manual_seed(seed)


def _rnd(shape, seed, scale=1.0):
  return torch.randn(shape, generator=_gen(seed)) * scale


def _uniform(shape, seed, lo, hi):
  return lo + (hi - lo) * torch.rand(shape, generator=_gen(seed))


def _block_offsets(B, rows, nbins, width, seed, lo, hi):
  """(B, rows, nbins * width): a value in [lo, hi] per (sample, 16-row block, bin), repeated over the block's rows and the bin's channels."""
  o = _uniform((B, (rows + 15) // 16, nbins), seed, lo, hi)
  return o.repeat_interleave(16, 1)[:, :rows].repeat_interleave(width, 2)


# ------------------------------------------------------------------------------------------------ consumer side
@functools.lru_cache(maxsize=None)
def consumer_acts(B, HW, C, bin, seed):
  """(B, HW, C) fp32 holding bf16 values (module docstring)."""
  scale = _uniform((B, 1, C // bin), seed + 1, 0.5, 2.0).repeat_interleave(bin, 2)
  return bf(_rnd((B, HW, C), seed) * scale + _block_offsets(B, HW, C // bin, bin, seed + 2, -3.0, 3.0))


@functools.lru_cache(maxsize=None)
def norm_params(C, seed):
  return 1.0 + 0.2 * _rnd((C,), seed), 0.3 * _rnd((C,), seed + 1)


def bin_totals(x, bin):
  """fp64 (B, C / bin, 2): {sum, sum of squares} of x (B, HW, C) per (sample, bin)."""
  B, HW, C = x.shape
  v = x.double().reshape(B, HW, C // bin, bin)
  return torch.stack([v.sum((1, 3)), (v * v).sum((1, 3))], -1)


def host_partials(tot, ns, seed):
  """fp32 (B, ns, nb, 2) adding up to tot (B, nb, 2) fp64: uneven positive shares per (sample, partial, bin, moment); shares 16, 512 and
  the last one (where they exist) are a quarter of all the others together."""
  B, nb, _ = tot.shape
  w = _uniform((B, ns, nb, 2), seed, 0.2, 1.0).double()
  big = sorted({i for i in (16, 512, ns - 1) if 0 <= i < ns})
  if len(big) < ns:
    rest = torch.ones(ns, dtype=torch.bool)
    rest[big] = False
    w[:, big] = 0.25 * w[:, rest].sum(1, keepdim=True) * _uniform((B, len(big), nb, 2), seed + 1, 0.8, 1.2).double()
  return (tot[:, None] * (w / w.sum(1, keepdim=True))).float().contiguous()


def _grouped(x, groups):
  B, HW, C = x.shape
  return x.double().reshape(B, HW, groups, C // groups)


def groupnorm_ref(x, groups, gamma, beta, eps, silu):
  """fp64 (B, HW, C): GroupNorm (+ SiLU) of the (concatenated) tensor x (B, HW, C)."""
  v = _grouped(x, groups)
  mean = v.mean((1, 3), keepdim=True)
  var = (v * v).mean((1, 3), keepdim=True) - mean * mean
  y = ((v - mean) * torch.rsqrt(var + eps)).reshape(x.shape) * gamma.double() + beta.double()
  return y * torch.sigmoid(y) if silu else y


def _group_moments(x, groups):
  """fp64 per-channel (B, C) views of the group's mean, E[x^2] and E|x|."""
  v = _grouped(x, groups)
  cg = v.shape[-1]
  return tuple(m.repeat_interleave(cg, 1) for m in (v.mean((1, 3)), (v * v).mean((1, 3)), v.abs().mean((1, 3))))


def scale_shift_ref(x, groups, gamma, beta, eps):
  """fp64 (B, 2, C): what ss_out should hold — y = x * scale + shift."""
  mean, e2, _ = _group_moments(x, groups)
  scale = torch.rsqrt(e2 - mean * mean + eps) * gamma.double()
  return torch.stack([scale, beta.double() - mean * scale], 1)


def table_figure(name, table, x, groups, gamma, beta, eps):
  """The table's error in STAT_BAR's unit (module docstring); prints and returns the worst entry's figure."""
  ref = scale_shift_ref(x, groups, gamma, beta, eps)
  mean, e2, eabs = _group_moments(x, groups)
  K = e2 / (e2 - mean * mean + eps)
  sc = ref[:, 0].abs().clamp_min(1e-30)
  err = (table.double().cpu() - ref).abs()
  fig = torch.stack([err[:, 0] / (sc * 1.5 * K), err[:, 1] / (sc * (eabs + 1.5 * K * mean.abs()))], 1)
  fig = torch.where(torch.isfinite(fig), fig, torch.full_like(fig, float("inf")))
  w = int(fig.argmax())
  print(f"[{name}] table: worst entry {w} of {fig.numel()}: figure {fig.flatten()[w].item():.3e} (bar {STAT_BAR:.1e})")
  return fig.max().item()


def group_figure(name, y, ref, groups):
  """test_ops_gpu._report's figure (max abs error over max |ref|) per (sample, group), in the style of kv_cache_util.report_rows."""
  err = _grouped((y.double().cpu() - ref).abs(), groups).amax((1, 3))
  rel = err / _grouped(ref.abs(), groups).amax((1, 3)).clamp_min(1e-6)
  rel = torch.where(torch.isfinite(rel), rel, torch.full_like(rel, float("inf")))
  w = int(rel.argmax())
  print(f"[{name}] worst (sample, group) {divmod(w, groups)}: max_abs={err.flatten()[w].item():.4e} rel_to_group_max={rel.flatten()[w].item():.4e}")
  return rel.max().item()


def _tree16(v):
  """v (..., 16) -> (...): the fixed tree of the 16-partial segments."""
  p = [v[..., i] for i in range(16)]
  return (((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]))) + (((p[8] + p[9]) + (p[10] + p[11])) + ((p[12] + p[13]) + (p[14] + p[15])))


def _emulate_totals_pass(st, stop_at_512):
  """groupnorm_total_kernel: st (B, ns, nb, 2) fp32 -> (B, nb, 2).  Slice q adds slabs q, q + 64, ... on eight accumulators (a trip of
  the loop takes 512 slabs), the accumulators on a tree, the 64 slices folded pairwise, halving."""
  B, ns, nb, _ = st.shape
  trips = 1 if stop_at_512 else (ns + 511) // 512
  pad = torch.zeros((B, trips * 512, nb, 2))
  n = min(ns, trips * 512)
  pad[:, :n] = st[:, :n]
  v = pad.reshape(B, trips, 8, 64, nb, 2)
  a = torch.zeros((B, 8, 64, nb, 2))
  for t in range(trips):
    a = a + v[:, t]
  part = ((a[:, 0] + a[:, 1]) + (a[:, 2] + a[:, 3])) + ((a[:, 4] + a[:, 5]) + (a[:, 6] + a[:, 7]))       # (B, 64, nb, 2)
  h = 32
  while h >= 1:
    part = part[:, :h] + part[:, h:2 * h]
    h //= 2
  return part[:, 0]


def _emulate_block_totals(st):
  """Phase 0 of groupnorm_apply_kernel: st (B, ns <= 64, nb, 2) fp32 -> (B, nb, 2)."""
  B, ns, nb, _ = st.shape
  pad = torch.zeros((B, 64, nb, 2))
  pad[:, :ns] = st
  seg = _tree16(pad.reshape(B, 4, 16, nb, 2).permute(0, 1, 3, 4, 2))      # (B, 4, nb, 2)
  return (seg[:, 0] + seg[:, 1]) + (seg[:, 2] + seg[:, 3])


def consumer_defect_applies(defect, C1, bin1, C2, bin2, ns1, ns2, groups=GROUPS):
  cg = (C1 + C2) // groups
  return {"dropped_last_partial": True, "dropped_partial_16": max(ns1, ns2) > 16, "partials_of_other_sample": True, "bin_off_by_one": True,
          "block2_offset_ignored": C2 > 0, "straddling_group_takes_block1_only": C2 > 0 and C1 % cg != 0,
          "totals_stop_at_512": max(ns1, ns2) > 512, "block2_totals_at_block1_offset": C2 > 0 and ns2 > 64}[defect]


def emulate_apply(x1, st1, bin1, gamma, beta, groups, eps, silu, x2=None, st2=None, bin2=0, defect=None):
  """fp32 restatement of groupnorm_apply_launch on x1 (B, HW, C1) [++ x2] with partials st1 (B, ns1, C1 / bin1, 2) [, st2].  Returns
  (y (B, HW, C) fp32 holding bf16 values, table (B, 2, C) fp32).  defect: one of CONSUMER_DEFECTS (reads past a block's bins give zeros)."""
  B, HW, C1 = x1.shape
  C2 = 0 if x2 is None else x2.shape[-1]
  C = C1 + C2
  cg = C // groups
  blocks = [st1.float()] + ([st2.float()] if C2 else [])
  if defect == "dropped_last_partial":
    blocks = [s[:, :-1] if s.shape[1] > 1 else torch.zeros_like(s) for s in blocks]
  if defect == "dropped_partial_16":
    blocks = [torch.cat([s[:, :16], s[:, 17:]], 1) if s.shape[1] > 16 else s for s in blocks]
  if defect == "partials_of_other_sample":
    blocks = [torch.roll(s, -1, 0) for s in blocks]
  nbs = [s.shape[2] for s in blocks]
  scratch = torch.zeros(B * sum(nbs) * 2)       # the totals scratch: block 1 at 0, block 2 after B * nb1 bins
  tots = []
  for k, s in enumerate(blocks):
    if s.shape[1] > 64:
      t = _emulate_totals_pass(s, defect == "totals_stop_at_512")
      off = 0 if k == 0 else B * nbs[0] * 2
      scratch[off:off + t.numel()] = t.flatten()
      if k == 1 and defect == "block2_totals_at_block1_offset":
        off = 0
      t = scratch[off:off + t.numel()].reshape(t.shape).clone()
      tots.append(_emulate_block_totals(t[:, None]))
    else:
      tots.append(_emulate_block_totals(s))
  if defect == "bin_off_by_one":
    tots = [torch.cat([t[:, 1:], torch.zeros_like(t[:, :1])], 1) for t in tots]
  r1, r2 = cg // bin1, (cg // bin2 if C2 else 0)
  o2 = 0 if (not C2 or defect == "block2_offset_ignored") else C1 // bin2
  a, q = torch.zeros(B, groups), torch.zeros(B, groups)
  for g in range(groups):
    ga, gq = torch.zeros(B), torch.zeros(B)
    e1 = min((g + 1) * r1, nbs[0])
    for b_ in range(g * r1, e1):
      ga, gq = ga + tots[0][:, b_, 0], gq + tots[0][:, b_, 1]
    if C2 and not (defect == "straddling_group_takes_block1_only" and g * r1 < e1):
      for b_ in range(max(g * r2 - o2, 0), g * r2 - o2 + r2):
        if b_ < nbs[1]:
          ga, gq = ga + tots[1][:, b_, 0], gq + tots[1][:, b_, 1]
    a[:, g], q[:, g] = ga, gq
  inv_n = torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(float(cg), dtype=torch.float32) * torch.tensor(float(HW), dtype=torch.float32))
  sm, sq = (a * inv_n).repeat_interleave(cg, 1), (q * inv_n).repeat_interleave(cg, 1)
  var = (sq - sm * sm).clamp_min(0)
  sc = torch.rsqrt(var + torch.tensor(eps, dtype=torch.float32)) * gamma.float()
  sh = beta.float() - sm * sc
  x = x1 if x2 is None else torch.cat([x1, x2], -1)
  y = (x.double() * sc.double()[:, None] + sh.double()[:, None]).float()       # fmaf: one rounding
  if silu:
    y = F.silu(y)
  return bf(y), torch.stack([sc, sh], 1)


# ------------------------------------------------------------------------------------------------ producer side
def filing_order(y, ups=False):
  """(B, rows, C): the rows of an NHWC tensor (B, OH, OW, C) (or (B, rows, C) as it is) in the order the producers cut into slabs: row-major
  pixels, or for the four-tap upsample form the four parity classes cls = 2 (oy % 2) + (ox % 2) one after the other, each in row-major order
  of its source pixels."""
  if not ups:
    return y.reshape(y.shape[0], -1, y.shape[-1])
  B, C = y.shape[0], y.shape[-1]
  return torch.cat([y[:, py::2, px::2].reshape(B, -1, C) for py in (0, 1) for px in (0, 1)], 1)


def partials_ref(y, slab_rows, bin, ups=False, defect=None, unrounded=None, resid=None):
  """fp64 ((B, nslab, C / bin, 2) {sum, sum of squares}, the same shape {sum |v|, sum v^2}: partials_figure's denominators) of the bf16
  tensor y per (sample, slab of slab_rows rows in filing_order, bin).  defect: one of PRODUCER_DEFECTS — slab_shifted_one rolls the (sample,
  slab) axis (the last slab of a sample lands in the next sample), sums_of_unrounded_values sums `unrounded` (the fp32 values y was rounded
  from), residual_left_out sums y - resid."""
  v = y.double()
  if defect == "sums_of_unrounded_values":
    v = unrounded.double()
  if defect == "residual_left_out":
    v = v - resid.double()
  def sums(t):      # noqa: E306
    t = filing_order(t, ups)
    B, rows, C = t.shape
    t = t.reshape(B, rows // slab_rows, slab_rows, C // bin, bin)
    return torch.stack([t.sum((2, 4)), (t * t).sum((2, 4))], -1), torch.stack([t.abs().sum((2, 4)), (t * t).sum((2, 4))], -1)
  s = sums(v)[0]
  if defect == "slab_shifted_one":
    s = torch.roll(s.flatten(0, 1), 1, 0).reshape(s.shape)
  if defect == "bin_shifted_one":
    s = torch.roll(s, 1, 2)
  return s, sums(y.double())[1]


def emulate_partials(y, slab_rows, bin, ups=False):
  """fp32 (B, nslab, C / bin, 2): the sums the way a producer forms them in fp32 — per column over the slab's rows, then over the bin's
  columns, each a chain of additions in index order (the kernels use trees over the row lanes: chains err no less)."""
  t = filing_order(y.float(), ups)
  B, rows, C = t.shape
  t = t.reshape(B, rows // slab_rows, slab_rows, C // bin, bin)
  out = []
  for m in (t, t * t):
    col = torch.zeros(B, rows // slab_rows, C // bin, bin)
    for r in range(slab_rows):
      col = col + m[:, :, r]
    acc = torch.zeros(B, rows // slab_rows, C // bin)
    for c in range(bin):
      acc = acc + col[..., c]
    out.append(acc)
  return torch.stack(out, -1)


def partials_figure(name, got, ref, denom):
  """max over partials and moments of |got - ref| / {sum |v|, sum v^2}; prints the worst partial."""
  fig = (got.double().cpu() - ref).abs() / denom.clamp_min(1e-30)
  fig = torch.where(torch.isfinite(fig), fig, torch.full_like(fig, float("inf")))
  w = int(fig.argmax())
  idx = []
  for d in reversed(fig.shape):
    w, r = divmod(w, d)
    idx.append(r)
  print(f"[{name}] partials: worst (sample, slab, bin, moment) {tuple(reversed(idx))}: figure {fig.max().item():.3e} (bar {STAT_BAR:.1e})")
  return fig.max().item()


# name -> form ("conv" | "ups" | "gemm"), B, H, W, C1, C2, Cout, bin, CS (fused shortcut channels), splitk, rowvec, resid
PRODUCER_CASES = {
  "tile128_bin4": ("conv", 2, 16, 16, 64, 0, 128, 4, 0, 1, False, False),            # four-wave 128-row tile
  "tile128_bin2": ("conv", 2, 16, 16, 64, 0, 128, 2, 0, 1, False, False),
  "tile128x160_one_slab": ("conv", 2, 8, 8, 128, 0, 160, 5, 0, 1, False, False),     # one slab per sample
  "pingpong_320": ("conv", 1, 16, 16, 64, 0, 320, 5, 0, 1, False, False),            # 256 x 160 ping-pong tile
  "pingpong_640_rowvec_resid": ("conv", 4, 16, 16, 128, 0, 640, 10, 0, 1, True, True),
  "two_sources": ("conv", 2, 16, 16, 64, 64, 160, 5, 0, 1, False, False),
  "fused_shortcut": ("conv", 2, 16, 16, 128, 0, 128, 4, 64, 1, False, False),
  "splitk4_640": ("conv", 2, 8, 8, 640, 0, 640, 10, 0, 4, True, True),               # the plain split-K reducer
  "splitk2_1280": ("conv", 2, 16, 16, 640, 0, 1280, 20, 0, 2, False, False),
  "splitk2_1280_reducer64": ("conv", 8, 32, 32, 64, 0, 1280, 20, 0, 2, False, True),  # 8 x 128 reducer blocks: its 64-row instantiation
  "chain_skip_320": ("conv", 2, 8, 8, 128, 0, 320, 5, 0, 1, False, False),             # the skip tensor of the chain test: one 64-row slab per sample
  "upsample_160": ("ups", 4, 16, 16, 64, 0, 160, 5, 0, 1, False, False),             # four-tap form: H x W is the SOURCE grid
  "upsample_128": ("ups", 1, 16, 16, 64, 0, 128, 4, 0, 1, False, False),
  "gemm_conv_in": ("gemm", 2, 16, 16, 64, 0, 512, 16, 0, 1, False, False),           # M = 2 x 256, K = 64: the VAE's im2col conv_in
  "gemm_to_out_resid": ("gemm", 2, 8, 8, 512, 0, 512, 16, 0, 1, False, True),        # M = 2 x 64, K = N = 512: its attention to_out
}


@functools.lru_cache(maxsize=None)
def producer_case(name):
  """dict of the case's operands (what the kernels read as bf16 holds bf16 values) and `ref`: the fp32 output (B, OH, OW, Cout) before
  its rounding to bf16 ((B, H * W, Cout) for the plain GEMM)."""
  form, B, H, W, C1, C2, Cout, bin, CS, sk, has_rv, has_res = PRODUCER_CASES[name]
  seed = 700 + sum(ord(c) for c in name)
  Cin, HW = C1 + C2, H * W
  K = Cin if form == "gemm" else 9 * Cin
  x = bf(0.5 * _rnd((B, HW, Cin), seed) + _block_offsets(B, HW, 1, Cin, seed + 1, -2.0, 2.0))
  d = dict(form=form, B=B, H=H, W=W, bin=bin, splitk=sk, ups=form == "ups")
  bias = _block_offsets(1, 1, Cout // bin, bin, seed + 2, -2.0, 2.0)[0, 0] + 0.1 * _rnd((Cout,), seed + 3)
  d["bias"] = bias
  if form == "gemm":
    w = bf(_rnd((Cout, K), seed + 4, 0.03) + 1.0 / K)
    d.update(a=x.reshape(B * HW, Cin), w=w)
    ref = x @ w.T + bias
    OHW = HW
  else:
    w = _rnd((Cout, Cin, 3, 3), seed + 4, 0.03) + 1.0 / K
    xi = x.reshape(B, H, W, Cin)
    d.update(x1=xi[..., :C1].contiguous(), x2=xi[..., C1:].contiguous() if C2 else None, w=w)
    xn = xi.permute(0, 3, 1, 2)
    if form == "ups":
      xn = F.interpolate(xn, scale_factor=2, mode="nearest")
    ref = F.conv2d(xn, bf(w), bias, padding=1).permute(0, 2, 3, 1)
    OHW = ref.shape[1] * ref.shape[2]
    if CS:
      xs, wsc = bf(_rnd((B, H, W, CS), seed + 5)), _rnd((Cout, CS), seed + 6, 0.05)
      d.update(xs1=xs, w_sc=wsc)
      ref = ref + xs @ bf(wsc).T
  if has_rv:
    rv = _block_offsets(B, 1, Cout // bin, bin, seed + 7, -1.5, 1.5)[:, 0]
    d["rowvec"] = rv
    ref = ref + rv.reshape((B,) + (1,) * (ref.dim() - 2) + (Cout,))
  if has_res:
    res = bf(0.5 * _rnd((B, OHW, Cout), seed + 8) + _block_offsets(B, OHW, Cout // bin, bin, seed + 9, -2.0, 2.0)).reshape(ref.shape)
    d["resid"] = res
    ref = ref + res
  d["ref"] = ref.contiguous()
  d["rows"] = OHW
  return d


def producer_defect_applies(defect, name):
  return defect != "residual_left_out" or PRODUCER_CASES[name][11]


def expected_slab_rows(name):
  """csrc/gemm_plan.hip gemm_gn_slab_rows(): 64 from the epilogue; from the split-K reducer 64 where its grid (blocks of 64 rows and 160, 80 or
  64 columns) has 1024 blocks or more, else 16."""
  form, B, H, W, C1, C2, Cout, bin, CS, sk, _, _ = PRODUCER_CASES[name]
  if sk <= 1:
    return 64
  width = 64 if 64 % bin == 0 else (160 if Cout % 160 == 0 and 160 % bin == 0 else 80)
  return 64 if math.ceil(Cout / width) * math.ceil(B * H * W / 64) >= 1024 else 16


# ------------------------------------------------------------------------------------------------ the consumer cases of both test files
def one_block_cases():
  """[(C, bin, B, HW, nslab, silu, eps)]: every geometry with SiLU on and off and eps 1e-5 (the UNet's norms) and 1e-6 (the VAE's, the transformers')."""
  return [g + (silu, eps) for g in ONE_BLOCK for silu in (True, False) for eps in (1e-5, 1e-6)]


def two_block_cases():
  """[(C1, bin1, C2, bin2, B, HW, nslab1, nslab2, silu, eps)]"""
  out = []
  for geo in TWO_BLOCK:
    for HW in TWO_BLOCK_HW:
      for ns in TWO_BLOCK_NSLAB:
        i = len(out)
        out.append(geo + (2, HW) + ns + (i % 2 == 0, 1e-6 if i % 3 == 0 else 1e-5))
  return out


@functools.lru_cache(maxsize=None)
def consumer_case(C1, bin1, C2, bin2, B, HW, ns1, ns2):
  """(x1, st1, x2, st2, gamma, beta): activations, host-made partials and the norm's parameters of a consumer case (x2, st2 None when C2 == 0)."""
  seed = 900 + C1 + 3 * C2 + 5 * HW + 7 * ns1 + 11 * ns2
  x1 = consumer_acts(B, HW, C1, bin1, seed)
  st1 = host_partials(bin_totals(x1, bin1), ns1, seed + 10)
  x2 = st2 = None
  if C2:
    x2 = consumer_acts(B, HW, C2, bin2, seed + 20)
    st2 = host_partials(bin_totals(x2, bin2), ns2, seed + 30)
  return (x1, st1, x2, st2) + norm_params(C1 + C2, seed + 40)
