"""The case list of tests/test_gemm_plan_host.py: deterministic descriptors for gill_gemm_plan (include/gill_amd.h) and the queries for
gill_gemm_query.  tests/golden/gemm_plans.npz holds what the launcher BEFORE the plan refactor did with exactly this list (recipe:
profiles/gemm_plan_isa.md); the list is rebuilt here on every run and must equal the one stored beside the recording.

Split factors "as the engines pick them" come from the RECORDED gemm_pick_splitk* answers (picks), never from the library under test."""
import itertools

import numpy as np

# ---- descriptor / row layouts (include/gill_amd.h) -------------------------------------------------------------------------------------------------
CASE_FIELDS = ("M N K lda ldc ldr K1 conv IH IW OH OW Cin stride ups pad_shift KX KX1 k_chunked alpha_is_one rows_per_batch resid_f32 act out_mode "
               "heads dp ntok splitk w_blk64 partials_only gn_groups gn_cg ln_planes wb_rows fn_cg "
               "A A2 X1 X2 W bias rowvec resid C ws gn_stats row_stats ln_stats ln_colsum fn_Y fn_gamma fn_beta coop_ctr fn_ss").split()
ROW_FIELDS = ("rc k_nwv k_bn k_conv k_epi k_stages k_kt k_mi grid_x grid_y grid_z ksteps ksteps_per_split tiles_m tiles_n npw groups_n nwv mi kt "
              "n_major xb_m xb_n M rows_per_batch tile_rows ncls splitk coop reduce reduce_M row_planes gn_slab_rows coop_counters").split()
CASE_INTS, ROW_INTS = len(CASE_FIELDS), len(ROW_FIELDS)
assert (CASE_INTS, ROW_INTS) == (54, 34)
R = {n: i for i, n in enumerate(ROW_FIELDS)}

ENVS = ((1, 1, 256), (0, 1, 256), (1, 0, 256), (1, 1, 64))      # (GILL_GEMM_PP, GILL_GEMM_COOP, CUs)

ACT_NONE, ACT_RELU, ACT_GELU, ACT_SILU, ACT_GEGLU, ACT_QUICK_GELU = range(6)
OUT_BF16, OUT_F32, OUT_QKV, OUT_SOFTMAX80 = range(4)
Q_PICK, Q_PICK_BLK64, Q_FUSED_GN_OK, Q_CONV_PINGPONG, Q_CONV_K_CHUNKED, Q_STREAM64_WEIGHTS = range(6)


def case(**kw):
  d = dict.fromkeys(CASE_FIELDS, 0)
  d.update(stride=1, alpha_is_one=1, rows_per_batch=1, ln_planes=1, splitk=1, A=1, W=1, C=1)
  d.update(kw)
  d.setdefault("lda", 0)
  if not d["conv"]:
    d["lda"] = d["lda"] or d["K"]
    d["K1"] = d["K1"] or d["K"]
  else:
    d["K1"] = d["K1"] or d["Cin"]
  d["ldc"] = d["ldc"] or d["N"]
  if d["resid"]:
    d["ldr"] = d["ldr"] or d["N"]
  if d["splitk"] > 1:
    d["ws"] = 1
  return tuple(int(d[f]) for f in CASE_FIELDS)


def plain(M, N, K, **kw):
  return case(M=M, N=N, K=K, **kw)


def qkv(M, N, K, heads=8, ntok=64, **kw):
  dp = N // heads if (N // heads) % 8 == 0 else 16
  return case(M=M, N=N, K=K, out_mode=OUT_QKV, heads=heads, dp=dp, ntok=ntok, C=0, bias=1, **kw)


def conv(B, IH, Cin, Cout, stride=1, ups=0, **kw):
  OH = IH * 2 if ups else IH // stride
  K = (4 if ups == 2 else 9) * Cin + kw.get("KX", 0)
  return case(M=B * OH * OH, N=Cout, K=K, conv=1, IH=IH, IW=IH, OH=OH, OW=OH, Cin=Cin, stride=stride, ups=ups, rows_per_batch=OH * OH, bias=1, **kw)


class Picks:
  """gemm_pick_splitk / gemm_pick_splitk_blk64 as recorded under PP = 1 and PP = 0.  Built without a table it only collects the questions."""

  def __init__(self, table=None):
    self.table, self.asked = table, {}

  def _ask(self, q):
    q = tuple(q) + (0,) * (7 - len(q))
    self.asked[q] = True
    return sorted(set(self.table[q])) if self.table is not None else [1]

  def pick(self, M, N, K, act=ACT_NONE, plain=False, generic=False):
    return self._ask((Q_PICK, M, N, K, act, int(plain), int(generic)))

  def blk64(self, M, N, K):
    return self._ask((Q_PICK_BLK64, M, N, K))


def with_split(c, s):
  d = dict(zip(CASE_FIELDS, c))
  d["splitk"] = s
  d["ws"] = 1 if s > 1 else d["ws"]
  return tuple(d[f] for f in CASE_FIELDS)


def build_cases(picks):
  out = []

  def add(c, splits=(1,)):
    for s in splits:
      out.append(with_split(c, s))

  # ---- shapes the launcher's comments name
  for M, N, K in ((8192, 640, 640), (2048, 1280, 1280), (8192, 640, 3200)):
    add(plain(M, N, K, bias=1, resid=1), picks.pick(M, N, K, plain=True) + [1, 2])
  for M, N, K in ((2048, 3840, 1280), (8192, 1920, 640)):
    add(qkv(M, N, K, ln_stats=1, ln_colsum=1, ln_planes=4), picks.pick(M, N, K, plain=True) + [1])
  for M in (1, 8, 128, 256):      # K = 129 x 64: the STREAM64 split without an empty trailing slice
    add(plain(M, 4096, 129 * 64, w_blk64=1, bias=1), picks.blk64(M, 4096, 129 * 64) + [1, 16])

  # ---- SD-1.5 UNet at UNet batch 2, 8, 16
  levels = ((64, 320), (32, 640), (16, 1280), (8, 1280))
  res_io = {320: ((320, 320), (640, 320), (960, 320)), 640: ((320, 640), (640, 640), (960, 640), (1280, 640), (1920, 640)),
            1280: ((640, 1280), (1280, 1280), (1920, 1280), (2560, 1280))}
  for B in (2, 8, 16):
    for li, (H, C) in enumerate(levels):
      M = B * H * H
      for cin, cout in res_io[C]:
        sk = picks.pick(M, cout, 9 * cin) + [1]
        two = dict(A2=1, K1=cin - cout) if cin > cout else {}
        for src in ({}, two) if two else ({},):
          add(conv(B, H, cin, cout, rowvec=1, **src), sk)
          for cg in (cout // 64, cout // 32):
            add(conv(B, H, cin, cout, rowvec=1, gn_stats=1, gn_cg=cg, gn_groups=cout // cg, **src), sk)
            # the consuming GroupNorm finished by the launch (COOP) or by the split-K reducer: Y or the scale / shift table, raw tensor kept or not
            fn = dict(gn_stats=1, gn_cg=cg, gn_groups=cout // cg, fn_gamma=1, fn_beta=1, fn_cg=cout // 32, coop_ctr=1)
            if li < 2:
              add(conv(B, H, cin, cout, rowvec=1, fn_Y=1, **fn, **src))
              add(conv(B, H, cin, cout, rowvec=1, fn_Y=1, C=0, **fn, **src))
              add(conv(B, H, cin, cout, rowvec=1, fn_ss=1, **fn, **src))
            else:
              add(conv(B, H, cin, cout, rowvec=1, fn_Y=1, **fn, **src), [s for s in sk if s > 1])
              fn0 = dict(fn, gn_stats=0, gn_cg=0, gn_groups=0)
              add(conv(B, H, cin, cout, rowvec=1, fn_Y=1, C=0, **fn0, **src), [s for s in sk if s > 1])
        # conv2 with the fused 1x1 shortcut segment over the block's raw input (one or two sources)
        if cin != cout:
          kx = dict(KX=cin, KX1=cin, X1=1) if not two else dict(KX=cin, KX1=two["K1"], X1=1, X2=1)
          skx = picks.pick(M, cout, 9 * cout + cin) + [1]
          add(conv(B, H, cout, cout, **kx), skx)
          add(conv(B, H, cout, cout, gn_stats=1, gn_cg=cout // 32, gn_groups=32, **kx), skx)
      if li < 3:      # downsample (stride 2) out of this level, upsample (9-tap gather and the 4-tap parity form) into it
        Mo = B * (H // 2) ** 2
        add(conv(B, H, C, C, stride=2), picks.pick(Mo, C, 9 * C) + [1])
        add(conv(B, H, C, C, stride=2, gn_stats=1, gn_cg=C // 32, gn_groups=32), picks.pick(Mo, C, 9 * C) + [1])
        Cu = levels[li + 1][1]
        for ups in (1, 2):
          Ku = (9 if ups == 1 else 4) * Cu
          sku = picks.pick(M, Cu, Ku) + [1]
          add(conv(B, H // 2, Cu, Cu, ups=ups), sku)
          add(conv(B, H // 2, Cu, Cu, ups=ups, gn_stats=1, gn_cg=Cu // 32, gn_groups=32), sku)
      # transformer block GEMMs of this level
      if li < 3:
        heads, d = 8, C // 8
        dp = 48 if d <= 48 else d
        ln = dict(ln_stats=1, ln_colsum=1, ln_planes=2 * -(-C // 160), bias=1)
        add(plain(M, 8 * C, C, act=ACT_GEGLU, **ln))
        add(plain(M, 8 * C, C, act=ACT_GEGLU, bias=1))
        for nseg in (1, 3):
          for fold in (ln, {}):
            add(case(M=M, N=nseg * heads * dp, K=C, out_mode=OUT_QKV, heads=heads, dp=dp, ntok=H * H, C=0, **fold),
                picks.pick(M, nseg * heads * dp, C, plain=True) + [1])
        for wb in (64, 256, 1024, 4096):
          if M % wb == 0:
            add(plain(M, 640, C, out_mode=OUT_SOFTMAX80, wb_rows=wb, **ln))
            add(plain(M, C, 640, wb_rows=wb, resid=1, row_stats=1))      # the values GEMM on the same per-sample operands
        for K in (C, 4 * C, 5 * C):      # proj_in / to_out / ff out (+ proj_out folded in: K = 5 C from two sources)
          two = dict(A2=1, K1=4 * C) if K == 5 * C else {}
          sk = picks.pick(M, C, K, plain=True) + [1]
          add(plain(M, C, K, bias=1, resid=1, **two), sk)
          add(plain(M, C, K, bias=1, resid=1, row_stats=1, **two), sk)
          add(plain(M, C, K, bias=1, resid=1, gn_stats=1, gn_cg=C // 32, gn_groups=32, rows_per_batch=H * H, **two), sk)
          add(plain(M, C, K, bias=1, resid=1, gn_stats=1, gn_cg=C // 64, gn_groups=64, rows_per_batch=H * H, **two), sk)
    add(plain(B, 1280, 320, act=ACT_SILU, bias=1))      # time embedding
    add(plain(B, 1280, 1280, bias=1), picks.pick(B, 1280, 1280, plain=True) + [1])

  # ---- VAE decoder: 128 / 256 / 512-channel convs, im2col conv_in, the mid block's attention chain
  for H, cin, cout in ((64, 512, 512), (128, 512, 512), (256, 512, 256), (256, 256, 256), (512, 256, 128), (512, 128, 128)):
    sk = picks.pick(H * H, cout, 9 * cin) + [1]
    add(conv(1, H, cin, cout), sk)
    add(conv(1, H, cin, cout, resid=1, gn_stats=1, gn_cg=cout // 32, gn_groups=32), sk)
    if cin != cout:
      add(conv(1, H, cout, cout, KX=cin, KX1=cin, X1=1), picks.pick(H * H, cout, 9 * cout + cin) + [1])
  for H, C in ((64, 512), (128, 512), (256, 256)):
    for ups in (1, 2):
      add(conv(1, H, C, C, ups=ups), picks.pick(4 * H * H, C, (9 if ups == 1 else 4) * C) + [1])
  add(plain(4096, 512, 64, bias=1, gn_stats=1, gn_cg=16, gn_groups=32, rows_per_batch=4096))      # conv_in as im2col
  add(plain(4096, 512, 64, bias=1))
  add(case(M=4096, N=1536, K=512, out_mode=OUT_QKV, heads=1, dp=512, ntok=4096, C=0, bias=1), picks.pick(4096, 1536, 512, plain=True) + [1])
  add(plain(4096, 4096, 512), picks.pick(4096, 4096, 512, plain=True) + [1])
  add(plain(4096, 512, 4096), picks.pick(4096, 512, 4096, plain=True) + [1])
  add(plain(4096, 512, 512, bias=1, resid=1, gn_stats=1, gn_cg=16, gn_groups=32, rows_per_batch=4096), picks.pick(4096, 512, 512, plain=True) + [1])

  # ---- one sample: in-kernel finishes whose grids fit a 64-CU device too
  for H, C in ((64, 320), (32, 640)):
    fn = dict(gn_stats=1, gn_cg=C // 32, gn_groups=32, fn_gamma=1, fn_beta=1, fn_cg=C // 32, coop_ctr=1)
    add(conv(1, H, C, C, rowvec=1, fn_Y=1, **fn))
    add(conv(1, H, C, C, rowvec=1, fn_ss=1, **fn))
  # ---- small grids: every epilogue on the 64-row tiles, and the upsample convolutions of a 128-wide tile under a split
  for M in (128, 256, 512):
    add(plain(M, 2560, 320, act=ACT_GEGLU, bias=1))
    add(plain(M, 512, 512, act=ACT_SILU, bias=1, gn_stats=1, gn_cg=16, gn_groups=32, rows_per_batch=64))
    add(plain(M, 320, 320, act=ACT_SILU, bias=1))
    add(plain(M, 320, 320, bias=1, resid=1, resid_f32=1))
    add(plain(M, 320, 320, bias=1, out_mode=OUT_F32))
  for ups in (1, 2):
    add(conv(1, 64, 512, 512, ups=ups), [2, 4])
    add(conv(1, 128, 256, 256, ups=ups), [2, 4])

  # ---- OPT-125m / OPT-6.7b, CLIP, mapper: blocked (STREAM64 layout) where the engines block the matrix, and row-major
  mats = [(D, F) for D, F in ((768, 3072), (4096, 16384))]
  for D, F in mats:
    for M in (1, 8, 77, 256, 257, 2048):
      for N, K, kw in ((3 * D, D, dict(out_mode=OUT_QKV, heads=D // 64, dp=64, ntok=max(M // 1, 1), C=0, bias=1)), (D, D, dict(bias=1, resid=1)),
                       (F, D, dict(bias=1, act=ACT_RELU)), (D, F, dict(bias=1, resid=1)), (D, D, dict(bias=1, out_mode=OUT_F32, resid=1, resid_f32=1))):
        add(plain(M, N, K, **kw), picks.pick(M, N, K, plain=True) + [1])
        add(plain(M, N, K, partials_only=1, **kw), [s for s in picks.pick(M, N, K, plain=True) if s > 1])
        add(plain(M, N, K, w_blk64=1, **kw), picks.blk64(M, N, K) + [1])
        add(plain(M, N, K, w_blk64=1, partials_only=1, **kw), [s for s in picks.blk64(M, N, K) if s > 1])
  for M in (257, 2 * 257, 77, 8 * 77):      # CLIP vision (1024 / 4096), CLIP text and mapper (768 / 3072 / 512)
    for N, K, kw in ((3072, 1024, dict(out_mode=OUT_QKV, heads=16, dp=64, ntok=257, C=0, bias=1)), (4096, 1024, dict(bias=1, act=ACT_QUICK_GELU)),
                     (1024, 4096, dict(bias=1, resid=1)), (2304, 768, dict(out_mode=OUT_QKV, heads=12, dp=64, ntok=77, C=0, bias=1)),
                     (3072, 768, dict(bias=1, act=ACT_QUICK_GELU)), (768, 3072, dict(bias=1, resid=1)), (512, 768, dict(bias=1)),
                     (2048, 512, dict(bias=1, act=ACT_RELU)), (768, 4096, dict(bias=1))):
      add(plain(M, N, K, **kw), picks.pick(M, N, K, plain=True) + [1])

  # ---- the plain cross product, as plain GEMM, QKV scatter and 3x3 convolution (K = input channels), splits given and picked
  Ms, Ns = (64, 128, 192, 256, 512, 2048, 8192, 16384), (128, 256, 320, 640, 1280, 1920, 2560, 3840, 5120, 10240)
  Ks = (64, 320, 640, 1280, 2560, 5120)
  flags = tuple(itertools.product((False, True), repeat=2))
  for M, N, K in itertools.product(Ms, Ns, Ks):
    if K % 64:
      continue
    given = [1, 2, 4, 16]
    add(plain(M, N, K, bias=1), sorted(set(given + [s for p, g in flags for s in picks.pick(M, N, K, ACT_NONE, p, g)])))
    add(qkv(M, N, K), sorted(set(given + [s for p, g in flags for s in picks.pick(M, N, K, ACT_NONE, p, g)])))
    add(case(M=M, N=N, K=9 * K, conv=1, IH=8, IW=8, OH=8, OW=8, Cin=K, rows_per_batch=64, bias=1),
        sorted(set(given + [s for p, g in flags for s in picks.pick(M, N, 9 * K, ACT_NONE, p, g)])))
  seen, uniq = set(), []
  for c in out:
    if c not in seen:
      seen.add(c)
      uniq.append(c)
  return np.asarray(uniq, dtype=np.int32).reshape(-1, CASE_INTS)


def build_queries(picks):
  """[what, six arguments] rows for gill_gemm_query: every split the case list asked for, and the engines' other pre-launch questions."""
  q = list(picks.asked)
  for N in (128, 256, 320, 512, 640, 960, 1280, 1920, 2560):
    for cg in (0, 4, 5, 8, 10, 16, 20, 30, 40, 64, 80, 160):
      q.append((Q_FUSED_GN_OK, N, cg, 0, 0, 0, 0))
  for rows in (64, 256, 1024, 4096, 4100, 9216, 65536):
    for C in (128, 320, 512, 640, 1280):
      q.append((Q_CONV_PINGPONG, rows, C, 0, 0, 0, 0))
      for cin in (128, 320, 640, 960, 1920):
        q.append((Q_CONV_K_CHUNKED, rows, cin, C, 0, 0, 0))
  for N in (768, 2304, 3072, 4096, 12288, 16384, 50272):
    for K in (768, 1000, 1024, 3072, 4096, 16384):
      q.append((Q_STREAM64_WEIGHTS, N, K, 0, 0, 0, 0))
  for M, N, K in itertools.product((1, 8, 77, 128, 256, 257), (768, 4096, 16384, 50304), (1024, 4096, 129 * 64, 16384)):
    q.append((Q_PICK_BLK64, M, N, K, 0, 0, 0))
  q.append((Q_PICK, 8192, 2560, 320, ACT_GEGLU, 1, 0))
  seen, uniq = set(), []
  for r in q:
    if r not in seen:
      seen.add(r)
      uniq.append(r)
  return np.asarray(uniq, dtype=np.int32).reshape(-1, 7)
