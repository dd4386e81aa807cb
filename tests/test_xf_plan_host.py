"""Which kernels a UNet transformer block runs, on the CPU (no GPU is touched): gill_unet_xf_plan against a literal table.

The table was worked out BY HAND FROM THE RULES OF THE COMMIT BEFORE xf_plan.h EXISTED (4dc5c56, gill_amd/csrc/unet.hip), not by running the code under
test.  Each row cites the rules it follows from:

  load time, Loader::xf (lines 260-286 there), H heads of padded dim dp, hdp = H * dp:
    L1  fp8 GEGLU rows:      f8 && C % 128 == 0 && !(ffn_fused_on() && ffn_fused_supported(C, 128))
    L2  XALG operands:       xalg_on() && H % 2 == 0 && ctx_len <= 80 && 80 * H <= hdp && dp <= 160 && C % 64 == 0 && ctx_dim % 64 == 0 && hw % 64 == 0
    L3  fused feed-forward:  ffn_fused_on() && ffn_fused_supported(C, 128)          (ffn.hip: C == 320 && M % 128 == 0 && M > 0)
    L4  ... its PRE form:    wpp allocated where hdp == 384
    L5  projection pairs:    lnproj_on() && lnproj_supported(C, 128, H, dp)         (lnproj.hip: C == 320 && M % 128 == 0 && M > 0 && H == 8 && dp == 48)
  run time, UNetRun::xf (lines 619-756 there), M = Bx * HW of the full batch:
    R1  ffn_fused = w1c && ffn_fused_supported(C, M) && HW % 128 == 0
    R2  lnproj = wqkv1p && !shared && lnproj_supported(C, M, H, dp) && HW % 32 == 0
    R3  table: lnproj && HW % 128 == 0                                              (also xf_wants_table(), line 609)
    R4  cross-attention: lnproj -> attention kernel; else xg ? two GEMMs : attention kernel
    R5  ffn_pre = ffn_fused && wpp (the attention-kernel branch only)
    R6  t8 / fp8 GEGLU where wff1_8, on the GEMM feed-forward only (the fused kernel returns first)
    R7  M1 = Bpre * HW, Bpre = Bx / 2 on the shared prefix
  padded head dim (ops.h attn_padded_dim): d <= 48 -> 48, <= 64 -> 64, <= 80 -> 80, <= 128 -> 128, <= 160 -> 160."""
import numpy as np
import pytest

from gill_amd import ops

ATTN, XALG = 0, 1                              # plan.cross
GEMM, GEMM_FP8, FUSED, FUSED_PRE = 0, 1, 2, 3  # plan.ffn
ON = (1, 1, 1)                                 # GILL_UNET_LNPROJ, GILL_UNET_XALG, GILL_UNET_FFN_FUSED

# geometry: (C, heads, ctx_len, ctx_dim)
SD15 = [(320, 8, 77, 768), (640, 8, 77, 768), (1280, 8, 77, 768), (1280, 8, 77, 768)]           # d 40 / 80 / 160 / 160 -> dp 48 / 80 / 160 / 160
SD21 = [(320, 5, 77, 1024), (640, 10, 77, 1024), (1280, 20, 77, 1024), (1280, 20, 77, 1024)]    # d 64 -> dp 64
TINY = [(64, 4, 77, 128), (128, 4, 77, 128), (256, 4, 77, 128), (256, 4, 77, 128)]              # d 16 / 32 / 64 / 64 -> dp 48 / 48 / 64 / 64
TINY2 = [(64, 1, 77, 128), (128, 2, 77, 128), (256, 4, 77, 128), (256, 4, 77, 128)]             # d 64 -> dp 64


def hw(sample, level):
  return (sample >> level) ** 2


# (name, geometry, hw, fp8, Bx, shared, switches) -> forms (lnproj, xalg, ffn_fused, ffn_pre, geglu_fp8), plan (lnproj, gn_table, cross, ffn, M, M1)
TABLE = [
  # --- SD-1.5 at sample 64, Bx 8
  # L5 (320, 8 heads, dp 48), L2 fails 80 * 8 = 640 > 384, L3, L4 hdp 384; R2 32768 % 128 == 0, R3 4096 % 128 == 0, R4 lnproj, R1 + R5
  ("sd15-64 L0", SD15[0], 4096, 0, 8, 0, ON, (1, 0, 1, 1, 0), (1, 1, ATTN, FUSED_PRE, 32768, 32768)),
  # L5 / L3 fail C != 320; L2: 640 <= 640, dp 80, 1024 % 64 == 0; R4 xg; R1 no w1c
  ("sd15-64 L1", SD15[1], 1024, 0, 8, 0, ON, (0, 1, 0, 0, 0), (0, 0, XALG, GEMM, 8192, 8192)),
  # L2: 640 <= 1280, dp 160 <= 160, 256 % 64 == 0
  ("sd15-64 L2", SD15[2], 256, 0, 8, 0, ON, (0, 1, 0, 0, 0), (0, 0, XALG, GEMM, 2048, 2048)),
  # L2: 64 % 64 == 0 (level 3 has no transformer block in the down / up path: this is the mid block's geometry)
  ("sd15-64 L3/mid", SD15[3], 64, 0, 8, 0, ON, (0, 1, 0, 0, 0), (0, 0, XALG, GEMM, 512, 512)),
  # the first down block of a CFG pair: forms as L0; R2 !shared fails, so R3 fails; R1 on the full M still holds, R5; R7 M1 = 4 * 4096
  ("sd15-64 L0 shared", SD15[0], 4096, 0, 8, 1, ON, (1, 0, 1, 1, 0), (0, 0, ATTN, FUSED_PRE, 32768, 16384)),
  # R2 / R1 at Bx 1: 4096 % 128 == 0
  ("sd15-64 L0 Bx1", SD15[0], 4096, 0, 1, 0, ON, (1, 0, 1, 1, 0), (1, 1, ATTN, FUSED_PRE, 4096, 4096)),
  # --- fp8 on
  # L1: 320 % 128 != 0 (and L3 holds)
  ("sd15-64 L0 fp8", SD15[0], 4096, 1, 8, 0, ON, (1, 0, 1, 1, 0), (1, 1, ATTN, FUSED_PRE, 32768, 32768)),
  # L1: 640 % 128 == 0, L3 fails; R6
  ("sd15-64 L1 fp8", SD15[1], 1024, 1, 8, 0, ON, (0, 1, 0, 0, 1), (0, 0, XALG, GEMM_FP8, 8192, 8192)),
  ("sd15-64 L2 fp8", SD15[2], 256, 1, 8, 0, ON, (0, 1, 0, 0, 1), (0, 0, XALG, GEMM_FP8, 2048, 2048)),   # L1: 1280 % 128 == 0; R6
  ("sd15-64 L3/mid fp8", SD15[3], 64, 1, 8, 0, ON, (0, 1, 0, 0, 1), (0, 0, XALG, GEMM_FP8, 512, 512)),   # as L2
  # --- GILL_UNET_LNPROJ=0: L5 fails -> R2 fails (no wqkv1p); the rest of L0 stands.  Levels 1-3 never had it
  ("sd15-64 L0 lnproj=0", SD15[0], 4096, 0, 8, 0, (0, 1, 1), (0, 0, 1, 1, 0), (0, 0, ATTN, FUSED_PRE, 32768, 32768)),
  ("sd15-64 L1 lnproj=0", SD15[1], 1024, 0, 8, 0, (0, 1, 1), (0, 1, 0, 0, 0), (0, 0, XALG, GEMM, 8192, 8192)),
  # --- GILL_UNET_XALG=0: L2 fails -> R4 attention kernel on levels 1-3; L0 never had it
  ("sd15-64 L0 xalg=0", SD15[0], 4096, 0, 8, 0, (1, 0, 1), (1, 0, 1, 1, 0), (1, 1, ATTN, FUSED_PRE, 32768, 32768)),
  ("sd15-64 L1 xalg=0", SD15[1], 1024, 0, 8, 0, (1, 0, 1), (0, 0, 0, 0, 0), (0, 0, ATTN, GEMM, 8192, 8192)),
  ("sd15-64 L2 xalg=0", SD15[2], 256, 0, 8, 0, (1, 0, 1), (0, 0, 0, 0, 0), (0, 0, ATTN, GEMM, 2048, 2048)),
  ("sd15-64 L3/mid xalg=0", SD15[3], 64, 0, 8, 0, (1, 0, 1), (0, 0, 0, 0, 0), (0, 0, ATTN, GEMM, 512, 512)),
  # --- GILL_UNET_FFN_FUSED=0: L3 fails -> no w1c, no wpp (L4 sits inside L3's branch) -> R1 fails; the projection pairs stand
  ("sd15-64 L0 ffn=0", SD15[0], 4096, 0, 8, 0, (1, 1, 0), (1, 0, 0, 0, 0), (1, 1, ATTN, GEMM, 32768, 32768)),
  ("sd15-64 L0 ffn=0 shared", SD15[0], 4096, 0, 8, 1, (1, 1, 0), (1, 0, 0, 0, 0), (0, 0, ATTN, GEMM, 32768, 16384)),
  # L1 with the fused kernel off: still 320 % 128 != 0
  ("sd15-64 L0 ffn=0 fp8", SD15[0], 4096, 1, 8, 0, (1, 1, 0), (1, 0, 0, 0, 0), (1, 1, ATTN, GEMM, 32768, 32768)),
  ("sd15-64 L1 ffn=0", SD15[1], 1024, 0, 8, 0, (1, 1, 0), (0, 1, 0, 0, 0), (0, 0, XALG, GEMM, 8192, 8192)),
  # --- SD-1.5 at sample 32, Bx 2
  ("sd15-32 L0", SD15[0], 1024, 0, 2, 0, ON, (1, 0, 1, 1, 0), (1, 1, ATTN, FUSED_PRE, 2048, 2048)),      # R2 2048 % 128 == 0, R3 1024 % 128 == 0
  ("sd15-32 L1", SD15[1], 256, 0, 2, 0, ON, (0, 1, 0, 0, 0), (0, 0, XALG, GEMM, 512, 512)),             # L2 256 % 64 == 0
  ("sd15-32 L2", SD15[2], 64, 0, 2, 0, ON, (0, 1, 0, 0, 0), (0, 0, XALG, GEMM, 128, 128)),              # L2 64 % 64 == 0
  # L2 fails 16 % 64 != 0: the case of test_sd15_full_width_small_latents_vs_oracle
  ("sd15-32 L3/mid", SD15[3], 16, 0, 2, 0, ON, (0, 0, 0, 0, 0), (0, 0, ATTN, GEMM, 32, 32)),
  # --- SD-1.5 at sample 96, Bx 2
  ("sd15-96 L0", SD15[0], 9216, 0, 2, 0, ON, (1, 0, 1, 1, 0), (1, 1, ATTN, FUSED_PRE, 18432, 18432)),    # 9216 = 72 * 128
  ("sd15-96 L2", SD15[2], 576, 0, 2, 0, ON, (0, 1, 0, 0, 0), (0, 0, XALG, GEMM, 1152, 1152)),           # L2 576 = 9 * 64
  ("sd15-96 mid", SD15[3], 144, 0, 2, 0, ON, (0, 0, 0, 0, 0), (0, 0, ATTN, GEMM, 288, 288)),            # L2 fails 144 % 64 == 16
  # --- SD-2.1-768 (sample 96), Bx 2: L5 fails on 5 heads; L2 fails on H % 2 (level 0) and on 80 H > 64 H (levels 1-3)
  # L3 holds (C == 320), L4 fails hdp = 5 * 64 = 320; R1 18432 % 128 == 0 and 9216 % 128 == 0, R5 no wpp
  ("sd21 L0", SD21[0], 9216, 0, 2, 0, ON, (0, 0, 1, 0, 0), (0, 0, ATTN, FUSED, 18432, 18432)),
  ("sd21 L1", SD21[1], 2304, 0, 2, 0, ON, (0, 0, 0, 0, 0), (0, 0, ATTN, GEMM, 4608, 4608)),
  ("sd21 L2", SD21[2], 576, 0, 2, 0, ON, (0, 0, 0, 0, 0), (0, 0, ATTN, GEMM, 1152, 1152)),
  ("sd21 L3/mid", SD21[3], 144, 0, 2, 0, ON, (0, 0, 0, 0, 0), (0, 0, ATTN, GEMM, 288, 288)),
  ("sd21 L0 shared", SD21[0], 9216, 0, 2, 1, ON, (0, 0, 1, 0, 0), (0, 0, ATTN, FUSED, 18432, 9216)),     # R1 looks at the full M; R7
  # --- UNetConfig.tiny(16) (4 heads: L2 fails 320 > 192 / 192 / 256 / 256) and tiny_sd2(16) (1 / 2 / 4 / 4 heads of 64: H odd, 160 > 128, 320 > 256), Bx 3:
  # no C is 320 (L3, L5)
  ("tiny L0", TINY[0], 256, 0, 3, 0, ON, (0, 0, 0, 0, 0), (0, 0, ATTN, GEMM, 768, 768)),
  ("tiny L1", TINY[1], 64, 0, 3, 0, ON, (0, 0, 0, 0, 0), (0, 0, ATTN, GEMM, 192, 192)),
  ("tiny L2", TINY[2], 16, 0, 3, 0, ON, (0, 0, 0, 0, 0), (0, 0, ATTN, GEMM, 48, 48)),
  ("tiny L3/mid", TINY[3], 4, 0, 3, 0, ON, (0, 0, 0, 0, 0), (0, 0, ATTN, GEMM, 12, 12)),
  ("tiny_sd2 L0", TINY2[0], 256, 0, 3, 0, ON, (0, 0, 0, 0, 0), (0, 0, ATTN, GEMM, 768, 768)),
  ("tiny_sd2 L1", TINY2[1], 64, 0, 3, 0, ON, (0, 0, 0, 0, 0), (0, 0, ATTN, GEMM, 192, 192)),
  ("tiny_sd2 L2", TINY2[2], 16, 0, 3, 0, ON, (0, 0, 0, 0, 0), (0, 0, ATTN, GEMM, 48, 48)),
  ("tiny_sd2 L3/mid", TINY2[3], 4, 0, 3, 0, ON, (0, 0, 0, 0, 0), (0, 0, ATTN, GEMM, 12, 12)),
  # tiny with fp8: L1 holds where C % 128 == 0 (128, 256), not at 64
  ("tiny L0 fp8", TINY[0], 256, 1, 3, 0, ON, (0, 0, 0, 0, 0), (0, 0, ATTN, GEMM, 768, 768)),
  ("tiny L1 fp8", TINY[1], 64, 1, 3, 0, ON, (0, 0, 0, 0, 1), (0, 0, ATTN, GEMM_FP8, 192, 192)),
  # --- the run-time size rules on the level-0 geometry
  # sample_size 24: HW = 576 = 4 * 128 + 64 -> R2 holds (1152 % 128 == 0, 576 % 32 == 0), R3 fails: the projection pairs WITHOUT the table; R1 fails on
  # HW % 128, so the GEMM feed-forward although the PRE layouts are loaded, and (R5) attn2.to_out as its own GEMM
  ("sd15-24 L0 Bx2", SD15[0], 576, 0, 2, 0, ON, (1, 0, 1, 1, 0), (1, 0, ATTN, GEMM, 1152, 1152)),
  # ... at Bx 1: R2 fails on 576 % 128 == 64
  ("sd15-24 L0 Bx1", SD15[0], 576, 0, 1, 0, ON, (1, 0, 1, 1, 0), (0, 0, ATTN, GEMM, 576, 576)),
  # sample_size 8: HW = 64, as above (128 % 128 == 0, 64 % 32 == 0, 64 % 128 != 0)
  ("sd15-8 L0 Bx2", SD15[0], 64, 0, 2, 0, ON, (1, 0, 1, 1, 0), (1, 0, ATTN, GEMM, 128, 128)),
  # R2's HW % 32 alone: no square map of a side that is a multiple of 8 has HW % 32 != 0, so directly — 144 tokens, 8 * 144 = 9 * 128 rows
  ("L0 geometry hw144 Bx8", SD15[0], 144, 0, 8, 0, ON, (1, 0, 1, 1, 0), (0, 0, ATTN, GEMM, 1152, 1152)),
  # R1's M rule alone: HW = 128, Bx 1 -> everything holds; the shared form of a pair of it: R2 fails, R1 holds on the full 256 rows
  ("L0 geometry hw128 Bx1", SD15[0], 128, 0, 1, 0, ON, (1, 0, 1, 1, 0), (1, 1, ATTN, FUSED_PRE, 128, 128)),
  ("L0 geometry hw128 pair", SD15[0], 128, 0, 2, 1, ON, (1, 0, 1, 1, 0), (0, 0, ATTN, FUSED_PRE, 256, 128)),
  # L2's other clauses on the level-1 geometry: 81 context tokens; a context width of 32 * 25; 8 heads of 160 are fine, of 168 have no kernel at all
  ("sd15-64 L1 ctx81", (640, 8, 81, 768), 1024, 0, 8, 0, ON, (0, 0, 0, 0, 0), (0, 0, ATTN, GEMM, 8192, 8192)),
  ("sd15-64 L1 ctxdim800", (640, 8, 77, 800), 1024, 0, 8, 0, ON, (0, 0, 0, 0, 0), (0, 0, ATTN, GEMM, 8192, 8192)),
  # L2 with d = 72 -> dp 80: 80 * 8 <= 8 * 80 holds; C = 576 = 9 * 64
  ("8 heads of 72", (576, 8, 77, 768), 1024, 0, 8, 0, ON, (0, 1, 0, 0, 0), (0, 0, XALG, GEMM, 8192, 8192)),
  # L2 with d = 64 on 8 heads: 640 > 512
  ("8 heads of 64", (512, 8, 77, 768), 1024, 0, 8, 0, ON, (0, 0, 0, 0, 0), (0, 0, ATTN, GEMM, 8192, 8192)),
]


def _cases(rows):
  return np.array([[*g, hw_, fp8, bx, shared] for _, g, hw_, fp8, bx, shared, _, _, _ in rows], dtype=np.int32)


def test_table_is_the_issue_list():
  names = [r[0] for r in TABLE]
  assert len(set(names)) == len(names) and 40 <= len(names) <= 80
  assert hw(64, 0) == 4096 and hw(64, 3) == 64 and hw(32, 3) == 16 and hw(96, 3) == 144 and hw(24, 0) == 576 and hw(16, 3) == 4
  for env in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
    assert any(r[6] == env for r in TABLE), env


@pytest.mark.parametrize("env", sorted({r[6] for r in TABLE}), ids=lambda e: "lnproj%d-xalg%d-ffn%d" % e)
def test_every_decision_is_the_tabled_one(env):
  rows = [r for r in TABLE if r[6] == env]
  got = ops.unet_xf_plan(_cases(rows), *env)
  assert got.shape == (len(rows), 11)
  bad = [(r[0], r[7] + r[8], tuple(int(v) for v in g)) for r, g in zip(rows, got) if tuple(int(v) for v in g) != r[7] + r[8]]
  assert not bad, "\n".join("%s: want %s, got %s" % b for b in bad)


def test_forms_never_exclude_each_other():
  # what xf_plan() relies on (xf_forms_consistent): the two-GEMM cross-attention never meets the projection pairs or the PRE feed-forward, the fp8
  # GEGLU never meets the fused feed-forward — over every geometry gill_unet_create accepts in this range
  cases = [(C, H, 77, 768, hw_, fp8, 2, 0) for C in range(64, 1344, 64) for H in (1, 2, 4, 5, 8, 10, 16, 20) if C % H == 0 and C // H <= 160
           for hw_ in (64, 144, 4096) for fp8 in (0, 1)]
  got = ops.unet_xf_plan(np.array(cases, dtype=np.int32))
  lnproj, xalg, fused, pre, f8 = got[:, :5].T
  assert len(cases) > 400 and xalg.any() and lnproj.any() and pre.any() and f8.any()
  assert not (xalg & (lnproj | pre)).any() and not (pre & ~fused).any() and not (f8 & fused).any()
  assert ((got[:, 5] == 0) | (lnproj == 1)).all() and ((got[:, 6] == 0) | (got[:, 5] == 1)).all()      # the plan never runs a form that was not loaded
  assert ((got[:, 8] < FUSED) | (fused == 1)).all() and ((got[:, 8] != FUSED_PRE) | (pre == 1)).all() and ((got[:, 8] != GEMM_FP8) | (f8 == 1)).all()
  assert np.array_equal(got[:, 7], xalg)


def test_bad_geometry_is_an_error():
  from gill_amd._native import GillNativeError
  for bad in ((320, 7, 77, 768, 4096, 0, 8, 0), (1280, 4, 77, 768, 64, 0, 8, 0), (320, 8, 77, 768, 4096, 0, 3, 1)):   # 7 does not divide 320; d = 320; odd pair
    with pytest.raises(GillNativeError):
      ops.unet_xf_plan(np.array([bad], dtype=np.int32))
