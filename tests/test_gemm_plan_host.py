"""The GEMM launcher's plan, on the CPU (no GPU is touched): every decision gemm_launch() makes — kernel instantiation, grid, the integers of the
kernel argument block, in-kernel finish, reducer — over ~8000 launches and four environments, against tests/golden/gemm_plans.npz.

The golden file was RECORDED FROM THE LAUNCHER BEFORE THE PLAN EXISTED (the parent commit's gemm.hip with its kernel launch, zero page and
environment getters stubbed: recipe in profiles/gemm_plan_isa.md), not from the code under test.  A pull request that moves a tile rule sees here
exactly which launches moved; it re-records the golden with the rows it means to change and says so.

  1. the case list rebuilt by gemm_plan_util equals the recorded one (the generator did not drift from the recording);
  2. gill_gemm_plan gives the recorded row for every case under every environment: (PP 1, COOP 1, 256 CUs), PP 0, COOP 0, 64 CUs;
  3. cases the old launcher refused are refused with the same return code;
  4. the accepted cases reach every gemm_kernel instantiation that any arguments can reach (56 of 63; the other seven are named below);
  5. gemm_pick_splitk / _blk64, gemm_fused_gn_ok, gemm_conv_pingpong, conv_k_chunked, gemm_stream64_weights give the recorded answers;
  6. structure: grid = tiles_m * groups_n x splitk x ncls, tile rows follow from (nwv, mi) and from the template pair, an in-kernel finish runs on
     the eight-wave 160-wide tile only, a reducer launch follows exactly the split launches that do not stop at the partials."""
import os

import numpy as np
import pytest

import gemm_plan_util as U
from gill_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "gemm_plans.npz"))
R = U.R

# (NWV, BN, CONV, EPI, STAGES, KT, MI) that exist in gemm.hip and that no argument set reaches (profiles/gemm_plan_isa.md, findings):
# the rules that pick the 64-row tile turn it into the four-wave form for these epilogues, the GEGLU / QKV 128-row tile is the eight-wave kernel,
# the softmax epilogue always runs mi = 2, and the QKV ping-pong rule only ever picks 256 rows
UNREACHABLE = {(2, 128, 0, 3, 2, 64, 4), (4, 128, 0, 1, 2, 64, 4), (4, 128, 0, 3, 2, 64, 4), (2, 160, 0, 4, 2, 64, 4), (2, 160, 0, 5, 2, 64, 4),
               (4, 160, 0, 5, 2, 64, 4), (8, 160, 0, 3, 3, 64, 2)}
N_INSTANTIATIONS = 63


def _table():
  q, a = GOLDEN["queries"], GOLDEN["answers"]
  return {tuple(int(v) for v in q[i]): [int(a[e, i]) for e in range(len(U.ENVS))] for i in range(len(q))}


@pytest.fixture(scope="module")
def cases():
  return U.build_cases(U.Picks(_table()))


@pytest.fixture(scope="module")
def planned(cases):
  return np.stack([ops.gemm_plan(cases, *env) for env in U.ENVS])


def test_case_list_is_the_recorded_one(cases):
  assert cases.shape == GOLDEN["cases"].shape and np.array_equal(cases, GOLDEN["cases"])
  picks = U.Picks(_table())
  U.build_cases(picks)
  assert np.array_equal(U.build_queries(picks), GOLDEN["queries"])
  rc = GOLDEN["rows"][:, :, R["rc"]]
  main = (rc == 0).all(axis=0)
  assert main.sum() >= 7500 and (~main).sum() <= 300      # the list is launches; the refusals are a short tail
  for shape in ((8192, 640, 640), (2048, 1280, 1280), (2048, 3840, 1280), (8192, 1920, 640), (8192, 640, 3200)):
    assert ((cases[:, :3] == shape).all(axis=1) & main).any(), shape
  blk = cases[:, U.CASE_FIELDS.index("w_blk64")] == 1
  assert (blk & (cases[:, 2] == 129 * 64) & main).any()


@pytest.mark.parametrize("e", range(len(U.ENVS)), ids=[f"pp{p}-coop{c}-cus{n}" for p, c, n in U.ENVS])
def test_every_decision_is_the_recorded_one(cases, planned, e):
  want, got = GOLDEN["rows"][e], planned[e]
  bad = np.flatnonzero((want != got).any(axis=1))
  msg = ""
  for i in bad[:10]:
    cols = np.flatnonzero(want[i] != got[i])
    msg += f"\n  case {i} {dict(zip(U.CASE_FIELDS, cases[i].tolist()))}: " + ", ".join(
        f"{U.ROW_FIELDS[c]} {want[i, c]} -> {got[i, c]}" for c in cols)
  assert len(bad) == 0, f"{len(bad)} of {len(cases)} launches moved under (pp, coop, cus) = {U.ENVS[e]}:{msg}"


def test_refusals_keep_their_return_code(planned):
  want = GOLDEN["rows"][:, :, R["rc"]]
  assert (want != 0).any() and np.array_equal(planned[:, :, R["rc"]], want)
  refused = planned[want != 0]
  assert (refused[:, 1:] == 0).all(), "a refused launch has no plan"


def test_every_reachable_instantiation_is_reached(planned):
  ok = planned[planned[:, :, R["rc"]] == 0]
  reached = {tuple(int(v) for v in r) for r in np.unique(ok[:, R["k_nwv"]:R["k_mi"] + 1], axis=0)}
  assert not (reached & UNREACHABLE)
  assert len(reached) == N_INSTANTIATIONS - len(UNREACHABLE), sorted(reached)


@pytest.mark.parametrize("e", range(len(U.ENVS)), ids=[f"pp{p}-coop{c}-cus{n}" for p, c, n in U.ENVS])
def test_engine_queries_are_the_recorded_ones(e):
  q = GOLDEN["queries"]
  got = ops.gemm_query(q, *U.ENVS[e])
  bad = np.flatnonzero(got != GOLDEN["answers"][e])
  assert len(bad) == 0, [(q[i].tolist(), int(GOLDEN["answers"][e][i]), int(got[i])) for i in bad[:10]]
  assert {int(w) for w in q[:, 0]} == set(range(6))


def test_plan_structure(cases, planned):
  for e in range(len(U.ENVS)):
    p = planned[e][planned[e][:, R["rc"]] == 0]
    c = cases[planned[e][:, R["rc"]] == 0]
    col = lambda n: p[:, R[n]]      # noqa: E731
    assert np.array_equal(col("grid_x"), col("tiles_m") * col("groups_n"))
    assert np.array_equal(col("grid_y"), col("splitk")) and np.array_equal(col("grid_z"), col("ncls"))
    assert np.array_equal(col("tile_rows"), (col("nwv") // 2) * col("mi") * 16)
    assert np.array_equal(col("tile_rows"), (col("k_nwv") // 2) * col("k_mi") * 16), "the kernel's tile is the tile the grid was sized with"
    assert np.array_equal(col("tiles_m"), -(-col("M") // col("tile_rows")))
    assert np.array_equal(col("groups_n"), -(-col("tiles_n") // col("npw")))
    assert np.array_equal(col("ksteps_per_split"), -(-col("ksteps") // col("splitk")))
    assert (col("kt") == 64).all() and (col("k_kt") == 64).all()
    coop = col("coop") == 1
    assert (p[coop][:, R["k_nwv"]:R["k_epi"] + 1] == (8, 160, 1, 6)).all() and ((col("k_epi") == 6) == coop).all()
    assert (col("splitk")[coop] == 1).all() and (col("grid_x")[coop] <= U.ENVS[e][2]).all()
    assert coop.any() == (U.ENVS[e][1] != 0 and U.ENVS[e][0] != 0)      # (the finish lives on the ping-pong convolution tiles)
    partials_only = c[:, U.CASE_FIELDS.index("partials_only")] == 1
    assert np.array_equal(col("reduce") == 1, (col("splitk") > 1) & ~partials_only)
    assert np.array_equal(col("reduce_M"), np.where(col("reduce") == 1, c[:, 0], 0))
    assert ((col("k_epi") == 2) == (col("splitk") > 1)).all()
    assert (col("npw")[col("nwv") == 8] == 1).all()
