"""The fused GroupNorm statistics on their own: what the producers of csrc/gemm.hip file through GemmArgs::gn_stats, and what
groupnorm_apply_launch (csrc/norm.hip) makes of partials — references, inputs, defects and bars in gn_stats_util.py; test_gn_stats_host.py shows
on the CPU that each check below fails for every defect of its lists."""
import pytest
import torch
import torch.nn.functional as F

import gn_stats_util as U

pytestmark = pytest.mark.gpu


def _dev(t, cuda, bf16=False):
  if t is None:
    return None
  return (t.bfloat16() if bf16 else t).to(cuda)


def _run_producer(name, cuda):
  from gill_amd import ops
  c = U.producer_case(name)
  if c["form"] == "gemm":
    return ops.gemm_gn_stats(_dev(c["a"], cuda, True), _dev(c["w"], cuda, True), c["bin"], c["rows"], bias=_dev(c["bias"], cuda),
                             resid=_dev(c.get("resid"), cuda, True), splitk=c["splitk"])
  return ops.conv3x3_gn_stats(_dev(c["x1"], cuda, True), _dev(c["w"], cuda), c["bin"], bias=_dev(c["bias"], cuda), x2=_dev(c["x2"], cuda, True),
                              rowvec=_dev(c.get("rowvec"), cuda), resid=_dev(c.get("resid"), cuda, True), xs1=_dev(c.get("xs1"), cuda, True),
                              w_sc=_dev(c.get("w_sc"), cuda), upsample=c["ups"], splitk=c["splitk"])


@pytest.mark.parametrize("name", list(U.PRODUCER_CASES))
def test_gn_stats_producer_partials(cuda, name):
  """The raw partials against fp64 sums of the tensor the kernel itself wrote (that tensor against the fp32 conv / GEMM reference at the
  project's bar), in the slab layout include/gill_amd.h states; nothing unwritten inside, nothing written beyond, two runs bit-identical."""
  c = U.producer_case(name)
  y, buf, slab_rows, nslab = _run_producer(name, cuda)
  y_cpu, buf_cpu = y.float().cpu(), buf.cpu()
  ref_t = c["ref"]
  rel = (y_cpu.reshape(ref_t.shape) - ref_t).abs().max().item() / ref_t.abs().max().item()
  print(f"[{name}] tensor rel_to_max={rel:.4e}")
  assert rel < U.TENSOR_BAR
  assert slab_rows == U.expected_slab_rows(name) and nslab == c["rows"] // slab_rows, (slab_rows, nslab)
  B, nb = c["B"], ref_t.shape[-1] // c["bin"]
  used = B * nslab * nb * 2
  assert torch.isfinite(buf_cpu[:used]).all(), "a partial was never written"
  assert torch.isnan(buf_cpu[used:]).all(), "the producer wrote beyond its B * nslab * bins partials"
  ref, den = U.partials_ref(y_cpu.reshape(ref_t.shape), slab_rows, c["bin"], c["ups"])
  fig = U.partials_figure(name, buf_cpu[:used].reshape(B, nslab, nb, 2), ref, den)
  assert fig < U.STAT_BAR
  y2, buf2, _, _ = _run_producer(name, cuda)
  assert torch.equal(y, y2) and torch.equal(buf[:used], buf2[:used])


def _consumer(case, silu, eps, cuda, want_table=False):
  from gill_amd import ops
  C1, bin1, C2, bin2, B, HW, ns1, ns2 = case
  x1, st1, x2, st2, gamma, beta = U.consumer_case(*case)
  d1, d2 = st1.to(cuda), _dev(st2, cuda)
  y, table, a1, a2 = ops.groupnorm_from_stats(_dev(x1, cuda, True), d1, bin1, gamma.to(cuda), beta.to(cuda), U.GROUPS, eps, silu,
                                              x2=_dev(x2, cuda, True), stats2=d2, bin2=bin2, want_table=want_table)
  # the apply must never modify a producer's partials: a skip tensor is normalised twice
  assert torch.equal(a1.cpu(), st1) and (st2 is None or torch.equal(a2.cpu(), st2)), "the statistics were modified"
  return y, table


def _check_y(tag, case, silu, eps, cuda):
  x1, _, x2, _, gamma, beta = U.consumer_case(*case)
  x = x1 if x2 is None else torch.cat([x1, x2], -1)
  y, _ = _consumer(case, silu, eps, cuda)
  assert U.group_figure(tag, y.float().cpu(), U.groupnorm_ref(x, U.GROUPS, gamma, beta, eps, silu), U.GROUPS) < U.Y_BAR
  assert torch.equal(y, _consumer(case, silu, eps, cuda)[0]), "two runs differ"
  return x, gamma, beta


@pytest.mark.parametrize("C,bin,B,HW,ns,silu,eps", U.one_block_cases())
def test_gn_stats_consumer_one_block(cuda, C, bin, B, HW, ns, silu, eps):
  case = (C, bin, 0, 0, B, HW, ns, 0)
  tag = f"gn_from_stats C {C}/{bin} HW {HW} ns {ns}"
  x, gamma, beta = _check_y(tag, case, silu, eps, cuda)
  _, table = _consumer(case, silu, eps, cuda, want_table=True)
  assert U.table_figure(tag, table, x, U.GROUPS, gamma, beta, eps) < U.STAT_BAR


@pytest.mark.parametrize("C1,bin1,C2,bin2,B,HW,ns1,ns2,silu,eps", U.two_block_cases())
def test_gn_stats_consumer_two_blocks(cuda, C1, bin1, C2, bin2, B, HW, ns1, ns2, silu, eps):
  _check_y(f"gn_from_stats C {C1}/{bin1}+{C2}/{bin2} HW {HW} ns {ns1},{ns2}", (C1, bin1, C2, bin2, B, HW, ns1, ns2), silu, eps, cuda)


def test_gn_stats_consumer_refuses_misaligned_bins(cuda):
  """(640, bin 20) + (320, bin 5) with 32 groups of 30: groupnorm_bins_align() says no — an error, not a result."""
  from gill_amd import _native as N, ops
  x1, x2 = U.consumer_acts(2, 64, 640, 20, 1), U.consumer_acts(2, 64, 320, 5, 2)
  st1, st2 = U.host_partials(U.bin_totals(x1, 20), 4, 3), U.host_partials(U.bin_totals(x2, 5), 4, 4)
  gamma, beta = U.norm_params(960, 5)
  with pytest.raises(N.GillNativeError):
    ops.groupnorm_from_stats(_dev(x1, cuda, True), st1.to(cuda), 20, gamma.to(cuda), beta.to(cuda), U.GROUPS, 1e-5, True,
                             x2=_dev(x2, cuda, True), stats2=st2.to(cuda), bin2=5)


def test_gn_stats_chain_two_producers_into_the_two_block_apply(cuda):
  """An up block's norm1 as the UNet runs it: the hidden tensor from a split-K conv (16-row slabs, bins of 10), the skip tensor from an unsplit
  conv (64-row slabs, bins of 5), normalised together from their partials — against F.group_norm of the two tensors they wrote."""
  from gill_amd import ops
  (yh, bh, _, nh), (ys, bs, _, nsk) = _run_producer("splitk4_640", cuda), _run_producer("chain_skip_320", cuda)
  B, HW = 2, 64
  sth = bh[:B * nh * 64 * 2].reshape(B, nh, 64, 2).contiguous()
  sts = bs[:B * nsk * 64 * 2].reshape(B, nsk, 64, 2).contiguous()
  assert nh != nsk
  gamma, beta = U.norm_params(960, 77)
  y, _, _, _ = ops.groupnorm_from_stats(yh.reshape(B, HW, 640), sth, 10, gamma.to(cuda), beta.to(cuda), U.GROUPS, 1e-5, True,
                                        x2=ys.reshape(B, HW, 320), stats2=sts, bin2=5)
  x = torch.cat([yh.reshape(B, HW, 640), ys.reshape(B, HW, 320)], -1).float().cpu()
  ref = F.silu(F.group_norm(x.double().permute(0, 2, 1), U.GROUPS, gamma.double(), beta.double(), 1e-5)).permute(0, 2, 1)
  assert U.group_figure("chain 640/10 (split-K) + 320/5", y.float().cpu(), ref, U.GROUPS) < U.Y_BAR
