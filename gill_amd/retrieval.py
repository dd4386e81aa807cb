"""Device-resident retrieval index (gill_ret_index_* of include/gill_amd.h; kernels in csrc/retrieval.hip).

The reference keeps the CC3M embedding matrix as a torch tensor and ranks with `emb_matrix @ ret_emb.T` + `topk` (gill/models.py:671-696,
:895-900).  GillRetrievalIndex holds the same rows in HBM as bf16, in the operand order of the matrix instruction, and `search` is one fused
score + top-k pass per 16 queries.  Build-defined API (not a reference class); torch only owns the memory of the inputs and outputs.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _native as N

MAX_K = 32
MAX_EXCLUDE = 64
_CHUNK_BYTES = 64 << 20       # host rows are uploaded in pieces of at most this many bytes


class GillRetrievalIndex:
  def __init__(self, dim: int, capacity: int, device: Union[str, torch.device] = "cuda"):
    self.dim, self.capacity = int(dim), int(capacity)
    self.device = torch.device(device)
    h = C.c_void_p()
    N.check(N.lib().gill_ret_index_create(C.byref(h), self.dim, self.capacity))
    self._h = h

  def __del__(self):
    h, self._h = getattr(self, "_h", None), None
    if h:
      N.lib().gill_ret_index_destroy(h)

  def __len__(self) -> int:
    return int(N.lib().gill_ret_index_size(self._h))

  @classmethod
  def from_embeddings(cls, matrix, scale: float = 1.0, normalize: bool = True, device: Union[str, torch.device] = "cuda") -> "GillRetrievalIndex":
    """An index that holds exactly the rows of `matrix` (N, dim): scale * row / ||row|| with normalize (gill/models.py:895-900), else as they are."""
    n, dim = matrix.shape
    index = cls(dim, max(1, n), device)
    index.add(matrix, normalize=normalize, scale=scale)
    return index

  def add(self, rows, normalize: bool = False, scale: float = 1.0) -> None:
    """Append rows (n, dim): a host or device tensor or a numpy array, fp32 / fp16 / bf16 (anything else is converted to fp32).  Host input goes
    up in bounded pieces, so a large array never needs a second full copy on either side."""
    if isinstance(rows, np.ndarray):
      rows = torch.from_numpy(rows)
    if rows.dim() != 2 or rows.shape[1] != self.dim:
      raise ValueError(f"add: rows must be (n, {self.dim}), got {tuple(rows.shape)}")
    n = rows.shape[0]
    if n > self.capacity - len(self):
      raise ValueError(f"add: {n} rows do not fit: {len(self)} of {self.capacity} are taken")
    step = n if rows.is_cuda else max(1, _CHUNK_BYTES // max(1, self.dim * rows.element_size()))
    for lo in range(0, n, max(1, step)):
      part = rows[lo:lo + step]
      if part.dtype not in N._DTYPES:
        part = part.float()
      part = part.to(self.device).contiguous()
      with torch.cuda.device(self.device):
        N.check(N.lib().gill_ret_index_add(self._h, N.ptr(part), N._DTYPES[part.dtype], part.shape[0], int(bool(normalize)), float(scale),
                                           N.current_stream()))
        if not rows.is_cuda:
          torch.cuda.current_stream().synchronize()     # the staging piece is released before the next one is made

  def rows(self, first: int, n: int) -> torch.Tensor:
    """Rows [first, first + n) as stored -> (n, dim) bf16."""
    if first < 0 or n < 0 or first + n > len(self):
      raise IndexError(f"rows: [{first}, {first + n}) is outside the {len(self)} rows held")
    out = torch.empty((n, self.dim), device=self.device, dtype=torch.bfloat16)
    with torch.cuda.device(self.device):
      N.check(N.lib().gill_ret_index_rows(self._h, first, n, N.ptr(out), N.current_stream()))
    return out

  def slabs(self) -> Tuple[int, int, int]:
    """(first row, number of per-wave lists, rows per list) of the main pass of a search of the index as it stands; the rows below the first
    are the prefix that is searched first.  For tests: no result depends on it."""
    fr, nl, rp = C.c_int64(), C.c_int(), C.c_int64()
    N.check(N.lib().gill_ret_index_slabs(self._h, C.byref(fr), C.byref(nl), C.byref(rp)))
    return fr.value, nl.value, rp.value

  def _exclude(self, exclude, Q: int) -> Optional[torch.Tensor]:
    if exclude is None:
      return None
    if isinstance(exclude, torch.Tensor):
      ex = exclude.to(device=self.device, dtype=torch.int64)
      if ex.dim() == 1:
        ex = ex[None, :].expand(Q, -1)
    else:
      lists = [list(int(i) for i in row) for row in exclude]
      width = max([len(row) for row in lists] + [1])
      ex = torch.full((len(lists), width), -1, dtype=torch.int64)
      for q, row in enumerate(lists):
        ex[q, :len(row)] = torch.tensor(row, dtype=torch.int64)
      ex = ex.to(self.device)
    if ex.dim() != 2 or ex.shape[0] != Q:
      raise ValueError(f"search: exclude must hold one list per query ({Q}), got {tuple(ex.shape)}")
    if ex.shape[1] > MAX_EXCLUDE:
      raise ValueError(f"search: at most {MAX_EXCLUDE} excluded rows per query, got {ex.shape[1]}")
    return ex.contiguous() if ex.shape[1] > 0 else None

  def search(self, queries: torch.Tensor, k: int, normalize: bool = True, exclude=None, penalty: float = 1000.0,
             _out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """queries (Q, dim) or (dim,) -> (scores (Q, k) fp32, idx (Q, k) int64): the exact top k by (score descending, row index ascending).
    exclude: per query the rows that compete with score - penalty (a list of lists, or a (Q, E) / (E,) tensor with -1 for empty slots).  No
    host synchronisation.  _out: caller-allocated outputs (the tests pass guarded ones)."""
    if isinstance(queries, np.ndarray):
      queries = torch.from_numpy(queries)
    if queries.dim() == 1:
      queries = queries[None, :]
    if queries.dim() != 2 or queries.shape[1] != self.dim or queries.shape[0] < 1:
      raise ValueError(f"search: queries must be (Q >= 1, {self.dim}), got {tuple(queries.shape)}")
    if not 1 <= k <= MAX_K:
      raise ValueError(f"search: 1 <= k <= {MAX_K}, got {k}")
    Q = queries.shape[0]
    q = queries.to(device=self.device, dtype=torch.float32).contiguous()
    ex = self._exclude(exclude, Q)
    if _out is None:
      scores = torch.empty((Q, k), device=self.device, dtype=torch.float32)
      idx = torch.empty((Q, k), device=self.device, dtype=torch.int64)
    else:
      scores, idx = _out
      assert scores.shape == (Q, k) and scores.dtype == torch.float32 and idx.shape == (Q, k) and idx.dtype == torch.int64
    with torch.cuda.device(self.device):
      N.check(N.lib().gill_ret_index_search(self._h, N.ptr(q), Q, int(bool(normalize)), int(k), N.ptr(ex), 0 if ex is None else ex.shape[1],
                                            float(penalty), N.ptr(scores), N.ptr(idx), N.current_stream()))
    return scores, idx
